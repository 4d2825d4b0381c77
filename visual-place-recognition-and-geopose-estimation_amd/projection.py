"""Descriptor projection for retrieval: PCA with optional whitening fitted on gallery descriptors, applied on the device
(include/vpr_amd_project.h) and followed by L2 re-normalisation, so that kNN rows are d wide instead of D.

`fit_projection` is PyTorch plumbing (f64 mean / covariance / eigh, run once per gallery); `DescriptorProjection.apply` is
the hot path, `ops.project_rows`.  The kernel multiplies by P = bf16(matrix) and adds c = -(P as f64) . mean rounded to f32:
the bias is formed from the ROUNDED matrix, so the centring matches what the kernel multiplies.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import ops


class DescriptorProjection:
    """matrix f32 [d, D] (the master copy; row j = eigenvector j, scaled when whitening), mean f64 [D], eigenvalues f64 [d]
    (descending), and how it was fitted (whiten, eps_rel, n_fit).  Device operands (P bf16, c f32) are derived once per device."""

    def __init__(self, matrix, mean, eigenvalues, whiten: bool = True, eps_rel: float = 1e-6, n_fit: int = 0):
        self.matrix = torch.as_tensor(matrix).detach().to("cpu", torch.float32).contiguous()
        self.mean = torch.as_tensor(mean).detach().to("cpu", torch.float64).contiguous()
        self.eigenvalues = torch.as_tensor(eigenvalues).detach().to("cpu", torch.float64).contiguous()
        if self.matrix.dim() != 2 or self.mean.shape != (self.matrix.shape[1],) or self.eigenvalues.shape != (self.matrix.shape[0],):
            raise ValueError("DescriptorProjection: matrix [d, D], mean [D], eigenvalues [d]")
        self.whiten, self.eps_rel, self.n_fit = bool(whiten), float(eps_rel), int(n_fit)
        self._operands: Dict[Tuple[str, Optional[int]], Tuple[torch.Tensor, torch.Tensor]] = {}

    @property
    def d(self) -> int:
        return self.matrix.shape[0]

    @property
    def d_in(self) -> int:
        return self.matrix.shape[1]

    def host_operands(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(P bf16 [d, D], c f32 [d]) on the host: P = bf16(matrix), c = f32(-(P as f64) . mean)."""
        P = self.matrix.to(torch.bfloat16)
        c = (-(P.to(torch.float64) @ self.mean)).to(torch.float32)
        return P, c

    def operands(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        device = torch.device(device)
        key = (device.type, device.index)
        if key not in self._operands:
            P, c = self.host_operands()
            self._operands[key] = (P.to(device).contiguous(), c.to(device).contiguous())
        return self._operands[key]

    def apply(self, x_bf16: torch.Tensor, want_f32: bool = False):
        """x bf16 [rows, D] on a GPU -> unit rows bf16 [rows, d]; want_f32: (f32 [rows, d], bf16 [rows, d])."""
        if not isinstance(x_bf16, torch.Tensor) or not x_bf16.is_cuda:
            raise RuntimeError("x: expected a GPU tensor (the HIP path has no CPU fallback)")
        P, c = self.operands(x_bf16.device)
        o32, o16 = ops.project_rows(x_bf16, P, c, True, want_f32=want_f32, want_bf16=True)
        return (o32, o16) if want_f32 else o16

    def save(self, path: str) -> None:
        """One .npz of arrays and scalars only (no pickled objects)."""
        with open(path, "wb") as f:
            np.savez(f, matrix=self.matrix.numpy(), mean=self.mean.numpy(), eigenvalues=self.eigenvalues.numpy(),
                     whiten=np.bool_(self.whiten), eps_rel=np.float64(self.eps_rel), n_fit=np.int64(self.n_fit))

    @classmethod
    def load(cls, path: str) -> "DescriptorProjection":
        with np.load(path, allow_pickle=False) as z:
            return cls(torch.from_numpy(z["matrix"].copy()), torch.from_numpy(z["mean"].copy()),
                       torch.from_numpy(z["eigenvalues"].copy()), bool(z["whiten"]), float(z["eps_rel"]), int(z["n_fit"]))


def subsample_rows(N: int, max_rows: int) -> torch.Tensor:
    """The rows fit_projection uses: all of them, or max_rows at a deterministic stride (row floor(i * N / max_rows))."""
    if N <= max_rows:
        return torch.arange(N)
    return (torch.arange(max_rows, dtype=torch.int64) * N) // max_rows


def _eigh(cov: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    if cov.is_cuda:
        try:
            w, v = torch.linalg.eigh(cov)
            return w.cpu(), v.cpu()
        except RuntimeError:          # no f64 eigensolver on this device build: the host has one
            cov = cov.cpu()
    return torch.linalg.eigh(cov)


@torch.no_grad()
def fit_projection(descriptors: torch.Tensor, d: int, whiten: bool = True, eps_rel: float = 1e-6, max_rows: int = 16384,
                   chunk: int = 4096, device=None) -> DescriptorProjection:
    """PCA (whiten=False) or PCA-whitening of `descriptors` [N, D] (bf16 or f32, host or device; rows are used at their bf16
    values, the values the kernel will see).  Mean and covariance (divided by n - 1) are accumulated in f64 chunk by chunk on
    `device` (None: where the descriptors live); the top d eigenpairs of an f64 eigh are kept (with fewer rows than columns,
    of the n x n form of the same problem).  Sign: the component of largest
    magnitude of every eigenvector is positive (ties: the lowest index).  whiten: row j is scaled by
    1 / sqrt(lambda_j + eps_rel * lambda_0)."""
    if descriptors.dim() != 2:
        raise ValueError("fit_projection: descriptors must be [N, D]")
    if descriptors.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("fit_projection: descriptors must be bfloat16 or float32")
    N, D = descriptors.shape
    d = int(d)
    sel = subsample_rows(N, int(max_rows))
    n = int(sel.numel())
    if d < 1 or d > D:
        raise ValueError(f"fit_projection: d = {d} must be in 1..D = {D}")
    if d % 64 != 0:
        raise ValueError(f"fit_projection: d = {d} must be a multiple of 64 (the kernels' tile)")
    if d >= n:
        raise ValueError(f"fit_projection: d = {d} needs more than d rows, {n} are used")
    dev = descriptors.device if device is None else torch.device(device)
    take_all = n == N

    def chunks():
        for lo in range(0, n, int(chunk)):
            rows = descriptors[lo:lo + chunk] if take_all else descriptors[sel[lo:lo + chunk].to(descriptors.device)]
            yield rows.to(torch.bfloat16).to(dev).to(torch.float64)

    total = torch.zeros(D, dtype=torch.float64, device=dev)
    for x in chunks():
        total += x.sum(0)
    mean = total / n
    if n >= D:
        gram = torch.zeros((D, D), dtype=torch.float64, device=dev)  # of the centred rows: no cancellation against n mean mean^T
        for x in chunks():
            x -= mean
            gram += x.T @ x
        cov = gram / (n - 1)
        w, v = _eigh((cov + cov.T) * 0.5)
        w, v = w.flip(0)[:d].contiguous(), v.flip(1)[:, :d].T.contiguous()        # descending; rows = eigenvectors
    else:
        # Fewer rows than columns: the covariance has rank < n, and its non-zero eigenpairs are those of the n x n matrix
        # Xc Xc^T / (n - 1): (lambda, u) there is (lambda, Xc^T u / sqrt((n - 1) lambda)) here — an n^3 problem, not a D^3 one.
        xc = torch.cat([x - mean for x in chunks()])
        small = (xc @ xc.T) / (n - 1)
        w, u = _eigh((small + small.T) * 0.5)
        w, u = w.flip(0)[:d].contiguous(), u.flip(1)[:, :d].contiguous()
        if not w[-1] > 1e-12 * w[0]:
            raise ValueError(f"fit_projection: the {n} rows span fewer than d = {d} directions")
        v = (u.T.to(dev) @ xc).cpu() / torch.sqrt((n - 1) * w)[:, None]
        v = (v / v.norm(dim=1, keepdim=True)).contiguous()
    big = v.abs().argmax(dim=1, keepdim=True)                                      # first index of the largest magnitude
    v = v * torch.where(v.gather(1, big) < 0, -1.0, 1.0)
    if whiten:
        v = v / torch.sqrt(w.clamp_min(0.0) + eps_rel * w[0])[:, None]
    return DescriptorProjection(v.to(torch.float32), mean.cpu(), w, whiten, eps_rel, n)
