"""GPU: vpr_retrieval_pose (include/vpr_amd_retrieval.h) through torch.ops.vpr.retrieval_pose, GraphedRetrieval, the pipeline
and evaluate.retrieval_metrics.

Reference: `reference()` below restates the header's contract in np.longdouble (eps < 2^-60 is asserted; on a platform
whose long double is narrower the comparisons against it are skipped).  gallery.label_transfer, numpy f64 on the host, is a
second reference held to the same bound wherever it is defined (neighbour 0 live, no index past the table).

Bound: E = 2^-50 (k + 16 + Smax / temperature), Smax = max over live j of vals[b,0] - vals[b,j]:
  k additions of a sum, a few f64 library functions (exp, sin, cos, atan2, the divisions) at about 2 ulp each -> 16, the
  error of the exponent's argument (one rounded difference and one rounded quotient of size <= Smax / temperature)
  amplified by exp -> Smax / temperature, all in units of 2^-53 relative, times a factor 4 of slack and rounded up: 2^-50.
  lat / lon:  |err| <= E max_j |label_j|            (the live neighbours' own magnitude)
  angle:      circular |err| <= E (180 / pi) / R    with R = hypot(S, C) of the reference (atan2's condition number);
              the inputs keep every query's neighbour angles within one arc of less than 90 degrees, so R >= 0.7.
  pose4:      |err| <= 2^-24 |value| + (the f64 bound) / scale   (one rounding to f32; the (sin, cos) entries carry the
              angle bound in radians, E / R)
  top-1 mode: the same formulas with Smax = 0.
Hits are integers and are compared for equality; d^2 and tau^2 are f64 numbers by contract, so the reference forms them
in f64 exactly as gallery.positives_by_distance does."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LD = np.longdouble
LD_OK = float(np.finfo(LD).eps) < 2.0 ** -60
PI = LD(4) * np.arctan(LD(1))
N = 300
ARC_ROWS = 74                        # neighbours of one query come from 74 consecutive rows (mod N): an arc of 88.8 degrees
SCALER = [219658.4252116651, 143506.67654437126, 918.58972058316, 1190.858018520488]     # postproc.CAMPUS_MEAN / _SCALE
MODES = ("top1", "weighted")


# ------------------------------------------------------------------------------------------------------- inputs
def make_labels(seed=0, n=N, phase=7.3):
    """Campus-magnitude lat / lon, angle = a ramp over the rows (so a window of rows is an arc; `phase` puts the 0 / 360
    seam inside the table), Region_ID in 0..5."""
    rng = np.random.default_rng(seed)
    lat = SCALER[0] + rng.normal(0, SCALER[2], n)
    lon = SCALER[1] + rng.normal(0, SCALER[3], n)
    ang = (np.arange(n) * (360.0 / n) + phase) % 360.0
    return np.stack([lat, lon, ang, rng.integers(0, 6, n).astype(np.float64)], 1)


def make_lists(rng, B, k, n=N, spread=1.5, pad=True, dead=True):
    """Descending scores with total spread <= `spread`, neighbours drawn from a window of rows with a random start (windows
    wrap, so arcs cross 0 / 360); pad: about a third of the rows get a tail of (-1, -inf); dead: row B // 2 has no neighbour."""
    idx = np.empty((B, k), dtype=np.int32)
    for b in range(B):
        idx[b] = (rng.integers(0, n) + rng.permutation(ARC_ROWS)[:k]) % n
    top = rng.uniform(0.3, 0.95, (B, 1))
    vals = np.sort(top - rng.uniform(0, spread, (B, k)) * (np.arange(k) > 0), axis=1)[:, ::-1].astype(np.float32)
    if pad and k > 1:
        for b in range(0, B, 3):
            cut = int(rng.integers(1, k))
            idx[b, cut:], vals[b, cut:] = -1, -np.inf
    if dead and B >= 3:
        idx[B // 2], vals[B // 2] = -1, -np.inf
    return np.ascontiguousarray(vals), idx


def make_targets(rng, idx, labels, tau):
    """Each query's own (lat, lon, Region_ID): near one of its neighbours (so hits land at every rank), and never within
    1e-9 tau^2 of the tau circle of any neighbour."""
    B, k = idx.shape
    q = np.empty((B, 3))
    for b in range(B):
        j = int(rng.integers(0, k))
        r = idx[b, j] if 0 <= idx[b, j] < len(labels) else int(rng.integers(0, len(labels)))
        q[b, :2] = labels[r, :2] + rng.normal(0, 0.7 * tau, 2)
        q[b, 2] = labels[r, 3] if rng.random() < 0.7 else 9.0
    live = (idx >= 0) & (idx < len(labels))
    g = labels[np.where(live, idx, 0)]
    d2 = (g[:, :, 0] - q[:, None, 0]) ** 2 + (g[:, :, 1] - q[:, None, 1]) ** 2
    assert (np.abs(d2 - tau * tau)[live] > 1e-9 * tau * tau).all()
    return q


# ---------------------------------------------------------------------------------------------------- reference
def reference(vals, idx, labels, mode, temperature, q=None, tau=0.0, scaler=None):
    """The contract of include/vpr_amd_retrieval.h in long double.  Returns pose64 [B,3], pose4 [B,4] (both LD, NaN rows
    where neighbour 0 is not live), hit_tau, hit_region (int), R [B] and Smax [B] (float) for the bounds."""
    B, k = idx.shape
    live = (idx >= 0) & (idx < len(labels))
    g = labels[np.where(live, idx, 0)]                                   # [B, k, 4] f64
    any0 = live[:, 0]
    lat, lon, ang = g[:, :, 0].astype(LD), g[:, :, 1].astype(LD), g[:, :, 2].astype(LD)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if mode == "top1":
            o_lat, o_lon, o_ang, R, smax = lat[:, 0], lon[:, 0], ang[:, 0] % LD(360), np.ones(B), np.zeros(B)
        else:
            v = vals.astype(LD)
            d = np.where(live, v - v[:, :1], LD(0))
            w = np.where(live, np.exp(d / LD(temperature)), LD(0))
            sw = w.sum(1)
            th = ang * PI / LD(180)
            S, C = (w * np.sin(th)).sum(1) / sw, (w * np.cos(th)).sum(1) / sw
            o_lat, o_lon = (w * lat).sum(1) / sw, (w * lon).sum(1) / sw
            o_ang = (np.arctan2(S, C) * LD(180) / PI) % LD(360)
            R = np.hypot(S, C).astype(np.float64)
            smax = np.where(live, -d, LD(0)).max(1).astype(np.float64)
        m = [LD(x) for x in (scaler if scaler is not None else (0.0, 0.0, 1.0, 1.0))]
        th = o_ang * PI / LD(180)
        pose4 = np.stack([(o_lat - m[0]) / m[2], (o_lon - m[1]) / m[3], np.sin(th), np.cos(th)], 1)
    pose64 = np.stack([o_lat, o_lon, o_ang], 1)
    pose64[~any0], pose4[~any0] = np.nan, np.nan
    R = np.where(any0, R, 1.0)
    smax = np.where(any0, smax, 0.0)
    ht, hr = np.full(B, -1, dtype=np.int64), np.full(B, -1, dtype=np.int64)
    if q is not None:
        d2 = (g[:, :, 0] - q[:, None, 0]) ** 2 + (g[:, :, 1] - q[:, None, 1]) ** 2          # f64, as positives_by_distance
        for hit, ok in ((ht, live & (d2 <= tau * tau)), (hr, live & (g[:, :, 3] == q[:, None, 2]))):
            has = ok.any(1) & any0
            hit[has] = ok.argmax(1)[has]
    return pose64, pose4, ht, hr, R, smax


def bounds(idx, labels, R, smax, temperature, scaler=None):
    """(b64 [B,3], b4 [B,4]) without pose4's 2^-24 |value| term: lat, lon, angle in degrees (circular)."""
    B, k = idx.shape
    live = (idx >= 0) & (idx < len(labels))
    g = np.abs(labels[np.where(live, idx, 0)]) * live[:, :, None]
    E = 2.0 ** -50 * (k + 16 + smax / temperature)
    b64 = np.stack([E * g[:, :, 0].max(1), E * g[:, :, 1].max(1), E * (180.0 / math.pi) / R], 1)
    s = scaler if scaler is not None else (0.0, 0.0, 1.0, 1.0)
    b4 = np.stack([b64[:, 0] / s[2], b64[:, 1] / s[3], E / R, E / R], 1)
    return b64, b4


def assert_pose_close(got64, got4, ref64, ref4, b64, b4, what=""):
    """got*: f64 / f32 numpy from the device (or label_transfer's f64 with got4 None)."""
    dead = np.isnan(ref64[:, 0].astype(np.float64))
    assert np.isnan(got64[dead]).all(), what
    assert not np.isnan(got64[~dead]).any(), what
    err = np.abs(got64.astype(LD) - ref64)
    err[:, 2] = np.minimum(err[:, 2], LD(360) - err[:, 2])
    ok = ~dead
    assert (err[ok] <= b64[ok]).all(), (what, float((err[ok] / b64[ok]).max()))
    if got4 is not None:
        assert ((got64[ok, 2] >= 0.0) & (got64[ok, 2] < 360.0)).all(), what      # the device's angle never rounds up to 360
        assert np.isnan(got4[dead]).all() and not np.isnan(got4[ok]).any(), what
        err4 = np.abs(got4.astype(LD) - ref4)
        lim = LD(2.0) ** -24 * np.abs(ref4) + b4
        assert (err4[ok] <= lim[ok]).all(), (what, float((err4[ok] / lim[ok]).max()))


def run_op(dev, vals, idx, labels, mode="top1", temperature=0.01, q=None, tau=0.0, scaler=None):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = torch.ops.vpr.retrieval_pose(t(vals), t(idx), t(labels), mode, temperature, t(q), tau, scaler)
    assert [o.dtype for o in out] == [torch.float64, torch.float32, torch.int32, torch.int32]
    B = idx.shape[0]
    assert [tuple(o.shape) for o in out] == [(B, 3), (B, 4), (B,), (B,)]
    return [o.cpu().numpy() for o in out]


def check(dev, vals, idx, labels, mode, temperature=0.01, q=None, tau=0.0, scaler=None, what=""):
    """Runs the op and holds all four outputs (and label_transfer, where defined) to the reference.  Returns the outputs."""
    from vpr_amd import gallery as G
    got = run_op(dev, vals, idx, labels, mode, temperature, q, tau, scaler)
    ref64, ref4, ht, hr, R, smax = reference(vals, idx, labels, mode, temperature, q, tau, scaler)
    assert np.array_equal(got[2], ht), (what, "hit_tau")
    assert np.array_equal(got[3], hr), (what, "hit_region")
    if not LD_OK:                       # no reference for the pose comparison on this platform: the hits were still compared
        return got
    b64, b4 = bounds(idx, labels, R, smax, temperature, scaler)
    assert_pose_close(got[0], got[1], ref64, ref4, b64, b4, what)
    rows = (idx[:, 0] >= 0) & (idx < len(labels)).all(1)                 # where the host function is defined
    if rows.any():
        with np.errstate(all="ignore"):
            host = G.label_transfer(torch.from_numpy(vals[rows]), torch.from_numpy(idx[rows]), labels, mode, temperature)
        assert_pose_close(host, None, ref64[rows], None, b64[rows], None, what + " label_transfer")
    return got


# -------------------------------------------------------------------------------------------------------- tests
def test_long_double_is_the_reference_it_is_taken_for():
    assert LD_OK, np.finfo(LD)


@pytest.mark.parametrize("k", [1, 2, 10, 63, 64])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 64, 65, 257])
def test_every_output_against_the_reference(dev, B, k):
    """Lane masks (k), workgroup tails (B mod 4), more than one workgroup: both modes, padded tails, a row without a
    neighbour, hits by distance and by region, the campus scaler."""
    labels = make_labels()
    rng = np.random.default_rng(1000 * B + k)
    tau = 600.0
    for mode in MODES:
        for temperature in ((0.01,) if mode == "top1" else (0.01, 0.05, 1.0)):
            vals, idx = make_lists(rng, B, k)
            q = make_targets(rng, idx, labels, tau)
            got = check(dev, vals, idx, labels, mode, temperature, q, tau, SCALER, what=f"{mode} T={temperature}")
            if B >= 3:
                assert np.isnan(got[0][B // 2]).all() and np.isnan(got[1][B // 2]).all()
                assert got[2][B // 2] == -1 and got[3][B // 2] == -1
            if B >= 64 and k >= 10:
                assert (got[2] >= 0).sum() > B // 4 and len(set(got[2].tolist())) > 3      # hits at several ranks, and misses
                assert (got[3] >= 0).sum() > B // 4 and (got[3] == -1).sum() > 1


def test_no_live_neighbour_gives_nan_and_minus_one(dev):
    labels = make_labels()
    rng = np.random.default_rng(2)
    vals, idx = make_lists(rng, 6, 10, pad=False, dead=False)
    q = make_targets(rng, idx, labels, 600.0)
    idx[1], vals[1] = -1, -np.inf                  # all padding
    idx[4, 0] = -1                                 # neighbour 0 alone is padding (its score stays finite): still no answer
    idx[5, 0] = N                                  # neighbour 0 past the table
    for mode in MODES:
        p64, p4, ht, hr = check(dev, vals, idx, labels, mode, 0.05, q, 600.0, SCALER, what=mode)
        for b in (1, 4, 5):
            assert np.isnan(p64[b]).all() and np.isnan(p4[b]).all() and ht[b] == -1 and hr[b] == -1
        for b in (0, 2, 3):
            assert not np.isnan(p64[b]).any() and not np.isnan(p4[b]).any()


def test_index_past_the_table_is_padding(dev):
    """idx >= n_labels is never used as an address: the outputs are bitwise those of the same list with -1 there."""
    labels = make_labels()
    rng = np.random.default_rng(3)
    vals, idx = make_lists(rng, 9, 10, pad=False, dead=False)
    q = make_targets(rng, idx, labels, 600.0)
    bad, clean = idx.copy(), idx.copy()
    spots = [(0, 3, N), (1, 9, N + 1), (2, 1, 2 ** 31 - 1), (3, 5, 1 << 20), (4, 0, N), (6, 2, -7), (7, 4, -(2 ** 31)), (7, 8, N)]
    for b, j, value in spots:
        bad[b, j], clean[b, j] = value, -1
    for mode in MODES:
        a = run_op(dev, vals, bad, labels, mode, 0.05, q, 600.0, SCALER)
        c = check(dev, vals, clean, labels, mode, 0.05, q, 600.0, SCALER, what=mode)
        for x, y in zip(a, c):
            assert x.tobytes() == y.tobytes()
    # the table's last row is still a row
    idx[:, :] = N - 1
    p64 = run_op(dev, vals, idx, labels, "top1")[0]
    assert (p64[:, :2] == labels[N - 1, :2]).all()


def test_equal_scores_give_equal_weights(dev):
    labels = make_labels()
    rng = np.random.default_rng(4)
    for k in (2, 10, 64):
        vals, idx = make_lists(rng, 5, k, pad=False, dead=False)
        vals[:] = vals[:, :1]
        p64 = check(dev, vals, idx, labels, "weighted", 0.01, what=f"k={k}")[0]
        mean = labels[idx][:, :, :2].mean(1)
        assert np.abs(p64[:, :2] - mean).max() <= 2.0 ** -50 * (k + 16) * np.abs(labels[:, :2]).max()


def test_weights_that_underflow_to_zero(dev):
    """Spread 1.5 at temperature 0.001: exp(-1500) is exactly 0, the weighted pose is neighbour 0's labels exactly."""
    labels = make_labels()
    rng = np.random.default_rng(5)
    vals, idx = make_lists(rng, 5, 10, pad=False, dead=False)
    vals[:, 1:] = vals[:, :1] - 1.5
    assert np.exp((vals[:, 1:].astype(np.float64) - vals[:, :1]) / 0.001).max() == 0.0
    p64, p4 = check(dev, vals, idx, labels, "weighted", 0.001, scaler=SCALER)[:2]
    assert (p64[:, :2] == labels[idx[:, 0], :2]).all()
    t64, t4 = run_op(dev, vals, idx, labels, "top1", scaler=SCALER)[:2]
    assert (p4[:, :2] == t4[:, :2]).all()


def test_angles_350_and_10_average_to_0(dev):
    labels = make_labels()
    labels[5, 2], labels[6, 2] = 350.0, 10.0
    labels[7, 2], labels[8, 2] = 10.0, 350.0
    idx = np.array([[5, 6], [8, 7], [6, 5]], dtype=np.int32)
    vals = np.full((3, 2), 0.75, dtype=np.float32)
    p64, p4 = check(dev, vals, idx, labels, "weighted", 0.01)[:2]
    R = math.cos(math.radians(10.0))
    lim = 2.0 ** -50 * (2 + 16) * (180.0 / math.pi) / R
    assert (np.minimum(p64[:, 2], 360.0 - p64[:, 2]) <= lim).all(), p64[:, 2]
    assert (np.abs(p4[:, 2]) <= 2.0 ** -50 * 18 / R).all() and (p4[:, 3] == 1.0).all()


def test_scaler_given_and_null_targets_given_and_null(dev):
    labels = make_labels()
    rng = np.random.default_rng(6)
    vals, idx = make_lists(rng, 7, 10)
    q = make_targets(rng, idx, labels, 600.0)
    for mode in MODES:
        with_s = check(dev, vals, idx, labels, mode, 0.05, q, 600.0, SCALER)
        no_s = check(dev, vals, idx, labels, mode, 0.05, q, 600.0, None)
        no_q = check(dev, vals, idx, labels, mode, 0.05, None, 0.0, SCALER)
        ok = ~np.isnan(no_s[0][:, 0])
        assert no_s[0].tobytes() == with_s[0].tobytes() == no_q[0].tobytes()          # pose64 does not see the scaler
        assert (no_s[1][ok, :2] == no_s[0][ok, :2].astype(np.float32)).all()          # NULL scaler = (0, 0, 1, 1)
        assert (np.abs(with_s[1][ok, :2]) < 10).all() and (no_s[1][:, 2:].tobytes() == with_s[1][:, 2:].tobytes())
        assert (no_q[2] == -1).all() and (no_q[3] == -1).all() and (with_s[2] >= 0).any()
        assert no_q[1].tobytes() == with_s[1].tobytes()


def test_exact_boundary_of_the_tau_circle(dev):
    """Integer coordinates, offset (3, 4): d^2 = 25 = tau^2 exactly at tau = 5 (a hit, <=), and a miss at tau = 4.999."""
    labels = make_labels()
    labels[:, 0], labels[:, 1] = 219000.0 + 100.0 * np.arange(N), 143000.0 + 100.0 * (np.arange(N) % 17)
    idx = np.array([[20, 21, 22, 23], [30, 31, 32, 33], [40, 41, 42, -1]], dtype=np.int32)
    vals = np.array([[0.9, 0.8, 0.7, 0.6]] * 3, dtype=np.float32)
    vals[2, 3] = -np.inf
    q = np.array([[labels[22, 0] + 3.0, labels[22, 1] - 4.0, 9.0], [labels[30, 0] - 4.0, labels[30, 1] - 3.0, 9.0],
                  [labels[43, 0] + 3.0, labels[43, 1] + 4.0, 9.0]])        # row 2: its only match is not in the list
    for mode in MODES:
        assert check(dev, vals, idx, labels, mode, 0.05, q, 5.0)[2].tolist() == [2, 0, -1]
        assert check(dev, vals, idx, labels, mode, 0.05, q, 4.999)[2].tolist() == [-1, -1, -1]
        assert check(dev, vals, idx, labels, mode, 0.05, q, 0.0)[2].tolist() == [-1, -1, -1]
    q[1, :2] = labels[31, :2]
    assert check(dev, vals, idx, labels, "top1", 0.05, q, 0.0)[2].tolist() == [-1, 1, -1]   # tau = 0: the point itself


def test_region_hits(dev):
    labels = make_labels()
    labels[:, 3] = np.arange(N) % 5
    idx = np.array([[11, 12, 13, 14, 10], [11, 12, 13, 14, 10], [11, 12, 13, 14, -1], [-1, 13, 13, 13, 13]], dtype=np.int32)
    vals = np.array([[0.9, 0.8, 0.7, 0.6, 0.5]] * 4, dtype=np.float32)
    q = np.array([[0, 0, 3.0], [0, 0, 0.0], [0, 0, 0.0], [0, 0, 3.0]]) + [labels[11, 0], labels[11, 1], 0]
    q = np.concatenate([q, [[labels[11, 0], labels[11, 1], np.nan]]])
    idx, vals = np.concatenate([idx, idx[:1]]), np.concatenate([vals, vals[:1]])
    for mode in MODES:
        assert check(dev, vals, idx, labels, mode, 0.05, q, 1.0)[3].tolist() == [2, 4, -1, -1, -1]


def test_recall_from_first_hit_equals_recall_at_k_on_the_same_data(dev):
    from vpr_amd import gallery as G, postproc
    labels = make_labels()
    rng = np.random.default_rng(8)
    B, k, tau = 65, 10, 600.0
    vals, idx = make_lists(rng, B, k)
    q = make_targets(rng, idx, labels, tau)
    _, _, ht, hr = check(dev, vals, idx, labels, "top1", 0.01, q, tau)
    pos_d = G.positives_by_distance(q[:, :2], labels[:, :2], tau)
    pos_r = G.positives_by_region(q[:, 2], labels[:, 3])
    seen = set()
    for j in range(1, k + 1):
        r = postproc.recall_from_first_hit(ht, j)
        assert r == postproc.recall_at_k(idx[:, :j], pos_d), j
        assert postproc.recall_from_first_hit(hr, j) == postproc.recall_at_k(idx[:, :j], pos_r), j
        seen.add(r)
    assert len(seen) > 3 and 0.0 < min(seen) and max(seen) < 1.0


def test_a_row_does_not_depend_on_its_batch_and_runs_repeat(dev):
    labels = make_labels()
    rng = np.random.default_rng(9)
    for k in (10, 64):
        vals, idx = make_lists(rng, 65, k)
        q = make_targets(rng, idx, labels, 600.0)
        for mode in MODES:
            full = run_op(dev, vals, idx, labels, mode, 0.05, q, 600.0, SCALER)
            again = run_op(dev, vals, idx, labels, mode, 0.05, q, 600.0, SCALER)
            for x, y in zip(full, again):
                assert x.tobytes() == y.tobytes()
            for b in (0, 1, 3, 4, 31, 32, 63, 64):
                one = run_op(dev, vals[b:b + 1], idx[b:b + 1], labels, mode, 0.05, q[b:b + 1], 600.0, SCALER)
                for x, y in zip(full, one):
                    assert x[b:b + 1].tobytes() == y.tobytes(), (mode, k, b)


def _gallery(dev, n, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, 8448, device=dev, generator=g), dim=1)


def test_graphed_retrieval_replays_the_pose(dev):
    """One rank, local search only: pose4 / pose64 after a replay are bitwise the eager op on the returned (vals, idx)."""
    from vpr_amd.retrieval import GraphedRetrieval, ShardedGallery
    n, B, k = 500, 4, 5
    gal = _gallery(dev, n, 1)
    labels = torch.from_numpy(make_labels(n=n)).to(dev)
    for mode in MODES:
        gr = GraphedRetrieval(ShardedGallery(gal.to(torch.bfloat16), n), B, k, labels=labels, mode=mode, temperature=0.05, scaler=SCALER)
        seen = []
        for trial in range(2):
            g = torch.Generator(device=dev).manual_seed(50 + trial)
            pos = torch.randint(0, n, (B,), device=dev, generator=g)
            qd = torch.nn.functional.normalize(gal[pos] + 0.1 * torch.randn(B, 8448, device=dev, generator=g), dim=1).to(torch.bfloat16)
            v, i = gr(qd)
            assert torch.equal(i[:, 0].long(), pos)
            p64, p4, _, _ = torch.ops.vpr.retrieval_pose(v.clone(), i.clone(), labels, mode, 0.05, None, 0.0, SCALER)
            assert gr.pose64.shape == (B, 3) and gr.pose4.shape == (B, 4)
            assert gr.pose64.cpu().numpy().tobytes() == p64.cpu().numpy().tobytes()
            assert gr.pose4.cpu().numpy().tobytes() == p4.cpu().numpy().tobytes()
            seen.append(gr.pose64.clone())
        assert not torch.equal(seen[0], seen[1])                  # two different batches, two different answers
        gr.close()
    plain = GraphedRetrieval(ShardedGallery(gal.to(torch.bfloat16), n), B, k)
    assert plain.pose64 is None and plain.pose4 is None
    plain.close()


def test_pipeline_fills_retrieval_pose(dev):
    """ViT-S, as smoke() builds it.  With labels: retrieval_pose is the op on the step's own topk_*, eager and graphed.
    Without: the field is None, and every other output is bitwise that of the step with labels."""
    import torch.nn as nn
    from vpr_amd.modules import DinoV2Salad, FusedGeoPoseHead
    from vpr_amd.pipeline import VPRGeoPosePipeline
    from vpr_amd.retrieval import ShardedGallery
    torch.manual_seed(0)
    ext = DinoV2Salad("vit_small").to(dev).to(torch.bfloat16).eval()
    ext.backbone.fold_layerscale()
    pos = nn.Sequential(nn.Linear(8448, 64), nn.ReLU(), nn.Linear(64, 2)).to(dev)
    ang = nn.Sequential(nn.Linear(8448, 64), nn.ReLU(), nn.Linear(64, 2)).to(dev)
    head = FusedGeoPoseHead(pos, ang, normalize=True)
    n, B, k = 500, 2, 5
    gal = _gallery(dev, n, 2).to(torch.bfloat16)
    labels_np = make_labels(n=n)
    labels = torch.from_numpy(labels_np).to(dev)
    images = torch.randn(B, 3, 224, 224, device=dev).to(torch.bfloat16)
    base = VPRGeoPosePipeline(ext, head, ShardedGallery(gal, n), k).step(images)
    assert base.retrieval_pose is None
    for kw in (dict(), dict(graph_retrieval=True), dict(retrieval_mode="weighted", temperature=0.05)):
        pipe = VPRGeoPosePipeline(ext, head, ShardedGallery(gal, n), k, labels=labels_np, scaler=SCALER, **kw)   # a host table is copied once
        for _ in range(2):
            out = pipe.step(images)
        torch.cuda.synchronize()
        want = torch.ops.vpr.retrieval_pose(out.topk_scores.contiguous(), out.topk_indices.contiguous(), labels,
                                            kw.get("retrieval_mode", "top1"), kw.get("temperature", 0.01), None, 0.0, SCALER)[1]
        assert out.retrieval_pose.shape == (B, 4) and out.retrieval_pose.dtype == torch.float32
        assert out.retrieval_pose.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
        assert not torch.isnan(out.retrieval_pose).any()
        for name in ("descriptors", "topk_scores", "topk_indices", "pose"):
            assert torch.equal(getattr(out, name), getattr(base, name)), (kw, name)


def test_retrieval_metrics_on_device_equals_the_host_path(dev):
    """Q = 37, k = 5 over N = 300.  Recalls: identical.  final_loss and maae: both paths are within the pose bound b of the
    long-double pose, so their poses differ by at most 2 b per entry, and
      final_loss = 0.5 / Q sum_q (dlat^2 + dlon^2):  |change| <= 0.5 / Q sum_q sum_c (2 |d_c| 2 b_c + (2 b_c)^2)
      maae = mean_q min(|a - t|, 360 - |a - t|), 1-Lipschitz in a circularly:  |change| <= mean_q 2 b_ang
    plus the roundings of evaluating the same formula on slightly different numbers: (Q + 4) 2^-52 relative for each mean,
    and 2^-52 * 360 for each angle difference."""
    from vpr_amd import evaluate
    labels = make_labels()
    rng = np.random.default_rng(12)
    Q, k, tau = 37, 5, 600.0
    vals, idx = make_lists(rng, Q, k, dead=False)
    q = make_targets(rng, idx, labels, tau)
    angles = (labels[idx[:, 0], 2] + rng.normal(0, 20, Q)) % 360.0
    tv, ti = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev)
    for mode in MODES:
        host = evaluate.retrieval_metrics(tv, ti, labels, q[:, :2], q[:, 2], angles, tau, mode, temperature=0.05)
        devm = evaluate.retrieval_metrics(tv, ti, labels, q[:, :2], q[:, 2], angles, tau, mode, on_device=True, temperature=0.05)
        assert list(host) == list(devm)
        for key in ("recall_at_1_tau", f"recall_at_{k}_tau", "recall_at_1_region"):
            assert host[key] == devm[key], key
        assert 0.0 < host["recall_at_1_tau"] <= host[f"recall_at_{k}_tau"] < 1.0
        assert np.array_equal(host["topk_indices"], devm["topk_indices"]) and np.array_equal(host["topk_scores"], devm["topk_scores"])
        _, _, _, _, R, smax = reference(vals, idx, labels, mode, 0.05)
        b64, _ = bounds(idx, labels, R, smax, 0.05)
        d = np.abs(host["pose"][:, :2] - q[:, :2])
        lim_loss = 0.5 / Q * (4 * d * b64[:, :2] + 4 * b64[:, :2] ** 2).sum() + (Q + 4) * 2.0 ** -52 * host["final_loss"]
        lim_maae = (2 * b64[:, 2]).mean() + (Q + 4) * 2.0 ** -52 * host["maae"] + 2.0 ** -52 * 360.0
        print(mode, "final_loss", host["final_loss"], abs(host["final_loss"] - devm["final_loss"]), lim_loss,
              "maae", host["maae"], abs(host["maae"] - devm["maae"]), lim_maae)
        assert abs(host["final_loss"] - devm["final_loss"]) <= lim_loss
        assert abs(host["maae"] - devm["maae"]) <= lim_maae
