"""Register allocation and LDS of a kernel as its kernel descriptor states them (what the dispatcher reserves per wave / per
workgroup), read from a code object: for library kernels such as hipBLASLt's, whose accumulation registers a kernel trace
reports as 0.  gfx90a and later: allocated registers per lane = 8 (granulated count + 1), arch + accumulation, the latter
from accum_offset up.  Needs llvm-readelf and, for a bundled .co, clang-offload-bundler (ROCm's llvm/bin); no GPU.
usage: python scripts/kernel_descriptor.py <file.co | file.hsaco> <kernel name> [gfx950]"""
import os, re, struct, subprocess, sys, tempfile

path, kernel = sys.argv[1], sys.argv[2]
arch = sys.argv[3] if len(sys.argv) > 3 else "gfx950"
llvm = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def tables(elf):
    run = lambda *a: subprocess.run([f"{llvm}/llvm-readelf", *a, elf], capture_output=True, text=True, check=True).stdout
    return open(elf, "rb").read(), run("-S"), run("-s")


if open(path, "rb").read(4) == b"\x7fELF":
    data, sections, symbols = tables(path)
else:                                       # an offload bundle: take the device object out
    with tempfile.TemporaryDirectory() as d:
        elf = os.path.join(d, "kernel.elf")
        subprocess.run([f"{llvm}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={path}",
                        f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}", f"--output={elf}"], check=True)
        data, sections, symbols = tables(elf)
sec = {}
for line in sections.splitlines():
    m = re.match(r"\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+[0-9a-f]+", line)
    if m:
        sec[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))      # address, file offset
line = next(l for l in symbols.splitlines() if l.strip().endswith(kernel + ".kd"))
f = line.split()
addr, (saddr, soff) = int(f[1], 16), sec[int(f[6])]
kd = data[soff + addr - saddr:soff + addr - saddr + 64]
lds, scratch = struct.unpack_from("<II", kd, 0)
rsrc3, rsrc1 = struct.unpack_from("<II", kd, 44)
alloc, accum_offset = ((rsrc1 & 0x3f) + 1) * 8, ((rsrc3 & 0x3f) + 1) * 4
print(f"{kernel}\n  registers per lane {alloc} (arch {accum_offset} + accumulation {alloc - accum_offset}), LDS {lds} B, scratch {scratch} B per lane\n"
      f"  beside one resident wave per SIMD a CU keeps {512 - alloc} registers per lane per SIMD and {160 * 1024 - lds} B of LDS")
