#!/usr/bin/env python3
"""Per-kernel register / scratch / LDS / occupancy from hipcc's kernel-resource-usage remarks, and
each kernel's code size from the symbol table of the device code object.

    python tools/resource_usage.py [--match name-regex] csrc/k_spmv.hip [csrc/k_march.hip ...]
(compiles the device code of each source for gfx950 into a temporary directory; prints ONE table
over all of them, one line per kernel, sorted by mangled name -- so the table of a file and the
table of the files it was split into compare with a plain diff.  Relative sources are resolved
against the package directory.)"""
import argparse
import os
import re
import subprocess
import tempfile

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dune-eigensolver_amd")
ROCM = "/opt/rocm"

ap = argparse.ArgumentParser()
ap.add_argument("--match", help="keep kernels whose demangled name matches this regex")
ap.add_argument("sources", nargs="+")
args = ap.parse_args()
pat = re.compile(args.match) if args.match else None

rows = {}  # mangled name -> remarks (+ "size")
with tempfile.TemporaryDirectory() as tmp:
    for src in args.sources:
        obj = os.path.join(tmp, os.path.basename(src) + ".o")
        cmd = [ROCM + "/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I../include",
               "--offload-arch=gfx950", "-munsafe-fp-atomics", "--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", obj,
               "-Rpass-analysis=kernel-resource-usage"]
        err = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, check=True).stderr
        cur = None
        for line in err.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = m.group(1)
                if cur in rows:
                    raise SystemExit(f"kernel defined twice: {cur}")
                rows[cur] = {}
                continue
            m = re.search(r"remark:\s+([^:]+): (\S+)", line)
            if cur and m:
                rows[cur][m.group(1).strip()] = m.group(2)
        syms = subprocess.run([ROCM + "/llvm/bin/llvm-readelf", "-sW", obj], capture_output=True, text=True,
                              check=True).stdout
        for line in syms.splitlines():
            f = line.split()
            if len(f) == 8 and f[3] == "FUNC" and f[7] in rows:
                rows[f[7]]["size"] = f[2]
for name in sorted(rows):
    r = rows[name]
    dn = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    if pat and not pat.search(dn):
        continue
    print(f"{name} vgpr {r.get('VGPRs', '?'):>4s} agpr {r.get('AGPRs', '?'):>3s} "
          f"sgpr {r.get('TotalSGPRs', '?'):>3s} scratch {r.get('ScratchSize [bytes/lane]', '?'):>4s} "
          f"lds {r.get('LDS Size [bytes/block]', '?'):>6s} occ {r.get('Occupancy [waves/SIMD]', '?'):>2s} "
          f"code {r.get('size', '?'):>6s}")
