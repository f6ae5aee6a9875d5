"""Host-side unit check of the smoothed-aggregation AMG setup (tests/cpp/amg_setup_test.cc with csrc/amg_setup.cpp,
csrc/mg_setup.cpp and csrc/dense.cpp): every row in exactly one aggregate, P against an independent dense
(I - omega D^-1 A) T on a 6 x 5 x 4 7-point grid and a 40-row random SPD pattern, A_c against a scattered P^T A P and
its bitwise symmetry, P^T's CSR the transpose of P's, every level of a three-level hierarchy, and the stall and
non-positive-diagonal refusals.  The same stand-alone program is also built with the address + undefined-behaviour
sanitizers and with the thread sanitizer (the products' rows are computed by threads)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                                      ["-fsanitize=thread"]], ids=["plain", "asan-ubsan", "tsan"])
def test_amg_setup(tmp_path, sanitize):
    out = str(tmp_path / "amg_setup_test")
    csrc = os.path.join(ROOT, "dune-eigensolver_amd", "csrc")
    # the test program and the three host sources alone: no library and no GPU runtime
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
                          + sanitize +
                          [os.path.join(ROOT, "tests", "cpp", "amg_setup_test.cc"), os.path.join(csrc, "amg_setup.cpp"),
                           os.path.join(csrc, "mg_setup.cpp"), os.path.join(csrc, "dense.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
