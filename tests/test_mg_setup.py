"""Host-side unit check of the multigrid hierarchy setup (tests/cpp/mg_setup_test.cc with csrc/mg_setup.cpp and
csrc/dense.cpp): the blocked Galerkin operator against an independent P^T A P on 66 x 9 x 17 (b = 3) and
17 x 40 x 12 (b = 4), its bitwise symmetry and 27-block rows, the block-Jacobi inverses and the block Gershgorin
bound against lower bounds of lambda_max(D^-1 A) and the dense spectrum, a literal coarse row of the scalar
(b = 1) path, and the refusals.  The same stand-alone program is also built with the address + undefined-behaviour
sanitizers and with the thread sanitizer (the Galerkin rows and the bound are computed by threads)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                                      ["-fsanitize=thread"]], ids=["plain", "asan-ubsan", "tsan"])
def test_mg_setup(tmp_path, sanitize):
    out = str(tmp_path / "mg_setup_test")
    csrc = os.path.join(ROOT, "dune-eigensolver_amd", "csrc")
    # the test program and the two host sources alone: no library and no GPU runtime
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
                          + sanitize +
                          [os.path.join(ROOT, "tests", "cpp", "mg_setup_test.cc"),
                           os.path.join(csrc, "mg_setup.cpp"), os.path.join(csrc, "dense.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
