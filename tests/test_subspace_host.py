"""Host-side unit check of the block eigensolvers' shared host arithmetic (tests/cpp/subspace_host_test.cc with
csrc/subspace_host.cpp and csrc/dense.cpp): Householder Q, LOBPCG's search coefficients, the small Rayleigh-Ritz
pick, the block tridiagonal, the shift-invert Ritz order, the convergence tests, the orthonormality deviation, the
Chebyshev-Jacobi scalars, CholQR2's reuse test and the MultiVector column unpack.  The same stand-alone program is
also built with the address + undefined-behaviour sanitizers and run as a program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan-ubsan"])
def test_subspace_host(tmp_path, sanitize):
    out = str(tmp_path / "subspace_host_test")
    csrc = os.path.join(ROOT, "dune-eigensolver_amd", "csrc")
    # the test program and the two host sources alone: no library and no GPU runtime
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
                          + sanitize +
                          [os.path.join(ROOT, "tests", "cpp", "subspace_host_test.cc"),
                           os.path.join(csrc, "subspace_host.cpp"), os.path.join(csrc, "dense.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
