"""Host-side unit check of the Krylov drivers' host arithmetic (tests/cpp/krylov_host_test.cc with
csrc/krylov_host.cpp and csrc/dense.cpp): the sparse-pattern updates behind the shifted copies of the inverse
and shift-invert drivers, the ARPACK++ defaults, the bookkeeping of one extension column with its breakdown
test, and the Arnoldi driver's Krylov-Schur restart (kept units, orthonormality and invariance of Z) on
12 x 12 Hessenberg matrices of known spectrum."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_krylov_host(tmp_path):
    out = str(tmp_path / "krylov_host_test")
    csrc = os.path.join(ROOT, "dune-eigensolver_amd", "csrc")
    # the test program and the two host sources alone: no library and no GPU runtime
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-ffp-contract=off",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "krylov_host_test.cc"),
                           os.path.join(csrc, "krylov_host.cpp"), os.path.join(csrc, "dense.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
