"""eigmi::Lobpcg, the C++ facade's wrapper over eig_lobpcg_* (include/eigmi.hh), compiled with the host
compiler against libeigmi.so the way tests/test_facade_cpp.py compiles its program:
tests/cpp/lobpcg_test.cc solves the 2-D Laplacian 16 x 16 and prints ALL OK."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lobpcg_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lobpcg") / "lobpcg_test")
    libdir = os.path.join(ROOT, "dune-eigensolver_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "lobpcg_test.cc"), "-L" + libdir, "-leigmi",
                           "-Wl,-rpath," + libdir, "-o", out])
    return out


def test_lobpcg_facade_compiles(lobpcg_bin):
    assert os.access(lobpcg_bin, os.X_OK)


@pytest.mark.gpu
def test_lobpcg_facade_on_gpu(lobpcg_bin):
    r = subprocess.run([lobpcg_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
