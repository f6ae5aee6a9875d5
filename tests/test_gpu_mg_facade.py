"""eigmi::Multigrid and eigmi::Lobpcg::precond_mg, the C++ facade's wrappers over eig_mg_* and
eig_lobpcg_precond_mg (include/eigmi.hh), compiled with the host compiler against libeigmi.so the way
tests/test_gpu_lobpcg_facade.py compiles its program: tests/cpp/mg_blocked_test.cc builds the multigrid on the
3x3-blocked q1elast(6), solves, runs LOBPCG with one V-cycle and prints ALL OK."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mg_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mg_blocked") / "mg_blocked_test")
    libdir = os.path.join(ROOT, "dune-eigensolver_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mg_blocked_test.cc"), "-L" + libdir, "-leigmi",
                           "-Wl,-rpath," + libdir, "-o", out])
    return out


def test_mg_facade_compiles(mg_bin):
    assert os.access(mg_bin, os.X_OK)


@pytest.mark.gpu
def test_mg_facade_on_gpu(mg_bin):
    r = subprocess.run([mg_bin], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
