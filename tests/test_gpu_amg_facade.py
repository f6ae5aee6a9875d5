"""eigmi::Multigrid::amg and level_info, the C++ facade's wrappers over eig_amg_create and eig_mg_level_info
(include/eigmi.hh), compiled with the host compiler against libeigmi.so the way tests/test_gpu_mg_facade.py compiles
its program: tests/cpp/amg_facade_test.cc builds the hierarchy of the 12^3 Poisson matrix without its grid, solves,
runs LOBPCG with one V-cycle and prints ALL OK."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amg_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("amg_facade") / "amg_facade_test")
    libdir = os.path.join(ROOT, "dune-eigensolver_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "amg_facade_test.cc"), "-L" + libdir, "-leigmi",
                           "-Wl,-rpath," + libdir, "-o", out])
    return out


def test_amg_facade_compiles(amg_bin):
    assert os.access(amg_bin, os.X_OK)


@pytest.mark.gpu
def test_amg_facade_on_gpu(amg_bin):
    r = subprocess.run([amg_bin], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
