"""Host-side unit check of the window filter's host code (tests/cpp/filter_host_test.cc with csrc/filter_host.cpp
and csrc/dense.cpp): the Jackson-damped coefficients, the scalars of the folded Clenshaw steps against the
textbook recurrence, the default degree, the refusals and the Lanczos spectrum bounds.  The same stand-alone
program is also built with the address + undefined-behaviour sanitizers and run as a program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan-ubsan"])
def test_filter_host(tmp_path, sanitize):
    out = str(tmp_path / "filter_host_test")
    csrc = os.path.join(ROOT, "dune-eigensolver_amd", "csrc")
    # the test program and the two host sources alone: no library and no GPU runtime
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
                          + sanitize +
                          [os.path.join(ROOT, "tests", "cpp", "filter_host_test.cc"),
                           os.path.join(csrc, "filter_host.cpp"), os.path.join(csrc, "dense.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
