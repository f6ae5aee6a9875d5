"""Host-side unit check of the matrix images (tests/cpp/mat_image_test.cc with csrc/mat_image.cpp and
csrc/gen.cpp): the SELL-64 image and its stencil slices read back to the input CSR, the symmetric band image read
back row by row, the cases in which no band image is built, the uniform / geometric / 27-point box decisions against
literal expectations, the interior / boundary slice split with its plane-march run, and a threaded build against a
one-thread build.  The same stand-alone program is also built with the address + undefined-behaviour sanitizers and
with the thread sanitizer (the passes share the band arrays and the masks across threads)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                                      ["-fsanitize=thread"]], ids=["plain", "asan-ubsan", "tsan"])
def test_mat_image(tmp_path, sanitize):
    out = str(tmp_path / "mat_image_test")
    csrc = os.path.join(ROOT, "dune-eigensolver_amd", "csrc")
    # the test program and the two host sources alone: no library and no GPU runtime
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
                          + sanitize +
                          [os.path.join(ROOT, "tests", "cpp", "mat_image_test.cc"),
                           os.path.join(csrc, "mat_image.cpp"), os.path.join(csrc, "gen.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
