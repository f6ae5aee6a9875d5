"""Host-side unit check of the march-variant table, selection and planning (tests/cpp/march_select_test.cc
with csrc/march_plan.cpp): the traits of every variant, the variant march_select returns for every image
class and tune value, that the P1 Kuhn value-pack marches are not chosen where their 32-bit buffer
descriptor would wrap, and the plans, kernel names and byte counts of march_plan, marchg_plan
and the kernel queries against literals."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kuhn_pack_descriptor_guard(tmp_path):
    out = str(tmp_path / "march_select_test")
    # the test program and the planning source alone: host code, no library and no GPU runtime
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "march_select_test.cc"),
                           os.path.join(ROOT, "dune-eigensolver_amd", "csrc", "march_plan.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
