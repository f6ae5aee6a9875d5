"""bench.py end to end on the GPU at a small grid (32^3): a plain run times exactly --steps steps,
reports ms_per_step, carries none of the --full measurements, and --dump-outputs writes the alpha /
beta of the W + K steps -- identical from run to run and within 1e-12 of the fused restatement (the
bar of the fused step everywhere in the suite); --full adds the side measurements and baselines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

N, K, W = 32, 17, 3
FULL_ONLY = ("cpu_baseline", "csr", "stencil_shortcut", "general")


def run_bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--N", str(N),
                        "--steps", str(K), "--warmup", str(W), *extra], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return run_bench("--dump-outputs", str(d / "a")), d / "a"


def test_plain_line(plain):
    line, _ = plain
    assert line["steps"] == K and line["warmup"] == W and line["n_gpus"] == 1 and line["full"] is False
    assert line["unit"] == "iters/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0 and line["recurrence_finite"] is True
    # value = K / (timed wall time), ms_per_step = that time / K, the latter rounded to 1e-4 ms
    assert 1e3 / line["value"] == pytest.approx(line["ms_per_step"], abs=5.1e-5)
    assert line["spmv"] is None and not any(k in line for k in FULL_ONLY)
    assert "measured_copy_GBs" not in (line["roofline"] or {})


def test_dump_is_the_recurrence(plain):
    import oracle
    _, d = plain
    assert sorted(os.listdir(d)) == ["alpha.npy", "beta.npy"]
    alpha, beta = np.load(d / "alpha.npy"), np.load(d / "beta.npy")
    assert alpha.dtype == np.float64 and beta.dtype == np.float64
    assert alpha.shape == (W + K,) and beta.shape == (W + K + 1,)
    A = oracle.poisson3d(N)
    ra, rb = oracle.lanczos_fused(A, oracle.random_vec(A.n, 123), W + K)
    assert np.allclose(alpha, ra, rtol=1e-12, atol=0) and np.allclose(beta, rb, rtol=1e-12, atol=0)


def test_dump_repeats_bitwise(plain, tmp_path):
    _, d = plain
    run_bench("--dump-outputs", str(tmp_path / "b"))
    for f in ("alpha.npy", "beta.npy"):
        assert np.array_equal(np.load(d / f), np.load(tmp_path / "b" / f)), f


def test_full_adds_the_side_measurements():
    line = run_bench("--full", "--side-steps", "5", "--general-steps", "5", "--cpu-steps", "5", "--scipy-steps", "3",
                     "--cpu-replicas", "2", "--cpu-replica-steps", "3")
    assert line["full"] is True and line["steps"] == K
    assert line["spmv"]["us"] > 0 and line["roofline"]["measured_copy_GBs"] > 0
    for k in ("csr", "stencil_shortcut", "general"):
        assert line[k]["value"] > 0, k
    cb = line["cpu_baseline"]
    assert cb["value"] > 0 and cb["alpha_max_rel_diff_vs_gpu"] is not None
    assert cb["scipy_crosscheck"]["value"] > 0 and cb["replicas"]["cores"] == 2
