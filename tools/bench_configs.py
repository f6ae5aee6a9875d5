#!/usr/bin/env python3
"""Per-configuration measurements beside bench.py's headline line (BASELINE.json configs):

  C1  2-D Poisson 64x64: StandardLargest (ini defaults) and the Lanczos solver on the GPU, the
      oracle (reference CPU path) timed on the same inputs
  C2  3-D Poisson 128^3: SpMV (cache-resident: 217 MB < 256 MB MALL), Lanczos step, the b = 8
      SpMM, block Gram-Schmidt (m = 8, 32) and one StandardLargest iteration vs the CPU path
  C3  3-D Q1 elasticity 64^3, 3x3 blocks: BCSR SpMV against 76 nnzb + 4 (nb+1) + 48 nb bytes, the
      blocked SpMM, the Lanczos step on blocks (two-kernel and fused, alternated twice), and the
      blocked pencil K, M = D + 0.3 (K - D): the Chebyshev step k_spmm_blk_mv8_cheb (m = 8, 32)
      beside the same run's product, and the block Lanczos k = 32 step's phase split
  INV inverse iteration with exported LU factors on the harness matrices:
      matmul_inverse_tallskinny_blocked (m = 8), StandardInverse, GeneralizedInverse (GenEO pencil)
      and computeGenSymShiftInvertMinMagnitude, GPU vs the oracle / scipy ARPACK on the host
  C5  generalised K x = lambda M x, P1 on the Kuhn split (15-pt shared pattern), block Lanczos
      k = 32: block steps/s with the phase split, the fused Chebyshev SpMM kernel against
      12 nnz + 4 (n+1) + (32 m + 8) n bytes per m-column launch (EIGMI_C5_N, default 256)
  LOBPCG  the smallest end of the C5 pencil by LOBPCG with one multigrid V-cycle per iteration, its two
      streaming kernels alone, the fused update A/B against four panel updates, and c5si beside it
  MGBLK  the blocked multigrid on the C3 matrix (q1elast 64^3, 3x3): setup, one V-cycle at m = 8 and 32, the
      blocked residual and the point Chebyshev step beside the same run's blocked product (interleaved), and
      LOBPCG block 32 on the C3 pencil with one V-cycle against Chebyshev-Jacobi degree 4; mgblk_stats turns
      the kernel-trace summary of that run into one line per blocked kernel (block-Jacobi step, transfers)
  AMG  smoothed-aggregation AMG on the bench's `general` matrix (3-D Poisson 128^3, scrambled + reverse
      Cuthill-McKee, SELL with explicit columns): setup, levels and operator complexity, one V-cycle at m = 8 and
      32 beside the geometric multigrid's on the unscrambled matrix in the same process (interleaved), the
      residual per cycle, the transfers' algorithmic bytes, and LOBPCG block 32 with one AMG V-cycle against
      Chebyshev-Jacobi degree 4; amg_stats turns a kernel trace of that run into one line per transfer kernel
      and level
  SLICE  the Chebyshev window filter's fused step (eig_filter_step_mv8's kernels) beside the Chebyshev-Jacobi
      step of the mass solve in one process on the same image, alternated: 128^3 row-class m = 8, 256^3
      variable-coefficient box image m = 32, the `general` SELL matrix 128^3 m = 32, C3 blocks m = 8 and 32;
      one outer iteration's split at 256^3 x 32; and a full run on kind 8 at 128^3 (a window of about 10
      eigenvalues sized with eig_filter_count, iterations to tol 1e-8).  EIGMI_SLICE_CASES picks a subset

One JSON line per measurement; algorithmic bytes per SURVEY 8(d); peak 8 TB/s.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dune-eigensolver_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

import eigmi  # noqa: E402
import oracle  # noqa: E402  (CPU baseline only)

PEAK = 8000.0


def emit(**kw):
    print(json.dumps(kw), flush=True)


def wall(f, reps=1):
    t0 = time.perf_counter()
    for _ in range(reps):
        r = f()
    return (time.perf_counter() - t0) / reps, r


def c1(ctx):
    A = oracle.laplace2d(64)
    M = eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val)
    eigmi.standard_largest(M, 0.0, 2e-3, 4000, 4, 123, want_evec=False)  # warm-up
    tg, (ev, _, it) = wall(lambda: eigmi.standard_largest(M, 0.0, 2e-3, 4000, 4, 123, want_evec=False), 3)
    tc, (rev, _, rit) = wall(lambda: oracle.standard_largest(A, 0.0, 2e-3, 4000, 4, 123), 3)
    emit(config="C1 2D Poisson 64^2", op="StandardLargest nev=4 tol=2e-3 seed=123", gpu_s=round(tg, 5),
         cpu_s=round(tc, 5), iterations=it, cpu_iterations=rit, ritz0=ev[0], max_abs_diff_vs_cpu=float(np.abs(ev - rev).max()))
    tl, (ev, _, res) = wall(lambda: eigmi.lanczos_solve(M, 4, 300, eigmi.WHICH_LA, want_evec=False))
    emit(config="C1 2D Poisson 64^2", op="Lanczos solve LA nev=4 ncv=300 (full re-orth)", gpu_s=round(tl, 5),
         eigenvalues=list(ev), max_residual=float(res.max()))


def c2(ctx):
    """Config C2 (3-D Poisson 128^3).  The band values are read from HBM (EIG_MAT_NO_UNIFORM, as the
    benchmark's image) unless EIGMI_C2_UNIFORM=1 (the constant-coefficient shortcut)."""
    N = 128
    n = N ** 3
    rp, c, v = eigmi.gen_matrix(eigmi.GEN_POISSON3D, N)
    nnz = int(rp[-1])
    uni = os.environ.get("EIGMI_C2_UNIFORM", "0") == "1"
    M = eigmi.Matrix.from_bcsr(ctx, rp, c, v, flags=0 if uni else eigmi.MAT_NO_UNIFORM)
    image = "stencil-only (values in the kernel arguments)" if uni else "value-streaming (band values read)"

    def emit(**kw):  # every C2 line names its image
        globals()["emit"](image=image, **kw)
    x = ctx.array(np.random.default_rng(0).standard_normal(n))
    y = ctx.zeros(n)
    M.mv_timed(x, y, 10)
    ms = M.mv_timed(x, y, 200)
    # algorithmic bytes of the image the kernel streams (band image: 8 B per band slot + the row
    # mask), the survey's CSR count beside it
    b = eigmi.image_bytes(M, "spmv")
    csr = eigmi.bytes_spmv(n, nnz)
    gbs = b / (ms * 1e-3) / 1e9
    A = oracle.CSR(n, rp, c, v)
    xh = x.get()
    tc, _ = wall(lambda: oracle.csr_mv(A, xh), 3)
    emit(config="C2 3D Poisson 128^3", op=f"SpMV (cache-resident: {b / 2**20:.0f} MiB < 256 MiB MALL)",
         us=round(ms * 1e3, 2), algorithmic_bytes=b, GBs=round(gbs, 1), frac=round(gbs / PEAK, 4),
         csr_bytes=csr, csr_equiv_GBs=round(csr / (ms * 1e-3) / 1e9, 1), cpu_us=round(tc * 1e6, 1),
         cpu_GBs=round(csr / tc / 1e9, 2))
    ws = eigmi.LanczosWorkspace(M, 210, seed=123)
    ws.step(10)
    t = ws.step(200, timed="detail")
    k1_name, k1_bytes = M.lanczos_kernel_info(False)
    emit(config="C2 3D Poisson 128^3", op="Lanczos step (classic: K1 + update)",
         it_per_s=round(200 / (t.total_ms * 1e-3), 1), k1=k1_name,
         k1_us=round(t.spmv_ms / 200 * 1e3, 2), k2_us=round(t.update_ms / 200 * 1e3, 2),
         step_frac=round((k1_bytes + 24 * n) / (t.total_ms / 200 * 1e-3) / 1e9 / PEAK, 4))
    ws.close()
    ws = eigmi.LanczosWorkspace(M, 210, seed=123, fused=True)
    ws.step(10)
    t = ws.step(200, timed=True)
    kf_name, kf_bytes = M.lanczos_kernel_info(True)
    emit(config="C2 3D Poisson 128^3", op="Lanczos step (fused, bench default)",
         it_per_s=round(200 / (t.total_ms * 1e-3), 1), kernel=kf_name, kernel_us=round(t.spmv_ms / 200 * 1e3, 2),
         kernel_frac=round(kf_bytes / (t.spmv_ms / 200 * 1e-3) / 1e9 / PEAK, 4))
    ws.close()
    for m in (8, 32):
        Qh = oracle.random_mv8(n, m, 1)
        Q, Y = ctx.array(Qh), ctx.zeros(n * m)
        eigmi.spmm_mv8(M, m, Q, Y)
        ctx.sync()

        def spmm_batch(reps=20):
            # kernel throughput: back-to-back launches, one synchronisation (a synchronisation per call
            # adds ~12 us of host round trip to a 47 us kernel)
            t0 = time.perf_counter()
            for _ in range(reps):
                eigmi.spmm_mv8(M, m, Q, Y)
            ctx.sync()
            return (time.perf_counter() - t0) / reps
        tg = min(spmm_batch() for _ in range(3))
        sb = eigmi.image_bytes(M, "spmm", m)
        emit(config="C2 3D Poisson 128^3", op=f"SpMM b=8 m={m}", us=round(tg * 1e6, 1), algorithmic_bytes=sb,
             GBs=round(sb / tg / 1e9, 1), frac=round(sb / tg / 1e9 / PEAK, 4),
             csr_equiv_GBs=round((12 * nnz + 4 * (n + 1) + 128 * n * (m // 8)) / tg / 1e9, 1))
        Q.upload(Qh)
        eigmi.orthonormalize_mv8(ctx, n, m, Q)
        ctx.sync()

        def ortho():
            Q.upload(Qh)
            ctx.sync()
            t0 = time.perf_counter()
            eigmi.orthonormalize_mv8(ctx, n, m, Q)
            ctx.sync()
            return time.perf_counter() - t0
        tg = min(ortho() for _ in range(3))
        tc, _ = wall(lambda: oracle.orthonormalize_mv8(Qh, n, m))
        ob = eigmi.lib.eig_bytes_orthonormalize_blocked(n, m, 8)
        of = eigmi.lib.eig_flops_orthonormalize(n, m)
        emit(config="C2 3D Poisson 128^3", op=f"orthonormalize_blocked (MGS) m={m}", gpu_ms=round(tg * 1e3, 3),
             cpu_ms=round(tc * 1e3, 1), model_bytes=ob, model_GBs=round(ob / tg / 1e9, 1),
             model_GFLOPs=round(of / tg / 1e9, 1), speedup=round(tc / tg, 1))
    # one StandardLargest iteration at m = 8, timed as the driver runs it (eigensolver.hh:78-96 with
    # the :78 product reused from the previous iteration's :84, SURVEY Appendix A.6: orthonormalize_blocked,
    # ONE SpMM, diagonal dots copied to the host for the stopping test) and in the reference's order
    # (two SpMMs); differencing whole solves of different lengths drowned the 10-iteration difference
    # in the host generation of the random start block
    m = 8
    Q1, Q2, dp = ctx.array(oracle.random_mv8(n, m, 1)), ctx.zeros(n * m), ctx.zeros(m)
    eigmi.orthonormalize_mv8(ctx, n, m, Q1)

    def iteration_two_spmm():
        eigmi.spmm_mv8(M, m, Q1, Q2)
        eigmi.orthonormalize_mv8(ctx, n, m, Q2)
        eigmi.spmm_mv8(M, m, Q2, Q1)
        eigmi.dot_diag_mv8(ctx, n, m, Q2, Q1, dp)
        dp.get()
    iteration_two_spmm()
    ctx.sync()
    tg2, _ = wall(iteration_two_spmm, 20)
    state = [Q1, Q2]
    eigmi.spmm_mv8(M, m, Q1, Q2)

    def iteration():
        q1, q2 = state  # q2 = A q1 (the previous iteration's second product)
        eigmi.orthonormalize_mv8(ctx, n, m, q2)
        eigmi.spmm_mv8(M, m, q2, q1)
        eigmi.dot_diag_mv8(ctx, n, m, q2, q1, dp)
        dp.get()
        state.reverse()  # the swap: Q1 <- the orthonormal block, Q2 <- its product
    iteration()
    ctx.sync()
    tg, _ = wall(iteration, 20)
    # the driver itself (one-iteration look-ahead, no host round trip between iterations): the
    # difference of 212- and 12-iteration solves (tol 0 runs to maxiter), best of 3 each
    k0, k1 = 12, 212
    ta = min(wall(lambda: eigmi.standard_largest(M, 0.0, 0.0, k0, 8, 123, want_evec=False))[0] for _ in range(3))
    tb = min(wall(lambda: eigmi.standard_largest(M, 0.0, 0.0, k1, 8, 123, want_evec=False))[0] for _ in range(3))
    td = (tb - ta) / (k1 - k0)
    tc1, _ = wall(lambda: oracle.standard_largest(A, 0.0, 0.0, 2, 8, 123))
    tc2, _ = wall(lambda: oracle.standard_largest(A, 0.0, 0.0, 3, 8, 123))
    emit(config="C2 3D Poisson 128^3", op="StandardLargest iteration m=8", gpu_ms_per_iter=round(td * 1e3, 3),
         gpu_ms_per_iter_synced=round(tg * 1e3, 3), gpu_ms_per_iter_two_spmm_synced=round(tg2 * 1e3, 3),
         cpu_ms_per_iter=round((tc2 - tc1) * 1e3, 1), speedup=round((tc2 - tc1) / td, 1),
         note="gpu_ms_per_iter: the driver (one SpMM per iteration, look-ahead); *_synced: python loops of "
              "the same primitives with a host round trip per iteration, with one or with the reference's two SpMMs; "
              "the CPU restatement runs the reference's two")


def gram(ctx):
    """a6 panel Gram G = Q1^T Q2 (k_gram_mv8) and a9 orthonormalize_blocked at C2 size (n = 128^3):
    per call, 50 back-to-back calls between two synchronisations; algorithmic bytes 8 n (m1 + m2)."""
    n = int(os.environ.get("EIGMI_GRAM_N", str(128 ** 3)))
    reps = 50
    for m1, m2 in ((8, 8), (8, 16), (8, 24), (32, 32)):
        Q1, Q2, G = ctx.array(oracle.random_mv8(n, m1, 1)), ctx.array(oracle.random_mv8(n, m2, 2)), ctx.zeros(m1 * m2)
        eigmi.gram_mv8(ctx, n, m1, m2, Q1, Q2, G)
        ctx.sync()
        def batch():
            t0 = time.perf_counter()
            for _ in range(reps):
                eigmi.gram_mv8(ctx, n, m1, m2, Q1, Q2, G)
            ctx.sync()
            return (time.perf_counter() - t0) / reps
        tg = min(batch() for _ in range(3))
        b = 8 * n * (m1 + m2)
        emit(config=f"gram n={n}", op=f"gram_mv8 m1={m1} m2={m2}", us=round(tg * 1e6, 2), algorithmic_bytes=b,
             GBs=round(b / tg / 1e9, 1), frac=round(b / tg / 1e9 / PEAK, 4))
        Q1.free(), Q2.free(), G.free()
    # block Lanczos panel products at C5 size (n = 256^3, eig_panel_gram_mv8: V^T (M Z) of CGS, k = 32)
    nc5 = int(os.environ.get("EIGMI_GRAM_N5", str(256 ** 3)))
    for m1, m2 in ((32, 32), (96, 32), (256, 32)):
        Q1, Q2, G = ctx.zeros(nc5 * m1), ctx.zeros(nc5 * m2), ctx.zeros(m1 * m2)
        # (timing only: a constant byte pattern, 0x3F3F... = 4.8e-4 per entry, instead of host random numbers)
        eigmi.lib.eig_memset(ctx.h, Q1.ptr, 0x3F, nc5 * m1 * 8)
        eigmi.lib.eig_memset(ctx.h, Q2.ptr, 0x3F, nc5 * m2 * 8)
        eigmi.panel_gram_mv8(ctx, nc5, m1, m2, Q1, Q2, G)
        ctx.sync()

        def batch5():
            t0 = time.perf_counter()
            for _ in range(5):
                eigmi.panel_gram_mv8(ctx, nc5, m1, m2, Q1, Q2, G)
            ctx.sync()
            return (time.perf_counter() - t0) / 5
        tg = min(batch5() for _ in range(3))
        b = 8 * nc5 * (m1 + m2)
        emit(config=f"panel gram n={nc5}", op=f"panel_gram_mv8 m1={m1} m2={m2}", us=round(tg * 1e6, 2),
             algorithmic_bytes=b, GBs=round(b / tg / 1e9, 1), frac=round(b / tg / 1e9 / PEAK, 4))
        Q1.free(), Q2.free(), G.free()
    for m in (8, 32):
        Qh = oracle.random_mv8(n, m, 1)
        Q = ctx.array(Qh)

        def ortho():
            Q.upload(Qh)
            ctx.sync()
            t0 = time.perf_counter()
            eigmi.orthonormalize_mv8(ctx, n, m, Q)
            ctx.sync()
            return time.perf_counter() - t0
        ortho()
        tg = min(ortho() for _ in range(5))
        ob = eigmi.lib.eig_bytes_orthonormalize_blocked(n, m, 8)
        emit(config=f"gram n={n}", op=f"orthonormalize_blocked (MGS) m={m}", gpu_ms=round(tg * 1e3, 3),
             model_bytes=ob, model_GBs=round(ob / tg / 1e9, 1))
        Q.free()


def ortho(ctx):
    """a9 orthonormalize_blocked at C2 size (n = 128^3), m = 8 / 32, best of 5 calls, against the
    reference's byte model (kernels_cpp.hh:157-175): the Gram look-ahead MGS with windows L = 8, 4, 2
    (EIG_ORTHO_LOOKAHEAD; read passes reported) and the stepwise replay (L = 1; EIGMI_MGS_INPLACE=1
    times the in-place passes there)."""
    n = 128 ** 3
    step_tag = ("in-place passes" if os.environ.get("EIGMI_MGS_INPLACE") else
                "one cooperative launch, grid barriers" if os.environ.get("EIGMI_MGS_COOP") else
                f"read-only replay passes, grid <= {os.environ.get('EIGMI_MGS_GRID', '512')}")
    for m in (8, 32):
        Qh = oracle.random_mv8(n, m, 1)
        Q = ctx.array(Qh)
        for L in (8, 4, 2, 1):
            var = eigmi.ORTHO_MGS | eigmi.ORTHO_LOOKAHEAD(L)

            def once():
                Q.upload(Qh)
                ctx.sync()
                t0 = time.perf_counter()
                eigmi.orthonormalize_mv8(ctx, n, m, Q, var)
                ctx.sync()
                return time.perf_counter() - t0
            once()
            tg = min(once() for _ in range(5))
            passes = eigmi.orthonormalize_passes(ctx) if L > 1 else 8
            tag = f"Gram look-ahead L={L}, {passes} read passes" if L > 1 else step_tag
            ob = eigmi.lib.eig_bytes_orthonormalize_blocked(n, m, 8)
            emit(config="C2 128^3", op=f"orthonormalize_blocked (MGS, {tag}) m={m}", gpu_ms=round(tg * 1e3, 4),
                 model_bytes=ob, model_GBs=round(ob / tg / 1e9, 1), model_frac=round(ob / tg / 1e9 / PEAK, 4))
        Q.free()


def c3(ctx):
    N = 64
    rp, c, v = eigmi.gen_matrix(eigmi.GEN_Q1ELAST3D, N)
    nb = N ** 3
    nnzb = int(rp[-1])
    M = eigmi.Matrix.from_bcsr(ctx, rp, c, v, 3, 3)
    x = ctx.array(np.random.default_rng(0).standard_normal(3 * nb))
    y = ctx.zeros(3 * nb)
    M.mv_timed(x, y, 5)
    ms = M.mv_timed(x, y, 100)
    b = 76 * nnzb + 4 * (nb + 1) + 48 * nb
    gbs = b / (ms * 1e-3) / 1e9
    A = oracle.CSR(nb, rp, c, v, 3, 3)
    xh = x.get()
    tc, _ = wall(lambda: oracle.csr_mv(A, xh))
    emit(config="C3 Q1 elasticity 64^3 3x3 BCSR", op="BCSR SpMV", us=round(ms * 1e3, 2), nnzb=nnzb,
         algorithmic_bytes=b, GBs=round(gbs, 1), frac=round(gbs / PEAK, 4), cpu_us=round(tc * 1e6, 1),
         cpu_GBs=round(b / tc / 1e9, 2))
    # the blocked tall-skinny product (k_spmm_blk_mv8) beside it: back-to-back launches, one
    # synchronisation (as C2's SpMM); the alternative a caller had before it is m eig_mv launches
    n = 3 * nb
    for m in (8, 32):
        Q, Y = ctx.array(oracle.random_mv8(n, m, 1)), ctx.zeros(n * m)
        eigmi.spmm_blk_mv8(M, m, Q, Y)
        ctx.sync()

        def spmm_batch(reps=20):
            t0 = time.perf_counter()
            for _ in range(reps):
                eigmi.spmm_blk_mv8(M, m, Q, Y)
            ctx.sync()
            return (time.perf_counter() - t0) / reps
        tg = min(spmm_batch() for _ in range(3))
        sb = 76 * nnzb + 4 * (nb + 1) + 2 * 8 * m * 3 * nb
        emit(config="C3 Q1 elasticity 64^3 3x3 BCSR", op=f"blocked SpMM m={m}", kernel=M.kernel("spmm8"),
             us=round(tg * 1e6, 2), algorithmic_bytes=sb, GBs=round(sb / tg / 1e9, 1),
             frac=round(sb / tg / 1e9 / PEAK, 4), mv_us=round(ms * 1e3, 2), m_mv_us=round(m * ms * 1e3, 2),
             ratio_vs_m_mv=round(tg / (m * ms * 1e-3), 4))
        Q.free(), Y.free()
    # the Lanczos step on the blocked image: the two-kernel step (k_lanczos_spmv_blk + k_lanczos_update)
    # and the fused one-reduction step (k_lanczos_fused_blk), alternated twice so the run-to-run
    # spread shows; per variant 10 warm-up steps, 200 steps untimed inside (step_us, from the batch's
    # two events) and 200 with per-kernel events (kernel_us); eig_mv timed again beside each
    steps = 200
    for rnd in range(2):
        for fused in (False, True):
            mv_ms = M.mv_timed(x, y, 100)
            ws = eigmi.LanczosWorkspace(M, 10 + 2 * steps, seed=123, fused=fused)
            ws.step(10)
            t = ws.step(steps)
            tk = ws.step(steps, timed=True if fused else "detail")
            launches = int(tk.spmv_launches)
            kus = tk.spmv_ms / launches * 1e3
            extra = {} if fused else {"k2_us": round(tk.update_ms / steps * 1e3, 2)}
            emit(config="C3 Q1 elasticity 64^3 3x3 BCSR", op="Lanczos step (fused)" if fused else "Lanczos step (classic: K1 + update)",
                 round=rnd, variant=ws.variant, step_us=round(t.total_ms / steps * 1e3, 2), kernel=ws.kernel,
                 kernel_us=round(kus, 2), kernel_launches=launches, model_bytes=ws.kernel_bytes,
                 kernel_frac=round(ws.kernel_bytes / (kus * 1e-6) / 1e9 / PEAK, 4), mv_us=round(mv_ms * 1e3, 2),
                 step_vs_mv=round(t.total_ms / steps / mv_ms, 4), kernel_vs_mv=round(kus * 1e-3 / mv_ms, 4), **extra)
            ws.close()
    c3_pencil(ctx, M, rp, c, v, nb, nnzb)


def c3_pencil(ctx, K, rp, c, v, nb, nnzb):
    """The blocked pencil of C3: K = q1elast(64) and M = D + 0.3 (K - D) built on the host (D the scalar
    diagonal of K, constant 16/3: same pattern, bitwise symmetric, spec(D^-1 M) = 0.7 + 0.3 spec(D^-1 K)
    inside the default Chebyshev bounds [0.5, 2.5]).  The Chebyshev step k_spmm_blk_mv8_cheb from the
    difference of two solve degrees beside the same run's blocked product, and the block step's split."""
    n = 3 * nb
    cfg = "C3 Q1 elasticity 64^3 3x3 BCSR"
    v3 = v.reshape(-1, 3, 3)
    dg = np.nonzero(c == np.repeat(np.arange(nb), np.diff(rp)))[0][:, None]
    r = np.arange(3)
    vm = 0.3 * v3
    vm[dg, r, r] = v3[dg, r, r]
    M = eigmi.Matrix.from_bcsr(ctx, rp, c, vm.reshape(-1), 3, 3)
    d0, d1 = 2, 22
    for m in (8, 32):
        B, X, R = ctx.array(oracle.random_mv8(n, m, 2)), ctx.zeros(n * m), ctx.zeros(n * m)
        # the tool's own check of the solve at the degree the block step uses
        eigmi.mass_solve_mv8(M, m, 36, B, X)
        eigmi.spmm_blk_mv8(M, m, X, R)
        bh = B.get()
        resid = float(np.linalg.norm(bh - R.get()) / np.linalg.norm(bh))
        assert resid <= 1e-12, f"mass solve residual {resid:.2e} at degree 36"
        eigmi.spmm_blk_mv8(K, m, B, R)
        ctx.sync()

        def spmm_batch(reps=20):
            t0 = time.perf_counter()
            for _ in range(reps):
                eigmi.spmm_blk_mv8(M, m, B, R)
            ctx.sync()
            return (time.perf_counter() - t0) / reps
        ts = min(spmm_batch() for _ in range(3))
        t0 = min(wall(lambda: (eigmi.mass_solve_mv8(M, m, d0, B, X), ctx.sync()), 5)[0] for _ in range(3))
        t1 = min(wall(lambda: (eigmi.mass_solve_mv8(M, m, d1, B, X), ctx.sync()), 5)[0] for _ in range(3))
        tc = (t1 - t0) / (d1 - d0)
        sb = 76 * nnzb + 4 * (nb + 1) + 2 * 8 * m * n   # the product
        add = 2 * 8 * m * n + 8 * n                     # b and x_{k-1}, dinv (the row's own x_k from L2)
        emit(config=cfg, op=f"blocked Chebyshev step m={m}", kernel="k_spmm_blk_mv8_cheb", us=round(tc * 1e6, 2),
             algorithmic_bytes=sb + add, GBs=round((sb + add) / tc / 1e9, 1), frac=round((sb + add) / tc / 1e9 / PEAK, 4),
             spmm_us=round(ts * 1e6, 2), spmm_GBs=round(sb / ts / 1e9, 1),
             spmm_plus_1p5_added_us=round(ts * 1e6 * (1.0 + 1.5 * add / sb), 2), degree36_residual=resid)
        B.free(), X.free(), R.free()
    steps, warm, b, degree = 4, 1, 32, 36
    bl = eigmi.BlockLanczos(K, M, block=b, max_steps=steps + warm, degree=degree, seed=123)
    bl.step(warm)
    t = bl.step(steps)
    ev, _, _ = bl.ritz(4, eigmi.WHICH_LA, want_resid=False)
    emit(config=cfg, op=f"block Lanczos k={b} step (Chebyshev degree {degree}, CGS2, CholQR2)",
         ms_per_step=round(t.total_ms / steps, 2), kspmm_ms=round(t.kspmm_ms / steps, 2),
         cheb_ms=round(t.cheb_ms / steps, 2), orth_ms=round(t.orth_ms / steps, 2), norm_ms=round(t.norm_ms / steps, 2),
         cheb_launches=int(t.cheb_launches), cheb_kernel_us=round(t.cheb_ms / t.cheb_launches * 1e3, 1),
         top_ritz=[float(x) for x in ev], steps_taken=steps + warm)
    bl.close()
    M.close()


def inv(ctx):
    import scipy.sparse.linalg as ssl
    N = int(os.environ.get("EIGMI_INV_N", "64"))
    A = oracle.laplace2d(N)
    n = A.n
    lu = eigmi.LU.from_bcsr(ctx, A.rowptr, A.col, A.val)
    f = oracle.LU(**lu.export())
    lnz, unz = f.Lp[-1], f.Up[-1]
    X = oracle.random_mv8(n, 8, 1)
    din, dout = ctx.array(X), ctx.zeros(n * 8)
    lu.inverse_mv8(8, din, dout)
    ctx.sync()
    reps = 20
    tg, _ = wall(lambda: (lu.inverse_mv8(8, din, dout), ctx.sync()), reps)
    tc, _ = wall(lambda: oracle.inverse_mv8(f, X, 8), 3)
    emit(config=f"INV 2D Dirichlet {N}^2", op="matmul_inverse_tallskinny_blocked m=8 (RCM envelope factors)",
         lnz=int(lnz), unz=int(unz), gpu_us=round(tg * 1e6, 1), cpu_us=round(tc * 1e6, 1), speedup=round(tc / tg, 2),
         note="triangular solves are a row dependency chain: latency-bound, no bandwidth roofline")
    M = eigmi.Matrix.from_bcsr(ctx, A.rowptr, A.col, A.val)
    eigmi.standard_inverse(M, 0.0, 1e-10, 2000, 8, 123, want_evec=False)
    tg, (ev, _, it) = wall(lambda: eigmi.standard_inverse(M, 0.0, 1e-10, 2000, 8, 123, want_evec=False))
    tc, (rev, _, rit) = wall(lambda: oracle.standard_inverse(A, f, 0.0, 1e-10, 2000, 8, 123))
    emit(config=f"INV 2D Dirichlet {N}^2", op="StandardInverse nev=8 tol=1e-10", gpu_s=round(tg, 4), cpu_s=round(tc, 4),
         iterations=it, cpu_iterations=rit, speedup=round(tc / tg, 2), max_rel_diff=float(np.max(np.abs(ev - rev) / np.abs(rev))),
         note="gpu_s includes the factorization (host RCM + device band LU + block-inverse image); cpu_s is the "
              "iteration with the factors given")
    # the same driver with the factors given on both sides (eigensolver.hh:156 factors inside the
    # driver; the factorisation is host work on both sides, so this row times the iteration alone)
    eigmi.standard_inverse(M, 0.0, 1e-10, 2000, 8, 123, lu=lu, want_evec=False)
    tg, (ev, _, it) = wall(lambda: eigmi.standard_inverse(M, 0.0, 1e-10, 2000, 8, 123, lu=lu, want_evec=False), 3)
    emit(config=f"INV 2D Dirichlet {N}^2", op="StandardInverse nev=8 tol=1e-10, factors given", gpu_s=round(tg, 4),
         cpu_s=round(tc, 4), iterations=it, cpu_iterations=rit, speedup=round(tc / tg, 2),
         max_rel_diff=float(np.max(np.abs(ev - rev) / np.abs(rev))))
    shift, reg = 1e-3, 0.0
    An, Bp = oracle.laplace2d(N, "neumann"), oracle.laplace2d(N, "pu", overlap=3)
    dA = eigmi.Matrix.from_bcsr(ctx, An.rowptr, An.col, An.val)
    dB = eigmi.Matrix.from_bcsr(ctx, Bp.rowptr, Bp.col, Bp.val)
    tg, (ev, _, it) = wall(lambda: eigmi.generalized_inverse(dA, dB, shift, reg, 1e-8, 4000, 8, 123, want_evec=False))
    As = oracle.CSR(An.nrows, An.rowptr, An.col, An.val + shift * Bp.val)
    fs = oracle.LU(**eigmi.LU.from_bcsr(None, As.rowptr, As.col, As.val).export())
    tc, (rev, _, rit) = wall(lambda: oracle.generalized_inverse(An, Bp, fs, shift, reg, 1e-8, 4000, 8, 123))
    emit(config=f"INV GenEO pencil {N}^2 (.cc:455-512)", op="GeneralizedInverse nev=8 tol=1e-8", gpu_s=round(tg, 4),
         cpu_s=round(tc, 4), iterations=it, cpu_iterations=rit, speedup=round(tc / tg, 2),
         note="gpu_s includes the shifted copy and the factorization (device band LU); cpu_s is the iteration with "
              "the factors given")
    lus = eigmi.LU.from_bcsr(ctx, As.rowptr, As.col, As.val)
    eigmi.generalized_inverse(dA, dB, shift, reg, 1e-8, 4000, 8, 123, lu=lus, want_evec=False)
    tg, (ev, _, it) = wall(lambda: eigmi.generalized_inverse(dA, dB, shift, reg, 1e-8, 4000, 8, 123, lu=lus,
                                                             want_evec=False), 3)
    emit(config=f"INV GenEO pencil {N}^2 (.cc:455-512)", op="GeneralizedInverse nev=8 tol=1e-8, factors given",
         gpu_s=round(tg, 4), cpu_s=round(tc, 4), iterations=it, cpu_iterations=rit, speedup=round(tc / tg, 2),
         max_diff_rel_to_largest=float(np.max(np.abs(ev - rev)) / np.max(np.abs(rev))))  # (the pencil has lambda = 0)
    As_, Bs_ = An.to_scipy(), Bp.to_scipy()
    tc, w = wall(lambda: ssl.eigsh(As_, k=8, M=Bs_, sigma=-shift, which="LM", tol=1e-10, return_eigenvectors=False))
    for method in ("block", "single"):
        tg, (ev, _, r) = wall(lambda: eigmi.shift_invert_solve(dA, 8, sigma=-shift, B=dB, tol=1e-10, want_evec=False,
                                                               method=method))
        emit(config=f"INV GenEO pencil {N}^2 (.cc:455-512)", op="computeGenSymShiftInvertMinMagnitude nev=8 tol=1e-10",
             method=method, gpu_s=round(tg, 4), scipy_arpack_cpu_s=round(tc, 4), restarts=r, speedup=round(tc / tg, 2),
             max_abs_diff_vs_arpack=float(np.max(np.abs(np.sort(ev) - np.sort(w)))),
             note="both sides include the factorisation (here: host RCM + device band LU + block-inverse image; "
                  "scipy: SuperLU)")


def c5_var():
    """EIGMI_C5_VAR=1: the variable-coefficient P1 K / M (eig_gen kinds 9 / 10, a coefficient per
    tetrahedron) uploaded with EIG_MAT_NO_CLASS -- every launch streams its box image."""
    return os.environ.get("EIGMI_C5_VAR", "0") == "1"


def c5_mats(ctx, N):
    var = c5_var()
    fl = eigmi.MAT_NO_CLASS if var else 0
    rk, ck, vk = eigmi.gen_matrix(eigmi.GEN_P1STIFF3D_VAR if var else eigmi.GEN_P1STIFF3D, N)
    K = eigmi.Matrix.from_bcsr(ctx, rk, ck, vk, flags=fl)
    del rk, ck, vk
    rm, cm, vm = eigmi.gen_matrix(eigmi.GEN_P1MASS3D_VAR if var else eigmi.GEN_P1MASS3D, N)
    nnz = int(rm[-1])
    M = eigmi.Matrix.from_bcsr(ctx, rm, cm, vm, flags=fl)
    return K, M, nnz


def c5(ctx):
    N = int(os.environ.get("EIGMI_C5_N", "256"))
    steps, warm, b, degree = 3, 1, 32, 36
    n = N ** 3
    t0 = time.perf_counter()
    K, M, nnz = c5_mats(ctx, N)
    bl = eigmi.BlockLanczos(K, M, block=b, max_steps=steps + warm, degree=degree, seed=123)
    setup_s = time.perf_counter() - t0
    bl.step(warm)
    t = bl.step(steps)
    ev, _, res = bl.ritz(4, eigmi.WHICH_LA, want_resid=False)
    cols = b // (t.cheb_launches // (steps * (degree - 1)))  # columns per launch
    # per launch, SURVEY 8(d) CSR count: matrix + (gather x_k, read x_{k-1}, read b, write x_{k+1}) per
    # column + dinv; and the bytes of the image the launch streams: the row-class kernel reads no
    # matrix data (class table in LDS, 1 / a_rr included), the box-image kernel one array per offset
    csr_bytes = 12 * nnz + 4 * (n + 1) + 32 * cols * n + 8 * n
    kname = M.kernel("cheb32")
    info = M.info
    if kname == "k_boxc_mv8_cheb":
        cheb_bytes = 32 * cols * n
    elif kname == "k_box_mv32_cheb":
        cheb_bytes = (8 * (2 * info.sym_arrays - 1) + info.sym_mask_bytes + 8) * n + 32 * cols * n
    else:
        cheb_bytes = csr_bytes
    cheb_us = t.cheb_ms / t.cheb_launches * 1e3
    emit(config=f"C5 P1 Kuhn K/M {N}^3, block Lanczos k={b}" + (" (variable coefficients, box image)" if c5_var() else ""),
         op=f"block step (Chebyshev degree {degree}, CGS2, CholQR2)",
         block_steps_per_s=round(steps / (t.total_ms * 1e-3), 3), ms_per_step=round(t.total_ms / steps, 2),
         kspmm_ms=round(t.kspmm_ms / steps, 2), cheb_ms=round(t.cheb_ms / steps, 2),
         orth_ms=round(t.orth_ms / steps, 2), norm_ms=round(t.norm_ms / steps, 2),
         cheb_kernel=kname, cheb_kernel_us=round(cheb_us, 1), cheb_bytes_per_launch=cheb_bytes,
         cheb_GBs=round(cheb_bytes / (cheb_us * 1e-6) / 1e9, 1),
         cheb_frac=round(cheb_bytes / (cheb_us * 1e-6) / 1e9 / PEAK, 4),
         cheb_csr_bytes=csr_bytes, cheb_csr_equiv_GBs=round(csr_bytes / (cheb_us * 1e-6) / 1e9, 1),
         nnz=nnz, setup_s=round(setup_s, 1),
         top_ritz=[float(x) for x in ev], steps_taken=steps + warm)
    bl.close()


def boxk(ctx):
    """Row-class box kernels alone at 256^3, m = 32 (the C5 / multigrid fine-level launches): the
    SpMM Y = K X (k_boxc_mv8<kBoxStore>, 2 vector streams = 16 m n bytes) and the mass solve's
    Chebyshev step (kBoxCheb, 4 streams = 32 m n bytes) from the difference of two solve degrees."""
    N = int(os.environ.get("EIGMI_C5_N", "256"))
    var = os.environ.get("EIGMI_BOXK_VAR", "0") == "1"
    b, n, reps = 32, N ** 3, 20

    def load(kind):
        # variable coefficients: a coefficient per tetrahedron (eig_gen kinds 9 / 10; the rows leave
        # their geometric class, so the box-image kernel runs; the pattern stays the same)
        r, c, v = eigmi.gen_matrix(kind, N)
        return eigmi.Matrix.from_bcsr(ctx, r, c, v, flags=eigmi.MAT_NO_CLASS if var else 0)
    K = load(eigmi.GEN_P1STIFF3D_VAR if var else eigmi.GEN_P1STIFF3D)
    M = load(eigmi.GEN_P1MASS3D_VAR if var else eigmi.GEN_P1MASS3D)
    X, Y = ctx.zeros(n * b), ctx.zeros(n * b)
    ctx.check(eigmi.lib.eig_fill_normal(ctx.h, n * b, 5, X.ptr))
    # box-image kernels (EIG_TUNE_BOX_COLS): 32 = k_box_mv32, 16 = k_box_mv16p (EIGMI_BOX_COLS list)
    # (a value 33 = 32 columns with the XCD-contiguous tile map, EIG_TUNE_BOX_MAP)
    cols_list = [int(c) for c in os.environ.get("EIGMI_BOX_COLS", "0").split(",")]
    tag = f"{N}^3 m={b}" + (" (variable coefficients)" if var else "")
    for cols in cols_list:
        K.tune(box_cols=min(cols, 32), box_map=int(cols == 33))
        M.tune(box_cols=min(cols, 32), box_map=int(cols == 33))
        eigmi.spmm_mv8(K, b, X, Y)
        ctx.sync()

        def spmm():
            for _ in range(reps):
                eigmi.spmm_mv8(K, b, X, Y)
            ctx.sync()
        ts, _ = wall(spmm)
        ts /= reps
        emit(config=f"P1 K {tag}", op="SpMM (kBoxStore)", kernel=K.kernel("spmm32"), box_map=int(cols == 33), us=round(ts * 1e6, 1),
             bytes=16 * b * n, frac=round(16 * b * n / ts / 1e9 / PEAK, 4))
        d0, d1 = 2, 22
        eigmi.mass_solve_mv8(M, b, d0, X, Y)
        ctx.sync()
        t0, _ = wall(lambda: (eigmi.mass_solve_mv8(M, b, d0, X, Y), ctx.sync()), 5)
        t1, _ = wall(lambda: (eigmi.mass_solve_mv8(M, b, d1, X, Y), ctx.sync()), 5)
        tc = (t1 - t0) / (d1 - d0)
        # vectors only for the row-class kernels; the box image adds its nd value arrays (+ D^-1 for
        # the Chebyshev step) per row
        img_s = 0 if K.kernel("spmm32") == "k_boxc_mv8" else 15 * 8 * n
        img_c = 0 if M.kernel("cheb32") == "k_boxc_mv8_cheb" else 15 * 8 * n + 8 * n
        emit(config=f"P1 K {tag}", op="SpMM bytes incl. image", kernel=K.kernel("spmm32"),
             bytes=16 * b * n + img_s, frac=round((16 * b * n + img_s) / ts / 1e9 / PEAK, 4))
        emit(config=f"P1 M {tag}", op="Chebyshev step (kBoxCheb)", kernel=M.kernel("cheb32"), box_map=int(cols == 33), us=round(tc * 1e6, 1),
             bytes=32 * b * n + img_c, frac=round((32 * b * n + img_c) / tc / 1e9 / PEAK, 4))
    X.free(), Y.free()
    K.close(), M.close()


def c5si(ctx):
    """C5 at the end GeneralizedInverse returns (eigensolver.hh:204-351): the smallest eigenvalues
    of the P1 pencil by block Lanczos on K^-1 M (sigma = 0) with the K solve by multigrid
    (eig_blanczos_create_si_mg).  The iteration count is picked at setup so that the solve's
    residual is <= 1e-12 on a random block; the line reports setup, the solve and the block step."""
    N = int(os.environ.get("EIGMI_C5_N", "256"))
    steps, warm, b = 2, 1, 32
    n = N ** 3
    t0 = time.perf_counter()
    K, M, _ = c5_mats(ctx, N)
    t1 = time.perf_counter()
    mg = eigmi.Multigrid(K, (N, N, N), max_cols=b, smooth_degree=2, smooth_ratio=5.0)
    mg_setup = time.perf_counter() - t1
    B, X = ctx.zeros(n * b), ctx.zeros(n * b)
    ctx.check(eigmi.lib.eig_fill_normal(ctx.h, n * b, 7, B.ptr))
    hist = {}
    cycles = None
    for c in (4, 8, 12, 14, 16, 18, 20):
        t2 = time.perf_counter()
        hist[c] = mg.solve(b, B, X, c, resid=True)
        hist[f"{c}_s"] = round(time.perf_counter() - t2, 4)
        if hist[c] <= 1e-12:
            cycles = c
            break
    cycles = cycles or 20
    B.free(), X.free()
    bl = eigmi.BlockLanczos(K, M, block=b, max_steps=steps + warm, Ks=K, sigma=0.0, mg=mg, cycles=cycles, seed=123)
    setup_s = time.perf_counter() - t0
    bl.step(warm)
    t = bl.step(steps)
    ev, _, _ = bl.ritz(4, eigmi.WHICH_SA, want_resid=False)
    h = 1.0 / (N + 1)
    emit(config=f"C5 P1 Kuhn K/M {N}^3, block Lanczos k={b}, smallest end (K^-1 M, multigrid K solve)" +
         (" (variable coefficients, box image)" if c5_var() else ""),
         op="block step (multigrid solve, CGS2, CholQR2)", block_steps_per_s=round(steps / (t.total_ms * 1e-3), 3),
         ms_per_step=round(t.total_ms / steps, 2), solve_ms=round(t.cheb_ms / steps, 2),
         kspmm_ms=round(t.kspmm_ms / steps, 2), orth_ms=round(t.orth_ms / steps, 2), norm_ms=round(t.norm_ms / steps, 2),
         mg=mg.info(), mg_setup_s=round(mg_setup, 2), cycles=cycles, solve_resid_history=hist,
         setup_s=round(setup_s, 1), smallest_ritz=[float(x) for x in ev], steps_taken=steps + warm,
         note=f"Ritz values after {steps + warm} block steps (Krylov dim {(steps + warm) * b}); the continuum "
              f"lowest eigenvalue of -Laplace on the unit cube is 3 pi^2 = {3 * np.pi ** 2:.4f} (h = {h:.5f})")
    bl.close()
    mg.close()


class _View:
    """A slice of a device buffer, for the wrappers that take an object with .ptr."""

    def __init__(self, ptr):
        self.ptr = ptr


def lobpcg(ctx):
    """The smallest end of the C5 pencil by LOBPCG (eig_lobpcg_*): block 32, nev 8, one multigrid
    V-cycle per iteration as the preconditioner, tol 1e-8, to convergence (at most EIGMI_LOBPCG_ITERS = 40
    iterations, one per call with a record each) -- iterations, the per-iteration split of
    eig_lobpcg_timing, the true residuals; then the two streaming kernels alone
    (k_lobpcg_resid, k_lobpcg_update against their algorithmic bytes) with an interleaved A/B, five
    rounds, of the fused update against the same update by four eig_panel_update_mv8 calls (two
    products into scratch panels, two copies back through the identity -- the kernels the update
    replaces); then c5si in the same process."""
    N = int(os.environ.get("EIGMI_C5_N", "256"))
    b, nev, tol = 32, 8, 1e-8
    n = N ** 3
    tag = f"C5 P1 Kuhn K/M {N}^3" + (" (variable coefficients, box image)" if c5_var() else "")
    t0 = time.perf_counter()
    K, M, _ = c5_mats(ctx, N)
    mg = eigmi.Multigrid(K, (N, N, N), max_cols=b, smooth_degree=2, smooth_ratio=5.0)
    s = eigmi.Lobpcg(K, M, block=b, seed=123, mg=(mg, 1))
    setup_s = time.perf_counter() - t0
    # one iteration per call, so that every iteration leaves a record: theta, the largest ||r_j|| / |theta_j|
    # of the nev wanted pairs (true residuals from fresh products; the convergence bar is on
    # ||r_j|| / (|theta_j| ||M x_j||), which is larger by 1 / ||M x_j||), and the counters since creation.
    # Each call ends with the residual its convergence test needs, so resid_ms counts two per iteration.
    it, conv, tw = 0, False, 0.0
    acc = dict(total_ms=0.0, resid_ms=0.0, precond_ms=0.0, orth_ms=0.0, spmm_ms=0.0, rr_ms=0.0)
    t = None
    for _ in range(int(os.environ.get("EIGMI_LOBPCG_ITERS", "40"))):
        try:
            dt, (done, conv, t) = wall(lambda: s.step(1, nev, tol))
        except eigmi.EigError as err:  # EIG_ERR_BREAKDOWN: recorded, the kernel measurements below still run
            emit(config=tag, op="LOBPCG iteration", iteration=it + 1, error=str(err))
            break
        tw += dt
        it += done
        for k in acc:
            acc[k] += getattr(t, k)
        ev, _, res = s.ritz(nev)
        emit(config=tag, op="LOBPCG iteration", iteration=it, converged=conv, theta=[float(x) for x in ev[:3]],
             theta_nev=float(ev[-1]), resid_over_theta=float((res / np.abs(ev)).max()),
             cholqr_recomputed=int(t.cholqr_recomputed), p_dropped=int(t.p_dropped),
             orth_rejected=int(t.orth_rejected), orth_dev=float(t.orth_dev))
        if conv or done == 0:
            break
    ev, _, res = s.ritz(nev)
    per = lambda x: round(x / max(it, 1), 2)  # noqa: E731
    emit(config=tag + f", LOBPCG block {b}, nev {nev}, one V-cycle, tol {tol:g}", op="solve to convergence",
         iterations=it, converged=conv, total_ms=round(acc["total_ms"], 1), wall_s=round(tw, 3),
         ms_per_iteration=per(acc["total_ms"]), resid_ms=per(acc["resid_ms"]), precond_ms=per(acc["precond_ms"]),
         orth_ms=per(acc["orth_ms"]), spmm_ms=per(acc["spmm_ms"]), rr_update_ms=per(acc["rr_ms"]),
         cholqr_recomputed=int(t.cholqr_recomputed), p_dropped=int(t.p_dropped), orth_rejected=int(t.orth_rejected),
         orth_dev=float(t.orth_dev), eigenvalues=[float(x) for x in ev], true_residuals=[float(x) for x in res],
         relative_residuals=[float(r / abs(e)) for r, e in zip(res, ev)], mg=mg.info(), setup_s=round(setup_s, 1))
    s.close()
    mg.close()
    K.close(), M.close()
    # the streaming kernels alone, one family: S = [X | W | P] random, C random orthonormal
    rng = np.random.default_rng(5)
    S = ctx.zeros(3 * n * b)
    ctx.check(eigmi.lib.eig_fill_normal(ctx.h, 3 * n * b, 7, S.ptr))
    C = np.linalg.qr(rng.standard_normal((3 * b, 2 * b)))[0]
    dC = ctx.array(C)
    dCx, dCp, dI = ctx.array(np.ascontiguousarray(C[:, :b])), ctx.array(np.ascontiguousarray(C[:, b:])), ctx.array(np.eye(b))
    T1, T2 = ctx.zeros(n * b), ctx.zeros(n * b)
    Xs, Ps = _View(S.offset(0)), _View(S.offset(2 * n * b))  # the X and P slices of S

    def fused():
        eigmi.lobpcg_update_mv8(ctx, n, b, 3, S, dC)
        ctx.sync()

    def four_calls():
        eigmi.panel_update_mv8(ctx, n, 3 * b, b, S, dCx, 1.0, 0.0, T1)
        eigmi.panel_update_mv8(ctx, n, 3 * b, b, S, dCp, 1.0, 0.0, T2)
        eigmi.panel_update_mv8(ctx, n, b, b, T1, dI, 1.0, 0.0, Xs)
        eigmi.panel_update_mv8(ctx, n, b, b, T2, dI, 1.0, 0.0, Ps)
        ctx.sync()

    fused(), four_calls()  # warm-up
    rounds = {"fused": [], "four_calls": []}
    for _ in range(5):
        rounds["fused"].append(wall(fused, 3)[0] * 1e3)
        rounds["four_calls"].append(wall(four_calls, 3)[0] * 1e3)
    upd_bytes = (3 * b + 2 * b) * 8 * n
    fm = float(np.median(rounds["fused"]))
    emit(config=tag, op=f"k_lobpcg_update m={b} kb=3, one family, against four eig_panel_update_mv8 calls (interleaved, 5 rounds)",
         fused_ms=[round(x, 3) for x in rounds["fused"]], four_calls_ms=[round(x, 3) for x in rounds["four_calls"]],
         fused_median_ms=round(fm, 3), four_calls_median_ms=round(float(np.median(rounds["four_calls"])), 3),
         bytes=upd_bytes, fused_GBs=round(upd_bytes / fm / 1e6, 1), frac=round(upd_bytes / fm / 1e6 / PEAK, 4))
    th, sums = ctx.array(rng.standard_normal(b)), ctx.zeros(2 * b)

    def resid():
        eigmi.lobpcg_resid_mv8(ctx, n, b, Xs, Ps, th, T1, sums)
        ctx.sync()

    resid()
    tr = wall(resid, 5)[0] * 1e3
    emit(config=tag, op=f"k_lobpcg_resid m={b}", ms=round(tr, 3), bytes=3 * b * 8 * n,
         GBs=round(3 * b * 8 * n / tr / 1e6, 1), frac=round(3 * b * 8 * n / tr / 1e6 / PEAK, 4))
    for d in (S, T1, T2, dC, dCx, dCp, dI, th, sums):
        d.free()
    c5si(ctx)


def mgblk(ctx):
    """The blocked multigrid at C3 size: K = q1elast(64) (3x3 blocks, 262,144 nodes), the pencil's M of c3_pencil.
    Hierarchy setup (host Galerkin, block inverses, block Gershgorin bounds, uploads); one V-cycle
    (eig_mg_solve, cycles = 1, smoother degree 2, ratio 5) at m = 8 and 32 with the residual after 1 and 8
    cycles; the blocked product, the blocked residual (eig_resid_mv8) and the point Chebyshev step (two solve
    degrees' difference) interleaved over five rounds; LOBPCG block 32, nev 8, tol 1e-8 with one V-cycle and with
    Chebyshev-Jacobi degree 4 on [g / 10, g] (at most EIGMI_MGBLK_ITERS = 300 iterations each; 0 skips it).  The
    block-Jacobi step and the two transfers have no entry point of their own: their times come from kernel
    traces of this config at one width each (EIGMI_MGBLK_M = 8 or 32, EIGMI_MGBLK_ITERS = 0; tools/gpu.sh mgblk,
    mgblk_stats below)."""
    N = int(os.environ.get("EIGMI_MGBLK_N", "64"))
    cfg = f"C3 Q1 elasticity {N}^3 3x3 BCSR, blocked multigrid"
    rp, c, v = eigmi.gen_matrix(eigmi.GEN_Q1ELAST3D, N)
    nb, n = N ** 3, 3 * N ** 3
    K = eigmi.Matrix.from_bcsr(ctx, rp, c, v, 3, 3)
    t0 = time.perf_counter()
    mg = eigmi.Multigrid(K, (N, N, N), max_cols=32, smooth_degree=2, smooth_ratio=5.0)
    emit(config=cfg, op="hierarchy setup (host Galerkin + block Jacobi data + uploads)",
         s=round(time.perf_counter() - t0, 2), mg=mg.info())
    v3 = v.reshape(-1, 3, 3)
    g = float((np.add.reduceat(np.abs(v3).sum(axis=2), rp[:-1], axis=0) / (16.0 / 3.0)).max())
    for m in [int(x) for x in os.environ.get("EIGMI_MGBLK_M", "8,32").split(",")]:
        B, X, R = ctx.array(oracle.random_mv8(n, m, 2)), ctx.zeros(n * m), ctx.zeros(n * m)
        r1 = mg.solve(m, B, X, 1, resid=True)
        r8 = mg.solve(m, B, X, 8, resid=True)
        tv = min(wall(lambda: mg.solve(m, B, X, 1), 10)[0] for _ in range(3))
        t3 = min(wall(lambda: mg.solve(m, B, X, 3), 5)[0] for _ in range(3))
        emit(config=cfg, op=f"one V-cycle m={m} (eig_mg_solve, cycles = 1, synchronous)", us=round(tv * 1e6, 1),
             three_cycles_us=round(t3 * 1e6, 1), residual_after_1=r1, residual_after_8=r8,
             contraction_per_cycle=round((r8 / r1) ** (1.0 / 7.0), 4))

        def batch(f, reps=20):
            t = time.perf_counter()
            for _ in range(reps):
                f()
            ctx.sync()
            return (time.perf_counter() - t) / reps * 1e6
        d0, d1 = 2, 12
        rounds = {"spmm": [], "resid": [], "cheb_point": []}
        eigmi.spmm_blk_mv8(K, m, B, R), eigmi.resid_mv8(K, m, B, X, R), eigmi.mass_solve_mv8(K, m, d1, B, X, g / 10, g)
        ctx.sync()
        for _ in range(5):
            rounds["spmm"].append(batch(lambda: eigmi.spmm_blk_mv8(K, m, B, R)))
            rounds["resid"].append(batch(lambda: eigmi.resid_mv8(K, m, B, X, R)))
            a = batch(lambda: eigmi.mass_solve_mv8(K, m, d0, B, X, g / 10, g), 5)
            b = batch(lambda: eigmi.mass_solve_mv8(K, m, d1, B, X, g / 10, g), 5)
            rounds["cheb_point"].append((b - a) / (d1 - d0))
        emit(config=cfg, op=f"blocked product / residual / point Chebyshev step m={m} (interleaved, 5 rounds)",
             **{k + "_us": [round(x, 1) for x in r] for k, r in rounds.items()},
             **{k + "_median_us": round(float(np.median(r)), 1) for k, r in rounds.items()})
        B.free(), X.free(), R.free()
    # the C3 pencil (c3_pencil's M = D + 0.3 (K - D)), LOBPCG block 32
    dg = np.nonzero(c == np.repeat(np.arange(nb), np.diff(rp)))[0][:, None]
    r = np.arange(3)
    vm = 0.3 * v3
    vm[dg, r, r] = v3[dg, r, r]
    M = eigmi.Matrix.from_bcsr(ctx, rp, c, vm.reshape(-1), 3, 3)
    b, nev, tol, cap = 32, 8, 1e-8, int(os.environ.get("EIGMI_MGBLK_ITERS", "300"))
    for name in ("one V-cycle", "Chebyshev-Jacobi degree 4") if cap > 0 else ():
        s = eigmi.Lobpcg(K, M, block=b, seed=123)
        if name == "one V-cycle":
            s.precond_mg(mg, 1)
        else:
            s.precond_cheb(4, g / 10.0, g)
        tw, (it, conv, t) = wall(lambda: s.step(cap, nev, tol))
        ev, _, res = s.ritz(nev)
        emit(config=cfg + f", LOBPCG block {b}, nev {nev}, tol {tol:g}", op=name, iterations=it, converged=conv,
             device_ms=round(t.total_ms, 1), ms_per_iteration=round(t.total_ms / max(it, 1), 2),
             precond_ms_per_iteration=round(t.precond_ms / max(it, 1), 2), wall_s=round(tw, 2),
             eigenvalues=[float(x) for x in ev], relative_residuals=[float(a / abs(e)) for a, e in zip(res, ev)])
        s.close()
    mg.close()
    K.close(), M.close()


def mgblk_stats(path, m):
    """The fine-level launches of the blocked multigrid's kernels in a rocprofv3 --kernel-trace of mgblk at one
    width m: per kernel the dispatches with the largest grid (the 64^3 level), their count, median and minimum."""
    import csv
    keys = ("k_spmm_blk_mv8", "k_cheb_init_bjac", "k_mg_restrict", "k_mg_prolong", "k_mv8_axpby")
    runs = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("eigmi::", "")
        if any(k in name for k in keys):
            grid = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"])
            runs.setdefault(name, {}).setdefault(grid, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, by_grid in sorted(runs.items()):
        t = by_grid[max(by_grid)]
        emit(m=int(m), kernel=name, level="fine (largest grid)", calls=len(t), median_us=round(float(np.median(t)), 2),
             min_us=round(min(t), 2), max_us=round(max(t), 2))


def amg(ctx):
    """Smoothed-aggregation AMG (eig_amg_create; theta 0.08, smoother degree 2, ratio 5) on the bench's `general`
    matrix: 3-D Poisson EIGMI_AMG_N^3 (default 128), scrambled + reverse Cuthill-McKee.  Host setup + uploads;
    levels, rows, stored entries, operator complexity; the fine-level transfers' algorithmic bytes (P's pattern
    from eig_amg_aggregate: 12 nnz(P) + 8 (rows + 1) of CSR, the input panel once, the output panel once -- twice for
    the prolongation, which adds in place); one V-cycle (eig_mg_solve, cycles = 1, synchronous) at the widths
    EIGMI_AMG_M (default 8,32) interleaved over three rounds with the geometric multigrid's V-cycle on the
    unscrambled matrix of the same size, and the residual after 1 and 8 cycles of both; LOBPCG block 32, nev 8,
    tol 1e-8 with one AMG V-cycle and with Chebyshev-Jacobi degree 4 on [g / 10, g] (at most EIGMI_AMG_ITERS = 400
    iterations each; 0 skips it).  The transfer kernels' own times come from a kernel trace of this config
    (tools/gpu.sh amg, amg_stats below)."""
    N = int(os.environ.get("EIGMI_AMG_N", "128"))
    n = N ** 3
    cfg = f"general 3-D Poisson {N}^3 (scrambled + RCM), smoothed-aggregation AMG"
    rp0, c0, v0 = eigmi.gen_matrix(eigmi.GEN_POISSON3D, N)
    t0 = time.perf_counter()
    rp, c, v = eigmi.scrambled_rcm(rp0, c0, v0)
    t_perm = time.perf_counter() - t0
    K = eigmi.Matrix.from_bcsr(ctx, rp, c, v)
    theta, nu, ratio = 0.08, 2, 5.0
    t0 = time.perf_counter()
    mg = eigmi.Multigrid.amg(K, theta, max_cols=32, smooth_degree=nu, smooth_ratio=ratio)
    setup_s = time.perf_counter() - t0
    lev = [mg.level_info(l) for l in range(mg.info()["levels"])]
    emit(config=cfg, op="hierarchy setup (host aggregation, P, P^T A P, uploads)", s=round(setup_s, 2),
         scramble_rcm_s=round(t_perm, 2), spmm32_kernel=K.kernel("spmm32"), theta=theta, smooth_degree=nu,
         smooth_ratio=ratio, rows=[L["rows"] for L in lev], nnz=[L["nnz"] for L in lev],
         operator_complexity=round(mg.complexity(), 4), mg=mg.info())
    agg, na = eigmi.amg_aggregate(rp, c, v, theta)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    nnz_p = int(np.unique(row * na + agg[c]).size)  # P's pattern: the aggregates of a row's stored columns
    Kg = eigmi.Matrix.from_bcsr(ctx, rp0, c0, v0)
    t0 = time.perf_counter()
    geo = eigmi.Multigrid(Kg, (N, N, N), max_cols=32, smooth_degree=nu, smooth_ratio=ratio)
    emit(config=cfg, op="geometric multigrid on the unscrambled matrix: setup", s=round(time.perf_counter() - t0, 2),
         spmm32_kernel=Kg.kernel("spmm32"), mg=geo.info(),
         rows=[geo.level_info(l)["rows"] for l in range(geo.info()["levels"])])
    for m in [int(x) for x in os.environ.get("EIGMI_AMG_M", "8,32").split(",")]:
        B, X = ctx.array(oracle.random_mv8(n, m, 2)), ctx.zeros(n * m)
        res = {}
        for name, h in (("amg", mg), ("geometric", geo)):
            r1 = h.solve(m, B, X, 1, resid=True)
            r8 = h.solve(m, B, X, 8, resid=True)
            res[name] = (r1, r8, (r8 / r1) ** (1.0 / 7.0))
        rounds = {"amg": [], "geometric": []}
        for _ in range(3):
            for name, h in (("amg", mg), ("geometric", geo)):
                rounds[name].append(wall(lambda: h.solve(m, B, X, 1), 10)[0] * 1e3)
        restrict_b = 12 * nnz_p + 8 * (na + 1) + 8 * m * (n + na)
        prolong_b = 12 * nnz_p + 8 * (n + 1) + 8 * m * (2 * n + na)
        emit(config=cfg, op=f"one V-cycle m={m} (eig_mg_solve, cycles = 1, synchronous; interleaved, 3 rounds of 10)",
             amg_ms=[round(x, 3) for x in rounds["amg"]], geometric_ms=[round(x, 3) for x in rounds["geometric"]],
             amg_min_ms=round(min(rounds["amg"]), 3), geometric_min_ms=round(min(rounds["geometric"]), 3),
             amg_residual_after_1=res["amg"][0], amg_residual_after_8=res["amg"][1],
             amg_contraction_per_cycle=round(res["amg"][2], 4), geometric_residual_after_1=res["geometric"][0],
             geometric_residual_after_8=res["geometric"][1], geometric_contraction_per_cycle=round(res["geometric"][2], 4),
             fine_aggregates=int(na), nnz_P=nnz_p, restrict_algorithmic_bytes=restrict_b,
             prolong_algorithmic_bytes=prolong_b)
        B.free(), X.free()
    geo.close()
    Kg.close()
    g = float((np.add.reduceat(np.abs(v), rp[:-1]) / v[c == row]).max())
    b, nev, tol, cap = 32, 8, 1e-8, int(os.environ.get("EIGMI_AMG_ITERS", "400"))
    for name in ("one AMG V-cycle", "Chebyshev-Jacobi degree 4") if cap > 0 else ():
        s = eigmi.Lobpcg(K, None, block=b, seed=123)
        if name == "one AMG V-cycle":
            s.precond_mg(mg, 1)
        else:
            s.precond_cheb(4, g / 10.0, g)
        tw, (it, conv, t) = wall(lambda: s.step(cap, nev, tol))
        ev, _, rs = s.ritz(nev)
        emit(config=cfg + f", LOBPCG block {b}, nev {nev}, tol {tol:g}", op=name, iterations=it, converged=conv,
             device_ms=round(t.total_ms, 1), ms_per_iteration=round(t.total_ms / max(it, 1), 2),
             precond_ms_per_iteration=round(t.precond_ms / max(it, 1), 2), wall_s=round(tw, 2),
             eigenvalues=[float(x) for x in ev], relative_residuals=[float(a / abs(e)) for a, e in zip(rs, ev)])
        s.close()
    mg.close()
    K.close()


def amg_stats(path, m):
    """The transfer kernels of both hierarchies in a rocprofv3 --kernel-trace of amg at one width m: per kernel and
    grid size (one per level, the largest first) the dispatches, their median and minimum."""
    import csv
    keys = ("k_amg_restrict", "k_amg_prolong_add", "k_mg_restrict", "k_mg_prolong_add")
    runs = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("eigmi::", "")
        if any(k in name for k in keys):
            grid = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"])
            runs.setdefault(name, {}).setdefault(grid, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, by_grid in sorted(runs.items()):
        for level, grid in enumerate(sorted(by_grid, reverse=True)):
            t = by_grid[grid]
            emit(m=int(m), kernel=name, level=level, grid_threads=grid, calls=len(t),
                 median_us=round(float(np.median(t)), 2), min_us=round(min(t), 2), max_us=round(max(t), 2))


def slice_step_pair(ctx, M, m, cfg, image_bytes, dinv_bytes, window):
    """The filter step and the Chebyshev-Jacobi step on M at m columns, each from the difference of two
    degrees (the first steps and the per-call setup cancel), alternated three times; medians.  Both degrees
    keep the device busy for milliseconds: at degree 4 eig_mass_solve_mv8's host setup (its buffers) outlasts
    the kernels at 128^3 x 8, and the difference then understates the step (52 us against the trace's 87)."""
    n = M.info.n
    a, b, lo, hi = window
    X, Y, W = ctx.zeros(n * m), ctx.zeros(n * m), ctx.zeros(n * m)
    ctx.check(eigmi.lib.eig_fill_normal(ctx.h, n * m, 5, X.ptr))
    d0, d1 = 24, 64

    def cheb(d):
        eigmi.mass_solve_mv8(M, m, d, X, Y)
        ctx.sync()

    def filt(d):
        eigmi.filter_mv8(M, m, a, b, lo, hi, d, X, Y, W)
        ctx.sync()
    for f in (cheb, filt):
        f(d0)
        f(d1)
    tc, tf = [], []
    for _ in range(3):
        tc.append((wall(lambda: cheb(d1), 2)[0] - wall(lambda: cheb(d0), 2)[0]) / (d1 - d0))
        tf.append((wall(lambda: filt(d1), 2)[0] - wall(lambda: filt(d0), 2)[0]) / (d1 - d0))
    tc, tf = float(np.median(tc)), float(np.median(tf))
    vec = 32 * m * n  # per row and column: 8 B gather, 8 B B, 16 B in place
    emit(config=cfg, m=m, op="Chebyshev step", kernel=M.kernel("cheb32" if m % 32 == 0 else "cheb8"),
         us=round(tc * 1e6, 1), bytes=vec + image_bytes + dinv_bytes,
         frac=round((vec + image_bytes + dinv_bytes) / tc / 1e9 / PEAK, 4))
    emit(config=cfg, m=m, op="filter step", kernel=M.kernel("filt32" if m % 32 == 0 else "filt8"),
         us=round(tf * 1e6, 1), bytes=vec + image_bytes, frac=round((vec + image_bytes) / tf / 1e9 / PEAK, 4),
         vs_cheb=round(tf / tc, 4))
    for d in (X, Y, W):
        d.free()


def slice_stats(path):
    """The Chebyshev and filter step kernels in a rocprofv3 --kernel-trace of the slice task: per kernel instance
    and grid the launches, median, minimum and maximum (the blocked kernels' m = 8 and m = 32 launches share a
    grid: their split is in the step pairs' own lines)."""
    import csv
    runs = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("eigmi::", "")
        if any(k in name for k in ("k_boxc_mv8", "k_box_mv32", "k_box_mv16p", "k_sell_mv8", "k_spmm_blk_mv8_cheb",
                                   "k_spmm_blk_mv8_filt")):
            key = (name, int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]))
            runs.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (name, gx, gy), t in sorted(runs.items()):
        emit(kernel=name, grid_threads=[gx, gy], calls=len(t), median_us=round(float(np.median(t)), 2),
             min_us=round(min(t), 2), max_us=round(max(t), 2))


def slice(ctx):
    cases = os.environ.get("EIGMI_SLICE_CASES", "class,general,c3,box,run").split(",")
    win = (1.0, 1.5, 0.0, 13.0)  # (the step's time does not depend on the window)
    if "class" in cases:
        r, c, v = eigmi.gen_matrix(eigmi.GEN_POISSON3D, 128)
        M = eigmi.Matrix.from_bcsr(ctx, r, c, v)
        slice_step_pair(ctx, M, 8, "7-pt Poisson 128^3, row-class image", 0, 0, win)
        M.close()
    if "general" in cases:
        r, c, v = eigmi.gen_matrix(eigmi.GEN_POISSON3D, 128)
        r, c, v = eigmi.scrambled_rcm(r, c, v, 123)
        M = eigmi.Matrix.from_bcsr(ctx, r, c, v)
        n, nnz = M.info.n, int(r[-1])
        slice_step_pair(ctx, M, 32, "general (scrambled + RCM) Poisson 128^3, SELL", 12 * nnz + 4 * (n + 1), 8 * n, win)
        M.close()
    if "c3" in cases:
        N = int(os.environ.get("EIGMI_C3_N", "64"))
        r, c, v = eigmi.gen_matrix(eigmi.GEN_Q1ELAST3D, N)
        M = eigmi.Matrix.from_bcsr(ctx, r, c, v, 3, 3)
        nb, nnzb = r.size - 1, int(r[-1])
        for m in (8, 32):
            slice_step_pair(ctx, M, m, f"C3 Q1 elasticity {N}^3 3x3 BCSR", 76 * nnzb + 4 * (nb + 1), 8 * M.info.n, win)
        M.close()
    if "box" in cases:
        N = int(os.environ.get("EIGMI_SLICE_N", "256"))
        r, c, v = eigmi.gen_matrix(eigmi.GEN_VARCOEF3D, N)
        M = eigmi.Matrix.from_bcsr(ctx, r, c, v)
        del r, c, v
        info = M.info
        n = info.n
        img = (8 * info.sym_offsets + info.sym_mask_bytes) * n
        slice_step_pair(ctx, M, 32, f"7-pt variable coefficients {N}^3, box image", img, 8 * n, win)
        # one outer iteration at block 32 (degree 40: the split, not a solve)
        sl = eigmi.Slice(M, 1.0, 1.5, 0.0, 13.0, block=32, degree=40, seed=123)
        sl.step(1, 0.0)
        it, _, t = sl.step(2, 0.0)
        emit(config=f"7-pt variable coefficients {N}^3, box image", op="slice iteration, block 32, degree 40",
             kernel=M.kernel("filt32"), ms_per_iter=round(t.total_ms / it, 2), filter_ms=round(t.filter_ms / it, 2),
             orth_ms=round(t.orth_ms / it, 2), rr_ms=round(t.rr_ms / it, 2), resid_ms=round(t.resid_ms / it, 2),
             filter_us_per_step=round(t.filter_ms / it / 40 * 1e3, 1),
             filter_frac=round((32 * 32 * n + img) / (t.filter_ms / it / 40 * 1e-3) / 1e9 / PEAK, 4))
        sl.close()
        M.close()
    if "run" in cases:
        # a full run: kind 8 at 128^3, SPD so lmin = 0, lmax from 30 Lanczos steps; the window starts above the
        # lowest eigenvalues and is widened until eig_filter_count sees about 10 eigenvalues
        N = int(os.environ.get("EIGMI_SLICE_RUN_N", "128"))
        r, c, v = eigmi.gen_matrix(eigmi.GEN_VARCOEF3D, N)
        M = eigmi.Matrix.from_bcsr(ctx, r, c, v)
        del r, c, v
        t0 = time.perf_counter()
        _, hi = eigmi.spectrum_bounds(M, 30, 123)
        bounds_s = time.perf_counter() - t0
        h2 = (np.pi / (N + 1)) ** 2
        a, b = 7.0 * h2, 9.0 * h2
        counts = []
        t0 = time.perf_counter()
        for _ in range(8):
            est = eigmi.filter_count(M, a, b, 0.0, hi, 0, 32, 7)
            counts.append([round(b / h2, 2), round(est, 2)])
            if est >= 9.0:
                break
            b += 0.75 * h2
        count_s = time.perf_counter() - t0
        block = 24
        degree = eigmi.filter_degree(a, b, 0.0, hi, 0)
        sl = eigmi.Slice(M, a, b, 0.0, hi, block=block, degree=0, seed=123)
        t0 = time.perf_counter()
        it, conv, t = sl.step(30, 1e-8)
        solve_s = time.perf_counter() - t0
        ev, _, res = sl.ritz()
        emit(config=f"7-pt variable coefficients {N}^3", op="slice run, tol 1e-8", window=[a, b], lmax=hi,
             count_sweep=counts, count_s=round(count_s, 2), bounds_s=round(bounds_s, 3), block=block, degree=degree,
             kernel=M.kernel("filt8"), iters=it, converged=bool(conv), found=int(ev.size), saturated=int(t.saturated),
             solve_s=round(solve_s, 3), filter_ms=round(t.filter_ms, 1), orth_ms=round(t.orth_ms, 1),
             rr_ms=round(t.rr_ms, 1), resid_ms=round(t.resid_ms, 1), max_resid=float(res.max()) if ev.size else None,
             eigenvalues_over_h2=[round(float(x / h2), 4) for x in ev])
        sl.close()
        M.close()


if __name__ == "__main__":
    if sys.argv[1:2] == ["mgblk_stats"]:
        mgblk_stats(sys.argv[2], sys.argv[3])
        sys.exit(0)
    if sys.argv[1:2] == ["slice_stats"]:
        slice_stats(sys.argv[2])
        sys.exit(0)
    if sys.argv[1:2] == ["amg_stats"]:
        amg_stats(sys.argv[2], sys.argv[3])
        sys.exit(0)
    ctx = eigmi.Context(0)
    which = sys.argv[1:] or ["c1", "c2", "c3", "inv"]
    for w in which:
        globals()[w](ctx)
