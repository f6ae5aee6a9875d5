// orth.h -- orthonormalisation of MultiVector<double,8> blocks: the dense tall-skinny launchers of
// k_orth.hip, the host policy of orth.cpp that picks among them, and the look-ahead MGS's state on a
// context.  A part of internal.h, which includes it after its typedefs and error macros; sources
// include internal.h.
#pragma once

struct eig_mat_s;

namespace eigmi {

#define EIG_MV8_CHECK(m)                                                                             \
  EIG_CHECK((m) % 8 == 0, EIG_ERR_SHAPE, "number of cols must be a multiple of block size");       \
  EIG_CHECK((m) >= 0, EIG_ERR_ARG, "negative column count")

// ---- kernel launchers (k_orth.hip) ----------------------------------------------------------
void launch_gram_mv8(i64 n, i64 m1, i64 m2, const double *Q1, const double *Q2, double *G, int ticket,
                     hipStream_t s, ReduceWS red);
int gram_mv8_chunks(i64 m1, i64 m2);  // tickets one launch_gram_mv8 takes
// The same Gram on window-layout panels (column blocks ld rows apart, pointers at owned row 0).
void launch_gram_panel(eig_ctx_t ctx, i64 n, i64 ld, i64 m1, i64 m2, const double *Q1, const double *Q2, double *G,
                       hipStream_t s);
// Block Gram-Schmidt building blocks, see k_orth.hip.
void launch_mgs_pass(i64 n, double *Qb, int k, double *S, int ticket, hipStream_t s, ReduceWS red);
// MGS with Gram look-ahead (k_orth.hip): L steps per read pass, gated; false when L <= 1 or n <= 0
bool launch_mgs_lookahead(eig_ctx_t ctx, i64 n, double *Qb, int L, bool coop, hipStream_t s);
// The look-ahead MGS of one 8-column block whose window Gram G (8 x 8 row-major, device) is already
// known: the first read pass is replaced by G (k_mgs_la_gram), then the last launch as usual.
bool launch_mgs_lookahead_gram(eig_ctx_t ctx, i64 n, double *Qb, const double *G, hipStream_t s);
// Whole column MGS of one 8-column block in one workgroup (n <= 4096, one rank); false = not taken.
bool launch_mgs_small(i64 n, double *Qb, hipStream_t s);
// The 9 read-only MGS passes in one cooperative launch with grid barriers (k_orth.hip k_mgs_coop; one
// rank); false = refused or timed out (nothing written): run the per-pass launches instead
bool launch_mgs_coop(eig_ctx_t ctx, i64 n, double *Qb, double *Ssum, hipStream_t s);
void launch_apply_upper(i64 n, double *Qb, const double *U, hipStream_t s);
void launch_cholqr_factor(const double *G, double *U, double *normmax, int flags, hipStream_t s);
void launch_project(i64 n, i64 mrest, const double *Qk, double *Qrest, const double *S, hipStream_t s);
void launch_max_offdiag(const double *S, i64 rows, i64 cols, bool upper_only, double *normmax, hipStream_t s);

// ---- the look-ahead MGS on a context (orth.cpp) ---------------------------------------------
constexpr int kMgsLookaheadDefault = 8;
int mgs_lookahead_default();  // EIGMI_MGS_LOOKAHEAD or kMgsLookaheadDefault

// Its device state (context scratch kSlotMgsLa; k_orth.hip "State"): the finished S rows, then 64
// words of which the kernels use st[0..1] (by launch parity), st[kMgsLaLast] and st[kMgsLaBar].
struct MgsLaState {
  double *Sfin;  // [8][8]
  unsigned *st;  // [64]
};
constexpr int kMgsLaBar = 32, kMgsLaLast = 2;  // st[] word indices: barrier counter, last call's final word
constexpr unsigned kMgsLaWritten = 16u;        // bit of a state word: the block has been written
// The state of this context, allocated and zeroed (on stream s) at first use.
MgsLaState mgs_lookahead_state(eig_ctx_t ctx, hipStream_t s);

// What eig_ctx_s keeps for it (host side).
struct MgsCtx {
  // a last launch (grid barriers without a cooperative launch) has been enqueued since the last
  // mgs_lookahead_check: its sticky error word must be read at the next sync point
  bool la_armed = false;
  // the sticky error word in page-locked, device-mapped host memory: the kernel stores into it, the
  // host reads it after any stream synchronisation without a copy (allocated at first use)
  int *err_host = nullptr, *err_dev = nullptr;
  // the window Gram whose product also zeroed the barrier word (launch_spmm_dot_gram_mv8); consumed
  // by the next launch_mgs_lookahead_gram of that Gram
  const double *bar_clean = nullptr;
};
int *mgs_err_word(eig_ctx_t ctx);  // device address of the error word
void mgs_release(eig_ctx_t ctx);   // frees the error word (eig_ctx_destroy)
int mgs_lookahead_passes(eig_ctx_t ctx);  // read passes of the last call (-1: none finished)
// After the stream is synchronised: throw EIG_ERR_HIP (and clear the sticky flag) when a look-ahead
// MGS last launch since the previous check timed out in its grid barrier (its rows are NaN)
void mgs_lookahead_check(eig_ctx_t ctx);

// ---- device-pointer helpers (orth.cpp) ------------------------------------------------------
void gram_device(eig_ctx_t ctx, i64 n, i64 m1, i64 m2, const double *Q1, const double *Q2, double *G);
// gram0 (or null): the window Gram of the first 8-column block, already summed by the caller's
// product (eig_orthonormalize_gram_mv8; MGS look-ahead on one rank only, else ignored)
void orthonormalize_device(eig_ctx_t ctx, i64 n, i64 m, double *Q, int variant, const double *gram0 = nullptr);
// Y = A X (one 8-column block), dp = diag(X^T Y), gram = Y^T Y (8 x 8): fused into the product where a
// kernel has the epilogue (launch_spmm_dot_gram_mv8), else product + panel Gram
void spmm_dot_gram_device(const eig_mat_s &A, const double *X, double *Y, double *dp, double *gram);
void b_orthonormalize_device(eig_mat_s &B, i64 m, double *Q, double *norm);

}  // namespace eigmi
