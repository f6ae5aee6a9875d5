// api.cpp -- the C ABI of libeigmi (include/eigmi.h): contexts, device memory, upload of a matrix's
// host images (built by mat_image.cpp: SELL-64, symmetric band, slice split), the halo plan of
// row-partitioned matrices, BlockVector and MultiVector operations.  Drivers live in drivers.cpp,
// the transports and their entry points in comm.cpp, the Gram and the orthonormalisations in orth.cpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <random>

#include "internal.h"
#include "mat_image.h"

using namespace eigmi;

// ============================================================================================
// internal helpers shared with drivers.cpp
// ============================================================================================
namespace eigmi {

void *ctx_buffer(eig_ctx_t ctx, CtxSlot slot, size_t bytes)
{
  if ((int)ctx->pool.size() <= slot) ctx->pool.resize(slot + 1, {nullptr, 0});
  auto &e = ctx->pool[slot];
  if (e.second < bytes)
  {
    if (e.first) EIG_HIP(hipFree(e.first));
    e.first = nullptr;
    e.second = 0;
    EIG_HIP(hipMalloc(&e.first, bytes));
    e.second = bytes;
  }
  return e.first;
}

// eigensolver.hh:49-55 generator (libstdc++ mt19937 + normal_distribution, bitwise the
// reference's sequence).
// The reference's start vectors: std::normal_distribution<double>{0, 1} over std::mt19937{seed}
// (eigensolver.hh:50-55), bitwise.  libstdc++ draws them by Marsaglia's polar method on pairs of
// generate_canonical<double, 53> uniforms (random.tcc: two 32-bit words per uniform, the second
// variate of an accepted pair kept for the next call); its generic generate_canonical recomputes
// long-double logarithms on every call, about two thirds of the 45 ns per variate it costs.  The
// same arithmetic with the constants folded (the words are exact in double, the scales powers of
// two) gives the same bits (tests/test_random_host.py against the oracle's std:: draws).
void host_random_normal(i64 count, unsigned seed, double *out)
{
  std::mt19937 urbg{seed};
  auto canonical = [&]() {
    double sum = 0.0;
    sum += double(urbg()) * 1.0;           // mt19937: min() = 0, range 2^32
    sum += double(urbg()) * 4294967296.0;  // x 2^32
    double r = sum / 18446744073709551616.0;  // / 2^64
    if (r >= 1.0) r = std::nextafter(1.0, 0.0);
    return r;
  };
  i64 i = 0;
  while (i < count)
  {
    double x, y, r2;
    do
    {
      x = 2.0 * canonical() - 1.0;
      y = 2.0 * canonical() - 1.0;
      r2 = x * x + y * y;
    } while (r2 > 1.0 || r2 == 0.0);
    const double mult = std::sqrt(-2 * std::log(r2) / r2);
    const double a = y * mult, b = x * mult;  // returned now / cached for the next call
    out[i++] = a * 1.0 + 0.0;                 // (ret * stddev + mean)
    if (i < count) out[i++] = b * 1.0 + 0.0;
  }
}

}  // namespace eigmi

// ============================================================================================
// context
// ============================================================================================
extern "C" int eig_random_normal(int64_t count, unsigned seed, double *out)
{
  return guard(nullptr, [&] {
    EIG_CHECK(count >= 0 && (out || count == 0), EIG_ERR_ARG, "eig_random_normal: bad argument");
    host_random_normal(count, seed, out);
  });
}

extern "C" int eig_device_count(int *count)
{
  return guard(nullptr, [&] {
    EIG_CHECK(count, EIG_ERR_ARG, "eig_device_count: null");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *count = (e == hipSuccess) ? c : 0;
  });
}

extern "C" const char *eig_version(void) { return "eigmi 0.2 gfx950 (band-image plane march SpMV / Lanczos / SpMM, SELL-64, MFMA f64 Gram, RCCL halo)"; }

extern "C" int eig_ctx_create(int device, eig_ctx_t *out)
{
  return guard(nullptr, [&] {
    EIG_CHECK(out, EIG_ERR_ARG, "eig_ctx_create: null output");
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c == 0) throw Error(EIG_ERR_NODEVICE, "no HIP device visible");
    EIG_CHECK(device >= 0 && device < c, EIG_ERR_ARG, "eig_ctx_create: bad device index");
    EIG_HIP(hipSetDevice(device));
    auto *ctx = new eig_ctx_s();
    ctx->device = device;
    try
    {
      EIG_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
      EIG_HIP(hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking));
      hipDeviceProp_t prop;
      EIG_HIP(hipGetDeviceProperties(&prop, device));
      ctx->num_cu = prop.multiProcessorCount;
      ctx->red.partials = dev_alloc<double>((size_t)kMaxRedBlocks * kMaxRedVals);
      ctx->red.tickets = dev_alloc<unsigned>((size_t)kNumTickets * kTicketStride);
      EIG_HIP(hipMemset(ctx->red.tickets, 0, (size_t)kNumTickets * kTicketStride * sizeof(unsigned)));
      ctx->scratch = dev_alloc<double>(4096);
      EIG_HIP(hipMemset(ctx->scratch, 0, 4096 * sizeof(double)));
    }
    catch (...)
    {
      eig_ctx_destroy(ctx);
      throw;
    }
    *out = ctx;
  });
}

extern "C" int eig_ctx_destroy(eig_ctx_t ctx)
{
  if (!ctx) return EIG_OK;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  mgs_release(ctx);
  comm_destroy(ctx);
  for (auto &e : ctx->pool)
    if (e.first) (void)hipFree(e.first);
  if (ctx->red.partials) (void)hipFree(ctx->red.partials);
  if (ctx->red.tickets) (void)hipFree(ctx->red.tickets);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->comm_stream) (void)hipStreamDestroy(ctx->comm_stream);
  if (ctx->red_stream) (void)hipStreamDestroy(ctx->red_stream);
  delete ctx;
  return EIG_OK;
}

namespace eigmi {
std::string &tls_error()
{
  thread_local std::string e;
  return e;
}
}  // namespace eigmi

extern "C" const char *eig_last_error(eig_ctx_t ctx) { return ctx ? ctx->last_error.c_str() : tls_error().c_str(); }

extern "C" int eig_ctx_sync(eig_ctx_t ctx)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx, EIG_ERR_ARG, "null context");
    EIG_HIP(hipStreamSynchronize(ctx->stream));
    mgs_lookahead_check(ctx);  // (eig_orthonormalize_mv8 is asynchronous: its barrier error surfaces here)
  });
}

extern "C" int eig_ctx_stream(eig_ctx_t ctx, void **stream)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && stream, EIG_ERR_ARG, "null argument");
    *stream = (void *)ctx->stream;
  });
}

// ============================================================================================
// device memory
// ============================================================================================
extern "C" int eig_malloc(eig_ctx_t ctx, size_t bytes, void **ptr)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && ptr, EIG_ERR_ARG, "eig_malloc: null argument");
    DeviceGuard dg(ctx->device);
    EIG_HIP(hipMalloc(ptr, bytes ? bytes : 1));
  });
}
extern "C" int eig_free(eig_ctx_t ctx, void *ptr)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx, EIG_ERR_ARG, "null context");
    if (ptr) EIG_HIP(hipFree(ptr));
  });
}
extern "C" int eig_memcpy_h2d(eig_ctx_t ctx, void *dst, const void *src, size_t bytes)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx, EIG_ERR_ARG, "null context");
    EIG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    EIG_HIP(hipStreamSynchronize(ctx->stream));
  });
}
extern "C" int eig_memcpy_d2h(eig_ctx_t ctx, void *dst, const void *src, size_t bytes)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx, EIG_ERR_ARG, "null context");
    EIG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    EIG_HIP(hipStreamSynchronize(ctx->stream));
  });
}
extern "C" int eig_memcpy_d2d(eig_ctx_t ctx, void *dst, const void *src, size_t bytes)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx, EIG_ERR_ARG, "null context");
    EIG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  });
}
extern "C" int eig_memset(eig_ctx_t ctx, void *dst, int value, size_t bytes)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx, EIG_ERR_ARG, "null context");
    EIG_HIP(hipMemsetAsync(dst, value, bytes, ctx->stream));
  });
}

// ============================================================================================
// matrices
// ============================================================================================
namespace {

template <class T>
T *dev_upload(const T *host, size_t count, hipStream_t s)
{
  T *d = dev_alloc<T>(count);
  EIG_HIP(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, s));
  return d;
}

// The SELL-C image (mat_image.cpp build_sell_image) onto the device; the host image is released on return.
void upload_sell(eig_mat_s &A, SellImage &&S)
{
  A.R = 1;  // one row per lane (2 / 4 measured slower for the fused Lanczos kernel)
  const i64 C = 64 * (i64)A.R, ns = S.nslices, total = S.nnzb_padded, bb = A.br * A.bc;
  hipStream_t s = A.ctx->stream;
  A.bandwidth = S.bandwidth;
  A.nslices = ns;
  A.nnzb_padded = total;
  A.slice_ptr = dev_upload(S.slice_ptr.data(), ns + 1, s);
  A.col = dev_upload(S.col.data(), total, s);
  A.val = dev_upload(S.val.data(), total * bb, s);
  A.n_stencil_slices = S.n_stencil_slices;
  A.sell_explicit = S.sell_explicit;
  if (A.n_stencil_slices > 0)
  {
    A.st_width = dev_upload(S.st_width.data(), ns, s);
    A.st_delta = dev_upload(S.st_delta.data(), 8 * ns, s);
    A.st_mask = dev_upload(S.st_mask.data(), ns * C, s);
  }
  EIG_HIP(hipStreamSynchronize(s));
  A.device_bytes = (ns + 1) * 8 + total * 4 + total * bb * 8 + (A.n_stencil_slices ? ns * (36 + C) : 0);
}

// The symmetric band image (mat_image.cpp build_sym_image) onto the device, where it was built.
void upload_sym(eig_mat_s &A, SymImage &&S)
{
  if (!S.built) return;
  const i64 ns = A.nslices;
  const int mb = S.mask_bytes;
  hipStream_t s = A.ctx->stream;
  A.sym_uniform = S.uniform;
  A.sym_geo = S.geo;
  A.sym_box27 = S.box27;
  A.sym_gx = S.gx;
  A.sym_gy = S.gy;
  A.sym_gz = S.gz;
  A.sym_gz0 = S.gz0;
  A.sym_val = dev_upload(S.val.data(), (size_t)S.nup * S.ld, s);
  A.sym_mask = mb == 1 ? (void *)dev_upload(S.mask8.data(), ns * 64, s)
                       : (void *)dev_upload(S.mask32.data(), ns * 64, s);
  EIG_HIP(hipStreamSynchronize(s));
  A.sym_mask_bytes = mb;
  A.sym_nd = S.nd;
  A.sym_nup = S.nup;
  A.sym_ld = S.ld;
  for (int k = 0; k < S.nd; ++k)
  {
    A.sym_off[k] = S.off[k];
    A.sym_dj[k] = S.dj[k];
  }
  for (int j = 0; j < S.nup; ++j) A.sym_uc[j] = S.uc[j];
  A.device_bytes += (i64)S.nup * S.ld * 8 + ns * 64 * mb;
}

void destroy_mat(eig_mat_s *A)
{
  if (!A) return;
  if (A->slice_ptr) (void)hipFree(A->slice_ptr);
  if (A->col) (void)hipFree(A->col);
  if (A->val) (void)hipFree(A->val);
  if (A->st_width) (void)hipFree(A->st_width);
  if (A->st_delta) (void)hipFree(A->st_delta);
  if (A->st_mask) (void)hipFree(A->st_mask);
  if (A->slice_list) (void)hipFree(A->slice_list);
  if (A->march_bnd) (void)hipFree(A->march_bnd);
  if (A->sym_val) (void)hipFree(A->sym_val);
  if (A->sym_pack) (void)hipFree(A->sym_pack);
  if (A->sym_mask) (void)hipFree(A->sym_mask);
  if (A->box_val) (void)hipFree(A->box_val);
  if (A->box_ctab) (void)hipFree(A->box_ctab);
  if (A->box_cmask) (void)hipFree(A->box_cmask);
  delete A;
}

// A new matrix of shape `sh` with the images of its `nb` owned rows (columns shifted by col_shift block columns
// into the window); `finish` completes it (the halo plan of a distributed matrix).  The SELL image is built,
// uploaded and released before the band image is built: the two never share the host.
template <class F>
eig_mat_s *create_mat(eig_ctx_t ctx, const MatShape &sh, i64 nb, i64 col_shift, const int64_t *rowptr,
                      const int32_t *col, const double *vals, F &&finish)
{
  auto *A = new eig_mat_s();
  A->ctx = ctx;
  A->kflags = sh.kflags;
  A->br = sh.br;
  A->bc = sh.bc;
  A->nb_rows = nb;
  A->nb_rows_global = sh.nb_rows_global;
  A->nb_cols = sh.nb_cols;
  A->row_begin = sh.row_begin;
  A->win_begin = col_shift * sh.bc;
  A->window = sh.window;
  A->own_offset = sh.own_offset;
  A->nnzb = rowptr[nb];
  try
  {
    upload_sell(*A, build_sell_image(sh, nb, rowptr, col, vals, col_shift));
    upload_sym(*A, build_sym_image(sh, A->nslices, A->nnzb_padded, nb, rowptr, col, vals));
    const DiagShare d = diag_share(sh.br, sh.bc, nb, sh.row_begin, rowptr, col, vals);
    A->diag_sum = d.sum;
    A->diag_count = d.count;
    finish(*A);
  }
  catch (...)
  {
    destroy_mat(A);
    throw;
  }
  return A;
}

}  // namespace

extern "C" int eig_mat_create_bcsr(eig_ctx_t ctx, int64_t nb_rows, int64_t nb_cols, int br, int bc,
                                   const int64_t *rowptr, const int32_t *col, const double *vals, eig_mat_t *out)
{
  return eig_mat_create_bcsr_ex(ctx, nb_rows, nb_cols, br, bc, rowptr, col, vals, 0, out);
}

extern "C" int eig_mat_create_bcsr_ex(eig_ctx_t ctx, int64_t nb_rows, int64_t nb_cols, int br, int bc,
                                      const int64_t *rowptr, const int32_t *col, const double *vals, int flags,
                                      eig_mat_t *out)
{
  return guard(ctx, [&] {
    EIG_CHECK((flags & ~EIG_MAT_FLAGS_ALL) == 0, EIG_ERR_ARG, "eig_mat_create_bcsr_ex: unknown flag");
    EIG_CHECK(ctx && out && rowptr && (rowptr[nb_rows] == 0 || (col && vals)), EIG_ERR_ARG,
              "eig_mat_create_bcsr: null argument");
    EIG_CHECK(nb_rows >= 0 && nb_cols >= 0, EIG_ERR_ARG, "eig_mat_create_bcsr: negative size");
    EIG_CHECK(br >= 1 && br <= 4 && bc >= 1 && bc <= 4, EIG_ERR_BLOCKSIZE, "block size must be in 1..4");
    EIG_CHECK(nb_cols * bc < (int64_t)INT32_MAX, EIG_ERR_SHAPE, "matrix too large for int32 column indices");
    DeviceGuard dg(ctx->device);
    validate_csr(nb_rows, nb_cols, rowptr, col);
    MatShape sh;
    sh.br = br;
    sh.bc = bc;
    sh.kflags = flags;
    sh.nb_rows_global = nb_rows;
    sh.nb_cols = nb_cols;
    sh.window = nb_cols * bc;
    *out = create_mat(ctx, sh, nb_rows, 0, rowptr, col, vals, [](eig_mat_s &) {});
  });
}

extern "C" int eig_mat_create_bcsr_dist(eig_ctx_t ctx, int64_t nb_rows_global, int64_t row_begin,
                                        int64_t nb_local, int br, int bc, const int64_t *rowptr, const int32_t *col,
                                        const double *vals, eig_mat_t *out)
{
  return eig_mat_create_bcsr_dist_ex(ctx, nb_rows_global, row_begin, nb_local, br, bc, rowptr, col, vals, 0, out);
}

extern "C" int eig_mat_create_bcsr_dist_ex(eig_ctx_t ctx, int64_t nb_rows_global, int64_t row_begin,
                                           int64_t nb_local, int br, int bc, const int64_t *rowptr,
                                           const int32_t *col, const double *vals, int flags, eig_mat_t *out)
{
  return guard(ctx, [&] {
    EIG_CHECK((flags & ~EIG_MAT_FLAGS_ALL) == 0, EIG_ERR_ARG, "eig_mat_create_bcsr_dist_ex: unknown flag");
    EIG_CHECK(ctx && out && rowptr, EIG_ERR_ARG, "eig_mat_create_bcsr_dist: null argument");
    EIG_CHECK(br == bc && br >= 1 && br <= 4, EIG_ERR_BLOCKSIZE, "distributed matrices need square blocks 1..4");
    EIG_CHECK(row_begin >= 0 && nb_local >= 0 && row_begin + nb_local <= nb_rows_global, EIG_ERR_SHAPE,
              "eig_mat_create_bcsr_dist: row range outside the matrix");
    EIG_CHECK(nb_rows_global * bc < (int64_t)INT32_MAX, EIG_ERR_SHAPE, "matrix too large for int32 column indices");
    DeviceGuard dg(ctx->device);
    validate_csr(nb_local, nb_rows_global, rowptr, col);
    const int P = ctx->nranks, me = ctx->rank;
    int64_t plan[5];
    {
      int rc = eig_plan_window(row_begin, nb_local, bc, rowptr, col, plan);
      EIG_CHECK(rc == EIG_OK, rc, "eig_plan_window failed");
    }
    const i64 wb_blk = plan[0], cmin = plan[3], cmax = plan[4];
    MatShape sh;
    sh.br = br;
    sh.bc = bc;
    sh.kflags = flags;
    sh.nb_rows_global = sh.nb_cols = nb_rows_global;
    sh.row_begin = row_begin;
    sh.window = plan[1];
    sh.own_offset = plan[2];
    *out = create_mat(ctx, sh, nb_local, wb_blk, rowptr, col, vals, [&](eig_mat_s &A) {
      // --- halo plan: allgather (row_begin, nb_local, cmin, cmax) of every rank ---
      const std::vector<i64> all = allgather_rows(ctx, {row_begin, nb_local, cmin, cmax});
      const int nr = ctx->distributed() ? P : 1;
      std::vector<int64_t> rv(3 * (size_t)nr), sd(3 * (size_t)nr);
      int nrecv = 0, nsend = 0;
      {
        int rc = eig_plan_halo(nr, nr > 1 ? me : 0, all.data(), bc, wb_blk, rv.data(), &nrecv, sd.data(), &nsend);
        EIG_CHECK(rc == EIG_OK, rc, "eig_plan_halo failed");
      }
      halo_staging_ensure(ctx, all, bc);
      for (int k = 0; k < nrecv; ++k) A.recvs.push_back({(int)rv[3 * k], rv[3 * k + 1], rv[3 * k + 2]});
      for (int k = 0; k < nsend; ++k) A.sends.push_back({(int)sd[3 * k], sd[3 * k + 1], sd[3 * k + 2]});
      for (auto &r : A.recvs) A.halo_recv += r.count;
      for (auto &r : A.sends) A.halo_send += r.count;
      // interior / boundary slices and the plane-march split (planes of D rows) of the interior planes
      i64 D;
      if (!march_geometry(A, D)) D = 0;
      const SliceSplit sp = split_slices(A.nslices, nb_local, row_begin, rowptr, col, D);
      A.n_interior = (i64)sp.interior.size();
      A.n_boundary = (i64)sp.boundary.size();
      std::vector<i32> lst(sp.interior);
      lst.insert(lst.end(), sp.boundary.begin(), sp.boundary.end());
      A.slice_list = dev_alloc<i32>(std::max<size_t>(lst.size(), 1));
      if (!lst.empty()) EIG_HIP(hipMemcpy(A.slice_list, lst.data(), lst.size() * sizeof(i32), hipMemcpyHostToDevice));
      if (sp.mz1 - sp.mz0 >= 2)
      {
        const std::vector<i32> &bnd = sp.march_bnd;
        A.mz0 = sp.mz0;
        A.mz1 = sp.mz1;
        A.n_march_bnd = (i64)bnd.size();
        A.march_bnd = dev_alloc<i32>(std::max<size_t>(bnd.size(), 1));
        if (!bnd.empty()) EIG_HIP(hipMemcpy(A.march_bnd, bnd.data(), bnd.size() * sizeof(i32), hipMemcpyHostToDevice));
      }
    });
  });
}

namespace eigmi {
void mat_download_bcsr(const eig_mat_s &A, std::vector<i64> &rowptr, std::vector<i32> &col, std::vector<double> &vals)
{
  EIG_CHECK(!A.ctx->distributed() || A.nb_rows == A.nb_rows_global, EIG_ERR_ARG, "download: single-rank matrix only");
  const i64 C = 64 * (i64)A.R, ns = A.nslices, bb = (i64)A.br * A.bc;
  std::vector<i64> sp(ns + 1);
  std::vector<i32> ci(std::max<i64>(A.nnzb_padded, 1));
  std::vector<double> vi(std::max<i64>(A.nnzb_padded * bb, 1));
  EIG_HIP(hipMemcpy(sp.data(), A.slice_ptr, (ns + 1) * sizeof(i64), hipMemcpyDeviceToHost));
  if (A.nnzb_padded)
  {
    EIG_HIP(hipMemcpy(ci.data(), A.col, A.nnzb_padded * sizeof(i32), hipMemcpyDeviceToHost));
    EIG_HIP(hipMemcpy(vi.data(), A.val, A.nnzb_padded * bb * sizeof(double), hipMemcpyDeviceToHost));
  }
  rowptr.assign(A.nb_rows + 1, 0);
  col.clear();
  vals.clear();
  for (i64 r = 0; r < A.nb_rows; ++r)
  {
    const i64 s = r / C, l = r % C, base = sp[s], w = (sp[s + 1] - base) / C;
    for (i64 k = 0; k < w; ++k)
    {
      const i32 c = ci[base + k * C + l];
      if (c < 0) continue;
      col.push_back(c + (i32)(A.win_begin / A.bc));
      for (i64 t = 0; t < bb; ++t) vals.push_back(vi[(base + k * C) * bb + t * C + l]);
    }
    rowptr[r + 1] = (i64)col.size();
  }
}
}  // namespace eigmi

extern "C" int eig_mat_destroy(eig_mat_t A)
{
  if (!A) return EIG_OK;
  (void)hipSetDevice(A->ctx->device);
  (void)hipStreamSynchronize(A->ctx->stream);
  destroy_mat(A);
  return EIG_OK;
}

extern "C" int eig_mat_get_info(eig_mat_t A, eig_mat_info *info)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && info, EIG_ERR_ARG, "null argument");
    info->n = A->nb_rows * A->br;
    info->n_global = A->nb_rows_global * A->br;
    info->ncols = A->nb_cols * A->bc;
    info->row_begin = A->row_begin * A->br;
    info->window = A->window;
    info->own_offset = A->own_offset;
    info->nnzb = A->nnzb;
    info->nnzb_padded = A->nnzb_padded;
    info->nslices = A->nslices;
    info->br = A->br;
    info->bc = A->bc;
    info->halo_recv = A->halo_recv;
    info->halo_send = A->halo_send;
    info->device_bytes = A->device_bytes;
    info->stencil_slices = A->n_stencil_slices;
    info->rows_per_lane = A->R;
    info->sym_offsets = A->sym_val ? A->sym_nd : 0;
    info->sym_arrays = A->sym_val ? A->sym_nup : 0;
    info->sym_mask_bytes = A->sym_val ? A->sym_mask_bytes : 0;
    info->sym_uniform = (A->sym_val && A->sym_uniform && !(A->kflags & EIG_MAT_NO_UNIFORM))
                            ? (A->sym_geo ? 2 : 1)
                            : 0;
    info->sym_geo = A->sym_val && A->sym_geo ? 1 : 0;
    info->march_variant = march_variant(*A, true);
    info->march_variant_mv = march_variant(*A, false);
    info->march_pipe = march_pipe(*A);
  });
}

extern "C" int eig_lanczos_kernel_info(eig_mat_t A, int fused, char *name, int name_len, int64_t *bytes)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && bytes && (name || name_len == 0), EIG_ERR_ARG, "eig_lanczos_kernel_info: null argument");
    std::string nm;
    i64 b = 0;
    lanczos_kernel_info(*A, fused != 0, nm, b);
    *bytes = b;
    if (name_len > 0)
    {
      const size_t k = std::min<size_t>(nm.size(), (size_t)name_len - 1);
      std::memcpy(name, nm.data(), k);
      name[k] = 0;
    }
  });
}

extern "C" int eig_mat_kernel_info(eig_mat_t A, int op, char *name, int name_len)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && name && name_len > 0, EIG_ERR_ARG, "eig_mat_kernel_info: null argument");
    EIG_CHECK(op >= EIG_OP_SPMV && op <= EIG_OP_FILT32, EIG_ERR_ARG, "eig_mat_kernel_info: bad op");
    const std::string nm = kernel_for(*A, op);
    const size_t k = std::min<size_t>(nm.size(), (size_t)name_len - 1);
    std::memcpy(name, nm.data(), k);
    name[k] = 0;
  });
}

extern "C" int eig_mat_shift_diag(eig_mat_t A, double shift)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A, EIG_ERR_ARG, "null matrix");
    EIG_CHECK(A->br == A->bc, EIG_ERR_BLOCKSIZE, "StandardLargest: blocks of input matrix must be square");
    DeviceGuard dg(A->ctx->device);
    launch_shift_diag(*A, shift, A->ctx->stream);
  });
}

extern "C" int eig_mat_tune(eig_mat_t A, int key, int value)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && value >= 0, EIG_ERR_ARG, "eig_mat_tune: bad argument");
    EIG_CHECK(key == EIG_TUNE_MARCH_RUNS || key == EIG_TUNE_BOX_SEGS || key == EIG_TUNE_MARCH_PREFETCH ||
                  key == EIG_TUNE_HALO || key == EIG_TUNE_CACHE || key == EIG_TUNE_BOX_COLS ||
                  key == EIG_TUNE_BOX_MAP || key == EIG_TUNE_SELL_CPF || key == EIG_TUNE_MARCH_LINES,
              EIG_ERR_ARG, "eig_mat_tune: unknown key");
    EIG_CHECK(key != EIG_TUNE_HALO || value <= 1, EIG_ERR_ARG, "eig_mat_tune: halo mode 0 / 1");
    EIG_CHECK(key != EIG_TUNE_MARCH_PREFETCH || value <= 18, EIG_ERR_ARG, "eig_mat_tune: march variant 0..18");
    if (key == EIG_TUNE_MARCH_RUNS)
      A->tune_march_runs = value;
    else if (key == EIG_TUNE_MARCH_PREFETCH)
      A->tune_march_prefetch = value;
    else if (key == EIG_TUNE_HALO)
      A->tune_halo_whole = value;
    else if (key == EIG_TUNE_CACHE)
      A->tune_cache = value;
    else if (key == EIG_TUNE_MARCH_LINES)
    {
      EIG_CHECK(value == 0 || value == 4, EIG_ERR_ARG, "eig_mat_tune: march lines 0 / 4");
      A->tune_march_lines = value;
    }
    else if (key == EIG_TUNE_SELL_CPF)
    {
      EIG_CHECK(value <= 2, EIG_ERR_ARG, "eig_mat_tune: column prefetch 0 / 1 / 2");
      A->tune_sell_cpf = value;
    }
    else if (key == EIG_TUNE_BOX_MAP)
    {
      EIG_CHECK(value <= 1, EIG_ERR_ARG, "eig_mat_tune: box map 0 / 1");
      A->tune_box_map = value;
    }
    else if (key == EIG_TUNE_BOX_COLS)
    {
      EIG_CHECK(value == 0 || value == 16 || value == 32, EIG_ERR_ARG, "eig_mat_tune: box columns 0 / 16 / 32");
      A->tune_box_cols = value;
    }
    else
      A->tune_box_segs = value;
  });
}

namespace eigmi {
// y = A x with halo exchange overlapped with the interior slices when distributed.
void mv_device(eig_mat_s &A, double *x, double *y)
{
  eig_ctx_t ctx = A.ctx;
  if (!ctx->distributed() || (A.recvs.empty() && A.sends.empty()))
  {
    launch_spmv(A, x, y, nullptr, 0, A.nslices, ctx->stream);
    return;
  }
  // interior / boundary split: the interior planes on the plane march when it applies, else the
  // interior slices
  const bool mz = march_split_active(A);
  auto interior = [&](hipStream_t s) {
    if (mz) launch_spmv(A, x, y, &kMarchInteriorTag, 0, 0, s);
    else launch_spmv(A, x, y, A.slice_list, 0, A.n_interior, s);
  };
  auto boundary = [&](hipStream_t s) {
    if (mz) launch_spmv(A, x, y, A.march_bnd, 0, A.n_march_bnd, s);
    else launch_spmv(A, x, y, A.slice_list, A.n_interior, A.n_boundary, s);
  };
  if (ctx->loopback())
  {
    // synchronous exchange, then the same interior / boundary launches as the RCCL path
    halo_exchange(A, x, ctx->stream);
    interior(ctx->stream);
    boundary(ctx->stream);
    return;
  }
  hipEvent_t e0, e1;
  EIG_HIP(hipEventCreateWithFlags(&e0, hipEventDisableTiming));
  EIG_HIP(hipEventCreateWithFlags(&e1, hipEventDisableTiming));
  EIG_HIP(hipEventRecord(e0, ctx->stream));
  EIG_HIP(hipStreamWaitEvent(ctx->comm_stream, e0, 0));
  halo_exchange(A, x, ctx->comm_stream);
  EIG_HIP(hipEventRecord(e1, ctx->comm_stream));
  interior(ctx->stream);
  EIG_HIP(hipStreamWaitEvent(ctx->stream, e1, 0));
  boundary(ctx->stream);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
}
}  // namespace eigmi

extern "C" int eig_mv(eig_mat_t A, const double *x, double *y)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && x && y, EIG_ERR_ARG, "eig_mv: null argument");
    DeviceGuard dg(A->ctx->device);
    mv_device(*A, const_cast<double *>(x), y);
  });
}

extern "C" int eig_mv_timed(eig_mat_t A, const double *x, double *y, int reps, double *avg_ms)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && x && y && avg_ms && reps > 0, EIG_ERR_ARG, "eig_mv_timed: bad argument");
    DeviceGuard dg(A->ctx->device);
    hipStream_t s = A->ctx->stream;
    hipEvent_t e0, e1;
    EIG_HIP(hipEventCreate(&e0));
    EIG_HIP(hipEventCreate(&e1));
    EIG_HIP(hipEventRecord(e0, s));
    for (int r = 0; r < reps; ++r) mv_device(*A, const_cast<double *>(x), y);
    EIG_HIP(hipEventRecord(e1, s));
    EIG_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    EIG_HIP(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = ms / reps;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  });
}

extern "C" int eig_mv_host(eig_mat_t A, const double *xh, double *yh)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && xh && yh, EIG_ERR_ARG, "eig_mv_host: null argument");
    DeviceGuard dg(A->ctx->device);
    eig_ctx_t ctx = A->ctx;
    const size_t wb = (size_t)A->window * sizeof(double);
    double *x = (double *)ctx_buffer(ctx, kSlotMvHostX, wb);
    double *y = (double *)ctx_buffer(ctx, kSlotMvHostY, wb);
    const i64 n = A->nb_rows * A->br;
    if (A->nb_rows_global == A->nb_rows && !ctx->distributed())
    {
      // square or rectangular single-rank operator: x has ncols entries
      EIG_HIP(hipMemcpyAsync(x, xh, (size_t)A->nb_cols * A->bc * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    else
    {
      EIG_HIP(hipMemsetAsync(x, 0, wb, ctx->stream));
      EIG_HIP(hipMemcpyAsync(x + A->own_offset, xh, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    mv_device(*A, x, y);
    EIG_HIP(hipMemcpyAsync(yh, y + A->own_offset, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    EIG_HIP(hipStreamSynchronize(ctx->stream));
  });
}

// ============================================================================================
// BlockVector ops
// ============================================================================================
extern "C" int eig_dot(eig_ctx_t ctx, int64_t n, const double *x, const double *y, double *result)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && x && y && result && n >= 0, EIG_ERR_ARG, "eig_dot: bad argument");
    DeviceGuard dg(ctx->device);
    launch_dot(n, x, y, result, 0, ctx->stream, ctx->red);
    allreduce_sum(ctx, result, 1, ctx->stream);
  });
}
extern "C" int eig_nrm2(eig_ctx_t ctx, int64_t n, const double *x, double *result)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && x && result && n >= 0, EIG_ERR_ARG, "eig_nrm2: bad argument");
    DeviceGuard dg(ctx->device);
    launch_nrm2sq(n, x, result, 0, ctx->stream, ctx->red);
    allreduce_sum(ctx, result, 1, ctx->stream);
    launch_sqrt_inplace(result, 1, ctx->stream);
  });
}
extern "C" int eig_lanczos_update(eig_ctx_t ctx, int64_t n, const double *alpha, const double *beta,
                                  const double *v, const double *vprev, double *w, double *result)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && alpha && v && w && result && n >= 0 && (!vprev || beta), EIG_ERR_ARG,
              "eig_lanczos_update: bad argument");
    DeviceGuard dg(ctx->device);
    launch_lanczos_update_ext(n, alpha, beta, v, vprev, w, result, 0, ctx->stream, ctx->red);
    allreduce_sum(ctx, result, 2, ctx->stream);  // ||w||^2 and v.w in ONE allreduce
    launch_sqrt_inplace(result, 1, ctx->stream);
  });
}
extern "C" int eig_axpy(eig_ctx_t ctx, int64_t n, double a, const double *x, double *y)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && x && y && n >= 0, EIG_ERR_ARG, "eig_axpy: bad argument");
    DeviceGuard dg(ctx->device);
    launch_axpy(n, a, x, y, ctx->stream);
  });
}
extern "C" int eig_scal(eig_ctx_t ctx, int64_t n, double a, double *x)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && x && n >= 0, EIG_ERR_ARG, "eig_scal: bad argument");
    DeviceGuard dg(ctx->device);
    launch_scal(n, a, x, ctx->stream);
  });
}
extern "C" int eig_copy(eig_ctx_t ctx, int64_t n, const double *x, double *y)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && x && y && n >= 0, EIG_ERR_ARG, "eig_copy: bad argument");
    DeviceGuard dg(ctx->device);
    EIG_HIP(hipMemcpyAsync(y, x, n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  });
}
extern "C" int eig_fill_normal(eig_ctx_t ctx, int64_t count, unsigned seed, double *x)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && x && count >= 0, EIG_ERR_ARG, "eig_fill_normal: bad argument");
    DeviceGuard dg(ctx->device);
    if (count > 0) launch_fill_normal(count, seed, x, ctx->stream);
  });
}

extern "C" int eig_stream_copy_timed(eig_ctx_t ctx, int64_t n, const double *x, double *y, int reps, int mode,
                                     double *avg_ms)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && x && y && n >= 0 && reps >= 1 && avg_ms, EIG_ERR_ARG, "eig_stream_copy_timed: bad argument");
    DeviceGuard dg(ctx->device);
    hipStream_t s = ctx->stream;
    hipEvent_t e0, e1;
    EIG_HIP(hipEventCreate(&e0));
    EIG_HIP(hipEventCreate(&e1));
    launch_stream_copy(n, x, y, ctx->num_cu, s, mode);  // warm-up
    EIG_HIP(hipEventRecord(e0, s));
    for (int r = 0; r < reps; ++r) launch_stream_copy(n, x, y, ctx->num_cu, s, mode);
    EIG_HIP(hipEventRecord(e1, s));
    EIG_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    EIG_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *avg_ms = ms / reps;
  });
}

// ============================================================================================
// MultiVector<double,8>
// ============================================================================================
// (the Gram and the orthonormalisations: orth.cpp)
extern "C" int eig_spmm_mv8(eig_mat_t A, int64_t m, const double *Qin, double *Qout)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && Qin && Qout, EIG_ERR_ARG, "eig_spmm_mv8: null argument");
    EIG_MV8_CHECK(m);
    // the reference's entry point keeps the reference's refusal; blocks go through eig_spmm_blk_mv8
    EIG_CHECK(A->br == 1 && A->bc == 1, EIG_ERR_BLOCKSIZE,
              "matmul_sparse_tallskinny_blocked: only implemented for FieldMatrix<..,1,1>");
    EIG_CHECK(A->nb_rows == A->nb_cols && !A->ctx->distributed(), EIG_ERR_SHAPE,
              "eig_spmm_mv8: square single-rank matrix required");
    DeviceGuard dg(A->ctx->device);
    if (m > 0) launch_spmm_mv8(*A, m, Qin, Qout, A->ctx->stream);
  });
}

extern "C" int eig_spmm_blk_mv8(eig_mat_t A, int64_t m, const double *Qin, double *Qout)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && Qin && Qout && Qin != Qout, EIG_ERR_ARG, "eig_spmm_blk_mv8: null or aliased argument");
    EIG_MV8_CHECK(m);
    EIG_CHECK(A->br == A->bc, EIG_ERR_BLOCKSIZE, "eig_spmm_blk_mv8: blocks of input matrix must be square");
    EIG_CHECK(A->nb_rows == A->nb_cols && !A->ctx->distributed(), EIG_ERR_SHAPE,
              "eig_spmm_blk_mv8: square single-rank matrix required");
    DeviceGuard dg(A->ctx->device);
    if (m > 0) launch_spmm_mv8(*A, m, Qin, Qout, A->ctx->stream);  // 1x1: the eig_spmm_mv8 kernels
  });
}

extern "C" int eig_resid_mv8(eig_mat_t A, int64_t m, const double *X, const double *B, double *R)
{
  return guard(A ? A->ctx : nullptr, [&] {
    EIG_CHECK(A && X && B && R, EIG_ERR_ARG, "eig_resid_mv8: null argument");
    EIG_CHECK(R != X, EIG_ERR_ARG, "eig_resid_mv8: R must not alias X");
    EIG_MV8_CHECK(m);
    EIG_CHECK(A->br == A->bc && A->br >= 1 && A->br <= 4, EIG_ERR_BLOCKSIZE,
              "eig_resid_mv8: square blocks 1..4 required");
    EIG_CHECK(A->nb_rows == A->nb_cols && !A->ctx->distributed(), EIG_ERR_SHAPE,
              "eig_resid_mv8: square single-rank matrix required");
    DeviceGuard dg(A->ctx->device);
    if (m > 0) launch_resid_mv8(*A, m, X, B, R, A->ctx->stream);
  });
}

extern "C" int eig_dot_diag_mv8(eig_ctx_t ctx, int64_t n, int64_t m, const double *Q1, const double *Q2, double *dp)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && Q1 && Q2 && dp && n >= 0, EIG_ERR_ARG, "eig_dot_diag_mv8: bad argument");
    EIG_MV8_CHECK(m);
    DeviceGuard dg(ctx->device);
    for (i64 b = 0; b < m; b += 8 * 32)
    {
      const i64 mm = std::min<i64>(m - b, 8 * 32);
      launch_dot_diag_mv8(n, mm, Q1 + b * n, Q2 + b * n, dp + b, 0, ctx->stream, ctx->red);
    }
    allreduce_sum(ctx, dp, m, ctx->stream);
  });
}

extern "C" int eig_random_mv8(eig_ctx_t ctx, int64_t n, int64_t m, unsigned seed, double *Q)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && Q && n >= 0, EIG_ERR_ARG, "eig_random_mv8: bad argument");
    EIG_MV8_CHECK(m);
    DeviceGuard dg(ctx->device);
    std::vector<double> h((size_t)(n * m));
    // (block, row, col) fill order == the flat block-column-major order
    host_random_normal(n * m, seed, h.data());
    EIG_HIP(hipMemcpyAsync(Q, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    EIG_HIP(hipStreamSynchronize(ctx->stream));
  });
}

// ============================================================================================
// partition planning (host only)
// ============================================================================================
extern "C" int eig_plan_window(int64_t row_begin, int64_t nb_local, int bc, const int64_t *rowptr,
                               const int32_t *col, int64_t out[5])
{
  if (!rowptr || !out || nb_local < 0 || row_begin < 0 || bc < 1) return EIG_ERR_ARG;
  if (rowptr[nb_local] > 0 && !col) return EIG_ERR_ARG;
  i64 cmin = row_begin, cmax = row_begin + nb_local;  // [cmin, cmax) in block columns
  for (i64 p = 0; p < rowptr[nb_local]; ++p)
  {
    cmin = std::min<i64>(cmin, col[p]);
    cmax = std::max<i64>(cmax, (i64)col[p] + 1);
  }
  const i64 lo = row_begin - cmin;
  const i64 pad = (8 - lo % 8) % 8;  // (lo + pad) * bc is a multiple of 8 scalar entries
  const i64 wb = cmin - pad;
  i64 wlen = (cmax - wb) * bc;
  wlen = (wlen + 7) / 8 * 8;
  out[0] = wb;
  out[1] = wlen;
  out[2] = (row_begin - wb) * bc;
  out[3] = cmin;
  out[4] = cmax;
  return EIG_OK;
}

extern "C" int eig_plan_halo(int nranks, int me, const int64_t *ranks, int bc, int64_t wb_blk, int64_t *recv,
                             int *nrecv, int64_t *send, int *nsend)
{
  if (!ranks || !recv || !send || !nrecv || !nsend || nranks < 1 || me < 0 || me >= nranks) return EIG_ERR_ARG;
  const i64 rb0 = ranks[4 * me], nl = ranks[4 * me + 1], cmin = ranks[4 * me + 2], cmax = ranks[4 * me + 3];
  int nr = 0, ns = 0;
  for (int q = 0; q < nranks; ++q)
  {
    if (q == me) continue;
    const i64 qb = ranks[4 * q], qe = ranks[4 * q] + ranks[4 * q + 1];
    // receive from q: q's rows inside my window
    const i64 rb = std::max(qb, cmin), re = std::min(qe, cmax);
    if (re > rb)
    {
      recv[3 * nr] = q;
      recv[3 * nr + 1] = (rb - wb_blk) * bc;
      recv[3 * nr + 2] = (re - rb) * bc;
      ++nr;
    }
    // send to q: my rows inside q's referenced range
    const i64 qwb = ranks[4 * q + 2], qwe = ranks[4 * q + 3];
    const i64 sb = std::max(rb0, qwb), se = std::min(rb0 + nl, qwe);
    if (se > sb)
    {
      send[3 * ns] = q;
      send[3 * ns + 1] = (sb - wb_blk) * bc;
      send[3 * ns + 2] = (se - sb) * bc;
      ++ns;
    }
  }
  *nrecv = nr;
  *nsend = ns;
  return EIG_OK;
}
