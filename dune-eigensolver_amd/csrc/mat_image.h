// mat_image.h -- the host images of a matrix that api.cpp uploads and every kernel reads: the SELL-64 image with
// its stencil slices, the symmetric band image with its uniform / geometric / box decisions, and the interior /
// boundary slice split of a distributed matrix.  Plain host arithmetic on a host CSR matrix: no device code, no
// HIP runtime call, no context and no eig_mat_s, so host tests compile mat_image.cpp (with gen.cpp) and no GPU.
#pragma once
#include "internal.h"

#include <cstdint>
#include <vector>

namespace eigmi {

// What the builders read of the matrix being created (eig_mat_s's fields of the same names).
struct MatShape {
  int br = 1, bc = 1, kflags = 0;
  i64 nb_rows_global = 0, nb_cols = 0, row_begin = 0;
  i64 window = 0, own_offset = 0;
};

// SELL-C image, C = 64 (layout: internal.h eig_mat_s).  st_* are sized also when no slice is a stencil slice
// (n_stencil_slices == 0: not uploaded).
struct SellImage {
  std::vector<i64> slice_ptr;
  std::vector<i32> col;
  std::vector<double> val;
  std::vector<i32> st_width, st_delta;
  std::vector<uint8_t> st_mask;
  i64 nslices = 0, nnzb_padded = 0, n_stencil_slices = 0, sell_explicit = 0, bandwidth = 0;
};
// `nb` block rows (rowptr/col/vals; global row = row_begin + r), columns shifted by col_shift into window-local
// block columns.
SellImage build_sell_image(const MatShape &A, i64 nb, const int64_t *rowptr, const int32_t *col, const double *vals,
                           i64 col_shift);

// Symmetric band image (internal.h eig_mat_s::sym_*); built == false: it does not apply, nothing else is set.
struct SymImage {
  bool built = false;
  int nd = 0, nup = 0, mask_bytes = 0;
  i64 ld = 0;
  i32 off[kSymMaxOff] = {};
  i32 dj[kSymMaxOff] = {};
  std::vector<double> val;        // nup * ld
  std::vector<uint8_t> mask8;     // nslices * 64 when mask_bytes == 1
  std::vector<uint32_t> mask32;   // nslices * 64 when mask_bytes == 4
  bool uniform = false;
  double uc[kSymMaxOff] = {};
  bool geo = false;
  unsigned box27 = 0;
  int gx = 0, gy = 0, gz = 0, gz0 = 0;
};
SymImage build_sym_image(const MatShape &A, i64 nslices, i64 nnzb_padded, i64 nb, const int64_t *rowptr,
                         const int32_t *col, const double *vals);

// Interior / boundary slices of the owned rows [row_begin, row_begin + nb) (a slice is interior when every column
// is owned) and the plane-march split: planes [mz0, mz1) of D rows (D = 0: no march geometry) are the longest run
// of at least 2 planes whose slices are all interior, march_bnd every slice outside them.  mz1 <= mz0: no split.
struct SliceSplit {
  std::vector<i32> interior, boundary, march_bnd;
  i64 mz0 = 0, mz1 = 0;
};
SliceSplit split_slices(i64 nslices, i64 nb, i64 row_begin, const int64_t *rowptr, const int32_t *col, i64 D);

void validate_csr(i64 nb, i64 ncols, const int64_t *rowptr, const int32_t *col);

// Diagonal share of the owned rows (global row = row_begin + r): sum of the stored diagonal
// entries of the diagonal blocks and the number of scalar rows that store one.
struct DiagShare {
  double sum = 0.0;
  i64 count = 0;
};
DiagShare diag_share(int br, int bc, i64 nb, i64 row_begin, const int64_t *rowptr, const int32_t *col,
                     const double *vals);

// Threads of the builders' passes over slices / rows: 0 = up to 16 hardware threads (the default), n > 0 =
// exactly n (host tests compare a threaded build with a one-thread build).  Passes under 4096 items stay serial.
extern int mat_image_threads;

}  // namespace eigmi
