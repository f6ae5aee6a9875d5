// The plane-march variants (k_march.hip): what each variant number IS, in one table.  The kernels'
// `if constexpr`s and __launch_bounds__ and the launch dispatch (k_march.hip), the selection (march_select),
// the run-count, direction and body rules of march_plan and the byte model of lanczos_kernel_info
// (march_plan.cpp) all read it; adding or retiring a variant is one row here plus its entry in MarchDispatch.  The numbers are public
// (eig_mat_info.march_variant, the profiler's kernel instance names) and do not change.
// Plain C++17: no HIP headers, so host tests include it as it is.
#pragma once

#include <utility>

namespace eigmi {

// Row-loop body a variant runs (templates of k_march.hip).
enum MarchFamily {
  kMarchMasked,  // march_rows' own body: masked selects, any band the march takes
  kMarchGeo,     // march_rows_geo<PF, PG>: whole planes, masks from the coordinates
  kMarchGeo2,    // march_rows_geo2<PF, PG, VAL>: no masks or selects (x extent % 64 == 0, window < 2 GiB)
  kMarchGeo2L2,  // march_rows_geo2_2l: geo2 on the value pack, two grid lines per wave (nd == 7, gy even)
  kMarchKuhn,    // march_rows_kuhn<KP, LX>: the P1 Kuhn 15-point box march
};
// Where the band values come from.
enum MarchValues {
  kMarchUniform,  // the plan's constants (uniform bands): no value stream
  kMarchArrays,   // the band arrays
  kMarchPack,     // the pair-packed copy of the arrays (eig_mat_s::sym_pack; built at the first launch)
};

struct MarchTraits {
  bool valid;
  MarchFamily family;
  int pf;   // geo / geo2: the +D operand is loaded pf + 1 planes ahead
  bool pg;  // geo / geo2: the neighbour gathers one plane ahead
  int val;  // geo2: 0 uniform values, 1 arrays, 2 arrays one plane ahead, 4 arrays through global addresses, 5 pack
  bool kp;  // Kuhn: values from the pack
  bool lx;  // Kuhn: the line exchange through LDS
  MarchValues values;
  bool geo_masks;    // row masks from the grid coordinates (false: the mask array is streamed)
  int mv_waves;      // __launch_bounds__ waves per SIMD of the eig_mv / K1 kernels
  int fused_waves;   // the same of the fused step (registers: no spills)
  int wide_runs;     // fused step on wide planes (>= 1024 columns): at most this many plane runs per column
  bool wide_two;     // fused step on wide planes: two plane runs per column (march_plan)
  bool line_groups;  // takes the 4-line workgroup mapping (EIG_TUNE_MARCH_LINES)
  // the 2-line kernels that also hold the downward body (MarchPlan::down; 24 spills marching upward alone)
  bool down_body;
  // ... whose fused kernel also holds the pipelined bodies (MarchPlan::pipe; 24 keeps the plain body)
  bool pipe_body;

  // whole planes: every marched row exists, no row test
  constexpr bool whole_planes() const { return family != kMarchMasked; }
  // the geo2-style kernel path: march_store (MarchPlan::tstore) and the scalar prologue run under the first loads
  constexpr bool geo2_path() const { return family == kMarchGeo2 || family == kMarchGeo2L2 || family == kMarchKuhn; }
  constexpr bool needs_pack() const { return values == kMarchPack; }
  // band arrays a launch streams per row (byte model): none, the 4 packed arrays of a 7-point band, or all nup
  constexpr int stream_arrays(int nup) const
  {
    return values == kMarchUniform ? 0 : values == kMarchPack && family != kMarchKuhn ? 4 : nup;
  }
  // kernel template head <MT, SPAN1>: <uint32_t, false> for Kuhn, <uint8_t, true> otherwise (variant 0
  // alone also runs as <uint8_t, false> and <uint32_t, false>: any band image)
  constexpr int mask_bytes() const { return family == kMarchKuhn ? 4 : 1; }
  constexpr bool span1() const { return family != kMarchKuhn; }
  constexpr bool any_head() const { return family == kMarchMasked && values == kMarchArrays; }
};

namespace march_kind {
constexpr MarchTraits masked(MarchValues v, bool geo_masks, int fused_waves)
{
  return {true, kMarchMasked, 0, false, 0, false, false, v, geo_masks, 8, fused_waves, 6, false, false};
}
constexpr MarchTraits geo(int pf, bool pg, int fused_waves)
{
  return {true, kMarchGeo, pf, pg, 0, false, false, kMarchUniform, true, 8, fused_waves, 6, false, false};
}
constexpr MarchTraits geo2(int pf, bool pg, int fused_waves, int wide_runs)
{
  return {true, kMarchGeo2, pf, pg, 0, false, false, kMarchUniform, true, 8, fused_waves, wide_runs, false, false};
}
constexpr MarchTraits value(int val, int fused_waves, bool line_groups, bool wide_two = false)
{
  return {true, kMarchGeo2, 0, false, val, false, false, val == 5 ? kMarchPack : kMarchArrays, true, 8, fused_waves,
          8, wide_two, line_groups};
}
constexpr MarchTraits two_line(int fused_waves, bool down_body, bool pipe_body)
{
  return {true, kMarchGeo2L2, 0, false, 0, false, false, kMarchPack, true, 5, fused_waves, 8, true, false,
          down_body, pipe_body};
}
constexpr MarchTraits kuhn(bool kp, bool lx, int fused_waves)
{
  return {true, kMarchKuhn, 0, false, 0, kp, lx, kp ? kMarchPack : kMarchArrays, true, 5, fused_waves, 8, true, false};
}
constexpr MarchTraits unused() { return {}; }
}  // namespace march_kind

constexpr int kMarchVariantEnd = 25;
constexpr MarchTraits kMarchTable[kMarchVariantEnd] = {
    /*  0 */ march_kind::masked(kMarchArrays, false, 7),   // band arrays and loaded row masks: any band
    /*  1 */ march_kind::masked(kMarchUniform, false, 8),  // uniform values, loaded row masks
    /*  2 */ march_kind::masked(kMarchUniform, true, 8),   // uniform values, masks from the coordinates
    /*  3 */ march_kind::geo(0, false, 7),                 // geometric, +D operand 1 plane ahead
    /*  4 */ march_kind::geo(1, false, 6),                 // ... 2 planes ahead
    /*  5 */ march_kind::geo(2, false, 5),                 // ... 3 planes ahead
    /*  6 */ march_kind::geo(2, true, 4),                  // ... 3 planes ahead, gathers 1 plane ahead
    /*  7 */ march_kind::geo2(0, false, 7, 8),             // geo2 with the prefetch of 3
    /*  8 */ march_kind::geo2(1, false, 6, 6),             // geo2 with the prefetch of 4
    /*  9 */ march_kind::geo2(2, true, 4, 6),              // geo2 with the prefetches of 6
    /* 10 */ march_kind::value(1, 6, true),                // value march: band arrays streamed on a geo2 grid
    /* 11 */ march_kind::value(2, 5, true),                // ... the value streams one plane ahead
    /* 12 */ march_kind::kuhn(false, false, 5),            // Kuhn box march on the band arrays
    /* 13 */ march_kind::unused(),
    /* 14 */ march_kind::value(4, 6, true),                // value march through global addresses
    /* 15 */ march_kind::value(5, 6, true, true),          // value march on the value pack
    /* 16 */ march_kind::kuhn(true, false, 4),             // Kuhn march on its value pack
    /* 17 */ march_kind::unused(),
    /* 18 */ march_kind::value(5, 7, false),               // 15 built for 7 waves per SIMD
    /* 19 */ march_kind::kuhn(true, false, 5),             // 16 built for 5 waves per SIMD
    /* 20 */ march_kind::kuhn(true, true, 4),              // Kuhn pack march with the line exchange in LDS
    /* 21 */ march_kind::unused(),
    /* 22 */ march_kind::two_line(5, true, true),          // value pack, two grid lines per wave
    /* 23 */ march_kind::two_line(4, true, true),          // 22 built for 4 waves per SIMD
    /* 24 */ march_kind::two_line(6, false, false),        // 22 built for 6 waves per SIMD: the upward plain body alone
};

constexpr MarchTraits march_traits(int variant)
{
  return variant >= 0 && variant < kMarchVariantEnd ? kMarchTable[variant] : MarchTraits{};
}

// The variants the launch dispatch instantiates, one kernel each with its traits' template head
// (variant 0 with all three heads).  The order is free: it only places the kernels in the code object
// (the compiler emits them last entry first), and this one keeps them where they have always been.
using MarchDispatch =
    std::integer_sequence<int, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 18, 24, 23, 22, 15, 14, 19, 20, 16, 12>;
template <int... V>
constexpr bool march_in(int variant, std::integer_sequence<int, V...>)
{
  return ((variant == V) || ...);
}
constexpr bool march_in_dispatch(int variant) { return march_in(variant, MarchDispatch{}); }
constexpr bool march_dispatch_complete()
{
  for (int v = 0; v < kMarchVariantEnd; ++v)
    if (march_traits(v).valid != march_in_dispatch(v)) return false;
  return true;
}
static_assert(march_dispatch_complete(), "MarchDispatch must list exactly the valid variants of kMarchTable");

// eig_mat_s::sym_box27 of the P1 Kuhn 15-point stencil: the box positions (a + 1) 9 + (b + 1) 3 + (c + 1) of
// {0, +-e_i, +-(e_i + e_j), +-(1, 1, 1)}
constexpr unsigned kKuhn15 = (1u << 0) | (1u << 1) | (1u << 3) | (1u << 4) | (1u << 9) | (1u << 10) | (1u << 12) |
                             (1u << 13) | (1u << 14) | (1u << 16) | (1u << 17) | (1u << 22) | (1u << 23) |
                             (1u << 25) | (1u << 26);

}  // namespace eigmi
