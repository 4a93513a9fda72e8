// Scattered epilogue of the 256 x 256 ping-pong view GEMM (tnh_gemm_view_scatter): the result tile goes straight into a
// dense destination whose axes are any permutation of [M-side free axes..., N-side free axes...], so that no K1 pass
// over the result runs before the next contraction.
//
// The destination offset of C[m][n] separates into rowoff(m) + coloff(n): m and n are mixed-radix numbers over the free
// axes of their operand and every digit carries its own 64-bit destination stride.  A wave owns 128 rows x 64 columns of
// the tile.  Per tile it fills a WAVE-PRIVATE table in LDS -- 128 row offsets and 16 column offsets (one per group of 4
// columns), 64-bit elements -- by magic-number division (2 - 3 offsets per lane instead of the 10 - 12 a lane needs),
// then stores along n: the innermost destination axis is the innermost digit of n, and a group of 4 (8-byte stores) or
// 8 (16-byte stores, the v_permlane16_swap pairing of store_wave_tile) consecutive n never crosses a run because the run
// is a multiple of the group and N a multiple of the run.  So a group is wholly inside or wholly outside the matrix:
// edge tiles need one predicate per group and no scalar path.
//
// The table is private to its wave and lives outside the staging buffers: the epilogue runs after the next tile's first
// LDS-DMA loads were issued and the ping-pong barriers are paired between the two wave groups, so this code adds no
// workgroup barrier.  LDS operations of one wave execute in order: the reads below see the writes above them.
#pragma once
#include "tnh_gemm_nt.h"
#include <type_traits>

namespace tnh {

constexpr int CVIEW_MAX_DIGITS = 6;

// One side (m or n) of the destination: digits innermost first.  The outermost digit takes what the divisions leave
// (`top`); the others are split off by q = (idx * mul) >> sh, exact for idx < 2^31 (mul = ceil(2^(31 + s) / ext),
// s = ceil(log2 ext), sh = 31 + s: Granlund & Montgomery, "Division by invariant integers using multiplication").
struct CViewSide {
  int ndiv;                                    // digits below the outermost one (0 .. 5)
  uint32_t ext[CVIEW_MAX_DIGITS - 1];
  uint32_t mul[CVIEW_MAX_DIGITS - 1];
  uint32_t sh[CVIEW_MAX_DIGITS - 1];
  int64_t stride[CVIEW_MAX_DIGITS - 1];        // destination elements per index
  int64_t top;                                 // destination elements per index of the outermost digit
};

struct NtScatArgs : NtArgs {
  CViewSide row, col;
};

constexpr int CVIEW_TAB = 128 + 16;            // 64-bit entries per wave: row offsets, then column-group offsets

__device__ __forceinline__ int64_t cview_offset(const CViewSide& s, uint32_t idx) {
  int64_t off = 0;
#pragma unroll
  for (int d = 0; d < CVIEW_MAX_DIGITS - 1; ++d) {
    if (d < s.ndiv) {                          // (wave-uniform)
      const uint32_t q = (uint32_t)(((uint64_t)idx * s.mul[d]) >> s.sh[d]);
      off += (int64_t)(idx - q * s.ext[d]) * s.stride[d];
      idx = q;
    }
  }
  return off + (int64_t)idx * s.top;
}

// Stores the wave's 128 x 64 part of a tile (FM = 8, FN = 4 fragments: a lane holds C[m = l & 15][n = 4 * (l >> 4) .. +3]
// of each 16 x 16 fragment).  V = 8: 16-byte stores of 8 consecutive n (non-temporal when c_vec == 3, as in
// store_wave_tile); V = 4: 8-byte stores of the lane's own 4.  Returns the number of store instructions the wave
// issued where that number is static (a full tile), 0 otherwise: the caller's early start of the next tile waits with
// vmcnt(that count).
template <bool IS_BF16, int V>
__device__ __forceinline__ int store_wave_tile_cview(const f32x4 (&acc)[8][4], const NtScatArgs& p, char* Cb, int64_t m0,
                                                     int64_t n0, int wave_m, int wave_n, int lane, int64_t* tab) {
  static_assert(V == 8 || V == 4, "16-byte or 8-byte stores");
  const int64_t mw = m0 + wave_m, nw = n0 + wave_n;      // < 2^31 + 256 (host check)
  tab[lane] = cview_offset(p.row, (uint32_t)(mw + lane));
  tab[64 + lane] = cview_offset(p.row, (uint32_t)(mw + 64 + lane));
  {
    const int64_t c = cview_offset(p.col, (uint32_t)(nw + 4 * (lane & 15)));
    if (lane < 16) tab[128 + lane] = c;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const bool full = (m0 + 256 <= p.M) && (n0 + 256 <= p.N);
  const int r = lane >> 4;
  constexpr int NG = V == 8 ? 2 : 4;                     // column groups per lane
  char* cb[NG];
  bool cin[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    // V = 8: after the swap of fragments (j, j + 1), j = 2g, lane row r holds columns (j + (r & 1)) * 16 + (r >> 1) * 8 .. +7
    const int nl = V == 8 ? (2 * g + (r & 1)) * 16 + (r >> 1) * 8 : g * 16 + 4 * r;
    cb[g] = Cb + tab[128 + (nl >> 2)] * 2;
    cin[g] = nw + nl < p.N;
  }
  auto rows = [&](auto fullc, auto ntc) {
    constexpr bool FULL = decltype(fullc)::value;
    auto put = [&](char* q, auto v, bool on) {
      if (!on) return;
      if constexpr (V == 8) {
        typedef unsigned v4u __attribute__((ext_vector_type(4)));
        // (non-temporal: see store_wave_tile -- the builtin compiles to a plain store with this toolchain, hence asm)
        if constexpr (decltype(ntc)::value) asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" : : "v"(q), "v"(v) : "memory");
        else *(v4u*)q = v;
      } else {
        *(uint2*)q = v;
      }
    };
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int ml = i * 16 + (lane & 15);
      const int64_t ro = tab[ml] * 2;
      const bool rin = FULL || mw + ml < p.M;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        if constexpr (V == 8) {
          typedef unsigned v4u __attribute__((ext_vector_type(4)));
          const f32x4 va = acc[i][2 * g], vb = acc[i][2 * g + 1];
          const auto sx = __builtin_amdgcn_permlane16_swap(pack2<IS_BF16>(va[0], va[1]), pack2<IS_BF16>(vb[0], vb[1]), false, false);
          const auto sy = __builtin_amdgcn_permlane16_swap(pack2<IS_BF16>(va[2], va[3]), pack2<IS_BF16>(vb[2], vb[3]), false, false);
          put(cb[g] + ro, v4u{sx[0], sy[0], sx[1], sy[1]}, FULL || (rin && cin[g]));
        } else {
          const f32x4 v = acc[i][g];
          uint2 o;
          o.x = pack2<IS_BF16>(v[0], v[1]);
          o.y = pack2<IS_BF16>(v[2], v[3]);
          put(cb[g] + ro, o, FULL || (rin && cin[g]));
        }
      }
    }
  };
  const bool nt = V == 8 && p.c_vec == 3;
  if (full) {
    if (nt) rows(std::true_type{}, std::true_type{});
    else rows(std::true_type{}, std::false_type{});
    return 8 * NG;
  }
  if (nt) rows(std::false_type{}, std::true_type{});
  else rows(std::false_type{}, std::false_type{});
  return 0;
}

}  // namespace tnh
