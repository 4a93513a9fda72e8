// Pieces shared by the gather GEMM kernels (tnh_gemm_gather.hip: small operands of up to 192 rows;
// tnh_gemm_gather_wide.hip: 193 ... 256 rows; tnh_gemm_gather_scatter.hip / tnh_gemm_gather_scatter_wide.hip: the same
// two ranges with the result written in the consumer's axis order): the descriptor arithmetic and the argument blocks.
#pragma once
#include "tnh_gemm_nt.h"

namespace tnh {

// ---- descriptor arithmetic shared by the kernels, the host-side validation and tnh_gemm_gather_plan
// Chunk e of a box (8 bytes: four elements of the innermost digit), e counted in memory order: e written in the
// mixed radix of the box digits gives the digit indices, hence the element offset in the box and the image position.
// A thread owns chunks tid, tid + 256, tid + 512, ...: tid is decoded with one division per digit, the step of
// 256 is added digit by digit with carries afterwards (the divisions of a direct decode of every chunk were ~10 us
// of prologue per launch: profiles/r04_gather_gemm.md).  Chunks past the end of the box repeat the last one.
template <int NB>
__host__ __device__ __forceinline__ void gather_thread_chunks(const tnh_gather_desc& g, int tid, int total,
                                                              int (&off)[NB], int (&row)[NB], int (&kcol)[NB]) {
  unsigned radix[TNH_GATHER_MAX_DIGITS], digit[TNH_GATHER_MAX_DIGITS], step[TNH_GATHER_MAX_DIGITS];
  {
    unsigned e = (unsigned)tid, inc = 256u;
#pragma unroll
    for (int d = 0; d < TNH_GATHER_MAX_DIGITS; ++d) {
      // digits the box does not have count modulo 1 (always 0, carries fall through); the top digit is unbounded
      radix[d] = 1u;
      digit[d] = 0u;
      step[d] = 0u;
      if (d < g.nd) {
        const unsigned ext = d == 0 ? (unsigned)g.ext[0] >> 2 : (unsigned)g.ext[d];
        radix[d] = ext;
        const unsigned qe = e / ext, qi = inc / ext;
        digit[d] = e - qe * ext;
        step[d] = inc - qi * ext;
        e = qe;
        inc = qi;
      }
    }
  }
  int last_off = 0, last_row = 0, last_k = 0;     // chunk total - 1: every digit at its maximum
#pragma unroll
  for (int d = 0; d < TNH_GATHER_MAX_DIGITS; ++d) {
    if (d < g.nd) {
      const int top = d == 0 ? g.ext[0] - 4 : g.ext[d] - 1;
      last_off += top * g.stride[d];
      if ((g.k_mask >> d) & 1) last_k += top * g.mult[d];
      else last_row += top * g.mult[d];
    }
  }
#pragma unroll
  for (int it = 0; it < NB; ++it) {
    if (it * 256 + tid >= total) {
      off[it] = last_off;
      row[it] = last_row;
      kcol[it] = last_k;
    } else {
      int o = 0, r = 0, k = 0;
#pragma unroll
      for (int d = 0; d < TNH_GATHER_MAX_DIGITS; ++d) {
        if (d < g.nd) {
          const int idx = d == 0 ? (int)(digit[0] << 2) : (int)digit[d];
          o += idx * g.stride[d];
          if ((g.k_mask >> d) & 1) k += idx * g.mult[d];
          else r += idx * g.mult[d];
        }
      }
      off[it] = o;
      row[it] = r;
      kcol[it] = k;
    }
    unsigned carry = 0;                            // next chunk of this thread: + 256 in the mixed radix
#pragma unroll
    for (int d = 0; d < TNH_GATHER_MAX_DIGITS; ++d) {
      unsigned v = digit[d] + step[d] + carry;
      carry = v >= radix[d] ? 1u : 0u;
      if (carry) v -= radix[d];
      digit[d] = v;
    }
  }
}

__host__ __device__ __forceinline__ int64_t gather_tile_base(const tnh_gather_desc& g, int tile) {
  int64_t base = 0;
  unsigned t = (unsigned)tile;
#pragma unroll
  for (int d = 0; d < TNH_GATHER_MAX_TILE_DIGITS; ++d) {
    if (d < g.nt) {
      const unsigned ext = (unsigned)g.text[d];
      const unsigned q = t / ext;
      base += (int64_t)(t - q * ext) * g.tstride[d];
      t = q;
    }
  }
  return base;
}

struct GatherArgs {
  tnh_gather_desc g;
  const uint16_t* S;   // small operand, [Ms][K] rows lds apart
  const uint16_t* L;   // the long tensor as it lies
  uint16_t* C;
  int64_t lds, ldc;
  int Ms, K;
  int ntiles;
};

// ---- the scattered epilogue (tnh_gemm_gather_scatter.hip, tnh_gemm_gather_scatter_wide.hip)
struct ScatterArgs {
  GatherArgs a;          // (a.C: the destination's first element; a.ldc unused)
  tnh_scatter_desc o;
};

// ---- destination arithmetic shared by the kernel and the host-side validation
// Row r of a box in the mixed radix of its FREE digits (innermost first: the weights `mult` of the descriptor).
__host__ __device__ __forceinline__ int64_t scatter_row_offset(const tnh_gather_desc& g, const tnh_scatter_desc& o, int r) {
  int64_t off = 0;
  unsigned rem = (unsigned)r;
#pragma unroll
  for (int d = 0; d < TNH_GATHER_MAX_DIGITS; ++d) {
    if (d < g.nd && !((g.k_mask >> d) & 1)) {
      const unsigned ext = (unsigned)g.ext[d];
      const unsigned q = rem / ext;
      off += (int64_t)(rem - q * ext) * o.omult[d];
      rem = q;
    }
  }
  return off;
}

// Row c of the small operand in the mixed radix of its free digits (innermost first).
__host__ __device__ __forceinline__ int64_t scatter_col_offset(const tnh_scatter_desc& o, int c) {
  int64_t off = 0;
  unsigned rem = (unsigned)c;
#pragma unroll
  for (int d = 0; d < TNH_SCATTER_MAX_SMALL_DIGITS; ++d) {
    if (d < o.ns) {
      const unsigned ext = (unsigned)o.sext[d];
      const unsigned q = rem / ext;
      off += (int64_t)(rem - q * ext) * o.sstride[d];
      rem = q;
    }
  }
  return off;
}

__host__ __device__ __forceinline__ int64_t scatter_tile_base(const tnh_gather_desc& g, const tnh_scatter_desc& o, int tile) {
  int64_t base = 0;
  unsigned t = (unsigned)tile;
#pragma unroll
  for (int d = 0; d < TNH_GATHER_MAX_TILE_DIGITS; ++d) {
    if (d < g.nt) {
      const unsigned ext = (unsigned)g.text[d];
      const unsigned q = t / ext;
      base += (int64_t)(t - q * ext) * o.otstride[d];
      t = q;
    }
  }
  return base;
}

// provided by tnh_gemm_gather.hip: everything the kernels rely on in a descriptor, checked on the host (the last few
// accepted ones are remembered).  Returns the tile height BN (48 / 64), or 0 with the reason in *why.
int gather_validate_cached(const tnh_gather_desc& g, int64_t K, int64_t Nl, int64_t l_elems, const char** why);

// provided by tnh_gemm_gather_wide.hip: 192 < Ms <= 256, one box of BN x K (K <= 256), descriptor already validated.
// TNH_ERR_UNSUPPORTED, nothing launched, when the images do not fit the 160 KB of a CU.
int launch_gather_wide(int bn, bool swap, bool kin, bool is_bf16, const GatherArgs& p, const char** name);

// provided by tnh_gemm_gather_scatter_wide.hip: the same range with the scattered epilogue; descriptor and destination
// already validated (`rows_long` / `vec`: staging form and elements per store, from scatter_validate).
// TNH_ERR_UNSUPPORTED, nothing launched, outside the range or when the images do not fit the 160 KB of a CU.
int launch_gather_scatter_wide(int bn, bool rows_long, bool kin, int vec, bool is_bf16, const ScatterArgs& q,
                               const char** name);

}  // namespace tnh
