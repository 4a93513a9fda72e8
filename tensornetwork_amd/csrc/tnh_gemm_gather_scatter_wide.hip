// K2, the WIDE gather GEMM with a SCATTERED EPILOGUE: 192 < Ms <= 256 small-operand rows against ONE box of up to 256
// contracted indices of a long tensor read where it lies (bond D = 16: 256 x 16 777 216 x 256), written straight into
// the axis order its consumer wants -- the K1 pass over the 8.6 GB result of such a product disappears.
//
// Input side and MFMA loop are those of gemm_gather_wide_kernel (tnh_gemm_gather_wide.hip), so results compare bit for
// bit with it: one workgroup of 256 threads per CU, one wave per SIMD with the whole register file, unpadded 512-byte
// image rows whose 16-byte chunk c of row r lies at chunk position c ^ (r & 15) (`img`), four small-operand fragments
// per wave, two boxes of register prefetch, mma16 over k in ascending steps of 32, pack2, and the zero refill of the k
// padding after the staging overwrote it.
//
// Output side is that of gemm_gather_scatter_kernel (tnh_gemm_gather_scatter.hip):
//
//   offset = scatter_tile_base(tile) + row_off[r] + col_off[c]          r < BN (row of the box), c < Ms (row of S)
//
// 64-bit throughout.  LDS:
//     [ small image: msp rows x 512 B (<= 128 KB) ][ R: BN rows x 512 B (>= 24 KB) ]           msp = Ms rounded up to 16
// The two offset tables (64 + 256 entries of 8 bytes: 2.5 KB) are computed once per workgroup into R BEFORE the first
// box image is written there, so the 160 KB budget at Ms > 240, BN = 64 is untouched.  Every thread adds up the
// offsets of its own output chunks from them once, before the tile loop (`esm`, 64-bit `eoff`): BN / 8 chunks at
// 16-byte stores, BN / 4 at 8-byte stores -- up to 48 registers, affordable because this kernel owns the whole register
// file.  Only the 64-bit tile base changes per tile.
//
// Staging follows the destination's innermost axis:
//   ROWS_LONG   a free axis of the small operand: [BN][msp] at the 512-byte pitch, swizzled like the images (the wide
//               kernel's SWAP staging); runs go along the small operand's axes;
//   otherwise   the innermost free digit of the box: [msp][BN] in 128-byte rows swizzled with row >> 1 (BN = 64) or
//               plain 96-byte rows (BN = 48); runs go along the box rows.
// Stores are 16 bytes (V = 8: run % 8 == 0, C 16-byte aligned) or 8 bytes (V = 4); neighbouring lanes take
// neighbouring chunks of a staging row.  The swizzles move whole 16-byte chunks, so the two 8-byte halves of one stay
// adjacent and the V = 4 read of the staging needs no second swizzle.
//
// Roofline: HBM.  Algorithmic bytes 2 * (Nl * K + Ms * K + Ms * Nl) -- against + 4 * Ms * Nl for the K1 pass it replaces.
#include "tnh_gemm_gather.h"

namespace tnh {

namespace {

constexpr int WIDE_PITCH = 512;                    // bytes per image row: 256 indices, no padding
constexpr size_t WIDE_LDS_MAX = 160 * 1024;        // LDS of a gfx950 CU

// byte offset of 16-byte chunk `c` of image row `row`
__device__ __forceinline__ int img(int row, int c) { return row * WIDE_PITCH + ((c ^ (row & 15)) << 4); }

// byte offset of 16-byte chunk `c` of staging row `row`.  ROWS_LONG: rows = long index, msp values each; else rows =
// small index, BN values each.
template <int BN, bool ROWS_LONG>
__device__ __forceinline__ int stage(int row, int c) {
  if constexpr (ROWS_LONG) return row * WIDE_PITCH + ((c ^ (row & 15)) << 4);
  else if constexpr (BN == 64) return row * 128 + ((c ^ ((row >> 1) & 7)) << 4);
  else return row * (BN * 2) + (c << 4);
}

// KIN: the innermost digit of the box is contracted (8-byte image stores); otherwise it is free (2-byte stores).
// ROWS_LONG / V: see the file header.
template <int BN, bool IS_BF16, bool ROWS_LONG, bool KIN, int V>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm_gather_scatter_wide_kernel(ScatterArgs q) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GatherArgs& p = q.a;
  constexpr int FN = BN / 16;                       // long-operand fragments per tile (every wave takes all of them)
  constexpr int MAX_MI = 4;                         // small-operand fragments per wave: 16 / 4
  constexpr int NB = BN / 4;                        // 8-B chunks of the box per thread at K = 256
  constexpr int NST = BN / V;                       // output chunks of V elements per thread at Ms = 256
  static_assert(BN == 48 || BN == 64, "tile rows");
  static_assert(V == 4 || V == 8, "8-byte or 16-byte stores");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = p.K, Ms = p.Ms;
  const int Kp = (K + 31) & ~31, cpr = Kp >> 3, kch = K >> 3, ksteps = Kp >> 5;
  const int msf = (Ms + 15) >> 4;
  const int msp = msf * 16;
  char* sS = smem;
  char* sR = smem + msp * WIDE_PITCH;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);

  // ---- first of all (the output descriptor's registers are free again afterwards): the two offset tables -- R is
  //      unused until the first image -- and from them this thread's output chunks:
  //      (staging byte offset, element offset in the destination from the tile's base)
  int esm[NST];
  int64_t eoff[NST];
  {
    int64_t* t_row = (int64_t*)sR;             // [BN]  (R is at least 48 x 512 bytes: 64 + 256 entries fit)
    int64_t* t_col = t_row + 64;               // [Ms]
    if (tid < BN) t_row[tid] = scatter_row_offset(p.g, q.o, tid);
    if (tid < Ms) t_col[tid] = scatter_col_offset(q.o, tid);
    __syncthreads();
    const int per_row = (ROWS_LONG ? Ms : BN) / V;
    const int total = (ROWS_LONG ? BN : Ms) * per_row;
#pragma unroll
    for (int it = 0; it < NST; ++it) {
      int idx = it * 256 + tid;
      if (idx >= total) idx = total - 1;       // chunks past the end repeat the last one
      const int row = idx / per_row, ch = idx - row * per_row;
      // V = 4: chunk ch is half (ch & 1) of the 16-byte chunk ch >> 1
      esm[it] = V == 8 ? stage<BN, ROWS_LONG>(row, ch) : stage<BN, ROWS_LONG>(row, ch >> 1) + (ch & 1) * 8;
      eoff[it] = ROWS_LONG ? t_row[row] + t_col[ch * V] : t_col[row] + t_row[ch * V];
    }
    __syncthreads();                           // tables consumed: R takes the first long image
  }

  // ---- small operand -> LDS, once (zero rows / zero k padding); S is addressed in 64 bits
  for (int idx = tid; idx < msp * cpr; idx += 256) {
    const int row = idx / cpr, c = idx - row * cpr;
    uint4 v = zero4;
    if (row < Ms && c < kch) v = *(const uint4*)(p.S + (int64_t)row * p.lds + c * 8);
    *(uint4*)(sS + img(row, c)) = v;
  }

  // ---- this thread's chunks of a box: (offset in the box, image position) is the same for every tile
  int loff[NB], lsm[NB];
  {
    int crow[NB], ccol[NB];
    gather_thread_chunks<NB>(p.g, tid, BN * (K >> 2), loff, crow, ccol);
#pragma unroll
    for (int it = 0; it < NB; ++it) lsm[it] = img(crow[it], ccol[it] >> 3) + (ccol[it] & 7) * 2;
  }
  uint2 rl0[NB], rl1[NB];
  auto load_long = [&](int tile, uint2 (&rl)[NB]) {
    const uint16_t* base = p.L + gather_tile_base(p.g, tile);
#pragma unroll
    for (int it = 0; it < NB; ++it) rl[it] = *(const uint2*)(base + loff[it]);
  };
  const int padch = cpr - kch;                     // 16-B chunks of zero k-padding per image row (0 ... 3)
  auto store_long = [&](const uint2 (&rl)[NB]) {
#pragma unroll
    for (int it = 0; it < NB; ++it) {
      if constexpr (KIN) {
        *(uint2*)(sR + lsm[it]) = rl[it];
      } else {
        // rows r ... r + 3 with r % 4 == 0 (digit 0 is free, contiguous, a multiple of 4 long and the image is covered
        // exactly once: host-checked), so row r + i swizzles with (r & 15) | i: bits 4-5 of the offset flip with i
        const int w = lsm[it];
        *(uint16_t*)(sR + w) = (uint16_t)(rl[it].x & 0xffffu);
        *(uint16_t*)(sR + ((w ^ 16) + WIDE_PITCH)) = (uint16_t)(rl[it].x >> 16);
        *(uint16_t*)(sR + ((w ^ 32) + 2 * WIDE_PITCH)) = (uint16_t)(rl[it].y & 0xffffu);
        *(uint16_t*)(sR + ((w ^ 48) + 3 * WIDE_PITCH)) = (uint16_t)(rl[it].y >> 16);
      }
    }
    // the staging area overwrote the padding columns: zero them again (LDS only -- no branch around a global access)
    for (int idx = tid; idx < BN * padch; idx += 256) {
      const int row = idx / padch, c = idx - row * padch;
      *(uint4*)(sR + img(row, kch + c)) = zero4;
    }
  };

  const int frag_row = lane & 15, frag_chk = lane >> 4;
  const int last = p.ntiles - 1;
  const int step = (int)gridDim.x;             // the host launches at most ntiles workgroups

  // One tile: `hold` has the NEXT tile's box (requested one body earlier), `fill` takes the one after it.  The image
  // of the next tile is written at the END of the body, after this tile's stores were issued.
  auto body = [&](int tile, uint2 (&hold)[NB], uint2 (&fill)[NB]) {
    __syncthreads();                            // long image (and, first time, the small image) complete
    {
      const int far = tile + 2 * step;
      load_long(far <= last ? far : last, fill);   // in flight during this tile and the next
    }

    f32x4 acc[MAX_MI][FN];
#pragma unroll
    for (int i = 0; i < MAX_MI; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ks = 0; ks < ksteps; ++ks) {
      const int koff = ((ks * 4 + frag_chk) ^ frag_row) << 4;     // img(): every fragment row has row & 15 == frag_row
      uint4 lf[FN];
#pragma unroll
      for (int j = 0; j < FN; ++j) lf[j] = *(const uint4*)(sR + (j * 16 + frag_row) * WIDE_PITCH + koff);
#pragma unroll
      for (int i = 0; i < MAX_MI; ++i) {
        const int mi = wid + 4 * i;
        if (mi < msf) {                         // wave-uniform
          const uint4 sf = *(const uint4*)(sS + (mi * 16 + frag_row) * WIDE_PITCH + koff);
#pragma unroll
          for (int j = 0; j < FN; ++j) {
            // first argument: the index a lane holds 4 consecutive values of
            if constexpr (ROWS_LONG) acc[i][j] = mma16<IS_BF16>(sf, lf[j], acc[i][j]);
            else acc[i][j] = mma16<IS_BF16>(lf[j], sf, acc[i][j]);
          }
        }
      }
    }
    __syncthreads();                            // long image consumed: R becomes the staging area

#pragma unroll
    for (int i = 0; i < MAX_MI; ++i) {
      const int mi = wid + 4 * i;
      if (mi < msf) {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          uint2 o;
          o.x = pack2<IS_BF16>(acc[i][j][0], acc[i][j][1]);
          o.y = pack2<IS_BF16>(acc[i][j][2], acc[i][j][3]);
          const int half = (frag_chk & 1) * 8;  // 4 values = half a 16-byte chunk
          if constexpr (ROWS_LONG) {   // row = long index (lane & 15), 4 consecutive small indices
            *(uint2*)(sR + stage<BN, ROWS_LONG>(j * 16 + frag_row, mi * 2 + (frag_chk >> 1)) + half) = o;
          } else {                     // row = small index (lane & 15), 4 consecutive long indices
            *(uint2*)(sR + stage<BN, ROWS_LONG>(mi * 16 + frag_row, j * 2 + (frag_chk >> 1)) + half) = o;
          }
        }
      }
    }
    __syncthreads();

    {
      uint16_t* cbase = p.C + scatter_tile_base(p.g, q.o, tile);
#pragma unroll
      for (int it = 0; it < NST; ++it) {
        if constexpr (V == 8) {
          const uint4 v = *(const uint4*)(sR + esm[it]);
          *(uint4*)(cbase + eoff[it]) = v;
        } else {
          const uint2 v = *(const uint2*)(sR + esm[it]);
          *(uint2*)(cbase + eoff[it]) = v;
        }
      }
    }
    __syncthreads();                            // staging consumed: R takes the next long image
    store_long(hold);
  };

  int tile = blockIdx.x;
  load_long(tile, rl0);
  store_long(rl0);
  load_long(tile + step <= last ? tile + step : last, rl0);
  for (;;) {
    body(tile, rl0, rl1);
    tile += step;
    if (tile > last) break;
    body(tile, rl1, rl0);
    tile += step;
    if (tile > last) break;
  }
}

template <int BN, bool ROWS_LONG, bool KIN, int V>
int launch_scatter_wide(bool is_bf16, const ScatterArgs& q, size_t lds_bytes) {
  static const int attr_rc = []() -> int {
    for (const void* k : {reinterpret_cast<const void*>(gemm_gather_scatter_wide_kernel<BN, true, ROWS_LONG, KIN, V>),
                          reinterpret_cast<const void*>(gemm_gather_scatter_wide_kernel<BN, false, ROWS_LONG, KIN, V>)})
      if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)WIDE_LDS_MAX) != hipSuccess) return 1;
    return 0;
  }();
  if (attr_rc) {
    set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for the wide scatter gather GEMM");
    return TNH_ERR_HIP;
  }
  // one workgroup per CU: the images take more than half of its LDS at every Ms of the range
  const int64_t gx = q.a.ntiles < num_cus() ? q.a.ntiles : num_cus();
  if (is_bf16)
    hipLaunchKernelGGL((gemm_gather_scatter_wide_kernel<BN, true, ROWS_LONG, KIN, V>), dim3((unsigned)gx), dim3(256), lds_bytes,
                       stream(), q);
  else
    hipLaunchKernelGGL((gemm_gather_scatter_wide_kernel<BN, false, ROWS_LONG, KIN, V>), dim3((unsigned)gx), dim3(256), lds_bytes,
                       stream(), q);
  TNH_LAUNCH_CHECK();
  return TNH_OK;
}

template <int BN, bool ROWS_LONG>
int launch_scatter_wide_form(bool kin, int vec, bool is_bf16, const ScatterArgs& q, size_t lds_bytes) {
  if (vec == 8)
    return kin ? launch_scatter_wide<BN, ROWS_LONG, true, 8>(is_bf16, q, lds_bytes)
               : launch_scatter_wide<BN, ROWS_LONG, false, 8>(is_bf16, q, lds_bytes);
  return kin ? launch_scatter_wide<BN, ROWS_LONG, true, 4>(is_bf16, q, lds_bytes)
             : launch_scatter_wide<BN, ROWS_LONG, false, 4>(is_bf16, q, lds_bytes);
}

}  // namespace

int launch_gather_scatter_wide(int bn, bool rows_long, bool kin, int vec, bool is_bf16, const ScatterArgs& q,
                               const char** name) {
  const GatherArgs& p = q.a;
  const int msp = (p.Ms + 15) / 16 * 16;
  // image rows and, in R, whichever of the box image and the staging area is larger (`stage`); the offset tables
  // (64 + 256 entries of 8 bytes) lie in R before the first image
  const size_t image = (size_t)bn * WIDE_PITCH;
  const size_t staging = rows_long ? (size_t)bn * WIDE_PITCH : (size_t)msp * (bn * 2);
  const size_t r_bytes = image > staging ? image : staging;
  const size_t lds_bytes = (size_t)msp * WIDE_PITCH + r_bytes;
  if ((bn != 48 && bn != 64) || (vec != 4 && vec != 8) || p.Ms <= 192 || p.Ms > 256 || p.K < 8 || p.K > 256 || p.K % 8 ||
      p.g.kl_ext != 1 || (rows_long && p.Ms % vec) || r_bytes < (64 + 256) * sizeof(int64_t) || lds_bytes > WIDE_LDS_MAX) {
    set_error("tnh_gemm_gather_scatter: outside the wide scatter kernel's range (Ms = %d, K = %d, %zu bytes of LDS)", p.Ms,
              p.K, lds_bytes);
    return TNH_ERR_UNSUPPORTED;
  }
  if (bn == 48) {
    *name = rows_long ? (vec == 8 ? "bf16_gather_scatter_wide_48xS_v16" : "bf16_gather_scatter_wide_48xS_v8")
                      : (vec == 8 ? "bf16_gather_scatter_wide_Sx48_v16" : "bf16_gather_scatter_wide_Sx48_v8");
    return rows_long ? launch_scatter_wide_form<48, true>(kin, vec, is_bf16, q, lds_bytes)
                     : launch_scatter_wide_form<48, false>(kin, vec, is_bf16, q, lds_bytes);
  }
  *name = rows_long ? (vec == 8 ? "bf16_gather_scatter_wide_64xS_v16" : "bf16_gather_scatter_wide_64xS_v8")
                    : (vec == 8 ? "bf16_gather_scatter_wide_Sx64_v16" : "bf16_gather_scatter_wide_Sx64_v8");
  return rows_long ? launch_scatter_wide_form<64, true>(kin, vec, is_bf16, q, lds_bytes)
                   : launch_scatter_wide_form<64, false>(kin, vec, is_bf16, q, lds_bytes);
}

}  // namespace tnh
