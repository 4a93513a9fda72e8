// K2, gather GEMM for WIDE small operands: 192 < Ms <= 256 rows against ONE box of up to 256 contracted indices
// (bond D = 16: 256 x 16 777 216 x 256 against a rank-9 tensor).  Same product, descriptor and index arithmetic as
// tnh_gemm_gather.hip -- the long tensor is read where it lies, one box of BN = 48 / 64 free tuples per tile -- but the
// narrow kernel's layout does not stretch to these widths: its padded images need 172 KB of the CU's 160 KB, it runs
// two waves per SIMD on half the register file each, and its non-swapped epilogue offsets are 32-bit.  This one has:
//
//   * ONE workgroup of 256 threads per CU, one wave per SIMD with the whole register file: 4 small-operand fragments
//     x BN / 16 long fragments of accumulators (64 registers at BN = 64) next to two boxes of register prefetch
//     (2 x 16 chunks of 8 bytes).
//   * LDS rows of a FIXED 512-byte pitch and no padding:
//         [ small image: msp rows x 512 B (<= 128 KB) ][ R: BN rows x 512 B (<= 32 KB) ]       msp = Ms rounded up to 16
//     R holds the box image and, after the MFMA loop, the output staging: 160 KB exactly at Ms > 240 and BN = 64.
//   * A 512-byte pitch puts the 16 rows of a fragment on the same banks, so the 16-byte chunk c of row r lives at
//     chunk position c ^ (r & 15) of its row (`img` below).  The small-image fill, the box-image stores (8-byte and
//     2-byte form), the zero fill of the k padding and the fragment reads all go through it.  The staging area is
//     swizzled the same way where its pitch is a power of two (`stage`): BN rows x 512 B for C[Nl, Ms], msp rows x 128 B
//     for C[Ms, Nl] at BN = 64 (row pairs share the 64 banks: chunk ^ (row >> 1)); msp rows x 96 B at BN = 48 are
//     left plain, 96 B walks the banks by itself.
//   * Output addresses are a 64-bit row base plus a column offset: Ms x ldc may exceed 2^30 (D = 16 at full size:
//     256 x 16 777 216).
//
// What is kept from the narrow kernel so that results compare: mma16 over k in ascending steps of 32, pack2, the
// persistent grid, the next two boxes prefetched in registers, gather_thread_chunks / gather_tile_base.
//
// Roofline: HBM.  Algorithmic bytes 2 * (Nl * K + Ms * K + Ms * Nl).
#include "tnh_gemm_gather.h"

namespace tnh {

namespace {

constexpr int WIDE_PITCH = 512;                    // bytes per image row: 256 indices, no padding
constexpr size_t WIDE_LDS_MAX = 160 * 1024;        // LDS of a gfx950 CU

// byte offset of 16-byte chunk `c` of image row `row`
__device__ __forceinline__ int img(int row, int c) { return row * WIDE_PITCH + ((c ^ (row & 15)) << 4); }

// byte offset of 16-byte chunk `c` of staging row `row`.  SWAP: rows = long index, msp values each; else rows = small
// index, BN values each.
template <int BN, bool SWAP>
__device__ __forceinline__ int stage(int row, int c) {
  if constexpr (SWAP) return row * WIDE_PITCH + ((c ^ (row & 15)) << 4);
  else if constexpr (BN == 64) return row * 128 + ((c ^ ((row >> 1) & 7)) << 4);
  else return row * (BN * 2) + (c << 4);
}

// KIN: the innermost digit of the box is contracted (8-byte image stores); otherwise it is free (2-byte stores).
template <int BN, bool IS_BF16, bool SWAP, bool KIN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm_gather_wide_kernel(GatherArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int FN = BN / 16;                       // long-operand fragments per tile (every wave takes all of them)
  constexpr int MAX_MI = 4;                         // small-operand fragments per wave: 16 / 4
  constexpr int NB = BN / 4;                        // 8-B chunks of the box per thread at K = 256
  constexpr int NST = BN / 8;                       // 16-B output chunks per thread at Ms = 256
  static_assert(BN == 48 || BN == 64, "tile rows");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = p.K, Ms = p.Ms;
  const int Kp = (K + 31) & ~31, cpr = Kp >> 3, kch = K >> 3, ksteps = Kp >> 5;
  const int msf = (Ms + 15) >> 4;
  const int msp = msf * 16;
  char* sS = smem;
  char* sR = smem + msp * WIDE_PITCH;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);

  // ---- small operand -> LDS, once (zero rows / zero k padding)
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
        const int q = lsm[it];
        *(uint16_t*)(sR + q) = (uint16_t)(rl[it].x & 0xffffu);
        *(uint16_t*)(sR + ((q ^ 16) + WIDE_PITCH)) = (uint16_t)(rl[it].x >> 16);
        *(uint16_t*)(sR + ((q ^ 32) + 2 * WIDE_PITCH)) = (uint16_t)(rl[it].y & 0xffffu);
        *(uint16_t*)(sR + ((q ^ 48) + 3 * WIDE_PITCH)) = (uint16_t)(rl[it].y >> 16);
      }
    }
    // the staging area overwrote the padding columns: zero them again (LDS only -- no branch around a global access)
    for (int idx = tid; idx < BN * padch; idx += 256) {
      const int row = idx / padch, c = idx - row * padch;
      *(uint4*)(sR + img(row, kch + c)) = zero4;
    }
  };

  // ---- this thread's output chunks: staging byte offset, row and column (elements) in C from the tile origin
  int esm[NST], erow[NST], ecol[NST];
  {
    const int per_row = SWAP ? Ms >> 3 : BN / 8;
    const int total = (SWAP ? BN : Ms) * per_row;
#pragma unroll
    for (int it = 0; it < NST; ++it) {
      int idx = it * 256 + tid;
      if (idx >= total) idx = total - 1;
      const int row = idx / per_row, ch = idx - row * per_row;
      esm[it] = stage<BN, SWAP>(row, ch);
      erow[it] = row;
      ecol[it] = ch * 8;
    }
  }

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
            if constexpr (SWAP) acc[i][j] = mma16<IS_BF16>(sf, lf[j], acc[i][j]);
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
          if constexpr (SWAP) {   // row = long index (lane & 15), 4 consecutive small indices
            *(uint2*)(sR + stage<BN, SWAP>(j * 16 + frag_row, mi * 2 + (frag_chk >> 1)) + half) = o;
          } else {                // row = small index (lane & 15), 4 consecutive long indices
            *(uint2*)(sR + stage<BN, SWAP>(mi * 16 + frag_row, j * 2 + (frag_chk >> 1)) + half) = o;
          }
        }
      }
    }
    __syncthreads();

    {
      // SWAP: C rows = long index (tile origin n0 * ldc); else C rows = small index (tile origin n0)
      uint16_t* cbase = p.C + (SWAP ? (int64_t)tile * BN * p.ldc : (int64_t)tile * BN);
#pragma unroll
      for (int it = 0; it < NST; ++it) {
        const uint4 v = *(const uint4*)(sR + esm[it]);
        *(uint4*)(cbase + ((int64_t)erow[it] * p.ldc + ecol[it])) = v;
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

template <int BN, bool SWAP, bool KIN>
int launch_wide(bool is_bf16, const GatherArgs& p, size_t lds_bytes) {
  static const int attr_rc = []() -> int {
    for (const void* k : {reinterpret_cast<const void*>(gemm_gather_wide_kernel<BN, true, SWAP, KIN>),
                          reinterpret_cast<const void*>(gemm_gather_wide_kernel<BN, false, SWAP, KIN>)})
      if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)WIDE_LDS_MAX) != hipSuccess) return 1;
    return 0;
  }();
  if (attr_rc) {
    set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for the wide gather GEMM");
    return TNH_ERR_HIP;
  }
  // one workgroup per CU: the images take more than half of its LDS at every Ms of the range
  const int64_t gx = p.ntiles < num_cus() ? p.ntiles : num_cus();
  if (is_bf16)
    hipLaunchKernelGGL((gemm_gather_wide_kernel<BN, true, SWAP, KIN>), dim3((unsigned)gx), dim3(256), lds_bytes, stream(), p);
  else
    hipLaunchKernelGGL((gemm_gather_wide_kernel<BN, false, SWAP, KIN>), dim3((unsigned)gx), dim3(256), lds_bytes, stream(), p);
  TNH_LAUNCH_CHECK();
  return TNH_OK;
}

template <int BN>
int launch_wide_bn(bool swap, bool kin, bool is_bf16, const GatherArgs& p, size_t lds_bytes) {
  if (swap) return kin ? launch_wide<BN, true, true>(is_bf16, p, lds_bytes) : launch_wide<BN, true, false>(is_bf16, p, lds_bytes);
  return kin ? launch_wide<BN, false, true>(is_bf16, p, lds_bytes) : launch_wide<BN, false, false>(is_bf16, p, lds_bytes);
}

}  // namespace

int launch_gather_wide(int bn, bool swap, bool kin, bool is_bf16, const GatherArgs& p, const char** name) {
  const int msp = (p.Ms + 15) / 16 * 16;
  // image rows and, in R, whichever of the box image and the staging area is larger (`stage`)
  const size_t image = (size_t)bn * WIDE_PITCH;
  const size_t staging = swap ? (size_t)bn * WIDE_PITCH : (size_t)msp * (bn * 2);
  const size_t lds_bytes = (size_t)msp * WIDE_PITCH + (image > staging ? image : staging);
  if ((bn != 48 && bn != 64) || p.Ms <= 192 || p.K > 256 || p.K % 8 || msp * 2 > WIDE_PITCH || lds_bytes > WIDE_LDS_MAX) {
    set_error("tnh_gemm_gather: outside the wide gather kernel's range (Ms = %d, K = %d, %zu bytes of LDS)", p.Ms, p.K,
              lds_bytes);
    return TNH_ERR_UNSUPPORTED;
  }
  if (bn == 48) {
    *name = swap ? "bf16_gather_wide_48xS" : "bf16_gather_wide_Sx48";
    return launch_wide_bn<48>(swap, kin, is_bf16, p, lds_bytes);
  }
  *name = swap ? "bf16_gather_wide_64xS" : "bf16_gather_wide_Sx64";
  return launch_wide_bn<64>(swap, kin, is_bf16, p, lds_bytes);
}

}  // namespace tnh
