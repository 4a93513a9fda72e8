// K2 (gather GEMM with a SCATTERED EPILOGUE): the product of tnh_gemm_gather.hip -- a small matrix S[Ms, K] against a
// very long many-axis tensor that is read where it lies -- written straight into the axis order its CONSUMER wants,
//
//   C = any dense tensor whose axes are a permutation of [long operand's free axes..., small operand's free axes...]
//
// so that the stand-alone K1 permute between two products of a replayed contraction path (read + rewrite of a tensor a
// GEMM has just written) disappears.  Input side, MFMA sequence, persistent grid and the two boxes of register
// prefetch are those of gemm_gather_kernel: sums are grouped identically and the result is bit-identical to
// tnh_gemm_gather followed by tnh_permute.
//
// Addressing.  The destination offset of an element is a sum of index x stride over the axes, so it separates:
//
//   offset = tile_out_base(tile) + row_off[r] + col_off[c]          r < BN (row of the box), c < Ms (row of S)
//
// tile_out_base: 64-bit, from the tile digits and one output stride per digit (the twin of gather_tile_base);
// row_off: from the FREE digits of the box and one output multiplier per digit; col_off: from the small operand's
// free digits.  Every workgroup computes both tables once into LDS (64-bit entries, in the area that later holds the
// long image) and every thread adds up the offsets of ITS output chunks from them once, before the tile loop -- as the
// gather kernel does with esm / eoff -- so only the tile base changes per tile.  Nothing is 32-bit: the destination
// may have 2^31 elements and more.
//
// Epilogue.  The staging form follows the destination's INNERMOST axis (chosen on the host):
//   ROWS_LONG   it is a free axis of the small operand: stage [BN][Ms] (the gather kernel's "swap" form: a lane holds
//               four consecutive small indices of one long row), runs go along c;
//   otherwise   it is the innermost free digit of the box: stage [Ms][BN], runs go along r.
// A RUN is the longest piece that is contiguous both in a staging row and in the destination: the leading digits of
// that side while each starts where the one before ends (D = 12: 12 or 144 elements, D = 16: 16 or 256).  Threads store
// runs in chunks of V elements, V = 8 (16-byte stores: run % 8 == 0, C 16-byte aligned) or V = 4 (8-byte stores: a
// 24-byte run of D = 12); consecutive threads take consecutive chunks of a staging row, so a run is written by
// neighbouring lanes.  Every stride outside the run is a multiple of the run (the destination is dense), hence every
// chunk is V-aligned when C is.
// LDS banks, [Ms][BN] form: rows are 128 / 96 bytes + 16 of padding = 36 / 28 dwords.  The 8-byte fragment stores of a
// half wave (16 rows x 2 chunks) land on dwords 4 * row (mod 32) + 0..3: two-way at worst, which is the floor for 256
// bytes on 32 banks; without the padding all 16 rows would start on the same bank.  The chunk reads walk a row
// contiguously and step 144 / 112 bytes to the next.
//
// Roofline: HBM.  Algorithmic bytes 2 * (Nl * K + Ms * K + Ms * Nl) -- against + 4 * Ms * Nl for the K1 pass it replaces.
#include "tnh_gemm_gather.h"

namespace tnh {

// LDS as in gemm_gather_kernel: [ small image: msf*16 rows x PA ][ R: max(long image BN x PA, staging) ]; the two
// offset tables lie in R before the first long image is written.
// KIN: the innermost digit of the box is contracted.  ROWS_LONG / V: see the file header.
template <int BN, bool IS_BF16, bool ROWS_LONG, bool KIN, int V>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_gather_scatter_kernel(ScatterArgs q) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GatherArgs& p = q.a;
  constexpr int FN = BN / 16;
  constexpr int MAX_MI = 3;
  constexpr int NB = (BN * 48 + 255) / 256;         // 8-B chunks of the box per thread at K = 192
  constexpr int NST = (192 * BN / V + 255) / 256;   // output chunks of V elements per thread at Ms = 192
  constexpr int VB = V * 2;
  static_assert(BN == 48 || BN == 64, "tile rows");
  static_assert(V == 4 || V == 8, "8-byte or 16-byte stores");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = p.K, Ms = p.Ms;
  const int Kp = (K + 31) & ~31, cpr = Kp >> 3, kch = K >> 3, ksteps = Kp >> 5;
  const int PA = Kp * 2 + 16;
  const int msf = (Ms + 15) >> 4;
  const int msp = msf * 16;
  char* sS = smem;
  char* sR = smem + msp * PA;
  const int EP = (ROWS_LONG ? msp : BN) * 2 + 16;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);

  // ---- first of all (the output descriptor's registers are free again afterwards): the two offset tables -- R is
  //      unused until the first image -- and from them this thread's output chunks:
  //      (staging byte offset, element offset in the destination from the tile's base)
  int esm[NST];
  int64_t eoff[NST];
  {
    int64_t* t_row = (int64_t*)sR;             // [BN]  (the host checks that R holds 64 + 192 entries)
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
      esm[it] = row * EP + ch * VB;
      eoff[it] = ROWS_LONG ? t_row[row] + t_col[ch * V] : t_col[row] + t_row[ch * V];
    }
    __syncthreads();                           // tables consumed: R takes the first long image
  }

  // ---- small operand -> LDS, once (zero rows / zero k padding)
  for (int idx = tid; idx < msp * cpr; idx += 256) {
    const int row = idx / cpr, c = idx - row * cpr;
    uint4 v = zero4;
    if (row < Ms && c < kch) v = *(const uint4*)(p.S + (int64_t)row * p.lds + c * 8);
    *(uint4*)(sS + row * PA + c * 16) = v;
  }

  int loff[NB], lsm[NB];
  {
    int crow[NB], ccol[NB];
    gather_thread_chunks<NB>(p.g, tid, BN * (K >> 2), loff, crow, ccol);
#pragma unroll
    for (int it = 0; it < NB; ++it) lsm[it] = crow[it] * PA + ccol[it] * 2;
  }
  uint2 rl0[NB], rl1[NB];
  auto load_long = [&](int tile, uint2 (&rl)[NB]) {
    const uint16_t* base = p.L + gather_tile_base(p.g, tile);
#pragma unroll
    for (int it = 0; it < NB; ++it) rl[it] = *(const uint2*)(base + loff[it]);
  };
  const int padch = cpr - kch;
  auto store_long = [&](const uint2 (&rl)[NB]) {
#pragma unroll
    for (int it = 0; it < NB; ++it) {
      if constexpr (KIN) {
        *(uint2*)(sR + lsm[it]) = rl[it];
      } else {
        char* w = sR + lsm[it];
        *(uint16_t*)(w) = (uint16_t)(rl[it].x & 0xffffu);
        *(uint16_t*)(w + PA) = (uint16_t)(rl[it].x >> 16);
        *(uint16_t*)(w + 2 * PA) = (uint16_t)(rl[it].y & 0xffffu);
        *(uint16_t*)(w + 3 * PA) = (uint16_t)(rl[it].y >> 16);
      }
    }
    for (int idx = tid; idx < BN * padch; idx += 256) {
      const int row = idx / padch, c = idx - row * padch;
      *(uint4*)(sR + row * PA + (kch + c) * 16) = zero4;
    }
  };

  int tile = blockIdx.x;
  const int last = p.ntiles - 1;
  const int step = (int)gridDim.x;             // the host launches at most ntiles workgroups
  load_long(tile, rl0);

  const int frag_row = lane & 15, frag_chk = lane >> 4;

  // One tile, as gemm_gather_kernel's: `hold` has the NEXT tile's box, `fill` takes the one after it.
  auto body = [&](int t, uint2 (&hold)[NB], uint2 (&fill)[NB]) {
    __syncthreads();                            // long image (and, first time, the small image) complete
    {
      const int far = t + 2 * step;
      load_long(far <= last ? far : last, fill);
    }

    f32x4 acc[MAX_MI][FN];
#pragma unroll
    for (int i = 0; i < MAX_MI; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ks = 0; ks < ksteps; ++ks) {
      const int koff = (ks * 4 + frag_chk) * 16;
      uint4 lf[FN];
#pragma unroll
      for (int j = 0; j < FN; ++j) lf[j] = *(const uint4*)(sR + (j * 16 + frag_row) * PA + koff);
#pragma unroll
      for (int i = 0; i < MAX_MI; ++i) {
        const int mi = wid + 4 * i;
        if (mi < msf) {                         // wave-uniform
          const uint4 sf = *(const uint4*)(sS + (mi * 16 + frag_row) * PA + koff);
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
          if constexpr (ROWS_LONG) {   // row = long index (lane & 15), 4 consecutive small indices
            *(uint2*)(sR + (j * 16 + frag_row) * EP + (mi * 16 + frag_chk * 4) * 2) = o;
          } else {                     // row = small index (lane & 15), 4 consecutive long indices
            *(uint2*)(sR + (mi * 16 + frag_row) * EP + (j * 16 + frag_chk * 4) * 2) = o;
          }
        }
      }
    }
    __syncthreads();

    {
      uint16_t* cbase = p.C + scatter_tile_base(p.g, q.o, t);
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

// ---- host side
// What the destination descriptor must be for the kernel to stay inside C: a BIJECTION of (tile, box row, small row)
// onto [0, Ms * Nl).  The offset is a sum of index x stride over independent digits, and such a sum is a bijection
// onto an interval exactly when the digits, sorted by stride, form a dense mixed radix (stride 1, then the extent of
// the digit before, ...): no enumeration of elements.  Returns TNH_OK with the staging form and the vector width, or
// TNH_ERR_INVALID (not a bijection / malformed) / TNH_ERR_UNSUPPORTED (a destination the kernel does not store).
static int scatter_validate(const tnh_gather_desc& g, const tnh_scatter_desc& o, int64_t Ms, int64_t Nl, const void* C,
                            bool* rows_long, int* vec, const char** why) {
  struct Digit {
    int64_t ext, stride;
    int kind, d;         // kind 0: free digit of the box, 1: tile digit, 2: free digit of the small operand
  };
  Digit dg[TNH_GATHER_MAX_DIGITS + TNH_GATHER_MAX_TILE_DIGITS + TNH_SCATTER_MAX_SMALL_DIGITS];
  int n = 0;
  int64_t w_row = 1;
  for (int d = 0; d < g.nd; ++d) {
    if ((g.k_mask >> d) & 1) continue;
    if (g.mult[d] != w_row) { *why = "row weights of the box are not its free digits' mixed radix"; return TNH_ERR_UNSUPPORTED; }
    w_row *= g.ext[d];
    dg[n++] = Digit{g.ext[d], o.omult[d], 0, d};
  }
  for (int d = 0; d < g.nt; ++d) dg[n++] = Digit{g.text[d], o.otstride[d], 1, d};
  if (o.ns < 1 || o.ns > TNH_SCATTER_MAX_SMALL_DIGITS) { *why = "small operand's digit count"; return TNH_ERR_INVALID; }
  int64_t small_rows = 1;
  for (int d = 0; d < o.ns; ++d) {
    if (o.sext[d] < 1) { *why = "small operand's extents"; return TNH_ERR_INVALID; }
    small_rows *= o.sext[d];
    if (small_rows > Ms) break;
    dg[n++] = Digit{o.sext[d], o.sstride[d], 2, d};
  }
  if (small_rows != Ms) { *why = "small operand's extents do not multiply to Ms"; return TNH_ERR_INVALID; }
  int m = 0;
  for (int i = 0; i < n; ++i) {                 // extent-1 digits carry no offset
    if (dg[i].ext == 1) continue;
    if (dg[i].stride < 1) { *why = "non-positive output stride"; return TNH_ERR_INVALID; }
    dg[m++] = dg[i];
  }
  n = m;
  for (int i = 1; i < n; ++i) {                 // by stride (stable: the order above breaks ties, which then fail below)
    const Digit x = dg[i];
    int j = i;
    for (; j > 0 && dg[j - 1].stride > x.stride; --j) dg[j] = dg[j - 1];
    dg[j] = x;
  }
  int64_t expect = 1;
  for (int i = 0; i < n; ++i) {
    if (dg[i].stride != expect) { *why = "the destination is not a bijection onto [0, Ms * Nl)"; return TNH_ERR_INVALID; }
    expect *= dg[i].ext;
  }
  if (expect != Ms * Nl || o.c_elems < expect) { *why = "the destination does not have Ms * Nl elements"; return TNH_ERR_INVALID; }
  // the innermost destination axis decides the staging form; the run: its side's digits, in their own order, while
  // they stay the innermost of the destination
  if (n == 0 || dg[0].kind == 1) { *why = "the innermost destination axis is a long digit outside the box"; return TNH_ERR_UNSUPPORTED; }
  const int kind = dg[0].kind;
  int64_t run = 1;
  {
    int at = 0;                                  // position in the sorted list
    const int count = kind == 2 ? o.ns : g.nd;
    for (int d = 0; d < count; ++d) {
      if (kind == 0 && ((g.k_mask >> d) & 1)) continue;
      const int64_t ext = kind == 2 ? o.sext[d] : g.ext[d];
      if (ext == 1) continue;
      if (at < n && dg[at].kind == kind && dg[at].d == d) {
        run *= ext;
        ++at;
      } else {
        break;
      }
    }
    if (at == 0) { *why = "the innermost destination axis is not the innermost digit of its side"; return TNH_ERR_UNSUPPORTED; }
  }
  *rows_long = kind == 2;
  if (run % 8 == 0 && ((uintptr_t)C % 16) == 0) *vec = 8;
  else if (run % 4 == 0 && ((uintptr_t)C % 8) == 0) *vec = 4;
  else { *why = "run not a multiple of 4 elements / destination alignment"; return TNH_ERR_UNSUPPORTED; }
  return TNH_OK;
}

static bool scatter_enabled() {
  static const bool on = []() { const char* e = getenv("TNH_GATHER_SCATTER"); return !(e && e[0] == '0'); }();
  return on;
}

// TNH_GATHER_WIDE=0: the wide form of this entry is off together with the wide gather kernel
static bool scatter_wide_enabled() {
  static const bool on = []() { const char* e = getenv("TNH_GATHER_WIDE"); return !(e && e[0] == '0'); }();
  return on;
}

template <int BN, bool ROWS_LONG, bool KIN, int V>
static int launch_scatter(bool is_bf16, const ScatterArgs& q, size_t lds_bytes) {
  static const int attr_rc = []() -> int {
    for (const void* k : {reinterpret_cast<const void*>(gemm_gather_scatter_kernel<BN, true, ROWS_LONG, KIN, V>),
                          reinterpret_cast<const void*>(gemm_gather_scatter_kernel<BN, false, ROWS_LONG, KIN, V>)})
      if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return 1;
    return 0;
  }();
  if (attr_rc) {
    set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for the scatter gather GEMM");
    return TNH_ERR_HIP;
  }
  auto go = [&](auto kernel) -> int {
    int per_cu = 0;
    TNH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, lds_bytes));
    if (per_cu < 1) per_cu = 1;
    int64_t gx = (int64_t)num_cus() * per_cu;
    if (gx > q.a.ntiles) gx = q.a.ntiles;
    hipLaunchKernelGGL(kernel, dim3((unsigned)gx), dim3(256), lds_bytes, stream(), q);
    return TNH_OK;
  };
  const int rc = is_bf16 ? go(gemm_gather_scatter_kernel<BN, true, ROWS_LONG, KIN, V>)
                         : go(gemm_gather_scatter_kernel<BN, false, ROWS_LONG, KIN, V>);
  if (rc) return rc;
  TNH_LAUNCH_CHECK();
  return TNH_OK;
}

template <int BN, bool ROWS_LONG>
static int launch_scatter_form(bool kin, int vec, bool is_bf16, const ScatterArgs& q, size_t lds_bytes) {
  if (vec == 8) return kin ? launch_scatter<BN, ROWS_LONG, true, 8>(is_bf16, q, lds_bytes) : launch_scatter<BN, ROWS_LONG, false, 8>(is_bf16, q, lds_bytes);
  return kin ? launch_scatter<BN, ROWS_LONG, true, 4>(is_bf16, q, lds_bytes) : launch_scatter<BN, ROWS_LONG, false, 4>(is_bf16, q, lds_bytes);
}

// See include/tnh.h.  TNH_ERR_UNSUPPORTED (nothing launched) outside the kernel's range: the caller runs
// tnh_gemm_gather (or permute + tnh_gemm) and tnh_permute.  TNH_ERR_INVALID for a destination that is no bijection.
int gemm_gather_scatter(int dtype, int64_t Ms, int64_t K, int64_t Nl, const void* S, int64_t lds, const void* L,
                        int64_t l_elems, const tnh_gather_desc* desc, void* C, const tnh_scatter_desc* out,
                        const char** name) {
  const char* why = nullptr;
  int bn = 0;
  // Ms > 192 or K > 192: the wide kernel (tnh_gemm_gather_scatter_wide.hip), which addresses S in 64 bits
  const bool wide = Ms > 192 || K > 192;
  const bool range_ok = wide ? scatter_wide_enabled() && Ms <= 256 && K <= 256 : Ms * lds < (int64_t(1) << 30);
  const bool shape_ok = scatter_enabled() && desc->kl_ext == 1 && Ms >= 4 && range_ok && K >= 8 && K % 8 == 0 &&
                        Nl >= 48 && lds % 8 == 0 && lds >= K && ((uintptr_t)S % 16) == 0 && ((uintptr_t)L % 8) == 0;
  // (the descriptor check bounds the span of ONE box by 2^31 elements and its width by 256 indices, the wide kernel's
  //  bound: the tensor itself may be larger)
  if (shape_ok) bn = gather_validate_cached(*desc, K, Nl, l_elems, &why);
  if (!bn) {
    set_error("tnh_gemm_gather_scatter: outside the kernel's range (%s)",
              why ? why : "shape / alignment / K loop / TNH_GATHER_SCATTER=0");
    return TNH_ERR_UNSUPPORTED;
  }
  bool rows_long = false;
  int vec = 0;
  const int rc = scatter_validate(*desc, *out, Ms, Nl, C, &rows_long, &vec, &why);
  if (rc != TNH_OK) {
    set_error("tnh_gemm_gather_scatter: %s", why);
    return rc;
  }
  ScatterArgs q;
  q.a.g = *desc;
  q.a.S = (const uint16_t*)S;
  q.a.L = (const uint16_t*)L;
  q.a.C = (uint16_t*)C;
  q.a.lds = lds;
  q.a.ldc = 0;
  q.a.Ms = (int)Ms;
  q.a.K = (int)K;
  q.a.ntiles = (int)(Nl / bn);
  q.o = *out;
  if (wide) return launch_gather_scatter_wide(bn, rows_long, desc->k_mask & 1, vec, dtype == TNH_BF16, q, name);
  const int Kp = (int)((K + 31) & ~31), PA = Kp * 2 + 16;
  const int msp = (q.a.Ms + 15) / 16 * 16;
  const size_t image = (size_t)bn * PA;          // >= 48 * 80 bytes: room for the two offset tables (256 x 8 bytes)
  const size_t staging = rows_long ? (size_t)bn * (msp * 2 + 16) : (size_t)msp * (bn * 2 + 16);
  const size_t lds_bytes = (size_t)msp * PA + (image > staging ? image : staging);
  const bool kin = desc->k_mask & 1;
  const bool is_bf16 = dtype == TNH_BF16;
  if (bn == 48) {
    *name = rows_long ? (vec == 8 ? "bf16_gather_scatter_48xS_v16" : "bf16_gather_scatter_48xS_v8")
                      : (vec == 8 ? "bf16_gather_scatter_Sx48_v16" : "bf16_gather_scatter_Sx48_v8");
    return rows_long ? launch_scatter_form<48, true>(kin, vec, is_bf16, q, lds_bytes)
                     : launch_scatter_form<48, false>(kin, vec, is_bf16, q, lds_bytes);
  }
  *name = rows_long ? (vec == 8 ? "bf16_gather_scatter_64xS_v16" : "bf16_gather_scatter_64xS_v8")
                    : (vec == 8 ? "bf16_gather_scatter_Sx64_v16" : "bf16_gather_scatter_Sx64_v8");
  return rows_long ? launch_scatter_form<64, true>(kin, vec, is_bf16, q, lds_bytes)
                   : launch_scatter_form<64, false>(kin, vec, is_bf16, q, lds_bytes);
}

}  // namespace tnh
