// K2 (complex part): strided-batched complex64 / complex128 GEMM on the matrix cores.
//
// Operands and result are interleaved (re, im) as NumPy stores them; A(m,k) = A[m*rsA + k*csA] and
// B(k,n) = B[k*rsB + n*csB] in complex elements, so the four transpose combinations are read in place.  One
// kernel template, gemm_mfma_cplx_kernel<R, BM, BN, BK, KC_A, KC_B>:
//
//   global -> registers   16-byte loads along each operand's contiguous direction (two complex64 or one complex128),
//                         issued one K-tile ahead of the MFMAs that consume them (as the f32 / f64 v2 kernels do).
//                         complex64 operands whose base, pitch or batch stride is odd (not 16-byte aligned) take
//                         8-byte loads in the same kernel (`a16` / `b16`, chosen per operand on the host).
//                         Rows beyond M / N are clamped (their products land in outputs that are never stored),
//                         k beyond K is zero.
//   registers -> LDS      de-interleaved into PLANAR images: one re plane and one im plane per operand and stage, two
//                         stages, one barrier per K-tile.  K-contiguous operands as [row][k] (pitch BK + 4 reals for
//                         f32, BK + 2 for f64), row-contiguous ones as [k][row] (pitch rows + 16).  With 64 banks of
//                         4 bytes a 16-row x 4-k fragment read of f32 touches 64 distinct banks in either image
//                         (row pitch 20: multiples of 4, all distinct mod 64; k pitch = 16 mod 64), and each 32-lane
//                         half of an f64 read (16 rows x 2 k) touches 32 distinct bank pairs (row pitch 10 doubles;
//                         k pitch = 16 mod 32).  Every B value is in LDS once.
//   LDS -> MFMA           per 16 x 16 x 4 block four v_mfma_{f32,f64}_16x16x4 into two accumulator sets:
//                           Cre += Ar Br,  Cre += (-Ai) Bi,  Cim += Ar Bi,  Cim += Ai Br
//                         with -Ai made once per A fragment (one sign flip in a register).  The four-multiply form:
//                         the error bound is that of a plain dot product of length 2K.
//   epilogue              (re, im) re-interleaved in registers, alpha / beta applied as the VALU kernel's scale_t does,
//                         one 8-byte (complex64) or 16-byte (complex128) store per element; C is read when beta != 0.
//
// Instantiations (4 waves as 2 x 2; per-wave accumulators = 2 sets x fragments x 4 (f32) or 8 (f64) registers), with
// .vgpr_count (unified, accumulation registers included) / .agpr_count / LDS bytes of the gfx950 code object, the
// largest over the four layouts:
//   mfma_c64_128x128x16    wave 64 x 64, 2 x 16 fragments = 128 acc registers     276 / 128 / 81920
//   mfma_c64_64x64x16      wave 32 x 32, 2 x  4 fragments =  32 acc registers      96 /  32 / 40960
//   mfma_c128_128x64x8     wave 64 x 32, 2 x  8 fragments = 128 acc registers     352 / 128 / 61440
//   mfma_c128_64x64x8      wave 32 x 32, 2 x  4 fragments =  64 acc registers     188 /  64 / 40960
// No instantiation spills (.vgpr_spill_count 0, no scratch).
//
// LDS budget: 2 stages x 2 planes x (A image + B image) reals, an image being max over the two orientations of
// rows x (BK + pad) and BK x (rows + 16).  Largest: complex64 128 x 128 x 16 = 2 x 2 x (2560 + 2560) x 4 = 81920
// bytes; complex128 128 x 64 x 8 = 2 x 2 x (1280 + 640) x 8 = 61440 bytes -- static_assert'ed against the 160 KiB
// of a gfx950 CU below.
#include <type_traits>
#include "tnh_types.h"

namespace tnh {

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f64x4 mma4(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// VEC complex elements (one 16-byte load) from p, of which the first `valid` exist; the rest are zero.
// complex64: one 16-byte load when both exist and the operand is 16-byte aligned, 8-byte loads otherwise.
__device__ __forceinline__ void load_vec(float (&v)[4], const float* p, int64_t valid, bool v16) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (valid >= 2) {
    if (v16) {
      const f32x4 q = *(const f32x4*)p;
      v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
      const f32x2 q0 = *(const f32x2*)p, q1 = *(const f32x2*)(p + 2);
      v[0] = q0[0]; v[1] = q0[1]; v[2] = q1[0]; v[3] = q1[1];
    }
  } else if (valid == 1) {
    const f32x2 q = *(const f32x2*)p;
    v[0] = q[0]; v[1] = q[1];
  }
}
__device__ __forceinline__ void load_vec(double (&v)[2], const double* p, int64_t valid, bool) {
  v[0] = v[1] = 0.0;
  if (valid >= 1) {
    const f64x2 q = *(const f64x2*)p;
    v[0] = q[0]; v[1] = q[1];
  }
}

template <typename R, int BM, int BN, int BK, bool KC_A, bool KC_B>
__global__ __launch_bounds__(256) void gemm_mfma_cplx_kernel(GemmArgs g, int a16, int b16) {
  constexpr bool F32 = std::is_same<R, float>::value;
  constexpr int VEC = F32 ? 2 : 1;                  // complex elements per 16-byte load
  constexpr int LDK = BK + (F32 ? 4 : 2);           // [row][k] pitch
  constexpr int LDA = BM + 16, LDB = BN + 16;       // [k][row] pitches
  constexpr int IMG_A = (BM * LDK > BK * LDA) ? BM * LDK : BK * LDA;
  constexpr int IMG_B = (BN * LDK > BK * LDB) ? BN * LDK : BK * LDB;
  static_assert(2 * 2 * (IMG_A + IMG_B) * sizeof(R) <= 160 * 1024, "LDS images exceed the 160 KiB of a gfx950 CU");
  static_assert((BM * BK / VEC) % 256 == 0 && (BN * BK / VEC) % 256 == 0 && BK % 4 == 0, "tile / thread mapping");
  constexpr int WM = BM / 2, WN = BN / 2, FI = WM / 16, FJ = WN / 16;
  typedef R acc_t __attribute__((ext_vector_type(4)));
  typedef R pair_t __attribute__((ext_vector_type(2)));

  __shared__ __attribute__((aligned(16))) R As[2][2][IMG_A];   // [stage][re | im]
  __shared__ __attribute__((aligned(16))) R Bs[2][2][IMG_B];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int64_t m0 = (int64_t)blockIdx.y * BM, n0 = (int64_t)blockIdx.x * BN;
  const R* A = (const R*)g.A + 2 * (int64_t)blockIdx.z * g.sA;
  const R* B = (const R*)g.B + 2 * (int64_t)blockIdx.z * g.sB;
  R* C = (R*)g.C + 2 * (int64_t)blockIdx.z * g.sC;
  const int64_t lda = KC_A ? g.rsA : g.csA, ldb = KC_B ? g.csB : g.rsB;

  constexpr int NVA = BM * BK / VEC / 256, NVB = BN * BK / VEC / 256;
  R ra[NVA][2 * VEC], rb[NVB][2 * VEC];

  // one operand tile = ROWS x BK complex = NV 16-byte vectors per thread, consecutive threads along the contiguous
  // direction
  auto load_op = [&](auto kc, auto rows_c, auto& r, const R* P, int64_t ld, int64_t row0, int64_t rows, int64_t k0,
                     bool v16) {
    constexpr bool KC = decltype(kc)::value;
    constexpr int ROWS = decltype(rows_c)::value;
    constexpr int NV = ROWS * BK / VEC / 256;
    constexpr int VPR = BK / VEC, VPK = ROWS / VEC;     // vectors per row (K-contiguous) / per k (row-contiguous)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if constexpr (KC) {
        int64_t row = row0 + tid / VPR + (256 / VPR) * j;
        if (row >= rows) row = rows - 1;
        const int64_t k = k0 + VEC * (tid % VPR);
        load_vec(r[j], P + 2 * (row * ld + k), g.K - k, v16);
      } else {
        const int64_t k = k0 + tid / VPK + (256 / VPK) * j;
        const int64_t row = row0 + VEC * (tid % VPK);
        load_vec(r[j], P + 2 * (k * ld + row), k < g.K ? rows - row : 0, v16);
      }
    }
  };
  // de-interleave: re of the vector's elements to the re plane, im to the im plane
  auto store_op = [&](auto kc, auto rows_c, const auto& r, R* Sre, R* Sim) {
    constexpr bool KC = decltype(kc)::value;
    constexpr int ROWS = decltype(rows_c)::value;
    constexpr int NV = ROWS * BK / VEC / 256;
    constexpr int VPR = BK / VEC, VPK = ROWS / VEC, LD = ROWS + 16;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      int idx;
      if constexpr (KC) idx = (tid / VPR + (256 / VPR) * j) * LDK + VEC * (tid % VPR);
      else idx = (tid / VPK + (256 / VPK) * j) * LD + VEC * (tid % VPK);
      if constexpr (F32) {
        *(pair_t*)(Sre + idx) = pair_t{r[j][0], r[j][2]};
        *(pair_t*)(Sim + idx) = pair_t{r[j][1], r[j][3]};
      } else {
        Sre[idx] = r[j][0];
        Sim[idx] = r[j][1];
      }
    }
  };
  using KA = std::integral_constant<bool, KC_A>;
  using KB = std::integral_constant<bool, KC_B>;
  using RA = std::integral_constant<int, BM>;
  using RB = std::integral_constant<int, BN>;

  acc_t cre[FI][FJ], cim[FI][FJ];
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int j = 0; j < FJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) cre[i][j][r] = cim[i][j][r] = (R)0;

  const int64_t nt = (g.K + BK - 1) / BK;
  load_op(KA{}, RA{}, ra, A, lda, m0, g.M, 0, a16 != 0);
  load_op(KB{}, RB{}, rb, B, ldb, n0, g.N, 0, b16 != 0);
  store_op(KA{}, RA{}, ra, As[0][0], As[0][1]);
  store_op(KB{}, RB{}, rb, Bs[0][0], Bs[0][1]);
  __syncthreads();
  // fragment element of this lane: row (lane & 15) of the fragment, k = lane >> 4 of the 4-deep step
  const int kl = lane >> 4, il = lane & 15;
  const int fa = KC_A ? (wm * WM + il) * LDK + kl : kl * LDA + wm * WM + il;
  const int fb = KC_B ? (wn * WN + il) * LDK + kl : kl * LDB + wn * WN + il;
  constexpr int ROW_A = KC_A ? 16 * LDK : 16, STEP_A = KC_A ? 1 : LDA;   // next fragment / next k in the image
  constexpr int ROW_B = KC_B ? 16 * LDK : 16, STEP_B = KC_B ? 1 : LDB;
  for (int64_t t = 0; t < nt; ++t) {
    const int cur = (int)(t & 1);
    if (t + 1 < nt) {
      load_op(KA{}, RA{}, ra, A, lda, m0, g.M, (t + 1) * BK, a16 != 0);
      load_op(KB{}, RB{}, rb, B, ldb, n0, g.N, (t + 1) * BK, b16 != 0);
    }
    const R *are = As[cur][0] + fa, *aim = As[cur][1] + fa, *bre = Bs[cur][0] + fb, *bim = Bs[cur][1] + fb;
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      R ar[FI], ai[FI], an[FI], br[FJ], bi[FJ];
#pragma unroll
      for (int i = 0; i < FI; ++i) {
        ar[i] = are[i * ROW_A + kk * STEP_A];
        ai[i] = aim[i * ROW_A + kk * STEP_A];
        an[i] = -ai[i];
      }
#pragma unroll
      for (int j = 0; j < FJ; ++j) {
        br[j] = bre[j * ROW_B + kk * STEP_B];
        bi[j] = bim[j * ROW_B + kk * STEP_B];
      }
#pragma unroll
      for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) {
          cre[i][j] = mma4(ar[i], br[j], cre[i][j]);
          cim[i][j] = mma4(ar[i], bi[j], cim[i][j]);
        }
#pragma unroll
      for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) {
          cre[i][j] = mma4(an[i], bi[j], cre[i][j]);
          cim[i][j] = mma4(ai[i], br[j], cim[i][j]);
        }
    }
    if (t + 1 < nt) {
      store_op(KA{}, RA{}, ra, As[cur ^ 1][0], As[cur ^ 1][1]);
      store_op(KB{}, RB{}, rb, Bs[cur ^ 1][0], Bs[cur ^ 1][1]);
    }
    __syncthreads();
  }

  // C / D layout: column = lane & 15; row = 4 * (lane >> 4) + r for f32, (lane >> 4) + 4 * r for f64
  const R alpha = (R)g.alpha, beta = (R)g.beta;
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int j = 0; j < FJ; ++j) {
      const int64_t n = n0 + wn * WN + j * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + wm * WM + i * 16 + (F32 ? 4 * (lane >> 4) + r : (lane >> 4) + 4 * r);
        if (m < g.M && n < g.N) {
          pair_t* c = (pair_t*)(C + 2 * (m * g.ldc + n));
          pair_t v = {cre[i][j][r] * alpha, cim[i][j][r] * alpha};
          if (g.beta != 0.0) {
            const pair_t old = *c;
            v[0] += old[0] * beta;
            v[1] += old[1] * beta;
          }
          *c = v;
        }
      }
    }
}

template <typename R, int BM, int BN, int BK>
void launch_layouts(const GemmArgs& g, dim3 grid, bool kc_a, bool kc_b, int a16, int b16) {
  if (kc_a && kc_b)
    hipLaunchKernelGGL((gemm_mfma_cplx_kernel<R, BM, BN, BK, true, true>), grid, dim3(256), 0, stream(), g, a16, b16);
  else if (kc_a)
    hipLaunchKernelGGL((gemm_mfma_cplx_kernel<R, BM, BN, BK, true, false>), grid, dim3(256), 0, stream(), g, a16, b16);
  else if (kc_b)
    hipLaunchKernelGGL((gemm_mfma_cplx_kernel<R, BM, BN, BK, false, true>), grid, dim3(256), 0, stream(), g, a16, b16);
  else
    hipLaunchKernelGGL((gemm_mfma_cplx_kernel<R, BM, BN, BK, false, false>), grid, dim3(256), 0, stream(), g, a16, b16);
}

}  // namespace

int gemm_complex_tile(int dtype, int64_t M, int64_t N, int64_t batch, int force, int* BM, int* BN, const char** name) {
  const bool c64 = (dtype == TNH_C64);
  const int lm = 128, ln = c64 ? 128 : 64;
  // the small tile: a side that one small tile covers, or too few large tiles to give every CU one
  bool large = !(M <= 64 || N <= 64 || ((M + lm - 1) / lm) * ((N + ln - 1) / ln) * batch < (int64_t)num_cus());
  if (force == 0) large = false;
  if (force == 1) large = true;
  *BM = large ? lm : 64;
  *BN = large ? ln : 64;
  *name = c64 ? (large ? "mfma_c64_128x128x16" : "mfma_c64_64x64x16")
              : (large ? "mfma_c128_128x64x8" : "mfma_c128_64x64x8");
  return large ? 1 : 0;
}

int gemm_complex_launch(int dtype, int large, const GemmArgs& g, dim3 grid) {
  TNH_REQUIRE(dtype == TNH_C64 || dtype == TNH_C128, "complex GEMM: dtype %d is not complex", dtype);
  const bool kc_a = (g.csA == 1), kc_b = (g.rsB == 1);
  TNH_REQUIRE((kc_a || g.rsA == 1) && (kc_b || g.csB == 1), "complex GEMM: an operand has no contiguous direction");
  if (dtype == TNH_C64) {
    // 16-byte loads of complex64 pairs: even pitch and batch stride, 16-byte aligned base
    const int64_t lda = kc_a ? g.rsA : g.csA, ldb = kc_b ? g.csB : g.rsB;
    const int a16 = ((uintptr_t)g.A % 16 == 0 && lda % 2 == 0 && g.sA % 2 == 0) ? 1 : 0;
    const int b16 = ((uintptr_t)g.B % 16 == 0 && ldb % 2 == 0 && g.sB % 2 == 0) ? 1 : 0;
    if (large) launch_layouts<float, 128, 128, 16>(g, grid, kc_a, kc_b, a16, b16);
    else launch_layouts<float, 64, 64, 16>(g, grid, kc_a, kc_b, a16, b16);
  } else {
    TNH_REQUIRE((uintptr_t)g.A % 16 == 0 && (uintptr_t)g.B % 16 == 0 && (uintptr_t)g.C % 16 == 0,
                "complex128 GEMM: operands must be 16-byte aligned");
    if (large) launch_layouts<double, 128, 64, 8>(g, grid, kc_a, kc_b, 1, 1);
    else launch_layouts<double, 64, 64, 8>(g, grid, kc_a, kc_b, 1, 1);
  }
  return TNH_OK;
}

}  // namespace tnh
