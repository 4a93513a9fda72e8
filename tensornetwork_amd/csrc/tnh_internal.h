// Internal helpers shared by the libtnhip.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/tnh.h"

namespace tnh {

// ---- error plumbing --------------------------------------------------------
void set_error(const char* fmt, ...);
hipStream_t stream();       // process stream (nullptr before tnh_init)
bool initialised();
bool capturing();        // between tnh_graph_begin and tnh_graph_end: no host synchronisation is legal on the stream
int num_cus();
int stream_wgs_per_cu(int64_t bytes);   // grid-stride streaming kernels: workgroups per CU for a buffer of this size

#define TNH_HIP(call)                                                        \
  do {                                                                       \
    hipError_t _e = (call);                                                  \
    if (_e != hipSuccess) {                                                  \
      tnh::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e),  \
                     __FILE__, __LINE__);                                    \
      return TNH_ERR_HIP;                                                    \
    }                                                                        \
  } while (0)

#define TNH_REQUIRE(cond, ...)                                               \
  do {                                                                       \
    if (!(cond)) {                                                           \
      tnh::set_error(__VA_ARGS__);                                           \
      return TNH_ERR_INVALID;                                                \
    }                                                                        \
  } while (0)

#define TNH_NEED_INIT()                                                      \
  do {                                                                       \
    if (!tnh::initialised()) {                                               \
      tnh::set_error("tnh_init() has not been called");                      \
      return TNH_ERR_NOT_INIT;                                               \
    }                                                                        \
  } while (0)

#define TNH_LAUNCH_CHECK()                                                   \
  do {                                                                       \
    hipError_t _e = hipGetLastError();                                       \
    if (_e != hipSuccess) {                                                  \
      tnh::set_error("kernel launch failed: %s (%s:%d)",                     \
                     hipGetErrorString(_e), __FILE__, __LINE__);             \
      return TNH_ERR_HIP;                                                    \
    }                                                                        \
  } while (0)

inline int dtype_size(int dt) {
  switch (dt) {
    case TNH_F32: return 4;
    case TNH_F64: return 8;
    case TNH_BF16: return 2;
    case TNH_F16: return 2;
    case TNH_C64: return 8;
    case TNH_C128: return 16;
    case TNH_I32: return 4;
    case TNH_I64: return 8;
    default: return 0;
  }
}

// ---- device-side scalar helpers ---------------------------------------------
struct cf32 { float re, im; };
struct cf64 { double re, im; };

__device__ __forceinline__ float bf16_to_f32(uint16_t h) {
  return __uint_as_float(((uint32_t)h) << 16);
}
// round-to-nearest-even, NaN preserved (same rule the host shim uses).
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float f16_to_f32(uint16_t h) {
  return __half2float(__ushort_as_half(h));
}
__device__ __forceinline__ uint16_t f32_to_f16(float f) {
  return __half_as_ushort(__float2half_rn(f));
}

// 64-lane wavefront sum via DPP-free shuffles.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// K9 fast path (f32, m >= n, n % 16 == 0): 16-wide panels factored by the band SVD's panel kernels (tnh_svd_band.hip).
// *status_host != 0: a panel was numerically rank-deficient, the caller must use the column-by-column path.
bool qr_panel16_supported(int dtype, int64_t m, int64_t n);
size_t qr_panel16_work_bytes(int dtype, int64_t m, int64_t n);
int qr_panel16(int dtype, int64_t m, int64_t n, const void* A, void* Q, void* R, void* work, int* status_host);

// K9 on complex64 / complex128 (tnh_qr_complex.hip): blocked Householder QR on interleaved (re, im) storage.
// `tall`: panels taller than 512 rows run the multi-workgroup form.  No host read-back, no synchronisation.
size_t qr_complex_work_bytes(int dtype, int64_t m, int64_t n);
int qr_complex(int dtype, int64_t m, int64_t n, const void* A, void* Q, void* R, void* work, bool tall);
// tnh_qr.hip, shared by the real and the complex path: W (32 x nt) = Vp^T C with Vp (mj x 32) and C (mj x nt, ldc), the
// long K cut into up to QR_SPLITS slices (+ one remainder slice) in Wpart and summed in fixed order.
constexpr int QR_SPLITS = 32;
int qr_vt_times_c(int dt, const void* Vp, const void* C, int64_t ldc, int64_t mj, int64_t nt, void* W, void* Wpart);

// ---- arguments of the general strided-batched GEMM kernels (tnh_gemm.hip, tnh_gemm_complex.hip) ----
// A(m,k) = A[m*rsA + k*csA], B(k,n) = B[k*rsB + n*csB] in elements of the input dtype; batch through blockIdx.z.
struct GemmArgs {
  const void* A;
  const void* B;
  void* C;
  int64_t M, N, K;
  int64_t rsA, csA, rsB, csB, ldc;
  int64_t sA, sB, sC;
  int out_dt;
  double alpha, beta;  // C = alpha * A B + beta * C (real scalars; beta == 0 never reads C)
  const int* run_if;   // non-null: the f32 kernels return at once unless *run_if != 0 (guard of the 3 x bf16 split)
};

// provided by tnh_gemm_complex.hip: complex64 / complex128 on v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64.
// gemm_complex_tile picks the workgroup tile (force: -1 auto, 0 small, 1 large), returns 1 for the large one and
// fills its extents and the kernel's name; gemm_complex_launch launches ONE grid of that tile (`g` already shifted
// to the grid's first batch entry).
int gemm_complex_tile(int dtype, int64_t M, int64_t N, int64_t batch, int force, int* BM, int* BN, const char** name);
int gemm_complex_launch(int dtype, int large, const GemmArgs& g, dim3 grid);

struct DimVec {
  int64_t v[TNH_MAX_RANK];
};

}  // namespace tnh
