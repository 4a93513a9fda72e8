// K9 on complex64 / complex128: thin Householder QR of a row-major matrix of interleaved (re, im) elements, read and
// written where they lie (no real embedding, no planar copies).  LAPACK zgeqrf + zungqr conventions:
//
//   H_c = I - tau_c v_c v_c^H,  A = H_0 H_1 ... R,  the factorisation applies H_c^H = I - conj(tau_c) v_c v_c^H.
//   zlarfg: beta = -sign(Re alpha) sqrt(|alpha|^2 + xnorm^2) is REAL, tau = ((beta - Re alpha) / beta, -Im alpha / beta),
//   v = x / (alpha - beta); tau = 0 (H = I) only when xnorm == 0 and Im alpha == 0.  R's diagonal is therefore real.
//
//   for each panel of 32 columns:
//     cqr_panel_kernel  ONE workgroup of 1024 threads = 32 columns x 32 row lanes, a thread owns one complex element of
//                       a panel row (a row is one 256-B / 512-B line); the pivot column's element reaches the other
//                       columns of its row by wave shuffles of its 32-bit halves.  Per column two passes:
//                       w_j = v^H P[:, j], then P[:, j] -= conj(tau) v w_j fused with the next column's norm.
//                       Then S = V^H V in one pass over the panel (32-row tiles staged in LDS, thread (k, j) owns
//                       S[k][j]: one accumulator per thread instead of 32) and T by the zlarft recurrence in LDS.
//                       Writes the clean V, Vc = conj(V), T and Tc = conj(T): tnh_gemm_ex transposes but does not
//                       conjugate, so V^H = Vc^T and T^H = Tc^T.
//     tall panels       (m_j > 512) the same recurrence over G workgroups, one launch per column: the dots
//                       d_j = sum_{r>c} conj(P[r][c]) P[r][j] give the norm (j = c) and every w_j = P[c][j] + conj(scale) d_j;
//                       the launch that applies reflector c accumulates the d_j of column c+1.
//     trailing update   C <- (I - V T^H V^H) C:  W = Vc^T C (long K cut into slices), W2 = Tc^T W, C -= V W2
//                       on the complex MFMA kernels (tnh_gemm_complex.hip).
//   Q like zungqr: Q = I_thin, panels applied last to first with W2 = T W.
// All panel arithmetic is in double, as in tnh_qr.hip.  No host read-back and no synchronisation: capturable.
#include "tnh_types.h"

namespace tnh {
namespace {

constexpr int CQB = 32;          // panel width
constexpr int CQR_MAX_WG = 256;  // workgroups of a tall panel

template <typename R> struct CxOf;
template <> struct CxOf<float> { using Z = cf32; using V = float2; };
template <> struct CxOf<double> { using Z = cf64; using V = double2; };

__device__ __forceinline__ cf64 cconj(cf64 a) { return {a.re, -a.im}; }

// one 8-byte / 16-byte access per element (the work buffers are 256-byte aligned, elements naturally aligned)
template <typename R>
__device__ __forceinline__ typename CxOf<R>::Z cld(const typename CxOf<R>::Z* p) {
  const typename CxOf<R>::V t = *reinterpret_cast<const typename CxOf<R>::V*>(p);
  return {t.x, t.y};
}
template <typename R>
__device__ __forceinline__ void cst(typename CxOf<R>::Z* p, typename CxOf<R>::Z v) {
  typename CxOf<R>::V t;
  t.x = v.re; t.y = v.im;
  *reinterpret_cast<typename CxOf<R>::V*>(p) = t;
}
template <typename Z> __device__ __forceinline__ cf64 widen(Z a) { return {(double)a.re, (double)a.im}; }
template <typename R> __device__ __forceinline__ typename CxOf<R>::Z narrow(cf64 a) { return {(R)a.re, (R)a.im}; }
// element of lane `src` (storage precision: two or four 32-bit shuffles)
template <typename Z> __device__ __forceinline__ Z cshfl(Z a, int src) {
  return {__shfl(a.re, src, 64), __shfl(a.im, src, 64)};
}

// zlarfg from alpha and the squared norm of the sub-column
__device__ __forceinline__ void clarfg(cf64 alpha, double xnorm2, cf64* tau, cf64* scale, double* beta) {
  *tau = {0.0, 0.0};
  *scale = {0.0, 0.0};
  *beta = alpha.re;
  if (xnorm2 > 0.0 || alpha.im != 0.0) {
    const double b = -copysign(sqrt(alpha.re * alpha.re + alpha.im * alpha.im + xnorm2), alpha.re);
    *beta = b;
    *tau = {(b - alpha.re) / b, -alpha.im / b};
    *scale = cf64{1.0, 0.0} / cf64{alpha.re - b, alpha.im};
  }
}

__device__ __forceinline__ double cqr_block_sum_1024(double v, double* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += red[i];
  return s;
}

// T (zlarft, forward / columnwise) from S = V^H V and tau; 1024 threads, T_s zeroed here.
__device__ __forceinline__ void clarft(cf64 (*T_s)[33], const cf64 (*S_s)[33], const cf64* tau_s, int jb) {
  const int tid = threadIdx.x;
  T_s[tid >> 5][tid & 31] = {0.0, 0.0};
  __syncthreads();
  for (int c = 0; c < jb; ++c) {
    if (tid < c) {
      cf64 s = {0.0, 0.0};
      for (int k = tid; k < c; ++k) s = s + T_s[tid][k] * S_s[k][c];
      const cf64 t = tau_s[c];
      T_s[tid][c] = cf64{-t.re, -t.im} * s;
    } else if (tid == c) {
      T_s[c][c] = tau_s[c];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// one-workgroup panel.  A: full matrix (row-major, lda); panel = rows j0 .., columns j0 .. j0+jb-1 (jb <= m - j0).
// Outputs: panel in place (R above the diagonal, V below), tau[j0 ..], Vp / Vc ((m-j0) x 32: clean V and its
// conjugate), Tm / Tc (32 x 32, zero outside the upper triangle).
// ---------------------------------------------------------------------------
template <typename R>
__global__ __launch_bounds__(1024) void cqr_panel_kernel(typename CxOf<R>::Z* __restrict__ A, int64_t lda, int64_t m,
                                                         int64_t j0, int jb, typename CxOf<R>::Z* __restrict__ tau,
                                                         typename CxOf<R>::Z* __restrict__ Tm,
                                                         typename CxOf<R>::Z* __restrict__ Tc,
                                                         typename CxOf<R>::Z* __restrict__ Vp,
                                                         typename CxOf<R>::Z* __restrict__ Vc) {
  using Z = typename CxOf<R>::Z;
  __shared__ cf64 X_s[32][33];   // column passes: per-row-lane partials; S pass: a 32-row tile of V
  __shared__ cf64 S_s[32][33];
  __shared__ cf64 T_s[32][33];
  __shared__ cf64 w_s[32];
  __shared__ cf64 tau_s[32];
  __shared__ double red[16];
  __shared__ cf64 sc_tau, sc_scale;
  __shared__ double sc_beta;
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5, lane = tid & 63;
  const int64_t mj = m - j0;
  Z* P = A + j0 * lda + j0;
  const bool col_ok = tx < jb;
  const Z zero = {(R)0, (R)0};

  double part = 0.0;
  for (int64_t li = 1 + tid; li < mj; li += 1024) part += (double)abs2(widen(cld<R>(P + li * lda)));
  double xnorm2 = cqr_block_sum_1024(part, red);

  for (int c = 0; c < jb; ++c) {
    if (tid == 0) {
      cf64 t, sc;
      double beta;
      clarfg(widen(cld<R>(P + (int64_t)c * lda + c)), xnorm2, &t, &sc, &beta);
      sc_tau = t; sc_scale = sc; sc_beta = beta;
      tau_s[c] = t;
    }
    __syncthreads();
    const cf64 t_c = sc_tau, scale = sc_scale;
    // ---- pass W: v = x * scale stored in place; w_j = P[c][j] + sum_r conj(v_r) P[r][j]  (j > c)
    cf64 wp = {0.0, 0.0};
    for (int64_t li = c + 1 + ty; li < mj; li += 32) {
      const Z a = col_ok ? cld<R>(P + li * lda + tx) : zero;
      const Z v = narrow<R>(widen(cshfl(a, (lane & 32) | c)) * scale);
      if (tx == c) cst<R>(P + li * lda + c, v);
      else if (tx > c) wp = wp + cconj(widen(v)) * widen(a);
    }
    X_s[ty][tx] = wp;
    __syncthreads();
    if (tid < 32) {
      cf64 s = {0.0, 0.0};
#pragma unroll
      for (int i = 0; i < 32; ++i) s = s + X_s[i][tid];
      if (tid > c && tid < jb) s = s + widen(cld<R>(P + (int64_t)c * lda + tid));
      w_s[tid] = s;
    }
    __syncthreads();
    // ---- pass U: P[r][j] -= conj(tau) v_r w_j (j > c); pivot row: v = 1; next column's norm
    const bool upd = tx > c && col_ok;
    const cf64 tw = upd ? cconj(t_c) * w_s[tx] : cf64{0.0, 0.0};
    double n2 = 0.0;
    if (ty == 0) {
      if (upd) cst<R>(P + (int64_t)c * lda + tx, narrow<R>(widen(cld<R>(P + (int64_t)c * lda + tx)) - tw));
      if (tx == c) cst<R>(P + (int64_t)c * lda + c, Z{(R)sc_beta, (R)0});
    }
    for (int64_t li = c + 1 + ty; li < mj; li += 32) {
      Z a = col_ok ? cld<R>(P + li * lda + tx) : zero;
      const Z v = cshfl(a, (lane & 32) | c);
      if (upd) {
        a = narrow<R>(widen(a) - widen(v) * tw);
        cst<R>(P + li * lda + tx, a);
        if (tx == c + 1 && li > c + 1) n2 += (double)abs2(widen(a));
      }
    }
    xnorm2 = cqr_block_sum_1024(n2, red);
  }

  // ---- clean V / conj(V) panels and S = V^H V: thread (k = ty, tx) owns S[k][tx]
  cf64 acc = {0.0, 0.0};
  for (int64_t base = 0; base < mj; base += 32) {
    const int64_t li = base + ty;
    Z v = zero;
    if (li < mj) {
      if (col_ok) {
        if (li > tx) v = cld<R>(P + li * lda + tx);
        else if (li == tx) v = Z{(R)1, (R)0};
      }
      cst<R>(Vp + li * CQB + tx, v);
      cst<R>(Vc + li * CQB + tx, Z{v.re, -v.im});
    }
    __syncthreads();
    X_s[ty][tx] = widen(v);
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < 32; ++r) acc = acc + cconj(X_s[r][ty]) * X_s[r][tx];
  }
  S_s[ty][tx] = acc;
  __syncthreads();
  clarft(T_s, S_s, tau_s, jb);
  if (tid < jb) cst<R>(tau + j0 + tid, narrow<R>(tau_s[tid]));
  const cf64 t = (ty < jb && tx < jb) ? T_s[ty][tx] : cf64{0.0, 0.0};
  cst<R>(Tm + ty * CQB + tx, narrow<R>(t));
  cst<R>(Tc + ty * CQB + tx, narrow<R>(cconj(t)));
}

// ---------------------------------------------------------------------------
// Tall panels: workgroup g owns rows [g * rpw, (g+1) * rpw) of the panel; 256 threads = 8 row lanes x 32 columns.
//   cqr_coldot_kernel  d_j partials of column 0, pivot row 0                 (once per panel)
//   cqr_col_kernel     reduce partials -> (tau, scale, w) -> update own rows -> partials and pivot row of column c+1
//   cqr_vts_kernel     clean V / conj(V) panels + partials of S = V^H V      (once per panel)
//   cqr_tmat_kernel    T / conj(T) from S and tau                            (once per panel, 1 WG)
// Partials are complex doubles.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void cqr_wg_reduce32(cf64 v, cf64 (*colred)[33], cf64* out_partial) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  __syncthreads();
  colred[ty][tx] = v;
  __syncthreads();
  if (threadIdx.x < 32) {
    cf64 s = {0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 8; ++i) s = s + colred[i][threadIdx.x];
    out_partial[threadIdx.x] = s;
  }
}

template <typename R>
__global__ __launch_bounds__(256) void cqr_coldot_kernel(const typename CxOf<R>::Z* __restrict__ P, int64_t lda,
                                                         int64_t mj, int jb, int64_t rpw, cf64* __restrict__ part_out,
                                                         cf64* __restrict__ row_out) {
  using Z = typename CxOf<R>::Z;
  __shared__ cf64 colred[8][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, lane = threadIdx.x & 63;
  const int64_t r0 = (int64_t)blockIdx.x * rpw;
  int64_t r1 = r0 + rpw;
  if (r1 > mj) r1 = mj;
  if (blockIdx.x == 0 && ty == 0) row_out[tx] = (tx < jb) ? widen(cld<R>(P + tx)) : cf64{0.0, 0.0};
  cf64 acc = {0.0, 0.0};
  for (int64_t li = r0 + ty; li < r1; li += 8) {
    const Z a = (tx < jb) ? cld<R>(P + li * lda + tx) : Z{(R)0, (R)0};
    const Z x = cshfl(a, (lane & 32) | 0);
    if (li > 0) acc = acc + cconj(widen(x)) * widen(a);
  }
  cqr_wg_reduce32(acc, colred, part_out + (int64_t)blockIdx.x * 32);
}

template <typename R>
__global__ __launch_bounds__(256) void cqr_col_kernel(typename CxOf<R>::Z* __restrict__ P, int64_t lda, int64_t mj,
                                                      int c, int jb, int64_t rpw, int nwg,
                                                      const cf64* __restrict__ part_in, cf64* __restrict__ part_out,
                                                      cf64* __restrict__ tau_out, const cf64* __restrict__ row_in,
                                                      cf64* __restrict__ row_out) {
  using Z = typename CxOf<R>::Z;
  __shared__ cf64 colred[8][33];
  __shared__ cf64 d_s[32];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5, lane = tid & 63;
  // 1. reduce the partial dots of column c (fixed order): lane ty sums every 8th workgroup's partial, 16 loads in
  //    flight at a time (clamped index, no branch around a load)
  {
    cf64 s = {0.0, 0.0};
    for (int q0 = 0; q0 < CQR_MAX_WG / 8; q0 += 16) {
      if (ty + 8 * q0 >= nwg) break;   // (no barrier inside this loop)
      cf64 pv[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int g = ty + 8 * (q0 + q);
        pv[q] = part_in[(int64_t)(g < nwg ? g : nwg - 1) * 32 + tx];
      }
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (ty + 8 * (q0 + q) < nwg) s = s + pv[q];
    }
    colred[ty][tx] = s;
    __syncthreads();
    if (tid < 32) {
      cf64 r = {0.0, 0.0};
#pragma unroll
      for (int i = 0; i < 8; ++i) r = r + colred[i][tid];
      d_s[tid] = r;
    }
  }
  __syncthreads();
  // 2. zlarfg: every thread derives the same scalars.  The pivot row comes from row_in (written by the previous
  //    launch): its owner rewrites P[c][:] below while other workgroups still need it.
  cf64 t_c, scale;
  double beta;
  clarfg(row_in[c], d_s[c].re, &t_c, &scale, &beta);
  const bool col_ok = tx < jb;
  const bool upd = tx > c && col_ok;
  const cf64 prow = row_in[tx];
  const cf64 tw = upd ? cconj(t_c) * (prow + cconj(scale) * d_s[tx]) : cf64{0.0, 0.0};   // conj(tau) w_j
  // 3. update own rows; accumulate the dots of column c+1 over rows > c+1
  const int64_t r0 = (int64_t)blockIdx.x * rpw;
  int64_t r1 = r0 + rpw;
  if (r1 > mj) r1 = mj;
  if (c >= r0 && c < r1 && ty == 0) {   // pivot row (v = 1)
    if (upd) cst<R>(P + (int64_t)c * lda + tx, narrow<R>(prow - tw));
    if (tx == c) cst<R>(P + (int64_t)c * lda + c, Z{(R)beta, (R)0});
    if (tx == 0) tau_out[c] = t_c;
  }
  cf64 acc = {0.0, 0.0};
  int64_t start = r0 + ty;
  if (start <= c) start += ((c - start) / 8 + 1) * 8;   // first row > c in this lane
  for (int64_t li = start; li < r1; li += 8) {
    Z a = col_ok ? cld<R>(P + li * lda + tx) : Z{(R)0, (R)0};
    const Z v = narrow<R>(widen(cshfl(a, (lane & 32) | c)) * scale);
    if (tx == c) {
      a = v;
      cst<R>(P + li * lda + c, a);
    } else if (upd) {
      a = narrow<R>(widen(a) - widen(v) * tw);
      cst<R>(P + li * lda + tx, a);
    }
    if (c + 1 < 32) {
      const Z y = cshfl(a, (lane & 32) | (c + 1));
      if (li > c + 1 && tx > c) acc = acc + cconj(widen(y)) * widen(a);
      if (li == c + 1) row_out[tx] = col_ok ? widen(a) : cf64{0.0, 0.0};   // next launch's pivot row
    }
  }
  cqr_wg_reduce32(acc, colred, part_out + (int64_t)blockIdx.x * 32);
}

// s_part[g][k][tx] = sum over the workgroup's rows of conj(v[r][k]) v[r][tx]; 32-row tiles staged in LDS, thread
// (ty, tx) owns k = ty, ty + 8, ty + 16, ty + 24.
template <typename R>
__global__ __launch_bounds__(256) void cqr_vts_kernel(const typename CxOf<R>::Z* __restrict__ P, int64_t lda,
                                                      int64_t mj, int jb, int64_t rpw,
                                                      typename CxOf<R>::Z* __restrict__ Vp,
                                                      typename CxOf<R>::Z* __restrict__ Vc, cf64* __restrict__ s_part) {
  using Z = typename CxOf<R>::Z;
  __shared__ cf64 X_s[32][33];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int64_t r0 = (int64_t)blockIdx.x * rpw;
  int64_t r1 = r0 + rpw;
  if (r1 > mj) r1 = mj;
  cf64 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = {0.0, 0.0};
  for (int64_t base = r0; base < r1; base += 32) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t li = base + ty + 8 * q;
      Z v = {(R)0, (R)0};
      if (li < r1) {
        if (tx < jb) {
          if (li > tx) v = cld<R>(P + li * lda + tx);
          else if (li == tx) v = Z{(R)1, (R)0};
        }
        cst<R>(Vp + li * CQB + tx, v);
        cst<R>(Vc + li * CQB + tx, Z{v.re, -v.im});
      }
      X_s[ty + 8 * q][tx] = widen(v);
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < 32; ++r) {
      const cf64 x = X_s[r][tx];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = acc[q] + cconj(X_s[r][ty + 8 * q]) * x;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) s_part[((int64_t)blockIdx.x * 32 + ty + 8 * q) * 32 + tx] = acc[q];
}

template <typename R>
__global__ __launch_bounds__(1024) void cqr_tmat_kernel(const cf64* __restrict__ s_part, int nwg,
                                                        const cf64* __restrict__ tau_d, int jb, int64_t j0,
                                                        typename CxOf<R>::Z* __restrict__ tau,
                                                        typename CxOf<R>::Z* __restrict__ Tm,
                                                        typename CxOf<R>::Z* __restrict__ Tc) {
  __shared__ cf64 S_s[32][33];
  __shared__ cf64 T_s[32][33];
  __shared__ cf64 tau_s[32];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  cf64 s = {0.0, 0.0};
  for (int g0 = 0; g0 < nwg; g0 += 8) {   // 8 partials in flight (clamped index; fixed summation order)
    cf64 pv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int g = g0 + q;
      pv[q] = s_part[((int64_t)(g < nwg ? g : nwg - 1) * 32 + ty) * 32 + tx];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (g0 + q < nwg) s = s + pv[q];
  }
  S_s[ty][tx] = s;   // S[k = ty][tx]
  if (tid < 32) tau_s[tid] = tid < jb ? tau_d[tid] : cf64{0.0, 0.0};
  __syncthreads();
  clarft(T_s, S_s, tau_s, jb);
  if (tid < jb) cst<R>(tau + j0 + tid, narrow<R>(tau_s[tid]));
  const cf64 t = (ty < jb && tx < jb) ? T_s[ty][tx] : cf64{0.0, 0.0};
  cst<R>(Tm + ty * CQB + tx, narrow<R>(t));
  cst<R>(Tc + ty * CQB + tx, narrow<R>(cconj(t)));
}

// scratch of a tall panel (complex doubles): 2 x [MAX_WG][32] ping-pong dot partials, [MAX_WG][32][32] S partials,
// [32] tau, 2 x [32] ping-pong pivot rows
constexpr size_t CQR_TALL_SCRATCH =
    ((size_t)2 * CQR_MAX_WG * 32 + (size_t)CQR_MAX_WG * 1024 + 32 + 64) * sizeof(cf64);

template <typename R>
int cqr_panel_tall(typename CxOf<R>::Z* Af, int64_t lda, int64_t m, int64_t j0, int jb, typename CxOf<R>::Z* tau,
                   typename CxOf<R>::Z* Tm, typename CxOf<R>::Z* Tc, typename CxOf<R>::Z* Vp, typename CxOf<R>::Z* Vc,
                   cf64* scratch) {
  using Z = typename CxOf<R>::Z;
  const int64_t mj = m - j0;
  int nwg = (int)((mj + 63) / 64);
  if (nwg > CQR_MAX_WG) nwg = CQR_MAX_WG;
  const int64_t rpw = ((mj + nwg - 1) / nwg + 7) / 8 * 8;
  nwg = (int)((mj + rpw - 1) / rpw);
  cf64* part[2] = {scratch, scratch + (size_t)CQR_MAX_WG * 32};
  cf64* s_part = scratch + (size_t)2 * CQR_MAX_WG * 32;
  cf64* tau_d = s_part + (size_t)CQR_MAX_WG * 1024;
  cf64* row[2] = {tau_d + 32, tau_d + 64};
  Z* P = Af + j0 * lda + j0;
  hipLaunchKernelGGL((cqr_coldot_kernel<R>), dim3(nwg), dim3(256), 0, stream(), (const Z*)P, lda, mj, jb, rpw, part[0],
                     row[0]);
  for (int c = 0; c < jb; ++c)
    hipLaunchKernelGGL((cqr_col_kernel<R>), dim3(nwg), dim3(256), 0, stream(), P, lda, mj, c, jb, rpw, nwg,
                       (const cf64*)part[c & 1], part[(c + 1) & 1], tau_d, (const cf64*)row[c & 1], row[(c + 1) & 1]);
  hipLaunchKernelGGL((cqr_vts_kernel<R>), dim3(nwg), dim3(256), 0, stream(), (const Z*)P, lda, mj, jb, rpw, Vp, Vc,
                     s_part);
  hipLaunchKernelGGL((cqr_tmat_kernel<R>), dim3(1), dim3(1024), 0, stream(), (const cf64*)s_part, nwg,
                     (const cf64*)tau_d, jb, j0, tau, Tm, Tc);
  TNH_LAUNCH_CHECK();
  return TNH_OK;
}

// Vp / Vc ((m-j0) x 32) <- clean V of the panel stored in the factored matrix, and its conjugate.
template <typename Z>
__global__ __launch_bounds__(256) void cqr_extract_v_kernel(const Z* __restrict__ A, int64_t lda, int64_t m, int64_t j0,
                                                            int jb, Z* __restrict__ Vp, Z* __restrict__ Vc) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t li = e >> 5;
  const int tx = (int)(e & 31);
  if (li >= m - j0) return;
  Z v = {0, 0};
  if (tx < jb) {
    if (li > tx) v = A[(j0 + li) * lda + j0 + tx];
    else if (li == tx) v = Z{1, 0};
  }
  Vp[li * CQB + tx] = v;
  Vc[li * CQB + tx] = Z{v.re, -v.im};
}

// R (k x n) = upper triangle of the factored matrix; Q (m x k) = thin identity.
template <typename Z>
__global__ __launch_bounds__(256) void cqr_triu_kernel(Z* __restrict__ Rm, const Z* __restrict__ A, int64_t lda,
                                                       int64_t k, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= k * n) return;
  const int64_t i = e / n, j = e % n;
  Rm[e] = (j >= i) ? A[i * lda + j] : Z{0, 0};
}
template <typename Z>
__global__ __launch_bounds__(256) void cqr_eye_kernel(Z* __restrict__ Q, int64_t m, int64_t k) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= m * k) return;
  Q[e] = (e / k == e % k) ? Z{1, 0} : Z{0, 0};
}

inline size_t calign256(size_t x) { return (x + 255) & ~(size_t)255; }

// W (32 x nt) = V^H C is qr_vt_times_c (tnh_qr.hip: split-K strided-batched GEMM + fixed-order sum) on Vc = conj(V).
struct CqrWork {
  char *Af, *Vp, *Vc, *Tm, *Tc, *W, *W2, *tau, *tall, *Wpart;
  size_t total;
};
CqrWork cqr_layout(char* base, int esz, int64_t m, int64_t n) {
  const int64_t k = m < n ? m : n;
  const int64_t np = (k + CQB - 1) / CQB;
  const int64_t wide = n > k ? n : k;
  CqrWork w;
  size_t off = 0;
  w.Af = base + off;    off += calign256((size_t)m * n * esz);
  w.Vp = base + off;    off += calign256((size_t)m * CQB * esz);
  w.Vc = base + off;    off += calign256((size_t)m * CQB * esz);
  w.Tm = base + off;    off += calign256((size_t)np * CQB * CQB * esz);
  w.Tc = base + off;    off += calign256((size_t)np * CQB * CQB * esz);
  w.W = base + off;     off += calign256((size_t)CQB * wide * esz);
  w.W2 = base + off;    off += calign256((size_t)CQB * wide * esz);
  w.tau = base + off;   off += calign256((size_t)(k + CQB) * esz);
  w.tall = base + off;  off += calign256(CQR_TALL_SCRATCH);
  w.Wpart = base + off; off += calign256((size_t)(QR_SPLITS + 1) * CQB * wide * esz);
  w.total = off;
  return w;
}

template <typename R>
int cqr_run(int dt, int64_t m, int64_t n, const void* A, void* Qv, void* Rv, char* work, bool tall) {
  using Z = typename CxOf<R>::Z;
  const int64_t k = m < n ? m : n;
  const CqrWork w = cqr_layout(work, sizeof(Z), m, n);
  Z* Af = (Z*)w.Af;
  Z* Vp = (Z*)w.Vp;
  Z* Vc = (Z*)w.Vc;
  Z* Q = (Z*)Qv;
  TNH_HIP(hipMemcpyAsync(Af, A, (size_t)m * n * sizeof(Z), hipMemcpyDeviceToDevice, stream()));
  // ---- factor (zgeqrf)
  for (int64_t j0 = 0; j0 < k; j0 += CQB) {
    const int jb = (int)((k - j0 < CQB) ? (k - j0) : CQB);
    const int64_t mj = m - j0;
    Z* Tm = (Z*)w.Tm + (j0 / CQB) * CQB * CQB;
    Z* Tc = (Z*)w.Tc + (j0 / CQB) * CQB * CQB;
    if (mj > 512 && tall) {
      const int rc = cqr_panel_tall<R>(Af, n, m, j0, jb, (Z*)w.tau, Tm, Tc, Vp, Vc, (cf64*)w.tall);
      if (rc) return rc;
    } else {
      hipLaunchKernelGGL((cqr_panel_kernel<R>), dim3(1), dim3(1024), 0, stream(), Af, n, m, j0, jb, (Z*)w.tau, Tm, Tc,
                         Vp, Vc);
      TNH_LAUNCH_CHECK();
    }
    const int64_t nt = n - j0 - jb;
    if (nt > 0) {
      Z* C = Af + j0 * n + j0 + jb;
      int rc = qr_vt_times_c(dt, Vc, C, n, mj, nt, w.W, w.Wpart);                                      // W = V^H C
      if (rc) return rc;
      rc = tnh_gemm_ex(dt, dt, 1, 0, CQB, nt, CQB, Tc, CQB, w.W, nt, w.W2, nt, 1, 0, 0, 0, 1.0, 0.0);   // W2 = T^H W
      if (rc) return rc;
      rc = tnh_gemm_ex(dt, dt, 0, 0, mj, nt, CQB, Vp, CQB, w.W2, nt, C, n, 1, 0, 0, 0, -1.0, 1.0);      // C -= V W2
      if (rc) return rc;
    }
  }
  // ---- R and Q (zungqr)
  {
    const int64_t ne = k * n;
    hipLaunchKernelGGL((cqr_triu_kernel<Z>), dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, stream(), (Z*)Rv,
                       (const Z*)Af, n, k, n);
    const int64_t nq = m * k;
    hipLaunchKernelGGL((cqr_eye_kernel<Z>), dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream(), Q, m, k);
    TNH_LAUNCH_CHECK();
  }
  const int64_t last = ((k - 1) / CQB) * CQB;
  for (int64_t j0 = last; j0 >= 0; j0 -= CQB) {
    const int jb = (int)((k - j0 < CQB) ? (k - j0) : CQB);
    const int64_t mj = m - j0;
    const int64_t nc = k - j0;  // columns j0 .. k-1 of Q are touched by this and later panels
    Z* Tm = (Z*)w.Tm + (j0 / CQB) * CQB * CQB;
    const int64_t ne = mj * CQB;
    hipLaunchKernelGGL((cqr_extract_v_kernel<Z>), dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, stream(),
                       (const Z*)Af, n, m, j0, jb, Vp, Vc);
    TNH_LAUNCH_CHECK();
    Z* C = Q + j0 * k + j0;
    int rc = qr_vt_times_c(dt, Vc, C, k, mj, nc, w.W, w.Wpart);                                      // W = V^H C
    if (rc) return rc;
    rc = tnh_gemm_ex(dt, dt, 0, 0, CQB, nc, CQB, Tm, CQB, w.W, nc, w.W2, nc, 1, 0, 0, 0, 1.0, 0.0);   // W2 = T W
    if (rc) return rc;
    rc = tnh_gemm_ex(dt, dt, 0, 0, mj, nc, CQB, Vp, CQB, w.W2, nc, C, k, 1, 0, 0, 0, -1.0, 1.0);      // C -= V W2
    if (rc) return rc;
  }
  return TNH_OK;
}

}  // namespace

size_t qr_complex_work_bytes(int dtype, int64_t m, int64_t n) {
  return cqr_layout(nullptr, dtype_size(dtype), m, n).total + 256;
}

int qr_complex(int dtype, int64_t m, int64_t n, const void* A, void* Q, void* R, void* work, bool tall) {
  char* base = (char*)(((uintptr_t)work + 255) & ~(uintptr_t)255);
  if (dtype == TNH_C64) return cqr_run<float>(dtype, m, n, A, Q, R, base, tall);
  return cqr_run<double>(dtype, m, n, A, Q, R, base, tall);
}

}  // namespace tnh
