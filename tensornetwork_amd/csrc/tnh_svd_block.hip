// K7 (speed path): block one-sided Jacobi for f32, the sweeps of tnh_svd_factor
// when min(m, n) > 64.
//
// The P x Q working matrix X (rows are orthogonalised; P, Q padded to multiples
// of 128 with zeros) is cut into nb = P/32 row blocks.  A round pairs the blocks
// by the circle method (nb/2 disjoint pairs, nb-1 rounds per sweep).  For every
// pair Y = [X_I; X_J] (64 x Q) a round runs three launches:
//
//   bj_gram_kernel    G = Y Y^T (64 x 64) on the f32 MFMA (v_mfma_f32_32x32x2_f32),
//                     operands straight from global memory (the A and B fragments
//                     of a Gram product are the same 16-byte row pieces), K split
//                     over waves and workgroups; partial tiles II / IJ / JJ are
//                     written per split and summed in f64 by the next kernel
//                     (fixed order: deterministic).
//   bj_eig_kernel     two-sided cyclic Jacobi on G in LDS (f64, 2x2-tile
//                     ownership: one barrier pair per inner round), giving the
//                     64 x 64 orthogonal V with V^T G V diagonal.
//   bj_update_kernel  Y <- V^T Y and the matching rows of the accumulated factor
//                     R, again on the MFMA; each wave owns a 128-column strip of
//                     all 64 rows, so the update is in place.
//
// Work per sweep: 8 p^2 q-ish flop on the matrix pipe instead of (p-1) launches of
// 2-row rotations; X and R stay resident in L2 / Infinity Cache (2 x 67 MB at
// 4096^2).  Bound: f32 MFMA (157 TF) for gram/update, LDS latency for the eig.
#include <math.h>
#include <stdlib.h>
#include "tnh_types.h"
#include "tnh_svd_block_sched.h"

namespace tnh {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// phase stamps (10 ns ticks of wall_clock64) of workgroup (0, 0) of the last gram / update launch, printed by TNH_SVD_TRACE=1
__device__ int g_bj_phase[8];

// ---------------------------------------------------------------------- gram
// grid (pairs, splits), 256 threads.  Wave w of split s covers the 8-column
// chunks [(4 s + w) cpw, +cpw).  Gp[((pair*S + s)*3 + t)*1024 + row*32 + col],
// t = 0: II, 1: IJ, 2: JJ.
// DIAG (A/B knob TNH_SVD_GRAMDIAG=1, default off): only the IJ tile goes through the MFMA; II and JJ are taken as
// diag(row norms^2), i.e. the rows inside a block are treated as orthogonal during the cross rounds (the Gram
// kernel sits on the f32 MFMA roofline: 1.6 Gflop per round = 10.2 us of its 17 us).  Measured at 4096^2: 9.15 ->
// 8.34 ms per sweep, but 17 sweeps instead of 16: 0.146 -> 0.142 s, same accuracy -- not worth a convergence risk.
template <bool DIAG>
__global__ __launch_bounds__(256) void bj_gram_kernel(const float* __restrict__ X, int64_t ldx, int nb,
                                                      int round, int chunks, int cpw,
                                                      float* __restrict__ Gp, int pair0, BjGroup grp) {
  __shared__ float red[4][3][1024];
  const long long ts0 = wall_clock64();
  const int pair = pair0 + blockIdx.x, split = blockIdx.y, S = gridDim.y;
  int bi, bj;
  bj_pair_group(grp, round, (int)blockIdx.x, bi, bj);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* xi = X + ((int64_t)bi * 32 + (lane & 31)) * ldx + 4 * (lane >> 5);
  const float* xj = X + ((int64_t)bj * 32 + (lane & 31)) * ldx + 4 * (lane >> 5);
  int c0 = (split * 4 + wid) * cpw;
  int c1 = c0 + cpw;
  if (c1 > chunks) c1 = chunks;
  f32x16 aII, aIJ, aJJ;
#pragma unroll
  for (int r = 0; r < 16; ++r) aII[r] = aIJ[r] = aJJ[r] = 0.f;
  // register ring of PF chunks in flight: the next loads are issued before the 12 MFMAs that consume the current
  // chunk.  Round 2: PF 4 -> 16.  wall_clock64 stamps (TNH_SVD_TRACE=1) showed 16.5 us in this loop for 5.1 us of
  // MFMA issue: four chunks cover 1.3 us of work, the loads come back from Infinity Cache / remote L2 in ~2 us, so
  // every chunk stalled.  16 chunks (the whole range of a wave at 4096 columns) are 128 VGPRs.
  constexpr int PF = 16;
  float nI = 0.f, nJ = 0.f;
  f32x4 ra[PF], rb[PF];
#pragma unroll
  for (int i = 0; i < PF; ++i)
    if (c0 + i < c1) {
      ra[i] = *(const f32x4*)(xi + 8 * (int64_t)(c0 + i));
      rb[i] = *(const f32x4*)(xj + 8 * (int64_t)(c0 + i));
    }
  for (int c = c0; c < c1; c += PF) {
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      if (c + i < c1) {
        const f32x4 a = ra[i], b = rb[i];
        if (c + i + PF < c1) {
          ra[i] = *(const f32x4*)(xi + 8 * (int64_t)(c + i + PF));
          rb[i] = *(const f32x4*)(xj + 8 * (int64_t)(c + i + PF));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if constexpr (DIAG) {
            nI += a[e] * a[e];
            nJ += b[e] * b[e];
          } else {
            aII = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], a[e], aII, 0, 0, 0);
            aJJ = __builtin_amdgcn_mfma_f32_32x32x2f32(b[e], b[e], aJJ, 0, 0, 0);
          }
          aIJ = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], aIJ, 0, 0, 0);
        }
      }
    }
  }
  const long long ts1 = wall_clock64();
  // C/D layout: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const int idx = row * 32 + (lane & 31);
    if constexpr (DIAG) {
      const float fI = nI + __shfl_xor(nI, 32, 64), fJ = nJ + __shfl_xor(nJ, 32, 64);   // both column halves of the row
      red[wid][0][idx] = (row == (lane & 31)) ? fI : 0.f;
      red[wid][2][idx] = (row == (lane & 31)) ? fJ : 0.f;
    } else {
      red[wid][0][idx] = aII[r];
      red[wid][2][idx] = aJJ[r];
    }
    red[wid][1][idx] = aIJ[r];
  }
  __syncthreads();
  float* out = Gp + ((int64_t)pair * S + split) * 3072;
  const float* r0 = &red[0][0][0];
  for (int e = tid; e < 3072; e += 256)
    out[e] = (r0[e] + r0[3072 + e]) + (r0[2 * 3072 + e] + r0[3 * 3072 + e]);
  if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) {
    g_bj_phase[0] = (int)(ts1 - ts0);
    g_bj_phase[1] = (int)(wall_clock64() - ts1);
  }
}

// ----------------------------------------------------------------------- eig
// One workgroup per pair.  V (64 x 64, row-major) -> Jout[pair]; pairflag says
// whether any rotation was applied (the update skips identity pairs).  Plain
// f64 version (index-space pairing, two barriers per round): the eigensolver of
// the f64 path; the f32 path uses bj_eig3_kernel below.  TILE = side of the Gram
// partial tiles (32: II/IJ/JJ of the f32 gram kernel, 16: the 10 upper tiles of
// the f64 gram kernel).
template <typename TG, int TILE>
__device__ __forceinline__ int bj_partial_index(int i, int j) {
  // element (i, j) of the symmetric 64 x 64 G inside one split's partial block
  constexpr int NT = 64 / TILE;
  int a = i / TILE, b = j / TILE, ii = i % TILE, jj = j % TILE;
  if (a > b) {
    int t = a; a = b; b = t;
    t = ii; ii = jj; jj = t;
  }
  const int tile = a * NT - a * (a - 1) / 2 + (b - a);   // upper-triangular tile number
  return tile * TILE * TILE + ii * TILE + jj;
}

template <typename TG, int TILE>
__global__ __launch_bounds__(256) void bj_eig_kernel(const TG* __restrict__ Gp, int S,
                                                     TG* __restrict__ Jout, int* __restrict__ pairflag,
                                                     int* __restrict__ flag, double tol, int max_inner,
                                                     int sort) {
  constexpr int PSZ = (64 / TILE) * (64 / TILE + 1) / 2 * TILE * TILE;   // partial block size
  constexpr int W = 64, LD = 65;
  __shared__ int rank[64];
  __shared__ double G[W * LD];
  __shared__ double V[W * LD];
  __shared__ double cs_c[32], cs_s[32];
  __shared__ int rotated;
  const int pair = blockIdx.x, tid = threadIdx.x;
  const TG* gp = Gp + (int64_t)pair * S * PSZ;
  for (int e = tid; e < W * W; e += 256) {
    const int i = e >> 6, j = e & 63;
    const int idx = bj_partial_index<TG, TILE>(i, j);
    // all S <= 16 partials requested before the first add (clamped index, no branch around a load)
    TG pv[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) pv[s] = gp[(int64_t)(s < S ? s : S - 1) * PSZ + idx];
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < 16; ++s) acc += (s < S) ? (double)pv[s] : 0.0;
    G[i * LD + j] = acc;
    V[i * LD + j] = (i == j) ? 1.0 : 0.0;
  }
  int any = 0;
  const int l = tid & 31;  // column pair owned in the tile phase / pair in the rotation phase
  for (int sweep = 0; sweep < max_inner; ++sweep) {
    __syncthreads();
    if (tid == 0) rotated = 0;
    for (int r = 0; r < W - 1; ++r) {
      __syncthreads();
      if (tid < 32) {
        int a, b;
        bj_pair(W, r, tid, a, b);
        const double gpp = G[a * LD + a], gqq = G[b * LD + b], gpq = G[a * LD + b];
        double c = 1.0, s = 0.0;
        if (fabs(gpq) > tol * sqrt(fabs(gpp * gqq))) {
          const double zeta = (gqq - gpp) / (2.0 * gpq);
          const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          c = 1.0 / sqrt(1.0 + t * t);
          s = c * t;
          rotated = 1;
        }
        cs_c[tid] = c;
        cs_s[tid] = s;
      }
      __syncthreads();
      int pl, ql;
      bj_pair(W, r, l, pl, ql);
      const double cl = cs_c[l], sl = cs_s[l];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int k = (tid >> 5) + 8 * jj;
        const double ck = cs_c[k], sk = cs_s[k];
        if (sk == 0.0 && sl == 0.0) continue;
        int pk, qk;
        bj_pair(W, r, k, pk, qk);
        const double t00 = G[pk * LD + pl], t01 = G[pk * LD + ql];
        const double t10 = G[qk * LD + pl], t11 = G[qk * LD + ql];
        const double u00 = ck * t00 - sk * t10, u01 = ck * t01 - sk * t11;
        const double u10 = sk * t00 + ck * t10, u11 = sk * t01 + ck * t11;
        double v00 = cl * u00 - sl * u01, v01 = sl * u00 + cl * u01;
        double v10 = cl * u10 - sl * u11, v11 = sl * u10 + cl * u11;
        if (k == l) v01 = v10 = 0.0;  // the annihilated element
        G[pk * LD + pl] = v00;
        G[pk * LD + ql] = v01;
        G[qk * LD + pl] = v10;
        G[qk * LD + ql] = v11;
      }
      if (sl != 0.0) {
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
          const int i = (tid >> 5) + 8 * jj;
          const double vp = V[i * LD + pl], vq = V[i * LD + ql];
          V[i * LD + pl] = cl * vp - sl * vq;
          V[i * LD + ql] = sl * vp + cl * vq;
        }
      }
    }
    __syncthreads();
    const int rot = rotated;
    if (!rot) break;
    any = 1;
  }
  __syncthreads();
  // de Rijk ordering: rows leave the pair sorted by decreasing norm (column i of V
  // goes to position rank[i]), which speeds up the outer convergence
  if (tid < W) {
    int rk = tid;
    if (sort && any) {
      const double di = G[tid * LD + tid];
      rk = 0;
      for (int j = 0; j < W; ++j) {
        const double dj = G[j * LD + j];
        rk += (dj > di || (dj == di && j < tid)) ? 1 : 0;
      }
    }
    rank[tid] = rk;
  }
  __syncthreads();
  TG* jo = Jout + (int64_t)pair * (W * W);
  for (int e = tid; e < W * W; e += 256) jo[(e >> 6) * W + rank[e & 63]] = (TG)V[(e >> 6) * LD + (e & 63)];
  if (tid == 0) {
    pairflag[pair] = any;
    if (any) *flag = 1;
  }
}

// Position-space variant (default).  Pair k always sits at positions (2k, 2k+1);
// after every round the rows/columns move by the fixed circle-method permutation
// bj_next_pos (period 63, so whole sweeps end where they started).  G and V live in
// LDS as component planes (see the kernel), results are scattered to destinations that
// are fixed per thread for the whole kernel (precomputed).  Per round and thread:
// 4 TPT + 2 VPT reads, 4 TPT + 2 VPT conflict-free scattered writes, the pair's rotation
// from a 32-entry LDS table that wave 0 fills for the NEXT round while the others move V.
// Measured with wall_clock64 inside the kernel (TNH_SVD_TRACE=1) at 4096^2: prologue
// 2.2 us (was 12.4: dword loads of the S partial tiles), 32 rounds 22.6 us -- a
// barrier / LDS-latency chain of ~0.7 us per round that neither 8 vs 16 waves, nor the
// broadcast, nor taking V off wave 0 changes.
__device__ __forceinline__ int bj_next_pos(int p) {
  if (p == 0) return 0;
  const int k = p >> 1;
  if ((p & 1) == 0) return k <= 30 ? 2 * (k + 1) : 63;
  return k >= 1 ? 2 * (k - 1) + 1 : 2;
}

// TT = scalar of G's planes and of the rotation that feeds them: float (f32 path) or double (f64 path: same
// kernel since round 2 -- the f64 path used the index-space bj_eig_kernel above, 134 us per launch = 79 % of an
// f64 SVD; V is f64 in both).
template <int NT, bool BCAST, typename TT>
__global__ __launch_bounds__(NT) void bj_eig3_kernel(const TT* __restrict__ Gp, int S,
                                                     TT* __restrict__ Jout, int* __restrict__ pairflag,
                                                     int* __restrict__ flag, TT tol, int max_inner,
                                                     int cross, int sort, int pair0) {
  constexpr bool F64 = sizeof(TT) == 8;
  constexpr int W = 64, NG = NT / 32, TPT = 32 / NG, VPT = 64 / NG;
  // Component planes (round 2).  Element (p, q) of G lives in plane (p & 1) * 2 + (q & 1) at [(p >> 1) * 32 + (q >> 1)],
  // V[i][pos] in plane (pos & 1) at [i * 32 + (pos >> 1)].  The scattered writes of a round move every element
  // to the position its row / column takes next: consecutive lanes write consecutive words of ONE plane (no bank
  // conflict).  Round 1 kept a 2 x 2 tile as one float4 and V row-major: one ds_read_b128 per tile, but the writes
  // of a wave then sat 16 bytes apart -- 4-way bank conflicts on all eight scattered writes of a round, which
  // (not the arithmetic, not the barrier) is what the 1.2 us per inner round were.
  __shared__ TT T[2][4 * 1024];
  __shared__ double Vt[2][2 * W * 32];
  __shared__ int rotated;
  __shared__ TT cs32[2][32][2];         // BCAST: (c, s) of the 32 pairs of a round (by round parity), f32 for the tiles ...
  __shared__ double2 cs64[2][32];        // ... and f64 (c^2 + s^2 = 1 to f64 accuracy) for V
  const int pair = pair0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const TT* gp = Gp + (int64_t)pair * S * (F64 ? 2560 : 3072);
  TT* T0 = &T[0][0];
  const long long ts0 = wall_clock64();
  // cross mode (only pairs with one row in each block are rotated, 32 rounds):
  // position 2k = row k of block I, position 2k+1 = a row of block J; the J side
  // shifts by one slot per round.  full mode: position == index, 63 rounds.
  auto pos_of = [&](int i) { return cross ? (i < 32 ? 2 * i : 2 * (i - 32) + 1) : i; };
  auto next_pos = [&](int p) {
    if (!cross) return bj_next_pos(p);
    return (p & 1) ? 2 * (((p >> 1) + 1) & 31) + 1 : p;
  };
  // G = sum of the S partial tiles (f64, fixed order: deterministic), read as 16-byte rows of the II / IJ / JJ
  // tiles (768 float4 groups, 8 loads each at 4096^2) -- the lower-left block of G is the mirror of IJ and is
  // written from the same registers.  Round 1 read dword by dword, 32 dependent round trips per thread; measured
  // with wall_clock64 the prologue was 12 of the kernel's 37 us.
  if constexpr (!F64) {
  for (int q = tid; q < 768; q += NT) {
    const int t = q >> 8, row = (q & 255) >> 3, c4 = (q & 7) * 4;
    const float* src = (const float*)gp + t * 1024 + row * 32 + c4;
    f32x4 part[16];
#pragma unroll
    for (int sI = 0; sI < 8; ++sI) part[sI] = *(const f32x4*)(src + (sI < S ? sI : S - 1) * 3072);
    if (S > 8) {
#pragma unroll
      for (int sI = 8; sI < 16; ++sI) part[sI] = *(const f32x4*)(src + (sI < S ? sI : S - 1) * 3072);
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int sI = 0; sI < 16; ++sI) {
      if (sI < S) {
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += (double)part[sI][u];
      }
    }
    const int i = (t == 2 ? 32 : 0) + row;
    const int pi = pos_of(i);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = (t == 0 ? 0 : 32) + c4 + u;
      const int pj = pos_of(j);
      const TT v = (TT)acc[u];
      T0[((pi & 1) * 2 + (pj & 1)) * 1024 + (pi >> 1) * 32 + (pj >> 1)] = v;
      if (t == 1) T0[((pj & 1) * 2 + (pi & 1)) * 1024 + (pj >> 1) * 32 + (pi >> 1)] = v;   // G[j][i]
    }
  }
  } else {
    // f64 partials: the 10 upper 16 x 16 tiles of the f64 gram kernel; all S <= 16 partials of an element in flight
    for (int e = tid; e < W * W; e += NT) {
      const int i = e >> 6, j = e & 63;
      const int idx = bj_partial_index<double, 16>(i, j);
      double pv[16];
#pragma unroll
      for (int sI = 0; sI < 16; ++sI) pv[sI] = (double)gp[(int64_t)(sI < S ? sI : S - 1) * 2560 + idx];
      double acc = 0.0;
#pragma unroll
      for (int sI = 0; sI < 16; ++sI) acc += (sI < S) ? pv[sI] : 0.0;
      const int pi = pos_of(i), pj = pos_of(j);
      T0[((pi & 1) * 2 + (pj & 1)) * 1024 + (pi >> 1) * 32 + (pj >> 1)] = (TT)acc;
    }
  }
  for (int e = tid; e < W * W; e += NT) {
    const int i = e >> 6, pj = pos_of(e & 63);
    Vt[0][(pj & 1) * 2048 + i * 32 + (pj >> 1)] = (i == (e & 63)) ? 1.0 : 0.0;
  }
  const long long tsA = wall_clock64();
  if (tid == 0) rotated = 0;
  const int l = tid & 31, g = tid >> 5;
  const int src_half = lane & 32;
  // fixed scatter destinations (float offsets inside a T buffer / double offsets inside a V row)
  const int nc0 = next_pos(2 * l), nc1 = next_pos(2 * l + 1);
  int dst[TPT][4];
#pragma unroll
  for (int jj = 0; jj < TPT; ++jj) {
    const int k = g + NG * jj;
    const int nr0 = next_pos(2 * k), nr1 = next_pos(2 * k + 1);
    dst[jj][0] = ((nr0 & 1) * 2 + (nc0 & 1)) * 1024 + (nr0 >> 1) * 32 + (nc0 >> 1);
    dst[jj][1] = ((nr0 & 1) * 2 + (nc1 & 1)) * 1024 + (nr0 >> 1) * 32 + (nc1 >> 1);
    dst[jj][2] = ((nr1 & 1) * 2 + (nc0 & 1)) * 1024 + (nr1 >> 1) * 32 + (nc0 >> 1);
    dst[jj][3] = ((nr1 & 1) * 2 + (nc1 & 1)) * 1024 + (nr1 >> 1) * 32 + (nc1 >> 1);
  }
  const int nrounds = cross ? 32 : W - 1;
  __syncthreads();
  const long long ts1 = wall_clock64();
  int any = 0, cur = 0;
  float thmax = 0.f;   // largest |g_pq| / sqrt(g_pp g_qq) met by this workgroup (convergence telemetry, flag[1])
  // Rotation of pair l from its diagonal elements (c, s in f32 for the tiles, in f64 with c^2 + s^2 = 1 to f64
  // accuracy for V).  (An absolute floor on the row norms -- skip pairs with a row below eps |A|_F -- was tried for
  // graded inputs: it converges in fewer sweeps but leaves the near-null vectors non-orthogonal; not kept.)
  auto rotation = [&](const TT* Tb, TT& c32, TT& s32, double& c64, double& s64, bool leader) {
    const TT gpp = Tb[l * 33], gpq = Tb[1024 + l * 33], gqq = Tb[3072 + l * 33];
    if constexpr (F64) {
      double t = 0.0;
      const double gden = sqrt(fabs(gpp)) * sqrt(fabs(gqq));   // (not sqrt(gpp gqq): the product underflows on graded inputs)
      if (leader && gden > 0.0) thmax = fmaxf(thmax, (float)(fabs(gpq) / gden));
      if (fabs(gpq) > tol * gden) {
        const double zeta = (gqq - gpp) / (2.0 * gpq);
        t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        if (!(fabs(t) <= 1.0)) t = 0.0;  // inf / nan guard
        if (leader && t != 0.0) rotated = 1;
      }
      c64 = 1.0 / sqrt(1.0 + t * t);
      s64 = c64 * t;
      c32 = c64;
      s32 = s64;
    } else {
      float tf = 0.f;
      // |g_pq| against tol sqrt(g_pp) sqrt(g_qq) with the two roots taken separately: g_pp g_qq and g_pq^2 underflow
      // in f32 as soon as two rows are below 1e-10 of the largest (every graded / rank-deficient input), and a test
      // on the squares then reads "already orthogonal" for rows that are not (caught by tools/svd_graded_probe.py)
      const float gden = __builtin_amdgcn_sqrtf(fabsf(gpp)) * __builtin_amdgcn_sqrtf(fabsf(gqq));
      if (leader && gden > 0.f) thmax = fmaxf(thmax, fabsf(gpq) * __builtin_amdgcn_rcpf(gden));
      if (fabsf(gpq) > tol * gden) {
        const float zeta = (gqq - gpp) * __builtin_amdgcn_rcpf(2.0f * gpq);
        const float den = fabsf(zeta) + __builtin_amdgcn_sqrtf(1.0f + zeta * zeta);
        tf = __builtin_amdgcn_rcpf(den);
        tf = (zeta >= 0.f) ? tf : -tf;
        if (!(fabsf(tf) <= 1.0f)) tf = 0.f;  // inf / nan guard
        if (leader && tf != 0.f) rotated = 1;
      }
      c32 = __builtin_amdgcn_rsqf(1.0f + tf * tf);
      s32 = c32 * tf;
      const double t = (double)tf, x = 1.0 + t * t;
      double y = (double)c32;          // 1 ulp of f32; one Newton step: c^2 + s^2 = 1 to 2^-46
      y = y * (1.5 - 0.5 * x * y * y);
      c64 = y;
      s64 = y * t;
    }
  };
  for (int sweep = 0; sweep < max_inner; ++sweep) {
    if constexpr (BCAST) {
      // rotations of round 0 (later rounds: computed by wave 0 while the other waves update V, see below)
      __syncthreads();
      if (tid < 32) {
        TT c32, s32;
        double c64, s64;
        rotation(T[cur], c32, s32, c64, s64, true);
        cs32[0][l][0] = c32;
        cs32[0][l][1] = s32;
        cs64[0][l] = make_double2(c64, s64);
      }
    }
    for (int r = 0; r < nrounds; ++r) {
      __syncthreads();
      const TT* Tc = T[cur];
      TT* Tn = T[cur ^ 1];
      const double* Vc = Vt[cur];
      double* Vn = Vt[cur ^ 1];
      TT clf, slf;
      double cl, sl;
      if constexpr (BCAST) {
        // ONE rotation per pair, broadcast through LDS (double-buffered by round parity).  Round 1 had every
        // thread derive its own copy and fetch its row partner's by shuffle.
        clf = cs32[r & 1][l][0];
        slf = cs32[r & 1][l][1];
      } else {
        rotation(Tc, clf, slf, cl, sl, g == 0);
      }
#pragma unroll
      for (int jj = 0; jj < TPT; ++jj) {
        const int k = g + NG * jj;
        TT ck, sk;
        if constexpr (BCAST) {
          ck = cs32[r & 1][k][0];
          sk = cs32[r & 1][k][1];
        } else {
          ck = __shfl(clf, k | src_half, 64);
          sk = __shfl(slf, k | src_half, 64);
        }
        const TT t0 = Tc[k * 32 + l], t1 = Tc[1024 + k * 32 + l], t2 = Tc[2048 + k * 32 + l], t3 = Tc[3072 + k * 32 + l];
        const TT u00 = ck * t0 - sk * t2, u01 = ck * t1 - sk * t3;
        const TT u10 = sk * t0 + ck * t2, u11 = sk * t1 + ck * t3;
        TT v00 = clf * u00 - slf * u01, v01 = slf * u00 + clf * u01;
        TT v10 = clf * u10 - slf * u11, v11 = slf * u10 + clf * u11;
        if (k == l && slf != (TT)0) v01 = v10 = (TT)0;  // the annihilated element
        Tn[dst[jj][0]] = v00;
        Tn[dst[jj][1]] = v01;
        Tn[dst[jj][2]] = v10;
        Tn[dst[jj][3]] = v11;
      }
      if constexpr (BCAST) {
        const double2 m64 = cs64[r & 1][l];
        cl = m64.x;
        sl = m64.y;
        __syncthreads();            // the next tiles are complete
        // wave 0 derives the NEXT round's rotations from them while everybody (wave 0 last) moves V: the
        // dependent chain of reciprocal / square-root steps hides behind the f64 work of the other 15 waves
        if (tid < 32 && r + 1 < nrounds) {
          TT c32, s32;
          double c64, s64;
          rotation(Tn, c32, s32, c64, s64, true);
          cs32[(r + 1) & 1][l][0] = c32;
          cs32[(r + 1) & 1][l][1] = s32;
          cs64[(r + 1) & 1][l] = make_double2(c64, s64);
        }
      }
#pragma unroll
      for (int jj = 0; jj < VPT; ++jj) {
        const int i = g + NG * jj;
        const double vp = Vc[i * 32 + l], vq = Vc[2048 + i * 32 + l];
        Vn[(nc0 & 1) * 2048 + i * 32 + (nc0 >> 1)] = cl * vp - sl * vq;
        Vn[(nc1 & 1) * 2048 + i * 32 + (nc1 >> 1)] = sl * vp + cl * vq;
      }
      cur ^= 1;
    }
    __syncthreads();
    const int rot = rotated;
    __syncthreads();
    if (!rot) break;
    any = 1;
    if (tid == 0) rotated = 0;
  }
  __syncthreads();
  const long long ts2 = wall_clock64();
  // whole sweeps = full periods of the permutation: positions are back where they started
  const double* Vf = Vt[cur];
  TT* jo = Jout + (int64_t)pair * (W * W);
  // de Rijk ordering (A/B knob TNH_SVD_SORT=1, default off): the rotated rows leave the pair sorted by
  // decreasing norm, the 32 largest into the lower-numbered block.  Measured on MI355X it does not pay in
  // this block scheme: 4096^2 Gaussian 17 -> 20 sweeps, 2048^2 with s_i = 2^(-i/32) 37 -> 35.
  // `rank` lives in the (idle) other T buffer.
  int* rank = (int*)&T[cur ^ 1][0];
  float* dg = (float*)(rank + W);
  if (sort && any) {
    __syncthreads();
    if (tid < W) {
      const int pi = pos_of(tid);
      dg[tid] = (float)T[cur][(pi & 1) * 3 * 1024 + (pi >> 1) * 33];
    }
    __syncthreads();
    if (tid < W) {
      const float di = dg[tid];
      int rk = 0;
      for (int j = 0; j < W; ++j) {
        const float dj = dg[j];
        rk += (dj > di || (dj == di && j < tid)) ? 1 : 0;
      }
      rank[tid] = rk;
    }
  } else {
    __syncthreads();
    if (tid < W) rank[tid] = tid;
  }
  __syncthreads();
  for (int e = tid; e < W * W; e += NT) {
    const int pp = pos_of(e & 63);
    jo[(e >> 6) * W + rank[e & 63]] = (TT)Vf[(pp & 1) * 2048 + (e >> 6) * 32 + (pp >> 1)];
  }
  if (tid < 64) {   // wave 0 holds the g == 0 lanes (tid < 32)
    float m = thmax;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (tid == 0) atomicMax((unsigned int*)(flag + 1), __float_as_uint(m));
  }
  if (tid == 0) {
    pairflag[pair] = any;
    if (any) *flag = 1;
    if (pair == 0) {   // timing probe (TNH_SVD_TRACE): 10 ns ticks of prologue / rounds / epilogue of pair 0
      flag[2] = (int)(ts1 - ts0) | ((int)(tsA - ts0) << 16);
      flag[3] = (int)(ts2 - ts1);
    }
  }
}

// -------------------------------------------------------------------- update
// grid (pairs, ceil(nss / 4)), 256 threads; wave = one 128-column super-strip of
// [X | R].  Y'[a][c] = sum_k V[k][a] Y[k][c].
__global__ __launch_bounds__(256) void bj_update_kernel(float* __restrict__ X, int64_t ldx, int nssX,
                                                        float* __restrict__ R, int64_t ldr, int nssR,
                                                        int nb, int round, const float* __restrict__ J,
                                                        const int* __restrict__ pairflag, int pair0, BjGroup grp) {
  const long long ts0 = wall_clock64();
  const int pair = pair0 + blockIdx.x;
  if (!pairflag[pair]) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // J (64 x 64) once per workgroup through LDS with 16-byte loads.  Round 1: every wave fetched its 64 fragment
  // values as dword loads -- 64 load instructions whose issue alone held the first MFMA back by ~6 us (stamps).
  __shared__ float Js[64 * 64];
  {
    const f32x4* jsrc = (const f32x4*)(J + (int64_t)pair * 4096);
#pragma unroll
    for (int q = 0; q < 4; ++q) ((f32x4*)Js)[tid + 256 * q] = jsrc[tid + 256 * q];
  }
  __syncthreads();
  const int ss = blockIdx.y * 4 + wid;
  if (ss >= nssX + nssR) return;
  int bi, bj;
  bj_pair_group(grp, round, (int)blockIdx.x, bi, bj);
  float* base;
  int64_t ld;
  if (ss < nssX) { base = X + (int64_t)ss * 128; ld = ldx; }
  else { base = R + (int64_t)(ss - nssX) * 128; ld = ldr; }
  const int i = lane & 31, kk = lane >> 5;
  auto grow = [&](int row) -> int64_t { return row < 32 ? (int64_t)bi * 32 + row : (int64_t)bj * 32 + (row - 32); };

  f32x4 bv[32];
#pragma unroll
  for (int ks = 0; ks < 32; ++ks) bv[ks] = *(const f32x4*)(base + grow(2 * ks + kk) * ld + 4 * i);
  float jf[2][32];
#pragma unroll
  for (int ks = 0; ks < 32; ++ks) {
    jf[0][ks] = Js[(2 * ks + kk) * 64 + i];
    jf[1][ks] = Js[(2 * ks + kk) * 64 + 32 + i];
  }

  long long ts1 = 0;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    f32x16 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
        acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(jf[it][ks], bv[ks][s], acc[s], 0, 0, 0);
      if (it == 0 && ks == 31) ts1 = wall_clock64();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * it + (r & 3) + 8 * (r >> 2) + 4 * kk;
      f32x4 o;
      o[0] = acc[0][r]; o[1] = acc[1][r]; o[2] = acc[2][r]; o[3] = acc[3][r];
      *(f32x4*)(base + grow(row) * ld + 4 * i) = o;
    }
  }
  if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) {
    g_bj_phase[2] = (int)(ts1 - ts0);
    g_bj_phase[3] = (int)(wall_clock64() - ts1);
  }
}

// ------------------------------------------------------------------ f64 path
// Same three-launch round on the f64 matrix pipe (v_mfma_f64_16x16x4_f64).  A pair
// is 4 row blocks of 16; the Gram kernel accumulates the 10 upper tiles of G.
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void bj_gram64_kernel(const double* __restrict__ X, int64_t ldx, int nb,
                                                        int round, int chunks, int cpw,
                                                        double* __restrict__ Gp, int pair0, BjGroup grp) {
  __shared__ double red[4][10 * 256];
  const int pair = pair0 + blockIdx.x, split = blockIdx.y, S = gridDim.y;
  int bi, bj;
  bj_pair_group(grp, round, (int)blockIdx.x, bi, bj);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const double* xr[4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
    const int64_t row = (rb < 2 ? (int64_t)bi * 32 + rb * 16 : (int64_t)bj * 32 + (rb - 2) * 16) + (lane & 15);
    xr[rb] = X + row * ldx + 2 * (lane >> 4);
  }
  int c0 = (split * 4 + wid) * cpw;
  int c1 = c0 + cpw;
  if (c1 > chunks) c1 = chunks;
  f64x4 acc[10];
#pragma unroll
  for (int t = 0; t < 10; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = 0.0;
  for (int c = c0; c < c1; ++c) {
    f64x2 f[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) f[rb] = *(const f64x2*)(xr[rb] + 8 * (int64_t)c);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      int t = 0;
#pragma unroll
      for (int ra = 0; ra < 4; ++ra)
#pragma unroll
        for (int rbb = ra; rbb < 4; ++rbb) {
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[ra][e], f[rbb][e], acc[t], 0, 0, 0);
          ++t;
        }
    }
  }
  // C/D layout: col = lane & 15, row = (lane >> 4) + 4 r
#pragma unroll
  for (int t = 0; t < 10; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wid][t * 256 + ((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[t][r];
  __syncthreads();
  double* out = Gp + ((int64_t)pair * S + split) * 2560;
  for (int e = tid; e < 2560; e += 256) out[e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
}

// grid (pairs, ceil(nss / 4)); wave = one 32-column strip of [X | R] (all 64 rows, in place).
__global__ __launch_bounds__(256) void bj_update64_kernel(double* __restrict__ X, int64_t ldx, int nssX,
                                                          double* __restrict__ R, int64_t ldr, int nssR,
                                                          int nb, int round, const double* __restrict__ J,
                                                          const int* __restrict__ pairflag, int pair0, BjGroup grp) {
  const int pair = pair0 + blockIdx.x;
  if (!pairflag[pair]) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int ss = blockIdx.y * 4 + wid;
  if (ss >= nssX + nssR) return;
  int bi, bj;
  bj_pair_group(grp, round, (int)blockIdx.x, bi, bj);
  double* base;
  int64_t ld;
  if (ss < nssX) { base = X + (int64_t)ss * 32; ld = ldx; }
  else { base = R + (int64_t)(ss - nssX) * 32; ld = ldr; }
  const int n = lane & 15, kk = lane >> 4;
  const double* Jp = J + (int64_t)pair * 4096;
  auto grow = [&](int row) -> int64_t { return row < 32 ? (int64_t)bi * 32 + row : (int64_t)bj * 32 + (row - 32); };
  f64x2 bv[16];
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) bv[ks] = *(const f64x2*)(base + grow(4 * ks + kk) * ld + 2 * n);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    f64x4 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc0[r] = acc1[r] = 0.0;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const double jf = Jp[(4 * ks + kk) * 64 + 16 * it + n];   // A operand: V[k][a], a = 16 it + n
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(jf, bv[ks][0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(jf, bv[ks][1], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * it + kk + 4 * r;
      f64x2 o;
      o[0] = acc0[r];
      o[1] = acc1[r];
      *(f64x2*)(base + grow(row) * ld + 2 * n) = o;
    }
  }
}

// Xp (P x Q, zero padded) = A (m x n row-major) or its transpose.
template <typename T, bool TRANS>
__global__ __launch_bounds__(256) void bj_pad_copy_kernel(T* __restrict__ Xp, int64_t Q,
                                                          const T* __restrict__ A, int64_t m, int64_t n) {
  __shared__ T tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int64_t r0 = (int64_t)blockIdx.y * 32, c0 = (int64_t)blockIdx.x * 32;  // tile origin in Xp
  if (!TRANS) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t r = r0 + ty + 8 * j, c = c0 + tx;
      Xp[r * Q + c] = (r < m && c < n) ? A[r * n + c] : (T)0;
    }
  } else {
    // Xp[r][c] = A[c][r]; rows of Xp index columns of A (r < n), cols of Xp index rows of A (c < m)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t ar = c0 + ty + 8 * j, ac = r0 + tx;
      tile[ty + 8 * j][tx] = (ar < m && ac < n) ? A[ar * n + ac] : (T)0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) Xp[(r0 + ty + 8 * j) * Q + c0 + tx] = tile[tx][ty + 8 * j];
  }
}

template <typename T>
int svd_block_pad_copy(T* Xp, int64_t P, int64_t Q, const T* A, int64_t m, int64_t n, bool trans) {
  const dim3 grid((unsigned)(Q / 32), (unsigned)(P / 32));
  if (trans) hipLaunchKernelGGL((bj_pad_copy_kernel<T, true>), grid, dim3(256), 0, stream(), Xp, Q, A, m, n);
  else hipLaunchKernelGGL((bj_pad_copy_kernel<T, false>), grid, dim3(256), 0, stream(), Xp, Q, A, m, n);
  TNH_LAUNCH_CHECK();
  return TNH_OK;
}
template int svd_block_pad_copy<float>(float*, int64_t, int64_t, const float*, int64_t, int64_t, bool);
template int svd_block_pad_copy<double>(double*, int64_t, int64_t, const double*, int64_t, int64_t, bool);

size_t svd_block_scratch_bytes(int esz, int64_t P, int64_t Q) {
  const int64_t pairs = P / 64;
  (void)Q;
  return (size_t)pairs * 16 * 3072 * esz   // Gram partials (<= 16 splits; 2560 per split for f64)
         + (size_t)pairs * 4096 * esz      // V per pair
         + (size_t)pairs * sizeof(int) + 256;   // pair flags
}

// auxiliary streams of the grouped round schedule (see svd_block_sweeps)
int svd_block_group_streams(int G, hipStream_t** aux, hipEvent_t** ev) {
  static hipStream_t g_aux[3] = {nullptr, nullptr, nullptr};     // streams of groups 1 .. 3 of the grouped schedule
  static hipEvent_t g_ev[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < G - 1; ++i)
    if (!g_aux[i]) TNH_HIP(hipStreamCreateWithFlags(&g_aux[i], hipStreamNonBlocking));
  for (int i = 0; i < G; ++i)
    if (!g_ev[i]) TNH_HIP(hipEventCreateWithFlags(&g_ev[i], hipEventDisableTiming));
  *aux = g_aux;
  *ev = g_ev;
  return TNH_OK;
}

// Sweeps until a whole sweep applies no rotation.  X: P x Q (ld Q), R: P x P.
template <typename T>
int svd_block_sweeps(T* X, T* R, int64_t P, int64_t Q, char* scratch, int* flag, double tol,
                     int max_sweeps, int* sweeps_out, bool* converged_out) {
  constexpr bool F64 = sizeof(T) == 8;
  const int nb = (int)(P / 32), pairs = nb / 2;
  T* Gp = (T*)scratch;
  T* J = Gp + (size_t)pairs * 16 * 3072;
  int* pairflag = (int*)(J + (size_t)pairs * 4096);
  const int chunks = (int)(Q / 8);
  // splits: enough workgroups to fill the chip, each wave with >= 4 chunks of work
  // (TNH_SVD_SPLITS: A/B knob; the two-group schedule launches half the pairs at a time)
  const char* envsp = getenv("TNH_SVD_SPLITS");
  int S = envsp ? atoi(envsp) : (2 * num_cus() + pairs - 1) / pairs;
  if (S > 16) S = 16;
  while (S > 1 && chunks / (4 * S) < 4) --S;
  if (S < 1) S = 1;
  const int cpw = (chunks + 4 * S - 1) / (4 * S);
  const int sw = F64 ? 32 : 128;    // strip width of the update kernel
  // R == nullptr: the rotations are not accumulated (top-k mode: the other side's vectors are
  // recovered from A by one GEMM, tnh_svd_vectors_topk) -- the update kernel then has half the strips
  const int nssX = (int)(Q / sw), nssR = R ? (int)(P / sw) : 0;
  const char* env = getenv("TNH_SVD_INNER");
  const int inner = env ? atoi(env) : 1;
  const char* envc = getenv("TNH_SVD_CROSS");
  const int crossv = envc ? atoi(envc) : 1;
  const char* envso = getenv("TNH_SVD_SORT");
  const int sortv = envso ? atoi(envso) : 0;      // de Rijk row ordering inside every pair: A/B knob, off (see bj_eig3_kernel)
  const char* envn = getenv("TNH_SVD_EIGNT");
  const int eig_nt = envn ? atoi(envn) : 1024;   // workgroup size of the LDS eigensolver (A/B knob)
  const char* enve64 = getenv("TNH_SVD_EIG64");
  const bool eig64_new = !(enve64 && enve64[0] == '0');   // f64 path on the position-space eigensolver (A/B knob)
  const char* envgd = getenv("TNH_SVD_GRAMDIAG");
  const bool gramdiag = envgd && envgd[0] == '1';
  const char* envb = getenv("TNH_SVD_BCAST");
  const bool bcast = !(envb && envb[0] == '0');   // rotations computed once per pair and broadcast through LDS (A/B knob)
  // Stop rule: a whole sweep that applies no rotation above `tol` (the last sweep only observes).
  // TNH_SVD_STOP=<theta> (A/B knob, default off) ends after a sweep whose largest normalised off-diagonal
  // theta = |g_pq| / sqrt(g_pp g_qq) is <= theta, betting on quadratic convergence.  Measured on MI355X
  // (profiles/r02_svd_convergence.txt): it saves exactly the observing sweep on configs[2] (17 -> 16, same
  // values) but is UNSAFE in general -- theta is small from the first sweep when all singular values are close
  // (eigh's shifted matrix A + |A|_F 1: theta ~ 1e-3 at sweep 1, nowhere near converged), so it stays off.
  // TNH_SVD_TRACE=1 prints theta per sweep.
  const char* envs = getenv("TNH_SVD_STOP");
  const float stop_theta = F64 ? 0.f : (envs ? (float)atof(envs) : 0.f);
  const bool trace = getenv("TNH_SVD_TRACE") != nullptr;
  // Grouped schedule (see BjGroup): G = 2 when nb % 4 == 0 and nb >= 64 (f32 and f64), else the plain circle method
  // on one stream; never inside a graph capture.  TNH_SVD_SCHED=1 / 2 / 4 forces the group count.  Measured on MI355X
  // (4096^2 / 2048^2 / 1024^2 / 512^2): G = 1 0.165 / 0.051 / 0.021 / 0.0093 s, G = 2 0.147 / 0.049 / 0.022 / 0.0095 s,
  // G = 4 0.139 (15 instead of 16 sweeps; the same 9.2 ms per sweep as G = 2) / 0.055 / 0.025 / 0.0126 s: the overlap
  // is exhausted with two chains, more streams only add launches.  (Round 2 also tried the SAME circle round cut into G groups on G streams with a fork /
  // join per round, TNH_SVD_GROUPS: G = 2 / 3 / 4 -> 0.243 / 0.269 / 0.307 s against 0.216 -- the per-round events
  // cost more than the overlap returned.  This schedule needs cross-stream events only at the phase boundaries.)
  // two chains pay from 2048 rows on (f32 1024^2: 0.0206 s on one stream, 0.0216 s on two; f64 512^2: 0.0150 / 0.0174)
  int G = bj_choose_groups(nb);
  if (F64 && !eig64_new) G = 1;
  if (G > 1) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream(), &cap);
    if (cap != hipStreamCaptureStatusNone) G = 1;     // inside a graph capture: stay on one stream
  }
  hipStream_t* g_aux = nullptr;
  hipEvent_t* g_ev = nullptr;
  if (G > 1) {
    const int rc = svd_block_group_streams(G, &g_aux, &g_ev);
    if (rc) return rc;
  }
  auto gstream = [&](int g) { return g == 0 ? stream() : g_aux[g - 1]; };
  // every stream has seen everything the others queued so far
  auto cross_sync = [&]() -> int {
    for (int g = 0; g < G; ++g) TNH_HIP(hipEventRecord(g_ev[g], gstream(g)));
    for (int g = 0; g < G; ++g)
      for (int o = 0; o < G; ++o)
        if (o != g) TNH_HIP(hipStreamWaitEvent(gstream(g), g_ev[o], 0));
    return TNH_OK;
  };
  // one round of a group: `np` pairs whose Gram / J slots start at global pair index p0, on stream st
  auto f32_round = [&](hipStream_t st, const BjGroup& grp, int r, int p0, int np, int cross) {
    if constexpr (F64) {
      const dim3 ug((unsigned)np, (unsigned)((nssX + nssR + 3) / 4));
      hipLaunchKernelGGL(bj_gram64_kernel, dim3((unsigned)np, (unsigned)S), dim3(256), 0, st, X, Q, nb, r, chunks, cpw, Gp,
                         p0, grp);
      if (eig64_new)
        hipLaunchKernelGGL((bj_eig3_kernel<1024, true, double>), dim3((unsigned)np), dim3(1024), 0, st, Gp, S, J, pairflag,
                           flag, tol, inner, cross, 0, p0);
      else   // (round-1 eigensolver: A/B only; it has no pair offset, so it runs ungrouped -- see below)
        hipLaunchKernelGGL((bj_eig_kernel<double, 16>), dim3((unsigned)np), dim3(256), 0, st, Gp, S, J, pairflag, flag,
                           tol, inner, 0);
      hipLaunchKernelGGL(bj_update64_kernel, ug, dim3(256), 0, st, X, Q, nssX, R, P, nssR, nb, r, J, pairflag, p0, grp);
    }
    if constexpr (!F64) {
      const dim3 ug((unsigned)np, (unsigned)((nssX + nssR + 3) / 4));
      if (gramdiag && cross)
        hipLaunchKernelGGL(bj_gram_kernel<true>, dim3((unsigned)np, (unsigned)S), dim3(256), 0, st, X, Q, nb, r, chunks,
                           cpw, Gp, p0, grp);
      else
        hipLaunchKernelGGL(bj_gram_kernel<false>, dim3((unsigned)np, (unsigned)S), dim3(256), 0, st, X, Q, nb, r, chunks,
                           cpw, Gp, p0, grp);
#define TNH_EIG3(NT_, B_)                                                                                               \
  hipLaunchKernelGGL((bj_eig3_kernel<NT_, B_, float>), dim3((unsigned)np), dim3(NT_), 0, st, Gp, S, J, pairflag, flag, \
                     (float)tol, inner, cross, sortv, p0)
      if (eig_nt == 512) { if (bcast) TNH_EIG3(512, true); else TNH_EIG3(512, false); }
      else if (eig_nt == 256) { if (bcast) TNH_EIG3(256, true); else TNH_EIG3(256, false); }
      else { if (bcast) TNH_EIG3(1024, true); else TNH_EIG3(1024, false); }
#undef TNH_EIG3
      hipLaunchKernelGGL(bj_update_kernel, ug, dim3(256), 0, st, X, Q, nssX, R, P, nssR, nb, r, J, pairflag, p0, grp);
    }
  };
  BjPhase phases[7];
  const int nphases = (G > 1) ? bj_build_schedule(nb, G, phases) : 0;
  const BjGroup whole{0, 0, 0, nb};
  int sweeps = 0;
  bool converged = false;
  while (!converged && sweeps < max_sweeps) {
    TNH_HIP(hipMemsetAsync(flag, 0, 4 * sizeof(int), stream()));
    if (G > 1) {
      const int np = pairs / G;   // pairs per group (part / 2 in the first phase, hq in the others)
      int rc = cross_sync();
      if (rc) return rc;
      for (int ph = 0; ph < nphases; ++ph) {
        for (int r = 0; r < phases[ph].rounds; ++r) {
          const int cross = (crossv && !(ph == 0 && r == 0)) ? 1 : 0;   // the first round also rotates inside the blocks
          for (int g = 0; g < G; ++g) f32_round(gstream(g), phases[ph].g[g], r, g * np, np, cross);
        }
        rc = cross_sync();
        if (rc) return rc;
      }
    } else {
      for (int r = 0; r < nb - 1; ++r) f32_round(stream(), whole, r, 0, pairs, (crossv && r > 0) ? 1 : 0);
    }
    TNH_LAUNCH_CHECK();
    int h[4] = {0, 0, 0, 0};
    TNH_HIP(hipMemcpyAsync(h, flag, 4 * sizeof(int), hipMemcpyDeviceToHost, stream()));
    TNH_HIP(hipStreamSynchronize(stream()));
    ++sweeps;
    float theta;
    memcpy(&theta, &h[1], sizeof(float));
    if (trace) {
      int ph[8] = {0};
      (void)hipMemcpyFromSymbol(ph, HIP_SYMBOL(g_bj_phase), sizeof(ph));
      fprintf(stderr, "[tnh svd] gram wg(0,0): loads + MFMA %.2f us, reduce + store %.2f us; update wg(0,0): loads + first half %.2f us, rest %.2f us\n",
              ph[0] * 0.01, ph[1] * 0.01, ph[2] * 0.01, ph[3] * 0.01);
    }
    if (trace)
      fprintf(stderr, "[tnh svd] sweep %d: rotated %d, max theta %.3e; last eig of pair 0: prologue %.2f us, rounds %.2f us, (of the prologue: loads + sums %.2f us)\n",
              sweeps, h[0], (double)theta, (h[2] & 0xffff) * 0.01, h[3] * 0.01, ((unsigned)h[2] >> 16) * 0.01);
    converged = (h[0] == 0) || (!F64 && stop_theta > 0.f && theta <= stop_theta);
  }
  *sweeps_out = sweeps;
  *converged_out = converged;
  return TNH_OK;
}
template int svd_block_sweeps<float>(float*, float*, int64_t, int64_t, char*, int*, double, int, int*, bool*);
template int svd_block_sweeps<double>(double*, double*, int64_t, int64_t, char*, int*, double, int, int*, bool*);

// The block pairs of one sweep in launch order (host only; tests): out[(round * nb/2 + pair) * 2 + {0, 1}].
int svd_block_schedule_pairs(int nb, int groups, int32_t* out, int* rounds_out) {
  int round = 0;
  const int pairs = nb / 2;
  if (groups <= 1) {
    for (int r = 0; r < nb - 1; ++r, ++round)
      for (int i = 0; i < pairs; ++i) {
        int a, b;
        bj_pair(nb, r, i, a, b);
        out[((int64_t)round * pairs + i) * 2] = a;
        out[((int64_t)round * pairs + i) * 2 + 1] = b;
      }
  } else {
    BjPhase phases[7];
    const int nphases = bj_build_schedule(nb, groups, phases);
    const int np = pairs / groups;
    for (int ph = 0; ph < nphases; ++ph)
      for (int r = 0; r < phases[ph].rounds; ++r, ++round)
        for (int g = 0; g < groups; ++g)
          for (int k = 0; k < np; ++k) {
            int a, b;
            bj_pair_group(phases[ph].g[g], r, k, a, b);
            out[((int64_t)round * pairs + g * np + k) * 2] = a;
            out[((int64_t)round * pairs + g * np + k) * 2 + 1] = b;
          }
  }
  *rounds_out = round;
  return TNH_OK;
}

}  // namespace tnh
