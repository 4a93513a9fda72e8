// Round schedule of the block one-sided Jacobi (K7 speed path), shared by the real kernels
// (tnh_svd_block.hip) and the complex ones (tnh_svd_block_complex.hip).
#pragma once
#include "tnh_types.h"

namespace tnh {

// Circle-method pairing of `n` (even) players: pair `i` of round `r` (a < b).
__host__ __device__ __forceinline__ void bj_pair(int n, int r, int i, int& a, int& b) {
  const int q = n - 1;
  if (i == 0) {
    a = q;
    b = r % q;
  } else {
    a = (r + i) % q;
    b = (r - i + q) % q;
  }
  if (a > b) {
    const int t = a;
    a = b;
    b = t;
  }
}

// Pairing of one GROUP of blocks in round r (k = pair index inside the group):
//   shift == 0: circle method over the q blocks [abase, abase + q)                    (q / 2 pairs, q - 1 rounds)
//   shift == 1: blocks [abase, abase + q) against [bbase, bbase + q), cyclic shifts   (q pairs, q rounds)
// The GROUPED schedule (round 2, svd_block_sweeps) cuts the blocks into G = 2 or 4 parts and a sweep into phases in
// which the G groups never touch the same block -- first the circle method inside every part, then, for every
// matching of the parts, half-part x half-part products in two sub-phases -- every block pair once per sweep in
// nb - 1 rounds, like the plain circle method.  Inside a phase each group runs its gram -> eig -> update chain on
// its own stream with NO synchronisation between rounds: one group's latency-bound LDS eigensolve overlaps the
// others' gram / update.
struct BjGroup {
  int shift, abase, bbase, q;
};
__host__ __device__ __forceinline__ void bj_pair_group(const BjGroup& g, int r, int k, int& a, int& b) {
  if (g.shift == 0) {
    bj_pair(g.q, r, k, a, b);
    a += g.abase;
    b += g.abase;
  } else {
    a = g.abase + k;
    b = g.bbase + (k + r) % g.q;
  }
}

// Phases of the grouped schedule for G = 2 or 4 groups (nb % (2 G) == 0): returns the phase count (3 or 7).
struct BjPhase {
  int rounds;
  BjGroup g[4];
};
static int bj_build_schedule(int nb, int G, BjPhase* phases) {
  int nphases = 0;
  const int part = nb / G, hq = part / 2;      // blocks per part, per half part
  BjPhase& p0 = phases[nphases++];
  p0.rounds = part - 1;
  for (int g = 0; g < G; ++g) p0.g[g] = BjGroup{0, g * part, 0, part};
  // matchings of the parts: G = 2: (0,1); G = 4: (0,1)(2,3), (0,2)(1,3), (0,3)(1,2)
  const int match2[1][1][2] = {{{0, 1}}};
  const int match4[3][2][2] = {{{0, 1}, {2, 3}}, {{0, 2}, {1, 3}}, {{0, 3}, {1, 2}}};
  const int nmatch = (G == 2) ? 1 : 3;
  for (int m = 0; m < nmatch; ++m)
    for (int t = 0; t < 2; ++t) {
      BjPhase& ph = phases[nphases++];
      ph.rounds = hq;
      for (int mi = 0; mi < G / 2; ++mi) {
        const int x = (G == 2) ? match2[0][mi][0] : match4[m][mi][0];
        const int y = (G == 2) ? match2[0][mi][1] : match4[m][mi][1];
        for (int u = 0; u < 2; ++u) ph.g[2 * mi + u] = BjGroup{1, x * part + u * hq, y * part + (u ^ t) * hq, hq};
      }
    }
  return nphases;
}

// Group count of a sweep: G = 2 when nb % 4 == 0 and nb >= 64, else the plain circle method on one stream;
// TNH_SVD_SCHED=1 / 2 / 4 forces the count (measurements: svd_block_sweeps in tnh_svd_block.hip).
static int bj_choose_groups(int nb) {
  int G = (nb % 4 == 0 && nb >= 64) ? 2 : 1;
  if (const char* envg = getenv("TNH_SVD_SCHED")) {
    const int want = atoi(envg);
    if (want == 1 || (want == 2 && nb % 4 == 0 && nb >= 8) || (want == 4 && nb % 8 == 0 && nb >= 16)) G = want;
  }
  return G;
}

// Streams of groups 1 .. 3 and the fork / join events of the grouped schedule (created on first use, G <= 4).
int svd_block_group_streams(int G, hipStream_t** aux, hipEvent_t** ev);

}  // namespace tnh
