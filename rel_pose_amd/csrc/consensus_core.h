// consensus_core.h -- the seeded hypothesise-and-verify core of the consensus libraries (csrc_consensus/consensus.hip,
// csrc_fivepoint/five_point.hip, csrc_homography/homography.hip), one definition of every stage they share.  The sampler and the
// tie-breaking rule are a documented contract (include/relpose_consensus.h: the same seed gives the same bits): a library differs from
// the others by its sample size, its minimal solver and its distance, which are template parameters or stay in its own file.
//
//   hypothesis kernel  grid n * ceil(M / 256) (problem-major, one dimension), 256 threads, one lane per hypothesis
//     consensus_stage   the flags "weight positive" of all rows go to LDS with coalesced loads; thread t then counts the flags of the
//                       CONTIGUOUS rows t * per .. t * per + per - 1 (per = ceil(P / 256) <= 7), the counts go to LDS, every thread reads
//                       them back in thread order (an ordered prefix sum, no atomics) and writes the numbers of its rows of positive
//                       weight: pos, ascending.  Points and weights are then gathered through pos, COMPACTED, with loads that are
//                       coalesced up to the gaps.  Four barriers, all inside; from there on no thread talks to another.
//     consensus_sample  Floyd's S draws without replacement from the K compacted rows, and the row numbers of the sample
//     consensus_cost    the lane walks the K compacted rows: every lane of the workgroup reads the SAME LDS address (a broadcast, no bank
//                       conflict) and adds to its own sums in the same fixed order -- no reduction, no barrier
//   select kernel      grid n, 256 threads
//     consensus_select  the lowest-index argmin of the costs over the valid slots (a tree in LDS on (cost, index)), the distances at the
//                       winner, w_out, and the thread's share of the four sums of stat; the kernel reduces them with block_sum
//   consensus_launch   host: the argument checks (shape, then size, then alignment) and the two launches
// LDS is declared by the __global__ function and passed in by reference (the convention of block_sum.h).
#pragma once
#include <float.h>
#include "common.h"
#include "block_sum.h"
#include "two_view.h"
#include "../../include/relpose_hip.h"

template <int MAXP>
struct ConsensusRows {
  float2 a[MAXP], b[MAXP];     // the rows of positive weight, ascending: x1, x2
  float w[MAXP];
  int pos[MAXP];               // their row numbers
  int cnt[BLOCK_SUM_THREADS];
};                             // 42 496 B at MAXP = 1728

RP_DEV uint32_t mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// the distance of the essential-matrix libraries
struct SampsonDistance {
  RP_DEV float operator()(const float (&e)[9], float2 a, float2 b) const { return sampson(e, a, b); }
};

// the flags of the rows (coalesced), the ordered prefix over contiguous runs of them, then the rows of positive weight; returns their
// number K
template <int MAXP>
RP_DEV int consensus_stage(ConsensusRows<MAXP>& sm, const float2* X1, const float2* X2, const float* W, int P) {
  constexpr int NT = BLOCK_SUM_THREADS, ROWS = (MAXP + NT - 1) / NT;      // ROWS: rows one thread stages, 7
  const int tid = threadIdx.x;
  for (int r = tid; r < P; r += NT) sm.pos[r] = (W ? fmaxf(W[r], 0.f) : 1.f) > 0.f ? 1 : 0;
  __syncthreads();
  const int per = (P + NT - 1) / NT;                // thread t numbers the rows t * per .. t * per + per - 1
  int flag[ROWS], mine = 0;
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = tid * per + i;
    flag[i] = i < per && r < P ? sm.pos[r] : 0;     // (into registers: pos is overwritten below)
    mine += flag[i];
  }
  sm.cnt[tid] = mine;
  __syncthreads();
  int at = 0, K = 0;
  for (int t = 0; t < NT; ++t) {
    const int c = sm.cnt[t];
    K += c;
    at += t < tid ? c : 0;
  }
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    if (flag[i]) sm.pos[at++] = tid * per + i;      // (every flag was read before the barrier above; at < K <= P)
  }
  __syncthreads();
  for (int j = tid; j < K; j += NT) {               // ascending rows: close to coalesced
    const int r = sm.pos[j];
    sm.a[j] = X1[r];
    sm.b[j] = X2[r];
    sm.w[j] = W ? W[r] : 1.f;
  }
  __syncthreads();
  return K;
}

// hypothesis m of problem b: c = S distinct draws from 0 .. K - 1 (zeros if K < S), their row numbers to samples (if asked for)
template <int S, int MAXP>
RP_DEV void consensus_sample(const ConsensusRows<MAXP>& sm, uint32_t seed, long long b, int m, int M, int K, int* samples,
                             uint32_t (&c)[S]) {
#pragma unroll
  for (int k = 0; k < S; ++k) c[k] = 0u;
  if (K >= S) {
    const uint32_t s = mix(mix(seed + 0x9E3779B9u * (uint32_t)(b + 1)) ^ (uint32_t)m);
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const uint32_t r = mix(s + 0x9E3779B9u * (uint32_t)(k + 1));
      const uint32_t j = (uint32_t)(K - S + k);
      const uint32_t t = (uint32_t)(((uint64_t)r * (uint64_t)(j + 1u)) >> 32);
      bool seen = false;
#pragma unroll
      for (int l = 0; l < k; ++l) seen = seen || c[l] == t;
      c[k] = seen ? j : t;
    }
  }
  if (samples) {
    int* SO = samples + (b * M + m) * S;
#pragma unroll
    for (int k = 0; k < S; ++k) SO[k] = K >= S ? sm.pos[c[k]] : 0;
  }
}

// the robust cost of the model e over the K compacted rows: sum w tau^2 log1p(d / tau^2) / sum w
template <int MAXP, class D>
RP_DEV float consensus_cost(const ConsensusRows<MAXP>& sm, const float (&e)[9], int K, float tau2, D dist) {
  float acc = 0.f, wsum = 0.f;
  for (int j = 0; j < K; ++j) {
    const float wt = sm.w[j];
    const float d = dist(e, sm.a[j], sm.b[j]);
    acc += wt * (tau2 * log1pf(d / tau2));
    wsum += wt;
  }
  return acc / wsum;
}

// the winner among the S slots of a problem (HC: their costs, HM: their models), -1 if none is valid; e: its model (zeros if none);
// w_out at the winner; s4: THIS THREAD's share of the sum of the weights, of those within tau, of the count of the positive ones and of
// the count of the valid slots.  bc, bi: LDS of the caller.
template <class D>
RP_DEV int consensus_select(float (&bc)[BLOCK_SUM_THREADS], int (&bi)[BLOCK_SUM_THREADS], const float2* X1, const float2* X2,
                            const float* W, float* WO, const float* HC, const float* HM, int S, int P, float ta, D dist, float (&e)[9],
                            float (&s4)[4]) {
  constexpr int NT = BLOCK_SUM_THREADS;
  const int tid = threadIdx.x;
  // ---- the lowest-index minimum among the valid slots, and their number
  float lo = FLT_MAX, nvalid = 0.f;
  int arg = -1;
  for (int m = tid; m < S; m += NT) {
    const float c = HC[m];
    nvalid += c < FLT_MAX ? 1.f : 0.f;
    if (c < lo) { lo = c; arg = m; }               // (ascending m: the first of equal costs stays)
  }
  bc[tid] = lo;
  bi[tid] = arg;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const float c = bc[tid + s];
      const int i = bi[tid + s];
      if (i >= 0 && (c < bc[tid] || bi[tid] < 0 || (c == bc[tid] && i < bi[tid]))) { bc[tid] = c; bi[tid] = i; }
    }
    __syncthreads();
  }
  const int win = bi[0];
#pragma unroll
  for (int i = 0; i < 9; ++i) e[i] = win >= 0 ? HM[win * 9 + i] : 0.f;
  const float tau2 = win >= 0 ? ta * ta : 1.f;
  // ---- the weights at the winner
  s4[0] = s4[1] = s4[2] = 0.f;
  s4[3] = nvalid;
  for (int r = tid; r < P; r += NT) {
    const float wt = W ? fmaxf(W[r], 0.f) : 1.f;
    const float d = dist(e, X1[r], X2[r]);
    s4[0] += wt;
    s4[1] += d <= tau2 ? wt : 0.f;
    s4[2] += wt > 0.f ? 1.f : 0.f;
    if (WO) WO[r] = win >= 0 ? wt / (1.f + d / tau2) : wt;
  }
  return win;
}

// host: the argument checks of a consensus entry point (sample size S; shape, then size, then alignment) and its two launches
template <int S, int MAXP, int MAXM, auto HYPOTHESIS, auto SELECT>
inline int consensus_launch(const float* x1, const float* x2, const float* w, const float* tau, int seed, float* model, int* best,
                            float* stat, float* w_out, float* hyp, float* hyp_cost, int* samples, int P, int M, int n, void* stream) {
  constexpr int NT = BLOCK_SUM_THREADS;
  if (n <= 0 || P < S || M < 1 || !x1 || !x2 || !tau || !model || !best || !stat || !hyp || !hyp_cost) return RP_EBADSHAPE;
  if (P > MAXP || M > MAXM) return RP_EUNSUPPORTED;
  const int chunks = (M + NT - 1) / NT;
  if ((long long)n * chunks > 2147483647LL) return RP_EUNSUPPORTED;
  if (((uintptr_t)x1 | (uintptr_t)x2) & 7) return RP_EALIGN;
  if (((uintptr_t)w | (uintptr_t)tau | (uintptr_t)model | (uintptr_t)best | (uintptr_t)stat | (uintptr_t)w_out | (uintptr_t)hyp |
       (uintptr_t)hyp_cost | (uintptr_t)samples) & 3)
    return RP_EALIGN;
  hipLaunchKernelGGL(HYPOTHESIS, dim3(n * chunks), dim3(NT), 0, (hipStream_t)stream, x1, x2, w, tau, (uint32_t)seed, hyp, hyp_cost,
                     samples, P, M, chunks);
  RP_CHECK_LAUNCH();
  hipLaunchKernelGGL(SELECT, dim3(n), dim3(NT), 0, (hipStream_t)stream, x1, x2, w, tau, hyp, hyp_cost, model, best, stat, w_out, P, M);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
