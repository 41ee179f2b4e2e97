// select.hip -- which two-view model the matches support (librelpose_select.so): rp_model_select.
// include/relpose_select.h states all arithmetic.
//
//   select_kernel   grid n, 256 threads.  A thread's rows (at most 7) and their residuals under every candidate (at most 8) stay in
//              registers; every loop over candidates and rows is unrolled under uniform guards, so every index is static and nothing
//              goes to scratch.  Four stages, 34 barriers: (1) the residuals, K and the in-band counts B_c -- one reduction of 9 values;
//              (2) the exact order statistic of every candidate at once by bisection over the 32 bits of a non-negative float -- one
//              reduction of C counts per bit (counts are whole numbers below 2^24: exact in fp32, whatever the order of the sum);
//              (3) the noise scale, uniform in every thread; (4) the inlier counts and sums -- one reduction of 16 values -- then the
//              criterion, the pick and the labels.
// No atomics, no workspace, no output is read.
#include <float.h>
#include "../csrc/common.h"
#include "../csrc/block_sum.h"
#include "../csrc/two_view.h"
#include "../../include/relpose_select.h"

namespace {

constexpr int NT = BLOCK_SUM_THREADS;                // threads per workgroup
constexpr int NW = BLOCK_SUM_WAVES;
constexpr int MAXP = RP_SELECT_MAX_P;
constexpr int MAXC = RP_SELECT_MAX_C;
constexpr int ROWS = (MAXP + NT - 1) / NT;           // rows one thread owns: 7
constexpr int RED = 2 * MAXC;                        // floats per wave in the reduction buffer
constexpr float DET_MIN = 1e-30f, E_MAX = 1e30f;     // the clamps of the residual
constexpr float LN4 = 1.386294361f;                  // ln 4, and the median of chi^2_2
constexpr float MED_CHI2_1 = 0.454936423f, MED_CHI2_2 = LN4;
constexpr int BAND_MIN = 16;                         // in-band rows a candidate needs to supply the scale
constexpr int K_MIN = 8;                             // rows a problem needs
constexpr float COST_MAX = 1e6f;
constexpr int KIND_BITS = 2;                         // the kinds travel as one kernel argument, two bits per candidate

// the model table: dimension of the manifold, parameters
RP_DEV float model_dim(int kind) { return kind == 0 ? 3.f : 2.f; }
RP_DEV float model_par(int kind) { return kind == 0 ? 5.f : kind == 1 ? 8.f : 3.f; }

// the Sampson error of the two constraints m_x - u m_z = 0, m_y - v m_z = 0 of x2h ~ h x1h; front: a row with m_z not > 0 costs the maximum
RP_DEV float two_constraint_residual(const float (&h)[9], float2 p, float2 q, bool front) {
  const float m0 = h[0] * p.x + h[1] * p.y + h[2], m1 = h[3] * p.x + h[4] * p.y + h[5], m2 = h[6] * p.x + h[7] * p.y + h[8];
  const float e0 = m0 - q.x * m2, e1 = m1 - q.y * m2;
  const float a0 = h[0] - q.x * h[6], a1 = h[1] - q.x * h[7], b0 = h[3] - q.y * h[6], b1 = h[4] - q.y * h[7];
  const float mm = m2 * m2;
  const float A = (a0 * a0 + a1 * a1) + mm, B = a0 * b0 + a1 * b1, D = (b0 * b0 + b1 * b1) + mm;
  const float det = A * D - B * B;
  const float s = ((D * (e0 * e0) - (2.f * B) * (e0 * e1)) + A * (e1 * e1)) / det;
  if (!(det > DET_MIN) || (front && !(m2 > 0.f))) return E_MAX;
  return s;
}

// e2 of one row under one candidate
RP_DEV float residual(const float (&h)[9], int kind, float2 p, float2 q) {
  const float s = kind == 0 ? sampson(h, p, q) : two_constraint_residual(h, p, q, kind == 2);
  return s == s ? fabsf(fminf(fmaxf(s, 0.f), E_MAX)) : E_MAX;      // (fabsf: a -0 has the bits of the largest pattern)
}

__global__ __launch_bounds__(NT) void select_kernel(const float* __restrict__ x1, const float* __restrict__ x2, const float* __restrict__ w,
                                                     const float* __restrict__ tau, const float* __restrict__ sigma,
                                                     const float* __restrict__ models, unsigned kinds, float ocost, int* pick, float* stat,
                                                     float* scale, float* resid, int* label, int P, int C) {
  __shared__ float red[2][NW][RED];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const float2* X1 = reinterpret_cast<const float2*>(x1) + b * P;
  const float2* X2 = reinterpret_cast<const float2*>(x2) + b * P;
  const float* W = w ? w + b * P : nullptr;
  // ---- the thread's rows, once
  float2 pa[ROWS], pb[ROWS];
  bool in[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = tid + i * NT;
    pa[i] = pb[i] = make_float2(0.f, 0.f);
    in[i] = false;
    if (r < P) {
      pa[i] = X1[r];
      pb[i] = X2[r];
      in[i] = W ? W[r] > 0.f : true;                 // (false for a NaN)
    }
  }
  const float ta = tau[b], tau2 = ta * ta;
  // ---- stage 1: the residuals, K and the in-band counts
  float e[MAXC][ROWS];
  bool valid[MAXC];
  float v9[MAXC + 1];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    valid[c] = false;
    v9[c] = 0.f;
#pragma unroll
    for (int i = 0; i < ROWS; ++i) e[c][i] = E_MAX;
    if (c < C) {                                     // (uniform)
      const int kind = (kinds >> (KIND_BITS * c)) & 3;
      float h[9], ss = 0.f;
      bool ok = true;
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        h[i] = models[(b * C + c) * 9 + i];
        ok = ok && fabsf(h[i]) <= RP_FINITE;
        ss += h[i] * h[i];
      }
      const float nrm = sqrtf(ss);
      valid[c] = ok && nrm >= RP_MIN_SCALE && nrm <= RP_FINITE;
#pragma unroll
      for (int i = 0; i < ROWS; ++i) {
        const int r = tid + i * NT;
        if (r < P) {
          if (valid[c]) e[c][i] = residual(h, kind, pa[i], pb[i]);
          if (resid) resid[(b * C + c) * P + r] = e[c][i];
          v9[c] += in[i] && e[c][i] <= tau2 ? 1.f : 0.f;
        }
      }
    }
  }
  v9[MAXC] = 0.f;
#pragma unroll
  for (int i = 0; i < ROWS; ++i) v9[MAXC] += in[i] ? 1.f : 0.f;
  int phase = 0;
  block_sum(v9, red, phase);
  const float K = v9[MAXC];
  // ---- stage 2: the element of rank B_c / 2 among the in-band residuals, by bisection over the bits
  unsigned ans[MAXC];
  float rank[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    ans[c] = 0u;
    rank[c] = (float)((int)v9[c] / 2);
  }
#pragma unroll 1
  for (int bit = 31; bit >= 0; --bit) {
    float cnt[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      cnt[c] = 0.f;
      if (c < C) {
        const unsigned trial = ans[c] | (1u << bit);
#pragma unroll
        for (int i = 0; i < ROWS; ++i) cnt[c] += in[i] && e[c][i] <= tau2 && __float_as_uint(e[c][i]) < trial ? 1.f : 0.f;
      }
    }
    block_sum(cnt, red, phase);
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (cnt[c] <= rank[c]) ans[c] |= 1u << bit;
  }
  // ---- stage 3: the noise scale (uniform)
  const float sg = sigma ? sigma[b] : 0.f;
  const bool given = sg > 0.f;                       // (false for a NaN)
  float s2 = given ? sg * sg : FLT_MAX;
  int src = -1;
  bool any = false;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    if (c < C) {
      const int kind = (kinds >> (KIND_BITS * c)) & 3;
      any = any || valid[c];
      if (!given && valid[c] && v9[c] >= (float)BAND_MIN) {
        const float s2c = __uint_as_float(ans[c]) / (kind == 0 ? MED_CHI2_1 : MED_CHI2_2);
        if (s2c < s2) {
          s2 = s2c;
          src = c;
        }
      }
    }
  }
  const bool degenerate = !(K >= (float)K_MIN) || !(ta > 0.f) || !any || !(given || src >= 0);
  const float fl = ta / 1024.f;
  s2 = degenerate ? 1.f : fminf(fmaxf(s2, fl * fl), E_MAX);
  // ---- stage 4: inliers, the criterion, the pick
  float v16[2 * MAXC], thr[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int kind = (kinds >> (KIND_BITS * c)) & 3;
    thr[c] = (ocost - LN4 * model_dim(kind)) * s2;
    v16[c] = v16[MAXC + c] = 0.f;
    if (c < C) {
#pragma unroll
      for (int i = 0; i < ROWS; ++i) {
        const bool inl = in[i] && e[c][i] < thr[c];
        v16[c] += inl ? 1.f : 0.f;
        v16[MAXC + c] += inl ? e[c][i] : 0.f;
      }
    }
  }
  block_sum(v16, red, phase);
  float G[MAXC], best = FLT_MAX;
  int win = -1;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int kind = (kinds >> (KIND_BITS * c)) & 3;
    const float dL = LN4 * model_dim(kind), I = v16[c];
    G[c] = ((v16[MAXC + c] / s2 + I * dL) + (K - I) * ocost) + model_par(kind) * logf(4.f * K);
    if (c < C && valid[c] && !degenerate && G[c] < best) {
      best = G[c];
      win = c;
    }
  }
  if (label) {
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const int r = tid + i * NT;
      if (r < P) {
        int bits = 0;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C && valid[c] && !degenerate && in[i] && e[c][i] < thr[c]) bits |= 1 << c;
        label[b * P + r] = bits;
      }
    }
  }
  if (tid == 0) {
    pick[b] = win;
    scale[b * 2] = degenerate ? 0.f : sqrtf(s2);
    scale[b * 2 + 1] = degenerate ? -1.f : (float)src;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c < C) {
        const bool on = valid[c] && !degenerate;
        float* S = stat + (b * C + c) * 4;
        S[0] = on ? G[c] : FLT_MAX;
        S[1] = on ? v16[c] : 0.f;
        S[2] = on ? thr[c] : 0.f;
        S[3] = on ? v9[c] : 0.f;
      }
    }
  }
}

}  // namespace

extern "C" int rp_select_abi_version(void) { return RP_SELECT_ABI_VERSION; }

extern "C" int rp_model_select(const float* x1, const float* x2, const float* w, const float* tau, const float* sigma,
                               const float* models, const int* kinds, float outlier_cost, int* pick, float* stat, float* scale,
                               float* resid, int* label, int P, int C, int n, void* stream) {
  if (n <= 0 || P < K_MIN || C < 1 || !x1 || !x2 || !tau || !models || !kinds || !pick || !stat || !scale) return RP_EBADSHAPE;
  if (!(outlier_cost > 3.f * LN4) || !(outlier_cost <= COST_MAX)) return RP_EBADSHAPE;
  if (((uintptr_t)kinds & 3) == 0) {                 // (a misaligned host array is refused below, unread)
    for (int c = 0; c < C && c < MAXC; ++c)
      if (kinds[c] < 0 || kinds[c] > 2) return RP_EBADSHAPE;
  }
  if (P > RP_SELECT_MAX_P || C > RP_SELECT_MAX_C) return RP_EUNSUPPORTED;
  if (((uintptr_t)x1 | (uintptr_t)x2) & 7) return RP_EALIGN;
  if (((uintptr_t)w | (uintptr_t)tau | (uintptr_t)sigma | (uintptr_t)models | (uintptr_t)kinds | (uintptr_t)pick | (uintptr_t)stat |
       (uintptr_t)scale | (uintptr_t)resid | (uintptr_t)label) & 3)
    return RP_EALIGN;
  unsigned packed = 0;
  for (int c = 0; c < C; ++c) packed |= (unsigned)kinds[c] << (KIND_BITS * c);
  hipLaunchKernelGGL(select_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, x1, x2, w, tau, sigma, models, packed, outlier_cost, pick,
                     stat, scale, resid, label, P, C);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
