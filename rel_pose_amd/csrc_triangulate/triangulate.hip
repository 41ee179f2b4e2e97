// triangulate.hip -- rp_triangulate: optimal correction and triangulation of the matches under a given pose (librelpose_triangulate.so).
//
// One workgroup of 256 threads per problem, one launch; include/relpose_triangulate.h states the arithmetic.
//   data     thread t owns the rows t, t + 256, .. (at most 7).  Their points and base weights are read from global memory first, all
//            of them (5 floats x 7 rows in registers), so the loads of a thread are in flight together; rows past P carry weight 0.
//   pass     ONE pass over the row slots in use, WITHOUT unrolling (the layout of csrc_refine/refine_pose.hip): Lindstrom's two steps,
//            the ray intersection, the parallax, the stores of the row, and the row's six terms of `stat`
//   reduce   ONE fused six-value block_sum: sum w, the count of positive w, sum w tau^2 log1p(d2 / tau^2), sum o, sum o [in front],
//            sum o phi
//   finish   thread 0 stores stat
// No atomics, no workspace, no matrix instruction; nothing is read from an output.  Every loop has a fixed trip count.
#include "../csrc/common.h"
#include "../csrc/block_sum.h"
#include "../csrc/two_view.h"
#include "../../include/relpose_triangulate.h"

namespace {

constexpr int NT = BLOCK_SUM_THREADS;                // threads per workgroup
constexpr int NW = BLOCK_SUM_WAVES;
constexpr int MAXP = RP_TRIANGULATE_MAX_P;
constexpr int ROWS = (MAXP + NT - 1) / NT;           // rows one thread owns: 7
constexpr int RED = 6;                               // floats per wave in the reduction buffer
constexpr float MIN_NORM = 1e-30f;                   // |t| or |q| below this: degenerate
constexpr float MIN_DEN = 1e-30f;                    // a denominator of the correction not above this: lambda = 0
constexpr float INF_SIN2 = 1e-10f;                   // |g|^2 below this times |x2ch|^2 |r|^2: the row is at infinity

__global__ __launch_bounds__(NT) void triangulate_kernel(const float* __restrict__ pose, const float* __restrict__ x1,
                                                          const float* __restrict__ x2, const float* __restrict__ w,
                                                          const float* __restrict__ tau, float* __restrict__ X, float* __restrict__ aux,
                                                          float* __restrict__ xc, float* __restrict__ stat, int P) {
  __shared__ float red[2][NW][RED];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const float2* X1 = reinterpret_cast<const float2*>(x1) + b * P;
  const float2* X2 = reinterpret_cast<const float2*>(x2) + b * P;
  const float* W = w ? w + b * P : nullptr;
  float* XO = X + b * P * 3;
  float* AO = aux + b * P * 4;
  float* CO = xc ? xc + b * P * 4 : nullptr;
  // ---- the thread's rows, once
  float ax[ROWS], ay[ROWS], bx[ROWS], by[ROWS], wt[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = tid + i * NT;
    ax[i] = ay[i] = bx[i] = by[i] = wt[i] = 0.f;
    if (r < P) {
      const float2 a = X1[r], c = X2[r];
      ax[i] = a.x; ay[i] = a.y; bx[i] = c.x; by[i] = c.y;
      wt[i] = W ? fmaxf(W[r], 0.f) : 1.f;
    }
  }
  const int nrows = (P + NT - 1) / NT;             // row slots in use (uniform)
  float p0[7], t[3], q[4];
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    p0[i] = pose[b * 7 + i];
    finite = finite && fabsf(p0[i]) <= RP_FINITE;
  }
  const float t0[3] = {p0[0], p0[1], p0[2]}, q0[4] = {p0[3], p0[4], p0[5], p0[6]};
  const float tn = unit(t0, t), qn = unit(q0, q);
  const float ta = tau[b];
  const bool degenerate = !finite || !(tn >= MIN_NORM) || !(qn >= MIN_NORM) || !(ta > 0.f);
  float tau2 = ta * ta;
  if (degenerate) {                                // (uniform) arithmetic below stays finite; of its results only K is used
    t[0] = 1.f; t[1] = t[2] = 0.f;
    q[0] = q[1] = q[2] = 0.f; q[3] = 1.f;
    tau2 = 1.f;
  }
  float R[9], e[9];
  quat_to_rot(q, R);
  cross_times(t, R, e);
  float s[RED];
#pragma unroll
  for (int i = 0; i < RED; ++i) s[i] = 0.f;
#pragma unroll 1
  for (int i = 0; i < nrows; ++i) {
    const int r = tid + i * NT;
    const float x = ax[i], y = ay[i], u = bx[i], v = by[i];
    // ---- the optimal correction: m = (E x1h)_xy, mp = (E^T x2h)_xy, c = x2h^T E x1h
    float m0 = e[0] * x + e[1] * y + e[2];
    float m1 = e[3] * x + e[4] * y + e[5];
    const float mz = e[6] * x + e[7] * y + e[8];
    float mp0 = e[0] * u + e[3] * v + e[6];
    float mp1 = e[1] * u + e[4] * v + e[7];
    const float c = u * m0 + v * m1 + mz;
    const float a = m0 * (e[0] * mp0 + e[1] * mp1) + m1 * (e[3] * mp0 + e[4] * mp1);
    const float hb = 0.5f * ((m0 * m0 + m1 * m1) + (mp0 * mp0 + mp1 * mp1));
    const float d = sqrtf(fmaxf(hb * hb - a * c, 0.f));
    const float den = hb + d;
    float lam = den > MIN_DEN ? c / den : 0.f;
    float d2x = lam * m0, d2y = lam * m1, d1x = lam * mp0, d1y = lam * mp1;
    m0 = m0 - (e[0] * d1x + e[1] * d1y);
    m1 = m1 - (e[3] * d1x + e[4] * d1y);
    mp0 = mp0 - (e[0] * d2x + e[3] * d2y);
    mp1 = mp1 - (e[1] * d2x + e[4] * d2y);
    const float den2 = (m0 * m0 + m1 * m1) + (mp0 * mp0 + mp1 * mp1);
    lam = den2 > MIN_DEN ? lam * (2.f * d) / den2 : 0.f;
    d2x = lam * m0; d2y = lam * m1; d1x = lam * mp0; d1y = lam * mp1;
    const float xa[3] = {x - d1x, y - d1y, 1.f}, xb[3] = {u - d2x, v - d2y, 1.f};
    const float dd = (d1x * d1x + d1y * d1y) + (d2x * d2x + d2y * d2y);
    // ---- the point
    float rr[3], g[3], txb[3], txr[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) rr[k] = (R[3 * k] * xa[0] + R[3 * k + 1] * xa[1]) + R[3 * k + 2];
    cross(xb, rr, g);
    cross(t, xb, txb);
    cross(t, rr, txr);
    const float gg = dot(g, g), nb = dot(xb, xb), nr = dot(rr, rr);
    const float phi = atan2f(sqrtf(gg), dot(xb, rr));
    const bool far = gg < INF_SIN2 * nb * nr;
    const float z1 = far ? 0.f : dot(txb, g) / gg;
    const float z2 = far ? 0.f : dot(txr, g) / gg;
    const float om = wt[i] / (1.f + dd / tau2);
    s[0] += wt[i];
    s[1] += wt[i] > 0.f ? 1.f : 0.f;
    s[2] += wt[i] * (tau2 * log1pf(dd / tau2));
    s[3] += om;
    s[4] += (z1 > 0.f && z2 > 0.f) ? om : 0.f;
    s[5] += om * phi;
    if (r < P) {
      const bool z = degenerate;                   // (uniform) a degenerate problem writes zeros, through the same stores
      XO[3 * r] = z ? 0.f : z1 * xa[0]; XO[3 * r + 1] = z ? 0.f : z1 * xa[1]; XO[3 * r + 2] = z ? 0.f : z1;
      AO[4 * r] = z ? 0.f : z1; AO[4 * r + 1] = z ? 0.f : z2; AO[4 * r + 2] = z ? 0.f : dd; AO[4 * r + 3] = z ? 0.f : phi;
      if (CO) {
        CO[4 * r] = z ? 0.f : xa[0]; CO[4 * r + 1] = z ? 0.f : xa[1]; CO[4 * r + 2] = z ? 0.f : xb[0]; CO[4 * r + 3] = z ? 0.f : xb[1];
      }
    }
  }
  int phase = 0;
  block_sum(s, red, phase);
  if (tid == 0) {
    const bool any = !degenerate && s[0] > 0.f;
    const bool some = any && s[3] > 0.f;
    stat[b * 4] = any ? s[2] / s[0] : 0.f;
    stat[b * 4 + 1] = some ? s[4] / s[3] : 0.f;
    stat[b * 4 + 2] = some ? s[5] / s[3] : 0.f;
    stat[b * 4 + 3] = s[1];
  }
}

}  // namespace

extern "C" int rp_triangulate_abi_version(void) { return RP_TRIANGULATE_ABI_VERSION; }

extern "C" int rp_triangulate(const float* pose, const float* x1, const float* x2, const float* w, const float* tau, float* X,
                              float* aux, float* xc, float* stat, int P, int n, void* stream) {
  if (n <= 0 || P < 1 || !pose || !x1 || !x2 || !tau || !X || !aux || !stat) return RP_EBADSHAPE;
  if (P > RP_TRIANGULATE_MAX_P) return RP_EUNSUPPORTED;
  if (((uintptr_t)x1 | (uintptr_t)x2) & 7) return RP_EALIGN;
  if (((uintptr_t)pose | (uintptr_t)w | (uintptr_t)tau | (uintptr_t)X | (uintptr_t)aux | (uintptr_t)xc | (uintptr_t)stat) & 3)
    return RP_EALIGN;
  hipLaunchKernelGGL(triangulate_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, pose, x1, x2, w, tau, X, aux, xc, stat, P);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
