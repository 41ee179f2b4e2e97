// refine_pose.hip -- rp_refine_pose: Levenberg-Marquardt refinement of a two-view pose on the essential manifold (librelpose_refine.so).
//
// One workgroup of 256 threads per problem, the whole iteration in one launch; include/relpose_refine.h states the iteration.
//   data     thread t owns the rows t, t + 256, .. (at most 7).  Their points and base weights are read from global memory ONCE and stay
//            in registers for the launch (5 floats x 7 rows); rows past P carry weight 0.  LDS holds the reduction buffer and nothing else.
//            The passes loop over the row slots in use WITHOUT unrolling (the slot index is uniform, the compiler keeps the five small
//            arrays in vector registers): unrolled seven times the passes need about 400 registers, rolled 254 and no scratch.
//   start    one three-value reduction: the sum of the weights, the count of positive ones, the cost at the start
//   per iteration, TWO barriers:
//     pass 1   residual s, exact Jacobian J [5] and Cauchy weight o of every owned row; the 15 upper entries of H = sum o J J^T and the
//              5 of g = sum o J s in ONE fused 20-value reduction
//     solve    (H + lambda diag H) delta = -g: diagonal scaling, 5 x 5 Cholesky (csrc/two_view.h), the retraction -- in every thread,
//              redundantly: the sums are bit-identical in all 256 threads (csrc/block_sum.h), so the breakdown and accept decisions
//              are uniform
//     pass 2   the cost at the trial pose: one one-value reduction
//   finish   the weights at the output pose (if asked for); thread 0 stores pose, E and stat
// No atomics, no workspace; nothing is read from an output.  pose may alias pose0: every thread has read pose0 before the first
// barrier, thread 0 writes pose behind the last.
#include "../csrc/common.h"
#include "../csrc/block_sum.h"
#include "../csrc/two_view.h"
#include "../../include/relpose_refine.h"

namespace {

constexpr int NT = BLOCK_SUM_THREADS;                // threads per workgroup
constexpr int NW = BLOCK_SUM_WAVES;
constexpr int MAXP = RP_REFINE_MAX_P;
constexpr int ROWS = (MAXP + NT - 1) / NT;           // rows one thread owns: 7
constexpr int RED = 20;                              // floats per wave in the reduction buffer: 15 of H + 5 of g
constexpr float MIN_NORM = 1e-30f;                   // |t0| or |q0| below this: degenerate
constexpr float LAMBDA0 = 1e-3f, LAMBDA_MIN = 1e-7f, LAMBDA_MAX = 1e7f;

// the basis of the tangent plane at the unit vector t: e_k of the smallest |t_k| (the lowest index on ties), b1 = normalise(e_k x t),
// b2 = t x b1
RP_DEV void tangent_basis(const float (&t)[3], float (&b1)[3], float (&b2)[3]) {
  const float a0 = fabsf(t[0]), a1 = fabsf(t[1]), a2 = fabsf(t[2]);
  int k = a1 < a0 ? 1 : 0;
  k = a2 < (k ? a1 : a0) ? 2 : k;
  float c[3];
  c[0] = k == 0 ? 0.f : k == 1 ? t[2] : -t[1];
  c[1] = k == 0 ? -t[2] : k == 1 ? 0.f : t[0];
  c[2] = k == 0 ? t[1] : k == 1 ? -t[0] : 0.f;
  const float s = sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) b1[i] = c[i] / s;
  b2[0] = t[1] * b1[2] - t[2] * b1[1];
  b2[1] = t[2] * b1[0] - t[0] * b1[2];
  b2[2] = t[0] * b1[1] - t[1] * b1[0];
}

// (m x1)_x, (m x1)_y, (m^T x2)_x, (m^T x2)_y and x2^T m x1 for a row-major 3 x 3 m and homogeneous points (x, y, 1)
struct Lines {
  float l2x, l2y, l1x, l1y, r;
};
RP_DEV Lines lines(const float (&m)[9], float ax, float ay, float bx, float by) {
  Lines o;
  o.l2x = m[0] * ax + m[1] * ay + m[2];
  o.l2y = m[3] * ax + m[4] * ay + m[5];
  const float l2z = m[6] * ax + m[7] * ay + m[8];
  o.l1x = m[0] * bx + m[3] * by + m[6];
  o.l1y = m[1] * bx + m[4] * by + m[7];
  o.r = bx * o.l2x + by * o.l2y + l2z;
  return o;
}

// s = x2^T E x1 / sqrt(den), 0 where den is 0; inv = 1 / sqrt(den), 0 there
RP_DEV float residual(const Lines& l, float& inv) {
  const float den = l.l2x * l.l2x + l.l2y * l.l2y + l.l1x * l.l1x + l.l1y * l.l1y;
  inv = den > 0.f ? 1.f / sqrtf(den) : 0.f;
  return l.r * inv;
}

// the trial pose of the header: q (x) (omega sin(theta / 2) / theta, cos(theta / 2)) and t + b1 beta_1 + b2 beta_2, both normalised
RP_DEV void retract(const float (&t)[3], const float (&q)[4], const float (&b1)[3], const float (&b2)[3], const float (&d)[5],
                    float (&t1)[3], float (&q1)[4]) {
  const float th = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  const float k = th < 1e-4f ? 0.5f - th * th / 48.f : sinf(0.5f * th) / th;
  const float pw = cosf(0.5f * th), p0 = d[0] * k, p1 = d[1] * k, p2 = d[2] * k;
  float nq[4];
  nq[0] = (q[3] * p0 + pw * q[0]) + (q[1] * p2 - q[2] * p1);
  nq[1] = (q[3] * p1 + pw * q[1]) + (q[2] * p0 - q[0] * p2);
  nq[2] = (q[3] * p2 + pw * q[2]) + (q[0] * p1 - q[1] * p0);
  nq[3] = q[3] * pw - ((q[0] * p0 + q[1] * p1) + q[2] * p2);
  const float qn = sqrtf(((nq[0] * nq[0] + nq[1] * nq[1]) + nq[2] * nq[2]) + nq[3] * nq[3]);
#pragma unroll
  for (int i = 0; i < 4; ++i) q1[i] = nq[i] / qn;
  float nt[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) nt[i] = (t[i] + b1[i] * d[3]) + b2[i] * d[4];
  const float tn = sqrtf((nt[0] * nt[0] + nt[1] * nt[1]) + nt[2] * nt[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) t1[i] = nt[i] / tn;
}

__global__ __launch_bounds__(NT) void refine_pose_kernel(const float* pose0, const float* __restrict__ x1, const float* __restrict__ x2,
                                                          const float* __restrict__ w, const float* __restrict__ tau, float* pose, float* E,
                                                          float* stat, float* w_out, int P, int iters) {
  __shared__ float red[2][NW][RED];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const float2* X1 = reinterpret_cast<const float2*>(x1) + b * P;
  const float2* X2 = reinterpret_cast<const float2*>(x2) + b * P;
  const float* W = w ? w + b * P : nullptr;
  float* WO = w_out ? w_out + b * P : nullptr;
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
#pragma unroll
  for (int i = 0; i < 7; ++i) p0[i] = pose0[b * 7 + i];
  const float t0[3] = {p0[0], p0[1], p0[2]}, q0[4] = {p0[3], p0[4], p0[5], p0[6]};
  const float tn = unit(t0, t), qn = unit(q0, q);
  const float ta = tau[b], tau2 = ta * ta;
  bool degenerate = !(tn >= MIN_NORM) || !(qn >= MIN_NORM) || !(ta > 0.f);
  if (degenerate) {                                // (uniform) arithmetic below stays finite; its results are not used
    t[0] = 1.f; t[1] = t[2] = 0.f;
    q[0] = q[1] = q[2] = 0.f; q[3] = 1.f;
  }
  float R[9], e[9];
  quat_to_rot(q, R);
  cross_times(t, R, e);
  int phase = 0;
  // ---- start: sum of the weights, count of the positive ones, cost
  float s3[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
  for (int i = 0; i < nrows; ++i) {
    {
      float inv;
      const float s = residual(lines(e, ax[i], ay[i], bx[i], by[i]), inv);
      s3[0] += wt[i];
      s3[1] += wt[i] > 0.f ? 1.f : 0.f;
      s3[2] += wt[i] * (tau2 * log1pf(s * s / tau2));
    }
  }
  block_sum(s3, red, phase);
  const float wsum = s3[0];
  degenerate = degenerate || s3[1] < 5.f;
  if (degenerate) {
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const int r = tid + i * NT;
      if (WO && r < P) WO[r] = wt[i];
    }
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < 7; ++i) pose[b * 7 + i] = p0[i];
#pragma unroll
      for (int i = 0; i < 9; ++i) E[b * 9 + i] = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) stat[b * 4 + i] = 0.f;
    }
    return;
  }
  const float c0 = s3[2] / wsum;
  float c = c0, lam = LAMBDA0, accepted = 0.f, last = 0.f;
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    // ---- the frame at the pose: E and the five derivative matrices D_k (the first three are columns of E, the compiler folds them)
    float b1[3], b2[3], D[5][9];
    quat_to_rot(q, R);
    cross_times(t, R, e);
    tangent_basis(t, b1, b2);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      D[0][3 * r] = 0.f;           D[0][3 * r + 1] = e[3 * r + 2]; D[0][3 * r + 2] = -e[3 * r + 1];
      D[1][3 * r] = -e[3 * r + 2]; D[1][3 * r + 1] = 0.f;          D[1][3 * r + 2] = e[3 * r];
      D[2][3 * r] = e[3 * r + 1];  D[2][3 * r + 1] = -e[3 * r];    D[2][3 * r + 2] = 0.f;
    }
    cross_times(b1, R, D[3]);
    cross_times(b2, R, D[4]);
    // ---- pass 1: H and g
    float a[RED];
#pragma unroll
    for (int i = 0; i < RED; ++i) a[i] = 0.f;
#pragma unroll 1
    for (int i = 0; i < nrows; ++i) {
      {
        const Lines l = lines(e, ax[i], ay[i], bx[i], by[i]);
        float inv;
        const float s = residual(l, inv);
        const float om = wt[i] / (1.f + s * s / tau2);
        float J[5], oJ[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const Lines d = lines(D[k], ax[i], ay[i], bx[i], by[i]);
          const float half = l.l2x * d.l2x + l.l2y * d.l2y + l.l1x * d.l1x + l.l1y * d.l1y;
          J[k] = (d.r - s * half * inv) * inv;
          oJ[k] = om * J[k];
        }
        int m = 0;
#pragma unroll
        for (int u = 0; u < 5; ++u)
#pragma unroll
          for (int v = u; v < 5; ++v) a[m++] += oJ[u] * J[v];
#pragma unroll
        for (int u = 0; u < 5; ++u) a[15 + u] += oJ[u] * s;
      }
    }
    block_sum(a, red, phase);
    // ---- the step and the trial pose (uniform)
    float delta[5], t1[3], q1[4], e1[9];
    const bool solved = lm_cholesky_solve(a, lam, delta);
    if (!solved) {
#pragma unroll
      for (int i = 0; i < 5; ++i) delta[i] = 0.f;
    }
    retract(t, q, b1, b2, delta, t1, q1);
    quat_to_rot(q1, R);
    cross_times(t1, R, e1);
    // ---- pass 2: the trial cost
    float c1[1] = {0.f};
#pragma unroll 1
    for (int i = 0; i < nrows; ++i) {
      {
        float inv;
        const float s = residual(lines(e1, ax[i], ay[i], bx[i], by[i]), inv);
        c1[0] += wt[i] * (tau2 * log1pf(s * s / tau2));
      }
    }
    block_sum(c1, red, phase);
    const float ct = c1[0] / wsum;
    if (solved && ct < c) {
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = t1[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] = q1[i];
      c = ct;
      lam = fmaxf(lam / 10.f, LAMBDA_MIN);
      accepted += 1.f;
      last = sqrtf((((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2]) + delta[3] * delta[3]) + delta[4] * delta[4]);
    } else {
      lam = fminf(lam * 10.f, LAMBDA_MAX);
    }
  }
  // ---- finish
  if (q[3] < 0.f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = -q[i];
  }
  quat_to_rot(q, R);
  cross_times(t, R, e);
  if (WO) {
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const int r = tid + i * NT;
      if (r < P) {
        float inv;
        const float s = residual(lines(e, ax[i], ay[i], bx[i], by[i]), inv);
        WO[r] = wt[i] / (1.f + s * s / tau2);
      }
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) pose[b * 7 + i] = t[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) pose[b * 7 + 3 + i] = q[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) E[b * 9 + i] = e[i];
    stat[b * 4] = c0; stat[b * 4 + 1] = c; stat[b * 4 + 2] = accepted; stat[b * 4 + 3] = last;
  }
}

}  // namespace

extern "C" int rp_refine_abi_version(void) { return RP_REFINE_ABI_VERSION; }

extern "C" int rp_refine_pose(const float* pose0, const float* x1, const float* x2, const float* w, const float* tau, float* pose,
                              float* E, float* stat, float* w_out, int P, int iters, int n, void* stream) {
  if (n <= 0 || P < 5 || iters < 0 || !pose0 || !x1 || !x2 || !tau || !pose || !E || !stat) return RP_EBADSHAPE;
  if (P > RP_REFINE_MAX_P || iters > RP_REFINE_MAX_ITERS) return RP_EUNSUPPORTED;
  if (((uintptr_t)x1 | (uintptr_t)x2) & 7) return RP_EALIGN;
  if (((uintptr_t)pose0 | (uintptr_t)w | (uintptr_t)tau | (uintptr_t)pose | (uintptr_t)E | (uintptr_t)stat | (uintptr_t)w_out) & 3)
    return RP_EALIGN;
  hipLaunchKernelGGL(refine_pose_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, pose0, x1, x2, w, tau, pose, E, stat, w_out, P, iters);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
