// covariance.hip -- rp_pose_covariance: the sandwich covariance A^-1 B A^-1 of a refined two-view pose (librelpose_covariance.so).
//
// One workgroup of 256 threads per problem, one launch; include/relpose_covariance.h states every step.
//   data     thread t owns the rows t, t + 256, .. (at most 7) and reads their points and base weights from global memory ONCE, as
//            csrc_refine/refine_pose.hip does; rows past P carry weight 0.  LDS holds the reduction buffer and nothing else.
//   pass     residual s, exact Jacobian J [5], influence psi and its derivative psi' of every owned row; the 15 upper entries of
//            A = sum psi' J J^T, the 15 of B = sum psi^2 J J^T and four scalars (sum w, rows of positive weight, rows with psi' < 0, the
//            robust cost) in ONE fused 34-value reduction, one barrier.  The loop over the row slots is NOT unrolled, for the reason
//            refine_pose.hip gives: the slot index is uniform, the five small arrays stay in vector registers, and unrolled seven times
//            the pass needs several hundred registers.
//   algebra  the scaling, the 5 x 5 Cholesky, the inverse, the sandwich product and the Jacobi sweeps (sym5.h) run in THREAD 0 ALONE.
//            The sums are bit-identical in all 256 threads (csrc/block_sum.h), so running them everywhere would be uniform, too -- but
//            nothing behind the reduction needs the result in another thread: there is no second pass over the rows, no further barrier
//            and no per-row output, and thread 0 stores everything.  Redundant execution would cost the same time in wave 0 and keep
//            the other three waves busy for nothing; this way they retire at the barrier.
// No atomics, no workspace, no matrix instruction, no inline assembly; nothing is read from an output.
#include "../csrc/common.h"
#include "../csrc/block_sum.h"
#include "../csrc/two_view.h"
#include "../../include/relpose_covariance.h"
#include "sym5.h"

namespace {

constexpr int NT = BLOCK_SUM_THREADS;                // threads per workgroup
constexpr int NW = BLOCK_SUM_WAVES;
constexpr int MAXP = RP_COVARIANCE_MAX_P;
constexpr int ROWS = (MAXP + NT - 1) / NT;           // rows one thread owns: 7
constexpr int RED = 34;                              // floats per wave in the reduction buffer: 15 of A + 15 of B + 4 scalars
constexpr float MIN_NORM = 1e-30f;                   // |t| or |q| below this: degenerate
constexpr float K_MIN = 6.f;                         // fewer rows of positive weight: degenerate

// (m x1)_x, (m x1)_y, (m^T x2)_x, (m^T x2)_y and x2^T m x1 for a row-major 3 x 3 m and homogeneous points (x, y, 1), as refine_pose.hip
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

__global__ __launch_bounds__(NT) void pose_covariance_kernel(const float* __restrict__ pose, const float* __restrict__ x1,
                                                              const float* __restrict__ x2, const float* __restrict__ w,
                                                              const float* __restrict__ tau, float* __restrict__ cov,
                                                              float* __restrict__ frame, float* __restrict__ eig, float* __restrict__ weak,
                                                              float* __restrict__ stat, float* __restrict__ normal, int P) {
  __shared__ float red[2][NW][RED];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const float2* X1 = reinterpret_cast<const float2*>(x1) + b * P;
  const float2* X2 = reinterpret_cast<const float2*>(x2) + b * P;
  const float* W = w ? w + b * P : nullptr;
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
  const int nrows = (P + NT - 1) / NT;               // row slots in use (uniform)
  // ---- the pose and its frame (uniform)
  float p0[7], t[3], q[4];
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    p0[i] = pose[b * 7 + i];
    finite = finite && fabsf(p0[i]) <= RP_FINITE;
  }
  const float t0[3] = {p0[0], p0[1], p0[2]}, q0[4] = {p0[3], p0[4], p0[5], p0[6]};
  const float tn = unit_exact(t0, t), qn = unit_exact(q0, q);
  const float ta = tau[b], tau2 = ta * ta;
  bool degenerate = !finite || !(tn >= MIN_NORM) || !(qn >= MIN_NORM) || !(ta > 0.f);
  if (degenerate) {                                  // (uniform) arithmetic below stays finite; its results are not used
    t[0] = 1.f; t[1] = t[2] = 0.f;
    q[0] = q[1] = q[2] = 0.f; q[3] = 1.f;
  }
  float R[9], e[9], b1[3], b2[3], D[5][9];
  quat_to_rot(q, R);
  cross_times(t, R, e);
  tangent_basis_exact(t, b1, b2);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    D[0][3 * r] = 0.f;           D[0][3 * r + 1] = e[3 * r + 2]; D[0][3 * r + 2] = -e[3 * r + 1];
    D[1][3 * r] = -e[3 * r + 2]; D[1][3 * r + 1] = 0.f;          D[1][3 * r + 2] = e[3 * r];
    D[2][3 * r] = e[3 * r + 1];  D[2][3 * r + 1] = -e[3 * r];    D[2][3 * r + 2] = 0.f;
  }
  cross_times(b1, R, D[3]);
  cross_times(b2, R, D[4]);
  // ---- the pass: A, B and the four scalars
  float a[RED];
#pragma unroll
  for (int i = 0; i < RED; ++i) a[i] = 0.f;
#pragma unroll 1
  for (int i = 0; i < nrows; ++i) {
    {
      const Lines l = lines(e, ax[i], ay[i], bx[i], by[i]);
      float inv;
      const float s = residual(l, inv);
      const float u = s * s / tau2, qq = 1.f + u;
      const float psi = wt[i] * s / qq, dpsi = wt[i] * (1.f - u) / (qq * qq), psi2 = psi * psi;
      float J[5], pJ[5], bJ[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const Lines d = lines(D[k], ax[i], ay[i], bx[i], by[i]);
        const float half = l.l2x * d.l2x + l.l2y * d.l2y + l.l1x * d.l1x + l.l1y * d.l1y;
        J[k] = (d.r - s * half * inv) * inv;
        pJ[k] = dpsi * J[k];
        bJ[k] = psi2 * J[k];
      }
      int m = 0;
#pragma unroll
      for (int u_ = 0; u_ < 5; ++u_)
#pragma unroll
        for (int v = u_; v < 5; ++v) {
          a[m] += pJ[u_] * J[v];
          a[15 + m] += bJ[u_] * J[v];
          ++m;
        }
      a[30] += wt[i];
      a[31] += wt[i] > 0.f ? 1.f : 0.f;
      a[32] += dpsi < 0.f ? 1.f : 0.f;
      a[33] += wt[i] * (tau2 * log1pf(s * s / tau2));
    }
  }
  int phase = 0;
  block_sum(a, red, phase);
  if (tid != 0) return;                              // the algebra and every store: thread 0 (see the head of the file)
  // ---- thread 0
  bool sums = true;
#pragma unroll
  for (int i = 0; i < RED; ++i) sums = sums && fabsf(a[i]) <= RP_FINITE;
  degenerate = degenerate || !sums || a[31] < K_MIN;
  float* COV = cov + b * 25;
  float* FR = frame + b * 6;
  float* EG = eig + b * 5;
  float* WK = weak + b * 5;
  float* ST = stat + b * 8;
  float* NM = normal ? normal + b * 30 : nullptr;
  if (degenerate) {
#pragma unroll
    for (int i = 0; i < 25; ++i) COV[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) FR[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) EG[i] = WK[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) ST[i] = 0.f;
    if (NM) {
#pragma unroll
      for (int i = 0; i < 30; ++i) NM[i] = 0.f;
    }
    return;
  }
  float ab[30];
#pragma unroll
  for (int i = 0; i < 30; ++i) ab[i] = a[i];
  float C[5][5], ev[5], wk[5], rho;
  const bool ok = sandwich5(ab, C, rho);
  float sd_rot = 0.f, sd_dir = 0.f;
  if (ok) {
    jacobi5(C, ev, wk);
    sd_rot = sqrtf(fmaxf((C[0][0] + C[1][1]) + C[2][2], 0.f));
    sd_dir = sqrtf(fmaxf(C[3][3] + C[4][4], 0.f));
  } else {
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      ev[i] = wk[i] = 0.f;
#pragma unroll
      for (int j = 0; j < 5; ++j) C[i][j] = 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = 0; j < 5; ++j) COV[5 * i + j] = C[i][j];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    FR[i] = b1[i];
    FR[3 + i] = b2[i];
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    EG[i] = ev[i];
    WK[i] = wk[i];
  }
  ST[0] = ok ? 1.f : -1.f; ST[1] = a[31]; ST[2] = sd_rot; ST[3] = sd_dir;
  ST[4] = rho; ST[5] = a[32]; ST[6] = a[33] / a[30]; ST[7] = 0.f;
  if (NM) {
#pragma unroll
    for (int i = 0; i < 30; ++i) NM[i] = a[i];
  }
}

}  // namespace

extern "C" int rp_covariance_abi_version(void) { return RP_COVARIANCE_ABI_VERSION; }

extern "C" int rp_pose_covariance(const float* pose, const float* x1, const float* x2, const float* w, const float* tau, float* cov,
                                  float* frame, float* eig, float* weak, float* stat, float* normal, int P, int n, void* stream) {
  if (n <= 0 || P < 6 || !pose || !x1 || !x2 || !tau || !cov || !frame || !eig || !weak || !stat) return RP_EBADSHAPE;
  if (P > RP_COVARIANCE_MAX_P) return RP_EUNSUPPORTED;
  if (((uintptr_t)x1 | (uintptr_t)x2) & 7) return RP_EALIGN;
  if (((uintptr_t)pose | (uintptr_t)w | (uintptr_t)tau | (uintptr_t)cov | (uintptr_t)frame | (uintptr_t)eig | (uintptr_t)weak |
       (uintptr_t)stat | (uintptr_t)normal) & 3)
    return RP_EALIGN;
  hipLaunchKernelGGL(pose_covariance_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, pose, x1, x2, w, tau, cov, frame, eig, weak, stat,
                     normal, P);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
