// resection.hip -- camera resection against the structure of a pair (librelpose_resection.so): rp_p3p_consensus, rp_pnp_refine.
// include/relpose_resection.h states all arithmetic.
//
//   hypothesis_kernel   grid n * ceil(M / 256) (problem-major), 256 threads: the staging of csrc/consensus_core.h as it is (flags, ordered
//              prefix, compacted rows in LDS; four barriers) with the image as BOTH of its float2 operands, the 3-D points of the same rows
//              gathered into an array of this file (one more barrier), then one lane per hypothesis: Floyd's three draws (the core),
//              Grunert's quartic by Ferrari's closed form in fp64 (fixed trip counts, static indices), up
//              to four poses, and ONE walk over the K compacted rows (LDS broadcast reads) with one running sum per solution.
//   select_kernel       grid n, 256 threads: the lowest-index argmin of hyp_cost (a min tree in LDS over 64-bit keys (cost bits, index):
//              the core's select is typed on two float2 operands and a 3 x 3 model), w_out and stat at the winner.
//   refine_kernel       grid n, 256 threads: Levenberg-Marquardt over the six parameters of a left rotation increment and a translation
//              increment.  A thread's rows (at most 7) stay in registers; per iteration ONE fused 27-value reduction (21 of the normal
//              matrix, 6 of the gradient), the 6 x 6 Cholesky (csrc/two_view.h) and the retraction redundantly in every thread, one
//              one-value reduction for the trial cost: two barriers.
// No atomics, no workspace; the only output that is read is hyp_cost / hyp_pose, by select_kernel after hypothesis_kernel wrote all of it.
#include <float.h>
#include "../csrc/common.h"
#include "../csrc/block_sum.h"
#include "../csrc/two_view.h"
#include "../csrc/consensus_core.h"
#include "../../include/relpose_resection.h"

namespace {

constexpr int NT = BLOCK_SUM_THREADS;                // threads per workgroup
constexpr int NW = BLOCK_SUM_WAVES;
constexpr int MAXP = RP_RESECTION_MAX_P;
constexpr int ROWS = (MAXP + NT - 1) / NT;           // rows one thread stages / owns: 7
constexpr int RED = 4;                               // floats per wave in the reduction buffer of select_kernel
constexpr int NPAR = 6;                              // degrees of freedom of a pose
constexpr int NTRI = NPAR * (NPAR + 1) / 2;          // 21
constexpr int LMRED = NTRI + NPAR;                   // 27: the upper triangle of the normal matrix and the gradient
constexpr int NSOL = 4;                              // solutions of a sample, at most
constexpr float DEN_MIN = 1e-30f, D_MAX = 1e30f;     // the clamps of the distance
constexpr float LAMBDA0 = 1e-3f, LAMBDA_MIN = 1e-7f, LAMBDA_MAX = 1e7f;
constexpr double SIDE_MIN = 1e-12, AREA_MIN = 1e-12, SPAN_MIN = 1e-12, LEAD_MIN = 1e-12, DEN_V_MIN = 1e-9, DISC_BAND = 1e-9,
                 RESOLVENT_MIN = 1e-14, FINITE64 = 1e300;

// m = R X + t and the distance of the header
RP_DEV float pose_distance(const float (&R)[9], const float (&t)[3], float X, float Y, float Z, float u, float v) {
  const float m0 = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0], m1 = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1],
              m2 = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2];
  const float ex = m0 - u * m2, ey = m1 - v * m2, den = m2 * m2;
  const float d = fminf((ex * ex + ey * ey) / fmaxf(den, DEN_MIN), D_MAX);
  return m2 > 0.f && den >= DEN_MIN ? d : D_MAX;
}

// the bits of a float (a cost >= +0 orders as they do)
RP_DEV uint32_t float_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}

// ---- fp64 helpers of the lane solver
RP_DEV double dot64(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

RP_DEV void cross64(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

RP_DEV void unit64(const double (&a)[3], double (&u)[3]) {
  const double s = sqrt(dot64(a, a));
#pragma unroll
  for (int i = 0; i < 3; ++i) u[i] = a[i] / s;
}

// the frame of three points: e[0] along p1 - p0, e[2] along e[0] x (p2 - p0), e[1] = e[2] x e[0]
RP_DEV void frame64(const double (&p0)[3], const double (&p1)[3], const double (&p2)[3], double (&e)[3][3]) {
  const double d1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, d2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  unit64(d1, e[0]);
  double c[3];
  cross64(e[0], d2, c);
  unit64(c, e[2]);
  cross64(e[2], e[0], e[1]);
}

// rot_to_quat of csrc/two_view.h in fp64
RP_DEV void rot_to_quat64(const double (&R)[9], double (&q)[4]) {
  const double tr = R[0] + R[4] + R[8];
  double v[4];
  if (tr > 0.) {
    v[3] = 1. + tr; v[0] = R[7] - R[5]; v[1] = R[2] - R[6]; v[2] = R[3] - R[1];
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    v[0] = 1. + R[0] - R[4] - R[8]; v[3] = R[7] - R[5]; v[1] = R[1] + R[3]; v[2] = R[2] + R[6];
  } else if (R[4] >= R[8]) {
    v[1] = 1. + R[4] - R[0] - R[8]; v[3] = R[2] - R[6]; v[0] = R[1] + R[3]; v[2] = R[5] + R[7];
  } else {
    v[2] = 1. + R[8] - R[0] - R[4]; v[3] = R[3] - R[1]; v[0] = R[2] + R[6]; v[1] = R[5] + R[7];
  }
  const double nrm = sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]);
  const double s = v[3] < 0. ? -1. : 1.;
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = nrm > 0. ? s * v[i] / nrm : (i == 3 ? 1. : 0.);
}

// the two roots of z^2 + b z + c in slot order (+, -); false: no real root
RP_DEV bool quadratic(double b, double c, double& zp, double& zm) {
  double disc = b * b - 4. * c;
  const double mag = b * b + fabs(4. * c);
  if (!(disc >= -DISC_BAND * mag)) return false;    // (false for a NaN, too)
  disc = fmax(disc, 0.);
  const double s = sqrt(disc);
  zp = (-b + s) / 2.;
  zm = (-b - s) / 2.;
  return true;
}

// Grunert's three-point solution on the rows (X_k, x_k): up to four poses (t, q) in fp32, ok[s] says which slots hold one; false: INVALID
RP_DEV bool p3p_solve(const float (&Xf)[3][3], const float2 (&xf)[3], float (&pose)[NSOL][7], bool (&ok)[NSOL]) {
#pragma unroll
  for (int s = 0; s < NSOL; ++s) {
    ok[s] = false;
#pragma unroll
    for (int i = 0; i < 7; ++i) pose[s][i] = 0.f;
  }
  // ---- 1. bearings, cosines, squared sides
  double X[3][3], f[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double u = (double)xf[k].x, v = (double)xf[k].y;
    const double nrm = sqrt((u * u + v * v) + 1.);
    f[k][0] = u / nrm; f[k][1] = v / nrm; f[k][2] = 1. / nrm;
#pragma unroll
    for (int i = 0; i < 3; ++i) X[k][i] = (double)Xf[k][i];
  }
  const double ca = dot64(f[1], f[2]), cb = dot64(f[0], f[2]), cg = dot64(f[0], f[1]);
  const double d12[3] = {X[1][0] - X[2][0], X[1][1] - X[2][1], X[1][2] - X[2][2]};
  const double d20[3] = {X[2][0] - X[0][0], X[2][1] - X[0][1], X[2][2] - X[0][2]};
  const double d10[3] = {X[1][0] - X[0][0], X[1][1] - X[0][1], X[1][2] - X[0][2]};
  const double a2 = dot64(d12, d12), b2 = dot64(d20, d20), c2 = dot64(d10, d10);
  // ---- 2. the degenerate samples
  const double big = fmax(a2, fmax(b2, c2));
  bool valid = big <= FINITE64 && a2 >= SIDE_MIN * big && b2 >= SIDE_MIN * big && c2 >= SIDE_MIN * big && big > 0.;
  double cr[3];
  cross64(d10, d20, cr);
  valid = valid && dot64(cr, cr) >= AREA_MIN * c2 * b2;
  cross64(f[1], f[2], cr);
  valid = valid && dot64(cr, cr) >= SPAN_MIN;
  cross64(f[0], f[2], cr);
  valid = valid && dot64(cr, cr) >= SPAN_MIN;
  cross64(f[0], f[1], cr);
  valid = valid && dot64(cr, cr) >= SPAN_MIN;
  if (!valid) return false;
  // ---- 3. the quartic
  const double k = (a2 - c2) / b2, l = c2 / b2;
  const double n0 = 1. + k, n1 = -2. * k * cb, n2 = k - 1.;
  const double d0 = 2. * cg, d1 = -2. * ca;
  const double e0 = d0 * d0, e1 = 2. * d0 * d1, e2 = d1 * d1;                                    // D^2
  const double nn[5] = {n0 * n0, 2. * n0 * n1, n1 * n1 + 2. * n0 * n2, 2. * n1 * n2, n2 * n2};  // N^2
  const double nd[4] = {n0 * d0, n0 * d1 + n1 * d0, n1 * d1 + n2 * d0, n2 * d1};                 // N D
  const double cd[5] = {e0, e1 - 2. * cb * e0, (e2 - 2. * cb * e1) + e0, e1 - 2. * cb * e2, e2};  // (1 - 2 cb v + v^2) D^2
  const double A0 = ((e0 + nn[0]) - 2. * cg * nd[0]) - l * cd[0];
  const double A1 = ((e1 + nn[1]) - 2. * cg * nd[1]) - l * cd[1];
  const double A2 = ((e2 + nn[2]) - 2. * cg * nd[2]) - l * cd[2];
  const double A3 = (nn[3] - 2. * cg * nd[3]) - l * cd[3];
  const double A4 = nn[4] - l * cd[4];
  const double amax = fmax(fmax(fabs(A0), fabs(A1)), fmax(fmax(fabs(A2), fabs(A3)), fabs(A4)));
  if (!(amax <= FINITE64) || !(fabs(A4) > LEAD_MIN * amax)) return false;
  // ---- 4. Ferrari
  const double q3 = A3 / A4, q2 = A2 / A4, q1 = A1 / A4, q0 = A0 / A4;
  const double sh = q3 / 4.;
  const double p = q2 - 6. * sh * sh;
  const double q = (q1 - 2. * q2 * sh) + 8. * sh * sh * sh;
  const double r = ((q0 - q1 * sh) + q2 * sh * sh) - 3. * (sh * sh) * (sh * sh);
  // the resolvent m^3 + p m^2 + c1 m + c0 and its largest real root
  const double c1 = p * p / 4. - r, c0 = -(q * q) / 8.;
  const double Pc = c1 - p * p / 3., Qc = (2. * p * p * p / 27. - p * c1 / 3.) + c0;
  const double disc = Qc * Qc / 4. + Pc * Pc * Pc / 27.;
  double m;
  if (disc > 0.) {
    const double sd = sqrt(disc);
    m = cbrt(-Qc / 2. + sd) + cbrt(-Qc / 2. - sd);
  } else {
    const double amp = 2. * sqrt(fmax(-Pc / 3., 0.));
    const double arg = Pc < 0. ? (3. * Qc / (2. * Pc)) * sqrt(-3. / Pc) : 1.;
    m = amp * cos(acos(fmin(fmax(arg, -1.), 1.)) / 3.);
  }
  m -= p / 3.;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double fv = ((m + p) * m + c1) * m + c0, fd = (3. * m + 2. * p) * m + c1;
    m = fd != 0. ? m - fv / fd : m;
  }
  double z[NSOL];
  bool real[NSOL];
  if (m > RESOLVENT_MIN * fmax(1., fabs(p))) {
    const double s = sqrt(2. * m), h = q / (2. * s);
    real[0] = real[1] = quadratic(-s, (p / 2. + m) + h, z[0], z[1]);
    real[2] = real[3] = quadratic(s, (p / 2. + m) - h, z[2], z[3]);
  } else {
    double zp = 0., zm = 0.;
    const bool any = quadratic(p, r, zp, zm);
    real[0] = real[1] = any && zp >= 0.;
    real[2] = real[3] = any && zm >= 0.;
    z[0] = sqrt(fmax(zp, 0.)); z[1] = -z[0];
    z[2] = sqrt(fmax(zm, 0.)); z[3] = -z[2];
  }
  if (!(fabs(m) <= FINITE64)) return false;
  // ---- 5., 6. the solutions and their poses
  double e[3][3];
  frame64(X[0], X[1], X[2], e);
  bool any = false;
#pragma unroll
  for (int s = 0; s < NSOL; ++s) {
    double v = real[s] ? z[s] - sh : 0.;
#pragma unroll
    for (int it = 0; it < 3; ++it) {
      const double fv = (((v + q3) * v + q2) * v + q1) * v + q0, fd = ((4. * v + 3. * q3) * v + 2. * q2) * v + q1;
      v = fd != 0. ? v - fv / fd : v;
    }
    const double Dv = d0 + d1 * v, Nv = (n0 + n1 * v) + n2 * v * v, den = (1. - 2. * cb * v) + v * v;
    bool good = real[s] && v > 0. && fabs(Dv) >= DEN_V_MIN && den > 0.;
    // y = N / D names the branch; its value is taken from the side X_0 X_1 alone, y^2 - 2 cg y + (1 - l den) = 0, which stays well
    // conditioned where N and D vanish together
    const double y0 = good ? Nv / Dv : 1.;
    const double w2 = (cg * cg - 1.) + l * den, rt = sqrt(fmax(w2, 0.));
    const double yp = cg + rt, ym = cg - rt;
    const double y = w2 >= 0. ? (fabs(yp - y0) <= fabs(ym - y0) ? yp : ym) : y0;
    good = good && y > 0.;
    const double s0 = sqrt(b2 / (good ? den : 1.)), s1 = y * s0, s2 = v * s0;
    double Y[3][3], g[3][3], R[9], qd[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      Y[0][i] = s0 * f[0][i]; Y[1][i] = s1 * f[1][i]; Y[2][i] = s2 * f[2][i];
    }
    frame64(Y[0], Y[1], Y[2], g);
#pragma unroll
    for (int rr = 0; rr < 3; ++rr)
#pragma unroll
      for (int c = 0; c < 3; ++c) R[3 * rr + c] = (g[0][rr] * e[0][c] + g[1][rr] * e[1][c]) + g[2][rr] * e[2][c];
    rot_to_quat64(R, qd);
    float v4[4], u4[4], tt[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) tt[i] = (float)(Y[0][i] - (((R[3 * i] * X[0][0] + R[3 * i + 1] * X[0][1]) + R[3 * i + 2] * X[0][2])));
#pragma unroll
    for (int i = 0; i < 4; ++i) v4[i] = (float)qd[i];
    const float nq = unit(v4, u4);
    good = good && nq > 0.5f && nq < 2.f;             // (false for a NaN: the frames of a collapsed solution)
#pragma unroll
    for (int i = 0; i < 3; ++i) good = good && fabsf(tt[i]) <= RP_FINITE;
    const float sg = u4[3] < 0.f ? -1.f : 1.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) pose[s][i] = good ? tt[i] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) pose[s][3 + i] = good ? sg * u4[i] : 0.f;
    ok[s] = good;
    any = any || good;
  }
  return any;
}

__global__ __launch_bounds__(NT) void hypothesis_kernel(const float* __restrict__ Xg, const float* __restrict__ xg,
                                                         const float* __restrict__ w, const float* __restrict__ tau, uint32_t seed,
                                                         float* hyp_pose, float* hyp_cost, int* hyp_count, int* samples, int P, int M,
                                                         int chunks) {
  __shared__ ConsensusRows<MAXP> sm;                 // the core's rows: a = b = the image (its staging takes two float2 operands)
  __shared__ float X3[MAXP][3];                      // the points of the same rows, gathered through sm.pos
  const int tid = threadIdx.x;
  const long long b = blockIdx.x / chunks;
  const int m = (blockIdx.x % chunks) * NT + tid;
  const float* XX = Xg + b * P * 3;
  const float2* xx = reinterpret_cast<const float2*>(xg) + b * P;
  const int K = consensus_stage(sm, xx, xx, w ? w + b * P : nullptr, P);
  for (int j = tid; j < K; j += NT) {               // (sm.pos is final behind the core's last barrier; K <= P <= MAXP)
    const int r = sm.pos[j];
    X3[j][0] = XX[3 * r]; X3[j][1] = XX[3 * r + 1]; X3[j][2] = XX[3 * r + 2];
  }
  __syncthreads();
  if (m >= M) return;                               // (behind the last barrier)
  uint32_t c[3];
  consensus_sample(sm, seed, b, m, M, K, samples, c);
  // ---- solve
  const float ta = tau[b], tau2 = ta * ta;
  float pose[NSOL][7] = {};
  bool ok[NSOL] = {false, false, false, false};
  bool valid = K >= 3 && ta > 0.f;
  if (valid) {
    float Xs[3][3];
    float2 xs[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int i = 0; i < 3; ++i) Xs[k][i] = X3[c[k]][i];
      xs[k] = sm.a[c[k]];
    }
    valid = p3p_solve(Xs, xs, pose, ok);
  }
  // ---- score: one walk, one running sum per solution
  float best_cost = FLT_MAX;
  int best_slot = -1, count = 0;
  if (valid) {
    float R[NSOL][9], acc[NSOL], wsum = 0.f;
#pragma unroll
    for (int s = 0; s < NSOL; ++s) {
      const float q4[4] = {pose[s][3], pose[s][4], pose[s][5], pose[s][6]};
      quat_to_rot(q4, R[s]);
      acc[s] = 0.f;
    }
    for (int j = 0; j < K; ++j) {
      const float wt = sm.w[j], X = X3[j][0], Y = X3[j][1], Z = X3[j][2];
      const float2 u = sm.a[j];
#pragma unroll
      for (int s = 0; s < NSOL; ++s) {
        const float t3[3] = {pose[s][0], pose[s][1], pose[s][2]};
        const float d = pose_distance(R[s], t3, X, Y, Z, u.x, u.y);
        acc[s] += wt * (tau2 * log1pf(d / tau2));
      }
      wsum += wt;
    }
#pragma unroll
    for (int s = 0; s < NSOL; ++s) {
      const float cs = acc[s] / wsum;
      const bool keep = ok[s] && cs < FLT_MAX;      // (false for a NaN, too)
      count += keep ? 1 : 0;
      if (keep && cs < best_cost) { best_cost = cs; best_slot = s; }
    }
  }
  float out[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    out[i] = 0.f;
#pragma unroll
    for (int s = 0; s < NSOL; ++s) out[i] = best_slot == s ? pose[s][i] : out[i];
  }
  float* HP = hyp_pose + (b * M + m) * 7;
#pragma unroll
  for (int i = 0; i < 7; ++i) HP[i] = out[i];
  hyp_cost[b * M + m] = best_slot >= 0 ? best_cost : FLT_MAX;
  if (hyp_count) hyp_count[b * M + m] = count;
}

__global__ __launch_bounds__(NT) void select_kernel(const float* __restrict__ Xg, const float* __restrict__ xg, const float* __restrict__ w,
                                                     const float* __restrict__ tau, const float* __restrict__ hyp_pose,
                                                     const float* __restrict__ hyp_cost, float* pose, int* best, float* stat, float* w_out,
                                                     int P, int M) {
  __shared__ float red[2][NW][RED];
  __shared__ unsigned long long key[NT];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const float* HC = hyp_cost + b * M;
  const float* XX = Xg + b * P * 3;
  const float2* xx = reinterpret_cast<const float2*>(xg) + b * P;
  const float* W = w ? w + b * P : nullptr;
  float* WO = w_out ? w_out + b * P : nullptr;
  // ---- the lowest-index minimum among the valid slots, and their number.  A cost is a float >= +0 (or FLT_MAX), whose bits order as
  // the float does: the smallest 64-bit key (bits of the cost, index) is the smallest cost and, among equal costs, the lowest index
  unsigned long long lo = ~0ull;
  float nvalid = 0.f;
  for (int m = tid; m < M; m += NT) {
    const float c = HC[m];
    nvalid += c < FLT_MAX ? 1.f : 0.f;
    const unsigned long long k = ((unsigned long long)float_bits(c) << 32) | (unsigned)m;
    lo = c < FLT_MAX && k < lo ? k : lo;
  }
  key[tid] = lo;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) key[tid] = key[tid + s] < key[tid] ? key[tid + s] : key[tid];
    __syncthreads();
  }
  const int win = key[0] == ~0ull ? -1 : (int)(unsigned)(key[0] & 0xffffffffull);
  float ps[7], R[9];
#pragma unroll
  for (int i = 0; i < 7; ++i) ps[i] = win >= 0 ? hyp_pose[(b * M + win) * 7 + i] : 0.f;
  const float q4[4] = {ps[3], ps[4], ps[5], ps[6]}, t3[3] = {ps[0], ps[1], ps[2]};
  quat_to_rot(q4, R);
  const float ta = tau[b], tau2 = win >= 0 ? ta * ta : 1.f;
  // ---- the weights at the winner
  float s4[4] = {0.f, 0.f, 0.f, nvalid};
  for (int r = tid; r < P; r += NT) {
    const float wt = W ? fmaxf(W[r], 0.f) : 1.f;
    const float2 u = xx[r];
    const float d = pose_distance(R, t3, XX[3 * r], XX[3 * r + 1], XX[3 * r + 2], u.x, u.y);
    s4[0] += wt;
    s4[1] += d <= tau2 ? wt : 0.f;
    s4[2] += wt > 0.f ? 1.f : 0.f;
    if (WO) WO[r] = win >= 0 ? wt / (1.f + d / tau2) : wt;
  }
  int phase = 0;
  block_sum(s4, red, phase);
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 7; ++i) pose[b * 7 + i] = ps[i];
    best[b] = win;
    stat[b * 4] = win >= 0 ? HC[win] : 0.f;
    stat[b * 4 + 1] = win >= 0 ? s4[1] / s4[0] : 0.f;
    stat[b * 4 + 2] = s4[3];
    stat[b * 4 + 3] = s4[2];
  }
}

// the robust cost term of one row
RP_DEV float cost_term(const float (&R)[9], const float (&t)[3], float X, float Y, float Z, float u, float v, float wt, float tau2) {
  return wt * (tau2 * log1pf(pose_distance(R, t, X, Y, Z, u, v) / tau2));
}

__global__ __launch_bounds__(NT) void refine_kernel(const float* pose0, const float* __restrict__ Xg, const float* __restrict__ xg,
                                                     const float* __restrict__ w, const float* __restrict__ tau, int iters, float* pose,
                                                     float* stat, float* w_out, int P) {
  __shared__ float red[2][NW][LMRED];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const float* XX = Xg + b * P * 3;
  const float2* xx = reinterpret_cast<const float2*>(xg) + b * P;
  const float* W = w ? w + b * P : nullptr;
  float* WO = w_out ? w_out + b * P : nullptr;
  // ---- the thread's rows, once
  float pX[ROWS], pY[ROWS], pZ[ROWS], bx[ROWS], by[ROWS], wt[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = tid + i * NT;
    pX[i] = pY[i] = pZ[i] = bx[i] = by[i] = wt[i] = 0.f;
    if (r < P) {
      const float2 c = xx[r];
      pX[i] = XX[3 * r]; pY[i] = XX[3 * r + 1]; pZ[i] = XX[3 * r + 2];
      bx[i] = c.x; by[i] = c.y;
      wt[i] = W ? fmaxf(W[r], 0.f) : 1.f;
    }
  }
  // ---- the start: t0, unit(q0) with w >= 0
  float p0[7], t[3], q[4], h[9];
  bool degenerate = false;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    p0[i] = pose0[b * 7 + i];
    degenerate = degenerate || !(fabsf(p0[i]) <= RP_FINITE);
  }
  const float q0[4] = {p0[3], p0[4], p0[5], p0[6]};
  const float nq0 = unit(q0, q);
  const float ta = tau[b], tau2 = ta * ta;
  degenerate = degenerate || !(nq0 >= RP_MIN_SCALE) || !(nq0 <= RP_FINITE) || !(ta > 0.f);
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = degenerate ? (i == 3 ? 1.f : 0.f) : (q[3] < 0.f ? -q[i] : q[i]);   // (uniform; the identity keeps the arithmetic below finite)
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = degenerate ? 0.f : p0[i];
  quat_to_rot(q, h);
  const int nrows = (P + NT - 1) / NT;             // row slots in use (uniform)
  int phase = 0;
  // ---- sum of the weights, count of the positive ones, cost
  float s3[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {                  // (unrolled under a uniform guard: static indices, nothing goes to scratch)
    if (i >= nrows) break;
    s3[0] += wt[i];
    s3[1] += wt[i] > 0.f ? 1.f : 0.f;
    s3[2] += cost_term(h, t, pX[i], pY[i], pZ[i], bx[i], by[i], wt[i], degenerate ? 1.f : tau2);
  }
  block_sum(s3, red, phase);
  const float wsum = s3[0];
  degenerate = degenerate || s3[1] < 3.f;
  if (degenerate) {
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const int r = tid + i * NT;
      if (WO && r < P) WO[r] = wt[i];
    }
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < 7; ++i) pose[b * 7 + i] = p0[i];
      stat[b * 4] = 0.f; stat[b * 4 + 1] = 0.f; stat[b * 4 + 2] = 0.f; stat[b * 4 + 3] = s3[1];
    }
    return;
  }
  float c = s3[2] / wsum, lam = LAMBDA0, accepted = 0.f;
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    // ---- pass 1: the normal matrix and the gradient
    float a[LMRED];
#pragma unroll
    for (int i = 0; i < LMRED; ++i) a[i] = 0.f;
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      if (i >= nrows) break;
      const float X = pX[i], Y = pY[i], Z = pZ[i];
      const float y0 = (h[0] * X + h[1] * Y) + h[2] * Z, y1 = (h[3] * X + h[4] * Y) + h[5] * Z, y2 = (h[6] * X + h[7] * Y) + h[8] * Z;
      const float m0 = y0 + t[0], m1 = y1 + t[1], m2 = y2 + t[2];
      const float ex = m0 - bx[i] * m2, ey = m1 - by[i] * m2, den = m2 * m2;
      const bool in = m2 > 0.f && den >= DEN_MIN;   // a row behind the camera or on its horizon has no derivative
      const float inv = in ? 1.f / m2 : 0.f;
      const float dd = fminf((ex * ex + ey * ey) / fmaxf(den, DEN_MIN), D_MAX);
      const float d = in ? dd : D_MAX;
      const float om = in ? wt[i] / (1.f + d / tau2) : 0.f;
      const float rx = ex * inv, ry = ey * inv, px = m0 * inv, py = m1 * inv;
      const float Jx[NPAR] = {inv * -(px * y1), inv * (y2 + px * y0), inv * -y1, inv, 0.f, inv * -px};
      const float Jy[NPAR] = {inv * -(y2 + py * y1), inv * (py * y0), inv * y0, 0.f, inv, inv * -py};
      int k = 0;
#pragma unroll
      for (int u = 0; u < NPAR; ++u)
#pragma unroll
        for (int v = u; v < NPAR; ++v) a[k++] += om * (Jx[u] * Jx[v] + Jy[u] * Jy[v]);
#pragma unroll
      for (int u = 0; u < NPAR; ++u) a[NTRI + u] += om * (Jx[u] * rx + Jy[u] * ry);
    }
    block_sum(a, red, phase);
    // ---- the step and the trial state (uniform): unit((omega / 2, 1) (x) q), t + upsilon
    float delta[NPAR], q1[4], h1[9], t1[3];
    bool solved = lm_cholesky_solve<NPAR>(a, lam, delta);
    if (!solved) {
#pragma unroll
      for (int i = 0; i < NPAR; ++i) delta[i] = 0.f;
    }
    const float px = delta[0] / 2.f, py = delta[1] / 2.f, pz = delta[2] / 2.f;
    const float v[4] = {((q[0] + px * q[3]) + py * q[2]) - pz * q[1], ((q[1] - px * q[2]) + py * q[3]) + pz * q[0],
                        ((q[2] + px * q[1]) - py * q[0]) + pz * q[3], ((q[3] - px * q[0]) - py * q[1]) - pz * q[2]};
    const float nq = unit(v, q1);
    if (!(nq > 0.f) || !(nq <= RP_FINITE)) {
      solved = false;
#pragma unroll
      for (int i = 0; i < 4; ++i) q1[i] = q[i];
    }
    if (q1[3] < 0.f) {
#pragma unroll
      for (int i = 0; i < 4; ++i) q1[i] = -q1[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) t1[i] = t[i] + delta[3 + i];
    quat_to_rot(q1, h1);
    // ---- pass 2: the trial cost
    float c1[1] = {0.f};
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      if (i >= nrows) break;
      c1[0] += cost_term(h1, t1, pX[i], pY[i], pZ[i], bx[i], by[i], wt[i], tau2);
    }
    block_sum(c1, red, phase);
    const float ct = c1[0] / wsum;
    if (solved && ct < c) {
#pragma unroll
      for (int i = 0; i < 9; ++i) h[i] = h1[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] = q1[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = t1[i];
      c = ct;
      lam = fmaxf(lam / 10.f, LAMBDA_MIN);
      accepted += 1.f;
    } else {
      lam = fminf(lam * 10.f, LAMBDA_MAX);
    }
  }
  // ---- finish: the weights and the inlier share at the output
  float inl[1] = {0.f};
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = tid + i * NT;
    if (r < P) {
      const float d = pose_distance(h, t, pX[i], pY[i], pZ[i], bx[i], by[i]);
      inl[0] += d <= tau2 ? wt[i] : 0.f;
      if (WO) WO[r] = wt[i] / (1.f + d / tau2);
    }
  }
  block_sum(inl, red, phase);
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) pose[b * 7 + i] = t[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) pose[b * 7 + 3 + i] = q[i];
    stat[b * 4] = c; stat[b * 4 + 1] = inl[0] / wsum; stat[b * 4 + 2] = accepted; stat[b * 4 + 3] = s3[1];
  }
}

}  // namespace

extern "C" int rp_resection_abi_version(void) { return RP_RESECTION_ABI_VERSION; }

extern "C" int rp_p3p_consensus(const float* X, const float* x, const float* w, const float* tau, int seed, float* pose, int* best,
                                float* stat, float* w_out, float* hyp_pose, float* hyp_cost, int* hyp_count, int* samples, int P, int M,
                                int n, void* stream) {
  if (n <= 0 || P < 3 || M < 1 || !X || !x || !tau || !pose || !best || !stat || !hyp_pose || !hyp_cost) return RP_EBADSHAPE;
  if (P > RP_RESECTION_MAX_P || M > RP_RESECTION_MAX_M) return RP_EUNSUPPORTED;
  const int chunks = (M + NT - 1) / NT;
  if ((long long)n * chunks > 2147483647LL) return RP_EUNSUPPORTED;
  if ((uintptr_t)x & 7) return RP_EALIGN;
  if (((uintptr_t)X | (uintptr_t)w | (uintptr_t)tau | (uintptr_t)pose | (uintptr_t)best | (uintptr_t)stat | (uintptr_t)w_out |
       (uintptr_t)hyp_pose | (uintptr_t)hyp_cost | (uintptr_t)hyp_count | (uintptr_t)samples) & 3)
    return RP_EALIGN;
  hipLaunchKernelGGL(hypothesis_kernel, dim3(n * chunks), dim3(NT), 0, (hipStream_t)stream, X, x, w, tau, (uint32_t)seed, hyp_pose,
                     hyp_cost, hyp_count, samples, P, M, chunks);
  RP_CHECK_LAUNCH();
  hipLaunchKernelGGL(select_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, X, x, w, tau, hyp_pose, hyp_cost, pose, best, stat, w_out, P,
                     M);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_pnp_refine(const float* X, const float* x, const float* w, const float* tau, const float* pose0, int iters, float* pose,
                             float* stat, float* w_out, int P, int n, void* stream) {
  if (n <= 0 || P < 3 || iters < 0 || !X || !x || !tau || !pose0 || !pose || !stat) return RP_EBADSHAPE;
  if (P > RP_RESECTION_MAX_P || iters > RP_RESECTION_MAX_ITERS) return RP_EUNSUPPORTED;
  if ((uintptr_t)x & 7) return RP_EALIGN;
  if (((uintptr_t)X | (uintptr_t)w | (uintptr_t)tau | (uintptr_t)pose0 | (uintptr_t)pose | (uintptr_t)stat | (uintptr_t)w_out) & 3)
    return RP_EALIGN;
  hipLaunchKernelGGL(refine_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, pose0, X, x, w, tau, iters, pose, stat, w_out, P);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
