// five_point.hip -- rp_five_point_consensus: the consensus of csrc/consensus_core.h with the calibrated five-point solver as its minimal
// solver (librelpose_fivepoint.so).
//
// Two launches; include/relpose_fivepoint.h states the sampler, the solve, the slots, the score and the selection.
//   hypothesis_kernel   grid n * ceil(M / 256) (problem-major, one dimension), 256 threads.
//     stage    the core: the rows of positive weight COMPACTED into LDS (42 496 B).  Four barriers; from there on no thread talks to
//              another.
//     solve    one lane, one sample, fp64: Floyd's five draws (the core), five Householder reflections of the 9 x 5 transpose, the
//              null-space basis X, Y, Z, W, the ten cubics by products of linear and quadratic forms (every index static), Gauss-Jordan
//              with row pivoting on the lane's private 10 x 20 array (runtime row indices: it lives in scratch, 1600 B per lane), Nister's
//              tenth-degree polynomial p = det B(z), its real roots by bracketing through the derivatives of p.  Every loop has a
//              fixed trip count: 48 halvings and 4 guarded Newton steps per bracket, at most d brackets at degree d.
//     score    fp32: each root is rounded at norm 1, projected with svd3x3_dev, signed, and walks the K compacted rows through the core's
//              cost loop (every lane reads the SAME LDS address: a broadcast); valid roots fill the sample's slots in ascending z, the
//              remaining slots are written as invalid.
//   select_kernel       grid n, 256 threads: the core's lowest-index argmin of hyp_cost over the 10 M slots, the Sampson distances at the
//              winner and w_out; the sums of stat by block_sum.
// No atomics, no workspace; the only output that is read is hyp_cost / hyp_E, by the second launch after the first wrote all of it.
#include <float.h>
#include "../csrc/common.h"
#include "../csrc/block_sum.h"
#include "../csrc/svd3x3.h"
#include "../csrc/two_view.h"
#include "../csrc/consensus_core.h"
#include "../../include/relpose_fivepoint.h"

namespace {

constexpr int NT = BLOCK_SUM_THREADS;                // threads per workgroup
constexpr int NW = BLOCK_SUM_WAVES;
constexpr int MAXP = RP_FIVEPOINT_MAX_P;
constexpr int RED = 4;                               // floats per wave in the reduction buffer of select_kernel
constexpr int NR = RP_FIVEPOINT_ROOTS;
constexpr double MIN_PIVOT = 1e-12;                  // a Householder column norm or an elimination pivot below this: breakdown
constexpr int HALVINGS = 48, NEWTON = 4;             // per bracket

// ---- polynomials in (x, y, z).  linear: x y z 1;  quadratic: x^2 y^2 z^2 xy xz yz x y z 1;  cubic: the 20 columns of the header
// q += s a b
RP_DEV void mul11(double (&q)[10], const double (&a)[4], const double (&b)[4], double s) {
  q[0] += s * (a[0] * b[0]);
  q[1] += s * (a[1] * b[1]);
  q[2] += s * (a[2] * b[2]);
  q[3] += s * (a[0] * b[1] + a[1] * b[0]);
  q[4] += s * (a[0] * b[2] + a[2] * b[0]);
  q[5] += s * (a[1] * b[2] + a[2] * b[1]);
  q[6] += s * (a[0] * b[3] + a[3] * b[0]);
  q[7] += s * (a[1] * b[3] + a[3] * b[1]);
  q[8] += s * (a[2] * b[3] + a[3] * b[2]);
  q[9] += s * (a[3] * b[3]);
}

// c += q l
RP_DEV void mul21(double* c, const double (&q)[10], const double (&l)[4]) {
  c[0] += q[0] * l[0];                                    // x^3
  c[1] += q[1] * l[1];                                    // y^3
  c[2] += q[0] * l[1] + q[3] * l[0];                      // x^2 y
  c[3] += q[1] * l[0] + q[3] * l[1];                      // x y^2
  c[4] += q[0] * l[2] + q[4] * l[0];                      // x^2 z
  c[5] += q[0] * l[3] + q[6] * l[0];                      // x^2
  c[6] += q[1] * l[2] + q[5] * l[1];                      // y^2 z
  c[7] += q[1] * l[3] + q[7] * l[1];                      // y^2
  c[8] += q[3] * l[2] + q[4] * l[1] + q[5] * l[0];        // x y z
  c[9] += q[3] * l[3] + q[6] * l[1] + q[7] * l[0];        // x y
  c[10] += q[6] * l[3] + q[9] * l[0];                     // x
  c[11] += q[4] * l[3] + q[6] * l[2] + q[8] * l[0];       // x z
  c[12] += q[2] * l[0] + q[4] * l[2];                     // x z^2
  c[13] += q[7] * l[3] + q[9] * l[1];                     // y
  c[14] += q[5] * l[3] + q[7] * l[2] + q[8] * l[1];       // y z
  c[15] += q[2] * l[1] + q[5] * l[2];                     // y z^2
  c[16] += q[9] * l[3];                                   // 1
  c[17] += q[8] * l[3] + q[9] * l[2];                     // z
  c[18] += q[2] * l[3] + q[8] * l[2];                     // z^2
  c[19] += q[2] * l[2];                                   // z^3
}

// out += s a b, polynomials in z, lowest coefficient first
template <int NA, int NB>
RP_DEV void pmul(double (&out)[NA + NB - 1], const double (&a)[NA], const double (&b)[NB], double s) {
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) out[i + j] += s * (a[i] * b[j]);
}

RP_DEV double horner10(const double (&c)[11], double z) {
  double v = c[10];
#pragma unroll
  for (int i = 9; i >= 0; --i) v = v * z + c[i];
  return v;
}

// one row of B(z) from the eliminated rows a (x^2z, y^2z, xyz) and b (x^2, y^2, xy): a - z b over the columns x xz xz^2 y yz yz^2 1 z z^2 z^3
RP_DEV void brow(const double* a, const double* b, double (&bx)[4], double (&by)[4], double (&b1)[5]) {
  bx[0] = a[0]; bx[1] = a[1] - b[0]; bx[2] = a[2] - b[1]; bx[3] = -b[2];
  by[0] = a[3]; by[1] = a[4] - b[3]; by[2] = a[5] - b[4]; by[3] = -b[5];
  b1[0] = a[6]; b1[1] = a[7] - b[6]; b1[2] = a[8] - b[7]; b1[3] = a[9] - b[8]; b1[4] = -b[9];
}

RP_DEV double eval3(const double (&c)[4], double z) { return ((c[3] * z + c[2]) * z + c[1]) * z + c[0]; }
RP_DEV double eval4(const double (&c)[5], double z) { return (((c[4] * z + c[3]) * z + c[2]) * z + c[1]) * z + c[0]; }

// the five-point solve of the header on five rows: the null-space basis N (X, Y, Z, W) and the real solutions (xs, ys, zs), ascending
// in z; returns their number, 0 on a breakdown
RP_DEV int five_point(const float2 (&p1)[5], const float2 (&p2)[5], double (&N)[4][9], double (&xs)[NR], double (&ys)[NR], double (&zs)[NR]) {
  // A[k] = x2^h (x) x1^h of row k: the k-th COLUMN of the 9 x 5 transpose
  double A[5][9];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const double ax = p1[k].x, ay = p1[k].y, bx = p2[k].x, by = p2[k].y;
    A[k][0] = bx * ax; A[k][1] = bx * ay; A[k][2] = bx;
    A[k][3] = by * ax; A[k][4] = by * ay; A[k][5] = by;
    A[k][6] = ax;      A[k][7] = ay;      A[k][8] = 1.0;
  }
  // Householder QR of the transpose, column by column (consensus.hip), H_j = I - beta_j v_j v_j^T, v_j in A[j][j ..]
  double beta[5];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    double sig = 0.0;
#pragma unroll
    for (int i = j; i < 9; ++i) sig += A[j][i] * A[j][i];
    const double nrm = sqrt(sig);
    ok = ok && nrm >= MIN_PIVOT;
    const double den = sig + fabs(A[j][j]) * nrm;
    beta[j] = den > 0.0 ? 1.0 / den : 0.0;
    A[j][j] += copysign(nrm, A[j][j]);
#pragma unroll
    for (int k = j + 1; k < 5; ++k) {
      double t = 0.0;
#pragma unroll
      for (int i = j; i < 9; ++i) t += A[j][i] * A[k][i];
      t *= beta[j];
#pragma unroll
      for (int i = j; i < 9; ++i) A[k][i] -= t * A[j][i];
    }
  }
  if (!ok) return 0;
  // the null space: the last four columns of Q = H_0 .. H_4
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int i = 0; i < 9; ++i) N[c][i] = i == 5 + c ? 1.0 : 0.0;
#pragma unroll
    for (int j = 4; j >= 0; --j) {
      double t = 0.0;
#pragma unroll
      for (int i = j; i < 9; ++i) t += A[j][i] * N[c][i];
      t *= beta[j];
#pragma unroll
      for (int i = j; i < 9; ++i) N[c][i] -= t * A[j][i];
    }
  }
  // ---- the ten cubics.  l[i]: entry i of E as a linear form in (x, y, z, 1)
  double l[9][4];
#pragma unroll
  for (int i = 0; i < 9; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) l[i][c] = N[c][i];
  double C[10][20];
#pragma unroll
  for (int r = 0; r < 10; ++r)
#pragma unroll
    for (int c = 0; c < 20; ++c) C[r][c] = 0.0;
  {  // det E, expanded along the first row
    double q0[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, q1[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, q2[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    mul11(q0, l[4], l[8], 1.0); mul11(q0, l[5], l[7], -1.0);
    mul11(q1, l[5], l[6], 1.0); mul11(q1, l[3], l[8], -1.0);
    mul11(q2, l[3], l[7], 1.0); mul11(q2, l[4], l[6], -1.0);
    mul21(C[0], q0, l[0]); mul21(C[0], q1, l[1]); mul21(C[0], q2, l[2]);
  }
  {  // (E E^T - tr(E E^T) / 2) E
    double G[3][3][10];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) {
#pragma unroll
        for (int t = 0; t < 10; ++t) G[i][j][t] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) mul11(G[i][j], l[3 * i + k], l[3 * j + k], 1.0);
      }
#pragma unroll
    for (int t = 0; t < 10; ++t) {
      const double h = 0.5 * (G[0][0][t] + G[1][1][t] + G[2][2][t]);
      G[0][0][t] -= h; G[1][1][t] -= h; G[2][2][t] -= h;
      G[1][0][t] = G[0][1][t]; G[2][0][t] = G[0][2][t]; G[2][1][t] = G[1][2][t];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) mul21(C[1 + 3 * i + j], G[i][k], l[3 * k + j]);
  }
  // ---- Gauss-Jordan on the first ten columns, row pivoting
#pragma unroll 1
  for (int j = 0; j < 10; ++j) {
    int piv = j;
    double big = fabs(C[j][j]);
    for (int r = j + 1; r < 10; ++r) {
      const double v = fabs(C[r][j]);
      if (v > big) { big = v; piv = r; }
    }
    if (!(big >= MIN_PIVOT)) return 0;
    if (piv != j) {
      for (int c = j; c < 20; ++c) { const double t = C[j][c]; C[j][c] = C[piv][c]; C[piv][c] = t; }
    }
    const double inv = 1.0 / C[j][j];
    for (int c = j; c < 20; ++c) C[j][c] *= inv;
    for (int r = 0; r < 10; ++r) {
      if (r == j) continue;
      const double f = C[r][j];
      for (int c = j; c < 20; ++c) C[r][c] -= f * C[j][c];
    }
  }
  // ---- B(z) and p = det B
  double B0x[4], B0y[4], B01[5], B1x[4], B1y[4], B11[5], B2x[4], B2y[4], B21[5];
  brow(&C[4][10], &C[5][10], B0x, B0y, B01);
  brow(&C[6][10], &C[7][10], B1x, B1y, B11);
  brow(&C[8][10], &C[9][10], B2x, B2y, B21);
  double p[11];
  {
    double m0[8], m1[8], m2[7];
#pragma unroll
    for (int i = 0; i < 8; ++i) m0[i] = m1[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 7; ++i) m2[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 11; ++i) p[i] = 0.0;
    pmul<4, 5>(m0, B1y, B21, 1.0); pmul<5, 4>(m0, B11, B2y, -1.0);        // ly m1 - l1 my
    pmul<5, 4>(m1, B11, B2x, 1.0); pmul<4, 5>(m1, B1x, B21, -1.0);        // l1 mx - lx m1
    pmul<4, 4>(m2, B1x, B2y, 1.0); pmul<4, 4>(m2, B1y, B2x, -1.0);        // lx my - ly mx
    pmul<4, 8>(p, B0x, m0, 1.0); pmul<4, 8>(p, B0y, m1, 1.0); pmul<5, 7>(p, B01, m2, 1.0);
  }
  if (!(fabs(p[10]) > 0.0)) return 0;
  double R = 0.0;
#pragma unroll
  for (int i = 0; i < 10; ++i) R = fmax(R, fabs(p[i] / p[10]));
  R += 1.0;
  if (!(R <= 1e300)) return 0;
  // ---- the real roots of p: those of the derivative of degree d - 1 bracket those of the derivative of degree d
  double prev[NR], next[NR];
  int nprev = 0;
#pragma unroll 1
  for (int d = 1; d <= 10; ++d) {
    double cur[11], der[11];                          // the (10 - d)-th derivative of p, zero padded, and its derivative
    const int sh = 10 - d;
#pragma unroll
    for (int i = 0; i < 11; ++i) {
      double f = 1.0;                                 // (i + 1) .. (i + 10 - d)
#pragma unroll
      for (int s = 0; s < 10; ++s) f *= s < sh ? (double)(i + s + 1) : 1.0;
      cur[i] = i <= d ? p[i <= d ? i + sh : 0] * f : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 10; ++i) der[i] = cur[i + 1] * (double)(i + 1);
    der[10] = 0.0;
    int nc = 0;
    double lo = -R, flo = horner10(cur, lo);
    for (int i = 0; i <= NR; ++i) {
      if (i > nprev) break;
      const double hi = i < nprev ? prev[i < NR ? i : NR - 1] : R;
      const double fhi = horner10(cur, hi);
      if ((flo < 0.0) != (fhi < 0.0) && nc < NR) {
        double a = lo, b = hi;
        const bool nega = flo < 0.0;
        for (int s = 0; s < HALVINGS; ++s) {
          const double mid = 0.5 * (a + b);
          if ((horner10(cur, mid) < 0.0) == nega) a = mid; else b = mid;
        }
        double z = 0.5 * (a + b);
        for (int s = 0; s < NEWTON; ++s) {
          const double zn = z - horner10(cur, z) / horner10(der, z);
          if (zn >= a && zn <= b) z = zn;             // (false for a NaN)
        }
        next[nc++] = z;
      }
      lo = hi;
      flo = fhi;
    }
    nprev = nc;                                       // (none at this degree: the next one has the single bracket [-R, R])
    for (int i = 0; i < NR; ++i) prev[i] = i < nc ? next[i] : 0.0;
  }
  // ---- (x, y) of every root: the null vector of B(z), the largest of the cross products of two of its rows
  for (int i = 0; i < NR; ++i) {
    const double z = prev[i < nprev ? i : 0];
    const double r0[3] = {eval3(B0x, z), eval3(B0y, z), eval4(B01, z)};
    const double r1[3] = {eval3(B1x, z), eval3(B1y, z), eval4(B11, z)};
    const double r2[3] = {eval3(B2x, z), eval3(B2y, z), eval4(B21, z)};
    double c0[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
    const double c1[3] = {r0[1] * r2[2] - r0[2] * r2[1], r0[2] * r2[0] - r0[0] * r2[2], r0[0] * r2[1] - r0[1] * r2[0]};
    const double c2[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
    double n0 = c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2];
    const double n1 = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2], n2 = c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2];
    if (n1 > n0) { n0 = n1; c0[0] = c1[0]; c0[1] = c1[1]; c0[2] = c1[2]; }
    if (n2 > n0) { n0 = n2; c0[0] = c2[0]; c0[1] = c2[1]; c0[2] = c2[2]; }
    xs[i] = c0[0] / c0[2];
    ys[i] = c0[1] / c0[2];
    zs[i] = z;
  }
  return nprev;
}

__global__ __launch_bounds__(NT) void hypothesis_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                         const float* __restrict__ w, const float* __restrict__ tau, uint32_t seed,
                                                         float* hyp_E, float* hyp_cost, int* samples, int P, int M, int chunks) {
  __shared__ ConsensusRows<MAXP> sm;
  const long long b = blockIdx.x / chunks;
  const int m = (blockIdx.x % chunks) * NT + threadIdx.x;
  const float2* X1 = reinterpret_cast<const float2*>(x1) + b * P;
  const float2* X2 = reinterpret_cast<const float2*>(x2) + b * P;
  const int K = consensus_stage(sm, X1, X2, w ? w + b * P : nullptr, P);
  if (m >= M) return;                               // (behind the last barrier)
  uint32_t c[5];
  consensus_sample(sm, seed, b, m, M, K, samples, c);
  // ---- solve
  const float ta = tau[b], tau2 = ta * ta;
  double N[4][9], xs[NR], ys[NR], zs[NR];
  int roots = 0;
  if (K >= 5 && ta > 0.f) {
    float2 p1[5], p2[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      p1[k] = sm.a[c[k]];
      p2[k] = sm.b[c[k]];
    }
    roots = five_point(p1, p2, N, xs, ys, zs);
  }
  // ---- finish and score every root; the valid ones fill the slots in order
  float* HE = hyp_E + (b * M + m) * (NR * 9);
  float* HC = hyp_cost + (b * M + m) * NR;
  int slot = 0;
  for (int i = 0; i < NR; ++i) {
    if (i >= roots) break;
    const double x = xs[i], y = ys[i], z = zs[i];
    double ed[9], nn = 0.0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      ed[t] = x * N[0][t] + y * N[1][t] + z * N[2][t] + N[3][t];
      nn += ed[t] * ed[t];
    }
    const double inv = 1.0 / sqrt(nn);
    float F[9];
    bool ok = nn > 0.0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      F[t] = (float)(ed[t] * inv);
      ok = ok && fabsf(F[t]) <= RP_FINITE;
    }
    if (!ok) continue;
    float u[3][3], sv[3], v[3][3], e[9];
    svd3x3_dev(F, u, sv, v);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) e[3 * r + cc] = u[0][r] * v[0][cc] + u[1][r] * v[1][cc];
    if (!all_finite(e)) continue;
    sign_rule(e);
    const float cost = consensus_cost(sm, e, K, tau2, SampsonDistance());
    if (!(cost < FLT_MAX)) continue;                  // (a NaN, too)
#pragma unroll
    for (int t = 0; t < 9; ++t) HE[slot * 9 + t] = e[t];
    HC[slot] = cost;
    ++slot;
  }
  for (int k = 0; k < NR; ++k) {
    if (k < slot) continue;
#pragma unroll
    for (int t = 0; t < 9; ++t) HE[k * 9 + t] = 0.f;
    HC[k] = FLT_MAX;
  }
}

__global__ __launch_bounds__(NT) void select_kernel(const float* __restrict__ x1, const float* __restrict__ x2, const float* __restrict__ w,
                                                     const float* __restrict__ tau, const float* __restrict__ hyp_E,
                                                     const float* __restrict__ hyp_cost, float* E, int* best, float* stat, float* w_out,
                                                     int P, int M) {
  __shared__ float red[2][NW][RED];
  __shared__ float bc[NT];
  __shared__ int bi[NT];
  const long long b = blockIdx.x;
  const int S = M * NR;                                // slots of this problem: at most 40 960
  const float* HC = hyp_cost + b * S;
  float e[9], s4[4];
  const int win = consensus_select(bc, bi, reinterpret_cast<const float2*>(x1) + b * P, reinterpret_cast<const float2*>(x2) + b * P,
                                   w ? w + b * P : nullptr, w_out ? w_out + b * P : nullptr, HC, hyp_E + b * S * 9, S, P, tau[b],
                                   SampsonDistance(), e, s4);
  int phase = 0;
  block_sum(s4, red, phase);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) E[b * 9 + i] = e[i];
    best[b * 2] = win >= 0 ? win / NR : -1;
    best[b * 2 + 1] = win >= 0 ? win % NR : -1;
    stat[b * 4] = win >= 0 ? HC[win] : 0.f;
    stat[b * 4 + 1] = win >= 0 ? s4[1] / s4[0] : 0.f;
    stat[b * 4 + 2] = s4[3];
    stat[b * 4 + 3] = s4[2];
  }
}

}  // namespace

extern "C" int rp_fivepoint_abi_version(void) { return RP_FIVEPOINT_ABI_VERSION; }

extern "C" int rp_five_point_consensus(const float* x1, const float* x2, const float* w, const float* tau, int seed, float* E, int* best,
                                       float* stat, float* w_out, float* hyp_E, float* hyp_cost, int* samples, int P, int M, int n,
                                       void* stream) {
  return consensus_launch<5, RP_FIVEPOINT_MAX_P, RP_FIVEPOINT_MAX_M, hypothesis_kernel, select_kernel>(
      x1, x2, w, tau, seed, E, best, stat, w_out, hyp_E, hyp_cost, samples, P, M, n, stream);
}
