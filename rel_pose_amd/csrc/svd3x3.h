// svd3x3.h -- the per-lane 3x3 one-sided Jacobi SVD (svd3x3_dev) and its plane rotation (rot), one definition: geom.hip (rp_svd3x3,
// rp_pose_from_essential) and ../csrc_eightpoint/eight_point.hip (the projection onto the essential manifold) both include it.
// The method is described at the top of geom.hip.
#pragma once
#include "common.h"

RP_DEV void rot(float& a, float& b, float c, float s) {
  const float x = c * a - s * b, y = s * a + c * b;
  a = x;
  b = y;
}

// one 3x3 SVD in registers: A row-major [9] -> u[col][row], sg[3] descending, v[col][row]
// Domain: finite float32 entries, the largest of them normal.  A is multiplied at entry by the exact power of two that brings its largest
// magnitude into [0.5, 1) and sg is scaled back at the end: the squared column norms and their products (alpha beta of the skip test
// overflows from |A| ~ 4e9 on, the norms go denormal below ~1e-19) then stay in range whatever the scale of A.  Every rotation decision
// is a ratio of such terms, so a matrix that was in range before gives the same bits with the scaling as without it.  (Entries more
// than 2^-126 below the largest are flushed by the scaling -- far below its rounding; sg overflows only if sigma_1 itself does.)
RP_DEV void svd3x3_dev(const float* A, float (&u)[3][3], float (&sg)[3], float (&v)[3][3]) {
  float w[3][3];                       // w[col][row]
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) amax = fmaxf(amax, fabsf(A[i]));
  int ex = 0;
  if (amax > 0.f && amax <= 3.402823466e38f) frexpf(amax, &ex);     // a zero (or non-finite) matrix is left as it is
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      w[c][r] = ldexpf(A[3 * r + c], -ex);
      v[c][r] = r == c ? 1.f : 0.f;
    }
#pragma unroll 1
  for (int sweep = 0; sweep < 6; ++sweep) {
#pragma unroll
    for (int pair = 0; pair < 3; ++pair) {
      const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2;
      const float al = w[p][0] * w[p][0] + w[p][1] * w[p][1] + w[p][2] * w[p][2];
      const float be = w[q][0] * w[q][0] + w[q][1] * w[q][1] + w[q][2] * w[q][2];
      const float ga = w[p][0] * w[q][0] + w[p][1] * w[q][1] + w[p][2] * w[q][2];
      if (fabsf(ga) > 1e-12f * sqrtf(al * be) && ga != 0.f) {
        const float zeta = (be - al) / (2.f * ga);
        const float t = copysignf(1.f, zeta) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
        const float c = 1.f / sqrtf(1.f + t * t), s = c * t;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          rot(w[p][r], w[q][r], c, s);
          rot(v[p][r], v[q][r], c, s);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) sg[c] = sqrtf(w[c][0] * w[c][0] + w[c][1] * w[c][1] + w[c][2] * w[c][2]);
  // sort columns by singular value, descending (3-element network; swaps carry w and v along)
#define RP_CSWAP(a, b)                                                            \
  if (sg[a] < sg[b]) {                                                            \
    float t_ = sg[a]; sg[a] = sg[b]; sg[b] = t_;                                  \
    _Pragma("unroll") for (int r = 0; r < 3; ++r) {                               \
      t_ = w[a][r]; w[a][r] = w[b][r]; w[b][r] = t_;                              \
      t_ = v[a][r]; v[a][r] = v[b][r]; v[b][r] = t_;                              \
    }                                                                             \
  }
  RP_CSWAP(0, 1) RP_CSWAP(1, 2) RP_CSWAP(0, 1)
#undef RP_CSWAP
  const float tiny = 1e-7f * fmaxf(sg[0], 1e-30f);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float inv = sg[c] > tiny ? 1.f / sg[c] : 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) u[c][r] = w[c][r] * inv;
  }
  // rank deficiency (an essential matrix has sigma_3 = 0): complete U with cross products so that it stays orthogonal
  if (sg[1] <= tiny) {                      // rank <= 1: any unit vector orthogonal to u0
    const float ax = fabsf(u[0][0]), ay = fabsf(u[0][1]), az = fabsf(u[0][2]);
    float e[3] = {ax <= ay && ax <= az ? 1.f : 0.f, (ay < ax && ay <= az) ? 1.f : 0.f, (az < ax && az < ay) ? 1.f : 0.f};
    if (sg[0] <= tiny) { u[0][0] = 1.f; u[0][1] = 0.f; u[0][2] = 0.f; e[0] = 0.f; e[1] = 1.f; e[2] = 0.f; }
    float cx = u[0][1] * e[2] - u[0][2] * e[1], cy = u[0][2] * e[0] - u[0][0] * e[2], cz = u[0][0] * e[1] - u[0][1] * e[0];
    const float nrm = 1.f / sqrtf(cx * cx + cy * cy + cz * cz);
    u[1][0] = cx * nrm; u[1][1] = cy * nrm; u[1][2] = cz * nrm;
  }
  if (sg[2] <= tiny) {
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) sg[c] = ldexpf(sg[c], ex);
}
