// shim_extra.h -- what csrc_submatch/submatch.hip needs beyond ../eightpoint_host/shim.h: float4 and its 16-byte accessors, exp2, the
// indexed wave shuffle (a yield, like __shfl_xor there) and the XCD work order of csrc/common.h.  Used by run.py only.
#pragma once
#include "shim.h"
#include <cstring>
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
// memcpy, not a cast: the sanitizers then see exactly the 16 bytes the device instruction touches
static inline float4 ld4(const float* p) { float4 v; memcpy(&v, p, 16); return v; }
static inline void st4(float* p, float4 v) { memcpy(p, &v, 16); }
#define RP_LOG2E 1.4426950408889634f
static inline float fast_exp2(float x) { return exp2f(x); }
static float __shfl(float v, int src, int) {
  const int t = threadIdx.x;
  slot[t] = v; yield_();
  float r = slot[(t & ~63) | (src & 63)]; yield_();
  return r;
}
static inline bool xcd_problem(int nq, int ZH, int& zh, int& qb) {
  const int j = blockIdx.x >> 3;
  zh = (j / nq) * 8 + (blockIdx.x & 7);
  qb = j % nq;
  return zh < ZH;
}
static inline int xcd_grid(int nq, int ZH) { return nq * ((ZH + 7) / 8) * 8; }
