// shim.h -- just enough of the HIP programming model to run csrc_eightpoint/eight_point.hip on the HOST, thread by thread: the 256
// threads of a workgroup are ucontext fibres scheduled round-robin, __syncthreads() and every __shfl_xor are yields (so a barrier that
// not every thread reaches, or an out-of-bounds LDS / global index, shows up under the host sanitizers), workgroups run one after
// another.  It checks the kernel's LOGIC and indexing; it says nothing about races between truly parallel threads, and host
// arithmetic does not contract multiply-adds the way the device compiler does.  Used by run.py only.
#pragma once
#include <ucontext.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __restrict__
#define __launch_bounds__(x)
#define RP_DEV inline
struct Idx { int x; };
static Idx threadIdx, blockIdx;
struct dim3 { int x; dim3(int a) : x(a) {} };
struct float2 { float x, y; };
static inline float2 make_float2(float x, float y) { return float2{x, y}; }
typedef void* hipStream_t;
static const int NTH = 256;
static ucontext_t mainctx, ctx[NTH];
static bool done[NTH];
static int cur;
static std::function<void()> body;
static void yield_() { swapcontext(&ctx[cur], &mainctx); }
static void __syncthreads() { yield_(); }
static float slot[NTH];
static float __shfl_xor(float v, int o, int) {
  const int t = threadIdx.x;
  slot[t] = v; yield_();
  float r = slot[(t & ~63) | ((t & 63) ^ o)]; yield_();
  return r;
}
RP_DEV float wave_sum(float v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; }
static void tramp() { body(); done[cur] = true; swapcontext(&ctx[cur], &mainctx); }
static void launch(int grid, std::function<void()> f) {
  body = f;
  static std::vector<char> stacks((size_t)NTH * (1 << 18));
  for (int b = 0; b < grid; ++b) {
    blockIdx.x = b;
    for (int t = 0; t < NTH; ++t) {
      getcontext(&ctx[t]); ctx[t].uc_stack.ss_sp = &stacks[(size_t)t << 18]; ctx[t].uc_stack.ss_size = 1 << 18; ctx[t].uc_link = &mainctx;
      makecontext(&ctx[t], tramp, 0); done[t] = false;
    }
    for (int left = NTH; left;) {              // one pass = one barrier phase: every live fibre runs to its next yield
      left = 0;
      for (int t = 0; t < NTH; ++t) {
        if (done[t]) continue;
        cur = t; threadIdx.x = t;
        swapcontext(&mainctx, &ctx[t]);
        left += !done[t];
      }
    }
  }
}
#define hipLaunchKernelGGL(k, grid, block, shm, stream, ...) launch((grid).x, [=] { k(__VA_ARGS__); })
#define RP_CHECK_LAUNCH() do {} while (0)
