// shim.h -- ../eightpoint_host/shim.h for kernels whose workgroups are not 256 threads: csrc/geom.hip launches 64 and indexes
// blockIdx.x * 64 + threadIdx.x, csrc/se3loss.hip launches 64 (blockDim.x) and 256.  The threads of a workgroup are ucontext fibres
// scheduled round-robin, __syncthreads() is a yield, workgroups run one after another, and the launch honours the block size it is given.
// It checks the kernels' LOGIC, branches and indexing under the host sanitizers; host arithmetic does not contract multiply-adds the way
// the device compiler does, so it says nothing about the last bit.  Used by run.py only.
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
static Idx threadIdx, blockIdx, blockDim;
struct dim3 { int x; dim3(int a) : x(a) {} };
typedef void* hipStream_t;
static const int NTH_MAX = 256;
static ucontext_t mainctx, ctx[NTH_MAX];
static bool done[NTH_MAX];
static int cur;
static std::function<void()> body;
static void __syncthreads() { swapcontext(&ctx[cur], &mainctx); }
static void tramp() { body(); done[cur] = true; swapcontext(&ctx[cur], &mainctx); }
static void launch(int grid, int block, std::function<void()> f) {
  if (block < 1 || block > NTH_MAX) { printf("block size %d\n", block); exit(2); }
  body = f;
  blockDim.x = block;
  static std::vector<char> stacks((size_t)NTH_MAX * (1 << 18));
  for (int b = 0; b < grid; ++b) {
    blockIdx.x = b;
    for (int t = 0; t < block; ++t) {
      getcontext(&ctx[t]); ctx[t].uc_stack.ss_sp = &stacks[(size_t)t << 18]; ctx[t].uc_stack.ss_size = 1 << 18; ctx[t].uc_link = &mainctx;
      makecontext(&ctx[t], tramp, 0); done[t] = false;
    }
    for (int left = block; left;) {            // one pass = one barrier phase: every live fibre runs to its next yield
      left = 0;
      for (int t = 0; t < block; ++t) {
        if (done[t]) continue;
        cur = t; threadIdx.x = t;
        swapcontext(&mainctx, &ctx[t]);
        left += !done[t];
      }
    }
  }
}
#define hipLaunchKernelGGL(k, grid, block, shm, stream, ...) launch((grid).x, (block).x, [=] { k(__VA_ARGS__); })
#define RP_CHECK_LAUNCH() do {} while (0)
