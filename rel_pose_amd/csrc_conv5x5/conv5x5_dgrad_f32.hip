// conv5x5_dgrad_f32.hip -- input gradient of the two valid 5x5 convolutions of extractor_final_conv (conv2 192 -> 192, downsample.0
// 128 -> 192; 28 x 28 -> 24 x 24), exact fp32, deterministic: no atomics, no split-K, no workspace, no filter preparation.
//
//     dx[n][y][x][ci] = res[n][y][x][ci] + sum_{r, s, co} dy[n][y - r][x - s][co] * w[co][r][s][ci]        (dy = 0 outside 0..23)
//
// Gathered over whole output tiles of consecutive pixels this is a GEMM of K = 25 x 192 whose rows multiply (28 / 24)^2 = 1.36 x the
// products the convolution has: the border pixels' taps that fall outside dy are zeros, and a 32-row matrix instruction cannot skip
// rows.  So the rows of a tile here are the SAME pixel (y, x) of 128 IMAGES: which taps fall inside dy is then a property of the
// workgroup, not of the row, and the workgroup simply walks the valid taps -- (min(y, 4) - max(0, y - 23) + 1) x (the same in x), 1 to
// 25 of them -- and forms no product with a zero.  The 784 pixels are dealt heaviest first (ORDER), so the chip's in-order dispatch
// balances the 14 400 tap-units over the CUs by itself.
//   * workgroup = [128 images x CI] accumulator tile of one pixel, 4 waves = 2 image halves x 2 channel halves, ONE wave per SIMD
//     (dw192_f32.hip: the fp32 matrix instruction holds its rate only so): 2 x CI / 64 accumulator tiles of 32 x 32 per wave;
//   * K walked as (64-channel chunk of dy) x (valid r) x (valid s): neighbouring pixels read the same dy rows one stage apart;
//   * both operands by LDS-DMA, two buffers (160 KB at CI = 192, which also keeps a second workgroup off the CU), one piece issued
//     per k-step in the shadow of that step's matrix instructions;
//   * filter stage: 64 rows of CI floats, 25 CI floats apart, copied as they lie and contracted along the ROW index: one conflict-free
//     4-byte read per lane and k-step (dw192_f32.hip's operand);
//   * activation stage: 256 contiguous bytes per image, contracted along the CONTIGUOUS index: a lane reads 16 bytes = 4 k-steps of
//     its image; the sixteen 16-byte chunks of row i sit at position chunk ^ (i & 15) -- laid out through the DMA's per-lane source
//     address --, so the sixteen lanes the LDS serves together hit sixteen different bank groups;
//   * images past N: loads clamped to image N - 1, stores masked.
#include "../csrc/common.h"
#include "../../include/relpose_conv5x5.h"

namespace {

constexpr int CO = 192;                  // channels of dy
constexpr int HO = 24;                   // dy is HO x HO,
constexpr int HI = 28;                   // dx HI x HI,
constexpr int KS = 5;                    // the filter KS x KS
constexpr int PIX = HI * HI;
constexpr int IB = 128;                  // images per workgroup
constexpr int SK = 64;                   // channels of dy per stage
constexpr int FOLD = 5;                  // stages per partial sum
constexpr int A_FL = IB * SK;            // floats of an activation stage (32 KB)
constexpr int DY_IMG = HO * HO * CO;     // floats of one image of dy

// the taps r with 0 <= v - r <= HO - 1 are lo(v) .. hi(v)
constexpr int tap_lo(int v) { return v > HO - 1 ? v - (HO - 1) : 0; }
constexpr int tap_hi(int v) { return v < KS - 1 ? v : KS - 1; }
constexpr int taps(int pix) {
  const int y = pix / HI, x = pix % HI;
  return (tap_hi(y) - tap_lo(y) + 1) * (tap_hi(x) - tap_lo(x) + 1);
}

// dispatch order of the pixels: most taps first, row-major among equals.  The 400 interior pixels (25 taps) lead; workgroup j runs on
// XCD j % 8, so those are dealt 50 consecutive ones to each XCD: the workgroups that share an L2 read overlapping rows of dy.
struct Order { unsigned short v[PIX]; };
constexpr Order make_order() {
  Order o{};
  int k = 0;
  for (int t = KS * KS; t >= 1; --t)
    for (int p = 0; p < PIX; ++p)
      if (taps(p) == t) o.v[k++] = (unsigned short)p;
  Order q = o;
  for (int j = 0; j < 400; ++j) q.v[j] = o.v[50 * (j & 7) + (j >> 3)];
  return q;
}
__constant__ Order ORDER = make_order();

struct Dg {
  const float* dy; const float* w; const float* res; float* dx;
  int N, groups;
};

template <int CI>
__global__ __launch_bounds__(256, 1) void conv5x5_dgrad_f32_kernel(Dg p) {
  constexpr int B_FL = SK * CI;          // floats of a filter stage (48 KB / 32 KB)
  constexpr int CB = CI / 64;            // 32-channel blocks of a wave's half of CI
  constexpr int NA = A_FL / 1024;        // 1-KB pieces of a stage per wave: 8 of the activations,
  constexpr int NB = B_FL / 1024;        // 12 / 8 of the filter
  constexpr int KSTEPS = SK / 2;
  static_assert(NA + NB <= KSTEPS, "one DMA piece per k-step");
  __shared__ __attribute__((aligned(16))) float As[2][A_FL];
  __shared__ __attribute__((aligned(16))) float Bs[2][B_FL];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, hi = lane >> 5;
  const int pos = blockIdx.x / p.groups, grp = blockIdx.x - pos * p.groups;
  const int pix = ORDER.v[pos], y = pix / HI, x = pix - y * HI;
  const int r0 = tap_lo(y), r1 = tap_hi(y), s0 = tap_lo(x), s1 = tap_hi(x);
  const int nst = (CO / SK) * (r1 - r0 + 1) * (s1 - s0 + 1);
  const int n0 = grp * IB;
  const float* dyb = p.dy + (long long)n0 * DY_IMG;

  // DMA plan.  Activations: piece q = rows 4 q .. 4 q + 3 of the stage image [128 images][16 chunks of 16 B]; lane (row, position)
  // fetches chunk position ^ (row & 15) of its image.  Filter: [64 rows][CI floats] copied as it lies.  Wave w moves pieces w, w + 4, ...
  unsigned aoff[NA], boff[NB];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int row = 4 * (wave + 4 * i) + (lane >> 4);
    const int img = min(row, p.N - 1 - n0);
    aoff[i] = (unsigned)img * (unsigned)(DY_IMG * 4) + (unsigned)((((lane & 15) ^ (row & 15))) << 4);
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int byte = (wave + 4 * i) * 1024 + lane * 16;
    const int row = byte / (CI * 4), c = byte % (CI * 4);
    boff[i] = (unsigned)(row * (KS * KS * CI * 4) + c);
  }
  const unsigned as0 = lds_byte_addr(&As[0][0]) + wave * 1024, bs0 = lds_byte_addr(&Bs[0][0]) + wave * 1024;
  auto a_src = [&](int ch, int r, int s) { return uniform_ptr(dyb + ((y - r) * HO + (x - s)) * CO + ch * SK); };
  auto b_src = [&](int ch, int r, int s) { return uniform_ptr(p.w + ((long long)(ch * SK) * (KS * KS) + r * KS + s) * CI); };

  const int wr = wave >> 1, wc = wave & 1;                     // this wave's 64 images x CI / 2 channels
  const int m15 = l31 & 15;
  const int ao = (64 * wr + l31) * (SK / 4);                   // in 16-byte chunks
  const int bo = 4 * hi * CI + (CI / 2) * wc + l31;            // k-step (g, e) contracts channel 8 g + 4 hi + e of the stage
  // Two levels of accumulation: a chain of 4800 fp32 additions per element has about three times the rounding error of MIOpen's
  // kernel on the same products, so the matrix instructions run on `acc` for FOLD stages (at most 320 products) and `sum` collects
  // those partial sums -- 15 of them at 25 taps.  The fold is 3 vector instructions per register every FOLD stages.
  f32x16 acc[2][CB], sum[2][CB];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int j = 0; j < CB; ++j) acc[b][j] = sum[b][j] = zero16();
  int fold = FOLD;

  int nch = 0, nr = r0, ns = s0;                               // the stage in flight
  {
    const void* sa = a_src(nch, nr, ns);
    const void* sb = b_src(nch, nr, ns);
#pragma unroll
    for (int i = 0; i < NA; ++i) glds16(sa, aoff[i], as0 + i * 4096);
#pragma unroll
    for (int i = 0; i < NB; ++i) glds16(sb, boff[i], bs0 + i * 4096);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  for (int st = 0; st < nst; ++st) {
    const int buf = st & 1;
    // next stage: s fastest, then r, then the channel chunk; the last stage re-fetches itself into the dead buffer (no branch below)
    if (st + 1 < nst) {
      if (ns < s1) ++ns;
      else {
        ns = s0;
        if (nr < r1) ++nr;
        else { nr = r0; ++nch; }
      }
    }
    const void* sa = a_src(nch, nr, ns);
    const void* sb = b_src(nch, nr, ns);
    const unsigned an0 = as0 + (buf ^ 1) * (A_FL * 4), bn0 = bs0 + (buf ^ 1) * (B_FL * 4);
    const float4* ap = reinterpret_cast<const float4*>(As[buf]) + ao;
    const unsigned bt = lds_byte_addr(Bs[buf] + bo);
    // operands one step ahead of their use (one wave per SIMD: nobody else hides the LDS latency): the filter values of k-step t + 1
    // and, every fourth step, the activation chunks of the next four are read while the matrix instructions of step t run
    float4 ac[2], an[2];
    float bf[CB], bn[CB];
#pragma unroll
    for (int b = 0; b < 2; ++b) ac[b] = ap[b * 32 * (SK / 4) + (hi ^ m15)];
    static_for<CB>([&](auto j) { bf[j] = lds_rd32<128 * j>(bt); });
    static_for<KSTEPS>([&](auto tt) {
      constexpr int t = tt, g = t / 4, e = t % 4;
      if constexpr (CB == 3) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bf[0]), "+v"(bf[1]), "+v"(bf[CB - 1]));
      else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bf[0]), "+v"(bf[1]));
      if constexpr (t + 1 < KSTEPS) {
        constexpr int g1 = (t + 1) / 4, e1 = (t + 1) % 4;
        static_for<CB>([&](auto j) { bn[j] = lds_rd32<((8 * g1 + e1) * CI + 32 * j) * 4>(bt); });
        if constexpr (e == 0 && g + 1 < KSTEPS / 4) {
#pragma unroll
          for (int b = 0; b < 2; ++b) an[b] = ap[b * 32 * (SK / 4) + ((2 * (g + 1) + hi) ^ m15)];
        }
      }
      if constexpr (t < NA) glds16(sa, aoff[t < NA ? t : 0], an0 + t * 4096);
      else if constexpr (t < NA + NB) glds16(sb, boff[t >= NA && t < NA + NB ? t - NA : 0], bn0 + (t - NA) * 4096);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const float av = e == 0 ? ac[b].x : e == 1 ? ac[b].y : e == 2 ? ac[b].z : ac[b].w;
#pragma unroll
        for (int j = 0; j < CB; ++j) acc[b][j] = mfma32(av, bf[j], acc[b][j]);
      }
      if constexpr (t + 1 < KSTEPS) {
#pragma unroll
        for (int j = 0; j < CB; ++j) bf[j] = bn[j];
        if constexpr (e == 3) {
          ac[0] = an[0];
          ac[1] = an[1];
        }
      }
      __builtin_amdgcn_sched_barrier(0);       // (the next step's wait stays behind this step's matrix instructions)
    });
    if (--fold == 0) {
      fold = FOLD;
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int j = 0; j < CB; ++j) {
          sum[b][j] += acc[b][j];
          acc[b][j] = zero16();
        }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int j = 0; j < CB; ++j) acc[b][j] += sum[b][j];

  // rows = images n0 + 64 wr + 32 b + acc_row(r, hi), columns = channels (CI / 2) wc + 32 j + l31: 128-byte segments of dx
  // (res is read at the clamped image, so a block's loads are all in flight together; the stores are masked)
  const int ci = (CI / 2) * wc + l31;
  const float* __restrict__ res = p.res;
  float* __restrict__ dx = p.dx;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int img0 = n0 + 64 * wr + 32 * b;
    if (res) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const size_t o = ((size_t)min(img0 + acc_row(r, hi), p.N - 1) * PIX + pix) * CI + ci;
#pragma unroll
        for (int j = 0; j < CB; ++j) acc[b][j][r] += res[o + 32 * j];
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int img = img0 + acc_row(r, hi);
      if (img < p.N) {
        const size_t o = ((size_t)img * PIX + pix) * CI + ci;
#pragma unroll
        for (int j = 0; j < CB; ++j) dx[o + 32 * j] = acc[b][j][r];
      }
    }
  }
}

}  // namespace

extern "C" int rp_conv5x5_abi_version(void) { return RP_CONV5X5_ABI_VERSION; }

extern "C" int rp_conv5x5_dgrad_f32(const float* dy, const float* w, float* dx, int N, int CI, const float* res, void* stream) {
  if (N < 1 || !dy || !w || !dx) return RP_EBADSHAPE;
  if (CI != 128 && CI != 192) return RP_EUNSUPPORTED;
  if (((uintptr_t)dy | (uintptr_t)w | (uintptr_t)dx | (uintptr_t)res) & 15) return RP_EALIGN;
  Dg p;
  p.dy = dy; p.w = w; p.res = res; p.dx = dx; p.N = N;
  p.groups = (N + IB - 1) / IB;
  const dim3 grid((unsigned)PIX * (unsigned)p.groups);
  if (CI == 192) hipLaunchKernelGGL(conv5x5_dgrad_f32_kernel<192>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(conv5x5_dgrad_f32_kernel<128>, grid, dim3(256), 0, (hipStream_t)stream, p);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
