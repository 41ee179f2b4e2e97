// submatch.hip -- rp_emm_submatch: where between the token centres a match of the Essential Matrix Module lies (librelpose_submatch.so).
//
// Per image z of a pair (partner z^1), head h and owner token (row i with swap = 0, column j with swap = 1), around the token n0 = idx
// that rp_emm_matches named: the exponents e = 2 S - rlse - clse (single: S - rlse) of the (2 radius + 1)^2 tokens of the window,
// their soft-argmax / mass / spread (win) and the vertex of the parabola through the centre and its two neighbours per axis (quad).
// include/relpose_submatch.h states the arithmetic.
//
// The work per owner is up to 25 dot products of length 64 against rows GATHERED around idx: loads and their latency, nothing for the
// matrix pipe.  Mapping: a group of 32 lanes per owner, a lane per window slot (slot s = (dy + radius) (2 radius + 1) + dx + radius, so
// neighbouring lanes read consecutive 256-byte rows), two owners per wave, eight per workgroup; 576 = 72 x 8, so a workgroup stays
// inside one (z, h) and the XCD-aware order of common.h keeps the 147 KB a problem gathers from in ONE L2.  A lane issues its sixteen
// 16-byte loads back to back and only then starts the FMA chain.  The owners' own vectors (always in bounds: they do not depend on idx)
// are staged once per workgroup in 2 KB of LDS and read from there as broadcasts.  Every reduction is an xor butterfly below 32: it
// stays inside the group, both partners add the same two numbers, so all 32 lanes hold the same bits and any of them may write.
// A slot outside the grid, and every slot of an invalid owner, skips the branch that forms the address; its exponent is -inf and its
// weight exactly 0.
#include "../csrc/common.h"
#include "../../include/relpose_submatch.h"

namespace {

constexpr int NT = 256;        // threads per workgroup
constexpr int OWN = NT / 32;   // owners per workgroup
constexpr int TOK = 576;       // tokens per image
constexpr int GRID = 24;       // tokens per row of the 24 x 24 token grid
constexpr int HD = 64;         // head dim

struct SubmatchP {
  const float* own; const float* loop;              // first of the H*64 columns of the owner / loop side (swap: k / q, else q / k)
  int ld_own, ld_loop;
  const float* own_lse; const float* loop_lse;      // [Z][H][576], or NULL: a side the single softmax does not normalise
  const int* idx; float* win; float* quad;
  float mul;                                        // (single ? 1 : 2) * scale
  int H, ZH, swap, radius;
};

RP_DEV float group_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

RP_DEV float group_max(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// one axis of the vertex: a, b, c the exponents at -1, 0, +1; both: the two neighbours are inside the grid
RP_DEV void vertex(float a, float b, float c, bool both, float& off, float& curv) {
  curv = both ? (b - a) + (b - c) : 0.f;
  off = (both && curv > 0.f) ? fminf(fmaxf(0.5f * (c - a) / curv, -0.5f), 0.5f) : 0.f;
}

__global__ __launch_bounds__(NT) void emm_submatch_kernel(SubmatchP p) {
  __shared__ __attribute__((aligned(16))) float Os[OWN * HD];
  const int tid = threadIdx.x, g = tid >> 5, s = tid & 31;
  int zh_, wgi;
  if (!xcd_problem(TOK / OWN, p.ZH, zh_, wgi)) return;
  const int h = zh_ % p.H, z = zh_ / p.H;
  const int own_img = p.swap ? z : (z ^ 1), loop_img = p.swap ? (z ^ 1) : z;
  const long long zh = zh_;

  // the eight owners' vectors: thread t stages floats 4 t .. 4 t + 3 of the 8 x 64 block (16 lanes per owner row)
  if (tid < OWN * HD / 4) {
    const int r = tid >> 4, c = tid & 15;
    const float* orow = p.own + ((long long)own_img * TOK + wgi * OWN + r) * p.ld_own + h * HD;
    st4(Os + 4 * tid, ld4(orow + 4 * c));
  }
  const int tok = wgi * OWN + g;                    // the owner token
  const long long o = zh * TOK + tok;
  const int n0 = p.idx[o];
  const bool valid = (unsigned)n0 < (unsigned)TOK;
  const int W = 2 * p.radius + 1;
  const int dx = s % W - p.radius, dy = s / W - p.radius;
  const int x0 = valid ? n0 % GRID : 0, y0 = valid ? n0 / GRID : 0;
  const int x = x0 + dx, y = y0 + dy;
  const bool live = valid && s < W * W && x >= 0 && x < GRID && y >= 0 && y < GRID;
  const float lse_own = p.own_lse ? p.own_lse[o] : 0.f;
  __syncthreads();

  float e = -INFINITY;
  if (live) {      // the only place an address depends on idx
    const int n = y * GRID + x;
    const float* row = p.loop + ((long long)loop_img * TOK + n) * p.ld_loop + h * HD;
    float4 kv[HD / 4];
#pragma unroll
    for (int c = 0; c < HD / 4; ++c) kv[c] = ld4(row + 4 * c);
    const float lse_loop = p.loop_lse ? p.loop_lse[zh * TOK + n] : 0.f;
    const float* ov = Os + g * HD;
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < HD / 4; ++c) {
      const float4 a = ld4(ov + 4 * c);
      dot = fmaf(a.x, kv[c].x, dot);
      dot = fmaf(a.y, kv[c].y, dot);
      dot = fmaf(a.z, kv[c].z, dot);
      dot = fmaf(a.w, kv[c].w, dot);
    }
    e = fmaf(p.mul, dot, -lse_own) - lse_loop;
  }

  // the window: every lane of the group ends up with the same bits
  const float emax = group_max(e);
  const float u = live ? fast_exp2((e - emax) * RP_LOG2E) : 0.f;
  const float fdx = (float)dx, fdy = (float)dy;
  const float su = group_sum(u);
  const float sx = group_sum(u * fdx);
  const float sy = group_sum(u * fdy);
  const float sm = group_sum(live ? fast_exp2(e * RP_LOG2E) : 0.f);
  const float mx = valid ? sx / su : 0.f, my = valid ? sy / su : 0.f;      // (an invalid owner: su = 0)
  const float rx = fdx - mx, ry = fdy - my;
  const float sv = group_sum(u * fmaf(rx, rx, ry * ry));

  // the vertex: the exponents of the centre and its four neighbours sit in lanes of this group
  const int base = (tid & 32) + p.radius * W + p.radius;
  const float eb = __shfl(e, base, 64);
  const float exm = __shfl(e, base - 1, 64), exp_ = __shfl(e, base + 1, 64);
  const float eym = __shfl(e, base - W, 64), eyp = __shfl(e, base + W, 64);
  float offx, offy, cx, cy;
  vertex(exm, eb, exp_, valid && x0 > 0 && x0 < GRID - 1, offx, cx);
  vertex(eym, eb, eyp, valid && y0 > 0 && y0 < GRID - 1, offy, cy);

  if (s == 0)
    st4(p.win + 4 * o, valid ? make_float4((float)x0 + mx, (float)y0 + my, sm, sv / su) : make_float4(-1.f, -1.f, 0.f, 0.f));
  if (s == 1)
    st4(p.quad + 4 * o, valid ? make_float4((float)x0 + offx, (float)y0 + offy, cx, cy) : make_float4(-1.f, -1.f, 0.f, 0.f));
}

bool misaligned(const void* ptr, uintptr_t a = 15) { return ((uintptr_t)ptr & a) != 0; }

}  // namespace

extern "C" int rp_submatch_abi_version(void) { return RP_SUBMATCH_ABI_VERSION; }

extern "C" int rp_emm_submatch(const float* q, const float* k, const float* rlse, const float* clse, const int* idx, float* win, float* quad,
                               int Z, int H, int ldq, int ldk, float scale, int swap, int single, int radius, void* stream) {
  if (Z <= 0 || (Z & 1) || H <= 0 || H * 64 > ldq || H * 64 > ldk) return RP_EBADSHAPE;
  if (!q || !k || !rlse || (!single && !clse) || !idx || !win || !quad) return RP_EBADSHAPE;
  if (radius < 1 || radius > 2) return RP_EUNSUPPORTED;
  if ((long long)Z * H > (long long)(0x7fffffff / (TOK / OWN)) - 8) return RP_EUNSUPPORTED;
  if ((ldq & 3) || (ldk & 3)) return RP_EALIGN;
  if (misaligned(q) || misaligned(k) || misaligned(rlse) || (!single && misaligned(clse)) || misaligned(idx, 3) || misaligned(win) ||
      misaligned(quad))
    return RP_EALIGN;
  SubmatchP p{};
  p.own = swap ? k : q; p.ld_own = swap ? ldk : ldq;
  p.loop = swap ? q : k; p.ld_loop = swap ? ldq : ldk;
  // single softmax: only the row side (rlse) normalises
  p.own_lse = swap ? (single ? nullptr : clse) : rlse;
  p.loop_lse = swap ? rlse : (single ? nullptr : clse);
  p.idx = idx; p.win = win; p.quad = quad;
  p.mul = (single ? 1.0f : 2.0f) * scale;
  p.H = H; p.ZH = Z * H; p.swap = swap ? 1 : 0; p.radius = radius;
  const dim3 grid(xcd_grid(TOK / OWN, Z * H)), block(NT);
  hipLaunchKernelGGL(emm_submatch_kernel, grid, block, 0, (hipStream_t)stream, p);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
