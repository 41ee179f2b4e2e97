// emm_readout.hip -- rp_emm_matches: which token the Essential Matrix Module paired with which (librelpose_readout.so).
//
// Per image z of a pair (partner z^1) and head h, with S = scale * q_{z^1} k_z^T [576 x 576] and the normalisers of rp_emm_stats:
//     A = exp(2 S - rlse_i - clse_j)      (single softmax: exp(S - rlse_i))
// and per "owner" (row i with swap = 0, column j with swap = 1) over the other index n:
//     idx = argmax_n of the exponent,  amax = A at idx,  mass = sum_n A,  (ex, ey) = sum_n A (n % 24, n / 24) / mass.
// The structure is rp_emm_apply's (../csrc/emm.hip): one wave = 32 owner tokens whose 64 features sit in registers (pre-scaled so that
// the accumulator is in log2 units), tiles of 32 "loop" tokens double buffered in LDS, the tile computed TRANSPOSED -- S^T[loop][owner]:
// the owner is the lane (l & 31), the 16 accumulator registers of a half-wave are 16 of the tile's 32 loop tokens -- so every
// reduction over the loop index is lane-local and the two half-waves meet in ONE xor-32 exchange at the very end.
// The normalisers cost no vector instruction: the 4 spare floats of a staged row (KST = 68) carry (-log2e lse_loop, 0, n % 24, n / 24),
// and a 33rd MFMA step  (1, -lse_loop) x (-lse_owner, 1)  adds both normalisers into the accumulator, which then IS the exponent.
// Per score that leaves: v_exp, compare + two selects (running maximum and its index), one add and two fmas.
// The dense A is a visualisation path: swap = 0 stores 16-byte runs straight from the accumulators (registers 4g .. 4g+3 of a lane
// are four consecutive j of its row i), swap = 1 stores each register as a 128-byte run per half-wave (32 consecutive j of one row i).
#include "../csrc/tile32.h"
#include "../../include/relpose_readout.h"

namespace {

// the 4 spare floats of a staged row (KST = 68): 64 features | -lse (log2 units) | 0 | n % 24 | n / 24
constexpr int NW = 3;        // waves per workgroup: 96 owner tokens
constexpr int NT = NW * 64;
constexpr int GRID = 24;     // tokens per row of the 24 x 24 token grid

struct ReadoutP {
  const float* own; const float* loop;      // first of the H*64 columns of the owner / loop side (swap: k / q, else q / k)
  int ld_own, ld_loop;
  const float* own_lse; const float* loop_lse;      // [Z][H][576]; a side the single softmax does not normalise has multiplier 0
  float own_mul, loop_mul;                  // -log2(e), or 0
  float mul;                                // owner prescale: (single ? 1 : 2) * scale * log2(e)
  int* idx; float* stat; float* a_out;
  int H, ZH, swap;
};

// the ride-along columns of loop token n = 32 t + tid (threads 0..31)
RP_DEV void aux_sstore(float* s, int tid, int t, float nlse) {
  const int n = 32 * t + tid;
  if (tid < 32) st4(s + tid * KST + 64, make_float4(nlse, 0.f, (float)(n % GRID), (float)(n / GRID)));
}

template <bool DENSE>
__global__ __launch_bounds__(NT, 3) void emm_readout_kernel(ReadoutP p) {
  __shared__ __attribute__((aligned(16))) float Ks[2 * 32 * KST];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
  int zh_, wgi;
  if (!xcd_problem(NTILE / NW, p.ZH, zh_, wgi)) return;
  const int h = zh_ % p.H, z = zh_ / p.H;
  const int o0 = wgi * (NW * 32) + wave * 32;
  const int own_img = p.swap ? z : (z ^ 1), loop_img = p.swap ? (z ^ 1) : z;
  const long long zh = zh_;
  const float* lb = p.loop + (long long)loop_img * NTOK * p.ld_loop + h * 64;

  float oreg[32];
  {      // = load_owner (tile32.h), written out: the call reschedules this kernel's prologue, and this file's device code is kept as it was
    const float* orow = p.own + ((long long)own_img * NTOK + o0 + l31) * p.ld_own + h * 64 + 32 * hi;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float4 x = ld4(orow + 4 * c);
      oreg[4 * c + 0] = x.x * p.mul; oreg[4 * c + 1] = x.y * p.mul; oreg[4 * c + 2] = x.z * p.mul; oreg[4 * c + 3] = x.w * p.mul;
    }
  }
  // the 33rd MFMA step: k = 0 (lower half-wave) pairs 1 with -lse_owner, k = 1 (upper) pairs -lse_loop with 1
  const float bx = hi ? 1.0f : p.own_lse[zh * NTOK + o0 + l31] * p.own_mul;

  const bf16x8 nopk[4] = {};      // (score_tile's bf16 operands: unused in its fp32 form)
  float4 kpre[3];
  // branch-free (every thread loads, threads 0..31 store): see emm_apply_kernel
  const float* lsrc = p.loop_lse + zh * NTOK + (tid & 31);
  float cpre = lsrc[0] * p.loop_mul;
  tile_gload<NT>(lb, p.ld_loop, tid, kpre);
  tile_sstore<NT, KST>(Ks, tid, kpre);
  aux_sstore(Ks, tid, 0, cpre);
  __syncthreads();

  float m = -INFINITY, mass = 0.f, sx = 0.f, sy = 0.f;
  int bi = 4 * hi;      // the lane's first loop token: what an owner whose exponents are all -inf reports
  for (int t = 0; t < NTILE; ++t) {
    const int cur = t & 1;
    if (t + 1 < NTILE) {
      tile_gload<NT>(lb + (long long)(t + 1) * 32 * p.ld_loop, p.ld_loop, tid, kpre);
      cpre = lsrc[(t + 1) * 32] * p.loop_mul;
    }
    const float* K = Ks + cur * 32 * KST;
    f32x16 s = score_tile<false>(K, l31, hi, oreg, nopk);      // S^T[loop][owner] in log2 units, then the exponent
    s = mfma32(hi ? K[l31 * KST + 64] : 1.0f, bx, s);
    const int n0 = 32 * t + 4 * hi;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2);      // acc_row(r, hi) - 4 hi
      const float2 xy = *reinterpret_cast<const float2*>(K + (row + 4 * hi) * KST + 66);
      const float e = s[r];
      const float a = fast_exp2(e);
      const bool g = e > m;      // strict: a lane visits its loop tokens in increasing order, ties keep the lowest
      m = g ? e : m;
      bi = g ? n0 + row : bi;
      mass += a;
      sx = fmaf(a, xy.x, sx);
      sy = fmaf(a, xy.y, sy);
      if (DENSE) s[r] = a;
    }
    if (DENSE) {
      if (p.swap) {      // owner = column j (lane), loop = row i (register)
        float* ab = p.a_out + (zh * NTOK + 32 * t + 4 * hi) * NTOK + o0 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) ab[((r & 3) + 8 * (r >> 2)) * NTOK] = s[r];
      } else {           // owner = row i (lane), loop = column j (register): registers 4g .. 4g+3 are columns 8g + 4hi .. +3
        float* ab = p.a_out + (zh * NTOK + o0 + l31) * NTOK + 32 * t + 4 * hi;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) st4(ab + 8 * g4, make_float4(s[4 * g4], s[4 * g4 + 1], s[4 * g4 + 2], s[4 * g4 + 3]));
      }
    }
    if (t + 1 < NTILE) {
      tile_sstore<NT, KST>(Ks + (cur ^ 1) * 32 * KST, tid, kpre);
      aux_sstore(Ks + (cur ^ 1) * 32 * KST, tid, t + 1, cpre);
    }
    __syncthreads();
  }

  // the two half-waves of an owner meet: (lo, hi) in this order in both lanes, so the sums are the same bits whichever lane writes
  const float m_o = __shfl_xor(m, 32, 64), mass_o = __shfl_xor(mass, 32, 64), sx_o = __shfl_xor(sx, 32, 64), sy_o = __shfl_xor(sy, 32, 64);
  const int bi_o = __shfl_xor(bi, 32, 64);
  if (hi) return;
  const bool take = m_o > m || (m_o == m && bi_o < bi);
  const float mb = take ? m_o : m;
  const int ib = take ? bi_o : bi;
  const float ms = mass + mass_o, px = sx + sx_o, py = sy + sy_o;
  const bool none = !(ms > 0.f);
  const long long o = zh * NTOK + o0 + l31;
  p.idx[o] = ib;
  st4(p.stat + 4 * o, make_float4(fast_exp2(mb), ms, none ? -1.0f : px / ms, none ? -1.0f : py / ms));
}

bool misaligned(const void* ptr) { return ((uintptr_t)ptr & 15) != 0; }

}  // namespace

extern "C" int rp_readout_abi_version(void) { return RP_READOUT_ABI_VERSION; }

extern "C" int rp_emm_matches(const float* q, const float* k, const float* rlse, const float* clse, int* idx, float* stat, float* a_out,
                              int Z, int H, int ldq, int ldk, float scale, int swap, int single, void* stream) {
  if (Z <= 0 || (Z & 1) || H <= 0 || H * 64 > ldq || H * 64 > ldk) return RP_EBADSHAPE;
  if (!q || !k || !rlse || (!single && !clse) || !idx || !stat) return RP_EBADSHAPE;
  if ((ldq & 3) || (ldk & 3)) return RP_EALIGN;
  if (misaligned(q) || misaligned(k) || misaligned(rlse) || (!single && misaligned(clse)) || misaligned(idx) || misaligned(stat) ||
      misaligned(a_out))
    return RP_EALIGN;
  ReadoutP p{};
  p.own = swap ? k : q; p.ld_own = swap ? ldk : ldq;
  p.loop = swap ? q : k; p.ld_loop = swap ? ldq : ldk;
  // single softmax: only the row side (rlse) normalises; the other side reads rlse too, with multiplier 0
  p.own_lse = (swap && !single) ? clse : rlse;
  p.loop_lse = (swap || single) ? rlse : clse;
  p.own_mul = (single && swap) ? 0.f : -RP_LOG2E;
  p.loop_mul = (single && !swap) ? 0.f : -RP_LOG2E;
  p.mul = (single ? 1.0f : 2.0f) * scale * RP_LOG2E;
  p.idx = idx; p.stat = stat; p.a_out = a_out;
  p.H = H; p.ZH = Z * H; p.swap = swap ? 1 : 0;
  const dim3 grid(xcd_grid(NTILE / NW, Z * H)), block(NT);
  if (a_out) hipLaunchKernelGGL(emm_readout_kernel<true>, grid, block, 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(emm_readout_kernel<false>, grid, block, 0, (hipStream_t)stream, p);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
