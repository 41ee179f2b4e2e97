// emm_guided.hip -- rp_emm_guided_matches: the EMM's matches read again under a pose (librelpose_guided.so).
//
// A sibling of emm_readout_kernel (../csrc_readout/emm_readout.hip), and its structure: one wave = 32 owner tokens whose 64 features
// sit in registers, tiles of 32 "loop" tokens double buffered in LDS, the tile computed TRANSPOSED -- S^T[loop][owner], the owner is
// the lane -- and the two normalisers added by a 33rd MFMA step, so the accumulator IS the exponent in log2 units.
// What is new is the admission of a pair under the fundamental matrix of image z's problem (include/relpose_guided.h states the
// arithmetic): with G = F_z 2^-k (max|G| in [0.5, 1)), l = G r_i the line of row token i and m = (G^T c_j)_xy,
//     rho = c_j . l,   den = (lx^2 + ly^2) + (mx^2 + my^2),   admitted iff not (den > 0) or rho^2 <= band^2 den.
// The owner's half of that is lane-local and formed once; the loop tokens' half is a float4 per token, all 576 formed once per
// workgroup into LDS beside the tiles (9 KB; the matrix is then out of the loop's registers):
//     swap = 0 (owner row i, loop column j):  owner (lx, ly, lz, l2),  loop (cx, cy, 0, m2)
//     swap = 1 (owner column j, loop row i):  owner (cx, cy, 1, m2),  loop (lx, ly, lz, l2)
// so that rho = fma(cx, lx, fma(cy, ly, lz)) has the same bits whichever side owns.  Per score that is, beside v_exp and the running
// maximum of the readout: two fmas, an add, two multiplies, a compare and the selects.  The aux read is one broadcast ds_read_b128
// per accumulator row (all lanes of a half-wave read the same address).
#include "../csrc/tile32.h"
#include "../csrc/two_view.h"
#include "../../include/relpose_guided.h"

namespace {

constexpr int NW = 3;        // waves per workgroup: 96 owner tokens
constexpr int NT = NW * 64;
constexpr int GRID = 24;     // tokens per row of the 24 x 24 token grid

struct GuidedP {
  const float* own; const float* loop;      // first of the H*64 columns of the owner / loop side (swap: k / q, else q / k)
  int ld_own, ld_loop;
  const float* own_lse; const float* loop_lse;      // [Z][H][576]; a side the single softmax does not normalise has multiplier 0
  float own_mul, loop_mul;                  // -log2(e), or 0
  float mul;                                // owner prescale: (single ? 1 : 2) * scale * log2(e)
  const float* F; const float* band;        // [Z][9], [Z]
  int* idx; float* stat;
  int H, ZH;
};

// token n as a ROW token of the problem: (lx, ly, lz, l2) of l = G r_n
RP_DEV float4 row_side(const float (&G)[9], int n) {
  const float x = (float)(n % GRID), y = (float)(n / GRID);
  const float lx = fmaf(G[0], x, fmaf(G[1], y, G[2])), ly = fmaf(G[3], x, fmaf(G[4], y, G[5])), lz = fmaf(G[6], x, fmaf(G[7], y, G[8]));
  return make_float4(lx, ly, lz, fmaf(lx, lx, ly * ly));
}

// token n as a COLUMN token: (cx, cy, z, m2) of m = (G^T c_n)_xy; z is the owner's 1 or the loop side's 0 (never read there)
RP_DEV float4 col_side(const float (&G)[9], int n, float z) {
  const float x = (float)(n % GRID), y = (float)(n / GRID);
  const float mx = fmaf(G[0], x, fmaf(G[3], y, G[6])), my = fmaf(G[1], x, fmaf(G[4], y, G[7]));
  return make_float4(x, y, z, fmaf(mx, mx, my * my));
}

// the ride-along value of loop token n = 32 t + tid (threads 0..31): -lse in the tile's spare column 64
RP_DEV void aux_sstore(float* s, int tid, float nlse) {
  if (tid < 32) st4(s + tid * KST + 64, make_float4(nlse, 0.f, 0.f, 0.f));
}

template <bool SWAP>
__global__ __launch_bounds__(NT, 3) void emm_guided_kernel(GuidedP p) {
  __shared__ __attribute__((aligned(16))) float Ks[2 * 32 * KST];
  __shared__ float4 Ax[NTOK];      // the loop side of the admission, all 576 tokens, formed once
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
  int zh_, wgi;
  if (!xcd_problem(NTILE / NW, p.ZH, zh_, wgi)) return;
  const int h = zh_ % p.H, z = zh_ / p.H;
  const int o0 = wgi * (NW * 32) + wave * 32;
  const int own_img = SWAP ? z : (z ^ 1), loop_img = SWAP ? (z ^ 1) : z;
  const long long zh = zh_;
  const long long o = zh * NTOK + o0 + l31;

  // the problem's matrix (uniform over the workgroup: scalar loads), its degeneracy, its scale
  float G[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) G[c] = p.F[z * 9 + c];
  const float band = p.band[z];
  float big = 0.f;
#pragma unroll
  for (int c = 0; c < 9; ++c) big = fmaxf(big, fabsf(G[c]));
  if (!all_finite(G) || !(big > 0.f) || !(band > 0.f)) {      // uniform: the whole workgroup leaves before any barrier
    if (!hi) {
      p.idx[o] = -1;
      st4(p.stat + 4 * o, make_float4(0.f, 0.f, 0.f, 0.f));
    }
    return;
  }
  int ex;      // max|F| = f 2^ex with f in [0.5, 1): the scaling by 2^-ex is exact, so integer matrices stay integer ratios
  (void)frexpf(big, &ex);
#pragma unroll
  for (int c = 0; c < 9; ++c) G[c] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ldexpf(G[c], -ex))));      // uniform: scalar registers
  const float b2 = band * band;
  const float4 ow = SWAP ? col_side(G, o0 + l31, 1.f) : row_side(G, o0 + l31);

  const float* lb = p.loop + (long long)loop_img * NTOK * p.ld_loop + h * 64;
  float oreg[32];
  load_owner(p.own + ((long long)own_img * NTOK + o0 + l31) * p.ld_own + h * 64, hi, p.mul, oreg);
  // the 33rd MFMA step: k = 0 (lower half-wave) pairs 1 with -lse_owner, k = 1 (upper) pairs -lse_loop with 1
  const float bx = hi ? 1.0f : p.own_lse[o] * p.own_mul;

  const bf16x8 nopk[4] = {};      // (score_tile's bf16 operands: unused in its fp32 form)
  float4 kpre[3];
  const float* lsrc = p.loop_lse + zh * NTOK + (tid & 31);
  float cpre = lsrc[0] * p.loop_mul;
  tile_gload<NT>(lb, p.ld_loop, tid, kpre);
  tile_sstore<NT, KST>(Ks, tid, kpre);
  aux_sstore(Ks, tid, cpre);
#pragma unroll
  for (int n = tid; n < NTOK; n += NT) Ax[n] = SWAP ? row_side(G, n) : col_side(G, n, 0.f);
  __syncthreads();

  float m = -INFINITY, mass = 0.f, bmass = 0.f;
  int bi = -1;
  for (int t = 0; t < NTILE; ++t) {
    const int cur = t & 1;
    if (t + 1 < NTILE) {
      tile_gload<NT>(lb + (long long)(t + 1) * 32 * p.ld_loop, p.ld_loop, tid, kpre);
      cpre = lsrc[(t + 1) * 32] * p.loop_mul;
    }
    const float* K = Ks + cur * 32 * KST;
    const float4* A = Ax + 32 * t + 4 * hi;
    f32x16 s = score_tile<false>(K, l31, hi, oreg, nopk);      // S^T[loop][owner] in log2 units, then the exponent
    s = mfma32(hi ? K[l31 * KST + 64] : 1.0f, bx, s);
    const int n0 = 32 * t + 4 * hi;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2);      // acc_row(r, hi) - 4 hi
      const float4 lp = A[row];
      const float e = s[r];
      const float a = fast_exp2(e);
      const float rho = SWAP ? fmaf(ow.x, lp.x, fmaf(ow.y, lp.y, lp.z)) : fmaf(lp.x, ow.x, fmaf(lp.y, ow.y, ow.z));
      const float den = SWAP ? lp.w + ow.w : ow.w + lp.w;      // l2 + m2
      const bool adm = !(den > 0.f) || rho * rho <= b2 * den;
      const bool g = adm && e > m;      // strict: a lane visits its loop tokens in increasing order, ties keep the lowest
      m = g ? e : m;
      bi = g ? n0 + row : bi;
      mass += a;
      bmass += adm ? a : 0.f;
    }
    if (t + 1 < NTILE) {
      tile_sstore<NT, KST>(Ks + (cur ^ 1) * 32 * KST, tid, kpre);
      aux_sstore(Ks + (cur ^ 1) * 32 * KST, tid, cpre);
    }
    __syncthreads();
  }

  // the two half-waves of an owner meet: (lo, hi) in this order in both lanes, so the sums are the same bits whichever lane writes
  const float m_o = __shfl_xor(m, 32, 64), mass_o = __shfl_xor(mass, 32, 64), bmass_o = __shfl_xor(bmass, 32, 64);
  const int bi_o = __shfl_xor(bi, 32, 64);
  if (hi) return;
  const bool take = m_o > m || (m_o == m && bi_o < bi);
  const float mb = take ? m_o : m;
  const int ib = take ? bi_o : bi;
  const bool none = ib < 0;
  const int me = o0 + l31, other = none ? 0 : ib;
  const int ri = SWAP ? other : me, cj = SWAP ? me : other;      // the chosen pair as (row token, column token)
  const float d2 = sampson(G, make_float2((float)(ri % GRID), (float)(ri / GRID)), make_float2((float)(cj % GRID), (float)(cj / GRID)));
  p.idx[o] = ib;
  st4(p.stat + 4 * o, make_float4(none ? 0.f : fast_exp2(mb), bmass + bmass_o, mass + mass_o, none ? 0.f : d2));
}

bool misaligned(const void* ptr, uintptr_t mask) { return ((uintptr_t)ptr & mask) != 0; }

}  // namespace

extern "C" int rp_guided_abi_version(void) { return RP_GUIDED_ABI_VERSION; }

extern "C" int rp_emm_guided_matches(const float* q, const float* k, const float* rlse, const float* clse, const float* F, const float* band,
                                     int* idx, float* stat, int Z, int H, int ldq, int ldk, float scale, int swap, int single, void* stream) {
  if (Z <= 0 || (Z & 1) || H <= 0 || H * 64 > ldq || H * 64 > ldk) return RP_EBADSHAPE;
  if (!q || !k || !rlse || (!single && !clse) || !F || !band || !idx || !stat) return RP_EBADSHAPE;
  if ((ldq & 3) || (ldk & 3)) return RP_EALIGN;
  if (misaligned(q, 15) || misaligned(k, 15) || misaligned(rlse, 15) || (!single && misaligned(clse, 15)) || misaligned(idx, 15) ||
      misaligned(stat, 15) || misaligned(F, 3) || misaligned(band, 3))
    return RP_EALIGN;
  GuidedP p{};
  p.own = swap ? k : q; p.ld_own = swap ? ldk : ldq;
  p.loop = swap ? q : k; p.ld_loop = swap ? ldq : ldk;
  // single softmax: only the row side (rlse) normalises; the other side reads rlse too, with multiplier 0
  p.own_lse = (swap && !single) ? clse : rlse;
  p.loop_lse = (swap || single) ? rlse : clse;
  p.own_mul = (single && swap) ? 0.f : -RP_LOG2E;
  p.loop_mul = (single && !swap) ? 0.f : -RP_LOG2E;
  p.mul = (single ? 1.0f : 2.0f) * scale * RP_LOG2E;
  p.F = F; p.band = band; p.idx = idx; p.stat = stat;
  p.H = H; p.ZH = Z * H;
  const dim3 grid(xcd_grid(NTILE / NW, Z * H)), block(NT);
  if (swap) hipLaunchKernelGGL(emm_guided_kernel<true>, grid, block, 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(emm_guided_kernel<false>, grid, block, 0, (hipStream_t)stream, p);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
