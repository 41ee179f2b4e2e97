// tile32.h -- the fp32 32 x 32 tile helpers of the 576-token kernels (attention.hip, emm.hip, ../csrc_readout/emm_readout.hip): one wave
// owns 32 "owner" rows whose 64 features sit in registers, tiles of 32 "loop" rows x 64 features are staged in LDS, and the score tile is
// computed TRANSPOSED (S^T[loop][owner]) so that the owner is the lane.
#pragma once
#include "common.h"

constexpr int NTOK = 576;
constexpr int KST = 68;   // LDS row stride (floats) for tiles read along d with ds_read_b128
constexpr int NTILE = NTOK / 32;

// cooperative global -> register prefetch of a [32][64] tile (32 rows x 16 float4).  No exec-masked guards: when the
// thread count does not divide 512 the surplus threads of the last round re-load (and later re-store) element 511-ish
// duplicates -- a guarded load becomes its own basic block and hipcc then drains vmcnt(0) before every one of them.
template <int NT, bool CLAMP = (512 % NT != 0)>
RP_DEV void tile_gload(const float* base, int ld, int tid, float4 (&r)[(512 + NT - 1) / NT]) {
#pragma unroll
  for (int j = 0; j < (512 + NT - 1) / NT; ++j) {
    int f = tid + NT * j;
    if (CLAMP) f = min(f, 511);
    r[j] = ld4(base + (long long)(f >> 4) * ld + (f & 15) * 4);
  }
}
template <int NT, int STRIDE, bool CLAMP = (512 % NT != 0)>
RP_DEV void tile_sstore(float* s, int tid, const float4 (&r)[(512 + NT - 1) / NT]) {
#pragma unroll
  for (int j = 0; j < (512 + NT - 1) / NT; ++j) {
    int f = tid + NT * j;
    if (CLAMP) f = min(f, 511);
    st4(s + (f >> 4) * STRIDE + (f & 15) * 4, r[j]);
  }
}

// S^T tile: s[r] = sum_d Ks[kv = acc_row(r,hi)][d] * breg[q = l31][d]; breg[t] holds d = 32*hi + t (fp32 mode) / bpk[c] = the
// same 32 values as 4 x 8 bf16 (bf16 operand mode, see common.h: 8 consecutive k-steps of a lane = one v_mfma_f32_32x32x16_bf16)
template <bool BF>
RP_DEV f32x16 score_tile(const float* Ks, int l31, int hi, const float (&breg)[32], const bf16x8 (&bpk)[4]) {
  f32x16 s = zero16();
  const float* kr = Ks + l31 * KST + 32 * hi;
  if (BF) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float4 x = ld4(kr + 8 * c), y = ld4(kr + 8 * c + 4);
      s = mfma_bf(pack8(x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w), bpk[c], s);
    }
    return s;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float4 kf = ld4(kr + 4 * c);
    s = mfma32(kf.x, breg[4 * c + 0], s);
    s = mfma32(kf.y, breg[4 * c + 1], s);
    s = mfma32(kf.z, breg[4 * c + 2], s);
    s = mfma32(kf.w, breg[4 * c + 3], s);
  }
  return s;
}

// load the owner operand (32 rows x 64) into registers: lane (row l31, half hi) keeps cols 32*hi .. +31
RP_DEV void load_owner(const float* row_ptr, int hi, float mul, float (&reg)[32]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float4 x = ld4(row_ptr + 32 * hi + 4 * c);
    reg[4 * c + 0] = x.x * mul; reg[4 * c + 1] = x.y * mul; reg[4 * c + 2] = x.z * mul; reg[4 * c + 3] = x.w * mul;
  }
}
