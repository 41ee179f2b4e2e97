// rowwise.hip -- HBM-bound row/column kernels around the MFMA contractions:
// LayerNorm fwd/bwd (reference vision_transformer.py:396 eps=1e-6; uses at :352-353,292,295; model.py:178),
// deterministic column sums (bias / affine / pos_embed gradients), the token layout + pos_embed add
// (model.py:136-141,170-171), closed-form positional features (vision_transformer.py:90-158),
// pose normalisation (model.py:145-159) and the small gather/scatter kernels of the EMM.
// All of these move each byte once with wave-coalesced 256-byte rows; none uses MFMA.
#include "common.h"
#include "../../include/relpose_hip.h"

namespace {

constexpr int LN_MAXJ = 8;  // C <= 512

// one wave per row; lane holds elements lane + 64*j
template <int J>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd, int rows,
                                                     float eps) {
  constexpr int C = 64 * J;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (long long)row * C;
  float v[J];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    v[j] = xr[lane + 64 * j];
    s += v[j];
  }
  float mu = wave_sum(s) * (1.0f / C);
  // keep the ROUNDED mean: contracted into v - mu the product stays unrounded, so the variance and the output are taken about another
  // mean than the stored one and a constant row (v - mu = 0 exactly) does not return beta
  asm volatile("" : "+v"(mu));
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const float d = v[j] - mu;
    q += d * d;
  }
  const float rs = 1.0f / sqrtf(wave_sum(q) * (1.0f / C) + eps);
  float* yr = y + (long long)row * C;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = lane + 64 * j;
    yr[c] = (v[j] - mu) * rs * gamma[c] + beta[c];
  }
  if (lane == 0) {
    if (mean) mean[row] = mu;
    if (rstd) rstd[row] = rs;
  }
}

constexpr int LNB_ROWS = 64;  // rows per block in the backward (4 waves x 16 rows)

template <int J>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                     const float* __restrict__ gamma, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ add,
                                                     float* __restrict__ dx, float* __restrict__ dgp,
                                                     float* __restrict__ dbp, int rows) {
  constexpr int C = 64 * J;
  __shared__ float red[3][4][C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float g[J], dg[J], db[J], da[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    g[j] = gamma[lane + 64 * j];
    dg[j] = 0.f;
    db[j] = 0.f;
    da[j] = 0.f;
  }
  for (int chunk = blockIdx.x; chunk * LNB_ROWS < rows; chunk += gridDim.x) {
  const int r0 = chunk * LNB_ROWS + wave * (LNB_ROWS / 4);
  for (int rr = 0; rr < LNB_ROWS / 4; ++rr) {
    const int row = r0 + rr;
    if (row >= rows) break;
    const float mu = mean[row], rs = rstd[row];
    float xh[J], dxh[J];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const long long o = (long long)row * C + lane + 64 * j;
      const float d = dy[o];
      xh[j] = (x[o] - mu) * rs;
      dxh[j] = d * g[j];
      s1 += dxh[j];
      s2 += dxh[j] * xh[j];
      dg[j] += d * xh[j];
      db[j] += d;
    }
    const float c1 = wave_sum(s1) * (1.0f / C), c2 = wave_sum(s2) * (1.0f / C);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const long long o = (long long)row * C + lane + 64 * j;
      float v = rs * (dxh[j] - c1 - xh[j] * c2);
      if (add) {
        const float a = add[o];
        da[j] += a;          // column sum of the residual-branch gradient = bias gradient of the Linear that produced it
        v += a;
      }
      dx[o] = v;
    }
  }
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    red[0][wave][lane + 64 * j] = dg[j];
    red[1][wave][lane + 64 * j] = db[j];
    red[2][wave][lane + 64 * j] = da[j];
  }
  __syncthreads();
  const int np = add ? 3 : 2;
  for (int c = threadIdx.x; c < C; c += 256) {
    // partials interleaved as [block][np][C] so ONE column-sum launch finishes dgamma, dbeta (and the column sums of `add`)
    float* p = dgp + (long long)blockIdx.x * np * C;
    p[c] = red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c];
    p[C + c] = red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c];
    if (add) p[2 * C + c] = red[2][0][c] + red[2][1][c] + red[2][2][c] + red[2][3][c];
  }
}

// column sums: block (bx, by) = 64 columns x 4 row lanes; rows [by*rpb, (by+1)*rpb); 4 independent loads in flight
// per thread, 256-byte coalesced row segments; fixed summation order (deterministic).
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ in, int rows, int cols, int ld,
                                                     int rpb, float* __restrict__ out) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const int r0 = blockIdx.y * rpb, r1 = min(rows, r0 + rpb);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (c < cols) {
    const float* base = in + c;
    int r = r0 + rl;
    for (; r + 12 < r1; r += 16) {
      s0 += base[(long long)r * ld];
      s1 += base[(long long)(r + 4) * ld];
      s2 += base[(long long)(r + 8) * ld];
      s3 += base[(long long)(r + 12) * ld];
    }
    for (; r < r1; r += 4) s0 += base[(long long)r * ld];
  }
  red[rl][cl] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (rl == 0 && c < cols) out[(long long)blockIdx.y * cols + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

// x[z][n][c] = feat[z][c][n] + pe[n][c]   (32x32 LDS tile transpose)
__global__ __launch_bounds__(256) void tokens_fwd_kernel(const float* __restrict__ feat, const float* __restrict__ pe,
                                                         float* __restrict__ x, int C, int N) {
  __shared__ float t[32][33];
  const int z = blockIdx.z, c0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + ty + 8 * k;
    t[ty + 8 * k][tx] = feat[((long long)z * C + c) * N + n0 + tx];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int n = n0 + ty + 8 * k, c = c0 + tx;
    x[((long long)z * N + n) * C + c] = t[tx][ty + 8 * k] + pe[(long long)n * C + c];
  }
}

// channels-last CNN map: memory is already [z][n][c]; only the pos_embed add remains (float4)
__global__ __launch_bounds__(256) void tokens_nhwc_kernel(const float* __restrict__ feat, const float* __restrict__ pe,
                                                          float* __restrict__ x, long long per_img4, long long total4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const float4 a = ld4(feat + 4 * i), b = ld4(pe + 4 * (i % per_img4));
  st4(x + 4 * i, make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w));
}

__global__ __launch_bounds__(256) void tokens_bwd_kernel(const float* __restrict__ dx, float* __restrict__ dfeat, int C,
                                                         int N) {
  __shared__ float t[32][33];
  const int z = blockIdx.z, c0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int n = n0 + ty + 8 * k;
    t[ty + 8 * k][tx] = dx[((long long)z * N + n) * C + c0 + tx];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + ty + 8 * k;
    dfeat[((long long)z * C + c) * N + n0 + tx] = t[tx][ty + 8 * k];
  }
}

__global__ __launch_bounds__(256) void posenc_kernel(const float* __restrict__ intr, const float* __restrict__ lin,
                                                     float* __restrict__ pos, int B, int l1) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * 576) return;
  const int b = idx / 576, n = idx % 576;
  float ix = 1.f, iy = 1.f;
  bool bad = false;
  if (intr) {
    const float fx = intr[b * 8 + 0], fy = intr[b * 8 + 1], cx = intr[b * 8 + 2], cy = intr[b * 8 + 3];
    ix = 1.0f / ((fx / (cx * 2.0f)) * 2.0f);
    iy = 1.0f / ((fy / (cy * 2.0f)) * 2.0f);
    // The reference stops here on inputs it does not support: an assert that the two images of a pair share their intrinsics
    // (vision_transformer.py:117) and a pdb trap when the first pair's principal point lies on an image axis (:124-126).
    // A host-side check would cost a device sync per step, so the condition is evaluated here and a violating pair's
    // encodings become NaN: its pose and the batch loss turn NaN instead of silently using image 0's intrinsics.
    bad = intr[b * 8 + 4] != fx || intr[b * 8 + 5] != fy || intr[b * 8 + 6] != cx || intr[b * 8 + 7] != cy ||
          intr[2] * intr[3] == 0.0f;
  }
  float p3 = lin[n % 24], p4 = lin[n / 24];
  if (intr) {
    p3 = p3 * iy;
    p4 = p4 * ix;
  }
  if (bad) p3 = p4 = __builtin_nanf("");
  float* o = pos + (long long)idx * 6;
  o[0] = l1 ? 1.0f : p3 * p3;     // l1: get_l1_positional_encodings (vision_transformer.py:37-87) = (1,1,1,p3,p4,1)
  o[1] = l1 ? 1.0f : p4 * p4;
  o[2] = l1 ? 1.0f : p3 * p4;
  o[3] = p3;
  o[4] = p4;
  o[5] = 1.0f;
}

// x[z][h][n][0:64] = qkv[z][n][384 + h*64 + e]; [64:70] = pos[z/2][n]; [70:96] = 0
__global__ __launch_bounds__(256) void emm_build_x_kernel(const float* __restrict__ qkv, const float* __restrict__ pos,
                                                          float* __restrict__ x, int H, int ld) {
  const int z = blockIdx.z, h = blockIdx.y;
  const int n = blockIdx.x * 8 + (threadIdx.x >> 5);  // 8 rows per block, 32 threads x 3 cols each
  const int t = threadIdx.x & 31;
  float* xr = x + (((long long)z * H + h) * 576 + n) * 96;
  const float* vr = qkv + ((long long)z * 576 + n) * ld + 384 + h * 64;
  xr[t] = vr[t];
  xr[32 + t] = vr[32 + t];
  float v = 0.f;
  if (t < 6) v = pos[((long long)(z >> 1) * 576 + n) * 6 + t];
  xr[64 + t] = v;
}

__global__ __launch_bounds__(256) void emm_build_x_bwd_kernel(const float* __restrict__ dx, float* __restrict__ dqkv,
                                                              int H, int ld) {
  const int z = blockIdx.z, h = blockIdx.y;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int t = threadIdx.x & 63;
  dqkv[((long long)z * 576 + n) * ld + 384 + h * 64 + t] = dx[(((long long)z * H + h) * 576 + n) * 96 + t];
}

// g[z^1][c][h*70 + a] = sum_wg fp[z][h][wg][a][c]; zero pad to ldg.  One workgroup per (z, h): the nwg partial 96 x 96 tiles are read
// with 16-byte row-contiguous loads and summed in wg order, the 70 x 70 corner goes through LDS (padded rows) and leaves transposed --
// rows of g are written 70 consecutive floats at a time.  Head 0's workgroup also writes the zero pad [H*70, ldg).
__global__ __launch_bounds__(256) void emm_finalize_kernel(const float* __restrict__ fp, float* __restrict__ g, int H,
                                                           int ldg, int nwg) {
  __shared__ float t[70][97];
  const int z = blockIdx.y, h = blockIdx.x;
  const float* f = fp + (((long long)z * H + h) * nwg) * 9216;
  for (int e = threadIdx.x; e < 70 * 24; e += 256) {           // 70 rows x 24 float4
    const int a = e / 24, c4 = (e % 24) * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int w = 0; w < nwg; ++w) {
      const float4 v = *reinterpret_cast<const float4*>(f + (long long)w * 9216 + a * 96 + c4);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    t[a][c4] = s.x; t[a][c4 + 1] = s.y; t[a][c4 + 2] = s.z; t[a][c4 + 3] = s.w;
  }
  __syncthreads();
  float* gz = g + (long long)(z ^ 1) * 70 * ldg;
  for (int e = threadIdx.x; e < 70 * 70; e += 256) {
    const int c = e / 70, a = e % 70;
    gz[(long long)c * ldg + h * 70 + a] = t[a][c];
  }
  if (h == 0) {
    const int padw = ldg - H * 70;
    for (int e = threadIdx.x; e < 70 * padw; e += 256) gz[(long long)(e / padw) * ldg + H * 70 + e % padw] = 0.f;
  }
}

// df[z][h][a][c] (96x96, zero outside 70x70) = dg[z^1][c][h*70+a]
__global__ __launch_bounds__(256) void emm_finalize_bwd_kernel(const float* __restrict__ dg, float* __restrict__ df,
                                                               int H, int ldg) {
  const int z = blockIdx.z, h = blockIdx.y, a = blockIdx.x;  // a in [0,96)
  float* o = df + (((long long)z * H + h) * 96 + a) * 96;
  for (int c = threadIdx.x; c < 96; c += 256) {
    float v = 0.f;
    if (a < 70 && c < 70) v = dg[((long long)(z ^ 1) * 70 + c) * ldg + h * 70 + a];
    o[c] = v;
  }
}

// out[r] = sum_c a[r][c] b[r][c], C = 96: two rows per wave -- a 32-lane half holds one row as 24 float4 (16-byte loads), DPP row sums
// + one cross-row exchange, no LDS
__global__ __launch_bounds__(256) void rowdot96_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       float* __restrict__ out, long long rows) {
  const int lane = threadIdx.x & 63, l31 = lane & 31;
  const long long row = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + (lane >> 5);
  float s = 0.f;
  if (row < rows && l31 < 24) {
    const float4 x = *reinterpret_cast<const float4*>(a + row * 96 + 4 * l31), y = *reinterpret_cast<const float4*>(b + row * 96 + 4 * l31);
    s = (x.x * y.x + x.y * y.y) + (x.z * y.z + x.w * y.w);
  }
  s = row16_sum(s);
  s += __shfl_xor(s, 16, 64);
  if (row < rows && l31 == 0) out[row] = s;
}

// delta[z][h][i] = sum_e dO[z][i][h*64+e] * O[z][i][h*64+e].  One wave per token row when the heads fill at most one wave of float4
// (H <= 4: 16 lanes x 16 bytes per head, DPP row sums, no LDS; the ViT's H = 3 uses 48 lanes) -- 16-byte loads and a third of the waves
// of the one-wave-per-(row, head) form below, which stays for wider layouts.
__global__ __launch_bounds__(256) void attn_delta_rows_kernel(const float* __restrict__ dout, const float* __restrict__ o,
                                                              float* __restrict__ delta, int H, int ld, long long rows) {
  const long long zi = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // token row index z*576 + i
  if (zi >= rows) return;
  const int lane = threadIdx.x & 63, h = lane >> 4;
  float s = 0.f;
  if (h < H) {
    const long long off = zi * ld + 4 * lane;                            // lane l holds columns 4l .. 4l+3 = head l / 16
    const float4 a = *reinterpret_cast<const float4*>(dout + off), b = *reinterpret_cast<const float4*>(o + off);
    s = (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
  }
  s = row16_sum(s);
  if (h < H && (lane & 15) == 0) {
    const long long z = zi / 576;
    const int i = (int)(zi % 576);
    delta[(z * H + h) * 576 + i] = s;
  }
}

__global__ __launch_bounds__(256) void attn_delta_kernel(const float* __restrict__ dout, const float* __restrict__ o,
                                                         float* __restrict__ delta, int H, int ld, long long total) {
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // index over (z*576+i)*H + h
  if (w >= total) return;
  const int lane = threadIdx.x & 63;
  const long long zi = w / H;
  const int h = (int)(w % H);
  const long long off = zi * ld + h * 64 + lane;
  const float s = wave_sum(dout[off] * o[off]);
  if (lane == 0) {
    const long long z = zi / 576;
    const int i = (int)(zi % 576);
    delta[(z * H + h) * 576 + i] = s;
  }
}

// images [Z,3,H,W] BGR 0..255  ->  out [Z,224,224,3] (channels-last memory of a [Z,3,224,224] tensor), RGB, normalised.
// Same fp32 operation order as the reference (src/model.py:115-118,124-125): v/255, -mean, /std; nearest source index
// floor(dst * (in/out)) in fp32 (PyTorch "nearest").  Resize and normalisation commute exactly (both are per-pixel), so
// gathering first touches 224^2 of the H*W pixels.
// pad > 0: the 224 x 224 result sits inside a `pad`-pixel zero frame (the stem convolution's padding, csrc/conv_stem.hip)
__global__ __launch_bounds__(256) void preprocess_kernel(const float* __restrict__ img, float* __restrict__ out, int H, int W,
                                                         float sy, float sx, long long total, int pad) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;   // over Z * (224 + 2 pad)^2 output pixels
  if (idx >= total) return;
  const int side = 224 + 2 * pad;
  const int xp = (int)(idx % side), yp = (int)((idx / side) % side);
  const long long z = idx / ((long long)side * side);
  const int x = xp - pad, y = yp - pad;
  if (x < 0 || x >= 224 || y < 0 || y >= 224) {
    float* o = out + idx * 3;
    o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
    return;
  }
  const int iy = min((int)floorf((float)y * sy), H - 1), ix = min((int)floorf((float)x * sx), W - 1);
  const float* p = img + (z * 3) * (long long)H * W + (long long)iy * W + ix;
  const float b = p[0], g = p[(long long)H * W], r = p[2 * (long long)H * W];
  float* o = out + idx * 3;
  o[0] = (r / 255.0f - 0.485f) / 0.229f;
  o[1] = (g / 255.0f - 0.456f) / 0.224f;
  o[2] = (b / 255.0f - 0.406f) / 0.225f;
}

__global__ void pose_norm_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ gs,
                                     float* __restrict__ out, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float* p = pred + b * 14 + 7;
  float* o = out + b * 14;
  for (int i = 0; i < 7; ++i) o[i] = gs[b * 14 + i];
  for (int i = 0; i < 3; ++i) o[7 + i] = p[i];
  const float n = sqrtf(p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6]);
  const float d = fmaxf(n, 0.01f);
  for (int i = 3; i < 7; ++i) o[7 + i] = p[i] / d;
}

__global__ void pose_norm_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ dout,
                                     float* __restrict__ dpred, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float* p = pred + b * 14 + 7;
  const float* g = dout + b * 14 + 7;
  float* d = dpred + b * 14;
  for (int i = 0; i < 7; ++i) d[i] = 0.f;
  for (int i = 0; i < 3; ++i) d[7 + i] = g[i];
  const float n = sqrtf(p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6]);
  if (n > 0.01f) {
    float dot = 0.f;
    for (int i = 3; i < 7; ++i) dot += p[i] * g[i];
    for (int i = 3; i < 7; ++i) d[7 + i] = g[i] / n - p[i] * dot / (n * n * n);
  } else {
    for (int i = 3; i < 7; ++i) d[7 + i] = g[i] / 0.01f;
  }
}

}  // namespace

#define LN_DISPATCH(J, KERNEL, GRID, ...)                                                   \
  case J:                                                                                   \
    hipLaunchKernelGGL((KERNEL<J>), GRID, dim3(256), 0, st, __VA_ARGS__);                   \
    break;

extern "C" int rp_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean,
                                float* rstd, int rows, int C, float eps, void* stream) {
  if (rows <= 0 || C <= 0 || (C & 63) || C > 64 * LN_MAXJ) return RP_EBADSHAPE;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((rows + 3) / 4);
  switch (C / 64) {
    LN_DISPATCH(1, ln_fwd_kernel, grid, x, gamma, beta, y, mean, rstd, rows, eps)
    LN_DISPATCH(2, ln_fwd_kernel, grid, x, gamma, beta, y, mean, rstd, rows, eps)
    LN_DISPATCH(3, ln_fwd_kernel, grid, x, gamma, beta, y, mean, rstd, rows, eps)
    LN_DISPATCH(4, ln_fwd_kernel, grid, x, gamma, beta, y, mean, rstd, rows, eps)
    LN_DISPATCH(6, ln_fwd_kernel, grid, x, gamma, beta, y, mean, rstd, rows, eps)
    LN_DISPATCH(8, ln_fwd_kernel, grid, x, gamma, beta, y, mean, rstd, rows, eps)
    default: return RP_EUNSUPPORTED;
  }
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// enough workgroups to saturate HBM (a 256-block grid left 4 waves per CU and ran ~2x slower), few enough that the
// interleaved [nblk][2][C] partials are finished by one two-stage column sum
extern "C" int rp_layernorm_bwd_blocks(int rows) { return min((rows + LNB_ROWS - 1) / LNB_ROWS, 2048); }

extern "C" int rp_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean,
                                const float* rstd, const float* add, float* dx, float* dgamma_part, float* dbeta_part,
                                int rows, int C, void* stream) {
  if (rows <= 0 || C <= 0 || (C & 63) || C > 64 * LN_MAXJ) return RP_EBADSHAPE;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(rp_layernorm_bwd_blocks(rows));
  switch (C / 64) {
    LN_DISPATCH(1, ln_bwd_kernel, grid, dy, x, gamma, mean, rstd, add, dx, dgamma_part, dbeta_part, rows)
    LN_DISPATCH(2, ln_bwd_kernel, grid, dy, x, gamma, mean, rstd, add, dx, dgamma_part, dbeta_part, rows)
    LN_DISPATCH(3, ln_bwd_kernel, grid, dy, x, gamma, mean, rstd, add, dx, dgamma_part, dbeta_part, rows)
    LN_DISPATCH(4, ln_bwd_kernel, grid, dy, x, gamma, mean, rstd, add, dx, dgamma_part, dbeta_part, rows)
    LN_DISPATCH(6, ln_bwd_kernel, grid, dy, x, gamma, mean, rstd, add, dx, dgamma_part, dbeta_part, rows)
    LN_DISPATCH(8, ln_bwd_kernel, grid, dy, x, gamma, mean, rstd, add, dx, dgamma_part, dbeta_part, rows)
    default: return RP_EUNSUPPORTED;
  }
  RP_CHECK_LAUNCH();
  return RP_OK;
}

static int colsum_stage1_rows(int rows) {
  int rpb = 256;
  while ((rows + rpb - 1) / rpb > 1024) rpb *= 2;
  return rpb;
}

extern "C" size_t rp_colsum_workspace_bytes(int rows, int cols) {
  const int rpb = colsum_stage1_rows(rows);
  const int nb = (rows + rpb - 1) / rpb;
  return nb > 1 ? (size_t)nb * cols * sizeof(float) : 0;
}

extern "C" int rp_colsum(const float* in, int rows, int cols, int ld, float* out, float* workspace,
                         size_t workspace_bytes, void* stream) {
  if (rows <= 0 || cols <= 0) return RP_EBADSHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int rpb = colsum_stage1_rows(rows);
  const int nb = (rows + rpb - 1) / rpb;
  const int gx = (cols + 63) / 64;
  if (nb == 1) {
    hipLaunchKernelGGL(colsum_kernel, dim3(gx, 1), dim3(256), 0, st, in, rows, cols, ld, rpb, out);
    RP_CHECK_LAUNCH();
    return RP_OK;
  }
  if (!workspace || workspace_bytes < rp_colsum_workspace_bytes(rows, cols)) return RP_EWORKSPACE;
  hipLaunchKernelGGL(colsum_kernel, dim3(gx, nb), dim3(256), 0, st, in, rows, cols, ld, rpb, workspace);
  RP_CHECK_LAUNCH();
  hipLaunchKernelGGL(colsum_kernel, dim3(gx, 1), dim3(256), 0, st, (const float*)workspace, nb, cols, cols, nb, out);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

// ---- several column sums in one pair of launches ------------------------------------------------------------------
// The backward of one reference module ends with 3-4 independent column sums (bias gradients, LayerNorm gamma / beta
// partials): each was two ~8 us launches of its own.  rp_colsum_multi runs up to RP_COLSUM_MAX of them as ONE stage-1 launch
// (every task's (column group, row block) workgroups, flattened) and ONE stage-2 launch; arithmetic and summation order per
// task are exactly rp_colsum's.
struct ColsumMultiP {
  const float* in[RP_COLSUM_MAX];
  float* dst[RP_COLSUM_MAX];          // stage 1: workspace slab (or the output when the task has a single row block)
  int rows[RP_COLSUM_MAX], cols[RP_COLSUM_MAX], ld[RP_COLSUM_MAX], rpb[RP_COLSUM_MAX], gx[RP_COLSUM_MAX];
  int blk_end[RP_COLSUM_MAX];         // exclusive prefix sums of the tasks' workgroup counts
  int n;
};

__global__ __launch_bounds__(256) void colsum_multi_kernel(ColsumMultiP p) {
  __shared__ float red[4][64];
  int t = 0;
  while (t + 1 < p.n && (int)blockIdx.x >= p.blk_end[t]) ++t;
  const int local = blockIdx.x - (t ? p.blk_end[t - 1] : 0);
  const int bx = local % p.gx[t], by = local / p.gx[t];
  const float* in = p.in[t];
  const int rows = p.rows[t], cols = p.cols[t], ld = p.ld[t], rpb = p.rpb[t];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = bx * 64 + cl;
  const int r0 = by * rpb, r1 = min(rows, r0 + rpb);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (c < cols) {
    const float* base = in + c;
    int r = r0 + rl;
    for (; r + 12 < r1; r += 16) {
      s0 += base[(long long)r * ld];
      s1 += base[(long long)(r + 4) * ld];
      s2 += base[(long long)(r + 8) * ld];
      s3 += base[(long long)(r + 12) * ld];
    }
    for (; r < r1; r += 4) s0 += base[(long long)r * ld];
  }
  red[rl][cl] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (rl == 0 && c < cols) p.dst[t][(long long)by * cols + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

extern "C" size_t rp_colsum_multi_workspace_bytes(const RpColsumTask* tasks, int n) {
  size_t tot = 0;
  for (int i = 0; i < n; ++i) tot += rp_colsum_workspace_bytes(tasks[i].rows, tasks[i].cols);
  return tot;
}

extern "C" int rp_colsum_multi(const RpColsumTask* tasks, int n, float* workspace, size_t workspace_bytes, void* stream) {
  if (!tasks || n <= 0 || n > RP_COLSUM_MAX) return RP_EBADSHAPE;
  if (workspace_bytes < rp_colsum_multi_workspace_bytes(tasks, n)) return RP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  ColsumMultiP p1{}, p2{};
  int blocks1 = 0, blocks2 = 0;
  float* ws = workspace;
  for (int i = 0; i < n; ++i) {
    const RpColsumTask& t = tasks[i];
    if (t.rows <= 0 || t.cols <= 0 || !t.in || !t.out) return RP_EBADSHAPE;
    const int rpb = colsum_stage1_rows(t.rows), nb = (t.rows + rpb - 1) / rpb, gx = (t.cols + 63) / 64;
    p1.in[i] = t.in; p1.rows[i] = t.rows; p1.cols[i] = t.cols; p1.ld[i] = t.ld; p1.rpb[i] = rpb; p1.gx[i] = gx;
    p1.dst[i] = nb == 1 ? t.out : ws;
    blocks1 += gx * nb;
    p1.blk_end[i] = blocks1;
    if (nb > 1) {                        // second stage over the nb partial rows, exactly as rp_colsum does
      const int j = p2.n++;
      p2.in[j] = ws; p2.rows[j] = nb; p2.cols[j] = t.cols; p2.ld[j] = t.cols; p2.rpb[j] = nb; p2.gx[j] = gx; p2.dst[j] = t.out;
      blocks2 += gx;
      p2.blk_end[j] = blocks2;
      ws += (size_t)nb * t.cols;
    }
  }
  p1.n = n;
  hipLaunchKernelGGL(colsum_multi_kernel, dim3(blocks1), dim3(256), 0, st, p1);
  RP_CHECK_LAUNCH();
  if (p2.n > 0) {
    hipLaunchKernelGGL(colsum_multi_kernel, dim3(blocks2), dim3(256), 0, st, p2);
    RP_CHECK_LAUNCH();
  }
  return RP_OK;
}

extern "C" int rp_tokens_fwd(const float* feat, const float* pos_embed, float* x, int Z, int C, int N, void* stream) {
  if (Z <= 0 || (C & 31) || (N & 31)) return RP_EBADSHAPE;
  hipLaunchKernelGGL(tokens_fwd_kernel, dim3(N / 32, C / 32, Z), dim3(256), 0, (hipStream_t)stream, feat, pos_embed, x,
                     C, N);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_tokens_fwd_nhwc(const float* feat, const float* pos_embed, float* x, int Z, int C, int N,
                                  void* stream) {
  if (Z <= 0 || (C & 3)) return RP_EBADSHAPE;
  const long long per4 = (long long)C * N / 4, tot4 = per4 * Z;
  hipLaunchKernelGGL(tokens_nhwc_kernel, dim3((unsigned)((tot4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, feat,
                     pos_embed, x, per4, tot4);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_tokens_bwd(const float* dx, float* dfeat, int Z, int C, int N, void* stream) {
  if (Z <= 0 || (C & 31) || (N & 31)) return RP_EBADSHAPE;
  hipLaunchKernelGGL(tokens_bwd_kernel, dim3(N / 32, C / 32, Z), dim3(256), 0, (hipStream_t)stream, dx, dfeat, C, N);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_posenc(const float* intrinsics, const float* lin24, float* pos, int B, int l1, void* stream) {
  if (B <= 0) return RP_EBADSHAPE;
  hipLaunchKernelGGL(posenc_kernel, dim3((B * 576 + 255) / 256), dim3(256), 0, (hipStream_t)stream, intrinsics, lin24,
                     pos, B, l1);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_emm_build_x(const float* qkv, const float* pos, float* x, int Z, int H, int ldqkv, void* stream) {
  if (Z <= 0 || (Z & 1) || H <= 0) return RP_EBADSHAPE;
  hipLaunchKernelGGL(emm_build_x_kernel, dim3(576 / 8, H, Z), dim3(256), 0, (hipStream_t)stream, qkv, pos, x, H, ldqkv);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_emm_build_x_bwd(const float* dx, float* dqkv, int Z, int H, int ldqkv, void* stream) {
  if (Z <= 0 || H <= 0) return RP_EBADSHAPE;
  hipLaunchKernelGGL(emm_build_x_bwd_kernel, dim3(576 / 4, H, Z), dim3(256), 0, (hipStream_t)stream, dx, dqkv, H,
                     ldqkv);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_emm_finalize(const float* f_part, float* g, int Z, int H, int ldg, void* stream) {
  if (Z <= 0 || (Z & 1) || H * 70 > ldg) return RP_EBADSHAPE;
  hipLaunchKernelGGL(emm_finalize_kernel, dim3(H, Z), dim3(256), 0, (hipStream_t)stream, f_part, g, H, ldg, 6);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_emm_finalize_parts(const float* f_part, float* g, int Z, int H, int ldg, int nparts, void* stream) {
  if (Z <= 0 || (Z & 1) || H * 70 > ldg || nparts <= 0) return RP_EBADSHAPE;
  hipLaunchKernelGGL(emm_finalize_kernel, dim3(H, Z), dim3(256), 0, (hipStream_t)stream, f_part, g, H, ldg, nparts);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_emm_finalize_bwd(const float* dg, float* df, int Z, int H, int ldg, void* stream) {
  if (Z <= 0 || (Z & 1) || H * 70 > ldg) return RP_EBADSHAPE;
  hipLaunchKernelGGL(emm_finalize_bwd_kernel, dim3(96, H, Z), dim3(256), 0, (hipStream_t)stream, dg, df, H, ldg);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_rowdot96(const float* a, const float* b, float* out, long long rows, void* stream) {
  if (rows <= 0) return RP_EBADSHAPE;
  hipLaunchKernelGGL(rowdot96_kernel, dim3((unsigned)((rows + 7) / 8)), dim3(256), 0, (hipStream_t)stream, a, b, out,
                     rows);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_attn_bwd_delta(const float* dout, const float* o, float* delta, int Z, int H, int ld, void* stream) {
  if (Z <= 0 || H <= 0) return RP_EBADSHAPE;
  const long long total = (long long)Z * 576 * H, rows = (long long)Z * 576;
  if (H <= 4 && (ld & 3) == 0)
    hipLaunchKernelGGL(attn_delta_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dout, o, delta, H, ld, rows);
  else
    hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dout, o,
                       delta, H, ld, total);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_preprocess_padded(const float* images, float* out, int Z, int H, int W, int pad, void* stream) {
  if (Z <= 0 || H <= 0 || W <= 0 || pad < 0 || pad > 16) return RP_EBADSHAPE;
  const long long total = (long long)Z * (224 + 2 * pad) * (224 + 2 * pad);
  hipLaunchKernelGGL(preprocess_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, images,
                     out, H, W, (float)H / 224.0f, (float)W / 224.0f, total, pad);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_preprocess(const float* images, float* out, int Z, int H, int W, void* stream) {
  return rp_preprocess_padded(images, out, Z, H, W, 0, stream);
}

extern "C" int rp_pose_normalize_fwd(const float* pred, const float* gs, float* out, int B, void* stream) {
  if (B <= 0) return RP_EBADSHAPE;
  hipLaunchKernelGGL(pose_norm_fwd_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, pred, gs, out, B);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_pose_normalize_bwd(const float* pred, const float* dout, float* dpred, int B, void* stream) {
  if (B <= 0) return RP_EBADSHAPE;
  hipLaunchKernelGGL(pose_norm_bwd_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, pred, dout, dpred, B);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_abi_version(void) { return RP_ABI_VERSION; }
extern "C" int rp_abi_export_count(void) { return RP_ABI_EXPORTS; }
extern "C" const char* rp_target_arch(void) { return "gfx950"; }
