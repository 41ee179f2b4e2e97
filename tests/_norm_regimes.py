"""Inputs, fp64 references, fp32 yardsticks, metrics and bounds for the normalisation-regime tests of the LayerNorm kernels
(csrc/rowwise.hip, linear_rows.hip, mlp_fused.hip, gemm epilogue, dx_lnbwd_bf16.hip) and the BatchNorm kernels (csrc/batchnorm.hip, the
statistics epilogues of the 3x3 convolutions).  torch (and numpy for one re-enactment) only, no GPU and no library at import:
tests/test_norm_regimes_cpu.py proves every regime's condition on the CPU, tests/test_gpu_norm_regimes.py runs the kernels.

LayerNorm input (ln_input): rows [M, 192] fp32 from a fixed seed; regime k of LN_REGIMES sits in the rows with row % 8 == k, so the 16 rows
of a wave and the 64 rows of a tile always mix all eight.  eps = 1e-6 INSIDE the root.
  control      randn.
  offset30     30 + randn:      |mean| / sigma ~ 30.
  offset1000   1000 + randn:    |mean| / sigma ~ 1000; the fp32 mean alone is good to 6e-5 of sigma.
  outlier      randn with one channel per row set to 300 (channel (37 (row // 8) + 11) % 192: every lane and register slot is hit); the
               channel holds > 99 % of the row's centred energy, sigma ~ 21.6.
  constant     every element of the row = 1.5 (1 + (row // 8) % 64): at most 8 significant bits, so every fp32 partial sum, the mean and
               x - mean = 0 are exact: the output is beta bit for bit and rstd is 1 / sqrt(eps) = 1000 to an ulp.
  nearconst    3 + 1e-3 randn:  variance ~ eps -- the regime that SEES the value and the placement of eps (1e-5 for 1e-6, or eps outside the
               root, moves the output by about half of its size; on `control` by 5.9e-6).
  tiny         2^-20 randn:     variance 9e-13 << eps, rstd ~ 1000.
  huge         2^30 randn:      variance 1.2e18, rstd ~ 9e-10.
gamma = 1 + 0.2 randn, beta = randn; cotangents and the residual-branch operand `add` are randn.  M = 328 (five 64-row tiles and a ragged
tile of 8 rows) and M = 2312 = 4 * 576 + 8 for the kernels that choose their form by size.

BatchNorm input (bn_input): [N, C, H, W] fp32 (the tests make it channels-last); regime k of BN_REGIMES sits in the channels with
c % 8 == k, so the 4 (fp32) or 8 (bf16) channels of one 16-byte access always mix regimes.  eps = 1e-5.
  control      1.7 randn + 0.6.
  offset30     30 + randn.
  offset1000   1000 + 0.01 randn.
  constant     1/3 + c/7 = (7 + 3 c) / 21 (never dyadic) in every element of channel c.
  nearconst    3 + sqrt(1e-5) randn: variance ~ eps.
  tiny         2^-20 randn.
  spike        randn with ONE element of the channel (not in row 0) set to 1e4.
  pivot        randn with only element [0, c, 0, 0] -- row 0 of the tensor, the pivot of bn_reduce_kernel -- set to D = 8 (c % 16 == 7) or
               D = 100 (c % 16 == 15).
bf16 storage: the input (and residual, cotangent) rounded to bf16 first; the reference, the yardstick and the conditions use the rounded
tensor (offset1000 collapses to the constant 1000 there, nearconst to 3 with rare steps of 2^-6).  Evaluation mode: running_var cycles
through {0, 1e-7, 1e-5, 1, 1e6} with c % 5 and running_mean through {0, 1000, -1000} with c % 3 (coprime to the 8 regimes).
Shapes (4, 64, 28, 28), (3, 192, 12, 12) -- 256 / (C / 4) is no whole number of row lanes -- and (2, 128, 9, 7).

References take the dtype to run in.  fp64 is the reference; fp32 is the YARDSTICK: the plain two-pass formula in torch ops -- mean, mean of
(x - mean)^2, 1 / sqrt(var + eps), the textbook backward -- NOT F.layer_norm / nn.BatchNorm2d, whose CPU accumulation differs between
versions.  Fused kernels are referenced as the whole operation (LN(x) W^T + b, the MLP, LN'(dy W)).  bf16-operand kernels (operand
precision 1): the yardstick rounds the normalised rows, hidden activations and weights to bf16 where the kernel does; the reference does not.

Metrics (each returns the worst value and where).  row_rel: max |a - b| / max |b| inside each row, for every [M, .] output.  chan_rel: the
same inside each channel, for every BatchNorm tensor.  elem_rel: |a - b| / max(|b|, scale) element by element, for mean / rstd / running_* /
dgamma / dbeta / column sums, with `scale` the absolute scale the quantity's own rounding lives on: the row's (channel's) standard deviation
for a mean, sqrt(sum t^2) of the summed terms for a column sum (what the sum would be without cancellation of signs), nothing for rstd, and
eps for a variance (it only ever acts through var + eps).

Bound rule (tests/_softmax_regimes.py's): an error is at most 8 x the yardstick's error on the same input under the same metric, per regime
(the rows / channels of one regime are judged against that regime's yardstick), with a floor of 4 ulps of the metric's unit, 4 * 2^-23, for
where the yardstick happens to be exact.  Stored-bf16 tensors get one bf16 rounding on top, 2^-8 of the row / channel maximum, as the
existing bf16 tests state.  No constant is fitted to a kernel.

Derived allowance (pivot_allowance), per channel, in fp64 from the reference, on top of the rule: the BatchNorm statistics sum d = x - p and
d^2 in fp32 over at most 64 rows per thread and in double above, with p = row 0 of the tensor (bn_reduce_kernel) or p = 0 (the convolution
epilogues).  A rounding of the running fp32 sum is eps32 of its size, so the variance carries up to eps32 E[d^2] = eps32 ((mu - p)^2 + s^2)
absolute and the mean up to eps32 sqrt(E[d^2]) -- where the two-pass yardstick has eps32 s^2.  Images, first order: rstd: half the variance's
over (s^2 + eps); y: |gamma| rstd (|x - mu| a_rstd + a_mean); dx: a_rstd (|dx| + 2 |gamma| rstd |xhat c2|); dgamma: a_rstd x its scale;
running_var / running_mean: momentum x the statistic's.  bn_reduce_kernel: channels of the pivot / spike / offset regimes only (zero for the
others), about row 0 for bn_reduce_kernel and about zero for the statistics from a convolution epilogue.  The fp32 epilogues
(conv3x3_f32.hip, conv3x3_c128_f32.hip) sum y and y^2 in double from the first addition -- an fp32 product is exact in double -- so there
the allowance is never needed (summed in fp32 over a tile's seven pixels, as they were, a constant channel at 6.5 had rstd 30 % off);
conv3x3_bf16.hip sums the stored bf16 values in fp32 per lane: 8-bit values whose squares and short sums are exact.

Max-pool windows (pool_keep).  Behind bn -> relu -> maxpool the gradient goes to the window's largest element; where fp64 cannot tell which
one that is -- the two largest distinct values of the window within 2 x the forward bound of each other -- or the pooled value is within the
bound of zero, the pooled cotangent is zeroed, for the reference and the kernel alike.  Cap on the undecided windows of a channel: MASK_CAP,
except in the offset1000 channels: there the YARDSTICK's forward error is 1e-3 of the channel (its fp32 mean is good to 6e-5 where sigma is
0.01), so the bound is 8e-3 x 7 sigma_y, the two largest of nine samples are closer than twice that in a quarter of the windows, and the
cap is POOL_CAP_OFFSET1000 = 0.3 (the gap of the two largest of nine normal samples has density ~ 2.3 / sigma at zero: P(gap < 0.11 sigma)
~ 0.25).

ReLU masks.  A y within the forward bound of zero may take the other side of the ReLU than fp64: in the backward tests the cotangent is zeroed
where the fp64 pre-ReLU value is within that channel's forward bound (rule + allowance) of zero, for the reference and the kernel alike; at
most 5 % of a channel's elements (MASK_CAP).  offset1000 / nearconst channels take beta = 3 |gamma|, constant channels beta = +-0.5."""
import functools
import math

import numpy as np
import torch

DIM = 192
LN_EPS, BN_EPS = 1e-6, 1e-5
EPS32 = 2.0 ** -23
FACTOR = 8.0
FLOOR = 4 * EPS32
BF16_STORE = 2.0 ** -8
MASK_CAP = 0.05
POOL_CAP_OFFSET1000 = 0.3
MOMENTUM = 0.1

LN_REGIMES = ("control", "offset30", "offset1000", "outlier", "constant", "nearconst", "tiny", "huge")
BN_REGIMES = ("control", "offset30", "offset1000", "constant", "nearconst", "tiny", "spike", "pivot")
LN_MS = (328, 2312)
BN_SHAPES = ((4, 64, 28, 28), (3, 192, 12, 12), (2, 128, 9, 7))
PIVOT_D = (8.0, 100.0)
SPIKE = 1e4
OUTLIER = 300.0


def bound(yard, floor=FLOOR, extra=0.0):
    return max(FACTOR * yard, floor) + extra


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# ------------------------------------------------------------------------------------------------ LayerNorm: inputs
def ln_groups(M):
    return {n: ln_rows(M, n) for n in LN_REGIMES}


def ln_rows(M, regime):
    """row indices of a regime"""
    return torch.arange(LN_REGIMES.index(regime), M, 8)


def outlier_channel(rows):
    return (37 * (rows // 8) + 11) % DIM


def constant_value(rows):
    return 1.5 * (1 + (rows // 8) % 64).float()


def ln_input(M, seed=301):
    x = torch.randn(M, DIM, generator=_gen(seed))
    r = lambda name: ln_rows(M, name)
    x[r("offset30")] += 30.0
    x[r("offset1000")] += 1000.0
    o = r("outlier")
    x[o, outlier_channel(o)] = OUTLIER
    c = r("constant")
    x[c] = constant_value(c)[:, None].expand(-1, DIM)
    x[r("nearconst")] = 3.0 + 1e-3 * x[r("nearconst")]
    x[r("tiny")] *= 2.0 ** -20
    x[r("huge")] *= 2.0 ** 30
    return x.contiguous()


def ln_params(seed=302):
    g = _gen(seed)
    return 1 + 0.2 * torch.randn(DIM, generator=g), torch.randn(DIM, generator=g)


def randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=_gen(seed)) * scale


def ln_weights(seed=303):
    """qkv (W [576,192], b), fc1 (w1 [768,192], b1), fc2 (w2 [192,768], b2)"""
    g = _gen(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(wq=rn(576, DIM) * DIM ** -0.5, bq=0.1 * rn(576), w1=rn(768, DIM) * DIM ** -0.5, b1=0.1 * rn(768),
                w2=rn(DIM, 768) * 768 ** -0.5, b2=0.1 * rn(DIM))


# ------------------------------------------------------------------------------------------------ LayerNorm: references
def bf16_round(t):
    return t.float().to(torch.bfloat16).to(t.dtype)


def ln_fwd(x, gamma, beta, dtype, eps=LN_EPS, eps_outside=False):
    """two-pass LayerNorm in `dtype` -> (xn [M,C], mean [M], rstd [M]); eps_outside: 1 / (sqrt(var) + eps), the defect the regimes must see"""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / (torch.sqrt(var) + eps) if eps_outside else 1.0 / torch.sqrt(var + eps)
    return d * rstd * gamma + beta, mu[:, 0], rstd[:, 0]


def ln_bwd(dxn, x, gamma, mean, rstd, dtype, add=None):
    """textbook LayerNorm backward in `dtype` from the given statistics -> dict(dx, dgamma, dbeta[, colsum]) and the summed terms' scales"""
    dxn, x, gamma, mean, rstd = (t.to(dtype) for t in (dxn, x, gamma, mean, rstd))
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dxn * gamma
    dx = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    out = dict(dx=dx, dgamma=(dxn * xh).sum(0), dbeta=dxn.sum(0))
    scale = dict(dgamma=(dxn * xh).square().sum(0).sqrt(), dbeta=dxn.square().sum(0).sqrt())
    if add is not None:
        add = add.to(dtype)
        out["dx"] = dx + add
        out["colsum"] = add.sum(0)
        scale["colsum"] = add.square().sum(0).sqrt()
    return out, scale


def gelu(t, form="erf"):
    return torch.nn.functional.gelu(t, approximate="tanh" if form == "tanh" else "none")


def gelu_grad(a, form="erf"):
    a = a.detach().clone().requires_grad_(True)
    gelu(a, form).sum().backward()
    return a.grad


def _op(t, dtype, bf):
    t = t.to(dtype)
    return bf16_round(t) if bf else t


def ln_linear(x, gamma, beta, W, b, dtype, act=0, bf=False, form="erf"):
    """act(LN(x) W^T + b) in `dtype` -> dict(y, pre, xn, mean, rstd); bf: the matrix operands (xn, W) rounded to bf16"""
    xn, mean, rstd = ln_fwd(x, gamma, beta, dtype)
    pre = _op(xn, dtype, bf) @ _op(W, dtype, bf).t() + b.to(dtype)
    return dict(y=gelu(pre, form) if act else pre, pre=pre, xn=xn, mean=mean, rstd=rstd)


def mlp(x, gamma, beta, w, dtype, bf=False, form="erf"):
    """x + fc2(GELU(fc1(LN(x)))) in `dtype` -> dict(y, xn, mean, rstd, h, hpre)"""
    r = ln_linear(x, gamma, beta, w["w1"], w["b1"], dtype, act=1, bf=bf, form=form)
    y = x.to(dtype) + _op(r["y"], dtype, bf) @ _op(w["w2"], dtype, bf).t() + w["b2"].to(dtype)
    return dict(y=y, xn=r["xn"], mean=r["mean"], rstd=r["rstd"], h=r["y"], hpre=r["pre"])


def mlp_bwd_ln(dy, hpre, x, gamma, mean, rstd, w, dtype, bf=False, form="erf"):
    """the MLP backward-data chain with the LayerNorm backward behind it, in `dtype`, from the given hpre and statistics:
    dhp = (dy W2) o GELU'(hpre), dxn = dhp W1, dx = LN'(dxn) + dy -> (dict(dhp, dxn, dx, dgamma, dbeta, colsum), scales)"""
    dhp = (_op(dy, dtype, bf) @ _op(w["w2"], dtype, bf)) * gelu_grad(hpre.to(dtype), form)
    dxn = _op(dhp, dtype, bf) @ _op(w["w1"], dtype, bf)
    out, scale = ln_bwd(dxn, x, gamma, mean, rstd, dtype, add=dy)
    out.update(dhp=dhp, dxn=dxn)
    return out, scale


def dx_lnbwd(dy, W, x, gamma, mean, rstd, dtype, add=None, bf=False, bf_dy=False):
    """LN'(dy W) in `dtype` from the given statistics -> (dict(dx, dgamma, dbeta[, colsum]), scales); bf / bf_dy: W / dy rounded to bf16"""
    return ln_bwd(_op(dy, dtype, bf_dy) @ _op(W, dtype, bf), x, gamma, mean, rstd, dtype, add=add)


# ------------------------------------------------------------------------------------------------ metrics
def _worst(err, ref):
    ratio = err / ref.clamp_min(1e-300)
    ratio = torch.where((err == 0) & (ref == 0), torch.zeros_like(ratio), ratio)
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), tuple(int(n) for n in np.unravel_index(i, tuple(ratio.shape)))


def _d(t):
    return t.detach().double().cpu()


def row_cells(a, b):
    """[M, .] -> (max |a - b|, max |b|) per row"""
    a, b = _d(a), _d(b)
    return (a - b).abs().amax(-1), b.abs().amax(-1)


def chan_cells(a, b):
    """[N, C, H, W] -> (max |a - b|, max |b|) per channel"""
    a, b = _d(a), _d(b)
    return (a - b).abs().amax((0, 2, 3)), b.abs().amax((0, 2, 3))


def elem_cells(a, b, scale=None):
    a, b = _d(a), _d(b)
    ref = b.abs() if scale is None else torch.maximum(b.abs(), _d(scale))
    return (a - b).abs(), ref


def row_rel(a, b, rows=None):
    e, r = row_cells(a, b)
    if rows is not None:
        w, at = _worst(e[rows], r[rows])
        return w, (int(rows[at[0]]),)
    return _worst(e, r)


def chan_rel(a, b, chans=None):
    e, r = chan_cells(a, b)
    if chans is not None:
        w, at = _worst(e[chans], r[chans])
        return w, (int(chans[at[0]]),)
    return _worst(e, r)


def elem_rel(a, b, scale=None, idx=None):
    e, r = elem_cells(a, b, scale)
    if idx is not None:
        w, at = _worst(e[idx], r[idx])
        return w, (int(idx[at[0]]),)
    return _worst(e, r)


def rel(a, b):
    """the tensor-wide metric of tests/test_gpu_kernels.py"""
    a, b = _d(a), _d(b)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def ulps32(a, b):
    """largest distance in fp32 ulps between two fp32 tensors of one sign"""
    ai, bi = a.detach().cpu().float().view(torch.int32).long(), b.detach().cpu().float().view(torch.int32).long()
    return int((ai - bi).abs().max())


def _ratio(d, lim):
    r = d / lim.clamp_min(1e-300)
    return torch.where((d == 0) & (lim == 0), torch.zeros_like(r), r)


def judge(kind, got, yard, want, groups, extra=0.0, allow=None, scale=None, floor=FLOOR, against=None):
    """The bound rule, per group of rows ("row"), channels ("chan") or elements ("elem"; scale: see elem_rel): the group's limit is
    bound(worst yardstick error of the group) (+ extra, relative) times each cell's reference maximum, + allow (absolute, per element of
    `want`).  against: |got - against| is held to the limit instead (two kernels computing the same thing).
    -> list of dict(group, err, yard, ratio = err / yard, of_limit = worst element's |got - want| / limit, allow_used, where)"""
    cells = {"row": row_cells, "chan": chan_cells, "elem": lambda a, b: elem_cells(a, b, scale)}[kind]
    e_y, r = cells(yard, want)
    other = want if against is None else against
    e_g = cells(got, other)[0]
    diff = (_d(got) - _d(other)).abs()
    al = None if allow is None else _d(allow)
    out = []
    for name, idx in groups.items():
        if len(idx) == 0:
            continue
        live = r[idx] > 0                               # a cell whose reference is all zero must be reproduced exactly, whatever fp32 makes of it
        y = _worst(e_y[idx][live], r[idx][live])[0] if bool(live.any()) else 0.0
        lim = bound(y, floor, extra) * r[idx]
        if kind == "row":
            lim, d, a = lim[:, None], diff[idx], None if al is None else al[idx]
        elif kind == "chan":
            lim, d, a = lim[None, :, None, None], diff[:, idx], None if al is None else al[:, idx]
        else:
            d, a = diff[idx], None if al is None else al[idx]
        used = 0.0 if a is None else float(_ratio((d - lim).clamp_min(0.0), a).max())      # share of the allowance the worst element needs
        lim = lim.expand_as(d) if a is None else lim + a
        err, at = _worst(e_g[idx], r[idx])
        out.append(dict(group=name, err=err, yard=y, ratio=err / max(y, 1e-30), of_limit=float(_ratio(d, lim).max()), allow_used=used,
                        where=int(idx[at[0]])))
    return out


# ------------------------------------------------------------------------------------------------ BatchNorm: inputs
def bn_chans(C, regime, D=None):
    """channel indices of a regime; pivot: D = 8 -> c % 16 == 7, D = 100 -> c % 16 == 15, None -> both"""
    ch = torch.arange(BN_REGIMES.index(regime), C, 8)
    if regime == "pivot" and D is not None:
        ch = ch[(ch % 16) == (7 if D == PIVOT_D[0] else 15)]
    return ch


def spike_position(c, N, H, W):
    """(n, h, w) of channel c's spike: never row 0 of the tensor"""
    R = N * H * W
    r = 1 + (131 * c + 17) % (R - 1)
    return r // (H * W), (r // W) % H, r % W


def bn_input(shape, bf16=False, seed=401):
    N, C, H, W = shape
    x = torch.randn(N, C, H, W, generator=_gen(seed + C))
    ch = lambda name, D=None: bn_chans(C, name, D)
    x[:, ch("control")] = 1.7 * x[:, ch("control")] + 0.6
    x[:, ch("offset30")] += 30.0
    x[:, ch("offset1000")] = 1000.0 + 0.01 * x[:, ch("offset1000")]
    for c in ch("constant").tolist():
        x[:, c] = (7.0 + 3.0 * c) / 21.0
    x[:, ch("nearconst")] = 3.0 + math.sqrt(1e-5) * x[:, ch("nearconst")]
    x[:, ch("tiny")] *= 2.0 ** -20
    for c in ch("spike").tolist():
        n, h, w = spike_position(c, N, H, W)
        x[n, c, h, w] = SPIKE
    for D in PIVOT_D:
        x[0, ch("pivot", D), 0, 0] = D
    return bf16_round(x) if bf16 else x


def bn_params(C, seed=402):
    """gamma (a negative one per 16 channels), beta (the ReLU-mask rule's overrides), running statistics for the evaluation mode"""
    g = _gen(seed + C)
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[5::16] *= -1.0
    beta = 0.3 * torch.randn(C, generator=g)
    for name in ("offset1000", "nearconst"):
        beta[bn_chans(C, name)] = 3.0 * gamma[bn_chans(C, name)].abs()
    cc = bn_chans(C, "constant")
    beta[cc] = torch.where((cc // 8) % 2 == 0, 0.5, -0.5)
    c = torch.arange(C)
    rv = torch.tensor([0.0, 1e-7, 1e-5, 1.0, 1e6])[c % 5]
    rm = torch.tensor([0.0, 1000.0, -1000.0])[c % 3]
    return gamma, beta, rm, rv


def bn_operands(shape, bf16=False, seed=403):
    """(residual, cotangent)"""
    g = _gen(seed + shape[1])
    res, cot = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    return (bf16_round(res), bf16_round(cot)) if bf16 else (res, cot)


# ------------------------------------------------------------------------------------------------ BatchNorm: references
def _c(v):
    return v[None, :, None, None]


def bn_fwd(x, gamma, beta, dtype, training=True, rm=None, rv=None, res=None, relu=True, eps=BN_EPS, eps_outside=False):
    """two-pass BatchNorm (+ residual, ReLU) in `dtype` -> dict(y, pre, mean, rstd, var, running_mean, running_var); evaluation mode
    normalises with (rm, rv) and leaves them unchanged"""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    R = x.numel() // x.shape[1]
    out = {}
    if training:
        mean = x.mean((0, 2, 3))
        d = x - _c(mean)
        var = (d * d).mean((0, 2, 3))
        if rm is not None:
            out["running_mean"] = (1 - MOMENTUM) * rm.to(dtype) + MOMENTUM * mean
            out["running_var"] = (1 - MOMENTUM) * rv.to(dtype) + MOMENTUM * var * (R / (R - 1))
    else:
        mean, var = rm.to(dtype), rv.to(dtype)
        d = x - _c(mean)
        out["running_mean"], out["running_var"] = mean, var
    rstd = 1.0 / (torch.sqrt(var) + eps) if eps_outside else 1.0 / torch.sqrt(var + eps)
    pre = d * _c(rstd) * _c(gamma) + _c(beta)
    if res is not None:
        pre = pre + res.to(dtype)
    out.update(y=pre.relu() if relu else pre, pre=pre, mean=mean, rstd=rstd, var=var)
    return out


def bn_bwd(cot, x, gamma, mean, rstd, pre, dtype, training=True, relu=True, has_res=False):
    """textbook BatchNorm backward in `dtype` from the given statistics and pre-ReLU values -> (dict(dx, dgamma, dbeta[, dres]), scales, c2)"""
    cot, x, gamma, mean, rstd = (t.to(dtype) for t in (cot, x, gamma, mean, rstd))
    g = cot * (pre > 0).to(dtype) if relu else cot
    xh = (x - _c(mean)) * _c(rstd)
    dgamma, dbeta = (g * xh).sum((0, 2, 3)), g.sum((0, 2, 3))
    R = x.numel() // x.shape[1]
    c2 = dgamma / R
    if training:
        dx = _c(gamma * rstd) * (g - _c(dbeta / R) - xh * _c(c2))
    else:
        dx = _c(gamma * rstd) * g
    out = dict(dx=dx, dgamma=dgamma, dbeta=dbeta)
    if has_res:
        out["dres"] = g
    scale = dict(dgamma=(g * xh).square().sum((0, 2, 3)).sqrt(), dbeta=g.square().sum((0, 2, 3)).sqrt())
    return out, scale, c2


def pivot_allowance(x, pivot, chans=None, eps=BN_EPS):
    """fp64 allowances per channel of statistics summed about `pivot` [C] (module docstring): dict(var, mean absolute; rstd relative).
    chans: the channels that get it (zero elsewhere)"""
    x = x.double()
    mu = x.mean((0, 2, 3))
    s2 = (x - _c(mu)).square().mean((0, 2, 3))
    e2 = (mu - pivot.double()).square() + s2
    a = dict(var=EPS32 * e2, mean=EPS32 * e2.sqrt(), rstd=0.5 * EPS32 * e2 / (s2 + eps))
    if chans is not None:
        keep = torch.zeros_like(mu)
        keep[chans] = 1.0
        a = {k: v * keep for k, v in a.items()}
    return a


def pivot_channels(C):
    """channels of the regimes that get bn_reduce_kernel's row-0 pivot allowance"""
    return torch.cat([bn_chans(C, n) for n in ("offset30", "offset1000", "spike", "pivot")]).sort().values


def dgamma_allowance(a, ref, scale):
    """dgamma = sum g xhat: rstd scales xhat, the mean shifts it by rstd a_mean"""
    return a["rstd"] * scale["dgamma"] + ref["rstd"] * a["mean"] * scale["dbeta"]


def allowance_images(a, x, gamma, ref, bwd=None, c2=None, scale=None):
    """first-order images (absolute, fp64) of the statistics' allowances `a` on y / dx [N,C,H,W] and dgamma / running statistics [C]; ref:
    bn_fwd's fp64 result, bwd / c2 / scale: bn_bwd's"""
    x, gamma = x.double(), gamma.double()
    rstd, mean = ref["rstd"], ref["mean"]
    R = x.numel() // x.shape[1]
    out = dict(y=_c(gamma.abs() * rstd) * ((x - _c(mean)).abs() * _c(a["rstd"]) + _c(a["mean"])), rstd=a["rstd"] * rstd, mean=a["mean"],
               running_mean=MOMENTUM * a["mean"], running_var=MOMENTUM * a["var"] * (R / (R - 1)))
    if bwd is not None:
        xh = (x - _c(mean)) * _c(rstd)
        # dx = gamma rstd (g - c1 - xhat c2): rstd scales the whole and xhat and c2 once each; the mean moves xhat by rstd a_mean
        out["dx"] = _c(a["rstd"]) * (bwd["dx"].abs() + 2 * _c(gamma.abs() * rstd * c2.abs()) * xh.abs()) + _c(
            gamma.abs() * rstd * rstd * c2.abs() * a["mean"])
        out["dgamma"] = dgamma_allowance(a, ref, scale)
    return out


def relu_mask(pre64, bound_abs):
    """1 where the cotangent is kept: the fp64 pre-ReLU value is further from zero than the forward bound (absolute: [C] or a full tensor)"""
    b = _c(bound_abs) if bound_abs.dim() == 1 else bound_abs
    return (pre64.abs() > b).to(pre64.dtype)


# ------------------------------------------------------------------------------------------------ the documented accumulation order
def bn_reduce_layout(R, C, group=4):
    """(row lanes per workgroup, rows per workgroup) of bn_reduce_kernel (group = 4 channels per thread) / bn_reduce_g_kernel (8)"""
    return 256 // (C // group), max(-(-R // 1024), 128)


def pivot_reenact(x_rc, pivot, nrl=1, rpb=None, flush=64, wide=False):
    """numpy fp32 re-enactment of the statistics' accumulation for ONE channel: x_rc [R] fp32 in row order, d = x - pivot and d^2 summed in
    fp32 over at most `flush` rows, in double above.  (nrl, rpb) = bn_reduce_layout(): a workgroup takes rpb consecutive rows and its row
    lane l the rows l, l + nrl, ... of them, four at a time with a flush after 64 and one after the tail, as bn_reduce_kernel does; the
    default is one lane over all rows in order.  wide: d and d^2 in double from the first addition (the fp32 convolution epilogues).
    -> (mean, var) as doubles"""
    x = np.asarray(x_rc, dtype=np.float32)
    p = np.float32(pivot)
    R = len(x)
    if wide:
        d = (x - p).astype(np.float64)
        md = float(d.sum()) / R
        return md + float(p), max(float((d * d).sum()) / R - md * md, 0.0)
    rpb = rpb or R
    a = b = 0.0
    for r0 in range(0, R, rpb):
        for lane in range(nrl):
            d = (x[r0 + lane:min(R, r0 + rpb):nrl] - p).astype(np.float32)
            sa, sb, cnt = np.float32(0), np.float32(0), 0
            full = len(d) - len(d) % 4                    # the unrolled loop counts rows in fours; the tail rows join the last run
            for i, v in enumerate(d):
                sa = np.float32(sa + v)
                sb = np.float32(sb + np.float32(v * v))
                cnt += 1
                if cnt >= flush and i < full and (i + 1) % 4 == 0:
                    a += float(sa)
                    b += float(sb)
                    sa, sb, cnt = np.float32(0), np.float32(0), 0
            a += float(sa)
            b += float(sb)
    md = a / R
    return md + float(p), max(b / R - md * md, 0.0)


# ------------------------------------------------------------------------------------------------ BatchNorm: one case, shared by the CPU and GPU tests
def bn_groups(C):
    g = {n: bn_chans(C, n) for n in BN_REGIMES if n != "pivot"}
    g["pivot8"], g["pivot100"] = bn_chans(C, "pivot", PIVOT_D[0]), bn_chans(C, "pivot", PIVOT_D[1])
    return g


def chan_bound(yard32, want, C, extra=0.0):
    """[C]: the rule's relative bound of every channel, from its regime's yardstick under chan_rel"""
    e, r = chan_cells(yard32, want)
    out = torch.zeros(C, dtype=torch.float64)
    for idx in bn_groups(C).values():
        live = idx[r[idx] > 0]
        if len(live):
            out[idx] = bound(_worst(e[live], r[live])[0], extra=extra)
    return out


@functools.lru_cache(maxsize=None)
def bn_case(shape, bf16=False, training=True, with_res=False, relu=True, pivot="row0"):
    """Everything one BatchNorm case needs, computed once: inputs, fp64 reference (f64, b64), fp32 yardstick (f32, b32), the allowances'
    images (allow), the masked cotangent (cot) and the fraction of every channel it zeroes (masked).  pivot: "row0" (bn_reduce_kernel:
    allowance on the pivot / spike / offset channels), "zero" (statistics from a convolution epilogue: the same channels, about zero)"""
    N, C, H, W = shape
    x = bn_input(shape, bf16)
    gamma, beta, rm, rv = bn_params(C)
    res, cot = bn_operands(shape, bf16)
    res = res if with_res else None
    f64 = bn_fwd(x, gamma, beta, torch.float64, training, rm, rv, res, relu)
    f32 = bn_fwd(x, gamma, beta, torch.float32, training, rm, rv, res, relu)
    if training:
        a = pivot_allowance(x, x[0, :, 0, 0] if pivot == "row0" else torch.zeros(C), pivot_channels(C))
    else:
        a = {k: torch.zeros(C, dtype=torch.float64) for k in ("var", "mean", "rstd")}
    allow = allowance_images(a, x, gamma, f64)
    if relu:
        pre_max = f64["pre"].abs().amax((0, 2, 3))
        mask = relu_mask(f64["pre"], _c(chan_bound(f32["pre"], f64["pre"], C) * pre_max) + allow["y"])
    else:
        mask = torch.ones_like(f64["pre"])
    cotm = cot * mask.to(cot.dtype)
    b64, sc, c2 = bn_bwd(cotm, x, gamma, f64["mean"], f64["rstd"], f64["pre"], torch.float64, training, relu, with_res)
    b32, _, _ = bn_bwd(cotm, x, gamma, f32["mean"], f32["rstd"], f32["pre"], torch.float32, training, relu, with_res)
    allow.update({k: v for k, v in allowance_images(a, x, gamma, f64, b64, c2, sc).items() if k in ("dx", "dgamma")})
    # (a variance only ever acts through var + eps: an absolute error far below eps is immaterial, so eps is its absolute scale)
    scale = dict(sc, mean=f64["var"].sqrt(), running_mean=MOMENTUM * f64["var"].sqrt(), running_var=torch.full((C,), MOMENTUM * BN_EPS))
    return dict(x=x, gamma=gamma, beta=beta, rm=rm, rv=rv, res=res, cot=cotm, f64=f64, f32=f32, b64=b64, b32=b32, allow=allow, scale=scale, a=a,
                masked=1.0 - mask.mean((0, 2, 3)), groups=bn_groups(C))


def pool_keep(relu_y, bound_abs):
    """[N,C,OH,OW] 1 / 0 and the undecided share per channel [C] for maxpool(3, 2, 1) of relu_y [N,C,H,W] >= 0 (fp64): a window is kept where
    its largest value is further than bound_abs [C] from zero and the runner-up is either equal (a tie: first in scan order wins everywhere)
    or more than 2 bound_abs below; undecided = largest above the bound, runner-up too close"""
    N, C, H, W = relu_y.shape
    win = torch.nn.functional.unfold(relu_y, 3, padding=1, stride=2).view(N, C, 9, -1)       # (zero padding = -inf padding after a ReLU)
    top = win.topk(2, dim=2).values
    b = bound_abs[None, :, None]
    told = (top[:, :, 0] - top[:, :, 1] > 2 * b) | (top[:, :, 0] == top[:, :, 1])
    alive = top[:, :, 0] > b
    keep = (told & alive).view(N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1).to(relu_y.dtype)
    return keep, (~told & alive).double().mean((0, 2))


def pool_bound(c):
    """[C] absolute forward bound (rule + allowance) of bn_case c's pre-ReLU values"""
    C = c["x"].shape[1]
    return chan_bound(c["f32"]["pre"], c["f64"]["pre"], C) * c["f64"]["pre"].abs().amax((0, 2, 3)) + c["allow"]["y"].amax((0, 2, 3))
