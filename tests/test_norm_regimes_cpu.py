"""The inputs of tests/test_gpu_norm_regimes.py, proved on the CPU (tests/_norm_regimes.py builds them): every regime holds its stated
condition at every shape (bf16: after rounding), the fp32 yardstick alone stays inside a recorded envelope and is exact where it is
stated to be, the ReLU-mask cap holds, the `nearconst` regime sees a wrong or misplaced eps at more than 100 x its bound, and the derived
pivot allowance covers a numpy fp32 re-enactment of the documented accumulation order.  No GPU, no library."""
import math

import pytest
import torch

from tests import _norm_regimes as R

F64, F32 = torch.float64, torch.float32

# recorded envelopes of the yardstick's row_rel / chan_rel on the forward output (about 3 x what it measures; the bound rule uses the
# measured value, these only catch a yardstick that has drifted, e.g. with another torch version)
LN_ENVELOPE = dict(control=6e-7, offset30=6e-6, offset1000=2e-4, outlier=6e-7, constant=0.0, nearconst=4e-4, tiny=1.2e-7, huge=6e-7)
BN_ENVELOPE = dict(control=8e-7, offset30=5e-6, offset1000=7e-3, constant=2e-3, nearconst=4e-5, tiny=2.5e-7, spike=6e-7, pivot8=6e-7,
                   pivot100=1.5e-6)


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_stats(x):
    x = x.double()
    mu = x.mean(1)
    var = (x - mu[:, None]).square().mean(1)
    return mu, var


@pytest.mark.parametrize("M", R.LN_MS)
def test_layernorm_regimes_hold_their_conditions(M):
    x = R.ln_input(M)
    assert x.shape == (M, R.DIM) and x.dtype == F32 and bool(torch.isfinite(x).all())
    assert torch.equal(x, R.ln_input(M))                                              # fixed seed
    mu, var = _ln_stats(x)
    ratio = mu.abs() / var.sqrt().clamp_min(1e-300)
    rows = lambda n: R.ln_rows(M, n)
    for k, n in enumerate(R.LN_REGIMES):
        assert bool((rows(n) % 8 == k).all()) and abs(len(rows(n)) - M / 8) < 1       # every 8 consecutive rows hold all eight regimes
    assert float(ratio[rows("control")].max()) < 0.5 and 0.6 < float(var[rows("control")].min()) < float(var[rows("control")].max()) < 1.5
    assert 20 < float(ratio[rows("offset30")].min()) and float(ratio[rows("offset30")].max()) < 45
    assert 700 < float(ratio[rows("offset1000")].min()) and float(ratio[rows("offset1000")].max()) < 1400
    o = rows("outlier")
    ch = R.outlier_channel(o)
    assert bool((x[o, ch] == R.OUTLIER).all())
    share = (x[o, ch].double() - mu[o]).square() / (var[o] * R.DIM)
    assert float(share.min()) > 0.99
    if M >= 8 * 64:                                                                   # every register slot (c % 4), lane group and 64-column block
        assert len(set((ch % 64).tolist())) == 64 and len(set((ch // 64).tolist())) == 3
    assert len(set((ch % 4).tolist())) == 4 and len(set((ch % 16).tolist())) == 16
    c = rows("constant")
    assert bool((x[c] == x[c][:, :1]).all()) and bool((x[c][:, 0] == R.constant_value(c)).all())
    v2 = (2 * x[c][:, 0]).long()                                                       # 3 (1 + k) <= 192: at most 8 significant bits
    assert bool((v2.float() == 2 * x[c][:, 0]).all()) and int(v2.max()) < 256
    nc = var[rows("nearconst")] / R.LN_EPS
    assert 0.6 < float(nc.min()) and float(nc.max()) < 1.6
    assert float((var[rows("tiny")] / R.LN_EPS).max()) < 2e-6
    assert float((var[rows("huge")] / R.LN_EPS).min()) > 1e23


@pytest.mark.parametrize("M", R.LN_MS)
def test_layernorm_yardstick_envelope_and_exact_rows(M):
    x = R.ln_input(M)
    g, b = R.ln_params()
    y64, m64, r64 = R.ln_fwd(x, g, b, F64)
    y32, m32, r32 = R.ln_fwd(x, g, b, F32)
    for n in R.LN_REGIMES:
        yard = R.row_rel(y32, y64, R.ln_rows(M, n))[0]
        assert yard <= LN_ENVELOPE[n], (n, yard)
    c = R.ln_rows(M, "constant")
    assert torch.equal(y32[c], b.expand(len(c), -1))                                   # beta bit for bit
    assert torch.equal(m32[c], x[c][:, 0])
    assert R.ulps32(r32[c], torch.full((len(c),), R.LN_EPS ** -0.5)) <= 1
    # the textbook backward of the constant rows: xhat = 0, dx = rstd (g - mean g): 1000-fold amplification, finite
    dy = R.randn(M, R.DIM, seed=311)
    out64, _ = R.ln_bwd(dy, x, g, m64, r64, F64)
    out32, _ = R.ln_bwd(dy, x, g, m32, r32, F32)
    assert R.row_rel(out32["dx"], out64["dx"], c)[0] < 1e-6 and float(out64["dx"][c].abs().max()) > 1e3


@pytest.mark.parametrize("M", R.LN_MS)
def test_nearconst_rows_see_a_wrong_or_misplaced_layernorm_eps(M):
    """eps = 1e-5 for 1e-6 (BatchNorm's for LayerNorm's), or eps outside the root: more than 100 x the regime's bound on `nearconst`,
    next to the existing tolerances (2e-6 / 5e-6) on `control`"""
    x = R.ln_input(M)
    g, b = R.ln_params()
    y64 = R.ln_fwd(x, g, b, F64)[0]
    y32 = R.ln_fwd(x, g, b, F32)[0]
    rows = R.ln_rows(M, "nearconst")
    limit = R.bound(R.row_rel(y32, y64, rows)[0])
    for kw in (dict(eps=1e-5), dict(eps_outside=True)):
        bad = R.ln_fwd(x, g, b, F64, **kw)[0]
        assert R.row_rel(bad, y64, rows)[0] > 100 * limit, (kw, limit)
        assert R.row_rel(bad, y64, R.ln_rows(M, "control"))[0] < 8e-6
        assert R.judge("row", bad, y32, y64, {"nearconst": rows})[0]["of_limit"] > 100
    assert R.row_rel(R.ln_fwd(x, g, b, F64, eps=1e-5)[0], y64, R.ln_rows(M, "tiny"))[0] > 100 * R.bound(
        R.row_rel(y32, y64, R.ln_rows(M, "tiny"))[0])


def test_fused_layernorm_references_are_the_whole_operation():
    """ln_linear / mlp / dx_lnbwd / mlp_bwd_ln against autograd of the same composition in fp64"""
    M = 64
    x = R.ln_input(M).double().requires_grad_(True)
    g, b = (t.double().requires_grad_(True) for t in R.ln_params())
    w = R.ln_weights()
    dy = R.randn(M, 576, seed=312)
    r = R.ln_linear(x, g, b, w["wq"], w["bq"], F64)
    (r["y"] * dy.double()).sum().backward()
    out, _ = R.dx_lnbwd(dy, w["wq"], x.detach(), g.detach(), r["mean"].detach(), r["rstd"].detach(), F64)
    assert R.rel(out["dx"], x.grad) < 1e-9 and R.rel(out["dgamma"], g.grad) < 1e-12 and R.rel(out["dbeta"], b.grad) < 1e-12
    x.grad = g.grad = b.grad = None
    m = R.mlp(x, g, b, w, F64)
    d2 = R.randn(M, R.DIM, seed=313)
    (m["y"] * d2.double()).sum().backward()
    out, _ = R.mlp_bwd_ln(d2, m["hpre"].detach(), x.detach(), g.detach(), m["mean"].detach(), m["rstd"].detach(), w, F64)
    assert R.rel(out["dx"], x.grad) < 1e-9 and R.rel(out["dgamma"], g.grad) < 1e-12 and R.rel(out["colsum"], d2.double().sum(0)) < 1e-14


# ------------------------------------------------------------------------------------------------ BatchNorm
def _bn_stats(x):
    x = x.double()
    mu = x.mean((0, 2, 3))
    return mu, (x - mu[None, :, None, None]).square().mean((0, 2, 3))


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", R.BN_SHAPES)
def test_batchnorm_regimes_hold_their_conditions(shape, bf16):
    N, C, H, W = shape
    x = R.bn_input(shape, bf16)
    assert x.shape == shape and bool(torch.isfinite(x).all()) and torch.equal(x, R.bn_input(shape, bf16))
    if bf16:
        assert torch.equal(x, R.bf16_round(x))
    mu, var = _bn_stats(x)
    sd = var.sqrt()
    ch = lambda n, D=None: R.bn_chans(C, n, D)
    for k, n in enumerate(R.BN_REGIMES):
        assert bool((ch(n) % 8 == k).all()) and len(ch(n)) == C // 8                  # the 4 / 8 channels of one access mix regimes
    assert float((mu[ch("control")] - 0.6).abs().max()) < 0.5 and float((sd[ch("control")] - 1.7).abs().max()) < 0.35
    assert float((mu[ch("offset30")] - 30).abs().max()) < 0.3 and float((sd[ch("offset30")] - 1).abs().max()) < 0.2
    o = ch("offset1000")
    if bf16:                                                                          # 1000 +- 0.01 is the one bf16 value 1000
        assert bool((x[:, o] == 1000.0).all())
    else:
        assert float((mu[o] - 1000).abs().max()) < 0.01 and float((sd[o] - 0.01).abs().max()) < 0.002
        assert float((mu[o].abs() / sd[o]).min()) > 8e4
    for c in ch("constant").tolist():
        v = x[0, c, 0, 0]
        assert bool((x[:, c] == v).all()) and abs(float(v) - (7 + 3 * c) / 21) < (0.1 if bf16 else 2e-6)
        assert bf16 or float(v) * 2 ** 10 != round(float(v) * 2 ** 10)                         # not dyadic: the fp32 sum of R copies rounds
    nc = var[ch("nearconst")] / R.BN_EPS
    assert (-1 if bf16 else 0.7) < float(nc.min()) and float(nc.max()) < (6 if bf16 else 1.4)
    assert float((var[ch("tiny")] / R.BN_EPS).max()) < 2e-7 and float(var[ch("tiny")].min()) > 0
    for c in ch("spike").tolist():
        n, h, w = R.spike_position(c, N, H, W)
        assert (n, h, w) != (0, 0, 0) and float(x[n, c, h, w]) == (R.SPIKE if not bf16 else float(R.bf16_round(torch.tensor(R.SPIKE))))
        rest = x[:, c].clone()
        rest[n, h, w] = 0
        assert float(rest.abs().max()) < 6
    for D in R.PIVOT_D:
        p = ch("pivot", D)
        assert len(p) == C // 16 and bool((x[0, p, 0, 0] == D).all())
        rest = x[:, p].clone()
        rest[0, :, 0, 0] = 0
        assert float(rest.abs().max()) < 6
    gamma, beta, rm, rv = R.bn_params(C)
    assert bool((gamma[5::16] < 0).all()) and float(gamma.abs().min()) >= 0.5
    for n in ("offset1000", "nearconst"):
        assert torch.equal(beta[ch(n)], 3 * gamma[ch(n)].abs())
    assert bool((beta[ch("constant")].abs() == 0.5).all()) and len(set(beta[ch("constant")].tolist())) == 2
    # evaluation mode: every regime meets every running variance and every running mean (C >= 120: every combination)
    combos = {(c % 8, float(rv[c]), float(rm[c])) for c in range(C)}
    assert len({(k, v) for k, v, _ in combos}) == 40 and len({(k, m) for k, _, m in combos}) == 24
    assert set(rv.tolist()) == {0.0, float(torch.tensor(1e-7)), float(torch.tensor(1e-5)), 1.0, 1e6} and set(rm.tolist()) == {0.0, 1000.0, -1000.0}


CASES = [(tr, res, relu) for tr in (True, False) for res, relu in ((False, True), (True, True), (False, False), (True, False))]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", R.BN_SHAPES)
def test_batchnorm_yardstick_envelope_exact_channels_and_mask_cap(shape, bf16):
    N, C, H, W = shape
    for training, with_res, relu in CASES:
        c = R.bn_case(shape, bf16, training, with_res, relu)
        assert float(c["masked"].max()) <= R.MASK_CAP, (training, with_res, relu, float(c["masked"].max()))
        if relu and training and N * H * W > 1000:
            assert float(c["masked"].max()) > 0                                        # the mask does something
        assert bool((c["cot"] == 0).float().mean() < R.MASK_CAP)
    c = R.bn_case(shape, bf16, True, False, False)
    for j in R.judge("chan", c["f32"]["y"], c["f32"]["y"], c["f64"]["y"], c["groups"]):
        assert j["yard"] <= BN_ENVELOPE[j["group"]], j
    # the pivoted path on a constant channel: d = x - pivot = 0 exactly, so mean = the constant, var = 0, y = fma(0, ., beta) = beta
    x = c["x"]
    for ch in R.bn_chans(C, "constant").tolist():
        col = x[:, ch].permute(0, 1, 2).reshape(-1).numpy()
        mean, var = R.pivot_reenact(col, col[0])
        assert mean == float(col[0]) and var == 0.0
        assert float(c["f64"]["rstd"][ch]) == pytest.approx(R.BN_EPS ** -0.5, rel=1e-12)
        assert bool((c["f64"]["y"][:, ch] == c["beta"][ch].double()).all())


@pytest.mark.parametrize("shape", R.BN_SHAPES)
def test_nearconst_channels_see_a_wrong_or_misplaced_batchnorm_eps(shape):
    C = shape[1]
    c = R.bn_case(shape, False, True, False, False)
    groups = {"nearconst": R.bn_chans(C, "nearconst")}
    for kw in (dict(eps=1e-6), dict(eps_outside=True)):
        bad = R.bn_fwd(c["x"], c["gamma"], c["beta"], F64, True, c["rm"], c["rv"], None, False, **kw)["y"]
        j = R.judge("chan", bad, c["f32"]["y"], c["f64"]["y"], groups)[0]
        assert j["of_limit"] > 100, (kw, j)


def _channel_rows(x, c):
    """channel c in the row order of the channels-last tensor"""
    return x[:, c].reshape(-1).numpy()


CONV_SHAPES = ((1, 64, 56, 56), (1, 128, 28, 28))


def _covered(x, c, m, v, a):
    """re-enacted (mean, var) of channel c inside rule + allowance a; the variance on its scale max(var, eps), as everywhere"""
    mu, var = _bn_stats(x[:, c:c + 1])
    mu, var = float(mu), float(var)
    rstd = (var + R.BN_EPS) ** -0.5
    return (abs(v - var) <= R.FLOOR * max(var, R.BN_EPS) + float(a["var"][c])
            and abs(m - mu) <= R.FLOOR * max(abs(mu), math.sqrt(var)) + float(a["mean"][c])
            and abs((v + R.BN_EPS) ** -0.5 - rstd) <= (R.FLOOR + float(a["rstd"][c])) * rstd)


@pytest.mark.parametrize("shape", R.BN_SHAPES + CONV_SHAPES)
def test_pivot_allowance_covers_the_documented_accumulation(shape):
    """bn_reduce_kernel -- d = x - row 0 and d^2 in fp32 over at most 64 rows per thread in the kernel's own row order, double above --
    re-enacted in numpy: the variance, the mean and rstd stay inside rule + allowance in EVERY channel that gets the allowance and inside
    the plain rule in every other one.  The fp32 convolution epilogues -- y and y^2 about zero, in double from the first addition --
    likewise, with the allowance of the same channels about a zero pivot and the plain floor in every other channel"""
    N, C, H, W = shape
    x = R.bn_input(shape)
    nrl, rpb = R.bn_reduce_layout(N * H * W, C)
    a = R.pivot_allowance(x, x[0, :, 0, 0], R.pivot_channels(C))
    a0 = R.pivot_allowance(x, torch.zeros(C), R.pivot_channels(C))
    none = {k: torch.zeros(C) for k in a}
    allowed = set(R.pivot_channels(C).tolist())
    for c in range(C):
        col = _channel_rows(x, c)
        assert _covered(x, c, *R.pivot_reenact(col, float(col[0]), nrl, rpb), a), ("row 0", c)
        assert _covered(x, c, *R.pivot_reenact(col, 0.0, wide=True), a0), ("zero, double", c)
        if c not in allowed:
            assert _covered(x, c, *R.pivot_reenact(col, 0.0, wide=True), none), ("zero, double, plain rule", c)


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_fp32_runs_about_a_zero_pivot_are_not_covered(shape):
    """what the fp32 epilogues did before -- y and y^2 about zero in fp32 over a tile's seven pixels, double above -- misses rule +
    allowance on constant and nearly constant channels (all seven roundings of a run fall the same way): why they sum in double now"""
    N, C, H, W = shape
    x = R.bn_input(shape)
    a0 = R.pivot_allowance(x, torch.zeros(C), R.pivot_channels(C))
    missed = [c for c in range(C) if not _covered(x, c, *R.pivot_reenact(_channel_rows(x, c), 0.0, flush=7), a0)]
    assert set(missed) & set(R.bn_chans(C, "constant").tolist()) and set(missed) & set(R.bn_chans(C, "nearconst").tolist()), missed


def test_bf16_convolution_statistics_accumulation_is_covered():
    """conv3x3_bf16.hip sums the STORED bf16 values and their squares in fp32: a lane adds its 2 or 4 pixels of a tile (one tile per
    workgroup up to 18 images), 32 lanes are combined in a five-level tree, double above -- at most 9 roundings per fp32 sum.  Re-enacted
    with MORE of them, as sequential fp32 runs of 64 rows: inside rule + zero-pivot allowance of the rounded tensor in every channel"""
    shape = CONV_SHAPES[0]
    x = R.bn_input(shape, True)
    C = shape[1]
    a0 = R.pivot_allowance(x, torch.zeros(C), R.pivot_channels(C))
    bad = [c for c in range(C) if not _covered(x, c, *R.pivot_reenact(_channel_rows(x, c), 0.0, flush=64), a0)]
    assert not bad, bad


def test_maxpool_window_mask_cap():
    """the share of a channel's 3x3 / 2 windows in which fp64 cannot tell the winner (pool_keep) is at most MASK_CAP, in the offset1000
    channels -- whose yardstick is 1e-3 of the channel -- at most POOL_CAP_OFFSET1000"""
    shape = R.BN_SHAPES[0]
    C = shape[1]
    c = R.bn_case(shape, False, True, False, True)
    keep, undecided = R.pool_keep(c["f64"]["pre"].relu(), R.pool_bound(c))
    loose = R.bn_chans(C, "offset1000")
    rest = torch.tensor([k for k in range(C) if k not in loose.tolist()])
    assert float(undecided[rest].max()) <= R.MASK_CAP, undecided
    assert float(undecided[loose].max()) <= R.POOL_CAP_OFFSET1000, undecided[loose]
    assert 0.3 < float(keep.mean()) < 1.0


@pytest.mark.parametrize("D", R.PIVOT_D)
def test_pivot_far_from_the_data_at_9216_rows(D):
    """one lane over R = 9216 rows of randn with x[0] = D, flushed every 64: the re-enacted pivot accumulation errs in the variance by
    some 1e-7 (D = 8) / 1e-4 (D = 100) of it where the two-pass yardstick makes some 1e-7 -- beyond the plain rule for D = 100 -- and the
    allowance is eps32 (D^2 + var) = 7.8e-6 / 1.2e-3 absolute"""
    x = torch.randn(9216, generator=torch.Generator().manual_seed(7))
    x[0] = D
    t = x.reshape(9216, 1, 1, 1).permute(1, 0, 2, 3).reshape(1, 1, 96, 96)
    xd = x.double()
    var = float((xd - xd.mean()).square().mean())
    _, v = R.pivot_reenact(x.numpy(), D)
    err = abs(v - var) / var
    v32 = float((x - x.mean()).square().mean())
    a = R.pivot_allowance(t, torch.tensor([D]))
    allow = float(a["var"][0]) / var
    assert 0.99 * R.EPS32 * D * D <= float(a["var"][0]) <= R.EPS32 * (D * D + 4) and err <= R.bound(abs(v32 - var) / var) + allow, (err, allow)
    if D == 100.0:
        assert err > R.bound(abs(v32 - var) / var)                                      # why the allowance exists
    # ... and with the pivot forced to zero on data at 1000 +- 0.01 (what the row-0 pivot prevents) the variance is lost altogether
    far = (1000.0 + 0.01 * torch.randn(9216, generator=torch.Generator().manual_seed(8)))
    fd = far.double()
    fv = float((fd - fd.mean()).square().mean())
    assert abs(R.pivot_reenact(far.numpy(), 0.0)[1] - fv) / fv > 0.5 and abs(R.pivot_reenact(far.numpy(), float(far[0]))[1] - fv) / fv < 1e-5
