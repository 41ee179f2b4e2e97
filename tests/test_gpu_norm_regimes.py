"""The LayerNorm and BatchNorm kernels where the statistics are ill-conditioned -- rows / channels far from zero, constant, of variance ~ eps,
tiny, huge, with one massive channel or element, with the statistics' pivot far from the data -- judged per row / per channel and per
regime against fp64.  Inputs, references, metrics, the bound rule and the derived allowances: tests/_norm_regimes.py; the conditions of the
inputs are proved on the CPU by tests/test_norm_regimes_cpu.py.

Every asserted error is at most 8 x the error the plain two-pass fp32 formula makes on the same input under the same metric in the same
regime (floor: 4 ulps; stored-bf16 tensors: + 2^-8; the pivot allowance on the BatchNorm channels that get one); constant rows / channels
are exact.  Every backward is handed the mean / rstd its own forward wrote.  Forms are reached by size (M = 328 / 2312) or through the
public switches (operand precision, ops.FUSE_LN_BWD, ops.FUSE_STEM_POOL).  Each measured error, the yardstick's and the share of the limit
used go to the test report (tests/test_gpu_kernels.py: report()), per output and regime.

The stem convolution's statistics epilogue (rp_conv_stem_fwd) is left out: a 7x7 / stride 2 convolution of a 3-channel image cannot
reproduce a channel regime in its 64 outputs; the 3x3 convolutions can (centre-tap identity filter) and are run here."""
import contextlib

import pytest
import torch

from tests import _norm_regimes as R
from tests.test_gpu_kernels import report

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
CL = torch.channels_last
ALL = {"all": torch.arange(R.DIM)}
_CACHE = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, ops as o
    _lib.load()
    yield o
    _CACHE.clear()
    R.bn_case.cache_clear()


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@contextlib.contextmanager
def gemm_precision(ops, p):
    prev = ops.GEMM_PRECISION
    ops.set_gemm_precision(p)
    try:
        yield
    finally:
        ops.set_gemm_precision(prev)


class Checks:
    """collects every judged output (tests/_norm_regimes.py: judge) and reports all of them before it asserts"""

    def __init__(self, name):
        self.name, self.kv, self.failed = name, {}, []

    def rule(self, what, kind, got, yard, want, groups, **kw):
        if not bool(torch.isfinite(got.float()).all()):
            self.failed.append("%s: not finite" % what)
            return
        for j in R.judge(kind, got, yard, want, groups, **kw):
            key = "%s.%s" % (what, j["group"])
            self.kv[key], self.kv[key + "_fp32"], self.kv[key + "_of_limit"] = j["err"], j["yard"], j["of_limit"]
            if kw.get("allow") is not None:
                self.kv[key + "_allowance_used"] = j["allow_used"]
            if not j["of_limit"] <= 1.0:
                self.failed.append("%s: %.3e at %d = %.1f x its limit (plain fp32: %.3e)" % (key, j["err"], j["where"], j["of_limit"], j["yard"]))

    def exact(self, what, ok):
        if not ok:
            self.failed.append("%s: not exact" % what)

    def done(self):
        report(self.name, **self.kv)
        assert not self.failed, self.name + " -- " + "; ".join(self.failed)


# ------------------------------------------------------------------------------------------------ LayerNorm family
def ln_data(M):
    def make():
        x = R.ln_input(M)
        g, b = R.ln_params()
        w = R.ln_weights()
        d = dict(x=x, g=g, b=b, w=w, dy=R.randn(M, R.DIM, seed=321), add=R.randn(M, R.DIM, seed=322), dyq=R.randn(M, 576, seed=323),
                 f64=R.ln_fwd(x, g, b, F64), f32=R.ln_fwd(x, g, b, F32), groups=R.ln_groups(M))
        d["sigma"] = x.double().var(1, unbiased=False).sqrt()
        d["cu"] = {k: v.cuda() for k, v in d.items() if isinstance(v, torch.Tensor)}
        d["cu"]["w"] = {k: v.cuda() for k, v in w.items()}
        return d
    return cached(("ln", M), make)


def check_stats(ck, d, M, xn, mean, rstd, xn_bf16=False, prefix=""):
    """xn / mean / rstd of any forward against the LayerNorm references; the constant rows exactly"""
    f64, f32, groups = d["f64"], d["f32"], d["groups"]
    ck.rule(prefix + "xn", "row", xn.float(), f32[0], f64[0], groups, extra=R.BF16_STORE if xn_bf16 else 0.0)
    ck.rule(prefix + "mean", "elem", mean, f32[1], f64[1], groups, scale=d["sigma"])
    ck.rule(prefix + "rstd", "elem", rstd, f32[2], f64[2], groups)
    c = groups["constant"]
    beta = d["b"].to(BF) if xn_bf16 else d["b"]
    ck.exact(prefix + "xn of constant rows = beta", torch.equal(xn.cpu()[c], beta.expand(len(c), -1)))
    ck.exact(prefix + "mean of constant rows", torch.equal(mean.cpu()[c], d["x"][c][:, 0]))
    ck.exact(prefix + "rstd of constant rows within 1 ulp of 1 / sqrt(eps)", R.ulps32(rstd.cpu()[c], torch.full((len(c),), R.LN_EPS ** -0.5)) <= 1)


def check_ln_bwd(ck, got, o32, o64, sc, groups, prefix=""):
    """(dx, dgamma, dbeta[, colsum]) of any LayerNorm backward"""
    ck.rule(prefix + "dx", "row", got[0], o32["dx"], o64["dx"], groups)
    for i, k in enumerate(("dgamma", "dbeta", "colsum")[:len(got) - 1]):
        ck.rule(prefix + k, "elem", got[1 + i], o32[k], o64[k], ALL, scale=sc[k])


@pytest.mark.parametrize("with_add", [True, False])
@pytest.mark.parametrize("M", R.LN_MS)
def test_layernorm_fwd_bwd_regimes(ops, M, with_add):
    """ops.layernorm_fwd / layernorm_bwd (csrc/rowwise.hip)"""
    d = ln_data(M)
    cu = d["cu"]
    ck = Checks("norm_regimes.layernorm[M=%d,add=%d]" % (M, with_add))
    y, mean, rstd = ops.layernorm_fwd(cu["x"], cu["g"], cu["b"])
    check_stats(ck, d, M, y, mean, rstd)
    add = d["add"] if with_add else None
    got = ops.layernorm_bwd(cu["dy"], cu["x"], cu["g"], mean, rstd, add=cu["add"] if with_add else None)
    o64, sc = R.ln_bwd(d["dy"], d["x"], d["g"], d["f64"][1], d["f64"][2], F64, add)
    o32, _ = R.ln_bwd(d["dy"], d["x"], d["g"], d["f32"][1], d["f32"][2], F32, add)
    check_ln_bwd(ck, got, o32, o64, sc, d["groups"])
    ck.done()


@pytest.mark.parametrize("precision,xn_bf16", [(0, False), (1, False), (1, True)])
@pytest.mark.parametrize("M", R.LN_MS)
def test_linear_rows_fused_layernorm_regimes(ops, M, precision, xn_bf16):
    """ops.linear_rows with ln= (csrc/linear_rows.hip): the qkv and the fc1 + GELU forms with want_ln_out, as LN(x) W^T + b; the inference
    call is bit-identical to the training call's y"""
    d = ln_data(M)
    cu, w = d["cu"], d["cu"]["w"]
    form = "tanh" if precision else "erf"
    ck = Checks("norm_regimes.linear_rows[M=%d,p=%d,xn_bf16=%d]" % (M, precision, xn_bf16))
    kw = dict(xn_dtype=BF) if xn_bf16 else {}
    with gemm_precision(ops, precision):
        for name, W, bias, act in (("qkv", "wq", "bq", 0), ("fc1", "w1", "b1", 1)):
            out = ops.linear_rows(cu["x"], w[W], w[bias], act=act, want_pre=bool(act), ln=(cu["g"], cu["b"]), want_ln_out=True, **kw)
            y, (xn, mean, rstd) = out[0], out[-3:]
            y_inf = ops.linear_rows(cu["x"], w[W], w[bias], act=act, ln=(cu["g"], cu["b"]))
            ck.exact(name + ": inference y = training y", torch.equal(y_inf, y))
            r64 = R.ln_linear(d["x"], d["g"], d["b"], d["w"][W], d["w"][bias], F64, act=act, form=form)
            r32 = R.ln_linear(d["x"], d["g"], d["b"], d["w"][W], d["w"][bias], F32, act=act, bf=bool(precision), form=form)
            ck.rule(name + ".y", "row", y, r32["y"], r64["y"], d["groups"])
            if act:
                ck.rule(name + ".pre", "row", out[1], r32["pre"], r64["pre"], d["groups"])
            check_stats(ck, d, M, xn, mean, rstd, xn_bf16, prefix=name + ".")
    ck.done()


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("M", R.LN_MS)
def test_fused_mlp_regimes(ops, M, precision):
    """ops.mlp_fused (csrc/mlp_fused.hip), inference and training form, as x + fc2(GELU(fc1(LN(x))))"""
    d = ln_data(M)
    cu, w = d["cu"], d["cu"]["w"]
    form = "tanh" if precision else "erf"
    ck = Checks("norm_regimes.mlp_fused[M=%d,p=%d]" % (M, precision))
    args = (cu["x"], cu["g"], cu["b"], w["w1"], w["b1"], w["w2"], w["b2"])
    with gemm_precision(ops, precision):
        y_inf = ops.mlp_fused(*args)
        y, xn, mean, rstd, h, hpre = ops.mlp_fused(*args, train=True)
    r64 = R.mlp(d["x"], d["g"], d["b"], d["w"], F64, form=form)
    r32 = R.mlp(d["x"], d["g"], d["b"], d["w"], F32, bf=bool(precision), form=form)
    ck.rule("y_inference", "row", y_inf, r32["y"], r64["y"], d["groups"])
    for k, got in (("y", y), ("h", h), ("hpre", hpre)):
        ck.rule(k, "row", got, r32[k], r64[k], d["groups"])
    check_stats(ck, d, M, xn, mean, rstd)
    ck.done()


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("M", R.LN_MS)
def test_fused_mlp_backward_with_layernorm_backward_regimes(ops, M, precision):
    """ops.mlp_fused_bwd(..., ln=): the LayerNorm backward folded into the MLP backward, handed the hpre / mean / rstd of the kernel's own
    training forward; against fp64 of the whole chain and -- exact fp32 operands -- against the unfused pair of kernels under the same rule"""
    d = ln_data(M)
    cu, w = d["cu"], d["cu"]["w"]
    form = "tanh" if precision else "erf"
    ck = Checks("norm_regimes.mlp_fused_bwd_ln[M=%d,p=%d]" % (M, precision))
    with gemm_precision(ops, precision):
        _, _, mean, rstd, _, hpre = ops.mlp_fused(cu["x"], cu["g"], cu["b"], w["w1"], w["b1"], w["w2"], w["b2"], train=True)
        dhp, got, _ = ops.mlp_fused_bwd(cu["dy"], hpre, w["w1"], w["w2"], ln=(cu["x"], cu["g"], mean, rstd))
        if not precision:
            _, dxn, _ = ops.mlp_fused_bwd(cu["dy"], hpre, w["w1"], w["w2"])
            pair = ops.layernorm_bwd(dxn, cu["x"], cu["g"], mean, rstd, add=cu["dy"])
    refs = []
    for dt in (F64, F32):
        bf = bool(precision) and dt == F32
        f = R.mlp(d["x"], d["g"], d["b"], d["w"], dt, bf=bf, form=form)
        refs.append(R.mlp_bwd_ln(d["dy"], f["hpre"], d["x"], d["g"], f["mean"], f["rstd"], d["w"], dt, bf=bf, form=form))
    (o64, sc), (o32, _) = refs
    ck.rule("dhp", "row", dhp, o32["dhp"], o64["dhp"], d["groups"])
    check_ln_bwd(ck, got, o32, o64, sc, d["groups"])
    if not precision:
        ck.rule("dx_vs_unfused", "row", got[0], o32["dx"], o64["dx"], d["groups"], against=pair[0])
        for i, k in enumerate(("dgamma", "dbeta", "colsum")):
            ck.rule(k + "_vs_unfused", "elem", got[1 + i], o32[k], o64[k], ALL, scale=sc[k], against=pair[1 + i])
    ck.done()


@pytest.mark.parametrize("with_add", [True, False])
@pytest.mark.parametrize("mode", ["fp32", "bf16_operands", "bf16_dy"])
@pytest.mark.parametrize("M", R.LN_MS)
def test_linear_dx_lnbwd_regimes(ops, M, mode, with_add):
    """ops.linear_dx_lnbwd -- the LayerNorm backward on the epilogue of the qkv input-gradient GEMM (csrc/gemm.hip; bf16 dY: rp_dx_lnbwd_bf16,
    csrc/dx_lnbwd_bf16.hip) -- with FUSE_LN_BWD on and off, as LN'(dy W), handed the statistics linear_rows wrote in the forward"""
    d = ln_data(M)
    cu, w = d["cu"], d["cu"]["w"]
    precision = 0 if mode == "fp32" else 1
    ck = Checks("norm_regimes.linear_dx_lnbwd[M=%d,%s,add=%d]" % (M, mode, with_add))
    dy = R.bf16_round(d["dyq"]) if mode == "bf16_dy" else d["dyq"]
    dyc = dy.cuda().to(BF) if mode == "bf16_dy" else dy.cuda()
    add = d["add"] if with_add else None
    keep = ops.FUSE_LN_BWD
    got = {}
    try:
        with gemm_precision(ops, precision):
            _, _, mean, rstd = ops.linear_rows(cu["x"], w["wq"], w["bq"], ln=(cu["g"], cu["b"]), want_ln_out=True)
            for fuse in ((True,) if mode == "bf16_dy" else (True, False)):
                ops.FUSE_LN_BWD = fuse
                got[fuse] = ops.linear_dx_lnbwd(dyc, w["wq"], cu["x"], cu["g"], mean, rstd, add=cu["add"] if with_add else None)
    finally:
        ops.FUSE_LN_BWD = keep
    o64, sc = R.dx_lnbwd(dy, d["w"]["wq"], d["x"], d["g"], d["f64"][1], d["f64"][2], F64, add)
    o32, _ = R.dx_lnbwd(dy, d["w"]["wq"], d["x"], d["g"], d["f32"][1], d["f32"][2], F32, add, bf=bool(precision), bf_dy=bool(precision))
    for fuse, g in got.items():
        check_ln_bwd(ck, g, o32, o64, sc, d["groups"], prefix="fused." if fuse else "unfused.")
    ck.done()


# ------------------------------------------------------------------------------------------------ BatchNorm family
def make_bn(c, training, C, momentum=R.MOMENTUM):
    bn = torch.nn.BatchNorm2d(C, eps=R.BN_EPS, momentum=momentum)
    with torch.no_grad():
        bn.weight.copy_(c["gamma"])
        bn.bias.copy_(c["beta"])
        bn.running_mean.copy_(c["rm"])
        bn.running_var.copy_(c["rv"])
    return bn.cuda().train(training)


def check_running(ck, c, bn, training):
    if not training:
        ck.exact("running statistics untouched in evaluation mode",
                 torch.equal(bn.running_mean.cpu(), c["rm"]) and torch.equal(bn.running_var.cpu(), c["rv"]))
        return
    for k, got in (("running_mean", bn.running_mean), ("running_var", bn.running_var)):
        ck.rule(k, "elem", got, c["f32"][k], c["f64"][k], c["groups"], scale=c["scale"][k], allow=c["allow"][k])


@pytest.mark.parametrize("with_res,relu", [(False, True), (True, True), (False, False), (True, False)])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", R.BN_SHAPES)
def test_bn_act_regimes(ops, shape, bf16, training, with_res, relu):
    """ops.bn_act (csrc/batchnorm.hip): y, dx, dres, dgamma, dbeta and the running statistics per channel and regime"""
    N, C, H, W = shape
    c = R.bn_case(shape, bf16, training, with_res, relu)
    dt = BF if bf16 else F32
    ck = Checks("norm_regimes.bn_act[%s,bf16=%d,train=%d,res=%d,relu=%d]" % ("x".join(map(str, shape)), bf16, training, with_res, relu))
    bn = make_bn(c, training, C)
    xg = c["x"].to(dt).cuda().contiguous(memory_format=CL).requires_grad_(True)
    rg = c["res"].to(dt).cuda().contiguous(memory_format=CL).requires_grad_(True) if with_res else None
    y = ops.bn_act(bn, xg, residual=rg, relu=relu)
    assert y.dtype == dt and y.is_contiguous(memory_format=CL)
    (y.float() * c["cot"].cuda()).sum().backward()
    extra = R.BF16_STORE if bf16 else 0.0
    f64, f32, b64, b32, al, g = c["f64"], c["f32"], c["b64"], c["b32"], c["allow"], c["groups"]
    ck.rule("y", "chan", y.detach().float(), f32["y"], f64["y"], g, extra=extra, allow=al["y"])
    ck.rule("dx", "chan", xg.grad.float(), b32["dx"], b64["dx"], g, extra=extra, allow=al["dx"])
    if with_res:
        ck.rule("dres", "chan", rg.grad.float(), b32["dres"], b64["dres"], g, extra=extra)
    ck.rule("dgamma", "elem", bn.weight.grad, b32["dgamma"], b64["dgamma"], g, scale=c["scale"]["dgamma"], allow=al["dgamma"])
    ck.rule("dbeta", "elem", bn.bias.grad, b32["dbeta"], b64["dbeta"], g, scale=c["scale"]["dbeta"])
    check_running(ck, c, bn, training)
    if training and not with_res:                      # d = x - pivot = 0 exactly: y = fma(0, rstd gamma, beta) = beta
        cc = g["constant"]
        want = (c["beta"][cc].relu() if relu else c["beta"][cc]).to(dt)
        ck.exact("y of constant channels = beta", bool((y.detach().cpu()[:, cc] == want[None, :, None, None]).all()))
    ck.done()


def _stats_abi(ops, xr, R_, C, bf, partials=None):
    """(mean, rstd) straight from rp_bn_stats / rp_bn_stats_from_partials, as BnActFn calls them"""
    from rel_pose_amd import _lib
    lib = _lib.load()
    mean, rstd = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    if partials is None:
        part = torch.empty(lib.rp_bn_partial_blocks(R_) * 2 * C, device="cuda", dtype=F64)
        lib.rp_bn_stats(ops._p(xr), R_, C, ops._p(part), ops._p(mean), ops._p(rstd), ops._p(rm), ops._p(rv), R.MOMENTUM, R.BN_EPS, bf, ops._st())
    else:
        lib.rp_bn_stats_from_partials(ops._p(partials), partials.shape[0], R_, C, ops._p(torch.zeros(C, device="cuda")), ops._p(mean),
                                      ops._p(rstd), ops._p(rm), ops._p(rv), R.MOMENTUM, R.BN_EPS, ops._st())
    return mean, rstd


def check_mean_rstd(ck, c, mean, rstd):
    ck.rule("mean", "elem", mean, c["f32"]["mean"], c["f64"]["mean"], c["groups"], scale=c["scale"]["mean"], allow=c["allow"]["mean"])
    ck.rule("rstd", "elem", rstd, c["f32"]["rstd"], c["f64"]["rstd"], c["groups"], allow=c["allow"]["rstd"])


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", R.BN_SHAPES)
def test_bn_statistics_regimes(ops, shape, bf16):
    """rp_bn_stats (bn_reduce_kernel / bn_reduce_g_kernel + bn_finalize_kernel): mean and rstd themselves; constant channels exactly"""
    N, C, H, W = shape
    c = R.bn_case(shape, bf16, True, False, False)
    ck = Checks("norm_regimes.bn_stats[%s,bf16=%d]" % ("x".join(map(str, shape)), bf16))
    xr = c["x"].to(BF if bf16 else F32).cuda().permute(0, 2, 3, 1).contiguous()
    mean, rstd = _stats_abi(ops, xr, N * H * W, C, int(bf16))
    check_mean_rstd(ck, c, mean, rstd)
    const = torch.cat([c["groups"]["constant"]] + ([c["groups"]["offset1000"]] if bf16 else []))
    ck.exact("mean of constant channels", torch.equal(mean.cpu()[const], c["x"][0, const, 0, 0]))
    ck.exact("rstd of constant channels within 1 ulp of 1 / sqrt(eps)", R.ulps32(rstd.cpu()[const], torch.full((len(const),), R.BN_EPS ** -0.5)) <= 1)
    ck.done()


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("kind", ["c64_f32", "c128_f32", "c64_bf16"])
def test_convolution_epilogue_statistics_regimes(ops, kind, N):
    """BatchNorm statistics from the partial sums of a convolution's epilogue (csrc/conv3x3_f32.hip, conv3x3_c128_f32.hip, conv3x3_bf16.hip:
    sums of y and y^2, a ZERO pivot) through ops.bn_act(..., stats=).  The filter is the centre-tap identity, so the output reproduces the
    regime channels of the input exactly; mean, rstd, y and the running statistics under the rule, with the allowance about a zero pivot on
    the pivot / spike / offset channels"""
    C, HW = (128, 28) if kind == "c128_f32" else (64, 56)
    bf16 = kind == "c64_bf16"
    dt = BF if bf16 else F32
    shape = (N, C, HW, HW)
    c = R.bn_case(shape, bf16, True, False, False, "zero")
    ck = Checks("norm_regimes.conv_stats[%s,N=%d]" % (kind, N))
    xr = c["x"].to(dt).cuda().permute(0, 2, 3, 1).contiguous()
    w = torch.zeros(C, 3, 3, C, device="cuda", dtype=dt)
    w[torch.arange(C), 1, 1, torch.arange(C)] = 1.0
    conv = dict(c64_f32=ops.conv3x3_c64_f32, c128_f32=ops.conv3x3_c128_f32, c64_bf16=ops.conv3x3_c64_bf16)[kind]
    y, stats = conv(xr, w, want_stats=True)
    assert torch.equal(y, xr), "the identity filter reproduces its input"
    mean, rstd = _stats_abi(ops, None, N * HW * HW, C, 0, partials=stats)
    check_mean_rstd(ck, c, mean, rstd)
    bn = make_bn(c, True, C)
    out = ops.bn_act(bn, y.permute(0, 3, 1, 2), relu=False, stats=stats)
    ck.rule("y", "chan", out.detach().float(), c["f32"]["y"], c["f64"]["y"], c["groups"], extra=R.BF16_STORE if bf16 else 0.0, allow=c["allow"]["y"])
    check_running(ck, c, bn, True)
    ck.done()


def _pool_reference(c, cot_pool, dtype, bound_abs):
    """pool(relu(bn(x))) and its backward in `dtype` from bn_case c: (pooled y, dict(dx, dgamma, dbeta), scales, keep) -- keep [N,C,OH,OW] = 0
    where fp64 cannot tell which element of the window wins (tests/_norm_regimes.py: pool_keep; its cap is proved on the CPU): the cotangent
    is zeroed there for the reference and the kernel alike (computed for fp64 only)"""
    import torch.nn.functional as Fn
    f = c["f64"] if dtype == F64 else c["f32"]
    r = f["pre"].relu().detach().requires_grad_(True)
    pooled = Fn.max_pool2d(r, 3, 2, 1)
    keep = None
    if bound_abs is not None:
        keep, _ = R.pool_keep(r.detach(), bound_abs)
        cot_pool = cot_pool * keep
    pooled.backward(cot_pool.to(dtype))
    out, sc, _ = R.bn_bwd(r.grad, c["x"], c["gamma"], f["mean"], f["rstd"], f["pre"], dtype, True, True, False)
    return pooled.detach(), out, sc, keep


def test_bn_relu_maxpool_regimes(ops):
    """ops.bn_relu_maxpool on the 64-channel regime tensor: the fused form bit-identical to the separate kernels in the forward (gradients to
    2e-6, as tests/test_gpu_kernels.py states), and against fp64 under the rule"""
    shape = R.BN_SHAPES[0]
    N, C, H, W = shape
    c = R.bn_case(shape, False, True, False, True)
    ck = Checks("norm_regimes.bn_relu_maxpool")
    pool = torch.nn.MaxPool2d(3, 2, 1)
    bound_abs = R.pool_bound(c)
    cot = R.randn(N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, seed=431)
    p64, o64, sc, keep = _pool_reference(c, cot, F64, bound_abs)
    cot = cot * keep.float()
    p32, o32, _, _ = _pool_reference(c, cot, F32, None)
    res = []
    prev = ops.FUSE_STEM_POOL
    try:
        for fused in (True, False):
            ops.FUSE_STEM_POOL = fused
            bn = make_bn(c, True, C)
            x = c["x"].cuda().contiguous(memory_format=CL).requires_grad_(True)
            y = ops.bn_relu_maxpool(bn, pool, x)
            y.backward(cot.cuda())
            res.append((y.detach(), x.grad, bn.weight.grad, bn.bias.grad, bn.running_mean.clone(), bn.running_var.clone(), bn))
    finally:
        ops.FUSE_STEM_POOL = prev
    ck.exact("fused forward and running statistics = separate kernels",
             torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][4], res[1][4]) and torch.equal(res[0][5], res[1][5]))
    for k, a, b in zip(("dx", "dgamma", "dbeta"), res[0][1:4], res[1][1:4]):
        ck.kv[k + "_fused_vs_separate"] = R.rel(a, b)
        ck.exact(k + ": fused within 2e-6 of separate", R.rel(a, b) < 2e-6)
    g = c["groups"]
    for name, (y, dx, dg, db, _, _, bn) in zip(("fused.", "separate."), res):
        pooled_allow = torch.nn.functional.max_pool2d(c["allow"]["y"], 3, 2, 1)
        ck.rule(name + "y", "chan", y, p32, p64, g, allow=pooled_allow)
        ck.rule(name + "dx", "chan", dx, o32["dx"], o64["dx"], g, allow=R.allowance_images(c["a"], c["x"], c["gamma"], c["f64"], o64, o64["dgamma"] / (N * H * W), sc)["dx"])
        ck.rule(name + "dgamma", "elem", dg, o32["dgamma"], o64["dgamma"], g, scale=sc["dgamma"], allow=R.dgamma_allowance(c["a"], c["f64"], sc))
        ck.rule(name + "dbeta", "elem", db, o32["dbeta"], o64["dbeta"], g, scale=sc["dbeta"])
    check_running(ck, c, res[0][6], True)
    ck.done()
