"""The transformer Block's dense kernels outside rp_gemm -- rp_linear_rows192, rp_mlp_fused_fwd / _bwd / _bwd_ln, rp_dw192_f32 / _split3 /
_bf16 with rp_splitk_reduce_multi, rp_ds_matmul / rp_ds_matmul_t, rp_dx_lnbwd_bf16 -- on operands for which the right answer is exact (tests/_block_cells.py: families, references, the mirror of
the stream-K partition and of the slab layout; tests/test_block_cells_cpu.py proves the premises on the CPU).

Every call goes through the C ABI (_lib.load()), so M below what `ops` would send here is reachable.  Operands with a leading dimension
carry NaN pad columns, every output and workspace is NaN before the call, a workspace has exactly the bytes the library reports, and 64
NaN elements of guard sit behind every output: stored values must equal the integer reference BIT FOR BIT (torch.equal; a bf16-stored
tensor: the reference rounded once to nearest even), pads and guards must still be NaN.  Every case asserts the partition class / slab
layout it was built to reach, computed by the mirror from rp_linear_rows192_grid / rp_mlp_fused_grid / rp_dw192_*_splits on this device.
The only bounded comparisons: GELU of arbitrary values, dx behind a LayerNorm backward, and y of the tiles the precision-1 training
forward finishes inside the MFMA (see test_mlp_fused_fwd_selector_cells) -- 8 x the plain fp32 restatement's error, floor 4 ulps, + 2^-8 for
a bf16-stored tensor; the worst share of the limit goes to the test report."""
import ctypes
import functools
import re

import pytest
import torch

from tests import _block_cells as B
from tests import _gemm_cells as G
from tests import _norm_regimes as R
from tests.test_gpu_kernels import report

pytestmark = pytest.mark.gpu

NAN = float("nan")
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
GUARD = 64
EPS = 1e-5


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    return _lib.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


def put(t, dtype=F32):
    return t.to("cuda").to(dtype).contiguous()


class Out:
    """an output of `shape`, NaN before the call, with GUARD NaN elements behind it"""

    def __init__(self, shape, dtype=F32):
        n = 1
        for s in shape:
            n *= s
        self.flat = torch.full((n + GUARD,), NAN, dtype=dtype, device="cuda")
        self.t = self.flat[:n].view(shape)

    def ptr(self):
        return self.flat.data_ptr()

    def guard_ok(self):
        return bool(self.flat[-GUARD:].isnan().all())


class Padded:
    """[rows, cols] with row stride ld inside a NaN-filled buffer"""

    def __init__(self, rows, cols, ld, dtype, data=None):
        self.shape, self.ld = (rows, cols), ld
        self.flat = torch.full((rows * ld + GUARD,), NAN, dtype=dtype, device="cuda")
        if data is not None:
            self.view().copy_(data)

    def view(self):
        return self.flat.as_strided(self.shape, (self.ld, 1))

    def ptr(self):
        return self.flat.data_ptr()

    def pads_untouched(self):
        r, c = self.shape
        return int(self.flat.isnan().sum()) == self.flat.numel() - r * c + int(self.view().isnan().sum())


class Judge:
    def __init__(self, key):
        self.key, self.failed, self.n, self.worst = key, [], 0, 0.0

    def fail(self, name, what):
        self.failed.append("%s: %s" % (name, what))

    def exact(self, name, what, got, want):
        if got.shape != want.shape or got.dtype != want.dtype or not torch.equal(got, want):
            if got.shape != want.shape:
                return self.fail(name, "%s: shape %s, want %s" % (what, tuple(got.shape), tuple(want.shape)))
            bad = (got.double() != want.double()) | got.isnan()
            at = tuple(int(i) for i in bad.nonzero()[0])
            self.fail(name, "%s: %d of %d elements differ, first at %s: got %r, want %r" % (
                what, int(bad.sum()), bad.numel(), at, float(got[at]), float(want[at])))

    def bounded(self, name, what, got, pre64, form, bf_store=False):
        """a GELU output under the bound rule of tests/_norm_regimes.py: element-wise error against fp64 GELU of the EXACT pre-activation
        at most 8 x the error of the plain fp32 torch restatement on the same input, floor 4 ulps, + 2^-8 for a bf16-stored tensor"""
        if not bool(torch.isfinite(got.float()).all()):
            return self.fail(name, what + ": not finite")
        if got.shape[0] > 4096:      # rows repeat with period B.PERIOD: more than one period and the last (ragged) tile carry every value
            rows = torch.cat([torch.arange(B.PERIOD + 69), torch.arange(got.shape[0] - 300, got.shape[0])]).to(got.device)
            got, pre64 = got[rows], pre64[rows]
        want, yard = R.gelu(pre64, form), R.gelu(pre64.float(), form)
        n = want.numel()
        j = R.judge("elem", got.flatten(), yard.flatten(), want.flatten(), {"all": torch.arange(n)}, scale=torch.ones(n, dtype=F64),
                    extra=R.BF16_STORE if bf_store else 0.0)[0]
        self.worst = max(self.worst, j["of_limit"])
        if not j["of_limit"] <= 1.0:
            self.fail(name, "%s: %.3e at %d = %.2f x its limit (plain fp32: %.3e)" % (what, j["err"], j["where"], j["of_limit"], j["yard"]))

    def sum_bounded(self, name, what, got, yard, want):
        """the same rule for a sum the kernel legitimately rounds its own way: yard = the plain fp32 restatement, want = fp64"""
        n = want.numel()
        j = R.judge("elem", got.flatten(), yard.flatten(), want.flatten(), {"all": torch.arange(n)}, scale=torch.ones(n, dtype=F64))[0]
        self.worst_sum = max(getattr(self, "worst_sum", 0.0), j["of_limit"])
        if not j["of_limit"] <= 1.0:
            self.fail(name, "%s: %.3e at %d = %.2f x its limit (plain fp32: %.3e)" % (what, j["err"], j["where"], j["of_limit"], j["yard"]))

    def guards(self, name, **outs):
        for k, o in outs.items():
            if o is not None and not o.guard_ok():
                self.fail(name, k + ": written past its end")

    def check(self, name, cond, what):
        if not cond:
            self.fail(name, what)

    def done(self, **kw):
        report("block_cells." + self.key, cases=self.n, worst_gelu_of_limit=self.worst, worst_sum_of_limit=getattr(self, "worst_sum", 0.0), **kw)
        assert not self.failed, "%d of %d cases -- " % (len({f.split(":")[0] for f in self.failed}), self.n) + "; ".join(self.failed[:8])


def store(t, bf):
    """an fp64 reference as the kernel stores it: fp32, or bf16 by ONE rounding to nearest even"""
    return t.float().to(BF) if bf else t.float()


# ------------------------------------------------------------------------------------------------ rp_linear_rows192
@functools.lru_cache(maxsize=None)
def linear_big_m(lib, ln, prec):
    """the smallest (ragged) M at N = 768 whose ranges hold two or more chunks, start inside tiles and run across tile boundaries"""
    def want(t, g):
        mid, cross, base = B.range_classes(t, B.NCHUNK, g)
        return base >= 2 and mid and cross
    return B.smallest_m(B.ROWS_LINEAR, B.NCHUNK, lambda M: lib.rp_linear_rows192_grid(M, 768, ln, prec), want, ragged=17)


def linear_partition(jd, lib, c, big):
    """assert the class the case was built for, from the grid the launch will use"""
    ln = int(c.form == "ln")
    g = lib.rp_linear_rows192_grid(c.M, c.N, ln, c.prec)
    tiles, nchunk = -(-c.M // lib.rp_linear_rows192_tile_rows()), c.N // B.CH
    assert lib.rp_linear_rows192_tile_rows() == B.ROWS_LINEAR and 0 < g <= tiles * nchunk, B.lname(c)
    mid, cross, base = B.range_classes(tiles, nchunk, g)
    if big:
        assert base >= 2 and mid and cross and tiles * nchunk > g, (B.lname(c), g, base, mid, cross)
    else:
        assert g == tiles * nchunk and base == 1 and not cross, (B.lname(c), g)        # items < slots: one chunk per workgroup
    return g


def run_linear(lib, c, o, act=0, side=True, want_pre=False):
    """one launch of a case; returns the outputs (Out objects or None)"""
    M, N, io, p1 = c.M, c.N, c.io, c.prec == 1
    x = put(o["x"], BF if io & 1 else F32)
    w = put(o["w"], BF if p1 else F32)
    ln = c.form == "ln"
    bias = put(o["bias"]) if c.form in B.BIASED else None
    res = put(o["res"]) if c.form in ("bias_res", "gelu_res") else None
    aux = put(o["aux"], BF if io & 4 else F32) if c.form == "dact_cs" else None
    gamma, beta = (put(o["gamma"]), put(o["beta"])) if ln else (None, None)
    ydt = BF if io & 2 else F32
    r = dict(y=Out((M, N), ydt), pre=Out((M, N), ydt) if want_pre else None, xn=None, mean=None, rstd=None, cs=None)
    if ln and side:
        r.update(xn=Out((M, B.C), BF if io & 8 else F32), mean=Out((M,)), rstd=Out((M,)))
    if c.form == "dact_cs":
        r["cs"] = Out((-(-M // B.ROWS_LINEAR), N))
    ptr = lambda k: None if r[k] is None else r[k].ptr()
    lib.rp_linear_rows192(_p(x), _p(w), _p(bias), _p(res), _p(gamma), _p(beta), EPS, ptr("y"), ptr("pre"), ptr("xn"), ptr("mean"),
                          ptr("rstd"), _p(aux), ptr("cs"), M, N, B.C, act, c.prec, io, _stream())
    return r


def check_linear(jd, lib, c):
    jd.n += 1
    nm = B.lname(c)
    o = B.linear_operands(c.form, c.fam, c.M, c.N)
    ybf = bool(c.io & 2)
    if c.form == "ln":
        tr = run_linear(lib, c, o)
        jd.guards(nm, **tr)
        xn = tr["xn"].t.double()
        if c.prec == 1 and not c.io & 8:
            xn = G.bf16_round(xn)                      # the MFMA consumed the stored fp32 rows rounded to nearest even
        pre64 = put(o["wv"], F64)[None, :] * xn[:, put(o["k"], torch.int64)]            # one product with a power of two: exact in fp32
        want = store(pre64, ybf)
        jd.check(nm, bool(torch.isfinite(tr["xn"].t.float()).all()), "xn_out not finite")
        jd.exact(nm, "y vs +-2^j xn_out[m, k(n)]", tr["y"].t, want)
        pr = run_linear(lib, c, o, act=1, want_pre=True)
        jd.guards(nm, **pr)
        jd.exact(nm, "y_pre of the GELU launch", pr["pre"].t, want)
        jd.bounded(nm, "GELU y", pr["y"].t, pre64, "tanh" if c.prec == 1 else "erf", ybf)
        for k in ("xn", "mean", "rstd"):
            jd.exact(nm, k + " of the two launches", pr[k].t, tr[k].t)
        if not c.io & 8:
            inf = run_linear(lib, c, o, side=False)
            jd.guards(nm, **inf)
            jd.exact(nm, "inference y vs training y", inf["y"].t, tr["y"].t)
        return
    v = {k: put(t, F64) for k, t in o.items()}
    y, pre, cs = B.linear_reference(c, v)
    gelu = c.form in ("gelu_pre", "gelu_res")
    r = run_linear(lib, c, o, act=int(gelu), want_pre=gelu)
    jd.guards(nm, **r)
    jd.exact(nm, "y", r["y"].t, store(y, ybf))
    if pre is not None:
        jd.exact(nm, "y_pre", r["pre"].t, store(pre, ybf))
    if cs is not None:                                   # (the last tile's partial counts nothing past M: the reference pads with zeros)
        jd.exact(nm, "colsum_part", r["cs"].t, cs.float())


def test_gelu_grad_at_its_two_exact_points_linear_dx(lib):
    """GELU'(0) = 0.5 and GELU'(x >= 8) = 1 read back through rp_linear_rows192 itself: dy = 1, W = I, so y = GELU'(aux); erf form
    (precision 0, v_exp_f32(-1)) and sigmoid form (precision 1, v_rcp_f32(2))"""
    M, N = 65, 192
    aux = B.preact(M, N, 99)
    got = {}
    for prec in (0, 1):
        c = B.LCase("dact_cs", M, N, prec, 0, "readback")
        o = dict(x=torch.ones(M, B.C), w=torch.eye(N), aux=aux)
        r = run_linear(lib, c, o)
        y = r["y"].t
        got[prec] = sorted(set(y.flatten().tolist()))
        assert torch.equal(y, B.gelu_grad_x(put(aux, F64)).float()), (prec, got[prec])
    assert got[0] == got[1] == [0.5, 1.0]
    report("block_cells.gelu_grad_readback.linear_dx", erf_at_0=got[0][0], erf_at_8_up=got[0][1], sigmoid_at_0=got[1][0], sigmoid_at_8_up=got[1][1])


LINEAR_KEYS = [(f, p) for f in B.LFORMS for p in (0, 1)]


@pytest.mark.parametrize("form,prec", LINEAR_KEYS, ids=["%s-p%d" % k for k in LINEAR_KEYS])
def test_linear_rows_cells(lib, form, prec):
    jd = Judge("linear_rows.%s.p%d" % (form, prec))
    big = linear_big_m(lib, int(form == "ln"), prec)
    grids = {}
    for io in B.linear_io(form, prec):
        for fam in B.linear_family(form, prec, io):
            for M, N in B.linear_shapes(big):
                c = B.LCase(form, M, N, prec, io, fam)
                grids[(M, N)] = linear_partition(jd, lib, c, M == big)
                check_linear(jd, lib, c)
    jd.done(big_m=big, grid_at_big_m=grids[(big, 768)])


# ------------------------------------------------------------------------------------------------ rp_mlp_fused_fwd / _bwd
@functools.lru_cache(maxsize=None)
def mlp_ms(lib, backward, train, prec):
    """((M, classes it must reach), ...): one row, one ragged tile, three tiles shared by all 24 chunks, and the smallest M with an
    owner-finished tile next to one shared by exactly two ranges"""
    rows = B.mlp_rows(backward, prec)
    grid_of = lambda M: lib.rp_mlp_fused_grid(M, backward, train, prec)
    big = B.smallest_m(rows, B.NCHUNK, grid_of, lambda t, g: {"owner", "two"} <= B.tile_classes(t, B.NCHUNK, g), ragged=11)
    return ((1, {"all"}), (rows - 11, {"all"}), (3 * rows - 5, {"all"}), (big, {"owner", "two"}))


def mlp_partition(lib, M, backward, train, prec, must):
    rows = B.mlp_rows(backward, prec)
    g = lib.rp_mlp_fused_grid(M, backward, train, prec)
    tiles = -(-M // rows)
    cls = B.tile_classes(tiles, B.NCHUNK, g)
    assert 0 < g <= tiles * B.NCHUNK and must <= cls and (must != {"all"} or cls == {"all"}), (M, g, cls, must)
    # the partial tiles of this launch fit the workspace the library reports (mlp_fused.hip: G ranges x P tiles a range can touch)
    base = B.split(tiles * B.NCHUNK, g)[0]
    need = g * ((base + 1 + B.NCHUNK - 1) // B.NCHUNK + 1) * rows * B.C * 4
    have = lib.rp_mlp_fused_bwd_workspace_bytes(M) if backward else lib.rp_mlp_fused_workspace_bytes(M)
    assert need <= have, (M, backward, train, prec, need, have)
    return g, cls, B.sharers(tiles, B.NCHUNK, g)


def big_case(seen):
    """figures of the largest M of a test for the report: M, its grid, how many tiles the owner finished and how many two ranges share"""
    M = max(seen)
    g, cls, share = seen[M]
    return dict(big_m=M, grid=g, owner_tiles=int((share == 1).sum()), two_way_tiles=int((share == 2).sum()), classes=len(cls))


def run_mlp_fwd(lib, M, prec, train, io):
    o = B.mlp_fwd_operands(M)
    v = {k: put(t, F64) for k, t in o.items()}
    x = B.periodic(v["c"], M)[:, None].expand(M, B.C).float().contiguous()
    wdt = BF if prec == 1 else F32
    w2 = B.second_weight(v["w2"], bool(io & 16)) if prec == 1 else v["w2"]
    ins = [x, v["gamma"].float(), v["beta"].float(), v["w1"].to(wdt).contiguous(), v["b1"].float(), w2.to(wdt).contiguous(), v["b2"].float()]
    nbytes = lib.rp_mlp_fused_workspace_bytes(M)
    assert nbytes % 4 == 0 and nbytes > 0
    r = dict(y=Out((M, B.C)), ws=Out((nbytes // 4,)), xn=None, mean=None, rstd=None, h=None, hpre=None)
    if train:
        r.update(xn=Out((M, B.C), BF if io & 8 else F32), mean=Out((M,)), rstd=Out((M,)),
                 h=Out((M, B.HID), BF if io & 2 else F32), hpre=Out((M, B.HID), BF if io & 2 else F32))
    ptr = lambda k: None if r[k] is None else r[k].ptr()
    lib.rp_mlp_fused_fwd(*[_p(t) for t in ins], ptr("y"), ptr("ws"), M, B.C, B.HID, EPS, ptr("xn"), ptr("mean"), ptr("rstd"), ptr("h"),
                         ptr("hpre"), prec, io, _stream())
    return r, v


FWD_KEYS = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 0, 16), (1, 1, 0), (1, 1, 2), (1, 1, 8), (1, 1, 16), (1, 1, 26)]


@pytest.mark.parametrize("prec,train,io", FWD_KEYS, ids=["p%d-train%d-io%d" % k for k in FWD_KEYS])
def test_mlp_fused_fwd_cells(lib, prec, train, io):
    """const_rows: LayerNorm gives beta back, both products, bias, GELU and the residual are integer arithmetic -- in the owner's epilogue
    and in the fix-up alike"""
    jd = Judge("mlp_fwd.p%d.train%d.io%d" % (prec, train, io))
    seen = {}
    for M, must in mlp_ms(lib, 0, train, prec):
        nm = "mlp_fwd M=%d" % M
        jd.n += 1
        seen[M] = mlp_partition(lib, M, 0, train, prec, must)
        r, v = run_mlp_fwd(lib, M, prec, train, io)
        jd.guards(nm, **r)
        y, hpre, h = B.mlp_fwd_reference(v, M)
        jd.exact(nm, "y", r["y"].t, y.float())
        if train:
            jd.exact(nm, "xn_out == beta", r["xn"].t, store(v["beta"][None, :].expand(M, B.C), io & 8))
            jd.exact(nm, "mean_out", r["mean"].t, B.periodic(v["c"], M).float())
            jd.exact(nm, "hpre_out", r["hpre"].t, store(hpre[None, :].expand(M, B.HID), io & 2))
            jd.exact(nm, "h_out", r["h"].t, store(h[None, :].expand(M, B.HID), io & 2))
            want_rstd = torch.full((M,), EPS, dtype=F32, device="cuda").rsqrt()
            jd.check(nm, bool(((r["rstd"].t - want_rstd).abs() <= 4 * 2.0 ** -23 * want_rstd).all()), "rstd_out")
        del r
    jd.done(**big_case(seen))


SEL_KEYS = [(0, 0), (1, 0), (1, 26)]


@pytest.mark.parametrize("prec,io", SEL_KEYS, ids=["p%d-io%d" % k for k in SEL_KEYS])
def test_mlp_fused_fwd_selector_cells(lib, prec, io):
    """arbitrary fp32 rows through the fused LayerNorm: hpre_out == +-2^j xn_out[m, k(u)] (precision 1: against the rows rounded to bf16,
    nearest even), y == fl(x + +-2^j h_out[m, u(n)]) with ONE rounding in the owner's epilogue and in the fix-up alike, the inference
    form's y equal to the training form's; h_out itself under the bound rule.  The four M classes use shifts 0..3: every hidden unit is
    selected by w2 once."""
    jd = Judge("mlp_fwd_selector.p%d.io%d" % (prec, io))
    seen = {}
    wdt = BF if prec == 1 else F32
    for shift, (M, must) in enumerate(mlp_ms(lib, 0, 1, prec)):
        nm = "mlp_fwd_selector M=%d" % M
        jd.n += 1
        seen[M] = mlp_partition(lib, M, 0, 1, prec, must)
        o = B.mlp_selector_operands(M, shift)
        v = {k: put(t, t.dtype) for k, t in o.items()}
        x = B.periodic(v["x"], M).contiguous()
        w2 = B.second_weight(v["w2"], bool(io & 16)) if prec == 1 else v["w2"]
        zero1, zero2 = torch.zeros(B.HID, device="cuda"), torch.zeros(B.C, device="cuda")
        ins = [x, v["gamma"], v["beta"], v["w1"].to(wdt).contiguous(), zero1, w2.to(wdt).contiguous(), zero2]
        nbytes = lib.rp_mlp_fused_workspace_bytes(M)
        outs = {}
        for train in (1, 0):
            if not train:                                    # (the inference form takes bit 4 only, and may cut its ranges differently)
                mlp_partition(lib, M, 0, 0, prec, set())
            r = dict(y=Out((M, B.C)), ws=Out((nbytes // 4,)), xn=None, mean=None, rstd=None, h=None, hpre=None)
            if train:
                r.update(xn=Out((M, B.C), BF if io & 8 else F32), mean=Out((M,)), rstd=Out((M,)),
                         h=Out((M, B.HID), BF if io & 2 else F32), hpre=Out((M, B.HID), BF if io & 2 else F32))
            ptr = lambda k: None if r[k] is None else r[k].ptr()
            lib.rp_mlp_fused_fwd(*[_p(t) for t in ins], ptr("y"), ptr("ws"), M, B.C, B.HID, EPS, ptr("xn"), ptr("mean"), ptr("rstd"),
                                 ptr("h"), ptr("hpre"), prec, io if train else io & 16, _stream())
            jd.guards(nm, **r)
            outs[train] = r
        r = outs[1]
        xn = r["xn"].t.double()
        if prec == 1 and not io & 8:
            xn = G.bf16_round(xn)
        pre64 = v["wv1"][None, :] * xn[:, v["k1"]]
        jd.exact(nm, "hpre_out vs +-2^j xn_out[m, k(u)]", r["hpre"].t, store(pre64, io & 2))
        jd.bounded(nm, "h_out", r["h"].t, pre64, "tanh" if prec == 1 else "erf", bool(io & 2))
        h = r["h"].t.double()
        if prec == 1:
            h = G.bf16_round(h)                              # the second product consumes h packed to bf16
        prod = (v["wv2"][None, :] * h[:, v["u2"]]).float()  # exact: a power of two
        # ONE rounding: the fp32 sum of two fp32 numbers.  Exception, read from mlp_fused.hip (ACCX): the precision-1 TRAINING form starts
        # the accumulators of a tile it owns at x + b2, so the product is added inside the bf16 MFMA, whose accumulate step is not an IEEE
        # round-to-nearest add (measured: 0.26 % of such elements one ulp off).  Those rows go by the bound rule; every other row -- fix-up
        # tiles, the inference form, precision 0 -- stays exact.
        exact_rows = torch.ones(M, dtype=torch.bool, device="cuda")
        if prec == 1:
            own = (seen[M][2] == 1).to("cuda")
            exact_rows = ~own[torch.arange(M, device="cuda") // B.mlp_rows(0, prec)]
        jd.exact(nm, "y vs fl(x + +-2^j h_out[m, u(n)])", r["y"].t[exact_rows], (x + prod)[exact_rows])
        jd.exact(nm, "inference y vs fl(x + +-2^j h_out[m, u(n)])", outs[0]["y"].t, x + prod)
        if not bool(exact_rows.all()):
            rows = (~exact_rows).nonzero()[:, 0][:B.PERIOD + 69]
            jd.sum_bounded(nm, "y of owner-finished tiles (MFMA accumulate)", r["y"].t[rows], (x + prod)[rows], x[rows].double() + prod[rows].double())
        del outs, r
    jd.done(**big_case(seen))


def test_mlp_fused_fwd_layouts_and_forms_agree(lib):
    """the chunk-major second weight gives the bits of the plain layout, the inference form those of the training form (precision 1; at
    precision 0 the two forms may cut their ranges differently and still must agree)"""
    M = 3 * 192 - 5
    base = run_mlp_fwd(lib, M, 1, 0, 0)[0]["y"].t
    for train, io in ((0, 16), (1, 0), (1, 16), (1, 26)):
        assert torch.equal(run_mlp_fwd(lib, M, 1, train, io)[0]["y"].t, base), (train, io)
    assert torch.equal(run_mlp_fwd(lib, M, 0, 1, 0)[0]["y"].t, run_mlp_fwd(lib, M, 0, 0, 0)[0]["y"].t)


def run_mlp_bwd(lib, M, prec, io, o=None):
    v = {k: put(t, F64) for k, t in (o or B.mlp_bwd_operands(M)).items()}
    dy, hpre = B.periodic(v["dy"], M).float().contiguous(), B.periodic(v["hpre"], M).to(BF if io & 4 else F32).contiguous()
    wdt = BF if prec == 1 else F32
    w1t = B.second_weight(v["w1t"], bool(io & 16)) if prec == 1 else v["w1t"]
    tiles = -(-M // lib.rp_mlp_fused_bwd_tile_rows())
    nbytes = lib.rp_mlp_fused_bwd_workspace_bytes(M)
    assert nbytes % 4 == 0 and nbytes > 0 and lib.rp_mlp_fused_bwd_tile_rows() == B.mlp_rows(1, prec)
    r = dict(dhp=Out((M, B.HID), BF if io & 2 else F32), dxn=Out((M, B.C)), cp=Out((tiles, B.HID)), ws=Out((nbytes // 4,)))
    w2k, w1k = v["w2t"].to(wdt).contiguous(), w1t.to(wdt).contiguous()           # (named: they must outlive the call)
    lib.rp_mlp_fused_bwd(_p(dy), _p(hpre), _p(w2k), _p(w1k), r["dhp"].ptr(), r["dxn"].ptr(), r["cp"].ptr(), r["ws"].ptr(), M, B.C, B.HID,
                         prec, io, _stream())
    return r, v


def test_gelu_grad_at_its_two_exact_points_mlp_bwd(lib):
    """the same two points read from dhp: dy = 1 and one unit weight per hidden unit make dh = 1, so dhp = GELU'(hpre)"""
    M = 150
    w2t = torch.zeros(B.HID, B.C, dtype=torch.int64)
    w2t[torch.arange(B.HID), torch.arange(B.HID) % B.C] = 1
    o = dict(B.mlp_bwd_operands(M), dy=torch.ones(M, B.C, dtype=torch.int64), w2t=w2t)
    got = {}
    for prec in (0, 1):
        r, v = run_mlp_bwd(lib, M, prec, 0, o)
        got[prec] = sorted(set(r["dhp"].t.flatten().tolist()))
        assert torch.equal(r["dhp"].t, B.gelu_grad_x(B.periodic(v["hpre"], M)).float()), (prec, got[prec])
    assert got[0] == got[1] == [0.5, 1.0]
    report("block_cells.gelu_grad_readback.mlp_bwd", erf_at_0=got[0][0], erf_at_8_up=got[0][1], sigmoid_at_0=got[1][0], sigmoid_at_8_up=got[1][1])


BWD_KEYS = [(0, 0), (1, 0), (1, 2), (1, 4), (1, 16), (1, 22)]


@pytest.mark.parametrize("prec,io", BWD_KEYS, ids=["p%d-io%d" % k for k in BWD_KEYS])
def test_mlp_fused_bwd_cells(lib, prec, io):
    """dhp, dxn and the column sums of dhp, exact on small_int x gelu_exact (GELU' is 0.5 or 1); precision 1 packs dhp to bf16 by
    round-to-nearest-even for the second product"""
    jd = Judge("mlp_bwd.p%d.io%d" % (prec, io))
    seen = {}
    for M, must in mlp_ms(lib, 1, 0, prec):
        nm = "mlp_bwd M=%d" % M
        jd.n += 1
        seen[M] = mlp_partition(lib, M, 1, 0, prec, must)
        r, v = run_mlp_bwd(lib, M, prec, io)
        jd.guards(nm, **r)
        dhp, dxn, cp = B.mlp_bwd_reference(v, M, prec)
        jd.exact(nm, "dhp", r["dhp"].t, store(dhp, io & 2))
        jd.exact(nm, "dxn", r["dxn"].t, dxn.float())
        jd.exact(nm, "colpart", r["cp"].t, cp.float())
        del r
    jd.done(**big_case(seen))


BWD_LN_KEYS = [(0, 0), (1, 0), (1, 22)]


@pytest.mark.parametrize("prec,io", BWD_LN_KEYS, ids=["p%d-io%d" % k for k in BWD_LN_KEYS])
def test_mlp_fused_bwd_ln_cells(lib, prec, io):
    """the LayerNorm backward folded into the epilogue: with an integer-grade xhat all three thirds of ln_part are exact, compared PER ROW
    BLOCK (owner-finished tiles: the whole tile in the first of its four rows, zeros behind; fix-up tiles: four blocks of 48 rows); dhp and
    colpart exact as in rp_mlp_fused_bwd; dx carries 1/192 means and goes by the bound rule"""
    jd = Judge("mlp_bwd_ln.p%d.io%d" % (prec, io))
    seen, worst_dx = {}, 0.0
    wdt = BF if prec == 1 else F32
    for M, must in mlp_ms(lib, 1, 0, prec):
        nm = "mlp_bwd_ln M=%d" % M
        jd.n += 1
        seen[M] = mlp_partition(lib, M, 1, 0, prec, must)
        v = {k: put(t, F64) for k, t in B.mlp_bwd_ln_operands(M).items()}
        dy64, hpre64 = B.periodic(v["dy"], M), B.periodic(v["hpre"], M)
        mean64, rstd64 = B.periodic(v["mean"], M), 2.0 ** B.periodic(v["rexp"], M)
        x64 = B.periodic(v["xc"], M) + mean64[:, None]
        dy, hpre = dy64.float().contiguous(), hpre64.to(BF if io & 4 else F32).contiguous()
        lnx, gamma, mean, rstd = x64.float().contiguous(), v["gamma"].float(), mean64.float().contiguous(), rstd64.float().contiguous()
        w1t = B.second_weight(v["w1t"], bool(io & 16)) if prec == 1 else v["w1t"]
        w2k, w1k = v["w2t"].to(wdt).contiguous(), w1t.to(wdt).contiguous()
        tiles = -(-M // 192)
        nbytes, prow = lib.rp_mlp_fused_bwd_workspace_bytes(M), lib.rp_mlp_fused_bwd_ln_part_rows(M)
        assert prow == tiles * B.LN_SUB
        r = dict(dhp=Out((M, B.HID), BF if io & 2 else F32), dx=Out((M, B.C)), cp=Out((tiles, B.HID)), ws=Out((nbytes // 4,)),
                 part=Out((prow, 3 * B.C)))
        lib.rp_mlp_fused_bwd_ln(_p(dy), _p(hpre), _p(w2k), _p(w1k), r["dhp"].ptr(), r["dx"].ptr(), r["cp"].ptr(), r["ws"].ptr(), M, B.C, B.HID,
                                prec, io, _p(lnx), _p(gamma), _p(mean), _p(rstd), r["part"].ptr(), _stream())
        jd.guards(nm, **r)
        dhp, dxn, cp = B.mlp_bwd_reference(v, M, prec)
        jd.exact(nm, "dhp", r["dhp"].t, store(dhp, io & 2))
        jd.exact(nm, "colpart", r["cp"].t, cp.float())
        xhat = (x64 - mean64[:, None]) * rstd64[:, None]
        jd.exact(nm, "ln_part per row block", r["part"].t, B.ln_part_reference(dxn, xhat, dy64, seen[M][2])[0].float())
        rows = torch.arange(M, device="cuda") if M <= 4096 else torch.cat([torch.arange(B.PERIOD + 69), torch.arange(M - 300, M)]).to("cuda")
        want = R.ln_bwd(dxn[rows], x64[rows], v["gamma"], mean64[rows], rstd64[rows], F64, add=dy64[rows])[0]["dx"]
        yard = R.ln_bwd(dxn[rows], x64[rows], v["gamma"], mean64[rows], rstd64[rows], F32, add=dy64[rows])[0]["dx"]
        got = r["dx"].t[rows]
        if not bool(torch.isfinite(got).all()):
            jd.fail(nm, "dx not finite")
        else:
            j = R.judge("row", got, yard, want, {"all": torch.arange(rows.numel())})[0]
            worst_dx = max(worst_dx, j["of_limit"])
            jd.check(nm, j["of_limit"] <= 1.0, "dx: %.3e in row %d = %.2f x its limit (plain fp32: %.3e)" % (j["err"], j["where"], j["of_limit"], j["yard"]))
        del r
    jd.done(worst_dx_of_limit=worst_dx, **big_case(seen))


@pytest.mark.parametrize("with_add", (0, 1), ids=["plain", "add"])
def test_dx_lnbwd_bf16_cells(lib, with_add):
    """dx = LayerNorm'(dY W) (+ add) on the bf16 data path: one ragged tile and several tiles (from rp_dx_lnbwd_bf16_tile_rows); with the
    integer-grade xhat every plane of `part` is exact; dx goes by the bound rule"""
    jd = Judge("dx_lnbwd_bf16.add%d" % with_add)
    rows_t = lib.rp_dx_lnbwd_bf16_tile_rows()
    worst_dx = 0.0
    for M in (rows_t - 11, 3 * rows_t - 5):
        nm = "dx_lnbwd_bf16 M=%d add=%d" % (M, with_add)
        jd.n += 1
        v = {k: put(t, F64) for k, t in B.dx_lnbwd_operands(M).items()}
        x64, rstd64 = v["xc"] + v["mean"][:, None], 2.0 ** v["rexp"]
        dy, wt = v["dy"].to(BF).contiguous(), v["wt"].to(BF).contiguous()
        x, gamma, mean, rstd = x64.float().contiguous(), v["gamma"].float(), v["mean"].float(), rstd64.float().contiguous()
        add = v["add"].float().contiguous() if with_add else None
        tiles = -(-M // rows_t)
        r = dict(dx=Out((M, B.C)), part=Out((tiles, 3 if with_add else 2, B.C)))
        lib.rp_dx_lnbwd_bf16(_p(dy), _p(wt), _p(x), _p(gamma), _p(mean), _p(rstd), _p(add), r["dx"].ptr(), r["part"].ptr(), M, 576, _stream())
        jd.guards(nm, **r)
        dxn = v["dy"] @ v["wt"].t()
        xhat = v["xc"] * rstd64[:, None]
        jd.exact(nm, "part", r["part"].t, B.dx_lnbwd_part(dxn, xhat, v["add"] if with_add else None, rows_t).float())
        a64 = v["add"] if with_add else None
        want = R.ln_bwd(dxn, x64, v["gamma"], v["mean"], rstd64, F64, add=a64)[0]["dx"]
        yard = R.ln_bwd(dxn, x64, v["gamma"], v["mean"], rstd64, F32, add=a64)[0]["dx"]
        if not bool(torch.isfinite(r["dx"].t).all()):
            jd.fail(nm, "dx not finite")
        else:
            j = R.judge("row", r["dx"].t, yard, want, {"all": torch.arange(M)})[0]
            worst_dx = max(worst_dx, j["of_limit"])
            jd.check(nm, j["of_limit"] <= 1.0, "dx: %.3e in row %d = %.2f x its limit (plain fp32: %.3e)" % (j["err"], j["where"], j["of_limit"], j["yard"]))
    jd.done(worst_dx_of_limit=worst_dx)


DX_REFUSALS = [("dy null", -1, dict(dy=None)), ("part null", -1, dict(part=None)), ("M=0", -1, dict(M=0)), ("K != 576", -4, dict(K=192)),
               ("dy misaligned", -2, dict(dy=("a", 4))), ("add misaligned", -2, dict(add=("c", 8)))]


@pytest.mark.parametrize("name,code,kw", DX_REFUSALS, ids=[re.sub(r"\W+", "_", r[0]) for r in DX_REFUSALS])
def test_dx_lnbwd_bf16_refusals(lib, rbufs, name, code, kw):
    a = dict(dy="a", part="out", M=64, K=576, add=None)
    a.update(kw)

    def ptr(k):
        return None if k is None else (rbufs[k].data_ptr() if isinstance(k, str) else rbufs[k[0]].data_ptr() + k[1])
    _refused(lambda: lib.rp_dx_lnbwd_bf16(ptr(a["dy"]), ptr("b"), ptr("c"), ptr("d"), ptr("e"), ptr("f"), ptr(a["add"]), ptr("out"), ptr(a["part"]),
                                          a["M"], a["K"], _stream()), code)
    torch.cuda.synchronize()
    assert bool(rbufs["out"].isnan().all()), name + ": an output was written by a refused call"


# ------------------------------------------------------------------------------------------------ rp_dw192_*
DW_KERNELS = ("f32", "split3", "bf16", "bf16_b32")


def dw_ms(kernel, N):
    sr = 64 if kernel.startswith("bf16") else 32
    small = (64, 128, 320) if sr == 64 else (64, 96, 160)
    return sr, small + (B.dw_smallest_m(N, sr, 2, 1), B.dw_smallest_m(N, sr, 3, 1))


def run_dw(lib, jd, kernel, fam, M, N, pad, trans_c):
    from rel_pose_amd import _lib
    sr, ms = dw_ms(kernel, N)
    bf = kernel.startswith("bf16")
    nm = "dw192_%s/%s M=%d N=%d lda=N+%d trans_c=%d" % (kernel, fam, M, N, pad, trans_c)
    jd.n += 1
    a, b = B.dw_values(fam, M, N, "cuda")
    if bf:
        a = G.bf16_round(a)
        b = G.bf16_round(b)                              # on the host for a bf16 b, on chip (nearest even) for an fp32 one
    A = Padded(M, N, N + pad, BF if bf else F32, a)
    Bm = put(B.dw_values(fam, M, N, "cuda")[1], BF if kernel == "bf16" else F32)
    splits = (lib.rp_dw192_bf16_splits if bf else lib.rp_dw192_f32_splits)(M, N)
    nbytes = (lib.rp_dw192_bf16_workspace_bytes if bf else lib.rp_dw192_f32_workspace_bytes)(M, N)
    sp, per, last = B.dw_slabs(M, N, sr)
    assert splits == sp and nbytes == sp * N * B.C * 4, (nm, splits, nbytes)
    if M == ms[3]:
        assert (per, last) == (2, 1), nm
    elif M == ms[4]:
        assert (per, last) == (3, 1), nm
    else:
        assert per == 1 and sp == max(2, M // sr), nm
    ws = Out((sp, N, B.C))
    if bf:
        lib.rp_dw192_bf16(A.ptr(), A.ld, _p(Bm), int(kernel == "bf16_b32"), M, N, ws.ptr(), nbytes, _stream())
    else:
        getattr(lib, "rp_dw192_" + kernel)(A.ptr(), A.ld, _p(Bm), M, N, ws.ptr(), nbytes, _stream())
    slabs = B.dw_reference(a, b, B.dw_slab_rows(M, N, sr))
    jd.exact(nm, "slabs", ws.t, slabs.float())
    jd.guards(nm, workspace=ws)
    jd.check(nm, A.pads_untouched(), "pads of a written")
    Cm = Padded(B.C, N, N + 4, F32) if trans_c else Padded(N, B.C, B.C + 4, F32)
    task = (_lib.RpSplitkTask * 1)()
    t = task[0]
    t.ws, t.C, t.M, t.N, t.ldc, t.split_k, t.trans_c = ws.ptr(), Cm.ptr(), N, B.C, Cm.ld, sp, trans_c
    lib.rp_splitk_reduce_multi(task, 1, _stream())
    full = a.t() @ b
    jd.exact(nm, "reduced", Cm.view(), (full.t() if trans_c else full).float())
    jd.check(nm, Cm.pads_untouched(), "pads of C written")


@pytest.mark.parametrize("N", B.DW_NS)
@pytest.mark.parametrize("kernel", DW_KERNELS)
def test_dw192_cells(lib, kernel, N):
    """slabs before the reduce against the per-slab integer reference, then the reduced matrix; the slab layout read from *_splits"""
    jd = Judge("dw192_%s.N%d" % (kernel, N))
    sr, ms = dw_ms(kernel, N)
    step = 8 if sr == 64 else 4                          # lda must stay a multiple of 8 bf16 / 4 fp32 elements
    for fi, fam in enumerate(B.DW_FAMILIES):
        if fam == "sel16" and sr == 64:
            continue                                     # (a bf16-stored operand cannot hold 16 bits)
        for mi, M in enumerate(ms if fam in ("small_int", "row_coded") else (ms[0], ms[2], ms[3])):
            for pad in (0, step):
                run_dw(lib, jd, kernel, fam, M, N, pad, (fi + mi + pad // step) & 1)
    jd.done(two_stage_m=ms[3], three_stage_m=ms[4])


# ------------------------------------------------------------------------------------------------ rp_ds_matmul / rp_ds_matmul_t
DS_KEYS = [(Z, kernel) for Z in (2, 4) for kernel in ("acc", "acc_bf16", "runs")]


@pytest.mark.parametrize("Z,kernel", DS_KEYS, ids=["Z%d-%s" % k for k in DS_KEYS])
def test_ds_matmul_cells(lib, Z, kernel):
    """integer ds placed into each tile layout by a function written from the header, H = 3; Z = 2 (6 problems: two idle slots of the
    8-wide work order) and Z = 4 (12 problems: the order wraps into a second group of 8); b_xor 0 / 1, colpart on / off; the bf16 tiles
    with a 12-bit b, so the on-chip rounding of b must be nearest even"""
    H = 3
    jd = Judge("ds_matmul.%s.Z%d" % (kernel, Z))
    assert Z * H > 8 if Z == 4 else Z * H < 8
    layout, bf = ("runs" if kernel == "runs" else "acc"), kernel == "acc_bf16"
    ds = B.ds_code(Z * H).to("cuda").double()
    img = B.ds_place(ds, layout).to(BF if bf else F32).contiguous()
    for b_xor in (0, 1):
        for with_cp in (0, 1):
            nm = "ds_matmul %s Z=%d b_xor=%d colpart=%d" % (kernel, Z, b_xor, with_cp)
            jd.n += 1
            b64 = B.ds_b(Z, H, bf, Z, b_xor, with_cp).to("cuda").double()
            Bm = Padded(Z * B.NTOK, H * 64, H * 64 + 4, F32, b64.view(Z * B.NTOK, H * 64))
            out = Padded(Z * B.NTOK, H * 64, H * 64 + 4, F32)
            cp = Padded(Z * B.NTOK // B.TILE, H * 64, H * 64 + 4, F32) if with_cp else None
            if kernel == "runs":
                lib.rp_ds_matmul_t(_p(img), Bm.ptr(), out.ptr(), Z, H, Bm.ld, out.ld, b_xor, None if cp is None else cp.ptr(), H * 64 + 4, _stream())
            else:
                lib.rp_ds_matmul(_p(img), Bm.ptr(), out.ptr(), Z, H, Bm.ld, out.ld, b_xor, int(bf), None if cp is None else cp.ptr(), H * 64 + 4,
                                 _stream())
            want, wcp = B.ds_reference(ds, G.bf16_round(b64) if bf else b64, Z, H, b_xor)
            jd.exact(nm, "out", out.view(), want.float())
            jd.check(nm, out.pads_untouched() and Bm.pads_untouched(), "pads of out / b written")
            if cp is not None:
                jd.exact(nm, "colpart", cp.view(), wcp.float())
                jd.check(nm, cp.pads_untouched(), "pads of colpart written")
    jd.done()


DS_REFUSALS = [("Z=0", -1, dict(Z=0)), ("H=0", -1, dict(H=0)), ("b_xor=2", -1, dict(b_xor=2)), ("b_xor with odd Z", -1, dict(Z=3, b_xor=1)),
               ("ds null", -1, dict(ds=None)), ("ldb%4", -2, dict(ldb=194)), ("ldo%4", -2, dict(ldo=194)), ("ldp < H*64", -1, dict(cp="c", ldp=128))]


@pytest.mark.parametrize("t", (0, 1), ids=["ds_matmul", "ds_matmul_t"])
@pytest.mark.parametrize("name,code,kw", DS_REFUSALS, ids=[re.sub(r"\W+", "_", r[0]) for r in DS_REFUSALS])
def test_ds_matmul_refusals(lib, rbufs, t, name, code, kw):
    a = dict(ds="a", Z=2, H=3, ldb=192, ldo=192, b_xor=0, cp=None, ldp=192)
    a.update(kw)
    ptr = lambda k: None if k is None else rbufs[k].data_ptr()
    if t:
        call = lambda: lib.rp_ds_matmul_t(ptr(a["ds"]), ptr("b"), ptr("out"), a["Z"], a["H"], a["ldb"], a["ldo"], a["b_xor"], ptr(a["cp"]), a["ldp"], _stream())
    else:
        call = lambda: lib.rp_ds_matmul(ptr(a["ds"]), ptr("b"), ptr("out"), a["Z"], a["H"], a["ldb"], a["ldo"], a["b_xor"], 0, ptr(a["cp"]), a["ldp"], _stream())
    _refused(call, code)
    torch.cuda.synchronize()
    assert bool(rbufs["out"].isnan().all()), name + ": an output was written by a refused call"


# ------------------------------------------------------------------------------------------------ refusals
EBADSHAPE, EALIGN, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4


def _refused(call, code):
    with pytest.raises(RuntimeError) as e:
        call()
    m = re.search(r"RP error (-?\d+)", str(e.value))
    assert m and int(m.group(1)) == code, str(e.value)


@pytest.fixture(scope="module")
def rbufs(lib):
    b = {k: torch.zeros(1 << 18, device="cuda") for k in ("a", "b", "c", "d", "e", "f", "g")}
    b["out"] = torch.full((1 << 18,), NAN, device="cuda")
    return b


def _refusal_rows():
    rows = []
    lin = dict(x="a", w="b", bias=None, res=None, gamma=None, beta=None, y="out", pre=None, xn=None, mean=None, rstd=None, aux=None,
               cs=None, M=65, N=192, K=192, act=0, prec=0, io=0)
    for name, code, kw in (("M=0", EBADSHAPE, dict(M=0)), ("K!=192", EBADSHAPE, dict(K=160)), ("N%32", EBADSHAPE, dict(N=200)),
                           ("N>1024", EBADSHAPE, dict(N=1056)), ("act=2", EBADSHAPE, dict(act=2)), ("x null", EBADSHAPE, dict(x=None)),
                           ("gamma without beta", EBADSHAPE, dict(gamma="c")), ("xn_out without LayerNorm", EBADSHAPE, dict(xn="out")),
                           ("precision 2", EUNSUPPORTED, dict(prec=2)), ("io at precision 0", EUNSUPPORTED, dict(io=2)),
                           ("unknown io bit", EUNSUPPORTED, dict(prec=1, io=16)), ("bf16 aux without aux", EUNSUPPORTED, dict(prec=1, io=4)),
                           ("bf16 x with LayerNorm", EUNSUPPORTED, dict(prec=1, io=1, gamma="c", beta="d")),
                           ("bf16 xn without xn_out", EUNSUPPORTED, dict(prec=1, io=8, gamma="c", beta="d"))):
        rows.append(("linear_rows192 " + name, "linear", code, dict(lin, **kw)))
    for k in ("f32", "split3", "bf16"):
        dw = dict(kernel=k, a="a", lda=192, b="b", M=128, N=192, ws="out", nbytes=None)
        for name, code, kw in (("a null", EBADSHAPE, dict(a=None)), ("M=0", EBADSHAPE, dict(M=0)), ("N%192", EBADSHAPE, dict(N=200, lda=200)),
                               ("M%stage", EBADSHAPE, dict(M=144)), ("lda<N", EBADSHAPE, dict(lda=184)), ("lda misaligned", EBADSHAPE, dict(lda=194)),
                               ("a misaligned", EALIGN, dict(a=("a", 4))), ("workspace misaligned", EALIGN, dict(ws=("out", 4))),
                               ("short workspace", EWORKSPACE, dict(nbytes=-4))):
            rows.append(("dw192_%s %s" % (k, name), "dw", code, dict(dw, **kw)))
        if k != "bf16":
            rows.append(("dw192_%s M<64" % k, "dw", EBADSHAPE, dict(dw, M=32)))
    fwd = dict(M=65, dim=192, hidden=768, train=0, prec=0, io=0, ws="g")
    for name, code, kw in (("M=0", EBADSHAPE, dict(M=0)), ("dim", EBADSHAPE, dict(dim=128)), ("hidden", EBADSHAPE, dict(hidden=384)),
                           ("no workspace", EBADSHAPE, dict(ws=None)), ("half a training set", EBADSHAPE, dict(train=1)),
                           ("precision 2", EUNSUPPORTED, dict(prec=2)), ("io at precision 0", EUNSUPPORTED, dict(io=16)),
                           ("training bits on the inference form", EUNSUPPORTED, dict(prec=1, io=2)),
                           ("unknown io bit", EUNSUPPORTED, dict(prec=1, train=2, io=1))):
        rows.append(("mlp_fused_fwd " + name, "fwd", code, dict(fwd, **kw)))
    bwd = dict(M=65, dim=192, hidden=768, prec=0, io=0, ws="g", ln=0, dx="out")
    for ln in (0, 1):
        for name, code, kw in (("M=0", EBADSHAPE, dict(M=0)), ("dim", EBADSHAPE, dict(dim=128)), ("no workspace", EBADSHAPE, dict(ws=None)),
                               ("precision 2", EUNSUPPORTED, dict(prec=2)), ("io at precision 0", EUNSUPPORTED, dict(io=2)),
                               ("unknown io bit", EUNSUPPORTED, dict(prec=1, io=8))):
            rows.append(("mlp_fused_bwd%s %s" % ("_ln" if ln else "", name), "bwd", code, dict(bwd, ln=ln, **kw)))
    rows.append(("mlp_fused_bwd_ln dx aliases dy", "bwd", EBADSHAPE, dict(bwd, ln=1, dx="a")))
    rows.append(("mlp_fused_bwd_ln without ln_x", "bwd", EBADSHAPE, dict(bwd, ln=2)))
    return rows


REFUSALS = _refusal_rows()


@pytest.mark.parametrize("name,kind,code,kw", REFUSALS, ids=[re.sub(r"\W+", "_", r[0]) for r in REFUSALS])
def test_refusals(lib, rbufs, name, kind, code, kw):
    """one call per `return RP_E*` condition of these entry points: host side only, the documented status, the NaN output untouched"""
    def ptr(v):
        if v is None:
            return None
        return rbufs[v].data_ptr() if isinstance(v, str) else rbufs[v[0]].data_ptr() + v[1]
    st = _stream()
    if kind == "linear":
        call = lambda: lib.rp_linear_rows192(ptr(kw["x"]), ptr(kw["w"]), ptr(kw["bias"]), ptr(kw["res"]), ptr(kw["gamma"]), ptr(kw["beta"]), EPS,
                                             ptr(kw["y"]), ptr(kw["pre"]), ptr(kw["xn"]), ptr(kw["mean"]), ptr(kw["rstd"]), ptr(kw["aux"]),
                                             ptr(kw["cs"]), kw["M"], kw["N"], kw["K"], kw["act"], kw["prec"], kw["io"], st)
    elif kind == "dw":
        k = kw["kernel"]
        need = (lib.rp_dw192_bf16_workspace_bytes if k == "bf16" else lib.rp_dw192_f32_workspace_bytes)(kw["M"], kw["N"])
        nbytes = (1 << 20) if kw["nbytes"] is None else need + kw["nbytes"]
        if k == "bf16":
            call = lambda: lib.rp_dw192_bf16(ptr(kw["a"]), kw["lda"], ptr(kw["b"]), 0, kw["M"], kw["N"], ptr(kw["ws"]), nbytes, st)
        else:
            call = lambda: getattr(lib, "rp_dw192_" + k)(ptr(kw["a"]), kw["lda"], ptr(kw["b"]), kw["M"], kw["N"], ptr(kw["ws"]), nbytes, st)
    elif kind == "fwd":
        tr = [ptr("out")] * 5 if kw["train"] == 2 else ([ptr("out"), None, None, None, None] if kw["train"] else [None] * 5)
        call = lambda: lib.rp_mlp_fused_fwd(ptr("a"), ptr("b"), ptr("c"), ptr("d"), ptr("e"), ptr("f"), ptr("b"), ptr("out"), ptr(kw["ws"]),
                                            kw["M"], kw["dim"], kw["hidden"], EPS, *tr, kw["prec"], kw["io"], st)
    else:
        head = (ptr("a"), ptr("b"), ptr("c"), ptr("d"), ptr("out"), ptr(kw["dx"]), ptr("out"), ptr(kw["ws"]), kw["M"], kw["dim"],
                kw["hidden"], kw["prec"], kw["io"])
        if kw["ln"]:
            call = lambda: lib.rp_mlp_fused_bwd_ln(*head, ptr("e") if kw["ln"] == 1 else None, ptr("f"), ptr("f"), ptr("f"), ptr("out"), st)
        else:
            call = lambda: lib.rp_mlp_fused_bwd(*head, st)
    _refused(call, code)
    torch.cuda.synchronize()
    assert bool(rbufs["out"].isnan().all()), name + ": an output was written by a refused call"


def test_grid_queries_refuse_what_the_launch_refuses(lib):
    assert lib.rp_linear_rows192_grid(0, 192, 0, 0) == 0 and lib.rp_linear_rows192_grid(65, 200, 0, 0) == 0
    assert lib.rp_linear_rows192_grid(65, 1056, 0, 0) == 0 and lib.rp_linear_rows192_grid(65, 192, 0, 2) == 0
    assert lib.rp_mlp_fused_grid(0, 0, 0, 0) == 0 and lib.rp_mlp_fused_grid(65, 1, 0, 2) == 0
    assert lib.rp_linear_rows192_grid(1, 32, 0, 0) == 1 and lib.rp_mlp_fused_grid(1, 0, 0, 0) == 24
