"""The attention and Essential-Matrix-Module kernels (csrc/attention.hip, csrc/emm.hip; exact-fp32 configuration) where the softmax is
peaked, flat, climbing or large, judged per 32-row block / per head against fp64 -- inputs, references, metrics and the bound rule:
tests/_softmax_regimes.py; the conditions of the inputs are proved on the CPU by tests/test_softmax_regimes_cpu.py.

Every launch form is reached BY SIZE, never through the RP_ATTN_* overrides: Z = 2 (Z H = 6: one partial XCD group, one-wave workgroups) and
Z = 20 (Z H = 60: a ragged last group and the smallest even Z at which the launchers take the two-wave workgroups, Z H 9 > 512).
Each asserted error is at most 8 x the error plain fp32 PyTorch makes on the same input under the same metric (lse: with a floor of 4 ulps;
in the CARRIED regimes the outputs that carry the fp32 log-sum-exp's rounding have the derived allowance of tests/_softmax_regimes.py on
top); every measured error, the yardstick's, their ratio and the tensor-wide metric of the same tensors go to the test report
(tests/test_gpu_kernels.py: report()), one line per case.

Hand check of the metrics (not committed): delta of ONE 32-row block of the last (image, head) times 1.01 in attn_bwd_dq_kernel fails all 18
recompute and cross cases (1e-3 .. 6e-2 per head against bounds of 8e-6 .. 2e-4); in `large8` / `large40` the tensor-wide metric of the same
tensors reads 4.4e-5 .. 5.0e-5 where the per-head one reads 1.1e-3 -- a 0.3 % error there is under the 2e-5 of test_attention_fwd_bwd and
three times over the bound here."""
import math

import pytest
import torch

from tests import _softmax_regimes as R
from tests.test_gpu_kernels import report

pytestmark = pytest.mark.gpu

ZS = [2, 20]
LOG2E = math.log2(math.e)
_CACHE = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, ops as o
    _lib.load()
    assert not o.ATTN_BF16 and o.GEMM_PRECISION == 0, "exact-fp32 configuration only"
    yield o
    _CACHE.clear()


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def case(name, Z, pairing):
    """the regime's input on the GPU: (qkv, perm or None)"""
    def make():
        qkv, perm = R.build(name, Z, pairing)
        return qkv.cuda(), None if perm is None else perm.cuda()
    return cached(("in", name, Z, pairing), make)


def pos_of(Z):
    return cached(("pos", Z), lambda: R.make_pos(Z).cuda())


def finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts if t is not None)


class Checks:
    """collects errors against bound(yardstick) and reports all of them before it asserts.  add(): a scalar (error, where) of a metric;
    cells(): (error, reference maximum) per cell of a metric, with an optional absolute allowance per cell on top of the 8 x rule (the
    carried normaliser of tests/_softmax_regimes.py, in its CARRIED regimes only)"""

    def __init__(self, name):
        self.name, self.kv, self.failed = name, {}, []

    def add(self, what, err_where, yard, floor=0.0):
        err, where = err_where
        limit = R.bound(yard, floor)
        self.kv[what], self.kv[what + "_fp32"], self.kv[what + "_ratio"] = err, yard, err / max(yard, 1e-30)
        if not err <= limit:
            self.failed.append("%s: %.3e at %s > %.3e (plain fp32: %.3e)" % (what, err, where, limit, yard))

    def cells(self, what, kind, got, want, yard, allow=None, ref_max=None):
        """kind: "block" | "head" | "global".  allow: an absolute allowance per ELEMENT of `want` on top of the 8 x rule -- every element
        is then held to 8 x yardstick x (its cell's largest reference value) + its own allowance.  ref_max: the cells' reference maxima
        where they are not `want`'s own"""
        err_c, ref_c = R.CELLS[kind](got, want)
        ref_c = ref_c if ref_max is None else ref_max
        err, where = R.worst((err_c, ref_c))
        self.kv[what], self.kv[what + "_fp32"], self.kv[what + "_ratio"] = err, yard, err / max(yard, 1e-30)
        if kind != "global":
            self.kv[what + "_global"] = R.rel(got, want)                      # what the tensor-wide metric makes of the same tensors
        if allow is None:
            if not bool((err_c <= R.bound(yard) * ref_c).all()):
                self.failed.append("%s: %.3e at %s > %.3e (plain fp32: %.3e)" % (what, err, where, R.bound(yard), yard))
            return
        want = want.detach().double()
        diff = (got.detach().double() - want).abs()
        limit = R.bound(yard) * R.spread(ref_c, want, kind) + allow
        of = float((diff / limit.clamp_min(1e-300)).max())
        self.kv[what + "_of_limit"] = of
        if not of <= 1.0:
            self.failed.append("%s: %.2f x its limit; worst cell %.3e at %s (plain fp32: %.3e)" % (what, of, err, where, yard))

    def done(self):
        report(self.name, **self.kv)
        assert not self.failed, self.name + " -- " + "; ".join(self.failed)


def partials_are_block_sums(part, d, Z):
    """[Z*18, C] fp32 column sums per 32-row block of the returned gradient d [Z*576, C]: an fp32 sum of 32 stored values in any order is
    within 31 eps32 sum |x| of the exact sum"""
    blocks = d.double().view(Z * 18, 32, -1)
    slack = 32 * R.EPS32 * blocks.abs().sum(1) + 1e-30
    return bool(((part.double() - blocks.sum(1)).abs() <= slack).all())


# ------------------------------------------------------------------------------------------------ attention: references
def attn_reference(name, Z, kv_xor):
    """fp64 (o, lse), the yardstick's errors and -- CARRIED regimes -- the allowances, once per (regime, Z)"""
    def make():
        qkv, _ = case(name, Z, "cross" if kv_xor else "self")
        o, lse, _ = R.attn_ref(qkv, Z, kv_xor)
        o32, lse32, _ = R.attn_ref(qkv, Z, kv_xor, dtype=torch.float32)
        ref = dict(o=R.heads_of(o, Z), lse=lse, y_o=R.block_rel(R.heads_of(o32, Z), R.heads_of(o, Z))[0], y_lse=R.lse_err(lse32, lse)[0],
                   do=R.cotangent((Z * R.N_TOK, R.HEADS * R.HD), seed=2).cuda(), allow_p=None, allow_dv=None)
        if name in R.CARRIED:
            # (o, dq and dk meet the plain rule in these regimes too and keep it)
            eps, P, sdv = R.attn_sensitivity(qkv, ref["do"], Z, kv_xor)
            ref.update(allow_p=eps[..., None, None] * P, allow_dv=eps[..., None, None] * sdv)
        return ref
    return cached(("attn", name, Z, kv_xor), make)


def attn_gradients(name, Z, kv_xor):
    def make():
        qkv, _ = case(name, Z, "cross" if kv_xor else "self")
        ref = attn_reference(name, Z, kv_xor)
        fn = lambda x: R.attn_ref(x, Z, kv_xor, dtype=x.dtype)[0]
        g64, g32 = R.grads(fn, qkv, ref["do"], Z, torch.float64), R.grads(fn, qkv, ref["do"], Z, torch.float32)
        return dict(do=ref["do"], g=g64, y=[R.head_rel(a, b)[0] for a, b in zip(g32, g64)], y_rel=[R.rel(a, b) for a, b in zip(g32, g64)],
                    allow=[None, None, ref["allow_dv"]])
    return cached(("attn_grad", name, Z, kv_xor), make)


def check_gradients(ck, dqkv, ref, Z, global_metric):
    """dq, dk, dv of dqkv [Z*576, 576] against fp64 per (image, head); `onehot` (its gradients cancel to nothing, plain fp32 itself is wrong
    by 2e-3 .. 4e-3 per head) under the global metric"""
    assert finite(dqkv)
    for i, (what, got) in enumerate(zip(("dq", "dk", "dv"), R.split_grad(dqkv, Z))):
        allow = ref["allow"][i]
        if global_metric:
            ck.cells(what, "global", got, ref["g"][i], ref["y_rel"][i], allow)
        else:
            assert ref["y"][i] <= R.GRAD_YARDSTICK_CAP                       # the condition on the input (tests/test_softmax_regimes_cpu.py)
            ck.cells(what, "head", got, ref["g"][i], ref["y"][i], allow)


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("Z", ZS)
@pytest.mark.parametrize("name", R.FORWARD_SELF)
def test_attention_forward(ops, name, Z):
    """rp_attn_fwd, one-wave (Z = 2) and two-wave (Z = 20) workgroups: o per 32-row block, lse per row; `onehot`: o[i] is v[pi(i)] to what
    the fp64 softmax leaves of the other rows; `flat`: lse = ln 576 and o = the column mean of v.
    measured (MI355X, error / plain fp32's): at most 2.6 x (o, `onehot`, Z = 2)."""
    qkv, perm = case(name, Z, "self")
    ref = attn_reference(name, Z, 0)
    o, lse = ops.attn_fwd(qkv, Z)
    assert finite(o, lse)
    oh = R.heads_of(o, Z)
    ck = Checks("regimes.attn_fwd[%s,Z=%d]" % (name, Z))
    ck.cells("o", "block", oh, ref["o"], ref["y_o"])
    ck.add("lse", R.lse_err(lse, ref["lse"]), ref["y_lse"], R.LSE_FLOOR)
    v = R.split(qkv, Z)[2].double()
    if name == "onehot":
        # |o - v_pi| <= |o - o64| + |o64 - v_pi| for every element: o's own limit (on max |o64| of the block) plus what the fp64 softmax leaves
        vpi = v.gather(2, perm[..., None].expand(-1, -1, -1, R.HD))
        ck.cells("o_vs_v_pi", "block", oh, vpi, ref["y_o"], (ref["o"] - vpi).abs(), ref_max=R.block_max(ref["o"]))
    if name == "flat":
        mean = v.mean(2, keepdim=True).expand(-1, -1, R.N_TOK, -1)
        for sel in ((slice(0, 1), slice(None)), (slice(1, 2), slice(1, 2))):          # image 0: q = 0; image 1, head 1: k = 0
            ck.add("flat_o%d" % sel[0].start, R.block_rel(oh[sel], mean[sel]), ref["y_o"])
            ck.add("flat_lse%d" % sel[0].start, R.lse_err(lse[sel], torch.full_like(ref["lse"][sel], R.LN_NTOK)), ref["y_lse"], R.LSE_FLOOR)
    ck.done()


@pytest.mark.parametrize("Z", ZS)
@pytest.mark.parametrize("name", ["onehot", "staircase_keys_up", "staircase_keys_down", "large40", "flat"])
def test_attention_stored_p(ops, name, Z):
    """rp_attn_fwd_savep: o / lse bit-identical to rp_attn_fwd, every stored value finite and in [0, 1], and pst exp2(mrun - lse2) -- the
    factor the stored-P backward applies -- is the fp64 probability per 32-row block (the running maximum the tiles are relative to moves
    at every tile in `staircase` up, never in down).
    measured: 6.8 x (`staircase` down, Z = 20); `onehot` 7.8 x and `large40` 8.05 x -- the carried normaliser, 0.34 of their limit."""
    qkv, _ = case(name, Z, "self")
    o0, lse0 = ops.attn_fwd(qkv, Z)
    o, lse, pst, mrun = ops.attn_fwd(qkv, Z, save_p=True)
    assert torch.equal(o, o0) and torch.equal(lse, lse0)
    assert finite(pst, mrun) and float(pst.min()) >= 0.0 and float(pst.max()) <= 1.0
    _, lse64, s64 = R.attn_ref(qkv, Z)
    p64 = torch.exp(s64 - lse64[..., None])
    y_p = R.block_rel(torch.softmax(s64.float(), -1), p64)[0]
    del s64
    # tile (query block qb, key tile t), element (i, j) at float ((j >> 2) * 32 + i) * 4 + (j & 3); mrun [Z,H,18 key tiles,576 queries], log2 units
    fac = torch.exp2(mrun.double() - lse.double().view(Z, R.HEADS, 1, R.N_TOK) * LOG2E)
    got = pst.view(Z, R.HEADS, 18, 18, 8, 32, 4).permute(0, 1, 2, 5, 3, 4, 6).reshape(Z, R.HEADS, R.N_TOK, R.N_TOK).double()
    got *= fac.permute(0, 1, 3, 2).repeat_interleave(32, dim=3)
    ck = Checks("regimes.attn_fwd_savep[%s,Z=%d]" % (name, Z))
    ck.cells("p", "block", got, p64, y_p, attn_reference(name, Z, 0)["allow_p"])
    ck.done()


@pytest.mark.parametrize("Z", ZS)
@pytest.mark.parametrize("form", ["stored_ds", "recompute", "stored_p"])
@pytest.mark.parametrize("name", R.GRADIENT_SELF + ("onehot",))
def test_attention_backward(ops, name, form, Z):
    """rp_attn_bwd_dkdv_ds + rp_ds_matmul (stored_ds), rp_attn_bwd (recompute: at Z = 20 the two-wave recompute kernels) and
    rp_attn_bwd_dkdv_p + rp_ds_matmul_t (stored_p) against fp64 autograd per (image, head); the bias partials are the 32-row block sums
    of the returned gradient.
    measured: 4.8 x (dq, `staircase`, stored_ds, Z = 20); dv of `onehot` 10.7 x under the global metric -- the carried normaliser, 0.39 of its limit."""
    qkv, _ = case(name, Z, "self")
    ref = attn_gradients(name, Z, 0)
    saved = None
    if form == "stored_p":
        o, lse, pst, mrun = ops.attn_fwd(qkv, Z, save_p=True)
        saved = (pst, mrun)
    else:
        o, lse = ops.attn_fwd(qkv, Z)
    keep, ops.ATTN_BWD_STORE_DS = ops.ATTN_BWD_STORE_DS, form != "recompute"
    try:
        dqkv, part = ops.attn_bwd(qkv, o, lse, ref["do"], Z, want_bias_partials=True, saved_p=saved)
    finally:
        ops.ATTN_BWD_STORE_DS = keep
    ck = Checks("regimes.attn_bwd[%s,%s,Z=%d]" % (name, form, Z))
    check_gradients(ck, dqkv, ref, Z, name == "onehot")
    if form == "recompute":
        assert part is None
    else:
        assert part.shape == (Z * 18, 576) and finite(part) and partials_are_block_sums(part, dqkv, Z)
    ck.done()


@pytest.mark.parametrize("Z", ZS)
@pytest.mark.parametrize("name", ["diffuse", "sharp"])
def test_cross_attention_against_its_own_reference(ops, name, Z):
    """rp_attn_fwd(k_xor = 3) and rp_attn_bwd_cross(kv_xor = 1) (at Z = 20 the two-wave cross backward) against fp64 attention on the
    partner image's keys and values written directly (vision_transformer.py:239-262), `sharp` planted across the pair.
    measured: 3.2 x (dk, `sharp`, Z = 20)."""
    qkv, _ = case(name, Z, "cross")
    ref, gref = attn_reference(name, Z, 1), attn_gradients(name, Z, 1)
    o, lse = ops.attn_fwd(qkv, Z, k_xor=3)
    assert finite(o, lse)
    ck = Checks("regimes.attn_cross[%s,Z=%d]" % (name, Z))
    ck.cells("o", "block", R.heads_of(o, Z), ref["o"], ref["y_o"])
    ck.add("lse", R.lse_err(lse, ref["lse"]), ref["y_lse"], R.LSE_FLOOR)
    check_gradients(ck, ops.attn_bwd(qkv, o, lse, gref["do"], Z, kv_xor=1), gref, Z, False)
    ck.done()


# ------------------------------------------------------------------------------------------------ EMM: references
VARIANTS = {"default": (False, False), "single": (True, False), "cross": (False, True)}


def emm_reference(name, Z, variant):
    def make():
        qkv, _ = case(name, Z, "cross")
        single, cross = VARIANTS[variant]
        F, T, U, X, A = R.emm_ref(qkv, pos_of(Z), Z, single, cross)
        y = R.emm_ref(qkv, pos_of(Z), Z, single, cross, dtype=torch.float32)
        ref = dict(F=F, T=T, U=U, X=X, amax=A.amax(-1), y_F=R.head_rel(y[0], F)[0], y_T=R.block_rel(y[1], T)[0], y_U=R.block_rel(y[2], U)[0],
                   allow_T=None, allow_U=None, allow_F=None)
        if name in R.CARRIED:
            sens = R.emm_sensitivity(qkv, pos_of(Z), None, Z, single, cross)
            ref.update(allow_T=sens["T"], allow_U=sens["U"], allow_F=sens["F"])
        return ref
    return cached(("emm", name, Z, variant), make)


def emm_gradients(name, Z, variant):
    def make():
        qkv, _ = case(name, Z, "cross")
        single, cross = VARIANTS[variant]
        cot = R.cotangent((Z, R.HEADS, 70, 70), seed=6).cuda()
        fn = lambda x: R.emm_ref(x, pos_of(Z), Z, single, cross, dtype=x.dtype)[0]
        g64, g32 = R.grads(fn, qkv, cot, Z, torch.float64), R.grads(fn, qkv, cot, Z, torch.float32)
        dF = torch.zeros(Z, R.HEADS, 96, 96, device="cuda")
        dF[..., :70, :70] = cot
        ref = dict(dF=dF, g=g64, y=[R.head_rel(a, b)[0] for a, b in zip(g32, g64)], y_rel=[R.rel(a, b) for a, b in zip(g32, g64)])
        for recomputed in (False, True):
            ref["allow", recomputed] = [None] * 3
            if name in R.CARRIED:
                sens = R.emm_sensitivity(qkv, pos_of(Z), cot, Z, single, cross, recomputed)
                ref["allow", recomputed] = [sens[k] for k in ("dq", "dk", "dv")]
        return ref
    return cached(("emm_grad", name, Z, variant), make)


def detile(sc, Z):
    """stored score / probability tiles [Z,H,18,18,1024] -> [Z,H,576,576]: tile (query block, key tile), element (i, j) at float
    ((j >> 2) * 32 + i) * 4 + (j & 3)"""
    return sc.view(Z, R.HEADS, 18, 18, 8, 32, 4).permute(0, 1, 2, 5, 3, 4, 6).reshape(Z, R.HEADS, R.N_TOK, R.N_TOK)


# ------------------------------------------------------------------------------------------------ EMM
@pytest.mark.parametrize("Z", ZS)
@pytest.mark.parametrize("name", R.FORWARD_CROSS)
def test_emm_statistics(ops, name, Z):
    """rp_emm_stats (one pass: rows online, columns from the 18 per-block partials -- `staircase` on the query axis moves every column's
    maximum from block to block), the two statistics-only passes it replaces, the single-softmax form and the stored score tiles (log2
    units): rlse / clse per row against fp64, the tiles per 32-row block; the statistics are bit-identical with and without the store.
    measured: 1.5 x at most (clse, `large40`), the stored tiles included."""
    qkv, _ = case(name, Z, "cross")
    r64, c64, s64 = R.emm_stats_ref(qkv, Z)
    s32 = R.scores(qkv, Z, "cross")
    y_r, y_c = R.lse_err(torch.logsumexp(s32, -1), r64)[0], R.lse_err(torch.logsumexp(s32, -2), c64)[0]
    y_s = R.block_rel(s32 * torch.tensor(LOG2E, dtype=torch.float32), s64 * LOG2E)[0]
    rlse, clse = ops.emm_stats(qkv, Z)
    r_s, c_s, sc = ops.emm_stats(qkv, Z, want_s=True)
    assert sc is not None and torch.equal(rlse, r_s) and torch.equal(clse, c_s)
    keep, ops.EMM_STATS_ONE_PASS = ops.EMM_STATS_ONE_PASS, False
    try:
        r2, c2 = ops.emm_stats(qkv, Z)
    finally:
        ops.EMM_STATS_ONE_PASS = keep
    r1, c1 = ops.emm_stats(qkv, Z, single=True)
    assert ops.EMM_STATS_ONE_PASS and c1 is r1 and finite(rlse, clse, r2, c2, r1, sc)
    ck = Checks("regimes.emm_stats[%s,Z=%d]" % (name, Z))
    for what, got, want, y in (("rlse", rlse, r64, y_r), ("clse", clse, c64, y_c), ("rlse_two_pass", r2, r64, y_r), ("clse_two_pass", c2, c64, y_c),
                               ("rlse_single", r1, r64, y_r)):
        ck.add(what, R.lse_err(got, want), y, R.LSE_FLOOR)
    ck.add("s", R.block_rel(detile(sc, Z), s64 * LOG2E), y_s)
    ck.done()


@pytest.mark.parametrize("Z", ZS)
@pytest.mark.parametrize("name", R.FORWARD_CROSS)
def test_emm_apply(ops, name, Z):
    """rp_emm_apply, recompute and stored-S, forward and swap, the single-softmax form (recompute: emm_stats(single=True) stores no tiles)
    and the cross-features F: T and U (columns :70) per 32-row block, F per head, the padding columns exactly zero; `onehot`: T[i] is
    A[i, pi(i)] X[pi(i)] to what the fp64 A leaves of the other entries.
    measured: 3.6 x outside the CARRIED regimes (F, single softmax, `flat`); in them U 10.5 x (`large40`) and 9.6 x (`onehot`, single) -- 0.42 of their limit."""
    qkv, perm = case(name, Z, "cross")
    ref = emm_reference(name, Z, "default")
    rlse, clse, sc = ops.emm_stats(qkv, Z, want_s=True)
    xa = ops.emm_build_x(qkv, pos_of(Z), Z)
    assert torch.equal(xa[..., :70].double(), ref["X"]) and float(xa[..., 70:].abs().max()) == 0.0
    ck = Checks("regimes.emm_apply[%s,Z=%d]" % (name, Z))

    def check(tag, t, u, fpart, rf):
        assert finite(t, u, fpart)
        ck.cells("T" + tag, "block", t[..., :70], rf["T"], rf["y_T"], rf["allow_T"])
        assert float(t[..., 70:].abs().max()) == 0.0
        if u is not None:
            ck.cells("U" + tag, "block", u[..., :70], rf["U"], rf["y_U"], rf["allow_U"])
            assert float(u[..., 70:].abs().max()) == 0.0
        F = fpart.double().sum(2)
        ck.cells("F" + tag, "head", F[..., :70, :70], rf["F"], rf["y_F"], rf["allow_F"])
        assert float(F[..., 70:, :].abs().max()) == 0.0 and float(F[..., :, 70:].abs().max()) == 0.0

    t, fpart = ops.emm_apply(qkv, xa, rlse, clse, Z)
    u, _ = ops.emm_apply(qkv, xa, rlse, clse, Z, swap=True, want_f=False)
    check("", t, u, fpart, ref)
    ts, fs = ops.emm_apply(qkv, xa, rlse, clse, Z, s=sc)
    us, _ = ops.emm_apply(qkv, xa, rlse, clse, Z, swap=True, want_f=False, s=sc)
    check("_stored_s", ts, us, fs, ref)
    r1, _ = ops.emm_stats(qkv, Z, single=True)
    t1, f1 = ops.emm_apply(qkv, xa, r1, r1, Z, single=True)
    u1, _ = ops.emm_apply(qkv, xa, r1, r1, Z, swap=True, want_f=False, single=True)
    check("_single", t1, u1, f1, emm_reference(name, Z, "single"))
    tx, fx = ops.emm_apply(qkv, xa, rlse, clse, Z, x_left=xa, s=sc)                      # cross features: F = X[z^1]^T A X, T unchanged
    check("_cross", tx, None, fx, emm_reference(name, Z, "cross"))
    if name == "onehot":
        # |T - a x_pi| <= |T - T64| + |T64 - a x_pi| for every element, as for o in test_attention_forward
        want = ref["amax"][..., None] * ref["X"].gather(2, perm[..., None].expand(-1, -1, -1, 70))
        for tag, got in (("", t), ("_stored_s", ts)):
            ck.cells("T_vs_x_pi" + tag, "block", got[..., :70], want, ref["y_T"], ref["allow_T"] + (ref["T"] - want).abs(), ref_max=R.block_max(ref["T"]))
    ck.done()


# (form, variant): stored dS with the forward's stored S / stored dS, S recomputed / rp_emm_grad for both sides.  emm_stats(single=True) stores
# no score tiles, so the single softmax has no stored-S form.
BACKWARD_FORMS = [(f, v) for f in ("stored_ds_s", "stored_ds", "recompute") for v in VARIANTS if (f, v) != ("stored_ds_s", "single")]
BACKWARD_CASES = [(f, v, 2) for f, v in BACKWARD_FORMS] + [("stored_ds_s", "default", 20), ("stored_ds", "single", 20), ("stored_ds_s", "cross", 20)]


@pytest.mark.parametrize("form,variant,Z", BACKWARD_CASES)
@pytest.mark.parametrize("name", R.GRADIENT_CROSS + ("onehot",))
def test_emm_backward(ops, name, form, variant, Z):
    """ops.emm_backward -- rp_emm_grad_ds + rp_ds_matmul_t (stored S) / rp_ds_matmul, or rp_emm_grad for the query and the key side
    (EMM_BWD_STORE_DS = False) -- default, single softmax and cross features, against fp64 autograd of F per (image, head); the full matrix
    at Z = 2, the form the model runs of each variant at Z = 20; deterministic from call to call.
    measured: 5.4 x outside the CARRIED regimes (dq, `staircase`, single, Z = 20); in them up to 121 x (`large40`, recomputed scores; 33 x with the stored
    scores, 11 x in `large8`, 23 x for the single softmax in `onehot` under the global metric) -- 0.17 of their limit at most."""
    qkv, _ = case(name, Z, "cross")
    single, cross = VARIANTS[variant]
    ref = emm_gradients(name, Z, variant)
    rlse, clse, sc = ops.emm_stats(qkv, Z, single, want_s=True)
    assert (sc is None) == single
    if form != "stored_ds_s":
        sc = None
    xa = ops.emm_build_x(qkv, pos_of(Z), Z)
    t, _ = ops.emm_apply(qkv, xa, rlse, clse, Z, single=single, x_left=xa if cross else None, s=sc)
    keep, ops.EMM_BWD_STORE_DS = ops.EMM_BWD_STORE_DS, form != "recompute"
    try:
        dqkv = ops.emm_backward(qkv, xa, t, rlse, clse, ref["dF"], Z, single=single, cross=cross, s=sc)
        again = ops.emm_backward(qkv, xa, t, rlse, clse, ref["dF"], Z, single=single, cross=cross, s=sc)
    finally:
        ops.EMM_BWD_STORE_DS = keep
    ck = Checks("regimes.emm_bwd[%s,%s,%s,Z=%d]" % (name, form, variant, Z))
    check_gradients(ck, dqkv, dict(ref, allow=ref["allow", form != "stored_ds_s"]), Z, name == "onehot")
    assert torch.equal(dqkv, again)
    ck.done()
