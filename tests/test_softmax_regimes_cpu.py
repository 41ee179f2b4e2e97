"""The softmax regimes of tests/_softmax_regimes.py without a GPU, at Z = 2: every builder produces the condition it is named for, the fp64
references are finite there, the metrics localise, and -- the condition on the INPUTS that makes a gradient case of
tests/test_gpu_softmax_regimes.py meaningful -- plain fp32 autograd is within GRAD_YARDSTICK_CAP = 2e-4 of fp64 per (image, head) in every
regime used for gradients.  (A regime that broke the cap would have its constant changed, not the cap.)

Measured (plain fp32 against fp64 on the CPU, Z = 2; `pytest -s` prints every figure): `sharp` median top probability 0.988, 5 % quantile
0.817; `onehot` minimum 0.997; `staircase` up 13 .. 14 increases at least, 99.3 .. 99.5 % of lines with >= 15; max |s| 777 (self) / 919 (cross)
in `large40`; attention o <= 3.7e-5 per block (`large40`; 1.4e-6 diffuse, 1.1e-5 staircase), T / U <= 3.1e-5, F <= 2.3e-5; gradients per head:
attention <= 2.5e-5, EMM <= 4.6e-5 (`large40`, single softmax; 4.0e-5 `sharp` with cross features) -- a quarter of the cap."""
import math

import pytest
import torch

from tests import _softmax_regimes as R

Z = 2


@pytest.fixture(scope="module")
def pos():
    return R.make_pos(Z)


def _score(name, pairing):
    qkv, perm = R.build(name, Z, pairing)
    return qkv, perm, R.scores(qkv.double(), Z, pairing)


@pytest.mark.parametrize("pairing", ["self", "cross"])
def test_sharp_and_onehot_put_the_mass_on_the_planted_entry(pairing):
    for name in ("sharp", "onehot"):
        qkv, perm, s = _score(name, pairing)
        rows, cols = R.top_probabilities(s)
        assert torch.equal(s.argmax(-1), perm), name                    # the planted key is the row's maximum ...
        assert torch.equal(s.argmax(-2).gather(-1, perm), torch.arange(R.N_TOK).expand(Z, R.HEADS, R.N_TOK)), name      # ... and the column's
        for side, p in (("rows", rows), ("columns", cols)):
            med, q05, lo = float(p.median()), float(p.flatten().quantile(0.05)), float(p.min())
            print("%s %s %s: median %.4f, 5 %% quantile %.4f, minimum %.4f" % (name, pairing, side, med, q05, lo))
            if name == "sharp":
                assert med >= 0.95 and q05 >= 0.7, (side, med, q05)
            else:
                assert lo >= 0.99, (side, lo)


@pytest.mark.parametrize("pairing", ["self", "cross"])
@pytest.mark.parametrize("axis", ["keys", "queries"])
def test_staircase_moves_the_running_maximum_at_nearly_every_tile(axis, pairing):
    _, _, s = _score("staircase_%s_up" % axis, pairing)
    n = R.running_max_increases(s, axis)
    share = float((n >= 15).double().mean())
    print("staircase %s %s up: minimum %d increases, %.2f %% of lines with >= 15" % (axis, pairing, int(n.min()), 100 * share))
    assert int(n.min()) >= 12 and share >= 0.98
    _, _, sd = _score("staircase_%s_down" % axis, pairing)
    nd = R.running_max_increases(sd, axis)
    assert float((nd <= 2).double().mean()) >= 0.98               # the flipped ramp: the maximum sits in the first tiles


@pytest.mark.parametrize("pairing", ["self", "cross"])
def test_large_scores_and_flat_rows(pairing):
    for f in (8, 40):
        _, _, s = _score("large%d" % f, pairing)
        assert torch.isfinite(s).all()
        if f == 40:
            assert float(s.abs().max()) > 500
    qkv, _, s = _score("flat", pairing)
    zq = 1 if pairing == "cross" else 0                            # the problem whose queries are image 0's
    assert float(s[zq].abs().max()) == 0.0 and float(s[1, 1].abs().max()) == 0.0 and float(s[1 - zq, 0].abs().max()) > 0.0
    lse = torch.logsumexp(s, -1)
    assert float((lse[zq] - R.LN_NTOK).abs().max()) < 1e-12


@pytest.mark.parametrize("name", R.FORWARD_SELF)
def test_attention_reference_is_finite_and_its_fp32_yardstick_is_small(name):
    qkv, _ = R.build(name, Z, "self")
    for kv_xor in (0, 1):
        o, lse, s = R.attn_ref(qkv, Z, kv_xor)
        assert all(bool(torch.isfinite(t).all()) for t in (o, lse, s))
        o32, lse32, _ = R.attn_ref(qkv, Z, kv_xor, dtype=torch.float32)
        e_o, where = R.block_rel(R.heads_of(o32, Z), R.heads_of(o, Z))
        e_l, _ = R.lse_err(lse32, lse)
        print("attention %s kv_xor=%d: fp32 o %.2e at %s, lse %.2e" % (name, kv_xor, e_o, where, e_l))
        assert e_o < 1e-4 and e_l < 1e-6


@pytest.mark.parametrize("name", R.FORWARD_CROSS)
def test_emm_reference_is_finite_and_its_fp32_yardstick_is_small(name, pos):
    qkv, _ = R.build(name, Z, "cross")
    for single, cross in ((False, False), (True, False), (False, True)):
        ref = R.emm_ref(qkv, pos, Z, single, cross)
        assert all(bool(torch.isfinite(t).all()) for t in ref)
        y = R.emm_ref(qkv, pos, Z, single, cross, dtype=torch.float32)
        e = dict(F=R.head_rel(y[0], ref[0])[0], T=R.block_rel(y[1], ref[1])[0], U=R.block_rel(y[2], ref[2])[0])
        print("EMM %s single=%d cross=%d: fp32 " % (name, single, cross) + ", ".join("%s %.2e" % kv for kv in e.items()))
        assert max(e.values()) < 1e-4


@pytest.mark.parametrize("name", R.GRADIENT_SELF)
@pytest.mark.parametrize("kv_xor", [0, 1])
def test_attention_gradient_yardstick_is_within_the_cap(name, kv_xor):
    qkv, _ = R.build(name, Z, "cross" if kv_xor else "self")
    cot = R.cotangent((Z * R.N_TOK, R.HEADS * R.HD), seed=2)
    fn = lambda x: R.attn_ref(x, Z, kv_xor, dtype=x.dtype)[0]
    g64, g32 = R.grads(fn, qkv, cot, Z, torch.float64), R.grads(fn, qkv, cot, Z, torch.float32)
    e = [R.head_rel(a, b) for a, b in zip(g32, g64)]
    print("attention %s kv_xor=%d: fp32 dq %.2e dk %.2e dv %.2e" % ((name, kv_xor) + tuple(x[0] for x in e)))
    assert all(bool(torch.isfinite(t).all()) for t in g64)
    assert max(x[0] for x in e) <= R.GRAD_YARDSTICK_CAP, e


@pytest.mark.parametrize("name", R.GRADIENT_CROSS)
@pytest.mark.parametrize("single,cross", [(False, False), (True, False), (False, True)])
def test_emm_gradient_yardstick_is_within_the_cap(name, single, cross, pos):
    qkv, _ = R.build(name, Z, "cross")
    cot = R.cotangent((Z, R.HEADS, 70, 70), seed=6)
    fn = lambda x: R.emm_ref(x, pos, Z, single, cross, dtype=x.dtype)[0]
    g64, g32 = R.grads(fn, qkv, cot, Z, torch.float64), R.grads(fn, qkv, cot, Z, torch.float32)
    e = [R.head_rel(a, b) for a, b in zip(g32, g64)]
    print("EMM %s single=%d cross=%d: fp32 dq %.2e dk %.2e dv %.2e" % ((name, single, cross) + tuple(x[0] for x in e)))
    assert all(bool(torch.isfinite(t).all()) for t in g64)
    assert max(x[0] for x in e) <= R.GRAD_YARDSTICK_CAP, e


def test_onehot_gradients_cancel_so_the_regime_is_forward_only():
    """with P one-hot, P (dP - delta) cancels to nothing: the gradient through the softmax is orders of magnitude below the values it is
    formed from, and plain fp32 is itself far outside the cap per head -- why `onehot` gradients are only bounded under the global metric"""
    qkv, _ = R.build("onehot", Z, "self")
    cot = R.cotangent((Z * R.N_TOK, R.HEADS * R.HD), seed=2)
    fn = lambda x: R.attn_ref(x, Z, dtype=x.dtype)[0]
    g64, g32 = R.grads(fn, qkv, cot, Z, torch.float64), R.grads(fn, qkv, cot, Z, torch.float32)
    assert float(g64[0].abs().max()) < 1e-2 * float(g64[2].abs().max())
    assert R.head_rel(g32[0], g64[0])[0] > R.GRAD_YARDSTICK_CAP


def test_block_metric_sees_what_the_global_one_hides():
    """an error of 1e-3 of ITS block's values in one 32-row block of one head, next to a spiky row elsewhere: 1e-3 under block_rel, at that
    block; below 5e-6 under the global metric"""
    g = torch.Generator().manual_seed(0)
    b = torch.randn(2, 3, 576, 64, generator=g, dtype=torch.float64)
    b[0, 0, 5] *= 1000.0
    a = b.clone()
    a[1, 2, 7 * 32:8 * 32] *= 1 + 1e-3
    e, where = R.block_rel(a, b)
    assert where == (1, 2, 7) and 0.5e-3 < e <= 1e-3
    assert R.rel(a, b) < 5e-6
    eh, wh = R.head_rel(a, b)
    assert wh == (1, 2) and 0.5e-3 < eh <= 1e-3
    l = torch.full((2, 3, 576), 700.0, dtype=torch.float64)
    l2 = l.clone()
    l2[1, 0, 17] += 7e-3
    e, where = R.lse_err(l2, l)
    assert where == (1, 0, 17) and abs(e - 1e-5) < 1e-9
    assert R.bound(1e-6) == 8e-6 and R.bound(1e-9, R.LSE_FLOOR) == 4 * 2.0 ** -23 and math.isclose(R.LN_NTOK, math.log(576))
