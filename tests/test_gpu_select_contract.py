"""The memory contract of rp_model_select (include/relpose_select.h) by the rules of tests/test_gpu_memory_contract.py, as
tests/test_gpu_rotation_contract.py does it for the rotation library: every operand between guard bands, outputs poisoned (a NaN
pattern in one run, a finite pattern in the other), packed layouts, with and without the optional operands (w, sigma; resid, label),
healthy and degenerate problems and an invalid candidate in one batch -- the guards come back untouched, every documented output element
is written and nothing else, the inputs are unchanged, the two runs agree bit for bit, and nothing non-finite is written."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _contract_cases as CC
from tests import _select_ref as S
from tests.test_gpu_kernels import report
from tests.test_gpu_memory_contract import run_case

pytestmark = pytest.mark.gpu
# (n, P, C): the smallest of each, one row past a multiple of the workgroup, every candidate slot in use
SHAPES = [(1, 8, 1), (3, 9, 5), (3, 257, 8), (2, 64, 5)]
_CONTRACT = [(n, P, Cn, ww, opt) for n, P, Cn in SHAPES for ww in (False, True) for opt in (False, True)]


def _inputs(n, P, Cn):
    x1, x2, _, models, kinds, _ = S.inputs("mixed", n, P, Cn, False)
    w = np.random.default_rng(P + n).uniform(0.05, 1.0, (n, P)).astype(np.float32)
    if P >= 24:
        w[:, ::3] = 0
        w[:, 4], w[:, 7] = -1.0, np.nan
    tau = np.full(n, S.TAU, np.float32)
    sigma = np.full(n, S.SIGMA if P < S.GIVEN_BELOW else 0.0, np.float32)
    models = models.copy()
    if n > 1:                                                     # a degenerate problem among the healthy ones: its outputs are written, too
        tau[1] = 0
    if Cn > 1:
        models[0, 1] = 0                                          # and an invalid candidate
    return x1, x2, w, tau, sigma, models, kinds


def _case(n, P, Cn, with_w, optional):
    x1, x2, w, tau, sigma, models, kinds = _inputs(n, P, Cn)
    ops_ = [CC.inp("x1", torch.from_numpy(x1).reshape(1, -1)), CC.inp("x2", torch.from_numpy(x2).reshape(1, -1)),
            CC.inp("tau", torch.from_numpy(tau).reshape(1, -1)), CC.inp("models", torch.from_numpy(models).reshape(1, -1)),
            CC.flat("pick", n, dtype=CC.I32), CC.flat("stat", n * Cn * 4), CC.flat("scale", n * 2)]
    given = P < S.GIVEN_BELOW
    if with_w:
        ops_.append(CC.inp("w", torch.from_numpy(w).reshape(1, -1)))
    if given or with_w:                                           # (without it the scale is estimated; below P = 32 it has to be given)
        ops_.append(CC.inp("sigma", torch.from_numpy(sigma).reshape(1, -1)))
    if optional:
        ops_ += [CC.flat("resid", n * Cn * P), CC.flat("label", n * P, dtype=CC.I32)]
    host = (ctypes.c_int * Cn)(*kinds)

    def call(lib, A_, st):
        lib.rp_model_select(CC.a_(A_, "x1"), CC.a_(A_, "x2"), CC.a_(A_, "w"), CC.a_(A_, "tau"), CC.a_(A_, "sigma"), CC.a_(A_, "models"),
                            ctypes.cast(host, ctypes.c_void_p), S.COST, CC.a_(A_, "pick"), CC.a_(A_, "stat"), CC.a_(A_, "scale"),
                            CC.a_(A_, "resid"), CC.a_(A_, "label"), P, Cn, n, st)

    def check(v, errs):
        cpu = {k: t.cpu().numpy().reshape(-1) for k, t in v.items()}
        if not all(np.isfinite(a).all() for a in cpu.values()):
            errs.append("non-finite output")
        pick, stat, scale = cpu["pick"].reshape(n), cpu["stat"].reshape(n, Cn, 4), cpu["scale"].reshape(n, 2)
        none = np.float32([S.FLT_MAX, 0, 0, 0])
        if n > 1 and (pick[1] != -1 or not (stat[1] == none).all() or scale[1].tolist() != [0, -1]):
            errs.append("degenerate problem: pick / stat / scale")
        if n > 1 and optional and cpu["label"].reshape(n, P)[1].any():
            errs.append("degenerate problem: label")
        if pick[0] < 0 or (Cn > 1 and (pick[0] == 1 or not (stat[0, 1] == none).all())):
            errs.append("healthy problem: pick, or the invalid candidate's stat")
        if optional:
            dev = S.Selection(pick, stat, scale, cpu["resid"].reshape(n, Cn, P), cpu["label"].reshape(n, P), None, None, None)
            try:
                S.consistent(dev, x1, x2, w if with_w else None, tau, sigma if (given or with_w) else None, models, kinds)
            except AssertionError as e:
                errs.append("outputs inconsistent with the device's own residuals: %s" % (e,))
        return {}
    return CC.Case(ops_, call, check)


@pytest.mark.parametrize("n,P,Cn,with_w,optional", _CONTRACT,
                         ids=["n%d-P%d-C%d-%s-%s" % (n, P, Cn, "w" if a else "now", "optional" if b else "required") for n, P, Cn, a, b in _CONTRACT])
def test_memory_contract(n, P, Cn, with_w, optional):
    """guards intact, every documented element written and nothing else, inputs unchanged, NaN-fill and finite-fill runs bit-identical"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    _lib.load()
    lib = _lib.load_select()
    builder = lambda: _case(n, P, Cn, with_w, optional)             # noqa: E731
    bad_a, va, c, ops_ = run_case(lib, builder, finite=False)
    bad_b, vb, _, _ = run_case(lib, builder, finite=True)
    bad = ["NaN-fill run: " + b for b in bad_a] + ["finite-fill run: " + b for b in bad_b]
    want = {"pick", "stat", "scale"} | ({"resid", "label"} if optional else set())
    assert set(va) == {o.name for o in ops_ if o.role == "out"} == want
    for k in va:
        bits = CC._BITS[va[k].dtype]
        if not torch.equal(va[k].view(bits), vb[k].view(bits)):
            bad.append("%s: result depends on what the output held before the call" % k)
    if not bad_a:
        c.check(va, bad)
    report("select_memory_contract_n%d_P%d_C%d_w%d_opt%d" % (n, P, Cn, with_w, optional), violations=len(bad))
    assert not bad, "\n".join(bad)
