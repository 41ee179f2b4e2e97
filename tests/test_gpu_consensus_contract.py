"""The memory contract of rp_eight_point_consensus (include/relpose_consensus.h) by the rules of tests/test_gpu_memory_contract.py: every
operand between guard bands, outputs poisoned (a NaN pattern in one run, a finite pattern in the other), with and without the optional
operands -- the guards come back untouched, every documented output element is written and nothing else, the inputs are unchanged,
the two runs agree bit for bit, and the values are those of tests/test_gpu_consensus.py at its bounds."""
import numpy as np
import pytest
import torch

from tests import _consensus_ref as C
from tests import _contract_cases as CC
from tests.test_gpu_kernels import report
from tests.test_gpu_memory_contract import run_case

pytestmark = pytest.mark.gpu
# (n, P, M): one chunk of hypotheses and several, M below, at and above a multiple of the workgroup; the largest P
SHAPES = [(3, 8, 1), (2, 257, 256), (2, 300, 513), (1, 1728, 300)]
_CONTRACT = [(n, P, M, ww, opt) for n, P, M in SHAPES for ww in (False, True) for opt in (False, True)]


def _case(n, P, M, with_w, optional):
    x1, x2, w, _ = C.inputs("exact", n, P, M, True)
    tau = np.full(n, C.TAU, np.float32)
    ops_ = [CC.inp("x1", torch.from_numpy(x1).reshape(1, -1)), CC.inp("x2", torch.from_numpy(x2).reshape(1, -1)),
            CC.inp("tau", torch.from_numpy(tau).reshape(1, -1)), CC.flat("E", n * 9), CC.flat("best", n, dtype=CC.I32),
            CC.flat("stat", n * 4), CC.flat("hyp_E", n * M * 9), CC.flat("hyp_cost", n * M)]
    if with_w:
        ops_.append(CC.inp("w", torch.from_numpy(w).reshape(1, -1)))
    if optional:
        ops_ += [CC.flat("w_out", n * P), CC.flat("samples", n * M * 8, dtype=CC.I32)]

    def call(lib, A_, st):
        lib.rp_eight_point_consensus(CC.a_(A_, "x1"), CC.a_(A_, "x2"), CC.a_(A_, "w"), CC.a_(A_, "tau"), C.SEED, CC.a_(A_, "E"),
                                     CC.a_(A_, "best"), CC.a_(A_, "stat"), CC.a_(A_, "w_out"), CC.a_(A_, "hyp_E"), CC.a_(A_, "hyp_cost"),
                                     CC.a_(A_, "samples"), P, M, n, st)

    def check(v, errs):
        ww = w if with_w else None
        ref = C.consensus_ref(x1, x2, ww, C.TAU, C.SEED, M)
        cpu = {k: t.cpu().numpy() for k, t in v.items()}
        wo = cpu["w_out"].reshape(n, P) if optional else C.weights64(cpu["E"].reshape(n, 3, 3), x1, x2, C.clamp(ww, n, P), tau).astype(np.float32)
        out = C.Consensus(cpu["E"].reshape(n, 3, 3), cpu["best"].reshape(n), cpu["stat"].reshape(n, 4), wo, cpu["hyp_E"].reshape(n, M, 3, 3),
                          cpu["hyp_cost"].reshape(n, M), cpu["samples"].reshape(n, M, 8) if optional else ref.samples, None)
        if not all(np.isfinite(a).all() for a in out[:6]):
            errs.append("non-finite output")
        if not np.array_equal(out.samples, ref.samples):
            errs.append("samples differ from the reference sampler")
        if not np.array_equal(out.best, out.hyp_cost.argmin(-1)):
            errs.append("best is not the lowest-index argmin of hyp_cost")
        r = C.ratios(out, ref, x1, x2, ww)
        e = {"E_ratio": CC._bound(errs, "hyp_E", r["E"], C.C_E["exact"]), "E_gain_ratio": CC._bound(errs, "hyp_E", r["E_gain"], C.C_E_GAIN),
             "cost_ratio": CC._bound(errs, "hyp_cost", r["cost"], C.C_COST)}
        if optional:
            e["w_ratio"] = CC._bound(errs, "w_out", r["w"], C.C_W)
        return e
    return CC.Case(ops_, call, check)


@pytest.mark.parametrize("n,P,M,with_w,optional", _CONTRACT,
                         ids=["n%d-P%d-M%d-%s-%s" % (n, P, M, "w" if a else "now", "optional" if b else "required") for n, P, M, a, b in _CONTRACT])
def test_memory_contract(n, P, M, with_w, optional):
    """guards intact, every documented element written and nothing else, inputs unchanged, NaN-fill and finite-fill runs bit-identical"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    _lib.load()
    lib = _lib.load_consensus()
    builder = lambda: _case(n, P, M, with_w, optional)             # noqa: E731
    bad_a, va, c, ops_ = run_case(lib, builder, finite=False)
    bad_b, vb, _, _ = run_case(lib, builder, finite=True)
    bad = ["NaN-fill run: " + b for b in bad_a] + ["finite-fill run: " + b for b in bad_b]
    want = {"E", "best", "stat", "hyp_E", "hyp_cost"} | ({"w_out", "samples"} if optional else set())
    assert set(va) == {o.name for o in ops_ if o.role == "out"} == want
    for k in va:
        bits = CC._BITS[va[k].dtype]
        if not torch.equal(va[k].view(bits), vb[k].view(bits)):
            bad.append("%s: result depends on what the output held before the call" % k)
    errs = c.check(va, bad) if not bad_a else {}
    report("consensus_memory_contract_n%d_P%d_M%d_w%d_opt%d" % (n, P, M, with_w, optional), violations=len(bad), **errs)
    assert not bad, "\n".join(bad)
