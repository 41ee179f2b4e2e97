"""The memory contract of rp_five_point_consensus (include/relpose_fivepoint.h) by the rules of tests/test_gpu_memory_contract.py, as
tests/test_gpu_consensus_contract.py does it for the eight-point consensus: every operand between guard bands, outputs poisoned (a NaN
pattern in one run, a finite pattern in the other), packed layouts, with and without the optional operands -- the guards come back
untouched, every documented output element is written and nothing else, the inputs are unchanged, the two runs agree bit for bit, and
the values pass the score and selection checks of tests/test_gpu_fivepoint.py at its bounds."""
import numpy as np
import pytest
import torch

from tests import _contract_cases as CC
from tests import _eightpoint_ref as R
from tests import _fivepoint_ref as F
from tests.test_gpu_kernels import report
from tests.test_gpu_memory_contract import run_case

pytestmark = pytest.mark.gpu
# (n, P, M): the smallest of each, and M one above a multiple of the workgroup (two chunks, the second nearly empty)
SHAPES = [(1, 5, 1), (3, 5, 257), (1, 64, 257), (3, 64, 1)]
_CONTRACT = [(n, P, M, ww, opt) for n, P, M in SHAPES for ww in (False, True) for opt in (False, True)]


def _case(n, P, M, with_w, optional):
    x1, x2, _ = R.scenes(n, P, seed=11)
    x1, x2 = x1.astype(np.float32), x2.astype(np.float32)
    w = np.random.default_rng(P + n).uniform(0.05, 1.0, (n, P)).astype(np.float32)
    if P >= 24:
        w[:, ::3] = 0
    tau = np.full(n, F.TAU, np.float32)
    ops_ = [CC.inp("x1", torch.from_numpy(x1).reshape(1, -1)), CC.inp("x2", torch.from_numpy(x2).reshape(1, -1)),
            CC.inp("tau", torch.from_numpy(tau).reshape(1, -1)), CC.flat("E", n * 9), CC.flat("best", n * 2, dtype=CC.I32),
            CC.flat("stat", n * 4), CC.flat("hyp_E", n * M * 90), CC.flat("hyp_cost", n * M * 10)]
    if with_w:
        ops_.append(CC.inp("w", torch.from_numpy(w).reshape(1, -1)))
    if optional:
        ops_ += [CC.flat("w_out", n * P), CC.flat("samples", n * M * 5, dtype=CC.I32)]

    def call(lib, A_, st):
        lib.rp_five_point_consensus(CC.a_(A_, "x1"), CC.a_(A_, "x2"), CC.a_(A_, "w"), CC.a_(A_, "tau"), F.SEED, CC.a_(A_, "E"),
                                    CC.a_(A_, "best"), CC.a_(A_, "stat"), CC.a_(A_, "w_out"), CC.a_(A_, "hyp_E"), CC.a_(A_, "hyp_cost"),
                                    CC.a_(A_, "samples"), P, M, n, st)

    def check(v, errs):
        ww = w if with_w else None
        cpu = {k: t.cpu().numpy() for k, t in v.items()}
        samples = F.sample_rows5(ww, n, P, F.SEED, M)[1]
        out = F.Consensus5(cpu["E"].reshape(n, 3, 3), cpu["best"].reshape(n, 2), cpu["stat"].reshape(n, 4),
                           cpu["w_out"].reshape(n, P) if optional else None, cpu["hyp_E"].reshape(n, M, 10, 3, 3),
                           cpu["hyp_cost"].reshape(n, M, 10), cpu["samples"].reshape(n, M, 5) if optional else samples)
        if not all(np.isfinite(a).all() for a in out if a is not None):
            errs.append("non-finite output")
        if not np.array_equal(out.samples, samples):
            errs.append("samples differ from the reference sampler")
        try:
            return F.check_consensus(out, x1, x2, ww, F.TAU)
        except AssertionError as e:
            errs.append("score / selection: %r" % (e,))
            return {}
    return CC.Case(ops_, call, check)


@pytest.mark.parametrize("n,P,M,with_w,optional", _CONTRACT,
                         ids=["n%d-P%d-M%d-%s-%s" % (n, P, M, "w" if a else "now", "optional" if b else "required") for n, P, M, a, b in _CONTRACT])
def test_memory_contract(n, P, M, with_w, optional):
    """guards intact, every documented element written and nothing else, inputs unchanged, NaN-fill and finite-fill runs bit-identical"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    _lib.load()
    lib = _lib.load_fivepoint()
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
    report("fivepoint_memory_contract_n%d_P%d_M%d_w%d_opt%d" % (n, P, M, with_w, optional), violations=len(bad), **errs)
    assert not bad, "\n".join(bad)
