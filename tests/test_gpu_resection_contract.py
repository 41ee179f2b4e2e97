"""The memory contract of the two launching entry points of include/relpose_resection.h by the rules of
tests/test_gpu_memory_contract.py, as tests/test_gpu_rotation_contract.py does it for the rotation library: every operand between guard
bands, outputs poisoned (a NaN pattern in one run, a finite pattern in the other), packed layouts, with and without the optional
operands, healthy and degenerate problems in one batch -- the guards come back untouched, every documented output element is written and
nothing else, the inputs are unchanged, the two runs agree bit for bit, and nothing non-finite is written."""
import numpy as np
import pytest
import torch

from tests import _contract_cases as CC
from tests import _resection_ref as T
from tests.test_gpu_kernels import report
from tests.test_gpu_memory_contract import run_case

pytestmark = pytest.mark.gpu
# (n, P, M): the smallest of each, and M one above a multiple of the workgroup (two chunks, the second nearly empty)
SHAPES = [(1, 3, 1), (3, 4, 257), (1, 64, 257), (3, 257, 1)]
_CONTRACT = [(e, n, P, M, ww, opt) for e in ("consensus", "refine") for n, P, M in SHAPES for ww in (False, True) for opt in (False, True)]


def _inputs(n, P):
    X, x, pose = T.exact_rows(n, P, 11)
    w = np.random.default_rng(P + n).uniform(0.05, 1.0, (n, P)).astype(np.float32)
    if P >= 24:
        w[:, ::3] = 0
        w[:, 4], w[:, 7] = -1.0, np.nan
    tau = np.full(n, T.TAU, np.float32)
    if n > 1:                                                     # a degenerate problem among the healthy ones: its outputs are written, too
        tau[1] = 0
    return X, x, w, tau, pose.astype(np.float32)


def _case(entry, n, P, M, with_w, optional):
    X, x, w, tau, p0 = _inputs(n, P)
    ops_ = [CC.inp("X", torch.from_numpy(X).reshape(1, -1)), CC.inp("x", torch.from_numpy(x).reshape(1, -1)),
            CC.inp("tau", torch.from_numpy(tau).reshape(1, -1))]
    if with_w:
        ops_.append(CC.inp("w", torch.from_numpy(w).reshape(1, -1)))
    if entry == "consensus":
        ops_ += [CC.flat("pose", n * 7), CC.flat("best", n, dtype=CC.I32), CC.flat("stat", n * 4), CC.flat("hyp_pose", n * M * 7),
                 CC.flat("hyp_cost", n * M)]
        if optional:
            ops_ += [CC.flat("w_out", n * P), CC.flat("hyp_count", n * M, dtype=CC.I32), CC.flat("samples", n * M * 3, dtype=CC.I32)]

        def call(lib, A_, st):
            lib.rp_p3p_consensus(CC.a_(A_, "X"), CC.a_(A_, "x"), CC.a_(A_, "w"), CC.a_(A_, "tau"), T.SEED, CC.a_(A_, "pose"),
                                 CC.a_(A_, "best"), CC.a_(A_, "stat"), CC.a_(A_, "w_out"), CC.a_(A_, "hyp_pose"), CC.a_(A_, "hyp_cost"),
                                 CC.a_(A_, "hyp_count"), CC.a_(A_, "samples"), P, M, n, st)
    else:
        ops_ += [CC.inp("pose0", torch.from_numpy(p0).reshape(1, -1)), CC.flat("pose", n * 7), CC.flat("stat", n * 4)]
        if optional:
            ops_.append(CC.flat("w_out", n * P))

        def call(lib, A_, st):
            lib.rp_pnp_refine(CC.a_(A_, "X"), CC.a_(A_, "x"), CC.a_(A_, "w"), CC.a_(A_, "tau"), CC.a_(A_, "pose0"), 3, CC.a_(A_, "pose"),
                              CC.a_(A_, "stat"), CC.a_(A_, "w_out"), P, n, st)

    def check(v, errs):
        cpu = {k: t.cpu().numpy().reshape(-1) for k, t in v.items()}
        if not all(np.isfinite(a).all() for a in cpu.values()):
            errs.append("non-finite output")
        deg = [1] if n > 1 else []
        for b in deg:                                             # the degenerate problem's documented outputs
            if entry == "consensus" and (cpu["pose"].reshape(n, 7)[b].any() or cpu["best"].reshape(n)[b] != -1
                                         or cpu["hyp_pose"].reshape(n, M, 7)[b].any()):
                errs.append("degenerate problem: pose / best / hyp_pose")
            if entry == "refine" and (not np.array_equal(cpu["pose"].reshape(n, 7)[b], p0[b]) or cpu["stat"].reshape(n, 4)[b, :3].any()):
                errs.append("degenerate problem: pose is not pose0 / stat")
        if entry == "consensus" and optional and not np.array_equal(cpu["samples"].reshape(n, M, 3),
                                                                    T.sample_rows3(w if with_w else None, n, P, T.SEED, M)[1]):
            errs.append("samples differ from the reference sampler")
        return {}
    return CC.Case(ops_, call, check)


@pytest.mark.parametrize("entry,n,P,M,with_w,optional", _CONTRACT,
                         ids=["%s-n%d-P%d-M%d-%s-%s" % (e, n, P, M, "w" if a else "now", "optional" if b else "required") for e, n, P, M, a, b in _CONTRACT])
def test_memory_contract(entry, n, P, M, with_w, optional):
    """guards intact, every documented element written and nothing else, inputs unchanged, NaN-fill and finite-fill runs bit-identical"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    _lib.load()
    lib = _lib.load_resection()
    builder = lambda: _case(entry, n, P, M, with_w, optional)       # noqa: E731
    bad_a, va, c, ops_ = run_case(lib, builder, finite=False)
    bad_b, vb, _, _ = run_case(lib, builder, finite=True)
    bad = ["NaN-fill run: " + b for b in bad_a] + ["finite-fill run: " + b for b in bad_b]
    want = {"consensus": {"pose", "best", "stat", "hyp_pose", "hyp_cost"} | ({"w_out", "hyp_count", "samples"} if optional else set()),
            "refine": {"pose", "stat"} | ({"w_out"} if optional else set())}[entry]
    assert set(va) == {o.name for o in ops_ if o.role == "out"} == want
    for k in va:
        bits = CC._BITS[va[k].dtype]
        if not torch.equal(va[k].view(bits), vb[k].view(bits)):
            bad.append("%s: result depends on what the output held before the call" % k)
    if not bad_a:
        c.check(va, bad)
    report("resection_memory_contract_%s_n%d_P%d_M%d_w%d_opt%d" % (entry, n, P, M, with_w, optional), violations=len(bad))
    assert not bad, "\n".join(bad)
