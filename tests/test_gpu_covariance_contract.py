"""The memory contract of rp_pose_covariance (include/relpose_covariance.h) by the rules of tests/test_gpu_memory_contract.py, as
tests/test_gpu_select_contract.py does it for the selection library: every operand between guard bands, outputs poisoned (a NaN pattern
in one run, a finite pattern in the other), packed layouts, with and without the optional operands (w; normal), healthy, degenerate and
undetermined problems in one batch -- the guards come back untouched, every documented output element is written and nothing else, the
inputs are unchanged, the two runs agree bit for bit, and nothing non-finite is written."""
import numpy as np
import pytest
import torch

from tests import _contract_cases as CC
from tests import _covariance_ref as C
from tests.test_gpu_kernels import report
from tests.test_gpu_memory_contract import run_case

pytestmark = pytest.mark.gpu
# (n, P): the smallest of each, one row past a multiple of the workgroup
SHAPES = [(1, 6), (3, 9), (3, 257), (2, 64)]
_CONTRACT = [(n, P, ww, opt) for n, P in SHAPES for ww in (False, True) for opt in (False, True)]
SIZES = {"cov": 25, "frame": 6, "eig": 5, "weak": 5, "stat": 8, "normal": 30}


def _inputs(n, P):
    pose, x1, x2, w, tau = C.gpu_case(n, P, True)
    tau = tau.copy()
    if n > 1:                                                     # a degenerate problem among the healthy ones: its outputs are written, too
        tau[1] = 0
    if n > 2:                                                     # and an undetermined one
        pose, x1, x2 = pose.copy(), x1.copy(), x2.copy()
        pose[2], x1[2], x2[2] = C.not_determined_problem(P)
        tau[2] = 3e-3
        w = w.copy()
        w[2] = 1.0
    return pose, x1, x2, w, tau


def _case(n, P, with_w, optional):
    pose, x1, x2, w, tau = _inputs(n, P)
    ops_ = [CC.inp("pose", torch.from_numpy(pose).reshape(1, -1)), CC.inp("x1", torch.from_numpy(x1).reshape(1, -1)),
            CC.inp("x2", torch.from_numpy(x2).reshape(1, -1)), CC.inp("tau", torch.from_numpy(tau).reshape(1, -1))]
    ops_ += [CC.flat(k, n * SIZES[k]) for k in ("cov", "frame", "eig", "weak", "stat")]
    if with_w:
        ops_.append(CC.inp("w", torch.from_numpy(w).reshape(1, -1)))
    if optional:
        ops_.append(CC.flat("normal", n * SIZES["normal"]))

    def call(lib, A_, st):
        lib.rp_pose_covariance(CC.a_(A_, "pose"), CC.a_(A_, "x1"), CC.a_(A_, "x2"), CC.a_(A_, "w"), CC.a_(A_, "tau"), CC.a_(A_, "cov"),
                               CC.a_(A_, "frame"), CC.a_(A_, "eig"), CC.a_(A_, "weak"), CC.a_(A_, "stat"), CC.a_(A_, "normal"), P, n, st)

    def check(v, errs):
        cpu = {k: t.cpu().numpy().reshape(n, -1) for k, t in v.items()}
        if not all(np.isfinite(a).all() for a in cpu.values()):
            errs.append("non-finite output")
        ref = C.covariance_f32(pose, x1, x2, w if with_w else None, tau)
        if not np.array_equal(cpu["stat"][:, :2], ref.stat[:, :2]) or not np.array_equal(cpu["frame"], ref.frame):
            errs.append("status, K or frame differ from the float32 restatement")
        if n > 1 and any(a[1].any() for a in cpu.values()):
            errs.append("degenerate problem: an output is not zero")
        if n > 2 and (cpu["stat"][2, 0] != C.NOT_DETERMINED or cpu["cov"][2].any() or cpu["eig"][2].any() or cpu["weak"][2].any()
                      or not cpu["frame"][2].any() or (optional and not cpu["normal"][2].any())):
            errs.append("undetermined problem: status, or what is zeroed and what is kept")
        if cpu["stat"][0, 0] == C.OK and not np.array_equal(cpu["cov"][0].reshape(5, 5), cpu["cov"][0].reshape(5, 5).T):
            errs.append("cov is not symmetric")
        return {}
    return CC.Case(ops_, call, check)


@pytest.mark.parametrize("n,P,with_w,optional", _CONTRACT,
                         ids=["n%d-P%d-%s-%s" % (n, P, "w" if a else "now", "optional" if b else "required") for n, P, a, b in _CONTRACT])
def test_memory_contract(n, P, with_w, optional):
    """guards intact, every documented element written and nothing else, inputs unchanged, NaN-fill and finite-fill runs bit-identical"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    _lib.load()
    lib = _lib.load_covariance()
    builder = lambda: _case(n, P, with_w, optional)                 # noqa: E731
    bad_a, va, c, ops_ = run_case(lib, builder, finite=False)
    bad_b, vb, _, _ = run_case(lib, builder, finite=True)
    bad = ["NaN-fill run: " + b for b in bad_a] + ["finite-fill run: " + b for b in bad_b]
    want = {"cov", "frame", "eig", "weak", "stat"} | ({"normal"} if optional else set())
    assert set(va) == {o.name for o in ops_ if o.role == "out"} == want
    for k in va:
        bits = CC._BITS[va[k].dtype]
        if not torch.equal(va[k].view(bits), vb[k].view(bits)):
            bad.append("%s: result depends on what the output held before the call" % k)
    if not bad_a:
        c.check(va, bad)
    report("covariance_memory_contract_n%d_P%d_w%d_opt%d" % (n, P, with_w, optional), violations=len(bad))
    assert not bad, "\n".join(bad)
