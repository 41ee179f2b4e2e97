"""The memory contract of rp_triangulate (include/relpose_triangulate.h) by the rules of tests/test_gpu_memory_contract.py, as
tests/test_gpu_homography_contract.py does it for the homography library: every operand between guard bands, outputs poisoned (a NaN
pattern in one run, a finite pattern in the other), packed layouts, with and without the optional operands (w in, xc out), a degenerate
problem in the batch -- the guards come back untouched, every documented output element is written and nothing else, the inputs are
unchanged, the two runs agree bit for bit, and nothing non-finite is written."""
import numpy as np
import pytest
import torch

from tests import _contract_cases as CC
from tests import _triangulate_ref as T
from tests.test_gpu_kernels import report
from tests.test_gpu_memory_contract import run_case

pytestmark = pytest.mark.gpu
# (n, P): the smallest, an odd one, one row past a full sweep of the workgroup (the second row slot nearly empty), a batch
SHAPES = [(1, 1), (3, 5), (1, 257), (3, 64)]
_CONTRACT = [(n, P, ww, opt) for n, P in SHAPES for ww in (False, True) for opt in (False, True)]


def _inputs(n, P):
    x1, x2, pose = T.scenes(n, P, 11, 3.0, 1e-3, 0.1 if P >= 10 else 0.0)[:3]
    w = np.random.default_rng(P + n).uniform(0.05, 1.0, (n, P)).astype(np.float32)
    if P >= 24:
        w[:, ::3] = 0
        w[:, 4], w[:, 7] = -1.0, np.nan
    tau = np.full(n, T.TAU, np.float32)
    pose = pose.astype(np.float32)
    if n > 1:                                                     # a degenerate problem among the healthy ones: its outputs are written, too
        pose[1, :3] = 0
    return pose, x1, x2, w, tau


def _case(n, P, with_w, optional):
    pose, x1, x2, w, tau = _inputs(n, P)
    ops_ = [CC.inp("pose", torch.from_numpy(pose).reshape(1, -1)), CC.inp("x1", torch.from_numpy(x1).reshape(1, -1)),
            CC.inp("x2", torch.from_numpy(x2).reshape(1, -1)), CC.inp("tau", torch.from_numpy(tau).reshape(1, -1))]
    if with_w:
        ops_.append(CC.inp("w", torch.from_numpy(w).reshape(1, -1)))
    ops_ += [CC.flat("X", n * P * 3), CC.flat("aux", n * P * 4), CC.flat("stat", n * 4)]
    if optional:
        ops_.append(CC.flat("xc", n * P * 4))

    def call(lib, A_, st):
        lib.rp_triangulate(CC.a_(A_, "pose"), CC.a_(A_, "x1"), CC.a_(A_, "x2"), CC.a_(A_, "w"), CC.a_(A_, "tau"), CC.a_(A_, "X"),
                           CC.a_(A_, "aux"), CC.a_(A_, "xc"), CC.a_(A_, "stat"), P, n, st)

    def check(v, errs):
        cpu = {k: t.cpu().numpy().reshape(-1) for k, t in v.items()}
        if not all(np.isfinite(a).all() for a in cpu.values()):
            errs.append("non-finite output")
        K = (T.clamp(w if with_w else None, n, P) > 0).sum(-1)
        if not np.array_equal(cpu["stat"].reshape(n, 4)[:, 3], K):
            errs.append("stat: K")
        if n > 1:                                                  # the degenerate problem's documented outputs
            if cpu["X"].reshape(n, -1)[1].any() or cpu["aux"].reshape(n, -1)[1].any() or cpu["stat"].reshape(n, 4)[1, :3].any():
                errs.append("degenerate problem: X / aux / stat")
            if optional and cpu["xc"].reshape(n, -1)[1].any():
                errs.append("degenerate problem: xc")
        if not cpu["X"].reshape(n, -1)[0].any() or not cpu["aux"].reshape(n, P, 4)[0, :, 2:].all():
            errs.append("healthy problem: X / d2 / phi not written")
        return {}
    return CC.Case(ops_, call, check)


@pytest.mark.parametrize("n,P,with_w,optional", _CONTRACT,
                         ids=["n%d-P%d-%s-%s" % (n, P, "w" if a else "now", "optional" if b else "required") for n, P, a, b in _CONTRACT])
def test_memory_contract(n, P, with_w, optional):
    """guards intact, every documented element written and nothing else, inputs unchanged, NaN-fill and finite-fill runs bit-identical"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    _lib.load()
    lib = _lib.load_triangulate()
    builder = lambda: _case(n, P, with_w, optional)                 # noqa: E731
    bad_a, va, c, ops_ = run_case(lib, builder, finite=False)
    bad_b, vb, _, _ = run_case(lib, builder, finite=True)
    bad = ["NaN-fill run: " + b for b in bad_a] + ["finite-fill run: " + b for b in bad_b]
    assert set(va) == {o.name for o in ops_ if o.role == "out"} == {"X", "aux", "stat"} | ({"xc"} if optional else set())
    for k in va:
        bits = CC._BITS[va[k].dtype]
        if not torch.equal(va[k].view(bits), vb[k].view(bits)):
            bad.append("%s: result depends on what the output held before the call" % k)
    if not bad_a:
        c.check(va, bad)
    report("triangulate_memory_contract_n%d_P%d_w%d_opt%d" % (n, P, with_w, optional), violations=len(bad))
    assert not bad, "\n".join(bad)
