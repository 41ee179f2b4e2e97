"""The memory contract of rp_emm_guided_matches (include/relpose_guided.h) by the rules of tests/test_gpu_memory_contract.py, as
tests/test_gpu_triangulate_contract.py does it for the triangulation library: every operand between guard bands, outputs poisoned (a
NaN pattern in one run, a finite pattern in the other), packed and strided q / k (one buffer, or one each with a row stride of their
own, bit-identical to the packed sibling), both swaps and softmaxes, a degenerate image in the batch -- the guards come back untouched,
every documented output element is written and nothing else, the inputs are unchanged, the two runs agree bit for bit, and nothing
non-finite is written."""
import numpy as np
import pytest
import torch

from tests import _contract_cases as CC
from tests import _guided_ref as G
from tests import _submatch_ref as S
from tests.test_gpu_kernels import report
from tests.test_gpu_memory_contract import run_case

pytestmark = pytest.mark.gpu
N, H = CC.N_TOK, CC.HEADS


def _F(Z, dead):
    F1 = G.grid_F(S.built_inputs(0)).reshape(3, 3)
    F = np.stack([F1.T.reshape(9), F1.reshape(9)] * (Z // 2)).astype(np.float32)
    band = np.full(Z, 1.5, np.float32)
    if dead == "F":
        F[Z - 1] = 0
    elif dead == "band":
        band[0] = np.nan
    return F, band


def _case(Z, ld, swap=False, single=False, split=False, dead=None):
    """one guarded call.  split: q and k in buffers of their own with row stride ld; otherwise one packed q | k buffer"""
    d = CC._emm_data(Z)
    q, k = d["qkv"][:, :CC.DIM], d["qkv"][:, CC.DIM:2 * CC.DIM]
    F, band = _F(Z, dead)
    if split:
        ops_ = [CC.inp("q", q, ld=ld), CC.inp("k", k, ld=ld)]
    else:
        ops_ = [CC.inp_multi("qk", Z * N, ld, {0: d["qkv"][:, :2 * CC.DIM]})]
    ops_ += [CC.inp("rlse", CC._f32(d["rlse"]).reshape(1, -1)), CC.inp("F", torch.from_numpy(F).reshape(1, -1)),
             CC.inp("band", torch.from_numpy(band).reshape(1, -1)), CC.flat("idx", Z * H * N, dtype=CC.I32), CC.flat("stat", Z * H * N * 4)]
    if not single:
        ops_.append(CC.inp("clse", CC._f32(d["clse"]).reshape(1, -1)))

    def call(lib, A_, st):
        P = CC.P
        qa, ka = (A_["q"].addr(), A_["k"].addr()) if split else (A_["qk"].addr(), A_["qk"].addr(CC.DIM))
        lib.rp_emm_guided_matches(P(qa), P(ka), P(A_["rlse"].addr()), None if single else P(A_["clse"].addr()), P(A_["F"].addr()),
                                  P(A_["band"].addr()), P(A_["idx"].addr()), P(A_["stat"].addr()), Z, H, ld, ld, CC.SCALE, int(swap), int(single), st)

    def check(v, errs):
        i, s = v["idx"].view(Z, H, N).cpu().numpy(), v["stat"].view(Z, H, N, 4).cpu().numpy()
        if not np.isfinite(s).all():
            errs.append("non-finite output")
        if not bool(((i >= -1) & (i < N)).all()):
            errs.append("idx outside -1..575")
        gone = G.degenerate(F, band)
        if not bool((i[gone] == -1).all()) or s[gone].any():
            errs.append("degenerate image: idx / stat")
        if not s[~gone][..., 2].all() or not (i[~gone] >= 0).any():
            errs.append("live image: mass / idx not written")
        if not bool((s[..., 1] <= s[..., 2]).all()):
            errs.append("bmass exceeds mass")
        return {"none": float((i[~gone] < 0).mean())}
    return CC.Case(ops_, call, check, sibling=(lambda: _case(Z, 2 * CC.DIM, swap, single, False, dead)) if split else None)


_CASES = [("Z2-packed", lambda: _case(2, 576)),
          ("Z2-packed-swap", lambda: _case(2, 576, swap=True)),
          ("Z4-ld640-dead-F", lambda: _case(4, 640, dead="F")),
          ("Z4-ld640-swap-dead-band", lambda: _case(4, 640, swap=True, dead="band")),
          ("Z2-ld640-single-swap", lambda: _case(2, 640, swap=True, single=True)),
          ("Z2-packed-single", lambda: _case(2, 576, single=True)),
          ("Z2-split-ld600", lambda: _case(2, 600, split=True)),
          ("Z2-split-ld600-swap-dead-F", lambda: _case(2, 600, swap=True, split=True, dead="F"))]


@pytest.mark.parametrize("ident, builder", _CASES, ids=[c[0] for c in _CASES])
def test_memory_contract(ident, builder):
    """guards intact, gaps untouched, every documented element written, inputs unchanged, NaN-fill and finite-fill runs bit-identical,
    the strided layout bit-identical to its packed sibling"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    _lib.load()
    lib = _lib.load_guided()
    bad_a, va, c, ops_ = run_case(lib, builder, finite=False)
    bad_b, vb, _, _ = run_case(lib, builder, finite=True)
    bad = ["NaN-fill run: " + b for b in bad_a] + ["finite-fill run: " + b for b in bad_b]
    assert set(va) == {o.name for o in ops_ if o.role == "out"} == {"idx", "stat"}
    for w in va:
        bits = CC._BITS[va[w].dtype]
        if not torch.equal(va[w].view(bits), vb[w].view(bits)):
            bad.append("%s: result depends on what the output held before the call" % w)
    if c.sibling is not None:
        bad_p, vp, _, _ = run_case(lib, c.sibling, finite=False)
        bad += ["packed sibling: " + b for b in bad_p]
        for w in va:
            if not torch.equal(va[w].view(CC._BITS[va[w].dtype]), vp[w].view(CC._BITS[vp[w].dtype])):
                bad.append("%s: the strided layout's result differs from the packed layout's" % w)
    figures = c.check(va, bad) if not bad_a else {}
    report("guided_memory_contract_" + ident.replace("-", "_"), violations=len(bad), **figures)
    assert not bad, "\n".join(bad)
