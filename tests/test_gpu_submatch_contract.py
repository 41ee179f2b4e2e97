"""The memory contract of rp_emm_submatch (include/relpose_submatch.h) by the rules of tests/test_gpu_memory_contract.py: every operand
between guard bands, outputs poisoned (a NaN pattern in one run, a finite pattern in the other), packed and strided q / k (the gap columns
hold NaN) -- the guards come back untouched, every documented output element is written (those of invalid and border owners included)
and nothing else, the inputs (idx among them) are unchanged, the two runs agree bit for bit, and the values are those of
tests/test_gpu_submatch.py at its bounds."""
import numpy as np
import pytest
import torch

from tests import _contract_cases as CC
from tests import _submatch_ref as S
from tests.test_gpu_kernels import report
from tests.test_gpu_memory_contract import run_case

pytestmark = pytest.mark.gpu
# (H, pad, swap, single, radius): packed rows (q | k | v, ld = 3 H 64) and strided ones; one head and three
_CONTRACT = [(3, 0, 0, 0, 2), (3, 0, 1, 1, 1), (1, 0, 1, 0, 2), (1, 0, 0, 1, 1), (3, 20, 1, 0, 2), (1, 44, 0, 1, 2), (1, 20, 0, 0, 1), (3, 44, 1, 1, 1)]
_IDS = ["H%d-pad%d-swap%d-single%d-r%d" % c for c in _CONTRACT]


def _case(H, pad, swap, single, radius):
    Z = 2
    q, k, rlse, clse = S.case_inputs("random", H)
    idx = S.table_idx(Z, H)                                        # corners, borders, one token for all, invalid entries
    ld, n = 3 * H * S.HD + pad, Z * H * S.TOK
    ops_ = [CC.inp_multi("qk", Z * S.TOK, ld, {0: torch.from_numpy(q.reshape(Z * S.TOK, -1)), H * S.HD: torch.from_numpy(k.reshape(Z * S.TOK, -1))}),
            CC.inp("rlse", torch.from_numpy(rlse).reshape(1, -1)), CC.inp("idx", torch.from_numpy(idx).reshape(1, -1), dtype=CC.I32),
            CC.flat("win", n * 4), CC.flat("quad", n * 4)]
    if not single:
        ops_.append(CC.inp("clse", torch.from_numpy(clse).reshape(1, -1)))

    def call(lib, A_, st):
        lib.rp_emm_submatch(CC.a_(A_, "qk"), CC.a_(A_, "qk", H * S.HD), CC.a_(A_, "rlse"), CC.a_(A_, "clse"), CC.a_(A_, "idx"), CC.a_(A_, "win"),
                            CC.a_(A_, "quad"), Z, H, ld, ld, S.SCALE, swap, single, radius, st)

    def check(v, errs):
        ref = S.submatch_ref(q, k, rlse, clse, idx, S.SCALE, swap, single, radius)
        win, quad = (v[n_].cpu().numpy().reshape(Z, H, S.TOK, 4) for n_ in ("win", "quad"))
        if not (np.isfinite(win).all() and np.isfinite(quad).all()):
            errs.append("non-finite output")
            return {}
        r = S.bound_ratios((win, quad), ref, radius)
        return {"wxy_ratio": CC._bound(errs, "win", r["wxy"], S.C_WXY), "wmass_ratio": CC._bound(errs, "win", r["wmass"], S.C_WMASS),
                "wvar_ratio": CC._bound(errs, "win", r["wvar"], S.C_WVAR), "curv_ratio": CC._bound(errs, "quad", r["curv"], S.C_CURV),
                "pxy_ratio": CC._bound(errs, "quad", r["pxy"], S.C_PXY)}
    return CC.Case(ops_, call, check)


@pytest.mark.parametrize("H,pad,swap,single,radius", _CONTRACT, ids=_IDS)
def test_memory_contract(H, pad, swap, single, radius):
    """guards intact, every documented element written and nothing else, inputs unchanged, NaN-fill and finite-fill runs bit-identical"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    _lib.load()
    lib = _lib.load_submatch()
    builder = lambda: _case(H, pad, swap, single, radius)          # noqa: E731
    bad_a, va, c, ops_ = run_case(lib, builder, finite=False)
    bad_b, vb, _, _ = run_case(lib, builder, finite=True)
    bad = ["NaN-fill run: " + b for b in bad_a] + ["finite-fill run: " + b for b in bad_b]
    assert set(va) == {o.name for o in ops_ if o.role == "out"} == {"win", "quad"}
    for k in va:
        bits = CC._BITS[va[k].dtype]
        if not torch.equal(va[k].view(bits), vb[k].view(bits)):
            bad.append("%s: result depends on what the output held before the call" % k)
    errs = c.check(va, bad) if not bad_a else {}
    report("submatch_memory_contract_" + _IDS[_CONTRACT.index((H, pad, swap, single, radius))].replace("-", "_"), violations=len(bad), **errs)
    assert not bad, "\n".join(bad)
