"""rp_triangulate (include/relpose_triangulate.h, csrc_triangulate/triangulate.hip) through the C ABI, and its wrapper, on a real MI355X.

The reference is tests/_triangulate_ref.py: the header's arithmetic in fp64, its optimal correction checked against a second route
(tests/test_triangulate_cpu.py).  Every bound is C eps32 scale(ref) with C = 8 x the worst ratio of the float32 restatement of the
kernel's arithmetic on these same inputs, measured on the CPU and asserted by
tests/test_triangulate_cpu.py::test_restatement_is_within_the_calibrated_bounds; nothing was fixed in advance.
    corrected points  scale 1                       restatement 0.89  -> C 7.12
    d2                sqrt(d2) + eps32                          2.65  -> 21.2
    phi               1                                         1.32  -> 10.6
    z1, z2            |z| / sin(phi)                            2.06  -> 16.5
    X                 |X| / sin(phi)                            1.78  -> 14.2
    cost              sqrt(c) + eps32, against the fp64 cost of the device's OWN d2 (the form of DESIGN.md 5.4)   0.0232 -> 0.186
    mean parallax     1                                         0.82  -> 6.56
    front share       the distance to the interval the fp64 share spans when the rows whose depth can carry either sign count either
                      way, over 1                               3.24  -> 25.9
Rows within a factor 4 of the at-infinity threshold in the reference may fall on either side and are left out of z and X (at most
0.78 % of a case here; the cap of 10 % is asserted).  Cases: _triangulate_ref.CASES -- the seven shapes x (no weights, depth 3, noise
1e-3 | weights with 40 % zeros, a negative and a NaN, depth 30, exact | weights, depth 300, noise 2e-2 | no weights, depth 300, exact),
10 % outliers, the pose a little off the truth, a pure rotation and a tau = 0 inside every batch that has room.  The device's own ratios
go to the test report."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _triangulate_ref as T
from tests.test_gpu_kernels import report

pytestmark = pytest.mark.gpu
IDS = ["n%d-P%d-%s-D%g-noise%g" % (n, P, "w" if wt else "now", D, nz) for n, P, wt, D, nz in T.CASES]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    _lib.load()
    return _lib.load_triangulate()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def call(lib, pose, x1, x2, w, tau, with_xc=True, fill=float("nan")):
    """rp_triangulate through ctypes on fresh, filled outputs -> (_triangulate_ref.Structure of numpy arrays, the device tensors)"""
    n, P = x1.shape[:2]
    X, aux, stat = (torch.full(s, fill, device="cuda") for s in ((n, P, 3), (n, P, 4), (n, 4)))
    xc = torch.full((n, P, 4), fill, device="cuda") if with_xc else None
    rc = lib.rp_triangulate(ptr(pose), ptr(x1), ptr(x2), ptr(w), ptr(tau), ptr(X), ptr(aux), ptr(xc), ptr(stat), P, n,
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    return T.Structure(X.cpu().numpy(), aux.cpu().numpy(), None if xc is None else xc.cpu().numpy(), stat.cpu().numpy()), (X, aux, xc, stat)


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_triangulation_against_the_reference(lib, case):
    n, P, weighted, depth, noise = case
    pose, x1, x2, w, tau = T.inputs(*case)
    ref = T.reference(*case)
    d = [dev(a) for a in (pose, x1, x2, w, tau)]
    out, t1 = call(lib, *d)
    assert all(np.isfinite(a).all() for a in out)
    r = T.ratios(out, ref, w, tau)
    share = T.share_ratio(out, ref, w, tau)
    print({k: float("%.3g" % v) for k, v in r.items()}, "share %.3g" % share)
    report("triangulate_" + IDS[T.CASES.index(case)].replace("-", "_").replace(".", "p"), share=share, **r)
    assert r["left_out"] <= 0.1 and r["flags"] == 0 and r["K"] == 0, r
    assert r["xc"] <= T.C_XC and r["d2"] <= T.C_D2 and r["phi"] <= T.C_PHI, r
    assert r["z"] <= T.C_Z and r["X"] <= T.C_X, r
    assert r["cost"] <= T.C_COST and r["par"] <= T.C_PAR and share <= T.C_SHARE, (r, share)
    # the point is the depth along the corrected ray, bit for bit; K counts the rows of positive weight
    assert np.array_equal(out.X[..., 2], out.aux[..., 0]) and np.array_equal(out.stat[:, 3], (T.clamp(w, n, P) > 0).sum(-1))
    # the degenerate problems inside the batch: zeros and (0, 0, 0, K); their neighbours are healthy
    for b in [1] * (n > 1) + [2] * (n > 2):
        assert not out.X[b].any() and not out.aux[b].any() and not out.xc[b].any() and not out.stat[b, :3].any()
    assert out.aux[0, :, 3].any() and (n < 4 or out.X[3].any())
    # bit-identical from call to call, whatever the outputs held, and with xc off
    again, t2 = call(lib, *d, fill=7.0)
    bare, t3 = call(lib, *d, with_xc=False)
    assert bare.xc is None
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(t1, t2))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(t1[:2] + t1[3:], t3[:2] + t3[3:]))


def test_weights_enter_stat_only(lib):
    """the rows are triangulated whatever their weight; with all weights 0 the rows are written and stat is 0"""
    case = (2, 257, True, 30.0, 0.0)
    pose, x1, x2, w, tau = T.inputs(*case)
    d = [dev(a) for a in (pose, x1, x2)]
    a, _ = call(lib, *d, dev(w), dev(tau))
    b, _ = call(lib, *d, None, dev(tau))
    z, _ = call(lib, *d, dev(np.where(np.arange(257) % 2 == 0, -1.0, np.nan).astype(np.float32)[None].repeat(2, 0)), dev(tau))
    for o in (b, z):
        assert np.array_equal(a.X, o.X) and np.array_equal(a.aux, o.aux) and np.array_equal(a.xc, o.xc)
    assert not z.stat.any() and b.stat[0, 3] == 257 and a.stat[0, 3] < 257 and not np.array_equal(a.stat[0], b.stat[0])


def test_wrapper_returns_the_structure(lib):
    from rel_pose_amd import triangulate
    case = (3, 5, True, 30.0, 0.0)
    pose, x1, x2, w, tau = T.inputs(*case)
    d = [dev(a) for a in (pose, x1, x2, w)]
    raw, _ = call(lib, *d, dev(tau))
    s = triangulate.triangulate(*d, tau=dev(tau), return_corrected=True)
    assert s.points.shape == (3, 5, 3) and s.depth1.shape == s.depth2.shape == s.reproj.shape == s.parallax.shape == (3, 5)
    assert s.stat.shape == (3, 4) and s.corrected.shape == (3, 5, 4)
    got = T.Structure(s.points.cpu().numpy(), torch.stack([s.depth1, s.depth2, s.reproj, s.parallax], -1).cpu().numpy(),
                      s.corrected.cpu().numpy(), s.stat.cpu().numpy())
    assert all(np.array_equal(a, b) for a, b in zip(raw, got))
    t = triangulate.triangulate(d[0][:1], d[1][:1], d[2][:1], tau=float(T.TAU))
    assert t.corrected is None and torch.equal(t.points, s.points[:1]) and t.stat[0, 3] == 5
