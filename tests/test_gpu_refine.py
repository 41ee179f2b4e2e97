"""rp_refine_pose (include/relpose_refine.h, csrc_refine/refine_pose.hip) and what is built on it, on a real MI355X.

The reference is tests/_refine_ref.py: refine_ref, the iteration of the header in fp64.

Inputs (parity_inputs): exact synthetic scenes with Gaussian noise of 1e-3 on both images, rounded to float32 (the reference sees the
same numbers), starts 0.03 rad away from the true pose in R and in the direction of t, tau = 0.02, with random weights in 0.05 .. 1 and
without.

Bounds.  A step solves the 5 x 5 normal equations; a relative perturbation eps of H and g moves its solution by about eps kappa, kappa the
condition number of the diagonally scaled H (the scaling is part of the algorithm).  Every compared problem is therefore bounded by
    C eps32 kappa(reference),
kappa taken at the start (one step) or at the output pose (converged), C = 8 x the largest ratio err / (eps32 kappa) that the numpy
float32 restatement of the kernel's arithmetic (_refine_ref.refine_f32: the same statements on float32 numbers, numpy's pairwise sums
instead of the kernel's per-thread / wave / LDS tree) shows on these same inputs; the factor 8 covers the different order of the sums.
Measured with the restatement on the CPU over all CASES, weighted and not (tests/test_refine_cpu.py repeats a subset):
    one step    pose 0.126, E 0.125 (P = 8, n = 130; 0.01 .. 0.11 elsewhere)                                        -> C_STEP = 1.01
    converged   pose 8.2, E 8.1 (P = 8, n = 130, kappa up to 8e3; 0.47 at P = 5, 0.006 .. 0.7 for P >= 9)          -> C_CONV = 66
The converged ratio is larger than the one-step ratio because a float32 trajectory stops where cost differences drop below the rounding
of the cost (a step is accepted only if the cost is strictly lower), which is earlier than where fp64 stops.
Only problems whose REFERENCE decides clearly are compared: one step -- its first step is accepted and lowers the cost by at least 10 %
(so accept / reject cannot flip on rounding); converged (iters = 12) -- its last accepted step is below 1e-7 and the cost moved by less
than 1e-6 relative over the last two iterations.  At least 80 % of every case's problems must qualify (measured: 99 .. 100 % one step,
95 .. 100 % converged; parity_inputs says how the five-point scenes are chosen).
Costs: c = sum w tau^2 log1p(s^2 / tau^2) / sum w with s of absolute rounding error ~eps32 (the terms of x2^T E x1 are of order 1), so c
moves by about 2 s ds + ds^2: |c - c_fp64(same pose)| <= C_COST eps32 (sqrt(c) + eps32), C_COST = 8 x the restatement's largest ratio
3.85 (the exact fit of five points, c ~ eps32^2; 0.01 .. 1.3 elsewhere) -> 31.
Weights at iters = 0: the form test_gpu_eightpoint.py derives, |w_out - w_ref| / w0 <= C_W eps32 / tau -- its constant 0.65 / sqrt(den)
grows where den is small --, C_W = 8 x the restatement's largest ratio 4.1 on these inputs (P = 513; 0.23 .. 1.4 elsewhere) -> 33.
The GPU's own worst ratios go to the test report (tests/test_gpu_kernels.py: report)."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import _contract_cases as CC
from tests import _refine_ref as F
from tests.test_gpu_kernels import report
from tests.test_gpu_memory_contract import _bf16_configuration, _model, run_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = 256                                        # threads of the kernel's workgroup
C_STEP, C_CONV, C_COST, C_W = 1.01, 66.0, 31.0, 33.0          # see the module docstring
TAU = 0.02
CASES = [(5, 130), (8, 130), (9, 3), (NT - 1, 1), (NT, 3), (NT + 1, 1), (2 * NT + 1, 3), (1728, 1)]
_IDS = dict(argvalues=[(P, n, wt) for P, n in CASES for wt in (False, True)],
            ids=["P%d-n%d-%s" % (P, n, "weighted" if wt else "ones") for P, n in CASES for wt in (False, True)])


@pytest.fixture(scope="module")
def rf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, refine
    _lib.load()
    _lib.load_refine()
    return refine


@functools.lru_cache(maxsize=None)
def parity_inputs(P, n, weighted):
    """float32 numpy: start poses [n,7], x1, x2 [n,P,2], weights [n,P] or None (see the module docstring)"""
    m = 2 * n if P == 5 else n                   # the minimal problem: twice as many candidates, see below
    x1, x2, _, truth = F.scenes_with_pose(m, P, seed=21)
    rng = np.random.default_rng(100 * P + n)
    x1 = (x1 + 1e-3 * rng.standard_normal(x1.shape)).astype(np.float32)
    x2 = (x2 + 1e-3 * rng.standard_normal(x2.shape)).astype(np.float32)
    start = F.perturbed(truth, rng).astype(np.float32)
    w = rng.uniform(0.05, 1.0, (m, P)).astype(np.float32) if weighted else None
    if m > n:
        # Five points leave no redundancy: about a quarter of random five-point scenes lie so close to a degenerate configuration
        # (kappa at the start above 1e4 .. 1e7) that the REFERENCE alternates between accepted and rejected steps for more than 12
        # iterations, and the converged share of the raw scenes is 72 %.  The case keeps the better-conditioned half of the candidates,
        # ranked by the reference's kappa at the start without weights -- a property of the inputs, not of the code under test.
        keep = np.sort(np.argsort(F.refine_ref(start, x1, x2, None, TAU, 1).kappa0, kind="stable")[:n])
        start, x1, x2, w = start[keep], x1[keep], x2[keep], None if w is None else w[keep]
    return start, x1, x2, w


@functools.lru_cache(maxsize=None)
def reference(P, n, weighted, iters):
    return F.refine_ref(*parity_inputs(P, n, weighted), TAU, iters)


def clear_first_step(ref):
    """problems whose reference accepted its one step with a cost at most 0.9 of the start's"""
    return (ref.stat[:, 2] == 1) & (ref.stat[:, 1] <= 0.9 * ref.stat[:, 0])


def converged(ref):
    """problems whose reference ended with an accepted step below 1e-7 and a cost that moved by less than 1e-6 relative in two iterations"""
    ok = np.zeros(len(ref.trace), bool)
    for b, tr in enumerate(ref.trace):
        # (+ 1e-30: s carries an absolute rounding error of about eps64 even in the reference, so a cost below eps64^2 ~ 5e-32 -- the exact
        # fit of five points -- is zero, and its relative changes mean nothing)
        ok[b] = len(tr) >= 3 and 0 < ref.stat[b, 3] < 1e-7 and abs(tr[-3][0] - tr[-1][0]) <= 1e-6 * tr[-1][0] + 1e-30
    return ok


def pose_ratio(pose, E, ref, kappa):
    """largest |pose - pose_ref| and |E - E_ref| entry per problem over eps32 kappa"""
    scale = F.EPS32 * kappa
    pose = np.asarray(pose, np.float64)
    d = np.abs(pose - ref.pose).max(-1)
    # q and -q are one rotation and the output has w >= 0: where the reference's |w| < 1e-3 rounding decides the sign of the other three
    flipped = np.concatenate([pose[:, :3], -pose[:, 3:]], -1)
    d = np.where(np.abs(ref.pose[:, 6]) < 1e-3, np.minimum(d, np.abs(flipped - ref.pose).max(-1)), d)
    return d / scale, np.abs(np.asarray(E, np.float64).reshape(-1, 9) - ref.E.reshape(-1, 9)).max(-1) / scale


def cost_ratio(stat, pose_in, pose_out, x1, x2, w, tau=TAU):
    """|c0 - c64(pose_in)|, |c - c64(pose_out)| over eps32 (sqrt(c64) + eps32), the larger per problem"""
    out = []
    for c, p in ((stat[:, 0], pose_in), (stat[:, 1], pose_out)):
        c64 = F.cost64(p, x1, x2, w, tau)
        out.append(np.abs(np.asarray(c, np.float64) - c64) / (F.EPS32 * (np.sqrt(c64) + F.EPS32)))
    return np.maximum(*out)


def weight_ratio(wo, pose, x1, x2, w, tau=TAU):
    """|w_out - w64(pose)| / w0 over eps32 / tau"""
    n, P = x1.shape[:2]
    w0 = np.ones((n, P)) if w is None else np.asarray(w, np.float64)
    want = np.stack([w0[b] / (1 + F.residual(F._frame(*_unit_pose(pose[b]))[0], x1[b].astype(np.float64), x2[b].astype(np.float64))[0] ** 2
                              / tau ** 2) for b in range(n)])
    return np.abs(np.asarray(wo, np.float64) - want) / w0 / (F.EPS32 / tau)


def _unit_pose(p):
    p = np.asarray(p, np.float64)
    return p[:3] / np.linalg.norm(p[:3]), p[3:] / np.linalg.norm(p[3:])


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


def _call(rf, P, n, weighted, iters, **kw):
    start, x1, x2, w = parity_inputs(P, n, weighted)
    return rf.refine_pose(dev(start), dev(x1), dev(x2), dev(w), tau=TAU, iters=iters, return_weights=True, **kw)


@pytest.mark.parametrize("P,n,weighted", **_IDS)
def test_one_step_parity(rf, P, n, weighted):
    start, x1, x2, w = parity_inputs(P, n, weighted)
    ref = reference(P, n, weighted, 1)
    ok = clear_first_step(ref)
    assert ok.mean() >= 0.8, ok.mean()
    out = _call(rf, P, n, weighted, 1)
    assert out.pose.shape == (n, 7) and out.E.shape == (n, 3, 3) and out.stat.shape == (n, 4) and out.weights.shape == (n, P)
    pr, er = pose_ratio(host(out.pose), host(out.E), ref, ref.kappa0)
    cr = cost_ratio(host(out.stat), start, host(out.pose), x1, x2, w)
    tag = "refine_step_P%d_n%d_%s" % (P, n, "w" if weighted else "ones")
    report(tag, pose_ratio=float(pr[ok].max()), E_ratio=float(er[ok].max()), cost_ratio=float(cr.max()), kappa_max=float(ref.kappa0[ok].max()),
           share=float(ok.mean()))
    print(tag, "pose %.3g E %.3g (C %.3g), cost %.3g (C %.3g), share %.2f" % (pr[ok].max(), er[ok].max(), C_STEP, cr.max(), C_COST, ok.mean()))
    assert float(pr[ok].max()) <= C_STEP and float(er[ok].max()) <= C_STEP
    assert float(cr.max()) <= C_COST
    st = host(out.stat)
    assert bool((st[:, 1] <= st[:, 0]).all())
    assert bool((st[ok, 2] == 1).all()) and bool((st[ok, 3] > 0).all())
    # E is [t]x R of the output pose, the pose is normalised with q.w >= 0
    p = host(out.pose)
    assert np.abs(np.linalg.norm(p[:, :3], axis=-1) - 1).max() < 1e-5 and np.abs(np.linalg.norm(p[:, 3:], axis=-1) - 1).max() < 1e-5
    assert bool((p[:, 6] >= 0).all())
    Ep = np.stack([F._frame(*_unit_pose(p[b]))[0] for b in range(n)])
    assert np.abs(Ep - host(out.E)).max() < 1e-5


@pytest.mark.parametrize("P,n,weighted", **_IDS)
def test_converged_parity(rf, P, n, weighted):
    start, x1, x2, w = parity_inputs(P, n, weighted)
    ref = reference(P, n, weighted, 12)
    ok = converged(ref)
    assert ok.mean() >= 0.8, ok.mean()
    out = _call(rf, P, n, weighted, 12)
    pr, er = pose_ratio(host(out.pose), host(out.E), ref, ref.kappa)
    cr = cost_ratio(host(out.stat), start, host(out.pose), x1, x2, w)
    tag = "refine_converged_P%d_n%d_%s" % (P, n, "w" if weighted else "ones")
    report(tag, pose_ratio=float(pr[ok].max()), E_ratio=float(er[ok].max()), cost_ratio=float(cr.max()), kappa_max=float(ref.kappa[ok].max()),
           share=float(ok.mean()))
    print(tag, "pose %.3g E %.3g (C %.3g), cost %.3g (C %.3g), share %.2f" % (pr[ok].max(), er[ok].max(), C_CONV, cr.max(), C_COST, ok.mean()))
    assert float(pr[ok].max()) <= C_CONV and float(er[ok].max()) <= C_CONV
    assert float(cr.max()) <= C_COST
    st = host(out.stat)
    assert bool((st[:, 1] <= st[:, 0]).all())                   # exactly: the kernel accepts only strict decreases in its own arithmetic


# ------------------------------------------------------------------------------------------------ wide baselines
WIDE_CASES = [(8, 24), (64, 6)]
_WIDE_IDS = dict(argvalues=[(k, P, n, wt) for k in ("beyond120", "half_turn") for P, n in WIDE_CASES for wt in (False, True)],
                 ids=["%s-P%d-n%d-%s" % (k, P, n, "weighted" if wt else "ones") for k in ("beyond120", "half_turn") for P, n in WIDE_CASES
                      for wt in (False, True)])


@functools.lru_cache(maxsize=None)
def wide_inputs(kind, P, n, weighted):
    """parity_inputs on F.wide_scenes: rotations of 2.2 .. 3.1 rad ("beyond120") or of exactly pi ("half_turn", q.w = 0 at the truth, so
    the perturbed starts lie on both sides of w = 0); the same noise, start perturbation and weights"""
    x1, x2, _, truth = F.wide_scenes(n, P, 21, kind)
    rng = np.random.default_rng(100 * P + n)
    x1 = (x1 + 1e-3 * rng.standard_normal(x1.shape)).astype(np.float32)
    x2 = (x2 + 1e-3 * rng.standard_normal(x2.shape)).astype(np.float32)
    start = F.perturbed(truth, rng).astype(np.float32)
    w = rng.uniform(0.05, 1.0, (n, P)).astype(np.float32) if weighted else None
    return start, x1, x2, w


@functools.lru_cache(maxsize=None)
def wide_reference(kind, P, n, weighted, iters):
    return F.refine_ref(*wide_inputs(kind, P, n, weighted), TAU, iters)


@pytest.mark.parametrize("kind,P,n,weighted", **_WIDE_IDS)
def test_one_step_parity_wide_baseline(rf, kind, P, n, weighted):
    """test_one_step_parity beyond 120 degrees and at a half-turn, the same bounds and constants (the restatement's largest ratio on these
    inputs: pose 0.33, E 0.34, cost 0.72 -- single scenes
    stand out, image coordinates reach 3 here against 0.55 in `scenes`; tests/test_refine_cpu.py); the reference accepts its first step in every problem"""
    start, x1, x2, w = wide_inputs(kind, P, n, weighted)
    ref = wide_reference(kind, P, n, weighted, 1)
    ok = clear_first_step(ref)
    assert ok.mean() >= 0.8, ok.mean()
    out = rf.refine_pose(dev(start), dev(x1), dev(x2), dev(w), tau=TAU, iters=1, return_weights=True)
    pr, er = pose_ratio(host(out.pose), host(out.E), ref, ref.kappa0)
    cr = cost_ratio(host(out.stat), start, host(out.pose), x1, x2, w)
    tag = "refine_step_%s_P%d_n%d_%s" % (kind, P, n, "w" if weighted else "ones")
    report(tag, pose_ratio=float(pr[ok].max()), E_ratio=float(er[ok].max()), cost_ratio=float(cr.max()), kappa_max=float(ref.kappa0[ok].max()),
           share=float(ok.mean()))
    print(tag, "pose %.3g E %.3g (C %.3g), cost %.3g (C %.3g), share %.2f" % (pr[ok].max(), er[ok].max(), C_STEP, cr.max(), C_COST, ok.mean()))
    assert float(pr[ok].max()) <= C_STEP and float(er[ok].max()) <= C_STEP
    assert float(cr.max()) <= C_COST
    st, p = host(out.stat), host(out.pose)
    assert bool((st[:, 1] <= st[:, 0]).all())
    assert bool((st[ok, 2] == 1).all()) and bool((st[ok, 3] > 0).all())
    assert np.abs(np.linalg.norm(p[:, :3], axis=-1) - 1).max() < 1e-5 and np.abs(np.linalg.norm(p[:, 3:], axis=-1) - 1).max() < 1e-5
    assert bool((p[:, 6] >= 0).all())
    Ep = np.stack([F._frame(*_unit_pose(p[b]))[0] for b in range(n)])
    assert np.abs(Ep - host(out.E)).max() < 1e-5


@pytest.mark.parametrize("kind,P,n,weighted", **_WIDE_IDS)
def test_converged_parity_wide_baseline(rf, kind, P, n, weighted):
    """test_converged_parity on the same inputs (the restatement's largest ratio: pose 1.37, E 1.39, at P = 8)"""
    start, x1, x2, w = wide_inputs(kind, P, n, weighted)
    ref = wide_reference(kind, P, n, weighted, 12)
    ok = converged(ref)
    assert ok.mean() >= 0.8, ok.mean()
    out = rf.refine_pose(dev(start), dev(x1), dev(x2), dev(w), tau=TAU, iters=12, return_weights=True)
    pr, er = pose_ratio(host(out.pose), host(out.E), ref, ref.kappa)
    cr = cost_ratio(host(out.stat), start, host(out.pose), x1, x2, w)
    tag = "refine_converged_%s_P%d_n%d_%s" % (kind, P, n, "w" if weighted else "ones")
    report(tag, pose_ratio=float(pr[ok].max()), E_ratio=float(er[ok].max()), cost_ratio=float(cr.max()), kappa_max=float(ref.kappa[ok].max()),
           share=float(ok.mean()))
    print(tag, "pose %.3g E %.3g (C %.3g), cost %.3g (C %.3g), share %.2f" % (pr[ok].max(), er[ok].max(), C_CONV, cr.max(), C_COST, ok.mean()))
    assert float(pr[ok].max()) <= C_CONV and float(er[ok].max()) <= C_CONV
    assert float(cr.max()) <= C_COST
    st, p = host(out.stat), host(out.pose)
    assert bool((st[:, 1] <= st[:, 0]).all())
    assert bool((p[:, 6] >= 0).all())


@functools.lru_cache(maxsize=None)
def chain_inputs():
    """three "beyond120" scenes of 300 points: Gaussian noise of 1e-3 on both images, 30 of x2 replaced by uniform noise; float32"""
    x1, x2, _, truth = F.wide_scenes(3, 300, 31, "beyond120")
    rng = np.random.default_rng(31)
    x1 = x1 + 1e-3 * rng.standard_normal(x1.shape)
    x2 = x2 + 1e-3 * rng.standard_normal(x2.shape)
    for b in range(3):
        bad = rng.permutation(300)[:30]
        x2[b, bad] = rng.uniform(-0.6, 0.6, (30, 2))
    return x1.astype(np.float32), x2.astype(np.float32), truth


def pose_distance(pose, truth):
    """(rotation angle, angle between the directions of t) in degrees per problem"""
    out = np.empty((len(pose), 2))
    for b in range(len(pose)):
        (Ra, ta), (Rb, tb) = F.pose_matrix(pose[b]), F.pose_matrix(truth[b])
        out[b] = F.rotation_angle(Ra, Rb), F.direction_angle(ta, tb)
    return out


def test_chain_beyond_120_degrees(rf):
    """eight_point(iters = 4) -> pose_from_essential -> refine_pose(12) on noisy scenes whose rotation is 2.2 .. 3.1 rad: the pose lands within
    twice the distance from the truth that the fp64 chain (eight_point_ref -> decode_pose -> refine_ref) reaches, in R and in the direction
    of t; the fp64 chain itself is within 2 degrees of the truth (noise of 1e-3 and 10 % outliers)"""
    from tests import _eightpoint_ref as R8
    from rel_pose_amd import _lib, eightpoint, geom
    _lib.load_eightpoint()
    x1, x2, truth = chain_inputs()
    tau = np.full(3, TAU, np.float32)
    Er, _, _ = R8.eight_point_ref(x1, x2, None, tau, 4)
    p0 = np.stack([F.decode_pose(Er[b], x1[b], x2[b]) for b in range(3)])
    want = pose_distance(F.refine_ref(p0, x1, x2, None, TAU, 12).pose, truth)
    assert want.max() < 2.0, want                                 # the reference chain finds the pose (0.33 degrees in R, 1.15 in t)
    e = eightpoint.eight_point(dev(x1), dev(x2), None, tau=dev(tau), iters=4)
    pose, count = geom.pose_from_essential(e.E, dev(x1), dev(x2))
    out = rf.refine_pose(pose, dev(x1), dev(x2), None, tau=TAU, iters=12)
    got = pose_distance(host(out.pose), truth)
    report("chain_beyond120", rot_deg=float(got[:, 0].max()), t_deg=float(got[:, 1].max()), ref_rot_deg=float(want[:, 0].max()),
           ref_t_deg=float(want[:, 1].max()), in_front_min=float(count.min()))
    print("chain: got", got, "fp64 chain", want)
    assert bool((got <= 2 * want).all()), (got, want)
    assert int(count.min()) >= 250                                # (30 of the 300 are outliers)


@pytest.mark.parametrize("P,n,weighted", **_IDS)
def test_scorer_and_repeatability(rf, P, n, weighted):
    from rel_pose_amd import _lib
    start, x1, x2, w = parity_inputs(P, n, weighted)
    out = _call(rf, P, n, weighted, 0)
    st, p = host(out.stat), host(out.pose)
    want = start.astype(np.float64)
    want = np.concatenate([want[:, :3] / np.linalg.norm(want[:, :3], axis=-1, keepdims=True),
                           want[:, 3:] / np.linalg.norm(want[:, 3:], axis=-1, keepdims=True)], -1)
    want[:, 3:] *= np.where(want[:, 6:] < 0, -1.0, 1.0)
    assert np.abs(p - want).max() < 4 * F.EPS32                   # the normalised start
    assert np.array_equal(st[:, 0], st[:, 1]) and not st[:, 2:].any()
    cr = cost_ratio(st, start, start, x1, x2, w)
    wr = weight_ratio(host(out.weights), start, x1, x2, w)
    tag = "refine_score_P%d_n%d_%s" % (P, n, "w" if weighted else "ones")
    report(tag, cost_ratio=float(cr.max()), w_ratio=float(wr.max()))
    print(tag, "cost %.3g (C %.3g), weights %.3g (C_W %.3g)" % (cr.max(), C_COST, wr.max(), C_W))
    assert float(cr.max()) <= C_COST and float(wr.max()) <= C_W
    # two calls: the same bits; pose aliasing pose0: the same bits
    for iters in (0, 3):
        a, b = _call(rf, P, n, weighted, iters), _call(rf, P, n, weighted, iters)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        lib = _lib.load_refine()
        pose = dev(start)
        E, stat, wo = torch.empty(n, 9, device="cuda"), torch.empty(n, 4, device="cuda"), torch.empty(n, P, device="cuda")
        Pv = ctypes.c_void_p
        ptr = lambda t: None if t is None else Pv(t.data_ptr())      # noqa: E731
        d1, d2, dw, dtau = dev(x1), dev(x2), dev(w), torch.full((n,), TAU, device="cuda")
        lib.rp_refine_pose(ptr(pose), ptr(d1), ptr(d2), ptr(dw), ptr(dtau), ptr(pose), ptr(E), ptr(stat), ptr(wo), P, iters, n,
                           Pv(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(pose, a.pose) and torch.equal(E.view(n, 3, 3), a.E) and torch.equal(stat, a.stat) and torch.equal(wo, a.weights)
    assert rf.refine_pose(dev(start), dev(x1), dev(x2), dev(w), tau=TAU, iters=1).weights is None
    # tau as a tensor is the same call
    t = torch.full((n,), TAU, device="cuda")
    assert all(torch.equal(u, v) for u, v in zip(_call(rf, P, n, weighted, 0), rf.refine_pose(dev(start), dev(x1), dev(x2), dev(w), tau=t, iters=0,
                                                                                               return_weights=True)))


def test_degenerate_problems_in_a_batch(rf):
    """four positive weights, all-zero weights and a zero t0 between healthy problems: exact documented outputs, and the healthy
    neighbours bit-identical to a call without the degenerate ones"""
    P = 300
    x1, x2, _, truth = F.scenes_with_pose(6, P, seed=22)
    rng = np.random.default_rng(3)
    x1, x2 = x1.astype(np.float32), x2.astype(np.float32)
    w0 = rng.uniform(0.05, 1.0, (6, P)).astype(np.float32)
    start = F.perturbed(truth, rng).astype(np.float32) * np.float32(1.7)                 # (not normalised: the copy must be bit for bit)
    w0[1] = 0
    w0[1, [3, 255, 256, 299]] = 0.5
    w0[1, 7] = -1.0                                               # negative: counts as 0
    w0[3] = 0
    start[5, :3] = 0
    for iters in (0, 3):
        out = rf.refine_pose(dev(start), dev(x1), dev(x2), dev(w0), tau=TAU, iters=iters, return_weights=True)
        pose, E, stat, wo = (t.cpu().numpy() for t in out)
        for b in (1, 3, 5):
            assert np.array_equal(pose[b], start[b]) and not E[b].any() and not stat[b].any(), (b, pose[b], E[b], stat[b])
            assert np.array_equal(wo[b], np.maximum(w0[b], 0))
        assert all(np.isfinite(a).all() for a in (pose, E, stat, wo))
        keep = [0, 2, 4]
        alone = rf.refine_pose(dev(start[keep]), dev(x1[keep]), dev(x2[keep]), dev(w0[keep]), tau=TAU, iters=iters, return_weights=True)
        assert all(torch.equal(p[keep], q) for p, q in zip(out, alone))
        assert np.allclose(np.linalg.norm(E[keep].reshape(3, 9), axis=-1), np.sqrt(2), atol=1e-5)


# ------------------------------------------------------------------------------------------------ memory contract
def _refine_case(P, with_w, with_w_out, iters, n=3):
    """one guarded rp_refine_pose call (tests/_contract_cases.py's Case, kept out of its table: that table is the main header's)"""
    start, x1, x2, w = parity_inputs.__wrapped__(P, n, True)
    tau = np.full(n, TAU, np.float32)
    ops_ = [CC.inp("pose0", torch.from_numpy(start).reshape(1, -1)), CC.inp("x1", torch.from_numpy(x1).reshape(1, -1)),
            CC.inp("x2", torch.from_numpy(x2).reshape(1, -1)), CC.inp("tau", torch.from_numpy(tau).reshape(1, -1)),
            CC.flat("pose", n * 7), CC.flat("E", n * 9), CC.flat("stat", n * 4)]
    if with_w:
        ops_.append(CC.inp("w", torch.from_numpy(w).reshape(1, -1)))
    if with_w_out:
        ops_.append(CC.flat("w_out", n * P))

    def call(lib, A_, st):
        lib.rp_refine_pose(CC.a_(A_, "pose0"), CC.a_(A_, "x1"), CC.a_(A_, "x2"), CC.a_(A_, "w"), CC.a_(A_, "tau"), CC.a_(A_, "pose"),
                           CC.a_(A_, "E"), CC.a_(A_, "stat"), CC.a_(A_, "w_out"), P, iters, n, st)

    def check(v, errs):
        e = {}
        if not all(bool(torch.isfinite(v[k]).all()) for k in v):
            errs.append("non-finite output")
        pose, stat = host(v["pose"]).reshape(n, 7), host(v["stat"]).reshape(n, 4)
        ww = w if with_w else None
        e["cost_ratio"] = CC._bound(errs, "stat", float(cost_ratio(stat, start, pose, x1, x2, ww).max()), C_COST)
        if with_w_out:
            e["w_ratio"] = CC._bound(errs, "w_out", float(weight_ratio(host(v["w_out"]).reshape(n, P), pose, x1, x2, ww).max()), C_W)
        return e
    return CC.Case(ops_, call, check)


_CONTRACT = [(P, ww, wo, it) for P in (5, NT + 1, 1728) for ww in (False, True) for wo in (False, True) for it in (0, 3)]


@pytest.mark.parametrize("P,with_w,with_w_out,iters", _CONTRACT,
                         ids=["P%d-%s-%s-iters%d" % (P, "w" if a else "now", "wout" if b else "nowout", i) for P, a, b, i in _CONTRACT])
def test_memory_contract(rf, P, with_w, with_w_out, iters):
    """guards intact, every documented element written and nothing else, inputs unchanged, NaN-fill and finite-fill runs bit-identical"""
    from rel_pose_amd import _lib
    lib = _lib.load_refine()
    builder = lambda: _refine_case(P, with_w, with_w_out, iters)      # noqa: E731
    bad_a, va, c, ops_ = run_case(lib, builder, finite=False)
    bad_b, vb, _, _ = run_case(lib, builder, finite=True)
    bad = ["NaN-fill run: " + b for b in bad_a] + ["finite-fill run: " + b for b in bad_b]
    assert set(va) == {o.name for o in ops_ if o.role == "out"} == {"pose", "E", "stat"} | ({"w_out"} if with_w_out else set())
    for k in va:
        bits = CC._BITS[va[k].dtype]
        if not torch.equal(va[k].view(bits), vb[k].view(bits)):
            bad.append("%s: result depends on what the output held before the call" % k)
    errs = c.check(va, bad) if not bad_a else {}
    report("refine_memory_contract_P%d_w%d_wout%d_iters%d" % (P, with_w, with_w_out, iters), violations=len(bad), **errs)
    assert not bad, "\n".join(bad)


def test_too_many_points_are_refused_with_outputs_untouched(rf):
    from rel_pose_amd import _lib
    n, P = 2, _lib.REFINE_MAX_P + 1
    x = torch.rand(n, P, 2, device="cuda")
    p0 = torch.tensor([[1.0, 0, 0, 0, 0, 0, 1]] * n, device="cuda")
    with pytest.raises(RuntimeError, match=r"rel_pose_amd: rp_refine_pose failed: unsupported \(RP error -4\)"):
        rf.refine_pose(p0, x, x.clone())
    lib = _lib.load_refine()
    pose, E, stat, wo = (torch.full(s, -7.0, device="cuda") for s in ((n, 7), (n, 9), (n, 4), (n, P)))
    tau = torch.full((n,), TAU, device="cuda")
    Pv = ctypes.c_void_p
    with pytest.raises(RuntimeError, match=r"unsupported \(RP error -4\)"):
        lib.rp_refine_pose(Pv(p0.data_ptr()), Pv(x.data_ptr()), Pv(x.data_ptr()), None, Pv(tau.data_ptr()), Pv(pose.data_ptr()),
                           Pv(E.data_ptr()), Pv(stat.data_ptr()), Pv(wo.data_ptr()), P, 0, n, Pv(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in (pose, E, stat, wo))                               # nothing ran
    with pytest.raises(ValueError):
        rf.refine_pose(p0, x[:, :64], x[:, :63])
    with pytest.raises(ValueError, match="pose0"):
        rf.refine_pose(p0[:1], x[:, :64].contiguous(), x[:, :64].contiguous())


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture
def repeatable_cnn():
    """as in tests/test_gpu_readout.py: a bit-for-bit comparison of two runs from IMAGES asks MIOpen for its repeatable solvers"""
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    yield
    torch.backends.cudnn.deterministic = keep


def test_model_refined_pose_from_matches(rf, repeatable_cnn):
    from oracle import relpose_oracle as O
    from rel_pose_amd import eightpoint, geom
    from rel_pose_amd.se3 import SE3
    m = _model().eval()
    B = 2
    images = O.synthetic_images(B, 384, 384, key=78).cuda()
    Gs = SE3(torch.tensor([0, 0, 0, 0, 0, 0, 1.0]).repeat(B, 2, 1).cuda())
    intr = torch.tensor([[0.9 * 384, 0.8 * 384, 192.0, 192.0]]).repeat(B, 2, 1).contiguous().cuda()
    keep_intr = intr.clone()

    def forward():
        with torch.no_grad():
            return m(images, Gs, intrinsics=intr.clone())[0].data.clone()
    forward()                                                    # (warm-up: first calls load code objects and pick solvers)
    before, state = forward(), {k: v.clone() for k, v in m.state_dict().items()}
    buffers = {k: v.clone() for k, v in m.named_buffers()}
    rp = m.refined_pose_from_matches(images, intr)
    assert torch.equal(intr, keep_intr)
    mp = m.pose_from_matches(images, intr)
    assert type(rp.initial) is type(mp) and all(torch.equal(a, b) for a, b in zip(rp.initial, mp))
    # the chain of the public pieces, bit for bit
    corr = m.correspondences(images)
    x1, x2, w = eightpoint.assemble_matches(corr, intr, (384, 384))
    tau = eightpoint.default_tau(intr, (384, 384))
    e = eightpoint.eight_point(x1, x2, w, tau=tau, iters=4, return_weights=True)
    pose, _ = geom.pose_from_essential(e.E, x1, x2)
    r = rf.refine_pose(pose, x1, x2, w, tau=tau, iters=10, return_weights=True)
    for got, want in zip(rp[:4], r):
        assert torch.equal(got, want)
    assert rp.pose.shape == (B, 7) and rp.E.shape == (B, 3, 3) and rp.stat.shape == (B, 4) and rp.weights.shape == (B, 1728)
    assert bool(torch.isfinite(rp.pose).all()) and bool((rp.pose[:, 6] >= 0).all())
    assert float((rp.pose[:, :3].norm(dim=-1) - 1).abs().max()) < 1e-5 and float((rp.pose[:, 3:].norm(dim=-1) - 1).abs().max()) < 1e-5
    assert bool((rp.stat[:, 1] <= rp.stat[:, 0]).all())
    report("refine_model_matches", cost_start=float(rp.stat[:, 0].max()), cost_end=float(rp.stat[:, 1].max()), accepted=float(rp.stat[:, 2].min()))
    # module state
    assert not m.training and all(not mod.training for mod in m.modules())
    after = m.state_dict()
    assert set(after) == set(state) and all(torch.equal(after[k], state[k]) for k in state)
    assert all(torch.equal(v, buffers[k]) for k, v in m.named_buffers())
    assert torch.equal(forward(), before)
    assert all(p.grad is None for p in m.parameters())


def test_model_refusals(rf):
    images = torch.zeros(1, 2, 3, 64, 64, device="cuda")
    intr = torch.ones(1, 2, 4, device="cuda")
    m = _model()
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.refined_pose_from_matches(images, intr)
    m.eval()
    _bf16_configuration(True)
    try:
        with pytest.raises(NotImplementedError):
            m.refined_pose_from_matches(torch.zeros(1, 2, 3, 384, 384, device="cuda"), intr)
    finally:
        _bf16_configuration(False)
    with pytest.raises(ValueError, match="noess"):
        _model(noess="1").eval().refined_pose_from_matches(torch.zeros(1, 2, 3, 384, 384, device="cuda"), intr)


def test_demo_refine_flag(capsys, repeatable_cnn):
    sys.path.insert(0, ROOT)
    import demo
    g = os.path.join(ROOT, "tests", "golden", "demo")
    argv = ["--img1", os.path.join(g, "matterport_1.png"), "--img2", os.path.join(g, "matterport_2.png")]
    torch.manual_seed(5)
    plain = demo.main(argv + ["--eight_point"])
    out_plain = capsys.readouterr().out
    torch.manual_seed(5)
    flagged = demo.main(argv + ["--eight_point", "--refine", "10"])
    out_flagged = capsys.readouterr().out
    assert plain.tobytes() == flagged.tobytes()
    assert "refined" not in out_plain and out_flagged.startswith(out_plain)
    extra = out_flagged[len(out_plain):].splitlines()
    assert len(extra) == 2 and extra[0].startswith("refined pose ") and extra[1].startswith("mean robust Sampson cost")
    number = r"-?\d+\.\d+(?:e[-+]\d+)?"
    numbers = [float(t) for t in re.findall(number, extra[0])]
    assert len(numbers) == 7 + 2 and all(np.isfinite(numbers))
    pose, angles = np.array(numbers[:7]), numbers[7:]
    assert abs(np.linalg.norm(pose[:3]) - 1) < 1e-4 and abs(np.linalg.norm(pose[3:]) - 1) < 1e-4 and pose[6] >= 0
    assert 0 <= angles[0] <= 180.001 and 0 <= angles[1] <= 180.001
    costs = [float(t) for t in re.findall(number, extra[1])]
    assert len(costs) == 3 and all(np.isfinite(costs)) and all(c >= 0 for c in costs)
    assert costs[2] <= costs[1] * (1 + 1e-4)                      # (printed to seven digits; the scorer normalises the pose once more)
    with pytest.raises(SystemExit):
        demo.main(argv + ["--refine", "10"])
    capsys.readouterr()
