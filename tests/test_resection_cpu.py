"""The resection library (include/relpose_resection.h, librelpose_resection.so, rel_pose_amd/resection.py) as far as it goes without a
GPU: the header and the binding derived from it, the build, the fixed points of the kernel source, the argument checks that precede any
launch, the refusals of the host wrappers, the sampler with three draws, the fp64 reference of tests/_resection_ref.py -- its
three-point solver against a second route, its Jacobian against finite differences, its documented outputs for degenerate problems, the
identity invariant c = a and the finding table of DESIGN.md 5.14 --, and the restatement of the kernels' arithmetic that calibrates the
GPU tests' bounds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _consensus_ref as C
from tests import _homography_ref as H
from tests import _resection_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rp_resection_abi_version", "rp_p3p_consensus", "rp_pnp_refine"}


# ------------------------------------------------------------------------------------------------ library and wrappers
def test_resection_header_parses_and_the_library_exports_it():
    from ctypes import c_int, c_void_p
    from rel_pose_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "relpose_resection.h")).read()
    consts, structs, sigs, status = _lib._header_contract(text, "relpose_resection.h")
    assert consts == {"RP_RESECTION_ABI_VERSION": 1, "RP_RESECTION_MAX_P": 1728, "RP_RESECTION_MAX_M": 4096, "RP_RESECTION_MAX_ITERS": 64}
    assert not structs
    assert (_lib.RESECTION_ABI_VERSION, _lib.RESECTION_MAX_P, _lib.RESECTION_MAX_M, _lib.RESECTION_MAX_ITERS) == (1, 1728, 4096, 64)
    P, I = c_void_p, c_int
    assert list(sigs.items()) == [("rp_resection_abi_version", (c_int, [])),
                                  ("rp_p3p_consensus", (c_int, [P, P, P, P, I, P, P, P, P, P, P, P, P, I, I, I, P])),
                                  ("rp_pnp_refine", (c_int, [P, P, P, P, P, I, P, P, P, I, I, P]))]
    assert status == NAMES - {"rp_resection_abi_version"} and tuple(sigs) == _lib.RESECTION_EXPORTS
    declared = set(re.findall(r"\b(rp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(sigs) == NAMES
    typed = _lib.load_resection()
    raw = ctypes.CDLL(_build.RESECTION_LIB)
    for sym in declared:
        assert hasattr(raw, sym), "missing export: " + sym
    assert typed.rp_resection_abi_version() == _lib.RESECTION_ABI_VERSION
    # a fifteenth library, not a change of the other fourteen: it exports none of their names and they export none of its
    others = set()
    for name in ("EXPORTS", "READOUT_EXPORTS", "EIGHTPOINT_EXPORTS", "REFINE_EXPORTS", "CONSENSUS_EXPORTS", "SUBMATCH_EXPORTS", "FIVEPOINT_EXPORTS",
                 "HOMOGRAPHY_EXPORTS", "TRIANGULATE_EXPORTS", "CONV5X5_EXPORTS", "GUIDED_EXPORTS", "ROTATION_EXPORTS", "SELECT_EXPORTS",
                 "COVARIANCE_EXPORTS"):
        others |= set(getattr(_lib, name))
    assert not declared & others
    for sym in others:
        assert not hasattr(raw, sym), "librelpose_resection.so exports " + sym
    for lib in (_build.LIB, _build.ROTATION_LIB, _build.TRIANGULATE_LIB, _build.CONSENSUS_LIB, _build.COVARIANCE_LIB, _build.SELECT_LIB):
        assert not any(hasattr(ctypes.CDLL(lib), sym) for sym in declared)
    hooked = {n for n in _lib.RESECTION_EXPORTS if getattr(typed, n).errcheck is not None}
    assert hooked == NAMES - {"rp_resection_abi_version"}
    assert typed.rp_pnp_refine.errcheck is _lib.load().rp_gemm.errcheck
    # the header documents the refusals in the order the library checks them: shape, then size, then alignment
    for entry in ("rp_p3p_consensus", "rp_pnp_refine"):
        doc = text[:text.index("int %s(" % entry)]
        doc = doc[doc.rindex("Argument checks before any launch"):]
        assert doc.index("RP_EBADSHAPE") < doc.index("RP_EUNSUPPORTED") < doc.index("RP_EALIGN")


def test_resection_build_is_a_library_of_its_own():
    from rel_pose_amd import _build
    assert os.path.basename(_build.RESECTION_LIB) == "librelpose_resection.so"
    assert os.path.basename(_build.RESECTION_CSRC) == "csrc_resection" and _build.RESECTION_SOURCES == ["resection.hip"]
    libs = {getattr(_build, n) for n in dir(_build) if n.endswith("LIB") and n.isupper()}
    assert len(libs) == 15
    for s in _build.RESECTION_SOURCES:
        assert os.path.isfile(os.path.join(ROOT, "rel_pose_amd", "csrc_resection", s))
    assert not _build.resection_needs_build() or _build.build(verbose=False) == _build.LIB
    assert not _build.resection_needs_build() and not _build.rotation_needs_build() and not _build.needs_build()
    assert os.path.join(ROOT, "include", "relpose_resection.h") in _build._resection_headers()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "load_resection().rp_resection_abi_version() == _lib.RESECTION_ABI_VERSION" in entry and "_build.RESECTION_LIB" in entry


def test_the_kernels_keep_to_the_fixed_points_of_their_design():
    """csrc_resection/ holds one file; it includes the shared headers unchanged and its own; no atomics, no allocation, no matrix
    instruction, no `while`; the constants of the header, the reference and the kernel are the same; no other library knows of it"""
    d = os.path.join(ROOT, "rel_pose_amd", "csrc_resection")
    assert sorted(n for n in os.listdir(d) if n.endswith((".hip", ".h"))) == ["resection.hip"]
    text = open(os.path.join(d, "resection.hip")).read()
    for needle in ("global_load_lds_dwordx4", "__builtin_amdgcn_mfma", "__shfl_xor", "atomicAdd", "atomicCAS", "atomicMax", "__hip_atomic", "hipMalloc"):
        assert needle not in text, needle
    assert not re.search(r"\bwhile\s*\(", text) and not re.search(r"\bdo\s*\{", text)
    for inc in ('#include "../csrc/common.h"', '#include "../csrc/block_sum.h"', '#include "../csrc/two_view.h"',
                '#include "../csrc/consensus_core.h"', '#include "../../include/relpose_resection.h"'):
        assert inc in text
    assert "lm_cholesky_solve<NPAR>(a, lam, delta)" in text and "NPAR = 6" in text and "LMRED = NTRI + NPAR" in text
    assert "DEN_MIN = 1e-30f, D_MAX = 1e30f" in text and (T.DEN_MIN, T.D_MAX) == (1e-30, 1e30)
    assert "LAMBDA0 = 1e-3f, LAMBDA_MIN = 1e-7f, LAMBDA_MAX = 1e7f" in text and (T.LAMBDA0, T.LAMBDA_MIN, T.LAMBDA_MAX) == (1e-3, 1e-7, 1e7)
    assert "SIDE_MIN = 1e-12, AREA_MIN = 1e-12, SPAN_MIN = 1e-12, LEAD_MIN = 1e-12, DEN_V_MIN = 1e-9, DISC_BAND = 1e-9" in text
    assert (T.SIDE_MIN, T.AREA_MIN, T.SPAN_MIN, T.LEAD_MIN, T.DEN_V_MIN, T.DISC_BAND, T.RESOLVENT_MIN) == (1e-12, 1e-12, 1e-12, 1e-12, 1e-9, 1e-9, 1e-14)
    assert text.count("block_sum(") == 5                                   # select 1; refine: start, 2 per iteration, finish
    # the staging and the sampler are the shared core's, called once each; nothing of the core is written out again
    assert text.count("consensus_stage(") == 1 and text.count("consensus_sample(") == 1 and "mix(" not in text and "0x9E3779B9" not in text
    pkg = os.path.join(ROOT, "rel_pose_amd")
    for sub in sorted(os.listdir(pkg)):
        if sub.startswith("csrc") and sub != "csrc_resection":
            for name in os.listdir(os.path.join(pkg, sub)):
                if name.endswith((".hip", ".h")):
                    assert "resection" not in open(os.path.join(pkg, sub, name)).read(), name


def test_argument_checks_come_before_any_launch():
    """no device is needed (or touched): the pointers are never dereferenced, the refusals precede the launch; shape, then size, then
    alignment"""
    from rel_pose_amd import _lib
    lib = _lib.load_resection()
    P = ctypes.c_void_p
    ok = [P(4096 * (i + 1)) for i in range(12)]          # X x w tau | pose best stat w_out hyp_pose hyp_cost hyp_count samples

    def cons(ptrs=ok, P_=8, M=4, n=1):
        return lib.rp_p3p_consensus(*ptrs[:4], 1, *ptrs[4:], P_, M, n, None)
    okr = [P(4096 * (i + 1)) for i in range(8)]          # X x w tau pose0 | pose stat w_out

    def ref(ptrs=okr, P_=8, iters=1, n=1):
        return lib.rp_pnp_refine(*ptrs[:5], iters, *ptrs[5:], P_, n, None)
    shape, unsup, align = r"bad shape \(RP error -1\)", r"unsupported \(RP error -4\)", r"misaligned pointer/stride \(RP error -2\)"
    swap = lambda lst, i, v: lst[:i] + [v] + lst[i + 1:]                                            # noqa: E731
    for kw in (dict(n=0), dict(P_=2), dict(M=0)) + tuple(dict(ptrs=swap(ok, i, None)) for i in (0, 1, 3, 4, 5, 6, 8, 9)):
        with pytest.raises(RuntimeError, match="rp_p3p_consensus failed: " + shape):
            cons(**kw)
    for kw in (dict(P_=1729), dict(M=4097)):
        with pytest.raises(RuntimeError, match=unsup):
            cons(**kw)
    for i in range(12):
        for off in ((4,) if i == 1 else (1, 2)):
            with pytest.raises(RuntimeError, match=align):
                cons(ptrs=swap(ok, i, P(4096 * (i + 1) + off)))
    cons.__doc__                                                   # (X needs 4-byte alignment only: its rows are 12 B)
    with pytest.raises(RuntimeError, match=shape):
        cons(ptrs=swap(ok, 1, P(8196)), n=0, P_=5000)
    with pytest.raises(RuntimeError, match=unsup):
        cons(ptrs=swap(ok, 1, P(8196)), P_=5000)
    for kw in (dict(n=0), dict(P_=2), dict(iters=-1)) + tuple(dict(ptrs=swap(okr, i, None)) for i in (0, 1, 3, 4, 5, 6)):
        with pytest.raises(RuntimeError, match="rp_pnp_refine failed: " + shape):
            ref(**kw)
    for kw in (dict(P_=1729), dict(iters=65)):
        with pytest.raises(RuntimeError, match=unsup):
            ref(**kw)
    for i in range(8):
        with pytest.raises(RuntimeError, match=align):
            ref(ptrs=swap(okr, i, P(4096 * (i + 1) + (4 if i == 1 else 2))))
    with pytest.raises(RuntimeError, match=unsup):
        ref(ptrs=swap(okr, 1, P(8196)), iters=65)


def test_host_argument_errors_raise_without_touching_a_library(monkeypatch):
    from rel_pose_amd import _lib, resection

    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load_resection", boom)
    X, x = torch.zeros(2, 8, 3), torch.zeros(2, 8, 2)
    bad = [lambda: resection.p3p_consensus(X, torch.zeros(2, 8, 3)), lambda: resection.p3p_consensus(torch.zeros(2, 8, 2), x),
           lambda: resection.p3p_consensus(X, x, torch.zeros(2, 7)), lambda: resection.p3p_consensus(X, x, tau=None),
           lambda: resection.p3p_consensus(X, x, tau=torch.zeros(3)), lambda: resection.p3p_consensus(X, x, seed=2 ** 32),
           lambda: resection.pnp_refine(X, x, None, torch.zeros(2, 6)), lambda: resection.pnp_refine(X, x[:1], None, torch.zeros(2, 7)),
           lambda: resection.pnp_refine(X, x, torch.zeros(2, 9), torch.zeros(2, 7)),
           lambda: resection.third_view_pose(None, torch.zeros(2, 2, 3, 8, 8), torch.zeros(2, 3, 4)),
           lambda: resection.third_view_pose(None, torch.zeros(2, 3, 3, 8, 8), torch.zeros(2, 2, 4))]
    for call in bad:
        with pytest.raises(ValueError):
            call()


def test_demo_third_needs_eight_point():
    import sys
    sys.path.insert(0, ROOT)
    import demo
    g = os.path.join(ROOT, "tests", "golden", "demo")
    argv = ["--img1", os.path.join(g, "matterport_1.png"), "--img2", os.path.join(g, "matterport_2.png")]
    with pytest.raises(SystemExit):
        demo.main(argv + ["--third", os.path.join(g, "matterport_2.png")])


# ------------------------------------------------------------------------------------------------ the sampler
def _draw3_scalar(seed, i, m, K):
    g, mask = C.GOLDEN, 0xFFFFFFFF
    mix = lambda v: int(C.mix(v))                                                                   # noqa: E731
    s = mix(mix((seed + g * (i + 1)) & mask) ^ m)
    c = []
    for k in range(3):
        r = mix((s + g * (k + 1)) & mask)
        j = K - 3 + k
        t = (r * (j + 1)) >> 32
        c.append(j if t in c else t)
    return c


def test_sampler_is_the_contract_sampler_with_three_draws():
    """draw3 equals a scalar restatement of relpose_consensus.h's rule with S = 3 and _consensus_ref's own mix; the draws are distinct,
    in range, and their first two stages are _rotation_ref.draw2's rule shifted by one row (the same Floyd recursion)"""
    for seed, i, K in ((0, 0, 3), (1, 5, 4), (7, 129, 64), (2 ** 32 - 1, 3, 1728), (-5, 2, 9)):
        got = T.draw3(seed, i, np.arange(300), K)
        want = np.array([_draw3_scalar(seed & 0xFFFFFFFF, i, m, K) for m in range(300)])
        assert np.array_equal(got, want)
        assert got.min() >= 0 and got.max() < K and all(len(set(r)) == 3 for r in got.tolist())
    # the 8-draw sampler of _consensus_ref uses j = K - 8 + k: with K' = K + 5 its first three draws are this rule's
    assert np.array_equal(C.draw(3, 2, np.arange(50), 40 + 5)[:, :3], T.draw3(3, 2, np.arange(50), 40))
    w = np.ones((2, 10), np.float32)
    w[1, [0, 3, 4, 5, 6, 7, 8, 9]] = 0, -1, np.nan, 0, 0, 0, 0, 0
    pos, smp = T.sample_rows3(w, 2, 10, 1, 20)
    assert list(pos[1]) == [1, 2] and not smp[1].any() and smp[0].max() <= 9 and smp.shape == (2, 20, 3)


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_solver_agrees_with_its_second_route_and_reaches_the_truth():
    """on exact rows (the images of the float32 points under the true pose, in fp64): every returned pose is a rotation and reproduces its three rows (substitution); the SET of solutions equals that of
    numpy.roots on the quartic, each root kept if the three depths are positive; the true pose is among the solutions of EVERY sample (no
    sample is excluded: the rule that could exclude one, INVALID of the header, does not fire on these cases)"""
    X, x, truth = T.exact_rows(6, 64, 21)
    _, smp = T.sample_rows3(None, 6, 64, 1, 256)
    total = 0
    for b in range(6):
        exact = T.proj(H.quat_to_rot(truth[b, 3:]), truth[b, :3], X[b].astype(np.float64))        # the images in fp64, not rounded
        Xs, xs = X[b][smp[b]].astype(np.float64), exact[smp[b]]
        pose, ok, margin = T.p3p(Xs, xs)
        alt = T.p3p_roots_lapack(Xs, xs)
        assert bool(ok.any(-1).all()) and bool(np.isfinite(margin).all())
        R = T.quat_to_rot(pose[..., 3:]).reshape(-1, 4, 3, 3)
        assert np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3))[ok].max() < 1e-12 and np.abs(np.linalg.det(R[ok]) - 1).max() < 1e-12
        lev, res = T.lever(pose, Xs[:, None], xs[:, None])
        # substitution: the residual of a sample row, in units of 1e-10 lever; near a double root of the quartic (margin -> 0) the roots
        # are determined to sqrt(eps64) only
        assert (res[ok] / lev[ok]).max() < 1e-7 and np.median(res[ok] / lev[ok]) < 1e-13
        for i in range(256):
            mine = np.sort(np.stack([np.linalg.norm(T.project(pose[i, k], Xs[i])[0], axis=-1) for k in range(4) if ok[i, k]]), 0)
            assert len(mine) == len(alt[i]) and np.abs(mine - np.sort(alt[i], 0)).max() <= 1e-6 * mine.max(), (b, i, margin[i])
            assert min(np.abs(pose[i, k] - truth[b]).max() for k in range(4) if ok[i, k]) < 1e-6, (b, i)
            total += 1
    assert total == 1536


def test_invalid_samples_of_the_reference():
    """coincident points, collinear points, coinciding bearings: INVALID; a healthy sample next to them is not"""
    X, x, _ = T.exact_rows(1, 8, 3)
    Xs, xs = X[0][[0, 1, 2]].astype(np.float64)[None].repeat(4, 0), x[0][[0, 1, 2]].astype(np.float64)[None].repeat(4, 0)
    Xs[1, 1] = Xs[1, 0]                                                   # coincident
    Xs[2, 2] = 0.25 * Xs[2, 0] + 0.75 * Xs[2, 1]                          # collinear
    xs[3, 1] = xs[3, 0]                                                   # two bearings coincide
    pose, ok, margin = T.p3p(Xs, xs)
    assert ok[0].any() and not ok[1:].any() and not pose[1:].any() and np.isinf(margin[1:]).all()


def test_jacobian_agrees_with_finite_differences():
    X, x, truth = T.exact_rows(1, 40, 5, sigma=1e-3)
    rng = np.random.default_rng(0)
    pose = truth[0] + 1e-2 * rng.normal(size=7)
    pose[3:] /= np.linalg.norm(pose[3:])
    Jx, Jy, r, d, ok = T.jacobian(pose, X[0], x[0])
    assert ok.all() and np.allclose(d, (r * r).sum(-1), rtol=1e-12)
    h = 1e-6
    for k in range(6):
        delta = np.zeros(6)
        delta[k] = h
        plus = np.concatenate([pose[:3] + delta[3:], T.RT.retract(pose[3:], delta[:3])[0]])
        minus = np.concatenate([pose[:3] - delta[3:], T.RT.retract(pose[3:], -delta[:3])[0]])
        fd = (T.jacobian(plus, X[0], x[0])[2] - T.jacobian(minus, X[0], x[0])[2]) / (2 * h)
        assert np.abs(fd[:, 0] - Jx[:, k]).max() < 1e-8 * max(1, np.abs(Jx[:, k]).max()), k
        assert np.abs(fd[:, 1] - Jy[:, k]).max() < 1e-8 * max(1, np.abs(Jy[:, k]).max()), k


def test_degenerate_problems_give_the_documented_outputs_in_the_reference():
    n, P = 6, 40
    X, x, _ = T.exact_rows(n, P, 12)
    w = np.random.default_rng(1).uniform(0.05, 1, (n, P)).astype(np.float32)
    w[1] = 0
    w[1, [9, 11]] = 0.5
    w[1, 7], w[1, 8] = -1, np.nan
    tau = np.full(n, T.TAU)
    tau[3], tau[5] = np.nan, 0
    X[4, :] = X[4, 0]                                                     # every sample is three coincident points
    for dt in (np.float64, np.float32):
        c = T.consensus(X, x, w, tau, 3, 70, dt)
        wc = C.clamp(w, n, P, dt)
        for b, K in ((1, 2), (3, 40), (4, 40), (5, 40)):
            assert not c.pose[b].any() and c.best[b] == -1 and np.array_equal(c.stat[b], [0, 0, 0, K])
            assert np.array_equal(c.weights[b], wc[b]) and not c.hyp_pose[b].any() and (c.hyp_cost[b] == T.FLT_MAX).all() and not c.hyp_count[b].any()
        assert not c.samples[1].any() and c.samples[4].any() and (c.best[[0, 2]] >= 0).all()
        p0 = c.pose.astype(np.float32).copy()
        p0[0, 2], p0[2, 3:] = np.inf, 0
        r = T.refine(X, x, w, tau, p0, 3, dt)
        for b, K in ((0, 40), (1, 2), (2, 40), (3, 40), (4, 40), (5, 40)):
            assert np.array_equal(r.pose[b], p0[b].astype(dt), equal_nan=True) and np.array_equal(r.stat[b], [0, 0, 0, K])
            assert np.array_equal(r.weights[b], wc[b])


def test_the_reference_leaves_out_less_than_the_cap():
    """the rule that leaves a hypothesis out of the GPU comparison -- a decision of the reference's solver within MARGIN_CMP of its
    threshold -- is a rule of the reference alone, and on the inputs of the GPU tests it fires for less than 5 % of a case's hypotheses"""
    worst = 0.0
    for case in T.CASES:
        ref = T.reference(*case)
        valid = ref.hyp_cost < T.FLT_MAX
        left = 1 - (valid & (ref.margin >= T.MARGIN_CMP)).sum() / max(valid.sum(), 1)
        worst = max(worst, left)
        assert left < T.LEFT_OUT_MAX, (case, left)
    print("left out, worst case: %.4f" % worst)


def test_float32_restatement_is_within_the_calibrated_bounds():
    """the GPU bounds are 8 x these figures: the restatement stays within WORST, and WORST is not looser than what it measures"""
    got = T.restatement_worst()
    print(got)
    for k, v in T.WORST.items():
        assert 0.9 * v <= got[k] <= v, (k, got[k], v)
    assert (T.C_UNIT, T.C_REPRO, T.C_COST, T.C_W) == tuple(8 * T.WORST[k] for k in ("unit", "repro", "cost", "w"))
    assert T.C_REFINE == {1: 8 * T.WORST["refine1"], 10: 8 * T.WORST["refine10"]}


# ------------------------------------------------------------------------------------------------ what it does
def test_identity_invariant_c_equals_a():
    """with c = a (x_c = x_a, noise-free) the resection returns pose_a with |t| = 1.  The bound is derived from the reference's
    conditioning: the rows carry the float32 rounding of x and X, which moves the minimiser from the truth by N^-1 g to first order (N, g
    the normal matrix and the gradient AT the truth); the test allows twice that step"""
    for seed in range(4):
        sc = T.three_views(seed, 576, 0.0, 0.0)
        r, cons, w, X = T.third_view(sc._replace(xc=sc.xa))
        N, g = T.normal_equations(sc.pose_a, X, sc.xa, w.astype(np.float64), T.TAU ** 2)
        step = np.linalg.solve(N, g)
        bound = 2 * np.abs(step).max() + 1e-12
        err = np.abs(r.pose[0] - sc.pose_a).max()
        scale = np.linalg.norm(r.pose[0, :3])
        print("seed %d: |pose - pose_a| %.3g (bound %.3g), |t| - 1 = %.3g, kappa %.1f" % (seed, err, bound, scale - 1, r.kappa[0]))
        assert cons.best[0] >= 0 and err <= bound and abs(scale - 1) <= bound and bound < 1e-5


def test_finding_table():
    """the table of DESIGN.md 5.14, re-measured: seeds 0 - 9, P = 576, M = 256, 10 iterations, the TRUE pose for pair (hub, a), wrong
    matches per pair 30 / 50 / 60 %, noise 1e-3 and half a token pitch; EVERY column asserted as measured (T.TABLE holds four decimals:
    the counts exactly, the ratios to 2e-3, the median errors in degrees to 2 % + 1e-3), then the statements the documents make of it"""
    got = T.table()
    assert set(got) == set(T.TABLE) and len(got) == 12
    for key, row in got.items():
        print(key, row)
        want = T.TABLE[key]
        assert row[0] == want[0] and row[3] == want[3], (key, row, want)
        assert all(abs(row[i] - want[i]) <= 2e-3 for i in (1, 2, 4)), (key, row, want)
        assert all(abs(row[i] - want[i]) <= 0.02 * want[i] + 1e-3 for i in (5, 6)), (key, row, want)
    # (a) with the first pair's Cauchy weights the scale is within 10 % in at least as many scenes as without, in every cell, and the
    # median rotation and direction errors are smaller: without the weights they are 1.2 - 6.1 x larger
    # (b) without them no fewer scenes fall towards |t| -> 0, and more at token-pitch noise; (c) the bias at token-pitch noise is low
    for sigma in T.TABLE_SIGMAS:
        for out in T.TABLE_OUTLIERS:
            wi, wo = got[(sigma, out, True)], got[(sigma, out, False)]
            assert wi[0] >= wo[0] and wi[3] <= wo[3]
            for i in (5, 6):
                assert 1.2 <= wo[i] / wi[i] <= 6.1, (sigma, out, i, wo[i] / wi[i])
    assert [got[(1e-3, out, True)][0] for out in T.TABLE_OUTLIERS] == [10, 9, 9] and [got[(0.012, out, True)][0] for out in T.TABLE_OUTLIERS] == [8, 7, 8]
    assert sum(got[(0.012, out, False)][3] for out in T.TABLE_OUTLIERS) > sum(got[(0.012, out, True)][3] for out in T.TABLE_OUTLIERS)
    for out in T.TABLE_OUTLIERS:
        assert got[(0.012, out, True)][4] < 1 and got[(0.012, out, True)][4] < got[(1e-3, out, True)][4]
        assert got[(0.012, out, False)][4] < got[(0.012, out, True)][4] and got[(0.012, out, True)][2] <= 1.011 + 2e-3


def test_row_weights_against_the_reference_statement():
    """resection.row_weights (pure torch) against tests/_resection_ref.row_weights, an independent numpy statement, on a hand-built
    Structure: the carried-over Cauchy factor, both depth gates, the parallax gate (default tau_a and a given floor), both base weights"""
    from rel_pose_amd import resection, triangulate
    rng = np.random.default_rng(3)
    B, P = 3, 60
    z1, z2 = rng.normal(2, 3, (B, P)), rng.normal(2, 3, (B, P))             # about a quarter of each negative
    d2 = rng.uniform(0, 9, (B, P)) * T.TAU ** 2
    tau = np.array([T.TAU, 2 * T.TAU, 0.5 * T.TAU])
    phi = rng.uniform(0, 3, (B, P)) * tau[:, None]                          # a third below tau_a
    z1[:, 0], z2[:, 1], phi[:, 2] = 0, 0, tau                               # on the gates: depth 0 is out, parallax = floor is in
    w_a, w_c = rng.uniform(0, 1, (B, P)), rng.uniform(0, 1, (B, P))
    w_a[:, 3], w_c[:, 4] = 0, 0
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))                                    # noqa: E731
    st = triangulate.Structure(torch.zeros(B, P, 3), f32(z1), f32(z2), f32(d2), f32(phi), torch.zeros(B, 4), None)
    z1, z2, d2, phi, w_a, w_c, tau = (np.asarray(a, np.float32).astype(np.float64) for a in (z1, z2, d2, phi, w_a, w_c, tau))
    for floor in (None, 0.02, np.array([0.0, 0.03, 1.0])):
        got = resection.row_weights(st, f32(w_a), f32(w_c), f32(tau), None if floor is None else floor if np.isscalar(floor) else f32(floor))
        fl = [None] * B if floor is None else np.broadcast_to(np.asarray(floor, np.float32).astype(np.float64), (B,))
        want = np.stack([T.row_weights(z1[b], z2[b], d2[b], phi[b], tau[b], w_a[b], w_c[b], min_parallax=fl[b]) for b in range(B)])
        assert got.shape == (B, P) and got.dtype == torch.float32
        assert np.abs(got.numpy() - want).max() <= 4 * T.EPS32 and np.array_equal(got.numpy() > 0, want > 0)
        assert 0.2 < (want > 0).mean() < 0.8                                # the gates and the zeros bite, and not everywhere
    assert not got[:, [0, 1, 3, 4]].any()
    one = resection.row_weights(triangulate.Structure(*[None if t is None else t[:1] for t in st]), f32(w_a[:1]), f32(w_c[:1]), float(tau[0]))
    assert torch.equal(one, resection.row_weights(st, f32(w_a), f32(w_c), f32(tau))[:1])            # tau_a as a number
    for bad in (lambda: resection.row_weights(st, f32(w_a), f32(w_c[:, :5]), f32(tau)), lambda: resection.row_weights(st, f32(w_a), f32(w_c), f32(tau[:2])),
                lambda: resection.row_weights(st, f32(w_a), f32(w_c), f32(tau), f32(tau[:2]))):
        with pytest.raises(ValueError):
            bad()


def test_third_view_tau_and_batch_slicing_are_checked_on_the_host():
    """a tau that is neither a number, [B] nor [2B] is a ValueError before the model runs; _part slices batch-leading tensors only"""
    from rel_pose_amd import resection
    with pytest.raises(ValueError, match="tau"):
        resection.third_view_pose(None, torch.zeros(2, 3, 3, 8, 8), torch.zeros(2, 3, 4), tau=torch.zeros(3))
    with pytest.raises(ValueError, match="tau"):
        resection.third_view_pose(None, torch.zeros(2, 3, 3, 8, 8), torch.zeros(2, 3, 4), tau=torch.zeros(2, 2))
    pair = resection.PnPRefined(torch.arange(28.).view(4, 7), torch.zeros(4, 4), None)
    got = resection._part((pair, "name", None), 4, slice(2, 4))
    assert torch.equal(got[0].pose, pair.pose[2:]) and got[0].weights is None and got[1:] == ("name", None) and type(got[0]) is resection.PnPRefined
    with pytest.raises(ValueError, match="does not lead"):
        resection._part((torch.zeros(3, 4),), 4, slice(2, 4))
