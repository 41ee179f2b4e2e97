"""rp_eight_point (include/relpose_eightpoint.h, csrc_eightpoint/eight_point.hip) and what is built on it, on a real MI355X.

The reference is tests/_eightpoint_ref.py: eight_point_ref, the same algorithm in fp64 with LAPACK.  Errors of E are taken up to sign,
min(|E - E_ref|_F, |E + E_ref|_F), except where the sign rule itself is tested.

Bounds.  E is built from the null vector of the weighted row matrix A; by perturbation theory a relative perturbation eps of A moves
that vector by about eps sigma_1 / sigma_8 (the gap to the next singular value), so every problem is bounded by
    C eps32 sigma_1 / sigma_8(reference),
C = 8 x the largest ratio err / (eps32 sigma_1 / sigma_8) that the numpy float32 restatement of the kernel's arithmetic
(_eightpoint_ref.eight_point_f32: same normalisation, same Jacobi order, threshold and sweep count; numpy's pairwise sums instead of the
kernel's wave / LDS tree) shows on these same inputs; the factor 8 covers the different order of the sums.  Measured on parity_inputs
over all PARITY_CASES, weighted and not (the restatement, on the CPU):
    E          largest ratio 1.37 (P = 8, n = 130, whose sigma_8 / sigma_1 goes down to 1e-5; 0.03 .. 0.58 for P >= 9)  -> C_PARITY = 11
    stat[0:3]  largest ratio |stat - stat_ref| / (eps32 sigma_1 / sigma_8) 0.93 (P = 8; 0.01 .. 0.32 for P >= 9)          -> C_STAT = 7.4
    (stat[0] = sigma_9 / sigma_1 and stat[1] are ratios to sigma_1 already, stat[2] = e2 / e1 is of order 1)
wsum is a plain sum of P positive numbers: the project's rel < 2e-6.
Re-weighting: with r = x2^T E x1 of absolute rounding error ~eps32 (its terms are of order 1) and u = sqrt(d) / tau, the weight
w0 / (1 + u^2) moves by w0 2u / (1 + u^2)^2 delta_r / (tau sqrt(den)) <= 0.65 w0 eps32 / (tau sqrt(den)): the bound is
    |w1 - w1_ref| / w0 <= C_W eps32 / tau,    C_W = 8 x the restatement's largest ratio 0.241 on reweight_inputs -> C_W = 1.9.
The GPU's own worst ratios go to the test report (tests/test_gpu_kernels.py: report)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from tests import _contract_cases as CC
from tests import _eightpoint_ref as R
from tests.test_gpu_kernels import report
from tests.test_gpu_memory_contract import _bf16_configuration, _model, run_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = 256                                        # threads of the kernel's workgroup
C_PARITY, C_STAT, C_W = 11.0, 7.4, 1.9         # see the module docstring
PARITY_CASES = [(8, 130), (9, 3), (NT - 1, 1), (NT, 3), (NT + 1, 1), (2 * NT + 1, 3), (1728, 1)]


@pytest.fixture(scope="module")
def ep():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, eightpoint
    _lib.load()
    _lib.load_eightpoint()
    return eightpoint


@functools.lru_cache(maxsize=None)
def parity_inputs(P, n, weighted):
    """float32 numpy x1, x2 [n,P,2] of n exact synthetic scenes (rounded to float32: the reference sees the same numbers) and random
    positive weights [n,P] in 0.05 .. 1 or None"""
    x1, x2, _ = R.scenes(n, P, seed=11)
    w = np.random.default_rng(P + n).uniform(0.05, 1.0, (n, P)).astype(np.float32) if weighted else None
    return x1.astype(np.float32), x2.astype(np.float32), w


@functools.lru_cache(maxsize=None)
def parity_reference(P, n, weighted):
    return R.eight_point_ref(*parity_inputs(P, n, weighted))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


def check_parity(tag, E, stat, Er, sr):
    """E [n,3,3], stat [n,4] of the GPU against the fp64 reference's, per problem at C eps32 sigma_1 / sigma_8(ref)"""
    scale = R.EPS32 / sr[:, 1]
    e = R.up_to_sign(host(E), Er) / scale
    s = np.abs(host(stat)[:, :3] - sr[:, :3]).max(-1) / scale
    ws = np.abs(host(stat)[:, 3] - sr[:, 3]) / sr[:, 3]
    report("eightpoint_" + tag, E_ratio=float(e.max()), stat_ratio=float(s.max()), wsum_rel=float(ws.max()),
           sigma8_over_sigma1_min=float(sr[:, 1].min()))
    print(tag, "E ratio %.3g (C %.3g), stat ratio %.3g (C %.3g), wsum %.2e" % (e.max(), C_PARITY, s.max(), C_STAT, ws.max()))
    assert float(e.max()) <= C_PARITY, (tag, e.max())
    assert float(s.max()) <= C_STAT, (tag, s.max())
    assert float(ws.max()) < 2e-6, (tag, ws.max())


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weighted"])
@pytest.mark.parametrize("P,n", PARITY_CASES)
def test_parity(ep, P, n, weighted):
    x1, x2, w = parity_inputs(P, n, weighted)
    Er, sr, _ = parity_reference(P, n, weighted)
    out = ep.eight_point(dev(x1), dev(x2), dev(w), return_weights=True)
    assert out.E.shape == (n, 3, 3) and out.stat.shape == (n, 4) and out.weights.shape == (n, P)
    check_parity("parity_P%d_n%d_%s" % (P, n, "w" if weighted else "ones"), out.E, out.stat, Er, sr)
    assert torch.equal(out.weights.cpu(), torch.ones(n, P) if w is None else torch.from_numpy(w))
    sv = np.linalg.svd(host(out.E), compute_uv=False)
    assert np.abs(sv - [1, 1, 0]).max() < 1e-5                    # on the essential manifold
    again = ep.eight_point(dev(x1), dev(x2), dev(w), return_weights=True)
    assert all(torch.equal(a, b) for a, b in zip(out, again))     # bit-identical from call to call
    assert ep.eight_point(dev(x1), dev(x2), dev(w)).weights is None


WIDE_CASES = [(8, 60), (64, 12), (300, 6)]


@functools.lru_cache(maxsize=None)
def wide_inputs(kind, P, n, weighted):
    """parity_inputs on R.wide_scenes: rotations of 2.2 .. 3.1 rad ("beyond120") or of exactly pi ("half_turn")"""
    x1, x2, _, _ = R.wide_scenes(n, P, 11, kind)
    w = np.random.default_rng(P + n).uniform(0.05, 1.0, (n, P)).astype(np.float32) if weighted else None
    return x1.astype(np.float32), x2.astype(np.float32), w


@functools.lru_cache(maxsize=None)
def wide_reference(kind, P, n, weighted):
    return R.eight_point_ref(*wide_inputs(kind, P, n, weighted))


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weighted"])
@pytest.mark.parametrize("P,n", WIDE_CASES)
@pytest.mark.parametrize("kind", ["beyond120", "half_turn"])
def test_parity_wide_baseline(ep, kind, P, n, weighted):
    """test_parity beyond a rotation of 120 degrees and at a half-turn, same bounds and constants (the restatement's largest ratios on
    these inputs: E 2.05 at P = 8, 0.93 for P >= 64; stat 1.07 -- tests/test_eightpoint_cpu.py)"""
    x1, x2, w = wide_inputs(kind, P, n, weighted)
    Er, sr, _ = wide_reference(kind, P, n, weighted)
    out = ep.eight_point(dev(x1), dev(x2), dev(w), return_weights=True)
    assert out.E.shape == (n, 3, 3) and out.stat.shape == (n, 4) and out.weights.shape == (n, P)
    check_parity("parity_%s_P%d_n%d_%s" % (kind, P, n, "w" if weighted else "ones"), out.E, out.stat, Er, sr)
    assert torch.equal(out.weights.cpu(), torch.ones(n, P) if w is None else torch.from_numpy(w))
    sv = np.linalg.svd(host(out.E), compute_uv=False)
    assert np.abs(sv - [1, 1, 0]).max() < 1e-5                    # on the essential manifold
    again = ep.eight_point(dev(x1), dev(x2), dev(w), return_weights=True)
    assert all(torch.equal(a, b) for a, b in zip(out, again))     # bit-identical from call to call


def test_sign_rule(ep):
    """where the reference's largest entry is at least 10 % above the runner-up the sign is determined: E equals E_ref, not -E_ref"""
    seen = 0
    for P, n in ((8, 130), (NT, 3), (2 * NT + 1, 3)):
        x1, x2, w = parity_inputs(P, n, True)
        Er, sr, _ = parity_reference(P, n, True)
        mag = np.sort(np.abs(Er.reshape(n, 9)), -1)
        clear = mag[:, 8] >= 1.1 * mag[:, 7]
        E = host(ep.eight_point(dev(x1), dev(x2), dev(w)).E).reshape(n, 9)
        err = np.linalg.norm(E - Er.reshape(n, 9), axis=-1) / (R.EPS32 / sr[:, 1])
        assert float(err[clear].max(initial=0)) <= C_PARITY
        lead = np.abs(E).argmax(-1)
        assert bool((E[np.arange(n), lead] > 0).all())            # for every problem: the largest entry is positive
        seen += int(clear.sum())
    assert seen >= 30                                             # (40 with these inputs)


@functools.lru_cache(maxsize=None)
def reweight_inputs():
    """three scenes of 300 points, noise of 1e-3, 30 of x2 replaced by uniform noise, random base weights; tau = 0.02"""
    x1, x2 = [], []
    for seed in (20, 21, 22):
        a, b, _, _ = R.noisy_scene(seed, P=300)
        x1.append(a[0])
        x2.append(b[0])
    w0 = np.random.default_rng(5).uniform(0.05, 1.0, (3, 300)).astype(np.float32)
    return np.stack(x1), np.stack(x2), w0, np.full(3, 0.02, np.float32)


def test_reweighting_one_step(ep):
    x1, x2, w0, tau = reweight_inputs()
    a, b, w, t = dev(x1), dev(x2), dev(w0), dev(tau)
    E0 = ep.eight_point(a, b, w).E
    one = ep.eight_point(a, b, w, tau=t, iters=1, return_weights=True)
    want = w0.astype(np.float64) / (1 + R.sampson64(host(E0), x1, x2) / tau[:, None].astype(np.float64) ** 2)
    ratio = np.abs(host(one.weights) - want) / w0 / (R.EPS32 / tau[:, None])
    report("eightpoint_reweight_one_step", w_ratio=float(ratio.max()), w_min=float(want.min()), w_max=float(want.max()))
    print("one step: weight ratio %.3g (C_W %.3g)" % (ratio.max(), C_W))
    assert float(ratio.max()) <= C_W
    assert float((want / w0).min()) < 0.01 and float((want / w0).max()) > 0.9            # the weights do discriminate
    again = ep.eight_point(a, b, one.weights)
    assert torch.equal(again.E, one.E) and torch.equal(again.stat, one.stat)             # bit-identical
    # a float tau is broadcast
    assert all(torch.equal(p, q) for p, q in zip(ep.eight_point(a, b, w, tau=0.02, iters=1, return_weights=True), one))


def test_reweighting_converged(ep):
    """576 points, 10 % of x2 uniform noise, Gaussian noise of 1e-3, tau = 0.01, iters = 8.  IRLS amplifies rounding until it has
    converged, so only seeds whose REFERENCE moved less than 1e-4 between rounds 7 and 8 count: the first four of them, and at least
    four of the first ten must qualify (with noisy_scene: eight do)"""
    tau = np.array([0.01], np.float32)
    chosen = []
    for seed in range(10):
        x1, x2, Et, _ = R.noisy_scene(seed)
        Er, sr, wr, hist = R.eight_point_ref(x1, x2, None, tau, 8, history=True)
        if np.abs(hist[0][8] - hist[0][7]).max() < 1e-4:
            chosen.append((seed, x1, x2, Et, Er, sr, wr))
    assert len(chosen) >= 4, [c[0] for c in chosen]
    for seed, x1, x2, Et, Er, sr, wr in chosen[:4]:
        truth = float(R.up_to_sign(Er, Et)[0])
        assert truth < 2e-2, (seed, truth)                        # the reference itself finds the pose
        out = ep.eight_point(dev(x1), dev(x2), None, tau=dev(tau), iters=8, return_weights=True)
        check_parity("irls_seed%d" % seed, out.E, out.stat, Er, sr)
        dw = float(np.abs(host(out.weights) - wr).max())
        report("eightpoint_irls_seed%d_more" % seed, ref_vs_truth=truth, weights_abs=dw)
        assert dw < 1e-3


def test_degenerate_problems_in_a_batch(ep):
    """seven positive weights, all-zero weights and coincident points between healthy problems: exact zero outputs, and the healthy
    neighbours bit-identical to a call without the degenerate ones"""
    P = 300
    x1, x2, w0, _ = reweight_inputs()
    x1, x2, w0 = np.repeat(x1, 2, 0).copy(), np.repeat(x2, 2, 0).copy(), np.repeat(w0, 2, 0).copy()      # problems 0, 2, 4 healthy
    w0[1] = 0
    w0[1, [3, 50, 100, 255, 256, 257, 299]] = 0.5
    w0[1, 7] = -1.0                                               # negative: counts as 0
    w0[3] = 0
    x1[5] = x1[5, 17]                                             # every point of image 0 the same
    tau = np.full(6, 0.02, np.float32)
    for iters in (0, 2):
        out = ep.eight_point(dev(x1), dev(x2), dev(w0), tau=dev(tau), iters=iters, return_weights=True)
        E, stat, wo = out.E.cpu().numpy(), out.stat.cpu().numpy(), out.weights.cpu().numpy()
        for b in (1, 3, 5):
            assert not E[b].any() and not stat[b, :3].any(), (b, E[b], stat[b])
            assert np.array_equal(wo[b], np.maximum(w0[b], 0))
        assert stat[1, 3] == 3.5 and stat[3, 3] == 0.0 and abs(stat[5, 3] - w0[5].sum(dtype=np.float64)) < 2e-6 * w0[5].sum()
        assert np.isfinite(E).all() and np.isfinite(stat).all() and np.isfinite(wo).all()
        keep = [0, 2, 4]
        alone = ep.eight_point(dev(x1[keep]), dev(x2[keep]), dev(w0[keep]), tau=dev(tau[keep]), iters=iters, return_weights=True)
        assert all(torch.equal(p[keep], q) for p, q in zip(out, alone))
        assert float(out.E[keep].abs().max()) > 0.3


# ------------------------------------------------------------------------------------------------ memory contract
def _eight_point_case(P, with_w, with_w_out, iters, n=3):
    """one guarded rp_eight_point call (tests/_contract_cases.py's Case, kept out of its table: that table is the main header's)"""
    x1, x2, w = parity_inputs(P, n, True)
    tau = np.full(n, 0.05, np.float32)
    ops_ = [CC.inp("x1", torch.from_numpy(x1).reshape(1, -1)), CC.inp("x2", torch.from_numpy(x2).reshape(1, -1)),
            CC.inp("tau", torch.from_numpy(tau).reshape(1, -1)), CC.flat("E", n * 9), CC.flat("stat", n * 4)]
    if with_w:
        ops_.append(CC.inp("w", torch.from_numpy(w).reshape(1, -1)))
    if with_w_out:
        ops_.append(CC.flat("w_out", n * P))

    def call(lib, A_, st):
        lib.rp_eight_point(CC.a_(A_, "x1"), CC.a_(A_, "x2"), CC.a_(A_, "w"), CC.a_(A_, "tau"), CC.a_(A_, "E"), CC.a_(A_, "stat"),
                           CC.a_(A_, "w_out"), P, iters, n, st)

    def check(v, errs):
        Er, sr, wr = R.eight_point_ref(x1, x2, w if with_w else None, tau, iters)
        e = {}
        if iters == 0:
            ratio = float((R.up_to_sign(host(v["E"]).reshape(n, 9), Er) / (R.EPS32 / sr[:, 1])).max())
            e["E_ratio"] = CC._bound(errs, "E", ratio, C_PARITY)
        if not bool(torch.isfinite(v["E"]).all()) or not bool(torch.isfinite(v["stat"]).all()):
            errs.append("non-finite output")
        if with_w_out:
            e["w_out"] = CC._bound(errs, "w_out", float(np.abs(host(v["w_out"]).reshape(n, P) - wr).max()), 1e-3)
        return e
    return CC.Case(ops_, call, check)


_CONTRACT = [(P, ww, wo, it) for P in (8, NT + 1, 1728) for ww in (False, True) for wo in (False, True) for it in (0, 2)]


@pytest.mark.parametrize("P,with_w,with_w_out,iters", _CONTRACT,
                         ids=["P%d-%s-%s-iters%d" % (P, "w" if a else "now", "wout" if b else "nowout", i) for P, a, b, i in _CONTRACT])
def test_memory_contract(ep, P, with_w, with_w_out, iters):
    """guards intact, every documented element written and nothing else, inputs unchanged, NaN-fill and finite-fill runs bit-identical"""
    from rel_pose_amd import _lib
    lib = _lib.load_eightpoint()
    builder = lambda: _eight_point_case(P, with_w, with_w_out, iters)      # noqa: E731
    bad_a, va, c, ops_ = run_case(lib, builder, finite=False)
    bad_b, vb, _, _ = run_case(lib, builder, finite=True)
    bad = ["NaN-fill run: " + b for b in bad_a] + ["finite-fill run: " + b for b in bad_b]
    assert set(va) == {o.name for o in ops_ if o.role == "out"} == {"E", "stat"} | ({"w_out"} if with_w_out else set())
    for k in va:
        bits = CC._BITS[va[k].dtype]
        if not torch.equal(va[k].view(bits), vb[k].view(bits)):
            bad.append("%s: result depends on what the output held before the call" % k)
    errs = c.check(va, bad) if not bad_a else {}
    report("eightpoint_memory_contract_P%d_w%d_wout%d_iters%d" % (P, with_w, with_w_out, iters), violations=len(bad), **errs)
    assert not bad, "\n".join(bad)


def test_too_many_points_are_refused_with_outputs_untouched(ep):
    from rel_pose_amd import _lib
    n, P = 2, _lib.EIGHTPOINT_MAX_P + 1
    x = torch.rand(n, P, 2, device="cuda")
    with pytest.raises(RuntimeError, match=r"rel_pose_amd: rp_eight_point failed: unsupported \(RP error -4\)"):
        ep.eight_point(x, x.clone())
    lib = _lib.load_eightpoint()
    E, stat, wo = (torch.full(s, -7.0, device="cuda") for s in ((n, 9), (n, 4), (n, P)))
    Pv = ctypes.c_void_p
    st = Pv(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(RuntimeError, match=r"unsupported \(RP error -4\)"):
        lib.rp_eight_point(Pv(x.data_ptr()), Pv(x.data_ptr()), None, None, Pv(E.data_ptr()), Pv(stat.data_ptr()), Pv(wo.data_ptr()),
                           P, 0, n, st)
    torch.cuda.synchronize()
    assert bool((E == -7).all()) and bool((stat == -7).all()) and bool((wo == -7).all())          # nothing ran
    with pytest.raises(ValueError):
        ep.eight_point(x[:, :64], x[:, :63])
    with pytest.raises(ValueError, match="tau"):
        ep.eight_point(x[:, :64].contiguous(), x[:, :64].contiguous(), iters=1)


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture
def repeatable_cnn():
    """as in tests/test_gpu_readout.py: a bit-for-bit comparison of two runs from IMAGES asks MIOpen for its repeatable solvers"""
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    yield
    torch.backends.cudnn.deterministic = keep


def test_model_pose_from_matches(ep, repeatable_cnn):
    from oracle import relpose_oracle as O
    from rel_pose_amd import geom
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
    mp = m.pose_from_matches(images, intr)
    assert torch.equal(intr, keep_intr)
    assert mp.pose.shape == (B, 7) and mp.E.shape == (B, 3, 3) and mp.stat.shape == (B, 4) and mp.count.shape == (B,)
    assert mp.weights.shape == (B, 1728) and mp.count.dtype == torch.int32
    # the chain of the public pieces, bit for bit
    corr = m.correspondences(images)
    x1, x2, w = ep.assemble_matches(corr, intr, (384, 384))
    tau = ep.default_tau(intr, (384, 384))
    assert torch.allclose(tau.cpu(), torch.full((B,), 0.5 * 16 / (0.9 * 384)))
    e = ep.eight_point(x1, x2, w, tau=tau, iters=4, return_weights=True)
    pose, count = geom.pose_from_essential(e.E, x1, x2)
    for got, want in zip(mp, (pose, e.E, e.stat, count, e.weights)):
        assert torch.equal(got, want)
    assert bool(torch.isfinite(mp.pose).all()) and bool((mp.pose[:, 6] >= 0).all())
    assert float((mp.pose[:, :3].norm(dim=-1) - 1).abs().max()) < 1e-5 and float((mp.pose[:, 3:].norm(dim=-1) - 1).abs().max()) < 1e-5
    # a subset of heads, no re-weighting: E against the fp64 reference fed the same assembled matches, at the parity bound
    for heads in ((0, 1, 2), (1,)):
        one = m.pose_from_matches(images, intr, heads=heads, iters=0)
        y1, y2, v = ep.assemble_matches(corr, intr, (384, 384), heads=heads)
        assert one.weights.shape == (B, 576 * len(heads)) and torch.equal(one.weights, v)
        Er, sr, _ = R.eight_point_ref(y1.cpu().numpy(), y2.cpu().numpy(), v.cpu().numpy())
        report("eightpoint_model_matches_heads%d" % len(heads), positive_weights_min=float((v > 0).sum(-1).min()))
        ok = sr[:, 1] > 0                                        # (fewer than eight mutual matches: both say "degenerate")
        if ok.any():
            check_parity("model_heads%d" % len(heads), one.E[torch.from_numpy(ok)], one.stat[torch.from_numpy(ok)], Er[ok], sr[ok])
        assert not Er[~ok].any() and not bool(one.E[torch.from_numpy(~ok)].any())
    # module state
    assert not m.training and all(not mod.training for mod in m.modules())
    after = m.state_dict()
    assert set(after) == set(state) and all(torch.equal(after[k], state[k]) for k in state)
    assert all(torch.equal(v, buffers[k]) for k, v in m.named_buffers())
    assert torch.equal(forward(), before)
    assert all(p.grad is None for p in m.parameters())


def test_model_refusals(ep):
    images = torch.zeros(1, 2, 3, 64, 64, device="cuda")
    intr = torch.ones(1, 2, 4, device="cuda")
    m = _model()
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.pose_from_matches(images, intr)
    m.eval()
    _bf16_configuration(True)
    try:
        with pytest.raises(NotImplementedError):
            m.pose_from_matches(torch.zeros(1, 2, 3, 384, 384, device="cuda"), intr)
    finally:
        _bf16_configuration(False)
    with pytest.raises(ValueError, match="noess"):
        _model(noess="1").eval().pose_from_matches(torch.zeros(1, 2, 3, 384, 384, device="cuda"), intr)


def test_demo_eight_point_flag(capsys, repeatable_cnn):
    import re
    sys.path.insert(0, ROOT)
    import demo
    g = os.path.join(ROOT, "tests", "golden", "demo")
    argv = ["--img1", os.path.join(g, "matterport_1.png"), "--img2", os.path.join(g, "matterport_2.png")]
    torch.manual_seed(5)
    plain = demo.main(argv)
    out_plain = capsys.readouterr().out
    torch.manual_seed(5)
    flagged = demo.main(argv + ["--eight_point"])
    out_flagged = capsys.readouterr().out
    assert plain.tobytes() == flagged.tobytes()
    assert "eight-point" not in out_plain and out_flagged.startswith(out_plain)
    extra = out_flagged[len(out_plain):].splitlines()
    assert len(extra) == 1 and extra[0].startswith("eight-point pose ")
    numbers = [float(t) for t in re.findall(r"-?\d+\.\d+", extra[0])]
    assert len(numbers) == 7 + 2 and all(np.isfinite(numbers))
    pose, angles = np.array(numbers[:7]), numbers[7:]
    assert abs(np.linalg.norm(pose[:3]) - 1) < 1e-4 and abs(np.linalg.norm(pose[3:]) - 1) < 1e-4 and pose[6] >= 0
    assert 0 <= angles[0] <= 180.001 and 0 <= angles[1] <= 180.001
