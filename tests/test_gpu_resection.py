"""rp_p3p_consensus, rp_pnp_refine (include/relpose_resection.h, csrc_resection/resection.hip) and what is built on them, on a real
MI355X.

The reference is tests/_resection_ref.py: every routine of the header in fp64, the three-point solver checked by a second route
(numpy.roots on the quartic) in tests/test_resection_cpu.py.  Every bound is C eps32 scale(ref) with C = 8 x the worst ratio of the
float32 restatement of the kernels' arithmetic on these same inputs, measured on the CPU and asserted by
tests/test_resection_cpu.py::test_float32_restatement_is_within_the_calibrated_bounds (T.WORST); nothing was fixed in advance.
    samples   equal the reference's exactly
    hyp_pose  | |q| - 1 | <= C_UNIT eps32, w >= 0, on every valid hypothesis; the sample's three rows reproduced: the largest residual
              <= C_REPRO eps32 lever, lever = (|X| + |t|) (1 + |x|) / m_z of the row, on the hypotheses whose reference decisions (real
              or complex root pair, the gates of a solution) are at least 1e-6 away from their thresholds -- a rule of the reference alone;
              left out: at most 0.8 %, cap 5 %, asserted
    hyp_cost  against the fp64 cost of the device's OWN hyp_pose, C_COST eps32 (sqrt(c) + eps32) plus the horizon term
    w_out     against the fp64 weights at the device's own pose, over eps32 / tau
    refine    pose <= C_REFINE eps32 kappa, kappa the condition number of the reference's scaled normal matrix, after 1 and 10 iterations
Winners are compared by cost through the bounds, never by index.  The device's own ratios go to the test report."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import _consensus_ref as C
from tests import _resection_ref as T
from tests.test_gpu_kernels import report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rs():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, resection
    _lib.load()
    _lib.load_resection()
    return resection


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to_numpy(out, cls):
    return cls(*[None if t is None else t.detach().cpu().numpy() for t in out])


def np_consensus(out):
    return T.Consensus(*[None if t is None else t.detach().cpu().numpy() for t in out], None)


IDS = ["%s-n%d-P%d-M%d-%s" % (k, n, P, M, "w" if wt else "now") for k, n, P, M, wt in T.CASES]


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_consensus_against_the_reference(rs, case):
    kind, n, P, M, weighted = case
    X, x, w = T.inputs(*case)
    ref = T.reference(*case)
    dout = rs.p3p_consensus(dev(X), dev(x), dev(w), tau=T.TAU, hypotheses=M, seed=T.SEED, return_weights=True, return_samples=True)
    assert dout.pose.shape == (n, 7) and dout.best.shape == (n,) and dout.stat.shape == (n, 4) and dout.weights.shape == (n, P)
    assert dout.hyp_pose.shape == (n, M, 7) and dout.hyp_cost.shape == (n, M) and dout.hyp_count.shape == (n, M) and dout.samples.shape == (n, M, 3)
    assert dout.best.dtype == torch.int32 and dout.samples.dtype == torch.int32 and dout.hyp_count.dtype == torch.int32
    out = np_consensus(dout)
    assert all(np.isfinite(a).all() for a in out if a is not None)
    assert np.array_equal(out.samples, ref.samples)
    r = T.check_consensus(out, ref, X, x, w)
    report("resection_consensus_" + IDS[T.CASES.index(case)].replace("-", "_"), **r)
    # bit-identical from call to call, with and without the optional outputs
    again = rs.p3p_consensus(dev(X), dev(x), dev(w), tau=torch.full((n,), T.TAU, device="cuda"), hypotheses=M, seed=T.SEED)
    assert again.weights is None and again.samples is None
    assert all(torch.equal(a, b) for a, b in zip(dout[:3] + dout[4:7], again[:3] + again[4:7]))


RIDS = ["%s-n%d-P%d-%s" % (k, n, P, "w" if wt else "now") for k, n, P, wt in T.REFINE_CASES]


@pytest.mark.parametrize("case", T.REFINE_CASES, ids=RIDS)
def test_refinement_against_the_reference(rs, case):
    """one step and converged against the fp64 reference at C eps32 kappa; iters = 0 is the scorer and returns (t0, unit(q0)); its cost and
    the consensus' cost of the same pose agree within the two cost bounds; pose may alias pose0; the cost never rises"""
    kind, n, P, weighted = case
    X, x, w, p0 = T.refine_inputs(*case)
    a, b, ww, r0 = dev(X), dev(x), dev(w), dev(p0)
    wc = C.clamp(w, n, P)
    figures = {}
    for iters in (1, 10):
        ref = T.refine_reference(*case, iters)
        d = rs.pnp_refine(a, b, ww, r0, tau=T.TAU, iters=iters, return_weights=True)
        o = to_numpy(d, rs.PnPRefined)
        assert all(np.isfinite(t).all() for t in o)
        r = T.refine_ratios(o.pose, o.stat, o.weights, ref, X, x, w)
        print("iters %d: pose ratio %.3g (C %.3g), unit %.3g (C %.3g), cost %.3g, w %.3g; kappa %.1f .. %.1f; accepted %s (reference %s)"
              % (iters, r["pose"], T.C_REFINE[iters], r["unit"], T.C_UNIT, r["cost"], r["w"], ref.kappa.min(), ref.kappa.max(), o.stat[:, 2], ref.stat[:, 2]))
        figures.update({"%s_%d" % (k, iters): v for k, v in r.items()})
        assert r["pose"] <= T.C_REFINE[iters] and r["unit"] <= T.C_UNIT and r["cost"] <= T.C_COST and r["w"] <= T.C_W, r
        assert bool((o.pose[:, 6] >= 0).all()) and np.array_equal(o.stat[:, 3], (wc > 0).sum(-1))
    report("resection_refine_" + RIDS[T.REFINE_CASES.index(case)].replace("-", "_"), **figures)
    score = rs.pnp_refine(a, b, ww, r0, tau=T.TAU, iters=0)
    assert bool((d.stat[:, 0] <= score.stat[:, 0]).all()) and not score.stat[:, 2].any() and score.weights is None
    one = rs.pnp_refine(a, b, ww, r0, tau=T.TAU, iters=1)
    assert bool((one.stat[:, 0] <= score.stat[:, 0]).all()) and bool((d.stat[:, 0] <= one.stat[:, 0]).all())       # the cost never rises
    # iters = 0: (t0, unit(q0)) -- t0 bit for bit, q0 came normalised -- and the fp64 cost of ITS pose
    assert torch.equal(score.pose[:, :3], r0[:, :3]) and float((score.pose[:, 3:] - r0[:, 3:]).abs().max()) <= T.C_UNIT * T.EPS32
    sp = score.pose.cpu().numpy()
    own = T.cost64(sp, X, x, wc, T.TAU)
    bound = T.cost_bound(own, T.C_COST, T.horizon(sp, X, x, wc, T.TAU))
    assert bool((np.abs(score.stat[:, 0].cpu().numpy() - own) <= bound).all())
    # a scaled quaternion is the same start
    scaled = r0.clone()
    scaled[:, 3:] *= -2.5
    sc = rs.pnp_refine(a, b, ww, scaled, tau=T.TAU, iters=0)
    assert float((sc.pose - score.pose).abs().max()) <= T.C_UNIT * T.EPS32
    # the consensus reports the same cost for the same pose: its winner scored by iters = 0, within the two cost bounds
    c = rs.p3p_consensus(a, b, ww, tau=T.TAU, hypotheses=64, seed=T.SEED)
    s2 = rs.pnp_refine(a, b, ww, c.pose, tau=T.TAU, iters=0)
    cp = c.pose.cpu().numpy()
    own = T.cost64(cp, X, x, wc, T.TAU)
    bound = T.cost_bound(own, T.C_COST, T.horizon(cp, X, x, wc, T.TAU))
    assert bool((c.best >= 0).all()) and bool((np.abs((c.stat[:, 0] - s2.stat[:, 0]).cpu().numpy()) <= 2 * bound).all())
    assert torch.equal(c.stat[:, 3], s2.stat[:, 3])
    # aliasing and call-to-call identity
    alias, taus = r0.clone(), torch.full((n,), T.TAU, device="cuda")
    stat = torch.empty_like(d.stat)
    P_ = ctypes.c_void_p
    d2 = rs._lib.load_resection().rp_pnp_refine(P_(a.data_ptr()), P_(b.data_ptr()), None if ww is None else P_(ww.data_ptr()),
                                                P_(taus.data_ptr()), P_(alias.data_ptr()), 10, P_(alias.data_ptr()), P_(stat.data_ptr()),
                                                None, P, n, P_(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert d2 == 0 and torch.equal(alias, d.pose) and torch.equal(stat, d.stat)


def test_degenerate_problems_in_a_batch(rs):
    """tau 0, negative and NaN; two positive weights (plus a negative one and a NaN); every point the same, where every hypothesis is
    invalid and best = -1; pose0 zero, with a NaN, with an infinity -- each between healthy neighbours, whose bits do not change"""
    n, P = 13, 40
    X, x, _ = T.exact_rows(n, P, 12)
    w = np.random.default_rng(1).uniform(0.05, 1, (n, P)).astype(np.float32)
    tau = np.full(n, T.TAU, np.float32)
    kw = dict(hypotheses=70, seed=3, return_weights=True, return_samples=True)
    healthy = rs.p3p_consensus(dev(X), dev(x), dev(w), tau=dev(tau), **kw)
    hr = rs.pnp_refine(dev(X), dev(x), dev(w), healthy.pose, tau=dev(tau), iters=3, return_weights=True)
    assert bool((healthy.best >= 0).all())
    tau[1], tau[3], tau[5] = 0, -0.02, np.nan
    w[7] = 0
    w[7, [9, 11]] = 0.5
    w[7, 4], w[7, 8] = -1.0, np.nan
    X = X.copy()
    X[9, :] = X[9, 0]
    a, b = dev(X), dev(x)
    out = rs.p3p_consensus(a, b, dev(w), tau=dev(tau), **kw)
    o = np_consensus(out)
    wc = C.clamp(w, n, P, np.float32)
    for i, K in ((1, 40), (3, 40), (5, 40), (7, 2), (9, 40)):
        assert not o.pose[i].any() and o.best[i] == -1 and np.array_equal(o.stat[i], [0, 0, 0, K]), (i, o.stat[i])
        assert np.array_equal(o.weights[i], wc[i]) and not o.hyp_pose[i].any() and bool((o.hyp_cost[i] == np.float32(T.FLT_MAX)).all())
        assert not o.hyp_count[i].any()
    assert not o.samples[7].any() and o.samples[9].any() and np.array_equal(o.samples, T.sample_rows3(w, n, P, 3, 70)[1])
    assert all(np.isfinite(t).all() for t in o if t is not None)
    keep = [0, 2, 4, 6, 8, 10, 11, 12]
    assert all(torch.equal(p[keep], q[keep]) for p, q in zip(out, healthy))
    # the refinement leaves a degenerate problem alone: pose0 copied bit for bit, stat = (0, 0, 0, K), the clamped weights
    bad = healthy.pose.clone()
    bad[11] = 0                                                       # the zero pose the consensus writes for a degenerate problem
    bad[1, 2] = float("nan")                                          # (tau = 0 there, too)
    bad[10, 4] = float("inf")
    r = rs.pnp_refine(a, b, dev(w), bad, tau=dev(tau), iters=3, return_weights=True)
    for i, K in ((1, 40), (3, 40), (5, 40), (7, 2), (10, 40), (11, 40)):
        assert torch.equal(r.pose[i].view(torch.int32), bad[i].view(torch.int32)), i
        assert r.stat[i].cpu().tolist() == [0, 0, 0, K] and np.array_equal(r.weights[i].cpu().numpy(), wc[i])
    keep = [0, 2, 4, 6, 8, 12]
    assert all(torch.equal(p[keep], q[keep]) for p, q in zip(r, hr))
    assert all(bool(torch.isfinite(t[[i for i in range(n) if i not in (1, 10)]]).all()) for t in r)


def test_refusals(rs):
    """every refusal returns its code before any launch, one call each, in the documented order: shape, then size, then alignment"""
    from rel_pose_amd import _lib
    X, x = torch.rand(2, _lib.RESECTION_MAX_P + 1, 3, device="cuda"), torch.rand(2, _lib.RESECTION_MAX_P + 1, 2, device="cuda")
    p0 = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device="cuda").repeat(2, 1)
    with pytest.raises(RuntimeError, match=r"rel_pose_amd: rp_p3p_consensus failed: unsupported \(RP error -4\)"):
        rs.p3p_consensus(X, x)
    Y, y = X[:, :64].contiguous(), x[:, :64].contiguous()
    with pytest.raises(RuntimeError, match=r"unsupported \(RP error -4\)"):
        rs.p3p_consensus(Y, y, hypotheses=_lib.RESECTION_MAX_M + 1)
    with pytest.raises(RuntimeError, match=r"bad shape \(RP error -1\)"):
        rs.p3p_consensus(Y[:, :2].contiguous(), y[:, :2].contiguous())
    with pytest.raises(RuntimeError, match=r"bad shape \(RP error -1\)"):
        rs.p3p_consensus(Y, y, hypotheses=0)
    with pytest.raises(RuntimeError, match=r"bad shape \(RP error -1\)"):                    # shape before size
        rs.p3p_consensus(Y[:, :2].contiguous(), y[:, :2].contiguous(), hypotheses=_lib.RESECTION_MAX_M + 1)
    with pytest.raises(RuntimeError, match=r"rp_pnp_refine failed: unsupported \(RP error -4\)"):
        rs.pnp_refine(Y, y, None, p0, iters=_lib.RESECTION_MAX_ITERS + 1)
    with pytest.raises(RuntimeError, match=r"rp_pnp_refine failed: unsupported \(RP error -4\)"):
        rs.pnp_refine(X, x, None, p0)
    with pytest.raises(RuntimeError, match=r"rp_pnp_refine failed: bad shape \(RP error -1\)"):
        rs.pnp_refine(Y, y, None, p0, iters=-1)
    # size before alignment, and alignment itself: x four bytes off an 8-byte boundary
    lib, P_ = _lib.load_resection(), ctypes.c_void_p
    buf = torch.zeros(4096, device="cuda")
    ptr = lambda k: P_(buf.data_ptr() + 256 * k)                                            # noqa: E731
    args = [ptr(1), P_(buf.data_ptr() + 512 + 4), None, ptr(3), 1, ptr(4), ptr(5), ptr(6), None, ptr(7), ptr(8), None, None]
    with pytest.raises(RuntimeError, match=r"misaligned pointer/stride \(RP error -2\)"):
        lib.rp_p3p_consensus(*args, 4, 2, 1, None)
    with pytest.raises(RuntimeError, match=r"unsupported \(RP error -4\)"):
        lib.rp_p3p_consensus(*args, 4, _lib.RESECTION_MAX_M + 1, 1, None)
    torch.cuda.synchronize()
    assert not buf.any()                                                                    # nothing was launched


def test_identity_invariant_c_equals_a_on_the_device(rs):
    """with c = a (x_c = x_a, noise-free) the device's resection returns pose_a with |t| = 1: within twice the first-order shift N^-1 g
    of the minimiser that the float32 rounding of the rows causes (tests/test_resection_cpu.py) plus the refinement's own bound
    C_REFINE eps32 kappa"""
    scs = [T.three_views(seed, 576, 0.0, 0.0) for seed in range(4)]
    Xs, ws = [], []
    for sc in scs:
        X, z1, z2, d2, phi = T.triangulate64(sc.pose_a, sc.x1, sc.xa)
        Xs.append(X.astype(np.float32))
        ws.append(T.row_weights(z1, z2, d2, phi, T.TAU).astype(np.float32))
    X, x, w = np.stack(Xs), np.stack([sc.xa for sc in scs]), np.stack(ws)
    c = rs.p3p_consensus(dev(X), dev(x), dev(w), tau=T.TAU, hypotheses=256, seed=0)
    r = rs.pnp_refine(dev(X), dev(x), dev(w), c.pose, tau=T.TAU, iters=10)
    pose = r.pose.cpu().numpy().astype(np.float64)
    figures = {}
    for b, sc in enumerate(scs):
        N, g = T.normal_equations(sc.pose_a, X[b], x[b], w[b].astype(np.float64), T.TAU ** 2)
        kappa = T.H.scaled_condition(N)
        bound = 2 * np.abs(np.linalg.solve(N, g)).max() + T.C_REFINE[10] * T.EPS32 * kappa
        err, scale = np.abs(pose[b] - sc.pose_a).max(), np.linalg.norm(pose[b, :3])
        print("scene %d: |pose - pose_a| %.3g, |t| - 1 = %.3g, bound %.3g (kappa %.1f)" % (b, err, scale - 1, bound, kappa))
        figures["err_%d" % b], figures["bound_%d" % b] = float(err), float(bound)
        assert int(c.best[b]) >= 0 and err <= bound and abs(scale - 1) <= bound
    report("resection_identity_invariant", **figures)


# ------------------------------------------------------------------------------------------------ model level
def _same(p, q):
    return all((a is None and b is None) or (torch.equal(a, b) if torch.is_tensor(a) else a == b if isinstance(a, (str, type(None))) else _same(a, b))
               for a, b in zip(p, q))


def test_model_third_view_pose_is_the_chain_of_the_public_pieces(rs):
    """third_view_pose_from_matches equals structure_from_matches on the 2B pairs -> row_weights -> p3p_consensus -> pnp_refine called by
    hand, bit for bit; the model's state and `intrinsics` are what they were; training mode is refused as by every chain"""
    from oracle import relpose_oracle as O
    from rel_pose_amd import triangulate
    from tests.test_gpu_memory_contract import _model
    m = _model().eval()
    B = 2
    images = O.synthetic_images(2 * B, 384, 384, key=81).cuda()
    images = torch.stack([images[:B, 0], images[:B, 1], images[B:, 1]], 1).contiguous()              # (hub, a, c)
    intr = torch.tensor([[0.9 * 384, 0.8 * 384, 192.0, 192.0]]).repeat(B, 3, 1).contiguous().cuda()
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        m.correspondences(images[:, :2].contiguous())                # (warm-up)
        state = {k: v.clone() for k, v in m.state_dict().items()}
        before = intr.clone()
        tv = m.third_view_pose_from_matches(images, intr, hypotheses=128, seed=5, iters=3)
        again = m.third_view_pose_from_matches(images, intr, hypotheses=128, seed=5, iters=3)
        pairs = torch.cat([images[:, [0, 1]], images[:, [0, 2]]]).contiguous()
        ms = m.structure_from_matches(pairs, torch.cat([intr[:, [0, 1]], intr[:, [0, 2]]]).contiguous(), chain="consensus", seed=5)
    finally:
        torch.backends.cudnn.deterministic = keep
    assert torch.equal(intr, before) and all(torch.equal(v, m.state_dict()[k]) for k, v in state.items()) and not m.training
    assert _same(tv, again)
    st = triangulate.Structure(*[t[:B].contiguous() for t in ms.structure])
    w = rs.row_weights(st, ms.weights[:B].contiguous(), ms.weights[B:].contiguous(), ms.tau[:B].contiguous())
    c = rs.p3p_consensus(st.points, ms.x2[B:].contiguous(), w, tau=ms.tau[B:].contiguous(), hypotheses=128, seed=5)
    r = rs.pnp_refine(st.points, ms.x2[B:].contiguous(), w, c.pose, tau=ms.tau[B:].contiguous(), iters=3)
    assert torch.equal(tv.weights, w) and torch.equal(tv.pose_c, r.pose) and torch.equal(tv.stat, r.stat)
    assert torch.equal(tv.pose_a, ms.pose[:B]) and torch.equal(tv.scale, r.pose[:, :3].norm(dim=-1))
    assert torch.equal(tv.two_view_c.pose, ms.chain.pose[B:]) and _same(tv.structure.structure, st)
    assert tv.pose_c.shape == (B, 7) and bool(torch.isfinite(tv.pose_c).all()) and tv.weights.shape == (B, 1728)
    # tau as a number reaches every piece as [2B]; [B] means one per triple
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        t1 = m.third_view_pose_from_matches(images, intr, hypotheses=128, seed=5, iters=3, tau=0.02)
        t2 = m.third_view_pose_from_matches(images, intr, hypotheses=128, seed=5, iters=3, tau=torch.full((B,), 0.02))
        others = [m.third_view_pose_from_matches(images, intr, chain=ch, hypotheses=64, seed=5, iters=3) for ch in ("eight", "refined", "planar")]
    finally:
        torch.backends.cudnn.deterministic = keep
    assert _same(t1, t2) and torch.equal(t1.structure.tau, torch.full((B,), 0.02, device="cuda")) and not torch.equal(t1.weights, tv.weights)
    for o in others:                                              # every chain's result leads with the 2B pairs: two_view_c is its rows B .. 2B - 1
        assert o.two_view_c.pose.shape == (B, 7) and o.pose_c.shape == (B, 7) and o.weights.shape == (B, 1728) and bool(torch.isfinite(o.pose_c).all())
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            m.third_view_pose_from_matches(images, intr)
    finally:
        m.eval()


def test_demo_third_flag(capsys):
    """demo.py --eight_point --third on the golden pair with image 2 again as the third image: the pose line in the usual format and
    the baseline ratio.  The run is seeded, so the outcome is fixed: the third view IS determined.  With c = a the matches of the two
    pairs are the same rows, pose_a reproduces every used row to within its epipolar correction, and the ratio must come out near 1:
    within the 10 % that DESIGN 5.14 counts as "the scale is determined" (measured: 0.9997 over 15 usable points)"""
    sys.path.insert(0, ROOT)
    import demo
    g = os.path.join(ROOT, "tests", "golden", "demo")
    argv = ["--img1", os.path.join(g, "matterport_1.png"), "--img2", os.path.join(g, "matterport_2.png"), "--eight_point",
            "--third", os.path.join(g, "matterport_2.png")]
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        torch.manual_seed(5)
        demo.main(argv)
        out = capsys.readouterr().out.splitlines()
        torch.manual_seed(5)
        demo.main(argv)
        again = capsys.readouterr().out.splitlines()
    finally:
        torch.backends.cudnn.deterministic = keep
    assert out == again
    lines = [l for l in out if l.startswith("third view")]
    print("\n".join(lines))
    assert len(lines) == 2, lines
    assert lines[0].startswith("third view pose x,y,z,qx,qy,qz,qw: ")
    pose = np.array([float(t) for t in lines[0].split(": ")[1].split()])
    assert pose.shape == (7,) and abs(np.linalg.norm(pose[3:]) - 1) < 1e-4 and pose[6] >= 0
    m = re.fullmatch(r"third view: baseline ratio \|t_c\| / \|t_a\| = (\S+) ; inlier weight share (\S+) over (\d+) points ; against the "
                     r"two-view chain for \(img1, img3\): rotation differs by (\S+) deg, translation direction by (\S+) deg", lines[1])
    assert m, lines[1]
    ratio, share, count, rot, dirn = (float(t) for t in m.groups())
    assert abs(ratio - 1) <= 0.1 and abs(ratio - np.linalg.norm(pose[:3])) < 1e-4
    assert 0 < share <= 1 and count >= 3 and 0 <= rot <= 180 and 0 <= dirn <= 180
    report("resection_demo_third", ratio=ratio, share=share, points=count, rotation_deg=rot, direction_deg=dirn)


def test_demo_third_says_not_determined_for_a_degenerate_result(rs, capsys):
    """demo.print_third on a constructed degenerate input: two usable points only.  The ThirdView is what the real kernels return for
    it (pose 0, best -1, stat (0, 0, 0, 2)), handed to the printer by a stand-in for the model; one line, `not determined`"""
    sys.path.insert(0, ROOT)
    import demo
    X, x, _ = T.exact_rows(1, 40, 12)
    w = np.zeros((1, 40), np.float32)
    w[0, [9, 11]] = 0.5
    c = rs.p3p_consensus(dev(X), dev(x), dev(w), tau=T.TAU, hypotheses=32, seed=0)
    r = rs.pnp_refine(dev(X), dev(x), dev(w), c.pose, tau=T.TAU, iters=3)
    assert int(c.best[0]) == -1 and not r.pose.any() and r.stat[0].tolist() == [0, 0, 0, 2]
    chain = rs.PnPRefined(torch.tensor([[0, 0, 1, 0, 0, 0, 1.0]], device="cuda"), r.stat, None)

    class StandIn:
        def third_view_pose_from_matches(self, images, intrinsics, **kw):
            return rs.ThirdView(chain.pose, r.pose, r.pose[:, :3].norm(dim=-1), r.stat, None, chain, dev(w))
    demo.print_third(StandIn(), torch.zeros(1, 3, 3, 384, 512, device="cuda"), [[517.97, 517.97, 320, 240]] * 2, (480, 640))
    out = capsys.readouterr().out.splitlines()
    assert out == ["third view: not determined (2 usable points)"]
