"""rp_homography_consensus, rp_homography_refine, rp_pose_from_homography (include/relpose_homography.h,
csrc_homography/homography.hip) and what is built on them, on a real MI355X.

The reference is tests/_homography_ref.py: every routine of the header in fp64 with LAPACK (the null vector by SVD, the 3 x 3 SVD), the
decomposition checked against a second route.  Every bound is C eps32 scale(ref) with C = 8 x the worst ratio of the float32
restatement of the kernels' arithmetic on these same inputs, measured on the CPU and asserted by tests/test_homography_cpu.py (the
test_*_restatement_is_within_the_calibrated_bounds tests); nothing was fixed in advance.
    hyp_H     error up to sign <= C_H eps32 sigma_1 / sigma_8 of the reference's 8 x 9 matrix (restatement 2.98 -> C_H = 23.9), on the
              hypotheses with sigma_1 / sigma_8 <= 1e4 -- a rule of the reference alone; left out: at most 2.5 %, cap 10 %, asserted
    hyp_cost  against the fp64 cost of the device's OWN hyp_H, the form of tests/_consensus_ref.py, C eps32 (sqrt(c) + eps32), plus the
              horizon term of _homography_ref.horizon (a row whose h3 . x1h is within rounding of 0); restatement 2.44 -> C_COST = 19.6
    w_out     against the fp64 weights at the device's own H, over eps32 / tau: 0.638 -> C_W = 5.11
    refine    H up to sign <= C eps32 kappa, kappa the condition number of the reference's scaled normal matrix: one step 0.184 -> 1.48,
              converged (10 iterations) 30.7 -> 246 -- float32 stops accepting steps about 1e-5 short of where fp64 ends
    decompose candidates matched up to their order (it follows the signs of the singular vectors), worst entry of (t, q, n) <=
              C eps32 decomposition_scale(sigma): 2.51 -> 20.1, flat from |t|/d = 1e-3 to 3; Sampson cost 0.333 -> 2.67; visibility
              beyond the horizon band 0.692 -> 5.54 eps32
Winners are compared by cost through the bounds, never by index.  The device's own ratios go to the test report."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _consensus_ref as C
from tests import _homography_ref as H
from tests.test_gpu_kernels import report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hg():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, homography
    _lib.load()
    _lib.load_homography()
    return homography


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to_numpy(out, cls):
    return cls(*[None if t is None else t.detach().cpu().numpy() for t in out])


def np_consensus(out):
    return H.Consensus(*[None if t is None else t.detach().cpu().numpy() for t in out], None)


IDS = ["%s-n%d-P%d-M%d-%s" % (k, n, P, M, "w" if wt else "now") for k, n, P, M, wt in H.CASES]


@pytest.mark.parametrize("case", H.CASES, ids=IDS)
def test_consensus_against_the_reference(hg, case):
    kind, n, P, M, weighted = case
    x1, x2, w = H.inputs(*case)
    ref = H.reference(*case)
    dout = hg.homography_consensus(dev(x1), dev(x2), dev(w), tau=H.TAU, hypotheses=M, seed=H.SEED, return_weights=True, return_samples=True)
    assert dout.H.shape == (n, 3, 3) and dout.best.shape == (n,) and dout.stat.shape == (n, 4) and dout.weights.shape == (n, P)
    assert dout.hyp_H.shape == (n, M, 3, 3) and dout.hyp_cost.shape == (n, M) and dout.samples.shape == (n, M, 4)
    assert dout.best.dtype == torch.int32 and dout.samples.dtype == torch.int32
    out = np_consensus(dout)
    assert all(np.isfinite(a).all() for a in out if a is not None)
    assert np.array_equal(out.samples, ref.samples)
    valid = out.hyp_cost < H.FLT_MAX
    nrm = np.linalg.norm(out.hyp_H.reshape(n, M, 9), axis=-1)
    assert np.abs(nrm[valid] - 1).max(initial=0) <= 4 * H.EPS32 and not out.hyp_H[~valid].any()
    lead = np.take_along_axis(out.hyp_H.reshape(n, M, 9), np.abs(out.hyp_H.reshape(n, M, 9)).argmax(-1)[..., None], -1)[..., 0]
    assert bool((lead[valid] > 0).all())
    r = H.check_consensus(out, ref, x1, x2, w)
    report("homography_consensus_" + IDS[H.CASES.index(case)].replace("-", "_"), **r)
    # bit-identical from call to call, with and without the optional outputs
    again = hg.homography_consensus(dev(x1), dev(x2), dev(w), tau=torch.full((n,), H.TAU, device="cuda"), hypotheses=M, seed=H.SEED)
    assert again.weights is None and again.samples is None
    assert all(torch.equal(a, b) for a, b in zip(dout[:3] + dout[4:6], again[:3] + again[4:6]))


@pytest.mark.parametrize("n,P,weighted", H.REFINE_CASES, ids=["n%d-P%d-%s" % (n, P, "w" if wt else "now") for n, P, wt in H.REFINE_CASES])
def test_refinement_against_the_reference(hg, n, P, weighted):
    """one step and converged against the fp64 reference at C eps32 kappa; iters = 0 is the scorer; H may alias H0; the cost never rises"""
    x1, x2, w, H0 = H.refine_inputs(n, P, weighted)
    a, b, ww, h0 = dev(x1), dev(x2), dev(w), dev(H0)
    figures = {}
    for iters in (1, 10):
        ref = H.refine_reference(n, P, weighted, iters)
        d = hg.homography_refine(a, b, ww, h0, tau=H.TAU, iters=iters, return_weights=True)
        o = to_numpy(d, hg.RefinedHomography)
        assert all(np.isfinite(t).all() for t in o)
        r = H.refine_ratios(o.H, o.stat, o.weights, ref, x1, x2, w)
        print("iters %d: H ratio %.3g (C %.3g), cost %.3g, w %.3g; kappa %.1f .. %.1f; accepted %s (reference %s)"
              % (iters, r["H"], H.C_REFINE_H[iters], r["cost"], r["w"], ref.kappa.min(), ref.kappa.max(), o.stat[:, 2], ref.stat[:, 2]))
        figures.update({"%s_%d" % (k, iters): v for k, v in r.items()})
        assert r["H"] <= H.C_REFINE_H[iters] and r["cost"] <= H.C_COST and r["w"] <= H.C_W, r
        assert np.abs(np.linalg.norm(o.H.reshape(n, 9), axis=-1) - 1).max() <= 4 * H.EPS32
        assert np.array_equal(o.stat[:, 3], (C.clamp(w, n, P) > 0).sum(-1))
    report("homography_refine_n%d_P%d_w%d" % (n, P, weighted), **figures)
    score = hg.homography_refine(a, b, ww, h0, tau=H.TAU, iters=0)
    assert bool((d.stat[:, 0] <= score.stat[:, 0]).all()) and not score.stat[:, 2].any() and score.weights is None
    assert float((score.H - h0).abs().max()) <= 4 * H.EPS32                     # H0 came normalised, with the sign rule
    # aliasing and call-to-call identity
    alias, taus = h0.clone(), torch.full((n,), H.TAU, device="cuda")
    d2 = hg._lib.load_homography().rp_homography_refine(ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()),
                                                       None if ww is None else ctypes.c_void_p(ww.data_ptr()),
                                                       ctypes.c_void_p(taus.data_ptr()),
                                                       ctypes.c_void_p(alias.data_ptr()), 10, ctypes.c_void_p(alias.data_ptr()),
                                                       ctypes.c_void_p(score.stat.data_ptr()), None, P, n,
                                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert d2 == 0 and torch.equal(alias, d.H) and torch.equal(score.stat, d.stat)


@pytest.mark.parametrize("kind", H.DECOMPOSE_KINDS)
def test_decomposition_against_the_reference(hg, kind):
    """refined homographies of the ten 30 % scenes, 130 exact scenes, and the edge cases among healthy neighbours"""
    inp = H.decompose_inputs(kind)
    Hm, x1, x2, w = inp
    ref = H.decompose_reference(kind)
    d = hg.pose_from_homography(dev(Hm), dev(x1), dev(x2), dev(w), tau=H.TAU)
    o = H.Poses(*[t.detach().cpu().numpy() for t in d], ref.sigma)
    assert all(np.isfinite(t).all() for t in o[:4])
    r = H.decompose_ratios(o, ref, inp)
    print("pose ratio %.3g (C %.3g), cost %.3g (C %.3g), visibility %.3g (C %.3g)"
          % (r["pose"].max(), H.C_DECOMPOSE, r["cost"].max(), H.C_DECOMPOSE_COST, r["vis"].max(), H.C_VIS))
    report("homography_decompose_" + kind, pose=float(r["pose"].max()), cost=float(r["cost"].max()), vis=float(r["vis"].max()))
    assert r["pose"].max() <= H.C_DECOMPOSE and r["cost"].max() <= H.C_DECOMPOSE_COST and r["vis"].max() <= H.C_VIS
    n = len(Hm)
    valid = o.cstat[..., 3] == 1
    assert np.abs(np.linalg.norm(o.pose[..., 3:], axis=-1)[valid] - 1).max() <= 4 * H.EPS32 and bool((o.pose[..., 6][valid] >= 0).all())
    for b in range(n):                                               # pick follows the device's own cstat by the header's rule
        order = sorted((k for k in range(4) if valid[b, k]), key=lambda k: (0 if o.cstat[b, k, 0] >= np.float32(0.99) else 1, o.cstat[b, k, 1], k))
        assert o.pick[b].tolist() == (order + [-1, -1])[:2]
    again = hg.pose_from_homography(dev(Hm), dev(x1), dev(x2), dev(w), tau=H.TAU)
    assert all(torch.equal(p, q) for p, q in zip(d, again))
    if kind == "edge":                                               # the healthy neighbours do not feel the edge cases between them
        kinds = H.edge_batch()[0]
        keep = [i for i, k in enumerate(kinds) if k == "healthy"]
        alone = hg.pose_from_homography(dev(Hm[keep]), dev(x1[keep]), dev(x2[keep]), None, tau=H.TAU)
        assert all(torch.equal(p[keep], q) for p, q in zip(d, alone))


@pytest.mark.parametrize("outliers", [0.3, 0.5])
def test_the_ten_scene_tables_through_the_c_abi(hg, outliers):
    """the tables of tests/test_homography_cpu.py on the device: the truth is among the candidates in 10 of 10, among the two picked in
    10 of 10, visibility decides 6 of 10 correctly; every scene is a call of its own (problem index 0), as the reference's table"""
    rows = H.table(outliers)
    errs, in_pick, decided = [], 0, 0
    for r in rows:
        sc = r[4]
        a, b = dev(sc.x1), dev(sc.x2)
        c = hg.homography_consensus(a, b, None, tau=H.TAU, hypotheses=256, seed=H.SEED)
        f = hg.homography_refine(a, b, None, c.H, tau=H.TAU, iters=10)
        d = hg.pose_from_homography(f.H, a, b, None, tau=H.TAU, vis_min=0.99)
        pose, normal, cstat, pick = [t[0].cpu().numpy() for t in d]
        e = H.candidate_error(pose, normal, cstat, sc.R, sc.t, sc.n)
        errs.append(e[:3])
        in_pick += e[3] in pick.tolist()
        passing = int(((cstat[:, 3] == 1) & (cstat[:, 0] >= np.float32(0.99))).sum())
        decided += passing == 1 and pick[0] == e[3]
        assert passing == r[3]
    errs = np.array(errs)
    ref = np.array([r[0] for r in rows])
    print("device: E %.4f rot %.3f t %.3f; reference: E %.4f rot %.3f t %.3f" % (tuple(errs.max(0)) + tuple(ref.max(0))))
    report("homography_table_%d" % int(100 * outliers), E=float(errs[:, 0].max()), rot=float(errs[:, 1].max()), t=float(errs[:, 2].max()))
    assert int((errs[:, 0] <= 0.02).sum()) == 10 and in_pick == 10 and decided == 6
    # the device's H is within C eps32 kappa of the reference's (converged), and E follows through the decomposition's scale
    bound = np.array([2 * H.C_REFINE_H[10] * H.EPS32 * r[5].refined.kappa[0] * H.decomposition_scale(r[5].poses.sigma[0]) for r in rows])
    assert bool((np.abs(errs[:, 0] - ref[:, 0]) <= bound).all()), (errs[:, 0], ref[:, 0], bound)


def test_degenerate_problems_in_a_batch(hg):
    """three positive weights (plus a negative one and a NaN) and tau = 0 between healthy problems, through all three entry points: the
    documented outputs, nothing non-finite, and the healthy neighbours bit-identical to the all-healthy batch"""
    x1, x2, Ht = H.exact_scenes(6, 40, 12)[:3]
    w = np.random.default_rng(1).uniform(0.05, 1, (6, 40)).astype(np.float32)
    tau = np.full(6, 0.02, np.float32)
    a, b = dev(x1), dev(x2)
    kw = dict(hypotheses=70, seed=3, return_weights=True, return_samples=True)
    healthy = hg.homography_consensus(a, b, dev(w), tau=dev(tau), **kw)
    hr = hg.homography_refine(a, b, dev(w), healthy.H, tau=dev(tau), iters=3, return_weights=True)
    hd = hg.pose_from_homography(hr.H, a, b, dev(w), tau=dev(tau))
    assert bool((healthy.best >= 0).all())
    w[1] = 0
    w[1, [3, 5, 9]] = 0.5
    w[1, 7], w[1, 8] = -1.0, np.nan
    tau[5] = 0
    out = hg.homography_consensus(a, b, dev(w), tau=dev(tau), **kw)
    o = np_consensus(out)
    wc = C.clamp(w, 6, 40, np.float32)
    for i, K in ((1, 3), (5, 40)):
        assert not o.H[i].any() and o.best[i] == -1 and np.array_equal(o.stat[i], [0, 0, 0, K])
        assert np.array_equal(o.weights[i], wc[i]) and not o.hyp_H[i].any() and bool((o.hyp_cost[i] == np.float32(H.FLT_MAX)).all())
    assert not o.samples[1].any() and o.samples[5].any() and np.array_equal(o.samples, H.sample_rows4(w, 6, 40, 3, 70)[1])
    assert all(np.isfinite(t).all() for t in o if t is not None)
    keep = [0, 2, 3, 4]
    assert all(torch.equal(p[keep], q[keep]) for p, q in zip(out, healthy))
    # the refinement leaves a degenerate problem alone: H0 copied bit for bit, stat = (0, 0, 0, K), the clamped weights
    h0 = healthy.H.clone()
    h0[3] = 0                                                         # and a zero start is degenerate, too
    r = hg.homography_refine(a, b, dev(w), h0, tau=dev(tau), iters=3, return_weights=True)
    for i, K in ((1, 3), (5, 40), (3, 40)):
        assert torch.equal(r.H[i], h0[i]) and r.stat[i].cpu().tolist() == [0, 0, 0, K] and np.array_equal(r.weights[i].cpu().numpy(), wc[i])
    assert all(torch.equal(p[[0, 2, 4]], q[[0, 2, 4]]) for p, q in zip(r, hr)) and bool(torch.isfinite(r.H).all())
    # the decomposition: tau = 0, a zero H, no positive weight -> four invalid candidates, pick = (-1, -1)
    w[2] = -1.0
    d = hg.pose_from_homography(r.H, a, b, dev(w), tau=dev(tau))
    for i in (2, 3, 5):
        assert not d.pose[i].any() and not d.normal[i].any() and not d.cstat[i].any() and d.pick[i].cpu().tolist() == [-1, -1]
    assert all(torch.equal(p[[0, 4]], q[[0, 4]]) for p, q in zip(d, hd)) and all(bool(torch.isfinite(t.float()).all()) for t in d)


def test_a_sample_with_three_collinear_points(hg):
    """P = 4 with three collinear rows: the one possible sample does not break down -- a finite hypothesis, or an invalid one, never a NaN"""
    x1 = np.array([[[0.0, 0.0], [0.1, 0.1], [0.2, 0.2], [0.3, -0.1]]], np.float32)
    x2 = (x1 * 1.1 + 0.01).astype(np.float32)
    out = np_consensus(hg.homography_consensus(dev(x1), dev(x2), None, tau=H.TAU, hypotheses=3, seed=0, return_weights=True))
    assert all(np.isfinite(t).all() for t in out if t is not None)
    d = hg.pose_from_homography(dev(out.H), dev(x1), dev(x2), None, tau=H.TAU)
    assert all(bool(torch.isfinite(t.float()).all()) for t in d)


def test_refusals(hg):
    from rel_pose_amd import _lib
    x = torch.rand(2, _lib.HOMOGRAPHY_MAX_P + 1, 2, device="cuda")
    Hm = torch.eye(3, device="cuda").repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match=r"rel_pose_amd: rp_homography_consensus failed: unsupported \(RP error -4\)"):
        hg.homography_consensus(x, x.clone())
    y = x[:, :64].contiguous()
    with pytest.raises(RuntimeError, match=r"unsupported \(RP error -4\)"):
        hg.homography_consensus(y, y.clone(), hypotheses=_lib.HOMOGRAPHY_MAX_M + 1)
    with pytest.raises(RuntimeError, match=r"bad shape \(RP error -1\)"):
        hg.homography_consensus(y[:, :3].contiguous(), y[:, :3].contiguous())
    with pytest.raises(RuntimeError, match=r"rp_homography_refine failed: unsupported \(RP error -4\)"):
        hg.homography_refine(y, y.clone(), None, Hm, iters=_lib.HOMOGRAPHY_MAX_ITERS + 1)
    with pytest.raises(RuntimeError, match=r"rp_pose_from_homography failed: unsupported \(RP error -4\)"):
        hg.pose_from_homography(Hm, x, x.clone())


# ------------------------------------------------------------------------------------------------ model level
def test_model_planar_pose_from_matches_is_the_chain_of_the_public_pieces(hg):
    """on the synthetic model input of tests/test_gpu_consensus.py: planar_pose_from_matches equals assemble_matches -> consensus ->
    refine on the base weights -> decomposition, bit for bit; prior = "regressed" changes the order of an ambiguous pair at most"""
    from oracle import relpose_oracle as O
    from rel_pose_amd import eightpoint
    from tests.test_gpu_memory_contract import _model
    m = _model().eval()
    B = 2
    images = O.synthetic_images(B, 384, 384, key=78).cuda()
    intr = torch.tensor([[0.9 * 384, 0.8 * 384, 192.0, 192.0]]).repeat(B, 2, 1).contiguous().cuda()
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        m.correspondences(images)                                # (warm-up)
        pp = m.planar_pose_from_matches(images, intr, hypotheses=128, seed=5, refine=3)
        before = intr.clone()
        pr = m.planar_pose_from_matches(images, intr, hypotheses=128, seed=5, refine=3, prior="regressed")
        assert torch.equal(intr, before)                         # the regression behind the prior does not write to `intrinsics`
        corr = m.correspondences(images)
    finally:
        torch.backends.cudnn.deterministic = keep
    x1, x2, w = eightpoint.assemble_matches(corr, intr, (384, 384))
    tau = eightpoint.default_tau(intr, (384, 384)).contiguous()
    c = hg.homography_consensus(x1, x2, w, tau=tau, hypotheses=128, seed=5)
    r = hg.homography_refine(x1, x2, w, c.H, tau=tau, iters=3)
    d = hg.pose_from_homography(r.H, x1, x2, w, tau=tau, vis_min=0.99)

    def same(p, q):
        return all((a is None and b is None) or (torch.equal(a, b) if torch.is_tensor(a) else same(a, b)) for a, b in zip(p, q))
    assert same(pp.consensus, c) and torch.equal(pp.H, r.H) and torch.equal(pp.stat, r.stat) and same(pp.candidates, d)
    assert torch.equal(pp.pick, d.pick) and pp.prior is None and pr.prior == "regressed"
    assert pp.pose.shape == (B, 7) and bool(torch.isfinite(pp.pose).all()) and pp.ambiguous.shape == (B,)
    first = d.pick[:, 0].long()
    want = d.pose[torch.arange(B, device="cuda"), first.clamp(min=0)] * (first >= 0).float()[:, None]
    assert torch.equal(pp.pose, want)
    assert same(pr.candidates, d) and torch.equal(pr.ambiguous, pp.ambiguous)
    assert torch.equal(pr.pick.sort(1).values, d.pick.sort(1).values) and torch.equal(pr.pick[~pp.ambiguous], d.pick[~pp.ambiguous])
