"""rp_rotation_consensus, rp_rotation_refine (include/relpose_rotation.h, csrc_rotation/rotation.hip) and what is built on them, on a
real MI355X.

The reference is tests/_rotation_ref.py: every routine of the header in fp64, the two-point rotation by a second route (the
least-squares rotation of the two bearing pairs by LAPACK).  Every bound is C eps32 scale(ref) with C = 8 x the worst ratio of the
float32 restatement of the kernels' arithmetic on these same inputs, measured on the CPU and asserted by tests/test_rotation_cpu.py (the
test_*_restatement_is_within_the_calibrated_bounds tests); nothing was fixed in advance.
    samples   equal the reference's exactly
    hyp_R     max |R^T R - I| <= C_ORTH eps32 on every valid hypothesis (restatement 5.07 -> C_ORTH = 40.6); Frobenius error <=
              C_R eps32 / min(|a_0 x a_1|, |b_0 x b_1|) (restatement 3.03 -> C_R = 24.3) on the hypotheses whose reference cross
              products are >= 1e-2 -- a rule of the reference alone; left out: at most 0.05 %, cap 5 %, asserted
    hyp_cost  against the fp64 cost of the device's OWN hyp_R, _homography_ref.cost_bound's form C eps32 (sqrt(c) + eps32), plus the
              horizon term of _rotation_ref.horizon (a row whose m_z is within rounding of 0); restatement 0.884 -> C_COST = 7.08
    w_out     against the fp64 weights at the device's own R, over eps32 / tau: 0.725 -> C_W = 5.81
    refine    R <= C eps32 kappa, kappa the condition number of the reference's scaled normal matrix: one step 1.27 -> 10.2, converged
              (10 iterations) 24.5 -> 197 -- float32 stops accepting steps short of where fp64 ends; pose against R: 0.690 -> 5.53 eps32
Winners are compared by cost through the bounds, never by index.  The device's own ratios go to the test report."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _consensus_ref as C
from tests import _homography_ref as H
from tests import _rotation_ref as T
from tests.test_gpu_kernels import report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, rotation
    _lib.load()
    _lib.load_rotation()
    return rotation


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to_numpy(out, cls):
    return cls(*[None if t is None else t.detach().cpu().numpy() for t in out])


def np_consensus(out):
    return T.Consensus(*[None if t is None else t.detach().cpu().numpy() for t in out], None)


IDS = ["%s-n%d-P%d-M%d-%s" % (k, n, P, M, "w" if wt else "now") for k, n, P, M, wt in T.CASES]


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_consensus_against_the_reference(rt, case):
    kind, n, P, M, weighted = case
    x1, x2, w = T.inputs(*case)
    ref = T.reference(*case)
    dout = rt.rotation_consensus(dev(x1), dev(x2), dev(w), tau=T.TAU, hypotheses=M, seed=T.SEED, return_weights=True, return_samples=True)
    assert dout.R.shape == (n, 3, 3) and dout.best.shape == (n,) and dout.stat.shape == (n, 4) and dout.weights.shape == (n, P)
    assert dout.hyp_R.shape == (n, M, 3, 3) and dout.hyp_cost.shape == (n, M) and dout.samples.shape == (n, M, 2)
    assert dout.best.dtype == torch.int32 and dout.samples.dtype == torch.int32
    out = np_consensus(dout)
    assert all(np.isfinite(a).all() for a in out if a is not None)
    assert np.array_equal(out.samples, ref.samples)
    valid = out.hyp_cost < T.FLT_MAX
    assert not out.hyp_R[~valid].any() and np.abs(np.linalg.det(out.hyp_R[valid].astype(np.float64)) - 1).max(initial=0) <= 3 * T.C_ORTH * T.EPS32
    r = T.check_consensus(out, ref, x1, x2, w)
    report("rotation_consensus_" + IDS[T.CASES.index(case)].replace("-", "_"), **r)
    # bit-identical from call to call, with and without the optional outputs
    again = rt.rotation_consensus(dev(x1), dev(x2), dev(w), tau=torch.full((n,), T.TAU, device="cuda"), hypotheses=M, seed=T.SEED)
    assert again.weights is None and again.samples is None
    assert all(torch.equal(a, b) for a, b in zip(dout[:3] + dout[4:6], again[:3] + again[4:6]))


RIDS = ["%s-n%d-P%d-%s" % (k, n, P, "w" if wt else "now") for k, n, P, wt in T.REFINE_CASES]


@pytest.mark.parametrize("case", T.REFINE_CASES, ids=RIDS)
def test_refinement_against_the_reference(rt, case):
    """one step and converged against the fp64 reference at C eps32 kappa; pose consistent with R; iters = 0 is the scorer and returns the
    normalised R0; R may alias R0; the cost never rises"""
    kind, n, P, weighted = case
    x1, x2, w, R0 = T.refine_inputs(*case)
    a, b, ww, r0 = dev(x1), dev(x2), dev(w), dev(R0)
    figures = {}
    for iters in (1, 10):
        ref = T.refine_reference(*case, iters)
        d = rt.rotation_refine(a, b, ww, r0, tau=T.TAU, iters=iters, return_weights=True)
        o = to_numpy(d, rt.RefinedRotation)
        assert all(np.isfinite(t).all() for t in o)
        r = T.refine_ratios(o.R, o.pose, o.stat, o.weights, ref, x1, x2, w)
        print("iters %d: R ratio %.3g (C %.3g), pose %.3g (C %.3g), cost %.3g, w %.3g; kappa %.1f .. %.1f; accepted %s (reference %s)"
              % (iters, r["R"], T.C_REFINE_R[iters], r["pose"], T.C_POSE, r["cost"], r["w"], ref.kappa.min(), ref.kappa.max(), o.stat[:, 2], ref.stat[:, 2]))
        figures.update({"%s_%d" % (k, iters): v for k, v in r.items()})
        assert r["R"] <= T.C_REFINE_R[iters] and r["pose"] <= T.C_POSE and r["cost"] <= T.C_COST and r["w"] <= T.C_W, r
        assert not o.pose[:, :3].any() and bool((o.pose[:, 6] >= 0).all())
        assert np.array_equal(o.stat[:, 3], (C.clamp(w, n, P) > 0).sum(-1))
    report("rotation_refine_" + RIDS[T.REFINE_CASES.index(case)].replace("-", "_"), **figures)
    score = rt.rotation_refine(a, b, ww, r0, tau=T.TAU, iters=0)
    assert bool((d.stat[:, 0] <= score.stat[:, 0]).all()) and not score.stat[:, 2].any() and score.weights is None
    # iters = 0: the normalised R0 (it came as a rotation, to float32 rounding of the fp64 winner) and its cost, the fp64 cost of ITS R
    assert float((score.R - r0).abs().max()) <= T.C_START * T.EPS32
    sR, wc = score.R.cpu().numpy(), C.clamp(w, n, P)
    own = T.cost64(sR, x1, x2, wc, T.TAU)
    assert bool((np.abs(score.stat[:, 0].cpu().numpy() - own) <= T.cost_bound(own, T.C_COST, T.horizon(sR, x1, x2, wc, T.TAU))).all())
    # a scaled start is the same start
    scaled = rt.rotation_refine(a, b, ww, (2.5 * r0).contiguous(), tau=T.TAU, iters=0)
    assert float((scaled.R - score.R).abs().max()) <= T.C_START_SCALED * T.EPS32
    # aliasing and call-to-call identity
    alias, taus = r0.clone(), torch.full((n,), T.TAU, device="cuda")
    pose, stat = torch.empty_like(d.pose), torch.empty_like(d.stat)
    P_ = ctypes.c_void_p
    d2 = rt._lib.load_rotation().rp_rotation_refine(P_(a.data_ptr()), P_(b.data_ptr()), None if ww is None else P_(ww.data_ptr()),
                                                   P_(taus.data_ptr()), P_(alias.data_ptr()), 10, P_(alias.data_ptr()), P_(pose.data_ptr()),
                                                   P_(stat.data_ptr()), None, P, n, P_(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert d2 == 0 and torch.equal(alias, d.R) and torch.equal(pose, d.pose) and torch.equal(stat, d.stat)


def test_the_two_libraries_sit_on_one_scale(rt):
    """rotation_refine(iters = 0)'s cost equals homography_refine(iters = 0)'s at H = R, within the two cost bounds, on scenes where every
    m_z > 0 (asserted): the distance is the transfer distance there"""
    from rel_pose_amd import homography
    sc = [T.rotation_scene(60 + s, 576, 0.3) for s in range(4)]
    x1, x2 = np.concatenate([s.x1 for s in sc]), np.concatenate([s.x2 for s in sc])
    Rt = np.stack([s.R for s in sc]).astype(np.float32)
    mz = np.einsum("bj,bpj->bp", Rt[:, 2].astype(np.float64), np.concatenate([x1, np.ones((4, 576, 1), np.float32)], -1).astype(np.float64))
    assert mz.min() > 0.1
    a, b, r0 = dev(x1), dev(x2), dev(Rt)
    ro = rt.rotation_refine(a, b, None, r0, tau=T.TAU, iters=0, return_weights=True)
    ho = homography.homography_refine(a, b, None, r0, tau=T.TAU, iters=0, return_weights=True)
    cr, ch = ro.stat[:, 0].cpu().numpy().astype(np.float64), ho.stat[:, 0].cpu().numpy().astype(np.float64)
    wc = np.ones((4, 576))
    own = T.cost64(ro.R.cpu().numpy(), x1, x2, wc, T.TAU)
    print("rotation %s homography %s fp64 %s" % (cr, ch, own))
    assert bool((np.abs(cr - ch) <= T.cost_bound(own, T.C_COST) + H.cost_bound(own, H.C_COST)).all())
    u = np.stack([T.distance(ro.R[b].cpu().numpy().astype(np.float64), x1[b].astype(np.float64), x2[b].astype(np.float64)) for b in range(4)]) / T.TAU ** 2
    band = (np.abs(u - 1) < 1e-4).mean(-1)                            # rows within rounding of the threshold may fall on either side
    assert bool((np.abs((ro.stat[:, 1] - ho.stat[:, 1]).cpu().numpy()) <= band + 1e-6).all()) and torch.equal(ro.stat[:, 3], ho.stat[:, 3])
    assert float((ro.weights - ho.weights).abs().max()) <= (T.C_W + H.C_W) * T.EPS32 / T.TAU


def test_degenerate_problems_in_a_batch(rt):
    """tau 0, negative and NaN; one positive weight (plus a negative one and a NaN); two identical rows, where every hypothesis is invalid
    and best = -1; R0 zero and R0 with a NaN -- each between healthy neighbours, whose bits do not change"""
    n, P = 13, 40
    x1, x2, Rt = T.exact_scenes(n, P, 12)
    w = np.random.default_rng(1).uniform(0.05, 1, (n, P)).astype(np.float32)
    tau = np.full(n, 0.02, np.float32)
    a, b = dev(x1), dev(x2)
    kw = dict(hypotheses=70, seed=3, return_weights=True, return_samples=True)
    healthy = rt.rotation_consensus(a, b, dev(w), tau=dev(tau), **kw)
    hr = rt.rotation_refine(a, b, dev(w), healthy.R, tau=dev(tau), iters=3, return_weights=True)
    assert bool((healthy.best >= 0).all())
    tau[1], tau[3], tau[5] = 0, -0.02, np.nan
    w[7] = 0
    w[7, 9] = 0.5
    w[7, 4], w[7, 8] = -1.0, np.nan
    w[9] = 0
    w[9, [2, 6]] = 0.7
    x1, x2 = x1.copy(), x2.copy()
    x1[9, 6], x2[9, 6] = x1[9, 2], x2[9, 2]                               # K = 2 and the two rows are one: no hypothesis spans a plane
    a, b = dev(x1), dev(x2)
    out = rt.rotation_consensus(a, b, dev(w), tau=dev(tau), **kw)
    o = np_consensus(out)
    wc = C.clamp(w, n, P, np.float32)
    for i, K in ((1, 40), (3, 40), (5, 40), (7, 1), (9, 2)):
        assert not o.R[i].any() and o.best[i] == -1 and np.array_equal(o.stat[i], [0, 0, 0, K]), (i, o.stat[i])
        assert np.array_equal(o.weights[i], wc[i]) and not o.hyp_R[i].any() and bool((o.hyp_cost[i] == np.float32(T.FLT_MAX)).all())
    assert not o.samples[7].any() and o.samples[9].any() and np.array_equal(o.samples, T.sample_rows2(w, n, P, 3, 70)[1])
    assert all(np.isfinite(t).all() for t in o if t is not None)
    keep = [0, 2, 4, 6, 8, 10, 11, 12]
    assert all(torch.equal(p[keep], q[keep]) for p, q in zip(out, healthy))
    # the refinement leaves a degenerate problem alone: R0 copied bit for bit, pose = 0, stat = (0, 0, 0, K), the clamped weights
    bad = healthy.R.clone()
    bad[11] = 0                                                       # the zero matrix the consensus writes for a degenerate problem
    bad[1, 1, 2] = float("nan")                                       # (tau = 0 there, too)
    bad[10, 0, 1] = float("inf")
    r = rt.rotation_refine(a, b, dev(w), bad, tau=dev(tau), iters=3, return_weights=True)
    for i, K in ((1, 40), (3, 40), (5, 40), (7, 1), (10, 40), (11, 40)):
        assert torch.equal(r.R[i].view(torch.int32), bad[i].view(torch.int32)) and not r.pose[i].any(), i
        assert r.stat[i].cpu().tolist() == [0, 0, 0, K] and np.array_equal(r.weights[i].cpu().numpy(), wc[i])
    keep = [0, 2, 4, 6, 8, 12]
    assert all(torch.equal(p[keep], q[keep]) for p, q in zip(r, hr))
    assert all(bool(torch.isfinite(t[[i for i in range(n) if i not in (1, 10)]]).all()) for t in r)
    # problem 9: two identical rows with K = 2 -- the polish runs (K >= 2, a finite start), and writes nothing non-finite
    assert bool(torch.isfinite(r.R[9]).all()) and r.stat[9, 3] == 2


def test_refusals(rt):
    """every refusal returns its code before any launch, one call each, in the documented order: shape, then size, then alignment"""
    from rel_pose_amd import _lib
    x = torch.rand(2, _lib.ROTATION_MAX_P + 1, 2, device="cuda")
    Rm = torch.eye(3, device="cuda").repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match=r"rel_pose_amd: rp_rotation_consensus failed: unsupported \(RP error -4\)"):
        rt.rotation_consensus(x, x.clone())
    y = x[:, :64].contiguous()
    with pytest.raises(RuntimeError, match=r"unsupported \(RP error -4\)"):
        rt.rotation_consensus(y, y.clone(), hypotheses=_lib.ROTATION_MAX_M + 1)
    with pytest.raises(RuntimeError, match=r"bad shape \(RP error -1\)"):
        rt.rotation_consensus(y[:, :1].contiguous(), y[:, :1].contiguous())
    with pytest.raises(RuntimeError, match=r"bad shape \(RP error -1\)"):
        rt.rotation_consensus(y, y.clone(), hypotheses=0)
    with pytest.raises(RuntimeError, match=r"bad shape \(RP error -1\)"):                    # shape before size
        rt.rotation_consensus(x[:, :1].contiguous(), x[:, :1].contiguous(), hypotheses=_lib.ROTATION_MAX_M + 1)
    with pytest.raises(RuntimeError, match=r"rp_rotation_refine failed: unsupported \(RP error -4\)"):
        rt.rotation_refine(y, y.clone(), None, Rm, iters=_lib.ROTATION_MAX_ITERS + 1)
    with pytest.raises(RuntimeError, match=r"rp_rotation_refine failed: unsupported \(RP error -4\)"):
        rt.rotation_refine(x, x.clone(), None, Rm)
    with pytest.raises(RuntimeError, match=r"rp_rotation_refine failed: bad shape \(RP error -1\)"):
        rt.rotation_refine(y, y.clone(), None, Rm, iters=-1)
    # size before alignment, and alignment itself: x1 four bytes off an 8-byte boundary
    lib, P_ = _lib.load_rotation(), ctypes.c_void_p
    buf = torch.zeros(4096, device="cuda")
    ptr = lambda k: P_(buf.data_ptr() + 256 * k)                                            # noqa: E731
    args = [ptr(1), ptr(2), None, ptr(3), 1, ptr(4), ptr(5), ptr(6), None, ptr(7), ptr(8), None]
    off = [P_(buf.data_ptr() + 4)] + args[1:]
    with pytest.raises(RuntimeError, match=r"misaligned pointer/stride \(RP error -2\)"):
        lib.rp_rotation_consensus(*off, 4, 2, 1, None)
    with pytest.raises(RuntimeError, match=r"unsupported \(RP error -4\)"):
        lib.rp_rotation_consensus(*off, 4, _lib.ROTATION_MAX_M + 1, 1, None)
    torch.cuda.synchronize()
    assert not buf.any()                                                                    # nothing was launched


# ------------------------------------------------------------------------------------------------ model level
def test_model_rotation_from_matches_is_the_chain_of_the_public_pieces(rt):
    """on the synthetic model input of tests/test_gpu_homography.py: rotation_from_matches (both subtoken forms) equals
    assemble_matches -> consensus -> refine on the base weights, bit for bit; the model's state, its correspondences and
    planar_pose_from_matches are what they were"""
    from oracle import relpose_oracle as O
    from rel_pose_amd import eightpoint
    from tests.test_gpu_memory_contract import _model
    m = _model().eval()
    B = 2
    images = O.synthetic_images(B, 384, 384, key=78).cuda()
    intr = torch.tensor([[0.9 * 384, 0.8 * 384, 192.0, 192.0]]).repeat(B, 2, 1).contiguous().cuda()
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True

    def same(p, q):
        return all((a is None and b is None) or (torch.equal(a, b) if torch.is_tensor(a) else a == b if isinstance(a, (str, type(None))) else same(a, b))
                   for a, b in zip(p, q))
    try:
        m.correspondences(images)                                # (warm-up)
        state = {k: v.clone() for k, v in m.state_dict().items()}
        corr0 = m.correspondences(images)
        pp0 = m.planar_pose_from_matches(images, intr, hypotheses=64, seed=5, refine=3)
        before = intr.clone()
        rp = m.rotation_from_matches(images, intr, hypotheses=128, seed=5, refine=3)
        rq = m.rotation_from_matches(images, intr, hypotheses=128, seed=5, refine=3, subtoken="quadratic")
        rw = m.rotation_from_matches(images, intr, hypotheses=128, seed=5, refine=3, subtoken="window")
        assert torch.equal(intr, before)
        corr = m.correspondences(images)
        sub = m.subtoken_correspondences(images)
        pp1 = m.planar_pose_from_matches(images, intr, hypotheses=64, seed=5, refine=3)
    finally:
        torch.backends.cudnn.deterministic = keep
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in state.items()) and not m.training
    assert same(corr0, corr) and same(pp0, pp1)
    tau = eightpoint.default_tau(intr, (384, 384)).contiguous()
    for got, kw in ((rp, {}), (rq, dict(sub=sub, subtoken="quadratic")), (rw, dict(sub=sub, subtoken="window"))):
        x1, x2, w = eightpoint.assemble_matches(sub.corr if kw else corr, intr, (384, 384), **kw)
        c = rt.rotation_consensus(x1, x2, w, tau=tau, hypotheses=128, seed=5)
        r = rt.rotation_refine(x1, x2, w, c.R, tau=tau, iters=3)
        assert same(got.consensus, c) and torch.equal(got.R, r.R) and torch.equal(got.stat, r.stat) and torch.equal(got.pose, r.pose)
        assert got.pose.shape == (B, 7) and bool(torch.isfinite(got.pose).all()) and not got.pose[:, :3].any()
    assert not torch.equal(rp.R, rq.R)                           # the sub-token positions are other matches
