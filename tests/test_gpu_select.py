"""rp_model_select (include/relpose_select.h, csrc_select/select.hip) and what is built on it, on a real MI355X.

The reference is tests/_select_ref.py.
    resid     against the fp64 residuals (kinds 1 and 2 by a second route, LAPACK's solve of the 2 x 2 system): C_RESID eps32 scale(row),
              scale the first-order rounding model of _select_ref.row_scale, C_RESID = 8 x the float32 restatement's worst ratio on these
              same inputs (1.805 -> 14.5; asserted by tests/test_select_cpu.py), on the rows the reference calls regular -- at least 90 %
              of them, asserted; where the reference says 1e30 on a regular row, so does the device
    B_c, I_c, label, scale, pick, the rules for invalid candidates and degenerate problems
              EXACTLY what follows from the device's OWN resid and thr (_select_ref.consistent): no tolerance
    G_c       against the fp64 sum of the device's residuals, to K eps32 relative
    pick      equal to the reference's wherever the reference's margin to its runner-up exceeds K eps32 G; no listed case is left out
The device's own ratios go to the test report."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _select_ref as S
from tests.test_gpu_kernels import report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sel():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, select
    _lib.load()
    _lib.load_select()
    return select


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to_numpy(out):
    return S.Selection(*[None if t is None else t.detach().cpu().numpy() for t in out], None, None, None)


def run(sel, x1, x2, w, models, kinds, tau=S.TAU, sigma=None, **kw):
    if isinstance(tau, np.ndarray):
        tau = dev(tau.astype(np.float32))
    if isinstance(sigma, np.ndarray):
        sigma = dev(sigma.astype(np.float32))
    return sel.model_select(dev(x1), dev(x2), dev(w), dev(models), kinds, tau=tau, sigma=sigma, return_residuals=True, return_labels=True, **kw)


IDS = ["%s-n%d-P%d-C%d-%s" % (k, n, P, Cn, "w" if wt else "now") for k, n, P, Cn, wt in S.CASES]


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_select_against_the_reference(sel, case):
    family, n, P, Cn, weighted = case
    x1, x2, w, models, kinds, sigma = S.inputs(*case)
    ref = S.reference(*case)
    dout = run(sel, x1, x2, w, models, kinds, sigma=sigma)
    assert dout.pick.shape == (n,) and dout.stat.shape == (n, Cn, 4) and dout.scale.shape == (n, 2)
    assert dout.residuals.shape == (n, Cn, P) and dout.labels.shape == (n, P)
    assert dout.pick.dtype == torch.int32 and dout.labels.dtype == torch.int32
    out = to_numpy(dout)
    assert all(np.isfinite(a).all() for a in out[:5])
    ratio, share, wrong = S.resid_ratio(out.resid, ref, x1, x2, models, kinds)
    g = S.consistent(out, x1, x2, w, S.TAU, sigma, models, kinds)
    bound = S.pick_bound(ref)
    compared = ref.margin > bound
    print("resid ratio %.3g (C %.3g), compared rows %.4f, G ratio %.3g K eps32, picks compared %d / %d, sigma-hat / reference %.6f .. %.6f"
          % (ratio, S.C_RESID, share, g, compared.sum(), n, (out.scale[:, 0] / ref.scale[:, 0]).min(), (out.scale[:, 0] / ref.scale[:, 0]).max()))
    report("select_" + IDS[S.CASES.index(case)].replace("-", "_"), resid=ratio, compared=share, G=g)
    assert ratio <= S.C_RESID and share >= S.COMPARED_MIN and wrong == 0
    assert bool(compared.all())                                   # the listed inputs leave out none (at most 1 in 20 may be)
    assert np.array_equal(out.pick[compared], ref.pick[compared])
    assert bool((ref.pick >= 0).all()) and np.array_equal(out.scale[:, 1], ref.scale[:, 1])
    # bit-identical from call to call, with and without the optional outputs
    again = sel.model_select(dev(x1), dev(x2), dev(w), dev(models), kinds, tau=torch.full((n,), S.TAU, device="cuda"), sigma=sigma)
    assert again.residuals is None and again.labels is None
    assert all(torch.equal(a, b) for a, b in zip(dout[:3], again[:3]))


def test_degenerate_problems_and_invalid_candidates_in_a_batch(sel):
    """K = 7 (and a negative weight and a NaN); tau 0, negative and NaN; every candidate invalid; no candidate with 16 rows in band --
    each between healthy neighbours, whose bits do not change; and every kind of invalid candidate next to valid ones: a NaN, an
    infinity, the zero matrix, a norm below 1e-30"""
    case = ("mixed", 13, 64, 5, False)
    x1, x2, _, models, kinds, _ = S.inputs(*case)
    n, P = 13, 64
    w = np.random.default_rng(1).uniform(0.05, 1, (n, P)).astype(np.float32)
    tau = np.full(n, S.TAU, np.float32)
    healthy = run(sel, x1, x2, w, models, kinds, tau=tau)
    assert bool((healthy.pick >= 0).all())
    models, w = models.copy(), w.copy()
    tau[1], tau[3], tau[5] = 0, -S.TAU, np.nan
    w[7] = 0
    w[7, 3:10] = 0.5
    w[7, 20], w[7, 21] = -1.0, np.nan
    models[9, :, 0, 0] = np.nan
    tau[11] = 1e-7                                                  # nothing inside the band: no scale
    models[0, 1, 1, 1], models[0, 2] = np.inf, 0                     # invalid candidates among valid ones
    models[2, 0] *= 1e-36
    models[2, 4, 2, 0] = np.nan
    models[4, 3] = 0
    dout = run(sel, x1, x2, w, models, kinds, tau=tau)
    out = to_numpy(dout)
    assert all(np.isfinite(a).all() for a in out[:5])
    S.consistent(out, x1, x2, w, tau, None, models, kinds)
    for b in (1, 3, 5, 7, 9, 11):
        assert out.pick[b] == -1 and out.scale[b].tolist() == [0, -1] and not out.label[b].any()
        assert bool((out.stat[b] == np.float32([S.FLT_MAX, 0, 0, 0])).all())
    assert bool((out.resid[9] == np.float32(1e30)).all()) and bool((out.resid[11] < 1e30).any())     # resid is written all the same
    assert np.array_equal(out.resid[1], healthy.residuals[1].cpu().numpy())
    for b, c in ((0, 1), (0, 2), (2, 0), (2, 4), (4, 3)):
        assert out.stat[b, c].tolist() == [np.float32(S.FLT_MAX), 0, 0, 0] and out.pick[b] not in (-1, c) and out.scale[b, 1] != c
        assert bool((out.resid[b, c] == np.float32(1e30)).all()) and not ((out.label[b] >> c) & 1).any()
    keep = [6, 8, 10, 12]
    assert all(torch.equal(p[keep], q[keep]) for p, q in zip(dout, healthy))


def test_a_given_sigma_is_used_as_it_is(sel):
    """per problem: an entry > 0 is the scale (source -1), any other entry -- 0, negative, NaN -- is estimated; the floor (tau / 1024)^2
    holds for a given sigma, too"""
    case = ("plane", 10, 576, 5, False)
    x1, x2, w, models, kinds, _ = S.inputs(*case)
    est = to_numpy(run(sel, x1, x2, w, models, kinds))
    sigma = np.array([2e-3, 0, -1, np.nan, 1e-3, 1e-9, 5e-4, 0, 3e-3, 1e-3], np.float32)
    out = to_numpy(run(sel, x1, x2, w, models, kinds, sigma=sigma))
    S.consistent(out, x1, x2, w, S.TAU, sigma, models, kinds)
    given = sigma > 0
    assert bool((out.scale[given, 1] == -1).all()) and bool((out.scale[~given, 1] >= 0).all())
    assert np.array_equal(out.scale[~given], est.scale[~given]) and np.array_equal(out.stat[~given], est.stat[~given])
    floor = np.sqrt((np.float32(S.TAU) / np.float32(1024)) ** 2)
    want = np.where(sigma[given] < floor, floor, np.sqrt(sigma[given] * sigma[given]))
    assert np.array_equal(out.scale[given, 0], want.astype(np.float32))
    one = to_numpy(run(sel, x1, x2, w, models, kinds, sigma=1e-3))                    # a number: the same for every problem
    assert bool((one.scale[:, 0] == np.sqrt(np.float32(1e-3) * np.float32(1e-3))).all()) and np.array_equal(one.stat[4], out.stat[4])
    ref = S.select(x1, x2, w, S.TAU, 1e-3, models, kinds)
    assert np.array_equal(one.pick, ref.pick) and bool((ref.margin > S.pick_bound(ref)).all())


def test_refusals(sel):
    """every refusal returns its code before any launch, in the documented order: shape, then size, then alignment"""
    from rel_pose_amd import _lib
    x = torch.rand(2, _lib.SELECT_MAX_P + 1, 2, device="cuda")
    m = torch.eye(3, device="cuda").repeat(2, 9, 1, 1)
    shape, size = r"rp_model_select failed: bad shape \(RP error -1\)", r"rp_model_select failed: unsupported \(RP error -4\)"
    with pytest.raises(RuntimeError, match=size):
        sel.model_select(x, x.clone(), None, m[:, :5].contiguous(), [0] * 5)
    y = x[:, :64].contiguous()
    with pytest.raises(RuntimeError, match=size):
        sel.model_select(y, y.clone(), None, m, [0] * 9)
    with pytest.raises(RuntimeError, match=shape):
        sel.model_select(y[:, :7].contiguous(), y[:, :7].contiguous(), None, m[:, :5].contiguous(), [0] * 5)
    with pytest.raises(RuntimeError, match=shape):
        sel.model_select(y, y.clone(), None, m[:, :0].contiguous(), [])
    for bad in ([0, 1, 3], [0, -1, 2]):
        with pytest.raises(RuntimeError, match=shape):
            sel.model_select(y, y.clone(), None, m[:, :3].contiguous(), bad)
    for cost in (3 * S.LN4, 4.0, 0.0, -8.0, float("nan"), float("inf"), 2e6):
        with pytest.raises(RuntimeError, match=shape):
            sel.model_select(y, y.clone(), None, m[:, :3].contiguous(), [0, 1, 2], outlier_cost=cost)
    with pytest.raises(RuntimeError, match=shape):                                            # shape before size
        sel.model_select(x[:, :7].contiguous(), x[:, :7].contiguous(), None, m, [0] * 9)
    lib, P_ = _lib.load_select(), ctypes.c_void_p
    buf = torch.zeros(8192, device="cuda")
    ptr = lambda k: P_(buf.data_ptr() + 2048 * k)                                            # noqa: E731
    kinds = (ctypes.c_int * 8)(0, 0, 0, 1, 2, 0, 1, 2)
    hk = ctypes.cast(kinds, P_)
    args = [ptr(1), ptr(2), None, ptr(3), None, ptr(4), hk, 8.0, ptr(5), ptr(6), ptr(7), None, None]
    for i, required in ((0, True), (1, True), (3, True), (5, True), (6, True), (8, True), (9, True), (10, True)):
        with pytest.raises(RuntimeError, match=shape):
            lib.rp_model_select(*(args[:i] + [None] + args[i + 1:]), 8, 2, 1, None)
    off = [P_(buf.data_ptr() + 2048 + 4)] + args[1:]
    with pytest.raises(RuntimeError, match=r"misaligned pointer/stride \(RP error -2\)"):
        lib.rp_model_select(*off, 8, 2, 1, None)
    for i in (2, 3, 4, 5, 8, 9, 10, 11, 12):
        with pytest.raises(RuntimeError, match=r"misaligned pointer/stride \(RP error -2\)"):
            lib.rp_model_select(*(args[:i] + [P_(buf.data_ptr() + 2048 * 7 + 256 + 2)] + args[i + 1:]), 8, 2, 1, None)
    with pytest.raises(RuntimeError, match=size):                                             # size before alignment
        lib.rp_model_select(*off, 8, _lib.SELECT_MAX_C + 1, 1, None)
    torch.cuda.synchronize()
    assert not buf.any()                                                                      # nothing was launched


# ------------------------------------------------------------------------------------------------ model level
def test_model_auto_pose_from_matches_is_the_chain_of_the_public_pieces(sel):
    """on the synthetic model input of tests/test_gpu_rotation.py: auto_pose_from_matches equals assemble_matches -> the three chains'
    public pieces -> model_select -> the gathered pose, bit for bit; its three chains equal the model's own chain methods; the model's
    state and `intrinsics` are what they were"""
    from oracle import relpose_oracle as O
    from rel_pose_amd import eightpoint, homography, refine
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
        before = intr.clone()
        ap = m.auto_pose_from_matches(images, intr, hypotheses=(128, 64, 64), seed=5, refine=3)
        aq = m.auto_pose_from_matches(images, intr, hypotheses=64, seed=5, refine=3, subtoken="quadratic", sigma=2e-3)
        assert torch.equal(intr, before)
        cp = m.consensus_pose_from_matches(images, intr, hypotheses=128, seed=5, refine=3)
        pp = m.planar_pose_from_matches(images, intr, hypotheses=64, seed=5, refine=3)
        rp = m.rotation_from_matches(images, intr, hypotheses=64, seed=5, refine=3)
        corr = m.correspondences(images)
    finally:
        torch.backends.cudnn.deterministic = keep
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in state.items()) and not m.training
    assert same(ap.consensus, cp) and same(ap.planar, pp) and same(ap.rotation, rp)
    tau = eightpoint.default_tau(intr, (384, 384)).contiguous()
    x1, x2, w = eightpoint.assemble_matches(corr, intr, (384, 384))
    rows = torch.arange(B, device="cuda")
    E, poses = [cp.E], [cp.pose]
    for k in range(2):
        idx = pp.pick[:, k].long()
        live = (idx >= 0) & (pp.candidates.cstat[rows, idx.clamp(min=0), 2] > 0)
        r = refine.refine_pose((pp.candidates.pose[rows, idx.clamp(min=0)] * live[:, None]).contiguous(), x1, x2, w, tau=tau, iters=3)
        E.append(r.E * live[:, None, None]), poses.append(r.pose * live[:, None])
    models = torch.stack(E + [pp.H, rp.R], 1).contiguous()
    s = sel.model_select(x1, x2, w, models, sel.AUTO_KINDS, tau=tau, return_labels=True)
    assert same(ap.selection, s)
    pick = s.pick.long()
    want = torch.stack(poses + [pp.pose, rp.pose], 1)[rows, pick.clamp(min=0)] * (pick >= 0)[:, None]
    kind = torch.where(pick >= 0, torch.tensor(sel.AUTO_KINDS, device="cuda", dtype=torch.int32)[pick.clamp(min=0)], torch.full_like(s.pick, -1))
    assert torch.equal(ap.pose, want) and torch.equal(ap.kind, kind) and ap.kind.dtype == torch.int32
    assert ap.pose.shape == (B, 7) and bool(torch.isfinite(ap.pose).all())
    assert bool((aq.selection.scale[:, 1] == -1).all()) and bool((aq.selection.scale[:, 0] == 2e-3).all() or (aq.selection.pick < 0).all())
    assert homography.PlanarMatchPose._fields == type(ap.planar)._fields
