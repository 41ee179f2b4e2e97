"""rp_five_point_consensus (include/relpose_fivepoint.h, csrc_fivepoint/five_point.hip) and what is built on it, on a real MI355X.

The reference is tests/_fivepoint_ref.py: five_point_ref, the header's solve in fp64 with LAPACK by another route than the kernel's (SVD
null space, fitted cubics, the eigenvectors of the action matrix), and consensus5_ref on top of it.  Errors of E are taken up to sign.

ROOTS.  n = 3, P = 64, M = 256, tau = 0.01, seed 1, on the exact scenes scenes(3, 64, 5) and on the first 64 rows of the 50 % noisy scenes
of seeds 0 .. 2.  The sampler is compared exactly.  A sample is ADMITTED by the reference alone: the condition number of its eliminated
10 x 10 block <= 1e4, its roots pairwise >= 1e-2 apart (up to sign), no complex eigenvalue of the action matrix within 1e-3 (relative)
of the real axis.  Left out by that: 5.73 % of the exact samples (5.08 % condition, 0.39 % separation, 0.26 % near-complex) and 0.65 %
of the noisy ones (0.52 %, 0, 0.13 %); the cap is 10 %, asserted and printed.
Bounds, each 8 x the largest error of the restatement of the kernel's arithmetic at the kernel's precisions (five_point_kernel: fp64 up to
the rounding at norm 1, float32 from there, LAPACK's float32 SVD for svd3x3_dev) against five_point_ref on these same inputs, measured
on the CPU and asserted by tests/test_fivepoint_cpu.py (test_restatement_is_within_the_calibrated_bounds):
    roots     every reference root of an admitted sample has a device root within C_ROOT: the restatement's largest distance is 1.895e-6
              on the exact scenes -> 1.52e-5, and 2.233e-7 on the noisy ones -> 1.79e-6 (there the float32 finish is all there is: the
              admitted samples' roots are accurate to 1e-9 before it)
    residual  every valid device slot, of EVERY sample, admitted or not: |x2h^T E x1h| on the sample's five rows <= C_RES; the
              restatement's largest is 3.102e-7 (exact) -> 2.49e-6 and 9.068e-8 (noisy) -> 7.26e-7.  A root of an ill-conditioned sample
              is still a combination of the null-space basis, so before the projection its residual is at fp64 rounding level
    essential every valid device slot has singular values within 1e-5 of (1, 1, 0), the figure tests/test_gpu_consensus.py holds the
              same projection to (the restatement: 1.2e-7)
The kernel source run on the host (tools/lab/fivepoint_host/run.py, the real svd3x3_dev, no contraction) gives 1.64e-6 / 6.6e-7 for the
roots and 3.8e-7 / 2.2e-7 for the residuals.
SCORE.  hyp_cost against the fp64 cost of the kernel's OWN hyp_E and w_out against the fp64 weights at the kernel's own E, with the forms
and constants of tests/_consensus_ref.py (cost_bound, C_COST = 3.01, C_W = 2.81): the scoring loop and the selection kernel repeat
csrc_consensus/consensus.hip expression for expression, on rows of the same magnitude, so the restatement those constants were
calibrated on (consensus_f32) is the restatement of this score too.  best is the lowest (m, k) of the kernel's own minimum, exactly;
against consensus5_ref only the COST of the winner is compared (check_winner states the bound).
SIXTY PERCENT.  Ten problems, P = 576, M = 1024, seed 1, 60 % of x2 uniform noise, against the TRUTH: best <= 0.1 and, after
eight_point(w = weights, iters = 4), <= 0.05 on 10 of 10.  Every scene is a call of its own, so its problem index is 0: that is how the
row of the table in DESIGN.md 5.6 was made (tests/test_fivepoint_cpu.py reproduces its cells, 0.034 / 0.022, from consensus5_ref).
Recorded next to it, not asserted: the ten scenes as ONE batch draw other samples (problem index = position) and reach 9 of 10 -- on
scene 9 a sample that holds two outliers has an exact root 0.561 from the truth whose robust cost 3.4492e-4 is BELOW the truth's
3.4553e-4; the selection rule picks it in the fp64 reference as on the device.
The GPU's own figures go to the test report (tests/test_gpu_kernels.py: report)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import _consensus_ref as C
from tests import _eightpoint_ref as R
from tests import _fivepoint_ref as F
from tests.test_gpu_kernels import report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fp():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, fivepoint
    _lib.load()
    _lib.load_fivepoint()
    return fivepoint


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


def to_numpy(out):
    return F.Consensus5(*[None if t is None else t.detach().cpu().numpy() for t in out])


@functools.lru_cache(maxsize=None)
def gpu_roots(kind):
    from rel_pose_amd import fivepoint
    x1, x2 = F.root_inputs(kind)
    return fivepoint.five_point_consensus(dev(x1), dev(x2), None, tau=F.TAU, hypotheses=F.ROOT_SHAPE[2], seed=F.SEED, return_weights=True,
                                          return_samples=True)


@pytest.mark.parametrize("kind", F.ROOT_CASES)
def test_roots_against_the_reference(fp, kind):
    n, P, M = F.ROOT_SHAPE
    x1, x2 = F.root_inputs(kind)
    dout = gpu_roots(kind)
    assert dout.E.shape == (n, 3, 3) and dout.best.shape == (n, 2) and dout.stat.shape == (n, 4) and dout.weights.shape == (n, P)
    assert dout.hyp_E.shape == (n, M, 10, 3, 3) and dout.hyp_cost.shape == (n, M, 10) and dout.samples.shape == (n, M, 5)
    assert dout.best.dtype == torch.int32 and dout.samples.dtype == torch.int32
    out = to_numpy(dout)
    assert all(np.isfinite(a).all() for a in out)
    figures = F.check_roots(kind, out, "MI355X ")
    report("fivepoint_roots_" + kind, **figures)
    ratios = F.check_consensus(out, x1, x2, None, F.TAU)
    print("cost ratio %.3g (C %.3g), w ratio %.3g (C %.3g)" % (ratios["cost"], C.C_COST, ratios["w"], C.C_W))
    report("fivepoint_score_" + kind, **ratios)
    F.check_winner(kind, out)
    # bit-identical from call to call, with and without the optional outputs, with w = None and with ones
    again = fp.five_point_consensus(dev(x1), dev(x2), None, tau=F.TAU, hypotheses=M, seed=F.SEED, return_weights=True, return_samples=True)
    assert all(torch.equal(a, b) for a, b in zip(dout, again))
    ones = fp.five_point_consensus(dev(x1), dev(x2), torch.ones(n, P, device="cuda"), tau=torch.full((n,), F.TAU, device="cuda"),
                                   hypotheses=M, seed=F.SEED)
    assert ones.weights is None and ones.samples is None and all(torch.equal(a, b) for a, b in zip(dout[:3], ones[:3]))
    assert torch.equal(ones.hyp_E, dout.hyp_E) and torch.equal(ones.hyp_cost, dout.hyp_cost)


@pytest.mark.parametrize("n,P,M", [(1, 5, 1), (2, 9, 257), (130, 64, 16), (1, 1728, 40)])
def test_score_and_selection_with_weights(fp, n, P, M):
    """the smallest problem, sizes off the workgroup, more than one chunk of samples, many problems, the largest P; random base weights,
    every third 0 where P >= 24"""
    x1, x2, _ = R.scenes(n, P, seed=11)
    x1, x2 = x1.astype(np.float32), x2.astype(np.float32)
    w = np.random.default_rng(P + n).uniform(0.05, 1.0, (n, P)).astype(np.float32)
    if P >= 24:
        w[:, ::3] = 0
    out = to_numpy(fp.five_point_consensus(dev(x1), dev(x2), dev(w), tau=F.TAU, hypotheses=M, seed=F.SEED, return_weights=True,
                                           return_samples=True))
    assert all(np.isfinite(a).all() for a in out)
    assert np.array_equal(out.samples, F.sample_rows5(w, n, P, F.SEED, M)[1])
    ratios = F.check_consensus(out, x1, x2, w, F.TAU)
    report("fivepoint_score_n%d_P%d_M%d" % (n, P, M), **ratios)
    # exact scenes: the truth is among the roots of every sample, so the winner is the truth up to the float32 finish
    _, _, Et = R.scenes(n, P, seed=11)
    assert float(R.up_to_sign(out.E, Et).max()) <= 1e-3


def test_sixty_percent_of_outliers(fp):
    """ten scenes, 576 matches, 60 % of x2 uniform noise, M = 1024, seed 1, each a problem of index 0 as in the table of DESIGN.md 5.6:
    best within 0.1 of the TRUTH on 10 of 10, and after eight_point(w = weights, iters = 4) within 0.05 on 10 of 10 (the reference:
    0.034 / 0.022).  The same scenes as one batch are recorded (module docstring)."""
    from rel_pose_amd import eightpoint
    x1, x2, Et, _ = C.noisy_batch(0.6)
    a, b = dev(x1), dev(x2)
    tau = torch.full((10,), F.TAU, device="cuda")
    outs = [fp.five_point_consensus(a[i:i + 1], b[i:i + 1], None, tau=F.TAU, hypotheses=1024, seed=1, return_weights=True) for i in range(10)]
    E, weights = torch.cat([o.E for o in outs]), torch.cat([o.weights for o in outs])
    best = R.up_to_sign(host(E), Et)
    chain = R.up_to_sign(host(eightpoint.eight_point(a, b, weights, tau=tau, iters=4).E), Et)
    batch = fp.five_point_consensus(a, b, None, tau=F.TAU, hypotheses=1024, seed=1, return_weights=True)
    assert torch.equal(batch.E[0], outs[0].E[0]) and torch.equal(batch.hyp_cost[0], outs[0].hyp_cost[0])      # index 0 is index 0
    best_b = R.up_to_sign(host(batch.E), Et)
    chain_b = R.up_to_sign(host(eightpoint.eight_point(a, b, batch.weights, tau=tau, iters=4).E), Et)
    report("fivepoint_noisy60", best_max=float(best.max()), chain_max=float(chain.max()), best_ok=int((best <= 0.1).sum()),
           chain_ok=int((chain <= 0.05).sum()), batch_best_ok=int((best_b <= 0.1).sum()), batch_chain_ok=int((chain_b <= 0.05).sum()))
    print("best", np.round(best, 3), "polished", np.round(chain, 3))
    print("as one batch (recorded): best", np.round(best_b, 3), "polished", np.round(chain_b, 3))
    assert int((best <= 0.1).sum()) == 10, best
    assert int((chain <= 0.05).sum()) == 10, chain


def test_degenerate_problems_in_a_batch(fp):
    """four positive weights (plus a negative one and a NaN), tau = 0 and a problem whose weights are mostly NaN or negative between
    healthy problems: the documented outputs, and the healthy neighbours bit-identical to the same batch with healthy problems in those
    slots"""
    x1, x2, _ = R.scenes(6, 40, seed=12)
    x1, x2 = x1.astype(np.float32), x2.astype(np.float32)
    w = np.random.default_rng(1).uniform(0.05, 1, (6, 40)).astype(np.float32)
    tau = np.full(6, 0.02, np.float32)
    M = 70
    kw = dict(hypotheses=M, seed=3, return_weights=True, return_samples=True)
    healthy = fp.five_point_consensus(dev(x1), dev(x2), dev(w), tau=dev(tau), **kw)
    assert bool((healthy.best >= 0).all()) and bool((healthy.stat[:, 2] >= M).all())
    w[1] = 0
    w[1, [3, 5, 9, 20]] = 0.5
    w[1, 7], w[1, 8] = -1.0, np.nan
    w[3, ::2], w[3, 1::4] = np.nan, -1.0                           # ten rows of positive weight are left: a healthy problem
    tau[5] = 0
    out = fp.five_point_consensus(dev(x1), dev(x2), dev(w), tau=dev(tau), **kw)
    o = to_numpy(out)
    for b, K in ((1, 4), (5, 40)):
        assert not o.E[b].any() and np.array_equal(o.best[b], [-1, -1]) and np.array_equal(o.stat[b], [0, 0, 0, K]), (b, o.best[b], o.stat[b])
        assert np.array_equal(o.weights[b], C.clamp(w, 6, 40, np.float32)[b])
        assert not o.hyp_E[b].any() and bool((o.hyp_cost[b] == np.float32(C.FLT_MAX)).all())
    assert not o.samples[1].any() and o.samples[5].any()
    assert np.array_equal(o.samples, F.sample_rows5(w, 6, 40, 3, M)[1])
    assert all(np.isfinite(a).all() for a in o)
    assert o.stat[3, 3] == 10 and o.best[3, 0] >= 0 and set(o.samples[3].ravel()) <= set(np.flatnonzero(C.clamp(w, 6, 40)[3] > 0))
    assert np.array_equal(o.weights[3] > 0, C.clamp(w, 6, 40)[3] > 0)
    keep = [0, 2, 4]
    assert all(torch.equal(p[keep], q[keep]) for p, q in zip(out, healthy))
    assert float(out.E[keep].abs().max()) > 0.3


def test_outputs_do_not_depend_on_what_they_held(fp):
    """the raw entry point on outputs filled with NaN and on outputs filled with a finite pattern: the same bits"""
    from rel_pose_amd import _lib
    lib = _lib.load_fivepoint()
    n, P, M = 3, 64, 257
    x1, x2 = F.root_inputs("exact")
    x1, x2 = dev(x1), dev(x2)
    tau = torch.full((n,), F.TAU, device="cuda")
    Pv = ctypes.c_void_p
    runs = []
    for fill in (float("nan"), 12345.0):
        f = [torch.full(s, fill, device="cuda") for s in ((n, 9), (n, 4), (n, P), (n, M, 90), (n, M, 10))]
        i = [torch.full(s, 0x7FC0DEAD if fill != fill else 0x12345678, dtype=torch.int32, device="cuda") for s in ((n, 2), (n, M, 5))]
        lib.rp_five_point_consensus(Pv(x1.data_ptr()), Pv(x2.data_ptr()), None, Pv(tau.data_ptr()), F.SEED, Pv(f[0].data_ptr()),
                                    Pv(i[0].data_ptr()), Pv(f[1].data_ptr()), Pv(f[2].data_ptr()), Pv(f[3].data_ptr()), Pv(f[4].data_ptr()),
                                    Pv(i[1].data_ptr()), P, M, n, Pv(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        runs.append([t.view(torch.int32) for t in f] + i)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert all(bool(torch.isfinite(t.view(torch.float32)).all()) for t in runs[0][:5])
    # the first 256 samples are those of the M = 256 run: a sample depends on (seed, problem, m) alone
    assert torch.equal(runs[0][6][:, :256], gpu_roots("exact").samples)
    assert torch.equal(runs[0][3].view(n, M, 90)[:, :256].reshape(-1), gpu_roots("exact").hyp_E.view(torch.int32).reshape(-1))


def test_refusals_leave_outputs_untouched(fp):
    from rel_pose_amd import _lib
    x = torch.rand(2, _lib.FIVEPOINT_MAX_P + 1, 2, device="cuda")
    with pytest.raises(RuntimeError, match=r"rel_pose_amd: rp_five_point_consensus failed: unsupported \(RP error -4\)"):
        fp.five_point_consensus(x, x.clone())
    y = x[:, :64].contiguous()
    with pytest.raises(RuntimeError, match=r"unsupported \(RP error -4\)"):
        fp.five_point_consensus(y, y.clone(), hypotheses=_lib.FIVEPOINT_MAX_M + 1)
    with pytest.raises(RuntimeError, match=r"bad shape \(RP error -1\)"):
        fp.five_point_consensus(y, y.clone(), hypotheses=0)
    with pytest.raises(RuntimeError, match=r"bad shape \(RP error -1\)"):
        fp.five_point_consensus(y[:, :4].contiguous(), y[:, :4].contiguous())


# ------------------------------------------------------------------------------------------------ model level
def test_model_consensus_pose_from_matches_minimal(fp):
    """on the synthetic model input of tests/test_gpu_consensus.py: minimal = "five" is the chain of the public pieces with
    five_point_consensus in front, bit for bit; minimal = "eight" returns bit for bit what the call without the argument returns"""
    from oracle import relpose_oracle as O
    from rel_pose_amd import consensus, eightpoint, geom, refine
    from tests.test_gpu_memory_contract import _model
    m = _model().eval()
    B = 2
    images = O.synthetic_images(B, 384, 384, key=78).cuda()
    intr = torch.tensor([[0.9 * 384, 0.8 * 384, 192.0, 192.0]]).repeat(B, 2, 1).contiguous().cuda()
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        m.correspondences(images)                                # (warm-up)
        plain = m.consensus_pose_from_matches(images, intr, hypotheses=128, seed=5, refine=3)
        eight = m.consensus_pose_from_matches(images, intr, hypotheses=128, seed=5, refine=3, minimal="eight")
        five = m.consensus_pose_from_matches(images, intr, hypotheses=128, seed=5, refine=3, minimal="five")
        corr = m.correspondences(images)
    finally:
        torch.backends.cudnn.deterministic = keep

    def same(p, q):
        return all((a is None and b is None) or (torch.equal(a, b) if torch.is_tensor(a) else same(a, b)) for a, b in zip(p, q))
    assert isinstance(plain.consensus, consensus.Consensus) and same(plain, eight)
    assert isinstance(five.consensus, fp.FivePointConsensus)
    x1, x2, w = eightpoint.assemble_matches(corr, intr, (384, 384))
    tau = eightpoint.default_tau(intr, (384, 384)).contiguous()
    c = fp.five_point_consensus(x1, x2, w, tau=tau, hypotheses=128, seed=5, return_weights=True)
    ep = eightpoint.eight_point(x1, x2, c.weights, tau=tau, iters=4, return_weights=True)
    pose, count = geom.pose_from_essential(ep.E, x1, x2)
    r = refine.refine_pose(pose, x1, x2, w, tau=tau, iters=3, return_weights=True)
    assert same(five[:4], r) and same(five.consensus, c) and same(five.initial, (pose, ep.E, ep.stat, count, ep.weights))
    assert five.pose.shape == (B, 7) and five.consensus.hyp_cost.shape == (B, 128, 10) and bool(torch.isfinite(five.pose).all())
    with pytest.raises(ValueError, match="minimal"):
        m.consensus_pose_from_matches(images, intr, minimal="seven")
