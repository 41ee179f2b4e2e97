"""rp_eight_point_consensus (include/relpose_consensus.h, csrc_consensus/consensus.hip) and what is built on it, on a real MI355X.

The reference is tests/_consensus_ref.py: consensus_ref, the header in fp64 -- every hypothesis is eight_point_ref on its eight rows.
Errors of E are taken up to sign, as in tests/test_gpu_eightpoint.py.

Cases: exact synthetic scenes at (n, P, M) = (1, 8, 1), (3, 9, 257), (2, 257, 256), (130, 64, 64), (2, 1728, 300), and the ten noisy
scenes with 50 % outliers as one batch (10, 576, 1024); each without weights and with (random base weights, a share of them 0).
tau = 0.01, seed 1.

Bounds, each C = 8 x the largest ratio that the numpy float32 restatement of the kernel's arithmetic (consensus_f32) shows on these
same inputs (measured on the CPU, tests/test_consensus_cpu.py asserts them; the constants, the cases and the ratios live in
tests/_consensus_ref.py, which both suites and the host harness import):
    hyp_E     a hypothesis is the null vector of its 8 x 9 row matrix A: a relative perturbation eps of A moves it by about
              eps sigma_1 / sigma_8, so |hyp_E - ref| <= C_E eps32 sigma_1 / sigma_8(ref).  Only hypotheses with eps32 sigma_1 / sigma_8
              <= 1e-2 are compared (beyond, the bound says nothing); that must be at least 95 % of a case (it is 99.6 .. 100 %).
              Largest ratio of the restatement on the exact scenes 2.32 (P = 1728, weighted; 0.02 .. 2.25 elsewhere) -> C_E = 19.
              On the noisy scenes 13.7 without and 124 with weights -> C_E = 995: a sample that holds outliers gives an F far from any
              essential matrix, and the projection to singular values (1, 1, 0) amplifies by 1 / (e2 - e3) of F, which this scale
              does not know -- with the admission filter that bound allows more than two essential matrices can differ by.  So every
              hypothesis is ALSO held to the scale that knows it:
    hyp_E, sharp   |hyp_E - ref| <= C_E_GAIN eps32 sigma_1 / sigma_8 max(1, e1 / (e2 - e3)), e the singular values of the reference's F
              (_consensus_ref.projection_gain), compared where that scale is <= 1e-2: at least 95 % of a case (99.6 .. 100 %).  Largest
              ratio of the restatement 2.32 on the exact scenes (the gain is 1 there) and 0.83 on the noisy ones (gain up to 755,
              median 3.5) -> C_E_GAIN = 19 for all cases.
    hyp_cost  against the fp64 cost of the kernel's OWN hyp_E, the form of tests/test_gpu_refine.py: the residual s = sqrt(d) of a row
              carries an absolute rounding error ds ~ eps32, s^2 moves by 2 s ds + ds^2:  |c - c64| <= C_COST eps32 (sqrt(c64) + eps32).
              Largest ratio 0.375 (the noisy scenes; 0.05 .. 0.33 on the exact ones, whose cost is of the order eps32^2) -> C_COST = 3.01.
    w_out     |w_out - w64(E)| / w <= C_W eps32 / tau (tests/test_gpu_eightpoint.py derives the form).  Largest ratio 0.351 (the noisy scenes;
              below 1e-4 on the exact ones, where d is of the order eps32^2) -> C_W = 2.81.
The winner.  best is the argmin of the kernel's own costs, exactly.  Against the reference only the COST of the winner is compared --
runner-up gaps of 1e-4 relative occur, the indices need not agree.  A change dE of E moves the residual of row p by at most
|dE|_F |x2h| |x1h| / sqrt(den_p), tau^2 log1p(d / tau^2) is 1-Lipschitz in d with sqrt(d) / (1 + d / tau^2) <= its square root, and Jensen
gives |c(E + dE) - c(E)| <= 2 k sqrt(c) + k^2, k = |dE|_F max_p |x2h| |x1h| / sqrt(den_p).  With |dE|_F = eps32 sigma_1 / sigma_8 that is
the scale D1(m) of the shift of hypothesis m's cost under the float32 solve:
    shift     |c64(own hyp_E[m]) - c_ref(m)| <= C_SHIFT D1(m) on the hypotheses NEAR the reference's winner r, c_ref(m) <= 2 c_ref(r) +
              1e-3 tau^2 -- the ones a selection can end on; they fit the inliers, so F is close to an essential matrix and its projection
              is well conditioned, unlike a hypothesis drawn from outliers.  Largest ratio of the restatement 0.107 (n = 130; 1e-5 .. 0.09 elsewhere) -> C_SHIFT = 0.86.
With b(c) = C_COST eps32 (sqrt(c) + eps32) the kernel's winner k then satisfies
    c64(E_k) <= c_k(k) + b <= c_k(r) + b <= c64(hyp_E[r]) + 2 b <= c_ref(r) + C_SHIFT D1(r) + 2 b,
and, where k is near r,  c_ref(r) <= c_ref(k) <= c64(E_k) + C_SHIFT D1(k).
The same argument bounds refine_pose(iters = 0) of the decoded pose against stat[0]: with E' = [t]x R the matrix refine_pose returns,
|c_refine - stat[0]| <= (C_COST + its own C_COST) eps32 (sqrt(c) + eps32) + 2 k sqrt(c) + k^2, k = |E' -+ E|_F max_p ..., and
|E' -+ E|_F <= 1e-5 (the figure of tests/test_gpu_refine.py for a decoded pose).
Measured on the MI355X: hyp_E ratios 0.30 .. 2.39 (exact) and 18 / 50 (noisy), cost ratios 0.02 .. 0.42, w_out ratios up to 0.59, shift
ratios up to 0.15.  The GPU's own worst ratios go to the test report (tests/test_gpu_kernels.py: report)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from tests import _consensus_ref as C
from tests._consensus_ref import (C_COST, C_E, C_E_GAIN, C_SHIFT, C_W, CASES, SEED, TAU, cost_bound, inputs, lipschitz, ratios,  # noqa: F401
                                  reference, shift_scale)
from tests import _eightpoint_ref as R
from tests.test_gpu_kernels import report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_COST_REFINE = 31.0                              # tests/test_gpu_refine.py: C_COST
_IDS = ["%s-n%d-P%d-M%d-%s" % (k, n, P, M, "weighted" if wt else "ones") for k, n, P, M, wt in CASES]


@pytest.fixture(scope="module")
def cs():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, consensus
    _lib.load()
    _lib.load_consensus()
    return consensus


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


def to_numpy(out):
    """rel_pose_amd.consensus.Consensus of device tensors -> tests._consensus_ref.Consensus of numpy arrays (float32 kept)"""
    return C.Consensus(*[None if t is None else t.detach().cpu().numpy() for t in out], None)


@functools.lru_cache(maxsize=None)
def gpu(kind, n, P, M, weighted):
    from rel_pose_amd import consensus
    x1, x2, w, _ = inputs(kind, n, P, M, weighted)
    return consensus.eight_point_consensus(dev(x1), dev(x2), dev(w), tau=TAU, hypotheses=M, seed=SEED, return_weights=True,
                                           return_samples=True)


@pytest.mark.parametrize("kind,n,P,M,weighted", CASES, ids=_IDS)
def test_parity(cs, kind, n, P, M, weighted):
    x1, x2, w, _ = inputs(kind, n, P, M, weighted)
    ref = reference(kind, n, P, M, weighted)
    dout = gpu(kind, n, P, M, weighted)
    assert dout.E.shape == (n, 3, 3) and dout.best.shape == (n,) and dout.stat.shape == (n, 4) and dout.weights.shape == (n, P)
    assert dout.hyp_E.shape == (n, M, 3, 3) and dout.hyp_cost.shape == (n, M) and dout.samples.shape == (n, M, 8)
    assert dout.best.dtype == torch.int32 and dout.samples.dtype == torch.int32
    out = to_numpy(dout)
    assert all(np.isfinite(a).all() for a in out[:7])
    # the sampler, exactly
    assert np.array_equal(out.samples, ref.samples)
    r = ratios(out, ref, x1, x2, w)
    tag = "consensus_%s_n%d_P%d_M%d_%s" % (kind, n, P, M, "w" if weighted else "ones")
    report(tag, E_ratio=r["E"], E_gain_ratio=r["E_gain"], cost_ratio=r["cost"], w_ratio=r["w"], shift_ratio=r["shift"], compared=r["compared"])
    print(tag, "hyp_E ratio %.3g (C %.3g), cost ratio %.3g (C %.3g), w ratio %.3g (C %.3g), shift ratio %.3g (C %.3g), compared %.4f"
          % (r["E"], C_E[kind], r["cost"], C_COST, r["w"], C_W, r["shift"], C_SHIFT, r["compared"]))
    print(tag, "sharp hyp_E ratio %.3g (C %.3g), compared %.4f" % (r["E_gain"], C_E_GAIN, r["compared_gain"]))
    assert r["compared"] >= 0.95 and r["compared_gain"] >= 0.95
    assert r["E_gain"] <= C_E_GAIN
    assert r["E"] <= C_E[kind] and r["cost"] <= C_COST and r["w"] <= C_W and r["shift"] <= C_SHIFT
    # selection: the lowest-index argmin of the kernel's own costs, and what follows from it bit for bit
    assert np.array_equal(out.best, out.hyp_cost.argmin(-1))
    pick = np.arange(n)
    assert np.array_equal(out.E.view(np.int32), out.hyp_E[pick, out.best].view(np.int32))
    assert np.array_equal(out.stat[:, 0].view(np.int32), out.hyp_cost[pick, out.best].view(np.int32))
    assert np.array_equal(out.stat[:, 2], (out.hyp_cost < C.FLT_MAX).sum(-1)) and np.array_equal(out.stat[:, 2:], ref.stat[:, 2:])
    sv = np.linalg.svd(out.E.astype(np.float64), compute_uv=False)
    assert np.abs(sv - [1, 1, 0]).max() < 1e-5                    # on the essential manifold
    lead = np.abs(out.E.reshape(n, 9)).argmax(-1)
    assert bool((out.E.reshape(n, 9)[pick, lead] > 0).all())      # the sign rule
    # the winner against the reference's: by cost (module docstring)
    wc, t = C.clamp(w, n, P), np.full(n, TAU)
    x1d, x2d = x1.astype(np.float64), x2.astype(np.float64)
    c_k = C.cost64(out.E, x1d, x2d, wc, t)
    c_kr = C.cost64(out.hyp_E[pick, ref.best], x1d, x2d, wc, t)
    c_ref = ref.hyp_cost[pick, ref.best]
    near = r["near"]
    assert bool(near[pick, ref.best].all())
    D1 = shift_scale(ref, x1, x2, wc, near)
    upper = c_ref + C_SHIFT * D1[pick, ref.best] + cost_bound(c_k) + cost_bound(c_kr)
    assert bool((c_k <= upper).all()), (c_k, upper)
    near_k = near[pick, out.best]
    assert bool((c_ref <= c_k + C_SHIFT * D1[pick, out.best])[near_k].all())
    report(tag + "_winner", same_index=float((out.best == ref.best).mean()), winner_near=float(near_k.mean()),
           cost_excess_max=float((c_k - c_ref).max()), allowed_min=float((upper - c_ref).min()))
    # the inlier weight share: up to the weight of the rows on the threshold
    share, edge = C.share64(out.E, x1, x2, wc, t)
    assert bool((np.abs(out.stat[:, 1] - share) <= edge + 4e-6).all()), (out.stat[:, 1], share, edge)
    # bit-identical from call to call
    from rel_pose_amd import consensus
    again = consensus.eight_point_consensus(dev(x1), dev(x2), dev(w), tau=TAU, hypotheses=M, seed=SEED, return_weights=True,
                                            return_samples=True)
    assert all(torch.equal(a, b) for a, b in zip(dout, again))
    bare = consensus.eight_point_consensus(dev(x1), dev(x2), dev(w), tau=torch.full((n,), TAU, device="cuda"), hypotheses=M, seed=SEED)
    assert bare.weights is None and bare.samples is None and all(torch.equal(a, b) for a, b in zip(dout[:3], bare[:3]))
    assert torch.equal(bare.hyp_E, dout.hyp_E) and torch.equal(bare.hyp_cost, dout.hyp_cost)


@pytest.mark.parametrize("kind,n,P,M,weighted", CASES, ids=_IDS)
def test_cost_is_the_one_refine_pose_reports(cs, kind, n, P, M, weighted):
    from rel_pose_amd import geom, refine
    x1, x2, w, _ = inputs(kind, n, P, M, weighted)
    dout = gpu(kind, n, P, M, weighted)
    a, b = dev(x1), dev(x2)
    pose, _ = geom.pose_from_essential(dout.E, a, b)
    r = refine.refine_pose(pose, a, b, dev(w), tau=TAU, iters=0)
    E, E2 = host(dout.E).reshape(n, 9), host(r.E).reshape(n, 9)
    delta = R.up_to_sign(E2, E)
    assert float(delta.max()) <= 1e-5, delta.max()
    c = host(dout.stat)[:, 0]
    k = delta * lipschitz(E, x1, x2, C.clamp(w, n, P))
    bound = cost_bound(c, C_COST + C_COST_REFINE) + 2 * k * np.sqrt(c) + k * k
    diff = np.abs(host(r.stat)[:, 0] - c)
    report("consensus_refine_cost_%s_n%d_P%d_%s" % (kind, n, P, "w" if weighted else "ones"), diff_over_bound=float((diff / bound).max()),
           decode_delta=float(delta.max()))
    assert bool((diff <= bound).all()), (diff, bound)


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weighted"])
def test_noisy_scenes_with_half_the_matches_wrong(cs, weighted):
    """ten scenes, 576 matches, 50 % of x2 uniform noise: the best hypothesis lies within 0.25 of the true E in 10 of 10, the chain
    consensus -> eight_point(consensus weights, iters = 4) within 0.1 in 10 of 10, while eight_point(iters = 4) from the all-data start
    is off by at least 0.4 in at least 8 of 10"""
    from rel_pose_amd import eightpoint
    x1, x2, w, Et = inputs("noisy", 10, 576, 1024, weighted)
    out = gpu("noisy", 10, 576, 1024, weighted)
    a, b = dev(x1), dev(x2)
    tau = torch.full((10,), TAU, device="cuda")
    best = R.up_to_sign(host(out.E), Et)
    chain = R.up_to_sign(host(eightpoint.eight_point(a, b, out.weights, tau=tau, iters=4).E), Et)
    plain = R.up_to_sign(host(eightpoint.eight_point(a, b, dev(w), tau=tau, iters=4).E), Et)
    report("consensus_noisy50_%s" % ("w" if weighted else "ones"), best_max=float(best.max()), chain_max=float(chain.max()),
           plain_min=float(plain.min()), plain_wrong=int((plain >= 0.4).sum()), share_min=float(out.stat[:, 1].min()))
    print("best", np.round(best, 3), "chain", np.round(chain, 3), "plain", np.round(plain, 2))
    assert int((best <= 0.25).sum()) == 10, best
    assert int((chain <= 0.1).sum()) == 10, chain
    assert int((plain >= 0.4).sum()) >= 8, plain


def _degenerate_batch():
    x1, x2, _ = R.scenes(6, 40, seed=12)
    x1, x2 = x1.astype(np.float32), x2.astype(np.float32)
    w = np.random.default_rng(1).uniform(0.05, 1, (6, 40)).astype(np.float32)
    tau = np.full(6, 0.02, np.float32)
    return x1, x2, w, tau


def test_degenerate_problems_in_a_batch(cs):
    """seven positive weights (plus a negative one and a NaN), coincident points and tau = 0 between healthy problems: the documented
    outputs, and the healthy neighbours bit-identical to the same batch with healthy problems in those slots (a problem's samples
    depend on its index, so the slots stay)"""
    x1, x2, w, tau = _degenerate_batch()
    M = 70
    healthy = cs.eight_point_consensus(dev(x1), dev(x2), dev(w), tau=dev(tau), hypotheses=M, seed=3, return_weights=True, return_samples=True)
    assert bool((healthy.best >= 0).all()) and bool((healthy.stat[:, 2] == M).all())
    w[1] = 0
    w[1, [3, 5, 9, 20, 30, 38, 39]] = 0.5
    w[1, 7], w[1, 8] = -1.0, np.nan
    x1[3] = x1[3, 17]                                             # every point of image 0 the same: no hypothesis is valid
    tau[5] = 0
    out = cs.eight_point_consensus(dev(x1), dev(x2), dev(w), tau=dev(tau), hypotheses=M, seed=3, return_weights=True, return_samples=True)
    o = to_numpy(out)
    for b, K in ((1, 7), (3, 40), (5, 40)):
        assert not o.E[b].any() and o.best[b] == -1 and np.array_equal(o.stat[b], [0, 0, 0, K]), (b, o.best[b], o.stat[b])
        assert np.array_equal(o.weights[b], C.clamp(w, 6, 40, np.float32)[b])
        assert not o.hyp_E[b].any() and bool((o.hyp_cost[b] == np.float32(C.FLT_MAX)).all())
    assert not o.samples[1].any()
    ref_samples = C.sample_rows(w, 6, 40, 3, M)[1]
    assert np.array_equal(o.samples, ref_samples) and o.samples[3].any() and o.samples[5].any()
    assert all(np.isfinite(a).all() for a in o[:7])
    keep = [0, 2, 4]
    assert all(torch.equal(p[keep], q[keep]) for p, q in zip(out, healthy))
    assert float(out.E[keep].abs().max()) > 0.3


def test_outputs_do_not_depend_on_what_they_held(cs):
    """the raw entry point on outputs filled with NaN and on outputs filled with a finite pattern: the same bits"""
    from rel_pose_amd import _lib
    lib = _lib.load_consensus()
    n, P, M = 3, 257, 300
    x1, x2, w, _ = inputs("exact", 2, 257, 256, True)
    x1, x2, w = dev(np.concatenate([x1, x1[:1]])), dev(np.concatenate([x2, x2[:1]])), dev(np.concatenate([w, w[:1]]))
    tau = torch.full((n,), TAU, device="cuda")
    Pv = ctypes.c_void_p
    runs = []
    for fill in (float("nan"), 12345.0):
        f = [torch.full(s, fill, device="cuda") for s in ((n, 9), (n, 4), (n, P), (n, M, 9), (n, M))]
        i = [torch.full(s, 0x7FC0DEAD if fill != fill else 0x12345678, dtype=torch.int32, device="cuda") for s in ((n,), (n, M, 8))]
        lib.rp_eight_point_consensus(Pv(x1.data_ptr()), Pv(x2.data_ptr()), Pv(w.data_ptr()), Pv(tau.data_ptr()), SEED, Pv(f[0].data_ptr()),
                                     Pv(i[0].data_ptr()), Pv(f[1].data_ptr()), Pv(f[2].data_ptr()), Pv(f[3].data_ptr()), Pv(f[4].data_ptr()),
                                     Pv(i[1].data_ptr()), P, M, n, Pv(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        runs.append([t.view(torch.int32) for t in f] + i)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert all(bool(torch.isfinite(t.view(torch.float32)).all()) for t in runs[0][:5])
    # problems 0 and 2 hold the same data under different indices: other samples
    assert not torch.equal(runs[0][6][0], runs[0][6][2])


def test_another_seed_draws_other_samples(cs):
    x1, x2, w, _ = inputs("exact", 2, 257, 256, False)
    a, b = dev(x1), dev(x2)
    one = gpu("exact", 2, 257, 256, False)
    two = cs.eight_point_consensus(a, b, None, tau=TAU, hypotheses=256, seed=2, return_samples=True)
    assert not torch.equal(one.samples, two.samples)
    assert np.array_equal(two.samples.cpu().numpy(), C.sample_rows(None, 2, 257, 2, 256)[1])
    # the seed is its 32-bit pattern: -1 and 2^32 - 1 are the same seed
    neg = cs.eight_point_consensus(a, b, None, tau=TAU, hypotheses=256, seed=-1, return_samples=True)
    pos = cs.eight_point_consensus(a, b, None, tau=TAU, hypotheses=256, seed=2 ** 32 - 1, return_samples=True)
    assert torch.equal(neg.samples, pos.samples) and torch.equal(neg.hyp_cost, pos.hyp_cost)
    assert np.array_equal(neg.samples.cpu().numpy(), C.sample_rows(None, 2, 257, -1, 256)[1])


def test_refusals_leave_outputs_untouched(cs):
    from rel_pose_amd import _lib
    x = torch.rand(2, _lib.CONSENSUS_MAX_P + 1, 2, device="cuda")
    with pytest.raises(RuntimeError, match=r"rel_pose_amd: rp_eight_point_consensus failed: unsupported \(RP error -4\)"):
        cs.eight_point_consensus(x, x.clone())
    y = x[:, :64].contiguous()
    with pytest.raises(RuntimeError, match=r"unsupported \(RP error -4\)"):
        cs.eight_point_consensus(y, y.clone(), hypotheses=_lib.CONSENSUS_MAX_M + 1)
    with pytest.raises(RuntimeError, match=r"bad shape \(RP error -1\)"):
        cs.eight_point_consensus(y, y.clone(), hypotheses=0)
    lib = _lib.load_consensus()
    n, P, M = 2, 64, 4097
    E, stat, hE, hc = (torch.full(s, -7.0, device="cuda") for s in ((n, 9), (n, 4), (n, 16, 9), (n, 16)))
    best = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    Pv = ctypes.c_void_p
    tau = torch.full((n,), TAU, device="cuda")
    with pytest.raises(RuntimeError, match=r"unsupported \(RP error -4\)"):
        lib.rp_eight_point_consensus(Pv(y.data_ptr()), Pv(y.data_ptr()), None, Pv(tau.data_ptr()), 0, Pv(E.data_ptr()), Pv(best.data_ptr()),
                                     Pv(stat.data_ptr()), None, Pv(hE.data_ptr()), Pv(hc.data_ptr()), None, P, M, n,
                                     Pv(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in (E, stat, hE, hc, best))                                # nothing ran


# ------------------------------------------------------------------------------------------------ model level
def test_model_consensus_pose_from_matches_is_the_chain_of_the_public_pieces(cs):
    """on the synthetic state of __graft_entry__.smoke(): bit for bit the chain assemble_matches -> eight_point_consensus ->
    eight_point(consensus weights) -> pose_from_essential -> refine_pose(base weights)"""
    from oracle import relpose_oracle as O
    from rel_pose_amd import eightpoint, geom, refine
    from tests.test_gpu_memory_contract import _model
    m = _model().eval()
    B = 2
    images = O.synthetic_images(B, 384, 384, key=78).cuda()
    intr = torch.tensor([[0.9 * 384, 0.8 * 384, 192.0, 192.0]]).repeat(B, 2, 1).contiguous().cuda()
    keep_intr = intr.clone()
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True      # two runs from images, bit for bit
    try:
        m.correspondences(images)                                # (warm-up: first calls load code objects and pick solvers)
        state = {k: v.clone() for k, v in m.state_dict().items()}
        cp = m.consensus_pose_from_matches(images, intr, hypotheses=256, seed=5, refine=3)
        assert torch.equal(intr, keep_intr)
        corr = m.correspondences(images)
    finally:
        torch.backends.cudnn.deterministic = keep
    x1, x2, w = eightpoint.assemble_matches(corr, intr, (384, 384))
    tau = eightpoint.default_tau(intr, (384, 384)).contiguous()
    c = cs.eight_point_consensus(x1, x2, w, tau=tau, hypotheses=256, seed=5, return_weights=True)
    ep = eightpoint.eight_point(x1, x2, c.weights, tau=tau, iters=4, return_weights=True)
    pose, count = geom.pose_from_essential(ep.E, x1, x2)
    r = refine.refine_pose(pose, x1, x2, w, tau=tau, iters=3, return_weights=True)
    for got, want in zip(cp[:4], r):
        assert torch.equal(got, want)
    for got, want in zip(cp.consensus, c):
        assert (got is None and want is None) or torch.equal(got, want)
    for got, want in zip(cp.initial, (pose, ep.E, ep.stat, count, ep.weights)):
        assert torch.equal(got, want)
    assert cp.pose.shape == (B, 7) and cp.consensus.hyp_cost.shape == (B, 256) and cp.consensus.samples is None
    assert bool(torch.isfinite(cp.pose).all()) and bool((cp.stat[:, 1] <= cp.stat[:, 0]).all())
    other = m.consensus_pose_from_matches(images, intr, hypotheses=256, seed=6, refine=3)
    assert not torch.equal(other.consensus.hyp_cost, cp.consensus.hyp_cost)
    after = m.state_dict()
    assert not m.training and set(after) == set(state) and all(torch.equal(after[k], state[k]) for k in state)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.consensus_pose_from_matches(images, intr)


def test_demo_consensus_flag(capsys):
    import re
    sys.path.insert(0, ROOT)
    import demo
    g = os.path.join(ROOT, "tests", "golden", "demo")
    argv = ["--img1", os.path.join(g, "matterport_1.png"), "--img2", os.path.join(g, "matterport_2.png"), "--eight_point"]
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        torch.manual_seed(5)
        demo.main(argv + ["--refine", "2"])
        plain = capsys.readouterr().out
        torch.manual_seed(5)
        demo.main(argv + ["--refine", "2", "--consensus", "128", "--seed", "4"])
        flagged = capsys.readouterr().out.splitlines()
    finally:
        torch.backends.cudnn.deterministic = keep
    lines = plain.splitlines()
    assert "consensus" not in plain
    assert len(flagged) == len(lines) + 1 and flagged[:-2] == lines[:-1]
    assert flagged[-2].startswith("consensus pose ") and flagged[-1].startswith(lines[-1] + ", consensus ")
    numbers = [float(t) for t in re.findall(r"-?\d+\.\d+", flagged[-2])]
    assert len(numbers) == 7 + 2 and all(np.isfinite(numbers))
    pose = np.array(numbers[:7])
    assert abs(np.linalg.norm(pose[:3]) - 1) < 1e-4 and abs(np.linalg.norm(pose[3:]) - 1) < 1e-4 and pose[6] >= 0
    assert np.isfinite(float(flagged[-1].rsplit(" ", 1)[1]))
    with pytest.raises(SystemExit):
        demo.main(argv[:4] + ["--consensus", "8"])
