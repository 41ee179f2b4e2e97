"""rp_pose_covariance (include/relpose_covariance.h, csrc_covariance/covariance.hip) and what is built on it, on a real MI355X.

The reference is tests/_covariance_ref.py; the constants are 8 x the worst value of its float32 restatement on these same inputs
(asserted by tests/test_covariance_cpu.py; restatement -> constant, and the worst value seen on the MI355X):
    normal    against the fp64 sums: C1 K eps32 sum |term| per entry                                       245.6 -> 2000     device 246
    cov, sd_rot, sd_dir, rho
              against the fp64 algebra applied to the DEVICE's own normal: |dC_ij| <= C2 eps32 kappa sqrt(C_ii C_jj), the three
              scalars to C2 eps32 kappa relative                                                           1.536 -> 12.5    device 1.81
    eig       against eigh of the device's own cov: C_EIG eps32 eig[0]                                     1.726 -> 14      device 1.79
    weak      against eigh's vector, sign rule applied, where eig[0] / eig[1] >= 2 (at least half of every batch, asserted on the
              CPU): angle <= C3 eps32 eig[0] / (eig[0] - eig[1])                                           1.668 -> 13.5    device 1.42
    c         against the fp64 cost: C_COST eps32 c                                                        303.7 -> 2500    device 294
    status, K, frame, the count of rows with psi' < 0
              EQUAL to the float32 restatement (frame: torch.equal with refine's basis rule); no row of these inputs lies within 8 eps32
              of u = 1 (cap: 1 % of the rows, asserted on the CPU), so the count is compared exactly
    cov       exactly symmetric; repeat calls bit-identical, with and without `normal`
The large constants of `normal` and c are the cancellation in x2^T E x1: terms of order 1 sum to a residual of order sigma = 1e-3, so s
carries eps32 / sigma relative error whatever the order of the sums.  The device's own ratios go to the test report."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import _covariance_ref as C
from tests.test_gpu_kernels import report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("cov", "frame", "eig", "weak", "stat", "normal")


@pytest.fixture(scope="module")
def cov():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, covariance
    _lib.load()
    _lib.load_covariance()
    return covariance


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def reference(case):
    a = C.gpu_case(*case)
    return a, C.covariance_ref(*a), C.covariance_f32(*a)


def to_numpy(out):
    n = out.stat.shape[0]
    return C.Covariance(out.cov.cpu().numpy(), out.frame.cpu().numpy().reshape(n, 6), out.eig.cpu().numpy(), out.weak.cpu().numpy(),
                        out.stat.cpu().numpy(), None if out.normal is None else out.normal.cpu().numpy(), None, None, None, None)


def run(cov, pose, x1, x2, w, tau, normal=True):
    return cov.pose_covariance(dev(pose), dev(x1), dev(x2), dev(w), tau=dev(tau), return_normal=normal)


IDS = ["n%d-P%d-%s" % (n, P, "w" if wt else "now") for n, P, wt in C.gpu_cases()]


@pytest.mark.parametrize("case", C.gpu_cases(), ids=IDS)
def test_covariance_against_the_reference(cov, case):
    n, P, weighted = case
    a, r64, r32 = reference(case)
    dout = run(cov, *a)
    assert dout.cov.shape == (n, 5, 5) and dout.frame.shape == (n, 2, 3) and dout.eig.shape == (n, 5) and dout.weak.shape == (n, 5)
    assert dout.stat.shape == (n, 8) and dout.normal.shape == (n, 30) and all(t.dtype == torch.float32 for t in dout)
    out = to_numpy(dout)
    assert all(np.isfinite(getattr(out, f)).all() for f in FIELDS)
    ratios = C.gpu_errors(out, r64)
    print("ratios (normal, cov, eig, weak, cost) %s of constants %s; status %s" %
          (" ".join("%.3g" % v for v in ratios), (C.C1_NORMAL, C.C2_COV, C.C_EIG, C.C3_WEAK, C.C_COST), np.unique(out.stat[:, 0], return_counts=True)))
    report("covariance_" + IDS[C.gpu_cases().index(case)].replace("-", "_"), normal=ratios[0], cov=ratios[1], eig=ratios[2], weak=ratios[3],
           cost=ratios[4])
    # what must be equal
    assert np.array_equal(out.stat[:, 0], r32.stat[:, 0]) and np.array_equal(out.stat[:, 1], r32.stat[:, 1])
    assert np.array_equal(out.stat[:, 5], r32.stat[:, 5]) and not out.stat[:, 7].any()
    assert torch.equal(dout.frame.reshape(n, 6), dev(r32.frame))
    assert torch.equal(dout.cov, dout.cov.transpose(1, 2))
    off = out.stat[:, 0] != C.OK
    assert not out.cov[off].any() and not out.eig[off].any() and not out.weak[off].any() and not out.stat[off, 2:4].any()
    ok = ~off
    assert (np.diff(out.eig[ok], axis=-1) <= 0).all() and (np.abs(np.linalg.norm(out.weak[ok], axis=-1) - 1) < 1e-5).all()
    assert (out.stat[ok, 4] > C.PIVOT_MIN).all() and (out.stat[ok, 4] <= 1).all()
    lead = np.take_along_axis(out.weak[ok], np.abs(out.weak[ok]).argmax(-1)[:, None], -1)
    assert (lead > 0).all()
    # what is bounded
    assert ratios[0] <= C.C1_NORMAL and ratios[1] <= C.C2_COV and ratios[2] <= C.C_EIG and ratios[3] <= C.C3_WEAK and ratios[4] <= C.C_COST
    # bit-identical from call to call, with and without the optional output
    again = run(cov, *a, normal=False)
    assert again.normal is None and all(torch.equal(p, q) for p, q in zip(dout[:5], again[:5]))
    third = run(cov, *a)
    assert all(torch.equal(p, q) for p, q in zip(dout, third))


def test_degenerate_and_undetermined_problems_between_healthy_neighbours(cov):
    """every cause of status 0 -- K = 5 (with a negative and a NaN weight), tau 0, negative and NaN, t = 0, |t| and |q| below 1e-30, a NaN
    and an infinity in the pose -- and a status -1 problem (most rows between tau and 3 tau), each between neighbours whose bits do not
    change; status 0 zeroes every output, status -1 keeps K, rho, the count, c, frame and normal"""
    n, P = 20, 64
    pose, x1, x2, w, tau = C.gpu_case(n, P, True)
    w = np.abs(np.nan_to_num(w)) + np.float32(0.05)
    healthy = run(cov, pose, x1, x2, w, tau)
    pose, x1, x2, w, tau = pose.copy(), x1.copy(), x2.copy(), w.copy(), tau.copy()
    tau[1], tau[2], tau[5] = 0, -3e-3, np.nan                       # the problems b % 4 in (1, 2); their neighbours b % 4 in (0, 3) stay
    w[6] = 0
    w[6, [3, 9, 20, 33, 60]] = 0.5
    w[6, 5], w[6, 7] = -1.0, np.nan
    pose[9, :3] = 0
    pose[10, :3] *= 1e-36
    pose[13, 3:] *= 1e-36
    pose[14, 4] = np.nan
    pose[17, 1] = np.inf
    pose[18], x1[18], x2[18] = C.not_determined_problem(P)
    tau[18], w[18] = 3e-3, 1.0
    dout = run(cov, pose, x1, x2, w, tau)
    out = to_numpy(dout)
    assert all(np.isfinite(getattr(out, f)).all() for f in FIELDS)
    for b in (1, 2, 5, 6, 9, 10, 13, 14, 17):
        assert all(not getattr(out, f)[b].any() for f in FIELDS), b
    r32 = C.covariance_f32(pose[18:19], x1[18:19], x2[18:19], w[18:19], tau[18:19])
    s = out.stat[18]
    assert s[0] == C.NOT_DETERMINED and s[1] == P and s[5] >= 0.7 * P and s[5] == r32.stat[0, 5] and s[6] > 0 and s[4] <= C.PIVOT_MIN and s[7] == 0
    assert not out.cov[18].any() and not out.eig[18].any() and not out.weak[18].any() and not s[2:4].any()
    assert np.array_equal(out.frame[18], r32.frame[0]) and out.normal[18].any()
    keep = [b for b in range(n) if b % 4 in (0, 3)]
    assert all(torch.equal(p[keep], q[keep]) for p, q in zip(dout, healthy))
    assert set(np.unique(out.stat[keep, 0]).tolist()) == {C.OK, C.NOT_DETERMINED}               # the neighbours are of both kinds


def test_refusals(cov):
    """every refusal returns its code before any launch, in the documented order: shape, then size, then alignment"""
    from rel_pose_amd import _lib
    shape, size = r"rp_pose_covariance failed: bad shape \(RP error -1\)", r"rp_pose_covariance failed: unsupported \(RP error -4\)"
    align = r"rp_pose_covariance failed: misaligned pointer/stride \(RP error -2\)"
    x = torch.rand(2, _lib.COVARIANCE_MAX_P + 1, 2, device="cuda")
    p = torch.tensor([[1.0, 0, 0, 0, 0, 0, 1]], device="cuda").repeat(2, 1)
    with pytest.raises(RuntimeError, match=size):
        cov.pose_covariance(p, x, x.clone())
    with pytest.raises(RuntimeError, match=shape):
        cov.pose_covariance(p, x[:, :5].contiguous(), x[:, :5].contiguous())
    lib, P_ = _lib.load_covariance(), ctypes.c_void_p
    buf = torch.zeros(16384, device="cuda")
    ptr = lambda k: P_(buf.data_ptr() + 4096 * k)                                            # noqa: E731
    args = [ptr(1), ptr(2), ptr(3), None, ptr(4), ptr(5), ptr(6), ptr(7), ptr(8), ptr(9), None]
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 9):
        with pytest.raises(RuntimeError, match=shape):
            lib.rp_pose_covariance(*(args[:i] + [None] + args[i + 1:]), 8, 1, None)
    for bad in (dict(P=8, n=0), dict(P=8, n=-1), dict(P=5, n=1)):
        with pytest.raises(RuntimeError, match=shape):
            lib.rp_pose_covariance(*args, bad["P"], bad["n"], None)
    for i in (1, 2):
        with pytest.raises(RuntimeError, match=align):
            lib.rp_pose_covariance(*(args[:i] + [P_(buf.data_ptr() + 4096 * (i + 1) + 4)] + args[i + 1:]), 8, 1, None)
    for i in range(11):
        with pytest.raises(RuntimeError, match=align):
            lib.rp_pose_covariance(*(args[:i] + [P_(buf.data_ptr() + 4096 * 12 + 2)] + args[i + 1:]), 8, 1, None)
    off = args[:1] + [P_(buf.data_ptr() + 4096 * 2 + 4)] + args[2:]
    with pytest.raises(RuntimeError, match=size):                                             # size before alignment
        lib.rp_pose_covariance(*off, _lib.COVARIANCE_MAX_P + 1, 1, None)
    with pytest.raises(RuntimeError, match=shape):                                            # shape before size and alignment
        lib.rp_pose_covariance(*off, _lib.COVARIANCE_MAX_P + 1, 0, None)
    torch.cuda.synchronize()
    assert not buf.any()                                                                      # nothing was launched


# ------------------------------------------------------------------------------------------------ model level
CHAINS = {"eight": ("pose_from_matches", dict(iters=2)), "refined": ("refined_pose_from_matches", dict(refine=3)),
          "consensus": ("consensus_pose_from_matches", dict(hypotheses=128, seed=5, refine=2)),
          "planar": ("planar_pose_from_matches", dict(hypotheses=128, seed=5, refine=3))}


@pytest.fixture(scope="module")
def setup(cov):
    from oracle import relpose_oracle as O
    from tests.test_gpu_memory_contract import _model
    m = _model().eval()
    B = 2
    images = O.synthetic_images(B, 384, 384, key=78).cuda()
    intr = torch.tensor([[0.9 * 384, 0.8 * 384, 192.0, 192.0]]).repeat(B, 2, 1).contiguous().cuda()
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    m.correspondences(images)                                    # (warm-up)
    yield m, images, intr
    torch.backends.cudnn.deterministic = keep


def same(p, q):
    return all((a is None and b is None) or (torch.equal(a, b) if torch.is_tensor(a) else a == b if not isinstance(a, tuple) else same(a, b))
               for a, b in zip(p, q))


@pytest.mark.parametrize("chain", list(CHAINS) + ["pose"])
def test_pose_uncertainty_from_matches_is_the_composition_of_the_public_pieces(cov, setup, chain):
    """the chain's result equals the model's own chain method, the covariance equals pose_covariance on eightpoint._matches_of's rows,
    their base weights and the default tau, bit for bit; the model's state and `intrinsics` are what they were"""
    from rel_pose_amd import eightpoint
    m, images, intr = setup
    B = images.shape[0]
    before = intr.clone()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    x1, x2, w, hw = eightpoint._matches_of(m, images, intr, (0, 1, 2), None, 2)
    tau = eightpoint.default_tau(intr, hw).to(x1.device).contiguous()
    if chain == "pose":                                          # the regressed pose, as a caller would pass it
        Gs = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device="cuda").repeat(B, 2, 1)
        with torch.no_grad():
            pose = m(images, Gs, intrinsics=intr.clone())[0].data[:, 1].contiguous()
        result, pc = m.pose_uncertainty_from_matches(images, intr, pose=pose)
        assert result is None
    else:
        name, kw = CHAINS[chain]
        want = getattr(m, name)(images, intr, **kw)
        pose = want.pose
        result, pc = m.pose_uncertainty_from_matches(images, intr, chain=chain, **kw)
        assert type(result) is type(want) and same(result, want)
    assert torch.equal(intr, before) and not m.training and all(torch.equal(v, m.state_dict()[k]) for k, v in state.items())
    assert type(pc) is cov.PoseCovariance and same(pc, cov.pose_covariance(pose.contiguous(), x1, x2, w, tau=tau, return_normal=True))
    assert pc.cov.shape == (B, 5, 5) and pc.normal.shape == (B, 30) and all(bool(torch.isfinite(t).all()) for t in pc)
    assert bool(((pc.stat[:, 0] == 1) | (pc.stat[:, 0] == 0) | (pc.stat[:, 0] == -1)).all())
    live = pc.stat[:, 0] != 0
    assert torch.equal(pc.stat[live, 1], (w > 0).sum(-1).float()[live])
    assert torch.equal(cov.rotation_sd_deg(pc), pc.stat[:, 2] * (180.0 / np.pi))
    c3 = cov.translation_cov3(pc)
    assert c3.shape == (B, 3, 3) and torch.allclose(c3.diagonal(dim1=1, dim2=2).sum(-1), pc.cov[:, 3, 3] + pc.cov[:, 4, 4], rtol=1e-4, atol=1e-12)


def test_pose_uncertainty_from_matches_raises_in_train_mode(setup):
    m, images, intr = setup
    m.train()
    try:
        for kw in ({}, dict(pose=torch.zeros(images.shape[0], 7, device="cuda")), dict(chain="eight")):
            with pytest.raises(RuntimeError, match="eval"):
                m.pose_uncertainty_from_matches(images, intr, **kw)
    finally:
        m.eval()


def test_demo_uncertainty_flag(cov, capsys):
    sys.path.insert(0, ROOT)
    import demo
    g = os.path.join(ROOT, "tests", "golden", "demo")
    argv = ["--img1", os.path.join(g, "matterport_1.png"), "--img2", os.path.join(g, "matterport_2.png"), "--eight_point", "--uncertainty"]
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        torch.manual_seed(5)
        demo.main(argv)
        out = [l for l in capsys.readouterr().out.splitlines() if l.startswith("uncertainty")]
        torch.manual_seed(5)
        demo.main(argv + ["--consensus", "64"])
        cons = [l for l in capsys.readouterr().out.splitlines() if l.startswith("uncertainty")]
    finally:
        torch.backends.cudnn.deterministic = keep
    for lines, chain in ((out, "refined"), (cons, "consensus")):
        assert lines[0].startswith("uncertainty (%s chain) pose x,y,z,qx,qy,qz,qw: " % chain) and lines[-1].startswith("uncertainty: rho ")
        rho, beyond, rows, cost = re.fullmatch(r"uncertainty: rho (\S+), (\d+) of (\d+) weighted matches beyond tau, robust cost (\S+)", lines[-1]).groups()
        assert np.isfinite([float(rho), float(cost)]).all() and 0 <= int(beyond) <= int(rows) <= 1728
        if len(lines) == 4:                                       # status 1: the pose with its "+-", and the weak direction
            sd = re.fullmatch(r"uncertainty: rotation \+- (\S+) deg, translation direction \+- (\S+) deg", lines[1])
            weak = re.fullmatch(r"uncertainty: weak direction \(w0 w1 w2 b1 b2\) ((?:\S+ ){4}\S+), \+- (\S+) deg along it", lines[2])
            assert sd and weak and all(np.isfinite(float(v)) and float(v) >= 0 for v in sd.groups()) and 0 < float(rho) <= 1
            v = np.array([float(t) for t in weak.group(1).split()])
            assert abs(np.linalg.norm(v) - 1) < 1e-3 and v[np.abs(v).argmax()] > 0
        else:                                                     # status -1 or 0: words in the place of the numbers
            assert len(lines) == 3 and lines[1] in ("uncertainty: not determined (the matches do not fix the pose at this tau)",
                                                    "uncertainty: degenerate (too few matches, or no pose)")
    with pytest.raises(SystemExit):
        demo.main(argv[:4] + ["--uncertainty"])
