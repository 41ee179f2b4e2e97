"""The scalar geometry kernels at wide baselines and at the edges of their domain, on a real MI355X: svd3x3_dev (csrc/svd3x3.h through
rp_svd3x3), the decode rp_pose_from_essential (csrc/geom.hip) and the geodesic loss (csrc/se3loss.hip).

Inputs, fp64 references, bounds and the calibration of every constant are in tests/_geometry_edges.py (the loss, the special matrices of
the SVD) and tests/_eightpoint_ref.py: wide_scenes (rotations up to a half-turn).  The bounds of the SVD and of the decode are those of
tests/test_gpu_kernels.py: test_svd3x3_and_essential_matrix_vs_lapack and test_pose_from_essential_round_trip, unchanged.
tools/lab/geom_host/run.py runs the same checks with the kernels compiled for the host.  The GPU's own worst figures go to the test report
(tests/test_gpu_kernels.py: report)."""
import numpy as np
import pytest
import torch

from oracle import svd3x3_oracle as SO
from tests import _eightpoint_ref as R
from tests import _geometry_edges as G
from tests.test_gpu_kernels import report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def geom():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, geom as g
    _lib.load()
    return g


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(*ts):
    return tuple(t.detach().cpu().numpy() for t in ts)


# ------------------------------------------------------------------------------------------------ decode
def test_decode_at_wide_baselines(geom):
    """rp_pose_from_essential on the float32 E_true of 90 scenes per kind of wide_scenes, P = 12: against the true pose (angle < 2e-3 rad,
    quaternions up to sign; cos of the direction of t > 1 - 1e-6; every point in front) and against the LAPACK decode on 40 of them (R and
    t within 5e-4).  The true rotations take every branch of the rotation -> quaternion conversion at least 20 times (measured: trace 180,
    R00 63, R11 58, R22 59).  The kernel compiled for the host reaches 8.1e-4 rad and R, t within 3e-7 of the oracle."""
    branches = np.zeros(4, int)
    for kind in R.WIDE_KINDS:
        E, x1, x2, pose = G.decode_inputs(kind)
        P = x1.shape[1]
        out, count = host(*geom.pose_from_essential(dev(E), dev(x1), dev(x2)))
        ang, cos_t = G.decode_errors(out, pose)
        Ro, to, co = SO.decode_essential(E[:40], x1[:40], x2[:40])
        dR = float(np.abs(SO.rotation_from_quat(out[:40, 3:]) - Ro).max())
        dt = float(np.abs(out[:40, :3].astype(np.float64) - to).max())
        report("decode_" + kind, max_angle=float(ang.max()), min_cos_t=float(cos_t.min()), oracle_R=dR, oracle_t=dt, count_min=float(count.min()))
        print(kind, "angle %.3g, 1 - cos_t %.3g, oracle R %.3g t %.3g" % (ang.max(), 1 - cos_t.min(), dR, dt))
        assert np.isfinite(out).all()
        assert bool((count == P).all()), (kind, count.min())
        assert float(ang.max()) < 2e-3 and float(cos_t.min()) > 1.0 - 1e-6, (kind, ang.max(), cos_t.min())
        assert float(np.abs(np.linalg.norm(out[:, :3], axis=-1) - 1).max()) < 1e-5 and bool((out[:, 6] >= 0).all())
        assert float(np.abs(np.linalg.norm(out[:, 3:], axis=-1) - 1).max()) < 1e-5
        assert dR < 5e-4 and dt < 5e-4, (kind, dR, dt)
        assert bool((co == P).all())
        branches += np.bincount([R.shepperd_branch(r) for r in SO.rotation_from_quat(pose[:, 3:])], minlength=4)
    assert int(branches.min()) >= 20, branches


# ------------------------------------------------------------------------------------------------ svd
def _svd(geom, A):
    return host(*geom.svd3x3(dev(A)))


@pytest.mark.parametrize("tag", ["rotation", "signed_permutation", "repeated_diagonal", "rank2_equal"])
def test_svd_of_matrices_with_equal_singular_values(geom, tag):
    """rotations (a triple singular value), the 48 signed permutations, diagonals with repeated and zero entries, U diag(1, 1, 0) V^T: the
    bounds of the existing per-tag checks (3e-6 on the singular values, the reconstruction and the orthogonality of U and V)"""
    A = G.svd_special()[tag]
    e_s, e_rec, e_orth, ordered = G.svd_errors(A, *_svd(geom, A))
    report("svd3x3_" + tag, values=e_s, reconstruction=e_rec, orthogonality=e_orth)
    assert ordered
    assert e_s < 3e-6 and e_rec < 3e-6 and e_orth < 3e-6, (tag, e_s, e_rec, e_orth)


@pytest.mark.parametrize("scale", [1e15, 1e-15, 1e30, 1e-30])
def test_svd_away_from_unit_scale(geom, scale):
    """N(0, 1) matrices times 1e+-15 and 1e+-30 against LAPACK at the unit-scale bounds.  Without the scaling at the entry of svd3x3_dev the
    skip test's alpha beta overflows from |A| ~ 4e9 on (at 1e15: singular values off by 0.66, U^T U - I of 1.0), and the squared column
    norms leave the normal range below ~1e-19."""
    A = G.svd_generic() * np.float32(scale)
    assert np.isfinite(A).all() and float(np.abs(A).max()) >= 1.2e-38
    e_s, e_rec, e_orth, ordered = G.svd_errors(A, *_svd(geom, A))
    report("svd3x3_scale_%g" % scale, values=e_s, reconstruction=e_rec, orthogonality=e_orth)
    assert ordered
    assert e_s < 3e-6 and e_rec < 3e-6 and e_orth < 3e-6, (scale, e_s, e_rec, e_orth)


def test_svd_is_scale_equivariant_bit_for_bit(geom):
    """S(2^k A) == 2^k S(A) and U, V bit-equal for k = -100 .. 100 (256 N(0, 1) matrices, all k in one launch).  For k = -20 .. 20 this
    held before A was scaled at entry: the scaling changed no in-range result."""
    A0 = G.svd_generic()
    ks = np.arange(-100, 101)
    A = np.ldexp(A0[None], ks[:, None, None, None]).astype(np.float32)
    assert np.array_equal(np.ldexp(A, -ks[:, None, None, None]), np.broadcast_to(A0, A.shape))         # the inputs are exact
    U0, S0, V0 = _svd(geom, A0)
    U, S, V = _svd(geom, A)
    bad = [int(k) for i, k in enumerate(ks)
           if not (np.array_equal(U[i], U0) and np.array_equal(V[i], V0) and np.array_equal(S[i], np.ldexp(S0, k)))]
    report("svd3x3_equivariance", scales_that_differ=float(len(bad)))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ loss
def test_loss_sweep_over_its_branch_thresholds(geom):
    """The fused loss over theta in LOSS_THETAS x |tau| in LOSS_TAUS (tests/_geometry_edges.py: inputs, fp64 references, the bounds and
    their constants C_ROT = 22.4, C_TR = 52, C_VAL_TR = 21.8, C_VAL_ROT = 22.3, each 8 x the float32 CPU run's worst ratio).  Gradients
    come from one call over all 85 pairs, values from B = 1 calls; everything is finite, the half-turn rows included.  The kernel compiled
    for the host reaches 3.4 / 6.5 / 2.3 / 3.4; with c(theta) from its closed form above 1e-4 its translation gradient reaches 239."""
    from rel_pose_amd.losses import geodesic_loss_tensors
    Ps, Gs, grid = G.loss_sweep()
    ref = G.loss_reference()
    g_tr, g_rot = G.loss_gradients(geodesic_loss_tensors, Ps.cuda(), Gs.cuda())
    v_tr, v_rot = G.loss_values(geodesic_loss_tensors, Ps.cuda(), Gs.cuda())
    assert all(np.isfinite(a).all() for a in (g_tr, g_rot, v_tr, v_rot))
    r_rot, r_tr, r_vtr, r_vrot, kink = G.loss_ratios(g_tr, g_rot, v_tr, v_rot, ref)
    worst = dict(rot=float(np.nanmax(r_rot)), tr=float(np.nanmax(r_tr)), value_tr=float(np.nanmax(r_vtr)), value_rot=float(np.nanmax(r_vrot)),
                 kink=kink)
    report("geodesic_loss_sweep", **worst)
    for name, r in (("rot", r_rot), ("tr", r_tr), ("value_tr", r_vtr), ("value_rot", r_vrot)):
        k = int(np.nanargmax(r))
        print("%s ratio %.3g at theta %.3g |tau| %.3g" % (name, np.nanmax(r), grid[k, 0], grid[k, 1]))
    assert worst["rot"] <= G.C_ROT and worst["tr"] <= G.C_TR, worst
    assert worst["value_tr"] <= G.C_VAL_TR and worst["value_rot"] <= G.C_VAL_ROT, worst
    assert kink <= 1 + 1e-5, kink


def test_fused_loss_under_the_tangent_gradient_convention(geom, monkeypatch):
    """GRADIENT_CONVENTION = "tangent": the fused kernel's gradient, converted by se3.tangent_gradient, equals the fp64 PyTorch path under the
    same convention on the 37 generic pairs of test_fused_geodesic_loss_matches_se3_autograd, at its 2e-5"""
    from rel_pose_amd import losses
    from rel_pose_amd.se3 import SE3, with_tangent_gradient
    from tests.test_gpu_kernels import rel
    monkeypatch.setattr(losses, "GRADIENT_CONVENTION", "tangent")
    g = torch.Generator(device="cpu").manual_seed(3)
    B = 37

    def poses(scale):
        q = torch.randn(B, 2, 4, generator=g)
        q = q / q.norm(dim=-1, keepdim=True)
        return torch.cat([torch.randn(B, 2, 3, generator=g) * scale, q], -1)
    Ps, Gs = poses(1.0), poses(0.7)
    Ps[:, 0] = torch.tensor([0, 0, 0, 0, 0, 0, 1.0])
    Gs[:, 0] = torch.tensor([0, 0, 0, 0, 0, 0, 1.0])
    Gs[0, 1] = Ps[0, 1]
    Gs[1, 1, 3:] = -Gs[1, 1, 3:]
    Gs[2, 1, 3:] = torch.tensor([0.0, 0.0, 0.96, -0.28])
    Gr = Gs.double().requires_grad_(True)
    ltr_r, lrot_r = losses.geodesic_loss_tensors_torch(SE3(Ps.double()), [with_tangent_gradient(SE3(Gr))])
    (10.0 * ltr_r + 7.0 * lrot_r).backward()
    Gg = Gs.cuda().requires_grad_(True)
    ltr, lrot = losses.geodesic_loss_tensors(SE3(Ps.cuda()), [SE3(Gg)])
    (10.0 * ltr + 7.0 * lrot).backward()
    e = dict(tr=rel(ltr, ltr_r), rot=rel(lrot, lrot_r), grad=rel(Gg.grad[1:], Gr.grad[1:]))
    report("geodesic_loss_tangent", **e)
    assert bool((Gg.grad[..., 6] == 0).all()) and float(Gr.grad[..., :6].abs().max()) > 0.01       # the embedded-tangent form
    assert torch.isfinite(Gg.grad).all()
    assert e["tr"] < 2e-6 and e["rot"] < 2e-6 and e["grad"] < 2e-5, e
