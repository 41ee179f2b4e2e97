"""How well the matches determine a two-view pose: the covariance of the refined pose, on the GPU.

Every chain of this package returns a pose and a cost; none says whether the rotation is good to 0.03 or to 3 degrees.
include/relpose_covariance.h (csrc_covariance/covariance.hip -- a library of its own) evaluates, at a pose, the sandwich covariance
A^-1 B A^-1 of the Cauchy M-estimator that refine.refine_pose minimises, in its five parameters (three rotation angles, two angles of
the direction of t) -- from the matches alone, without a noise scale:

    chain, pc = model.eval().pose_uncertainty_from_matches(images, intrinsics)
    rotation_sd_deg(pc), direction_sd_deg(pc)     # per pair: the "+-" behind the rotation and the direction of t, in degrees
    pc.weak, pc.stat[:, 0]                        # the least determined direction of (omega, beta); 1 ok, 0 degenerate, -1 not determined
    # or, piece by piece (pose, x1, x2, w, tau as in rel_pose_amd/refine.py):
    pc = pose_covariance(pose, x1, x2, w, tau=tau)

A covariance is a variance, not a bias: with many wrong matches inside a wide tau the robust fit is biased and no covariance says so.
There is no fallback for the kernel."""
import collections
import math

import torch

from . import _lib, ops
from .homography import _rows
from .ops import _chk, _p, _st

OK, DEGENERATE, NOT_DETERMINED = 1, 0, -1

PoseCovariance = collections.namedtuple("PoseCovariance", "cov frame eig weak stat normal")
PoseCovariance.__doc__ = """cov [n,5,5] the covariance of (omega_0, omega_1, omega_2, beta_1, beta_2) in radians squared, exactly symmetric;
frame [n,2,3] = (b1, b2), the tangent basis at t the two beta coordinates refer to; eig [n,5] the eigenvalues of cov, descending; weak
[n,5] the unit eigenvector of eig[:, 0], the least determined direction; stat [n,8] = (status: 1 ok, 0 degenerate, -1 not determined;
the rows of positive weight; sd_rot and sd_dir in radians; rho, the smallest pivot of the scaled A; the number of rows with psi' < 0;
the robust cost of refine.refine_pose's stat[:, 1]; 0); normal [n,30] the upper entries of A, then of B, or None.  cov, eig, weak,
sd_rot and sd_dir are zero unless the status is 1."""


def pose_covariance(pose, x1, x2, w=None, tau=0.01, return_normal=False):
    """pose [n,7] = (t, q xyzw) with X2 = R X1 + t -- normally the output of refine.refine_pose --, x1, x2 [n,P,2] normalised image
    coordinates, w [n,P] base weights (None: ones), tau: float or [n], the scale of the robust cost the pose was refined with ->
    PoseCovariance.  6 <= P <= 1728."""
    n, P, tau = _rows(x1, x2, w, tau)
    if tuple(pose.shape) != (n, 7):
        raise ValueError("pose must be [n,7]")
    lib = _lib.load_covariance()
    _chk(pose, x1, x2, w, tau)
    cov = ops._empty(n, 5, 5, like=x1)
    frame = ops._empty(n, 2, 3, like=x1)
    eig = ops._empty(n, 5, like=x1)
    weak = ops._empty(n, 5, like=x1)
    stat = ops._empty(n, 8, like=x1)
    normal = ops._empty(n, 30, like=x1) if return_normal else None
    lib.rp_pose_covariance(_p(pose), _p(x1), _p(x2), _p(w), _p(tau), _p(cov), _p(frame), _p(eig), _p(weak), _p(stat), _p(normal), P, n, _st())
    return PoseCovariance(cov, frame, eig, weak, stat, normal)


def rotation_sd_deg(pc):
    """[n]: the standard deviation of the rotation, sqrt(trace of the rotation block), in degrees (0 unless the status is 1)"""
    return pc.stat[:, 2] * (180.0 / math.pi)


def direction_sd_deg(pc):
    """[n]: the standard deviation of the direction of t, sqrt(trace of the direction block), in degrees (0 unless the status is 1)"""
    return pc.stat[:, 3] * (180.0 / math.pi)


def translation_cov3(pc):
    """[n,3,3]: the covariance of the unit vector t, [b1 b2] C_bb [b1 b2]^T -- of rank two, t itself is its null direction"""
    basis = pc.frame.transpose(1, 2)                                 # [n,3,2], columns b1, b2
    return basis @ pc.cov[:, 3:, 3:] @ pc.frame


def pose_uncertainty_from_matches(model, images, intrinsics, pose=None, chain="consensus", **chain_kwargs):
    """ViTEss.pose_uncertainty_from_matches: the composition of the public pieces and nothing else -- eightpoint._matches_of -> the named
    chain (model.pose_from_matches, refined_pose_from_matches, consensus_pose_from_matches or planar_pose_from_matches with
    `chain_kwargs`; "planar" uses its first pick) -> pose_covariance on the same matches, base weights and tau, with `normal` ->
    (what the chain returned, PoseCovariance).  A given pose [B,7] is used as it is and no chain runs (the first result is None).  Of
    chain_kwargs, heads, subtoken, radius and tau also select the matches the covariance is evaluated on."""
    from . import eightpoint
    from .triangulate import CHAINS
    if chain not in CHAINS:
        raise ValueError("chain must be one of %s" % (CHAINS,))
    heads, subtoken, radius = chain_kwargs.get("heads", (0, 1, 2)), chain_kwargs.get("subtoken"), chain_kwargs.get("radius", 2)
    x1, x2, w, hw = eightpoint._matches_of(model, images, intrinsics, heads, subtoken, radius)
    tau = chain_kwargs.get("tau")
    if tau is None:
        tau = eightpoint.default_tau(intrinsics, hw).to(x1.device).contiguous()
    result = None
    if pose is None:
        method = {"eight": model.pose_from_matches, "refined": model.refined_pose_from_matches,
                  "consensus": model.consensus_pose_from_matches, "planar": model.planar_pose_from_matches}[chain]
        result = method(images, intrinsics, **chain_kwargs)
        pose = result.pose
    elif tuple(pose.shape) != (x1.shape[0], 7):
        raise ValueError("pose must be [B,7]")
    pose = pose.to(device=x1.device, dtype=torch.float32).contiguous()
    return result, pose_covariance(pose, x1, x2, w, tau=tau, return_normal=True)
