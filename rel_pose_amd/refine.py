"""Refinement of a two-view pose on the essential manifold, and the robust score of a pose against matches.

rp_refine_pose (include/relpose_refine.h, csrc_refine/refine_pose.hip -- a library of its own) follows the linear eight-point solve with
what every classical pipeline puts behind it: Levenberg-Marquardt on the Cauchy-robust Sampson cost over the five degrees of freedom of
(R, t) -- one launch, one workgroup per problem.  With iters = 0 it scores any pose against the matches on one scale.

    rp = model.eval().refined_pose_from_matches(images, intrinsics)    # RefinedMatchPose, all on the GPU
    # or, piece by piece (x1, x2, w, tau, pose as in rel_pose_amd/eightpoint.py):
    r = refine_pose(pose, x1, x2, w, tau=tau, iters=10)
    score = refine_pose(any_pose, x1, x2, w, tau=tau, iters=0).stat[:, 0]

There is no fallback for the kernel."""
import collections

import torch

from . import _lib, ops
from .ops import _chk, _p, _st

RefinedPose = collections.namedtuple("RefinedPose", "pose E stat weights")
RefinedPose.__doc__ = """pose [n,7] = (t unit, q xyzw unit with w >= 0), E [n,3,3] = [t]x R of it (all zero for a degenerate problem, whose
pose is the start unchanged), stat [n,4] = (cost at the start, cost at the output pose, accepted steps, 2-norm of the last accepted step),
weights [n,P] the Cauchy weights at the output pose, or None"""

RefinedMatchPose = collections.namedtuple("RefinedMatchPose", "pose E stat weights initial")
RefinedMatchPose.__doc__ = """pose, E, stat, weights as in RefinedPose; initial: the eightpoint.MatchPose the refinement started from"""


def refine_pose(pose0, x1, x2, w=None, tau=0.01, iters=10, return_weights=False):
    """pose0 [n,7] = (t, q xyzw) with X2 = R X1 + t, x1, x2 [n,P,2] normalised image coordinates, w [n,P] base weights (None: ones),
    tau: float or [n], the scale of the robust cost mean(w tau^2 log1p(sampson / tau^2)) -> RefinedPose after `iters`
    Levenberg-Marquardt iterations (0: only the score).  5 <= P <= 1728, iters <= 32."""
    if x1.dim() != 3 or x1.shape[-1] != 2 or x1.shape != x2.shape:
        raise ValueError("x1 and x2 must have the same shape [n,P,2]")
    n, P = x1.shape[:2]
    if tuple(pose0.shape) != (n, 7):
        raise ValueError("pose0 must be [n,7]")
    if w is not None and tuple(w.shape) != (n, P):
        raise ValueError("w must be [n,P]")
    if tau is None:
        raise ValueError("the robust cost needs tau")
    if not torch.is_tensor(tau):
        tau = torch.full((n,), float(tau), device=x1.device, dtype=torch.float32)
    if tuple(tau.shape) != (n,):
        raise ValueError("tau must be a number or [n]")
    lib = _lib.load_refine()
    _chk(pose0, x1, x2, w, tau)
    pose = ops._empty(n, 7, like=x1)
    E = ops._empty(n, 3, 3, like=x1)
    stat = ops._empty(n, 4, like=x1)
    wo = ops._empty(n, P, like=x1) if return_weights else None
    lib.rp_refine_pose(_p(pose0), _p(x1), _p(x2), _p(w), _p(tau), _p(pose), _p(E), _p(stat), _p(wo), P, int(iters), n, _st())
    return RefinedPose(pose, E, stat, wo)


def refined_pose_from_matches(model, images, intrinsics, heads=(0, 1, 2), iters=4, tau=None, refine=10, subtoken=None, radius=2):
    """ViTEss.refined_pose_from_matches: the chain of eightpoint.pose_from_matches and, behind it, refine_pose on the same matches with
    their BASE weights and the same tau.  subtoken, radius: as for eightpoint.pose_from_matches."""
    from . import eightpoint, geom
    x1, x2, w, hw = eightpoint._matches_of(model, images, intrinsics, heads, subtoken, radius)
    if tau is None:
        tau = eightpoint.default_tau(intrinsics, hw).to(x1.device).contiguous()
    ep = eightpoint.eight_point(x1, x2, w, tau=tau, iters=iters, return_weights=True)
    pose, count = geom.pose_from_essential(ep.E, x1, x2)
    r = refine_pose(pose, x1, x2, w, tau=tau, iters=refine, return_weights=True)
    return RefinedMatchPose(r.pose, r.E, r.stat, r.weights, eightpoint.MatchPose(pose, ep.E, ep.stat, count, ep.weights))
