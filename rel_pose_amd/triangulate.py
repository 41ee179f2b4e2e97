"""Two-view structure: the matches triangulated under a pose, on the GPU.

Every chain of this package answers "where is camera 2?" and reports the Sampson distance.  include/relpose_triangulate.h
(csrc_triangulate/triangulate.hip -- a library of its own) answers "where are the points?": per match the optimal correction onto the
epipolar constraint of the pose (Lindstrom's two steps), the point the two corrected rays meet in, its depth in both cameras, the
parallax and the squared reprojection error, and per problem the robust reprojection cost, the share of the points in front of both
cameras and the mean parallax:

    s = model.eval().structure_from_matches(images, intrinsics)                  # the refined chain's pose
    s = model.eval().structure_from_matches(images, intrinsics, pose=regressed)  # the structure the regressed pose implies
    # or, piece by piece (x1, x2, w, tau as in rel_pose_amd/eightpoint.py):
    st = triangulate(pose, x1, x2, w, tau=tau)
    front = (st.depth1 > 0) & (st.depth2 > 0)

Convention: X2 = R X1 + t with t normalised, so points and depths are in units of the baseline; points are in the frame of camera 1.
There is no fallback for the kernel."""
import collections

import torch

from . import _lib, ops
from .ops import _chk, _p, _st

Structure = collections.namedtuple("Structure", "points depth1 depth2 reproj parallax stat corrected")
Structure.__doc__ = """points [n,P,3] in the frame of camera 1 (all zero for a row at infinity and for a degenerate problem), depth1 /
depth2 [n,P] the depths in camera 1 / camera 2 (a negative depth is information about the match), reproj [n,P] the squared reprojection
error summed over both images, parallax [n,P] in radians, stat [n,4] = (the robust reprojection cost, the Cauchy-weighted share in front
of both cameras, the Cauchy-weighted mean parallax in radians, the number of rows of positive weight), corrected [n,P,4] = (x1c, x2c)
the corrected matches, or None"""
MatchStructure = collections.namedtuple("MatchStructure", "structure pose x1 x2 weights tau chain")
MatchStructure.__doc__ = """structure: the Structure of the matches under `pose` [B,7]; x1, x2 [B,P,2], weights [B,P] and tau [B] the matches,
their base weights and the scale it was computed with; chain: what the named chain returned, or None where the pose was passed"""

CHAINS = ("eight", "refined", "consensus", "planar")


def triangulate(pose, x1, x2, w=None, tau=0.01, return_corrected=False):
    """pose [n,7] = (t, q xyzw) with X2 = R X1 + t (normalised internally), x1, x2 [n,P,2] calibrated image coordinates, w [n,P] base
    weights (None: ones; they enter `stat` only), tau: float or [n], the scale of the robust cost
    mean(w tau^2 log1p(reproj / tau^2)) -> Structure.  1 <= P <= 1728."""
    if x1.dim() != 3 or x1.shape[-1] != 2 or x1.shape != x2.shape:
        raise ValueError("x1 and x2 must have the same shape [n,P,2]")
    n, P = x1.shape[:2]
    if tuple(pose.shape) != (n, 7):
        raise ValueError("pose must be [n,7]")
    if w is not None and tuple(w.shape) != (n, P):
        raise ValueError("w must be [n,P]")
    if tau is None:
        raise ValueError("the robust cost needs tau")
    if not torch.is_tensor(tau):
        tau = torch.full((n,), float(tau), device=x1.device, dtype=torch.float32)
    if tuple(tau.shape) != (n,):
        raise ValueError("tau must be a number or [n]")
    lib = _lib.load_triangulate()
    _chk(pose, x1, x2, w, tau)
    X = ops._empty(n, P, 3, like=x1)
    aux = ops._empty(n, P, 4, like=x1)
    stat = ops._empty(n, 4, like=x1)
    xc = ops._empty(n, P, 4, like=x1) if return_corrected else None
    lib.rp_triangulate(_p(pose), _p(x1), _p(x2), _p(w), _p(tau), _p(X), _p(aux), _p(xc), _p(stat), P, n, _st())
    return Structure(X, aux[..., 0], aux[..., 1], aux[..., 2], aux[..., 3], stat, xc)


def structure_from_matches(model, images, intrinsics, pose=None, chain="refined", **chain_kwargs):
    """ViTEss.structure_from_matches: the composition of the public pieces and nothing else -- eightpoint._matches_of -> the named chain
    (model.pose_from_matches, refined_pose_from_matches, consensus_pose_from_matches or planar_pose_from_matches with `chain_kwargs`;
    "planar" uses its first pick) -> triangulate on the same matches, base weights and tau -> MatchStructure.  A given pose [B,7] is used
    as it is and no chain runs: that is how the structure and the reprojection cost implied by the network's own regressed pose are
    obtained.  Of chain_kwargs, heads, subtoken, radius and tau also select the matches that are triangulated."""
    from . import eightpoint
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
    return MatchStructure(triangulate(pose, x1, x2, w, tau=tau, return_corrected=True), pose, x1, x2, w, tau, result)
