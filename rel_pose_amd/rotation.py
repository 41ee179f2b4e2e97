"""Pure-rotation pairs: the model x2h ~ R x1h behind the matches -- two-point consensus and a three-parameter polish, on the GPU.

With t = 0 every E = [t]x R fits the matches, for any t: the essential-matrix chains of rel_pose_amd/consensus.py return a translation
direction that means nothing, and the planar chain of rel_pose_amd/homography.py spends four matches and eight degrees of freedom where
two and three would do.  include/relpose_rotation.h (csrc_rotation/rotation.hip -- a library of its own) fits the rotation itself: two
matches per hypothesis, Levenberg-Marquardt over the three parameters of R on the robust transfer cost:

    rp = model.eval().rotation_from_matches(images, intrinsics)
    rp.stat[:, 1]                                 # the inlier weight share: the evidence for "this pair only rotates"
    # or, piece by piece (x1, x2, w, tau as in rel_pose_amd/eightpoint.py):
    c = rotation_consensus(x1, x2, w, tau=tau, hypotheses=256, seed=0)
    r = rotation_refine(x1, x2, w, c.R, tau=tau, iters=10)

Convention: x2h ~ R x1h, quaternions xyzw with w >= 0; pose = (0, 0, 0, q).  The same seed gives the same samples and the same bits.
There is no fallback for the kernels."""
import collections

import torch

from . import _lib, ops
from .homography import _rows
from .ops import _chk, _p, _st

RotationConsensus = collections.namedtuple("RotationConsensus", "R best stat weights hyp_R hyp_cost samples")
RotationConsensus.__doc__ = """R [n,3,3] the best hypothesis (all zero for a degenerate problem), best [n] int32 its index (-1: degenerate),
stat [n,4] = (its cost, the inlier weight share at it, the number of valid hypotheses, the number of rows of positive weight), weights
[n,P] the Cauchy weights w / (1 + d / tau^2) at R, or None, hyp_R [n,M,3,3] and hyp_cost [n,M] every hypothesis (an invalid one: zeros and
FLT_MAX), samples [n,M,2] int32 the sampled rows, or None"""
RefinedRotation = collections.namedtuple("RefinedRotation", "R pose stat weights")
RefinedRotation.__doc__ = """R [n,3,3], pose [n,7] = (0, 0, 0, q xyzw with w >= 0), stat [n,4] = (the robust cost, the inlier weight share,
the number of accepted steps, the number of rows of positive weight), weights [n,P] the Cauchy weights at R, or None"""
RotationMatchPose = collections.namedtuple("RotationMatchPose", "pose R stat consensus")
RotationMatchPose.__doc__ = """pose [n,7] = (0, 0, 0, q), R [n,3,3] and stat [n,4] the refined rotation and its RefinedRotation.stat --
stat[:, 1], the inlier weight share, is the evidence for "this pair only rotates" --, consensus the RotationConsensus"""


def rotation_consensus(x1, x2, w=None, tau=0.01, hypotheses=256, seed=0, return_weights=False, return_samples=False):
    """x1, x2 [n,P,2] calibrated image coordinates, w [n,P] base weights (None: ones), tau: float or [n], the scale of the robust cost
    mean(w tau^2 log1p(d / tau^2)) of the distance d of include/relpose_rotation.h, `hypotheses` samples of two per problem drawn from
    `seed` -> RotationConsensus.  2 <= P <= 1728, hypotheses <= 4096."""
    n, P, tau = _rows(x1, x2, w, tau)
    M, seed = int(hypotheses), int(seed)
    if not -2 ** 31 <= seed < 2 ** 32:
        raise ValueError("seed must fit 32 bits")
    seed = seed - 2 ** 32 if seed >= 2 ** 31 else seed               # the same 32-bit pattern as a C int
    lib = _lib.load_rotation()
    _chk(x1, x2, w, tau)
    R = ops._empty(n, 3, 3, like=x1)
    stat = ops._empty(n, 4, like=x1)
    hyp_R = ops._empty(n, max(M, 0), 3, 3, like=x1)
    hyp_cost = ops._empty(n, max(M, 0), like=x1)
    best = torch.empty(n, dtype=torch.int32, device=x1.device)
    wo = ops._empty(n, P, like=x1) if return_weights else None
    samples = torch.empty(n, max(M, 0), 2, dtype=torch.int32, device=x1.device) if return_samples else None
    lib.rp_rotation_consensus(_p(x1), _p(x2), _p(w), _p(tau), seed, _p(R), _p(best), _p(stat), _p(wo), _p(hyp_R), _p(hyp_cost),
                              _p(samples), P, M, n, _st())
    return RotationConsensus(R, best, stat, wo, hyp_R, hyp_cost, samples)


def rotation_refine(x1, x2, w, R0, tau=0.01, iters=10, return_weights=False):
    """`iters` Levenberg-Marquardt iterations on the robust cost from R0 [n,3,3] (a near-rotation of any scale) -> RefinedRotation;
    iters = 0 scores R0.  0 <= iters <= 64."""
    n, P, tau = _rows(x1, x2, w, tau)
    if tuple(R0.shape) != (n, 3, 3):
        raise ValueError("R0 must be [n,3,3]")
    lib = _lib.load_rotation()
    _chk(x1, x2, w, tau, R0)
    R = ops._empty(n, 3, 3, like=x1)
    pose = ops._empty(n, 7, like=x1)
    stat = ops._empty(n, 4, like=x1)
    wo = ops._empty(n, P, like=x1) if return_weights else None
    lib.rp_rotation_refine(_p(x1), _p(x2), _p(w), _p(tau), _p(R0), int(iters), _p(R), _p(pose), _p(stat), _p(wo), P, n, _st())
    return RefinedRotation(R, pose, stat, wo)


def rotation_from_matches(model, images, intrinsics, heads=(0, 1, 2), hypotheses=256, seed=0, refine=10, tau=None, subtoken=None, radius=2):
    """ViTEss.rotation_from_matches: the chain of the public pieces and nothing else -- eightpoint.assemble_matches ->
    rotation_consensus -> rotation_refine on the BASE weights -> RotationMatchPose."""
    from . import eightpoint
    x1, x2, w, hw = eightpoint._matches_of(model, images, intrinsics, heads, subtoken, radius)
    if tau is None:
        tau = eightpoint.default_tau(intrinsics, hw).to(x1.device).contiguous()
    c = rotation_consensus(x1, x2, w, tau=tau, hypotheses=hypotheses, seed=seed)
    r = rotation_refine(x1, x2, w, c.R, tau=tau, iters=refine)
    return RotationMatchPose(r.pose, r.R, r.stat, c)
