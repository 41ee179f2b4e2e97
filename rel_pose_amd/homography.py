"""Planar scenes: the plane-induced homography behind the matches -- consensus, polish and decomposition, on the GPU.

Two essential matrices fit the matches of one plane and the Sampson score cannot tell them apart: on a wall, a floor
or a facade that fills both views every chain of rel_pose_amd/consensus.py fails.  include/relpose_homography.h
(csrc_homography/homography.hip -- a library of its own) solves that case: four matches per hypothesis, Levenberg-Marquardt over the
eight degrees of freedom of H on the robust transfer cost, and the closed-form decomposition into at most two physically possible
(R, t, n):

    pp = model.eval().planar_pose_from_matches(images, intrinsics)
    # or, piece by piece (x1, x2, w, tau as in rel_pose_amd/eightpoint.py):
    c = homography_consensus(x1, x2, w, tau=tau, hypotheses=256, seed=0)
    r = homography_refine(x1, x2, w, c.H, tau=tau, iters=10)
    d = pose_from_homography(r.H, x1, x2, w, tau=tau, vis_min=0.99)
    pose = d.pose[torch.arange(len(d.pick)), d.pick[:, 0].long().clamp(min=0)]      # pick = -1: no candidate

Convention: X2 = R X1 + t, the plane n^T X1 = d, x2h ~ H x1h, H ~ R + t n^T / d.  The same seed gives the same samples and the same
bits.  There is no fallback for the kernels."""
import collections

import torch

from . import _lib, ops
from .ops import _chk, _p, _st

HomographyConsensus = collections.namedtuple("HomographyConsensus", "H best stat weights hyp_H hyp_cost samples")
HomographyConsensus.__doc__ = """H [n,3,3] the best hypothesis (Frobenius norm 1; all zero for a degenerate problem), best [n] int32 its
index (-1: degenerate), stat [n,4] = (its cost, the inlier weight share at it, the number of valid hypotheses, the number of rows of
positive weight), weights [n,P] the Cauchy weights w / (1 + d / tau^2) at H, or None, hyp_H [n,M,3,3] and hyp_cost [n,M] every hypothesis
(an invalid one: zeros and FLT_MAX), samples [n,M,4] int32 the sampled rows, or None"""
RefinedHomography = collections.namedtuple("RefinedHomography", "H stat weights")
RefinedHomography.__doc__ = """H [n,3,3] (Frobenius norm 1, the largest entry positive), stat [n,4] = (the robust transfer cost, the inlier
weight share, the number of accepted steps, the number of rows of positive weight), weights [n,P] the Cauchy weights at H, or None"""
HomographyPoses = collections.namedtuple("HomographyPoses", "pose normal cstat pick")
HomographyPoses.__doc__ = """pose [n,4,7] the candidates (t unit, q xyzw, w >= 0) in the order of include/relpose_homography.h, normal
[n,4,3] their plane normals, cstat [n,4,4] = (visibility share, robust Sampson cost, |t| / d, valid 1 / 0), pick [n,2] int32 the two best
(-1: none).  |t| / d = 0 on a valid candidate flags a pure rotation."""
PlanarMatchPose = collections.namedtuple("PlanarMatchPose", "pose H stat candidates pick ambiguous prior consensus")
PlanarMatchPose.__doc__ = """pose [n,7] the picked candidate (zeros where there is none), H [n,3,3] and stat [n,4] the refined homography and
its RefinedHomography.stat, candidates the HomographyPoses, pick [n,2] int32 (re-ordered if `prior` was used), ambiguous [n] bool: a second
candidate also passes vis_min, prior: None or the name of the prior that re-ordered pick, consensus the HomographyConsensus"""


def _rows(x1, x2, w, tau):
    if x1.dim() != 3 or x1.shape[-1] != 2 or x1.shape != x2.shape:
        raise ValueError("x1 and x2 must have the same shape [n,P,2]")
    n, P = x1.shape[:2]
    if w is not None and tuple(w.shape) != (n, P):
        raise ValueError("w must be [n,P]")
    if tau is None:
        raise ValueError("the robust cost needs tau")
    if not torch.is_tensor(tau):
        tau = torch.full((n,), float(tau), device=x1.device, dtype=torch.float32)
    if tuple(tau.shape) != (n,):
        raise ValueError("tau must be a number or [n]")
    return n, P, tau


def homography_consensus(x1, x2, w=None, tau=0.01, hypotheses=256, seed=0, return_weights=False, return_samples=False):
    """x1, x2 [n,P,2] calibrated image coordinates, w [n,P] base weights (None: ones), tau: float or [n], the scale of the robust cost
    mean(w tau^2 log1p(d / tau^2)) of the transfer distance d, `hypotheses` samples of four per problem drawn from `seed` ->
    HomographyConsensus.  4 <= P <= 1728, hypotheses <= 4096."""
    n, P, tau = _rows(x1, x2, w, tau)
    M, seed = int(hypotheses), int(seed)
    if not -2 ** 31 <= seed < 2 ** 32:
        raise ValueError("seed must fit 32 bits")
    seed = seed - 2 ** 32 if seed >= 2 ** 31 else seed               # the same 32-bit pattern as a C int
    lib = _lib.load_homography()
    _chk(x1, x2, w, tau)
    H = ops._empty(n, 3, 3, like=x1)
    stat = ops._empty(n, 4, like=x1)
    hyp_H = ops._empty(n, max(M, 0), 3, 3, like=x1)
    hyp_cost = ops._empty(n, max(M, 0), like=x1)
    best = torch.empty(n, dtype=torch.int32, device=x1.device)
    wo = ops._empty(n, P, like=x1) if return_weights else None
    samples = torch.empty(n, max(M, 0), 4, dtype=torch.int32, device=x1.device) if return_samples else None
    lib.rp_homography_consensus(_p(x1), _p(x2), _p(w), _p(tau), seed, _p(H), _p(best), _p(stat), _p(wo), _p(hyp_H), _p(hyp_cost),
                                _p(samples), P, M, n, _st())
    return HomographyConsensus(H, best, stat, wo, hyp_H, hyp_cost, samples)


def homography_refine(x1, x2, w, H0, tau=0.01, iters=10, return_weights=False):
    """`iters` Levenberg-Marquardt iterations on the robust transfer cost from H0 [n,3,3] (any scale) -> RefinedHomography; iters = 0
    scores H0.  0 <= iters <= 64."""
    n, P, tau = _rows(x1, x2, w, tau)
    if tuple(H0.shape) != (n, 3, 3):
        raise ValueError("H0 must be [n,3,3]")
    lib = _lib.load_homography()
    _chk(x1, x2, w, tau, H0)
    H = ops._empty(n, 3, 3, like=x1)
    stat = ops._empty(n, 4, like=x1)
    wo = ops._empty(n, P, like=x1) if return_weights else None
    lib.rp_homography_refine(_p(x1), _p(x2), _p(w), _p(tau), _p(H0), int(iters), _p(H), _p(stat), _p(wo), P, n, _st())
    return RefinedHomography(H, stat, wo)


def pose_from_homography(H, x1, x2, w=None, tau=0.01, vis_min=0.99):
    """The closed-form decomposition of H [n,3,3] into four candidates (R, t, n), each with its visibility share and its robust Sampson
    cost over the rows -> HomographyPoses."""
    n, P, tau = _rows(x1, x2, w, tau)
    if tuple(H.shape) != (n, 3, 3):
        raise ValueError("H must be [n,3,3]")
    lib = _lib.load_homography()
    _chk(x1, x2, w, tau, H)
    pose = ops._empty(n, 4, 7, like=x1)
    normal = ops._empty(n, 4, 3, like=x1)
    cstat = ops._empty(n, 4, 4, like=x1)
    pick = torch.empty(n, 2, dtype=torch.int32, device=x1.device)
    lib.rp_pose_from_homography(_p(H), _p(x1), _p(x2), _p(w), _p(tau), float(vis_min), _p(pose), _p(normal), _p(cstat), _p(pick), P, n, _st())
    return HomographyPoses(pose, normal, cstat, pick)


PRIORS = ("regressed",)


def pose_distance(a, b):
    """[...]: rotation angle between the poses a, b [...,7] (t, q xyzw) plus the angle between their translation directions, radians"""
    qa, qb = a[..., 3:] / a[..., 3:].norm(dim=-1, keepdim=True).clamp(min=1e-30), b[..., 3:] / b[..., 3:].norm(dim=-1, keepdim=True).clamp(min=1e-30)
    ta, tb = a[..., :3] / a[..., :3].norm(dim=-1, keepdim=True).clamp(min=1e-30), b[..., :3] / b[..., :3].norm(dim=-1, keepdim=True).clamp(min=1e-30)
    return 2 * torch.acos((qa * qb).sum(-1).abs().clamp(max=1)) + torch.acos((ta * tb).sum(-1).clamp(-1, 1))


def order_by_prior(d, vis_min, prior_pose):
    """(pick [n,2] int32, ambiguous [n] bool): where both picked candidates of the HomographyPoses d pass vis_min, they are ordered by
    pose_distance to prior_pose [n,7] (None: left as they are); host torch on [n,2] numbers"""
    pick = d.pick.cpu().clone()
    cs, pose = d.cstat.cpu(), d.pose.double().cpu()
    idx = pick.long().clamp(min=0)
    rows = torch.arange(len(pick))
    passes = (pick >= 0) & (torch.stack([cs[rows, idx[:, k], 0] for k in range(2)], 1) >= vis_min)
    ambiguous = passes[:, 0] & passes[:, 1]
    if prior_pose is not None:
        dist = torch.stack([pose_distance(pose[rows, idx[:, k]], prior_pose.double().cpu()) for k in range(2)], 1)
        swap = ambiguous & (dist[:, 1] < dist[:, 0])
        pick[swap] = pick[swap].flip(1)
    return pick.to(d.pick.device), ambiguous.to(d.pick.device)


def planar_pose_from_matches(model, images, intrinsics, heads=(0, 1, 2), hypotheses=256, seed=0, refine=10, tau=None, subtoken=None,
                             radius=2, vis_min=0.99, prior=None):
    """ViTEss.planar_pose_from_matches: the chain of the public pieces and nothing else -- eightpoint.assemble_matches ->
    homography_consensus -> homography_refine on the BASE weights -> pose_from_homography -> PlanarMatchPose.  prior = "regressed":
    where two candidates pass vis_min they are ordered by pose_distance to the network's own regressed pose."""
    from . import eightpoint
    if prior is not None and prior not in PRIORS:
        raise ValueError("prior must be None or one of %s" % (PRIORS,))
    x1, x2, w, hw = eightpoint._matches_of(model, images, intrinsics, heads, subtoken, radius)
    if tau is None:
        tau = eightpoint.default_tau(intrinsics, hw).to(x1.device).contiguous()
    c = homography_consensus(x1, x2, w, tau=tau, hypotheses=hypotheses, seed=seed)
    r = homography_refine(x1, x2, w, c.H, tau=tau, iters=refine)
    d = pose_from_homography(r.H, x1, x2, w, tau=tau, vis_min=vis_min)
    regressed = None
    if prior == "regressed":
        Gs = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=images.device).repeat(images.shape[0], 2, 1)
        with torch.no_grad():
            regressed = model(images, Gs, intrinsics=intrinsics.clone())[0].data[:, 1]      # (forward rescales its intrinsics in place)
    pick, ambiguous = order_by_prior(d, vis_min, regressed)
    first = pick[:, 0].long()
    pose = d.pose[torch.arange(len(first), device=first.device), first.clamp(min=0)] * (first >= 0).to(d.pose.dtype)[:, None]
    return PlanarMatchPose(pose, r.H, r.stat, d, pick, ambiguous, prior, c)
