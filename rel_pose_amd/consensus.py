"""Consensus eight-point: a seeded hypothesise-and-verify in front of the eight-point solver, on the GPU.

eight_point and refine_pose are local methods started from the all-data least-squares solution; with 30 % of outliers among the matches
that start lies in a wrong basin.  rp_eight_point_consensus (include/relpose_consensus.h, csrc_consensus/consensus.hip
-- a library of its own) draws `hypotheses` minimal samples of eight matches per problem with a counter-based sampler, solves each,
scores each against all matches with the robust cost refine_pose reports, and returns the best together with the Cauchy weights at it:

    cp = model.eval().consensus_pose_from_matches(images, intrinsics)            # ConsensusMatchPose, all on the GPU
    # or, piece by piece (x1, x2, w, tau as in rel_pose_amd/eightpoint.py):
    c = eight_point_consensus(x1, x2, w, tau=tau, hypotheses=1024, seed=0, return_weights=True)
    ep = eight_point(x1, x2, c.weights, tau=tau, iters=4)                         # the all-data solve, started in the right basin
    pose, count = geom.pose_from_essential(ep.E, x1, x2)
    r = refine_pose(pose, x1, x2, w, tau=tau, iters=10)

The same seed gives the same samples and the same bits.  There is no fallback for the kernels."""
import collections

import torch

from . import _lib, ops
from .ops import _chk, _p, _st

Consensus = collections.namedtuple("Consensus", "E best stat weights hyp_E hyp_cost samples")
Consensus.__doc__ = """E [n,3,3] the best hypothesis (all zero for a degenerate problem), best [n] int32 its index (-1: degenerate),
stat [n,4] = (its cost, the inlier weight share at it, the number of valid hypotheses, the number of rows of positive weight),
weights [n,P] the Cauchy weights w / (1 + sampson / tau^2) at E, or None, hyp_E [n,M,3,3] and hyp_cost [n,M] every hypothesis and its
cost (an invalid one: zeros and FLT_MAX), samples [n,M,8] int32 the sampled rows, or None"""

ConsensusMatchPose = collections.namedtuple("ConsensusMatchPose", "pose E stat weights consensus initial")
ConsensusMatchPose.__doc__ = """pose, E, stat, weights as in refine.RefinedPose; consensus: the Consensus the chain started from;
initial: the eightpoint.MatchPose of the all-data solve on the consensus weights, which the refinement started from"""


def eight_point_consensus(x1, x2, w=None, tau=0.01, hypotheses=1024, seed=0, return_weights=False, return_samples=False):
    """x1, x2 [n,P,2] normalised image coordinates (X2 = R X1 + t), w [n,P] base weights (None: ones), tau: float or [n], the scale of
    the robust cost mean(w tau^2 log1p(sampson / tau^2)), `hypotheses` minimal samples per problem drawn from `seed` -> Consensus.
    8 <= P <= 1728, hypotheses <= 4096."""
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
    M, seed = int(hypotheses), int(seed)
    if not -2 ** 31 <= seed < 2 ** 32:
        raise ValueError("seed must fit 32 bits")
    seed = seed - 2 ** 32 if seed >= 2 ** 31 else seed               # the same 32-bit pattern as a C int
    lib = _lib.load_consensus()
    _chk(x1, x2, w, tau)
    E = ops._empty(n, 3, 3, like=x1)
    stat = ops._empty(n, 4, like=x1)
    hyp_E = ops._empty(n, max(M, 0), 3, 3, like=x1)
    hyp_cost = ops._empty(n, max(M, 0), like=x1)
    best = torch.empty(n, dtype=torch.int32, device=x1.device)
    wo = ops._empty(n, P, like=x1) if return_weights else None
    samples = torch.empty(n, max(M, 0), 8, dtype=torch.int32, device=x1.device) if return_samples else None
    lib.rp_eight_point_consensus(_p(x1), _p(x2), _p(w), _p(tau), seed, _p(E), _p(best), _p(stat), _p(wo), _p(hyp_E), _p(hyp_cost),
                                 _p(samples), P, M, n, _st())
    return Consensus(E, best, stat, wo, hyp_E, hyp_cost, samples)


def consensus_pose_from_matches(model, images, intrinsics, heads=(0, 1, 2), hypotheses=1024, seed=0, iters=4, tau=None, refine=10,
                                subtoken=None, radius=2, minimal="eight"):
    """ViTEss.consensus_pose_from_matches: the chain of the public pieces and nothing else -- eightpoint.assemble_matches ->
    eight_point_consensus (minimal = "five": fivepoint.five_point_consensus, whose FivePointConsensus is then `consensus`) -> eightpoint.eight_point on the consensus weights (tau, iters) -> geom.pose_from_essential ->
    refine.refine_pose on the BASE weights (tau, refine) -> ConsensusMatchPose.  subtoken, radius: as for eightpoint.pose_from_matches."""
    from . import eightpoint, geom
    from . import refine as refine_
    if minimal not in ("eight", "five"):
        raise ValueError('minimal must be "eight" or "five"')
    x1, x2, w, hw = eightpoint._matches_of(model, images, intrinsics, heads, subtoken, radius)
    if tau is None:
        tau = eightpoint.default_tau(intrinsics, hw).to(x1.device).contiguous()
    if minimal == "five":
        from . import fivepoint
        c = fivepoint.five_point_consensus(x1, x2, w, tau=tau, hypotheses=hypotheses, seed=seed, return_weights=True)
    else:
        c = eight_point_consensus(x1, x2, w, tau=tau, hypotheses=hypotheses, seed=seed, return_weights=True)
    ep = eightpoint.eight_point(x1, x2, c.weights, tau=tau, iters=iters, return_weights=True)
    pose, count = geom.pose_from_essential(ep.E, x1, x2)
    r = refine_.refine_pose(pose, x1, x2, w, tau=tau, iters=refine, return_weights=True)
    return ConsensusMatchPose(r.pose, r.E, r.stat, r.weights, c, eightpoint.MatchPose(pose, ep.E, ep.stat, count, ep.weights))
