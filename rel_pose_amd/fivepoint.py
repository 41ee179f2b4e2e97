"""Calibrated five-point consensus: the consensus of rel_pose_amd/consensus.py with a five-point minimal solver, on the GPU.

eight_point_consensus draws eight matches per hypothesis; with 60 % of outliers a sample is clean once in 1400 draws and 1024 hypotheses
hold none.  The intrinsics are known here, so five matches determine the essential matrix up to ten solutions.
rp_five_point_consensus (include/relpose_fivepoint.h, csrc_fivepoint/five_point.hip -- a library of its own) draws `hypotheses` samples
of five with the same counter-based sampler, solves each in fp64, scores every solution against all matches with the robust cost
refine_pose reports, and returns the best together with the Cauchy weights at it:

    cp = model.eval().consensus_pose_from_matches(images, intrinsics, minimal="five")
    # or, piece by piece (x1, x2, w, tau as in rel_pose_amd/eightpoint.py):
    c = five_point_consensus(x1, x2, w, tau=tau, hypotheses=1024, seed=0, return_weights=True)
    ep = eight_point(x1, x2, c.weights, tau=tau, iters=4)

The same seed gives the same samples and the same bits.  There is no fallback for the kernels."""
import collections

import torch

from . import _lib, ops
from .ops import _chk, _p, _st

FivePointConsensus = collections.namedtuple("FivePointConsensus", "E best stat weights hyp_E hyp_cost samples")
FivePointConsensus.__doc__ = """E [n,3,3] the best root (all zero for a degenerate problem), best [n,2] int32 its (sample, slot) ((-1, -1):
degenerate), stat [n,4] = (its cost, the inlier weight share at it, the number of valid slots, the number of rows of positive weight),
weights [n,P] the Cauchy weights w / (1 + sampson / tau^2) at E, or None, hyp_E [n,M,10,3,3] and hyp_cost [n,M,10] every sample's ten slots
(an invalid one: zeros and FLT_MAX; the valid ones come first, in ascending z), samples [n,M,5] int32 the sampled rows, or None"""


def five_point_consensus(x1, x2, w=None, tau=0.01, hypotheses=1024, seed=0, return_weights=False, return_samples=False):
    """x1, x2 [n,P,2] calibrated image coordinates (X2 = R X1 + t), w [n,P] base weights (None: ones), tau: float or [n], the scale of
    the robust cost mean(w tau^2 log1p(sampson / tau^2)), `hypotheses` samples of five per problem drawn from `seed` -> FivePointConsensus.
    5 <= P <= 1728, hypotheses <= 4096."""
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
    lib = _lib.load_fivepoint()
    _chk(x1, x2, w, tau)
    R = _lib.FIVEPOINT_ROOTS
    E = ops._empty(n, 3, 3, like=x1)
    stat = ops._empty(n, 4, like=x1)
    hyp_E = ops._empty(n, max(M, 0), R, 3, 3, like=x1)
    hyp_cost = ops._empty(n, max(M, 0), R, like=x1)
    best = torch.empty(n, 2, dtype=torch.int32, device=x1.device)
    wo = ops._empty(n, P, like=x1) if return_weights else None
    samples = torch.empty(n, max(M, 0), 5, dtype=torch.int32, device=x1.device) if return_samples else None
    lib.rp_five_point_consensus(_p(x1), _p(x2), _p(w), _p(tau), seed, _p(E), _p(best), _p(stat), _p(wo), _p(hyp_E), _p(hyp_cost),
                                _p(samples), P, M, n, _st())
    return FivePointConsensus(E, best, stat, wo, hyp_E, hyp_cost, samples)
