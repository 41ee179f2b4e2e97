"""Which two-view model do the matches support -- the essential matrix, the plane-induced homography or the pure rotation -- decided on
the GPU by an information criterion.

Every essential-matrix chain fails on a plane, every chain returns a meaningless translation on a rotating pair, and the planar chain
spends eight parameters on a rotation.  include/relpose_select.h (csrc_select/select.hip -- a library of its own) puts the candidates the
three chains return on one scale: the Sampson residual of every match under every candidate, a noise scale estimated
from the residuals themselves, and per candidate the cost of coding each match as an inlier of the model or, at a price that is the same
under every model, as an outlier:

    ap = model.eval().auto_pose_from_matches(images, intrinsics)
    ap.kind                                       # per pair: 0 essential, 1 homography, 2 rotation, -1 none
    ap.pose                                       # the pose of the chosen model
    # or, piece by piece (x1, x2, w, tau as in rel_pose_amd/eightpoint.py; models [n,C,3,3], kinds a list of C ints):
    s = model_select(x1, x2, w, models, kinds, tau=tau)
    s.pick, s.stat[..., 0]                        # the chosen candidate, the criterion of each

There is no fallback for the kernel."""
import collections
import ctypes

import torch

from . import _lib, ops
from .homography import _rows
from .ops import _chk, _p, _st

ESSENTIAL, HOMOGRAPHY, ROTATION = 0, 1, 2
KIND_NAMES = ("essential", "homography", "rotation")
# the candidates of auto_pose_from_matches, in their fixed order
AUTO_KINDS = (ESSENTIAL, ESSENTIAL, ESSENTIAL, HOMOGRAPHY, ROTATION)
AUTO_NAMES = ("E of the consensus chain", "E of planar pick 0", "E of planar pick 1", "H", "R")

Selection = collections.namedtuple("Selection", "pick stat scale residuals labels")
Selection.__doc__ = """pick [n] int32 the chosen candidate (-1: degenerate), stat [n,C,4] = (the criterion G_c, the number of inliers, the
inlier gate on e^2, the number of rows inside the tau band) -- (FLT_MAX, 0, 0, 0) for an invalid candidate and for a degenerate problem
--, scale [n,2] = (the noise scale sigma, the candidate that supplied it or -1 if it was given), residuals [n,C,P] e^2 of every row, or
None, labels [n,P] int32 with bit c set where the row is an inlier of candidate c, or None"""
AutoMatchPose = collections.namedtuple("AutoMatchPose", "pose kind selection consensus planar rotation")
AutoMatchPose.__doc__ = """pose [n,7] the pose of the chosen model (all zero where nothing was chosen), kind [n] int32 its kind: 0
essential, 1 homography, 2 rotation, -1 none; selection the Selection over the five candidates of AUTO_NAMES (with labels), consensus,
planar, rotation: the consensus.ConsensusMatchPose, homography.PlanarMatchPose and rotation.RotationMatchPose of the three chains"""


def model_select(x1, x2, w, models, kinds, tau=0.01, sigma=None, outlier_cost=8.0, return_residuals=False, return_labels=False):
    """x1, x2 [n,P,2] calibrated image coordinates, w [n,P] (None: ones; only its sign is used), models [n,C,3,3] the candidates, kinds:
    C ints of {0 essential, 1 homography, 2 rotation}, tau: float or [n], the band of the scale estimate, sigma: None (estimated), a
    float or [n] (an entry > 0 is used as given), outlier_cost: the cost of coding a match as an outlier -> Selection.
    8 <= P <= 1728, C <= 8."""
    n, P, tau = _rows(x1, x2, w, tau)
    kinds = [int(k) for k in kinds]
    C = len(kinds)
    if models.dim() != 4 or tuple(models.shape) != (n, C, 3, 3):
        raise ValueError("models must be [n,C,3,3] with one kind per candidate")
    if sigma is not None and not torch.is_tensor(sigma):
        sigma = torch.full((n,), float(sigma), device=x1.device, dtype=torch.float32)
    if sigma is not None and tuple(sigma.shape) != (n,):
        raise ValueError("sigma must be None, a number or [n]")
    lib = _lib.load_select()
    _chk(x1, x2, w, tau, sigma, models)
    pick = torch.empty(n, dtype=torch.int32, device=x1.device)
    stat = ops._empty(n, C, 4, like=x1)
    scale = ops._empty(n, 2, like=x1)
    resid = ops._empty(n, C, P, like=x1) if return_residuals else None
    label = torch.empty(n, P, dtype=torch.int32, device=x1.device) if return_labels else None
    host_kinds = (ctypes.c_int * max(C, 1))(*kinds)
    lib.rp_model_select(_p(x1), _p(x2), _p(w), _p(tau), _p(sigma), _p(models), ctypes.cast(host_kinds, ctypes.c_void_p), float(outlier_cost),
                        _p(pick), _p(stat), _p(scale), _p(resid), _p(label), P, C, n, _st())
    return Selection(pick, stat, scale, resid, label)


def auto_pose_from_matches(model, images, intrinsics, heads=(0, 1, 2), hypotheses=(1024, 256, 256), seed=0, refine=10, tau=None, sigma=None,
                           subtoken=None, radius=2, minimal="eight"):
    """ViTEss.auto_pose_from_matches: the chain of the public pieces and nothing else.  eightpoint.assemble_matches, once; on those
    matches the three chains as consensus.consensus_pose_from_matches (iters = 4; minimal as there), homography.planar_pose_from_matches
    (vis_min = 0.99, no prior) and rotation.rotation_from_matches run them -- hypotheses: one number for all three, or (consensus,
    planar, rotation) --; five candidates in the order of AUTO_NAMES: the E of the refined consensus pose, the E of planar picks 0 and 1
    after `refine` iterations of refine.refine_pose on the base weights (a zero matrix, hence invalid, where the pick is -1 or the planar
    chain's case is "pure rotation"), H and R; model_select (sigma as there); the chosen pose gathered on the device -- for an E
    candidate its refined pose, for H the planar chain's first pick, for R (0, 0, 0, q) -> AutoMatchPose."""
    from . import consensus, eightpoint, geom, homography, rotation
    from . import refine as refine_
    if minimal not in ("eight", "five"):
        raise ValueError('minimal must be "eight" or "five"')
    hyp = tuple(int(h) for h in hypotheses) if isinstance(hypotheses, (tuple, list)) else (int(hypotheses),) * 3
    if len(hyp) != 3:
        raise ValueError("hypotheses must be one number or (consensus, planar, rotation)")
    x1, x2, w, hw = eightpoint._matches_of(model, images, intrinsics, heads, subtoken, radius)
    if tau is None:
        tau = eightpoint.default_tau(intrinsics, hw).to(x1.device).contiguous()
    # ---- the consensus chain
    if minimal == "five":
        from . import fivepoint
        cc = fivepoint.five_point_consensus(x1, x2, w, tau=tau, hypotheses=hyp[0], seed=seed, return_weights=True)
    else:
        cc = consensus.eight_point_consensus(x1, x2, w, tau=tau, hypotheses=hyp[0], seed=seed, return_weights=True)
    ep = eightpoint.eight_point(x1, x2, cc.weights, tau=tau, iters=4, return_weights=True)
    pose0, count = geom.pose_from_essential(ep.E, x1, x2)
    cr = refine_.refine_pose(pose0, x1, x2, w, tau=tau, iters=refine, return_weights=True)
    cons = consensus.ConsensusMatchPose(cr.pose, cr.E, cr.stat, cr.weights, cc, eightpoint.MatchPose(pose0, ep.E, ep.stat, count, ep.weights))
    # ---- the planar chain
    hc = homography.homography_consensus(x1, x2, w, tau=tau, hypotheses=hyp[1], seed=seed)
    hr = homography.homography_refine(x1, x2, w, hc.H, tau=tau, iters=refine)
    hd = homography.pose_from_homography(hr.H, x1, x2, w, tau=tau, vis_min=0.99)
    hpick, ambiguous = homography.order_by_prior(hd, 0.99, None)
    rows = torch.arange(x1.shape[0], device=x1.device)
    first = hpick[:, 0].long()
    planar = homography.PlanarMatchPose(hd.pose[rows, first.clamp(min=0)] * (first >= 0).to(hd.pose.dtype)[:, None], hr.H, hr.stat, hd, hpick,
                                        ambiguous, None, hc)
    # ---- the rotation chain
    rc = rotation.rotation_consensus(x1, x2, w, tau=tau, hypotheses=hyp[2], seed=seed)
    rr = rotation.rotation_refine(x1, x2, w, rc.R, tau=tau, iters=refine)
    rot = rotation.RotationMatchPose(rr.pose, rr.R, rr.stat, rc)
    # ---- the five candidates
    cand_E, cand_pose = [cr.E], [cr.pose]
    for k in range(2):
        idx = hpick[:, k].long()
        live = (idx >= 0) & (hd.cstat[rows, idx.clamp(min=0), 2] > 0)           # |t| / d = 0 on a valid candidate: the "pure rotation" case
        start = (hd.pose[rows, idx.clamp(min=0)] * live.to(hd.pose.dtype)[:, None]).contiguous()
        pr = refine_.refine_pose(start, x1, x2, w, tau=tau, iters=refine)
        cand_E.append(pr.E * live.to(pr.E.dtype)[:, None, None])
        cand_pose.append(pr.pose * live.to(pr.pose.dtype)[:, None])
    models = torch.stack(cand_E + [hr.H, rr.R], 1).contiguous()
    sel = model_select(x1, x2, w, models, AUTO_KINDS, tau=tau, sigma=sigma, return_labels=True)
    # ---- the chosen pose, gathered on the device
    poses = torch.stack(cand_pose + [planar.pose, rr.pose], 1)
    pick = sel.pick.long()
    chosen = pick >= 0
    pose = poses[rows, pick.clamp(min=0)] * chosen.to(poses.dtype)[:, None]
    kind = torch.where(chosen, torch.tensor(AUTO_KINDS, dtype=torch.int32, device=x1.device)[pick.clamp(min=0)],
                       torch.full_like(sel.pick, -1))
    return AutoMatchPose(pose, kind, sel, cons, planar, rot)
