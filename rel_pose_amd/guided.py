"""Epipolar-guided matching: the Essential Matrix Module's matches read again under a pose.

readout.emm_matches takes the argmax of every row of the EMM's attention over all 576 tokens of the other image; a row whose strongest
peak is a distractor is a wrong match that every later stage can only down-weight.  rp_emm_guided_matches (include/relpose_guided.h,
csrc_guided/emm_guided.hip -- a library of its own) searches every token's partner again, only within `band` token pitches of the
epipolar line a pose assigns to it, and reports the share of the attention's mass inside that band -- a score of the pose against the
attention itself, on which any two poses can be ranked without going through hard matches:

    g = model.eval().guided_pose_from_matches(images, intrinsics, prior="consensus")     # GuidedMatchPose, all on the GPU
    s = model.pose_support(images, intrinsics, any_pose)                                 # [2B,3]: in-band mass share per image and head
    # or, piece by piece:
    gc = guided_correspondences(model, images, intrinsics, pose, band=1.5)
    x1, x2, w = eightpoint.assemble_matches(gc, intrinsics, images.shape[-2:])
    r = refine.refine_pose(pose, x1, x2, w, tau=tau, iters=10)

Guided matches lie near the prior's lines BY CONSTRUCTION: a low Sampson cost after guiding is no evidence for the pose, and a prior that
is far off confirms itself.  The evidence is the support, which is low for such a prior.  Nothing is known about a trained model's
attention: every figure in DESIGN.md is from built scenes.  The band is in token pitches per axis; with H != W the pitches differ.

grid_fundamental_from_E and the tuple helpers are plain torch and run on any device.  There is no fallback for the kernel."""
import collections
import ctypes

import torch

from . import _lib, ops, readout
from .ops import DIM, HEADS, N_TOK, _chk, _p, _st

GuidedCorrespondences = collections.namedtuple("GuidedCorrespondences", "row_idx row_stat col_idx col_stat mutual support")
GuidedCorrespondences.__doc__ = """Per image z (partner z^1) and head h, under F_z and band_z (include/relpose_guided.h):
row_idx [2B,3,576] int32   argmax over the ADMITTED columns j of row i, -1 where none    row_stat [2B,3,576,4]  (amax, bmass, mass, d2)
col_idx [2B,3,576] int32   argmax over the admitted rows i of column j                  col_stat [2B,3,576,4]  the same over i
mutual  [2B,3,576] bool    row_idx[i] >= 0 and col_idx[row_idx[i]] == i                 support  [2B,3]        sum bmass / sum mass over the rows
The first five fields are those eightpoint.assemble_matches reads of a readout.Correspondences: a row at -1 has amax 0 and is not mutual."""

GuidedMatchPose = collections.namedtuple("GuidedMatchPose", "pose E stat weights support_before support_after unmatched prior")
GuidedMatchPose.__doc__ = """pose [B,7], E [B,3,3], stat [B,4], weights [B,P] of the last refine.refine_pose (RefinedPose); support_before /
support_after [2B,3]: the in-band mass share under the prior and under `pose`; unmatched [B]: the share of the matches' owners (image 0's
tokens, the heads used) that had no admitted partner in the last round; prior [B,7]: the pose the first round was guided by"""

PRIORS = ("consensus", "regressed")


def grid_fundamental_from_E(E, intrinsics, image_hw):
    """E [B,3,3] (x2^T E x1 = 0 in normalised coordinates), intrinsics [B,2,4] = (fx, fy, cx, cy) of image 0 / image 1 in pixels of
    image_hw = (H, W) -> F [2B,9] float32 in token-grid units: with M_a the map from grid coordinates g of image a to normalised ones,
    ((g + 0.5) W / 24 - cx) / fx on x and likewise on y,  F_{2b+1} = M_1^T E M_0  and  F_{2b} its transpose, each scaled to Frobenius
    norm 1 (all zero where E is).  Formed in float64.  Plain torch, any device."""
    B = E.shape[0]
    if tuple(E.shape) != (B, 3, 3) or tuple(intrinsics.shape) != (B, 2, 4):
        raise ValueError("E must be [B,3,3] and intrinsics [B,2,4]")
    Hh, W = image_hw
    k = intrinsics.to(device=E.device, dtype=torch.float64)
    M = torch.zeros(B, 2, 3, 3, device=E.device, dtype=torch.float64)
    px, py = W / readout.GRID, Hh / readout.GRID
    M[..., 0, 0], M[..., 0, 2] = px / k[..., 0], (0.5 * px - k[..., 2]) / k[..., 0]
    M[..., 1, 1], M[..., 1, 2] = py / k[..., 1], (0.5 * py - k[..., 3]) / k[..., 1]
    M[..., 2, 2] = 1
    F1 = M[:, 1].transpose(-1, -2) @ E.to(torch.float64) @ M[:, 0]
    nrm = F1.flatten(1).norm(dim=1)
    F1 = F1 / torch.where(nrm > 0, nrm, torch.ones_like(nrm))[:, None, None]
    return torch.stack([F1.transpose(-1, -2), F1], 1).reshape(2 * B, 9).to(torch.float32).contiguous()


def grid_fundamental(pose, intrinsics, image_hw):
    """pose [B,7] = (t, q xyzw) with X2 = R X1 + t -> F [2B,9]: geom.essential_from_pose -> grid_fundamental_from_E"""
    from . import geom
    if pose.dim() != 2 or pose.shape[1] != 7:
        raise ValueError("pose must be [B,7]")
    return grid_fundamental_from_E(geom.essential_from_pose(pose.to(torch.float32).contiguous()), intrinsics, image_hw)


def _band(band, Z, device):
    if not torch.is_tensor(band):
        band = torch.full((Z,), float(band), device=device, dtype=torch.float32)
    if tuple(band.shape) != (Z,):
        raise ValueError("band must be a number or [Z]")
    return band


def emm_guided_matches(qkv, rlse, clse, F, band, Z, swap=False, single=False):
    """qkv, rlse, clse, Z, swap, single as for readout.emm_matches; F [Z,9] in token-grid units (grid_fundamental), band: float or [Z]
    token pitches -> (idx int32 [Z,3,576], -1 where no token is admitted, stat [Z,3,576,4] = (amax, bmass, mass, d2))"""
    lib = _lib.load_guided()
    if tuple(F.shape) != (Z, 9):
        raise ValueError("F must be [Z,9]")
    band = _band(band, Z, qkv.device)
    _chk(qkv, rlse, clse, F, band)
    idx = torch.empty(Z, HEADS, N_TOK, device=qkv.device, dtype=torch.int32)
    stat = ops._empty(Z, HEADS, N_TOK, 4, like=qkv)
    b, ld = qkv.data_ptr(), qkv.shape[1]
    lib.rp_emm_guided_matches(ctypes.c_void_p(b), ctypes.c_void_p(b + 4 * DIM), _p(rlse), _p(clse), _p(F), _p(band), _p(idx), _p(stat), Z, HEADS,
                              ld, ld, (DIM // HEADS) ** -0.5, 1 if swap else 0, 1 if single else 0, _st())
    return idx, stat


def mutual(row_idx, col_idx):
    """[...,576] bool: row i has a match and that column's best row is i -- readout.mutual, formed safely where an index is -1"""
    i = torch.arange(row_idx.shape[-1], device=row_idx.device).expand(row_idx.shape)
    return (row_idx >= 0) & (torch.gather(col_idx.long(), -1, row_idx.long().clamp(min=0)) == i)


def support_of(row_stat):
    """[Z,3,576,4] -> [Z,3]: sum of bmass / sum of mass over the rows (0 where there is no mass)"""
    b, m = row_stat[..., 1].sum(-1), row_stat[..., 2].sum(-1)
    return torch.where(m > 0, b / torch.where(m > 0, m, torch.ones_like(m)), torch.zeros_like(m))


def _guided(qkv, rlse, clse, Z, single, F, band):
    row_idx, row_stat = emm_guided_matches(qkv, rlse, clse, F, band, Z, swap=False, single=single)
    col_idx, col_stat = emm_guided_matches(qkv, rlse, clse, F, band, Z, swap=True, single=single)
    return GuidedCorrespondences(row_idx, row_stat, col_idx, col_stat, mutual(row_idx, col_idx), support_of(row_stat))


def _submatch(qkv, rlse, clse, Z, single, gc, radius):
    """rp_emm_submatch around the guided matches (it treats an index outside 0 .. 575 as invalid) -> readout.SubtokenCorrespondences"""
    row_win, row_quad = readout.emm_submatch(qkv, rlse, clse, gc.row_idx, Z, swap=False, single=single, radius=radius)
    col_win, col_quad = readout.emm_submatch(qkv, rlse, clse, gc.col_idx, Z, swap=True, single=single, radius=radius)
    return readout.SubtokenCorrespondences(gc, row_win, row_quad, col_win, col_quad)


def _scores(model, images):
    if model.training:          # (before the CNN runs: its BatchNorm layers would update their running statistics)
        raise RuntimeError("correspondences are read out of a model in eval() mode")
    with torch.no_grad():
        fmap, _ = model.cnn_map(images)
        return readout._scores_from_map(model, fmap)


def _pose_arg(pose, B, device):
    if not torch.is_tensor(pose) or tuple(pose.shape) != (B, 7):
        raise ValueError("pose must be [B,7] with B = %d pairs" % B)
    return pose.to(device=device, dtype=torch.float32).contiguous()


def guided_correspondences(model, images, intrinsics, pose, band=1.5):
    """ViTEss.guided_correspondences: images [B,2,3,H,W], intrinsics [B,2,4] in pixels of (H, W), pose [B,7] -> GuidedCorrespondences:
    the model's own path up to the EMM's scores (readout), grid_fundamental of the pose, two rp_emm_guided_matches (rows, columns)."""
    qkv, rlse, clse, Z, single = _scores(model, images)
    hw = tuple(int(s) for s in images.shape[-2:])
    with torch.no_grad():
        F = grid_fundamental(_pose_arg(pose, Z // 2, qkv.device), intrinsics, hw)
        return _guided(qkv, rlse, clse, Z, single, F, band)


def pose_support(model, images, intrinsics, pose, band=1.5):
    """ViTEss.pose_support: [2B,3], the share of the attention's mass within `band` of the pose's epipolar lines, per image and head --
    guided_correspondences(...).support"""
    return guided_correspondences(model, images, intrinsics, pose, band).support


def guided_pose_from_matches(model, images, intrinsics, prior="consensus", band=1.5, rounds=1, iters=10, heads=(0, 1, 2), tau=None,
                             subtoken=None, radius=2):
    """ViTEss.guided_pose_from_matches: prior -> guided correspondences -> eightpoint.assemble_matches -> refine.refine_pose FROM the
    prior, `rounds` times with the refined pose as the next prior -> GuidedMatchPose.  prior: "consensus"
    (model.consensus_pose_from_matches with the same heads, tau, subtoken, radius), "regressed" (the network's own pose) or a pose [B,7].
    subtoken = "window" / "quadratic": rp_emm_submatch around the guided matches localises x2 (pass a smaller tau then)."""
    from . import eightpoint, refine
    if subtoken is not None and subtoken not in eightpoint.SUBTOKEN:
        raise ValueError("subtoken must be None or one of %s" % (eightpoint.SUBTOKEN,))
    if rounds < 1:
        raise ValueError("rounds must be >= 1")
    if isinstance(prior, str) and prior not in PRIORS:
        raise ValueError("prior must be a pose [B,7] or one of %s" % (PRIORS,))
    qkv, rlse, clse, Z, single = _scores(model, images)
    hw = tuple(int(s) for s in images.shape[-2:])
    if isinstance(prior, str) and prior == "consensus":
        prior = model.consensus_pose_from_matches(images, intrinsics, heads=heads, tau=tau, subtoken=subtoken, radius=radius).pose
    elif isinstance(prior, str):
        Gs = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=images.device).repeat(images.shape[0], 2, 1)
        with torch.no_grad():
            prior = model(images, Gs, intrinsics=intrinsics.clone())[0].data[:, 1]      # (forward rescales its intrinsics in place)
    prior = _pose_arg(prior, Z // 2, qkv.device)
    if tau is None:
        tau = eightpoint.default_tau(intrinsics, hw).to(qkv.device).contiguous()
    pose, before = prior, None
    with torch.no_grad():
        for _ in range(rounds):
            gc = _guided(qkv, rlse, clse, Z, single, grid_fundamental(pose, intrinsics, hw), band)
            sub = None if subtoken is None else _submatch(qkv, rlse, clse, Z, single, gc, radius)
            x1, x2, w = eightpoint.assemble_matches(gc, intrinsics, hw, heads, sub=sub, subtoken=subtoken or "window")
            r = refine.refine_pose(pose, x1, x2, w, tau=tau, iters=iters, return_weights=True)
            before = gc.support if before is None else before
            unmatched = (gc.row_idx[1::2][:, list(heads)] < 0).flatten(1).float().mean(1)
            pose = r.pose
        after = support_of(emm_guided_matches(qkv, rlse, clse, grid_fundamental(pose, intrinsics, hw), band, Z, swap=False, single=single)[1])
    return GuidedMatchPose(r.pose, r.E, r.stat, r.weights, before, after, unmatched, prior)
