"""The classical eight-point algorithm on the GPU, next to the network that learns it implicitly.

rp_eight_point (include/relpose_eightpoint.h, csrc_eightpoint/eight_point.hip -- a library of its own) turns weighted correspondences
into essential matrices: weighted Hartley normalisation, the null vector of the row matrix by a one-sided Jacobi iteration, projection
onto the essential manifold, and rounds of Cauchy re-weighting on the Sampson distance -- one launch, one workgroup per problem.
It closes the chain  images -> correspondences -> E -> (R, t)  on the device:

    mp = model.eval().pose_from_matches(images, intrinsics)            # MatchPose, all on the GPU
    # or, piece by piece:
    corr = model.correspondences(images)
    x1, x2, w = assemble_matches(corr, intrinsics, images.shape[-2:])
    ep = eight_point(x1, x2, w, tau=0.01, iters=4)
    pose, count = geom.pose_from_essential(ep.E, x1, x2)

assemble_matches is plain torch and runs on any device.  There is no fallback for the kernel."""
import collections

import torch

from . import _lib, geom, ops, readout
from .ops import _chk, _p, _st

EightPoint = collections.namedtuple("EightPoint", "E stat weights")
EightPoint.__doc__ = """E [n,3,3] (singular values 1, 1, 0; x2^T E x1 = 0; the entry of largest magnitude positive; all zero for a
degenerate problem), stat [n,4] = (sigma_9 / sigma_1, sigma_8 / sigma_1 of the weighted row matrix, e2 / e1 of F before the projection,
sum of the weights) of the last solve, weights [n,P] the last solve used, or None"""

MatchPose = collections.namedtuple("MatchPose", "pose E stat count weights")
MatchPose.__doc__ = """pose [B,7] = (t unit, q xyzw with w >= 0) of camera 2 against camera 1 (X2 = R X1 + t), E [B,3,3] and stat [B,4]
as in EightPoint, count [B] int32 the matches in front of both cameras, weights [B,P] the final robust weights of the matches"""


def eight_point(x1, x2, w=None, tau=None, iters=0, return_weights=False):
    """x1, x2 [n,P,2] normalised image coordinates (X2 = R X1 + t), w [n,P] base weights (None: ones), tau: float or [n], the scale
    of the Cauchy weight w / (1 + sampson / tau^2) of the `iters` re-weighting rounds -> EightPoint.  8 <= P <= 1728, iters <= 16."""
    lib = _lib.load_eightpoint()
    if x1.dim() != 3 or x1.shape[-1] != 2 or x1.shape != x2.shape:
        raise ValueError("x1 and x2 must have the same shape [n,P,2]")
    n, P = x1.shape[:2]
    if w is not None and tuple(w.shape) != (n, P):
        raise ValueError("w must be [n,P]")
    if tau is not None and not torch.is_tensor(tau):
        tau = torch.full((n,), float(tau), device=x1.device, dtype=torch.float32)
    if tau is not None and tuple(tau.shape) != (n,):
        raise ValueError("tau must be a number or [n]")
    if tau is None and iters > 0:
        raise ValueError("re-weighting (iters > 0) needs tau")
    _chk(x1, x2, w, tau)
    E = ops._empty(n, 3, 3, like=x1)
    stat = ops._empty(n, 4, like=x1)
    wo = ops._empty(n, P, like=x1) if return_weights else None
    lib.rp_eight_point(_p(x1), _p(x2), _p(w), _p(tau), _p(E), _p(stat), _p(wo), P, int(iters), n, _st())
    return EightPoint(E, stat, wo)


SUBTOKEN = ("window", "quadratic")


def assemble_matches(corr, intrinsics, image_hw, heads=(0, 1, 2), sub=None, subtoken="window"):
    """readout.Correspondences -> (x1 [B,576 len(heads),2], x2 the same, w [B,576 len(heads)]) for eight_point, head after head.
    For pair b the matches are those of image z = 2b + 1's attention (readout.matches_xy): x1 the normalised centres of all 576 tokens
    of image 0, x2 those of their partners row_idx[z,h] in image 1, w = (A at the match) x (the match is mutual) -- fixed shapes, a
    non-mutual row has weight 0.  intrinsics [B,2,4] = (fx, fy, cx, cy) of image 0 / image 1 in pixels of image_hw = (H, W); it is
    only read.  sub: a readout.SubtokenCorrespondences of the same images -- x2 is then the localised position of the match,
    sub.row_win ("window") or sub.row_quad ("quadratic"), instead of the partner's centre; x1 and w are what they are without it."""
    if sub is not None and subtoken not in SUBTOKEN:
        raise ValueError("subtoken must be one of %s" % (SUBTOKEN,))
    B = corr.row_idx.shape[0] // 2
    if tuple(intrinsics.shape) != (B, 2, 4):
        raise ValueError("intrinsics must be [B,2,4] with B = %d pairs" % B)
    dev, dt = corr.row_stat.device, corr.row_stat.dtype
    c = readout.token_centres(image_hw, device=dev, dtype=dt)                       # [576,2]
    heads = list(heads)
    idx = corr.row_idx[1::2][:, heads].long()                                       # [B,h,576]
    xy1 = c.expand(B, len(heads), *c.shape)
    if sub is None:
        xy2 = c[idx]                                                                # [B,h,576,2]
    else:
        xy2 = readout.subtoken_xy((sub.row_win if subtoken == "window" else sub.row_quad)[1::2][:, heads], image_hw).to(dt)
    # readout.normalised slices its intrinsics row along the FIRST axis: coordinates first, [2,B,h,576] against [4,B,1,1]
    k = intrinsics.to(device=dev, dtype=dt).permute(2, 1, 0)[..., None, None]       # [4,2,B,1,1]
    x1 = readout.normalised(xy1.permute(3, 0, 1, 2), k[:, 0]).permute(1, 2, 3, 0)
    x2 = readout.normalised(xy2.permute(3, 0, 1, 2), k[:, 1]).permute(1, 2, 3, 0)
    w = corr.row_stat[1::2][:, heads][..., 0] * corr.mutual[1::2][:, heads].to(dt)
    P = len(heads) * c.shape[0]
    return x1.reshape(B, P, 2).contiguous(), x2.reshape(B, P, 2).contiguous(), w.reshape(B, P).contiguous()


def default_tau(intrinsics, image_hw):
    """[B]: half a token pitch of image 0 in normalised units, 0.5 (W / 24) / fx -- the matches are token centres, so that is their
    quantisation scale.  With sub-token matches (assemble_matches(sub=...)) the caller should pass a smaller tau; how much smaller is
    not known for a trained model."""
    return (0.5 * image_hw[1] / readout.GRID) / intrinsics[:, 0, 0].to(torch.float32)


def _matches_of(model, images, intrinsics, heads, subtoken, radius):
    """(x1, x2, w, hw) of the pose chains: model.correspondences, or with `subtoken` model.subtoken_correspondences, -> assemble_matches"""
    hw = tuple(int(s) for s in images.shape[-2:])
    if subtoken is None:
        return assemble_matches(model.correspondences(images), intrinsics, hw, heads) + (hw,)
    if subtoken not in SUBTOKEN:
        raise ValueError("subtoken must be None or one of %s" % (SUBTOKEN,))
    sub = model.subtoken_correspondences(images, radius)
    return assemble_matches(sub.corr, intrinsics, hw, heads, sub=sub, subtoken=subtoken) + (hw,)


def pose_from_matches(model, images, intrinsics, heads=(0, 1, 2), iters=4, tau=None, subtoken=None, radius=2):
    """ViTEss.pose_from_matches: images [B,2,3,H,W], intrinsics [B,2,4] in pixels of (H, W) -> MatchPose.  The chain of the public
    pieces: model.correspondences -> assemble_matches -> eight_point -> geom.pose_from_essential; with subtoken = "window" /
    "quadratic": model.subtoken_correspondences(images, radius) -> assemble_matches(sub.corr, ..., sub=sub, subtoken=subtoken) -> the same."""
    x1, x2, w, hw = _matches_of(model, images, intrinsics, heads, subtoken, radius)
    if tau is None:
        tau = default_tau(intrinsics, hw).to(x1.device).contiguous()
    ep = eight_point(x1, x2, w, tau=tau, iters=iters, return_weights=True)
    pose, count = geom.pose_from_essential(ep.E, x1, x2)
    return MatchPose(pose, ep.E, ep.stat, count, ep.weights)
