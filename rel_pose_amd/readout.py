"""Readout of the Essential Matrix Module: which token of one image the module paired with which token of the other.

The EMM's dual-softmax attention A_z = softmax_rows(S_z) * softmax_cols(S_z), S_z = scale q_{z^1} k_z^T (rows: tokens of the partner
image z^1, columns: tokens of image z), is never in memory on the model's path (include/relpose_hip.h: rp_emm_stats, rp_emm_apply).
rp_emm_matches (include/relpose_readout.h, csrc_readout/emm_readout.hip -- a library of its own) reads it out per row and per column:
argmax, its weight, the total mass and a soft-argmax position on the 24 x 24 token grid, optionally the dense matrix.
rp_emm_submatch (include/relpose_submatch.h, csrc_submatch/submatch.hip -- again a library of its own) localises each match between the
token centres: model.subtoken_correspondences(images).

    corr = model.eval().correspondences(images)                      # Correspondences, all on the GPU
    x1, x2, conf = matches_xy(corr, 1, h, images.shape[-2:])         # pixel centres in image 0 / image 1 of pair 0
    pose, count = geom.pose_from_essential(E, normalised(x1, K)[None], normalised(x2, K)[None])

The helpers below the kernel wrapper are plain torch and run on any device and dtype.  There is no fallback for the kernel."""
import collections
import ctypes

import torch

from . import _lib, ops
from .ops import DIM, HEADS, N_TOK, _chk, _p, _st

GRID = 24      # tokens per row / column of the feature map (src/model.py:19-23)

Correspondences = collections.namedtuple("Correspondences", "row_idx row_stat col_idx col_stat mutual attention")
Correspondences.__doc__ = """Per image z (partner z^1) and head h, of M_z = A_z [576 rows i: tokens of image z^1, 576 columns j: tokens of image z]:
row_idx [2B,3,576] int32    argmax_j of row i            row_stat [2B,3,576,4]  (A at the argmax, sum_j A, soft-argmax column, row of j)
col_idx [2B,3,576] int32    argmax_i of column j         col_stat [2B,3,576,4]  the same over i
mutual  [2B,3,576] bool     col_idx[row_idx[i]] == i     attention [2B,3,576,576] or None"""


def emm_matches(qkv, rlse, clse, Z, swap=False, single=False, dense=False):
    """qkv [Z*576, >= 384] (q | k packed as the model's qkv Linear writes them), rlse / clse [Z,3,576] from ops.emm_stats ->
    (idx int32 [Z,3,576], stat [Z,3,576,4] = (amax, mass, ex, ey), A [Z,3,576,576] or None).
    swap=False: per row i of A_z over the columns j; swap=True: per column j over the rows i."""
    lib = _lib.load_readout()
    _chk(qkv, rlse, clse)
    idx = torch.empty(Z, HEADS, N_TOK, device=qkv.device, dtype=torch.int32)
    stat = ops._empty(Z, HEADS, N_TOK, 4, like=qkv)
    a = ops._empty(Z, HEADS, N_TOK, N_TOK, like=qkv) if dense else None
    b, ld = qkv.data_ptr(), qkv.shape[1]
    lib.rp_emm_matches(ctypes.c_void_p(b), ctypes.c_void_p(b + 4 * DIM), _p(rlse), _p(clse), _p(idx), _p(stat), _p(a), Z, HEADS, ld, ld,
                       (DIM // HEADS) ** -0.5, 1 if swap else 0, 1 if single else 0, _st())
    return idx, stat, a


SubtokenCorrespondences = collections.namedtuple("SubtokenCorrespondences", "corr row_win row_quad col_win col_quad")
SubtokenCorrespondences.__doc__ = """corr: the Correspondences; around corr.row_idx / corr.col_idx, per image z, head h and owner token (include/relpose_submatch.h):
row_win / col_win [2B,3,576,4]    (wx, wy, wmass, wvar): soft-argmax position over the window in token-grid units, its mass, its spread
row_quad / col_quad [2B,3,576,4]  (px, py, cx, cy): vertex of the parabola through the argmax and its neighbours per axis, the curvatures"""


def emm_submatch(qkv, rlse, clse, idx, Z, swap=False, single=False, radius=2):
    """qkv, rlse, clse as for emm_matches, idx int32 [Z,3,576] the window centres (emm_matches' idx) -> (win [Z,3,576,4] = (wx, wy, wmass,
    wvar), quad [Z,3,576,4] = (px, py, cx, cy)): where between the token centres the match lies, positions in token-grid units.
    An idx outside 0 .. 575 gives (-1, -1, 0, 0) in both."""
    lib = _lib.load_submatch()
    if idx.dtype != torch.int32 or tuple(idx.shape) != (Z, HEADS, N_TOK):
        raise ValueError("idx must be int32 [Z,%d,%d]" % (HEADS, N_TOK))
    _chk(qkv, rlse, clse)
    if not (idx.is_cuda and idx.is_contiguous()):
        raise RuntimeError("rel_pose_amd ops need contiguous GPU tensors (no CPU fallback exists); got idx on %s contiguous=%s"
                           % (idx.device, idx.is_contiguous()))
    win = ops._empty(Z, HEADS, N_TOK, 4, like=qkv)
    quad = ops._empty(Z, HEADS, N_TOK, 4, like=qkv)
    b, ld = qkv.data_ptr(), qkv.shape[1]
    lib.rp_emm_submatch(ctypes.c_void_p(b), ctypes.c_void_p(b + 4 * DIM), _p(rlse), _p(clse), _p(idx), _p(win), _p(quad), Z, HEADS, ld, ld,
                        (DIM // HEADS) ** -0.5, 1 if swap else 0, 1 if single else 0, int(radius), _st())
    return win, quad


def mutual(row_idx, col_idx):
    """[...,576] bool: row i's best column names row i as its own best row"""
    i = torch.arange(row_idx.shape[-1], device=row_idx.device).expand(row_idx.shape)
    return torch.gather(col_idx.long(), -1, row_idx.long()) == i


def _scores_from_map(model, fmap):
    """the shared prefix of the readouts: CNN map [2B,192,24,24] -> (qkv [2B*576, 576], rlse, clse [2B,3,576], Z, single) of the last block"""
    if model.training:
        raise RuntimeError("correspondences are read out of a model in eval() mode")
    if model.noess:
        raise ValueError("a noess model has no Essential Matrix Module to read correspondences from")
    if ops.GEMM_PRECISION == 1 or ops.ATTN_BF16 or ops.CNN_PRECISION == 1:
        raise NotImplementedError("the readout runs on the exact-fp32 path only (the bf16 configuration is set)")
    ft = model.fusion_transformer
    if fmap.dtype != torch.float32:
        fmap = fmap.float()
    x = ops.TokensFn.apply(fmap, ft.pos_embed[0])
    for layer in range(model.transformer_depth - 1):
        x = ft.blocks[layer](x)
    blk = ft.blocks[model.transformer_depth - 1]
    a = blk.cross_attn
    Z = x.shape[0]
    qkv = ops.ln_linear(x.contiguous().view(Z * N_TOK, DIM), blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.qkv.bias, train=False)[0]
    single = bool(a.use_single_softmax)
    rlse, clse = ops.emm_stats(qkv, Z, single)
    return qkv, rlse, clse, Z, single


def _matches(qkv, rlse, clse, Z, single, dense):
    row_idx, row_stat, att = emm_matches(qkv, rlse, clse, Z, swap=False, single=single, dense=dense)
    col_idx, col_stat, _ = emm_matches(qkv, rlse, clse, Z, swap=True, single=single)
    return Correspondences(row_idx, row_stat, col_idx, col_stat, mutual(row_idx, col_idx), att)


def correspondences_from_map(model, fmap, dense=False):
    """ViTEss.correspondences_from_map: CNN map [2B,192,24,24] -> Correspondences.  The model's own inference path up to the EMM's
    scores -- tokens, the first depth-1 blocks, the last block's LayerNorm + qkv Linear, rp_emm_stats -- then two rp_emm_matches
    (rows, columns).  No intrinsics: positional features enter V only."""
    with torch.no_grad():
        qkv, rlse, clse, Z, single = _scores_from_map(model, fmap)
        return _matches(qkv, rlse, clse, Z, single, dense)


def subtoken_correspondences_from_map(model, fmap, radius=2):
    """ViTEss.subtoken_correspondences_from_map: correspondences_from_map and, on the same scores, two rp_emm_submatch around its row
    and column matches -> SubtokenCorrespondences"""
    with torch.no_grad():
        qkv, rlse, clse, Z, single = _scores_from_map(model, fmap)
        corr = _matches(qkv, rlse, clse, Z, single, False)
        row_win, row_quad = emm_submatch(qkv, rlse, clse, corr.row_idx, Z, swap=False, single=single, radius=radius)
        col_win, col_quad = emm_submatch(qkv, rlse, clse, corr.col_idx, Z, swap=True, single=single, radius=radius)
        return SubtokenCorrespondences(corr, row_win, row_quad, col_win, col_quad)


def correspondences(model, images, dense=False):
    """ViTEss.correspondences: images [B,2,3,H,W] fp32 BGR 0..255 -> Correspondences"""
    if model.training:          # (before the CNN runs: its BatchNorm layers would update their running statistics)
        raise RuntimeError("correspondences are read out of a model in eval() mode")
    with torch.no_grad():
        fmap, _ = model.cnn_map(images)
    return correspondences_from_map(model, fmap, dense)


def subtoken_correspondences(model, images, radius=2):
    """ViTEss.subtoken_correspondences: images [B,2,3,H,W] fp32 BGR 0..255 -> SubtokenCorrespondences"""
    if model.training:
        raise RuntimeError("correspondences are read out of a model in eval() mode")
    with torch.no_grad():
        fmap, _ = model.cnn_map(images)
    return subtoken_correspondences_from_map(model, fmap, radius)


# ------------------------------------------------------------------------------------------------ plain torch
def subtoken_xy(win_or_quad, image_hw):
    """[...,>=2] positions in token-grid units (the first two columns of a win or quad) -> [...,2] pixels (x, y) of an image of (H, W)
    pixels: (p + 0.5) (W / 24) on x, (p + 0.5) (H / 24) on y -- token_centres at the integers"""
    H, W = image_hw
    p = win_or_quad[..., :2]
    return torch.stack([(p[..., 0] + 0.5) * (W / GRID), (p[..., 1] + 0.5) * (H / GRID)], -1)


def token_centres(image_hw, device=None, dtype=torch.float32):
    """[576,2] pixel centres (x, y) of the tokens in an image of (H, W) pixels: token n sits at column n % 24, row n / 24"""
    H, W = image_hw
    n = torch.arange(GRID * GRID, device=device)
    x = ((n % GRID).to(dtype) + 0.5) * (W / GRID)
    y = (torch.div(n, GRID, rounding_mode="floor").to(dtype) + 0.5) * (H / GRID)
    return torch.stack([x, y], -1)


def matches_xy(corr, z, h, image_hw, mutual_only=True):
    """Hard matches of M_z, head h: (xy [M,2] in image z^1, xy [M,2] in image z, confidence [M] = A at the match), in pixels.
    Row i of M_z is token i of image z^1, its match the token row_idx[z,h,i] of image z.  With z odd the first array lies in the
    pair's image 0 and the second in its image 1: (x1, x2) of geom.pose_from_essential once normalised."""
    idx = corr.row_idx[z, h].long()
    c = token_centres(image_hw, device=idx.device, dtype=corr.row_stat.dtype)
    keep = corr.mutual[z, h] if mutual_only else torch.ones_like(idx, dtype=torch.bool)
    return c[keep], c[idx[keep]], corr.row_stat[z, h, :, 0][keep]


def normalised(xy, intrinsics_row):
    """pixels [...,2] -> normalised image coordinates with intrinsics_row = (fx, fy, cx, cy) in the same pixels"""
    k = torch.as_tensor(intrinsics_row, dtype=xy.dtype, device=xy.device)
    return (xy - k[2:4]) / k[0:2]


def sampson_distance(E, x1, x2):
    """First-order geometric error of correspondences x1 <-> x2 [...,P,2] (normalised coordinates) under E [...,3,3], in the convention of
    geom.pose_from_essential / geom.essential_from_pose: X2 = R X1 + t, E = [t]x R, x2^T E x1 = 0.
    (x2^T E x1)^2 / ((E x1)_x^2 + (E x1)_y^2 + (E^T x2)_x^2 + (E^T x2)_y^2), [...,P]."""
    one = torch.ones_like(x1[..., :1])
    h1, h2 = torch.cat([x1, one], -1), torch.cat([x2, one], -1)
    l2 = h1 @ E.transpose(-1, -2)          # rows (E x1)^T: the epipolar lines in image 2
    l1 = h2 @ E                            # rows (E^T x2)^T
    num = (h2 * l2).sum(-1) ** 2
    return num / (l2[..., 0] ** 2 + l2[..., 1] ** 2 + l1[..., 0] ** 2 + l1[..., 1] ** 2)
