"""Third view: the pose of a camera against the structure of a pair -- three-point (P3P) consensus and a six-parameter polish, on the GPU.

Every two-view chain of this package returns a translation DIRECTION, and rel_pose_amd/triangulate.py writes points in units of the
baseline: two pairs that share an image give two baselines of unknown ratio.  include/relpose_resection.h (csrc_resection/resection.hip
-- a library of its own) fits the pose of a camera to 3-D points and their images; the length of its translation is that ratio
(DESIGN.md, 5.14).  The readout makes the three-view tracks for free: row p of pairs (hub, a) and (hub, c) is the same token of the hub.

    tv = model.eval().third_view_pose_from_matches(images, intrinsics)            # images [B,3,3,H,W] = (hub, a, c)
    tv.scale                                      # |t_c| / |t_a|: the baseline of (hub, c) in units of the baseline of (hub, a)
    # or, piece by piece (X [n,P,3] points, x [n,P,2] their calibrated images):
    c = p3p_consensus(X, x, w, tau=tau, hypotheses=256, seed=0)
    r = pnp_refine(X, x, w, c.pose, tau=tau, iters=10)

Convention: m = R X + t, x ~ m_xy / m_z; a pose is (t, q xyzw) with w >= 0 and t NOT normalised.  The same seed gives the same samples
and the same bits.  There is no fallback for the kernels."""
import collections

import torch

from . import _lib, ops
from .ops import _chk, _p, _st

P3PConsensus = collections.namedtuple("P3PConsensus", "pose best stat weights hyp_pose hyp_cost hyp_count samples")
P3PConsensus.__doc__ = """pose [n,7] the best hypothesis (all zero for a degenerate problem), best [n] int32 its index (-1: degenerate),
stat [n,4] = (its cost, the inlier weight share at it, the number of valid hypotheses, the number of rows of positive weight), weights
[n,P] the Cauchy weights w / (1 + d / tau^2) at pose, or None, hyp_pose [n,M,7] and hyp_cost [n,M] every hypothesis (an invalid one:
zeros and FLT_MAX), hyp_count [n,M] int32 the number of solutions of every sample, samples [n,M,3] int32 the sampled rows, or None"""
PnPRefined = collections.namedtuple("PnPRefined", "pose stat weights")
PnPRefined.__doc__ = """pose [n,7] = (t, q xyzw with w >= 0), stat [n,4] = (the robust cost, the inlier weight share, the number of
accepted steps, the number of rows of positive weight), weights [n,P] the Cauchy weights at pose, or None"""
ThirdView = collections.namedtuple("ThirdView", "pose_a pose_c scale stat structure two_view_c weights")
ThirdView.__doc__ = """pose_a [B,7] the pose of (hub, a) in unit baseline, pose_c [B,7] the pose of c against the structure of (hub, a), in
units of that baseline, scale [B] = |t_c| (0 for a degenerate result), stat [B,4] the PnPRefined.stat of pose_c, structure the
triangulate.MatchStructure of (hub, a) (its `chain` is None: the chain ran on both pairs at once), two_view_c the named chain's result
for (hub, c): rows B .. 2B - 1 of its ONE call on the 2B pairs (hub, a), (hub, c) -- a chain that draws samples seeds a problem by its
index in the batch, so this is not bit-equal to a separate call on the B pairs (hub, c) --, weights [B,P] the row weights the resection
ran on"""


def _rows(X, x, w, tau):
    """the host argument checks of both entry points -> (n, P, tau [n])"""
    if x.dim() != 3 or x.shape[-1] != 2:
        raise ValueError("x must be [n,P,2]")
    n, P = x.shape[:2]
    if tuple(X.shape) != (n, P, 3):
        raise ValueError("X must be [n,P,3]")
    if w is not None and tuple(w.shape) != (n, P):
        raise ValueError("w must be [n,P]")
    if tau is None:
        raise ValueError("the robust cost needs tau")
    if not torch.is_tensor(tau):
        tau = torch.full((n,), float(tau), device=x.device, dtype=torch.float32)
    if tuple(tau.shape) != (n,):
        raise ValueError("tau must be a number or [n]")
    return n, P, tau


def p3p_consensus(X, x, w=None, tau=0.01, hypotheses=256, seed=0, return_weights=False, return_samples=False):
    """X [n,P,3] points, x [n,P,2] their calibrated images, w [n,P] base weights (None: ones), tau: float or [n], the scale of the
    robust cost mean(w tau^2 log1p(d / tau^2)) of the distance d of include/relpose_resection.h, `hypotheses` samples of three per
    problem drawn from `seed` -> P3PConsensus.  3 <= P <= 1728, hypotheses <= 4096."""
    n, P, tau = _rows(X, x, w, tau)
    M, seed = int(hypotheses), int(seed)
    if not -2 ** 31 <= seed < 2 ** 32:
        raise ValueError("seed must fit 32 bits")
    seed = seed - 2 ** 32 if seed >= 2 ** 31 else seed               # the same 32-bit pattern as a C int
    lib = _lib.load_resection()
    _chk(X, x, w, tau)
    pose = ops._empty(n, 7, like=x)
    stat = ops._empty(n, 4, like=x)
    hyp_pose = ops._empty(n, max(M, 0), 7, like=x)
    hyp_cost = ops._empty(n, max(M, 0), like=x)
    best = torch.empty(n, dtype=torch.int32, device=x.device)
    hyp_count = torch.empty(n, max(M, 0), dtype=torch.int32, device=x.device)
    wo = ops._empty(n, P, like=x) if return_weights else None
    samples = torch.empty(n, max(M, 0), 3, dtype=torch.int32, device=x.device) if return_samples else None
    lib.rp_p3p_consensus(_p(X), _p(x), _p(w), _p(tau), seed, _p(pose), _p(best), _p(stat), _p(wo), _p(hyp_pose), _p(hyp_cost),
                         _p(hyp_count), _p(samples), P, M, n, _st())
    return P3PConsensus(pose, best, stat, wo, hyp_pose, hyp_cost, hyp_count, samples)


def pnp_refine(X, x, w, pose0, tau=0.01, iters=10, return_weights=False):
    """`iters` Levenberg-Marquardt iterations on the robust cost from pose0 [n,7] = (t, q) -> PnPRefined; iters = 0 scores pose0.
    0 <= iters <= 64."""
    n, P, tau = _rows(X, x, w, tau)
    if tuple(pose0.shape) != (n, 7):
        raise ValueError("pose0 must be [n,7]")
    lib = _lib.load_resection()
    _chk(X, x, w, tau, pose0)
    pose = ops._empty(n, 7, like=x)
    stat = ops._empty(n, 4, like=x)
    wo = ops._empty(n, P, like=x) if return_weights else None
    lib.rp_pnp_refine(_p(X), _p(x), _p(w), _p(tau), _p(pose0), int(iters), _p(pose), _p(stat), _p(wo), P, n, _st())
    return PnPRefined(pose, stat, wo)


def row_weights(structure, w_a, w_c, tau_a, min_parallax=None):
    """the row weights of third_view_pose: w_a / (1 + reproj / tau_a^2) w_c [depth1 > 0 and depth2 > 0] [parallax >= min_parallax];
    structure: the triangulate.Structure of pair (hub, a), w_a, w_c [B,P] the base weights of the two pairs, tau_a [B] or a number;
    min_parallax (radians, a number or [B]) None: tau_a -- below it the relative depth error of DESIGN.md 5.8, noise over parallax, is at
    least 1"""
    B = w_a.shape[0]
    if w_a.dim() != 2 or w_c.shape != w_a.shape or structure.reproj.shape != w_a.shape:
        raise ValueError("w_a, w_c and the structure's rows must be [B,P]")

    def per_pair(v, name):
        v = torch.as_tensor(v, device=w_a.device, dtype=torch.float32)
        if v.dim() == 0:
            v = v.expand(B)
        if tuple(v.shape) != (B,):
            raise ValueError("%s must be a number or [B]" % name)
        return v[:, None]
    tau_a = per_pair(tau_a, "tau_a")
    floor = tau_a if min_parallax is None else per_pair(min_parallax, "min_parallax")
    keep = (structure.depth1 > 0) & (structure.depth2 > 0) & (structure.parallax >= floor)
    return (w_a * (1.0 / (1.0 + structure.reproj / (tau_a * tau_a))) * w_c * keep.to(w_a.dtype)).contiguous()


def third_view_pose(model, images, intrinsics, chain="consensus", hypotheses=256, seed=0, iters=10, min_parallax=None, **chain_kwargs):
    """ViTEss.third_view_pose_from_matches: images [B,3,3,H,W] = (hub, a, c), intrinsics [B,3,4] in pixels of (H, W) -> ThirdView.  The
    composition of the public pieces and nothing else: ONE call of triangulate.structure_from_matches (the named chain with
    `chain_kwargs`, then rp_triangulate) on the 2B pairs (hub, a), (hub, c) -- the first B rows are the structure, the last B rows of the
    chain's result are two_view_c --, row_weights, p3p_consensus and pnp_refine with the tau of pair (hub, c).  `seed` also seeds a
    chain that draws samples, unless chain_kwargs names another.  chain_kwargs' `tau` may be a number, [B] (one per triple, used for both
    of its pairs) or [2B] (the pairs (hub, a), then the pairs (hub, c))."""
    from . import triangulate
    if images.dim() != 5 or images.shape[1] != 3:
        raise ValueError("images must be [B,3,3,H,W]: (hub, a, c)")
    B = images.shape[0]
    if tuple(intrinsics.shape) != (B, 3, 4):
        raise ValueError("intrinsics must be [B,3,4]")
    pairs = torch.cat([images[:, [0, 1]], images[:, [0, 2]]]).contiguous()
    intr = torch.cat([intrinsics[:, [0, 1]], intrinsics[:, [0, 2]]]).contiguous()
    if chain in ("consensus", "planar"):
        chain_kwargs.setdefault("seed", seed)
    if chain_kwargs.get("tau") is not None:
        tau = torch.as_tensor(chain_kwargs["tau"], device=images.device, dtype=torch.float32)
        if tau.dim() == 0:
            tau = tau.expand(2 * B)
        elif tuple(tau.shape) == (B,):
            tau = torch.cat([tau, tau])
        if tuple(tau.shape) != (2 * B,):
            raise ValueError("tau must be a number, [B] or [2B]")
        chain_kwargs["tau"] = tau.contiguous()
    ms = triangulate.structure_from_matches(model, pairs, intr, chain=chain, **chain_kwargs)
    st = triangulate.Structure(*_part(tuple(ms.structure), 2 * B, slice(0, B)))
    structure = triangulate.MatchStructure(st, *_part(tuple(ms[1:6]), 2 * B, slice(0, B)), None)
    tau_c, w_c, x = _part((ms.tau, ms.weights, ms.x2), 2 * B, slice(B, 2 * B))
    w = row_weights(st, structure.weights, w_c, structure.tau, min_parallax)
    c = p3p_consensus(st.points, x, w, tau=tau_c, hypotheses=hypotheses, seed=seed)
    r = pnp_refine(st.points, x, w, c.pose, tau=tau_c, iters=iters)
    return ThirdView(structure.pose, r.pose, r.pose[:, :3].norm(dim=-1), r.stat, structure, _part(ms.chain, 2 * B, slice(B, 2 * B)), w)


def _part(t, n, rows):
    """the rows `rows` of every tensor in a (nested) tuple of per-problem results; every tensor must lead with the batch of n problems
    -- one that does not is an error, not something to pass through or to slice by coincidence of sizes; None and non-tensors stay"""
    if torch.is_tensor(t):
        if t.dim() == 0 or t.shape[0] != n:
            raise ValueError("a chain result of shape %s does not lead with the %d pairs of the call" % (tuple(t.shape), n))
        return t[rows].contiguous()
    if isinstance(t, tuple):
        parts = [_part(e, n, rows) for e in t]
        return type(t)(*parts) if hasattr(t, "_fields") else tuple(parts)
    return t
