"""References for rp_emm_submatch (include/relpose_submatch.h), numpy only, no GPU and no library.

  submatch_ref     the header's definitions in fp64, from the DENSE exponent e[z][h][i][j]
  submatch_f32     the kernel's statements restated in numpy float32 in the kernel's order: the 64-term fused multiply-add chain, the
                   exponent, exp2 of (e - e_max) log2(e), the xor butterflies over the 32 lanes of a group, the vertex.  The GPU tests'
                   constants are 8 x its largest ratio on the same inputs.
  built_inputs     one pair whose scores are exact Gaussians around the true sub-token position of every token's partner
  random_inputs    standard_normal q, k at scale 0.125: flat, multi-modal rows
  chain_errors     x2 from token centres / win / quad -> eight_point_ref -> decode_pose -> refine_ref -> errors against the true pose

Layout everywhere: q, k [Z,576,H,64] float32 (token-major, as the packed qkv holds them), rlse / clse [Z,H,576] float32, idx [Z,H,576] int32;
image z's problem has rows i = tokens of image z ^ 1 (q) and columns j = tokens of image z (k)."""
import collections

import numpy as np

from tests import _eightpoint_ref as R
from tests import _refine_ref as F

EPS32 = float(np.finfo(np.float32).eps)
GRID, TOK, HD = 24, 576, 64
SCALE = HD ** -0.5
LOG2E = np.float32(1.4426950408889634)
INT_MIN = -2 ** 31

Sub = collections.namedtuple("Sub", "win quad delta_e off_x off_y both_x both_y valid x0 y0")
Sub.__doc__ = """win, quad [Z,H,576,4]; delta_e [Z,H,576] the bound scale of the header's exponent per owner (reference only); off_x / off_y the
UNCLAMPED vertex offsets 0.5 (c - a) / cx (nan where undefined); both_x / both_y: the two neighbours exist (owner valid); valid, x0, y0 [Z,H,576]: of the window centre"""


# ------------------------------------------------------------------------------------------------ shared pieces
def _slots(radius):
    W = 2 * radius + 1
    s = np.arange(32)
    return W, s % W - radius, s // W - radius, s < W * W


def _window(idx, radius):
    """per owner and lane: (valid [..], live [..,32], n [..,32] clipped into range, dx, dy [32], x0, y0 [..])"""
    W, dx, dy, used = _slots(radius)
    idx = np.asarray(idx, np.int64)
    valid = (idx >= 0) & (idx < TOK)
    n0 = np.where(valid, idx, 0)
    x0, y0 = n0 % GRID, n0 // GRID
    x, y = x0[..., None] + dx, y0[..., None] + dy
    live = valid[..., None] & used & (x >= 0) & (x < GRID) & (y >= 0) & (y < GRID)
    n = np.where(live, y * GRID + x, 0)
    return valid, live, n, dx, dy, x0, y0


def _sides(q, k, rlse, clse, swap, single):
    """(owner vectors [Z,H,576,64], loop vectors, owner lse [Z,H,576] or None, loop lse or None) of image z's problem"""
    Z = q.shape[0]
    partner = np.arange(Z) ^ 1
    rows, cols = q[partner].transpose(0, 2, 1, 3), k.transpose(0, 2, 1, 3)          # rows i: q of the partner image; columns j: k of image z
    if swap:
        return cols, rows, (None if single else clse), rlse
    return rows, cols, rlse, (None if single else clse)


def dense_exponent(q, k, rlse, clse, scale=SCALE, single=False):
    """e [Z,H,576 i,576 j] in fp64 from float32 inputs"""
    rows, cols, _, _ = _sides(np.asarray(q, np.float64), np.asarray(k, np.float64), None, None, False, single)
    S = scale * rows @ cols.transpose(0, 1, 3, 2)
    if single:
        return S - np.asarray(rlse, np.float64)[..., :, None]
    return 2 * S - np.asarray(rlse, np.float64)[..., :, None] - np.asarray(clse, np.float64)[..., None, :]


def stats64(q, k, scale=SCALE):
    """(rlse, clse) [Z,H,576] float32: logsumexp of S over j / over i, as rp_emm_stats defines them"""
    rows, cols, _, _ = _sides(np.asarray(q, np.float64), np.asarray(k, np.float64), None, None, False, False)
    S = scale * rows @ cols.transpose(0, 1, 3, 2)

    def lse(a, axis):
        m = a.max(axis, keepdims=True)
        return (m + np.log(np.exp(a - m).sum(axis, keepdims=True))).squeeze(axis)
    return lse(S, -1).astype(np.float32), lse(S, -2).astype(np.float32)


def argmax_idx(q, k, rlse, clse, scale=SCALE, swap=False, single=False):
    """what rp_emm_matches writes as idx, from the fp64 exponent: [Z,H,576] int32"""
    e = dense_exponent(q, k, rlse, clse, scale, single)
    return (e.argmax(-2) if swap else e.argmax(-1)).astype(np.int32)


def _vertex(a, b, c, both, dt):
    with np.errstate(all="ignore"):
        curv = np.where(both, (b - a) + (b - c), 0).astype(dt)
        raw = (dt(0.5) * (c - a) / curv).astype(dt)
        on = both & (curv > 0)
        off = np.where(on, np.minimum(np.maximum(raw, dt(-0.5)), dt(0.5)), 0).astype(dt)
    return off, curv, np.where(on, raw, np.nan)


def _finish(e, live, valid, dx, dy, x0, y0, radius, dt, summer, exp_):
    """e [...,32] with -inf on dead lanes -> (win, quad, raw offsets, both flags); summer: the sum over the lanes"""
    W = 2 * radius + 1
    with np.errstate(all="ignore"):
        emax = e.max(-1, keepdims=True)
        u = np.where(live, exp_(e - emax), 0).astype(dt)
        fdx, fdy = dx.astype(dt), dy.astype(dt)
        su, sx, sy = summer(u), summer(u * fdx), summer(u * fdy)
        sm = summer(np.where(live, exp_(e), 0).astype(dt))
        mx, my = np.where(valid, sx / su, 0).astype(dt), np.where(valid, sy / su, 0).astype(dt)
        rx, ry = fdx - mx[..., None], fdy - my[..., None]
        if dt is np.float32:          # fmaf(rx, rx, ry * ry)
            t = (rx.astype(np.float64) * rx + (ry * ry).astype(np.float64)).astype(np.float32)
        else:
            t = rx * rx + ry * ry
        sv = summer(u * t)
        win = np.stack([x0 + mx, y0 + my, sm, sv / su], -1).astype(dt)
    c0 = radius * W + radius
    bx, by = valid & (x0 > 0) & (x0 < GRID - 1), valid & (y0 > 0) & (y0 < GRID - 1)
    ox, cx, rawx = _vertex(e[..., c0 - 1], e[..., c0], e[..., c0 + 1], bx, dt)
    oy, cy, rawy = _vertex(e[..., c0 - W], e[..., c0], e[..., c0 + W], by, dt)
    quad = np.stack([x0 + ox, y0 + oy, cx, cy], -1).astype(dt)
    flag = np.array([-1, -1, 0, 0], dt)
    win, quad = np.where(valid[..., None], win, flag), np.where(valid[..., None], quad, flag)
    return win, quad, rawx, rawy, bx, by


# ------------------------------------------------------------------------------------------------ fp64 reference
def submatch_ref(q, k, rlse, clse, idx, scale=SCALE, swap=False, single=False, radius=2):
    """the header in fp64 from the dense exponent -> Sub"""
    e = dense_exponent(q, k, rlse, clse, scale, single)
    if swap:
        e = e.transpose(0, 1, 3, 2)                     # owner-major
    valid, live, n, dx, dy, x0, y0 = _window(idx, radius)
    ew = np.where(live, np.take_along_axis(e, n, -1), -np.inf)
    win, quad, rawx, rawy, bx, by = _finish(ew, live, valid, dx, dy, x0, y0, radius, np.float64, lambda v: v.sum(-1), np.exp)
    # the bound scale: eps32 (m scale max_window sum_d |q_d k_d| + |lse_owner| + max_window |lse_other|)
    own, loop, lo, ll = _sides(np.abs(np.asarray(q, np.float64)), np.abs(np.asarray(k, np.float64)),
                               None if rlse is None else np.abs(np.asarray(rlse, np.float64)),
                               None if clse is None else np.abs(np.asarray(clse, np.float64)), swap, single)
    ab = np.where(live, np.take_along_axis(own @ loop.transpose(0, 1, 3, 2), n, -1), 0).max(-1)
    lse = 0 if lo is None else lo
    if ll is not None:
        lse = lse + np.where(live, np.take_along_axis(ll[..., None, :].repeat(TOK, -2), n, -1), 0).max(-1)
    delta_e = EPS32 * ((1 if single else 2) * scale * ab + lse)
    return Sub(win, quad, delta_e, rawx, rawy, bx, by, valid, x0, y0)


# ------------------------------------------------------------------------------------------------ float32 restatement
def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _butterfly(v):
    """the xor butterfly 16, 8, 4, 2, 1 over the 32 lanes of a group: every lane ends with the same bits; lane 0's are returned"""
    lanes = np.arange(32)
    v = v.astype(np.float32)
    for o in (16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def submatch_f32(q, k, rlse, clse, idx, scale=SCALE, swap=False, single=False, radius=2):
    """the kernel's statements in float32, in its order -> Sub (delta_e = None)"""
    q, k = np.asarray(q, np.float32), np.asarray(k, np.float32)
    own, loop, lo, ll = _sides(q, k, None if rlse is None else np.asarray(rlse, np.float32),
                               None if clse is None else np.asarray(clse, np.float32), swap, single)
    valid, live, n, dx, dy, x0, y0 = _window(idx, radius)
    Z, H = own.shape[:2]
    zi, hi = np.arange(Z)[:, None, None, None], np.arange(H)[None, :, None, None]
    rows = loop[zi, hi, n]                              # [Z,H,576,32,64]
    dot = np.zeros(n.shape, np.float32)
    for d in range(HD):
        dot = _fma32(own[..., None, d], rows[..., d], dot)
    mul = np.float32(1.0 if single else 2.0) * np.float32(scale)
    lse_own = np.zeros(own.shape[:3], np.float32) if lo is None else lo
    lse_loop = np.zeros(n.shape, np.float32) if ll is None else ll[zi, hi, n]
    e = _fma32(np.broadcast_to(mul, dot.shape), dot, -np.broadcast_to(lse_own[..., None], dot.shape)) - lse_loop
    e = np.where(live, e, np.float32(-np.inf)).astype(np.float32)
    win, quad, rawx, rawy, bx, by = _finish(e, live, valid, dx, dy, x0, y0, radius, np.float32, _butterfly,
                                            lambda a: np.exp2((a * LOG2E).astype(np.float32)).astype(np.float32))
    return Sub(win, quad, None, rawx, rawy, bx, by, valid, x0, y0)


# ------------------------------------------------------------------------------------------------ inputs
Built = collections.namedtuple("Built", "q k p inside x1 R t focal g")
Built.__doc__ = """q, k [2,576,H,64] float32; p [576,2] the true position of every token's partner in image 1, token-grid units (fp64);
inside [576] the partner lies inside image 1; x1 [576,2] the normalised centres of image 0; R, t the true motion X2 = R X1 + t"""


def _orthogonal(rng, n):
    Q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return Q * np.sign(np.diag(r))


def built_inputs(s, g=0.5, focal=0.9 * GRID, seed0=4000, H=1, scale=SCALE, dtype=np.float32):
    """Scene s, drawn like _eightpoint_ref.noisy_scene (rotation <= 0.3 rad, |t| 1 .. 1.5, depths 2 .. 8) from seed seed0 + s.  The token
    grid is image 0 (principal point at the grid's middle, focal length `focal` token units); S[i][j] = -g |p_i - c_j|^2 exactly in
    real arithmetic, as rank-4 vectors  q_i = (2 g p, -g |p|^2, 1) / scale,  k_j = (c, 1, -g |c|^2)  (coordinates about the grid's
    middle) mixed into 64 dimensions by a random orthogonal matrix per head.  Both images carry the same q and the same k, so both
    problems of the pair are this one.  dtype: float32 as the kernel reads them, or float64 (the peak then IS a Gaussian to fp64 rounding)."""
    rng = np.random.default_rng(seed0 + s)
    Rm = R._rotation(rng, 0.3)
    t = rng.standard_normal(3)
    t *= rng.uniform(1.0, 1.5) / np.linalg.norm(t)
    z = rng.uniform(2.0, 8.0, TOK)
    tok = np.arange(TOK)
    mid = (GRID - 1) / 2
    c = np.stack([tok % GRID, tok // GRID], -1) - mid                      # centres about the middle
    x1 = c / focal
    X2 = np.concatenate([x1 * z[:, None], z[:, None]], -1) @ Rm.T + t
    assert X2[:, 2].min() > 0.2
    pc = X2[:, :2] / X2[:, 2:] * focal                                     # partner positions about the middle
    p = pc + mid
    inside = ((p > -0.5) & (p < GRID - 0.5)).all(-1)
    q4 = np.concatenate([2 * g * pc, -g * (pc * pc).sum(-1, keepdims=True), np.ones((TOK, 1))], -1) / scale
    k4 = np.concatenate([c, np.ones((TOK, 1)), -g * (c * c).sum(-1, keepdims=True)], -1)
    q, k = np.zeros((2, TOK, H, HD), dtype), np.zeros((2, TOK, H, HD), dtype)
    for h in range(H):
        M = _orthogonal(rng, HD)[:4]
        q[:, :, h], k[:, :, h] = (q4 @ M).astype(dtype), (k4 @ M).astype(dtype)
    return Built(q, k, p, inside, x1, Rm, t / np.linalg.norm(t), focal, g)


def random_inputs(seed, Z=2, H=3, std=0.125):
    """standard_normal q, k at scale `std`: flat rows with many modes"""
    rng = np.random.default_rng(9000 + seed)
    return (std * rng.standard_normal((Z, TOK, H, HD))).astype(np.float32), (std * rng.standard_normal((Z, TOK, H, HD))).astype(np.float32)


def table_idx(Z, H, invalid=True):
    """the hand-made window centres [Z,H,576]: the four corners, every border token, all owners of one (z, h) on one token, and (invalid)
    -1, 576 and INT_MIN among valid neighbours"""
    tok = np.arange(TOK)
    border = tok[(tok % GRID == 0) | (tok % GRID == GRID - 1) | (tok // GRID == 0) | (tok // GRID == GRID - 1)]
    corners = np.array([0, GRID - 1, TOK - GRID, TOK - 1])
    base = np.concatenate([corners, border, (tok * 7 + 3) % TOK])[:TOK]
    idx = np.empty((Z, H, TOK), np.int64)
    for z in range(Z):
        for h in range(H):
            idx[z, h] = np.roll(base, 5 * (z * H + h))
    idx[Z - 1, H - 1] = 301                                                # all owners on one token
    if invalid:
        idx[0, 0, [2, 40, 41, 300, 575]] = [-1, TOK, INT_MIN, 2 ** 31 - 1, -TOK]
    return idx.astype(np.int32)


# ------------------------------------------------------------------------------------------------ bounds
FLAG = (-1.0, -1.0, 0.0, 0.0)


def bound_ratios(got, ref, radius, built=False):
    """largest error of `got` (win, quad [Z,H,576,4]) over the bounds of tests/test_gpu_submatch.py WITHOUT their constant C, per bound.
    Every valid owner is compared for win and for the curvatures (an invalid one must hold the flag exactly); px / py where the two
    neighbours exist and the reference's curvature is >= 1e-3 (built: every such owner, and the curvature must be positive) -- where a
    clamp is active only if both sides clamp, and then the positions must be equal."""
    win, quad = np.asarray(got[0], np.float64), np.asarray(got[1], np.float64)
    v = ref.valid
    assert bool((win[~v] == FLAG).all()) and bool((quad[~v] == FLAG).all()), "an invalid owner does not hold the flag"
    de, r2 = ref.delta_e[v], 2 * radius
    out = {"wxy": float((np.abs(win[v][:, :2] - ref.win[v][:, :2]).max(-1) / (r2 * de)).max()),
           "wmass": float((np.abs(win[v][:, 2] - ref.win[v][:, 2]) / ref.win[v][:, 2] / de).max()),
           "wvar": float((np.abs(win[v][:, 3] - ref.win[v][:, 3]) / (r2 ** 2 * de)).max()),
           "curv": float((np.abs(quad[v][:, 2:] - ref.quad[v][:, 2:]).max(-1) / (4 * de)).max())}
    worst, compared, total = 0.0, 0, 0
    for a, (raw, both, centre) in enumerate(((ref.off_x, ref.both_x, ref.x0), (ref.off_y, ref.both_y, ref.y0))):
        c_ref = ref.quad[..., 2 + a]
        assert not built or bool((c_ref[both] > 0).all())
        want = both if built else both & (c_ref >= 1e-3)
        with np.errstate(all="ignore"):
            bound = 4 * ref.delta_e * (1 + 2 * np.abs(raw)) / c_ref
        off_g, off_r = quad[..., a] - centre, ref.quad[..., a] - centre
        clamped_r, clamped_g = np.abs(raw) >= 0.5, np.abs(off_g) >= 0.5
        free, pinned = want & ~clamped_r & ~clamped_g, want & clamped_r & clamped_g
        assert bool((off_g[pinned] == off_r[pinned]).all())
        if free.any():
            worst = max(worst, float((np.abs(off_g - off_r)[free] / bound[free]).max()))
        compared, total = compared + int(free.sum() + pinned.sum()), total + int(want.sum())
    out["pxy"], out["compared"] = worst, compared / max(total, 1)
    return out


# ------------------------------------------------------------------------------------------------ the chain
def chain_errors(b, pos, tau_tokens, w=None):
    """pos [576,2] positions in image 1 (token-grid units) of the partners of image 0's tokens -> (rotation error, translation-direction
    error) in degrees of eight_point_ref(iters = 4) -> decode_pose -> refine_ref(iters = 10) against the scene's motion"""
    x1 = b.x1[None]
    x2 = ((np.asarray(pos, np.float64) - (GRID - 1) / 2) / b.focal)[None]
    w = b.inside.astype(np.float64)[None] if w is None else w
    tau = np.array([tau_tokens / b.focal])
    E = R.eight_point_ref(x1, x2, w, tau, 4)[0]
    pose = F.decode_pose(E[0], x1[0][w[0] > 0], x2[0][w[0] > 0])
    r = F.refine_ref(pose[None], x1, x2, w, tau, 10)
    Rm, t = F.pose_matrix(r.pose[0])
    return F.rotation_angle(Rm, b.R), F.direction_angle(t, b.t)


def centres_of(idx):
    idx = np.asarray(idx, np.int64)
    return np.stack([idx % GRID, idx // GRID], -1).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the parity cases (CPU calibration and GPU test)
# (kind, H, swap, single, radius, idx source).  built: scene 0 with its argmax as the centre -- a clean peak, the quad positions of every
# interior owner are compared (swap = 0; with swap = 1 the rows i form a warped grid and the rule of the random inputs applies).
# random: flat rows, with the argmax and with the hand-made table (corners, borders, one token for all, invalid entries).
CASES = [("built", H, swap, single, radius, "argmax") for H in (1, 3) for swap in (0, 1) for single in (0, 1) for radius in (1, 2)] + \
        [("random", H, swap, single, radius, src) for H in (1, 3) for swap in (0, 1) for single in (0, 1) for radius in (1, 2)
         for src in ("argmax", "table")]
# C = 8 x the largest ratio submatch_f32 shows over CASES (tests/test_submatch_cpu.py recomputes them), rounded up; the restatement's
# ratio beside each
C_WXY = 5.4        # 0.665  |wx|, |wy| error / (2 radius delta_e)
C_WMASS = 5.3      # 0.657  wmass relative error / delta_e
C_WVAR = 0.93      # 0.116  wvar error / ((2 radius)^2 delta_e)
C_CURV = 3.6       # 0.450  cx, cy error / (4 delta_e)
C_PXY = 3.2        # 0.396  px, py error / (4 delta_e (1 + 2 |offset_ref|) / c_ref)
_INPUTS = {}


def case_inputs(kind, H):
    """(q, k, rlse, clse) of a case, float32, computed once"""
    if (kind, H) not in _INPUTS:
        q, k = built_inputs(0, H=H)[:2] if kind == "built" else random_inputs(H, 2, H)
        _INPUTS[kind, H] = (q, k) + stats64(q, k)
    return _INPUTS[kind, H]


def case_idx(case, q, k, rlse, clse):
    kind, H, swap, single, radius, src = case
    return table_idx(2, H) if src == "table" else argmax_idx(q, k, rlse, clse, SCALE, swap, single)
