"""References for rp_emm_guided_matches (include/relpose_guided.h), numpy only, no GPU and no library.

  guided_ref       the header's definitions in fp64 from the DENSE exponent (tests/_submatch_ref.py: dense_exponent), with the scales of
                   the GPU tests' bounds and the owners that have a pair on the edge of the band
  admission_f32    the header's admission restated in numpy float32 in the header's order
  guided_f32       the kernel's statements in float32: the 64-term fused multiply-add chain, the two normalisers, exp2, the admission,
                   the sequential sums of a lane's two halves.  The GPU tests' constants are 8 x its largest ratio on the same inputs.
  two_peak_inputs  built scenes whose rows have the true partner's peak (height 0.8) and, in a share f of the rows, a higher distractor
  grid_F           the fundamental matrix of a built scene in token-grid units

Layout as in tests/_submatch_ref.py: q, k [Z,576,H,64] float32, rlse / clse [Z,H,576], F [Z,9], band [Z]; image z's problem has rows
i = tokens of image z ^ 1 (q) and columns j = tokens of image z (k), and c_j^T F_z r_i = 0."""
import collections

import numpy as np

from tests import _refine_ref as RF
from tests import _submatch_ref as S

EPS32, GRID, TOK, HD, SCALE, LOG2E = S.EPS32, S.GRID, S.TOK, S.HD, S.SCALE, S.LOG2E
EDGE = 1e-4          # |rho^2 / (band^2 den) - 1| <= EDGE in fp64: the pair may fall on either side of the admission

Guided = collections.namedtuple("Guided", "idx stat ratio e A adm edge_owner de degenerate")
Guided.__doc__ = """idx [Z,H,576] int64, stat [Z,H,576,4] = (amax, bmass, mass, d2) fp64; ratio: admitted runner-up / maximum of A (0 with
fewer than two admitted); e, A [Z,H,576 owner,576 other] the exponent and exp of it, owner-major; adm [Z,576 owner,576 other] bool;
edge_owner [Z,576] the owner has a pair within EDGE of the band's edge; de [Z,H,576] the bound scale of the exponent; degenerate [Z]"""


def _tokens(dt=np.float64):
    n = np.arange(TOK)
    return np.stack([n % GRID, n // GRID, np.ones(TOK)], -1).astype(dt)


def degenerate(F, band):
    F, band = np.asarray(F, np.float64).reshape(-1, 9), np.asarray(band, np.float64)
    with np.errstate(all="ignore"):
        return ~np.isfinite(F).all(-1) | ~(np.abs(F).max(-1) > 0) | ~(band > 0)


def pair_terms(F):
    """fp64, per image: rho [Z,576 i,576 j], den the same, rho_abs = sum |c_a| |F_ab| |r_b| (the scale of rho's rounding)"""
    F = np.asarray(F, np.float64).reshape(-1, 3, 3)
    F = np.where(np.isfinite(F), F, 0)
    G = F                                                  # (the kernel's scaling by a power of two changes nothing here)
    t = _tokens()
    l = np.einsum("zab,ib->zia", G, t)                   # G r_i
    m = np.einsum("zab,ja->zjb", G, t)                   # G^T c_j
    rho = np.einsum("zia,ja->zij", l, t)
    den = (l[..., 0] ** 2 + l[..., 1] ** 2)[:, :, None] + (m[..., 0] ** 2 + m[..., 1] ** 2)[:, None, :]
    rho_abs = np.einsum("zab,ib,ja->zij", np.abs(G), t, t)
    return rho, den, rho_abs


def guided_ref(q, k, rlse, clse, F, band, scale=SCALE, swap=False, single=False):
    e = S.dense_exponent(q, k, rlse, clse, scale, single)
    Z, H = e.shape[:2]
    band = np.asarray(band, np.float64)
    dead = degenerate(F, band)
    rho, den, _ = pair_terms(F)
    with np.errstate(all="ignore"):
        b2 = np.where(dead, 1.0, band * band)[:, None, None]
        rel = np.where(den > 0, rho * rho / (b2 * den), 0.0)
    adm = ~(den > 0) | (rel <= 1)
    edge = (den > 0) & (np.abs(rel - 1) <= EDGE)
    d2 = np.where(den > 0, rho * rho / np.where(den > 0, den, 1), 0.0)
    if swap:
        e, adm, edge, d2 = e.transpose(0, 1, 3, 2), adm.transpose(0, 2, 1), edge.transpose(0, 2, 1), d2.transpose(0, 2, 1)
    A = np.exp(e)
    ea = np.where(adm[:, None], e, -np.inf)
    order = np.argsort(-ea, -1, kind="stable")[..., :2]                 # stable: the lowest index first among equals
    top = np.take_along_axis(ea, order, -1)
    none = ~np.isfinite(top[..., 0])
    idx = np.where(none, -1, order[..., 0])
    amax = np.where(none, 0, np.exp(top[..., 0]))
    with np.errstate(all="ignore"):
        ratio = np.where(np.isfinite(top[..., 1]) & ~none, np.exp(top[..., 1] - top[..., 0]), 0.0)
    stat = np.stack([amax, (A * adm[:, None]).sum(-1), A.sum(-1),
                     np.where(none, 0, np.take_along_axis(np.broadcast_to(d2[:, None], e.shape), np.maximum(idx, 0)[..., None], -1)[..., 0])], -1)
    idx[dead], stat[dead] = -1, 0
    own, loop, lo, ll = S._sides(np.abs(np.asarray(q, np.float64)), np.abs(np.asarray(k, np.float64)),
                                 None if rlse is None else np.abs(np.asarray(rlse, np.float64)),
                                 None if clse is None else np.abs(np.asarray(clse, np.float64)), swap, single)
    de = (1 if single else 2) * scale * (own @ loop.transpose(0, 1, 3, 2)).max(-1) + (0 if lo is None else lo) + (0 if ll is None else ll.max(-1, keepdims=True))
    return Guided(idx, stat, ratio, e, A, adm, edge.any(-1), EPS32 * de, dead)


def d2_at(F, idx, swap):
    """fp64 Sampson distance of the pairs (owner, idx) and the scale of its bound rho_abs^2 / den; both 0 where idx < 0 or den is 0"""
    rho, den, rho_abs = pair_terms(F)
    if swap:
        rho, den, rho_abs = rho.transpose(0, 2, 1), den.transpose(0, 2, 1), rho_abs.transpose(0, 2, 1)
    idx = np.asarray(idx, np.int64)
    at = lambda a: np.take_along_axis(np.broadcast_to(a[:, None], idx.shape + (TOK,)), np.maximum(idx, 0)[..., None], -1)[..., 0]      # noqa: E731
    r, d, ra = at(rho), at(den), at(rho_abs)
    ok = (idx >= 0) & (d > 0)
    d = np.where(ok, d, 1)
    return np.where(ok, r * r / d, 0), np.where(ok, ra * ra / d, 0)


# ------------------------------------------------------------------------------------------------ float32 restatement
_fma = S._fma32


def _sides_f32(F):
    """G = F 2^-k (max|G| in [0.5, 1)) and the header's (lx, ly, lz, l2) per row token, (mx, my, m2) per column token, all float32: [Z,576] each"""
    F = np.asarray(F, np.float32).reshape(-1, 9)
    with np.errstate(all="ignore"):
        G = np.ldexp(F, -np.frexp(np.abs(F).max(-1, keepdims=True))[1]).astype(np.float32)
    t = _tokens(np.float32)
    x, y = t[None, :, 0], t[None, :, 1]
    g = lambda c: np.broadcast_to(G[:, c, None], (len(G), TOK))      # noqa: E731
    lx, ly, lz = _fma(g(0), x, _fma(g(1), y, g(2))), _fma(g(3), x, _fma(g(4), y, g(5))), _fma(g(6), x, _fma(g(7), y, g(8)))
    mx, my = _fma(g(0), x, _fma(g(3), y, g(6))), _fma(g(1), x, _fma(g(4), y, g(7)))
    return G, (lx, ly, lz, _fma(lx, lx, ly * ly)), (mx, my, _fma(mx, mx, my * my))


def admission_f32(F, band):
    """[Z,576 i,576 j] bool in the header's order; a degenerate image admits nothing"""
    band = np.asarray(band, np.float32)
    t = _tokens(np.float32)
    with np.errstate(all="ignore"):
        _, (lx, ly, lz, l2), (_, _, m2) = _sides_f32(F)
        full = (len(band), TOK, TOK)
        cx, cy = np.broadcast_to(t[None, None, :, 0], full), np.broadcast_to(t[None, None, :, 1], full)
        bc = lambda a: np.broadcast_to(a[:, :, None], full)      # noqa: E731
        rho = _fma(cx, bc(lx), _fma(cy, bc(ly), bc(lz)))
        den = (l2[:, :, None] + m2[:, None, :]).astype(np.float32)
        b2 = (band * band).astype(np.float32)[:, None, None]
        adm = ~(den > 0) | ((rho * rho).astype(np.float32) <= (b2 * den).astype(np.float32))
    return adm & ~degenerate(F, band)[:, None, None]


def _sampson_f32(G, a, b):
    """csrc/two_view.h's Sampson distance in float32 (no contraction): G [Z,9], a, b [..., 2] broadcast against Z"""
    f = np.float32
    e = [G[:, c].reshape((-1,) + (1,) * (a.ndim - 2)).astype(f) for c in range(9)]
    ax, ay, bx, by = a[..., 0].astype(f), a[..., 1].astype(f), b[..., 0].astype(f), b[..., 1].astype(f)
    l2x, l2y, l2z = e[0] * ax + e[1] * ay + e[2], e[3] * ax + e[4] * ay + e[5], e[6] * ax + e[7] * ay + e[8]
    l1x, l1y = e[0] * bx + e[3] * by + e[6], e[1] * bx + e[4] * by + e[7]
    r = bx * l2x + by * l2y + l2z
    den = l2x * l2x + l2y * l2y + l1x * l1x + l1y * l1y
    with np.errstate(all="ignore"):
        return np.where(den > 0, r * r / np.where(den > 0, den, 1), 0).astype(f)


def guided_f32(q, k, rlse, clse, F, band, scale=SCALE, swap=False, single=False):
    """the kernel's statements in float32 -> (idx [Z,H,576] int64, stat [Z,H,576,4] float32)"""
    f = np.float32
    q, k = np.asarray(q, f), np.asarray(k, f)
    own, loop, lo, ll = S._sides(q, k, None if rlse is None else np.asarray(rlse, f), None if clse is None else np.asarray(clse, f), swap, single)
    Z, H = own.shape[:2]
    mul = f(f(1.0 if single else 2.0) * f(scale) * LOG2E)
    own = (own * mul).astype(f)
    acc = np.zeros((Z, H, TOK, TOK), f)
    for d in range(HD):
        acc = _fma(np.broadcast_to(loop[:, :, None, :, d], acc.shape), np.broadcast_to(own[:, :, :, None, d], acc.shape), acc)
    bo = np.zeros((Z, H, TOK), f) if lo is None else (lo * -LOG2E).astype(f)
    bl = np.zeros((Z, H, TOK), f) if ll is None else (ll * -LOG2E).astype(f)
    e = ((acc + bo[..., :, None]).astype(f) + bl[..., None, :]).astype(f)
    a = np.exp2(e).astype(f)
    adm = admission_f32(F, band)
    if swap:
        adm = adm.transpose(0, 2, 1)
    adm = np.broadcast_to(adm[:, None], e.shape)
    n = np.arange(TOK)
    halves = [n[(n % 8) < 4], n[(n % 8) >= 4]]                           # the loop tokens of a lane's lower / upper half-wave
    seq = lambda v: sum(np.add.accumulate(v[..., hv], axis=-1, dtype=f)[..., -1] for hv in halves).astype(f)      # noqa: E731
    mass, bmass = seq(a), seq(np.where(adm, a, f(0)))
    ea = np.where(adm, e, f(-np.inf))
    idx = ea.argmax(-1)
    top = np.take_along_axis(ea, idx[..., None], -1)[..., 0]
    none = ~np.isfinite(top)
    idx = np.where(none, -1, idx)
    amax = np.where(none, f(0), np.exp2(top)).astype(f)
    G = _sides_f32(F)[0]
    tok = _tokens(f)[:, :2]
    me, other = np.broadcast_to(tok[None, None], (Z, H, TOK, 2)), tok[np.maximum(idx, 0)]
    d2 = np.where(none, f(0), _sampson_f32(G, other if swap else me, me if swap else other))
    stat = np.stack([amax, bmass, mass, d2], -1).astype(f)
    dead = degenerate(F, band)
    idx[dead], stat[dead] = -1, 0
    return idx, stat


def stat_ratios(idx, stat, ref, F, swap):
    """largest error of a result over the GPU tests' bounds WITHOUT their constants: amax against A_ref at the result's own index and d2
    against the fp64 distance of the result's own pair (every live owner), bmass where the owner has no pair on the band's edge, mass
    everywhere.  Scales: de A_ref for the three sums of A (de: the exponent's rounding scale), eps32 rho_abs^2 / den for d2."""
    idx, stat = np.asarray(idx, np.int64), np.asarray(stat, np.float64)
    live = np.broadcast_to(~ref.degenerate[:, None, None], idx.shape)
    at = np.take_along_axis(ref.A, np.maximum(idx, 0)[..., None], -1)[..., 0]
    d2, d2s = d2_at(F, idx, swap)
    clear = live & ~np.broadcast_to(ref.edge_owner[:, None], idx.shape)
    has = live & (idx >= 0)

    def worst(err, scale, sel):
        with np.errstate(all="ignore"):
            r = np.where(err == 0, 0.0, err / scale)      # an error against a scale of 0 is infinitely bad
        return float(r[sel].max()) if sel.any() else 0.0
    return {"amax": worst(np.abs(stat[..., 0] - at), ref.de * at, has),
            "bmass": worst(np.abs(stat[..., 1] - ref.stat[..., 1]), ref.de * ref.stat[..., 1], clear),
            "mass": worst(np.abs(stat[..., 2] - ref.stat[..., 2]), ref.de * ref.stat[..., 2], live),
            "d2": worst(np.abs(stat[..., 3] - d2), EPS32 * d2s, has)}


def index_report(idx, ref, tau=1e-3):
    """check_indices of tests/test_gpu_readout.py over the owners without an edge pair, against the ADMITTED runner-up:
    (owners compared, owners left out / all, wrong where the runner-up is below (1 - tau) max, differing / compared)"""
    idx = np.asarray(idx, np.int64)
    keep = np.broadcast_to(~ref.edge_owner[:, None], idx.shape) | np.broadcast_to(ref.degenerate[:, None, None], idx.shape)
    clear = keep & (ref.ratio < 1 - tau)
    return {"compared": int(keep.sum()), "left_out": float(1 - keep.mean()), "wrong_clear": int((idx != ref.idx)[clear].sum()),
            "differ": float((idx != ref.idx)[keep].sum() / max(int(keep.sum()), 1))}


# ------------------------------------------------------------------------------------------------ inputs
def grid_F(b, pose=None):
    """[9]: the fundamental matrix of built scene b (tests/_submatch_ref.py: built_inputs) in token-grid units, for the problem whose rows
    are image 0's tokens and whose columns are image 1's; pose [7] = (t, q xyzw): another motion than the scene's own.  Frobenius norm 1."""
    Rm, t = (b.R, b.t) if pose is None else RF.pose_matrix(pose)
    E = RF.cross_matrix(np.asarray(t, np.float64)) @ Rm
    mid = (GRID - 1) / 2
    M = np.array([[1 / b.focal, 0, -mid / b.focal], [0, 1 / b.focal, -mid / b.focal], [0, 0, 1]])
    Fm = M.T @ E @ M
    return (Fm / np.linalg.norm(Fm)).reshape(9)


def true_pose(b):
    return np.concatenate([b.t, RF.rot_to_quat(b.R)])


TwoPeak = collections.namedtuple("TwoPeak", "q k built distracted")
GAIN = 12.0          # the score is GAIN (0.8 bump(p_i - c_j) + [distracted] 1.0 bump(d_i - c_j)), bump(0) = 1
_FREQ = None


def _frequencies():
    """32 lattice frequencies 2 pi (u, v) / 48, (u, v) distinct integer pairs in -10 .. 10 without (0, 0) and without a pair's negative:
    the period, 48 tokens, is twice the grid, so a bump has no second copy inside it"""
    global _FREQ
    if _FREQ is None:
        rng = np.random.default_rng(77)
        seen, out = set(), []
        while len(out) < HD // 2:
            u, v = (int(a) for a in rng.integers(-10, 11, 2))
            if (u, v) != (0, 0) and (u, v) not in seen and (-u, -v) not in seen:
                seen.add((u, v))
                out.append((u, v))
        _FREQ = 2 * np.pi * np.array(out, np.float64) / 48
    return _FREQ


def _features(p):
    ph = np.asarray(p, np.float64) @ _frequencies().T
    return np.concatenate([np.cos(ph), np.sin(ph)], -1)


def two_peak_inputs(s, f, H=1, scale=SCALE):
    """scene s of built_inputs with two-peaked rows: k_j = features(c_j), q_i = GAIN / (32 scale) (0.8 features(p_i) + 1.0 features(d_i) for
    a share f of the rows, d_i uniform over the grid).  Both images carry the same q and k, every head too."""
    b = S.built_inputs(s, H=1)
    rng = np.random.default_rng(5000 + 10 * s + int(round(10 * f)))
    distracted = rng.uniform(size=TOK) < f
    d = rng.uniform(-0.5, GRID - 0.5, (TOK, 2))
    tok = _tokens()[:, :2]
    q1 = GAIN / (HD // 2 * scale) * (0.8 * _features(b.p) + distracted[:, None] * _features(d))
    k1 = _features(tok)
    q = np.broadcast_to(q1[None, :, None, :], (2, TOK, H, HD)).astype(np.float32).copy()
    k = np.broadcast_to(k1[None, :, None, :], (2, TOK, H, HD)).astype(np.float32).copy()
    return TwoPeak(q, k, b, distracted)


def correct_share(b, idx, tol=0.75):
    """share of the in-image rows whose match idx [576] lies within `tol` tokens of the true partner"""
    idx = np.asarray(idx, np.int64)
    pos = np.stack([idx % GRID, idx // GRID], -1)
    ok = (idx >= 0) & (np.linalg.norm(pos - b.p, axis=-1) <= tol)
    return float(ok[b.inside].mean())


def refine_errors(b, idx, pose0, tau_tokens=0.5, iters=10):
    """refine_ref from pose0 on the matches idx [576] of image 0's tokens (weight 1 where the row is in the image and has a match) ->
    (rotation, translation-direction error in degrees, the robust cost at the end)"""
    idx = np.asarray(idx, np.int64)
    w = (b.inside & (idx >= 0)).astype(np.float64)[None]
    x2 = ((S.centres_of(np.maximum(idx, 0)) - (GRID - 1) / 2) / b.focal)[None]
    r = RF.refine_ref(np.asarray(pose0, np.float64)[None], b.x1[None], x2, w, np.array([tau_tokens / b.focal]), iters)
    Rm, t = RF.pose_matrix(r.pose[0])
    return RF.rotation_angle(Rm, b.R), RF.direction_angle(t, b.t), float(r.stat[0, 1])


# ------------------------------------------------------------------------------------------------ the parity cases (CPU calibration and GPU test)
def special_F(kind):
    """[9] in token-grid units: `sideways` a pure translation along x (every line is the owner's own grid row: parallel lines),
    `forward` a translation along the optical axis with the epipole at the grid token (11, 13) in both images (den = 0 exactly there),
    `miss` a sideways translation plus an offset of 30 rows, so that the lines of most owners miss the grid (-1 among live neighbours)"""
    if kind == "sideways":
        return np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float64)           # c_y - r_y = 0
    if kind == "forward":
        ep = np.array([11.0, 13.0, 1.0])
        return RF.cross_matrix(ep).reshape(9)                                 # c^T [e]x r = 0: c, r and the epipole collinear
    if kind == "miss":
        return np.array([0, 0, 0, 0, 0, -1, 0, 1, -18.25], np.float64)      # r_y - c_y = 18.25: only owners near the top / bottom rows have a token in the band
    raise ValueError(kind)


BANDS = (0.75, 1.5, 1e9)
# (inputs, H, swap, single, F kind, band): the issue's grid -- random (flat rows) and built (two-peaked scene 0, f = 0.5) inputs, both
# swaps and softmaxes, the three bands on a scene's F; the special matrices on H = 1 at band 1.5 (and 0.75 for the forward motion)
CASES = [(kind, 1, swap, single, "scene", band) for kind in ("random", "built") for swap in (0, 1) for single in (0, 1) for band in BANDS] + \
        [("random", 3, swap, single, "scene", 1.5) for swap in (0, 1) for single in (0, 1)] + \
        [("random", 1, swap, 0, Fk, 1.5) for swap in (0, 1) for Fk in ("sideways", "forward", "miss")] + \
        [("built", 1, swap, 1, "forward", 0.75) for swap in (0, 1)]
_INPUTS = {}


def case_inputs(kind, H):
    """(q, k, rlse, clse, scene) of a case, float32, computed once"""
    if (kind, H) not in _INPUTS:
        if kind == "built":
            tp = two_peak_inputs(0, 0.5, H=H)
            q, k, b = tp.q, tp.k, tp.built
        else:
            (q, k), b = S.random_inputs(40 + H, 2, H), S.built_inputs(0)
        _INPUTS[kind, H] = (q, k) + S.stats64(q, k) + (b,)
    return _INPUTS[kind, H]


def case_F(case, b):
    """F [2,9] float32 (image 1: the matrix named, image 0: its transpose) and band [2] float32"""
    Fk, band = case[4], case[5]
    F1 = (grid_F(b) if Fk == "scene" else special_F(Fk)).reshape(3, 3)
    return np.stack([F1.T.reshape(9), F1.reshape(9)]).astype(np.float32), np.full(2, band, np.float32)


def case_lse(case, q, k, rlse, clse):
    """the normalisers a case passes: the dual softmax's, or for `single` the row softmax's alone (rlse IS the row log-sum-exp)"""
    return (rlse, None) if case[3] else (rlse, clse)


# C = 8 x the largest ratio guided_f32 shows over CASES (tests/test_guided_cpu.py recomputes them), rounded up; the restatement's ratio
# beside each
C_AMAX = 11.5       # 1.426  |amax - A_ref at idx| / (de A_ref)
C_BMASS = 10.9      # 1.360  |bmass - ref| / (de bmass_ref), owners without a pair on the band's edge
C_MASS = 10.9       # 1.360  |mass - ref| / (de mass_ref)
C_D2 = 8.9          # 1.105  |d2 - ref at idx| / (eps32 rho_abs^2 / den)
