"""References for include/relpose_rotation.h (librelpose_rotation.so), shared by tests/test_rotation_cpu.py,
tests/test_gpu_rotation.py and tests/test_gpu_rotation_contract.py.

Every routine is written ONCE, over a dtype: with float64 it is the reference -- and there the two-point rotation is NOT the header's
frames but a second route, the least-squares rotation of the two bearing pairs by LAPACK (Kabsch: the polar factor of sum b_k a_k^T) --,
with float32 and the kernel's statements in the kernel's order it is the restatement that calibrates the GPU bounds: a bound is
C eps32 scale(ref) with C = 8 x the restatement's worst ratio on the same inputs.  The sampler is the contract sampler restated with two
draws, as _homography_ref.draw4 restates it with four.  Scene builders: the pure-rotation recipe of DESIGN.md 5.11 and its exact variant."""
import collections

import numpy as np

from tests import _consensus_ref as C
from tests import _homography_ref as H

FLT_MAX = C.FLT_MAX
EPS32 = H.EPS32
MIN_SCALE, DEN_MIN, D_MAX, FINITE = 1e-30, 1e-30, 1e30, 3.0e38
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-7, 1e7
SPAN_MIN = 1e-6
TAU, SEED = 0.01, 1

Consensus = collections.namedtuple("Consensus", "R best stat weights hyp_R hyp_cost samples span")
Refined = collections.namedtuple("Refined", "R pose stat weights kappa")


# ------------------------------------------------------------------------------------------------ the sampler
def draw2(seed, i, m, K):
    """the two indices c_0, c_1 into pos of hypotheses m (an int array) of problem i: [len(m), 2]; K >= 2"""
    m = np.atleast_1d(np.asarray(m, np.uint64))
    base = C.mix((np.uint64(seed & 0xFFFFFFFF) + np.uint64(C.GOLDEN) * np.uint64(i + 1)) & np.uint64(0xFFFFFFFF))
    s = C.mix(base ^ m)
    c = np.zeros((len(m), 2), np.int64)
    for k in range(2):
        r = C.mix((s + np.uint64((C.GOLDEN * (k + 1)) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF))
        j = K - 2 + k
        t = ((r * np.uint64(j + 1)) >> np.uint64(32)).astype(np.int64)
        seen = (c[:, :k] == t[:, None]).any(-1)
        c[:, k] = np.where(seen, j, t)
    return c


def sample_rows2(w, n, P, seed, M, first=0):
    """(pos per problem, samples [n,M,2] of row numbers; zeros where K < 2); problem b of the batch has index first + b"""
    wc = C.clamp(w, n, P)
    pos = [np.flatnonzero(wc[b] > 0) for b in range(n)]
    samples = np.zeros((n, M, 2), np.int64)
    for b in range(n):
        if len(pos[b]) >= 2:
            samples[b] = pos[b][draw2(seed, first + b, np.arange(M), len(pos[b]))]
    return pos, samples


# ------------------------------------------------------------------------------------------------ shared arithmetic, over a dtype
def distance(Rm, a, b):
    """the distance of the header: Rm [...,3,3] (dtype decides), a, b [P,2] -> [...,P]"""
    f = Rm.dtype.type
    h = Rm.reshape(Rm.shape[:-2] + (1, 9))
    x, y, u, v = a[:, 0].astype(f), a[:, 1].astype(f), b[:, 0].astype(f), b[:, 1].astype(f)
    with np.errstate(all="ignore"):
        m0 = h[..., 0] * x + h[..., 1] * y + h[..., 2]
        m1 = h[..., 3] * x + h[..., 4] * y + h[..., 5]
        m2 = h[..., 6] * x + h[..., 7] * y + h[..., 8]
        ex, ey = m0 - u * m2, m1 - v * m2
        d = np.fmin((ex * ex + ey * ey) / np.maximum(m2 * m2, f(DEN_MIN)), f(D_MAX))
        return np.where(m2 > 0, d, f(D_MAX))


def cost(Rm, a, b, w, tau):
    """the robust cost of Rm [...,3,3] on the rows a, b [K,2] with weights w [K] (already clamped, in Rm's dtype)"""
    f = Rm.dtype.type
    t2 = f(tau) * f(tau)
    with np.errstate(all="ignore"):
        return H._seqsum(w * (t2 * np.log1p(distance(Rm, a, b) / t2))) / H._seqsum(w)


def unit(v):
    """unit<N> of csrc/two_view.h on v [S,N]: (v / |v| with the largest magnitude divided out first, |v|)"""
    f = v.dtype.type
    with np.errstate(all="ignore"):
        m = np.abs(v).max(-1)
        ok = m > 0
        u = v / np.where(ok, m, f(1))[:, None]
        ss = np.zeros(len(v), v.dtype)
        for i in range(v.shape[1]):
            ss = ss + u[:, i] * u[:, i]
        s = np.sqrt(ss)
        u = u / np.where(ok, s, f(1))[:, None]
    return np.where(ok[:, None], u, v), np.where(ok, m * s, f(0))


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)


def bearings(p):
    """p [S,2] -> unit(x, y, 1) [S,3]"""
    return unit(np.concatenate([p, np.ones((len(p), 1), p.dtype)], -1))[0]


def frame(p0, p1):
    """(e [S,3,3] the rows e_1, e_2, e_3, |p0 x p1| [S])"""
    e1 = unit(p0 + p1)[0]
    nrm, span = unit(cross(p0, p1))
    e2 = unit(cross(nrm, e1))[0]
    return np.stack([e1, e2, cross(e1, e2)], 1), span


def minimal(p1, p2, lapack):
    """the two-point rotation of the header on samples p1, p2 [S,2,2] (their dtype decides) -> (R [S,3,3], valid [S],
    min(|a_0 x a_1|, |b_0 x b_1|) [S] in fp64); lapack: the least-squares rotation by SVD instead of the header's frames"""
    dt = p1.dtype
    a0, a1, b0, b1 = bearings(p1[:, 0]), bearings(p1[:, 1]), bearings(p2[:, 0]), bearings(p2[:, 1])
    e, sa = frame(a0, a1)
    f, sb = frame(b0, b1)
    if lapack:
        B = b0[:, :, None] * a0[:, None, :] + b1[:, :, None] * a1[:, None, :]
        U, _, Vt = np.linalg.svd(B)
        det = np.linalg.det(U @ Vt)
        Rm = U @ (np.stack([np.ones_like(det), np.ones_like(det), det], -1)[:, :, None] * Vt)
    else:
        Rm = np.empty((len(p1), 3, 3), dt)
        for r in range(3):
            for c in range(3):
                Rm[:, r, c] = (f[:, 0, r] * e[:, 0, c] + f[:, 1, r] * e[:, 1, c]) + f[:, 2, r] * e[:, 2, c]
    fin = np.isfinite(Rm).all((1, 2))
    valid = (sa >= dt.type(SPAN_MIN)) & (sb >= dt.type(SPAN_MIN)) & fin
    a64, b64 = [bearings(p1[:, k].astype(np.float64)) for k in range(2)], [bearings(p2[:, k].astype(np.float64)) for k in range(2)]
    span = np.minimum(np.linalg.norm(np.cross(a64[0], a64[1]), axis=-1), np.linalg.norm(np.cross(b64[0], b64[1]), axis=-1))
    return np.where(fin[:, None, None], Rm, 0), valid, span


# ------------------------------------------------------------------------------------------------ entry point 1
def consensus(x1, x2, w=None, tau=TAU, seed=SEED, M=256, dt=np.float64, first=0):
    """rp_rotation_consensus: dt = float64 the reference, float32 the restatement; x1, x2 [n,P,2], w [n,P] or None, tau a number or [n]"""
    n, P = x1.shape[:2]
    f = np.dtype(dt).type
    tau = np.broadcast_to(np.asarray(tau, np.float64), (n,))
    wc = C.clamp(w, n, P, dt)
    pos, samples = sample_rows2(w, n, P, seed, M, first)
    out = Consensus(np.zeros((n, 3, 3), dt), np.full(n, -1, np.int64), np.zeros((n, 4), dt), wc.copy(), np.zeros((n, M, 3, 3), dt),
                    np.full((n, M), FLT_MAX, dt), samples, np.zeros((n, M)))
    for b in range(n):
        K = len(pos[b])
        out.stat[b, 3] = K
        if K < 2 or not tau[b] > 0:
            continue
        a, c = x1[b].astype(dt), x2[b].astype(dt)
        Rm, valid, span = minimal(a[samples[b]], c[samples[b]], lapack=dt == np.float64)
        cs = cost(Rm, a[pos[b]], c[pos[b]], wc[b][pos[b]], tau[b])
        valid = valid & (cs < FLT_MAX)
        out.hyp_R[b] = np.where(valid[:, None, None], Rm, 0)
        out.hyp_cost[b] = np.where(valid, cs, FLT_MAX)
        out.span[b] = span
        out.stat[b, 2] = valid.sum()
        if not valid.any():
            continue
        win = int(np.argmin(out.hyp_cost[b]))
        out.best[b], out.R[b] = win, out.hyp_R[b, win]
        d = distance(out.R[b], a, c)
        t2 = f(tau[b]) * f(tau[b])
        out.stat[b, 0] = out.hyp_cost[b, win]
        out.stat[b, 1] = (wc[b] * (d <= t2)).sum() / wc[b].sum()
        out.weights[b] = wc[b] / (1 + d / t2)
    return out


# ------------------------------------------------------------------------------------------------ entry point 2
def _cholesky_step(N, g, lam):
    """(N + lam diag N) delta = -g in the diagonally scaled form, the loops of lm_cholesky_solve, in N's dtype -> delta or None"""
    f = N.dtype.type
    k = len(g)
    dg = np.diag(N)
    if not ((dg > 0) & (dg <= f(FINITE))).all():
        return None
    sc = f(1) / np.sqrt(dg)
    rhs = g * sc
    L = np.zeros((k, k), N.dtype)
    for j in range(k):
        p = f(1) + f(lam)
        for m in range(j):
            p = p - L[j, m] * L[j, m]
        if not (p > 0 and p <= f(FINITE)):
            return None
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, k):
            v = N[i, j] * sc[i] * sc[j]
            for m in range(j):
                v = v - L[i, m] * L[j, m]
            L[i, j] = v / L[j, j]
    y, z = np.zeros(k, N.dtype), np.zeros(k, N.dtype)
    for i in range(k):
        v = rhs[i]
        for m in range(i):
            v = v - L[i, m] * y[m]
        y[i] = v / L[i, i]
    for i in range(k - 1, -1, -1):
        v = y[i]
        for m in range(i + 1, k):
            v = v - L[m, i] * z[m]
        z[i] = v / L[i, i]
    delta = -(z * sc)
    return delta if np.isfinite(delta).all() else None


def normal_equations(h, a, c, wc, t2):
    """(N [3,3], g [3]) of the header at h [9], in h's dtype"""
    f = h.dtype.type
    x, y, u, v = a[:, 0], a[:, 1], c[:, 0], c[:, 1]
    with np.errstate(all="ignore"):
        m0, m1, m2 = h[0] * x + h[1] * y + h[2], h[3] * x + h[4] * y + h[5], h[6] * x + h[7] * y + h[8]
        ex, ey, den = m0 - u * m2, m1 - v * m2, m2 * m2
        ok = (m2 > 0) & (den >= f(DEN_MIN))
        inv = np.where(ok, f(1) / np.where(ok, m2, f(1)), f(0))
        d = np.where(m2 > 0, np.fmin((ex * ex + ey * ey) / np.maximum(den, f(DEN_MIN)), f(D_MAX)), f(D_MAX))
        om = np.where(ok, wc / (f(1) + d / t2), f(0))
    rx, ry, px, py = ex * inv, ey * inv, m0 * inv, m1 * inv
    Jx = np.stack([-(px * py), f(1) + px * px, -py], -1)
    Jy = np.stack([-(f(1) + py * py), px * py, px], -1)
    N = (om[:, None, None] * (Jx[:, :, None] * Jx[:, None, :] + Jy[:, :, None] * Jy[:, None, :])).sum(0, dtype=h.dtype)
    g = (om[:, None] * (Jx * rx[:, None] + Jy * ry[:, None])).sum(0, dtype=h.dtype)
    return N, g


def retract(q, delta):
    """unit((delta / 2, 1) (x) q) with w >= 0, the header's product, in q's dtype -> (q', ok)"""
    f = q.dtype.type
    px, py, pz = delta[0] / f(2), delta[1] / f(2), delta[2] / f(2)
    v = np.array([((q[0] + px * q[3]) + py * q[2]) - pz * q[1], ((q[1] - px * q[2]) + py * q[3]) + pz * q[0],
                  ((q[2] + px * q[1]) - py * q[0]) + pz * q[3], ((q[3] - px * q[0]) - py * q[1]) - pz * q[2]], q.dtype)
    u, nrm = unit(v[None])
    if not (nrm[0] > 0 and nrm[0] <= f(FINITE)):
        return q, False
    u = u[0]
    return (-u if u[3] < 0 else u), True


def start(R0, dt):
    """(q, R) the state of the header for the start R0 [3,3], or None for a degenerate one"""
    f = np.dtype(dt).type
    h0 = np.asarray(R0, dt).reshape(9)
    if not np.isfinite(h0).all():
        return None
    ss = f(0)
    for i in range(9):
        ss = ss + h0[i] * h0[i]
    nrm = np.sqrt(ss)
    if not (nrm >= f(MIN_SCALE) and nrm <= f(FINITE)):
        return None
    q = H.rot_to_quat(((h0 / nrm) * f(np.sqrt(3.0))).astype(dt))
    return q, H.quat_to_rot(q).astype(dt)


def refine(x1, x2, w, tau, R0, iters, dt=np.float64):
    """rp_rotation_refine -> Refined(R [n,3,3], pose [n,7], stat [n,4], weights [n,P], kappa [n]: the condition number of the scaled
    normal matrix at the start)"""
    n, P = x1.shape[:2]
    f = np.dtype(dt).type
    tau = np.broadcast_to(np.asarray(tau, np.float64), (n,))
    wc = C.clamp(w, n, P, dt)
    out = Refined(np.array(R0, dt).reshape(n, 3, 3).copy(), np.zeros((n, 7), dt), np.zeros((n, 4), dt), wc.copy(), np.full(n, np.nan))
    for b in range(n):
        K = int((wc[b] > 0).sum())
        out.stat[b, 3] = K
        st = start(R0[b], dt)
        if st is None or K < 2 or not tau[b] > 0:
            continue
        q, h = st
        a, c = x1[b].astype(dt), x2[b].astype(dt)
        t2 = f(tau[b]) * f(tau[b])
        cst = lambda hh: (wc[b] * (t2 * np.log1p(distance(hh.reshape(3, 3), a, c) / t2))).sum(dtype=dt) / wc[b].sum(dtype=dt)   # noqa: E731
        cur, lam, acc = cst(h), LAMBDA0, 0
        for it in range(iters):
            N, g = normal_equations(h.reshape(9), a, c, wc[b], t2)
            if it == 0:
                with np.errstate(all="ignore"):
                    out.kappa[b] = H.scaled_condition(N)
            delta = _cholesky_step(N, g, lam)
            solved = delta is not None
            q1 = q
            if solved:
                q1, solved = retract(q, delta.astype(dt))
            h1 = H.quat_to_rot(q1).astype(dt)
            ct = cst(h1) if solved else cur
            if solved and ct < cur:
                q, h, cur, lam, acc = q1, h1, ct, max(lam / 10, LAMBDA_MIN), acc + 1
            else:
                lam = min(lam * 10, LAMBDA_MAX)
        d = distance(h.reshape(3, 3), a, c)
        out.R[b] = h.reshape(3, 3)
        out.pose[b, 3:] = q
        out.stat[b, :3] = cur, (wc[b] * (d <= t2)).sum(dtype=dt) / wc[b].sum(dtype=dt), acc
        out.weights[b] = wc[b] / (1 + d / t2)
    return out


# ------------------------------------------------------------------------------------------------ scenes
Scene = collections.namedtuple("Scene", "x1 x2 R inlier")


def axis_angle(axis, angle):
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def rotation_scene(seed, P=576, outliers=0.3, sigma=1e-3, max_angle=1.2, half=1.0, fixed_angle=None):
    """the pure-rotation recipe of DESIGN.md 5.11: axis uniform on the sphere, angle uniform in [0.1, max_angle] (fixed_angle: that
    angle instead); x1 uniform in |xy| <= half, kept only if R x1h has m_z > 0.2 and lands within `half` in image 2 (both views see the
    point); Gaussian noise `sigma` on both images; a share `outliers` of x2 replaced by points uniform in |xy| <= half.  No seed is
    rejected.  x1, x2 float32 [1,P,2]"""
    rng = np.random.default_rng(12000 + seed)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    angle = rng.uniform(0.1, max_angle)
    if fixed_angle is not None:
        angle = fixed_angle
    Rm = axis_angle(axis, angle)
    kept = np.zeros((0, 2))
    while len(kept) < P:
        xy = rng.uniform(-half, half, (4096, 2))
        m = np.concatenate([xy, np.ones((len(xy), 1))], -1) @ Rm.T
        ok = (m[:, 2] > 0.2) & (np.abs(m[:, 0]) <= half * m[:, 2]) & (np.abs(m[:, 1]) <= half * m[:, 2])
        kept = np.concatenate([kept, xy[ok]])
    xy = kept[:P]
    m = np.concatenate([xy, np.ones((P, 1))], -1) @ Rm.T
    x1 = xy[None] + sigma * rng.standard_normal((1, P, 2))
    x2 = (m[:, :2] / m[:, 2:])[None] + sigma * rng.standard_normal((1, P, 2))
    bad = rng.permutation(P)[:int(round(outliers * P))]
    x2[0, bad] = rng.uniform(-half, half, (len(bad), 2))
    inlier = np.ones(P, bool)
    inlier[bad] = False
    return Scene(x1.astype(np.float32), x2.astype(np.float32), Rm, inlier)


def exact_scenes(n, P, seed, fixed_angle=None):
    """n exact pure-rotation scenes of P points (no noise, no outliers), float32 inputs: (x1, x2 [n,P,2], R_true [n,3,3]).  For P = 2 the
    two rows are the pair, among 16 points of the scene, whose bearings span the widest angle: a minimal sample that is well apart"""
    x1, x2, Rs = [], [], []
    for b in range(n):
        s = rotation_scene(1000 * seed + b, max(P, 16) if P == 2 else P, 0.0, 0.0, fixed_angle=fixed_angle)
        a, c = s.x1[0], s.x2[0]
        if P == 2:
            ba = bearings(a.astype(np.float64))
            sp = np.linalg.norm(np.cross(ba[:, None], ba[None, :]), axis=-1)
            i, j = np.unravel_index(np.argmax(sp), sp.shape)
            a, c = a[[i, j]], c[[i, j]]
        x1.append(a), x2.append(c), Rs.append(s.R)
    return np.stack(x1), np.stack(x2), np.stack(Rs)


def angle_deg(Ra, Rb):
    """the angle of Ra^T Rb in degrees"""
    return float(np.degrees(np.arccos(np.clip((np.trace(np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)) - 1) / 2, -1, 1))))


def nearest_rotation(Hm):
    """the rotation nearest to the homography Hm [3,3] (any scale and sign): U diag(1, 1, det) V^T of the sign with a positive determinant"""
    Hm = np.asarray(Hm, np.float64)
    Hm = Hm if np.linalg.det(Hm) >= 0 else -Hm
    U, _, Vt = np.linalg.svd(Hm)
    return U @ np.diag([1, 1, np.linalg.det(U @ Vt)]) @ Vt


# ------------------------------------------------------------------------------------------------ the cases, the ratios and their constants
# The shapes of _homography_ref.EXACT with 2 for the minimum: the minimal sample, the 256-thread and the 7-rows-per-thread boundaries in
# P, the workgroup boundaries in M, the maximum.
EXACT = [(1, 2, 1), (3, 3, 255), (1, 8, 256), (3, 9, 257), (130, 64, 16), (1, 256, 1024), (3, 257, 16), (1, 512, 16), (3, 513, 16), (1, 1728, 40)]
CASES = [("exact", n, P, M, wt) for n, P, M in EXACT for wt in (False, True)] + [("noisy", 10, 576, 256, wt) for wt in (False, True)] + \
        [("large", 6, 64, 64, wt) for wt in (False, True)]
SPAN_CMP = 1e-2           # a hypothesis is compared where both cross products of the reference's bearings are at least this
LEFT_OUT_MAX = 0.05
_CACHE = {}


def inputs(kind, n, P, M, weighted):
    """float32 x1, x2 [n,P,2], w [n,P] or None: exact scenes, the ten 50 % noisy ones, or exact scenes with the angle fixed at 1.2 rad
    (rows near the field's edge, m_z small).  weighted: uniform(0.05, 1) with, from P = 24 on, 40 % zeros, a negative one and a NaN per
    problem"""
    key = ("in", kind, n, P, weighted)
    if key not in _CACHE:
        if kind == "noisy":
            sc = [rotation_scene(s, P, 0.5) for s in range(n)]
            x1, x2 = np.concatenate([s.x1 for s in sc]), np.concatenate([s.x2 for s in sc])
        elif kind == "large":
            x1, x2 = exact_scenes(n, P, 13, fixed_angle=1.2)[:2]
        else:
            x1, x2 = exact_scenes(n, P, 11)[:2]
        w = None
        if weighted:
            rng = np.random.default_rng(P + n)
            w = rng.uniform(0.05, 1.0, (n, P)).astype(np.float32)
            if P >= 24:
                w[rng.uniform(size=w.shape) < 0.4] = 0
                w[:, 5], w[:, 11] = -0.5, np.nan
        _CACHE[key] = (x1, x2, w)
    return _CACHE[key]


def reference(kind, n, P, M, weighted):
    key = ("ref", kind, n, P, M, weighted)
    if key not in _CACHE:
        x1, x2, w = inputs(kind, n, P, M, weighted)
        _CACHE[key] = consensus(x1, x2, w, TAU, SEED, M)
    return _CACHE[key]


def cost64(Rm, x1, x2, wc, tau):
    """the fp64 robust cost of Rm [n,3,3] or [n,M,3,3] per problem (and hypothesis)"""
    Rm = np.asarray(Rm, np.float64)
    out = []
    for b in range(len(Rm)):
        with np.errstate(all="ignore"):
            t2 = float(tau) ** 2
            d = distance(Rm[b], x1[b].astype(np.float64), x2[b].astype(np.float64))
            out.append((wc[b] * t2 * np.log1p(d / t2)).sum(-1) / wc[b].sum())
    return np.stack(out)


def horizon(Rm, x1, x2, wc, tau):
    """_homography_ref.horizon for the distance of this header: a row whose m_z = r3 . x1h is within rounding of 0 -- its d carries a
    relative error of about 4 rho, rho = 2 eps32 mu / |m_z|, mu = |r6 x| + |r7 y| + |r8|, and once rho reaches 1 it may fall on either
    side of the horizon, where the distance is the maximum: the row's term moves by at most min(tau^2, d) min(4 rho, 80)"""
    Rm = np.asarray(Rm, np.float64)
    out = []
    for b in range(len(Rm)):
        h = Rm[b].reshape(Rm[b].shape[:-2] + (1, 9))
        x, y = x1[b][:, 0].astype(np.float64), x1[b][:, 1].astype(np.float64)
        with np.errstate(all="ignore"):
            mz = h[..., 6] * x + h[..., 7] * y + h[..., 8]
            mu = np.abs(h[..., 6] * x) + np.abs(h[..., 7] * y) + np.abs(h[..., 8])
            rho = np.where(mz != 0, 2 * EPS32 * mu / np.where(mz != 0, np.abs(mz), 1), np.inf)
            d = distance(Rm[b], x1[b].astype(np.float64), x2[b].astype(np.float64))
            out.append((wc[b] * np.minimum(float(tau) ** 2, d) * np.minimum(4 * rho, 80)).sum(-1) / wc[b].sum())
    return np.stack(out)


cost_bound = H.cost_bound


def orthonormality(Rm):
    """max |R^T R - I| per matrix of Rm [...,3,3], fp64"""
    Rm = np.asarray(Rm, np.float64)
    return np.abs(np.swapaxes(Rm, -1, -2) @ Rm - np.eye(3)).max((-1, -2))


def consensus_ratios(out, ref, x1, x2, w, tau=TAU):
    """out: a Consensus-like tuple of numpy arrays (the device's or the restatement's), ref: the fp64 Consensus of the same inputs ->
    the ratios of the bounds: R (Frobenius error over eps32 / min(|a_0 x a_1|, |b_0 x b_1|) on the compared hypotheses), orth (max
    |R^T R - I| over eps32 on the valid ones), cost and w (against the fp64 values at out's OWN R), and the compared share"""
    n, P = x1.shape[:2]
    wc = C.clamp(w, n, P)
    valid = ref.hyp_cost < FLT_MAX
    compared = valid & (ref.span >= SPAN_CMP)
    ovalid = out.hyp_cost < FLT_MAX
    assert np.array_equal(ovalid[compared], valid[compared]), "validity differs on a compared hypothesis"
    err = np.linalg.norm((out.hyp_R.astype(np.float64) - ref.hyp_R).reshape(valid.shape + (9,)), axis=-1)
    rR = (err / (EPS32 / np.where(compared, ref.span, 1)))[compared]
    ro = (orthonormality(out.hyp_R) / EPS32)[ovalid]
    own = cost64(out.hyp_R, x1, x2, wc, tau)
    both = ovalid & np.isfinite(own)
    hor = horizon(out.hyp_R, x1, x2, wc, tau)
    rc = (np.abs(out.hyp_cost.astype(np.float64) - own) / cost_bound(np.where(both, own, 1), 1.0, hor))[both]
    won = out.best >= 0
    rw = np.zeros(0)
    if won.any():
        t2 = float(tau) ** 2
        want = np.stack([wc[b] / (1 + distance(out.R[b].astype(np.float64), x1[b].astype(np.float64), x2[b].astype(np.float64)) / t2)
                         for b in np.flatnonzero(won)])
        rw = (np.abs(out.weights[won].astype(np.float64) - want) / np.where(wc[won] > 0, wc[won], 1) / (EPS32 / tau))[wc[won] > 0]
    return dict(R=float(rR.max(initial=0)), orth=float(ro.max(initial=0)), cost=float(rc.max(initial=0)), w=float(rw.max(initial=0)),
                compared=float(compared.sum() / max(valid.sum(), 1)))


def check_consensus(out, ref, x1, x2, w, tau=TAU):
    """the device's rp_rotation_consensus against the reference, at the calibrated bounds; returns the ratios"""
    n, P = x1.shape[:2]
    wc = C.clamp(w, n, P)
    r = consensus_ratios(out, ref, x1, x2, w, tau)
    print("R ratio %.3g (C %.3g), orthonormality %.3g (C %.3g), cost ratio %.3g (C %.3g), w ratio %.3g (C %.3g), compared %.4f"
          % (r["R"], C_R, r["orth"], C_ORTH, r["cost"], C_COST, r["w"], C_W, r["compared"]))
    assert r["compared"] >= 1 - LEFT_OUT_MAX
    assert r["R"] <= C_R and r["orth"] <= C_ORTH and r["cost"] <= C_COST and r["w"] <= C_W, r
    K = (wc > 0).sum(-1)
    assert np.array_equal(out.stat[:, 3], K) and np.array_equal(out.stat[:, 2], (out.hyp_cost < FLT_MAX).sum(-1))
    for b in range(n):
        if K[b] < 2 or not (out.hyp_cost[b] < FLT_MAX).any():
            assert out.best[b] == -1 and not out.R[b].any() and not out.stat[b, :2].any()
            assert np.array_equal(out.weights[b], wc[b].astype(np.float32))
            continue
        win = int(np.argmin(out.hyp_cost[b]))                        # the lowest index of the device's own minimum, exactly
        assert out.best[b] == win and np.array_equal(out.R[b], out.hyp_R[b, win]) and out.stat[b, 0] == out.hyp_cost[b, win]
        # against the reference the winner is compared by COST: the device's winner costs (fp64, its own R) no more than the device's
        # version of the reference's winner, up to the two cost bounds
        pair = out.hyp_R[b:b + 1, [win, int(ref.best[b])]]
        own = cost64(pair, x1[b:b + 1], x2[b:b + 1], wc[b:b + 1], tau)[0]
        hor = horizon(pair, x1[b:b + 1], x2[b:b + 1], wc[b:b + 1], tau)[0]
        assert own[0] <= own[1] + cost_bound(own[0], C_COST, hor[0]) + cost_bound(own[1], C_COST, hor[1]), (b, own)
        t2 = float(tau) ** 2
        u = distance(out.R[b].astype(np.float64), x1[b].astype(np.float64), x2[b].astype(np.float64)) / t2
        share, band = (wc[b] * (u <= 1)).sum() / wc[b].sum(), (wc[b] * (np.abs(u - 1) < 1e-4)).sum() / wc[b].sum()
        assert abs(out.stat[b, 1] - share) <= band + 1e-5, (b, out.stat[b, 1], share, band)
    return r


# refinement: the reference's kappa scales the bound, one step and converged
REFINE_CASES = [("noisy", 10, 576, False), ("noisy", 10, 576, True), ("noisy", 3, 257, True), ("noisy", 1, 1728, False), ("noisy", 2, 3, False),
                ("large", 6, 64, False)]


def refine_inputs(kind, n, P, weighted):
    """(x1, x2, w, R0 float32): noisy 30 % scenes (exact ones below P = 24; "large": exact ones with the angle fixed at 1.2 rad) and the
    reference consensus winner (M = 64) rounded to float32 as the start"""
    key = ("rin", kind, n, P, weighted)
    if key not in _CACHE:
        if kind == "large":
            x1, x2 = exact_scenes(n, P, 13, fixed_angle=1.2)[:2]
        else:
            sc = [rotation_scene(40 + s, P, 0.3 if P >= 24 else 0.0, 1e-3 if P >= 24 else 0.0) for s in range(n)]
            x1, x2 = np.concatenate([s.x1 for s in sc]), np.concatenate([s.x2 for s in sc])
        w = None
        if weighted:
            rng = np.random.default_rng(P + n)
            w = rng.uniform(0.05, 1.0, (n, P)).astype(np.float32)
            w[rng.uniform(size=w.shape) < 0.4] = 0
            w[:, 5], w[:, 11] = -0.5, np.nan
        R0 = consensus(x1, x2, w, TAU, SEED, 64).R.astype(np.float32)
        _CACHE[key] = (x1, x2, w, R0)
    return _CACHE[key]


def refine_reference(kind, n, P, weighted, iters):
    key = ("rref", kind, n, P, weighted, iters)
    if key not in _CACHE:
        x1, x2, w, R0 = refine_inputs(kind, n, P, weighted)
        _CACHE[key] = refine(x1, x2, w, TAU, R0, iters)
    return _CACHE[key]


def refine_ratios(Rm, pose, stat, weights, ref, x1, x2, w, tau=TAU):
    """R: Frobenius error over eps32 kappa; pose: max |quat_to_rot(q) - R| and | |q| - 1 | over eps32; cost and weights against fp64 at
    the output's own R"""
    n, P = x1.shape[:2]
    wc = C.clamp(w, n, P)
    kap = np.where(np.isfinite(ref.kappa), ref.kappa, 1.0)
    rR = np.linalg.norm((Rm.astype(np.float64) - ref.R).reshape(n, 9), axis=-1) / (EPS32 * kap)
    q = pose[:, 3:].astype(np.float64)
    rp = np.array([max(np.abs(H.quat_to_rot(q[b]) - Rm[b]).max(), abs(np.linalg.norm(q[b]) - 1)) for b in range(n)]) / EPS32
    own = cost64(Rm, x1, x2, wc, tau)
    rc = np.abs(stat[:, 0].astype(np.float64) - own) / cost_bound(own, 1.0, horizon(Rm, x1, x2, wc, tau))
    t2 = float(tau) ** 2
    want = np.stack([wc[b] / (1 + distance(Rm[b].astype(np.float64), x1[b].astype(np.float64), x2[b].astype(np.float64)) / t2) for b in range(n)])
    rw = (np.abs(weights.astype(np.float64) - want) / np.where(wc > 0, wc, 1) / (EPS32 / tau))[wc > 0]
    return dict(R=float(rR.max()), pose=float(rp.max()), cost=float(rc.max()), w=float(rw.max(initial=0)))


# 8 x the restatement's worst ratio on these same inputs (tests/test_rotation_cpu.py asserts the restatement within C / 8 and above
# 0.9 C / 8: the constants are these figures, not looser ones)
C_R, C_ORTH, C_COST, C_W = 24.3, 40.6, 7.08, 5.81        # the restatement: 3.025, 5.066, 0.884, 0.725
C_REFINE_R = {1: 10.2, 10: 197.0}                      # one step 1.266; converged 24.50: float32 stops accepting steps short of where fp64 ends
C_POSE = 5.53                                          # 0.690: quat_to_rot(q) against R, | |q| - 1 |, in eps32
C_START, C_START_SCALED = 12.0, 16.0                   # iters = 0: the normalised R0 against R0 1.5 eps32, against that of 2.5 R0 2.0
WORST = dict(R=3.025, orth=5.066, cost=0.884, w=0.725, refine1=1.266, refine10=24.50, pose=0.690)
# the "what it does" table of the fp64 reference (table(f), seeds 0 - 9, M = 256, 10 iterations): the worst rotation error in degrees per
# share of wrong matches; tests/test_rotation_cpu.py asserts every scene within twice that
TABLE_WORST_DEG = {0.3: 0.0118, 0.5: 0.0110, 0.7: 0.0174, 0.8: 0.0277}


# ------------------------------------------------------------------------------------------------ the rotation chain and its tables
OUTLIERS = (0.3, 0.5, 0.7, 0.8)
Row = collections.namedtuple("Row", "error consensus_error share homography_error scene")


def table(outliers, seeds=range(10), M=256, iters=10):
    """per scene of the recipe at the share `outliers` of wrong matches, all fp64: the rotation error (degrees) after consensus + `iters`
    refinement iterations on the base weights, after the consensus alone, the inlier share of the refined rotation, and the error of the
    rotation nearest to the homography of _homography_ref's planar chain (its consensus -> its refine, the calls of
    _homography_ref.chain with its M, seed and tau; the decomposition behind them has no translation to compare on these scenes)"""
    key = ("table", outliers, tuple(seeds), M, iters)
    if key not in _CACHE:
        rows = []
        for s in seeds:
            sc = rotation_scene(s, 576, outliers)
            c = consensus(sc.x1, sc.x2, None, TAU, SEED, M)
            r = refine(sc.x1, sc.x2, None, TAU, c.R, iters)
            hc = H.consensus(sc.x1, sc.x2, None, H.TAU, H.SEED, M)
            hr = H.refine(sc.x1, sc.x2, None, H.TAU, hc.H, iters)
            he = angle_deg(nearest_rotation(hr.H[0]), sc.R) if hc.best[0] >= 0 else 180.0
            rows.append(Row(angle_deg(r.R[0], sc.R), angle_deg(c.R[0], sc.R), float(r.stat[0, 1]), he, sc))
        _CACHE[key] = rows
    return _CACHE[key]


def translating_shares(outliers, seeds=range(10), M=256, iters=10):
    """the inlier share of the refined best rotation on scenes that TRANSLATE, at the same share of wrong matches:
    (_eightpoint_ref.noisy_scene [len(seeds)], _homography_ref.plane_scene [len(seeds)])"""
    from tests import _eightpoint_ref as R8
    key = ("shares", outliers, tuple(seeds), M, iters)
    if key not in _CACHE:
        out = ([], [])
        for s in seeds:
            for k, (x1, x2) in enumerate((R8.noisy_scene(s, 576, outliers)[:2], H.plane_scene(s, 576, outliers)[:2])):
                c = consensus(x1, x2, None, TAU, SEED, M)
                out[k].append(float(refine(x1, x2, None, TAU, c.R, iters).stat[0, 1]))
        _CACHE[key] = (np.array(out[0]), np.array(out[1]))
    return _CACHE[key]


def essential_rotations(E):
    """the two rotations U W V^T, U W^T V^T of an essential matrix [3,3]"""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64))
    U, Vt = (U if np.linalg.det(U) > 0 else -U), (Vt if np.linalg.det(Vt) > 0 else -Vt)
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    return U @ W @ Vt, U @ W.T @ Vt


def eight_point_chain_errors(outliers, seeds=range(10), M=1024, iters=4):
    """what the essential-matrix chain already does on the rotation scenes, fp64: _consensus_ref.consensus_ref (M hypotheses) ->
    _eightpoint_ref.eight_point_ref(iters) on its weights; the rotation error in degrees of the NEARER of E's two rotations -- the
    cheirality vote between them has nothing to vote on when t = 0, so this is the chain at its best"""
    from tests import _eightpoint_ref as R8
    key = ("eight", outliers, tuple(seeds), M, iters)
    if key not in _CACHE:
        errs = []
        for s in seeds:
            sc = rotation_scene(s, 576, outliers)
            c = C.consensus_ref(sc.x1, sc.x2, None, TAU, SEED, M)
            E = R8.eight_point_ref(sc.x1, sc.x2, c.weights, np.full(1, TAU), iters=iters)[0]
            errs.append(min(angle_deg(r, sc.R) for r in essential_rotations(E[0])))
        _CACHE[key] = np.array(errs)
    return _CACHE[key]
