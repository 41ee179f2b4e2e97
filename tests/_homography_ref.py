"""References for include/relpose_homography.h (librelpose_homography.so), shared by tests/test_homography_cpu.py,
tests/test_gpu_homography.py and tests/test_gpu_homography_contract.py.

Every routine is written ONCE, over a dtype: with float64 (and LAPACK for the null vector and the 3 x 3 SVD) it is the reference, with
float32 (and the kernel's Householder null vector, the kernel's order of operations) it is the restatement of the kernels' arithmetic
that calibrates the GPU bounds -- the project's rule: a bound is C eps32 scale(ref) with C = 8 x the restatement's worst ratio on the
same inputs.  The decomposition is checked against a second route (the eigen-decomposition of H^T H).  Scene builders: the one-plane
recipe of DESIGN.md 5.7, its off-plane variant, exact scenes and the edge scenes of the decomposition."""
import collections

import numpy as np

from tests import _consensus_ref as C
from tests import _eightpoint_ref as R

FLT_MAX = C.FLT_MAX
EPS32 = float(np.finfo(np.float32).eps)
MIN_SCALE, DEN_MIN, D_MAX, FINITE = 1e-30, 1e-30, 1e30, 3.0e38
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-7, 1e7
ROTATION_GAP, RANK_MIN = 1e-4, 1e-6
TAU, SEED = 0.01, 1

Consensus = collections.namedtuple("Consensus", "H best stat weights hyp_H hyp_cost samples cond")
Refined = collections.namedtuple("Refined", "H stat weights kappa")
Poses = collections.namedtuple("Poses", "pose normal cstat pick sigma")


# ------------------------------------------------------------------------------------------------ the sampler
def draw4(seed, i, m, K):
    """the four indices c_0 .. c_3 into pos of hypotheses m (an int array) of problem i: [len(m), 4]; K >= 4"""
    m = np.atleast_1d(np.asarray(m, np.uint64))
    base = C.mix((np.uint64(seed & 0xFFFFFFFF) + np.uint64(C.GOLDEN) * np.uint64(i + 1)) & np.uint64(0xFFFFFFFF))
    s = C.mix(base ^ m)
    c = np.zeros((len(m), 4), np.int64)
    for k in range(4):
        r = C.mix((s + np.uint64((C.GOLDEN * (k + 1)) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF))
        j = K - 4 + k
        t = ((r * np.uint64(j + 1)) >> np.uint64(32)).astype(np.int64)
        seen = (c[:, :k] == t[:, None]).any(-1)
        c[:, k] = np.where(seen, j, t)
    return c


def sample_rows4(w, n, P, seed, M, first=0):
    """(pos per problem, samples [n,M,4] of row numbers; zeros where K < 4); problem b of the batch has index first + b"""
    wc = C.clamp(w, n, P)
    pos = [np.flatnonzero(wc[b] > 0) for b in range(n)]
    samples = np.zeros((n, M, 4), np.int64)
    for b in range(n):
        if len(pos[b]) >= 4:
            samples[b] = pos[b][draw4(seed, first + b, np.arange(M), len(pos[b]))]
    return pos, samples


# ------------------------------------------------------------------------------------------------ shared arithmetic, over a dtype
def transfer(H, a, b):
    """the clamped squared transfer distance: H [...,3,3] (dtype decides), a, b [P,2] -> [...,P]"""
    f = H.dtype.type
    h = H.reshape(H.shape[:-2] + (1, 9))
    x, y, u, v = a[:, 0].astype(f), a[:, 1].astype(f), b[:, 0].astype(f), b[:, 1].astype(f)
    with np.errstate(all="ignore"):
        m0 = h[..., 0] * x + h[..., 1] * y + h[..., 2]
        m1 = h[..., 3] * x + h[..., 4] * y + h[..., 5]
        m2 = h[..., 6] * x + h[..., 7] * y + h[..., 8]
        ex, ey = m0 - u * m2, m1 - v * m2
        return np.fmin((ex * ex + ey * ey) / np.maximum(m2 * m2, f(DEN_MIN)), f(D_MAX))


def _seqsum(t):
    """sum over the last axis; float32: one term after the other, as a lane of the hypothesis kernel adds them"""
    if t.dtype != np.float32:
        return t.sum(-1)
    acc = np.zeros(t.shape[:-1], np.float32)
    for j in range(t.shape[-1]):
        acc = acc + t[..., j]
    return acc


def cost(H, a, b, w, tau):
    """the robust transfer cost of H [...,3,3] on the rows a, b [K,2] with weights w [K] (already clamped, in H's dtype)"""
    f = H.dtype.type
    t2 = f(tau) * f(tau)
    with np.errstate(all="ignore"):
        return _seqsum(w * (t2 * np.log1p(transfer(H, a, b) / t2))) / _seqsum(w)


def frob_sign(h, sign=True):
    """h [S,9] -> (h / |h|_F with the sign rule, ok [S])"""
    f = h.dtype.type
    with np.errstate(all="ignore"):
        ss = np.zeros(len(h), h.dtype)
        for i in range(9):
            ss = ss + h[:, i] * h[:, i]
        nrm = np.sqrt(ss)
        ok = (nrm >= f(MIN_SCALE)) & (nrm <= f(FINITE))
        h = h / np.where(ok, nrm, f(1))[:, None]
    if sign:
        lead = h[np.arange(len(h)), np.argmax(np.abs(h), -1)]                  # argmax: the first of equal ones
        h = np.where((lead < 0)[:, None], -h, h)
    return h, ok


def _normalise4(p):
    f = p.dtype.type
    sx, sy = np.zeros(len(p), p.dtype), np.zeros(len(p), p.dtype)
    for k in range(4):
        sx, sy = sx + (p[:, k, 0] - p[:, 0, 0]), sy + (p[:, k, 1] - p[:, 0, 1])
    cx, cy = p[:, 0, 0] + sx / f(4), p[:, 0, 1] + sy / f(4)
    m = np.zeros(len(p), p.dtype)
    for k in range(4):
        dx, dy = p[:, k, 0] - cx, p[:, k, 1] - cy
        m = m + np.sqrt(dx * dx + dy * dy)
    m = m / f(4)
    ok = m >= f(MIN_SCALE)
    return cx, cy, np.sqrt(f(2)) / np.where(ok, m, f(1)), ok


def householder_null(A):
    """the null vector of A [S,8,9] by the kernel's eight Householder reflections of the transpose, in A's dtype"""
    A = A.copy()
    S = len(A)
    beta = np.zeros((S, 8), A.dtype)
    with np.errstate(all="ignore"):
        for j in range(8):
            sig = np.zeros(S, A.dtype)
            for i in range(j, 9):
                sig = sig + A[:, j, i] * A[:, j, i]
            nrm = np.sqrt(sig)
            den = sig + np.abs(A[:, j, j]) * nrm
            beta[:, j] = np.where(den > 0, 1 / np.where(den > 0, den, 1), 0)
            A[:, j, j] += np.copysign(nrm, A[:, j, j])
            for k in range(j + 1, 8):
                t = np.zeros(S, A.dtype)
                for i in range(j, 9):
                    t = t + A[:, j, i] * A[:, k, i]
                t = t * beta[:, j]
                for i in range(j, 9):
                    A[:, k, i] -= t * A[:, j, i]
        f = np.zeros((S, 9), A.dtype)
        f[:, 8] = 1
        for j in range(7, -1, -1):
            t = np.zeros(S, A.dtype)
            for i in range(j, 9):
                t = t + A[:, j, i] * f[:, i]
            t = t * beta[:, j]
            for i in range(j, 9):
                f[:, i] -= t * A[:, j, i]
    return f


def minimal(p1, p2, lapack):
    """the four-point DLT of the header on samples p1, p2 [S,4,2] (their dtype decides) -> (H [S,3,3], valid [S], sigma_1 / sigma_8 of
    the 8 x 9 matrix [S]); lapack: the null vector by SVD instead of the kernel's reflections"""
    dt = p1.dtype
    S = len(p1)
    c1x, c1y, s1, ok1 = _normalise4(p1)
    c2x, c2y, s2, ok2 = _normalise4(p2)
    A = np.zeros((S, 8, 9), dt)
    for k in range(4):
        ax, ay = (p1[:, k, 0] - c1x) * s1, (p1[:, k, 1] - c1y) * s1
        bx, by = (p2[:, k, 0] - c2x) * s2, (p2[:, k, 1] - c2y) * s2
        A[:, 2 * k, 0], A[:, 2 * k, 1], A[:, 2 * k, 2] = ax, ay, 1
        A[:, 2 * k, 6], A[:, 2 * k, 7], A[:, 2 * k, 8] = -bx * ax, -bx * ay, -bx
        A[:, 2 * k + 1, 3], A[:, 2 * k + 1, 4], A[:, 2 * k + 1, 5] = ax, ay, 1
        A[:, 2 * k + 1, 6], A[:, 2 * k + 1, 7], A[:, 2 * k + 1, 8] = -by * ax, -by * ay, -by
    A = np.where((ok1 & ok2)[:, None, None], A, 0)
    sv = np.linalg.svd(A.astype(np.float64), compute_uv=False)
    cond = sv[:, 0] / np.maximum(sv[:, 7], 1e-300)
    if lapack:
        f = np.linalg.svd(A)[2][:, 8]
    else:
        f = householder_null(A)
    f = f.reshape(S, 3, 3)
    G = np.empty_like(f)
    G[:, :, 0], G[:, :, 1] = f[:, :, 0] * s1[:, None], f[:, :, 1] * s1[:, None]
    G[:, :, 2] = f[:, :, 2] - s1[:, None] * (c1x[:, None] * f[:, :, 0] + c1y[:, None] * f[:, :, 1])
    H = np.empty_like(f)
    H[:, 0] = G[:, 0] / s2[:, None] + c2x[:, None] * G[:, 2]
    H[:, 1] = G[:, 1] / s2[:, None] + c2y[:, None] * G[:, 2]
    H[:, 2] = G[:, 2]
    fin = np.isfinite(H).all((1, 2))
    h, ok = frob_sign(np.where(fin[:, None, None], H, 0).reshape(S, 9))
    return h.reshape(S, 3, 3), ok1 & ok2 & fin & ok, cond


# ------------------------------------------------------------------------------------------------ entry point 1
def consensus(x1, x2, w=None, tau=TAU, seed=SEED, M=256, dt=np.float64, first=0):
    """rp_homography_consensus: dt = float64 the reference, float32 the restatement; x1, x2 [n,P,2], w [n,P] or None, tau a number or [n]"""
    n, P = x1.shape[:2]
    f = np.dtype(dt).type
    tau = np.broadcast_to(np.asarray(tau, np.float64), (n,))
    wc = C.clamp(w, n, P, dt)
    pos, samples = sample_rows4(w, n, P, seed, M, first)
    out = Consensus(np.zeros((n, 3, 3), dt), np.full(n, -1, np.int64), np.zeros((n, 4), dt), wc.copy(), np.zeros((n, M, 3, 3), dt),
                    np.full((n, M), FLT_MAX, dt), samples, np.full((n, M), np.inf))
    for b in range(n):
        K = len(pos[b])
        out.stat[b, 3] = K
        if K < 4 or not tau[b] > 0:
            continue
        a, c = x1[b].astype(dt), x2[b].astype(dt)
        H, valid, cond = minimal(a[samples[b]], c[samples[b]], lapack=dt == np.float64)
        cs = cost(H, a[pos[b]], c[pos[b]], wc[b][pos[b]], tau[b])
        valid = valid & (cs < FLT_MAX)
        out.hyp_H[b] = np.where(valid[:, None, None], H, 0)
        out.hyp_cost[b] = np.where(valid, cs, FLT_MAX)
        out.cond[b] = cond
        out.stat[b, 2] = valid.sum()
        if not valid.any():
            continue
        win = int(np.argmin(out.hyp_cost[b]))
        out.best[b], out.H[b] = win, out.hyp_H[b, win]
        d = transfer(out.H[b], a, c)
        t2 = f(tau[b]) * f(tau[b])
        out.stat[b, 0] = out.hyp_cost[b, win]
        out.stat[b, 1] = (wc[b] * (d <= t2)).sum() / wc[b].sum()
        out.weights[b] = wc[b] / (1 + d / t2)
    return out


# ------------------------------------------------------------------------------------------------ entry point 2
def _cholesky_step(N, g, lam):
    """(N + lam diag N) delta = -g in the diagonally scaled form, the kernel's loops, in N's dtype -> delta or None"""
    f = N.dtype.type
    dg = np.diag(N)
    if not ((dg > 0) & (dg <= f(FINITE))).all():
        return None
    sc = f(1) / np.sqrt(dg)
    rhs = g * sc
    L = np.zeros((8, 8), N.dtype)
    for j in range(8):
        p = f(1) + f(lam)
        for m in range(j):
            p = p - L[j, m] * L[j, m]
        if not (p > 0 and p <= f(FINITE)):
            return None
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, 8):
            v = N[i, j] * sc[i] * sc[j]
            for m in range(j):
                v = v - L[i, m] * L[j, m]
            L[i, j] = v / L[j, j]
    y, z = np.zeros(8, N.dtype), np.zeros(8, N.dtype)
    for i in range(8):
        v = rhs[i]
        for m in range(i):
            v = v - L[i, m] * y[m]
        y[i] = v / L[i, i]
    for i in range(7, -1, -1):
        v = y[i]
        for m in range(i + 1, 8):
            v = v - L[m, i] * z[m]
        z[i] = v / L[i, i]
    delta = -(z * sc)
    return delta if np.isfinite(delta).all() else None


def normal_equations(h, a, c, wc, t2):
    """(N [8,8], g [8]) of the header at h [9], in h's dtype"""
    f = h.dtype.type
    x, y, u, v = a[:, 0], a[:, 1], c[:, 0], c[:, 1]
    with np.errstate(all="ignore"):
        m0, m1, m2 = h[0] * x + h[1] * y + h[2], h[3] * x + h[4] * y + h[5], h[6] * x + h[7] * y + h[8]
        ex, ey, den = m0 - u * m2, m1 - v * m2, m2 * m2
        ok = den >= f(DEN_MIN)
        inv = np.where(ok, f(1) / np.where(ok, m2, f(1)), f(0))
        d = np.fmin((ex * ex + ey * ey) / np.maximum(den, f(DEN_MIN)), f(D_MAX))
        om = np.where(ok, wc / (f(1) + d / t2), f(0))
    rx, ry, px, py = ex * inv, ey * inv, m0 * inv, m1 * inv
    c0, c1, c2 = (h[0] - px * h[6]) * inv, (h[1] - px * h[7]) * inv, (h[2] - px * h[8]) * inv
    e0, e1, e2 = (h[3] - py * h[6]) * inv, (h[4] - py * h[7]) * inv, (h[5] - py * h[8]) * inv
    Jx = np.stack([y * c0, c0, x * c1, c1, x * c2, y * c2, x * c0 - y * c1, y * c1 - c2], -1)
    Jy = np.stack([y * e0, e0, x * e1, e1, x * e2, y * e2, x * e0 - y * e1, y * e1 - e2], -1)
    N = (om[:, None, None] * (Jx[:, :, None] * Jx[:, None, :] + Jy[:, :, None] * Jy[:, None, :])).sum(0, dtype=h.dtype)
    g = (om[:, None] * (Jx * rx[:, None] + Jy * ry[:, None])).sum(0, dtype=h.dtype)
    return N, g


def scaled_condition(N):
    d = 1 / np.sqrt(np.diag(N).astype(np.float64))
    return float(np.linalg.cond(N.astype(np.float64) * d[:, None] * d[None]))


def retract(h, delta):
    D = np.array([[delta[6], delta[0], delta[1]], [delta[2], delta[7] - delta[6], delta[3]], [delta[4], delta[5], -delta[7]]], h.dtype)
    Hm = h.reshape(3, 3)
    h1, ok = frob_sign((Hm + Hm @ D).reshape(1, 9), sign=False)
    return h1[0], bool(ok[0])


def refine(x1, x2, w, tau, H0, iters, dt=np.float64):
    """rp_homography_refine -> Refined(H [n,3,3], stat [n,4], weights [n,P], kappa [n]: the condition number of the scaled normal matrix
    at the start)"""
    n, P = x1.shape[:2]
    f = np.dtype(dt).type
    tau = np.broadcast_to(np.asarray(tau, np.float64), (n,))
    wc = C.clamp(w, n, P, dt)
    out = Refined(np.array(H0, dt).reshape(n, 3, 3).copy(), np.zeros((n, 4), dt), wc.copy(), np.full(n, np.nan))
    for b in range(n):
        K = int((wc[b] > 0).sum())
        out.stat[b, 3] = K
        h0 = np.asarray(H0[b], dt).reshape(1, 9)
        if not np.isfinite(h0).all() or K < 4 or not tau[b] > 0:
            continue
        h, ok = frob_sign(h0, sign=False)
        if not ok[0]:
            continue
        h = h[0]
        a, c = x1[b].astype(dt), x2[b].astype(dt)
        t2 = f(tau[b]) * f(tau[b])
        cst = lambda hh: (wc[b] * (t2 * np.log1p(transfer(hh.reshape(3, 3), a, c) / t2))).sum(dtype=dt) / wc[b].sum(dtype=dt)   # noqa: E731
        cur, lam, acc = cst(h), LAMBDA0, 0
        for it in range(iters):
            N, g = normal_equations(h, a, c, wc[b], t2)
            if it == 0:
                with np.errstate(all="ignore"):
                    out.kappa[b] = scaled_condition(N)
            delta = _cholesky_step(N, g, lam)
            solved = delta is not None
            h1 = h
            if solved:
                h1, solved = retract(h, delta)
            ct = cst(h1) if solved else cur
            if solved and ct < cur:
                h, cur, lam, acc = h1, ct, max(lam / 10, LAMBDA_MIN), acc + 1
            else:
                lam = min(lam * 10, LAMBDA_MAX)
        h = frob_sign(h.reshape(1, 9))[0][0]
        d = transfer(h.reshape(3, 3), a, c)
        out.H[b] = h.reshape(3, 3)
        out.stat[b, :3] = cur, (wc[b] * (d <= t2)).sum(dtype=dt) / wc[b].sum(dtype=dt), acc
        out.weights[b] = wc[b] / (1 + d / t2)
    return out


# ------------------------------------------------------------------------------------------------ entry point 3
def rot_to_quat(Rm):
    f = Rm.dtype.type
    R_ = Rm.reshape(9)
    tr = R_[0] + R_[4] + R_[8]
    v = np.zeros(4, Rm.dtype)
    if tr > 0:
        v[:] = R_[7] - R_[5], R_[2] - R_[6], R_[3] - R_[1], f(1) + tr
    elif R_[0] >= R_[4] and R_[0] >= R_[8]:
        v[:] = f(1) + R_[0] - R_[4] - R_[8], R_[1] + R_[3], R_[2] + R_[6], R_[7] - R_[5]
    elif R_[4] >= R_[8]:
        v[:] = R_[1] + R_[3], f(1) + R_[4] - R_[0] - R_[8], R_[5] + R_[7], R_[2] - R_[6]
    else:
        v[:] = R_[2] + R_[6], R_[5] + R_[7], f(1) + R_[8] - R_[0] - R_[4], R_[3] - R_[1]
    nrm = np.sqrt((v * v).sum(dtype=Rm.dtype))
    if not nrm > 0:
        return np.array([0, 0, 0, 1], Rm.dtype)
    return (v if v[3] >= 0 else -v) / nrm


def quat_to_rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], q.dtype)


def cross_matrix(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], t.dtype)


def _sampson(E, a, c):
    x, y, u, v = a[:, 0], a[:, 1], c[:, 0], c[:, 1]
    e = E.reshape(9)
    l2x, l2y, l2z = e[0] * x + e[1] * y + e[2], e[3] * x + e[4] * y + e[5], e[6] * x + e[7] * y + e[8]
    l1x, l1y = e[0] * u + e[3] * v + e[6], e[1] * u + e[4] * v + e[7]
    r = u * l2x + v * l2y + l2z
    den = l2x * l2x + l2y * l2y + l1x * l1x + l1y * l1y
    return np.where(den > 0, r * r / np.where(den > 0, den, 1), 0).astype(E.dtype)


def _factors(h, route):
    """(singular values descending, V columns as rows) of h [3,3]: route "svd" (LAPACK) or "eigh" (H^T H, the second route)"""
    if route == "svd":
        U, s, Vt = np.linalg.svd(h)
        return U, s, Vt
    lam, V = np.linalg.eigh(h.T @ h)
    order = np.argsort(-lam)
    s = np.sqrt(np.maximum(lam[order], 0))
    Vt = V[:, order].T
    U = (h @ Vt.T / np.maximum(s, 1e-300)).T
    return U.T, s, Vt


def decompose(H, x1, x2, w, tau, vis_min=0.99, dt=np.float64, route="svd"):
    """rp_pose_from_homography -> Poses(pose [n,4,7], normal [n,4,3], cstat [n,4,4], pick [n,2], sigma [n,2] = (sigma_1, sigma_3))"""
    n, P = x1.shape[:2]
    f = np.dtype(dt).type
    tau = np.broadcast_to(np.asarray(tau, np.float64), (n,))
    wc_ = C.clamp(w, n, P, dt)
    out = Poses(np.zeros((n, 4, 7), dt), np.zeros((n, 4, 3), dt), np.zeros((n, 4, 4), dt), np.full((n, 2), -1, np.int64), np.full((n, 2), np.nan))
    for b in range(n):
        h = np.asarray(H[b], dt).reshape(3, 3)
        if not np.isfinite(h).all() or not tau[b] > 0:
            continue
        U, s, Vt = _factors(h, route)
        if not (s[1] > 0 and s[1] >= f(RANK_MIN) * s[0]):
            continue
        h = h / s[1]
        a, c = x1[b].astype(dt), x2[b].astype(dt)
        t2 = f(tau[b]) * f(tau[b])
        wcau = wc_[b] / (1 + transfer(h, a, c) / t2)
        m = np.concatenate([a, np.ones((P, 1), dt)], -1) @ h.T
        side = (c[:, 0] * m[:, 0] + c[:, 1] * m[:, 1]) + m[:, 2]
        sgn = -1 if (wcau * np.sign(side)).sum(dtype=dt) < 0 else 1
        wcsum, wsum = wcau.sum(dtype=dt), wc_[b].sum(dtype=dt)
        if not wcsum > 0:
            continue
        h = sgn * h
        sig1, sig3 = (s[0] / s[1]) ** 2, (s[2] / s[1]) ** 2
        out.sigma[b] = sig1, sig3
        gap = sig1 - sig3
        cands = []
        if not gap >= f(ROTATION_GAP):
            uc, vc = np.cross(U[:, 0], U[:, 1]), np.cross(Vt[0], Vt[1])
            Rm = sgn * (np.outer(U[:, 0], Vt[0]) + np.outer(U[:, 1], Vt[1])) + np.outer(uc, vc)
            cands.append((np.zeros(3, dt), rot_to_quat(Rm.astype(dt)), np.zeros(3, dt), f(0), None))
        else:
            ca, cb = np.sqrt(max(1 - sig3, 0) / gap), np.sqrt(max(sig1 - 1, 0) / gap)
            v2 = Vt[1]
            hv2 = h @ v2
            for sb in (cb, -cb):
                uu = ca * Vt[0] + sb * Vt[2]
                nn = np.cross(v2, uu)
                hu = h @ uu
                Rm = np.outer(hv2, v2) + np.outer(hu, uu) + np.outer(np.cross(hv2, hu), nn)
                td = h @ nn - Rm @ nn
                q = rot_to_quat(Rm.astype(dt))
                tn = np.sqrt((td * td).sum(dtype=dt))
                tu = td / tn if tn > 0 else np.zeros(3, dt)
                for sg in (1, -1):
                    cands.append(((sg * tu).astype(dt), q, (sg * nn).astype(dt), tn, cross_matrix((sg * tu).astype(dt)) @ quat_to_rot(q)))
        vis, cst, valid = np.zeros(4), np.zeros(4), np.zeros(4, bool)
        for k, (t, q, nn, tn, E) in enumerate(cands):
            if E is None:
                vis[k], cst[k], valid[k] = 1, 0, True
            else:
                front = (nn[0] * a[:, 0] + nn[1] * a[:, 1]) + nn[2]
                vis[k] = (wcau * (front > 0)).sum(dtype=dt) / wcsum
                cst[k] = (wc_[b] * (t2 * np.log1p(_sampson(E, a, c) / t2))).sum(dtype=dt) / wsum
                valid[k] = tn > 0 and np.isfinite(tn) and np.isfinite(cst[k])
            if valid[k]:
                out.pose[b, k, :3], out.pose[b, k, 3:], out.normal[b, k] = t, q, nn
                out.cstat[b, k] = vis[k], cst[k], tn, 1
        order = sorted((k for k in range(4) if valid[k]), key=lambda k: (0 if vis[k] >= vis_min else 1, cst[k], k))
        out.pick[b, :len(order[:2])] = order[:2]
    return out


# ------------------------------------------------------------------------------------------------ scenes
Scene = collections.namedtuple("Scene", "x1 x2 R t n d E H inlier")


def pose_of(Rm, t):
    """[7]: (t unit, q xyzw with w >= 0)"""
    return np.concatenate([t / np.linalg.norm(t), rot_to_quat(np.asarray(Rm, np.float64))])


def plane_scene(seed, P=576, outliers=0.3, sigma=1e-3, off_plane=0.0):
    """the one-plane recipe of DESIGN.md 5.7: a rotation of up to 0.3 rad, |t| 1 .. 1.5 lifted along camera 2's axis until every
    z2 >= 2, plane normal (a, b, 1) / |.| with a, b uniform in +-0.6, plane distance 3 .. 6, P points with |xy| <= 0.55, Gaussian noise
    `sigma` on both images, a share `outliers` of x2 replaced by uniform noise; off_plane: that share of the points lies 2 .. 8 deep
    instead of on the plane.  No seed is rejected: every point is asserted to lie in front of both cameras.  x1, x2 float32 [1,P,2]"""
    rng = np.random.default_rng(9000 + seed)
    Rm = R._rotation(rng, 0.3)
    t = rng.standard_normal(3)
    t *= rng.uniform(1.0, 1.5) / np.linalg.norm(t)
    nrm = np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6), 1.0])
    nrm /= np.linalg.norm(nrm)
    d = rng.uniform(3.0, 6.0)
    xy = rng.uniform(-0.55, 0.55, (P, 2))
    xh = np.concatenate([xy, np.ones((P, 1))], -1)
    z = d / (xh @ nrm)
    off = rng.permutation(P)[:int(round(off_plane * P))]
    z[off] = rng.uniform(2.0, 8.0, len(off))
    X1 = xh * z[:, None]
    X2 = X1 @ Rm.T + t
    lift = max(0.0, 2.0 - X2[:, 2].min())
    t = t + np.array([0, 0, lift])
    X2 = X1 @ Rm.T + t
    assert X1[:, 2].min() > 0 and X2[:, 2].min() >= 2.0 - 1e-12
    x1 = xy[None] + sigma * rng.standard_normal((1, P, 2))
    x2 = (X2[:, :2] / X2[:, 2:])[None] + sigma * rng.standard_normal((1, P, 2))
    bad = rng.permutation(P)[:int(round(outliers * P))]
    x2[0, bad] = rng.uniform(-0.6, 0.6, (len(bad), 2))
    inlier = np.ones(P, bool)
    inlier[bad] = False
    Hm = Rm + np.outer(t, nrm) / d
    return Scene(x1.astype(np.float32), x2.astype(np.float32), Rm, t, nrm, d, R.true_essential(Rm, t)[None], Hm / np.linalg.norm(Hm), inlier)


def exact_scenes(n, P, seed):
    """n exact one-plane scenes of P points (no noise, no outliers), float32 inputs: (x1, x2 [n,P,2], H_true [n,3,3] Frobenius 1 with the
    sign rule, poses [n,7], normals [n,3], |t| / d [n])"""
    x1, x2, Hs, poses, ns, td = [], [], [], [], [], []
    for b in range(n):
        s = plane_scene(1000 * seed + b, P, 0.0, 0.0)
        x1.append(s.x1[0]), x2.append(s.x2[0])
        Hs.append(frob_sign(s.H.reshape(1, 9))[0][0].reshape(3, 3))
        poses.append(pose_of(s.R, s.t)), ns.append(s.n), td.append(np.linalg.norm(s.t) / s.d)
    return np.stack(x1), np.stack(x2), np.stack(Hs), np.stack(poses), np.stack(ns), np.array(td)


EDGE_KINDS = ("healthy", "pure_rotation", "t_parallel_n", "t_perp_n", "small_t", "large_t", "rank2", "zero", "nan")


def edge_homography(kind, rng):
    """(H [3,3] fp64, R, t / d, n) of one edge case of the decomposition (R, t / d, n None where there is no pose to recover)"""
    Rm = R._rotation(rng, 0.3)
    nrm = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), 1.0])
    nrm /= np.linalg.norm(nrm)
    t = rng.standard_normal(3)
    t /= np.linalg.norm(t)
    scale = 0.3
    if kind == "pure_rotation":
        return Rm.copy(), Rm, None, None
    if kind == "zero":
        return np.zeros((3, 3)), None, None, None
    if kind == "nan":
        Hm = Rm.copy()
        Hm[1, 2] = np.nan
        return Hm, None, None, None
    if kind == "t_parallel_n":
        t = Rm @ nrm
    if kind == "t_perp_n":
        t = np.cross(Rm @ nrm, [0.3, -0.5, 0.8])
        t /= np.linalg.norm(t)
    if kind == "small_t":
        scale = 1e-3
    if kind == "large_t":                                 # camera 2 stays on camera 1's side of the plane: 1 + n^T R^T t / d > 0
        scale = 3.0
        t = t if nrm @ (Rm.T @ t) > 0 else -t
    if kind == "rank2":                                   # the plane passes through camera 2's centre: n^T (-R^T t) = d
        t = -Rm @ nrm
        t = t + 0.4 * np.cross(Rm @ nrm, [0.2, 0.9, -0.1])   # any t with n^T R^T t = -d keeps H singular
        scale = -1.0 / float(nrm @ (Rm.T @ t))
    td = scale * t
    return Rm + np.outer(td, nrm), Rm, td, nrm


def edge_batch(seed=3, P=64):
    """one problem per EDGE_KINDS entry, each between two healthy neighbours: (kinds [3 len], H [n,3,3] float32, x1, x2 [n,P,2] float32
    points of the plane seen through H (for the pose-less kinds: through a healthy H), truth list)"""
    rng = np.random.default_rng(seed)
    kinds = []
    for k in EDGE_KINDS[1:]:
        kinds += ["healthy", k]
    kinds.append("healthy")
    Hs, x1, x2, truth = [], [], [], []
    for k in kinds:
        Hm, Rm, td, nrm = edge_homography(k, rng)
        Hv = Hm if np.isfinite(Hm).all() and abs(np.linalg.det(Hm)) > 1e-6 else edge_homography("healthy", rng)[0]
        xy = rng.uniform(-0.4, 0.4, (P, 2))
        m = np.concatenate([xy, np.ones((P, 1))], -1) @ Hv.T
        if k == "rank2":
            m = np.concatenate([xy, np.ones((P, 1))], -1) @ Hm.T
            m[:, 2] = np.where(np.abs(m[:, 2]) < 1e-3, 1e-3, m[:, 2])
        x1.append(xy), x2.append(m[:, :2] / m[:, 2:])
        Hs.append(Hm), truth.append((Rm, td, nrm))
    return kinds, np.stack(Hs).astype(np.float32), np.stack(x1).astype(np.float32), np.stack(x2).astype(np.float32), truth


# ------------------------------------------------------------------------------------------------ comparisons
def candidate_error(pose, normal, cstat, Rm, t, nrm):
    """the smallest (E error up to sign, rotation angle in degrees, translation direction angle in degrees, index) over the valid candidates
    whose normal agrees with nrm in sign"""
    best = (np.inf, np.inf, np.inf, -1)
    Et = R.true_essential(Rm, t)
    for k in range(4):
        if cstat[k, 3] != 1 or not np.any(pose[k, :3]):
            continue
        q, tu = pose[k, 3:].astype(np.float64), pose[k, :3].astype(np.float64)
        Rk = quat_to_rot(q)
        e = float(R.up_to_sign(cross_matrix(tu) @ Rk, Et)[0])
        ra = np.degrees(np.arccos(np.clip((np.trace(Rk.T @ Rm) - 1) / 2, -1, 1)))
        ta = np.degrees(np.arccos(np.clip(tu @ t / np.linalg.norm(t), -1, 1)))
        if normal[k].astype(np.float64) @ nrm > 0 and ra + ta < best[1] + best[2]:
            best = (e, ra, ta, k)
    return best


def match_candidates(a, b):
    """the assignment of b's candidates to a's (Poses of ONE problem each: pose [4,7], normal [4,3], cstat [4,4]) that minimises the
    summed distance: the order of the candidates follows the signs of the singular vectors, which two SVDs need not share ->
    (permutation [4], worst entry difference over pose (q up to sign), normal, visibility and Sampson cost after matching)"""
    import itertools
    best = None
    for perm in itertools.permutations(range(4)):
        tot, worst = 0.0, 0.0
        for k in range(4):
            j = perm[k]
            if a.cstat[k, 3] != b.cstat[j, 3]:
                tot = np.inf
                break
            if a.cstat[k, 3] == 0:
                continue
            qa, qb = a.pose[k, 3:].astype(np.float64), b.pose[j, 3:].astype(np.float64)
            dq = min(np.abs(qa - qb).max(), np.abs(qa + qb).max())
            dd = max(dq, np.abs(a.pose[k, :3].astype(np.float64) - b.pose[j, :3]).max(), np.abs(a.normal[k].astype(np.float64) - b.normal[j]).max())
            tot += dd
            worst = max(worst, dd)
        if best is None or tot < best[0]:
            best = (tot, perm, worst)
    return np.array(best[1]), best[2]


def decomposition_scale(sigma):
    """the sensitivity of (t^, n) to a relative perturbation of H: the coefficients of u are sqrt((1 - sigma_3) / gap) and
    sqrt((sigma_1 - 1) / gap), gap = sigma_1 - sigma_3; a perturbation eps of a sigma moves the smaller of them by
    eps / sqrt(min(1 - sigma_3, sigma_1 - 1) gap) (a double root, floored at eps: there the error is sqrt(eps / gap)), and the singular
    vectors by eps sigma_1 / gap"""
    s1, s3 = sigma
    gap = s1 - s3
    small = max(min(1 - s3, s1 - 1), EPS32)
    return max(1.0, s1 / gap, s1 / np.sqrt(small * gap))


# ------------------------------------------------------------------------------------------------ the cases, the ratios and their constants
# The shapes: the minimal sample, the 256-thread and the 7-rows-per-thread boundaries in P, the workgroup boundaries in M, the maximum.
EXACT = [(1, 4, 1), (3, 5, 255), (1, 8, 256), (3, 9, 257), (130, 64, 16), (1, 256, 1024), (3, 257, 16), (1, 512, 16), (3, 513, 16), (1, 1728, 40)]
CASES = [("exact", n, P, M, wt) for n, P, M in EXACT for wt in (False, True)] + [("noisy", 10, 576, 256, wt) for wt in (False, True)]
COND_MAX = 1e4            # a hypothesis is compared where sigma_1 / sigma_8 of the reference's 8 x 9 matrix is at most this
LEFT_OUT_MAX = 0.10
_CACHE = {}


def inputs(kind, n, P, M, weighted):
    """float32 x1, x2 [n,P,2], w [n,P] or None: exact one-plane scenes, or the ten 50 % noisy ones.  weighted: uniform(0.05, 1) with, from
    P = 24 on, 40 % zeros, a negative one and a NaN per problem"""
    key = ("in", kind, n, P, weighted)
    if key not in _CACHE:
        if kind == "noisy":
            sc = [plane_scene(s, P, 0.5) for s in range(n)]
            x1, x2 = np.concatenate([s.x1 for s in sc]), np.concatenate([s.x2 for s in sc])
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


def cost64(H, x1, x2, wc, tau):
    """the fp64 robust transfer cost of H [n,3,3] or [n,M,3,3] per problem (and hypothesis)"""
    H = np.asarray(H, np.float64)
    out = []
    for b in range(len(H)):
        with np.errstate(all="ignore"):
            t2 = float(tau) ** 2
            d = transfer(H[b], x1[b].astype(np.float64), x2[b].astype(np.float64))
            out.append((wc[b] * t2 * np.log1p(d / t2)).sum(-1) / wc[b].sum())
    return np.stack(out)


def horizon(H, x1, x2, wc, tau):
    """the part of the cost's rounding error that the form of tests/_consensus_ref.py does not know: a row NEAR THE HORIZON of H.  The
    third coordinate m_z = h3 . x1h is evaluated with an absolute error of up to 2 eps32 mu, mu = |h6 x| + |h7 y| + |h8|, so d carries a
    relative error of about 4 rho, rho = 2 eps32 mu / |m_z| -- of any size once rho approaches 1, up to the clamp (log1p(1e30 / tau^2)
    < 80).  The row's term moves by at most min(tau^2, d) min(4 rho, 80); the weighted mean of that, per problem (and hypothesis), fp64.
    For a row away from the horizon rho is about 2 eps32 and the term is negligible against eps32 sqrt(c)."""
    H = np.asarray(H, np.float64)
    out = []
    for b in range(len(H)):
        h = H[b].reshape(H[b].shape[:-2] + (1, 9))
        x, y = x1[b][:, 0].astype(np.float64), x1[b][:, 1].astype(np.float64)
        with np.errstate(all="ignore"):
            mz = h[..., 6] * x + h[..., 7] * y + h[..., 8]
            mu = np.abs(h[..., 6] * x) + np.abs(h[..., 7] * y) + np.abs(h[..., 8])
            rho = np.where(mz != 0, 2 * EPS32 * mu / np.where(mz != 0, np.abs(mz), 1), np.inf)
            d = transfer(H[b], x1[b].astype(np.float64), x2[b].astype(np.float64))
            out.append((wc[b] * np.minimum(float(tau) ** 2, d) * np.minimum(4 * rho, 80)).sum(-1) / wc[b].sum())
    return np.stack(out)


def cost_bound(c, C_, hor=0.0):
    return C_ * (EPS32 * (np.sqrt(c) + EPS32) + hor)


def consensus_ratios(out, ref, x1, x2, w, tau=TAU):
    """out: a Consensus-like tuple of numpy arrays (the device's or the restatement's), ref: the fp64 Consensus of the same inputs ->
    the ratios of the bounds: H (error up to sign over eps32 sigma_1 / sigma_8 on the compared hypotheses), cost and w (against the
    fp64 values at out's OWN H, the forms of tests/_consensus_ref.py), and the compared share"""
    n, P = x1.shape[:2]
    wc = C.clamp(w, n, P)
    valid = ref.hyp_cost < FLT_MAX
    compared = valid & (ref.cond <= COND_MAX)
    ovalid = out.hyp_cost < FLT_MAX
    assert np.array_equal(ovalid[compared], valid[compared]), "validity differs on a compared hypothesis"
    err = R.up_to_sign(out.hyp_H.reshape(-1, 9), ref.hyp_H.reshape(-1, 9)).reshape(valid.shape)
    rH = (err / (EPS32 * np.where(compared, ref.cond, 1)))[compared]
    own = cost64(out.hyp_H, x1, x2, wc, tau)
    both = ovalid & np.isfinite(own)
    hor = horizon(out.hyp_H, x1, x2, wc, tau)
    rc = (np.abs(out.hyp_cost.astype(np.float64) - own) / cost_bound(np.where(both, own, 1), 1.0, hor))[both]
    won = out.best >= 0
    rw = np.zeros(0)
    if won.any():
        t2 = float(tau) ** 2
        want = np.stack([wc[b] / (1 + transfer(out.H[b].astype(np.float64), x1[b].astype(np.float64), x2[b].astype(np.float64)) / t2)
                         for b in np.flatnonzero(won)])
        rw = (np.abs(out.weights[won].astype(np.float64) - want) / np.where(wc[won] > 0, wc[won], 1) / (EPS32 / tau))[wc[won] > 0]
    return dict(H=float(rH.max(initial=0)), cost=float(rc.max(initial=0)), w=float(rw.max(initial=0)), compared=float(compared.sum() / max(valid.sum(), 1)))


def check_consensus(out, ref, x1, x2, w, tau=TAU):
    """the device's rp_homography_consensus against the reference, at the calibrated bounds; returns the ratios"""
    n, P = x1.shape[:2]
    M = ref.hyp_cost.shape[1]
    wc = C.clamp(w, n, P)
    r = consensus_ratios(out, ref, x1, x2, w, tau)
    print("H ratio %.3g (C %.3g), cost ratio %.3g (C %.3g), w ratio %.3g (C %.3g), compared %.4f" % (r["H"], C_H, r["cost"], C_COST, r["w"], C_W, r["compared"]))
    assert r["compared"] >= 1 - LEFT_OUT_MAX
    assert r["H"] <= C_H and r["cost"] <= C_COST and r["w"] <= C_W, r
    K = (wc > 0).sum(-1)
    assert np.array_equal(out.stat[:, 3], K) and np.array_equal(out.stat[:, 2], (out.hyp_cost < FLT_MAX).sum(-1))
    for b in range(n):
        if K[b] < 4 or not (out.hyp_cost[b] < FLT_MAX).any():
            assert out.best[b] == -1 and not out.H[b].any() and not out.stat[b, :2].any()
            assert np.array_equal(out.weights[b], wc[b].astype(np.float32))
            continue
        win = int(np.argmin(out.hyp_cost[b]))                        # the lowest index of the device's own minimum, exactly
        assert out.best[b] == win and np.array_equal(out.H[b], out.hyp_H[b, win]) and out.stat[b, 0] == out.hyp_cost[b, win]
        # against the reference the winner is compared by COST: the device's winner costs (fp64, its own H) no more than the device's
        # version of the reference's winner, up to the two cost bounds
        pair = out.hyp_H[b:b + 1, [win, int(ref.best[b])]]
        own = cost64(pair, x1[b:b + 1], x2[b:b + 1], wc[b:b + 1], tau)[0]
        hor = horizon(pair, x1[b:b + 1], x2[b:b + 1], wc[b:b + 1], tau)[0]
        assert own[0] <= own[1] + cost_bound(own[0], C_COST, hor[0]) + cost_bound(own[1], C_COST, hor[1]), (b, own)
        t2 = float(tau) ** 2
        u = transfer(out.H[b].astype(np.float64), x1[b].astype(np.float64), x2[b].astype(np.float64)) / t2
        share, band = (wc[b] * (u <= 1)).sum() / wc[b].sum(), (wc[b] * (np.abs(u - 1) < 1e-4)).sum() / wc[b].sum()
        assert abs(out.stat[b, 1] - share) <= band + 1e-5, (b, out.stat[b, 1], share, band)
    return r


# refinement: the reference's kappa scales the bound, one step and converged, as DESIGN.md 5.3
REFINE_CASES = [(10, 576, False), (10, 576, True), (3, 257, True), (1, 1728, False), (2, 5, False)]


def refine_inputs(n, P, weighted):
    """(x1, x2, w, H0 float32): noisy 30 % one-plane scenes and the reference consensus winner (M = 64) rounded to float32 as the start"""
    key = ("rin", n, P, weighted)
    if key not in _CACHE:
        sc = [plane_scene(40 + s, P, 0.3 if P >= 24 else 0.0) for s in range(n)]
        x1, x2 = np.concatenate([s.x1 for s in sc]), np.concatenate([s.x2 for s in sc])
        w = None
        if weighted:
            rng = np.random.default_rng(P + n)
            w = rng.uniform(0.05, 1.0, (n, P)).astype(np.float32)
            w[rng.uniform(size=w.shape) < 0.4] = 0
            w[:, 5], w[:, 11] = -0.5, np.nan
        H0 = consensus(x1, x2, w, TAU, SEED, 64).H.astype(np.float32)
        _CACHE[key] = (x1, x2, w, H0)
    return _CACHE[key]


def refine_reference(n, P, weighted, iters):
    key = ("rref", n, P, weighted, iters)
    if key not in _CACHE:
        x1, x2, w, H0 = refine_inputs(n, P, weighted)
        _CACHE[key] = refine(x1, x2, w, TAU, H0, iters)
    return _CACHE[key]


def refine_ratios(H, stat, weights, ref, x1, x2, w, tau=TAU):
    """H error up to sign over eps32 kappa; cost and weights against fp64 at the output's own H"""
    n, P = x1.shape[:2]
    wc = C.clamp(w, n, P)
    kap = np.where(np.isfinite(ref.kappa), ref.kappa, 1.0)
    rH = R.up_to_sign(H.reshape(-1, 9), ref.H.reshape(-1, 9)) / (EPS32 * kap)
    own = cost64(H, x1, x2, wc, tau)
    rc = np.abs(stat[:, 0].astype(np.float64) - own) / cost_bound(own, 1.0, horizon(H, x1, x2, wc, tau))
    t2 = float(tau) ** 2
    want = np.stack([wc[b] / (1 + transfer(H[b].astype(np.float64), x1[b].astype(np.float64), x2[b].astype(np.float64)) / t2) for b in range(n)])
    rw = (np.abs(weights.astype(np.float64) - want) / np.where(wc > 0, wc, 1) / (EPS32 / tau))[wc > 0]
    return dict(H=float(rH.max()), cost=float(rc.max()), w=float(rw.max(initial=0)))


# decomposition
def decompose_inputs(kind):
    """(H float32 [n,3,3], x1, x2, w): "refined" -- the ten 30 % scenes at the reference's refined H; "exact" -- 130 exact scenes of 64
    points at the true H; "edge" -- edge_batch()"""
    key = ("din", kind)
    if key not in _CACHE:
        if kind == "edge":
            _, H, x1, x2, _ = edge_batch()
        elif kind == "exact":
            x1, x2, H = exact_scenes(130, 64, 21)[:3]
        else:
            sc = [plane_scene(s, 576, 0.3) for s in range(10)]
            x1, x2 = np.concatenate([s.x1 for s in sc]), np.concatenate([s.x2 for s in sc])
            H = refine(x1, x2, None, TAU, consensus(x1, x2, None, TAU, SEED, 256).H, 10).H
        _CACHE[key] = (np.asarray(H, np.float32), x1, x2, None)
    return _CACHE[key]


DECOMPOSE_KINDS = ("refined", "exact", "edge")


def decompose_reference(kind):
    key = ("dref", kind)
    if key not in _CACHE:
        H, x1, x2, w = decompose_inputs(kind)
        _CACHE[key] = decompose(H, x1, x2, w, TAU)
    return _CACHE[key]


def decompose_ratios(out, ref, inp):
    """per problem: the candidates matched up to the order (match_candidates), the worst entry difference over eps32 decomposition_scale;
    the visibility shares of matched candidates: their absolute difference beyond the horizon band, over eps32; their Sampson costs: the difference over
    eps32 sc (sqrt(c) + eps32 sc), sc the decomposition's scale -- E moves by eps32 sc, the residuals with it"""
    n = len(ref.pose)
    H, x1, x2, w = inp
    wc = C.clamp(w, n, x1.shape[1])
    r, rc, rv = np.zeros(n), np.zeros(n), np.zeros(n)
    for b in range(n):
        nv = int(ref.cstat[b, :, 3].sum())
        assert int(out.cstat[b, :, 3].sum()) == nv, (b, out.cstat[b], ref.cstat[b])
        if nv == 0:
            assert not out.pose[b].any() and not out.normal[b].any() and not out.cstat[b].any() and np.array_equal(out.pick[b], [-1, -1])
            continue
        one = lambda p: Poses(p.pose[b], p.normal[b], p.cstat[b], None, None)      # noqa: E731
        if nv == 1:                                                                # pure rotation: candidate 0 on both sides
            qa, qb = ref.pose[b, 0, 3:], out.pose[b, 0, 3:].astype(np.float64)
            r[b] = min(np.abs(qa - qb).max(), np.abs(qa + qb).max()) / EPS32
            assert not out.pose[b, 0, :3].any() and np.array_equal(out.cstat[b, 0], [1, 0, 0, 1]) and np.array_equal(out.pick[b], [0, -1])
            continue
        perm, worst = match_candidates(one(ref), one(out))
        r[b] = worst / (EPS32 * decomposition_scale(ref.sigma[b]))
        for k in range(4):
            j = perm[k]
            # a row within the normal's error of the plane's horizon n^T x1h = 0 may fall on either side: its Cauchy weight share is the band
            xh = np.concatenate([x1[b].astype(np.float64), np.ones((x1.shape[1], 1))], -1)
            hs = np.asarray(H[b], np.float64) / np.linalg.svd(np.asarray(H[b], np.float64), compute_uv=False)[1]
            wcau = wc[b] / (1 + transfer(hs, x1[b].astype(np.float64), x2[b].astype(np.float64)) / TAU ** 2)
            near = np.abs(xh @ ref.normal[b, k]) <= C_DECOMPOSE * EPS32 * decomposition_scale(ref.sigma[b]) * np.linalg.norm(xh, axis=-1)
            band = (wcau * near).sum() / wcau.sum()
            rv[b] = max(rv[b], max(abs(ref.cstat[b, k, 0] - out.cstat[b, j, 0]) - band, 0) / EPS32)
            sc = decomposition_scale(ref.sigma[b])                 # E moves by eps32 sc: sqrt(c) by about that, in units of the residual
            rc[b] = max(rc[b], abs(ref.cstat[b, k, 1] - out.cstat[b, j, 1]) / (EPS32 * sc * (np.sqrt(ref.cstat[b, k, 1]) + EPS32 * sc)))
    return dict(pose=r, cost=rc, vis=rv)


# 8 x the restatement's worst ratio on these same inputs (tests/test_homography_cpu.py asserts the restatement within C / 8 and above
# 0.9 C / 8: the constants are these figures, not looser ones)
C_H, C_COST, C_W = 23.9, 19.6, 5.11                    # the restatement: 2.983, 2.442, 0.638
C_REFINE_H = {1: 1.48, 10: 246.0}                      # one step 0.184; converged 30.67: float32 stops accepting steps 1e-5 short of fp64
C_DECOMPOSE, C_DECOMPOSE_COST, C_VIS = 20.1, 2.67, 5.54  # 2.51, 0.333, 0.692 (visibility: beyond the horizon band, in eps32)
WORST = dict(H=2.983, cost=2.442, w=0.638, refine1=0.184, refine10=30.67, decompose=2.51, decompose_cost=0.333, vis=0.692)


# ------------------------------------------------------------------------------------------------ the planar chain and its tables
Chain = collections.namedtuple("Chain", "consensus refined poses truth_k error")


def chain(scene, M=256, iters=10, vis_min=0.99, dt=np.float64, first=0):
    """consensus -> refine on the base weights -> decomposition of one Scene; truth_k: the candidate nearest the truth among those whose
    normal has the truth's sign, error = candidate_error at it"""
    c = consensus(scene.x1, scene.x2, None, TAU, SEED, M, dt, first)
    r = refine(scene.x1, scene.x2, None, TAU, c.H, iters, dt)
    d = decompose(r.H, scene.x1, scene.x2, None, TAU, vis_min, dt)
    e = candidate_error(d.pose[0], d.normal[0], d.cstat[0], scene.R, scene.t, scene.n)
    return Chain(c, r, d, e[3], e[:3])


def table(outliers, off_plane=0.0, vis_min=0.99, seeds=range(10)):
    """per scene: (E error, rotation deg, translation deg) of the candidate nearest the truth, its index, pick [2], the number of
    candidates passing vis_min, the scene"""
    key = ("table", outliers, off_plane, vis_min, tuple(seeds))
    if key not in _CACHE:
        rows = []
        for s in seeds:
            sc = plane_scene(s, 576, outliers, 1e-3, off_plane)
            ch = chain(sc)
            cs = ch.poses.cstat[0]
            rows.append((ch.error, ch.truth_k, ch.poses.pick[0].tolist(), int(((cs[:, 3] == 1) & (cs[:, 0] >= vis_min)).sum()), sc, ch))
        _CACHE[key] = rows
    return _CACHE[key]
