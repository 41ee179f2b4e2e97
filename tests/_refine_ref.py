"""References for rp_refine_pose (include/relpose_refine.h), numpy only, no GPU and no library.

  refine_ref     the iteration of the header in fp64: Levenberg-Marquardt on the Cauchy-robust Sampson cost over the five degrees of
                 freedom of (R, t), exact analytic Jacobian, 5 x 5 Cholesky of the diagonally scaled normal matrix.
  refine_f32     the kernel's arithmetic restated in numpy float32: the same statements in the same order on float32 numbers.  Only the
                 order of the sums differs (numpy's pairwise sums against the kernel's per-thread / wave / LDS tree).  The GPU tests'
                 bounds are calibrated against it: 8 x its largest error on the same inputs.
  decode_pose    E -> (R, t) by the cheirality vote, fp64 (the counterpart of rp_pose_from_essential), and the helpers around poses:
                 quaternion <-> rotation, the retraction, angles between poses, perturbed starts.
  scenes / wide_scenes / noisy_scene come from tests/_eightpoint_ref.py; scenes_with_pose adds the true pose to `scenes`.
"""
import collections

import numpy as np

from tests._eightpoint_ref import EPS32, noisy_scene, scenes, wide_scenes  # noqa: F401  (re-exported)

MIN_NORM = 1e-30     # |t0| or |q0| below this: degenerate
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-7, 1e7
SMALL_ANGLE = 1e-4   # below it sin(theta / 2) / theta is taken from its series

Refined = collections.namedtuple("Refined", "pose E stat weights kappa0 kappa trace")
Refined.__doc__ = """pose [n,7], E [n,3,3], stat [n,4], weights [n,P] as the header documents them; kappa0 / kappa [n]: the condition
number (fp64) of the diagonally scaled normal matrix at the start / at the output pose (0 for a degenerate problem); trace: per problem
the list of (cost, accepted, |step|) of every iteration"""


# ------------------------------------------------------------------------------------------------ poses
def quat_to_rot(q):
    x, y, z, w = q
    one, two = q.dtype.type(1), q.dtype.type(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype=q.dtype)


def rot_to_quat(R):
    """fp64, xyzw, w >= 0 (Shepperd: the branch with the largest pivot)"""
    R = np.asarray(R, np.float64)
    k = int(np.argmax([R[0, 0], R[1, 1], R[2, 2], np.trace(R)]))
    if k == 3:
        q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1 + np.trace(R)])
    elif k == 0:
        q = np.array([1 + R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0], R[2, 1] - R[1, 2]])
    elif k == 1:
        q = np.array([R[0, 1] + R[1, 0], 1 + R[1, 1] - R[0, 0] - R[2, 2], R[1, 2] + R[2, 1], R[0, 2] - R[2, 0]])
    else:
        q = np.array([R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1 + R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]])
    q /= np.linalg.norm(q)
    return -q if q[3] < 0 else q


def cross_matrix(t):
    z = t.dtype.type(0)
    return np.array([[z, -t[2], t[1]], [t[2], z, -t[0]], [-t[1], t[0], z]], dtype=t.dtype)


def tangent_basis(t):
    """(b1, b2): e_k for the smallest |t_k| (the lowest index on ties), b1 = normalise(e_k x t), b2 = t x b1"""
    k = int(np.argmin(np.abs(t)))
    e = np.zeros(3, t.dtype)
    e[k] = 1
    b1 = np.cross(e, t).astype(t.dtype)
    b1 = b1 / np.sqrt((b1 * b1).sum(dtype=t.dtype))
    return b1, np.cross(t, b1).astype(t.dtype)


def retract(t, q, delta):
    """R <- R exp([omega]x) as q <- normalise(q (x) (omega sin(theta / 2) / theta, cos(theta / 2))), t <- normalise(t + b1 beta1 + b2 beta2)"""
    dt = t.dtype.type
    om = delta[:3]
    th = np.sqrt((om * om).sum(dtype=dt))
    k = dt(0.5) - th * th / dt(48) if th < dt(SMALL_ANGLE) else np.sin(dt(0.5) * th) / th
    pv, pw = (om * k).astype(dt), np.cos(dt(0.5) * th)
    qv, qw = q[:3], q[3]
    nv = qw * pv + pw * qv + np.cross(qv, pv).astype(dt)
    nw = qw * pw - (qv * pv).sum(dtype=dt)
    nq = np.concatenate([nv, [nw]]).astype(dt)
    nq = nq / np.sqrt((nq * nq).sum(dtype=dt))
    b1, b2 = tangent_basis(t)
    nt = (t + b1 * delta[3] + b2 * delta[4]).astype(dt)
    return nt / np.sqrt((nt * nt).sum(dtype=dt)), nq


def _unit(v):
    """v / |v| with the largest magnitude taken out first (no overflow, no underflow), and |v|"""
    dt = v.dtype.type
    m = np.abs(v).max()
    if not m > 0:
        return v, dt(0)
    u = v / m
    s = np.sqrt((u * u).sum(dtype=dt))
    return u / s, m * s


def rotation_angle(Ra, Rb):
    """degrees"""
    c = (np.trace(np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1))))


def direction_angle(ta, tb):
    """degrees"""
    ta, tb = np.asarray(ta, np.float64), np.asarray(tb, np.float64)
    return float(np.degrees(np.arccos(np.clip(ta @ tb / np.linalg.norm(ta) / np.linalg.norm(tb), -1, 1))))


def decode_pose(E, x1, x2):
    """E [3,3], x1, x2 [P,2] -> pose [7] = (t unit, q xyzw, w >= 0) in fp64: the candidate (U W V^T | U W^T V^T, +-u_2) with the most
    points in front of both cameras (X2 = R X1 + t)"""
    E, x1, x2 = np.asarray(E, np.float64).reshape(3, 3), np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    h1 = np.concatenate([x1, np.ones_like(x1[:, :1])], -1)
    h2 = np.concatenate([x2, np.ones_like(x2[:, :1])], -1)
    best, pose = -1, None
    for R in (U @ W @ Vt, U @ W.T @ Vt):
        m = h1 @ R.T
        for t in (U[:, 2], -U[:, 2]):
            # l1 m - l2 h2 = -t per point, least squares
            mm, xx, mx = (m * m).sum(-1), (h2 * h2).sum(-1), (m * h2).sum(-1)
            mt, xt = m @ t, h2 @ t
            det = mm * xx - mx * mx
            ok = det > 1e-12 * mm * xx
            d = np.where(ok, det, 1)
            l1, l2 = (-mt * xx + mx * xt) / d, (-mt * mx + mm * xt) / d
            count = int((ok & (l1 > 0) & (l2 > 0)).sum())
            if count > best:
                best, pose = count, np.concatenate([t, rot_to_quat(R)])
    return pose


def scenes_with_pose(n, P, seed):
    """`scenes` and the true poses [n,7] of its E_true, decoded with its own exact points"""
    x1, x2, Et = scenes(n, P, seed)
    return x1, x2, Et, np.stack([decode_pose(Et[b], x1[b], x2[b]) for b in range(n)])


def perturbed(pose, rng, angle=0.03):
    """pose [n,7] moved by `angle` rad in R and by `angle` rad in the direction of t (fp64)"""
    out = np.empty_like(pose)
    for b in range(len(pose)):
        om = rng.standard_normal(3)
        be = rng.standard_normal(2)
        d = np.concatenate([om / np.linalg.norm(om) * angle, be / np.linalg.norm(be) * np.tan(angle)])
        t, q = retract(pose[b, :3].copy(), pose[b, 3:].copy(), d)
        out[b] = np.concatenate([t, q])
    return out


# ------------------------------------------------------------------------------------------------ the iteration (dtype generic)
def _frame(t, q):
    """E = [t]x R and the five derivative matrices D_k = dE / d(omega_0..2, beta_1..2) at delta = 0"""
    dt = t.dtype
    R = quat_to_rot(q)
    E = (cross_matrix(t) @ R).astype(dt)
    b1, b2 = tangent_basis(t)
    z = np.zeros(3, dt)
    D = np.stack([np.stack([z, E[:, 2], -E[:, 1]], -1), np.stack([-E[:, 2], z, E[:, 0]], -1), np.stack([E[:, 1], -E[:, 0], z], -1),
                  (cross_matrix(b1) @ R).astype(dt), (cross_matrix(b2) @ R).astype(dt)])
    return E, D


def _lines(E, x1, x2):
    """(E h1)_x, (E h1)_y, (E^T h2)_x, (E^T h2)_y, h2^T E h1 with h = (x, y, 1), written out as the kernel does"""
    ax, ay, bx, by = x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1]
    l2x, l2y, l2z = (E[r, 0] * ax + E[r, 1] * ay + E[r, 2] for r in range(3))
    l1x, l1y = (E[0, c] * bx + E[1, c] * by + E[2, c] for c in range(2))
    return l2x, l2y, l1x, l1y, bx * l2x + by * l2y + l2z


def residual(E, x1, x2):
    """s [P] = x2^T E x1 / sqrt(den) (0 where den is 0), and 1 / sqrt(den) (0 there)"""
    dt = x1.dtype.type
    l2x, l2y, l1x, l1y, r = _lines(E, x1, x2)
    den = l2x * l2x + l2y * l2y + l1x * l1x + l1y * l1y
    inv = np.where(den > 0, dt(1) / np.sqrt(np.where(den > 0, den, dt(1))), dt(0))
    return r * inv, inv, (l2x, l2y, l1x, l1y)


def jacobian(E, D, x1, x2):
    """s [P] and the exact J [P,5] = ds / d(omega, beta)"""
    s, inv, (l2x, l2y, l1x, l1y) = residual(E, x1, x2)
    J = np.empty((len(s), 5), x1.dtype)
    for k in range(5):
        mx, my, nx, ny, dr = _lines(D[k], x1, x2)
        half = l2x * mx + l2y * my + l1x * nx + l1y * ny            # half the derivative of den
        J[:, k] = (dr - s * half * inv) * inv
    return s, J


def _cost(s, w, wsum, tau2):
    dt = s.dtype.type
    return (w * (tau2 * np.log1p(s * s / tau2))).sum(dtype=dt) / wsum


def _solve(H, g, lam):
    """(H + lam diag H) delta = -g in the diagonally scaled form, by Cholesky; None if it breaks down"""
    dt = H.dtype.type
    d = np.diag(H)
    if not bool((d > 0).all()) or not bool(np.isfinite(d).all()):
        return None
    sc = dt(1) / np.sqrt(d)
    A = (H * sc[:, None] * sc[None, :]).astype(H.dtype)
    rhs = (g * sc).astype(H.dtype)
    L = np.zeros((5, 5), H.dtype)
    for j in range(5):
        p = dt(1) + lam                                               # the scaled diagonal is 1 by construction
        for k in range(j):
            p = p - L[j, k] * L[j, k]
        if not p > 0 or not np.isfinite(p):
            return None
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, 5):
            v = A[i, j]
            for k in range(j):
                v = v - L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    y = np.zeros(5, H.dtype)
    for i in range(5):
        v = rhs[i]
        for k in range(i):
            v = v - L[i, k] * y[k]
        y[i] = v / L[i, i]
    z = np.zeros(5, H.dtype)
    for i in range(4, -1, -1):
        v = y[i]
        for k in range(i + 1, 5):
            v = v - L[k, i] * z[k]
        z[i] = v / L[i, i]
    delta = (-(z * sc)).astype(H.dtype)
    return delta if bool(np.isfinite(delta).all()) else None


def scaled_condition(H):
    H = np.asarray(H, np.float64)
    d = np.diag(H)
    if not bool((d > 0).all()):
        return 0.0
    sc = 1 / np.sqrt(d)
    return float(np.linalg.cond(H * sc[:, None] * sc[None, :]))


def normal_matrix(t, q, x1, x2, w, tau2):
    """H [5,5], g [5] at the pose (t, q) with the Cauchy weights there"""
    dt = x1.dtype
    E, D = _frame(t, q)
    s, J = jacobian(E, D, x1, x2)
    om = (w / (dt.type(1) + s * s / tau2)).astype(dt)
    H = np.empty((5, 5), dt)
    for i in range(5):
        for j in range(i, 5):
            H[i, j] = H[j, i] = (om * J[:, i] * J[:, j]).sum(dtype=dt)
    g = np.array([(om * J[:, i] * s).sum(dtype=dt) for i in range(5)], dt)
    return H, g


def _one(pose0, x1, x2, w0, tau, iters, dt):
    """one problem -> (pose [7], E [9], stat [4], weights [P], kappa0, kappa, trace)"""
    f = dt
    P = len(x1)
    w = np.ones(P, dt) if w0 is None else np.where(np.asarray(w0, dt) > 0, np.asarray(w0, dt), f(0)).astype(dt)
    p0 = np.asarray(pose0, dt)
    t, tn = _unit(p0[:3])
    q, qn = _unit(p0[3:])
    tau = f(tau)
    if int((w > 0).sum()) < 5 or not tn >= f(MIN_NORM) or not qn >= f(MIN_NORM) or not tau > 0:
        return p0.copy(), np.zeros(9, dt), np.zeros(4, dt), w, 0.0, 0.0, []
    tau2 = tau * tau
    wsum = w.sum(dtype=dt)
    c = c0 = _cost(residual(_frame(t, q)[0], x1, x2)[0], w, wsum, tau2)
    lam, accepted, last, trace, kappa0 = f(LAMBDA0), 0, f(0), [], None
    for _ in range(iters):
        H, g = normal_matrix(t, q, x1, x2, w, tau2)
        if kappa0 is None:
            kappa0 = scaled_condition(H)
        delta = _solve(H, g, lam)
        ok = False
        if delta is not None:
            t1, q1 = retract(t, q, delta)
            c1 = _cost(residual(_frame(t1, q1)[0], x1, x2)[0], w, wsum, tau2)
            ok = bool(c1 < c)
        if ok:
            t, q, c = t1, q1, c1
            lam = max(lam / f(10), f(LAMBDA_MIN))
            accepted += 1
            last = np.sqrt((delta * delta).sum(dtype=dt))
        else:
            lam = min(lam * f(10), f(LAMBDA_MAX))
        trace.append((float(c), ok, float(np.sqrt((delta * delta).sum())) if delta is not None else 0.0))
    if q[3] < 0:
        q = -q
    E = _frame(t, q)[0]
    s = residual(E, x1, x2)[0]
    wo = (w / (f(1) + s * s / tau2)).astype(dt)
    Hf = normal_matrix(t, q, x1, x2, w, tau2)[0]
    kappa = scaled_condition(Hf)
    return (np.concatenate([t, q]).astype(dt), E.reshape(9), np.array([c0, c, accepted, last], dt), wo,
            kappa if kappa0 is None else kappa0, kappa, trace)


def _batch(pose0, x1, x2, w, tau, iters, dt):
    n, P = x1.shape[:2]
    tau = np.broadcast_to(np.asarray(tau, dt), (n,))
    out = [_one(pose0[b], x1[b], x2[b], None if w is None else w[b], tau[b], iters, dt) for b in range(n)]
    return Refined(np.stack([o[0] for o in out]), np.stack([o[1] for o in out]).reshape(n, 3, 3), np.stack([o[2] for o in out]),
                   np.stack([o[3] for o in out]), np.array([o[4] for o in out]), np.array([o[5] for o in out]), [o[6] for o in out])


def refine_ref(pose0, x1, x2, w=None, tau=0.01, iters=10):
    """fp64 reference of rp_refine_pose: pose0 [n,7], x1, x2 [n,P,2], w [n,P] or None, tau a number or [n] -> Refined"""
    return _batch(np.asarray(pose0, np.float64), np.asarray(x1, np.float64), np.asarray(x2, np.float64), w, tau, iters, np.float64)


def refine_f32(pose0, x1, x2, w=None, tau=0.01, iters=10):
    """the kernel's arithmetic in numpy float32 (see the module docstring); same arguments and results as refine_ref"""
    return _batch(np.asarray(pose0, np.float32), np.asarray(x1, np.float32), np.asarray(x2, np.float32), w, tau, iters, np.float32)


def cost64(pose, x1, x2, w, tau):
    """the cost c of the header at the given poses, fp64: pose [n,7] (normalised here), -> [n]"""
    pose, x1, x2 = np.asarray(pose, np.float64), np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    n, P = x1.shape[:2]
    tau = np.broadcast_to(np.asarray(tau, np.float64), (n,))
    out = np.empty(n)
    for b in range(n):
        wb = np.ones(P) if w is None else np.maximum(np.nan_to_num(np.asarray(w[b], np.float64)), 0)
        E = _frame(_unit(pose[b, :3])[0], _unit(pose[b, 3:])[0])[0]
        out[b] = _cost(residual(E, x1[b], x2[b])[0], wb, wb.sum(), tau[b] * tau[b])
    return out


def pose_matrix(pose):
    """[7] -> (R [3,3], t [3]) fp64"""
    pose = np.asarray(pose, np.float64)
    return quat_to_rot(pose[3:] / np.linalg.norm(pose[3:])), pose[:3] / np.linalg.norm(pose[:3])
