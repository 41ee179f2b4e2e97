"""References for rp_pose_covariance (include/relpose_covariance.h), numpy only, no GPU and no library.

  covariance_ref  fp64: A = sum psi' J J^T, B = sum psi^2 J J^T on tests/_refine_ref.jacobian, C = A^-1 B A^-1 in the diagonally scaled
                  form (numpy Cholesky), a SECOND route for C (LAPACK solve on the unscaled A), eigenpairs by eigh, and the sums of the
                  absolute terms that the GPU bounds need.
  algebra_ref     the fp64 algebra alone, applied to given upper entries of A and B (the device's own `normal`).
  covariance_f32  the kernel's arithmetic restated in numpy float32: the header's statements in the header's order -- the rows summed
                  per thread, per wave by the xor butterfly, then the four waves --, the scaled Cholesky, the inverse, the sandwich
                  product, the Jacobi sweeps.  Only fused multiply-adds differ.  The GPU tests' constants are 8 x its worst error.
  naive_ref       sigma^2 H^-1 with H the Gauss-Newton matrix of the refinement: the formula NOT shipped.
  mc_geometry / mc_draw / mc_error   the Monte-Carlo scenes of the calibration: a geometry from default_rng(g) by noisy_scene's recipe,
                  noise and wrong matches from a second generator, and the error of a refined pose in the five parameters.
  gpu_case        the inputs of tests/test_gpu_covariance.py, shared with the CPU test that fixes its constants.
"""
import collections

import numpy as np

from tests import _refine_ref as R
from tests._eightpoint_ref import EPS32, _rotation

MIN_NORM = 1e-30
K_MIN = 6
PIVOT_MIN = 1e-6
SWEEPS = 6
FINITE = 3.0e38
OK, DEGENERATE, NOT_DETERMINED = 1, 0, -1
CHI2_5_95 = 11.07                     # the 95 % point of chi^2 with 5 degrees of freedom

# ---- the constants of the GPU bounds: 8 x the worst value of covariance_f32 against fp64 over gpu_cases(), rounded up
# (tests/test_covariance_cpu.py re-measures the restatement and holds each constant to [8 x, 8.5 x] of it)
C1_NORMAL = 2000.0                    # |normal - fp64 sums| <= C1 K eps32 sum |term|                       restatement: 245.6
C2_COV = 12.5                         # |dC_ij| <= C2 eps32 kappa sqrt(C_ii C_jj); sd_rot, sd_dir, rho relative restatement: 1.536
C_EIG = 14.0                          # |eig - eigh(cov)| <= C_EIG eps32 eig[0]                              restatement: 1.726
C3_WEAK = 13.5                        # angle(weak, eigh's vector) <= C3 eps32 eig[0] / (eig[0] - eig[1])    restatement: 1.668
C_COST = 2500.0                       # |c - fp64 c| <= C_COST eps32 c (x2^T E x1 cancels to sigma: eps32 / sigma relative) restatement: 303.7
RESTATEMENT = (245.6, 1.536, 1.726, 1.668, 303.7)   # the measured values above, in the order of gpu_errors
NEG_WINDOW = 8 * EPS32                # a row with |u - 1| inside it may differ in the count of psi' < 0
NEG_CAP = 0.01                        # at most this share of a problem's rows may lie inside the window
GAP_MIN = 2.0                         # weak is compared where eig[0] / eig[1] >= this

Covariance = collections.namedtuple("Covariance", "cov frame eig weak stat normal abs_normal kappa cov_solve vec")
Covariance.__doc__ = """cov [n,5,5], frame [n,6], eig [n,5], weak [n,5], stat [n,8], normal [n,30] as the header documents them; abs_normal
[n,30] the sums of the absolute values of the terms of `normal`; kappa [n] the condition number of the scaled A (0 unless status 1);
cov_solve [n,5,5] C by the second route (fp64 only, else None); vec [n,5,5] all eigenvectors, columns, in the order of eig (fp64 only)"""


# ------------------------------------------------------------------------------------------------ the pose, restatable bit for bit
def unit_exact(v):
    """v / |v| with the largest magnitude taken out first, every sum left to right, and |v|"""
    dt = v.dtype.type
    m = dt(np.nanmax(np.abs(v))) if not np.isnan(v).all() else dt(0)      # (fmaxf passes a NaN over)
    if not m > 0:
        return v.copy(), dt(0)
    with np.errstate(all="ignore"):
        u = (v / m).astype(v.dtype)
        ss = dt(0)
        for x in u:
            ss = dt(ss + dt(x * x))
        s = np.sqrt(ss)
        return (u / s).astype(v.dtype), dt(m * s)


def tangent_basis_exact(t):
    dt = t.dtype.type
    a = np.abs(t)
    k = 1 if a[1] < a[0] else 0
    k = 2 if a[2] < a[k] else k
    z = dt(0)
    c = [np.array([z, -t[2], t[1]], t.dtype), np.array([t[2], z, -t[0]], t.dtype), np.array([-t[1], t[0], z], t.dtype)][k]
    s = np.sqrt(dt(dt(dt(c[0] * c[0]) + dt(c[1] * c[1])) + dt(c[2] * c[2])))
    b1 = (c / s).astype(t.dtype)
    b2 = np.array([dt(t[1] * b1[2]) - dt(t[2] * b1[1]), dt(t[2] * b1[0]) - dt(t[0] * b1[2]), dt(t[0] * b1[1]) - dt(t[1] * b1[0])], t.dtype)
    return b1, b2


def _frame(t, q, b1, b2):
    """E and the five D_k as tests/_refine_ref._frame, with the given basis"""
    dt = t.dtype
    Rm = R.quat_to_rot(q)
    E = (R.cross_matrix(t) @ Rm).astype(dt)
    z = np.zeros(3, dt)
    D = np.stack([np.stack([z, E[:, 2], -E[:, 1]], -1), np.stack([-E[:, 2], z, E[:, 0]], -1), np.stack([E[:, 1], -E[:, 0], z], -1),
                  (R.cross_matrix(b1) @ Rm).astype(dt), (R.cross_matrix(b2) @ Rm).astype(dt)])
    return E, D


# ------------------------------------------------------------------------------------------------ the sums
def _block_sum(v, dt):
    """sum of v [P, ...] in the kernel's order: thread t its rows t, t + 256, .. in turn; the 64 lanes of a wave by the xor butterfly;
    ((w0 + w1) + w2) + w3.  fp64: a plain sum."""
    if dt is np.float64:
        return v.sum(0)
    P = v.shape[0]
    slots = (P + 255) // 256
    pad = np.zeros((slots * 256,) + v.shape[1:], dt)
    pad[:P] = v
    pad = pad.reshape((slots, 256) + v.shape[1:])
    acc = np.zeros((256,) + v.shape[1:], dt)
    for i in range(slots):
        acc = (acc + pad[i]).astype(dt)
    acc = acc.reshape((4, 64) + v.shape[1:])
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[:, lane ^ o]).astype(dt)
    w = acc[:, 0]
    return ((w[0] + w[1]).astype(dt) + w[2]).astype(dt) + w[3]


_IU = np.triu_indices(5)


def _sums(pose, x1, x2, w0, tau, dt):
    """one problem -> dict: degenerate (by the pose / tau), frame, the 34 reduced values, the sums of absolute terms, u [P], w [P]"""
    f = dt
    P = len(x1)
    w = np.ones(P, dt) if w0 is None else np.where(np.asarray(w0, dt) > 0, np.asarray(w0, dt), f(0)).astype(dt)
    p0 = np.asarray(pose, dt)
    finite = bool((np.abs(p0) <= f(FINITE)).all())
    t, tn = unit_exact(p0[:3])
    q, qn = unit_exact(p0[3:])
    tau = f(tau)
    deg = not finite or not tn >= f(MIN_NORM) or not qn >= f(MIN_NORM) or not tau > 0
    if deg:
        t, q = np.array([1, 0, 0], dt), np.array([0, 0, 0, 1], dt)
    b1, b2 = tangent_basis_exact(t)
    E, D = _frame(t, q, b1, b2)
    with np.errstate(all="ignore"):
        tau2 = f(tau * tau)
        s, J = R.jacobian(E, D, x1, x2)
        u = (s * s / tau2).astype(dt)
        qq = (f(1) + u).astype(dt)
        psi = (w * s / qq).astype(dt)
        dpsi = (w * (f(1) - u) / (qq * qq)).astype(dt)
        psi2 = (psi * psi).astype(dt)
        pJ, bJ = (dpsi[:, None] * J).astype(dt), (psi2[:, None] * J).astype(dt)
        termA = (pJ[:, _IU[0]] * J[:, _IU[1]]).astype(dt)
        termB = (bJ[:, _IU[0]] * J[:, _IU[1]]).astype(dt)
        cost = (w * (tau2 * np.log1p(s * s / tau2))).astype(dt)
        scal = np.stack([w, (w > 0).astype(dt), (dpsi < 0).astype(dt), cost], -1)
        red = _block_sum(np.concatenate([termA, termB, scal], -1), dt)
        absn = np.abs(np.concatenate([termA, termB], -1)).astype(np.float64).sum(0)
    return dict(degenerate=deg, frame=np.concatenate([b1, b2]), red=red, absn=absn, u=u, w=w)


# ------------------------------------------------------------------------------------------------ the algebra
def _full(upper, dt):
    M = np.zeros((5, 5), dt)
    M[_IU] = upper
    return (M + np.triu(M, 1).T).astype(dt)


def _algebra_f32(normal):
    """steps 1 - 5 of the header and the Jacobi sweeps in float32 -> (ok, C, rho, eig, weak)"""
    f = np.float32
    A, B = _full(normal[:15], f), _full(normal[15:], f)
    zero = (False, np.zeros((5, 5), f), f(0), np.zeros(5, f), np.zeros(5, f))
    dg = np.diag(A)
    if not bool(((dg > 0) & (dg <= f(FINITE))).all()):
        return zero
    d = (f(1) / np.sqrt(dg)).astype(f)
    L = np.zeros((5, 5), f)
    low = f(1)
    for j in range(5):
        p = f(1)
        for m in range(j):
            p = f(p - f(L[j, m] * L[j, m]))
        if not p > f(PIVOT_MIN):
            return zero[:2] + (p if abs(p) <= f(FINITE) else f(0),) + zero[3:]
        low = min(low, p)
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, 5):
            v = f(f(A[i, j] * d[i]) * d[j])
            for m in range(j):
                v = f(v - f(L[i, m] * L[j, m]))
            L[i, j] = f(v / L[j, j])
    M = np.zeros((5, 5), f)
    for c in range(5):
        y, z = np.zeros(5, f), np.zeros(5, f)
        for i in range(5):
            v = f(1 if i == c else 0)
            for m in range(i):
                v = f(v - f(L[i, m] * y[m]))
            y[i] = f(v / L[i, i])
        for i in range(4, -1, -1):
            v = y[i]
            for m in range(i + 1, 5):
                v = f(v - f(L[m, i] * z[m]))
            z[i] = f(v / L[i, i])
        M[:, c] = z
    T = np.zeros((5, 5), f)
    for i in range(5):
        for l in range(5):
            v = f(0)
            for m in range(5):
                v = f(v + f(M[i, m] * f(f(B[m, l] * d[m]) * d[l])))
            T[i, l] = v
    C = np.zeros((5, 5), f)
    ok = True
    with np.errstate(all="ignore"):
        for i in range(5):
            for j in range(i, 5):
                v = f(0)
                for l in range(5):
                    v = f(v + f(T[i, l] * M[j, l]))
                v = f(f(d[i] * v) * d[j])
                ok = ok and bool(abs(v) <= f(FINITE))
                C[i, j] = C[j, i] = v
    if not ok:
        return (False, np.zeros((5, 5), f), low) + zero[3:]
    a, V = C.copy(), np.eye(5, dtype=f)
    for _ in range(SWEEPS):
        for p in range(4):
            for q in range(p + 1, 5):
                apq = a[p, q]
                t = f(0)
                if apq != 0:
                    with np.errstate(all="ignore"):
                        theta = f(f(a[q, q] - a[p, p]) / f(f(2) * apq))
                        t = f(f(1 if theta >= 0 else -1) / f(abs(theta) + np.sqrt(f(f(theta * theta) + f(1)))))
                c = f(f(1) / np.sqrt(f(f(t * t) + f(1))))
                s = f(t * c)
                a[p, p] = f(a[p, p] - f(t * apq))
                a[q, q] = f(a[q, q] + f(t * apq))
                a[p, q] = a[q, p] = 0
                for r in range(5):
                    if r != p and r != q:
                        x, y = a[r, p], a[r, q]
                        a[r, p] = a[p, r] = f(f(c * x) - f(s * y))
                        a[r, q] = a[q, r] = f(f(s * x) + f(c * y))
                    x, y = V[r, p], V[r, q]
                    V[r, p] = f(f(c * x) - f(s * y))
                    V[r, q] = f(f(s * x) + f(c * y))
    dg = np.diag(a)
    weak = sign_rule(V[:, int(np.argmax(dg))].copy())
    return True, C, low, np.sort(dg)[::-1].copy(), weak


def sign_rule(v):
    """the component of largest magnitude, the lowest index on ties, is positive"""
    return -v if v[int(np.argmax(np.abs(v)))] < 0 else v


def algebra_ref(normal):
    """the fp64 algebra on the 30 given upper entries -> dict(ok, cov, cov_solve, rho, kappa, eig, vec, weak, sd_rot, sd_dir); the scaled
    route by numpy's Cholesky, the second route by LAPACK solve on the unscaled A"""
    normal = np.asarray(normal, np.float64)
    A, B = _full(normal[:15], np.float64), _full(normal[15:], np.float64)
    out = dict(ok=False, cov=np.zeros((5, 5)), cov_solve=np.zeros((5, 5)), rho=0.0, kappa=0.0, eig=np.zeros(5), vec=np.zeros((5, 5)),
               weak=np.zeros(5), sd_rot=0.0, sd_dir=0.0)
    dg = np.diag(A)
    if not bool((dg > 0).all()):
        return out
    d = 1 / np.sqrt(dg)
    Ah, Bh = A * d[:, None] * d[None, :], B * d[:, None] * d[None, :]
    piv = np.empty(5)                                               # the pivots of the header: the Schur complements' diagonals
    S = Ah.copy()
    for j in range(5):
        piv[j] = S[j, j]
        if not piv[j] > PIVOT_MIN:
            out["rho"] = float(piv[j])
            return out
        S[j + 1:, j + 1:] -= np.outer(S[j + 1:, j], S[j, j + 1:]) / S[j, j]
    Lc = np.linalg.cholesky(Ah)
    Mi = np.linalg.inv(Lc)
    Mh = Mi.T @ Mi
    Ch = Mh @ Bh @ Mh
    C = Ch * d[:, None] * d[None, :]
    C = (C + C.T) / 2
    X = np.linalg.solve(A, B)
    Cs = np.linalg.solve(A, X.T)
    ev, vec = np.linalg.eigh(C)
    ev, vec = ev[::-1].copy(), vec[:, ::-1].copy()
    out.update(ok=True, cov=C, cov_solve=(Cs + Cs.T) / 2, rho=float(piv.min()), kappa=float(np.linalg.cond(Ah)), eig=ev, vec=vec,
               weak=sign_rule(vec[:, 0].copy()), sd_rot=float(np.sqrt(max(C[0, 0] + C[1, 1] + C[2, 2], 0))),
               sd_dir=float(np.sqrt(max(C[3, 3] + C[4, 4], 0))))
    return out


def _one(pose, x1, x2, w0, tau, dt):
    s = _sums(pose, x1, x2, w0, tau, dt)
    red = s["red"]
    zero = (np.zeros((5, 5), dt), np.zeros(6, dt), np.zeros(5, dt), np.zeros(5, dt), np.zeros(8, dt), np.zeros(30, dt), s["absn"], 0.0,
            np.zeros((5, 5)), np.zeros((5, 5)))
    if s["degenerate"] or not bool((np.abs(red) <= FINITE).all()) or red[31] < K_MIN:
        return zero
    with np.errstate(all="ignore"):
        cost = dt(red[33] / red[30])
    if dt is np.float32:
        ok, C, rho, eig, weak = _algebra_f32(red[:30])
        kappa, Cs, vec = 0.0, np.zeros((5, 5)), np.zeros((5, 5))
        sd_rot = np.sqrt(max(dt(dt(C[0, 0] + C[1, 1]) + C[2, 2]), dt(0)))
        sd_dir = np.sqrt(max(dt(C[3, 3] + C[4, 4]), dt(0)))
    else:
        a = algebra_ref(red[:30])
        ok, C, rho, eig, weak, kappa, Cs, vec, sd_rot, sd_dir = (a[k] for k in ("ok", "cov", "rho", "eig", "weak", "kappa", "cov_solve", "vec",
                                                                                "sd_rot", "sd_dir"))
    stat = np.array([1 if ok else -1, red[31], sd_rot, sd_dir, rho, red[32], cost, 0], dt)
    return (C.astype(dt), s["frame"].astype(dt), np.asarray(eig, dt), np.asarray(weak, dt), stat, red[:30].astype(dt), s["absn"], kappa, Cs, vec)


def _batch(pose, x1, x2, w, tau, dt):
    n = x1.shape[0]
    tau = np.broadcast_to(np.asarray(tau, dt), (n,))
    out = [_one(pose[b], x1[b], x2[b], None if w is None else w[b], tau[b], dt) for b in range(n)]
    return Covariance(*(np.stack([o[k] for o in out]) for k in range(7)), np.array([o[7] for o in out]),
                      np.stack([o[8] for o in out]) if dt is np.float64 else None, np.stack([o[9] for o in out]) if dt is np.float64 else None)


def covariance_ref(pose, x1, x2, w=None, tau=0.01):
    """fp64 reference of rp_pose_covariance: pose [n,7], x1, x2 [n,P,2], w [n,P] or None, tau a number or [n] -> Covariance"""
    return _batch(np.asarray(pose, np.float64), np.asarray(x1, np.float64), np.asarray(x2, np.float64), w, tau, np.float64)


def covariance_f32(pose, x1, x2, w=None, tau=0.01):
    """the kernel's arithmetic in numpy float32 (see the module docstring); same arguments and results as covariance_ref"""
    return _batch(np.asarray(pose, np.float32), np.asarray(x1, np.float32), np.asarray(x2, np.float32), w, tau, np.float32)


def window_rows(pose, x1, x2, w, tau):
    """[n]: per problem the number of rows of positive weight whose u lies within NEG_WINDOW of 1 (fp64)"""
    n = len(x1)
    tau = np.broadcast_to(np.asarray(tau, np.float64), (n,))
    out = np.zeros(n, int)
    for b in range(n):
        s = _sums(np.asarray(pose[b], np.float64), np.asarray(x1[b], np.float64), np.asarray(x2[b], np.float64),
                  None if w is None else w[b], tau[b], np.float64)
        out[b] = int(((np.abs(s["u"] - 1) <= NEG_WINDOW) & (s["w"] > 0)).sum())
    return out


def naive_ref(pose, x1, x2, w, tau, sigma):
    """sigma^2 H^-1, H = sum o_p J_p J_p^T with the Cauchy weights of the refinement (one problem, fp64) -- the formula NOT shipped"""
    pose = np.asarray(pose, np.float64)
    t, q = unit_exact(pose[:3])[0], unit_exact(pose[3:])[0]
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    wv = np.ones(len(x1)) if w is None else np.maximum(np.nan_to_num(np.asarray(w, np.float64)), 0)
    H, _ = R.normal_matrix(t, q, x1, x2, wv, float(tau) ** 2)
    return sigma * sigma * np.linalg.inv(H)


# ------------------------------------------------------------------------------------------------ the calibration scenes
Geometry = collections.namedtuple("Geometry", "x1 x2 R t pose")


def mc_geometry(g, P):
    """the geometry of calibration scene g by noisy_scene's recipe: a rotation of up to 0.3 rad, |t| 1 .. 1.5, depths 2 .. 8, field
    +-0.55 -> exact x1, x2 [P,2] (fp64), R, t, and the true pose [7]"""
    rng = np.random.default_rng(g)
    Rm = _rotation(rng, 0.3)
    t = rng.standard_normal(3)
    t *= rng.uniform(1.0, 1.5) / np.linalg.norm(t)
    z = rng.uniform(2.0, 8.0, P)
    xy = rng.uniform(-0.55, 0.55, (P, 2))
    X1 = np.concatenate([xy * z[:, None], z[:, None]], -1)
    X2 = X1 @ Rm.T + t
    assert X2[:, 2].min() > 0.2
    return Geometry(xy, X2[:, :2] / X2[:, 2:], Rm, t, np.concatenate([t / np.linalg.norm(t), R.rot_to_quat(Rm)]))


def mc_draw(geom, rng, sigma, f):
    """one draw on a geometry: Gaussian noise of sigma on both images, a share f of x2 replaced by uniform noise over +-0.6 -> x1, x2 [P,2]"""
    P = len(geom.x1)
    x1 = geom.x1 + sigma * rng.standard_normal((P, 2))
    x2 = geom.x2 + sigma * rng.standard_normal((P, 2))
    bad = rng.permutation(P)[:int(round(f * P))]
    x2[bad] = rng.uniform(-0.6, 0.6, (len(bad), 2))
    return x1, x2


def mc_error(pose_hat, pose_true):
    """the true pose seen from the estimate in the estimate's own five parameters: omega = log(R_hat^T R_true), beta_i = b_i(t_hat) .
    t_true / (t_hat . t_true) -- what the covariance at pose_hat is the covariance of (up to sign and second order)"""
    Rh, th = R.pose_matrix(pose_hat)
    Rt, tt = R.pose_matrix(pose_true)
    dR = Rh.T @ Rt
    ang = np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))
    ax = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2
    om = ax * (ang / np.sin(ang) if ang > 1e-12 else 1.0)
    b1, b2 = tangent_basis_exact(th)
    return np.concatenate([om, [b1 @ tt / (th @ tt), b2 @ tt / (th @ tt)]])


def mc_run(g, P, sigma, f, tau_over_sigma, trials, seed=0, iters=15):
    """`trials` draws on geometry g: refine_ref from the true pose, the sandwich and the naive covariance at the result -> dict of the
    coverage of both at CHI2_5_95 (over the trials with status 1), their mean Mahalanobis^2 / 5, the predicted (root mean C) and the
    empirical (root mean square error) sd_rot / sd_dir in degrees, and the share of status -1"""
    geom = mc_geometry(g, P)
    rng = np.random.default_rng([seed, g, P, int(round(f * 100)), int(round(tau_over_sigma))])
    tau = tau_over_sigma * sigma
    m2s, m2n, pred, emp, bad = [], [], [], [], 0
    for _ in range(trials):
        x1, x2 = mc_draw(geom, rng, sigma, f)
        pose = R.refine_ref(geom.pose[None], x1[None], x2[None], None, tau, iters).pose[0]
        c = covariance_ref(pose[None], x1[None], x2[None], None, tau)
        if c.stat[0, 0] != OK:
            bad += 1
            continue
        e = mc_error(pose, geom.pose)
        m2s.append(float(e @ np.linalg.solve(c.cov[0], e)))
        m2n.append(float(e @ np.linalg.solve(naive_ref(pose, x1, x2, None, tau, sigma), e)))
        pred.append([c.stat[0, 2] ** 2, c.stat[0, 3] ** 2])
        emp.append([e[:3] @ e[:3], e[3:] @ e[3:]])
    m2s, m2n = np.array(m2s), np.array(m2n)
    pred, emp = np.degrees(np.sqrt(np.mean(pred, 0))), np.degrees(np.sqrt(np.mean(emp, 0)))
    return dict(g=g, P=P, f=f, tau_over_sigma=tau_over_sigma, trials=trials, not_determined=bad / trials,
                coverage=float((m2s < CHI2_5_95).mean()), coverage_naive=float((m2n < CHI2_5_95).mean()),
                m2_over_5=float(m2s.mean() / 5), m2_over_5_naive=float(m2n.mean() / 5),
                sd_rot_pred=float(pred[0]), sd_rot_emp=float(emp[0]), sd_dir_pred=float(pred[1]), sd_dir_emp=float(emp[1]))


# ------------------------------------------------------------------------------------------------ the GPU cases
SIGMA = 1e-3
GPU_SHAPES = [(1, 6), (3, 9), (1, 255), (3, 256), (1, 257), (130, 64), (3, 513), (2, 1728)]
ANGLES = (0.0, 3e-4, 1e-3, 0.03)      # the perturbation of problem b is ANGLES[b % 4] rad, in R and in the direction of t
# the seed of every batch, chosen (tools/covariance_table.py --seeds) so that at least half of its problems have status 1 and
# eig[0] / eig[1] >= GAP_MIN, weighted and not
GPU_SEEDS = {(1, 6): 0, (3, 9): 0, (1, 255): 0, (3, 256): 0, (1, 257): 0, (130, 64): 0, (3, 513): 1, (2, 1728): 0}


def gpu_case(n, P, weighted, seed=None):
    """the inputs of one GPU case, float32: pose [n,7], x1, x2 [n,P,2], w [n,P] or None, tau [n].  Problem b: a geometry of its own by
    mc_geometry's recipe, noise SIGMA, 30 % wrong matches for odd b (none below P = 32), tau = 3 SIGMA for b % 4 < 2 else 10 SIGMA, the
    true pose perturbed by ANGLES[b % 4] rad.  weighted: uniform weights in 0.05 .. 1 with a zero, a negative and a NaN weight among them
    (P = 6 keeps all six positive: fewer than six rows is the degenerate case, tested apart)."""
    seed = GPU_SEEDS.get((n, P), 0) if seed is None else seed
    rng = np.random.default_rng([77, n, P, seed])
    pose, x1, x2, tau = np.empty((n, 7)), np.empty((n, P, 2)), np.empty((n, P, 2)), np.empty(n)
    for b in range(n):
        geom = mc_geometry(int(rng.integers(1 << 30)), P)
        x1[b], x2[b] = mc_draw(geom, rng, SIGMA, 0.3 if (b % 2 == 1 and P >= 32) else 0.0)
        tau[b] = (3 if b % 4 < 2 else 10) * SIGMA
        ang = ANGLES[b % 4]
        pose[b] = R.perturbed(geom.pose[None], rng, ang)[0] if ang > 0 else geom.pose
    w = None
    if weighted:
        w = rng.uniform(0.05, 1.0, (n, P)).astype(np.float32)
        if P >= 9:
            w[:, 2], w[:, 5], w[:, P - 1] = 0.0, -1.0, np.nan
    return pose.astype(np.float32), x1.astype(np.float32), x2.astype(np.float32), w, tau.astype(np.float32)


def gpu_cases():
    return [(n, P, weighted) for n, P in GPU_SHAPES for weighted in (False, True)]


def not_determined_problem(P, seed=0, tau=3e-3):
    """a status -1 problem: exact matches of a geometry, then 97 % of the x2 moved 2.2 tau along the normal of their epipolar line, to
    either side: |s| lies between tau and 3 tau for most rows, psi' is negative there, A is not positive definite.
    -> pose [7], x1, x2 [P,2] float32"""
    geom = mc_geometry(5000 + seed, P)
    rng = np.random.default_rng([5, P, seed])
    Rm, t = R.pose_matrix(geom.pose)
    E = R.cross_matrix(t) @ Rm
    l2 = np.concatenate([geom.x1, np.ones((P, 1))], -1) @ E.T
    nrm = l2[:, :2] / np.linalg.norm(l2[:, :2], axis=-1, keepdims=True)
    side = np.where(rng.random(P) < 0.5, -1.0, 1.0) * (rng.random(P) < 0.97)
    x2 = geom.x2 + nrm * (2.2 * tau * side)[:, None]
    return geom.pose.astype(np.float32), geom.x1.astype(np.float32), x2.astype(np.float32)


def gpu_errors(dev, ref):
    """the five ratios the GPU bounds are stated in, of a result `dev` (anything with cov, eig, weak, stat, normal as arrays) against the
    fp64 reference `ref` of the same inputs: (normal, cov / sd / rho, eig, weak, cost) -- each the worst over the batch of error / (bound
    without its constant); the algebra is referred to dev's OWN normal, eig and weak to eigh of dev's OWN cov"""
    r1 = r2 = r3 = r4 = r5 = 0.0
    n = len(dev.stat)
    for b in range(n):
        if ref.stat[b, 0] == DEGENERATE:
            continue
        K = float(ref.stat[b, 1])
        scale = K * EPS32 * ref.abs_normal[b]
        live = scale > 0
        err = np.abs(np.asarray(dev.normal[b], np.float64) - ref.normal[b])
        if live.any():
            r1 = max(r1, float((err[live] / scale[live]).max()))
        r5 = max(r5, abs(float(dev.stat[b, 6]) - ref.stat[b, 6]) / (EPS32 * ref.stat[b, 6]))
        if dev.stat[b, 0] != OK:
            continue
        a = algebra_ref(dev.normal[b])
        if not a["ok"]:
            continue
        sd = np.sqrt(np.diag(a["cov"]))
        unit = EPS32 * a["kappa"]
        r2 = max(r2, float((np.abs(np.asarray(dev.cov[b], np.float64).reshape(5, 5) - a["cov"]) / (unit * np.outer(sd, sd))).max()))
        for k, key in ((2, "sd_rot"), (3, "sd_dir"), (4, "rho")):
            r2 = max(r2, abs(float(dev.stat[b, k]) - a[key]) / (unit * a[key]))
        ev, vec = np.linalg.eigh(np.asarray(dev.cov[b], np.float64).reshape(5, 5))
        ev, vec = ev[::-1], vec[:, ::-1]
        r3 = max(r3, float(np.abs(np.asarray(dev.eig[b], np.float64) - ev).max() / (EPS32 * ev[0])))
        if ev[0] >= GAP_MIN * ev[1]:
            wk = sign_rule(vec[:, 0].copy())
            dw = np.asarray(dev.weak[b], np.float64)
            chord = float(np.linalg.norm(dw / np.linalg.norm(dw) - wk))                  # the sign rule is part of what is compared
            r4 = max(r4, 2 * np.arcsin(min(chord / 2, 1.0)) / (EPS32 * ev[0] / (ev[0] - ev[1])))
    return r1, r2, r3, r4, r5
