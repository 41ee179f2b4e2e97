"""References for include/relpose_triangulate.h (librelpose_triangulate.so), shared by tests/test_triangulate_cpu.py,
tests/test_gpu_triangulate.py, tests/test_gpu_triangulate_contract.py and tools/lab/triangulate_host/run.py.

Every routine is written ONCE, over a dtype: with float64 it is the reference, with float32 (the kernel's order of operations, its
row ownership and the tree of its one reduction) it is the restatement of the kernel's arithmetic that calibrates the GPU bounds -- the
project's rule: a bound is C eps32 scale(ref) with C = 8 x the restatement's worst ratio on the same inputs.  The optimal correction
is checked against a second, independent fp64 route (`second_route`: a Gauss-Newton minimisation over the corrected point of image 1).
Scene builder: the recipe of DESIGN.md 5.8."""
import collections
import functools

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
MIN_NORM, MIN_DEN, INF_SIN2 = 1e-30, 1e-30, 1e-10
TAU = 0.01
NT, ROWS = 256, 7

Structure = collections.namedtuple("Structure", "X aux xc stat")
Structure.__doc__ = "X [n,P,3], aux [n,P,4] = (z1, z2, d2, phi), xc [n,P,4] = (x1c, x2c), stat [n,4]"


# ------------------------------------------------------------------------------------------------ shared arithmetic, over a dtype
def _unit(v):
    """v / |v| with the largest magnitude taken out first, and |v| -- the kernel's `unit`"""
    dt = v.dtype.type
    with np.errstate(all="ignore"):
        m = np.abs(v).max()
        if not m > 0:
            return v, dt(0)
        u = v / m
        ss = dt(0)
        for x in u:
            ss = ss + x * x
        s = np.sqrt(ss)
        return u / s, m * s


def quat_to_rot(q):
    x, y, z, w = q
    one, two = q.dtype.type(1), q.dtype.type(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype=q.dtype)


def cross_times(a, R):
    """[a]x R, row by row as the kernel writes it"""
    return np.stack([a[1] * R[2] - a[2] * R[1], a[2] * R[0] - a[0] * R[2], a[0] * R[1] - a[1] * R[0]]).astype(R.dtype)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def clamp(w, n, P, dt=np.float64):
    """the base weights as the kernel takes them: NULL = ones, a negative weight or a NaN = 0"""
    if w is None:
        return np.ones((n, P), dt)
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(w) > 0, w, 0).astype(dt)


def block_sum(v):
    """sum of v [P] as the kernel forms it in float32: a thread adds its rows t, t + 256, .. one after the other, a wave sums by xor
    shuffles (32, 16, .. 1), the four waves are added ((w0 + w1) + w2) + w3; any other dtype: the plain sum"""
    if v.dtype != np.float32:
        return v.sum()
    pad = np.zeros(NT * ROWS, np.float32)
    pad[:len(v)] = v
    acc = np.zeros(NT, np.float32)
    for i in range((len(v) + NT - 1) // NT):
        acc = acc + pad[i * NT:(i + 1) * NT]
    acc = acc.reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ o]
    wv = acc[:, 0]
    return ((wv[0] + wv[1]) + wv[2]) + wv[3]


def correct(E, x, y, u, v):
    """Lindstrom's two steps for the rows (x, y) <-> (u, v) under E [3,3]: (d1x, d1y, d2x, d2y), the corrections of image 1 and 2"""
    dt = E.dtype.type
    e = E.reshape(9)
    with np.errstate(all="ignore"):
        m0 = e[0] * x + e[1] * y + e[2]
        m1 = e[3] * x + e[4] * y + e[5]
        mz = e[6] * x + e[7] * y + e[8]
        mp0 = e[0] * u + e[3] * v + e[6]
        mp1 = e[1] * u + e[4] * v + e[7]
        c = u * m0 + v * m1 + mz
        a = m0 * (e[0] * mp0 + e[1] * mp1) + m1 * (e[3] * mp0 + e[4] * mp1)
        hb = dt(0.5) * ((m0 * m0 + m1 * m1) + (mp0 * mp0 + mp1 * mp1))
        d = np.sqrt(np.maximum(hb * hb - a * c, dt(0)))
        den = hb + d
        ok = den > dt(MIN_DEN)
        lam = np.where(ok, c / np.where(ok, den, dt(1)), dt(0))
        d2x, d2y, d1x, d1y = lam * m0, lam * m1, lam * mp0, lam * mp1
        m0 = m0 - (e[0] * d1x + e[1] * d1y)
        m1 = m1 - (e[3] * d1x + e[4] * d1y)
        mp0 = mp0 - (e[0] * d2x + e[3] * d2y)
        mp1 = mp1 - (e[1] * d2x + e[4] * d2y)
        den2 = (m0 * m0 + m1 * m1) + (mp0 * mp0 + mp1 * mp1)
        ok = den2 > dt(MIN_DEN)
        lam = np.where(ok, lam * (dt(2) * d) / np.where(ok, den2, dt(1)), dt(0))
        return lam * mp0, lam * mp1, lam * m0, lam * m1


def _one(pose, x1, x2, w, tau, dt):
    """one problem: pose [7], x1, x2 [P,2], w [P] clamped -> (X [P,3], aux [P,4], xc [P,4], stat [4]) in dt"""
    P = len(x1)
    f = dt
    pose = pose.astype(dt)
    K = f((w > 0).sum())
    with np.errstate(all="ignore"):
        t, tn = _unit(pose[:3])
        q, qn = _unit(pose[3:])
        ta = f(tau)
        if not np.isfinite(pose).all() or not tn >= f(MIN_NORM) or not qn >= f(MIN_NORM) or not ta > 0:
            return np.zeros((P, 3), dt), np.zeros((P, 4), dt), np.zeros((P, 4), dt), np.array([0, 0, 0, K], dt)
        tau2 = ta * ta
        R = quat_to_rot(q)
        E = cross_times(t, R)
        x, y, u, v = (a.astype(dt) for a in (x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1]))
        d1x, d1y, d2x, d2y = correct(E, x, y, u, v)
        one = np.ones(P, dt)
        xa, xb = [x - d1x, y - d1y, one], [u - d2x, v - d2y, one]
        dd = (d1x * d1x + d1y * d1y) + (d2x * d2x + d2y * d2y)
        rr = [(R[k, 0] * xa[0] + R[k, 1] * xa[1]) + R[k, 2] for k in range(3)]
        g, txb, txr = _cross(xb, rr), _cross(t, xb), _cross(t, rr)
        gg, nb, nr = _dot(g, g), _dot(xb, xb), _dot(rr, rr)
        phi = np.arctan2(np.sqrt(gg), _dot(xb, rr))
        far = gg < f(INF_SIN2) * nb * nr
        safe = np.where(far, f(1), gg)
        z1 = np.where(far, f(0), _dot(txb, g) / safe)
        z2 = np.where(far, f(0), _dot(txr, g) / safe)
        om = w / (f(1) + dd / tau2)
        s = [block_sum(a.astype(dt)) for a in (w, w * (tau2 * np.log1p(dd / tau2)), om, np.where((z1 > 0) & (z2 > 0), om, f(0)), om * phi)]
        stat = np.array([s[1] / s[0] if s[0] > 0 else 0, s[3] / s[2] if s[0] > 0 and s[2] > 0 else 0,
                         s[4] / s[2] if s[0] > 0 and s[2] > 0 else 0, K], dt)
        X = np.stack([z1 * xa[0], z1 * xa[1], z1], -1)
        return X.astype(dt), np.stack([z1, z2, dd, phi], -1).astype(dt), np.stack([xa[0], xa[1], xb[0], xb[1]], -1).astype(dt), stat


def _batch(pose, x1, x2, w, tau, dt):
    n, P = x1.shape[:2]
    wc = clamp(w, n, P, dt)
    tau = np.broadcast_to(np.asarray(tau, np.float32), (n,))
    return Structure(*[np.stack(a) for a in zip(*[_one(np.asarray(pose[b]), x1[b], x2[b], wc[b], tau[b], dt) for b in range(n)])])


def triangulate_ref(pose, x1, x2, w=None, tau=TAU):
    """the reference: float64"""
    return _batch(pose, x1, x2, w, tau, np.float64)


def triangulate_f32(pose, x1, x2, w=None, tau=TAU):
    """the restatement: float32 in the kernel's order of operations"""
    return _batch(np.asarray(pose, np.float32), x1, x2, w, tau, np.float32)


def pose_matrices(pose):
    """pose [7] -> (R, t unit, E = [t]x R) in fp64"""
    p = np.asarray(pose, np.float64)
    t, q = p[:3] / np.linalg.norm(p[:3]), p[3:] / np.linalg.norm(p[3:])
    R = quat_to_rot(q)
    return R, t, cross_times(t, R)


# ------------------------------------------------------------------------------------------------ the second route
def second_route(E, x1, x2, iters=60):
    """the squared reprojection error by an independent route, fp64: minimise over the corrected point p of image 1
    f(p) = |x1 - p|^2 + dist^2(x2, the epipolar line E ph) by Gauss-Newton on the three residuals (p - x1, s(p)), s the signed distance
    of x2 from the line, started at x1.  At convergence J^T r = 0: a stationary point of f itself, not of an approximation."""
    E = np.asarray(E, np.float64)
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    h2 = np.concatenate([x2, np.ones_like(x2[:, :1])], -1)
    mp = (h2 @ E)[:, :2]                                     # d (x2h^T E ph) / d p, constant
    p = x1.copy()
    for _ in range(iters):
        l = np.concatenate([p, np.ones_like(p[:, :1])], -1) @ E.T
        c = (h2 * l).sum(-1)
        nn = np.sqrt(l[:, 0] ** 2 + l[:, 1] ** 2)
        s = c / nn
        gn = (l[:, :1] * E[0, :2] + l[:, 1:2] * E[1, :2]) / nn[:, None]
        gs = mp / nn[:, None] - (c / nn ** 2)[:, None] * gn
        # (I + gs gs^T) delta = -((p - x1) + gs s), by Sherman-Morrison
        rhs = -((p - x1) + gs * s[:, None])
        p = p + rhs - gs * ((gs * rhs).sum(-1) / (1 + (gs * gs).sum(-1)))[:, None]
    l = np.concatenate([p, np.ones_like(p[:, :1])], -1) @ E.T
    return ((p - x1) ** 2).sum(-1) + (h2 * l).sum(-1) ** 2 / (l[:, 0] ** 2 + l[:, 1] ** 2), p


# ------------------------------------------------------------------------------------------------ scenes
def scenes(n, P, seed, depth=3.0, noise=0.0, outliers=0.0):
    """n problems of P points: a rotation of at most 0.3 rad about a random axis, a unit baseline in a random sideways direction (|t_z| <= 0.3 |t_xy|), points of image 1
    uniform in [-0.5, 0.5]^2 at depth `depth` U(0.7, 1.3), gaussian noise of sigma `noise` on both images, a share `outliers` of x2
    replaced by uniform noise -> (x1, x2 [n,P,2] float32, pose [n,7] fp64 (t unit, q xyzw), the true points X [n,P,3] fp64 in the frame
    of camera 1, outlier mask [n,P])"""
    rng = np.random.default_rng(1000 * seed + 17)
    x1 = np.empty((n, P, 2))
    x2 = np.empty((n, P, 2))
    pose = np.empty((n, 7))
    Xt = np.empty((n, P, 3))
    bad = np.zeros((n, P), bool)
    for b in range(n):
        ax = rng.standard_normal(3)
        ang = rng.uniform(0.05, 0.3)
        ax = ax / np.linalg.norm(ax) * np.sin(ang / 2)
        q = np.array([ax[0], ax[1], ax[2], np.cos(ang / 2)])
        az = rng.uniform(0, 2 * np.pi)
        t = np.array([np.cos(az), np.sin(az), rng.uniform(-0.3, 0.3)])     # sideways: the epipoles lie outside the images
        t /= np.linalg.norm(t)
        R = quat_to_rot(q)
        p = rng.uniform(-0.5, 0.5, (P, 2))
        z = depth * rng.uniform(0.7, 1.3, P)
        X = np.concatenate([p, np.ones((P, 1))], -1) * z[:, None]
        Y = X @ R.T + t
        x1[b], x2[b] = p, Y[:, :2] / Y[:, 2:]
        x1[b] += noise * rng.standard_normal((P, 2))
        x2[b] += noise * rng.standard_normal((P, 2))
        k = int(round(outliers * P))
        if k:
            idx = rng.choice(P, k, replace=False)
            x2[b, idx] = rng.uniform(-0.5, 0.5, (k, 2))
            bad[b, idx] = True
        pose[b], Xt[b] = np.concatenate([t, q]), X
    return x1.astype(np.float32), x2.astype(np.float32), pose, Xt, bad


def weights(n, P, seed):
    """base weights with 40 % zeros, a negative one and a NaN per problem (where P allows)"""
    rng = np.random.default_rng(seed + 7 * P + n)
    w = rng.uniform(0.05, 1.0, (n, P)).astype(np.float32)
    w[rng.uniform(size=(n, P)) < 0.4] = 0
    if P >= 5:
        w[:, 1], w[:, 3] = -1.0, np.nan
    return w


# the GPU test's cases: (n, P) x weights x depth x noise; the degenerate problems ride in the batches with n > 1
SHAPES = [(1, 1), (3, 5), (2, 255), (2, 256), (2, 257), (1, 1728), (130, 64)]
CASES = [(n, P, wt, D, nz) for (n, P) in SHAPES for wt, D, nz in ((False, 3.0, 1e-3), (True, 30.0, 0.0), (True, 300.0, 2e-2), (False, 300.0, 0.0))]


@functools.lru_cache(maxsize=None)
def inputs(n, P, weighted, depth, noise):
    """(pose float32 [n,7], x1, x2, w or None, tau [n]) of a case: 10 % outliers, the pose moved off the truth a little (so that exact
    scenes, too, have a correction to make), problem 1 of a batch degenerate (t = 0), problem 2 with tau = 0"""
    x1, x2, pose, _, _ = scenes(n, P, 3 + n + P, depth, noise, 0.1 if P >= 10 else 0.0)
    rng = np.random.default_rng(n * P)
    pose = pose + 1e-3 * rng.standard_normal(pose.shape)
    pose[:, :3] *= rng.uniform(0.5, 2.0, (n, 1))                 # any scale: normalised internally
    tau = np.full(n, TAU, np.float32)
    if n > 1:
        pose[1, :3] = 0
    if n > 2:
        tau[2] = 0
    return pose.astype(np.float32), x1, x2, (weights(n, P, 5) if weighted else None), tau


@functools.lru_cache(maxsize=None)
def reference(n, P, weighted, depth, noise):
    pose, x1, x2, w, tau = inputs(n, P, weighted, depth, noise)
    return triangulate_ref(pose, x1, x2, w, tau)


# ------------------------------------------------------------------------------------------------ the comparison
def cost64(d2, w, tau):
    """the robust cost in fp64 of given d2 [n,P] under clamped weights w [n,P]: [n] (0 where the weights sum to 0 or tau is not > 0)"""
    d2, w = np.asarray(d2, np.float64), np.asarray(w, np.float64)
    t2 = np.asarray(tau, np.float64)[:, None] ** 2
    with np.errstate(all="ignore"):
        c = (w * t2 * np.log1p(d2 / t2)).sum(-1) / w.sum(-1)
    return np.where((w.sum(-1) > 0) & (t2[:, 0] > 0), c, 0.0)


def ratios(out, ref, w, tau):
    """the worst error of `out` (the device's, the restatement's or the host run's Structure) against the fp64 `ref`, each over
    eps32 x its scale:
        xc     1                                  d2     sqrt(d2) + eps32          phi    1
        z, X   |value| / sin(phi): eps / sin(phi), relative, is the conditioning of a ray intersection (X: the norm of the point)
        cost   against the fp64 cost of out's OWN d2, sqrt(c) + eps32 (the form of 5.4)
        share  the distance to the interval the fp64 share spans when every row with |z| inside `band` eps32 |z| / sin(phi) counts
               either way, over 1
        par    against the fp64 mean of the reference, over 1
    Rows within a factor 4 of the at-infinity threshold in the reference may fall on either side: they are left out of z and X, and
    their share is returned (`left_out`); `flags` counts the other rows that are at infinity on one side only."""
    n, P = ref.X.shape[:2]
    r = {}
    z1, z2, d2, phi = (ref.aux[..., k] for k in range(4))
    sin = np.sin(phi)
    edge = (sin > 0.25e-5) & (sin < 4e-5)
    r["left_out"] = float(edge.mean())
    keep = ~edge                                                  # (a degenerate problem is all zero on both sides: its rows stay in)
    r["flags"] = float(((out.aux[..., 0] == 0) != (z1 == 0))[keep].sum())          # rows at infinity on one side only
    r["xc"] = float(np.abs(out.xc - ref.xc).max() / EPS32) if out.xc is not None else 0.0
    r["d2"] = float((np.abs(out.aux[..., 2] - d2) / (EPS32 * (np.sqrt(d2) + EPS32))).max())
    r["phi"] = float(np.abs(out.aux[..., 3] - phi).max() / EPS32)
    s = np.where(sin > 0, sin, 1.0)
    zr = 0.0
    for k, z in enumerate((z1, z2)):
        m = keep & (z != 0)
        zr = max(zr, float((np.abs(out.aux[..., k] - z)[m] * s[m] / (EPS32 * np.abs(z[m]))).max(initial=0)))
        m0 = keep & (z == 0)
        zr = max(zr, float(np.abs(out.aux[..., k][m0]).max(initial=0)) / EPS32)       # a reference depth of exactly 0: at infinity, or degenerate
    r["z"] = zr
    nX = np.linalg.norm(ref.X, axis=-1)
    m = keep & (nX > 0)
    r["X"] = float((np.abs(out.X - ref.X).max(-1)[m] * s[m] / (EPS32 * nX[m])).max(initial=0))
    r["X"] = max(r["X"], float(np.abs(out.X[keep & (nX == 0)]).max(initial=0)) / EPS32)
    wc = clamp(w, n, P)
    tau = np.broadcast_to(np.asarray(tau, np.float64), (n,))
    c = cost64(out.aux[..., 2], wc, tau) * (np.abs(out.stat[:, :3]).sum(-1) + np.abs(ref.stat[:, :3]).sum(-1) > 0)
    r["cost"] = float((np.abs(out.stat[:, 0] - c) / (EPS32 * (np.sqrt(c) + EPS32))).max())
    r["par"] = float(np.abs(out.stat[:, 2] - ref.stat[:, 2]).max() / EPS32)
    r["K"] = float(np.abs(out.stat[:, 3] - ref.stat[:, 3]).max())
    return r


def share_ratio(out, ref, w, tau, band=None):
    """the front share of `out` against the fp64 interval [lo, hi] of the reference: a row whose |z1| or |z2| is within
    band eps32 |z| / sin(phi) of 0 -- it can carry either sign in float32 --, or within a factor 4 of the at-infinity threshold, counts
    as not in front for lo and as in front for hi; the distance to the interval over eps32"""
    n, P = ref.X.shape[:2]
    band = C_Z if band is None else band
    z1, z2, d2, phi = (ref.aux[..., k] for k in range(4))
    sin = np.sin(phi)
    wc = clamp(w, n, P)
    t2 = np.broadcast_to(np.asarray(tau, np.float64), (n,))[:, None] ** 2
    with np.errstate(all="ignore"):
        om = np.where(t2 > 0, wc / (1 + d2 / np.where(t2 > 0, t2, 1)), 0)
    edge = (sin > 0.25e-5) & (sin < 4e-5)
    # |z - z_ref| <= band eps |z_ref| / sin(phi) leaves the sign alone unless band eps / sin(phi) >= 1
    unsure = edge | ((band * EPS32 >= sin) & (sin >= 1e-5))
    front = (z1 > 0) & (z2 > 0)
    tot = om.sum(-1)
    ok = tot > 0
    lo = np.where(ok, (om * (front & ~unsure)).sum(-1) / np.where(ok, tot, 1), 0)
    hi = np.where(ok, (om * (front | unsure)).sum(-1) / np.where(ok, tot, 1), 0)
    dead = np.abs(ref.stat[:, :3]).sum(-1) == 0
    lo, hi = np.where(dead, 0, lo), np.where(dead, 0, hi)
    s = out.stat[:, 1]
    return float(np.maximum(np.maximum(lo - s, s - hi), 0).max() / EPS32)


# the worst ratios of the float32 restatement over CASES, measured on the CPU (tests/test_triangulate_cpu.py asserts that it stays
# inside them), and the bounds of the GPU test and of the host run: C = 8 x each -- the project's rule; nothing was fixed in advance
RESTATEMENT = {"xc": 0.89, "d2": 2.65, "phi": 1.32, "z": 2.06, "X": 1.78, "cost": 0.0232, "par": 0.82, "share": 3.24}
C_XC, C_D2, C_PHI, C_Z, C_X, C_COST, C_PAR, C_SHARE = (8 * RESTATEMENT[k] for k in ("xc", "d2", "phi", "z", "X", "cost", "par", "share"))


def within(r, share):
    return (r["xc"] <= C_XC and r["d2"] <= C_D2 and r["phi"] <= C_PHI and r["z"] <= C_Z and r["X"] <= C_X and r["cost"] <= C_COST
            and r["par"] <= C_PAR and r["K"] == 0 and share <= C_SHARE and r["left_out"] <= 0.1 and r["flags"] == 0)
