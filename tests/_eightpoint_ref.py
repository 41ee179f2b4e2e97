"""References for rp_eight_point (include/relpose_eightpoint.h), numpy only, no GPU and no library.

  eight_point_ref    the algorithm of the header in fp64 with LAPACK: weighted Hartley normalisation about a pivot, the rows
                     sqrt(w) (x2h (x) x1h), the null vector from the FULL V of numpy.linalg.svd (at P = 8 the thin SVD has no ninth
                     vector), F = T2^T F^ T1, E = U diag(1, 1, 0) V^T, the sign rule, Cauchy IRLS on the Sampson distance.
  eight_point_f32    the kernel's arithmetic restated in numpy float32: the same normalisation, the one-sided (Hestenes) Jacobi on
                     the row matrix with the kernel's pair order, threshold and sweep count, column norms as singular values.  Only
                     the order of the sums differs (numpy's pairwise sums against the kernel's wave / LDS tree).  The GPU tests'
                     bounds are calibrated against it: 8 x its largest error on the same inputs.
  scenes / true_essential / sampson64   synthetic two-view geometry in the convention X2 = R X1 + t, x2^T E x1 = 0.
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
SWEEPS = 9           # csrc_eightpoint/eight_point.hip: SWEEPS
SKIP = 1e-12         # the relative rotation threshold of svd3x3_dev
MIN_SCALE = 1e-30    # a weighted mean distance below this counts as 0


# ------------------------------------------------------------------------------------------------ synthetic scenes
def _rotation(rng, max_angle):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(0.3, 1.0) * max_angle
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def true_essential(R, t):
    t = t / np.linalg.norm(t)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ R


def scenes(n, P, seed, max_angle=0.5):
    """n two-view scenes of P points in general position, fp64: x1, x2 [n,P,2], E_true [n,3,3] (singular values 1, 1, 0).
    Points lie 2 .. 8 units in front of camera 1 inside a field of view of about 60 degrees; |t| is 0.5 .. 1.5."""
    rng = np.random.default_rng(1000 * seed + P)
    x1, x2, E = np.empty((n, P, 2)), np.empty((n, P, 2)), np.empty((n, 3, 3))
    for b in range(n):
        R = _rotation(rng, max_angle)
        t = rng.standard_normal(3)
        t *= rng.uniform(0.5, 1.5) / np.linalg.norm(t)
        z = rng.uniform(2.0, 8.0, P)
        xy = rng.uniform(-0.55, 0.55, (P, 2))
        X1 = np.concatenate([xy * z[:, None], z[:, None]], -1)
        X2 = X1 @ R.T + t
        assert X2[:, 2].min() > 0.2
        x1[b], x2[b], E[b] = xy, X2[:, :2] / X2[:, 2:], true_essential(R, t)
    return x1, x2, E


WIDE_KINDS = ("wide", "beyond120", "half_turn", "axis_t")
MAX_X2 = 3.6         # wide_scenes: the largest image coordinate it accepts (the bounds of the GPU tests assume terms of order 1)


def shepperd_branch(R):
    """which pivot the rotation -> quaternion code takes: 0 the trace (> 0), 1 / 2 / 3 the largest of R00 / R11 / R22"""
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return 0
    if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        return 1
    return 2 if R[1, 1] > R[2, 2] else 3


def _axis_angle(axis, a):
    """(R, q xyzw with w >= 0) of a rotation by 0 <= a <= pi about the unit axis; a = pi exactly: R = 2 a a^T - I, w = 0"""
    if a == np.pi:
        return 2 * np.outer(axis, axis) - np.eye(3), np.concatenate([axis, [0.0]])
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K, np.concatenate([axis * np.sin(a / 2), [np.cos(a / 2)]])


def wide_scenes(n, P, seed, kind):
    """n two-view scenes with a wide relative rotation, fp64: x1, x2 [n,P,2], E_true [n,3,3] (singular values 1, 1, 0) and the true pose
    [n,7] = (t unit, q xyzw with w >= 0), X2 = R X1 + t.  kind:
      "wide"       angle uniform in 0.5 .. 2.0 rad about a random axis
      "beyond120"  angle uniform in 2.2 .. 3.1 rad (the trace of R is negative) about e_(b mod 3) + 0.25 N(0, 1): each of the three
                   non-trace pivots of the rotation -> quaternion conversion is the largest for a third of the problems
      "half_turn"  angle pi exactly about the same axes, q.w = 0; problems 0, 1, 2 turn about e_0, e_1, e_2 themselves (R diagonal)
      "axis_t"     a "wide" rotation; even problems have t = +-e_k exactly, odd ones a t whose two smallest magnitudes are equal
    Points as in `scenes` (2 .. 8 in front of camera 1, |xy| <= 0.55 z); t (0.5 .. 1.5 long) is then lifted along camera 2's axis until
    every point has z2 >= 2 and moved sideways by half the mean lateral offset of the points in camera 2, so nothing is rejected.
    "axis_t" cannot move t: its points are a box of side 1.2 centred 8 .. 10 along the bisector of the two optical axes (|t| = 1).
    Asserted here: every point is in front of both cameras, |x2| <= MAX_X2, and for the two large-angle kinds every non-trace pivot is
    taken by at least n / 4 problems."""
    assert kind in WIDE_KINDS, kind
    rng = np.random.default_rng(1000 * seed + P + 100003 * (1 + WIDE_KINDS.index(kind)))
    x1, x2, E, pose = np.empty((n, P, 2)), np.empty((n, P, 2)), np.empty((n, 3, 3)), np.empty((n, 7))
    branch = np.empty(n, int)
    for b in range(n):
        if kind in ("wide", "axis_t"):
            axis, a = rng.standard_normal(3), rng.uniform(0.5, 2.0)
        else:
            axis = np.eye(3)[b % 3] + (0.25 * rng.standard_normal(3) if (kind == "beyond120" or b >= 3) else 0.0)
            a = rng.uniform(2.2, 3.1) if kind == "beyond120" else np.pi
        axis = axis / np.linalg.norm(axis)
        R, q = _axis_angle(axis, a)
        if kind == "axis_t":
            k, sgn = (b // 2) % 3, 1.0 - 2.0 * ((b // 6) % 2)
            if b % 2 == 0:
                t = sgn * np.eye(3)[k]
            else:
                small = rng.uniform(0.1, 0.5)
                t = np.full(3, small) * rng.choice([-1.0, 1.0], 3)
                t[k] = sgn * np.sqrt(1 - 2 * small * small)
            d = np.array([0, 0, 1.0]) + R.T[:, 2]                   # the bisector of the optical axes, in camera 1's frame
            X1 = rng.uniform(8.0, 10.0) * d / np.linalg.norm(d) + rng.uniform(-0.6, 0.6, (P, 3))
            X2 = X1 @ R.T + t
        else:
            t = rng.standard_normal(3)
            t *= rng.uniform(0.5, 1.5) / np.linalg.norm(t)
            z = rng.uniform(2.0, 8.0, P)
            X1 = np.concatenate([rng.uniform(-0.55, 0.55, (P, 2)) * z[:, None], z[:, None]], -1)
            Xr = X1 @ R.T
            t[2] += max(0.0, 2.0 - (Xr[:, 2] + t[2]).min())
            t[:2] -= 0.5 * (Xr[:, :2] + t[:2]).mean(0)
            X2 = Xr + t
        assert X1[:, 2].min() > 0.5 and X2[:, 2].min() > 0.5, (kind, b)
        x1[b], x2[b], E[b] = X1[:, :2] / X1[:, 2:], X2[:, :2] / X2[:, 2:], true_essential(R, t)
        pose[b] = np.concatenate([t / np.linalg.norm(t), q])
        branch[b] = shepperd_branch(R)
    assert np.abs(x2).max() <= MAX_X2 and np.abs(x1).max() <= MAX_X2, (kind, np.abs(x1).max(), np.abs(x2).max())
    if kind in ("beyond120", "half_turn"):
        assert all(int((branch == k).sum()) >= n // 4 for k in (1, 2, 3)), np.bincount(branch, minlength=4)
    return x1, x2, E, pose


def noisy_scene(seed, P=576, outliers=0.1, sigma=1e-3):
    """one wide-baseline scene (|t| 1 .. 1.5 against depths of 2 .. 8, a rotation of up to 0.3 rad) of P points with Gaussian noise of
    `sigma` on both images and a share `outliers` of x2 replaced by uniform noise over the field of view:
    float32 x1, x2 [1,P,2], E_true [1,3,3], inlier mask [P]"""
    rng = np.random.default_rng(7000 + seed)
    R = _rotation(rng, 0.3)
    t = rng.standard_normal(3)
    t *= rng.uniform(1.0, 1.5) / np.linalg.norm(t)
    z = rng.uniform(2.0, 8.0, P)
    xy = rng.uniform(-0.55, 0.55, (P, 2))
    X1 = np.concatenate([xy * z[:, None], z[:, None]], -1)
    X2 = X1 @ R.T + t
    assert X2[:, 2].min() > 0.2
    x1 = xy[None] + sigma * rng.standard_normal((1, P, 2))
    x2 = (X2[:, :2] / X2[:, 2:])[None] + sigma * rng.standard_normal((1, P, 2))
    bad = rng.permutation(P)[:int(round(outliers * P))]
    x2[0, bad] = rng.uniform(-0.6, 0.6, (len(bad), 2))
    inlier = np.ones(P, bool)
    inlier[bad] = False
    return x1.astype(np.float32), x2.astype(np.float32), true_essential(R, t)[None], inlier


def up_to_sign(E, ref):
    """min(|E - ref|_F, |E + ref|_F) per problem"""
    E, ref = np.asarray(E, np.float64).reshape(-1, 9), np.asarray(ref, np.float64).reshape(-1, 9)
    return np.minimum(np.linalg.norm(E - ref, axis=-1), np.linalg.norm(E + ref, axis=-1))


def sampson64(E, x1, x2):
    """readout.sampson_distance in fp64 numpy; a zero denominator gives 0.  E [n,3,3] or [n,9], x [n,P,2] -> [n,P]"""
    E = np.asarray(E, np.float64).reshape(-1, 3, 3)
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    one = np.ones_like(x1[..., :1])
    h1, h2 = np.concatenate([x1, one], -1), np.concatenate([x2, one], -1)
    l2 = h1 @ E.transpose(0, 2, 1)
    l1 = h2 @ E
    num = (h2 * l2).sum(-1) ** 2
    den = l2[..., 0] ** 2 + l2[..., 1] ** 2 + l1[..., 0] ** 2 + l1[..., 1] ** 2
    return np.where(den > 0, num / np.where(den > 0, den, 1), 0.0)


# ------------------------------------------------------------------------------------------------ shared steps (dtype generic)
def _normalise(x, w, wsum, dt):
    """weighted Hartley transform of one image's points about the pivot x[0]: (normalised points, scale, centroid) or None"""
    d = x - x[0]
    c = x[0] + (w[:, None] * d).sum(0, dtype=dt) / wsum
    r = x - c
    m = (w * np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])).sum(dtype=dt) / wsum
    if not m >= MIN_SCALE:
        return None
    s = dt(np.sqrt(dt(2))) / m
    return r * s, s, c


def _rows(x1n, x2n, w, dt):
    q = np.sqrt(w)
    one = np.ones_like(q)
    cols = [x2n[:, 0] * x1n[:, 0], x2n[:, 0] * x1n[:, 1], x2n[:, 0], x2n[:, 1] * x1n[:, 0], x2n[:, 1] * x1n[:, 1], x2n[:, 1],
            x1n[:, 0], x1n[:, 1], one]
    return np.stack([q * c for c in cols], -1).astype(dt)


def _finish(f, sig, s1, c1, s2, c2, wsum, dt, svd3):
    """null vector f [9] of the normalised rows and their singular values (any order) -> (E [9], stat [4])"""
    Fh = f.reshape(3, 3)
    T1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1]], dtype=dt)
    T2 = np.array([[s2, 0, -s2 * c2[0]], [0, s2, -s2 * c2[1]], [0, 0, 1]], dtype=dt)
    F = T2.T @ Fh @ T1
    U, S, Vt = svd3(F)
    E = (U[:, :2] @ Vt[:2]).reshape(9)
    k = int(np.argmax(np.abs(E)))            # the first of equal maxima
    if E[k] < 0:
        E = -E
    sig = np.sort(sig)[::-1]
    stat = np.array([sig[8] / sig[0], sig[7] / sig[0], S[1] / S[0] if S[0] > 0 else 0, wsum], dtype=dt)
    return E.astype(dt), stat


def _solve(x1, x2, w, dt, null_space, svd3):
    """one weighted solve of one problem -> (E [9], stat [4])"""
    wsum = w.sum(dtype=dt)
    degenerate = (np.zeros(9, dt), np.array([0, 0, 0, wsum], dtype=dt))
    if int((w > 0).sum()) < 8:
        return degenerate
    n1, n2 = _normalise(x1, w, wsum, dt), _normalise(x2, w, wsum, dt)
    if n1 is None or n2 is None:
        return degenerate
    f, sig = null_space(_rows(n1[0], n2[0], w, dt))
    return _finish(f, sig, n1[1], n1[2], n2[1], n2[2], wsum, dt, svd3)


def _irls(x1, x2, w, tau, iters, dt, null_space, svd3, sampson, history):
    n, P = x1.shape[:2]
    E, stat, wk = np.zeros((n, 9), dt), np.zeros((n, 4), dt), np.empty((n, P), dt)
    hist = []
    for b in range(n):
        w0 = np.ones(P, dt) if w is None else np.maximum(np.asarray(w[b], dt), 0)
        cur, track = w0, []
        for k in range(iters + 1):
            if k:
                d = sampson(E[b][None], x1[b][None], x2[b][None])[0].astype(dt)
                cur = np.where(d > 0, w0 / (1 + d / (dt(tau[b]) * dt(tau[b]))), w0).astype(dt)
            E[b], stat[b] = _solve(x1[b], x2[b], cur, dt, null_space, svd3)
            track.append(E[b].copy())
            if not E[b].any():                   # a degenerate solve ends its problem
                break
        wk[b] = cur
        hist.append(track)
    return (E.reshape(n, 3, 3), stat, wk) + ((hist,) if history else ())


# ------------------------------------------------------------------------------------------------ fp64, LAPACK
def _null_lapack(A):
    _, s, Vt = np.linalg.svd(A, full_matrices=A.shape[0] < 9)
    sig = np.zeros(9)
    sig[:len(s)] = s
    return Vt[8], sig


def _svd3_lapack(F):
    return np.linalg.svd(F)


def eight_point_ref(x1, x2, w=None, tau=None, iters=0, history=False):
    """fp64 reference of rp_eight_point: x1, x2 [n,P,2], w [n,P] or None, tau [n] -> (E [n,3,3], stat [n,4], weights of the last
    solve [n,P]); history=True appends the E of every round per problem"""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    return _irls(x1, x2, w, tau, iters, np.float64, _null_lapack, _svd3_lapack, sampson64, history)


# ------------------------------------------------------------------------------------------------ float32 restatement
def jacobi_null_f32(A, sweeps=SWEEPS):
    """one-sided Jacobi on the columns of A [P,9] float32: cyclic pairs (0,1), (0,2), ... (7,8), `sweeps` times, a rotation skipped when
    |gamma| <= 1e-12 sqrt(alpha beta) -> (V column of the smallest column norm, the nine column norms)"""
    f = np.float32
    W, V = np.array(A, dtype=f), np.eye(9, dtype=f)
    with np.errstate(over="ignore"):             # zeta^2 may overflow to inf: t = 0, no rotation -- as in the kernel
        return _jacobi_sweeps(W, V, sweeps, f)


def _jacobi_sweeps(W, V, sweeps, f):
    for _ in range(sweeps):
        for p in range(8):
            for q in range(p + 1, 9):
                a, b = W[:, p], W[:, q]
                al, be, ga = (a * a).sum(dtype=f), (b * b).sum(dtype=f), (a * b).sum(dtype=f)
                if not (abs(ga) > f(SKIP) * np.sqrt(al * be) and ga != 0):
                    continue
                zeta = (be - al) / (f(2) * ga)
                t = np.copysign(f(1), zeta) / (abs(zeta) + np.sqrt(f(1) + zeta * zeta))
                c = f(1) / np.sqrt(f(1) + t * t)
                s = c * t
                W[:, p], W[:, q] = c * a - s * b, s * a + c * b
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
    sig = np.sqrt((W * W).sum(0, dtype=f))
    return V[:, int(np.argmin(sig))], sig


def _svd3_f32(F):
    U, S, Vt = np.linalg.svd(F.astype(np.float32))
    return U, S, Vt


def _sampson32(E, x1, x2):
    f = np.float32
    E = E.reshape(3, 3).astype(f)
    x1, x2 = x1[0].astype(f), x2[0].astype(f)
    l2 = [E[r, 0] * x1[:, 0] + E[r, 1] * x1[:, 1] + E[r, 2] for r in range(3)]
    l1 = [E[0, c] * x2[:, 0] + E[1, c] * x2[:, 1] + E[2, c] for c in range(2)]
    r = x2[:, 0] * l2[0] + x2[:, 1] * l2[1] + l2[2]
    den = l2[0] * l2[0] + l2[1] * l2[1] + l1[0] * l1[0] + l1[1] * l1[1]
    return np.where(den > 0, r * r / np.where(den > 0, den, f(1)), f(0))[None]


def eight_point_f32(x1, x2, w=None, tau=None, iters=0, sweeps=SWEEPS, history=False):
    """the kernel's arithmetic in numpy float32 (see the module docstring); same arguments and results as eight_point_ref"""
    x1, x2 = np.asarray(x1, np.float32), np.asarray(x2, np.float32)
    return _irls(x1, x2, w, tau, iters, np.float32, lambda A: jacobi_null_f32(A, sweeps), _svd3_f32, _sampson32, history)
