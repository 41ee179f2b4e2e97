"""References for include/relpose_resection.h (librelpose_resection.so), shared by tests/test_resection_cpu.py,
tests/test_gpu_resection.py, tests/test_gpu_resection_contract.py and tools/lab/resection_host/run.py.

Every routine of the header is written ONCE, over a dtype.  The three-point solver is fp64 in the kernel, too, so for it the dtype only
decides how the poses are rounded; the SECOND ROUTE that checks its solution set is all roots of Grunert's quartic by numpy.roots
(p3p_roots_lapack), each kept if the three depths are positive.  With float64 the scoring, the selection and the Levenberg-Marquardt
iteration are the reference; with float32 and the kernel's statements in the kernel's order they are the restatement that calibrates
the GPU bounds: a bound is C eps32 scale(ref) with C = 8 x the restatement's worst ratio on the same inputs (WORST below).  The sampler
is the contract sampler restated with three draws.  Scene builders: three views (hub, a, c) of one point cloud, and the first pair's
structure by the header of rp_triangulate restated in fp64."""
import collections

import numpy as np

from tests import _consensus_ref as C
from tests import _homography_ref as H
from tests import _rotation_ref as RT

FLT_MAX = C.FLT_MAX
EPS32 = H.EPS32
MIN_SCALE, DEN_MIN, D_MAX, FINITE = 1e-30, 1e-30, 1e30, 3.0e38
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-7, 1e7
SIDE_MIN, AREA_MIN, SPAN_MIN, LEAD_MIN, DEN_V_MIN, DISC_BAND, RESOLVENT_MIN = 1e-12, 1e-12, 1e-12, 1e-12, 1e-9, 1e-9, 1e-14
TAU, SEED = 0.012, 1                                     # half a token pitch of the scenes below

Consensus = collections.namedtuple("Consensus", "pose best stat weights hyp_pose hyp_cost hyp_count samples margin")
Consensus.__doc__ = """pose [n,7], best [n], stat [n,4], weights [n,P], hyp_pose [n,M,7], hyp_cost [n,M], hyp_count [n,M], samples [n,M,3]
as the header documents them; margin [n,M]: how far the sample's decisions (real or complex roots, the gates of a solution) are from
their thresholds, relative -- a rule of the reference alone (inf for an invalid sample)"""
Refined = collections.namedtuple("Refined", "pose stat weights kappa")


# ------------------------------------------------------------------------------------------------ the sampler
def draw3(seed, i, m, K):
    """the three indices c_0, c_1, c_2 into pos of hypotheses m (an int array) of problem i: [len(m), 3]; K >= 3"""
    m = np.atleast_1d(np.asarray(m, np.uint64))
    base = C.mix((np.uint64(seed & 0xFFFFFFFF) + np.uint64(C.GOLDEN) * np.uint64(i + 1)) & np.uint64(0xFFFFFFFF))
    s = C.mix(base ^ m)
    c = np.zeros((len(m), 3), np.int64)
    for k in range(3):
        r = C.mix((s + np.uint64((C.GOLDEN * (k + 1)) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF))
        j = K - 3 + k
        t = ((r * np.uint64(j + 1)) >> np.uint64(32)).astype(np.int64)
        seen = (c[:, :k] == t[:, None]).any(-1)
        c[:, k] = np.where(seen, j, t)
    return c


def sample_rows3(w, n, P, seed, M, first=0):
    """(pos per problem, samples [n,M,3] of row numbers; zeros where K < 3); problem b of the batch has index first + b"""
    wc = C.clamp(w, n, P)
    pos = [np.flatnonzero(wc[b] > 0) for b in range(n)]
    samples = np.zeros((n, M, 3), np.int64)
    for b in range(n):
        if len(pos[b]) >= 3:
            samples[b] = pos[b][draw3(seed, first + b, np.arange(M), len(pos[b]))]
    return pos, samples


# ------------------------------------------------------------------------------------------------ shared arithmetic, over a dtype
def quat_to_rot(q):
    """q [...,4] xyzw -> R [...,9], the statements of csrc/two_view.h in q's dtype"""
    f = q.dtype.type
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([f(1) - f(2) * (y * y + z * z), f(2) * (x * y - z * w), f(2) * (x * z + y * w),
                     f(2) * (x * y + z * w), f(1) - f(2) * (x * x + z * z), f(2) * (y * z - x * w),
                     f(2) * (x * z - y * w), f(2) * (y * z + x * w), f(1) - f(2) * (x * x + y * y)], -1)


def project(pose, X):
    """(m [...,P,3], Y = R X [...,P,3]) of the header at pose [...,7] for X [P,3], in pose's dtype"""
    f = pose.dtype.type
    R = quat_to_rot(pose[..., 3:])[..., None, :]
    t = pose[..., None, :3]
    Xx, Xy, Xz = X[:, 0].astype(f), X[:, 1].astype(f), X[:, 2].astype(f)
    Y = np.stack([(R[..., 3 * i] * Xx + R[..., 3 * i + 1] * Xy) + R[..., 3 * i + 2] * Xz for i in range(3)], -1)
    return Y + t, Y


def distance(pose, X, x):
    """the distance of the header: pose [...,7] (dtype decides), X [P,3], x [P,2] -> [...,P]"""
    f = pose.dtype.type
    with np.errstate(all="ignore"):
        m, _ = project(pose, X)
        u, v = x[:, 0].astype(f), x[:, 1].astype(f)
        ex, ey, den = m[..., 0] - u * m[..., 2], m[..., 1] - v * m[..., 2], m[..., 2] * m[..., 2]
        d = np.fmin((ex * ex + ey * ey) / np.maximum(den, f(DEN_MIN)), f(D_MAX))
        return np.where((m[..., 2] > 0) & (den >= f(DEN_MIN)), d, f(D_MAX))


def cost(pose, X, x, w, tau):
    """the robust cost of pose [...,7] on the rows X, x with weights w [K] (already clamped, in pose's dtype)"""
    f = pose.dtype.type
    t2 = f(tau) * f(tau)
    with np.errstate(all="ignore"):
        return H._seqsum(w * (t2 * np.log1p(distance(pose, X, x) / t2))) / H._seqsum(w)


# ------------------------------------------------------------------------------------------------ the three-point solver, fp64
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _unit3(a):
    return a / np.sqrt(_dot(a, a))[..., None]


def _frame(p0, p1, p2):
    e0 = _unit3(p1 - p0)
    e2 = _unit3(_cross(e0, p2 - p0))
    return e0, _cross(e2, e0), e2


def _rot_to_quat(R):
    """Shepperd's branches on R [S,9], fp64, w >= 0"""
    tr = R[:, 0] + R[:, 4] + R[:, 8]
    b0 = tr > 0
    b1 = ~b0 & (R[:, 0] >= R[:, 4]) & (R[:, 0] >= R[:, 8])
    b2 = ~b0 & ~b1 & (R[:, 4] >= R[:, 8])
    v0 = np.stack([R[:, 7] - R[:, 5], R[:, 2] - R[:, 6], R[:, 3] - R[:, 1], 1 + tr], -1)
    v1 = np.stack([1 + R[:, 0] - R[:, 4] - R[:, 8], R[:, 1] + R[:, 3], R[:, 2] + R[:, 6], R[:, 7] - R[:, 5]], -1)
    v2 = np.stack([R[:, 1] + R[:, 3], 1 + R[:, 4] - R[:, 0] - R[:, 8], R[:, 5] + R[:, 7], R[:, 2] - R[:, 6]], -1)
    v3 = np.stack([R[:, 2] + R[:, 6], R[:, 5] + R[:, 7], 1 + R[:, 8] - R[:, 0] - R[:, 4], R[:, 3] - R[:, 1]], -1)
    v = np.where(b0[:, None], v0, np.where(b1[:, None], v1, np.where(b2[:, None], v2, v3)))
    nrm = np.sqrt(((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) + v[:, 3] * v[:, 3])
    s = np.where(v[:, 3] < 0, -1.0, 1.0)
    return np.where((nrm > 0)[:, None], s[:, None] * v / np.where(nrm > 0, nrm, 1)[:, None], np.array([0, 0, 0, 1.0]))


def _quadratic(b, c):
    """the roots of z^2 + b z + c in slot order (+, -), whether they are real, and the relative distance of that decision"""
    disc = b * b - 4 * c
    mag = b * b + np.abs(4 * c)
    real = disc >= -DISC_BAND * mag
    s = np.sqrt(np.maximum(disc, 0))
    return (-b + s) / 2, (-b - s) / 2, real, np.abs(disc) / np.where(mag > 0, mag, 1)


def quartic(Xs, xs):
    """steps 1 - 3 of the header on samples Xs [S,3,3], xs [S,3,2] (fp64): a dict of the named quantities"""
    Xs, xs = np.asarray(Xs, np.float64), np.asarray(xs, np.float64)
    u, v = xs[..., 0], xs[..., 1]
    nrm = np.sqrt((u * u + v * v) + 1)
    f = np.stack([u / nrm, v / nrm, 1 / nrm], -1)                                  # [S,3,3]
    ca, cb, cg = _dot(f[:, 1], f[:, 2]), _dot(f[:, 0], f[:, 2]), _dot(f[:, 0], f[:, 1])
    d12, d20, d10 = Xs[:, 1] - Xs[:, 2], Xs[:, 2] - Xs[:, 0], Xs[:, 1] - Xs[:, 0]
    a2, b2, c2 = _dot(d12, d12), _dot(d20, d20), _dot(d10, d10)
    big = np.maximum(a2, np.maximum(b2, c2))
    valid = np.isfinite(big) & (a2 >= SIDE_MIN * big) & (b2 >= SIDE_MIN * big) & (c2 >= SIDE_MIN * big) & (big > 0)
    cr = _cross(d10, d20)
    valid &= _dot(cr, cr) >= AREA_MIN * c2 * b2
    for i, j in ((1, 2), (0, 2), (0, 1)):
        cr = _cross(f[:, i], f[:, j])
        valid &= _dot(cr, cr) >= SPAN_MIN
    safe = np.where(valid, b2, 1)
    k, l = (a2 - c2) / safe, c2 / safe
    n0, n1, n2 = 1 + k, -2 * k * cb, k - 1
    d0, d1 = 2 * cg, -2 * ca
    e0, e1, e2 = d0 * d0, 2 * d0 * d1, d1 * d1
    nn = [n0 * n0, 2 * n0 * n1, n1 * n1 + 2 * n0 * n2, 2 * n1 * n2, n2 * n2]
    nd = [n0 * d0, n0 * d1 + n1 * d0, n1 * d1 + n2 * d0, n2 * d1]
    cd = [e0, e1 - 2 * cb * e0, (e2 - 2 * cb * e1) + e0, e1 - 2 * cb * e2, e2]
    A = np.stack([((e0 + nn[0]) - 2 * cg * nd[0]) - l * cd[0], ((e1 + nn[1]) - 2 * cg * nd[1]) - l * cd[1],
                  ((e2 + nn[2]) - 2 * cg * nd[2]) - l * cd[2], (nn[3] - 2 * cg * nd[3]) - l * cd[3], nn[4] - l * cd[4]], -1)
    amax = np.abs(A).max(-1)
    valid &= np.isfinite(amax) & (np.abs(A[:, 4]) > LEAD_MIN * amax)
    return dict(X=Xs, f=f, cb=cb, cg=cg, l=l, b2=b2, n=(n0, n1, n2), d=(d0, d1), A=A, valid=valid)


def _poses_of(Q, v, good):
    """steps 5 - 6: the gates of a solution at the root v [S] and its pose (t, q) in fp64 [S,7]; also y and D(v)"""
    (n0, n1, n2), (d0, d1), cb, cg, l, b2, f, X = Q["n"], Q["d"], Q["cb"], Q["cg"], Q["l"], Q["b2"], Q["f"], Q["X"]
    with np.errstate(all="ignore"):
        Dv, Nv, den = d0 + d1 * v, (n0 + n1 * v) + n2 * v * v, (1 - 2 * cb * v) + v * v
        good = good & (v > 0) & (np.abs(Dv) >= DEN_V_MIN) & (den > 0)
        y0 = np.where(good, Nv / np.where(good, Dv, 1), 1.0)
        w2 = (cg * cg - 1) + l * den
        rt = np.sqrt(np.maximum(w2, 0))
        yp, ym = cg + rt, cg - rt
        y = np.where(w2 >= 0, np.where(np.abs(yp - y0) <= np.abs(ym - y0), yp, ym), y0)
        good = good & (y > 0)
        s0 = np.sqrt(b2 / np.where(good, den, 1))
        Y = np.stack([s0[:, None] * f[:, 0], (y * s0)[:, None] * f[:, 1], (v * s0)[:, None] * f[:, 2]], 1)
        e, g = _frame(X[:, 0], X[:, 1], X[:, 2]), _frame(Y[:, 0], Y[:, 1], Y[:, 2])
        R = np.stack([(g[0][:, r] * e[0][:, c] + g[1][:, r] * e[1][:, c]) + g[2][:, r] * e[2][:, c] for r in range(3) for c in range(3)], -1)
        t = np.stack([Y[:, 0, i] - ((R[:, 3 * i] * X[:, 0, 0] + R[:, 3 * i + 1] * X[:, 0, 1]) + R[:, 3 * i + 2] * X[:, 0, 2]) for i in range(3)], -1)
        q = _rot_to_quat(np.where(np.isfinite(R), R, 0))
    return np.concatenate([t, q], -1), good, y, Dv


def p3p(Xs, xs, dt=np.float64):
    """the header's solver on samples Xs [S,3,3], xs [S,3,2] -> (pose [S,4,7] in dt with the header's fp32 rounding where dt is float32,
    ok [S,4], margin [S])"""
    Q = quartic(Xs, xs)
    S = len(Q["valid"])
    A, valid = Q["A"], Q["valid"]
    with np.errstate(all="ignore"):
        a4 = np.where(valid, A[:, 4], 1)
        q3, q2, q1, q0 = A[:, 3] / a4, A[:, 2] / a4, A[:, 1] / a4, A[:, 0] / a4
        sh = q3 / 4
        p = q2 - 6 * sh * sh
        q = (q1 - 2 * q2 * sh) + 8 * sh * sh * sh
        r = ((q0 - q1 * sh) + q2 * sh * sh) - 3 * (sh * sh) * (sh * sh)
        c1, c0 = p * p / 4 - r, -(q * q) / 8
        Pc, Qc = c1 - p * p / 3, (2 * p * p * p / 27 - p * c1 / 3) + c0
        disc = Qc * Qc / 4 + Pc * Pc * Pc / 27
        sd = np.sqrt(np.maximum(disc, 0))
        one = np.cbrt(-Qc / 2 + sd) + np.cbrt(-Qc / 2 - sd)
        amp = 2 * np.sqrt(np.maximum(-Pc / 3, 0))
        arg = np.where(Pc < 0, (3 * Qc / (2 * np.where(Pc < 0, Pc, -1))) * np.sqrt(-3 / np.where(Pc < 0, Pc, -1)), 1.0)
        three = amp * np.cos(np.arccos(np.clip(arg, -1, 1)) / 3)
        m = np.where(disc > 0, one, three) - p / 3
        for _ in range(2):
            fv, fd = ((m + p) * m + c1) * m + c0, (3 * m + 2 * p) * m + c1
            m = np.where(fd != 0, m - fv / np.where(fd != 0, fd, 1), m)
        ferrari = m > RESOLVENT_MIN * np.maximum(1, np.abs(p))
        s = np.sqrt(2 * np.where(ferrari, m, 1))
        h = q / (2 * s)
        z0, z1, r01, g01 = _quadratic(-s, (p / 2 + m) + h)
        z2, z3, r23, g23 = _quadratic(s, (p / 2 + m) - h)
        zp, zm, rb, gb = _quadratic(p, r)
        y0, y2 = np.sqrt(np.maximum(zp, 0)), np.sqrt(np.maximum(zm, 0))
        z = np.where(ferrari[:, None], np.stack([z0, z1, z2, z3], -1), np.stack([y0, -y0, y2, -y2], -1))
        real = np.where(ferrari[:, None], np.stack([r01, r01, r23, r23], -1), np.stack([rb & (zp >= 0), rb & (zp >= 0), rb & (zm >= 0), rb & (zm >= 0)], -1))
        margin = np.where(ferrari, np.minimum(g01, g23), gb)
        valid = valid & np.isfinite(m)
        pose, ok = np.zeros((S, 4, 7)), np.zeros((S, 4), bool)
        for k in range(4):
            v = np.where(real[:, k], z[:, k] - sh, 0.0)
            for _ in range(3):
                fv, fd = (((v + q3) * v + q2) * v + q1) * v + q0, ((4 * v + 3 * q3) * v + 2 * q2) * v + q1
                v = np.where(fd != 0, v - fv / np.where(fd != 0, fd, 1), v)
            ps, good, y, Dv = _poses_of(Q, v, real[:, k] & valid)
            gate = np.minimum(np.abs(v), np.minimum(np.abs(y), np.abs(Dv)))
            margin = np.where(real[:, k] & valid, np.minimum(margin, gate), margin)
            pose[:, k], ok[:, k] = ps, good
    f = np.dtype(dt).type
    out = pose.astype(dt)
    if dt == np.float32:                                       # the header's rounding: (t, q) to fp32, q normalised again by unit<4>
        qn, nq = RT.unit(out[..., 3:].reshape(-1, 4))
        qn, nq = qn.reshape(S, 4, 4), nq.reshape(S, 4)
        ok &= (nq > f(0.5)) & (nq < f(2))
        out[..., 3:] = np.where(qn[..., 3:] < 0, -qn, qn)
    ok &= np.isfinite(out).all(-1)
    out[~ok] = 0
    return out, ok, np.where(valid, margin, np.inf)


def p3p_roots_lapack(Xs, xs):
    """the SECOND ROUTE: per sample the depth triples (s_0, s_1, s_2) of all real roots of the quartic by numpy.roots (the companion
    matrix's eigenvalues), each kept if the three depths are positive.  A root counts as real if |Im| <= 1e-7 (1 + |Re|).  The ROOTS are
    the independent part; the depths follow from a root by step 5 of the header."""
    Q = quartic(Xs, xs)
    (n0, n1, n2), (d0, d1), cb, b2 = Q["n"], Q["d"], Q["cb"], Q["b2"]
    out = []
    for i in range(len(Q["valid"])):
        sols = []
        if Q["valid"][i]:
            for root in np.roots(Q["A"][i, ::-1]):
                if abs(root.imag) > 1e-7 * (1 + abs(root.real)):
                    continue
                v = root.real
                Dv, den = d0[i] + d1[i] * v, (1 - 2 * cb[i] * v) + v * v
                if not (v > 0 and abs(Dv) >= DEN_V_MIN and den > 0):
                    continue
                y = ((n0[i] + n1[i] * v) + n2[i] * v * v) / Dv
                w2 = (Q["cg"][i] ** 2 - 1) + Q["l"][i] * den          # step 5 of the header: N / D names the branch only
                if w2 >= 0:
                    y = min((Q["cg"][i] + np.sqrt(w2), Q["cg"][i] - np.sqrt(w2)), key=lambda c: abs(c - y))
                if y > 0:
                    s0 = np.sqrt(b2[i] / den)
                    sols.append((s0, y * s0, v * s0))
        out.append(np.array(sols).reshape(-1, 3))
    return out


# ------------------------------------------------------------------------------------------------ entry point 1
def consensus(X, x, w=None, tau=TAU, seed=SEED, M=256, dt=np.float64, first=0):
    """rp_p3p_consensus: dt = float64 the reference, float32 the restatement; X [n,P,3], x [n,P,2], w [n,P] or None, tau a number or [n]"""
    n, P = x.shape[:2]
    f = np.dtype(dt).type
    tau = np.broadcast_to(np.asarray(tau, np.float64), (n,))
    wc = C.clamp(w, n, P, dt)
    pos, samples = sample_rows3(w, n, P, seed, M, first)
    out = Consensus(np.zeros((n, 7), dt), np.full(n, -1, np.int64), np.zeros((n, 4), dt), wc.copy(), np.zeros((n, M, 7), dt),
                    np.full((n, M), FLT_MAX, dt), np.zeros((n, M), np.int64), samples, np.full((n, M), np.inf))
    for b in range(n):
        K = len(pos[b])
        out.stat[b, 3] = K
        if K < 3 or not tau[b] > 0:
            continue
        pose, ok, margin = p3p(X[b][samples[b]], x[b][samples[b]], dt)
        cs = cost(pose, X[b][pos[b]], x[b][pos[b]], wc[b][pos[b]], tau[b])            # [M,4]
        with np.errstate(all="ignore"):
            keep = ok & (cs < FLT_MAX)
        cs = np.where(keep, cs, np.inf)
        slot = np.argmin(cs, -1)                                                   # the first of equal costs
        valid = keep.any(-1)
        out.hyp_pose[b] = np.where(valid[:, None], pose[np.arange(M), slot], 0)
        out.hyp_cost[b] = np.where(valid, cs[np.arange(M), slot], FLT_MAX)
        out.hyp_count[b] = keep.sum(-1)
        out.margin[b] = margin
        out.stat[b, 2] = valid.sum()
        if not valid.any():
            continue
        win = int(np.argmin(out.hyp_cost[b]))
        out.best[b], out.pose[b] = win, out.hyp_pose[b, win]
        d = distance(out.pose[b], X[b], x[b])
        t2 = f(tau[b]) * f(tau[b])
        out.stat[b, 0] = out.hyp_cost[b, win]
        out.stat[b, 1] = (wc[b] * (d <= t2)).sum() / wc[b].sum()
        out.weights[b] = wc[b] / (1 + d / t2)
    return out


# ------------------------------------------------------------------------------------------------ entry point 2
def jacobian(pose, X, x):
    """(Jx [P,6], Jy [P,6], r [P,2], d [P], has a derivative [P]) of the header at pose [7], in pose's dtype"""
    f = pose.dtype.type
    with np.errstate(all="ignore"):
        m, Y = project(pose, X)
        u, v = x[:, 0].astype(f), x[:, 1].astype(f)
        ex, ey, den = m[:, 0] - u * m[:, 2], m[:, 1] - v * m[:, 2], m[:, 2] * m[:, 2]
        ok = (m[:, 2] > 0) & (den >= f(DEN_MIN))
        inv = np.where(ok, f(1) / np.where(ok, m[:, 2], f(1)), f(0))
        d = np.where(ok, np.fmin((ex * ex + ey * ey) / np.maximum(den, f(DEN_MIN)), f(D_MAX)), f(D_MAX))
        px, py = m[:, 0] * inv, m[:, 1] * inv
        z, o = np.zeros_like(inv), inv
        Jx = np.stack([inv * -(px * Y[:, 1]), inv * (Y[:, 2] + px * Y[:, 0]), inv * -Y[:, 1], o, z, inv * -px], -1)
        Jy = np.stack([inv * -(Y[:, 2] + py * Y[:, 1]), inv * (py * Y[:, 0]), inv * Y[:, 0], z, o, inv * -py], -1)
    return Jx, Jy, np.stack([ex * inv, ey * inv], -1), d, ok


def normal_equations(pose, X, x, wc, t2):
    f = pose.dtype.type
    Jx, Jy, r, d, ok = jacobian(pose, X, x)
    with np.errstate(all="ignore"):
        om = np.where(ok, wc / (f(1) + d / t2), f(0))
    N = (om[:, None, None] * (Jx[:, :, None] * Jx[:, None, :] + Jy[:, :, None] * Jy[:, None, :])).sum(0, dtype=pose.dtype)
    g = (om[:, None] * (Jx * r[:, :1] + Jy * r[:, 1:])).sum(0, dtype=pose.dtype)
    return N, g


def start(pose0, dt):
    """the state of the header for the start pose0 [7], or None for a degenerate one"""
    p0 = np.asarray(pose0, dt)
    if not (np.abs(p0) <= dt(FINITE)).all():
        return None
    q, nq = RT.unit(p0[None, 3:])
    if not (nq[0] >= dt(MIN_SCALE) and nq[0] <= dt(FINITE)):
        return None
    q = q[0]
    return np.concatenate([p0[:3], -q if q[3] < 0 else q]).astype(dt)


def refine(X, x, w, tau, pose0, iters, dt=np.float64):
    """rp_pnp_refine -> Refined(pose [n,7], stat [n,4], weights [n,P], kappa [n]: the condition number of the scaled normal matrix at
    the start)"""
    n, P = x.shape[:2]
    f = np.dtype(dt).type
    tau = np.broadcast_to(np.asarray(tau, np.float64), (n,))
    wc = C.clamp(w, n, P, dt)
    out = Refined(np.array(pose0, dt).reshape(n, 7).copy(), np.zeros((n, 4), dt), wc.copy(), np.full(n, np.nan))
    for b in range(n):
        K = int((wc[b] > 0).sum())
        out.stat[b, 3] = K
        ps = start(pose0[b], f)
        if ps is None or K < 3 or not tau[b] > 0:
            continue
        t2 = f(tau[b]) * f(tau[b])
        cst = lambda pp: (wc[b] * (t2 * np.log1p(distance(pp, X[b], x[b]) / t2))).sum(dtype=dt) / wc[b].sum(dtype=dt)   # noqa: E731
        cur, lam, acc = cst(ps), LAMBDA0, 0
        for it in range(iters):
            N, g = normal_equations(ps, X[b], x[b], wc[b], t2)
            if it == 0:
                with np.errstate(all="ignore"):
                    out.kappa[b] = H.scaled_condition(N)
            delta = RT._cholesky_step(N, g, lam)
            solved = delta is not None
            p1 = ps
            if solved:
                q1, solved = RT.retract(ps[3:], delta[:3].astype(dt))
                p1 = np.concatenate([ps[:3] + delta[3:].astype(dt), q1]).astype(dt)
            ct = cst(p1) if solved else cur
            if solved and ct < cur:
                ps, cur, lam, acc = p1, ct, max(lam / 10, LAMBDA_MIN), acc + 1
            else:
                lam = min(lam * 10, LAMBDA_MAX)
        d = distance(ps, X[b], x[b])
        out.pose[b] = ps
        out.stat[b, :3] = cur, (wc[b] * (d <= t2)).sum(dtype=dt) / wc[b].sum(dtype=dt), acc
        out.weights[b] = wc[b] / (1 + d / t2)
    return out


# ------------------------------------------------------------------------------------------------ scenes
GRID, PITCH = 24, 0.024                                    # 576 token centres, half a pitch = TAU
ThreeViews = collections.namedtuple("ThreeViews", "x1 xa xc X pose_a pose_c inlier_a inlier_c")


def pose_of(R, t):
    return np.concatenate([t, H.rot_to_quat(np.asarray(R, np.float64))])


def proj(R, t, X):
    m = X @ R.T + t
    return m[:, :2] / m[:, 2:]


def three_views(seed, P=576, outliers=0.3, sigma=1e-3, angle=0.2, depth=(3.0, 9.0)):
    """the scenes of DESIGN.md 5.14: P points on the hub's token grid (random positions in the same field below P = 576) at depth 3 - 9
    baselines of pair (hub, a); cameras a and c rotated by `angle` about random axes; |t_a| = 1, |t_c| uniform in [0.5, 2]; Gaussian
    noise sigma on the images in a and c; a share `outliers` of the rows of EACH pair, drawn independently, replaced by uniform points"""
    rng = np.random.default_rng(1000 + seed)
    half = GRID * PITCH / 2
    if P == GRID * GRID:
        c = (np.arange(GRID) + 0.5) * PITCH - half
        x1 = np.stack(np.meshgrid(c, c, indexing="xy"), -1).reshape(-1, 2)
    else:
        x1 = rng.uniform(-half, half, (P, 2))
    X = np.concatenate([x1, np.ones((P, 1))], -1) * rng.uniform(depth[0], depth[1], (P, 1))
    views = []
    for scale in (1.0, rng.uniform(0.5, 2.0)):
        axis, t = rng.normal(size=3), rng.normal(size=3)
        views.append((RT.axis_angle(axis / np.linalg.norm(axis), angle), scale * t / np.linalg.norm(t)))
    out = []
    for R, t in views:
        xi = proj(R, t, X) + sigma * rng.normal(size=(P, 2))
        bad = rng.uniform(size=P) < outliers
        xi[bad] = rng.uniform(-half, half, (int(bad.sum()), 2))
        out += [xi, ~bad]
    return ThreeViews(x1.astype(np.float32), out[0].astype(np.float32), out[2].astype(np.float32), X, pose_of(*views[0]), pose_of(*views[1]),
                      out[1], out[3])


def triangulate64(pose, x1, x2):
    """include/relpose_triangulate.h restated in fp64 for one problem: (X [P,3], z1, z2, d2, phi)"""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    t = pose[:3] / np.linalg.norm(pose[:3])
    R = H.quat_to_rot(pose[3:] / np.linalg.norm(pose[3:]))
    E = H.cross_matrix(t) @ R
    P = len(x1)
    a_, b_ = np.concatenate([x2, np.ones((P, 1))], -1), np.concatenate([x1, np.ones((P, 1))], -1)
    Et = E[:2, :2]
    with np.errstate(all="ignore"):
        m, mp = (b_ @ E.T)[:, :2], (a_ @ E)[:, :2]
        a = np.einsum("pi,ij,pj->p", m, Et, mp)
        b = ((m * m).sum(-1) + (mp * mp).sum(-1)) / 2
        c = np.einsum("pi,ij,pj->p", a_, E, b_)
        d = np.sqrt(np.maximum(b * b - a * c, 0))
        lam = np.where(b + d > 1e-30, c / np.where(b + d > 1e-30, b + d, 1), 0)
        D2, D1 = lam[:, None] * m, lam[:, None] * mp
        m, mp = m - D1 @ Et.T, mp - D2 @ Et
        s = (m * m).sum(-1) + (mp * mp).sum(-1)
        lam = np.where(s > 1e-30, lam * 2 * d / np.where(s > 1e-30, s, 1), 0)
        D2, D1 = lam[:, None] * m, lam[:, None] * mp
        x2c, x1c = np.concatenate([x2 - D2, np.ones((P, 1))], -1), np.concatenate([x1 - D1, np.ones((P, 1))], -1)
        r = x1c @ R.T
        g = np.cross(x2c, r)
        gg = (g * g).sum(-1)
        inf = gg < 1e-10 * (x2c * x2c).sum(-1) * (r * r).sum(-1)
        z1 = np.where(inf, 0, (np.cross(t, x2c) * g).sum(-1) / np.where(inf, 1, gg))
        z2 = np.where(inf, 0, (np.cross(t, r) * g).sum(-1) / np.where(inf, 1, gg))
        phi = np.arctan2(np.sqrt(gg), (x2c * r).sum(-1))
    return z1[:, None] * x1c, z1, z2, (D1 * D1).sum(-1) + (D2 * D2).sum(-1), phi


def row_weights(z1, z2, d2, phi, tau_a, w_a=None, w_c=None, cauchy=True, min_parallax=None):
    """the row weights of resection.third_view_pose"""
    mp = tau_a if min_parallax is None else min_parallax
    w = ((z1 > 0) & (z2 > 0) & (phi >= mp)).astype(np.float64)
    if cauchy:
        w = w / (1 + d2 / tau_a ** 2)
    for extra in (w_a, w_c):
        if extra is not None:
            w = w * C.clamp(extra[None], 1, len(z1))[0]
    return w


def third_view(sc, tau=TAU, M=256, seed=0, iters=10, cauchy=True, pose_a=None, dt=np.float64):
    """the chain of resection.third_view_pose on a ThreeViews scene with the pose of (hub, a) given (the TRUE one by default):
    triangulate -> row weights -> consensus -> refine; returns (Refined, the consensus, w, X)"""
    pa = sc.pose_a if pose_a is None else pose_a
    X, z1, z2, d2, phi = triangulate64(pa, sc.x1, sc.xa)
    w = row_weights(z1, z2, d2, phi, tau, cauchy=cauchy).astype(np.float32)
    Xf = X.astype(np.float32)
    cons = consensus(Xf[None], sc.xc[None], w[None], tau, seed, M, dt)
    return refine(Xf[None], sc.xc[None], w[None], tau, cons.pose, iters, dt), cons, w, Xf


def pose_errors(pose, truth):
    """(|t| / |t_true|, the rotation error in degrees, the angle between the translation directions in degrees)"""
    Ra, Rb = H.quat_to_rot(pose[3:].astype(np.float64)), H.quat_to_rot(truth[3:])
    ta, tb = pose[:3].astype(np.float64), truth[:3]
    na, nb = np.linalg.norm(ta), np.linalg.norm(tb)
    cosd = np.clip(ta @ tb / max(na * nb, 1e-300), -1, 1)
    return na / nb, RT.angle_deg(Ra, Rb), float(np.degrees(np.arccos(cosd)))


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
EXACT = [(1, 3, 1), (3, 4, 255), (1, 8, 256), (3, 9, 257), (130, 64, 16), (3, 257, 16), (1, 513, 16), (1, 1728, 40)]
CASES = [(kind, n, P, M, wt) for kind in ("exact", "noisy") for n, P, M in EXACT for wt in (False, True)]
REFINE_CASES = [("noisy", 4, 576, False), ("noisy", 4, 576, True), ("noisy", 3, 257, True), ("noisy", 1, 1728, False), ("exact", 2, 3, False),
                ("exact", 3, 9, True)]
MARGIN_CMP = 1e-6          # a hypothesis is compared where every decision of the reference's solver is at least this far from its threshold
LEFT_OUT_MAX = 0.05
_CACHE = {}


def exact_rows(n, P, seed, sigma=0.0, outliers=0.0):
    """(X [n,P,3] float32, x [n,P,2] float32, pose [n,7]): n problems of P rows; the images are those of the float32 points, rounded"""
    Xs, xs, ps = [], [], []
    for b in range(n):
        sc = three_views(seed * 1000 + b, P, outliers, 0.0)
        Xf = sc.X.astype(np.float32)
        R, t = H.quat_to_rot(sc.pose_c[3:]), sc.pose_c[:3]
        xi = proj(R, t, Xf.astype(np.float64))
        rng = np.random.default_rng(seed * 7919 + b)
        xi = xi + sigma * rng.normal(size=xi.shape)
        bad = rng.uniform(size=P) < outliers
        xi[bad] = rng.uniform(-0.288, 0.288, (int(bad.sum()), 2))
        Xs.append(Xf); xs.append(xi.astype(np.float32)); ps.append(sc.pose_c)
    return np.stack(Xs), np.stack(xs), np.stack(ps)


def inputs(kind, n, P, M, weighted):
    """(X, x, w): exact rows, or rows with noise 1e-3 and (from P = 64) 30 % wrong images"""
    key = ("in", kind, n, P, weighted)
    if key not in _CACHE:
        X, x, _ = exact_rows(n, P, 21 if kind == "exact" else 22, 0.0 if kind == "exact" else 1e-3, 0.3 if kind == "noisy" and P >= 64 else 0.0)
        w = None
        if weighted:
            rng = np.random.default_rng(P + n)
            w = rng.uniform(0.05, 1.0, (n, P)).astype(np.float32)
            if P >= 8:
                w[rng.uniform(size=w.shape) < 0.3] = 0
                w[:, 5], w[:, 7] = -0.5, np.nan
        _CACHE[key] = (X, x, w)
    return _CACHE[key]


def reference(kind, n, P, M, weighted):
    key = ("ref", kind, n, P, M, weighted)
    if key not in _CACHE:
        X, x, w = inputs(kind, n, P, M, weighted)
        _CACHE[key] = consensus(X, x, w, TAU, SEED, M)
    return _CACHE[key]


def cost64(pose, X, x, wc, tau):
    """the fp64 robust cost of pose [n,7] or [n,M,7] per problem (and hypothesis)"""
    pose = np.asarray(pose, np.float64)
    out = []
    for b in range(len(pose)):
        with np.errstate(all="ignore"):
            t2 = float(tau) ** 2
            out.append((wc[b] * t2 * np.log1p(distance(pose[b], X[b], x[b]) / t2)).sum(-1) / wc[b].sum())
    return np.stack(out)


def horizon(pose, X, x, wc, tau):
    """_rotation_ref.horizon for m_z = r3 . X + t_z: a row whose m_z is within rounding of 0 may fall on either side of the horizon"""
    pose = np.asarray(pose, np.float64)
    out = []
    for b in range(len(pose)):
        R = quat_to_rot(pose[b][..., 3:])[..., None, :]
        Xb = X[b].astype(np.float64)
        with np.errstate(all="ignore"):
            terms = [R[..., 6] * Xb[:, 0], R[..., 7] * Xb[:, 1], R[..., 8] * Xb[:, 2], pose[b][..., None, 2] + 0 * Xb[:, 0]]
            mz, mu = sum(terms), sum(np.abs(t) for t in terms)
            rho = np.where(mz != 0, 2 * EPS32 * mu / np.where(mz != 0, np.abs(mz), 1), np.inf)
            d = distance(pose[b], X[b], x[b])
            out.append((wc[b] * np.minimum(float(tau) ** 2, d) * np.minimum(4 * rho, 80)).sum(-1) / wc[b].sum())
    return np.stack(out)


cost_bound = H.cost_bound


def lever(pose, Xs, xs):
    """the scale of a pose's reprojection error on rows Xs [...,3,3], xs [...,3,2] under fp32 rounding of (t, q): per row
    (|X| + |t|) (1 + |x|) / m_z, the largest of the rows; pose [...,7] fp64"""
    R = quat_to_rot(pose[..., 3:])
    m = np.stack([(R[..., None, 3 * i] * Xs[..., 0] + R[..., None, 3 * i + 1] * Xs[..., 1]) + R[..., None, 3 * i + 2] * Xs[..., 2]
                  for i in range(3)], -1) + pose[..., None, :3]
    with np.errstate(all="ignore"):
        s = (np.linalg.norm(Xs, axis=-1) + np.linalg.norm(pose[..., None, :3], axis=-1)) * (1 + np.linalg.norm(xs, axis=-1)) / m[..., 2]
        res = np.linalg.norm(m[..., :2] / m[..., 2:] - xs, axis=-1)
    return s.max(-1), res.max(-1)


def consensus_ratios(out, ref, X, x, w, tau=TAU):
    """out: a Consensus-like tuple of numpy arrays (the device's or the restatement's), ref: the fp64 Consensus of the same inputs ->
    the ratios of the bounds: unit (| |q| - 1 | over eps32 on the valid hypotheses), repro (the largest reprojection residual of the
    sample rows under out's OWN pose over eps32 lever, on the compared hypotheses), cost and w (against the fp64 values at out's OWN
    pose), and the compared share"""
    n, P = x.shape[:2]
    wc = C.clamp(w, n, P)
    valid = ref.hyp_cost < FLT_MAX
    compared = valid & (ref.margin >= MARGIN_CMP)
    ovalid = out.hyp_cost < FLT_MAX
    assert np.array_equal(ovalid[compared], valid[compared]), "validity differs on a compared hypothesis"
    assert not out.hyp_pose[~ovalid].any()
    hp = out.hyp_pose.astype(np.float64)
    ru = (np.abs(np.linalg.norm(hp[..., 3:], axis=-1) - 1) / EPS32)[ovalid]
    assert bool((hp[..., 6][ovalid] >= 0).all())
    Xs = np.stack([X[b][ref.samples[b]] for b in range(n)]).astype(np.float64)
    xs = np.stack([x[b][ref.samples[b]] for b in range(n)]).astype(np.float64)
    lev, res = lever(hp, Xs, xs)
    rr = (res / (EPS32 * np.where(compared & ovalid, lev, 1)))[compared & ovalid]
    own = cost64(out.hyp_pose, X, x, wc, tau)
    both = ovalid & np.isfinite(own)
    hor = horizon(out.hyp_pose, X, x, wc, tau)
    rc = (np.abs(out.hyp_cost.astype(np.float64) - own) / cost_bound(np.where(both, own, 1), 1.0, hor))[both]
    won = out.best >= 0
    rw = np.zeros(0)
    if won.any():
        t2 = float(tau) ** 2
        want = np.stack([wc[b] / (1 + distance(out.pose[b].astype(np.float64), X[b], x[b]) / t2) for b in np.flatnonzero(won)])
        rw = (np.abs(out.weights[won].astype(np.float64) - want) / np.where(wc[won] > 0, wc[won], 1) / (EPS32 / tau))[wc[won] > 0]
    return dict(unit=float(ru.max(initial=0)), repro=float(rr.max(initial=0)), cost=float(rc.max(initial=0)), w=float(rw.max(initial=0)),
                compared=float(compared.sum() / max(valid.sum(), 1)))


def check_consensus(out, ref, X, x, w, tau=TAU):
    """the device's rp_p3p_consensus against the reference, at the calibrated bounds; returns the ratios"""
    n, P = x.shape[:2]
    wc = C.clamp(w, n, P)
    r = consensus_ratios(out, ref, X, x, w, tau)
    print("unit %.3g (C %.3g), reprojection %.3g (C %.3g), cost ratio %.3g (C %.3g), w ratio %.3g (C %.3g), compared %.4f"
          % (r["unit"], C_UNIT, r["repro"], C_REPRO, r["cost"], C_COST, r["w"], C_W, r["compared"]))
    assert r["compared"] >= 1 - LEFT_OUT_MAX
    assert r["unit"] <= C_UNIT and r["repro"] <= C_REPRO and r["cost"] <= C_COST and r["w"] <= C_W, r
    K = (wc > 0).sum(-1)
    assert np.array_equal(out.stat[:, 3], K) and np.array_equal(out.stat[:, 2], (out.hyp_cost < FLT_MAX).sum(-1))
    if out.hyp_count is not None:
        assert np.array_equal(out.hyp_count > 0, out.hyp_cost < FLT_MAX) and out.hyp_count.max(initial=0) <= 4 and out.hyp_count.min(initial=0) >= 0
    for b in range(n):
        if K[b] < 3 or not (out.hyp_cost[b] < FLT_MAX).any():
            assert out.best[b] == -1 and not out.pose[b].any() and not out.stat[b, :2].any()
            assert np.array_equal(out.weights[b], wc[b].astype(np.float32))
            continue
        win = int(np.argmin(out.hyp_cost[b]))                        # the lowest index of the device's own minimum, exactly
        assert out.best[b] == win and np.array_equal(out.pose[b], out.hyp_pose[b, win]) and out.stat[b, 0] == out.hyp_cost[b, win]
        # against the reference the winner is compared by COST: the device's winner costs (fp64, its own pose) no more than the device's
        # version of the reference's winner, up to the two cost bounds
        pair = out.hyp_pose[b:b + 1, [win, int(ref.best[b])]]
        own = cost64(pair, X[b:b + 1], x[b:b + 1], wc[b:b + 1], tau)[0]
        hor = horizon(pair, X[b:b + 1], x[b:b + 1], wc[b:b + 1], tau)[0]
        if out.hyp_cost[b, int(ref.best[b])] < FLT_MAX:
            assert own[0] <= own[1] + cost_bound(own[0], C_COST, hor[0]) + cost_bound(own[1], C_COST, hor[1]), (b, own)
        t2 = float(tau) ** 2
        u = distance(out.pose[b].astype(np.float64), X[b], x[b]) / t2
        share, band = (wc[b] * (u <= 1)).sum() / wc[b].sum(), (wc[b] * (np.abs(u - 1) < 1e-4)).sum() / wc[b].sum()
        assert abs(out.stat[b, 1] - share) <= band + 1e-5, (b, out.stat[b, 1], share, band)
    return r


def refine_inputs(kind, n, P, weighted):
    """(X, x, w, pose0 float32): the rows of `inputs` and the reference consensus winner (M = 64) rounded to float32 as the start"""
    key = ("rin", kind, n, P, weighted)
    if key not in _CACHE:
        X, x, w = inputs(kind, n, P, 64, weighted)
        _CACHE[key] = (X, x, w, consensus(X, x, w, TAU, SEED, 64).pose.astype(np.float32))
    return _CACHE[key]


def refine_reference(kind, n, P, weighted, iters):
    key = ("rref", kind, n, P, weighted, iters)
    if key not in _CACHE:
        X, x, w, p0 = refine_inputs(kind, n, P, weighted)
        _CACHE[key] = refine(X, x, w, TAU, p0, iters)
    return _CACHE[key]


def refine_ratios(pose, stat, weights, ref, X, x, w, tau=TAU):
    """pose: max(|q - q_ref|, |t - t_ref| / max(|t_ref|, 1)) over eps32 kappa; unit: | |q| - 1 | over eps32; cost and weights against
    fp64 at the output's own pose"""
    n, P = x.shape[:2]
    wc = C.clamp(w, n, P)
    kap = np.where(np.isfinite(ref.kappa), ref.kappa, 1.0)
    p64 = pose.astype(np.float64)
    err = np.maximum(np.linalg.norm(p64[:, 3:] - ref.pose[:, 3:], axis=-1),
                     np.linalg.norm(p64[:, :3] - ref.pose[:, :3], axis=-1) / np.maximum(np.linalg.norm(ref.pose[:, :3], axis=-1), 1))
    rp = err / (EPS32 * kap)
    ru = np.abs(np.linalg.norm(p64[:, 3:], axis=-1) - 1) / EPS32
    own = cost64(pose, X, x, wc, tau)
    rc = np.abs(stat[:, 0].astype(np.float64) - own) / cost_bound(own, 1.0, horizon(pose, X, x, wc, tau))
    t2 = float(tau) ** 2
    want = np.stack([wc[b] / (1 + distance(p64[b], X[b], x[b]) / t2) for b in range(n)])
    rw = (np.abs(weights.astype(np.float64) - want) / np.where(wc > 0, wc, 1) / (EPS32 / tau))[wc > 0]
    return dict(pose=float(rp.max()), unit=float(ru.max()), cost=float(rc.max()), w=float(rw.max(initial=0)))


def restatement_worst():
    """the worst ratios of the float32 restatement on the inputs of the GPU tests: what WORST records"""
    worst = dict(unit=0.0, repro=0.0, cost=0.0, w=0.0, refine1=0.0, refine10=0.0, left_out=0.0)
    for case in CASES:
        X, x, w = inputs(*case)
        r = consensus_ratios(consensus(X, x, w, TAU, SEED, case[3], np.float32), reference(*case), X, x, w)
        for k in ("unit", "repro", "cost", "w"):
            worst[k] = max(worst[k], r[k])
        worst["left_out"] = max(worst["left_out"], 1 - r["compared"])
    for case in REFINE_CASES:
        X, x, w, p0 = refine_inputs(*case)
        for iters in (1, 10):
            o = refine(X, x, w, TAU, p0, iters, np.float32)
            r = refine_ratios(o.pose, o.stat, o.weights, refine_reference(*case, iters), X, x, w)
            worst["refine%d" % iters] = max(worst["refine%d" % iters], r["pose"])
            worst["unit"], worst["cost"], worst["w"] = max(worst["unit"], r["unit"]), max(worst["cost"], r["cost"]), max(worst["w"], r["w"])
    return worst


# 8 x the restatement's worst ratio on these same inputs (tests/test_resection_cpu.py asserts the restatement within C / 8 and above
# 0.9 C / 8: the constants are these figures, not looser ones)
WORST = dict(unit=1.018, repro=0.7822, cost=0.8413, w=0.9321, refine1=0.03067, refine10=2.245)
C_UNIT, C_REPRO, C_COST, C_W = (8 * WORST[k] for k in ("unit", "repro", "cost", "w"))
C_REFINE = {1: 8 * WORST["refine1"], 10: 8 * WORST["refine10"]}


# ------------------------------------------------------------------------------------------------ the finding table of DESIGN.md 5.14
TABLE_SIGMAS, TABLE_OUTLIERS = (1e-3, 0.012), (0.3, 0.5, 0.6)


def table(seeds=range(10), M=256, iters=10):
    """(noise, wrong matches per pair, with the first pair's Cauchy weights) -> (scenes with |t_c| within 10 % of the truth, the lowest
    and the highest ratio |t_c| / truth, scenes with a ratio below 0.5 -- the basin |t| -> 0 --, the median ratio, the median rotation
    error and the median direction error in degrees) of third_view on three_views(seed), the TRUE pose for pair (hub, a)"""
    out = {}
    for sigma in TABLE_SIGMAS:
        for share in TABLE_OUTLIERS:
            for cauchy in (True, False):
                rows = []
                for seed in seeds:
                    sc = three_views(seed, GRID * GRID, share, sigma)
                    rows.append(pose_errors(third_view(sc, M=M, iters=iters, cauchy=cauchy)[0].pose[0], sc.pose_c))
                rows = np.array(rows)
                out[(sigma, share, cauchy)] = (int((np.abs(rows[:, 0] - 1) <= 0.1).sum()), float(rows[:, 0].min()), float(rows[:, 0].max()),
                                               int((rows[:, 0] < 0.5).sum()), float(np.median(rows[:, 0])), float(np.median(rows[:, 1])),
                                               float(np.median(rows[:, 2])))
    return out


# what table() measured (tests/test_resection_cpu.py::test_finding_table asserts it): within 10 %, lowest, highest, basin, medians
TABLE = {
    (0.001, 0.3, True): (10, 0.9928, 1.0028, 0, 0.9993, 0.0282, 0.0659),
    (0.001, 0.3, False): (9, 0.0710, 1.0006, 1, 0.9969, 0.0888, 0.2801),
    (0.001, 0.5, True): (9, 0.1294, 1.0024, 1, 0.9989, 0.0618, 0.2513),
    (0.001, 0.5, False): (9, 0.0160, 1.0011, 1, 0.9920, 0.2058, 0.7027),
    (0.001, 0.6, True): (9, 0.0579, 1.0054, 1, 0.9969, 0.0524, 0.3755),
    (0.001, 0.6, False): (9, 0.1721, 0.9980, 1, 0.9911, 0.3152, 1.3455),
    (0.012, 0.3, True): (8, 0.2437, 1.0108, 1, 0.9625, 0.6774, 1.9637),
    (0.012, 0.3, False): (8, 0.0629, 0.9950, 1, 0.9512, 0.8772, 2.4284),
    (0.012, 0.5, True): (7, 0.1166, 0.9870, 1, 0.9399, 0.7352, 2.3095),
    (0.012, 0.5, False): (6, 0.0240, 0.9859, 2, 0.9228, 1.2509, 4.3433),
    (0.012, 0.6, True): (8, 0.0206, 1.0024, 1, 0.9448, 0.6466, 2.1692),
    (0.012, 0.6, False): (5, 0.1493, 0.9705, 2, 0.8952, 1.8896, 7.5162),
}
# What the table says, next to the figures of the request that led to this library (a try with other scenes): (a) with the first pair's
# Cauchy weights 10 / 9 / 9 of 10 scenes are within 10 % at noise 1e-3 (ratio 0.993 - 1.005 on those) and 8 / 7 / 8 at token-pitch noise
# -- not the 10 of 10 of that try.  The scene that fails in every cell but one (seed 4) is a camera c that moves BACKWARDS
# (t_c = (0.73, 0.63, -1.38)): a row whose point is wrong (a wrong match of pair (hub, a) survives with a small weight) and lies nearer
# than |t_z| falls behind camera c under the TRUE pose and costs the maximum distance, tau^2 log1p(1e30 / tau^2) = 78 tau^2, twelve times a
# wrong match in front of the camera; the pose with |t| -> 0 keeps every point in front, and its robust cost is BELOW the cost that the
# polish reaches from the truth (7.06e-4 against 8.06e-4 at 50 %, noise 1e-3; 4096 hypotheses change nothing).  (b) Without the Cauchy
# weights that basin takes one more scene at token-pitch noise (2 of 10 at 50 % and 60 %) and the scenes within 10 % drop to 6 and 5.
# (c) At token-pitch noise the scale is biased LOW: the median ratio is 0.96 / 0.94 / 0.94, the highest 1.011.
