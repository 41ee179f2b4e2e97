"""References for include/relpose_select.h (librelpose_select.so), shared by tests/test_select_cpu.py, tests/test_gpu_select.py and
tests/test_gpu_select_contract.py.

select() is written ONCE, over a dtype.  With float64 it is the reference: the order statistic by numpy's sort, the residual of kinds 1
and 2 by a second route (eps^T (J J^T)^-1 eps with the 2 x 4 Jacobian written out and LAPACK's solve) and that of kind 0 by
_eightpoint_ref.sampson64.  With float32 the residuals are the header's statements in the header's association order: the restatement
that calibrates the GPU bound on `resid`, C eps32 scale(row) with C = 8 x the restatement's worst ratio on the GPU tests' own inputs.
Behind the residuals the kernel's outputs are checked EXACTLY against its own residuals (consistent()), so nothing else needs a bound.

Also here: the published robust GRIC, the flip algebra of DESIGN.md 5.12, the candidates of the fp64 reference chains and the table of
what the criterion chooses on the three scene families."""
import collections

import numpy as np

from tests import _consensus_ref as C
from tests import _eightpoint_ref as R8
from tests import _homography_ref as H
from tests import _refine_ref as RF
from tests import _rotation_ref as T

FLT_MAX = C.FLT_MAX
EPS32 = H.EPS32
E_MAX, DET_MIN, MIN_SCALE = 1e30, 1e-30, 1e-30
LN4 = 1.386294361
MED_CHI2 = {1: 0.454936423, 2: 1.386294361}          # by codimension
DIM = {0: 3, 1: 2, 2: 2}                             # kind -> d
PAR = {0: 5, 1: 8, 2: 3}                             # kind -> k
BAND_MIN, K_MIN = 16, 8
TAU, SIGMA, COST = 0.01, 1e-3, 8.0

Selection = collections.namedtuple("Selection", "pick stat scale resid label margin K margin_kind")


# ------------------------------------------------------------------------------------------------ residuals
def _two_constraint32(h, a, b, front):
    """the header's statements for kinds 1 and 2 in float32, in its association order: h [9], a, b [P,2] float32 -> [P]"""
    f = np.float32
    x, y, u, v = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    with np.errstate(all="ignore"):
        m0, m1, m2 = h[0] * x + h[1] * y + h[2], h[3] * x + h[4] * y + h[5], h[6] * x + h[7] * y + h[8]
        e0, e1 = m0 - u * m2, m1 - v * m2
        a0, a1, b0, b1 = h[0] - u * h[6], h[1] - u * h[7], h[3] - v * h[6], h[4] - v * h[7]
        mm = m2 * m2
        A, B, D = (a0 * a0 + a1 * a1) + mm, a0 * b0 + a1 * b1, (b0 * b0 + b1 * b1) + mm
        det = A * D - B * B
        s = ((D * (e0 * e0) - (f(2) * B) * (e0 * e1)) + A * (e1 * e1)) / det
        bad = ~(det > f(DET_MIN)) | (~(m2 > 0) if front else False)
    return np.where(bad, f(E_MAX), s).astype(f)


def _two_constraint64(h, a, b, front):
    """the second route, fp64: eps^T (J J^T)^-1 eps, J the 2 x 4 Jacobian of eps in (x, y, u, v), solved by LAPACK"""
    Hm = h.reshape(3, 3)
    xh = np.concatenate([a, np.ones((len(a), 1))], -1)
    m = xh @ Hm.T
    eps = np.stack([m[:, 0] - b[:, 0] * m[:, 2], m[:, 1] - b[:, 1] * m[:, 2]], -1)
    J = np.zeros((len(a), 2, 4))
    J[:, 0, :2] = Hm[0, :2] - b[:, :1] * Hm[2, :2]
    J[:, 1, :2] = Hm[1, :2] - b[:, 1:] * Hm[2, :2]
    J[:, 0, 2] = J[:, 1, 3] = -m[:, 2]
    M = J @ J.transpose(0, 2, 1)
    det = M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] ** 2
    ok = det > DET_MIN
    M[~ok] = np.eye(2)
    s = (eps * np.linalg.solve(M, eps[:, :, None])[:, :, 0]).sum(-1)
    bad = ~ok | ((m[:, 2] <= 0) if front else False)
    return np.where(bad, E_MAX, s)


def valid_model(h, dt=np.float64):
    """a finite matrix of Frobenius norm >= 1e-30 (the nine squares summed in order, in dt)"""
    h = np.asarray(h, dt).reshape(9)
    if not np.isfinite(h).all():
        return False
    ss = dt(0)
    with np.errstate(all="ignore"):
        for i in range(9):
            ss = ss + h[i] * h[i]
        nrm = np.sqrt(ss)
    return bool(nrm >= dt(MIN_SCALE) and np.isfinite(nrm))


def residuals(models, kinds, a, b, dt=np.float64):
    """e^2 [C,P] of one problem: models [C,3,3] (float32 values), a, b [P,2]; an invalid candidate's row is 1e30"""
    f = np.dtype(dt).type
    out = np.full((len(kinds), len(a)), E_MAX, dt)
    a, b = a.astype(dt), b.astype(dt)
    for c, kind in enumerate(kinds):
        if not valid_model(models[c], np.float32):
            continue
        h = np.asarray(models[c], dt).reshape(9)
        with np.errstate(all="ignore"):
            if kind == 0:
                s = C.sampson32(h.reshape(1, 9), a, b)[0] if dt == np.float32 else R8.sampson64(h.reshape(1, 3, 3), a[None], b[None])[0]
            elif dt == np.float32:
                s = _two_constraint32(h, a, b, kind == 2)
            else:
                s = _two_constraint64(h, a, b, kind == 2)
            s = np.asarray(s, dt)
            out[c] = np.where(np.isnan(s), f(E_MAX), np.abs(np.fmin(np.fmax(s, f(0)), f(E_MAX))))
    return out


def row_scale(models, kinds, a, b):
    """(scale [C,P], regular [C,P]) in fp64.  The residual is eps^T M^-1 eps with eps a sum of products of the inputs: rounding moves
    every eps_i by about eps32 mu_i (mu_i the sum of the magnitudes of its terms) and M^-1 by about eps32 kappa / lambda_min, so e^2
    moves by eps32 times
        scale = ((|eps| + eps32 mu) mu + |eps|^2 kappa) / lambda,
    kind 0: lambda = den, kappa = 1; kinds 1, 2: lambda = det / (A + D) <= lambda_min(M), kappa = (A D + B^2) / det.
    regular: the rows that are compared -- the fp64 residual is below 1e29, lambda > 0, and for kinds 1 and 2 m_z stands off its horizon (either side) by
    more than 1e-4 of the magnitudes of its terms (a rule of the reference alone)"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    x, y, u, v = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    sc, reg = np.ones((len(kinds), len(a))), np.zeros((len(kinds), len(a)), bool)
    for c, kind in enumerate(kinds):
        if not valid_model(models[c], np.float32):
            continue
        h = np.asarray(models[c], np.float64).reshape(9)
        ab = np.abs(h)
        with np.errstate(all="ignore"):
            if kind == 0:
                l2 = np.stack([h[0] * x + h[1] * y + h[2], h[3] * x + h[4] * y + h[5], h[6] * x + h[7] * y + h[8]])
                m2 = np.stack([ab[0] * abs(x) + ab[1] * abs(y) + ab[2], ab[3] * abs(x) + ab[4] * abs(y) + ab[5], ab[6] * abs(x) + ab[7] * abs(y) + ab[8]])
                l1x, l1y = h[0] * u + h[3] * v + h[6], h[1] * u + h[4] * v + h[7]
                r = u * l2[0] + v * l2[1] + l2[2]
                mu = abs(u) * m2[0] + abs(v) * m2[1] + m2[2]
                lam = l2[0] ** 2 + l2[1] ** 2 + l1x ** 2 + l1y ** 2
                sc[c] = ((np.abs(r) + EPS32 * mu) * mu + r * r) / np.where(lam > 0, lam, 1)
                reg[c] = lam > 0
            else:
                m = np.stack([h[0] * x + h[1] * y + h[2], h[3] * x + h[4] * y + h[5], h[6] * x + h[7] * y + h[8]])
                mm = np.stack([ab[0] * abs(x) + ab[1] * abs(y) + ab[2], ab[3] * abs(x) + ab[4] * abs(y) + ab[5], ab[6] * abs(x) + ab[7] * abs(y) + ab[8]])
                e0, e1 = m[0] - u * m[2], m[1] - v * m[2]
                mu = np.sqrt((mm[0] + abs(u) * mm[2]) ** 2 + (mm[1] + abs(v) * mm[2]) ** 2)
                a0, a1, b0, b1 = h[0] - u * h[6], h[1] - u * h[7], h[3] - v * h[6], h[4] - v * h[7]
                A, B, D = a0 * a0 + a1 * a1 + m[2] ** 2, a0 * b0 + a1 * b1, b0 * b0 + b1 * b1 + m[2] ** 2
                det = A * D - B * B
                ok = det > DET_MIN
                det = np.where(ok, det, 1)
                ne = np.sqrt(e0 * e0 + e1 * e1)
                sc[c] = ((ne + EPS32 * mu) * mu + ne * ne * (A * D + B * B) / det) * (A + D) / det
                reg[c] = ok & (np.abs(m[2]) > 1e-4 * mm[2])
    return sc, reg


# ------------------------------------------------------------------------------------------------ the entry point
def positive(w, n, P):
    """[n,P] bool: the rows of positive weight (a NaN is none)"""
    if w is None:
        return np.ones((n, P), bool)
    with np.errstate(invalid="ignore"):
        return np.asarray(w) > 0


def select(x1, x2, w, tau, sigma, models, kinds, outlier_cost=COST, dt=np.float64, resid=None):
    """rp_model_select: dt = float64 the reference, float32 the restatement; x1, x2 [n,P,2], w [n,P] or None, tau, sigma numbers or [n]
    (sigma None: estimated), models [n,C,3,3], kinds [C].  resid [n,C,P]: these residuals instead of computed ones -- with the device's
    own and dt = float32 every other output must then equal the device's exactly (consistent()).  margin: G of the runner-up minus G of
    the pick (inf with one valid candidate); margin_kind: the same to the best candidate of ANOTHER kind"""
    n, P = x1.shape[:2]
    Cn = len(kinds)
    f = np.dtype(dt).type
    tau = np.broadcast_to(np.asarray(tau, dt), (n,))
    sigma = np.zeros(n, dt) if sigma is None else np.broadcast_to(np.asarray(sigma, dt), (n,))
    pos = positive(w, n, P)
    out = Selection(np.full(n, -1, np.int64), np.zeros((n, Cn, 4), dt), np.zeros((n, 2), dt), np.zeros((n, Cn, P), dt),
                    np.zeros((n, P), np.int64), np.full(n, np.inf), pos.sum(-1), np.full(n, np.inf))
    out.stat[..., 0] = FLT_MAX
    out.scale[:, 1] = -1
    for b in range(n):
        e = residuals(models[b], kinds, x1[b], x2[b], dt) if resid is None else np.asarray(resid[b], dt)
        out.resid[b] = e
        valid = np.array([valid_model(models[b, c], np.float32) for c in range(Cn)])
        K, t = int(pos[b].sum()), tau[b]
        if K < K_MIN or not t > 0 or not valid.any():
            continue
        t2 = t * t
        band = pos[b][None] & (e <= t2)
        Bc = band.sum(-1)
        given = bool(sigma[b] > 0)
        s2, src = (sigma[b] * sigma[b], -1) if given else (f(FLT_MAX), -1)
        if not given:
            for c in range(Cn):
                if valid[c] and Bc[c] >= BAND_MIN:
                    med = np.sort(e[c][band[c]])[Bc[c] // 2]
                    s2c = med / f(MED_CHI2[4 - DIM[kinds[c]]])
                    if s2c < s2:
                        s2, src = s2c, c
            if src < 0:
                continue
        fl = t / f(1024)
        s2 = f(min(max(s2, fl * fl), f(E_MAX)))
        out.scale[b] = np.sqrt(s2), src
        G = np.full(Cn, np.inf)
        for c in range(Cn):
            if not valid[c]:
                continue
            dL = f(LN4) * f(DIM[kinds[c]])
            thr = (f(outlier_cost) - dL) * s2
            inl = pos[b] & (e[c] < thr)
            I = f(inl.sum())
            S = e[c][inl].sum(dtype=dt)
            G[c] = ((S / s2 + I * dL) + (f(K) - I) * f(outlier_cost)) + f(PAR[kinds[c]]) * np.log(f(4) * f(K))
            out.stat[b, c] = G[c], I, thr, Bc[c]
            out.label[b] |= inl.astype(np.int64) << c
        out.pick[b] = int(np.argmin(G))
        rest = np.sort(G[np.isfinite(G)])
        out.margin[b] = rest[1] - rest[0] if len(rest) > 1 else np.inf
        other = [G[c] for c in range(Cn) if np.isfinite(G[c]) and kinds[c] != kinds[out.pick[b]]]
        out.margin_kind[b] = min(other) - rest[0] if other else np.inf
    return out


def consistent(dev, x1, x2, w, tau, sigma, models, kinds, outlier_cost=COST):
    """EXACT consistency of the device's outputs (a Selection-like tuple of numpy arrays: pick stat scale resid label) with its OWN
    resid and thr, no tolerance: K, B_c, I_c, label, the order statistic (through scale) and the rules for invalid candidates and
    degenerate problems are recomputed from dev.resid in float32; G_c against the fp64 sum of those residuals to K eps32 relative; pick
    is the lowest index of the device's own minimum.  Returns the worst G ratio in units of K eps32"""
    n, P = x1.shape[:2]
    own = select(x1, x2, w, np.asarray(tau, np.float32), None if sigma is None else np.asarray(sigma, np.float32), models, kinds,
                 outlier_cost, np.float32, dev.resid)
    pos = positive(w, n, P)
    worst = 0.0
    for b in range(n):
        live = own.scale[b, 0] > 0
        assert (dev.pick[b] >= 0) == bool(live), (b, dev.pick[b], own.scale[b])
        assert np.array_equal(dev.scale[b], own.scale[b].astype(np.float32)), (b, dev.scale[b], own.scale[b])
        if not live:
            assert dev.pick[b] == -1 and not dev.label[b].any() and bool((dev.stat[b] == np.float32([FLT_MAX, 0, 0, 0])).all()), b
            continue
        thr = dev.stat[b, :, 2]
        lab = np.zeros(P, np.int64)
        Gd = dev.stat[b, :, 0].astype(np.float64)
        for c, kind in enumerate(kinds):
            if not valid_model(models[b, c], np.float32):
                assert bool((dev.stat[b, c] == np.float32([FLT_MAX, 0, 0, 0])).all()) and bool((dev.resid[b, c] == np.float32(E_MAX)).all()), (b, c)
                continue
            assert dev.stat[b, c, 3] == own.stat[b, c, 3], (b, c, "B_c")
            inl = pos[b] & (dev.resid[b, c] < thr[c])
            assert dev.stat[b, c, 1] == inl.sum(), (b, c, "I_c")
            lab |= inl.astype(np.int64) << c
            s2 = float(dev.scale[b, 0]) ** 2
            K, I = int(pos[b].sum()), int(inl.sum())
            G64 = dev.resid[b, c][inl].astype(np.float64).sum() / s2 + I * LN4 * DIM[kind] + (K - I) * outlier_cost + PAR[kind] * np.log(4.0 * K)
            worst = max(worst, abs(Gd[c] - G64) / (K * EPS32 * G64))
            # thr is the header's (outlier_cost - L d) sigma^2: to a few roundings
            assert abs(float(thr[c]) - (outlier_cost - LN4 * DIM[kind]) * s2) <= 8 * EPS32 * outlier_cost * s2, (b, c, "thr")
        assert np.array_equal(dev.label[b], lab), (b, "label")
        assert dev.pick[b] == int(np.argmin(np.where(Gd < FLT_MAX, Gd, np.inf))), (b, "pick")
    assert worst <= 1.0, worst
    return worst


# ------------------------------------------------------------------------------------------------ the published criterion and the flip algebra
def gric_torr(e, sigma2, kind, K):
    """Torr's robust GRIC of residuals e [K] (every row counts): sum min(e / sigma2, 2 (r - d)) + ln 4 d K + ln(4 K) k, r = 4"""
    d = DIM[kind]
    return float(np.minimum(e / sigma2, 2.0 * (4 - d)).sum() + LN4 * d * K + np.log(4.0 * K) * PAR[kind])


def expected_cost(kind, f, published, under=1.0):
    """the expected cost per row, up to the k ln(4 K) term, of a CORRECT model of `kind` at a share f of wrong matches, the noise scale
    under-estimated by the factor `under` (sigma-hat = under sigma): an inlier's e^2 / sigma^2 has mean (4 - d) / under^2 (the gate cuts
    little of it), an outlier costs 2 (r - d) + ln 4 d in the published criterion and outlier_cost = 8 in this one"""
    d = DIM[kind]
    inl = (4 - d) / under ** 2 + LN4 * d
    out = 2.0 * (4 - d) + LN4 * d if published else COST
    return (1 - f) * inl + f * out


# ------------------------------------------------------------------------------------------------ GPU cases: candidates from the truth
SHAPES = [(1, 8, 1), (3, 9, 5), (1, 255, 5), (3, 256, 8), (1, 257, 5), (130, 64, 5), (3, 513, 5), (2, 1728, 8)]
FAMILIES = ("general", "plane", "rotation")
CASES = [("mixed", n, P, Cn, wt) for n, P, Cn in SHAPES for wt in (False, True)] + [(fam, 10, 576, 5, False) for fam in FAMILIES]
KINDS8 = (0, 0, 0, 1, 2, 0, 1, 2)
LEVELS8 = (0.0, 3e-3, 1e-2, 0.0, 0.0, 3e-2, 1e-2, 1e-2)     # the size of the random perturbation of each candidate, relative to its norm
GIVEN_BELOW = 32                                            # below this P no candidate can have 16 rows in band: sigma is given
_CACHE = {}


def _scene(family, seed, P, outliers):
    """(x1, x2 [P,2] float32, E0, H0, R0 [3,3] fp64): one scene of the family and a candidate of every kind from its truth -- where the
    truth has none (a general scene has no plane, a rotating pair no translation) a plausible wrong one"""
    rng = np.random.default_rng(500 + seed)
    if family == "general":
        x1, x2, E, _ = R8.noisy_scene(seed, P, outliers)
        Rm = T.essential_rotations(E[0])[0]
        return x1[0], x2[0], E[0], Rm + 0.05 * rng.standard_normal((3, 3)), Rm
    if family == "plane":
        s = H.plane_scene(seed, P, outliers)
        return s.x1[0], s.x2[0], s.E[0], s.H, s.R
    s = T.rotation_scene(seed, P, outliers)
    t = rng.standard_normal(3)
    return s.x1[0], s.x2[0], H.cross_matrix(t / np.linalg.norm(t)) @ s.R, s.R + 2e-3 * rng.standard_normal((3, 3)), s.R


def inputs(family, n, P, Cn, weighted):
    """float32 x1, x2 [n,P,2], w [n,P] or None, models [n,Cn,3,3] float32, kinds, sigma (None: estimated; SIGMA below P = 32).  family
    "mixed": problem b is of family b mod 3; 30 % wrong matches and noise 1e-3 (50 % in the three 10 x 576 batches); candidate j is the
    truth-derived matrix of kind KINDS8[j], scaled by a random factor in [0.5, 2] and perturbed by LEVELS8[j] of its norm.  weighted:
    uniform(0.05, 1) with, from P = 24 on, 40 % zeros, a negative one and a NaN per problem"""
    key = ("in", family, n, P, Cn, weighted)
    if key not in _CACHE:
        rng = np.random.default_rng(7 * P + n + Cn)
        x1, x2, models = [], [], []
        for b in range(n):
            fam = FAMILIES[b % 3] if family == "mixed" else family
            a, c, E0, H0, R0 = _scene(fam, 100 * P + b if family == "mixed" else b, P, 0.3 if family == "mixed" else 0.5)
            base = {0: E0, 1: H0, 2: R0}
            ms = []
            for j in range(Cn):
                m = base[KINDS8[j]] / np.linalg.norm(base[KINDS8[j]])
                m = (m + LEVELS8[j] * rng.standard_normal((3, 3)) / 3) * rng.uniform(0.5, 2.0)
                ms.append(m if KINDS8[j] != 0 or b % 2 else -m)           # (an essential matrix of either sign)
            x1.append(a), x2.append(c), models.append(np.stack(ms))
        w = None
        if weighted:
            w = rng.uniform(0.05, 1.0, (n, P)).astype(np.float32)
            if P >= 24:
                w[rng.uniform(size=w.shape) < 0.4] = 0
                w[:, 5], w[:, 11] = -0.5, np.nan
        _CACHE[key] = (np.stack(x1), np.stack(x2), w, np.stack(models).astype(np.float32), KINDS8[:Cn], SIGMA if P < GIVEN_BELOW else None)
    return _CACHE[key]


def reference(*case):
    key = ("ref",) + case
    if key not in _CACHE:
        x1, x2, w, models, kinds, sigma = inputs(*case)
        _CACHE[key] = select(x1, x2, w, TAU, sigma, models, kinds)
    return _CACHE[key]


def resid_ratio(resid, ref, x1, x2, models, kinds):
    """(the worst |resid - ref.resid| / (eps32 scale) over the regular rows, the share of the rows of valid candidates that were
    compared, the number of regular rows where the reference says 1e30 and `resid` does not)"""
    worst, seen, total, wrong = 0.0, 0, 0, 0
    for b in range(len(x1)):
        sc, reg = row_scale(models[b], kinds, x1[b], x2[b])
        top = reg & (ref.resid[b] >= 1e29)
        wrong += int((resid[b][top] != np.float32(E_MAX)).sum())
        cmp_ = reg & ~top
        r = np.abs(resid[b].astype(np.float64) - ref.resid[b]) / (EPS32 * sc)
        worst = max(worst, float(r[cmp_].max(initial=0)))
        seen, total = seen + int(reg.sum()), total + sum(valid_model(models[b, c], np.float32) for c in range(len(kinds))) * x1.shape[1]
    return worst, seen / max(total, 1), wrong


def pick_bound(ref):
    """the bound behind which a pick is compared: K eps32 relative on the reference's G of its pick, per problem"""
    G = np.where(ref.pick >= 0, ref.stat[np.arange(len(ref.pick)), np.maximum(ref.pick, 0), 0], 0.0)
    return ref.K * EPS32 * G


# 8 x the restatement's worst ratio over CASES (tests/test_select_cpu.py asserts the restatement within C / 8 and above 0.9 C / 8)
C_RESID = 14.5                                       # the restatement: 1.805
WORST = dict(resid=1.805)
COMPARED_MIN = 0.90       # the share of the rows of valid candidates that the rule `regular` keeps, at least


# ------------------------------------------------------------------------------------------------ what it chooses: the fp64 chains
SHARES = (0.3, 0.5, 0.7)
AUTO_KINDS = (0, 0, 0, 1, 2)


def chain_candidates(x1, x2, tau=TAU):
    """the five candidates of select.auto_pose_from_matches from the fp64 reference chains on one scene (x1, x2 [1,P,2]): E of
    _consensus_ref.consensus_ref (M = 1024, the seed of _rotation_ref) -> eight_point_ref (4 rounds); the E of each planar pick with |t| / d > 0 after
    _refine_ref.refine_ref (10 iterations), else zero; H of _homography_ref's consensus -> refine (M = 256, 10 iterations); R of
    _rotation_ref's consensus -> refine -> [5,3,3] float32"""
    c = C.consensus_ref(x1, x2, None, tau, T.SEED, 1024)
    E = R8.eight_point_ref(x1, x2, c.weights, np.full(1, tau), iters=4)[0][0]
    hc = H.consensus(x1, x2, None, tau, H.SEED, 256)
    hr = H.refine(x1, x2, None, tau, hc.H, 10)
    d = H.decompose(hr.H, x1, x2, None, tau)
    planar = []
    for k in d.pick[0]:
        if k >= 0 and d.cstat[0, k, 2] > 0:
            planar.append(RF.refine_ref(d.pose[0, k][None], x1, x2, None, tau, 10).E[0])
        else:
            planar.append(np.zeros((3, 3)))
    rc = T.consensus(x1, x2, None, tau, T.SEED, 256)
    rr = T.refine(x1, x2, None, tau, rc.R, 10)
    return np.stack([E, planar[0], planar[1], hr.H[0], rr.R[0]]).astype(np.float32)


def family_scene(family, seed, outliers):
    if family == "general":
        return R8.noisy_scene(seed, 576, outliers)[:2]
    if family == "plane":
        return H.plane_scene(seed, 576, outliers)[:2]
    if family == "mixed":
        return H.plane_scene(seed, 576, outliers, 1e-3, 0.2)[:2]
    s = T.rotation_scene(seed, 576, outliers)
    return s.x1, s.x2


Row = collections.namedtuple("Row", "kind margin ratio kind_true margin_true")


def candidates(family, seed, outliers):
    """(x1, x2, the chain_candidates [1,5,3,3]) of one scene of the family, kept"""
    key = ("cand", family, seed, outliers)
    if key not in _CACHE:
        x1, x2 = family_scene(family, seed, outliers)
        _CACHE[key] = (x1, x2, chain_candidates(x1, x2)[None])
    return _CACHE[key]


def chosen_kinds(family, outliers, sigma, seeds=range(10)):
    """the kind chosen per scene at the given sigma (None: estimated)"""
    out = []
    for s in seeds:
        x1, x2, m = candidates(family, s, outliers)
        r = select(x1, x2, None, TAU, sigma, m, AUTO_KINDS)
        out.append(AUTO_KINDS[r.pick[0]] if r.pick[0] >= 0 else -1)
    return out


def table(family, outliers, seeds=range(10)):
    """per scene: the kind chosen with the ESTIMATED scale, the margin to the best candidate of another kind, sigma-hat / sigma, and
    kind and margin at the TRUE sigma = 1e-3"""
    key = ("table", family, outliers, tuple(seeds))
    if key not in _CACHE:
        rows = []
        for s in seeds:
            x1, x2, m = candidates(family, s, outliers)
            est = select(x1, x2, None, TAU, None, m, AUTO_KINDS)
            tru = select(x1, x2, None, TAU, SIGMA, m, AUTO_KINDS)
            rows.append(Row(AUTO_KINDS[est.pick[0]] if est.pick[0] >= 0 else -1, float(est.margin_kind[0]), float(est.scale[0, 0] / SIGMA),
                            AUTO_KINDS[tru.pick[0]] if tru.pick[0] >= 0 else -1, float(tru.margin_kind[0])))
        _CACHE[key] = rows
    return _CACHE[key]


def torr_kinds(family, outliers, seeds=range(3)):
    """the kind the PUBLISHED robust GRIC chooses per scene, at the true sigma, over the same candidates"""
    out = []
    for s in seeds:
        x1, x2, m = candidates(family, s, outliers)
        e = residuals(m[0], AUTO_KINDS, x1[0], x2[0])
        g = [gric_torr(e[c], SIGMA ** 2, AUTO_KINDS[c], x1.shape[1]) if valid_model(m[0, c], np.float32) else np.inf for c in range(5)]
        out.append(AUTO_KINDS[int(np.argmin(g))])
    return out


# the smallest margin of the chosen candidate to the best candidate of another kind, per family and share of wrong matches, as table()
# gives them over seeds 0 - 9 (tests/test_select_cpu.py asserts them to the printed digit); DESIGN.md 5.12
MARGINS = {"general": {0.3: 1111.4, 0.5: 790.1, 0.7: 61.9}, "plane": {0.3: 160.9, 0.5: 100.0, 0.7: 32.0},
           "rotation": {0.3: 32.0, 0.5: 33.2, 0.7: 32.5}}                     # with the ESTIMATED scale
MARGINS_TRUE = {"general": {0.3: 1087.1, 0.5: 777.2, 0.7: 2.8}, "plane": {0.3: 161.1, 0.5: 93.3, 0.7: 48.3},
                "rotation": {0.3: 31.2, 0.5: 32.9, 0.7: 32.5}}                # at the true sigma
RATIO_RANGE = (0.853, 1.211)                                                 # sigma-hat / sigma over those, the general family at 0.7 excluded
MIXED_ESSENTIAL = {0.3: 8, 0.5: 7, 0.7: 4}                                   # plane_scene(off_plane = 0.2): how many of 10 chose E (the rest H)
