"""References for rp_eight_point_consensus (include/relpose_consensus.h), numpy only, no GPU and no library.

  mix / draw / sample_rows   the counter-based sampler of the header in uint32 / uint64 numpy, vectorised over the hypotheses
  consensus_ref     the header in fp64: every hypothesis is _eightpoint_ref.eight_point_ref on its eight rows, the score is built from
                    sampson64; also returns sigma_8 / sigma_1 of every hypothesis' row matrix (`gap`), the scale of the bounds
  consensus_f32     the kernel's arithmetic restated in numpy float32: the same normalisation sums, the same Householder reflections
                    in the same order, the cost summed row after row (a cumulative sum).  What differs from the kernel: numpy does not
                    contract a * b + c, LAPACK's float32 SVD stands in for svd3x3_dev, numpy's log1p for the device's.  The GPU tests'
                    bounds are calibrated against it: C = 8 x its largest ratio on the same inputs.
  cost64 / weights64 / share64   the score, the Cauchy weights and the inlier weight share of any E in fp64
  CASES / inputs / reference / ratios / C_*   the cases of the GPU tests, the error ratios they bound and the calibrated constants
"""
import collections
import functools

import numpy as np

from tests import _eightpoint_ref as R

FLT_MAX = float(np.finfo(np.float32).max)
GOLDEN = 0x9E3779B9
MIN_SCALE = 1e-30

Consensus = collections.namedtuple("Consensus", "E best stat weights hyp_E hyp_cost samples gap")
Consensus.__doc__ = """E [n,3,3], best [n], stat [n,4], weights [n,P], hyp_E [n,M,3,3], hyp_cost [n,M], samples [n,M,8] as the header
documents them; gap [n,M]: sigma_8 / sigma_1 of the hypothesis' normalised 8 x 9 row matrix in fp64 (0 for an invalid one)"""


# ------------------------------------------------------------------------------------------------ the sampler
def mix(x):
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & m
    return x ^ (x >> np.uint64(16))


def draw(seed, i, m, K):
    """the eight indices c_0 .. c_7 into pos of hypotheses m (an int array) of problem i: [len(m), 8]; K >= 8"""
    m = np.atleast_1d(np.asarray(m, np.uint64))
    base = mix((np.uint64(seed & 0xFFFFFFFF) + np.uint64(GOLDEN) * np.uint64(i + 1)) & np.uint64(0xFFFFFFFF))
    s = mix(base ^ m)
    c = np.zeros((len(m), 8), np.int64)
    for k in range(8):
        r = mix((s + np.uint64((GOLDEN * (k + 1)) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF))
        j = K - 8 + k
        t = ((r * np.uint64(j + 1)) >> np.uint64(32)).astype(np.int64)
        seen = (c[:, :k] == t[:, None]).any(-1)
        c[:, k] = np.where(seen, j, t)
    return c


def clamp(w, n, P, dt=np.float64):
    if w is None:
        return np.ones((n, P), dt)
    w = np.asarray(w, dt)
    return np.where(w > 0, w, 0).astype(dt)                    # a negative weight and a NaN count as 0


def sample_rows(w, n, P, seed, M, first=0):
    """(pos per problem, samples [n,M,8] of row numbers; zeros where K < 8); problem b of the batch has index first + b"""
    wc = clamp(w, n, P)
    pos = [np.flatnonzero(wc[b] > 0) for b in range(n)]
    samples = np.zeros((n, M, 8), np.int64)
    for b in range(n):
        if len(pos[b]) >= 8:
            samples[b] = pos[b][draw(seed, first + b, np.arange(M), len(pos[b]))]
    return pos, samples


# ------------------------------------------------------------------------------------------------ fp64
def cost64(E, x1, x2, w, tau):
    """sum w tau^2 log1p(d / tau^2) / sum w per problem; E [n,3,3] or [n,M,3,3] (then [n,M]); w clamped [n,P], tau [n]"""
    E = np.asarray(E, np.float64)
    n = x1.shape[0]
    t2 = (np.asarray(tau, np.float64) ** 2).reshape(n, 1)
    if E.ndim == 4:                                            # problem by problem, every hypothesis against the same points
        M = E.shape[1]
        return np.stack([cost64(E[b], np.broadcast_to(x1[b], (M,) + x1[b].shape), np.broadcast_to(x2[b], (M,) + x2[b].shape),
                                np.broadcast_to(w[b], (M,) + w[b].shape), np.full(M, np.asarray(tau, np.float64).reshape(n)[b]))
                         for b in range(n)])
    d = R.sampson64(E, x1, x2)
    return (w * t2 * np.log1p(d / t2)).sum(-1) / w.sum(-1)


def weights64(E, x1, x2, w, tau):
    t2 = (np.asarray(tau, np.float64) ** 2).reshape(-1, 1)
    return w / (1 + R.sampson64(E, x1, x2) / t2)


def share64(E, x1, x2, w, tau):
    """(share, weight of the rows with |d / tau^2 - 1| < 1e-4, as a share) per problem"""
    t2 = (np.asarray(tau, np.float64) ** 2).reshape(-1, 1)
    u = R.sampson64(E, x1, x2) / t2
    return (w * (u <= 1)).sum(-1) / w.sum(-1), (w * (np.abs(u - 1) < 1e-4)).sum(-1) / w.sum(-1)


def hypotheses64(x1, x2, samples):
    """eight_point_ref (iters = 0, unit weights) on the sampled rows: (hyp_E [n,M,3,3], gap [n,M])"""
    n, M = samples.shape[:2]
    idx = samples.reshape(n, M * 8)
    a = np.take_along_axis(np.asarray(x1, np.float64), idx[..., None], 1).reshape(n * M, 8, 2)
    b = np.take_along_axis(np.asarray(x2, np.float64), idx[..., None], 1).reshape(n * M, 8, 2)
    E, stat, _ = R.eight_point_ref(a, b)
    return E.reshape(n, M, 3, 3), stat[:, 1].reshape(n, M)


def projection_gain(x1, x2, samples):
    """e1 / (e2 - e3), at least 1, of the singular values e of every hypothesis' F = T2^T F^ T1 in fp64, [n,M]: what the projection to
    singular values (1, 1, 0) multiplies a perturbation of F by.  1 for an F that is an essential matrix; large for a sample that holds
    outliers.  (The sign and pivot conventions of the solver do not touch singular values, so plain means and a batched SVD do.)"""
    n, M = samples.shape[:2]
    idx = samples.reshape(n, M * 8)

    def norm(x):
        p = np.take_along_axis(np.asarray(x, np.float64), idx[..., None], 1).reshape(n * M, 8, 2)
        c = p.mean(1, keepdims=True)
        m = np.linalg.norm(p - c, axis=-1).mean(1)
        s = np.sqrt(2) / np.where(m > 0, m, 1)
        T = np.zeros((n * M, 3, 3))
        T[:, 0, 0] = T[:, 1, 1] = s
        T[:, 0, 2], T[:, 1, 2], T[:, 2, 2] = -s * c[:, 0, 0], -s * c[:, 0, 1], 1
        return (p - c) * s[:, None, None], T
    (a, T1), (b, T2) = norm(x1), norm(x2)
    one = np.ones_like(a[..., :1])
    A = (np.concatenate([b, one], -1)[..., :, None] * np.concatenate([a, one], -1)[..., None, :]).reshape(n * M, 8, 9)
    f = np.linalg.svd(A)[2][:, 8].reshape(-1, 3, 3)
    e = np.linalg.svd(T2.transpose(0, 2, 1) @ f @ T1, compute_uv=False)
    return np.maximum(1, e[:, 0] / np.maximum(e[:, 1] - e[:, 2], 1e-300)).reshape(n, M)


def _select(wc, K, hyp_E, hyp_cost, dt):
    """the selection of the header: (E, best, stat with the cost, the valid count and K filled in, the clamped base weights)"""
    n, P = wc.shape
    E, best, stat, wo = np.zeros((n, 3, 3), dt), np.full(n, -1, np.int64), np.zeros((n, 4), dt), wc.astype(dt).copy()
    for b in range(n):
        valid = hyp_cost[b] < FLT_MAX
        stat[b, 2], stat[b, 3] = valid.sum(), K[b]
        if not valid.any():
            continue
        best[b] = int(np.argmin(hyp_cost[b]))                       # the first of equal minima; invalid ones hold FLT_MAX
        E[b] = hyp_E[b, best[b]]
        stat[b, 0] = hyp_cost[b, best[b]]
    return E, best, stat, wo


def consensus_ref(x1, x2, w=None, tau=0.01, seed=0, M=1024, first=0):
    """fp64 reference of rp_eight_point_consensus -> Consensus"""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    n, P = x1.shape[:2]
    tau = np.broadcast_to(np.asarray(tau, np.float64), (n,))
    wc = clamp(w, n, P)
    pos, samples = sample_rows(w, n, P, seed, M, first)
    K = np.array([len(p) for p in pos])
    hyp_E, hyp_cost, gap = np.zeros((n, M, 3, 3)), np.full((n, M), FLT_MAX), np.zeros((n, M))
    live = (K >= 8) & (tau > 0)
    if live.any():
        hE, g = hypotheses64(x1[live], x2[live], samples[live])
        ok = hE.reshape(hE.shape[0], M, 9).any(-1) & np.isfinite(hE).all((-1, -2))
        c = cost64(hE, x1[live], x2[live], wc[live], tau[live])
        ok &= np.isfinite(c) & (c < FLT_MAX)
        hyp_E[live] = np.where(ok[..., None, None], hE, 0)
        hyp_cost[live] = np.where(ok, c, FLT_MAX)
        gap[live] = np.where(ok, g, 0)
    E, best, stat, wo = _select(wc, K, hyp_E, hyp_cost, np.float64)
    won = best >= 0
    if won.any():
        wo[won] = weights64(E[won], x1[won], x2[won], wc[won], tau[won])
        stat[won, 1] = share64(E[won], x1[won], x2[won], wc[won], tau[won])[0]
    return Consensus(E, best, stat, wo, hyp_E, hyp_cost, samples, gap)


# ------------------------------------------------------------------------------------------------ float32 restatement
def _normalise8_f32(p):
    """p [H,8,2] float32 -> (centroid [H,2], scale [H], ok [H]) with the kernel's sums: about p[:, 0], one row after the other"""
    f = np.float32
    s = np.zeros((p.shape[0], 2), f)
    for k in range(8):
        s = s + (p[:, k] - p[:, 0])
    c = p[:, 0] + s / f(8)
    m = np.zeros(p.shape[0], f)
    for k in range(8):
        d = p[:, k] - c
        m = m + np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    m = m / f(8)
    ok = m >= f(MIN_SCALE)
    return c, np.sqrt(f(2)) / np.where(ok, m, f(1)), ok


def householder_null_f32(A):
    """A [H,8,9] float32, A[:, k] the k-th row of the row matrix: the kernel's eight reflections and their product applied to e_9"""
    f = np.float32
    A = np.array(A, dtype=f)
    H = A.shape[0]
    beta = np.zeros((H, 8), f)
    for j in range(8):
        sig = np.zeros(H, f)
        for i in range(j, 9):
            sig = sig + A[:, j, i] * A[:, j, i]
        nrm = np.sqrt(sig)
        den = sig + np.abs(A[:, j, j]) * nrm
        beta[:, j] = np.where(den > 0, f(1) / np.where(den > 0, den, f(1)), f(0))
        A[:, j, j] = A[:, j, j] + np.copysign(nrm, A[:, j, j])
        for k in range(j + 1, 8):
            t = np.zeros(H, f)
            for i in range(j, 9):
                t = t + A[:, j, i] * A[:, k, i]
            t = t * beta[:, j]
            for i in range(j, 9):
                A[:, k, i] = A[:, k, i] - t * A[:, j, i]
    z = np.zeros((H, 9), f)
    z[:, 8] = 1
    for j in range(7, -1, -1):
        t = np.zeros(H, f)
        for i in range(j, 9):
            t = t + A[:, j, i] * z[:, i]
        t = t * beta[:, j]
        for i in range(j, 9):
            z[:, i] = z[:, i] - t * A[:, j, i]
    return z


def minimal_solve_f32(p1, p2):
    """p1, p2 [H,8,2] float32 -> (E [H,9] float32, valid [H])"""
    f = np.float32
    c1, s1, ok1 = _normalise8_f32(p1)
    c2, s2, ok2 = _normalise8_f32(p2)
    a = (p1 - c1[:, None]) * s1[:, None, None]
    b = (p2 - c2[:, None]) * s2[:, None, None]
    one = np.ones_like(a[..., 0])
    A = np.stack([b[..., 0] * a[..., 0], b[..., 0] * a[..., 1], b[..., 0], b[..., 1] * a[..., 0], b[..., 1] * a[..., 1], b[..., 1],
                  a[..., 0], a[..., 1], one], -1).astype(f)
    z = householder_null_f32(A).reshape(-1, 3, 3)
    G = np.empty_like(z)
    G[:, :, 0] = z[:, :, 0] * s1[:, None]
    G[:, :, 1] = z[:, :, 1] * s1[:, None]
    G[:, :, 2] = z[:, :, 2] - s1[:, None] * (c1[:, None, 0] * z[:, :, 0] + c1[:, None, 1] * z[:, :, 1])
    F = np.empty_like(z)
    F[:, 0] = s2[:, None] * G[:, 0]
    F[:, 1] = s2[:, None] * G[:, 1]
    F[:, 2] = G[:, 2] - s2[:, None] * (c2[:, None, 0] * G[:, 0] + c2[:, None, 1] * G[:, 1])
    ok = ok1 & ok2 & np.isfinite(F).all((-1, -2))
    U, _, Vt = np.linalg.svd(np.where(ok[:, None, None], F, np.eye(3, dtype=f)).astype(f))
    E = (U[:, :, :2] @ Vt[:, :2]).reshape(-1, 9).astype(f)
    lead = np.abs(E).argmax(-1)                                   # the first of equal maxima
    E = np.where((E[np.arange(len(E)), lead] < 0)[:, None], -E, E)
    ok &= np.isfinite(E).all(-1)
    return np.where(ok[:, None], E, f(0)).astype(f), ok


def sampson32(E, a, b):
    """E [H,9], a, b [K,2] float32 -> d [H,K] with the kernel's expression"""
    f = np.float32
    e = [E[:, i, None].astype(f) for i in range(9)]
    ax, ay, bx, by = a[None, :, 0], a[None, :, 1], b[None, :, 0], b[None, :, 1]
    l2x, l2y, l2z = e[0] * ax + e[1] * ay + e[2], e[3] * ax + e[4] * ay + e[5], e[6] * ax + e[7] * ay + e[8]
    l1x, l1y = e[0] * bx + e[3] * by + e[6], e[1] * bx + e[4] * by + e[7]
    r = bx * l2x + by * l2y + l2z
    den = l2x * l2x + l2y * l2y + l1x * l1x + l1y * l1y
    return np.where(den > 0, r * r / np.where(den > 0, den, f(1)), f(0)).astype(f)


def consensus_f32(x1, x2, w=None, tau=0.01, seed=0, M=1024, first=0):
    """the kernels' arithmetic in numpy float32 (see the module docstring) -> Consensus (gap is not computed: zeros)"""
    f = np.float32
    x1, x2 = np.asarray(x1, f), np.asarray(x2, f)
    n, P = x1.shape[:2]
    tau = np.broadcast_to(np.asarray(tau, f), (n,))
    wc = clamp(w, n, P, f)
    pos, samples = sample_rows(w, n, P, seed, M, first)
    K = np.array([len(p) for p in pos])
    hyp_E, hyp_cost = np.zeros((n, M, 9), f), np.full((n, M), FLT_MAX, f)
    with np.errstate(all="ignore"):
        for b in range(n):
            if K[b] < 8 or not tau[b] > 0:
                continue
            E, ok = minimal_solve_f32(x1[b][samples[b]], x2[b][samples[b]])
            t2 = tau[b] * tau[b]
            d = sampson32(E, x1[b][pos[b]], x2[b][pos[b]])
            wp = wc[b][pos[b]]
            acc = np.cumsum(wp[None] * (t2 * np.log1p(d / t2)), axis=1, dtype=f)[:, -1]
            c = acc / np.cumsum(wp, dtype=f)[-1]
            ok &= c < f(FLT_MAX)
            hyp_E[b], hyp_cost[b] = np.where(ok[:, None], E, f(0)), np.where(ok, c, f(FLT_MAX))
        E, best, stat, wo = _select(wc, K, hyp_E.reshape(n, M, 3, 3), hyp_cost, f)
        for b in np.flatnonzero(best >= 0):
            t2 = tau[b] * tau[b]
            d = sampson32(E[b].reshape(1, 9), x1[b], x2[b])[0]
            wo[b] = wc[b] / (f(1) + d / t2)
            stat[b, 1] = (wc[b] * (d <= t2)).sum(dtype=f) / wc[b].sum(dtype=f)
    return Consensus(E, best, stat, wo, hyp_E.reshape(n, M, 3, 3), hyp_cost, samples, np.zeros((n, M)))


# ------------------------------------------------------------------------------------------------ the noisy scenes of the issue
def noisy_batch(outliers, weighted=False, seeds=range(10)):
    """noisy_scene(seed, 576, outliers, 1e-3) for the seeds, stacked: x1, x2 [10,576,2] float32, E_true [10,3,3], w [10,576] or None.
    weighted: base weights uniform(0.1, 1) with 40 % of them set to 0"""
    x1, x2, Et = [], [], []
    for s in seeds:
        a, b, e, _ = R.noisy_scene(s, 576, outliers, 1e-3)
        x1.append(a[0]); x2.append(b[0]); Et.append(e[0])
    w = None
    if weighted:
        rng = np.random.default_rng(99)
        w = rng.uniform(0.1, 1.0, (len(x1), 576)).astype(np.float32)
        w[rng.uniform(size=w.shape) < 0.4] = 0
    return np.stack(x1), np.stack(x2), np.stack(Et), w


# ------------------------------------------------------------------------------------------------ the cases, the ratios and their constants
# tests/test_gpu_consensus.py derives the forms of the bounds in its docstring; tests/test_consensus_cpu.py asserts that the restatement
# stays within C / 8 on these cases; tools/lab/consensus_host/run.py applies them to the kernel source run on the host.
C_E, C_E_GAIN, C_COST, C_W, C_SHIFT = {"exact": 19.0, "noisy": 995.0}, 19.0, 3.01, 2.81, 0.86      # derived in the docstring of tests/test_gpu_consensus.py
TAU, SEED = 0.01, 1
EXACT = [(1, 8, 1), (3, 9, 257), (2, 257, 256), (130, 64, 64), (2, 1728, 300)]
CASES = [("exact", n, P, M, wt) for n, P, M in EXACT for wt in (False, True)] + [("noisy", 10, 576, 1024, wt) for wt in (False, True)]


@functools.lru_cache(maxsize=None)
def inputs(kind, n, P, M, weighted):
    """float32 numpy x1, x2 [n,P,2], w [n,P] or None (exact scenes: random weights in 0.05 .. 1, every third 0 where P >= 24), E_true"""
    if kind == "noisy":
        x1, x2, Et, w = noisy_batch(0.5, weighted)
        return x1, x2, w, Et
    x1, x2, Et = R.scenes(n, P, seed=11)
    w = None
    if weighted:
        w = np.random.default_rng(P + n).uniform(0.05, 1.0, (n, P)).astype(np.float32)
        if P >= 24:
            w[:, ::3] = 0
    return x1.astype(np.float32), x2.astype(np.float32), w, Et


@functools.lru_cache(maxsize=None)
def reference(kind, n, P, M, weighted):
    x1, x2, w, _ = inputs(kind, n, P, M, weighted)
    return consensus_ref(x1, x2, w, TAU, SEED, M)


def lipschitz(E, x1, x2, wc):
    """max over the rows of positive weight of |x2h| |x1h| / sqrt(den_p) at E, per problem, fp64"""
    E = np.asarray(E, np.float64).reshape(-1, 3, 3)
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    one = np.ones_like(x1[..., :1])
    h1, h2 = np.concatenate([x1, one], -1), np.concatenate([x2, one], -1)
    l2, l1 = h1 @ E.transpose(0, 2, 1), h2 @ E
    den = l2[..., 0] ** 2 + l2[..., 1] ** 2 + l1[..., 0] ** 2 + l1[..., 1] ** 2
    k = np.linalg.norm(h1, axis=-1) * np.linalg.norm(h2, axis=-1) / np.sqrt(np.where(den > 0, den, np.inf))
    return np.where(wc > 0, k, 0).max(-1)


def shift_scale(ref, x1, x2, wc, where):
    """D1 of the module docstring for the hypotheses selected by `where` [n,M] (1 elsewhere)"""
    D = np.ones(where.shape)
    for b in range(where.shape[0]):
        m = np.flatnonzero(where[b])
        if len(m):
            bc = lambda a: np.broadcast_to(a[b], (len(m),) + a[b].shape)       # noqa: E731
            k = R.EPS32 / ref.gap[b, m] * lipschitz(ref.hyp_E[b, m], bc(x1), bc(x2), bc(wc))
            D[b, m] = 2 * k * np.sqrt(ref.hyp_cost[b, m]) + k * k
    return D


def cost_bound(c, C_=C_COST):
    return C_ * R.EPS32 * (np.sqrt(c) + R.EPS32)


def ratios(out, ref, x1, x2, w, tau=TAU):
    """out, ref: _consensus_ref.Consensus of numpy arrays -> the four ratios of the module docstring, the share of hypotheses compared
    and the mask of the hypotheses near the reference's winner"""
    n, P = x1.shape[:2]
    M = ref.hyp_cost.shape[1]
    wc = clamp(w, n, P)
    t = np.full(n, tau)
    valid = ref.hyp_cost < FLT_MAX
    assert np.array_equal(out.hyp_cost < FLT_MAX, valid)
    compared = valid & (R.EPS32 <= 1e-2 * ref.gap)
    scale = R.EPS32 / np.where(compared, ref.gap, 1)
    err = R.up_to_sign(out.hyp_E.reshape(-1, 9), ref.hyp_E.reshape(-1, 9)).reshape(n, M)
    e = (err / scale)[compared]
    sharp = R.EPS32 / np.where(valid, ref.gap, 1) * projection_gain(x1, x2, ref.samples)       # the scale that knows the projection
    compared_gain = valid & (sharp <= 1e-2)
    eg = (err / sharp)[compared_gain]
    own = cost64(out.hyp_E, x1.astype(np.float64), x2.astype(np.float64), wc, t)
    c = (np.abs(out.hyp_cost.astype(np.float64) - own) / cost_bound(own, 1.0))[valid]
    won = out.best >= 0
    want = weights64(out.E[won], x1[won], x2[won], wc[won], t[won])
    wr = (np.abs(out.weights[won].astype(np.float64) - want) / np.where(wc[won] > 0, wc[won], 1) / (R.EPS32 / tau))[wc[won] > 0]
    near = compared & (ref.hyp_cost <= 2 * ref.hyp_cost.min(-1, keepdims=True) + 1e-3 * tau * tau)
    sh = np.abs(own - ref.hyp_cost)[near] / shift_scale(ref, x1, x2, wc, near)[near]
    return dict(E=float(e.max(initial=0)), E_gain=float(eg.max(initial=0)), compared_gain=float(compared_gain.mean()), cost=float(c.max(initial=0)), w=float(wr.max(initial=0)), shift=float(sh.max(initial=0)),
                compared=float(compared.mean()), near=near)
