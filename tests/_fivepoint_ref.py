"""References for rp_five_point_consensus (include/relpose_fivepoint.h), numpy only, no GPU and no library.

  draw5 / sample_rows5    the sampler of the header (the mixer of tests/_consensus_ref.py, five draws)
  five_point_ref    the solve of the header in fp64 with LAPACK, batched over the samples, by ANOTHER route than the kernel's: the null
                    space by SVD, the ten cubics fitted from their values at 40 points (no product tables), the monomials in graded
                    order, `solve` of the 10 x 10 cubic block, the eigenvectors of the 10 x 10 action matrix of x.  Also returns what
                    the GPU test's admission criterion needs: the condition number of the eliminated block, the smallest distance
                    between two roots, whether a complex eigenvalue lies within 1e-3 (relative) of the real axis
  consensus5_ref    sampler, five_point_ref per sample, the fp64 score of tests/_consensus_ref.py, the selection
  five_point_kernel the kernel's arithmetic restated at the kernel's precisions, batched: Householder null space, the product tables
                    (built here from the exponents, not copied), Gauss-Jordan with row pivoting, Nister's polynomial, the derivative
                    brackets with 48 halvings and 4 guarded Newton steps, the cross products, fp64 throughout; then the rounding to
                    float32 at norm 1 and the projection, where LAPACK's float32 SVD stands in for svd3x3_dev.  numpy does not contract
                    a * b + c.  The GPU tests' bounds are 8 x its largest error against five_point_ref on the same inputs.
  ROOT_CASES / root_inputs / root_reference / root_errors / C_*   the cases of the GPU tests, the errors they bound, the constants
"""
import collections
import functools
import itertools

import numpy as np

from tests import _consensus_ref as C
from tests import _eightpoint_ref as R

FLT_MAX = C.FLT_MAX
NR = 10
MIN_PIVOT = 1e-12
HALVINGS, NEWTON = 48, 4

Consensus5 = collections.namedtuple("Consensus5", "E best stat weights hyp_E hyp_cost samples")
Consensus5.__doc__ = """E [n,3,3], best [n,2], stat [n,4], weights [n,P], hyp_E [n,M,10,3,3], hyp_cost [n,M,10], samples [n,M,5] as the
header documents them (the reference orders a sample's roots by its own eigenvalues: the slot k need not be the kernel's)"""

Roots = collections.namedtuple("Roots", "E count cond sep near_complex")
Roots.__doc__ = """E [S,10,3,3] the real solutions, finished (zeros beyond count [S]); cond [S] the 2-norm condition number of the
eliminated 10 x 10 block; sep [S] the smallest distance, up to sign, between two solutions (inf below two); near_complex [S]: a
complex eigenvalue of the action matrix has |imag| <= 1e-3 |eigenvalue|"""


# ------------------------------------------------------------------------------------------------ the sampler
def draw5(seed, i, m, K):
    """the five indices c_0 .. c_4 into pos of samples m (an int array) of problem i: [len(m), 5]; K >= 5"""
    m = np.atleast_1d(np.asarray(m, np.uint64))
    base = C.mix((np.uint64(seed & 0xFFFFFFFF) + np.uint64(C.GOLDEN) * np.uint64(i + 1)) & np.uint64(0xFFFFFFFF))
    s = C.mix(base ^ m)
    c = np.zeros((len(m), 5), np.int64)
    for k in range(5):
        r = C.mix((s + np.uint64((C.GOLDEN * (k + 1)) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF))
        j = K - 5 + k
        t = ((r * np.uint64(j + 1)) >> np.uint64(32)).astype(np.int64)
        seen = (c[:, :k] == t[:, None]).any(-1)
        c[:, k] = np.where(seen, j, t)
    return c


def sample_rows5(w, n, P, seed, M, first=0):
    """(pos per problem, samples [n,M,5] of row numbers; zeros where K < 5); problem b of the batch has index first + b"""
    wc = C.clamp(w, n, P)
    pos = [np.flatnonzero(wc[b] > 0) for b in range(n)]
    samples = np.zeros((n, M, 5), np.int64)
    for b in range(n):
        if len(pos[b]) >= 5:
            samples[b] = pos[b][draw5(seed, first + b, np.arange(M), len(pos[b]))]
    return pos, samples


# ------------------------------------------------------------------------------------------------ fp64, LAPACK
def rows(a, b):
    """a, b [S,5,2] -> the rows x2h (x) x1h [S,5,9]"""
    one = np.ones_like(a[..., :1])
    return (np.concatenate([b, one], -1)[..., :, None] * np.concatenate([a, one], -1)[..., None, :]).reshape(a.shape[0], 5, 9)


def _monomials(q, exps):
    return np.stack([q[:, 0] ** i * q[:, 1] ** j * q[:, 2] ** k for i, j, k in exps], -1)


# graded order: the ten cubic monomials, then x^2 xy xz y^2 yz z^2 x y z 1
_REF_EXPS = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
             (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_FIT_Q = np.random.default_rng(5).uniform(-1, 1, (40, 3))
_FIT_PINV = np.linalg.pinv(_monomials(_FIT_Q, _REF_EXPS))


def constraints(Em):
    """the ten cubics at E [..,3,3]: det E and the nine entries of 2 E E^T E - tr(E E^T) E -> [..,10]"""
    EEt = Em @ np.swapaxes(Em, -1, -2)
    tr = np.trace(EEt, axis1=-2, axis2=-1)[..., None, None]
    T = 2 * EEt @ Em - tr * Em
    return np.concatenate([np.linalg.det(Em)[..., None], T.reshape(T.shape[:-2] + (9,))], -1)


def finish(E):
    """[..,3,3] fp64 -> the projection U diag(1,1,0) V^T and the sign rule of rp_eight_point"""
    U, _, Vt = np.linalg.svd(E)
    Ep = U[..., :, :2] @ Vt[..., :2, :]
    flat = Ep.reshape(-1, 9)
    lead = np.abs(flat).argmax(-1)
    flat = np.where((flat[np.arange(len(flat)), lead] < 0)[:, None], -flat, flat)
    return flat.reshape(E.shape)


def five_point_ref(a, b):
    """a, b [S,5,2] -> Roots (fp64)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    S = a.shape[0]
    basis = np.linalg.svd(rows(a, b))[2][:, 5:].reshape(S, 4, 3, 3)              # X, Y, Z, W
    q1 = np.concatenate([_FIT_Q, np.ones((40, 1))], -1)                           # [40,4]
    Em = np.einsum("qc,scij->sqij", q1, basis)
    A = np.swapaxes(np.einsum("mq,sqr->smr", _FIT_PINV, constraints(Em)), 1, 2)   # [S,10,20]
    cond = np.linalg.cond(A[:, :, :10])
    good = np.isfinite(cond) & (cond < 1e13)
    A = np.where(good[:, None, None], A, np.concatenate([np.eye(10), np.eye(10)], 1))
    Mt = np.linalg.solve(A[:, :, :10], A[:, :, 10:])
    T = np.zeros((S, 10, 10))
    T[:, :6] = -Mt[:, :6]
    T[:, 6, 0] = T[:, 7, 1] = T[:, 8, 2] = T[:, 9, 6] = 1
    lam, vec = np.linalg.eig(T)
    real = (lam.imag == 0) & good[:, None]
    near = ((lam.imag != 0) & (np.abs(lam.imag) <= 1e-3 * np.abs(lam))).any(-1)
    v = np.swapaxes(vec.real, 1, 2)                                               # [S,10 eigenvectors,10]
    with np.errstate(all="ignore"):
        xyz1 = np.concatenate([v[..., 6:9] / v[..., 9:10], np.ones((S, 10, 1))], -1)
    real &= np.isfinite(xyz1).all(-1)
    Er = np.einsum("skc,scij->skij", np.where(real[..., None], xyz1, 0), basis)
    nrm = np.linalg.norm(Er, axis=(-1, -2))
    real &= nrm > 0
    Er = np.where(real[..., None, None], Er / np.where(real, nrm, 1)[..., None, None], np.eye(3))
    Er = finish(Er)
    order = np.argsort(~real, axis=1, kind="stable")                              # the real ones first, in LAPACK's order
    Er = np.take_along_axis(Er, order[..., None, None], 1)
    count = real.sum(1)
    Er = np.where((np.arange(10)[None] < count[:, None])[..., None, None], Er, 0)
    sep = np.full(S, np.inf)
    for i, j in itertools.combinations(range(10), 2):
        d = R.up_to_sign(Er[:, i], Er[:, j])
        sep = np.where(j < count, np.minimum(sep, d), sep)
    return Roots(Er, count, cond, sep, near)


def consensus5_ref(x1, x2, w=None, tau=0.01, seed=0, M=1024, first=0):
    """fp64 reference of rp_five_point_consensus -> Consensus5"""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    n, P = x1.shape[:2]
    tau = np.broadcast_to(np.asarray(tau, np.float64), (n,))
    wc = C.clamp(w, n, P)
    pos, samples = sample_rows5(w, n, P, seed, M, first)
    K = np.array([len(p) for p in pos])
    hyp_E, hyp_cost = np.zeros((n, M, NR, 3, 3)), np.full((n, M, NR), FLT_MAX)
    E, best, stat, wo = np.zeros((n, 3, 3)), np.full((n, 2), -1, np.int64), np.zeros((n, 4)), wc.copy()
    stat[:, 3] = K
    for b in range(n):
        if K[b] < 5 or not tau[b] > 0:
            continue
        r = five_point_ref(x1[b][samples[b]], x2[b][samples[b]])
        valid = np.arange(NR)[None] < r.count[:, None]
        with np.errstate(all="ignore"):
            c = C.cost64(r.E.reshape(1, M * NR, 3, 3), x1[b:b + 1], x2[b:b + 1], wc[b:b + 1], tau[b:b + 1]).reshape(M, NR)
        valid &= np.isfinite(c) & (c < FLT_MAX)
        hyp_E[b], hyp_cost[b] = np.where(valid[..., None, None], r.E, 0), np.where(valid, c, FLT_MAX)
        stat[b, 2] = valid.sum()
        if valid.any():
            s = int(np.argmin(hyp_cost[b].ravel()))                                # the first of equal minima
            best[b] = divmod(s, NR)
            E[b] = hyp_E[b].reshape(-1, 3, 3)[s]
            stat[b, 0] = hyp_cost[b].ravel()[s]
            wo[b] = C.weights64(E[b:b + 1], x1[b:b + 1], x2[b:b + 1], wc[b:b + 1], tau[b:b + 1])[0]
            stat[b, 1] = C.share64(E[b:b + 1], x1[b:b + 1], x2[b:b + 1], wc[b:b + 1], tau[b:b + 1])[0][0]
    return Consensus5(E, best, stat, wo, hyp_E, hyp_cost, samples)


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic
_LIN = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_QUAD = [(2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
# the header's columns: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | x xz xz^2 y yz yz^2 1 z z^2 z^3
_CUBE = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
         (1, 0, 0), (1, 0, 1), (1, 0, 2), (0, 1, 0), (0, 1, 1), (0, 1, 2), (0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3)]


def _add(e, f):
    return tuple(p + q for p, q in zip(e, f))


def _mul11(a, b):
    """linear x linear [S,4] -> quadratic [S,10]"""
    q = np.zeros(a.shape[:-1] + (10,))
    for i, j in itertools.product(range(4), range(4)):
        q[..., _QUAD.index(_add(_LIN[i], _LIN[j]))] += a[..., i] * b[..., j]
    return q


def _mul21(q, l):
    """quadratic x linear -> cubic [S,20]"""
    c = np.zeros(q.shape[:-1] + (20,))
    for i, j in itertools.product(range(10), range(4)):
        c[..., _CUBE.index(_add(_QUAD[i], _LIN[j]))] += q[..., i] * l[..., j]
    return c


def _householder_null(A):
    """A [S,5,9] fp64: the kernel's five reflections -> (N [S,4,9], ok [S])"""
    A = np.array(A, np.float64)
    S = A.shape[0]
    beta, ok = np.zeros((S, 5)), np.ones(S, bool)
    for j in range(5):
        sig = np.zeros(S)
        for i in range(j, 9):
            sig = sig + A[:, j, i] * A[:, j, i]
        nrm = np.sqrt(sig)
        ok &= nrm >= MIN_PIVOT
        den = sig + np.abs(A[:, j, j]) * nrm
        beta[:, j] = np.where(den > 0, 1 / np.where(den > 0, den, 1), 0)
        A[:, j, j] = A[:, j, j] + np.copysign(nrm, A[:, j, j])
        for k in range(j + 1, 5):
            t = np.zeros(S)
            for i in range(j, 9):
                t = t + A[:, j, i] * A[:, k, i]
            t = t * beta[:, j]
            A[:, k, j:] = A[:, k, j:] - t[:, None] * A[:, j, j:]
    N = np.zeros((S, 4, 9))
    for c in range(4):
        N[:, c, 5 + c] = 1
        for j in range(4, -1, -1):
            t = np.zeros(S)
            for i in range(j, 9):
                t = t + A[:, j, i] * N[:, c, i]
            t = t * beta[:, j]
            N[:, c, j:] = N[:, c, j:] - t[:, None] * A[:, j, j:]
    return N, ok


def _pmul(a, b):
    out = np.zeros(a.shape[:-1] + (a.shape[-1] + b.shape[-1] - 1,))
    for i in range(a.shape[-1]):
        for j in range(b.shape[-1]):
            out[..., i + j] += a[..., i] * b[..., j]
    return out


def _horner(c, z):
    v = c[..., -1]
    for i in range(c.shape[-1] - 2, -1, -1):
        v = v * z + c[..., i]
    return v


def _brow(a, b):
    z = np.zeros_like(a[:, 0])
    bx = np.stack([a[:, 0], a[:, 1] - b[:, 0], a[:, 2] - b[:, 1], -b[:, 2]], -1)
    by = np.stack([a[:, 3], a[:, 4] - b[:, 3], a[:, 5] - b[:, 4], -b[:, 5]], -1)
    b1 = np.stack([a[:, 6], a[:, 7] - b[:, 6], a[:, 8] - b[:, 7], a[:, 9] - b[:, 8], -b[:, 9]], -1)
    del z
    return bx, by, b1


def five_point_kernel(a, b):
    """a, b [S,5,2] float32 -> (E [S,10,3,3] float32, the roots in ascending z, zeros beyond count; count [S])"""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    S = a.shape[0]
    with np.errstate(all="ignore"):
        N, ok = _householder_null(rows(a, b))
        l = np.swapaxes(N, 1, 2)                                                  # [S,9,4]
        Cm = np.zeros((S, 10, 20))
        Cm[:, 0] = (_mul21(_mul11(l[:, 4], l[:, 8]) - _mul11(l[:, 5], l[:, 7]), l[:, 0])
                    + _mul21(_mul11(l[:, 5], l[:, 6]) - _mul11(l[:, 3], l[:, 8]), l[:, 1])
                    + _mul21(_mul11(l[:, 3], l[:, 7]) - _mul11(l[:, 4], l[:, 6]), l[:, 2]))
        G = [[sum(_mul11(l[:, 3 * i + k], l[:, 3 * j + k]) for k in range(3)) for j in range(3)] for i in range(3)]
        h = 0.5 * (G[0][0] + G[1][1] + G[2][2])
        for i in range(3):
            G[i][i] = G[i][i] - h
        for i in range(3):
            for j in range(3):
                Cm[:, 1 + 3 * i + j] = sum(_mul21(G[i][k], l[:, 3 * k + j]) for k in range(3))
        ar = np.arange(S)
        for j in range(10):
            piv = np.abs(Cm[:, j:, j]).argmax(1) + j                              # the first of equal maxima
            ok &= np.abs(Cm[ar, piv, j]) >= MIN_PIVOT
            rj, rp = Cm[ar, j].copy(), Cm[ar, piv].copy()
            Cm[ar, piv], Cm[ar, j] = rj, rp
            Cm[:, j] = Cm[:, j] * (1 / Cm[:, j, j])[:, None]
            f = Cm[:, :, j].copy()
            f[:, j] = 0
            Cm = Cm - f[:, :, None] * Cm[:, j][:, None, :]
        Bm = [_brow(Cm[:, 4 + 2 * r, 10:], Cm[:, 5 + 2 * r, 10:]) for r in range(3)]
        (kx, ky, k1), (lx, ly, l1), (mx, my, m1) = Bm
        p = _pmul(kx, _pmul(ly, m1) - _pmul(l1, my)) + _pmul(ky, _pmul(l1, mx) - _pmul(lx, m1)) + _pmul(k1, _pmul(lx, my) - _pmul(ly, mx))
        ok &= np.abs(p[:, 10]) > 0
        Rb = np.abs(p[:, :10] / p[:, 10:]).max(-1) + 1
        ok &= Rb <= 1e300
        Rb = np.where(ok, Rb, 1.0)
        p = np.where(ok[:, None], p, 0.0)
        prev, nprev = np.zeros((S, NR)), np.zeros(S, np.int64)
        for d in range(1, 11):
            cur = np.zeros((S, 11))
            for i in range(d + 1):
                f = 1.0
                for s in range(10 - d):
                    f *= i + s + 1
                cur[:, i] = p[:, i + 10 - d] * f
            der = np.zeros((S, 11))
            der[:, :10] = cur[:, 1:] * np.arange(1, 11)
            nxt, nc = np.zeros((S, NR)), np.zeros(S, np.int64)
            lo = -Rb
            flo = _horner(cur, lo)
            for i in range(NR + 1):
                act = i <= nprev
                hi = np.where(i < nprev, prev[:, min(i, NR - 1)], Rb)
                fhi = _horner(cur, hi)
                hit = act & ((flo < 0) != (fhi < 0)) & (nc < NR)
                if hit.any():
                    x, y, nega = lo.copy(), hi.copy(), flo < 0
                    for _ in range(HALVINGS):
                        mid = 0.5 * (x + y)
                        same = (_horner(cur, mid) < 0) == nega
                        x, y = np.where(same, mid, x), np.where(same, y, mid)
                    z = 0.5 * (x + y)
                    for _ in range(NEWTON):
                        zn = z - _horner(cur, z) / _horner(der, z)
                        z = np.where((zn >= x) & (zn <= y), zn, z)
                    nxt[hit, nc[hit]] = z[hit]
                    nc = nc + hit
                lo, flo = np.where(act, hi, lo), np.where(act, fhi, flo)
            prev, nprev = nxt, nc
        count = np.where(ok, nprev, 0)
        z = prev
        ev = lambda c: _horner(c[:, None, :], z)                                   # noqa: E731
        r0, r1, r2 = (np.stack([ev(x), ev(y), ev(o)], -1) for x, y, o in Bm)
        cr = np.stack([np.cross(r0, r1), np.cross(r0, r2), np.cross(r1, r2)], 2)   # [S,10,3 pairs,3]
        pick = (cr * cr).sum(-1).argmax(-1)                                        # the first of equal maxima, as the kernel's > does
        nv = np.take_along_axis(cr, pick[..., None, None], 2)[:, :, 0]
        xyz1 = np.stack([nv[..., 0] / nv[..., 2], nv[..., 1] / nv[..., 2], z, np.ones_like(z)], -1)
        Ed = np.einsum("skc,sci->ski", xyz1, N)
        nn = np.sqrt((Ed * Ed).sum(-1))
        F = (Ed / nn[..., None]).astype(np.float32)
        live = (np.arange(NR)[None] < count[:, None]) & np.isfinite(F).all(-1) & (nn > 0)
        F = np.where(live[..., None], F, np.eye(3, dtype=np.float32).reshape(9)).reshape(S, NR, 3, 3)
        U, _, Vt = np.linalg.svd(F)
        Ep = (U[..., :, :2] @ Vt[..., :2, :]).astype(np.float32).reshape(-1, 9)
        lead = np.abs(Ep).argmax(-1)
        Ep = np.where((Ep[np.arange(len(Ep)), lead] < 0)[:, None], -Ep, Ep).reshape(S, NR, 3, 3)
    # compact the live roots to the front, keeping their order
    order = np.argsort(~live, axis=1, kind="stable")
    Ep = np.take_along_axis(Ep, order[..., None, None], 1)
    count = live.sum(1)
    return np.where((np.arange(NR)[None] < count[:, None])[..., None, None], Ep, np.float32(0)), count


# ------------------------------------------------------------------------------------------------ the GPU tests' root cases
TAU, SEED = 0.01, 1
ROOT_SHAPE = (3, 64, 256)                                                          # n, P, M
ROOT_CASES = ("exact", "noisy")
COND_MAX, SEP_MIN, LEFT_OUT_MAX = 1e4, 1e-2, 0.10


@functools.lru_cache(maxsize=None)
def root_inputs(kind):
    """float32 x1, x2 [3,64,2]: scenes(3, 64, 5), or the first 64 rows of the 50 % noisy scenes of seeds 0 .. 2"""
    n, P, _ = ROOT_SHAPE
    if kind == "exact":
        x1, x2, _ = R.scenes(n, P, 5)
        return x1.astype(np.float32), x2.astype(np.float32)
    x1, x2, _, _ = C.noisy_batch(0.5, False, seeds=range(n))
    return np.ascontiguousarray(x1[:, :P]), np.ascontiguousarray(x2[:, :P])


@functools.lru_cache(maxsize=None)
def root_reference(kind):
    """(samples [n,M,5], Roots over the n M samples, kept [n M]: the admission criterion, from the reference alone)"""
    n, P, M = ROOT_SHAPE
    x1, x2 = root_inputs(kind)
    samples = sample_rows5(None, n, P, SEED, M)[1]
    a = np.take_along_axis(x1, samples.reshape(n, M * 5, 1), 1).reshape(n * M, 5, 2)
    b = np.take_along_axis(x2, samples.reshape(n, M * 5, 1), 1).reshape(n * M, 5, 2)
    r = five_point_ref(a, b)
    kept = (r.cond <= COND_MAX) & (r.sep >= SEP_MIN) & ~r.near_complex
    return samples, a, b, r, kept


def root_errors(E, count, a, b, ref, kept):
    """E [S,10,3,3], count [S]: roots of some implementation.  -> (the largest, over the reference roots of the kept samples, of the
    distance up to sign to the nearest of the implementation's roots; the largest epipolar residual |x2h^T E x1h| of a valid slot on
    its five rows, over ALL samples; the largest distance of a valid slot's singular values from (1, 1, 0))"""
    S = E.shape[0]
    E = np.asarray(E, np.float64)
    valid = np.arange(NR)[None] < np.asarray(count)[:, None]
    d = np.full((S, NR, NR), np.inf)                                               # [sample, reference root, own root]
    for i in range(NR):
        for j in range(NR):
            d[:, i, j] = np.where(valid[:, j], R.up_to_sign(E[:, j], ref.E[:, i]), np.inf)
    nearest = d.min(-1)
    want = (np.arange(NR)[None] < ref.count[:, None]) & kept[:, None]
    root = float(nearest[want].max(initial=0))
    res = np.abs(np.einsum("skr,sjr->skj", rows(np.asarray(a, np.float64), np.asarray(b, np.float64)), E.reshape(S, NR, 9)))
    res = float(np.where(valid[:, None, :], res, 0).max(initial=0))
    sv = np.linalg.svd(E, compute_uv=False)
    ess = float(np.where(valid, np.abs(sv - [1, 1, 0]).max(-1), 0).max(initial=0))
    return root, res, ess


# 8 x the restatement's largest error on the inputs above: 1.895e-6 / 2.233e-7 (roots) and 3.102e-7 / 9.068e-8 (residuals), exact / noisy
# (tests/test_fivepoint_cpu.py asserts them; derivation in the docstring of tests/test_gpu_fivepoint.py)
C_ROOT = {"exact": 1.52e-5, "noisy": 1.79e-6}
C_RES = {"exact": 2.49e-6, "noisy": 7.26e-7}
ESSENTIAL = 1e-5                                     # singular values against (1, 1, 0): the figure of tests/test_gpu_consensus.py


def slots(out):
    """(E [S,10,3,3], count [S]) of a Consensus5 of numpy arrays; asserts that a sample's valid slots come first and that invalid slots
    hold zeros and FLT_MAX"""
    hc = out.hyp_cost.reshape(-1, NR)
    E = out.hyp_E.reshape(-1, NR, 3, 3)
    valid = hc < FLT_MAX
    count = valid.sum(1)
    assert np.array_equal(valid, np.arange(NR)[None] < count[:, None]), "a valid slot behind an invalid one"
    assert not E[~valid].any() and bool((hc[~valid] == np.float32(FLT_MAX)).all())
    return E, count


def check_roots(kind, out, tag=""):
    """what tests/test_gpu_fivepoint.py asserts of the device's roots on root_inputs(kind) (tau TAU, seed SEED, the shape ROOT_SHAPE);
    tools/lab/fivepoint_host/run.py asserts the same of the kernel source run on the host.  Returns the figures."""
    samples, a, b, ref, kept = root_reference(kind)
    assert np.array_equal(out.samples, samples), "the sampler"
    E, count = slots(out)
    root, res, ess = root_errors(E, count, a, b, ref, kept)
    left = 1 - float(kept.mean())
    print("%s%s: left out %.4f (cap %.2f), root error %.3g (bound %.3g), residual %.3g (bound %.3g), singular values off by %.3g"
          % (tag, kind, left, LEFT_OUT_MAX, root, C_ROOT[kind], res, C_RES[kind], ess))
    assert left <= LEFT_OUT_MAX
    assert root <= C_ROOT[kind] and res <= C_RES[kind] and ess <= ESSENTIAL, (kind, root, res, ess)
    return dict(left_out=left, root=root, residual=res, essential=ess)


def check_consensus(out, x1, x2, w, tau):
    """costs, best, stat and w_out of a Consensus5 of numpy arrays against the fp64 score of its OWN roots, with the bounds of
    tests/_consensus_ref.py (the scoring loop is that kernel's, expression for expression): cost_bound / C_COST, C_W; the selection
    exactly.  tau: a number.  Returns the largest ratios."""
    n, P = x1.shape[:2]
    M = out.hyp_cost.shape[1]
    wc, t = C.clamp(w, n, P), np.full(n, tau)
    x1d, x2d = x1.astype(np.float64), x2.astype(np.float64)
    E, count = slots(out)
    hc = out.hyp_cost.reshape(n, M * NR)
    valid = hc < FLT_MAX
    own = C.cost64(out.hyp_E.reshape(n, M * NR, 3, 3), x1d, x2d, wc, t)
    cr = float((np.abs(hc.astype(np.float64) - own) / C.cost_bound(np.where(valid, own, 1), 1.0))[valid].max(initial=0))
    assert cr <= C.C_COST, cr
    flat = hc.argmin(-1)                                                           # the first of equal minima
    pick = np.arange(n)
    assert bool(valid.any(-1).all())
    assert np.array_equal(out.best, np.stack([flat // NR, flat % NR], -1))
    assert np.array_equal(out.E.view(np.int32), out.hyp_E.reshape(n, M * NR, 3, 3)[pick, flat].view(np.int32))
    assert np.array_equal(out.stat[:, 0].view(np.int32), hc[pick, flat].view(np.int32))
    assert np.array_equal(out.stat[:, 2], valid.sum(-1)) and np.array_equal(out.stat[:, 3], (wc > 0).sum(-1))
    lead = np.abs(out.E.reshape(n, 9)).argmax(-1)
    assert bool((out.E.reshape(n, 9)[pick, lead] > 0).all())                       # the sign rule
    wr = 0.0
    if out.weights is not None:
        want = C.weights64(out.E, x1d, x2d, wc, t)
        wr = float((np.abs(out.weights.astype(np.float64) - want) / np.where(wc > 0, wc, 1) / (R.EPS32 / tau))[wc > 0].max(initial=0))
        assert wr <= C.C_W, wr
        assert np.array_equal(out.weights[wc == 0], np.zeros_like(out.weights[wc == 0]))
    share, edge = C.share64(out.E, x1d, x2d, wc, t)
    assert bool((np.abs(out.stat[:, 1] - share) <= edge + 4e-6).all()), (out.stat[:, 1], share, edge)
    return dict(cost=cr, w=wr)


def check_winner(kind, out):
    """the winner against consensus5_ref's on root_inputs(kind), by cost (tests/test_gpu_consensus.py derives the form): where the
    reference's winning sample passes the admission criterion the kernel holds a root within C_ROOT of the reference's winner, whose
    cost differs by at most 2 k sqrt(c) + k^2, k = C_ROOT max_p |x2h| |x1h| / sqrt(den_p); the kernel's own argmin is no worse, up to
    the rounding of the two costs"""
    n, P, M = ROOT_SHAPE
    x1, x2 = root_inputs(kind)
    ref = consensus5_ref(x1, x2, None, TAU, SEED, M)
    kept = root_reference(kind)[4].reshape(n, M)
    wc, t = np.ones((n, P)), np.full(n, TAU)
    c_k = C.cost64(out.E, x1.astype(np.float64), x2.astype(np.float64), wc, t)
    k = C_ROOT[kind] * C.lipschitz(ref.E, x1, x2, wc)
    upper = ref.stat[:, 0] + 2 * k * np.sqrt(ref.stat[:, 0]) + k * k + 2 * C.cost_bound(np.maximum(c_k, ref.stat[:, 0]))
    ok = kept[np.arange(n), ref.best[:, 0]]
    print("winner %s: own cost" % kind, c_k, "reference", ref.stat[:, 0], "allowed", upper, "reference winner admitted", ok)
    assert bool(ok.any()) and bool((c_k <= upper)[ok].all()), (c_k, upper)
    assert np.array_equal(out.stat[:, 3], ref.stat[:, 3])
