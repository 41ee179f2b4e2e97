"""Inputs, fp64 references and bounds for the edge-of-domain tests of the scalar geometry kernels (csrc/svd3x3.h, csrc/geom.hip,
csrc/se3loss.hip).  numpy / torch on the CPU only, no GPU and no library: tests/test_gpu_geometry_edges.py runs them on the GPU,
tests/test_host_cpu.py calibrates the loss constants with the float32 CPU run of rel_pose_amd/se3.py, tools/lab/geom_host/run.py runs
the kernels themselves on the host.

Loss sweep.  One pair per (theta, |tau|) of LOSS_THETAS x LOSS_TAUS: random poses Ps, G[:, 0] = P[:, 0] and G[:, 1] = Delta * P[:, 1] with
Delta = Exp(|tau| d, theta a) for random unit d, a, composed in fp64 and rounded to float32 -- the first term of the pair then has the
residual Delta, the second a conjugate of its inverse.  theta = 0 copies the quaternion and tau = 0 the translation bit for bit.
The references see the same float32 numbers:
  gradients   rel_pose_amd.losses.geodesic_loss_tensors_torch in fp64; per pair g = d(mean) / dG[b] * 2B, 14 numbers for each of the two losses
  values      scipy.linalg.logm of the 4 x 4 matrix of each term.  From theta = pi - 1e-5 on the fp64 formulas stand in: the principal
              logarithm is ill-conditioned at the cut (eigenvalues -1 +- 1e-5 i and closer), and which of the two half-turn logarithms it
              returns decides |tau|; tests/test_host_cpu.py pins the fp64 formulas to logm on every other row.
Bounds per pair, theta and |tau| the smaller of the reference's two terms, T the largest translation entry of the pair:
  rotation      |g - g64|_inf <= C_ROT eps32 (1 + 1 / theta) |g64|_inf      (phi = 2 atan2(n, w) u / n: n carries an absolute error eps32)
  translation   |g - g64|_inf <= C_TR eps32 (1 + T / |tau|) |g64|_inf       (tau carries an absolute error eps32 T)
  values        |tau| within C_VAL_TR eps32 (1 + T), |phi| within C_VAL_ROT eps32, absolute
A nominal theta = 0 (|tau| = 0) puts the pair on the kink of |phi| (|tau|): that gradient is the unit direction of rounding noise in any
implementation.  A nominal theta = pi puts it on the cut of the logarithm: the inputs' |w| is of the size of their float32 rounding, its
sign picks one of the two half-turn logarithms, |phi| has its ridge there and tau jumps.  On these rows the affected gradients are only
required to be finite and within a Lipschitz bound: KINK = 4 for |phi| (the existing loss test's: two terms, |d phi / dq| <= 2 each) and
KINK_TR (1 + T) for |tau| (per term |V^-1| <= 3.6 times |d t / dG| of order 1 + 4 |t|, plus |dV^-1 / dphi| |t| |dphi / dq| of the same
order: 16 (1 + T) per term, two terms, a factor 2 of slack -- it is there to catch a blow-up, not a digit); at theta = pi the value of
|tau| is only required to be finite, |phi| is continuous across the cut and keeps its bound.
Each constant is 8 x the largest ratio that the float32 CPU run of rel_pose_amd/se3.py shows on these same inputs (the factor covers
fused multiply-adds and the device's sinf / cosf / atan2f); tests/test_host_cpu.py: test_loss_sweep_constants repeats the measurement:
    rotation gradient     2.80 (theta = 9e-7, |tau| = 5)                 -> C_ROT = 22.4
    translation gradient  6.51 (theta = 1e-3, |tau| = 1e-6; 4.97 outside theta = 1.1e-4 .. 1e-2)   -> C_TR = 52
    |tau| values          2.73     |phi| values  2.79                   -> C_VAL_TR = 21.8, C_VAL_ROT = 22.3
With c(theta) taken from its closed form above 1e-4 (before C_SERIES = 0.5) the same run gives up to 571 for the translation gradient in
theta = 1.1e-4 .. 1e-2 (at theta = 3e-4, |tau| = 5), which C_TR rejects."""
import functools
import itertools

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
LOSS_THETAS = (0.0, 1e-7, 9e-7, 1.1e-6, 1e-5, 9e-5, 1.1e-4, 3e-4, 1e-3, 1e-2, 0.1, 1.0, 2.0, np.pi - 0.1, np.pi - 1e-3, np.pi - 1e-5, np.pi)
LOSS_TAUS = (0.0, 1e-6, 1e-3, 1.0, 5.0)
LOGM_UP_TO = np.pi - 1e-4          # rows with a larger nominal theta take their reference values from the fp64 formulas
C_ROT, C_TR, C_VAL_TR, C_VAL_ROT = 22.4, 52.0, 21.8, 22.3
KINK, KINK_TR = 4.0, 64.0


# ------------------------------------------------------------------------------------------------ the loss
def _hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def _rot(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


@functools.lru_cache(maxsize=None)
def loss_sweep(seed=5):
    """(Ps, Gs) float32 torch [B,2,7], B = len(LOSS_THETAS) * len(LOSS_TAUS), row = theta-major; and the nominal (theta, |tau|) [B,2]"""
    rng = np.random.default_rng(seed)
    grid = list(itertools.product(LOSS_THETAS, LOSS_TAUS))
    B = len(grid)
    Ps, Gs = np.empty((B, 2, 7), np.float32), np.empty((B, 2, 7), np.float32)
    for b, (th, nt) in enumerate(grid):
        for k in range(2):
            q = rng.standard_normal(4)
            Ps[b, k] = np.concatenate([rng.standard_normal(3), q / np.linalg.norm(q)])
        Gs[b] = Ps[b]
        p1 = Ps[b, 1].astype(np.float64)
        a, d = _unit(rng), _unit(rng)
        if th > 0:
            K = _hat(a)
            V = np.eye(3) + (1 - np.cos(th)) / th * K + (th - np.sin(th)) / th * K @ K
            dq = np.concatenate([a * np.sin(th / 2), [np.cos(th / 2)]])
            Gs[b, 1, 3:] = _qmul(dq, p1[3:])
            Gs[b, 1, :3] = V @ (nt * d) + _rot(dq) @ p1[:3]
        elif nt > 0:
            Gs[b, 1, :3] = nt * d + p1[:3]
    return torch.from_numpy(Ps), torch.from_numpy(Gs), np.array(grid)


def loss_gradients(fn, Ps, Gs):
    """per-pair gradients [B,14] of the two losses fn(SE3(Ps), [SE3(Gs)]) w.r.t. Gs, times 2B (so that a pair's gradient does not depend
    on the batch it is in), as fp64 numpy"""
    from rel_pose_amd.se3 import SE3
    G = Gs.clone().requires_grad_(True)
    ltr, lrot = fn(SE3(Ps), [SE3(G)])
    gtr, = torch.autograd.grad(ltr, G, retain_graph=True)
    grot, = torch.autograd.grad(lrot, G)
    B = Gs.shape[0]
    return tuple((2 * B * g).reshape(B, 14).double().cpu().numpy() for g in (gtr, grot))


def loss_terms64(Ps, Gs):
    """the fp64 formulas per term: (|tau| [B,2], |phi| [B,2]) and the 4 x 4 matrices [B,2,4,4] of the residuals"""
    from rel_pose_amd.se3 import SE3
    P, G = SE3(Ps.double()), SE3(Gs.double())
    dP, dG = SE3(P.data.flip(1)) * P.inv(), SE3(G.data.flip(1)) * G.inv()
    d = dG * dP.inv()
    tau, phi = d.log().split([3, 3], dim=-1)
    M = np.zeros(tuple(d.data.shape[:2]) + (4, 4))
    dn = d.data.numpy()
    for b in range(M.shape[0]):
        for j in range(2):
            M[b, j, :3, :3], M[b, j, :3, 3], M[b, j, 3, 3] = _rot(dn[b, j, 3:]), dn[b, j, :3], 1.0
    return tau.norm(dim=-1).numpy(), phi.norm(dim=-1).numpy(), M


@functools.lru_cache(maxsize=None)
def loss_reference(seed=5):
    """dict: g_tr, g_rot [B,14] (fp64 autograd), v_tr, v_rot [B] (the two loss values of each pair alone: logm below LOGM_UP_TO, the fp64
    formulas above), theta, tau [B] (the smaller of the reference's two terms), T [B]"""
    from rel_pose_amd.losses import geodesic_loss_tensors_torch
    try:
        from scipy.linalg import logm
    except ImportError:                      # without scipy the fp64 formulas are the value reference on every row
        logm = None
    Ps, Gs, grid = loss_sweep(seed)
    g_tr, g_rot = loss_gradients(geodesic_loss_tensors_torch, Ps.double(), Gs.double())
    nt, nphi, M = loss_terms64(Ps, Gs)
    v_tr, v_rot = nt.mean(-1), nphi.mean(-1)
    for b in np.nonzero(grid[:, 0] <= LOGM_UP_TO)[0] if logm else ():
        L = [np.real(logm(M[b, j])) for j in range(2)]
        v_tr[b] = np.mean([np.linalg.norm(l[:3, 3]) for l in L])
        v_rot[b] = np.mean([np.linalg.norm([l[2, 1], l[0, 2], l[1, 0]]) for l in L])
    T = np.maximum(np.abs(Ps.numpy()[:, :, :3]).max((1, 2)), np.abs(Gs.numpy()[:, :, :3]).max((1, 2))).astype(np.float64)
    return dict(g_tr=g_tr, g_rot=g_rot, v_tr=v_tr, v_rot=v_rot, theta=nphi.min(-1), tau=nt.min(-1), T=T, grid=grid)


def loss_ratios(g_tr, g_rot, v_tr, v_rot, ref):
    """the four error ratios of the module docstring per pair [B] (nan where the pair is on that loss's kink), and the kink rows' largest
    gradient entries over their bound: (r_rot, r_tr, r_vtr, r_vrot, kink)"""
    grid, T = ref["grid"], ref["T"]
    with np.errstate(divide="ignore", invalid="ignore"):
        r_rot = np.abs(g_rot - ref["g_rot"]).max(-1) / (EPS32 * (1 + 1 / ref["theta"]) * np.abs(ref["g_rot"]).max(-1))
        r_tr = np.abs(g_tr - ref["g_tr"]).max(-1) / (EPS32 * (1 + T / ref["tau"]) * np.abs(ref["g_tr"]).max(-1))
    cut = grid[:, 0] == np.pi
    on_rot, on_tr = (grid[:, 0] == 0) | cut, (grid[:, 1] == 0) | cut
    kink = max(float((np.abs(g_rot[on_rot]).max(-1) / KINK).max()), float((np.abs(g_tr[on_tr]).max(-1) / (KINK_TR * (1 + T[on_tr]))).max()))
    r_rot[on_rot], r_tr[on_tr] = np.nan, np.nan
    r_vtr = np.abs(v_tr - ref["v_tr"]) / (EPS32 * (1 + T))
    r_vtr[cut] = np.nan
    return r_rot, r_tr, r_vtr, np.abs(v_rot - ref["v_rot"]) / EPS32, kink


def loss_values(fn, Ps, Gs):
    """the two loss values of every pair alone (B = 1 calls): v_tr, v_rot [B] fp64 numpy"""
    from rel_pose_amd.se3 import SE3
    out = np.empty((Gs.shape[0], 2))
    for b in range(Gs.shape[0]):
        ltr, lrot = fn(SE3(Ps[b:b + 1]), [SE3(Gs[b:b + 1])])
        out[b] = float(ltr), float(lrot)
    return out[:, 0], out[:, 1]


# ------------------------------------------------------------------------------------------------ the 3 x 3 SVD
def random_rotations(n, rng):
    q = rng.standard_normal((n, 4))
    return np.stack([_rot(v) for v in q])


@functools.lru_cache(maxsize=None)
def svd_special():
    """{tag: float32 [n,3,3]}: matrices whose singular values coincide -- rotations (a triple), the 48 signed permutations, diagonals with
    repeated and zero entries in every position and sign, and U diag(1, 1, 0) V^T for random rotations U, V"""
    rng = np.random.default_rng(48)
    perms = []
    for p in itertools.permutations(range(3)):
        for s in itertools.product((1.0, -1.0), repeat=3):
            M = np.zeros((3, 3))
            M[np.arange(3), list(p)] = s
            perms.append(M)
    diags = [np.diag(np.array(d, float) * s) for d in ((2, 2, 1), (2, 1, 2), (1, 2, 2), (1, 1, 2), (1, 2, 1), (2, 1, 1), (3, 3, 3), (1, 1, 0),
                                                       (1, 0, 1), (0, 1, 1), (0, 0, 1), (0, 1, 0), (1, 0, 0), (0.5, 0.5, 1e-3))
             for s in itertools.product((1.0, -1.0), repeat=3)]
    U, V = random_rotations(64, rng), random_rotations(64, rng)
    return {"rotation": random_rotations(64, rng).astype(np.float32), "signed_permutation": np.stack(perms).astype(np.float32),
            "repeated_diagonal": np.stack(diags).astype(np.float32),
            "rank2_equal": (U @ np.diag([1.0, 1.0, 0.0]) @ V.transpose(0, 2, 1)).astype(np.float32)}


def svd_errors(A, U, S, V):
    """(e_s, e_rec, e_orth) of tests/test_gpu_kernels.py's SVD test against LAPACK in fp64: singular values and U diag(S) V^T - A relative to
    sigma_1, U^T U - I and V^T V - I; and whether S is ordered and non-negative.  A zero matrix is measured absolutely."""
    A, U, S, V = (np.asarray(a, np.float64) for a in (A, U, S, V))
    s_ref = np.linalg.svd(A, compute_uv=False)
    scale = np.where(s_ref[:, :1] > 0, s_ref[:, :1], 1.0)
    e_s = float((np.abs(S - s_ref) / scale).max())
    rec = (U * S[:, None, :]) @ V.transpose(0, 2, 1)
    e_rec = float((np.abs(rec - A).max((1, 2)) / scale[:, 0]).max())
    eye = np.eye(3)
    e_orth = max(float(np.abs(U.transpose(0, 2, 1) @ U - eye).max()), float(np.abs(V.transpose(0, 2, 1) @ V - eye).max()))
    ordered = bool((S[:, 0] >= S[:, 1]).all() and (S[:, 1] >= S[:, 2]).all() and (S >= 0).all())
    return e_s, e_rec, e_orth, ordered


@functools.lru_cache(maxsize=None)
def svd_generic(n=256, seed=9):
    return np.random.default_rng(seed).standard_normal((n, 3, 3)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the decode
DECODE_N, DECODE_P, DECODE_SEED = 90, 12, 7


@functools.lru_cache(maxsize=None)
def decode_inputs(kind):
    """float32 E_true [n,3,3], x1, x2 [n,P,2] and the fp64 true pose [n,7] of tests/_eightpoint_ref.wide_scenes"""
    from tests import _eightpoint_ref as R
    x1, x2, E, pose = R.wide_scenes(DECODE_N, DECODE_P, DECODE_SEED, kind)
    return E.astype(np.float32), x1.astype(np.float32), x2.astype(np.float32), pose


def decode_errors(out, pose):
    """rotation angle [n] (rad; quaternions compared up to sign) and cos of the angle between the directions of t [n]"""
    out, pose = np.asarray(out, np.float64), np.asarray(pose, np.float64)
    qd = np.clip(np.abs((out[:, 3:] * pose[:, 3:]).sum(-1)), 0, 1)
    tn = pose[:, :3] / np.linalg.norm(pose[:, :3], axis=-1, keepdims=True)
    return 2 * np.arccos(qd), (out[:, :3] * tn).sum(-1)
