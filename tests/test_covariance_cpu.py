"""The pose-covariance library (include/relpose_covariance.h, librelpose_covariance.so, rel_pose_amd/covariance.py) as far as it goes
without a GPU: the header and the binding derived from it, the build, the fixed points of the kernel source, the argument checks that
precede any launch, the refusals of the host wrappers, the fp64 reference of tests/_covariance_ref.py by two routes, an analytic check,
the status rules, the float32 restatement that fixes the constants of tests/test_gpu_covariance.py, the rules its batch seeds obey, and
THE CALIBRATION: the sandwich covariance covers the error of the refined pose with wrong matches in the data, sigma^2 H^-1 does not
(DESIGN.md, 5.13)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _covariance_ref as C
from tests import _refine_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rp_covariance_abi_version", "rp_pose_covariance"}


# ------------------------------------------------------------------------------------------------ library and wrappers
def test_covariance_header_parses_and_the_library_exports_it():
    from ctypes import c_int, c_void_p
    from rel_pose_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "relpose_covariance.h")).read()
    consts, structs, sigs, status = _lib._header_contract(text, "relpose_covariance.h")
    assert consts == {"RP_COVARIANCE_ABI_VERSION": 1, "RP_COVARIANCE_MAX_P": 1728, "RP_COVARIANCE_SWEEPS": 6}
    assert not structs
    assert (_lib.COVARIANCE_ABI_VERSION, _lib.COVARIANCE_MAX_P, _lib.COVARIANCE_SWEEPS) == (1, 1728, C.SWEEPS)
    P, I = c_void_p, c_int
    assert list(sigs.items()) == [("rp_covariance_abi_version", (c_int, [])),
                                  ("rp_pose_covariance", (c_int, [P] * 11 + [I, I, P]))]
    assert status == NAMES - {"rp_covariance_abi_version"} and tuple(sigs) == _lib.COVARIANCE_EXPORTS
    declared = set(re.findall(r"\b(rp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(sigs) == NAMES
    typed = _lib.load_covariance()
    raw = ctypes.CDLL(_build.COVARIANCE_LIB)
    for sym in declared:
        assert hasattr(raw, sym), "missing export: " + sym
    assert typed.rp_covariance_abi_version() == _lib.COVARIANCE_ABI_VERSION
    # a fourteenth library, not a change of the other thirteen: it exports none of their names and they export none of its
    others = (set(_lib.EXPORTS) | set(_lib.READOUT_EXPORTS) | set(_lib.EIGHTPOINT_EXPORTS) | set(_lib.REFINE_EXPORTS)
              | set(_lib.CONSENSUS_EXPORTS) | set(_lib.SUBMATCH_EXPORTS) | set(_lib.FIVEPOINT_EXPORTS) | set(_lib.HOMOGRAPHY_EXPORTS)
              | set(_lib.TRIANGULATE_EXPORTS) | set(_lib.CONV5X5_EXPORTS) | set(_lib.GUIDED_EXPORTS) | set(_lib.ROTATION_EXPORTS)
              | set(_lib.SELECT_EXPORTS))
    assert not declared & others
    for sym in others:
        assert not hasattr(raw, sym), "librelpose_covariance.so exports " + sym
    for lib in (_build.LIB, _build.READOUT_LIB, _build.EIGHTPOINT_LIB, _build.REFINE_LIB, _build.CONSENSUS_LIB, _build.SUBMATCH_LIB,
                _build.FIVEPOINT_LIB, _build.HOMOGRAPHY_LIB, _build.TRIANGULATE_LIB, _build.CONV5X5_LIB, _build.GUIDED_LIB, _build.ROTATION_LIB,
                _build.SELECT_LIB):
        assert not any(hasattr(ctypes.CDLL(lib), sym) for sym in declared)
    assert _lib.SELECT_EXPORTS == ("rp_select_abi_version", "rp_model_select") and _lib.SELECT_ABI_VERSION == 1
    assert _lib.REFINE_EXPORTS == ("rp_refine_abi_version", "rp_refine_pose") and _lib.REFINE_ABI_VERSION == 1
    # the same errcheck as every other launching entry point
    assert typed.rp_pose_covariance.errcheck is _lib.load().rp_gemm.errcheck is _lib.load_refine().rp_refine_pose.errcheck
    assert typed.rp_covariance_abi_version.errcheck is None
    # the header documents the refusals in the order the library checks them: shape, then size, then alignment
    doc = text[:text.index("int rp_pose_covariance(")]
    doc = doc[doc.rindex("Argument checks before any launch"):]
    assert doc.index("RP_EBADSHAPE") < doc.index("RP_EUNSUPPORTED") < doc.index("RP_EALIGN")
    # and states the estimator, its sign, and how every sum associates
    for needle in ("psi'_p = w_p (1 - u_p) / (q_p q_p)", "NEGATIVE for a row beyond tau", "C = A^-1 B A^-1", "every sum of this header is taken left to right",
                   "((w0 + w1) + w2) + w3", "NOT DETERMINED", "Nothing non-finite is written for finite inputs"):
        assert needle in text, needle


def test_covariance_build_is_a_library_of_its_own():
    from rel_pose_amd import _build
    assert os.path.basename(_build.COVARIANCE_LIB) == "librelpose_covariance.so"
    libs = {_build.COVARIANCE_LIB, _build.SELECT_LIB, _build.ROTATION_LIB, _build.GUIDED_LIB, _build.CONV5X5_LIB, _build.TRIANGULATE_LIB,
            _build.HOMOGRAPHY_LIB, _build.FIVEPOINT_LIB, _build.SUBMATCH_LIB, _build.CONSENSUS_LIB, _build.REFINE_LIB, _build.EIGHTPOINT_LIB,
            _build.READOUT_LIB, _build.LIB}
    dirs = {_build.COVARIANCE_CSRC, _build.SELECT_CSRC, _build.ROTATION_CSRC, _build.GUIDED_CSRC, _build.CONV5X5_CSRC, _build.TRIANGULATE_CSRC,
            _build.HOMOGRAPHY_CSRC, _build.FIVEPOINT_CSRC, _build.SUBMATCH_CSRC, _build.CONSENSUS_CSRC, _build.REFINE_CSRC, _build.EIGHTPOINT_CSRC,
            _build.READOUT_CSRC, _build.CSRC}
    assert len(libs) == 14 and len(dirs) == 14
    assert os.path.basename(_build.COVARIANCE_CSRC) == "csrc_covariance" and _build.COVARIANCE_SOURCES == ["covariance.hip"]
    for s in _build.COVARIANCE_SOURCES:
        assert os.path.isfile(os.path.join(ROOT, "rel_pose_amd", "csrc_covariance", s))
        assert not any(os.path.exists(os.path.join(d, s)) for d in dirs - {_build.COVARIANCE_CSRC})
    assert not _build.covariance_needs_build() or _build.build(verbose=False) == _build.LIB
    assert not _build.covariance_needs_build() and not _build.select_needs_build() and not _build.needs_build()
    hdrs = _build._covariance_headers()
    assert os.path.join(ROOT, "include", "relpose_covariance.h") in hdrs and os.path.join(_build.COVARIANCE_CSRC, "sym5.h") in hdrs
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "load_covariance().rp_covariance_abi_version() == _lib.COVARIANCE_ABI_VERSION" in entry and "_build.COVARIANCE_LIB" in entry


def test_the_kernel_keeps_to_the_fixed_points_of_its_design():
    """csrc_covariance/ holds the kernel and its 5 x 5 algebra; they include the shared headers unchanged; ONE block_sum, a rolled row
    loop and a rolled sweep loop; no atomics, no allocation, no matrix instruction, no inline assembly, no `while`; LDS holds the
    reduction buffer only; the constants are those of the header and of the reference; no other library knows of it"""
    d = os.path.join(ROOT, "rel_pose_amd", "csrc_covariance")
    assert sorted(n for n in os.listdir(d) if n.endswith((".hip", ".h"))) == ["covariance.hip", "sym5.h"]
    text, alg = open(os.path.join(d, "covariance.hip")).read(), open(os.path.join(d, "sym5.h")).read()
    for needle in ("global_load_lds_dwordx4", "__builtin_amdgcn_mfma", "mfma32(", "mfma16(", "__shfl", "atomicAdd", "atomicCAS", "atomicMax",
                   "__hip_atomic", "hipMalloc", "asm(", "asm volatile", "std::sort", "consensus_core.h"):
        assert needle not in text and needle not in alg, needle
    for src in (text, alg):
        assert not re.search(r"\bwhile\s*\(", src) and not re.search(r"\bdo\s*\{", src)
    for inc in ('#include "../csrc/common.h"', '#include "../csrc/block_sum.h"', '#include "../csrc/two_view.h"',
                '#include "../../include/relpose_covariance.h"', '#include "sym5.h"'):
        assert inc in text
    assert text.count("block_sum(a, red, phase)") == 1 and len(re.findall(r"\bblock_sum\(", text)) == 1
    assert text.count("__shared__") == 1 and "__shared__ float red[2][NW][RED];" in text and "__shared__" not in alg
    assert "constexpr int RED = 34;" in text and "dim3(n), dim3(NT)" in text and "NT = BLOCK_SUM_THREADS" in text
    assert text.count("#pragma unroll 1") == 1 and alg.count("#pragma unroll 1") == 1              # the row loop; the Jacobi sweeps
    assert "sweep < RP_COVARIANCE_SWEEPS" in alg and "if (tid != 0) return;" in text
    assert "COV_PIVOT_MIN = 1e-6f" in alg and C.PIVOT_MIN == 1e-6
    assert "MIN_NORM = 1e-30f" in text and "K_MIN = 6.f" in text and (C.MIN_NORM, C.K_MIN) == (1e-30, 6)
    assert alg.count("#pragma clang fp contract(off)") == 2                                       # the normalisation and the basis
    for other in ("csrc_refine/refine_pose.hip", "csrc_select/select.hip", "csrc_consensus/consensus.hip", "csrc/two_view.h", "csrc/block_sum.h",
                  "csrc/common.h"):
        assert "covariance" not in open(os.path.join(ROOT, "rel_pose_amd", other)).read()


def test_argument_checks_come_before_any_launch():
    """no device is needed (or touched): the device pointers are never dereferenced, the refusals precede the launch, in the documented
    order"""
    from rel_pose_amd import _lib
    lib = _lib.load_covariance()
    P = ctypes.c_void_p
    ok = [P(4096 * (i + 1)) for i in range(11)]                   # pose x1 x2 w tau | cov frame eig weak stat normal
    shape = r"rel_pose_amd: rp_pose_covariance failed: bad shape \(RP error -1\)"
    unsupported = r"rel_pose_amd: rp_pose_covariance failed: unsupported \(RP error -4\)"
    align = r"rel_pose_amd: rp_pose_covariance failed: misaligned pointer/stride \(RP error -2\)"

    def call(ptrs=ok, P_=64, n=3):
        return lib.rp_pose_covariance(*ptrs, P_, n, None)

    def swap(i, v):
        return ok[:i] + [v] + ok[i + 1:]
    required = (0, 1, 2, 4, 5, 6, 7, 8, 9)
    for kw in [dict(n=0), dict(n=-1), dict(P_=5), dict(P_=0), dict(P_=-3)] + [dict(ptrs=swap(i, None)) for i in required]:
        with pytest.raises(RuntimeError, match=shape):
            call(**kw)
    for kw in (dict(P_=1729), dict(P_=1 << 20)):
        with pytest.raises(RuntimeError, match=unsupported):
            call(**kw)
    for i in range(11):
        for off in ((4, 2) if i in (1, 2) else (1, 2, 3)):
            with pytest.raises(RuntimeError, match=align):
                call(ptrs=swap(i, P(4096 * (i + 1) + off)))
    # the order of the checks: shape, then size, then alignment
    with pytest.raises(RuntimeError, match=shape):
        call(ptrs=swap(1, P(4100)), n=0, P_=5000)
    with pytest.raises(RuntimeError, match=shape):
        call(ptrs=swap(0, None), P_=5000)
    with pytest.raises(RuntimeError, match=unsupported):
        call(ptrs=swap(1, P(4100)), P_=5000)


def test_wrappers_refuse_bad_shapes_before_touching_a_device():
    from rel_pose_amd import covariance
    x, w, p = torch.zeros(3, 64, 2), torch.zeros(3, 64), torch.zeros(3, 7)
    for args, kw, match in (((p, x, x[:, :63]), {}, "x1 and x2"), ((p, x[..., :1], x[..., :1]), {}, "x1 and x2"), ((p, x[0], x[0]), {}, "x1 and x2"),
                            ((p, x, x, w[:, :5]), {}, "w must be"), ((p, x, x, w), dict(tau=torch.ones(2)), "tau"), ((p, x, x, w), dict(tau=None), "tau"),
                            ((p[:2], x, x), {}, "pose must be"), ((p[:, :6], x, x), {}, "pose must be")):
        with pytest.raises(ValueError, match=match):
            covariance.pose_covariance(*args, **kw)
    with pytest.raises(RuntimeError, match="GPU tensors"):         # well-formed, but not on a device: refused by the shared operand check
        covariance.pose_covariance(p, x, x, w)
    assert covariance.PoseCovariance._fields == ("cov", "frame", "eig", "weak", "stat", "normal")
    assert (covariance.OK, covariance.DEGENERATE, covariance.NOT_DETERMINED) == (C.OK, C.DEGENERATE, C.NOT_DETERMINED) == (1, 0, -1)
    # the device-side helpers are plain tensor arithmetic: checked here on the reference's numbers
    a = C.gpu_case(3, 256, False)
    r = C.covariance_ref(*a)
    pc = covariance.PoseCovariance(*(torch.from_numpy(np.ascontiguousarray(v)) for v in (r.cov, r.frame.reshape(3, 2, 3), r.eig, r.weak, r.stat)), None)
    assert torch.allclose(covariance.rotation_sd_deg(pc), torch.from_numpy(np.degrees(r.stat[:, 2])))
    assert torch.allclose(covariance.direction_sd_deg(pc), torch.from_numpy(np.degrees(r.stat[:, 3])))
    c3 = covariance.translation_cov3(pc).numpy()
    for b in range(3):
        t = C.unit_exact(a[0][b, :3].astype(np.float64))[0]
        assert np.abs(c3[b] @ t).max() < 1e-12 * np.abs(c3[b]).max() and np.allclose(c3[b], c3[b].T)
        assert abs(np.trace(c3[b]) - (r.cov[b, 3, 3] + r.cov[b, 4, 4])) < 1e-12 * np.trace(c3[b])


def test_pose_uncertainty_from_matches_checks_before_touching_a_device():
    import inspect
    from rel_pose_amd import covariance
    from rel_pose_amd.model import ViTEss
    from tests.test_host_cpu import make_args
    for f in (covariance.pose_uncertainty_from_matches, ViTEss.pose_uncertainty_from_matches):
        p = inspect.signature(f).parameters
        assert [n for n in p if n in ("images", "intrinsics", "pose", "chain", "chain_kwargs")] == ["images", "intrinsics", "pose", "chain", "chain_kwargs"]
        assert p["pose"].default is None and p["chain"].default == "consensus"
    doc = ViTEss.pose_uncertainty_from_matches.__doc__
    assert "eval() mode\n        only" in doc and "no module state" in doc and "does not write to `intrinsics`" in doc
    m = ViTEss(make_args()).train()
    with pytest.raises(RuntimeError, match="eval"):
        m.pose_uncertainty_from_matches(torch.zeros(1, 2, 3, 64, 64), torch.ones(1, 2, 4))
    with pytest.raises(ValueError, match="chain must be"):
        m.eval().pose_uncertainty_from_matches(torch.zeros(1, 2, 3, 64, 64), torch.ones(1, 2, 4), chain="rotation")


def test_demo_uncertainty_needs_eight_point():
    import sys
    sys.path.insert(0, ROOT)
    import demo
    g = os.path.join(ROOT, "tests", "golden", "demo")
    argv = ["--img1", os.path.join(g, "matterport_1.png"), "--img2", os.path.join(g, "matterport_2.png")]
    with pytest.raises(SystemExit):
        demo.main(argv + ["--uncertainty"])


# ------------------------------------------------------------------------------------------------ the reference
@pytest.fixture(scope="module")
def cases():
    """the inputs of every GPU case with their fp64 reference and float32 restatement, computed once"""
    out = {}
    for n, P, weighted in C.gpu_cases():
        a = C.gpu_case(n, P, weighted)
        out[(n, P, weighted)] = (a, C.covariance_ref(*a), C.covariance_f32(*a))
    return out


def test_both_fp64_routes_agree(cases):
    """C by the scaled Cholesky and by LAPACK's solve on the unscaled A: 1e-9 relative in the scaled form, |dC_ij| <= 1e-9 sqrt(C_ii C_jj);
    C is symmetric positive semi-definite, eig and weak are its eigenpair, sd_rot and sd_dir its block traces"""
    seen = 0
    for (n, P, weighted), (a, r, _) in cases.items():
        for b in range(n):
            if r.stat[b, 0] != C.OK:
                assert not r.cov[b].any() and not r.eig[b].any() and not r.weak[b].any() and not r.stat[b, 2:4].any()
                continue
            seen += 1
            sd = np.sqrt(np.diag(r.cov[b]))
            assert (np.abs(r.cov[b] - r.cov_solve[b]) <= 1e-9 * np.outer(sd, sd)).all(), (n, P, b)
            assert np.array_equal(r.cov[b], r.cov[b].T) and r.eig[b, 4] > -1e-12 * r.eig[b, 0] and (np.diff(r.eig[b]) <= 0).all()
            assert np.abs(r.cov[b] @ r.weak[b] - r.eig[b, 0] * r.weak[b]).max() <= 1e-9 * r.eig[b, 0]
            assert abs(np.linalg.norm(r.weak[b]) - 1) < 1e-12 and r.weak[b][np.argmax(np.abs(r.weak[b]))] > 0
            assert abs(r.stat[b, 2] ** 2 - np.trace(r.cov[b][:3, :3])) <= 1e-12 * r.stat[b, 2] ** 2
            assert abs(r.stat[b, 3] ** 2 - np.trace(r.cov[b][3:, 3:])) <= 1e-12 * r.stat[b, 3] ** 2
            assert 0 < r.stat[b, 4] <= 1 and r.kappa[b] >= 1
    assert seen >= 100


def test_without_wrong_matches_and_with_a_wide_tau_the_sandwich_is_the_textbook_formula():
    """w = 1, tau = 1e6 sigma, no wrong matches: psi = s and psi' = 1 up to u <= 1e-10, so A = H = sum J J^T and B = sum s^2 J J^T, and

        C - sh^2 H^-1 = H^-1 (sum_p (s_p^2 - sh^2) J_p J_p^T) H^-1,        sh^2 = sum s^2 / K.

    With H = L L^T and v_p = L^-1 J_p (sum_p v_p v_p^T = I, the leverages h_p = |v_p|^2 sum to 5) the whitened difference is
    D = L^T (C - sh^2 H^-1) L = sum_p (s_p^2 - sh^2) v_p v_p^T -- an identity, checked to 1e-9.  D does not vanish for one draw of the
    noise: its terms are independent with mean 0 (s_p ~ N(0, sigma^2): Var s^2 = 2 sigma^4), so E |D|_F^2 = 2 sigma^4 sum_p h_p^2 <=
    2 sigma^4 . 5 max h = O(1 / K) -- |D|_F / sh^2 is O(K^-1/2), the sampling error of a second moment, not O(1 / K).  The bound asserted is
    four standard deviations of it, |D|_F <= 4 sh^2 sqrt(2 sum h_p^2), and, as a deterministic companion, trace(D) = sum_p s_p^2 h_p - 5 sh^2
    exactly.  Measured at P = 576: |D|_F / sh^2 = 0.25 - 0.37 against bounds of 1.42 - 1.49 (a few rows carry
    most of the leverage: sum h^2 = 0.065, not 25 / K = 0.043)."""
    for g in (1, 2, 3):
        geom = C.mc_geometry(g, 576)
        x1, x2 = C.mc_draw(geom, np.random.default_rng([9, g]), C.SIGMA, 0.0)
        tau = 1e6 * C.SIGMA
        pose = R.refine_ref(geom.pose[None], x1[None], x2[None], None, tau, 10).pose[0]
        r = C.covariance_ref(pose[None], x1[None], x2[None], None, tau)
        assert r.stat[0, 0] == C.OK and r.stat[0, 1] == 576 and r.stat[0, 5] == 0
        t, q = C.unit_exact(pose[:3])[0], C.unit_exact(pose[3:])[0]
        E, D5 = C._frame(t, q, *C.tangent_basis_exact(t))
        s, J = R.jacobian(E, D5, x1, x2)
        H = J.T @ J
        assert np.abs(C._full(r.normal[0, :15], np.float64) / H - 1).max() < 1e-9                   # A = H: psi' = 1 - O(1e-10)
        sh2 = (s * s).sum() / 576
        L = np.linalg.cholesky(H)
        v = np.linalg.solve(L, J.T).T
        h = (v * v).sum(-1)
        assert abs(h.sum() - 5) < 1e-9
        D = L.T @ (r.cov[0] - sh2 * np.linalg.inv(H)) @ L
        direct = (v * (s * s - sh2)[:, None]).T @ v
        assert np.abs(D - direct).max() < 1e-9 * sh2
        assert abs(np.trace(D) - ((s * s * h).sum() - 5 * sh2)) < 1e-9 * sh2
        bound = 4 * np.sqrt(2 * (h * h).sum())
        print("geometry %d: |D|_F / sh^2 = %.3f, bound %.3f, sh / sigma = %.3f" % (g, np.linalg.norm(D) / sh2, bound, np.sqrt(sh2) / C.SIGMA))
        assert np.linalg.norm(D) / sh2 <= bound


def test_status_rules():
    """0: K < 6, |t| or |q| below 1e-30, a pose entry that is not finite, tau not > 0 -- every output zero; -1: most rows between tau and
    3 tau -- cov, eig, weak, sd zero, the rest written; in fp64 and in the float32 restatement alike"""
    pose, x1, x2, w, tau = C.gpu_case(3, 64, True)
    w = np.abs(np.nan_to_num(w)) + 0.05
    for ref in (C.covariance_ref, C.covariance_f32):
        base = ref(pose, x1, x2, w, tau)
        assert (base.stat[:, 0] == C.OK).all() and (base.stat[:, 1] == 64).all()

        def one(kw, b=1):
            p, ww, tt = pose.copy(), w.copy(), tau.copy()
            for k, v in kw.items():
                if k == "tau":
                    tt[b] = v
                elif k == "w":
                    ww[b] = v
                else:
                    p[b, {"t": slice(0, 3), "q": slice(3, 7)}.get(k, k)] = v
            return ref(p, x1, x2, ww, tt)
        few = np.zeros(64, np.float32)
        few[[3, 9, 20, 33, 60]] = 0.5
        few[5], few[6] = -1.0, np.nan
        six = few.copy()
        six[41] = 1e-3
        for kw in (dict(tau=0), dict(tau=-3e-3), dict(tau=np.nan), dict(t=0), dict(t=1e-31), dict(q=0), dict(q=1e-31), {0: np.nan}, {5: np.inf},
                   {2: -np.inf}, dict(w=few), dict(w=0)) + ((dict(tau=1e-30),) if ref is C.covariance_f32 else ()):     # (tau^2 leaves fp32)
            out = one(kw)
            assert all(not getattr(out, f)[1].any() for f in ("cov", "frame", "eig", "weak", "stat", "normal")), kw
            for f in ("cov", "frame", "eig", "weak", "stat", "normal"):
                assert np.array_equal(getattr(out, f)[[0, 2]], getattr(base, f)[[0, 2]])
        out = one(dict(tau=1e-30))
        assert out.stat[1, 0] != C.OK and all(np.isfinite(getattr(out, f)).all() for f in ("cov", "frame", "eig", "weak", "stat", "normal"))
        out = one(dict(w=six))
        assert out.stat[1, 1] == 6 and out.stat[1, 0] != C.DEGENERATE
        # status -1
        P = 64
        p1, a1, a2 = C.not_determined_problem(P)
        out = ref(p1[None], a1[None], a2[None], None, 3e-3)
        assert out.stat[0, 0] == C.NOT_DETERMINED and out.stat[0, 1] == P and out.stat[0, 5] >= 0.7 * P and out.stat[0, 6] > 0 and out.stat[0, 7] == 0
        assert out.stat[0, 4] <= C.PIVOT_MIN and np.isfinite(out.stat).all()
        assert not out.cov.any() and not out.eig.any() and not out.weak.any() and not out.stat[0, 2:4].any()
        assert out.frame.any() and out.normal.any() and abs(np.linalg.norm(out.frame[0, :3]) - 1) < 1e-6
        u = C._sums(p1.astype(np.float64), a1.astype(np.float64), a2.astype(np.float64), None, 3e-3, np.float64)["u"]
        assert ((u > 1) & (u < 9)).mean() >= 0.7


def test_the_frame_is_refines_basis_rule_bit_for_bit():
    """tangent_basis_exact on float32 numbers gives the bits of tests/_refine_ref.tangent_basis (the rule of relpose_refine.h) -- for
    every choice of e_k and on ties"""
    rng = np.random.default_rng(3)
    ts = [rng.standard_normal(3) for _ in range(200)] + [np.array(v, float) for v in ((1, 1, 1), (1, -1, 2), (2, 1, 1), (0, 0, 1), (0, 1, 0), (1, 0, 0),
                                                                                      (3, -3, 3), (1, 2, 1))]
    ks = set()
    for t in ts:
        t = C.unit_exact(t.astype(np.float32))[0]
        b1, b2 = C.tangent_basis_exact(t)
        r1, r2 = R.tangent_basis(t)
        assert b1.dtype == np.float32 and np.array_equal(b1, r1) and np.array_equal(b2, r2)
        ks.add(int(np.argmin(np.abs(t))))
        assert abs(b1 @ t) < 1e-6 and abs(b2 @ t) < 1e-6 and abs(b1 @ b2) < 1e-6
    assert ks == {0, 1, 2}


# ------------------------------------------------------------------------------------------------ what the GPU test relies on
def test_the_constants_of_the_gpu_bounds_are_eight_times_the_restatement(cases):
    """the worst ratios of the float32 restatement against fp64 over exactly the GPU cases; every constant of tests/_covariance_ref.py
    lies in [8, 8.5] x its ratio; the recorded ratios are the measured ones"""
    worst = np.zeros(5)
    for key, (a, r64, r32) in cases.items():
        worst = np.maximum(worst, C.gpu_errors(r32, r64))
    print("restatement (normal, cov, eig, weak, cost): %s" % (worst,))
    assert np.allclose(worst, C.RESTATEMENT, rtol=2e-3)
    for const, ratio in zip((C.C1_NORMAL, C.C2_COV, C.C_EIG, C.C3_WEAK, C.C_COST), worst):
        assert 8 * ratio <= const <= 8.5 * ratio, (const, ratio)


def test_the_gpu_batches_obey_their_rules(cases):
    """status, K, the count of negative rows and the frame of the restatement equal fp64's (the frame after rounding the fp64 pose's
    basis is NOT compared: the restatement's own is); no row within NEG_WINDOW of u = 1 (cap: NEG_CAP of the rows); at least half of every
    batch has status 1 and eig[0] / eig[1] >= GAP_MIN; every status occurs; the restated cov is exactly symmetric"""
    statuses = set()
    for (n, P, weighted), (a, r64, r32) in cases.items():
        assert np.array_equal(r64.stat[:, 0], r32.stat[:, 0]) and np.array_equal(r64.stat[:, 1], r32.stat[:, 1])
        win = C.window_rows(*a)
        assert (win <= C.NEG_CAP * P).all()
        assert (np.abs(r64.stat[:, 5] - r32.stat[:, 5]) <= win).all()
        good = (r64.stat[:, 0] == C.OK) & (r64.eig[:, 0] >= C.GAP_MIN * np.maximum(r64.eig[:, 1], 1e-300))
        assert 2 * good.sum() >= n, (n, P, weighted, good.sum())
        assert np.array_equal(r32.cov, np.swapaxes(r32.cov, 1, 2)) and r32.cov.dtype == np.float32
        assert np.isfinite(r32.stat).all() and np.isfinite(r32.cov).all()
        if weighted and P >= 9:
            assert (r64.stat[:, 1] == P - 3).all()
        statuses |= set(r64.stat[:, 0].astype(int).tolist())
        cost = R.cost64(a[0], a[1], a[2], a[3], a[4])
        assert np.abs(r64.stat[:, 6] / cost - 1).max() < 1e-9                                     # refine's cost, the same scale
    assert statuses == {C.OK, C.NOT_DETERMINED}


# ------------------------------------------------------------------------------------------------ the calibration
@pytest.mark.parametrize("g", [1, 2])
def test_the_sandwich_covers_the_error_and_the_naive_formula_does_not(g):
    """THE FINDING.  Geometry g, P = 576, sigma = 1e-3, 100 fresh draws of noise and wrong matches, refine_ref for 15
    iterations from the true pose.  Coverage = the share of draws with Mahalanobis^2 below 11.07 (should be 0.95).
      sandwich at (f, tau / sigma) = (0, 10), (0.3, 10), (0.3, 3): >= 0.80     measured 0.92 / 0.90 / 0.90 (g = 1), 0.96 / 0.97 / 0.96 (g = 2)
      sigma^2 H^-1 at (0.3, 10):                                   <= 0.50     measured 0.18 (g = 1), 0.21 (g = 2)
    No figure lies within 0.05 of its line with these seeds."""
    for f, ts in ((0.0, 10), (0.3, 10), (0.3, 3)):
        r = C.mc_run(g, 576, C.SIGMA, f, ts, 100)
        print("g %d f %.1f tau %2d sigma: coverage %.2f (naive %.2f), M2/5 %.2f (naive %.1f), sd_rot %.4f / %.4f deg, sd_dir %.4f / %.4f deg, -1: %.2f"
              % (g, f, ts, r["coverage"], r["coverage_naive"], r["m2_over_5"], r["m2_over_5_naive"], r["sd_rot_pred"], r["sd_rot_emp"],
                 r["sd_dir_pred"], r["sd_dir_emp"], r["not_determined"]))
        assert r["not_determined"] == 0
        assert r["coverage"] >= 0.80
        assert abs(r["coverage"] - 0.80) > 0.05
        if (f, ts) == (0.3, 10):
            assert r["coverage_naive"] <= 0.50
            assert abs(r["coverage_naive"] - 0.50) > 0.05
