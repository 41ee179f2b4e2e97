"""The model-selection library (include/relpose_select.h, librelpose_select.so, rel_pose_amd/select.py) as far as it goes without a GPU:
the header and the binding derived from it, the build, the fixed points of the kernel source, the argument checks that precede any
launch, the refusals of the host wrappers, the fp64 reference of tests/_select_ref.py on hand-computable cases, the flip algebra of the
published criterion and of this one, the restatement of the kernel's residuals that calibrates the GPU bound, and what the criterion
chooses on the three scene families -- the tables of DESIGN.md 5.12."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _homography_ref as H
from tests import _rotation_ref as T
from tests import _select_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rp_select_abi_version", "rp_model_select"}


# ------------------------------------------------------------------------------------------------ library and wrappers
def test_select_header_parses_and_the_library_exports_it():
    from ctypes import c_float, c_int, c_void_p
    from rel_pose_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "relpose_select.h")).read()
    consts, structs, sigs, status = _lib._header_contract(text, "relpose_select.h")
    assert consts == {"RP_SELECT_ABI_VERSION": 1, "RP_SELECT_MAX_P": 1728, "RP_SELECT_MAX_C": 8}
    assert not structs
    assert (_lib.SELECT_ABI_VERSION, _lib.SELECT_MAX_P, _lib.SELECT_MAX_C) == (1, 1728, 8)
    P, I, F = c_void_p, c_int, c_float
    assert list(sigs.items()) == [("rp_select_abi_version", (c_int, [])),
                                  ("rp_model_select", (c_int, [P, P, P, P, P, P, P, F, P, P, P, P, P, I, I, I, P]))]
    assert status == NAMES - {"rp_select_abi_version"} and tuple(sigs) == _lib.SELECT_EXPORTS
    declared = set(re.findall(r"\b(rp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(sigs) == NAMES
    typed = _lib.load_select()
    raw = ctypes.CDLL(_build.SELECT_LIB)
    for sym in declared:
        assert hasattr(raw, sym), "missing export: " + sym
    assert typed.rp_select_abi_version() == _lib.SELECT_ABI_VERSION
    # a thirteenth library, not a change of the other twelve: it exports none of their names and they export none of its
    others = (set(_lib.EXPORTS) | set(_lib.READOUT_EXPORTS) | set(_lib.EIGHTPOINT_EXPORTS) | set(_lib.REFINE_EXPORTS)
              | set(_lib.CONSENSUS_EXPORTS) | set(_lib.SUBMATCH_EXPORTS) | set(_lib.FIVEPOINT_EXPORTS) | set(_lib.HOMOGRAPHY_EXPORTS)
              | set(_lib.TRIANGULATE_EXPORTS) | set(_lib.CONV5X5_EXPORTS) | set(_lib.GUIDED_EXPORTS) | set(_lib.ROTATION_EXPORTS))
    assert not declared & others
    for sym in others:
        assert not hasattr(raw, sym), "librelpose_select.so exports " + sym
    for lib in (_build.LIB, _build.READOUT_LIB, _build.EIGHTPOINT_LIB, _build.REFINE_LIB, _build.CONSENSUS_LIB, _build.SUBMATCH_LIB,
                _build.FIVEPOINT_LIB, _build.HOMOGRAPHY_LIB, _build.TRIANGULATE_LIB, _build.CONV5X5_LIB, _build.GUIDED_LIB, _build.ROTATION_LIB):
        assert not any(hasattr(ctypes.CDLL(lib), sym) for sym in declared)
    assert _lib.ROTATION_EXPORTS == ("rp_rotation_abi_version", "rp_rotation_consensus", "rp_rotation_refine") and _lib.ROTATION_ABI_VERSION == 1
    # the same errcheck as every other launching entry point
    assert typed.rp_model_select.errcheck is _lib.load().rp_gemm.errcheck is _lib.load_rotation().rp_rotation_refine.errcheck
    assert typed.rp_select_abi_version.errcheck is None
    # the header documents the refusals in the order the library checks them: shape, then size, then alignment
    doc = text[:text.index("int rp_model_select(")]
    doc = doc[doc.rindex("Argument checks before any launch"):]
    assert doc.index("RP_EBADSHAPE") < doc.index("RP_EUNSUPPORTED") < doc.index("RP_EALIGN")
    # and says that the criterion counts a row once, and how every residual associates
    assert "counts a\n *   row ONCE" in text and "every sum is taken left to right unless" in text


def test_select_build_is_a_library_of_its_own():
    from rel_pose_amd import _build
    assert os.path.basename(_build.SELECT_LIB) == "librelpose_select.so"
    libs = {_build.SELECT_LIB, _build.ROTATION_LIB, _build.GUIDED_LIB, _build.CONV5X5_LIB, _build.TRIANGULATE_LIB, _build.HOMOGRAPHY_LIB,
            _build.FIVEPOINT_LIB, _build.SUBMATCH_LIB, _build.CONSENSUS_LIB, _build.REFINE_LIB, _build.EIGHTPOINT_LIB, _build.READOUT_LIB, _build.LIB}
    dirs = {_build.SELECT_CSRC, _build.ROTATION_CSRC, _build.GUIDED_CSRC, _build.CONV5X5_CSRC, _build.TRIANGULATE_CSRC, _build.HOMOGRAPHY_CSRC,
            _build.FIVEPOINT_CSRC, _build.SUBMATCH_CSRC, _build.CONSENSUS_CSRC, _build.REFINE_CSRC, _build.EIGHTPOINT_CSRC, _build.READOUT_CSRC,
            _build.CSRC}
    assert len(libs) == 13 and len(dirs) == 13
    assert os.path.basename(_build.SELECT_CSRC) == "csrc_select" and _build.SELECT_SOURCES == ["select.hip"]
    for s in _build.SELECT_SOURCES:
        assert os.path.isfile(os.path.join(ROOT, "rel_pose_amd", "csrc_select", s))
        assert not any(os.path.exists(os.path.join(d, s)) for d in dirs - {_build.SELECT_CSRC})
    assert not _build.select_needs_build() or _build.build(verbose=False) == _build.LIB
    assert not _build.select_needs_build() and not _build.rotation_needs_build() and not _build.needs_build()
    assert os.path.join(ROOT, "include", "relpose_select.h") in _build._select_headers()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "load_select().rp_select_abi_version() == _lib.SELECT_ABI_VERSION" in entry and "_build.SELECT_LIB" in entry


def test_the_kernel_keeps_to_the_fixed_points_of_its_design():
    """csrc_select/ holds one file; it includes the shared headers unchanged and its own; it uses sampson() of csrc/two_view.h as it is
    and sums through block_sum; no atomics, no allocation, no matrix instruction, no inline assembly, no sort, no `while`; the constants
    are those of the header and of the reference; the other solver files know nothing of it"""
    d = os.path.join(ROOT, "rel_pose_amd", "csrc_select")
    assert sorted(n for n in os.listdir(d) if n.endswith((".hip", ".h"))) == ["select.hip"]
    text = open(os.path.join(d, "select.hip")).read()
    for needle in ("global_load_lds_dwordx4", "__builtin_amdgcn_mfma", "__shfl", "atomicAdd", "atomicCAS", "atomicMax", "__hip_atomic",
                   "hipMalloc", "asm(", "asm volatile", "std::sort", "consensus_core.h"):
        assert needle not in text, needle
    assert not re.search(r"\bwhile\s*\(", text) and not re.search(r"\bdo\s*\{", text)
    for inc in ('#include "../csrc/common.h"', '#include "../csrc/block_sum.h"', '#include "../csrc/two_view.h"',
                '#include "../../include/relpose_select.h"'):
        assert inc in text
    assert text.count("sampson(h, p, q)") == 1 and text.count("block_sum(") == 3          # counts; one per bit; inliers
    assert text.count("__shared__") == 1 and "__shared__ float red[2][NW][RED];" in text  # LDS holds the reduction buffer only
    assert "for (int bit = 31; bit >= 0; --bit)" in text
    assert "DET_MIN = 1e-30f, E_MAX = 1e30f" in text and (S.DET_MIN, S.E_MAX) == (1e-30, 1e30)
    assert "LN4 = 1.386294361f" in text and "MED_CHI2_1 = 0.454936423f, MED_CHI2_2 = LN4" in text
    assert (S.LN4, S.MED_CHI2) == (1.386294361, {1: 0.454936423, 2: 1.386294361})
    assert abs(S.LN4 - np.log(4)) < 1e-9 and abs(S.MED_CHI2[1] - 0.6744897501960817 ** 2) < 1e-9      # the medians of chi^2_2, chi^2_1
    assert "BAND_MIN = 16" in text and "K_MIN = 8" in text and (S.BAND_MIN, S.K_MIN) == (16, 8)
    assert "kind == 0 ? 3.f : 2.f" in text and "kind == 0 ? 5.f : kind == 1 ? 8.f : 3.f" in text
    assert (S.DIM, S.PAR) == ({0: 3, 1: 2, 2: 2}, {0: 5, 1: 8, 2: 3})
    for other in ("csrc_consensus/consensus.hip", "csrc_homography/homography.hip", "csrc_rotation/rotation.hip", "csrc/two_view.h",
                  "csrc/block_sum.h"):
        assert "select.h" not in open(os.path.join(ROOT, "rel_pose_amd", other)).read()


def test_argument_checks_come_before_any_launch():
    """no device is needed (or touched): the device pointers are never dereferenced, the refusals precede the launch, in the documented
    order; `kinds` is a host array and IS read"""
    from rel_pose_amd import _lib
    lib = _lib.load_select()
    P = ctypes.c_void_p
    kinds = (ctypes.c_int * 8)(0, 0, 0, 1, 2, 0, 1, 2)
    ok = [P(4096 * (i + 1)) for i in range(12)]                   # x1 x2 w tau sigma models | pick stat scale resid label ; kinds apart
    shape = r"rel_pose_amd: rp_model_select failed: bad shape \(RP error -1\)"
    unsupported = r"rel_pose_amd: rp_model_select failed: unsupported \(RP error -4\)"
    align = r"rel_pose_amd: rp_model_select failed: misaligned pointer/stride \(RP error -2\)"

    def call(ptrs=ok, P_=64, C=5, n=3, cost=8.0, k=kinds):
        return lib.rp_model_select(*ptrs[:6], None if k is None else ctypes.cast(k, P), cost, *ptrs[6:11], P_, C, n, None)

    def swap(i, v):
        return ok[:i] + [v] + ok[i + 1:]
    bad = [dict(n=0), dict(n=-1), dict(P_=7), dict(P_=0), dict(C=0), dict(C=-2), dict(k=None), dict(cost=4.0), dict(cost=3 * S.LN4),
           dict(cost=float("nan")), dict(cost=float("inf")), dict(cost=1.5e6), dict(k=(ctypes.c_int * 5)(0, 1, 3, 0, 0)),
           dict(k=(ctypes.c_int * 5)(0, 1, 2, 0, -1))]
    for kw in bad + [dict(ptrs=swap(i, None)) for i in (0, 1, 3, 5, 6, 7, 8)]:
        with pytest.raises(RuntimeError, match=shape):
            call(**kw)
    for kw in (dict(P_=1729), dict(P_=1 << 20), dict(C=9), dict(C=1 << 20)):
        with pytest.raises(RuntimeError, match=unsupported):
            call(**kw)
    for i in range(11):
        for off in ((4, 2) if i < 2 else (1, 2, 3)):
            with pytest.raises(RuntimeError, match=align):
                call(ptrs=swap(i, P(4096 * (i + 1) + off)))
    with pytest.raises(RuntimeError, match=align):                                # a host array two bytes off: refused unread
        lib.rp_model_select(*ok[:6], P(ctypes.addressof(kinds) + 2), 8.0, *ok[6:11], 64, 5, 3, None)
    for i in (2, 4, 9, 10):                                                       # the optional operands may be absent
        assert i not in (0, 1, 3, 5, 6, 7, 8)
    # the order of the checks: shape, then size, then alignment
    with pytest.raises(RuntimeError, match=shape):
        call(ptrs=swap(0, P(4100)), n=0, P_=5000)
    with pytest.raises(RuntimeError, match=shape):
        call(ptrs=swap(0, P(4100)), C=9, k=(ctypes.c_int * 9)(0, 0, 0, 0, 0, 0, 0, 5, 0))
    with pytest.raises(RuntimeError, match=unsupported):
        call(ptrs=swap(0, P(4100)), P_=5000)
    with pytest.raises(RuntimeError, match=unsupported):
        call(ptrs=swap(3, P(4 * 4096 + 1)), C=9, k=(ctypes.c_int * 9)(*([0] * 9)))


def test_wrappers_refuse_bad_shapes_before_touching_a_device():
    from rel_pose_amd import select
    x, w, m = torch.zeros(3, 64, 2), torch.zeros(3, 64), torch.zeros(3, 5, 3, 3)
    k = select.AUTO_KINDS
    for args, kw, match in (((x, x[:, :63], None, m, k), {}, "x1 and x2"), ((x[..., :1], x[..., :1], None, m, k), {}, "x1 and x2"),
                            ((x[0], x[0], None, m, k), {}, "x1 and x2"), ((x, x, w[:, :5], m, k), {}, "w must be"),
                            ((x, x, w, m, k), dict(tau=torch.ones(2)), "tau"), ((x, x, w, m, k), dict(tau=None), "tau"),
                            ((x, x, w, m[:, :4], k), {}, "models must be"), ((x, x, w, m[:2], k), {}, "models must be"),
                            ((x, x, w, m.reshape(3, 5, 9), k), {}, "models must be"), ((x, x, w, m, k[:4]), {}, "models must be"),
                            ((x, x, w, m, k), dict(sigma=torch.ones(2)), "sigma must be")):
        with pytest.raises(ValueError, match=match):
            select.model_select(*args, **kw)
    with pytest.raises(RuntimeError, match="GPU tensors"):         # well-formed, but not on a device: refused by the shared operand check
        select.model_select(x, x, w, m, k)
    assert select.Selection._fields == ("pick", "stat", "scale", "residuals", "labels")
    assert select.AUTO_KINDS == S.AUTO_KINDS == (0, 0, 0, 1, 2) and len(select.AUTO_NAMES) == 5 and select.KIND_NAMES == ("essential", "homography", "rotation")


def test_auto_pose_from_matches_checks_before_touching_a_device():
    import inspect
    from rel_pose_amd import select
    from rel_pose_amd.model import ViTEss
    from tests.test_host_cpu import make_args
    for f in (select.auto_pose_from_matches, ViTEss.auto_pose_from_matches):
        p = inspect.signature(f).parameters
        names = ("heads", "hypotheses", "seed", "refine", "tau", "sigma", "subtoken", "radius", "minimal")
        assert [n for n in p if n in names] == list(names)
        assert [p[k].default for k in names] == [(0, 1, 2), (1024, 256, 256), 0, 10, None, None, None, 2, "eight"]
    assert select.AutoMatchPose._fields == ("pose", "kind", "selection", "consensus", "planar", "rotation")
    doc = ViTEss.auto_pose_from_matches.__doc__
    assert "eval() mode only" in doc and "no module state" in doc and "does not write to\n        `intrinsics`" in doc
    m = ViTEss(make_args()).train()
    with pytest.raises(RuntimeError, match="eval"):
        m.auto_pose_from_matches(torch.zeros(1, 2, 3, 64, 64), torch.ones(1, 2, 4))
    with pytest.raises(ValueError, match="minimal"):
        m.eval().auto_pose_from_matches(torch.zeros(1, 2, 3, 64, 64), torch.ones(1, 2, 4), minimal="seven")
    with pytest.raises(ValueError, match="hypotheses"):
        m.auto_pose_from_matches(torch.zeros(1, 2, 3, 64, 64), torch.ones(1, 2, 4), hypotheses=(64, 64))


def test_demo_auto_needs_eight_point():
    import sys
    sys.path.insert(0, ROOT)
    import demo
    g = os.path.join(ROOT, "tests", "golden", "demo")
    argv = ["--img1", os.path.join(g, "matterport_1.png"), "--img2", os.path.join(g, "matterport_2.png")]
    with pytest.raises(SystemExit):
        demo.main(argv + ["--auto"])


# ------------------------------------------------------------------------------------------------ the reference on hand-computable cases
def test_residuals_vanish_under_the_true_model_of_an_exact_scene():
    """exact scenes (float32 inputs): e^2 under the true model is at the level of the inputs' rounding, (4 eps32)^2 of the field, for
    every kind, by both routes; a wrong model of the same kind is far above; a row that R sends behind the camera costs 1e30"""
    x1, x2, Ht, poses, _, _ = H.exact_scenes(3, 40, 5)
    for b in range(3):
        E = H.cross_matrix(poses[b, :3]) @ H.quat_to_rot(poses[b, 3:])
        m = np.stack([E, Ht[b]]).astype(np.float32)
        for dt in (np.float64, np.float32):
            e = S.residuals(m, (0, 1), x1[b], x2[b], dt)
            assert e.dtype == dt and e.max() < (8 * S.EPS32) ** 2, (b, dt, e.max())
        wrong = S.residuals(np.stack([E.T, Ht[b].T]).astype(np.float32), (0, 1), x1[b], x2[b])
        assert np.median(wrong, -1).min() > 1e-6
    x1, x2, Rt = T.exact_scenes(3, 40, 6)
    for b in range(3):
        m = np.stack([Rt[b], 2.5 * Rt[b]]).astype(np.float32)
        for dt in (np.float64, np.float32):
            e = S.residuals(m, (2, 1), x1[b], x2[b], dt)
            assert e.max() < (8 * S.EPS32) ** 2
        back = S.residuals(-m, (2, 1), x1[b], x2[b])                      # -R: every row behind the camera; as a homography the same fit
        assert bool((back[0] == S.E_MAX).all()) and back[1].max() < (8 * S.EPS32) ** 2
    # the two routes of kinds 1 and 2 agree on noisy rows
    s = H.plane_scene(1, 100, 0.3)
    h = (s.H + 0.01 * np.random.default_rng(0).standard_normal((3, 3))).reshape(9)
    a, c = s.x1[0].astype(np.float64), s.x2[0].astype(np.float64)
    r64, r32 = S._two_constraint64(h, a, c, False), S._two_constraint32(h.astype(np.float32), s.x1[0], s.x2[0], False)
    x, y, u, v = a[:, 0], a[:, 1], c[:, 0], c[:, 1]
    m = np.stack([h[0] * x + h[1] * y + h[2], h[3] * x + h[4] * y + h[5], h[6] * x + h[7] * y + h[8]])
    e0, e1 = m[0] - u * m[2], m[1] - v * m[2]
    A = (h[0] - u * h[6]) ** 2 + (h[1] - u * h[7]) ** 2 + m[2] ** 2
    D = (h[3] - v * h[6]) ** 2 + (h[4] - v * h[7]) ** 2 + m[2] ** 2
    B = (h[0] - u * h[6]) * (h[3] - v * h[6]) + (h[1] - u * h[7]) * (h[4] - v * h[7])
    closed = (D * e0 * e0 - 2 * B * e0 * e1 + A * e1 * e1) / (A * D - B * B)
    assert np.abs(r64 - closed).max() <= 1e-12 * closed.max() and np.abs(r32 - closed).max() <= 1e-4 * closed.max()
    # to first order it is the squared distance to the model's manifold: half the transfer distance where only image 2 carries the error
    assert np.abs(closed / H.transfer(h.reshape(3, 3), a, c) - 1).max() < 1.0


def test_the_order_statistic_and_the_criterion_on_a_constructed_list():
    """one candidate, 40 rows with chosen residuals: 25 inside the band tau^2 = 1e-4, so rank 12 of the band in ascending order; the
    scale, the gate, the inlier count and G follow by hand"""
    P = 40
    x = np.zeros((1, P, 2), np.float32)
    m = np.eye(3, dtype=np.float32)[None, None]
    band = (np.arange(25) + 1) * 3e-6                                      # 3e-6 .. 7.5e-5
    e = np.concatenate([band, np.full(15, 5e-3)])
    e = e[np.random.default_rng(4).permutation(P)][None, None]
    for kind, med_chi2, d, k in ((0, 0.454936423, 3, 5), (1, 1.386294361, 2, 8), (2, 1.386294361, 2, 3)):
        r = S.select(x, x, None, 0.01, None, m, (kind,), resid=e)
        s2 = band[12] / med_chi2
        assert r.stat[0, 0, 3] == 25 and abs(r.scale[0, 0] - np.sqrt(s2)) < 1e-15 and r.scale[0, 1] == 0 and r.pick[0] == 0
        thr = (8 - S.LN4 * d) * s2
        inl = band[band < thr]
        assert abs(r.stat[0, 0, 2] - thr) < 1e-12 * thr and r.stat[0, 0, 1] == len(inl)
        G = inl.sum() / s2 + len(inl) * S.LN4 * d + (P - len(inl)) * 8 + k * np.log(4 * P)
        assert abs(r.stat[0, 0, 0] - G) < 1e-7 * G
        assert np.array_equal(r.label[0] == 1, e[0, 0] < thr)
    # weights only say which rows exist: their size changes nothing, a zero, a negative one and a NaN take the row out
    w = np.ones((1, P), np.float32)
    out = np.flatnonzero(e[0, 0] < 1e-4)[:3]
    w[0, out] = 0, -2, np.nan
    a = S.select(x, x, w, 0.01, None, m, (0,), resid=e)
    b = S.select(x, x, np.where(w > 0, 0.01, w).astype(np.float32), 0.01, None, m, (0,), resid=e)
    assert a.K[0] == P - 3 and a.stat[0, 0, 3] == 22 and np.array_equal(a.stat, b.stat) and not a.label[0, out].any()
    # a given sigma is used as it is; the floor (tau / 1024)^2 holds for it, too; fewer than 16 rows in band give no scale
    g = S.select(x, x, None, 0.01, 2e-3, m, (0,), resid=e)
    assert g.scale[0].tolist() == [2e-3, -1] and S.select(x, x, None, 0.01, 1e-9, m, (0,), resid=e).scale[0, 0] == 0.01 / 1024
    few = S.select(x, x, None, 2e-3 ** 0.5 * 0.1, None, m, (0,), resid=e)                  # tau^2 = 2e-5: 6 rows in band
    assert few.pick[0] == -1 and few.scale[0].tolist() == [0, -1] and few.stat[0, 0].tolist() == [S.FLT_MAX, 0, 0, 0]


def test_the_flip_shares_of_the_published_criterion_and_of_this_one():
    """Torr's robust GRIC caps an outlier at 2 (r - d): 6.16 under E, 6.77 under H and R.  Per inlier the correct two-dimensional model
    gains 0.386 over E, per outlier it loses 0.614: the published criterion flips to E at a share 0.386 of wrong matches.  This one
    charges 8 under every model: no share flips it.  It flips when sigma is under-estimated by more than sqrt(1.386)"""
    assert abs((2 * 1 + S.LN4 * 3) - 6.16) < 0.005 and abs((2 * 2 + S.LN4 * 2) - 6.77) < 0.005
    gain = S.expected_cost(0, 0, True) - S.expected_cost(1, 0, True)
    loss = S.expected_cost(1, 1, True) - S.expected_cost(0, 1, True)
    assert abs(gain - 0.386) < 5e-4 and abs(loss - 0.614) < 5e-4 and abs(gain / (gain + loss) - 0.386) < 5e-4
    for f in np.linspace(0, 0.99, 100):
        assert (S.expected_cost(1, f, True) < S.expected_cost(0, f, True)) == (f < gain / (gain + loss))
        assert S.expected_cost(1, f, False) < S.expected_cost(0, f, False)
        assert abs((S.expected_cost(0, f, False) - S.expected_cost(1, f, False)) - (1 - f) * gain) < 1e-12     # outliers cancel
    edge = 1 / np.sqrt(S.LN4)
    for under in (0.5, 0.7, 0.84, 0.86, 1.0, 1.5, 3.0):
        assert (S.expected_cost(1, 0.5, False, under) < S.expected_cost(0, 0.5, False, under)) == (under > edge)
    # on built scenes: the published criterion, at the true sigma and over the same candidates, picks H on the planes at 30 % and E at
    # 50 % and 70 %; R on the rotations at 30 % and E from 50 % on (3 seeds)
    assert S.torr_kinds("plane", 0.3) == [1, 1, 1] and S.torr_kinds("plane", 0.7) == [0, 0, 0]
    assert S.torr_kinds("rotation", 0.3) == [2, 2, 2] and S.torr_kinds("rotation", 0.5) == [0, 0, 0] and S.torr_kinds("rotation", 0.7) == [0, 0, 0]
    # gric_torr on a list by hand
    e = np.array([0.0, 1e-6, 2e-6, 1.0])
    assert abs(S.gric_torr(e, 1e-6, 1, 4) - ((0 + 1 + 2 + 4) + S.LN4 * 2 * 4 + np.log(16) * 8)) < 1e-9


# ------------------------------------------------------------------------------------------------ the calibration of the GPU bound
def test_restatement_is_within_the_calibrated_bound_and_the_listed_inputs_leave_out_no_pick():
    """C_RESID = 8 x the restatement's worst ratio on the GPU tests' own inputs: within C / 8, and above 0.9 C / 8 -- the constant is that
    figure, not a looser one.  The restatement is consistent with itself exactly as the device must be.  Under the reference every
    listed problem has a pick whose margin exceeds the bound K eps32 G: the GPU test compares every pick"""
    worst, share = 0.0, 1.0
    for case in S.CASES:
        x1, x2, w, models, kinds, sigma = S.inputs(*case)
        ref = S.reference(*case)
        res = S.select(x1, x2, w, S.TAU, sigma, models, kinds, dt=np.float32)
        r, sh, wrong = S.resid_ratio(res.resid, ref, x1, x2, models, kinds)
        worst, share = max(worst, r), min(share, sh)
        assert wrong == 0 and sh >= S.COMPARED_MIN, (case, sh)
        S.consistent(res, x1, x2, w, S.TAU, sigma, models, kinds)
        assert bool((ref.pick >= 0).all()) and bool((ref.margin > S.pick_bound(ref)).all()), case
        assert np.array_equal(res.pick, ref.pick) and np.array_equal(res.scale[:, 1], ref.scale[:, 1])
    print("restatement: resid %.4g, compared share >= %.4f" % (worst, share))
    assert 0.9 * S.C_RESID / 8 <= worst <= S.C_RESID / 8, (worst, S.C_RESID)
    assert abs(worst - S.WORST["resid"]) <= 0.01 * S.WORST["resid"] + 1e-3
    # the three families of the noisy batches are chosen as what they are, all ten
    for fam, kind in (("general", 0), ("plane", 1), ("rotation", 2)):
        ref = S.reference(fam, 10, 576, 5, False)
        assert [S.KINDS8[p] for p in ref.pick] == [kind] * 10


# ------------------------------------------------------------------------------------------------ what it chooses: the tables of DESIGN.md 5.12
@pytest.mark.parametrize("family,kind", [("general", 0), ("plane", 1), ("rotation", 2)])
def test_the_three_pure_families_are_chosen_ten_of_ten(family, kind):
    """the candidates of the fp64 reference chains, P = 576, noise 1e-3, tau = 0.01, seeds 0 - 9, 30 / 50 / 70 % wrong matches: with
    the ESTIMATED scale and at the true sigma the family's own model is chosen 10 of 10; sigma-hat / sigma stays within [0.8, 1.3]
    (the general family at 70 % excluded: the eight-point consensus itself is past its limit there); the margins are those recorded"""
    for f in S.SHARES:
        rows = S.table(family, f)
        ratio = [r.ratio for r in rows]
        print("%s f = %.1f: estimated %s margin %.1f, sigma-hat / sigma %.3f .. %.3f; true sigma %s margin %.1f"
              % (family, f, [r.kind for r in rows], min(r.margin for r in rows), min(ratio), max(ratio), [r.kind_true for r in rows],
                 min(r.margin_true for r in rows)))
        assert [r.kind for r in rows] == [kind] * 10 and [r.kind_true for r in rows] == [kind] * 10
        if (family, f) != ("general", 0.7):
            assert 0.8 <= min(ratio) and max(ratio) <= 1.3
            assert S.RATIO_RANGE[0] - 5e-4 <= min(ratio) and max(ratio) <= S.RATIO_RANGE[1] + 5e-4
        assert abs(min(r.margin for r in rows) - S.MARGINS[family][f]) <= 0.051
        assert abs(min(r.margin_true for r in rows) - S.MARGINS_TRUE[family][f]) <= 0.051


def test_the_mixed_family_is_never_a_rotation():
    """plane_scene(off_plane = 0.2): a fifth of the points off the plane -- E and H both describe it and the choice splits between them
    (recorded, not asserted beyond its count); R is never chosen.  The labels separate the off-plane points: most of them are inliers of E and
    outliers of H"""
    for f in S.SHARES:
        kinds = [r.kind for r in S.table("mixed", f)]
        print("mixed f = %.1f: %s" % (f, kinds))
        assert 2 not in kinds and -1 not in kinds
        assert kinds.count(0) == S.MIXED_ESSENTIAL[f]
    x1, x2, m = S.candidates("mixed", 0, 0.3)
    r = S.select(x1, x2, None, S.TAU, None, m, S.AUTO_KINDS)
    on_E, on_H = (r.label[0] & 1) > 0, (r.label[0] >> 3 & 1) > 0
    off = 0.2 * 0.7 * 576                                                  # the off-plane points that are no wrong matches: 81
    print("inliers of E alone %d, of H alone %d, of both %d" % ((on_E & ~on_H).sum(), (on_H & ~on_E).sum(), (on_E & on_H).sum()))
    assert 0.5 * off <= (on_E & ~on_H).sum() <= off + 0.05 * 576


def test_the_criterion_needs_a_scale_that_is_not_under_estimated():
    """sigma given as 0.7 of the truth (under the edge 1 / sqrt(1.386) = 0.85): the plane and rotation rows break up -- E is chosen on
    some of every ten --, as the algebra says; at 1.5 of the truth everything holds"""
    for fam, kind in (("general", 0), ("plane", 1), ("rotation", 2)):
        for f in S.SHARES:
            over = S.chosen_kinds(fam, f, 1.5 * S.SIGMA)
            under = S.chosen_kinds(fam, f, 0.7 * S.SIGMA)
            print("%s f = %.1f: at 0.7 sigma %s, at 1.5 sigma %s" % (fam, f, under, over))
            assert over == [kind] * 10
            if kind != 0:
                assert under.count(0) >= 3
