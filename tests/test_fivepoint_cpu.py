"""The calibrated five-point consensus (include/relpose_fivepoint.h, librelpose_fivepoint.so, rel_pose_amd/fivepoint.py) as far as it
goes without a GPU: the header and the binding derived from it, the build, the fixed points of the kernel source, the argument checks
that precede any launch, the refusals of the host wrappers, the sampler, the fp64 reference of tests/_fivepoint_ref.py on exact and
on noisy scenes -- the table of DESIGN.md 5.6 --, and the restatement of the kernel's arithmetic that calibrates the GPU tests' bounds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _consensus_ref as C
from tests import _eightpoint_ref as R
from tests import _fivepoint_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ library and wrappers
def test_fivepoint_header_parses_and_the_library_exports_it():
    from ctypes import c_int, c_void_p
    from rel_pose_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "relpose_fivepoint.h")).read()
    consts, structs, sigs, status = _lib._header_contract(text, "relpose_fivepoint.h")
    assert consts == {"RP_FIVEPOINT_ABI_VERSION": 1, "RP_FIVEPOINT_MAX_P": 1728, "RP_FIVEPOINT_MAX_M": 4096, "RP_FIVEPOINT_ROOTS": 10}
    assert not structs
    assert (_lib.FIVEPOINT_ABI_VERSION, _lib.FIVEPOINT_MAX_P, _lib.FIVEPOINT_MAX_M, _lib.FIVEPOINT_ROOTS) == (1, 1728, 4096, 10)
    P, I = c_void_p, c_int
    assert list(sigs.items()) == [("rp_fivepoint_abi_version", (c_int, [])),
                                  ("rp_five_point_consensus", (c_int, [P, P, P, P, I, P, P, P, P, P, P, P, I, I, I, P]))]
    assert status == {"rp_five_point_consensus"} and tuple(sigs) == _lib.FIVEPOINT_EXPORTS
    # the declarations as a C reader sees them (comments stripped), independently of the parser: exactly the two names
    declared = set(re.findall(r"\b(rp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(sigs) == {"rp_fivepoint_abi_version", "rp_five_point_consensus"}
    typed = _lib.load_fivepoint()
    raw = ctypes.CDLL(_build.FIVEPOINT_LIB)
    for sym in declared:
        assert hasattr(raw, sym), "missing export: " + sym
    assert typed.rp_fivepoint_abi_version() == _lib.FIVEPOINT_ABI_VERSION
    # a seventh library, not a change of the other six: it exports none of their names and their headers declare none of its
    others = (set(_lib.EXPORTS) | set(_lib.READOUT_EXPORTS) | set(_lib.EIGHTPOINT_EXPORTS) | set(_lib.REFINE_EXPORTS)
              | set(_lib.CONSENSUS_EXPORTS) | set(_lib.SUBMATCH_EXPORTS))
    assert not declared & others
    for sym in others:
        assert not hasattr(raw, sym), "librelpose_fivepoint.so exports " + sym
    for h in ("relpose_hip.h", "relpose_readout.h", "relpose_eightpoint.h", "relpose_refine.h", "relpose_consensus.h", "relpose_submatch.h"):
        t = open(os.path.join(ROOT, "include", h)).read()
        assert "fivepoint" not in t and "five_point" not in t
    for lib in (_build.LIB, _build.READOUT_LIB, _build.EIGHTPOINT_LIB, _build.REFINE_LIB, _build.CONSENSUS_LIB, _build.SUBMATCH_LIB):
        assert not any(hasattr(ctypes.CDLL(lib), sym) for sym in declared)
    # the consensus library is what it was: the two names its own tests pin
    assert _lib.CONSENSUS_EXPORTS == ("rp_consensus_abi_version", "rp_eight_point_consensus") and _lib.CONSENSUS_ABI_VERSION == 1
    # the same errcheck as every other launching entry point
    hooked = {n for n in _lib.FIVEPOINT_EXPORTS if getattr(typed, n).errcheck is not None}
    assert hooked == {"rp_five_point_consensus"}
    assert typed.rp_five_point_consensus.errcheck is _lib.load().rp_gemm.errcheck is _lib.load_consensus().rp_eight_point_consensus.errcheck
    assert typed.rp_fivepoint_abi_version.restype is ctypes.c_int


def test_fivepoint_build_is_a_library_of_its_own():
    from rel_pose_amd import _build
    assert os.path.basename(_build.FIVEPOINT_LIB) == "librelpose_fivepoint.so"
    libs = {_build.FIVEPOINT_LIB, _build.SUBMATCH_LIB, _build.CONSENSUS_LIB, _build.REFINE_LIB, _build.EIGHTPOINT_LIB, _build.READOUT_LIB, _build.LIB}
    dirs = {_build.FIVEPOINT_CSRC, _build.SUBMATCH_CSRC, _build.CONSENSUS_CSRC, _build.REFINE_CSRC, _build.EIGHTPOINT_CSRC, _build.READOUT_CSRC,
            _build.CSRC}
    assert len(libs) == 7 and len(dirs) == 7
    assert os.path.basename(_build.FIVEPOINT_CSRC) == "csrc_fivepoint" and _build.FIVEPOINT_SOURCES == ["five_point.hip"]
    rest = (set(_build.SOURCES) | set(_build.READOUT_SOURCES) | set(_build.EIGHTPOINT_SOURCES) | set(_build.REFINE_SOURCES)
            | set(_build.CONSENSUS_SOURCES) | set(_build.SUBMATCH_SOURCES))
    assert not set(_build.FIVEPOINT_SOURCES) & rest
    for s in _build.FIVEPOINT_SOURCES:
        assert os.path.isfile(os.path.join(ROOT, "rel_pose_amd", "csrc_fivepoint", s))
        assert not any(os.path.exists(os.path.join(d, s)) for d in dirs - {_build.FIVEPOINT_CSRC})
    assert not _build.fivepoint_needs_build() or _build.build(verbose=False) == _build.LIB
    assert not _build.fivepoint_needs_build() and not _build.submatch_needs_build() and not _build.consensus_needs_build()
    assert not _build.refine_needs_build() and not _build.eightpoint_needs_build() and not _build.readout_needs_build()
    assert not _build.needs_build()
    assert os.path.join(ROOT, "include", "relpose_fivepoint.h") in _build._fivepoint_headers()


def test_the_kernel_keeps_to_the_fixed_points_of_its_design():
    """csrc_fivepoint/ holds one file; it includes the shared headers and its own; no atomics, no allocation, no matrix instruction, no
    second definition of a shared device primitive, no loop without a bound: every `for` has a constant or an argument-bounded trip
    count and there is no `while`"""
    texts = {}
    for d in ("csrc", "csrc_readout", "csrc_eightpoint", "csrc_refine", "csrc_consensus", "csrc_submatch", "csrc_fivepoint"):
        for name in sorted(os.listdir(os.path.join(ROOT, "rel_pose_amd", d))):
            if name.endswith((".hip", ".h")):
                texts[d + "/" + name] = open(os.path.join(ROOT, "rel_pose_amd", d, name)).read()
    mine = {f: t for f, t in texts.items() if f.startswith("csrc_fivepoint/")}
    assert set(mine) == {"csrc_fivepoint/five_point.hip"}
    text = mine["csrc_fivepoint/five_point.hip"]
    for needle in ("global_load_lds_dwordx4", "__builtin_amdgcn_mfma", "mfma32(", "hipDeviceAttributeMultiprocessorCount", "void svd3x3_dev(",
                   "RP_DEV void rot(", "__shfl_xor", "atomicAdd", "atomicCAS", "atomicMax", "__hip_atomic", "hipMalloc", "RP_DEV float4 ld4(",
                   "RP_DEV float wave_sum("):
        assert needle not in text, needle
    assert not re.search(r"\bwhile\s*\(", text) and not re.search(r"\bdo\s*\{", re.sub(r"#define.*", "", text))
    assert [f for f, t in texts.items() if "void svd3x3_dev(" in t] == ["csrc/svd3x3.h"]
    assert [f for f, t in texts.items() if re.search(r"\bvoid\s+block_sum\s*\(", t)] == ["csrc/block_sum.h"]
    assert [f for f, t in texts.items() if "RP_DEV float wave_sum(" in t] == ["csrc/common.h"]
    assert [f for f, t in texts.items() if "RP_DEV float4 ld4(" in t] == ["csrc/common.h"]
    for inc in ('#include "../csrc/common.h"', '#include "../csrc/block_sum.h"', '#include "../csrc/svd3x3.h"',
                '#include "../../include/relpose_fivepoint.h"'):
        assert inc in text
    assert "svd3x3_dev(" in text and "block_sum(" in text
    # the fixed trip counts the header names are the source's and the restatement's
    assert "HALVINGS = 48, NEWTON = 4" in text and (F.HALVINGS, F.NEWTON) == (48, 4)
    assert "MIN_PIVOT = 1e-12" in text and F.MIN_PIVOT == 1e-12
    # csrc_consensus/consensus.hip is untouched by this library: it still holds its two entry points and nothing of this one
    assert "five" not in texts["csrc_consensus/consensus.hip"]


def test_argument_checks_come_before_any_launch():
    """no device is needed (or touched): the pointers are never dereferenced, the refusals precede the launch"""
    from rel_pose_amd import _lib
    lib = _lib.load_fivepoint()
    P = ctypes.c_void_p
    ok = [P(4096 * (i + 1)) for i in range(11)]                   # x1 x2 w tau | E best stat w_out hyp_E hyp_cost samples

    def call(ptrs=ok, P_=64, M=100, n=3, seed=1):
        return lib.rp_five_point_consensus(*ptrs[:4], seed, *ptrs[4:], P_, M, n, None)

    def swap(i, v):
        return ok[:i] + [v] + ok[i + 1:]
    shape = r"rel_pose_amd: rp_five_point_consensus failed: bad shape \(RP error -1\)"
    unsupported = r"rel_pose_amd: rp_five_point_consensus failed: unsupported \(RP error -4\)"
    align = r"rel_pose_amd: rp_five_point_consensus failed: misaligned pointer/stride \(RP error -2\)"
    required = (0, 1, 3, 4, 5, 6, 8, 9)                           # w, w_out and samples may be NULL
    for kw in [dict(n=0), dict(n=-1), dict(P_=4), dict(P_=0), dict(M=0), dict(M=-5)] + [dict(ptrs=swap(i, None)) for i in required]:
        with pytest.raises(RuntimeError, match=shape):
            call(**kw)
    for kw in (dict(P_=1729), dict(P_=1 << 20), dict(M=4097), dict(M=1 << 30), dict(n=1 << 28, M=4096)):
        with pytest.raises(RuntimeError, match=unsupported):
            call(**kw)
    for i, off in ((0, 4), (1, 4), (0, 2), (2, 2), (3, 1), (4, 2), (5, 3), (6, 1), (7, 2), (8, 1), (9, 2), (10, 3)):
        with pytest.raises(RuntimeError, match=align):
            call(ptrs=swap(i, P(4096 * (i + 1) + off)))
    # the order of the checks: shape, then size, then alignment
    with pytest.raises(RuntimeError, match=shape):
        call(ptrs=swap(0, P(4100)), n=0, P_=5000)
    with pytest.raises(RuntimeError, match=unsupported):
        call(ptrs=swap(0, P(4100)), P_=5000)


def test_five_point_consensus_refuses_bad_shapes_before_touching_a_device():
    from rel_pose_amd import fivepoint
    x, w = torch.zeros(3, 64, 2), torch.zeros(3, 64)
    for args, kw, match in (((x, x[:, :63]), {}, "x1 and x2"), ((x[..., :1], x[..., :1]), {}, "x1 and x2"), ((x[0], x[0]), {}, "x1 and x2"),
                            ((x, x, w[:, :5]), {}, "w must be"), ((x, x, w), dict(tau=torch.ones(2)), "tau"), ((x, x, w), dict(tau=None), "tau"),
                            ((x, x, w), dict(seed=2 ** 32), "seed"), ((x, x, w), dict(seed=-2 ** 31 - 1), "seed")):
        with pytest.raises(ValueError, match=match):
            fivepoint.five_point_consensus(*args, **kw)
    with pytest.raises(RuntimeError, match="GPU tensors"):         # well-formed, but not on a device: refused by the shared operand check
        fivepoint.five_point_consensus(x, x, w)


def test_minimal_is_checked_before_touching_a_device():
    import inspect
    from rel_pose_amd import consensus
    from rel_pose_amd.model import ViTEss
    from tests.test_host_cpu import make_args
    for f in (consensus.consensus_pose_from_matches, ViTEss.consensus_pose_from_matches):
        assert inspect.signature(f).parameters["minimal"].default == "eight"
    m = ViTEss(make_args()).eval()
    for bad in ("seven", "", None, 5):
        with pytest.raises(ValueError, match="minimal"):
            m.consensus_pose_from_matches(torch.zeros(1, 2, 3, 64, 64), torch.ones(1, 2, 4), minimal=bad)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.consensus_pose_from_matches(torch.zeros(1, 2, 3, 64, 64), torch.ones(1, 2, 4), minimal="five")


def test_demo_minimal_needs_consensus():
    import sys
    sys.path.insert(0, ROOT)
    import demo
    g = os.path.join(ROOT, "tests", "golden", "demo")
    argv = ["--img1", os.path.join(g, "matterport_1.png"), "--img2", os.path.join(g, "matterport_2.png")]
    for extra in (["--minimal", "five"], ["--eight_point", "--minimal", "five"], ["--eight_point", "--consensus", "8", "--minimal", "six"]):
        with pytest.raises(SystemExit):
            demo.main(argv + extra)


# ------------------------------------------------------------------------------------------------ the sampler
def test_sampler_vectors():
    """five draws of the consensus header's sampler: the same s, so draw k of a sample equals the eight-point sampler's draw k at K + 3"""
    for K in (5, 6, 37, 576):
        c5, c8 = F.draw5(1, 0, np.arange(50), K), C.draw(1, 0, np.arange(50), K + 3)
        assert np.array_equal(c5, c8[:, :5])
    for m in range(50):
        assert sorted(F.draw5(1, 0, [m], 5)[0].tolist()) == list(range(5))
    assert np.array_equal(F.draw5(-1, 3, np.arange(9), 100), F.draw5(2 ** 32 - 1, 3, np.arange(9), 100))
    w = np.ones((1, 80), np.float32)
    w[0, ::2] = 0
    w[0, 5] = -2.0
    w[0, 7] = np.nan
    pos, s = F.sample_rows5(w, 1, 80, 1, 300)
    assert np.array_equal(pos[0], [i for i in range(1, 80, 2) if i not in (5, 7)])
    assert np.array_equal(s[0], pos[0][F.draw5(1, 0, np.arange(300), 38)]) and set(s.ravel()) <= set(pos[0])
    assert not F.sample_rows5(w[:, :10], 1, 10, 1, 10)[1].any()        # K = 3: no samples


def test_samples_are_distinct_and_uniform():
    """20 000 draws at K = 37: five distinct indices below K every time, every index's share within 0.9 .. 1.1 of uniform (the band of
    tests/test_consensus_cpu.py); a problem's samples depend on its index in the batch, not on its neighbours"""
    c = F.draw5(1, 0, np.arange(20000), 37)
    assert c.min() >= 0 and c.max() < 37
    assert bool((np.diff(np.sort(c, -1), axis=-1) > 0).all())
    share = np.bincount(c.ravel(), minlength=37) / (20000 * 5 / 37)
    print("share of uniform: %.3f .. %.3f" % (share.min(), share.max()))
    assert 0.9 <= share.min() and share.max() <= 1.1, (share.min(), share.max())
    assert not np.array_equal(c[:100], F.draw5(1, 1, np.arange(100), 37)) and not np.array_equal(c[:100], F.draw5(2, 0, np.arange(100), 37))
    w = np.ones((3, 40))
    whole = F.sample_rows5(w, 3, 40, 7, 50)[1]
    w[1, :38] = 0                                                       # the neighbour turns degenerate
    assert np.array_equal(F.sample_rows5(w, 3, 40, 7, 50)[1][[0, 2]], whole[[0, 2]])
    assert np.array_equal(F.sample_rows5(w[2:], 1, 40, 7, 50, first=2)[1][0], whole[2])


# ------------------------------------------------------------------------------------------------ the reference
def test_the_truth_is_among_the_roots_on_exact_scenes():
    """200 exact five-point problems (fp64): the true E is a root every time (measured: median 6e-14, max 1.2e-9; 4.6 real roots on
    average, at most 10); every root is an essential matrix whose five epipolar residuals are at rounding level (measured 6e-9: the
    ill-conditioned samples); the kernel's route, restated, finds the same number of roots"""
    x1, x2, Et = R.scenes(200, 5, 3)
    r = F.five_point_ref(x1, x2)
    valid = np.arange(10)[None] < r.count[:, None]
    d = np.stack([R.up_to_sign(r.E[:, k], Et) for k in range(10)], 1)
    d = np.where(valid, d, np.inf).min(1)
    res = np.abs(np.einsum("skr,sjr->skj", F.rows(x1, x2), r.E.reshape(200, 10, 9)))
    res = np.where(valid[:, None, :], res, 0).max()
    print("truth among the roots: median %.3g max %.3g; roots mean %.2f max %d; residual %.3g" % (np.median(d), d.max(), r.count.mean(), r.count.max(), res))
    assert d.max() <= 1e-7 and np.median(d) <= 1e-12
    assert 1 <= r.count.min() and r.count.max() <= 10 and res <= 1e-7
    sv = np.linalg.svd(r.E[valid], compute_uv=False)
    assert np.abs(sv - [1, 1, 0]).max() <= 1e-12
    Ek, ck = F.five_point_kernel(x1, x2)
    dk = np.stack([R.up_to_sign(Ek[:, k], Et) for k in range(10)], 1)
    dk = np.where(np.arange(10)[None] < ck[:, None], dk, np.inf).min(1)
    print("the restatement: truth within %.3g (median %.3g), same count in %.3f" % (dk.max(), np.median(dk), (ck == r.count).mean()))
    assert np.median(dk) <= 2e-6 and (ck == r.count).mean() >= 0.97


def _row(outliers, M, first=None, seeds=range(10)):
    """(best, polished) error against the truth per scene: consensus5_ref on noisy_scene(seed, 576, outliers, 1e-3), tau 0.01, sampler
    seed 1; polished = eight_point_ref(w = the consensus weights, iters = 4).  Every scene is a batch of one, so its problem index is
    0 (first = None): that is how the table of DESIGN.md 5.6 was made -- all four of its five-point cells come out to the digit.
    first = k: the scene of seed s gets problem index s + k, as in a batch of the ten scenes."""
    best, pol = [], []
    for seed in seeds:
        x1, x2, Et, _ = R.noisy_scene(seed, 576, outliers, 1e-3)
        c = F.consensus5_ref(x1, x2, None, 0.01, 1, M, first=0 if first is None else seed + first)
        assert c.stat[0, 3] == 576 and c.best[0, 0] >= 0
        best.append(R.up_to_sign(c.E, Et)[0])
        pol.append(R.up_to_sign(R.eight_point_ref(x1, x2, c.weights, np.array([0.01]), 4)[0], Et)[0])
    return np.array(best), np.array(pol)


def test_sixty_percent_of_outliers():
    """the 60 % row of DESIGN.md 5.6: five-point consensus, M = 1024, seed 1: best <= 0.1 on 10 of 10 scenes, polished <= 0.05 on 10 of
    10 (measured: 0.034 / 0.022, the figures of the table), where consensus_ref with eight rows per hypothesis reaches 0.1 on 4 of 10.
    Recorded, not asserted: the same ten scenes as ONE batch (problem index = scene seed, other samples) give 9 of 10 -- on scene 9 a
    sample that holds two outliers has an exact root 0.561 from the truth whose robust cost, 3.4492e-4, is below the truth's 3.4553e-4
    and below that of every root near the truth (3.4524e-4 at best): the limit is moved to 60 %, the cost's margin there is 0.1 %"""
    best, pol = _row(0.6, 1024)
    print("60 %%, M = 1024: best max %.3f polished max %.3f" % (best.max(), pol.max()), np.round(best, 3), np.round(pol, 3))
    assert int((best <= 0.1).sum()) == 10, best
    assert int((pol <= 0.05).sum()) == 10, pol
    assert abs(best.max() - 0.034) < 1e-3 and abs(pol.max() - 0.022) < 1e-3           # the table's cell
    eight = []
    for seed in range(10):
        x1, x2, Et, _ = R.noisy_scene(seed, 576, 0.6, 1e-3)
        eight.append(R.up_to_sign(C.consensus_ref(x1, x2, None, 0.01, 1, 1024).E, Et)[0])
    print("eight-point consensus at 60 %:", np.round(eight, 3))
    assert int((np.array(eight) < 0.1).sum()) == 4, eight
    best, pol = _row(0.6, 1024, first=0)
    print("60 %, M = 1024, the ten scenes as one batch (recorded): best", np.round(best, 3), "polished", np.round(pol, 3))


def test_fifty_percent_with_a_quarter_of_the_samples():
    """the 50 % row at M = 256: best <= 0.1 and polished <= 0.05 on 10 of 10 (measured 0.040 / 0.010, the table's cell); the 70 % row is
    recorded, not asserted: nothing is claimed there"""
    best, pol = _row(0.5, 256)
    print("50 %%, M = 256: best max %.3f polished max %.3f" % (best.max(), pol.max()))
    assert int((best <= 0.1).sum()) == 10, best
    assert int((pol <= 0.05).sum()) == 10, pol
    assert abs(best.max() - 0.040) < 1e-3 and abs(pol.max() - 0.010) < 1e-3
    for M in (256, 1024):
        best, pol = _row(0.7, M)
        print("70 %%, M = %d (recorded): best < 0.1 in %d of 10, polished < 0.1 in %d of 10" % (M, (best < 0.1).sum(), (pol < 0.1).sum()))


def test_reference_degenerate_problems():
    x1, x2, _ = R.scenes(4, 40, seed=12)
    w = np.random.default_rng(1).uniform(0.05, 1, (4, 40))
    w[1] = 0
    w[1, [3, 5, 9, 20]] = 0.5
    w[1, 7], w[1, 8] = -1.0, np.nan
    tau = np.array([0.02, 0.02, 0.02, 0.0])
    o = F.consensus5_ref(x1, x2, w, tau, 3, 70)
    for b, K in ((1, 4), (3, 40)):
        assert not o.E[b].any() and np.array_equal(o.best[b], [-1, -1]) and np.array_equal(o.stat[b], [0, 0, 0, K])
        assert np.array_equal(o.weights[b], C.clamp(w, 4, 40)[b])
        assert not o.hyp_E[b].any() and bool((o.hyp_cost[b] == C.FLT_MAX).all())
    assert not o.samples[1].any() and o.samples[3].any()
    assert o.best[0, 0] >= 0 and 0 < o.stat[0, 1] <= 1 and abs(np.linalg.norm(o.E[0]) - np.sqrt(2)) < 1e-9


# ------------------------------------------------------------------------------------------------ the calibration of the GPU bounds
@pytest.mark.parametrize("kind", F.ROOT_CASES)
def test_restatement_is_within_the_calibrated_bounds(kind):
    """the calibration of tests/test_gpu_fivepoint.py: on its inputs the restatement of the kernel's arithmetic (five_point_kernel) stays
    within C / 8 of five_point_ref, on every root of every sample the reference admits, and the share left out is under the cap
    (measured: 5.7 % exact, 0.65 % noisy, with all three clauses)"""
    samples, a, b, ref, kept = F.root_reference(kind)
    E, count = F.five_point_kernel(a, b)
    root, res, ess = F.root_errors(E, count, a, b, ref, kept)
    left = 1 - kept.mean()
    print("%s: left out %.4f (cond %.4f, separation %.4f, near-complex %.4f); restatement root error %.4g residual %.4g singular values %.3g"
          % (kind, left, (ref.cond > F.COND_MAX).mean(), (ref.sep < F.SEP_MIN).mean(), ref.near_complex.mean(), root, res, ess))
    assert left <= F.LEFT_OUT_MAX
    assert bool((count == ref.count)[kept].all())
    assert root <= F.C_ROOT[kind] / 8 * 1.001 and res <= F.C_RES[kind] / 8 * 1.001 and ess <= F.ESSENTIAL / 8
    assert root >= F.C_ROOT[kind] / 8 * 0.9 and res >= F.C_RES[kind] / 8 * 0.9          # the constants are these figures, not looser ones
