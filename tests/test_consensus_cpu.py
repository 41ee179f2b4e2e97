"""The consensus eight-point (include/relpose_consensus.h, librelpose_consensus.so, rel_pose_amd/consensus.py) as far as it goes without a
GPU: the header and the binding derived from it, the build, the argument checks that precede any launch, the one-definition rule for
the shared device code, the sampler, the fp64 reference chain of tests/_consensus_ref.py on the noisy scenes, the float32 restatement
that calibrates the GPU tests' bounds, and the refusals of the host wrappers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _consensus_ref as C
from tests import _eightpoint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_consensus_header_parses_and_the_library_exports_it():
    from ctypes import c_int, c_void_p
    from rel_pose_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "relpose_consensus.h")).read()
    consts, structs, sigs, status = _lib._header_contract(text, "relpose_consensus.h")
    assert consts == {"RP_CONSENSUS_ABI_VERSION": 1, "RP_CONSENSUS_MAX_P": 1728, "RP_CONSENSUS_MAX_M": 4096} and not structs
    assert (_lib.CONSENSUS_ABI_VERSION, _lib.CONSENSUS_MAX_P, _lib.CONSENSUS_MAX_M) == (1, 1728, 4096)
    P, I = c_void_p, c_int
    assert list(sigs.items()) == [("rp_consensus_abi_version", (c_int, [])),
                                  ("rp_eight_point_consensus", (c_int, [P, P, P, P, I, P, P, P, P, P, P, P, I, I, I, P]))]
    assert status == {"rp_eight_point_consensus"} and tuple(sigs) == _lib.CONSENSUS_EXPORTS
    # the declarations as a C reader sees them (comments stripped), independently of the parser: exactly the two names
    declared = set(re.findall(r"\b(rp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(sigs) == {"rp_consensus_abi_version", "rp_eight_point_consensus"}
    typed = _lib.load_consensus()
    raw = ctypes.CDLL(_build.CONSENSUS_LIB)
    for sym in declared:
        assert hasattr(raw, sym), "missing export: " + sym
    assert typed.rp_consensus_abi_version() == _lib.CONSENSUS_ABI_VERSION
    # a fifth library, not a change of the other four: it exports none of their names and their headers declare none of its
    others = set(_lib.EXPORTS) | set(_lib.READOUT_EXPORTS) | set(_lib.EIGHTPOINT_EXPORTS) | set(_lib.REFINE_EXPORTS)
    assert not declared & others
    for sym in others:
        assert not hasattr(raw, sym), "librelpose_consensus.so exports " + sym
    for h in ("relpose_hip.h", "relpose_readout.h", "relpose_eightpoint.h", "relpose_refine.h"):
        assert "consensus" not in open(os.path.join(ROOT, "include", h)).read()
    for lib in (_build.LIB, _build.READOUT_LIB, _build.EIGHTPOINT_LIB, _build.REFINE_LIB):
        assert not any(hasattr(ctypes.CDLL(lib), sym) for sym in declared)
    # the same errcheck as every other launching entry point
    hooked = {n for n in _lib.CONSENSUS_EXPORTS if getattr(typed, n).errcheck is not None}
    assert hooked == {"rp_eight_point_consensus"}
    assert typed.rp_eight_point_consensus.errcheck is _lib.load().rp_gemm.errcheck is _lib.load_refine().rp_refine_pose.errcheck
    assert typed.rp_consensus_abi_version.restype is ctypes.c_int


def test_consensus_build_is_a_library_of_its_own():
    from rel_pose_amd import _build
    assert os.path.basename(_build.CONSENSUS_LIB) == "librelpose_consensus.so"
    assert len({_build.CONSENSUS_LIB, _build.REFINE_LIB, _build.EIGHTPOINT_LIB, _build.READOUT_LIB, _build.LIB}) == 5
    assert len({_build.CONSENSUS_CSRC, _build.REFINE_CSRC, _build.EIGHTPOINT_CSRC, _build.READOUT_CSRC, _build.CSRC}) == 5
    assert os.path.basename(_build.CONSENSUS_CSRC) == "csrc_consensus" and _build.CONSENSUS_SOURCES == ["consensus.hip"]
    rest = set(_build.SOURCES) | set(_build.READOUT_SOURCES) | set(_build.EIGHTPOINT_SOURCES) | set(_build.REFINE_SOURCES)
    assert not set(_build.CONSENSUS_SOURCES) & rest
    for s in _build.CONSENSUS_SOURCES:
        assert os.path.isfile(os.path.join(ROOT, "rel_pose_amd", "csrc_consensus", s))
        assert not any(os.path.exists(os.path.join(d, s)) for d in (_build.CSRC, _build.READOUT_CSRC, _build.EIGHTPOINT_CSRC, _build.REFINE_CSRC))
    assert not _build.consensus_needs_build() or _build.build(verbose=False) == _build.LIB
    assert not _build.consensus_needs_build() and not _build.refine_needs_build() and not _build.eightpoint_needs_build()
    assert not _build.readout_needs_build() and not _build.needs_build()
    assert os.path.join(ROOT, "include", "relpose_consensus.h") in _build._consensus_headers()


def test_argument_checks_come_before_any_launch():
    """no device is needed (or touched): the pointers are never dereferenced, the refusals precede the launch"""
    from rel_pose_amd import _lib
    lib = _lib.load_consensus()
    P = ctypes.c_void_p
    ok = [P(4096 * (i + 1)) for i in range(11)]                   # x1 x2 w tau | E best stat w_out hyp_E hyp_cost samples

    def call(ptrs=ok, P_=64, M=100, n=3, seed=1):
        return lib.rp_eight_point_consensus(*ptrs[:4], seed, *ptrs[4:], P_, M, n, None)

    def swap(i, v):
        return ok[:i] + [v] + ok[i + 1:]
    shape = r"rel_pose_amd: rp_eight_point_consensus failed: bad shape \(RP error -1\)"
    unsupported = r"rel_pose_amd: rp_eight_point_consensus failed: unsupported \(RP error -4\)"
    align = r"rel_pose_amd: rp_eight_point_consensus failed: misaligned pointer/stride \(RP error -2\)"
    required = (0, 1, 3, 4, 5, 6, 8, 9)                           # w, w_out and samples may be NULL
    for kw in [dict(n=0), dict(n=-1), dict(P_=7), dict(P_=0), dict(M=0), dict(M=-5)] + [dict(ptrs=swap(i, None)) for i in required]:
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


def test_the_new_directory_brings_no_copy_of_a_shared_device_primitive():
    """csrc_consensus/ holds one file, which includes csrc/common.h, csrc/block_sum.h and csrc/svd3x3.h: svd3x3_dev, rot, block_sum and
    wave_sum keep their one definition across the five source directories"""
    texts = {}
    for d in ("csrc", "csrc_readout", "csrc_eightpoint", "csrc_refine", "csrc_consensus"):
        for name in sorted(os.listdir(os.path.join(ROOT, "rel_pose_amd", d))):
            if name.endswith((".hip", ".h")):
                texts[d + "/" + name] = open(os.path.join(ROOT, "rel_pose_amd", d, name)).read()
    mine = {f: t for f, t in texts.items() if f.startswith("csrc_consensus/")}
    assert set(mine) == {"csrc_consensus/consensus.hip"}
    text = mine["csrc_consensus/consensus.hip"]
    for needle in ("global_load_lds_dwordx4", "__builtin_amdgcn_mfma", "hipDeviceAttributeMultiprocessorCount", "void svd3x3_dev(",
                   "RP_DEV void rot(", "__shfl_xor", "atomicAdd", "atomicCAS", "__hip_atomic", "hipMalloc"):
        assert needle not in text, needle
    assert [f for f, t in texts.items() if "void svd3x3_dev(" in t] == ["csrc/svd3x3.h"]
    assert [f for f, t in texts.items() if re.search(r"\bvoid\s+block_sum\s*\(", t)] == ["csrc/block_sum.h"]
    assert [f for f, t in texts.items() if "RP_DEV float wave_sum(" in t] == ["csrc/common.h"]
    for inc in ('#include "../csrc/common.h"', '#include "../csrc/block_sum.h"', '#include "../csrc/svd3x3.h"',
                '#include "../../include/relpose_consensus.h"'):
        assert inc in text
    assert "svd3x3_dev(" in text and "block_sum(" in text


# ------------------------------------------------------------------------------------------------ the sampler
def test_sampler_vectors():
    assert C.draw(1, 0, [0, 1], 576).tolist() == [[329, 443, 239, 44, 566, 20, 128, 411], [153, 324, 232, 184, 407, 388, 45, 212]]
    for m in range(50):
        assert sorted(C.draw(1, 0, [m], 8)[0].tolist()) == list(range(8))
    # a negative seed is its 32-bit pattern
    assert np.array_equal(C.draw(-1, 3, np.arange(9), 100), C.draw(2 ** 32 - 1, 3, np.arange(9), 100))
    # the rows are pos[c]: with every second weight 0 only the others are drawn
    w = np.ones((1, 80), np.float32)
    w[0, ::2] = 0
    w[0, 5] = -2.0
    w[0, 7] = np.nan
    pos, s = C.sample_rows(w, 1, 80, 1, 300)
    assert np.array_equal(pos[0], [i for i in range(1, 80, 2) if i not in (5, 7)])
    assert np.array_equal(s[0], pos[0][C.draw(1, 0, np.arange(300), 38)]) and set(s.ravel()) <= set(pos[0])
    assert not C.sample_rows(w[:, :14], 1, 14, 1, 10)[1].any()        # K = 5: no samples


def test_samples_are_distinct_and_uniform():
    """20 000 draws at K = 37: eight distinct indices below K every time, every index's share within 0.9 .. 1.1 of uniform (measured
    0.967 .. 1.036)"""
    c = C.draw(1, 0, np.arange(20000), 37)
    assert c.min() >= 0 and c.max() < 37
    assert bool((np.diff(np.sort(c, -1), axis=-1) > 0).all())
    share = np.bincount(c.ravel(), minlength=37) / (20000 * 8 / 37)
    assert 0.9 <= share.min() and share.max() <= 1.1, (share.min(), share.max())
    # other problems and other seeds draw other samples
    assert not np.array_equal(c[:100], C.draw(1, 1, np.arange(100), 37)) and not np.array_equal(c[:100], C.draw(2, 0, np.arange(100), 37))


# ------------------------------------------------------------------------------------------------ the reference chain
@pytest.mark.parametrize("outliers", [0.3, 0.5])
def test_reference_chain_on_the_noisy_scenes(outliers):
    """noisy_scene(seed, 576, outliers, 1e-3), seeds 0 .. 9, M = 1024, seed 1, problem index = scene seed, tau = 0.01: the best
    hypothesis within 0.25 of the true E and the chain best -> eight_point_ref(w = its Cauchy weights, iters = 4) within 0.1 in 10 of
    10 scenes, plain eight_point_ref(iters = 4) off by at least 0.4 in at least 8 (measured: best <= 0.038 / 0.165, chain <= 0.016 /
    0.054, plain wrong in 8 / 10 scenes at 30 % / 50 %)"""
    tau = np.array([0.01])
    best, chain, plain = [], [], []
    for seed in range(10):
        x1, x2, Et, _ = R.noisy_scene(seed, 576, outliers, 1e-3)
        c = C.consensus_ref(x1, x2, None, 0.01, 1, 1024, first=seed)
        assert c.stat[0, 2] == 1024 and c.stat[0, 3] == 576 and c.best[0] == int(np.argmin(c.hyp_cost[0]))
        best.append(R.up_to_sign(c.E, Et)[0])
        chain.append(R.up_to_sign(R.eight_point_ref(x1, x2, c.weights, tau, 4)[0], Et)[0])
        plain.append(R.up_to_sign(R.eight_point_ref(x1, x2, None, tau, 4)[0], Et)[0])
    best, chain, plain = np.array(best), np.array(chain), np.array(plain)
    print(outliers, "best %.3f chain %.3f plain" % (best.max(), chain.max()), np.round(plain, 2))
    assert int((best <= 0.25).sum()) == 10, best
    assert int((chain <= 0.1).sum()) == 10, chain
    assert int((plain >= 0.4).sum()) >= 8, plain


def test_reference_degenerate_problems():
    x1, x2, _ = R.scenes(4, 40, seed=12)
    w = np.random.default_rng(1).uniform(0.05, 1, (4, 40))
    w[1] = 0
    w[1, [3, 5, 9, 20, 30, 38, 39]] = 0.5
    w[1, 7], w[1, 8] = -1.0, np.nan
    x1[2] = x1[2, 17]
    tau = np.array([0.02, 0.02, 0.02, 0.0])
    for f in (C.consensus_ref, C.consensus_f32):
        o = f(x1, x2, w, tau, 3, 70)
        for b, K in ((1, 7), (2, 40), (3, 40)):
            assert not o.E[b].any() and o.best[b] == -1 and np.array_equal(o.stat[b], [0, 0, 0, K])
            assert np.array_equal(o.weights[b], C.clamp(w, 4, 40)[b].astype(o.weights.dtype))
            assert not o.hyp_E[b].any() and bool((o.hyp_cost[b] == C.FLT_MAX).all())
        assert not o.samples[1].any() and o.samples[2].any() and o.samples[3].any()
        assert o.best[0] >= 0 and o.stat[0, 2] == 70 and 0 < o.stat[0, 1] <= 1 and abs(np.linalg.norm(o.E[0]) - np.sqrt(2)) < 1e-5


def test_float32_restatement_is_within_the_calibrated_bounds():
    """the calibration of the GPU tests' bounds: consensus_f32 stays within C / 8 of consensus_ref on the inputs of
    tests/test_gpu_consensus.py, every hypothesis and every case, and picks a winner within the cost bound of the reference's"""
    worst = dict(exact=0.0, noisy=0.0, E_gain=0.0, cost=0.0, w=0.0, shift=0.0)
    for case in C.CASES:
        kind, n, P, M, weighted = case
        x1, x2, w, _ = C.inputs(*case)
        ref = C.reference(*case)
        f32 = C.consensus_f32(x1, x2, w, C.TAU, C.SEED, M)
        assert np.array_equal(f32.samples, ref.samples) and np.array_equal(f32.stat[:, 2:], ref.stat[:, 2:])
        r = C.ratios(f32, ref, x1, x2, w)
        print(case, {k: v for k, v in r.items() if k != "near"})
        assert r["compared"] >= 0.95 and r["compared_gain"] >= 0.95
        for k in ("E_gain", "cost", "w", "shift"):
            worst[k] = max(worst[k], r[k])
        worst[kind] = max(worst[kind], r["E"])
        # the restatement's winner against the reference's, by the bound the GPU test uses
        pick = np.arange(n)
        wc, t = C.clamp(w, n, P), np.full(n, C.TAU)
        c_k = C.cost64(f32.E, x1.astype(np.float64), x2.astype(np.float64), wc, t)
        c_kr = C.cost64(f32.hyp_E[pick, ref.best], x1.astype(np.float64), x2.astype(np.float64), wc, t)
        D1 = C.shift_scale(ref, x1, x2, wc, r["near"])
        assert bool(r["near"][pick, ref.best].all())
        upper = ref.hyp_cost[pick, ref.best] + C.C_SHIFT * D1[pick, ref.best] + C.cost_bound(c_k) + C.cost_bound(c_kr)
        assert bool((c_k <= upper).all()), (case, c_k, upper)
    print("largest ratios of the restatement:", worst)
    assert worst["exact"] <= C.C_E["exact"] / 8 and worst["noisy"] <= C.C_E["noisy"] / 8, worst
    assert worst["E_gain"] <= C.C_E_GAIN / 8, worst
    assert worst["cost"] <= C.C_COST / 8 and worst["w"] <= C.C_W / 8 and worst["shift"] <= C.C_SHIFT / 8, worst


# ------------------------------------------------------------------------------------------------ the host wrappers
def test_eight_point_consensus_refuses_bad_shapes_before_touching_a_device():
    from rel_pose_amd import consensus
    x, w = torch.zeros(3, 64, 2), torch.zeros(3, 64)
    for args, kw, match in (((x, x[:, :63]), {}, "x1 and x2"), ((x[..., :1], x[..., :1]), {}, "x1 and x2"), ((x[0], x[0]), {}, "x1 and x2"),
                            ((x, x, w[:, :5]), {}, "w must be"), ((x, x, w), dict(tau=torch.ones(2)), "tau"), ((x, x, w), dict(tau=None), "tau"),
                            ((x, x, w), dict(seed=2 ** 32), "seed"), ((x, x, w), dict(seed=-2 ** 31 - 1), "seed")):
        with pytest.raises(ValueError, match=match):
            consensus.eight_point_consensus(*args, **kw)
    with pytest.raises(RuntimeError, match="GPU tensors"):         # well-formed, but not on a device: refused by the shared operand check
        consensus.eight_point_consensus(x, x, w)


def test_consensus_pose_from_matches_refuses_training_mode_before_touching_a_device():
    from rel_pose_amd.model import ViTEss
    from tests.test_host_cpu import make_args
    intr = torch.ones(1, 2, 4)
    m = ViTEss(make_args())
    assert m.training
    with pytest.raises(RuntimeError, match="eval"):
        m.consensus_pose_from_matches(torch.zeros(1, 2, 3, 64, 64), intr)
    assert torch.equal(intr, torch.ones(1, 2, 4))
