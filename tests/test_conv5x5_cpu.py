"""The 5x5 input-gradient library (include/relpose_conv5x5.h, librelpose_conv5x5.so) as far as it goes without a GPU: the header and the
binding derived from it, the build, the fixed points of the kernel source, the argument checks that precede any launch, the dispatch
rule, and the kernel's index arithmetic (dispatch order, tap ranges, LDS image) restated in numpy."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rp_conv5x5_abi_version", "rp_conv5x5_dgrad_f32"}
SOURCE = os.path.join(ROOT, "rel_pose_amd", "csrc_conv5x5", "conv5x5_dgrad_f32.hip")


def test_conv5x5_header_parses_and_the_library_exports_it():
    from ctypes import c_int, c_void_p
    from rel_pose_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "relpose_conv5x5.h")).read()
    consts, structs, sigs, status = _lib._header_contract(text, "relpose_conv5x5.h")
    assert consts == {"RP_CONV5X5_ABI_VERSION": 1} and not structs and _lib.CONV5X5_ABI_VERSION == 1
    P, I = c_void_p, c_int
    assert list(sigs.items()) == [("rp_conv5x5_abi_version", (c_int, [])), ("rp_conv5x5_dgrad_f32", (c_int, [P, P, P, I, I, P, P]))]
    assert status == {"rp_conv5x5_dgrad_f32"} and tuple(sigs) == _lib.CONV5X5_EXPORTS == ("rp_conv5x5_abi_version", "rp_conv5x5_dgrad_f32")
    declared = set(re.findall(r"\b(rp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(sigs) == NAMES
    typed = _lib.load_conv5x5()
    raw = ctypes.CDLL(_build.CONV5X5_LIB)
    for sym in declared:
        assert hasattr(raw, sym), "missing export: " + sym
    assert typed.rp_conv5x5_abi_version() == _lib.CONV5X5_ABI_VERSION == 1
    # a tenth library, not a change of the other nine: it exports none of their names and they export none of its
    others = (set(_lib.EXPORTS) | set(_lib.READOUT_EXPORTS) | set(_lib.EIGHTPOINT_EXPORTS) | set(_lib.REFINE_EXPORTS)
              | set(_lib.CONSENSUS_EXPORTS) | set(_lib.SUBMATCH_EXPORTS) | set(_lib.FIVEPOINT_EXPORTS) | set(_lib.HOMOGRAPHY_EXPORTS)
              | set(_lib.TRIANGULATE_EXPORTS))
    assert not declared & others
    for sym in others:
        assert not hasattr(raw, sym), "librelpose_conv5x5.so exports " + sym
    for lib in (_build.LIB, _build.READOUT_LIB, _build.EIGHTPOINT_LIB, _build.REFINE_LIB, _build.CONSENSUS_LIB, _build.SUBMATCH_LIB,
                _build.FIVEPOINT_LIB, _build.HOMOGRAPHY_LIB, _build.TRIANGULATE_LIB):
        assert not any(hasattr(ctypes.CDLL(lib), sym) for sym in declared)
    # the main library's surface holds nothing of this library (112 = the 110 of then + the two stream-K grid queries)
    assert len(_lib.EXPORTS) == _lib.ABI_EXPORTS == 112 and not any("5x5" in n for n in _lib.EXPORTS)
    # the same errcheck as every other launching entry point
    assert typed.rp_conv5x5_dgrad_f32.errcheck is _lib.load().rp_gemm.errcheck and typed.rp_conv5x5_abi_version.errcheck is None


def test_conv5x5_build_is_a_library_of_its_own():
    from rel_pose_amd import _build, _lib
    _lib.load_conv5x5()
    assert os.path.basename(_build.CONV5X5_LIB) == "librelpose_conv5x5.so"
    assert os.path.basename(_build.CONV5X5_CSRC) == "csrc_conv5x5" and _build.CONV5X5_SOURCES == ["conv5x5_dgrad_f32.hip"]
    assert sorted(f for f in os.listdir(_build.CONV5X5_CSRC) if f.endswith((".hip", ".h"))) == ["conv5x5_dgrad_f32.hip"]
    assert os.path.join(ROOT, "include", "relpose_conv5x5.h") in _build._conv5x5_headers()
    assert not _build.conv5x5_needs_build()                                       # (the loader built it)
    assert "conv5x5_dgrad_f32.hip" not in _build.SOURCES


def test_the_kernel_keeps_to_the_fixed_points_of_its_design():
    """one file and the shared header; the shared LDS-DMA, LDS-read and matrix helpers and no copy of one -- nor the name of the
    instruction behind one, not even in a comment; one launcher, exact fp32 only, no atomics, no allocation, no workspace"""
    text = open(SOURCE).read()
    for needle in ("global_load_lds", "ds_read", "ds_write", "__builtin_amdgcn_mfma", "v_mfma", "buffer_load", "atomicAdd", "__hip_atomic", "hipMalloc",
                   "hipMemset", "bf16", "RP_DEV void glds16(", "lds_rd32(unsigned", "workspace_bytes"):
        assert needle not in text, needle
    for inc in ('#include "../csrc/common.h"', '#include "../../include/relpose_conv5x5.h"'):
        assert inc in text
    assert len(re.findall(r"#include", text)) == 2
    for helper in ("glds16(", "lds_rd32<", "mfma32(", "uniform_ptr(", "lds_byte_addr(", "static_for<"):
        assert helper in text, helper
    assert len(re.findall(r'extern "C"', text)) == 2 and text.count("RP_CHECK_LAUNCH();") == 1
    assert "__launch_bounds__(256, 1)" in text


def test_argument_checks_come_before_any_launch():
    """no device is needed (or touched): the pointers are never dereferenced, the refusals precede the launch"""
    from rel_pose_amd import _lib
    lib = _lib.load_conv5x5()
    V = ctypes.c_void_p
    dy, w, dx, res = (V(4096 * (i + 1)) for i in range(4))
    shape = r"rel_pose_amd: rp_conv5x5_dgrad_f32 failed: bad shape \(RP error -1\)"
    unsupported = r"rel_pose_amd: rp_conv5x5_dgrad_f32 failed: unsupported \(RP error -4\)"
    align = r"rel_pose_amd: rp_conv5x5_dgrad_f32 failed: misaligned pointer/stride \(RP error -2\)"
    for args in ((dy, w, dx, 0, 192, res), (dy, w, dx, -5, 128, None), (None, w, dx, 1, 192, None), (dy, None, dx, 1, 192, None),
                 (dy, w, None, 1, 192, res)):
        with pytest.raises(RuntimeError, match=shape):
            lib.rp_conv5x5_dgrad_f32(*args, None)
    for CI in (0, 64, 160, 256, -128):
        with pytest.raises(RuntimeError, match=unsupported):
            lib.rp_conv5x5_dgrad_f32(dy, w, dx, 2, CI, None, None)
    for i in range(4):
        for off in (4, 8, 12):
            ptrs = [dy, w, dx, res]
            ptrs[i] = V(ptrs[i].value + off)
            with pytest.raises(RuntimeError, match=align):
                lib.rp_conv5x5_dgrad_f32(ptrs[0], ptrs[1], ptrs[2], 2, 128, ptrs[3], None)
    # the order of the checks: shape, then support, then alignment
    with pytest.raises(RuntimeError, match=shape):
        lib.rp_conv5x5_dgrad_f32(V(4100), w, dx, 0, 7, None, None)
    with pytest.raises(RuntimeError, match=unsupported):
        lib.rp_conv5x5_dgrad_f32(V(4100), w, dx, 1, 7, None, None)


def test_wrapper_and_dispatch_refuse_before_touching_a_device():
    from rel_pose_amd import ops
    with pytest.raises(RuntimeError, match="GPU tensor expected"):
        ops.conv5x5_dgrad_f32(torch.zeros(1, 24, 24, 192), torch.zeros(192, 5, 5, 192))
    m = torch.nn.Conv2d(192, 192, 5)
    assert not ops.conv5x5_dgrad_f32_ok(m, torch.zeros(128, 192, 28, 28, requires_grad=True))        # (not on a device)
    assert ops.CONV5X5_DGRAD_IMAGES == 128 and 1 <= ops.CONV5X5_DGRAD_F32_MIN_N <= 128
    # no timed(...) bracket around the launch: bench.py's TAG_SYMBOLS has no entry for it
    import inspect
    assert "timed(" not in inspect.getsource(ops.conv5x5_dgrad_f32).replace("no timed(...)", "")


# ------------------------------------------------------------------------------------------------ the index arithmetic, restated
def _constants():
    text = open(SOURCE).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (\w+) = (\d+)[;,]", text)}


def tap_range(v):
    return max(0, v - 23), min(4, v)


def order():
    """make_order() of the kernel: most taps first, row-major among equals; the 400 interior pixels dealt 50 consecutive to each j % 8"""
    taps = [(tap_range(p // 28)[1] - tap_range(p // 28)[0] + 1) * (tap_range(p % 28)[1] - tap_range(p % 28)[0] + 1) for p in range(784)]
    o = [p for t in range(25, 0, -1) for p in range(784) if taps[p] == t]
    q = list(o)
    for j in range(400):
        q[j] = o[50 * (j & 7) + (j >> 3)]
    return q, taps


def test_dispatch_order_covers_every_pixel_once_heaviest_first():
    c = _constants()
    assert (c["HO"], c["HI"], c["KS"], c["IB"], c["SK"]) == (24, 28, 5, 128, 64) and "j < 400" in open(SOURCE).read()
    q, taps = order()
    assert sorted(q) == list(range(784))
    t = [taps[p] for p in q]
    assert t == sorted(t, reverse=True) and t[:400] == [25] * 400 and t[400] == 20 and t[-4:] == [1] * 4
    assert sum(taps) == 24 * 24 * 25                                 # exactly the products of the convolution: none with a padding zero
    # greedy in-order dispatch over 256 CUs, longest first: Graham's bound for it is (4/3 - 1/(3 m)) x the optimum, and the optimum is
    # at least the mean (56.25 tap-units); the busiest CU of this list carries 60
    load = np.zeros(256)
    for tp in t:
        load[load.argmin()] += tp
    print("makespan %g of mean %.2f" % (load.max(), sum(t) / 256))
    assert load.max() <= (4 / 3 - 1 / (3 * 256)) * np.ceil(sum(t) / 256)
    # the taps a workgroup walks are exactly those inside dy
    for v in range(28):
        lo, hi = tap_range(v)
        assert [r for r in range(5) if 0 <= v - r <= 23] == list(range(lo, hi + 1))


def test_activation_image_is_conflict_free_and_read_back_whole():
    """the LDS image of an activation stage: DMA lane (piece, lane) writes 16-byte slot piece * 64 + lane with chunk (lane & 15) ^ (row & 15)
    of row 4 piece + (lane >> 4); reader lane (i, hi) of step group g reads slot row * 16 + ((2 g + hi) ^ (i & 15)).  Every (row, chunk) is
    found where the reader looks, and the 16 lanes the LDS serves together (the 16-byte read's lane groups) hit 16 different bank groups."""
    slot = {}
    for piece in range(32):
        for lane in range(64):
            row = 4 * piece + (lane >> 4)
            slot[piece * 64 + lane] = (row, (lane & 15) ^ (row & 15))
    assert len(set(slot.values())) == 128 * 16
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    for base in (0, 32, 64, 96):
        for g in range(8):
            for hi in (0, 1):
                for i in range(32):
                    assert slot[(base + i) * 16 + ((2 * g + hi) ^ (i & 15))] == (base + i, 2 * g + hi)
                for grp in groups:
                    banks = {((base + i) * 16 + ((2 * g + hi) ^ (i & 15))) % 16 for i in grp}
                    assert len(banks) == 16
