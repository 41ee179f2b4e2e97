"""The sub-token match localisation (include/relpose_submatch.h, librelpose_submatch.so, rel_pose_amd/readout.py) as far as it goes without a
GPU: the header and the binding derived from it, the build, the argument checks that precede any launch, the fp64 reference of
tests/_submatch_ref.py on the built scenes -- what localisation buys the classical chain, and that the vertex of a Gaussian peak is its
centre --, the float32 restatement that calibrates the GPU tests' constants, and the refusals of the host wrappers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _submatch_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_submatch_header_parses_and_the_library_exports_it():
    from ctypes import c_float, c_int, c_void_p
    from rel_pose_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "relpose_submatch.h")).read()
    consts, structs, sigs, status = _lib._header_contract(text, "relpose_submatch.h")
    assert consts == {"RP_SUBMATCH_ABI_VERSION": 1} and not structs
    assert _lib.SUBMATCH_ABI_VERSION == 1
    P, I, F = c_void_p, c_int, c_float
    assert list(sigs.items()) == [("rp_submatch_abi_version", (c_int, [])),
                                  ("rp_emm_submatch", (c_int, [P, P, P, P, P, P, P, I, I, I, I, F, I, I, I, P]))]
    assert status == {"rp_emm_submatch"} and tuple(sigs) == _lib.SUBMATCH_EXPORTS
    # the declarations as a C reader sees them (comments stripped), independently of the parser: exactly the two names
    declared = set(re.findall(r"\b(rp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(sigs) == {"rp_submatch_abi_version", "rp_emm_submatch"}
    typed = _lib.load_submatch()
    raw = ctypes.CDLL(_build.SUBMATCH_LIB)
    for sym in declared:
        assert hasattr(raw, sym), "missing export: " + sym
    assert typed.rp_submatch_abi_version() == _lib.SUBMATCH_ABI_VERSION
    # a sixth library, not a change of the other five: it exports none of their names and their headers declare none of its
    others = (set(_lib.EXPORTS) | set(_lib.READOUT_EXPORTS) | set(_lib.EIGHTPOINT_EXPORTS) | set(_lib.REFINE_EXPORTS)
              | set(_lib.CONSENSUS_EXPORTS))
    assert not declared & others
    for sym in others:
        assert not hasattr(raw, sym), "librelpose_submatch.so exports " + sym
    for h in ("relpose_hip.h", "relpose_readout.h", "relpose_eightpoint.h", "relpose_refine.h", "relpose_consensus.h"):
        assert "submatch" not in open(os.path.join(ROOT, "include", h)).read()
    for lib in (_build.LIB, _build.READOUT_LIB, _build.EIGHTPOINT_LIB, _build.REFINE_LIB, _build.CONSENSUS_LIB):
        assert not any(hasattr(ctypes.CDLL(lib), sym) for sym in declared)
    # the same errcheck as every other launching entry point
    hooked = {n for n in _lib.SUBMATCH_EXPORTS if getattr(typed, n).errcheck is not None}
    assert hooked == {"rp_emm_submatch"}
    assert typed.rp_emm_submatch.errcheck is _lib.load().rp_gemm.errcheck is _lib.load_readout().rp_emm_matches.errcheck
    assert typed.rp_submatch_abi_version.restype is ctypes.c_int


def test_submatch_build_is_a_library_of_its_own():
    from rel_pose_amd import _build
    assert os.path.basename(_build.SUBMATCH_LIB) == "librelpose_submatch.so"
    libs = {_build.SUBMATCH_LIB, _build.CONSENSUS_LIB, _build.REFINE_LIB, _build.EIGHTPOINT_LIB, _build.READOUT_LIB, _build.LIB}
    dirs = {_build.SUBMATCH_CSRC, _build.CONSENSUS_CSRC, _build.REFINE_CSRC, _build.EIGHTPOINT_CSRC, _build.READOUT_CSRC, _build.CSRC}
    assert len(libs) == 6 and len(dirs) == 6
    assert os.path.basename(_build.SUBMATCH_CSRC) == "csrc_submatch" and _build.SUBMATCH_SOURCES == ["submatch.hip"]
    rest = (set(_build.SOURCES) | set(_build.READOUT_SOURCES) | set(_build.EIGHTPOINT_SOURCES) | set(_build.REFINE_SOURCES)
            | set(_build.CONSENSUS_SOURCES))
    assert not set(_build.SUBMATCH_SOURCES) & rest
    for s in _build.SUBMATCH_SOURCES:
        assert os.path.isfile(os.path.join(ROOT, "rel_pose_amd", "csrc_submatch", s))
        assert not any(os.path.exists(os.path.join(d, s)) for d in dirs - {_build.SUBMATCH_CSRC})
    assert not _build.submatch_needs_build() or _build.build(verbose=False) == _build.LIB
    assert not _build.submatch_needs_build() and not _build.consensus_needs_build() and not _build.refine_needs_build()
    assert not _build.eightpoint_needs_build() and not _build.readout_needs_build() and not _build.needs_build()
    assert os.path.join(ROOT, "include", "relpose_submatch.h") in _build._submatch_headers()


def test_the_kernel_keeps_to_the_fixed_points_of_its_design():
    """no atomics, no allocation, no matrix instruction, no second definition of a shared device primitive: csrc_submatch/ holds one file,
    which includes csrc/common.h"""
    names = sorted(os.listdir(os.path.join(ROOT, "rel_pose_amd", "csrc_submatch")))
    assert [n for n in names if n.endswith((".hip", ".h"))] == ["submatch.hip"]
    text = open(os.path.join(ROOT, "rel_pose_amd", "csrc_submatch", "submatch.hip")).read()
    for needle in ("atomicAdd", "atomicCAS", "atomicMax", "__hip_atomic", "hipMalloc", "__builtin_amdgcn_mfma", "mfma32(", "RP_DEV float wave_sum(",
                   "RP_DEV float4 ld4(", "bool xcd_problem("):
        assert needle not in text, needle
    for inc in ('#include "../csrc/common.h"', '#include "../../include/relpose_submatch.h"'):
        assert inc in text


def test_argument_checks_come_before_any_launch():
    """no device is needed (or touched): the pointers are never dereferenced, the refusals precede the launch"""
    from rel_pose_amd import _lib
    lib = _lib.load_submatch()
    P = ctypes.c_void_p
    ok = [P(4096 * (i + 1)) for i in range(7)]                    # q k rlse clse idx | win quad

    def call(ptrs=ok, Z=2, H=3, ldq=576, ldk=576, single=0, radius=2, swap=0):
        return lib.rp_emm_submatch(*ptrs, Z, H, ldq, ldk, 0.125, swap, single, radius, None)

    def put(i, v):
        return ok[:i] + [v] + ok[i + 1:]
    shape = r"rel_pose_amd: rp_emm_submatch failed: bad shape \(RP error -1\)"
    unsupported = r"rel_pose_amd: rp_emm_submatch failed: unsupported \(RP error -4\)"
    align = r"rel_pose_amd: rp_emm_submatch failed: misaligned pointer/stride \(RP error -2\)"
    # the checks of rp_emm_matches, and idx / win / quad required; clse only with the dual softmax
    for kw in [dict(Z=0), dict(Z=-2), dict(Z=3), dict(H=0), dict(H=-1), dict(ldq=191), dict(ldk=188), dict(H=4, ldq=252)] + \
              [dict(ptrs=put(i, None)) for i in (0, 1, 2, 3, 4, 5, 6)] + [dict(ptrs=put(4, None), single=1)]:
        with pytest.raises(RuntimeError, match=shape):
            call(**kw)
    for kw in (dict(radius=0), dict(radius=3), dict(radius=-1), dict(radius=1 << 20), dict(Z=1 << 30, H=1, ldq=64, ldk=64)):
        with pytest.raises(RuntimeError, match=unsupported):
            call(**kw)
    for kw in [dict(ldq=578), dict(ldk=577)] + [dict(ptrs=put(i, P(4096 * (i + 1) + off))) for i, off in
                                                ((0, 4), (1, 8), (2, 4), (3, 12), (4, 2), (4, 1), (5, 4), (5, 8), (6, 4), (6, 12))]:
        with pytest.raises(RuntimeError, match=align):
            call(**kw)
    # the order of the checks: shape, then what is unsupported, then alignment
    with pytest.raises(RuntimeError, match=shape):
        call(ptrs=put(0, P(4100)), Z=3, radius=5)
    with pytest.raises(RuntimeError, match=unsupported):
        call(ptrs=put(0, P(4100)), radius=5)


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_on_hand_made_windows():
    """one peak whose exponents are known in closed form: e = -g ((x - px)^2 + (y - py)^2) + const on the whole grid"""
    g, px, py = 0.4, 7.3, 0.2                                       # the peak sits on the top border row
    tok = np.arange(S.TOK)
    c = np.stack([tok % S.GRID, tok // S.GRID], -1).astype(np.float64)
    e = -g * ((c[:, 0] - px) ** 2 + (c[:, 1] - py) ** 2)
    # q = e_0 for every row, k_j = (e_j / scale, 0 ...): S[i][j] = e_j; single softmax with rlse = 0 makes the exponent e_j itself
    q, k = np.zeros((2, S.TOK, 1, S.HD)), np.zeros((2, S.TOK, 1, S.HD))
    q[..., 0], k[:, :, 0, 0] = 1.0, e / S.SCALE
    rlse = np.zeros((2, 1, S.TOK))
    idx = np.full((2, 1, S.TOK), 7, np.int32)
    idx[0, 0, :4] = [-1, 576, S.INT_MIN, 0]
    r = S.submatch_ref(q, k, rlse, None, idx, single=True, radius=2)
    win, quad = r.win[1, 0, 0], r.quad[1, 0, 0]
    live = (np.abs(c[:, 0] - 7) <= 2) & (c[:, 1] <= 2)             # 5 x 3: the window is clipped at the border
    u = np.exp(e[live])
    assert np.allclose(win, [(u * c[live, 0]).sum() / u.sum(), (u * c[live, 1]).sum() / u.sum(), u.sum(),
                             (u * ((c[live, 0] - win[0]) ** 2 + (c[live, 1] - win[1]) ** 2)).sum() / u.sum()], rtol=1e-12, atol=0)
    assert np.allclose(quad, [px, 0.0, 2 * g, 0.0], rtol=1e-12, atol=1e-12)          # x: the vertex; y: a neighbour is missing
    assert np.array_equal(r.win[0, 0, :3], [S.FLAG] * 3) and np.array_equal(r.quad[0, 0, :3], [S.FLAG] * 3)
    # the corner: both axes lack a neighbour; the centre is far from the peak, so the clamp would be active were there a vertex
    assert np.array_equal(r.quad[0, 0, 3], [0, 0, 0, 0]) and 0 < r.win[0, 0, 3, 0] <= 2 and 0 < r.win[0, 0, 3, 1] <= 2
    f = S.submatch_f32(q, k, rlse, None, idx, single=True, radius=2)
    assert np.array_equal(f.win[0, 0, :3], np.float32([S.FLAG] * 3)) and np.allclose(f.win[1, 0, 0], win, rtol=1e-5)


@pytest.fixture(scope="module")
def chains():
    """the ten built scenes, dual softmax, fp64: (rotation, translation-direction) errors in degrees of the chain with x2 taken from the token
    centre (tau half a token) and from win at radius 2 (tau a twentieth of a token), and the position errors in tokens"""
    out = {"centre": [], "window": []}
    pos = {"centre": [], "window": []}
    for s in range(10):
        b = S.built_inputs(s)
        rlse, clse = S.stats64(b.q, b.k)
        idx = S.argmax_idx(b.q, b.k, rlse, clse)
        r = S.submatch_ref(b.q, b.k, rlse, clse, idx, radius=2)
        for name, p, tau in (("centre", S.centres_of(idx[1, 0]), 0.5), ("window", r.win[1, 0, :, :2], 0.05)):
            out[name].append(S.chain_errors(b, p, tau))
            pos[name].append(np.median(np.linalg.norm(p - b.p, axis=-1)[b.inside]))
    return {k: np.array(v) for k, v in out.items()}, {k: float(np.median(v)) for k, v in pos.items()}


def test_localisation_halves_the_errors_of_the_reference_chain(chains):
    """eight_point_ref(iters = 4) -> decode_pose -> refine_ref(iters = 10) on the ten built scenes (seeds 4000 .. 4009, g = 0.5, dual
    softmax): with x2 from win at radius 2 the median rotation error and the median translation-direction error are each at most HALF
    of the token-centre chain's.  Measured: rotation 0.206 against 1.010 degrees, translation direction 0.496 against 1.267 degrees;
    median position error 0.082 against 0.401 tokens."""
    err, pos = chains
    med = {k: np.median(v, 0) for k, v in err.items()}
    print("median (rotation, translation) errors:", med, "max:", {k: v.max(0) for k, v in err.items()}, "position:", pos)
    assert med["window"][0] <= 0.5 * med["centre"][0], med
    assert med["window"][1] <= 0.5 * med["centre"][1], med
    assert pos["window"] <= 0.5 * pos["centre"], pos


def test_vertex_of_a_gaussian_peak_is_its_centre():
    """single softmax, fp64 inputs: the exponent along either axis is an exact parabola about p, so quad = p to 1e-9 for every interior
    owner -- the partner inside image 1 and the argmax token off the border; there |p - centre| <= 0.5 and the curvature is 2 g"""
    for s in (0, 1):
        b = S.built_inputs(s, dtype=np.float64)
        rlse, clse = S.stats64(b.q, b.k)
        idx = S.argmax_idx(b.q, b.k, rlse.astype(np.float64), None, single=True)
        r = S.submatch_ref(b.q, b.k, rlse.astype(np.float64), None, idx, single=True, radius=1)
        interior = b.inside & r.both_x[1, 0] & r.both_y[1, 0]
        assert int(interior.sum()) > 300
        assert float(np.abs(S.centres_of(idx[1, 0]) - b.p)[interior].max()) <= 0.5 + 1e-9
        assert float(np.abs(r.quad[1, 0, :, :2] - b.p)[interior].max()) <= 1e-9
        assert float(np.abs(r.quad[1, 0, :, 2:] - 2 * b.g)[interior].max()) <= 1e-9


def test_float32_restatement_is_within_the_calibrated_constants():
    """the calibration of the GPU tests' constants: over the cases of tests/test_gpu_submatch.py submatch_f32 stays within C / 8 of
    submatch_ref for every bound, all owners compared, nothing non-finite"""
    worst = dict(wxy=0.0, wmass=0.0, wvar=0.0, curv=0.0, pxy=0.0)
    for case in S.CASES:
        kind, H, swap, single, radius, src = case
        q, k, rlse, clse = S.case_inputs(kind, H)
        idx = S.case_idx(case, q, k, rlse, clse)
        ref = S.submatch_ref(q, k, rlse, clse, idx, S.SCALE, swap, single, radius)
        f32 = S.submatch_f32(q, k, rlse, clse, idx, S.SCALE, swap, single, radius)
        assert np.isfinite(f32.win).all() and np.isfinite(f32.quad).all() and f32.win.dtype == np.float32
        r = S.bound_ratios(f32[:2], ref, radius, built=kind == "built" and not swap)
        assert r["compared"] >= 0.99, (case, r)
        if src == "table":
            assert int((~ref.valid).sum()) == 5
        for n in worst:
            worst[n] = max(worst[n], r[n])
    print("largest ratios of the restatement:", worst)
    assert worst["wxy"] <= S.C_WXY / 8 and worst["wmass"] <= S.C_WMASS / 8 and worst["wvar"] <= S.C_WVAR / 8, worst
    assert worst["curv"] <= S.C_CURV / 8 and worst["pxy"] <= S.C_PXY / 8, worst
    # and the constants are those 8 x ratios, not more (rounded up in the second digit)
    assert S.C_WXY <= 8.2 * worst["wxy"] and S.C_WMASS <= 8.2 * worst["wmass"] and S.C_WVAR <= 8.2 * worst["wvar"], worst
    assert S.C_CURV <= 8.2 * worst["curv"] and S.C_PXY <= 8.2 * worst["pxy"], worst


def test_curvature_of_the_built_inputs_is_what_the_bound_assumes():
    """on the built inputs (swap = 0) the reference's curvature is 2 g with the single softmax -- the exponent is -g |p - c|^2 -- and
    within a factor 2 of 4 g with the dual softmax (2 S and the column normaliser's own curvature), for every owner with both neighbours"""
    q, k, rlse, clse = S.case_inputs("built", 1)
    g = 0.5
    for single in (0, 1):
        idx = S.argmax_idx(q, k, rlse, clse, S.SCALE, 0, single)
        r = S.submatch_ref(q, k, rlse, clse, idx, S.SCALE, 0, single, 2)
        c = np.concatenate([r.quad[..., 2][r.both_x], r.quad[..., 3][r.both_y]])
        if single:
            assert float(np.abs(c - 2 * g).max()) <= 4 * float(r.delta_e.max()), (c.min(), c.max())
        else:
            assert 2 * g <= c.min() and c.max() <= 8 * g, (c.min(), c.max())


# ------------------------------------------------------------------------------------------------ the host wrappers
def test_subtoken_xy_and_assemble_matches_on_the_cpu():
    from rel_pose_amd import eightpoint, readout
    hw = (240, 384)
    tok = torch.arange(576)
    grid = torch.stack([tok % 24, tok // 24], -1).float()
    assert torch.equal(readout.subtoken_xy(grid, hw), readout.token_centres(hw))
    assert torch.equal(readout.subtoken_xy(torch.tensor([[0.5, -0.5, 7.0, 9.0]]), hw), torch.tensor([[16.0, 0.0]]))
    # sub = None is what the function was; with sub whose positions are the centres of row_idx it gives the same x2
    B = 2
    gen = torch.Generator().manual_seed(3)
    row_idx = torch.randint(0, 576, (2 * B, 3, 576), generator=gen, dtype=torch.int32)
    stat = torch.rand(2 * B, 3, 576, 4, generator=gen)
    mut = torch.rand(2 * B, 3, 576, generator=gen) > 0.5
    corr = readout.Correspondences(row_idx, stat, row_idx, stat, mut, None)
    intr = torch.tensor([[300.0, 280.0, 190.0, 120.0], [310.0, 290.0, 180.0, 130.0]]).repeat(B, 1, 1)
    x1, x2, w = eightpoint.assemble_matches(corr, intr, hw)
    pos = torch.cat([grid[row_idx.long()], torch.zeros(2 * B, 3, 576, 2)], -1)
    moved = pos + torch.tensor([0.25, -0.125, 0, 0])
    sub = readout.SubtokenCorrespondences(corr, pos, moved, pos, moved)
    y1, y2, v = eightpoint.assemble_matches(corr, intr, hw, sub=sub, subtoken="window")
    assert torch.equal(y1, x1) and torch.equal(v, w) and torch.allclose(y2, x2, rtol=0, atol=1e-6)
    z1, z2, u = eightpoint.assemble_matches(corr, intr, hw, heads=(2, 0), sub=sub, subtoken="quadratic")
    a1, a2, _ = eightpoint.assemble_matches(corr, intr, hw, heads=(2, 0))
    shift = torch.tensor([0.25 * 16 / 310.0, -0.125 * 10 / 290.0])
    assert torch.equal(z1, a1) and torch.allclose(z2, a2 + shift, rtol=0, atol=1e-6)
    with pytest.raises(ValueError, match="subtoken"):
        eightpoint.assemble_matches(corr, intr, hw, sub=sub, subtoken="cubic")
    assert "smaller tau" in eightpoint.default_tau.__doc__


def test_wrappers_refuse_before_touching_a_device():
    from rel_pose_amd import readout
    from rel_pose_amd.model import ViTEss
    from tests.test_host_cpu import make_args
    qkv, lse = torch.zeros(2 * 576, 576), torch.zeros(2, 3, 576)
    for bad in (torch.zeros(2, 3, 576, dtype=torch.int64), torch.zeros(2, 3, 575, dtype=torch.int32)):
        with pytest.raises(ValueError, match="idx must be"):
            readout.emm_submatch(qkv, lse, lse, bad, 2)
    with pytest.raises(RuntimeError, match="GPU tensors"):         # well-formed, but not on a device
        readout.emm_submatch(qkv, lse, lse, torch.zeros(2, 3, 576, dtype=torch.int32), 2)
    intr = torch.ones(1, 2, 4)
    m = ViTEss(make_args())
    assert m.training
    for call in (lambda: m.subtoken_correspondences(torch.zeros(1, 2, 3, 64, 64)),
                 lambda: m.subtoken_correspondences_from_map(torch.zeros(2, 192, 24, 24)),
                 lambda: m.pose_from_matches(torch.zeros(1, 2, 3, 64, 64), intr, subtoken="window"),
                 lambda: m.refined_pose_from_matches(torch.zeros(1, 2, 3, 64, 64), intr, subtoken="quadratic"),
                 lambda: m.consensus_pose_from_matches(torch.zeros(1, 2, 3, 64, 64), intr, subtoken="window")):
        with pytest.raises(RuntimeError, match="eval"):
            call()
    with pytest.raises(ValueError, match="subtoken"):
        m.eval().pose_from_matches(torch.zeros(1, 2, 3, 64, 64), intr, subtoken="cubic")
    assert torch.equal(intr, torch.ones(1, 2, 4))
