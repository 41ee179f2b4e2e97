"""Guided matching without a GPU: the references of tests/_guided_ref.py against each other and on built scenes, grid_fundamental in
torch on the CPU, and the ABI of librelpose_guided.so (header, exports, version).

The scene figures asserted here are the reference's own on scenes 0 .. 2 (seeds 4000 .. 4002 of _submatch_ref.built_inputs) at distractor
shares f = 0.3, 0.5, 0.7; DESIGN.md 5.10 quotes the table.  Every margin is what the three seeds show, none was fixed in advance."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _guided_ref as G
from tests import _refine_ref as RF
from tests import _submatch_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rp_guided_abi_version", "rp_emm_guided_matches"}


# ------------------------------------------------------------------------------------------------ ABI
def test_guided_header_parses_and_the_library_exports_it():
    from ctypes import c_float, c_int, c_void_p
    from rel_pose_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "relpose_guided.h")).read()
    consts, structs, sigs, status = _lib._header_contract(text, "relpose_guided.h")
    assert consts == {"RP_GUIDED_ABI_VERSION": 1} and not structs and _lib.GUIDED_ABI_VERSION == 1
    P, I = c_void_p, c_int
    assert list(sigs.items()) == [("rp_guided_abi_version", (c_int, [])), ("rp_emm_guided_matches", (c_int, [P] * 8 + [I] * 4 + [c_float, I, I, P]))]
    assert status == {"rp_emm_guided_matches"} and tuple(sigs) == _lib.GUIDED_EXPORTS
    declared = set(re.findall(r"\b(rp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(sigs) == NAMES
    typed = _lib.load_guided()
    raw = ctypes.CDLL(_build.GUIDED_LIB)
    for sym in declared:
        assert hasattr(raw, sym), "missing export: " + sym
    assert typed.rp_guided_abi_version() == _lib.GUIDED_ABI_VERSION
    # an eleventh library, not a change of the other ten: it exports none of their names and they export none of its
    others = (set(_lib.EXPORTS) | set(_lib.READOUT_EXPORTS) | set(_lib.EIGHTPOINT_EXPORTS) | set(_lib.REFINE_EXPORTS) | set(_lib.CONSENSUS_EXPORTS)
              | set(_lib.SUBMATCH_EXPORTS) | set(_lib.FIVEPOINT_EXPORTS) | set(_lib.HOMOGRAPHY_EXPORTS) | set(_lib.TRIANGULATE_EXPORTS)
              | set(_lib.CONV5X5_EXPORTS))
    assert not declared & others
    for sym in others:
        assert not hasattr(raw, sym), "librelpose_guided.so exports " + sym
    assert not any(hasattr(ctypes.CDLL(_build.READOUT_LIB), sym) for sym in declared)
    assert _lib.READOUT_EXPORTS == ("rp_readout_abi_version", "rp_emm_matches") and _lib.READOUT_ABI_VERSION == 1
    assert typed.rp_emm_guided_matches.errcheck is _lib.load().rp_gemm.errcheck and typed.rp_guided_abi_version.errcheck is None


def test_guided_build_is_a_library_of_its_own():
    from rel_pose_amd import _build, _lib
    _lib.load_guided()
    assert os.path.basename(_build.GUIDED_LIB) == "librelpose_guided.so"
    assert os.path.basename(_build.GUIDED_CSRC) == "csrc_guided" and _build.GUIDED_SOURCES == ["emm_guided.hip"]
    assert sorted(f for f in os.listdir(_build.GUIDED_CSRC) if f.endswith((".hip", ".h"))) == ["emm_guided.hip"]
    assert os.path.join(ROOT, "include", "relpose_guided.h") in _build._guided_headers()
    assert not _build.guided_needs_build()                                        # (the loader built it)
    src = open(os.path.join(_build.GUIDED_CSRC, "emm_guided.hip")).read()
    assert '#include "../csrc/two_view.h"' in src and '#include "../csrc/tile32.h"' in src        # included, not copied


def test_a_stale_guided_library_is_refused(monkeypatch):
    from rel_pose_amd import _lib
    _lib.load_guided()
    monkeypatch.setattr(_lib, "_GUIDED_LIB", None)
    monkeypatch.setattr(_lib, "GUIDED_ABI_VERSION", 2)
    with pytest.raises(RuntimeError, match=r"librelpose_guided\.so has ABI version 1, this package binds version 2"):
        _lib.load_guided()


# ------------------------------------------------------------------------------------------------ the references against each other
@pytest.fixture(scope="module")
def calibration():
    """every parity case once: the float32 restatement against the fp64 reference"""
    out = {}
    for case in G.CASES:
        kind, H, swap, single, Fk, band = case
        q, k, rl, cl, b = G.case_inputs(kind, H)
        rl, cl = G.case_lse(case, q, k, rl, cl)
        F, bd = G.case_F(case, b)
        ref = G.guided_ref(q, k, rl, cl, F, bd, swap=swap, single=single)
        idx, stat = G.guided_f32(q, k, rl, cl, F, bd, swap=swap, single=single)
        out[case] = (ref, idx, stat, G.stat_ratios(idx, stat, ref, F, swap), G.index_report(idx, ref))
    return out


def test_the_constants_are_eight_times_the_restatements_worst_ratio(calibration):
    worst = {key: max(v[3][key] for v in calibration.values()) for key in ("amax", "bmass", "mass", "d2")}
    print("guided_f32 worst ratios:", worst)
    for key, C in (("amax", G.C_AMAX), ("bmass", G.C_BMASS), ("mass", G.C_MASS), ("d2", G.C_D2)):
        assert 8 * worst[key] <= C <= 8 * worst[key] + 0.1, (key, worst[key], C)


def test_the_cases_keep_the_edge_owners_under_the_cap_and_the_restatement_agrees_on_the_indices(calibration):
    """the reference alone decides which owners have a pair within 1e-4 of the band's edge: at most 5 % of a case's owners"""
    most = 0.0
    for case, (ref, idx, stat, _, rep) in calibration.items():
        most = max(most, rep["left_out"])
        assert rep["left_out"] <= 0.05, (case, rep)
        assert rep["wrong_clear"] == 0 and rep["differ"] <= 0.005, (case, rep)
        assert np.isfinite(stat).all() and bool((stat[..., 1] <= stat[..., 2]).all())
    print("largest share of owners with an edge pair: %.4f" % most)
    # the cases cover what they are there for: owners without any admitted token among live ones, and den = 0 at the epipole
    miss = calibration[("random", 1, 0, 0, "miss", 1.5)][0]
    assert 0.5 < float((miss.idx < 0).mean()) < 0.9
    fwd = calibration[("random", 1, 0, 0, "forward", 1.5)][0]
    ep = 13 * G.GRID + 11
    assert bool(fwd.adm[1, ep].all()) and float(G.pair_terms(G.case_F(("random", 1, 0, 0, "forward", 1.5), None)[0])[1][1, ep, ep]) == 0.0


def test_the_full_band_is_the_plain_readout(calibration):
    for case, (ref, idx, stat, _, _) in calibration.items():
        kind, H, swap, single, Fk, band = case
        if band != 1e9:
            continue
        q, k, rl, cl, _ = G.case_inputs(kind, H)
        rl, cl = G.case_lse(case, q, k, rl, cl)
        assert np.array_equal(ref.idx, S.argmax_idx(q, k, rl, cl, swap=swap, single=single))
        assert bool(ref.adm.all()) and np.array_equal(ref.stat[..., 1], ref.stat[..., 2])
        assert np.array_equal(stat[..., 1], stat[..., 2])                          # the restatement: bit for bit


def test_admission_f32_is_the_fp64_admission_off_the_edge():
    b = S.built_inputs(1)
    for F1 in (G.grid_F(b), G.special_F("forward"), G.special_F("miss")):
        F = np.stack([F1.reshape(3, 3).T.reshape(9), F1]).astype(np.float32)
        for band in (0.75, 1.5, 7.0):
            bd = np.full(2, band, np.float32)
            rho, den, _ = G.pair_terms(F)
            rel = np.where(den > 0, rho * rho / (band * band * np.where(den > 0, den, 1)), 0)
            off = np.abs(rel - 1) > G.EDGE
            a32 = G.admission_f32(F, bd)
            assert np.array_equal(a32[off], (~(den > 0) | (rel <= 1))[off])
            both = off[0] & off[1].T                                               # F_0 = F_1^T: the transposed problem, rho formed from the
            assert np.array_equal(a32[0][both], a32[1].T[both])                    # other side's line -- the same admission off the edge
    # a scaled F is the same F; a degenerate image admits nothing
    assert np.array_equal(G.admission_f32(F * np.float32(1e20), bd), G.admission_f32(F, bd))
    live = G.admission_f32(F, np.full(2, 1.5, np.float32))[1]
    for bad_F, bad_band in ((np.zeros(9), 1.5), (np.r_[np.nan, np.ones(8)], 1.5), (F[1], 0.0), (F[1], -1.0), (F[1], np.nan)):
        Fd, bdd = np.stack([np.asarray(bad_F, np.float32), F[1]]), np.array([bad_band, 1.5], np.float32)
        a = G.admission_f32(Fd, bdd)
        assert not a[0].any() and np.array_equal(a[1], live)


# ------------------------------------------------------------------------------------------------ built scenes
@pytest.fixture(scope="module")
def scenes():
    """scene s, distractor share f -> the reference's figures (problem 1: rows are image 0's tokens), computed once"""
    out = {}
    for s in range(3):
        for f in (0.3, 0.5, 0.7):
            tp = G.two_peak_inputs(s, f)
            b = tp.built
            rl, _ = S.stats64(tp.q, tp.k)
            plain = S.argmax_idx(tp.q, tp.k, rl, None, single=True)[1, 0]
            pose = G.true_pose(b)
            rng = np.random.default_rng(100 + s)
            near, far = RF.perturbed(pose[None], rng, 0.03)[0], RF.perturbed(pose[None], rng, 0.5)[0]

            def guided(p, band):
                F = np.stack([G.grid_F(b, p)] * 2).astype(np.float32)
                r = G.guided_ref(tp.q, tp.k, rl, None, F, np.full(2, band, np.float32), single=True)
                return r.idx[1, 0], float(r.stat[1, 0, :, 1].sum() / r.stat[1, 0, :, 2].sum())
            g_true, _ = guided(pose, 1.0)
            g_near, sup_near = guided(near, 1.5)
            g_far, sup_far = guided(far, 1.5)
            out[s, f] = dict(plain=G.correct_share(b, plain), guided=G.correct_share(b, g_true), sup_true=guided(pose, 1.5)[1], sup_near=sup_near,
                             sup_far=sup_far, ref_plain=G.refine_errors(b, plain, near), ref_guided=G.refine_errors(b, g_near, near),
                             far_guided=G.refine_errors(b, g_far, far), far_plain_cost=G.refine_errors(b, plain, far)[2])
            print("scene %d f %.1f:" % (s, f), {k_: np.round(v, 4).tolist() for k_, v in out[s, f].items()})
    return out


def test_guided_matches_recover_rows_the_argmax_loses(scenes):
    """share of the in-image rows matched within 0.75 token of the truth: plain argmax 0.29 .. 0.71 (about 1 - f), argmax within one token
    of the true pose's lines 0.84 .. 0.94"""
    for (s, f), v in scenes.items():
        assert abs(v["plain"] - (1 - f)) < 0.05, (s, f, v["plain"])
        assert v["guided"] > v["plain"] + 0.2 and v["guided"] > 0.84, (s, f, v)


def test_guided_refinement_from_a_near_start_ends_nearer_the_truth(scenes):
    """refine_ref(iters = 10) from 0.03 rad off, at f = 0.7 where the plain matches are mostly wrong: on the guided matches (band 1.5 around
    the START's lines) it ends at 0.4 .. 2.3 deg / 1.7 .. 3.4 deg, on the plain ones at 1.9 .. 4.7 / 2.5 .. 9.8.  (At f = 0.5 scene 2's plain
    refinement happens to end 0.2 / 0.3 deg off and beats the guided one's 0.2 / 1.0: with half the rows right the gain is not uniform.)"""
    for s in range(3):
        v = scenes[s, 0.7]
        assert v["ref_guided"][0] < 0.6 * v["ref_plain"][0] and v["ref_guided"][1] < 0.7 * v["ref_plain"][1], (s, v)
        assert v["ref_guided"][0] < 2.5 and v["ref_guided"][1] < 3.5


def test_the_support_flags_a_far_prior_and_its_refinement_does_not(scenes):
    """in-band mass share (band 1.5): 0.36 .. 0.67 at the true pose, within 0.01 of that 0.03 rad off -- the share does not resolve an
    error well inside the band -- and 0.05 .. 0.29 at 0.5 rad off, at least 0.17 below.  The far prior confirms itself: refined on its own
    guided matches it stays 17 .. 37 deg wrong at a robust cost BELOW that of the plain matches refined from the same start, and below
    that of the plain matches refined from 0.03 rad off: the cost after guiding says nothing about the pose."""
    for (s, f), v in scenes.items():
        assert abs(v["sup_true"] - v["sup_near"]) < 0.011, (s, f, v)
        assert min(v["sup_true"], v["sup_near"]) > v["sup_far"] + 0.17, (s, f, v)
        assert v["sup_true"] > 0.36 and v["sup_far"] < 0.30
        assert v["far_guided"][0] > 15 and v["far_guided"][1] > 20, (s, f, v)
        assert v["far_guided"][2] < 0.9 * min(v["far_plain_cost"], v["ref_plain"][2]), (s, f, v)      # (the ratios: 0.28 .. 0.80)


# ------------------------------------------------------------------------------------------------ grid_fundamental, on the CPU in torch
def test_grid_fundamental_puts_every_true_partner_on_its_line():
    from rel_pose_amd import guided
    hw = (384, 512)                                                             # H != W: the token pitches differ
    intr = torch.tensor([[[410.0, 395.0, 250.0, 180.0], [380.0, 402.0, 262.0, 199.0]]], dtype=torch.float64)     # non-square, off-centre
    rng = np.random.default_rng(3)
    Rm = RF.quat_to_rot(np.array([0.05, -0.08, 0.03, 0.995]) / np.linalg.norm([0.05, -0.08, 0.03, 0.995]))
    t = np.array([0.9, -0.2, 0.3])
    E = torch.from_numpy(RF.cross_matrix(t) @ Rm)[None]
    F = guided.grid_fundamental_from_E(E, intr, hw)
    assert F.shape == (2, 9) and F.dtype == torch.float32
    assert torch.equal(F[0].view(3, 3), F[1].view(3, 3).t())
    assert abs(float(F[1].double().norm()) - 1) < 1e-6 and abs(float(F[0].double().norm()) - 1) < 1e-6
    # every token of image 0 at a random depth, its true partner in image 1 in grid units of image 1: d2 at rounding level
    k = intr[0].numpy()
    tok = G._tokens()[:, :2]
    pix0 = (tok + 0.5) * np.array([hw[1] / 24, hw[0] / 24])
    x1 = (pix0 - k[0, 2:]) / k[0, :2]
    X2 = np.concatenate([x1, np.ones((576, 1))], -1) * rng.uniform(2, 8, (576, 1)) @ Rm.T + t
    pix1 = X2[:, :2] / X2[:, 2:] * k[1, :2] + k[1, 2:]
    g1 = pix1 / np.array([hw[1] / 24, hw[0] / 24]) - 0.5
    Fm = F[1].double().numpy().reshape(3, 3)
    r, c = np.concatenate([tok, np.ones((576, 1))], -1), np.concatenate([g1, np.ones((576, 1))], -1)
    l, m = r @ Fm.T, c @ Fm
    d2 = np.einsum("na,na->n", c, l) ** 2 / (l[:, 0] ** 2 + l[:, 1] ** 2 + m[:, 0] ** 2 + m[:, 1] ** 2)
    assert float(d2.max()) < 1e-9, float(d2.max())                              # squared token pitches; F is float32
    # the same through the even image's matrix with the roles exchanged
    Ft = F[0].double().numpy().reshape(3, 3)
    assert np.allclose(np.einsum("na,ab,nb->n", r, Ft, c), np.einsum("na,na->n", c, l), atol=1e-12)
    # a zero E gives a zero (degenerate) F, not a NaN
    assert not guided.grid_fundamental_from_E(torch.zeros(1, 3, 3), intr, hw).any()
    with pytest.raises(ValueError):
        guided.grid_fundamental_from_E(E, intr[:, :1], hw)


def test_grid_fundamental_agrees_with_the_reference_scene_matrix():
    """on the built scenes' camera (square pixels, principal point at the grid's middle) it is _guided_ref.grid_F up to float32"""
    from rel_pose_amd import guided
    b = S.built_inputs(0)
    px = 16.0                                                                   # pixels per token: a 384 x 384 image
    intr = torch.tensor([[[b.focal * px, b.focal * px, 12 * px, 12 * px]] * 2], dtype=torch.float64)
    F = guided.grid_fundamental_from_E(torch.from_numpy(RF.cross_matrix(b.t) @ b.R)[None], intr, (384, 384))
    assert np.abs(F[1].numpy() - G.grid_F(b)).max() < 1e-7


def test_mutual_and_support_are_safe_where_there_is_no_match():
    from rel_pose_amd import guided
    row = torch.tensor([[2, -1, 0, 1]], dtype=torch.int32)
    col = torch.tensor([[2, -1, 0, -1]], dtype=torch.int32)
    assert guided.mutual(row, col).tolist() == [[True, False, True, False]]
    stat = torch.zeros(2, 1, 4, 4)
    stat[0, 0, :, 1], stat[0, 0, :, 2] = torch.tensor([0.1, 0.0, 0.2, 0.1]), torch.tensor([0.5, 0.5, 0.5, 0.5])
    assert torch.allclose(guided.support_of(stat), torch.tensor([[0.2], [0.0]]))
