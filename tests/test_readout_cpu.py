"""The EMM readout (include/relpose_readout.h, librelpose_readout.so, rel_pose_amd/readout.py) as far as it goes without a GPU: the
header and the binding derived from it, the argument checks that precede any launch, and the plain-torch helpers."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_readout_header_parses_and_the_library_exports_it():
    from ctypes import c_float, c_int, c_void_p
    from rel_pose_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "relpose_readout.h")).read()
    consts, structs, sigs, status = _lib._header_contract(text, "relpose_readout.h")
    assert consts == {"RP_READOUT_ABI_VERSION": _lib.READOUT_ABI_VERSION} and not structs
    P, I = c_void_p, c_int
    assert list(sigs.items()) == [("rp_readout_abi_version", (c_int, [])),
                                  ("rp_emm_matches", (c_int, [P, P, P, P, P, P, P, I, I, I, I, c_float, I, I, P]))]
    assert status == {"rp_emm_matches"} and tuple(sigs) == _lib.READOUT_EXPORTS
    # the declarations as a C reader sees them (comments stripped), independently of the parser
    declared = set(re.findall(r"\b(rp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(sigs)
    typed = _lib.load_readout()
    raw = ctypes.CDLL(_build.READOUT_LIB)
    for sym in declared:
        assert hasattr(raw, sym), "missing export: " + sym
    assert typed.rp_readout_abi_version() == _lib.READOUT_ABI_VERSION
    # a second library, not a change of the first: the main header declares none of this
    assert not declared & set(_lib.EXPORTS)
    main = open(os.path.join(ROOT, "include", "relpose_hip.h")).read()
    assert "rp_emm_matches" not in main and "rp_readout" not in main


def test_parser_names_the_header_it_reads():
    from rel_pose_amd import _lib
    with pytest.raises(ValueError, match=r"^relpose_readout\.h: "):
        _lib._header_contract("short rp_x(int a);", "relpose_readout.h")
    with pytest.raises(ValueError, match=r"^relpose_hip\.h: "):
        _lib._header_contract("short rp_x(int a);")


def test_readout_build_is_a_library_of_its_own():
    from rel_pose_amd import _build
    assert os.path.basename(_build.READOUT_LIB) == "librelpose_readout.so" and _build.READOUT_LIB != _build.LIB
    assert _build.READOUT_SOURCES and not set(_build.READOUT_SOURCES) & set(_build.SOURCES)
    for s in _build.READOUT_SOURCES:
        assert os.path.isfile(os.path.join(ROOT, "rel_pose_amd", "csrc_readout", s))
        assert not os.path.exists(os.path.join(_build.CSRC, s))        # the hot path's source set is what it was
    assert not _build.readout_needs_build() or _build.build(verbose=False) == _build.LIB
    assert not _build.readout_needs_build() and not _build.needs_build()


def test_launching_entry_points_check_their_status():
    from rel_pose_amd import _lib
    lib = _lib.load_readout()
    hooked = {n for n in _lib.READOUT_EXPORTS if getattr(lib, n).errcheck is not None}
    assert hooked == {"rp_emm_matches"} and lib.rp_emm_matches.errcheck is _lib.load().rp_gemm.errcheck
    assert lib.rp_readout_abi_version.restype is ctypes.c_int


def test_argument_checks_come_before_any_launch():
    """no device is needed (or touched): the pointers are never dereferenced, the refusals precede the launch"""
    from rel_pose_amd import _lib
    lib = _lib.load_readout()
    P = ctypes.c_void_p
    ok = [P(4096), P(8192), P(12288), P(16384), P(20480), P(24576), None]

    def call(ptrs=ok, Z=2, H=3, ldq=576, ldk=576, single=0):
        return lib.rp_emm_matches(*ptrs, Z, H, ldq, ldk, 0.125, 0, single, None)
    shape = r"rel_pose_amd: rp_emm_matches failed: bad shape \(RP error -1\)"
    align = r"rel_pose_amd: rp_emm_matches failed: misaligned pointer/stride \(RP error -2\)"
    for kw in (dict(Z=3), dict(Z=0), dict(Z=-2), dict(H=0), dict(ldq=188), dict(ldk=128), dict(ptrs=[None] + ok[1:]),
               dict(ptrs=ok[:3] + [None] + ok[4:])):                       # (clse may be NULL with the single softmax only)
        with pytest.raises(RuntimeError, match=shape):
            call(**kw)
    for kw in (dict(ldq=578), dict(ldk=598), dict(ptrs=[P(4100)] + ok[1:]), dict(ptrs=ok[:4] + [P(20488)] + ok[5:]),
               dict(ptrs=ok[:6] + [P(28676)]), dict(ptrs=ok[:2] + [P(12292)] + ok[3:], single=1)):
        with pytest.raises(RuntimeError, match=align):
            call(**kw)


def _random_pose(seed):
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    R = q * torch.sign(torch.linalg.det(q))
    t = torch.randn(3, generator=g, dtype=torch.float64)
    tx = torch.tensor([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], dtype=torch.float64)
    X1 = torch.randn(200, 3, generator=g, dtype=torch.float64) + torch.tensor([0, 0, 6.0], dtype=torch.float64)
    X2 = X1 @ R.T + t
    return tx @ R, X1[:, :2] / X1[:, 2:], X2[:, :2] / X2[:, 2:]


def test_sampson_distance_in_the_convention_of_pose_from_essential():
    from rel_pose_amd import readout
    f = 500.0
    for seed in range(3):
        E, x1, x2 = _random_pose(seed)
        d = readout.sampson_distance(E, x1, x2)
        assert d.shape == (200,) and float(d.max()) < 1e-12
        # one pixel (1 / f) across the epipolar line in image 2: the squared point-to-line distance (1/f)^2 times the share of the
        # squared gradient of x2^T E x1 that lies in image 2 -- the closed form, with the norms taken here -- and for every point at
        # least six orders of magnitude above the rounding residue of its exact projection
        one = torch.ones(200, 1, dtype=torch.float64)
        line = torch.cat([x1, one], -1) @ E.T
        n = line[:, :2] / line[:, :2].norm(dim=-1, keepdim=True)
        d1 = readout.sampson_distance(E, x1, x2 + n / f)
        g2 = (line[:, :2] ** 2).sum(-1)
        g1 = ((torch.cat([x2 + n / f, one], -1) @ E)[:, :2] ** 2).sum(-1)
        assert torch.allclose(d1, g2 / (g1 + g2) / f ** 2, rtol=1e-9, atol=0)
        assert bool((d1 > 1e6 * d).all()) and float(d1.min()) > 0 and float(d1.max()) <= 1.0001 / f ** 2
        # the roles of the two images are not interchangeable
        assert float(readout.sampson_distance(E, x2, x1).max()) > 1e-6
        # batched E and points
        db = readout.sampson_distance(torch.stack([E, 2 * E]), torch.stack([x1, x1]), torch.stack([x2, x2 + n / f]))
        assert db.shape == (2, 200) and float(db[0].max()) < 1e-12 and torch.allclose(db[1], d1, rtol=1e-9, atol=0)


def test_token_centres_and_normalised():
    from rel_pose_amd import readout
    c = readout.token_centres((384, 512), dtype=torch.float64)
    assert c.shape == (576, 2) and c.dtype == torch.float64
    assert c[0].tolist() == [0.5 * 512 / 24, 0.5 * 384 / 24] and c[1].tolist() == [1.5 * 512 / 24, 0.5 * 384 / 24]
    assert c[24].tolist() == [0.5 * 512 / 24, 1.5 * 384 / 24] and c[575].tolist() == [23.5 * 512 / 24, 23.5 * 384 / 24]
    assert readout.token_centres((24, 24)).dtype == torch.float32
    assert torch.equal(readout.token_centres((24, 24))[100], torch.tensor([100 % 24 + 0.5, 100 // 24 + 0.5]))
    xy = torch.tensor([[320.0, 240.0], [837.97, 240.0 - 517.97]], dtype=torch.float64)
    nx = readout.normalised(xy, [517.97, 517.97, 320, 240])
    assert nx.dtype == torch.float64 and torch.allclose(nx, torch.tensor([[0.0, 0.0], [1.0, -1.0]], dtype=torch.float64), atol=1e-15)


def _hand_made():
    """Z = 2, H = 1: image 1's rows follow a permutation except rows 5 and 7, which both pick column 9 (column 9 answers row 7)"""
    from rel_pose_amd import readout
    g = torch.Generator().manual_seed(5)
    perm = torch.randperm(576, generator=g)
    row = torch.stack([torch.arange(576), perm]).view(2, 1, 576).int()
    col = torch.stack([torch.arange(576), torch.argsort(perm)]).view(2, 1, 576).int()
    j5, j7 = int(perm[5]), int(perm[7])
    row[1, 0, 5] = j7                       # two rows claim column j7; the column's own best row stays 7
    stat = torch.zeros(2, 1, 576, 4)
    stat[..., 0] = torch.arange(576) / 1000.0
    m = readout.mutual(row, col)
    return readout.Correspondences(row, stat, col, stat.clone(), m, None), perm, j5, j7


def test_mutual_on_hand_made_indices():
    corr, perm, j5, j7 = _hand_made()
    assert corr.mutual.dtype == torch.bool and corr.mutual.shape == (2, 1, 576)
    assert bool(corr.mutual[0].all())
    expect = torch.ones(576, dtype=torch.bool)
    expect[5] = False
    assert torch.equal(corr.mutual[1, 0], expect)


def test_matches_xy_on_hand_made_indices():
    from rel_pose_amd import readout
    corr, perm, j5, j7 = _hand_made()
    c = readout.token_centres((240, 480))
    a, b, conf = readout.matches_xy(corr, 1, 0, (240, 480))
    keep = torch.arange(576) != 5
    assert a.shape == (575, 2) and torch.equal(a, c[keep]) and torch.equal(b, c[perm[keep]])
    assert torch.equal(conf, (torch.arange(576) / 1000.0)[keep])
    a, b, conf = readout.matches_xy(corr, 1, 0, (240, 480), mutual_only=False)
    assert a.shape == (576, 2) and torch.equal(a, c) and torch.equal(b[5], c[j7]) and torch.equal(b[6], c[perm[6]])
    assert float(conf[5]) == pytest.approx(0.005)


def test_readout_refuses_what_it_cannot_read_before_touching_a_device():
    from rel_pose_amd.model import ViTEss
    from tests.test_host_cpu import make_args
    fmap = torch.zeros(2, 192, 24, 24)
    m = ViTEss(make_args())
    assert m.training
    with pytest.raises(RuntimeError, match="eval"):
        m.correspondences_from_map(fmap)
    with pytest.raises(RuntimeError, match="eval"):
        m.correspondences(torch.zeros(1, 2, 3, 64, 64))
    with pytest.raises(ValueError, match="noess"):
        ViTEss(make_args(noess="1")).eval().correspondences_from_map(fmap)
