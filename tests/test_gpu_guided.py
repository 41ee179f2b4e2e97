"""rp_emm_guided_matches (include/relpose_guided.h) on the GPU against the fp64 reference of tests/_guided_ref.py, and the model-level
entry points of rel_pose_amd/guided.py.

Parity runs one pair (Z = 2) with H = 1 and 3 heads over tests/_guided_ref.py: CASES -- flat random rows and the two-peaked built scene,
swap and single each both ways, band 0.75, 1.5 and 1e9 on a scene's F, a sideways translation (parallel lines), forward motion with
the epipole on a token (den = 0 there), lines that miss the grid for most owners (-1 among live neighbours) -- each also with padded
rows, which must give the same bits.

  edge pairs   a pair with |rho^2 / (band^2 den) - 1| <= 1e-4 in fp64 may fall on either side of the admission: an owner that has one is
               left out of the idx and bmass comparison; at most 5 % of a case's owners (tests/test_guided_cpu.py holds the reference
               alone to that cap; it shows <= 1.6 %)
  indices      check_indices of tests/test_gpu_readout.py against the ADMITTED runner-up: equal wherever it is below (1 - 1e-3) max, at
               most 0.5 % of the owners differing, A_ref at the reported index within 1e-3 of the admitted maximum
  stat         |amax - A_ref at idx| <= C_AMAX de A_ref, |bmass - ref| <= C_BMASS de bmass_ref, |mass - ref| <= C_MASS de mass_ref with
               de = eps32 (m scale max sum_d |q_d k_d| + |lse_owner| + max |lse_other|) per owner, |d2 - ref at idx| <= C_D2 eps32
               rho_abs^2 / den; C = 8 x the float32 restatement's worst ratio on these inputs (tests/_guided_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _guided_ref as G
from tests import _submatch_ref as S
from tests.test_gpu_kernels import report
from tests.test_gpu_submatch import matches_idx, rows, same_bits

pytestmark = pytest.mark.gpu
_IDS = ["%s-H%d-swap%d-single%d-%s-band%g" % c for c in G.CASES]
P = ctypes.c_void_p
_DEV = {}


@pytest.fixture(scope="module")
def libs():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    _lib.load()
    return _lib.load_readout(), _lib.load_guided()


def _stream():
    return P(torch.cuda.current_stream().cuda_stream)


def device_inputs(case, pad):
    kind, H = case[0], case[1]
    key = (kind, H, bool(case[3]), pad)
    if key not in _DEV:
        q, k, rl, cl, _ = G.case_inputs(kind, H)
        buf, ld = rows(q, k, pad)
        _DEV[key] = (buf, ld, torch.from_numpy(rl).cuda(), torch.from_numpy(cl).cuda())
    return _DEV[key]


def guided(libs, buf, ld, rlse, clse, F, band, Z, H, swap, single, fill=float("nan"), ifill=-7):
    idx = torch.full((Z, H, S.TOK), ifill, dtype=torch.int32, device="cuda")
    stat = torch.full((Z, H, S.TOK, 4), fill, device="cuda")
    libs[1].rp_emm_guided_matches(P(buf.data_ptr()), P(buf.data_ptr() + 4 * H * S.HD), P(rlse.data_ptr()), None if single else P(clse.data_ptr()),
                                  P(F.data_ptr()), P(band.data_ptr()), P(idx.data_ptr()), P(stat.data_ptr()), Z, H, ld, ld, S.SCALE, swap,
                                  single, _stream())
    torch.cuda.synchronize()
    return idx, stat


def check_against(ref, idx, stat, F, swap, tag):
    """the module docstring's rules -> the figures"""
    i, s = idx.cpu().numpy().astype(np.int64), stat.cpu().numpy()
    assert np.isfinite(s).all(), tag
    rep, r = G.index_report(i, ref), G.stat_ratios(i, s, ref, F, swap)
    print(tag, rep, r)
    report("guided_" + tag, **rep, **r)
    assert rep["left_out"] <= 0.05, (tag, rep)
    assert rep["wrong_clear"] == 0, (tag, rep)
    assert rep["differ"] <= 0.005, (tag, rep)
    keep = np.broadcast_to(~ref.edge_owner[:, None], i.shape) & ~np.broadcast_to(ref.degenerate[:, None, None], i.shape)
    assert np.array_equal(i[keep] < 0, ref.idx[keep] < 0), tag                                      # no match exactly where none is admitted
    has = keep & (i >= 0)
    at = np.take_along_axis(ref.A, np.maximum(i, 0)[..., None], -1)[..., 0]
    adm_at = np.take_along_axis(np.broadcast_to(ref.adm[:, None], ref.A.shape), np.maximum(i, 0)[..., None], -1)[..., 0]
    assert bool(adm_at[has].all()) and bool((at[has] >= (1 - 1e-3) * ref.stat[..., 0][has]).all()), tag
    assert r["amax"] <= G.C_AMAX and r["bmass"] <= G.C_BMASS and r["mass"] <= G.C_MASS and r["d2"] <= G.C_D2, (tag, r)
    assert bool((s[..., 1] <= s[..., 2]).all()) and bool((s[..., 0] <= s[..., 1] * (1 + 1e-6)).all()), tag
    dead = np.broadcast_to(ref.degenerate[:, None, None], i.shape)
    assert bool((i[dead] == -1).all()) and not s[dead].any(), tag
    return rep, r


@pytest.mark.parametrize("case", G.CASES, ids=_IDS)
def test_parity(libs, case):
    kind, H, swap, single, Fk, band = case
    q, k, rl, cl, b = G.case_inputs(kind, H)
    rl, cl = G.case_lse(case, q, k, rl, cl)
    F, bd = G.case_F(case, b)
    buf, ld, d_rl, d_cl = device_inputs(case, 0)
    dF, dbd = torch.from_numpy(F).cuda(), torch.from_numpy(bd).cuda()
    idx, stat = guided(libs, buf, ld, d_rl, d_cl, dF, dbd, 2, H, swap, single)
    # padded rows: the same values at another stride -> the same bits
    pbuf, pld, _, _ = device_inputs(case, 20)
    pidx, pstat = guided(libs, pbuf, pld, d_rl, d_cl, dF, dbd, 2, H, swap, single, fill=12345.0, ifill=99)
    assert torch.equal(idx, pidx) and same_bits(stat, pstat)
    ref = G.guided_ref(q, k, rl, cl, F, bd, swap=swap, single=single)
    check_against(ref, idx, stat, F, swap, _IDS[G.CASES.index(case)].replace("-", "_").replace("+", ""))
    if band == 1e9:
        # the full band: every pair admitted -- bmass IS mass, and the index is rp_emm_matches' under the same rule
        assert same_bits(stat[..., 1], stat[..., 2])
        pidx, _ = matches_idx(libs, buf, ld, d_rl, d_cl, 2, H, swap, single)
        rep = G.index_report(pidx.cpu().numpy(), ref)
        assert rep["wrong_clear"] == 0 and rep["differ"] <= 0.005, rep
        assert float((pidx != idx).float().mean()) <= 0.005
    if Fk == "miss":
        none = (idx < 0).float().mean().item()
        assert 0.5 < none < 0.9                                                                     # -1 among live neighbours


_DEGENERATE = [("F-zero", np.zeros(9, np.float32), 1.5), ("F-nan", None, 1.5), ("band-zero", "live", 0.0), ("band-negative", "live", -1.5),
               ("band-nan", "live", float("nan"))]


@pytest.mark.parametrize("what,Fbad,bbad", _DEGENERATE, ids=[d[0] for d in _DEGENERATE])
@pytest.mark.parametrize("swap", [0, 1])
def test_a_degenerate_image_is_flagged_and_its_partner_untouched(libs, what, Fbad, bbad, swap):
    case = ("random", 3, swap, 0, "scene", 1.5)
    q, k, rl, cl, b = G.case_inputs("random", 3)
    F, bd = G.case_F(case, b)
    buf, ld, d_rl, d_cl = device_inputs(case, 0)
    live = guided(libs, buf, ld, d_rl, d_cl, torch.from_numpy(F).cuda(), torch.from_numpy(bd).cuda(), 2, 3, swap, 0)
    for z in (0, 1):
        F2, bd2 = F.copy(), bd.copy()
        if Fbad is None:
            F2[z, 4] = np.nan
        elif not isinstance(Fbad, str):
            F2[z] = Fbad
        bd2[z] = bbad
        idx, stat = guided(libs, buf, ld, d_rl, d_cl, torch.from_numpy(F2).cuda(), torch.from_numpy(bd2).cuda(), 2, 3, swap, 0)
        assert bool((idx[z] == -1).all()) and not bool(stat[z].view(torch.int32).any())           # flagged: -1 and +0.0 everywhere
        assert torch.equal(idx[z ^ 1], live[0][z ^ 1]) and same_bits(stat[z ^ 1], live[1][z ^ 1])  # the partner: unchanged to the bit
        assert np.array_equal(G.degenerate(F2, bd2), np.arange(2) == z)


def test_swap_is_the_transposed_problem(libs):
    """S'_z = S_z^T is the problem with q'[z] = k[z ^ 1], k'[z] = q[z ^ 1], the normalisers exchanged and F' = F^T: its rows are the columns
    of the original -- the same products in the same order.  rho is formed from the other side's line there, so a pair on the band's edge
    may flip: owners without one have the same idx, amax and bmass bits, every owner the same mass bits; d2 is the same number formed in
    another order."""
    H, case = 3, ("random", 3, 1, 0, "scene", 1.5)
    q, k, rl, cl, b = G.case_inputs("random", H)
    F, bd = G.case_F(case, b)
    buf, ld, d_rl, d_cl = device_inputs(case, 0)
    tbuf, tld = rows(np.ascontiguousarray(k[::-1]), np.ascontiguousarray(q[::-1]))
    Ft = np.ascontiguousarray(F.reshape(2, 3, 3).transpose(0, 2, 1)).reshape(2, 9)
    dbd = torch.from_numpy(bd).cuda()
    a = guided(libs, buf, ld, d_rl, d_cl, torch.from_numpy(F).cuda(), dbd, 2, H, 1, 0)
    t = guided(libs, tbuf, tld, d_cl, d_rl, torch.from_numpy(Ft).cuda(), dbd, 2, H, 0, 0)
    ref = G.guided_ref(q, k, rl, cl, F, bd, swap=True)
    keep = torch.from_numpy(np.broadcast_to(~ref.edge_owner[:, None], (2, H, S.TOK)).copy()).cuda()
    assert float(keep.float().mean()) >= 0.95
    assert same_bits(a[1][..., 2], t[1][..., 2])
    assert torch.equal(a[0][keep], t[0][keep]) and same_bits(a[1][..., :2][keep], t[1][..., :2][keep])
    d2, scale = G.d2_at(F, a[0].cpu().numpy(), True)
    assert float(np.abs(t[1][..., 3].cpu().numpy() - d2)[keep.cpu().numpy()].max()) <= G.C_D2 * G.EPS32 * float(scale.max())


def test_results_are_bit_identical_from_call_to_call_and_whatever_the_outputs_held(libs):
    for case in (("random", 3, 0, 0, "scene", 1.5), ("built", 1, 1, 1, "forward", 0.75)):
        kind, H, swap, single = case[:4]
        F, bd = G.case_F(case, G.case_inputs(kind, H)[4])
        buf, ld, d_rl, d_cl = device_inputs(case, 0)
        dF, dbd = torch.from_numpy(F).cuda(), torch.from_numpy(bd).cuda()
        a = guided(libs, buf, ld, d_rl, d_cl, dF, dbd, 2, H, swap, single)
        b = guided(libs, buf, ld, d_rl, d_cl, dF, dbd, 2, H, swap, single)
        c = guided(libs, buf, ld, d_rl, d_cl, dF, dbd, 2, H, swap, single, fill=12345.0, ifill=0x12345678)
        assert torch.equal(a[0], b[0]) and torch.equal(a[0], c[0]) and same_bits(a[1], b[1]) and same_bits(a[1], c[1])


def test_refusals_come_before_any_launch(libs):
    case = ("random", 3, 0, 0, "scene", 1.5)
    buf, ld, rl, cl = device_inputs(case, 0)
    F, bd = (torch.from_numpy(a).cuda() for a in G.case_F(case, G.case_inputs("random", 3)[4]))
    idx = torch.full((2, 3, S.TOK), -7, dtype=torch.int32, device="cuda")
    stat = torch.full((2, 3, S.TOK, 4), -7.0, device="cuda")
    lib, b, st = libs[1], buf.data_ptr(), _stream()
    good = dict(q=b, k=b + 4 * 192, rlse=rl.data_ptr(), clse=cl.data_ptr(), F=F.data_ptr(), band=bd.data_ptr(), idx=idx.data_ptr(),
                stat=stat.data_ptr(), Z=2, H=3, ldq=ld, ldk=ld)

    def call(single=0, **kw):
        a = dict(good, **kw)
        ptr = lambda v: None if v is None else P(v)      # noqa: E731
        lib.rp_emm_guided_matches(ptr(a["q"]), ptr(a["k"]), ptr(a["rlse"]), ptr(a["clse"]), ptr(a["F"]), ptr(a["band"]), ptr(a["idx"]),
                                  ptr(a["stat"]), a["Z"], a["H"], a["ldq"], a["ldk"], 0.125, 0, single, st)
    shape = r"rel_pose_amd: rp_emm_guided_matches failed: bad shape \(RP error -1\)"
    align = r"rel_pose_amd: rp_emm_guided_matches failed: misaligned pointer/stride \(RP error -2\)"
    for kw in (dict(Z=3), dict(Z=0), dict(H=0), dict(ldq=128), dict(ldk=188), dict(q=None), dict(k=None), dict(rlse=None), dict(clse=None),
               dict(F=None), dict(band=None), dict(idx=None), dict(stat=None), dict(Z=3, q=b + 4)):      # shape comes before alignment
        with pytest.raises(RuntimeError, match=shape):
            call(**kw)
    for kw in (dict(q=b + 4), dict(k=b + 4 * 193), dict(rlse=rl.data_ptr() + 4), dict(clse=cl.data_ptr() + 8), dict(idx=idx.data_ptr() + 4),
               dict(stat=stat.data_ptr() + 4), dict(F=F.data_ptr() + 2), dict(band=bd.data_ptr() + 1), dict(ldq=ld + 2), dict(ldk=ld + 1)):
        with pytest.raises(RuntimeError, match=align):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((stat == -7.0).all())                                  # nothing ran
    call(single=1, clse=None)                                                                      # the single softmax needs no clse ...
    F3 = torch.cat([F[:1], F]).contiguous()                                                        # ... and F, band 4-byte alignment only
    call(F=F3.data_ptr() + 4 * 9, band=torch.cat([bd[:1], bd]).contiguous().data_ptr() + 4)
    torch.cuda.synchronize()
    assert bool((idx != -7).all())


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def pair():
    """one pair on a randomly initialised ViTEss in eval(), MIOpen's repeatable solvers asked for (tests/test_gpu_readout.py says why)"""
    from oracle import relpose_oracle as O
    from tests.test_gpu_memory_contract import _model
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    m = _model().eval()
    images = O.synthetic_images(1, 384, 384, key=78).cuda()
    intr = torch.tensor([[0.9 * 384, 0.8 * 384, 190.0, 196.0]]).repeat(1, 2, 1).contiguous().cuda()
    pose = torch.tensor([[0.8, -0.1, 0.3, 0.02, -0.05, 0.01, 0.998]], device="cuda")
    m.correspondences(images)                                                                      # (warm-up: code objects, solvers)
    yield m, images, intr, pose
    torch.backends.cudnn.deterministic = keep


def test_model_guided_correspondences_are_the_public_pieces(pair):
    from rel_pose_amd import guided, readout
    m, images, intr, pose = pair
    gc = m.guided_correspondences(images, intr, pose, band=1.5)
    with torch.no_grad():
        qkv, rlse, clse, Z, single = readout._scores_from_map(m, m.cnn_map(images)[0])
    F = guided.grid_fundamental(pose, intr, (384, 384))
    assert F.shape == (2, 9) and torch.equal(F[0].view(3, 3), F[1].view(3, 3).t())
    ri, rs = guided.emm_guided_matches(qkv, rlse, clse, F, 1.5, Z, swap=False, single=single)
    ci, cs = guided.emm_guided_matches(qkv, rlse, clse, F, torch.full((2,), 1.5, device="cuda"), Z, swap=True, single=single)
    assert torch.equal(gc.row_idx, ri) and torch.equal(gc.row_stat, rs) and torch.equal(gc.col_idx, ci) and torch.equal(gc.col_stat, cs)
    assert torch.equal(gc.mutual, guided.mutual(ri, ci)) and gc.mutual.dtype == torch.bool
    i = torch.arange(576, device="cuda")
    assert torch.equal(gc.mutual, (ri >= 0) & (torch.gather(ci.long(), -1, ri.long().clamp(min=0)) == i))
    assert torch.equal(gc.support, rs[..., 1].sum(-1) / rs[..., 2].sum(-1)) and gc.support.shape == (2, 3)
    assert torch.equal(m.pose_support(images, intr, pose, band=1.5), gc.support)
    assert bool((gc.support > 0).all()) and bool((gc.support < 1).all())
    # the full band is the plain readout: support 1, and the plain indices (ties aside)
    full = m.guided_correspondences(images, intr, pose, band=1e9)
    plain = m.correspondences(images)
    assert bool((full.support == 1).all()) and float((full.row_idx != plain.row_idx).float().mean()) <= 0.01
    # a pose without a direction: a zero F, every owner flagged, support 0 -- no NaN
    dead = m.guided_correspondences(images, intr, torch.tensor([[0, 0, 0, 0, 0, 0, 1.0]], device="cuda"))
    assert bool((dead.row_idx == -1).all()) and not bool(dead.mutual.any()) and not bool(dead.support.any())


@pytest.mark.parametrize("prior,subtoken", [("consensus", None), ("regressed", None), ("pose", None), ("pose", "window"), ("pose", "quadratic")])
def test_model_guided_pose_is_the_chain_of_the_public_pieces(pair, prior, subtoken):
    from rel_pose_amd import eightpoint, guided, readout, refine
    m, images, intr, pose = pair
    rounds = 2 if prior == "pose" and subtoken is None else 1
    keep = intr.clone()
    g = m.guided_pose_from_matches(images, intr, prior=pose if prior == "pose" else prior, band=1.5, rounds=rounds, iters=6, subtoken=subtoken)
    assert torch.equal(intr, keep)
    if prior == "consensus":
        p0 = m.consensus_pose_from_matches(images, intr).pose
    elif prior == "regressed":
        Gs = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device="cuda").repeat(1, 2, 1)
        with torch.no_grad():
            p0 = m(images, Gs, intrinsics=intr.clone())[0].data[:, 1].contiguous()
    else:
        p0 = pose
    assert torch.equal(g.prior, p0)
    tau = eightpoint.default_tau(intr, (384, 384)).cuda().contiguous()
    with torch.no_grad():
        qkv, rlse, clse, Z, single = readout._scores_from_map(m, m.cnn_map(images)[0])
    p = p0
    for r_ in range(rounds):
        gc = m.guided_correspondences(images, intr, p, band=1.5)
        if r_ == 0:
            assert torch.equal(g.support_before, gc.support)
        sub = None
        if subtoken is not None:
            rw, rq = readout.emm_submatch(qkv, rlse, clse, gc.row_idx, Z, swap=False, single=single, radius=2)
            sub = readout.SubtokenCorrespondences(gc, rw, rq, None, None)
            assert bool((rw[gc.row_idx < 0] == torch.tensor([-1.0, -1.0, 0.0, 0.0], device="cuda")).all())      # -1 is an invalid centre there
        x1, x2, w = eightpoint.assemble_matches(gc, intr, (384, 384), sub=sub, subtoken=subtoken or "window")
        assert bool((w.view(1, 3, 576)[gc.row_idx[1::2] < 0] == 0).all())                          # an owner without a match weighs nothing
        r = refine.refine_pose(p, x1, x2, w, tau=tau, iters=6, return_weights=True)
        p = r.pose
    assert torch.equal(g.pose, r.pose) and torch.equal(g.E, r.E) and torch.equal(g.stat, r.stat) and torch.equal(g.weights, r.weights)
    assert torch.equal(g.support_after, m.pose_support(images, intr, g.pose, band=1.5))
    assert torch.equal(g.unmatched, (gc.row_idx[1::2] < 0).flatten(1).float().mean(1))
    assert bool(torch.isfinite(g.pose).all()) and g.support_before.shape == g.support_after.shape == (2, 3)


def test_model_state_and_the_existing_entry_points_are_what_they_were(pair):
    m, images, intr, pose = pair
    state = {k: v.clone() for k, v in m.state_dict().items()}
    corr, mp = m.correspondences(images), m.pose_from_matches(images, intr)
    m.guided_pose_from_matches(images, intr, prior="regressed", rounds=2)
    m.pose_support(images, intr, pose)
    assert not m.training and all(not mod.training for mod in m.modules())
    after = m.state_dict()
    assert set(after) == set(state) and all(torch.equal(after[k], state[k]) for k in state)
    assert all(p.grad is None for p in m.parameters())
    again, mp2 = m.correspondences(images), m.pose_from_matches(images, intr)
    assert all(torch.equal(a, b) for a, b in zip(corr[:5], again[:5]))
    assert all(torch.equal(a, b) for a, b in zip(mp, mp2))


def test_model_refusals(pair):
    from tests.test_gpu_memory_contract import _bf16_configuration, _model
    _, images, intr, pose = pair
    m = _model()
    m.train()
    for call in (lambda: m.guided_correspondences(images, intr, pose), lambda: m.pose_support(images, intr, pose),
                 lambda: m.guided_pose_from_matches(images, intr, prior=pose)):
        with pytest.raises(RuntimeError, match="eval"):
            call()
    m.eval()
    _bf16_configuration(True)
    try:
        with pytest.raises(NotImplementedError):
            m.guided_correspondences(images, intr, pose)
    finally:
        _bf16_configuration(False)
    with pytest.raises(ValueError, match="prior"):
        m.guided_pose_from_matches(images, intr, prior="oracle")
    with pytest.raises(ValueError, match="pose"):
        m.guided_correspondences(images, intr, pose[:, :6])
    with pytest.raises(ValueError, match="subtoken"):
        m.guided_pose_from_matches(images, intr, prior=pose, subtoken="cubic")


def test_demo_guided_flag(capsys):
    """demo.py --eight_point --guided BAND: the lines in front of it are what they were; three more -- the guided pose, the share of
    owners without a partner in the band, and the support of the regressed, the consensus and the guided pose on one scale"""
    import os
    import re
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import demo
    g = os.path.join(root, "tests", "golden", "demo")
    argv = ["--img1", os.path.join(g, "matterport_1.png"), "--img2", os.path.join(g, "matterport_2.png"), "--eight_point"]
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        torch.manual_seed(5)
        plain = demo.main(argv)
        out_plain = capsys.readouterr().out
        torch.manual_seed(5)
        flagged = demo.main(argv + ["--guided", "1.5"])
        out_flagged = capsys.readouterr().out
    finally:
        torch.backends.cudnn.deterministic = keep
    assert plain.tobytes() == flagged.tobytes()
    assert "guided" not in out_plain and out_flagged.startswith(out_plain)
    extra = out_flagged[len(out_plain):].splitlines()
    assert len(extra) == 3, extra
    assert extra[0].startswith("guided pose x,y,z,qx,qy,qz,qw: ")
    assert extra[1].startswith("guided: prior consensus, band 1.5 token pitches, ")
    assert extra[2].startswith("in-band share of the attention's mass: regressed ")
    shares = [float(v) for v in re.findall(r"(?:regressed|consensus|guided) (\d\.\d+)", extra[2])]
    assert len(shares) == 3 and all(0 <= v <= 1 for v in shares), extra[2]
    with pytest.raises(SystemExit):
        demo.main(argv[:4] + ["--guided", "1.5"])                                                  # --guided needs --eight_point
    capsys.readouterr()
