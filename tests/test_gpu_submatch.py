"""rp_emm_submatch (include/relpose_submatch.h) on the GPU against the fp64 reference of tests/_submatch_ref.py.

Parity runs one pair (Z = 2) with H = 1 and 3 heads, packed rows (ld = 3 H 64, q | k | v as the qkv Linear writes them) and padded rows
(bit-identical to the packed ones), swap, single and radius each both ways, on the built inputs (a clean Gaussian peak around every
match) and on random inputs (flat, multi-modal rows); the window centres come from rp_emm_matches and from a hand-made table (corners,
every border, all owners on one token, -1 / 576 / INT_MIN / INT_MAX among valid neighbours).

Bounds, with delta_e = eps32 (m scale max_window sum_d |q_d k_d| + |lse_owner| + max_window |lse_other|) per owner and C = 8 x the largest
ratio of the float32 restatement on the same inputs (tests/_submatch_ref.py; recomputed in tests/test_submatch_cpu.py):
    |wx|, |wy| error <= C_WXY 2 radius delta_e       wmass relative error <= C_WMASS delta_e       wvar error <= C_WVAR (2 radius)^2 delta_e
    cx, cy error <= C_CURV 4 delta_e                 px, py error <= C_PXY 4 delta_e (1 + 2 |offset_ref|) / c_ref
every owner compared for win and the curvatures; px / py for every owner with both neighbours on the built inputs (swap = 0), where
c_ref >= 1e-3 otherwise, and where a clamp is active only if both sides clamp (then the positions are equal)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _submatch_ref as S
from tests.test_gpu_kernels import report

pytestmark = pytest.mark.gpu
_IDS = ["%s-H%d-swap%d-single%d-r%d-%s" % c for c in S.CASES]
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def libs():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    _lib.load()
    return _lib.load_readout(), _lib.load_submatch()


def _stream():
    return P(torch.cuda.current_stream().cuda_stream)


def rows(q, k, pad=0):
    """q, k [Z,576,H,64] -> one device buffer [Z*576, ld] holding q | k | (v's place and the padding: NaN, which a kernel must not use)"""
    Z, _, H, _ = q.shape
    ld = 3 * H * S.HD + pad
    t = torch.full((Z * S.TOK, ld), float("nan"))
    t[:, :H * S.HD] = torch.from_numpy(q.reshape(Z * S.TOK, -1))
    t[:, H * S.HD:2 * H * S.HD] = torch.from_numpy(k.reshape(Z * S.TOK, -1))
    return t.cuda(), ld


def matches_idx(libs, buf, ld, rlse, clse, Z, H, swap, single):
    idx = torch.empty(Z, H, S.TOK, dtype=torch.int32, device="cuda")
    stat = torch.empty(Z, H, S.TOK, 4, device="cuda")
    libs[0].rp_emm_matches(P(buf.data_ptr()), P(buf.data_ptr() + 4 * H * S.HD), P(rlse.data_ptr()), None if single else P(clse.data_ptr()),
                           P(idx.data_ptr()), P(stat.data_ptr()), None, Z, H, ld, ld, S.SCALE, swap, single, _stream())
    return idx, stat


def submatch(libs, buf, ld, rlse, clse, idx, Z, H, swap, single, radius, fill=float("nan")):
    win = torch.full((Z, H, S.TOK, 4), fill, device="cuda")
    quad = torch.full((Z, H, S.TOK, 4), fill, device="cuda")
    libs[1].rp_emm_submatch(P(buf.data_ptr()), P(buf.data_ptr() + 4 * H * S.HD), P(rlse.data_ptr()), None if single else P(clse.data_ptr()),
                            P(idx.data_ptr()), P(win.data_ptr()), P(quad.data_ptr()), Z, H, ld, ld, S.SCALE, swap, single, radius, _stream())
    torch.cuda.synchronize()
    return win, quad


@functools.lru_cache(maxsize=None)
def device_inputs(kind, H, pad):
    q, k, rlse, clse = S.case_inputs(kind, H)
    buf, ld = rows(q, k, pad)
    return buf, ld, torch.from_numpy(rlse).cuda(), torch.from_numpy(clse).cuda()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("case", S.CASES, ids=_IDS)
def test_parity(libs, case):
    kind, H, swap, single, radius, src = case
    q, k, rlse, clse = S.case_inputs(kind, H)
    buf, ld, d_rlse, d_clse = device_inputs(kind, H, 0)
    if src == "table":
        idx = torch.from_numpy(S.table_idx(2, H)).cuda()
    else:
        idx, _ = matches_idx(libs, buf, ld, d_rlse, d_clse, 2, H, swap, single)
    win, quad = submatch(libs, buf, ld, d_rlse, d_clse, idx, 2, H, swap, single, radius)
    assert bool(torch.isfinite(win).all()) and bool(torch.isfinite(quad).all())
    # padded rows: the same values at another stride -> the same bits
    pbuf, pld, _, _ = device_inputs(kind, H, 20)
    pwin, pquad = submatch(libs, pbuf, pld, d_rlse, d_clse, idx, 2, H, swap, single, radius)
    assert same_bits(win, pwin) and same_bits(quad, pquad)
    ref = S.submatch_ref(q, k, rlse, clse, idx.cpu().numpy(), S.SCALE, swap, single, radius)
    built = kind == "built" and not swap
    if built:                    # the bound on px, py assumes this curvature: 2 g (single), within a factor 2 of 4 g (dual); g = 0.5
        c = np.concatenate([ref.quad[..., 2][ref.both_x], ref.quad[..., 3][ref.both_y]])
        assert (abs(c - 1.0).max() <= 4 * ref.delta_e.max()) if single else (1.0 <= c.min() and c.max() <= 4.0), (c.min(), c.max())
    r = S.bound_ratios((win.cpu().numpy(), quad.cpu().numpy()), ref, radius, built=built)
    print(case, r)
    report("submatch_parity_" + _IDS[S.CASES.index(case)].replace("-", "_"), **r)
    assert r["compared"] >= 0.99, r
    assert r["wxy"] <= S.C_WXY and r["wmass"] <= S.C_WMASS and r["wvar"] <= S.C_WVAR, r
    assert r["curv"] <= S.C_CURV and r["pxy"] <= S.C_PXY, r


@pytest.mark.parametrize("H,swap,single,radius", [(3, 0, 0, 2), (1, 1, 1, 1), (3, 1, 0, 1), (1, 0, 1, 2)])
def test_invalid_centres_are_flagged_and_do_not_disturb_their_neighbours(libs, H, swap, single, radius):
    buf, ld, rlse, clse = device_inputs("random", H, 0)
    dirty, clean = S.table_idx(2, H), S.table_idx(2, H, invalid=False)
    bad = (dirty < 0) | (dirty >= S.TOK)
    assert int(bad.sum()) == 5 and {-1, S.TOK, S.INT_MIN} <= set(dirty[bad].tolist())
    win, quad = submatch(libs, buf, ld, rlse, clse, torch.from_numpy(dirty).cuda(), 2, H, swap, single, radius)
    win0, quad0 = submatch(libs, buf, ld, rlse, clse, torch.from_numpy(clean).cuda(), 2, H, swap, single, radius)
    flag = torch.tensor(S.FLAG, device="cuda")
    m = torch.from_numpy(bad).cuda()
    assert bool((win[m] == flag).all()) and bool((quad[m] == flag).all())
    assert same_bits(win[~m], win0[~m]) and same_bits(quad[~m], quad0[~m])
    assert bool((win0[..., 0] >= 0).all()) and bool((quad0[..., 0] >= 0).all())
    # all owners of the last (z, h) sit on one token: one window, 576 different owner vectors
    assert int((torch.from_numpy(clean)[-1, -1] == 301).all())


def test_results_are_bit_identical_from_call_to_call_and_whatever_the_outputs_held(libs):
    for kind, H, swap, single, radius in (("random", 3, 0, 0, 2), ("built", 1, 1, 1, 1)):
        buf, ld, rlse, clse = device_inputs(kind, H, 0)
        idx, _ = matches_idx(libs, buf, ld, rlse, clse, 2, H, swap, single)
        a = submatch(libs, buf, ld, rlse, clse, idx, 2, H, swap, single, radius)
        b = submatch(libs, buf, ld, rlse, clse, idx, 2, H, swap, single, radius)
        c = submatch(libs, buf, ld, rlse, clse, idx, 2, H, swap, single, radius, fill=12345.0)
        for x, y, z in zip(a, b, c):
            assert same_bits(x, y) and same_bits(x, z) and bool(torch.isfinite(x).all())


@pytest.mark.parametrize("radius", [1, 2])
def test_swap_is_the_transposed_problem(libs, radius):
    """dual softmax: S'_z = S_z^T is the problem with q'[z] = k[z ^ 1], k'[z] = q[z ^ 1] and the two normalisers exchanged; its rows are
    the columns of the original -- the same products in the same order, so the same bits"""
    H = 3
    q, k, rlse, clse = S.case_inputs("random", H)
    buf, ld, d_rlse, d_clse = device_inputs("random", H, 0)
    tbuf, tld = rows(np.ascontiguousarray(k[::-1]), np.ascontiguousarray(q[::-1]))
    idx, _ = matches_idx(libs, buf, ld, d_rlse, d_clse, 2, H, 1, 0)
    a = submatch(libs, buf, ld, d_rlse, d_clse, idx, 2, H, 1, 0, radius)
    b = submatch(libs, tbuf, tld, d_clse, d_rlse, idx, 2, H, 0, 0, radius)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


# ------------------------------------------------------------------------------------------------ the chain, through the C ABI
def test_gpu_chain_on_the_built_scenes_halves_the_errors():
    """the ten built scenes as one batch (Z = 20, three heads carrying the same scores in three different mixes, packed qkv rows) through
    rp_emm_stats -> rp_emm_matches -> rp_emm_submatch (radius 2) -> rp_eight_point (iters 4) -> rp_pose_from_essential -> rp_refine_pose
    (iters 10) on head 0: with x2 from win the median rotation error and the median translation-direction error are each at most half
    of the token-centre chain's (tests/test_submatch_cpu.py: the same claim on the fp64 reference)."""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    from tests import _refine_ref as F
    core, ro, sm, ep, rf = _lib.load(), _lib.load_readout(), _lib.load_submatch(), _lib.load_eightpoint(), _lib.load_refine()
    H, n = 3, 10
    scenes = [S.built_inputs(s, H=H) for s in range(n)]
    buf, ld = rows(np.concatenate([b.q for b in scenes]), np.concatenate([b.k for b in scenes]))
    Z, st = 2 * n, _stream()
    qp, kp = P(buf.data_ptr()), P(buf.data_ptr() + 4 * H * S.HD)
    new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device="cuda")          # noqa: E731
    rlse, clse = new(Z, H, S.TOK), new(Z, H, S.TOK)
    ws = new(core.rp_emm_stats_workspace_bytes(Z, H) // 4)
    core.rp_emm_stats(qp, kp, P(rlse.data_ptr()), P(clse.data_ptr()), P(ws.data_ptr()), None, Z, H, ld, ld, S.SCALE, 0, st)
    idx, stat, win, quad = new(Z, H, S.TOK, dtype=torch.int32), new(Z, H, S.TOK, 4), new(Z, H, S.TOK, 4), new(Z, H, S.TOK, 4)
    ro.rp_emm_matches(qp, kp, P(rlse.data_ptr()), P(clse.data_ptr()), P(idx.data_ptr()), P(stat.data_ptr()), None, Z, H, ld, ld, S.SCALE, 0, 0, st)
    sm.rp_emm_submatch(qp, kp, P(rlse.data_ptr()), P(clse.data_ptr()), P(idx.data_ptr()), P(win.data_ptr()), P(quad.data_ptr()), Z, H, ld, ld,
                       S.SCALE, 0, 0, 2, st)
    torch.cuda.synchronize()
    mid, focal = (S.GRID - 1) / 2, scenes[0].focal
    x1 = torch.from_numpy(np.stack([b.x1 for b in scenes]).astype(np.float32)).cuda().contiguous()
    w = torch.from_numpy(np.stack([b.inside for b in scenes]).astype(np.float32)).cuda().contiguous()
    i0 = idx[1::2, 0].long()
    centre = torch.stack([i0 % S.GRID, i0 // S.GRID], -1).float()
    err, pos = {}, {}
    for name, p, tau_tokens in (("centre", centre, 0.5), ("window", win[1::2, 0, :, :2], 0.05)):
        x2 = ((p - mid) / focal).contiguous()
        tau = torch.full((n,), tau_tokens / focal, device="cuda")
        E, est, pose0, count = new(n, 9), new(n, 4), new(n, 7), new(n, dtype=torch.int32)
        pose, E2, rst = new(n, 7), new(n, 9), new(n, 4)
        ep.rp_eight_point(P(x1.data_ptr()), P(x2.data_ptr()), P(w.data_ptr()), P(tau.data_ptr()), P(E.data_ptr()), P(est.data_ptr()), None,
                          S.TOK, 4, n, st)
        core.rp_pose_from_essential(P(E.data_ptr()), P(x1.data_ptr()), P(x2.data_ptr()), S.TOK, P(pose0.data_ptr()), P(count.data_ptr()), n, st)
        rf.rp_refine_pose(P(pose0.data_ptr()), P(x1.data_ptr()), P(x2.data_ptr()), P(w.data_ptr()), P(tau.data_ptr()), P(pose.data_ptr()),
                          P(E2.data_ptr()), P(rst.data_ptr()), None, S.TOK, 10, n, st)
        torch.cuda.synchronize()
        out = pose.double().cpu().numpy()
        assert np.isfinite(out).all()
        e = []
        for b, o in zip(scenes, out):
            Rm, t = F.pose_matrix(o)
            e.append((F.rotation_angle(Rm, b.R), F.direction_angle(t, b.t)))
        err[name] = np.array(e)
        pp = p.double().cpu().numpy()
        pos[name] = float(np.median([np.median(np.linalg.norm(pp[s] - b.p, axis=-1)[b.inside]) for s, b in enumerate(scenes)]))
    med = {k: np.median(v, 0) for k, v in err.items()}
    print("median (rotation, translation) errors:", med, "max:", {k: v.max(0) for k, v in err.items()}, "position:", pos)
    report("submatch_gpu_chain", rot_centre=med["centre"][0], rot_window=med["window"][0], tr_centre=med["centre"][1],
           tr_window=med["window"][1], rot_centre_max=err["centre"][:, 0].max(), rot_window_max=err["window"][:, 0].max(),
           tr_centre_max=err["centre"][:, 1].max(), tr_window_max=err["window"][:, 1].max(), pos_centre=pos["centre"], pos_window=pos["window"])
    assert med["window"][0] <= 0.5 * med["centre"][0], med
    assert med["window"][1] <= 0.5 * med["centre"][1], med


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def scene():
    """the synthetic state of __graft_entry__.smoke() and one batch of synthetic images"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from oracle import relpose_oracle as O
    from tests.test_gpu_memory_contract import _model
    m = _model().eval()
    B = 2
    images = O.synthetic_images(B, 384, 384, key=78).cuda()
    intr = torch.tensor([[0.9 * 384, 0.8 * 384, 192.0, 192.0]]).repeat(B, 2, 1).contiguous().cuda()
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True      # runs from images, bit for bit
    m.correspondences(images)                                    # (warm-up: first calls load code objects and pick solvers)
    yield m, images, intr
    torch.backends.cudnn.deterministic = keep


def test_subtoken_correspondences_are_emm_submatch_on_the_pieces(scene):
    from rel_pose_amd import ops, readout
    from rel_pose_amd.ops import DIM, N_TOK
    m, images, _ = scene
    state = {k: v.clone() for k, v in m.state_dict().items()}
    sub = m.subtoken_correspondences(images)
    corr = m.correspondences(images)
    for got, want in zip(sub.corr, corr):
        assert (got is None and want is None) or torch.equal(got, want)
    # the pieces: the model's own path up to the last block's qkv, rp_emm_stats, then the kernel around the matches
    ft = m.fusion_transformer
    with torch.no_grad():
        fmap, _ = m.cnn_map(images)
        x = ops.TokensFn.apply(fmap.float(), ft.pos_embed[0])
        for layer in range(m.transformer_depth - 1):
            x = ft.blocks[layer](x)
        blk = ft.blocks[m.transformer_depth - 1]
        Z = x.shape[0]
        qkv = ops.ln_linear(x.contiguous().view(Z * N_TOK, DIM), blk.norm1.weight, blk.norm1.bias, blk.cross_attn.qkv.weight,
                            blk.cross_attn.qkv.bias, train=False)[0]
        rlse, clse = ops.emm_stats(qkv, Z, False)
    for swap, idx, win, quad in ((False, corr.row_idx, sub.row_win, sub.row_quad), (True, corr.col_idx, sub.col_win, sub.col_quad)):
        w, q = readout.emm_submatch(qkv, rlse, clse, idx, Z, swap=swap, radius=2)
        assert same_bits(w, win) and same_bits(q, quad)
        assert win.shape == (4, 3, 576, 4) and bool(torch.isfinite(win).all()) and bool(torch.isfinite(quad).all())
        # a valid centre everywhere: the positions stay within the window / half a token of the centre
        c = torch.stack([idx % 24, idx // 24], -1).float()
        assert float((win[..., :2] - c).abs().max()) <= 2.0 and float((quad[..., :2] - c).abs().max()) <= 0.5
        assert bool((win[..., 2] > 0).all()) and bool((win[..., 3] >= 0).all())
    r1 = m.subtoken_correspondences(images, radius=1)
    assert same_bits(r1.row_quad, sub.row_quad) and not same_bits(r1.row_win, sub.row_win)
    with torch.no_grad():
        fm = m.subtoken_correspondences_from_map(m.cnn_map(images)[0])
    assert same_bits(fm.row_win, sub.row_win) and same_bits(fm.col_quad, sub.col_quad)
    after = m.state_dict()
    assert not m.training and set(after) == set(state) and all(torch.equal(after[k], state[k]) for k in state)


@pytest.mark.parametrize("subtoken", ["window", "quadratic"])
def test_pose_from_matches_with_subtoken_is_the_chain_of_the_public_pieces(scene, subtoken):
    from rel_pose_amd import consensus, eightpoint, geom, readout, refine
    m, images, intr = scene
    keep_intr = intr.clone()
    hw = (384, 384)
    sub = m.subtoken_correspondences(images, 1 if subtoken == "quadratic" else 2)
    x1, x2, w = eightpoint.assemble_matches(sub.corr, intr, hw, sub=sub, subtoken=subtoken)
    y1, y2, v = eightpoint.assemble_matches(sub.corr, intr, hw)
    assert torch.equal(x1, y1) and torch.equal(w, v) and not torch.equal(x2, y2)
    px = readout.subtoken_xy((sub.row_win if subtoken == "window" else sub.row_quad)[1::2], hw)          # [B,3,576,2] pixels in image 1
    want = (px - intr[:, 1, 2:4][:, None, None, :]) / intr[:, 1, 0:2][:, None, None, :]
    assert torch.allclose(x2.view(2, 3, 576, 2), want, rtol=0, atol=1e-6)
    tau = (0.1 * eightpoint.default_tau(intr, hw)).contiguous()
    ep = eightpoint.eight_point(x1, x2, w, tau=tau, iters=4, return_weights=True)
    pose, count = geom.pose_from_essential(ep.E, x1, x2)
    kw = dict(tau=tau, subtoken=subtoken, radius=1 if subtoken == "quadratic" else 2)
    mp = m.pose_from_matches(images, intr, **kw)
    for got, want in zip(mp, (pose, ep.E, ep.stat, count, ep.weights)):
        assert torch.equal(got, want)
    assert bool(torch.isfinite(mp.pose).all())
    r = refine.refine_pose(pose, x1, x2, w, tau=tau, iters=3, return_weights=True)
    rp = m.refined_pose_from_matches(images, intr, refine=3, **kw)
    for got, want in zip(rp[:4], r):
        assert torch.equal(got, want)
    for got, want in zip(rp.initial, mp):
        assert torch.equal(got, want)
    c = consensus.eight_point_consensus(x1, x2, w, tau=tau, hypotheses=128, seed=5, return_weights=True)
    ep2 = eightpoint.eight_point(x1, x2, c.weights, tau=tau, iters=4, return_weights=True)
    pose2, _ = geom.pose_from_essential(ep2.E, x1, x2)
    r2 = refine.refine_pose(pose2, x1, x2, w, tau=tau, iters=3, return_weights=True)
    cp = m.consensus_pose_from_matches(images, intr, hypotheses=128, seed=5, refine=3, **kw)
    for got, want in zip(cp[:4], r2):
        assert torch.equal(got, want)
    assert torch.equal(intr, keep_intr)


def test_pose_from_matches_without_the_keyword_is_what_it_was(scene):
    """the chain as it stood before the keyword existed, written out from the pieces: bit for bit"""
    from rel_pose_amd import eightpoint, geom, readout
    m, images, intr = scene
    hw = (384, 384)
    corr = m.correspondences(images)
    c = readout.token_centres(hw, device=intr.device)
    idx = corr.row_idx[1::2].long()
    k = intr.permute(2, 1, 0)[..., None, None]
    x1 = readout.normalised(c.expand(2, 3, 576, 2).permute(3, 0, 1, 2), k[:, 0]).permute(1, 2, 3, 0).reshape(2, 1728, 2).contiguous()
    x2 = readout.normalised(c[idx].permute(3, 0, 1, 2), k[:, 1]).permute(1, 2, 3, 0).reshape(2, 1728, 2).contiguous()
    w = (corr.row_stat[1::2][..., 0] * corr.mutual[1::2].float()).reshape(2, 1728).contiguous()
    a1, a2, aw = eightpoint.assemble_matches(corr, intr, hw)
    assert torch.equal(a1, x1) and torch.equal(a2, x2) and torch.equal(aw, w)
    tau = eightpoint.default_tau(intr, hw).contiguous()
    ep = eightpoint.eight_point(x1, x2, w, tau=tau, iters=4, return_weights=True)
    pose, count = geom.pose_from_essential(ep.E, x1, x2)
    for mp in (m.pose_from_matches(images, intr), m.pose_from_matches(images, intr, subtoken=None, radius=1)):
        for got, want in zip(mp, (pose, ep.E, ep.stat, count, ep.weights)):
            assert torch.equal(got, want)
