"""rp_emm_matches (include/relpose_readout.h, csrc_readout/emm_readout.hip) and the readout built on it, on a real MI355X.

The reference is fp64 and is computed here: S_z = scale q_{z^1} k_z^T, its log-sum-exp both ways, the exponent 2 S - rlse - clse, A,
and per row / per column the argmax, the maximum, the sum and the two position sums.  rel = max|a - b| / max|b| as in the other GPU
tests.  Bounds:
  norm-wise   rel(A), rel(amax), rel(mass), rel(ex), rel(ey) < 1e-5 -- the project's bound for T = A X and F against fp64 with the same
              A (test_emm_forward_pieces);
  elementwise amax, mass within relative tau = 1e-4, ex / ey within 2 tau 23 tokens: a worst-case bound of a 64-term exact-fp32 dot
              product at unit-scale inputs gives ~4e-5 on A (the same arithmetic in fp32 on the CPU: 5e-6);
  indices     equal to the reference's wherever its runner-up is below (1 - tau) max; for EVERY owner A_ref at the reported index is
              >= (1 - tau) max; at most 0.5 % of the owners differ at all (the reference has 0-3 of 6912 owners with a runner-up
              within 1e-4 on such inputs).
"""
import ctypes
import os
import sys

import pytest
import torch

from tests import _contract_cases as CC
from tests.test_gpu_kernels import rel, report, rnd
from tests.test_gpu_memory_contract import _bf16_configuration, _model, run_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 1e-4
N, H = 576, 3


@pytest.fixture(scope="module")
def ro():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, readout
    _lib.load()
    _lib.load_readout()
    return readout


def scores(qkv64, Z):
    """S [Z,3,576 i,576 j] = q_{z^1}[i] . k_z[j] / 8 of a packed q | k | v"""
    t = qkv64.view(Z, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    return (t[0][[z ^ 1 for z in range(Z)]] @ t[1].transpose(-1, -2)) * 0.125


def exponent(S, single=False):
    rl, cl = torch.logsumexp(S, -1), torch.logsumexp(S, -2)
    return (S - rl[..., None]) if single else (2 * S - rl[..., None] - cl[..., None, :]), rl, cl


def reduce_ref(E):
    """per owner (second to last index) over the last one: index, A at it, runner-up / maximum, mass, soft-argmax (x, y)"""
    A = E.exp()
    top = E.topk(2, -1)
    n = torch.arange(N, dtype=torch.float64)
    mass = A.sum(-1)
    return dict(E=E, A=A, idx=top.indices[..., 0], amax=top.values[..., 0].exp(), ratio=(top.values[..., 1] - top.values[..., 0]).exp(),
                mass=mass, ex=(A * (n % 24)).sum(-1) / mass, ey=(A * torch.div(n, 24, rounding_mode="floor")).sum(-1) / mass)


def check_indices(idx, ref, tau, cap, tag):
    idx = idx.cpu().long()
    at = torch.gather(ref["A"], -1, idx[..., None])[..., 0]
    clear = ref["ratio"] < 1 - tau
    differ = int((idx != ref["idx"]).sum())
    report("readout_idx_" + tag, owners=idx.numel(), near_ties=int((~clear).sum()), differ=differ,
           worst_at_idx=float((at / ref["amax"]).min()))
    assert bool((idx[clear] == ref["idx"][clear]).all()), "%s: index differs where the runner-up is below (1 - tau) max" % tag
    assert bool((at >= (1 - tau) * ref["amax"]).all()), "%s: A at the reported index is not within tau of the maximum" % tag
    assert differ <= cap * idx.numel(), "%s: %d of %d owners differ in index" % (tag, differ, idx.numel())


def check_values(stat, ref, tag):
    s = stat.double().cpu()
    e = {k: rel(s[..., i], ref[k]) for i, k in enumerate(("amax", "mass", "ex", "ey"))}
    el = {k: float(((s[..., i] - ref[k]).abs() / ref[k]).max()) for i, k in enumerate(("amax", "mass"))}
    pos = max(float((s[..., 2] - ref["ex"]).abs().max()), float((s[..., 3] - ref["ey"]).abs().max()))
    report("readout_" + tag, **e, amax_elementwise=el["amax"], mass_elementwise=el["mass"], position_abs=pos)
    assert max(e.values()) < 1e-5, (tag, e)
    assert max(el.values()) < TAU and pos < 2 * TAU * 23, (tag, el, pos)


def check_side(ro, qkv, rl, cl, Z, ref, swap, single, tag, dense_ref=None):
    idx, stat, A = ro.emm_matches(qkv, rl, cl, Z, swap=swap, single=single, dense=dense_ref is not None)
    assert idx.dtype == torch.int32 and idx.shape == (Z, H, N) and stat.shape == (Z, H, N, 4)
    check_values(stat, ref, tag)
    check_indices(idx, ref, TAU, 0.005, tag)
    # amax is A at the reported index, mass the sum it belongs to
    assert bool((stat[..., 0] <= stat[..., 1]).all()) and bool((stat[..., 0] > 0).all())
    if dense_ref is not None:
        assert A.shape == (Z, H, N, N)
        e = rel(A, dense_ref)
        report("readout_dense_" + tag, A=e)
        assert e < 1e-5, (tag, e)
        got = torch.gather(A if not swap else A.transpose(-1, -2), -1, idx.long()[..., None])[..., 0]
        assert torch.equal(got, stat[..., 0]), "%s: amax is not the dense A at idx" % tag
    else:
        assert A is None
    return idx, stat, A


@pytest.fixture(scope="module")
def random4():
    """Z = 4 (two pairs: the z ^ 1 pairing matters), the reference of both sides, computed once"""
    Z = 4
    qkv = rnd(Z * N, 576, seed=21)
    E, rl, cl = exponent(scores(qkv.double().cpu(), Z))
    return dict(Z=Z, qkv=qkv, rl=rl, cl=cl, A=E.exp(), rows=reduce_ref(E), cols=reduce_ref(E.transpose(-1, -2)))


@pytest.mark.parametrize("stats", ["fp64_rounded", "emm_stats"])
def test_random_parity(ro, random4, stats):
    from rel_pose_amd import ops
    d, Z = random4, random4["Z"]
    if stats == "emm_stats":
        rl, cl = ops.emm_stats(d["qkv"], Z)
    else:
        rl, cl = d["rl"].float().cuda(), d["cl"].float().cuda()
    check_side(ro, d["qkv"], rl, cl, Z, d["rows"], False, False, "rows_" + stats, dense_ref=d["A"])
    check_side(ro, d["qkv"], rl, cl, Z, d["cols"], True, False, "cols_" + stats, dense_ref=d["A"])
    # deterministic from call to call
    again = ro.emm_matches(d["qkv"], rl, cl, Z, swap=False, dense=True)
    first = ro.emm_matches(d["qkv"], rl, cl, Z, swap=False, dense=True)
    assert all(torch.equal(a, b) for a, b in zip(again, first))


def test_planted_permutation(ro):
    """q_{z^1}[i] = 4 k_z[pi(i)], another permutation per (z, h): the row argmax IS pi, the column argmax its inverse -- no tie slack, so
    a wrong partner image, head, transposed index or accumulator-row mapping cannot pass"""
    from rel_pose_amd import ops
    Z = 2
    g = torch.Generator().manual_seed(77)
    qkv = torch.randn(Z * N, 576, generator=g)
    k = qkv.view(Z, N, 3, H, 64)[:, :, 1]                          # [Z,576,H,64]
    perms = torch.stack([torch.stack([torch.randperm(N, generator=g) for _ in range(H)]) for _ in range(Z)])      # [Z,H,576]
    q = qkv.view(Z, N, 3, H, 64)[:, :, 0]
    for z in range(Z):
        for h in range(H):
            q[z ^ 1, :, h] = 4 * k[z, perms[z, h], h]
    E, rl, cl = exponent(scores(qkv.double(), Z))
    rows, cols = reduce_ref(E), reduce_ref(E.transpose(-1, -2))
    assert float(rows["ratio"].max()) < 0.5 and float(cols["ratio"].max()) < 0.5
    assert torch.equal(rows["idx"], perms) and torch.equal(cols["idx"], torch.argsort(perms, -1))
    dev = qkv.cuda()
    r, c = ops.emm_stats(dev, Z)
    row_idx, row_stat, _ = ro.emm_matches(dev, r, c, Z, swap=False)
    col_idx, col_stat, _ = ro.emm_matches(dev, r, c, Z, swap=True)
    assert torch.equal(row_idx.cpu().long(), perms)
    assert torch.equal(col_idx.cpu().long(), torch.argsort(perms, -1))
    assert bool(ro.mutual(row_idx, col_idx).all())


def test_large_scores(ro):
    """one head of one image times 40, as in test_attention_stats_partner: exponents of magnitude 1e3, A underflowing for whole owners"""
    Z = 4
    qkv = rnd(Z * N, 576, seed=3).clone()
    qkv[:N, :64] *= 40.0
    E, rl, cl = exponent(scores(qkv.double().cpu(), Z))
    r, c = rl.float().cuda(), cl.float().cuda()
    empty = 0
    for swap, Es in ((False, E), (True, E.transpose(-1, -2))):
        idx, stat, A = ro.emm_matches(qkv, r, c, Z, swap=swap, dense=True)
        assert bool(torch.isfinite(stat).all()) and bool(torch.isfinite(A).all())
        amax, mass, ex, ey = stat.unbind(-1)
        assert bool((amax >= 0).all()) and bool((amax <= mass).all()) and bool((mass <= 1 + 1e-3).all())
        top = Es.topk(2, -1)
        clear = (top.values[..., 1] - top.values[..., 0]).exp() < 0.5
        assert bool((idx.cpu().long()[clear] == top.indices[..., 0][clear]).all())
        none = mass == 0
        empty += int(none.sum())
        assert bool((ex[none] == -1).all()) and bool((ey[none] == -1).all())
        assert bool((ex[~none] >= 0).all()) and bool((ex[~none] <= 23.01).all()) and bool((ey[~none] >= 0).all()) and bool((ey[~none] <= 23.01).all())
        report("readout_large_swap%d" % swap, clear_owners=int(clear.sum()), empty_owners=int(none.sum()), mass_max=float(mass.max()))
    # normalisers 1000 nats too large: every A underflows to exactly 0 -- no mass, no position, and the argmax of the exponent stands
    idx, stat, _ = ro.emm_matches(qkv, r + 1000.0, c, Z, swap=False)
    top = E.topk(2, -1)
    clear = (top.values[..., 1] - top.values[..., 0]).exp() < 0.5
    assert bool((stat[..., :2] == 0).all()) and bool((stat[..., 2:] == -1).all())
    assert bool((idx.cpu().long()[clear] == top.indices[..., 0][clear]).all())
    # the unscaled heads are as exact as ever
    ref = reduce_ref(E[2:])
    idx, stat, _ = ro.emm_matches(qkv, r, c, Z, swap=False)
    check_values(stat[2:], ref, "large_other_pair")


def test_single_softmax(ro):
    from rel_pose_amd import ops
    Z = 2
    qkv = rnd(Z * N, 576, seed=22)
    E, rl, _ = exponent(scores(qkv.double().cpu(), Z), single=True)
    r = rl.float().cuda()
    rows, cols = reduce_ref(E), reduce_ref(E.transpose(-1, -2))
    junk = torch.full_like(r, float("nan"))                       # clse is unused
    _, stat, _ = check_side(ro, qkv, r, junk, Z, rows, False, True, "single_rows", dense_ref=E.exp())
    assert float((stat[..., 1] - 1).abs().max()) < TAU              # a row softmax sums to one
    check_side(ro, qkv, r, junk, Z, cols, True, True, "single_cols", dense_ref=E.exp())
    r2, _ = ops.emm_stats(qkv, Z, single=True)
    check_side(ro, qkv, r2, r2, Z, rows, False, True, "single_rows_emm_stats")


# ------------------------------------------------------------------------------------------------ memory contract
def _matches_case(Z, ld, swap=False, single=False, dense=True, split=False):
    """one guarded rp_emm_matches call (tests/_contract_cases.py's Case, kept out of its table: that table is the main header's).
    split: q and k in buffers of their own with row stride ld; otherwise one packed q | k buffer."""
    d = CC._emm_data(Z)
    q, k = d["qkv"][:, :CC.DIM], d["qkv"][:, CC.DIM:2 * CC.DIM]
    if split:
        ops_ = [CC.inp("q", q, ld=ld), CC.inp("k", k, ld=ld)]
    else:
        ops_ = [CC.inp_multi("qk", Z * N, ld, {0: d["qkv"][:, :2 * CC.DIM]})]
    ops_ += [CC.inp("rlse", CC._f32(d["rlse"]).reshape(1, -1)), CC.flat("idx", Z * H * N, dtype=CC.I32), CC.flat("stat", Z * H * N * 4)]
    if not single:
        ops_.append(CC.inp("clse", CC._f32(d["clse"]).reshape(1, -1)))
    if dense:
        ops_.append(CC.flat("a_out", Z * H * N * N))

    def call(lib, A_, st):
        P = CC.P
        qa, ka = (A_["q"].addr(), A_["k"].addr()) if split else (A_["qk"].addr(), A_["qk"].addr(CC.DIM))
        lib.rp_emm_matches(P(qa), P(ka), P(A_["rlse"].addr()), None if single else P(A_["clse"].addr()), P(A_["idx"].addr()),
                           P(A_["stat"].addr()), P(A_["a_out"].addr()) if dense else None, Z, H, ld, ld, CC.SCALE, int(swap), int(single), st)

    def check(v, errs):
        e = {}
        if dense and not single:
            A = (2 * d["S2"] / CC.LOG2E - d["rlse"][..., None] - d["clse"][..., None, :]).exp()
            e["A"] = CC._bound(errs, "a_out", CC.rel(v["a_out"].view(Z, H, N, N), A), 1e-5)
        i = v["idx"].view(-1)
        if not bool(((i >= 0) & (i < N)).all()):
            errs.append("idx outside 0..575")
        return e
    return CC.Case(ops_, call, check, sibling=(lambda: _matches_case(Z, 2 * CC.DIM, swap, single, dense)) if split else None)


_CASES = [("Z2-packed-dense", lambda: _matches_case(2, 576)),
          ("Z2-packed-swap-dense", lambda: _matches_case(2, 576, swap=True)),
          ("Z4-ld640-no-dense", lambda: _matches_case(4, 640, dense=False)),
          ("Z2-ld640-single-swap", lambda: _matches_case(2, 640, swap=True, single=True, dense=False)),
          ("Z2-split-ld600-dense", lambda: _matches_case(2, 600, split=True)),
          ("Z2-split-ld600-swap-dense", lambda: _matches_case(2, 600, swap=True, split=True))]


@pytest.mark.parametrize("ident, builder", _CASES, ids=[c[0] for c in _CASES])
def test_memory_contract(ro, ident, builder):
    """guards intact, gaps untouched, every documented element written, inputs unchanged, NaN-fill and finite-fill runs bit-identical,
    the strided layout bit-identical to its packed sibling"""
    from rel_pose_amd import _lib
    lib = _lib.load_readout()
    bad_a, va, c, ops_ = run_case(lib, builder, finite=False)
    bad_b, vb, _, _ = run_case(lib, builder, finite=True)
    bad = ["NaN-fill run: " + b for b in bad_a] + ["finite-fill run: " + b for b in bad_b]
    assert set(va) == {o.name for o in ops_ if o.role == "out"} and {"idx", "stat"} <= set(va)
    for w in va:
        bits = CC._BITS[va[w].dtype]
        if not torch.equal(va[w].view(bits), vb[w].view(bits)):
            bad.append("%s: result depends on what the output held before the call" % w)
    if c.sibling is not None:
        bad_p, vp, _, _ = run_case(lib, c.sibling, finite=False)
        bad += ["packed sibling: " + b for b in bad_p]
        assert set(vp) == set(va)
        for w in va:
            if not torch.equal(va[w].view(CC._BITS[va[w].dtype]), vp[w].view(CC._BITS[vp[w].dtype])):
                bad.append("%s: the strided layout's result differs from the packed layout's" % w)
    errs = c.check(va, bad) if not bad_a else {}
    report("readout_memory_contract_" + ident.replace("-", "_"), violations=len(bad), **errs)
    assert not bad, "\n".join(bad)


def test_errors_are_raised_before_any_launch(ro):
    Z = 2
    qkv = rnd(Z * N, 576, seed=23)
    rl = torch.zeros(Z, H, N, device="cuda")
    with pytest.raises(RuntimeError, match=r"rel_pose_amd: rp_emm_matches failed: bad shape \(RP error -1\)"):
        ro.emm_matches(torch.cat([qkv, qkv[:N]]), torch.zeros(3, H, N, device="cuda"), torch.zeros(3, H, N, device="cuda"), 3)
    from rel_pose_amd import _lib
    lib = _lib.load_readout()
    idx = torch.full((Z, H, N), -7, device="cuda", dtype=torch.int32)
    stat = torch.full((Z, H, N, 4), -7.0, device="cuda")
    P, b = ctypes.c_void_p, qkv.data_ptr()
    st = P(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(RuntimeError, match=r"rel_pose_amd: rp_emm_matches failed: misaligned pointer/stride \(RP error -2\)"):
        lib.rp_emm_matches(P(b + 4), P(b + 4 * 192), P(rl.data_ptr()), P(rl.data_ptr()), P(idx.data_ptr()), P(stat.data_ptr()), None,
                           Z, H, 576, 576, 0.125, 0, 0, st)
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((stat == -7.0).all())          # nothing ran


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture
def repeatable_cnn():
    """The CNN front-end goes through MIOpen, and at two images the solver it picks by default for resnet.layer2's 3 x 3 / 128 -> 128
    convolution is not repeatable from call to call (measured: layer2.0.conv2's output differs between two calls on bit-identical input,
    the map by 1.3e-4 of values up to 223; every layer in front of it repeats).  A bit-for-bit comparison of two runs from IMAGES therefore
    asks MIOpen for its repeatable solvers, as any PyTorch program that needs run-to-run identity does; with the flag all twelve
    convolutions it runs repeat.  Nothing of the readout or of this library depends on it."""
    keep, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    yield
    torch.backends.cudnn.deterministic = keep


def _oracle_scores(sd64, tok64):
    """the EMM's scores from oracle functions only: + pos_embed, five Blocks, LayerNorm, cross_attention's s1 / s2"""
    from oracle import relpose_oracle as O
    x = tok64 + sd64["fusion_transformer.pos_embed"]
    for l in range(5):
        x = O.block(sd64, "fusion_transformer.blocks.%d." % l, x)
    p = "fusion_transformer.blocks.5."
    xp = x.reshape(-1, 2, N, 192)
    n1w, n1b = sd64[p + "norm1.weight"], sd64[p + "norm1.bias"]
    _, _, parts = O.cross_attention(sd64, p + "cross_attn.", O.layernorm(xp[:, 0], n1w, n1b), O.layernorm(xp[:, 1], n1w, n1b),
                                    return_parts=True)
    return torch.stack([parts["s1"], parts["s2"]], 1).reshape(-1, H, N, N)      # image 2b: s1[b] = q_{2b+1} k_{2b}^T; image 2b+1: s2[b]


def test_model_correspondences_vs_oracle(ro):
    from oracle import relpose_oracle as O
    shapes = dict(O.vit_param_shapes())
    shapes.update(O.cnn_param_shapes())
    sd64 = O.make_state(shapes, torch.float64)
    m = _model().eval()
    tok = O.synthetic_tokens(4)
    fmap = tok.permute(0, 2, 1).contiguous().view(4, 192, 24, 24).cuda()
    E, _, _ = exponent(_oracle_scores(sd64, tok.double()))
    rows, cols = reduce_ref(E), reduce_ref(E.transpose(-1, -2))
    corr = m.correspondences_from_map(fmap, dense=True)
    assert corr.attention.shape == (4, H, N, N) and corr.row_idx.shape == (4, H, N) and corr.mutual.dtype == torch.bool
    e = rel(corr.attention, E.exp())
    report("readout_model_dense", A=e, near_ties_1e3=int((rows["ratio"] >= 1 - 1e-3).sum()) + int((cols["ratio"] >= 1 - 1e-3).sum()))
    assert e < 1e-4          # the project's R,t parity target
    check_indices(corr.row_idx, rows, 1e-3, 0.01, "model_rows")
    check_indices(corr.col_idx, cols, 1e-3, 0.01, "model_cols")
    assert torch.equal(corr.mutual, ro.mutual(corr.row_idx, corr.col_idx))
    assert torch.equal(corr.mutual.cpu(), torch.gather(corr.col_idx.cpu().long(), -1, corr.row_idx.cpu().long()) == torch.arange(N))
    lean = m.correspondences_from_map(fmap)
    assert lean.attention is None and all(torch.equal(a, b) for a, b in zip(lean[:5], corr[:5]))


def test_model_correspondences_from_images_and_module_state(ro, repeatable_cnn):
    from oracle import relpose_oracle as O
    from rel_pose_amd.se3 import SE3
    m = _model().eval()
    images = O.synthetic_images(1, 384, 384, key=78).cuda()
    Gs = SE3(torch.tensor([0, 0, 0, 0, 0, 0, 1.0]).repeat(1, 2, 1).cuda())
    intr = torch.tensor([[0.9 * 384, 0.8 * 384, 192.0, 192.0]]).repeat(1, 2, 1).contiguous().cuda()

    def forward():
        with torch.no_grad():
            return m(images, Gs, intrinsics=intr.clone())[0].data.clone()
    forward()                                                    # (warm-up: first calls load code objects and pick solvers)
    before, state = forward(), {k: v.clone() for k, v in m.state_dict().items()}
    buffers = {k: v.clone() for k, v in m.named_buffers()}
    corr = m.correspondences(images, dense=True)
    with torch.no_grad():
        fmap = m.cnn_map(images)[0]
    again = m.correspondences_from_map(fmap, dense=True)
    assert all(torch.equal(a, b) for a, b in zip(corr, again))
    assert not m.training and all(not mod.training for mod in m.modules())
    after = m.state_dict()
    assert set(after) == set(state) and all(torch.equal(after[k], state[k]) for k in state)
    assert all(torch.equal(v, buffers[k]) for k, v in m.named_buffers())
    assert torch.equal(forward(), before)
    assert all(p.grad is None for p in m.parameters())


def test_model_refusals(ro):
    fmap = torch.zeros(2, 192, 24, 24, device="cuda")
    m = _model()
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.correspondences_from_map(fmap)
    with pytest.raises(RuntimeError, match="eval"):
        m.correspondences(torch.zeros(1, 2, 3, 64, 64, device="cuda"))
    m.eval()
    _bf16_configuration(True)
    try:
        with pytest.raises(NotImplementedError):
            m.correspondences_from_map(fmap)
    finally:
        _bf16_configuration(False)
    with pytest.raises(ValueError, match="noess"):
        _model(noess="1").eval().correspondences_from_map(fmap)
    single = _model(use_single_softmax=True).eval()
    corr = single.correspondences_from_map(torch.rand(2, 192, 24, 24, device="cuda"))
    assert float((corr.row_stat[..., 1] - 1).abs().max()) < TAU    # single softmax: every row of A sums to one


def test_demo_matches_flag(tmp_path, capsys, repeatable_cnn):
    import numpy as np
    sys.path.insert(0, ROOT)
    import demo
    g = os.path.join(ROOT, "tests", "golden", "demo")
    argv = ["--img1", os.path.join(g, "matterport_1.png"), "--img2", os.path.join(g, "matterport_2.png")]
    torch.manual_seed(5)
    plain = demo.main(argv)
    out_plain = capsys.readouterr().out
    path = str(tmp_path / "matches.npz")
    torch.manual_seed(5)
    flagged = demo.main(argv + ["--matches", path])
    out_flagged = capsys.readouterr().out
    assert plain.tobytes() == flagged.tobytes()
    assert "matches" not in out_plain and out_flagged.startswith(out_plain)
    extra = out_flagged[len(out_plain):].splitlines()
    assert len(extra) == 1 and extra[0].startswith("mutual matches per head: ")
    f = np.load(path)
    shapes = {"row_idx": (2, H, N), "col_idx": (2, H, N), "mutual": (2, H, N), "row_stat": (2, H, N, 4), "col_stat": (2, H, N, 4)}
    for h in range(H):
        shapes.update({"match_xy0_h%d" % h: None, "match_xy1_h%d" % h: None, "match_conf_h%d" % h: None})
    assert set(f.files) == set(shapes)
    assert all(f[k].shape == s for k, s in shapes.items() if s is not None)
    assert f["row_idx"].dtype == np.int32 and f["mutual"].dtype == np.bool_
    counts = [int(c) for c in extra[0].split(": ")[1].split(" -> ")[0].split()]
    for h in range(H):
        n = int(f["mutual"][1, h].sum())
        assert counts[h] == n and f["match_xy0_h%d" % h].shape == (n, 2) and f["match_xy1_h%d" % h].shape == (n, 2)
        assert f["match_conf_h%d" % h].shape == (n,)
        xy = np.concatenate([f["match_xy0_h%d" % h], f["match_xy1_h%d" % h]])
        assert xy.size == 0 or (xy.min() > 0 and xy[:, 0].max() < 512 and xy[:, 1].max() < 384)      # the 384 x 512 the model saw
