"""CPU proofs behind tests/test_gpu_conv_cells.py (no GPU, no library): the references of tests/_conv_cells.py equal fp64 F.conv2d, its
autograd and an int64 unfold-matmul; every operand family keeps every partial sum exact (sum |a| |b| < 2^24, the fp32 statistics chains
included); bf16 operands are bf16 numbers and the sparse expectations have at most 8 significant bits; a reference with exactly one of
the faults the old tolerances let through (a dropped product at a run boundary, truncation, round-half-up, a double rounding, the mask >=
for >, an activated pad column, a pixel counted twice, a rotation without the channel swap) differs from the right one on the chosen
operands; and the case table holds every cell required() derives."""
import pytest
import torch
import torch.nn.functional as F

from tests import _conv_cells as V

F64, BF = torch.float64, torch.bfloat16
SLOTS = (256, 512, 768)            # resident stem workgroups a device may report: the wrap case is sized from the device's own figure


def _case(kernel, form, family, N, H=None, W=None):
    g = V.GEOM[kernel]
    return V.Case(kernel, form, family, N, g[0] if H is None else H, g[1] if W is None else W)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _unfold_int(x, w, stride, pad):
    """int64 reference: im2col by F.unfold on exact small floats -> int64 matmul"""
    co, kh, kw, ci = w.shape
    cols = F.unfold(_nchw(x).double(), (kh, kw), padding=pad, stride=stride).round().long()       # [N, ci kh kw, L], channel-major
    wm = w.permute(0, 3, 1, 2).reshape(co, -1)                                                     # [co, ci kh kw]
    N, H, W, _ = x.shape
    oh, ow = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    return (wm @ cols).view(N, co, oh, ow).permute(0, 2, 3, 1)


@pytest.mark.parametrize("k,stride,pad,H,W", [(3, 1, 1, 9, 11), (7, 2, 3, 14, 18), (7, 2, 3, 13, 18), (5, 1, 0, 9, 9)])
def test_references_equal_conv2d_its_autograd_and_an_int64_unfold_matmul(k, stride, pad, H, W):
    x, w = V._ints((2, H, W, 5), -3, 3, 1, k), V._ints((6, k, k, 5), -7, 7, 2, k)
    want = _unfold_int(x, w, stride, pad)
    xd, wd = x.double(), w.double()
    ref = V.conv_ref(xd, wd, stride, pad)
    assert torch.equal(ref, want.double())
    xt, wt = _nchw(xd).clone().requires_grad_(True), _nchw(wd).clone().requires_grad_(True)
    y = F.conv2d(xt, wt, None, stride, pad)
    assert torch.equal(_nchw(ref), y)
    if pad == 3:                                                    # the stem's framed form: padding 0 on the framed image
        assert torch.equal(V.conv_ref(V.frame(xd), wd, stride, 0), ref)
    dy = V._ints(tuple(ref.shape), -3, 3, 3, k).double()
    y.backward(_nchw(dy))
    assert torch.equal(V.wgrad_ref(xd, dy, k, stride, pad), wt.grad.permute(0, 2, 3, 1))
    if stride == 1:
        assert torch.equal(V.conv_ref(dy, V.rot(wd), 1, k - 1 - pad), xt.grad.permute(0, 2, 3, 1))
    # exact in float32 as well, on an implementation that is not ours
    y32 = F.conv2d(_nchw(xd).float(), _nchw(wd).float(), None, stride, pad)
    assert torch.equal(y32.double(), y.detach())


def _sized(c, slots=512):
    if c.N is not None:
        return c
    blocks = lambda N, H, W: min(-(-V.stem_tiles(N, H, W) // V.STEM_SNW), slots)
    return c._replace(N=V.wrap_n(blocks, c.H, c.W))


def test_every_sum_is_below_two_to_the_24():
    worst = {}
    for c in V.table():
        c = _sized(c)._replace(N=V.WRAP_MAX_N) if c.N is None else c          # the wrap case at its largest admissible N
        if c.family == "sparse":
            continue
        if c.N == 37 and c.family != "dense":
            continue                                                           # (operand ranges do not depend on N)
        b = V.sum_bound(c._replace(N=min(c.N, 3)))
        if "wgrad" in c.kernel:
            b = b // min(c.N, 3) * c.N
        assert b < V.LIM, (V.name(c), b)
        worst[c.kernel] = max(worst.get(c.kernel, 0), b)
    assert worst["wgrad_f32"] == 37 * 3136 * 9 and worst["stem_wgrad_f32"] == 5 * 12544 * 9
    assert worst["c64_bf16"] == 576 * 16 * 31 and worst["stem_bf16"] == 147 * 15 * 31


@pytest.mark.parametrize("N", [1, 3, 37])
def test_sparse_weight_gradient_family(N):
    c = _case("wgrad_bf16", "dw", "sparse", N)
    o, v = V.operands(c), V.values(c)
    count = V.wgrad_ref(v["x"].abs(), v["dy"].abs())
    assert float(count.max()) <= 255 and float(count.min()) >= 1             # every output sums at least one and at most 255 products of +-1
    ref = V.wgrad_ref(v["x"], v["dy"])
    assert torch.equal(ref, ref.round()) and torch.equal(V.bf16_rne(ref).double(), ref)       # <= 8 significant bits: stored exactly
    for d in (-1.0, 1.0):                                                      # ... and so is the sum with any one +-1 product dropped
        assert torch.equal(V.bf16_rne(ref + d).double(), ref + d)
    assert set(o["x"].unique().tolist()) == {-1, 1} and set(o["dy"].unique().tolist()) == {-1, 0, 1}
    nz = (o["dy"] != 0).view(N, 56, 56, 64)
    assert bool((nz.sum(-1).flatten().unique() == torch.tensor([0, 4])).all())
    pix = nz.any(-1)                                                           # [N, 56, 56]
    assert bool(nz.any(0).any(0).any(0).all())                                 # every output channel
    assert bool(pix[:, 0].any()) and bool(pix[:, 55].any()) and bool(pix[:, :, 0].any()) and bool(pix[:, :, 55].any())
    strips = pix.view(N, 14, 4, 56)
    assert bool(strips[:, :, 0].any(-1).all()) and bool(strips[:, :, 3].any(-1).all())        # first and last row of EVERY strip
    flat = pix.view(N * 14, 224)
    for lo, hi in ((48, 63), (160, 175)):                                      # k-steps 3 and 10: pixels on both sides of the row change
        assert bool(flat[:, lo].any()) and bool(flat[:, hi].any()) and lo // 56 != hi // 56
    for t0, t1 in V.runs("wgrad_bf16", N):
        assert t0 < t1 and bool(flat[t0, 0]) and bool(flat[t1 - 1, 223])       # first and last pixel of every workgroup's run


def test_bf16_operands_are_bf16_numbers():
    for c in V.table():
        if not (c.kernel in ("c64_bf16", "wgrad_bf16", "stem_bf16", "stem_wgrad_bf16")) or (c.N or 99) > 3:
            continue
        v = V.values(c)
        ts = [v["x"], v["dy"]] + ([] if "wgrad" in c.kernel else [v["w"]]) + ([V.bn_on_load(v)] if c.form.startswith("bn") else [])
        for t in ts:
            assert torch.equal(t.float().to(BF).double(), t), V.name(c)


def test_fp32_statistics_chains_stay_exact():
    """conv3x3_bf16.hip and the stems add y and y^2 in fp32 per lane over a workgroup's run / a wave's tiles: the whole run's sum of y^2
    (an upper bound of every partial sum in it, of |y| too) stays below 2^24 on the dense_small / bn_exact_small operands"""
    seen = 0
    for c in V.table():
        if c.kernel not in V.FP32_STATS or "stats" not in c.form:
            continue
        for slots in (SLOTS if c.kernel.startswith("stem") else (None,)):
            cs = _sized(c, slots or 512)
            v = V.values(cs)
            y = V.stored(cs, V.reference(cs, v)["out"]).double()
            blocks = None if slots is None else min(-(-V.stem_tiles(cs.N, cs.H, cs.W) // V.STEM_SNW), slots)
            b = V.stat_group_bound(cs, y, blocks)
            assert 0 < b < V.LIM, (V.name(cs), b)
            assert torch.equal(y, V.reference(cs, v)["out"])                  # (small values: the stored bf16 is the exact value)
            seen += 1
    assert seen == 2 * 3 + 2 * 4 * len(SLOTS)


def test_wrap_case_is_sized_from_the_device():
    for slots, n in ((256, 3), (512, 6), (768, 8), (4096, None)):
        blocks = lambda N, H, W: min(-(-V.stem_tiles(N, H, W) // V.STEM_SNW), slots)
        assert V.wrap_n(blocks) == n
        if n:
            assert V.stem_tiles(n, 224, 224) > 8 * blocks(n, 224, 224) and V.stem_tiles(n - 1, 224, 224) <= 8 * blocks(n - 1, 224, 224)


def test_launch_mirror_at_37_images():
    assert [V.tiles_of(k, 37) for k in ("c64_f32", "c64_bf16", "wgrad_bf16", "wgrad_f32", "c128_f32/128")] == [1036, 518, 518, 2072, 259]
    assert all(V.seam(k, 37) == "multi" and V.seam(k, 1) == "single" for k in V.NS if not k.startswith("stem"))
    assert [V.tiles_of("stem_wgrad_f32", n) for n in (1, 3, 5)] == [112, 336, 560]
    assert [V.seam("stem_wgrad_f32", n) for n in (1, 3, 5)] == ["single", "multi", "multi"]
    assert [V.seam("stem_wgrad_bf16", n) for n in (1, 3, 5)] == ["single", "single", "multi"]
    for k in V.NS:                                                             # runs start and end inside an image at the multi-tile size
        n = V.NS[k][-1]
        tpi = V.GEOM[k][6]
        assert any(t0 % tpi and t1 % tpi for t0, t1 in V.runs(k, n)), k
    assert V.groups_of("c128_f32/128", 37) == 128 and V.groups_of("c128_f32/192", 37) == 80 and V.groups_of("c128_f32/128", 1) == 8


# ------------------------------------------------------------------------------------------------ roundings
def test_rounding_helpers():
    g = torch.Generator().manual_seed(5)
    t = torch.cat([torch.randint(-(1 << 20), 1 << 20, (20000,), generator=g).double(), torch.tensor([384.0, 385.0, 386.0, 387.0, 1.0, 0.0, -257.0, -258.0, -259.0])])
    assert torch.equal(V.bf16_rne(t), V.bf16_rne_int(t))                      # torch's conversion IS round to nearest even
    assert V.bf16_rne(torch.tensor([257.0, 259.0, 258.5])).tolist() == [256.0, 260.0, 258.0]
    assert V.bf16_trunc(torch.tensor([259.0, -259.0])).tolist() == [258.0, -258.0]
    assert V.bf16_half_up(torch.tensor([257.0, -257.0])).tolist() == [258.0, -258.0]
    assert V.bf16_double(torch.tensor([2057.0])).tolist() == [2048.0] and V.bf16_rne(torch.tensor([2057.0])).tolist() == [2064.0]


BF16_DENSE = [_case("c64_bf16", "plain", "dense", 1), _case("c64_bf16", "dx_fn", "dense", 1), _case("c64_bf16", "bn", "bn_exact", 1),
              _case("stem_bf16", "fwd", "dense", 1, 32, 32), _case("stem_bf16", "fwd", "dense", 2, 37, 44), _case("wgrad_bf16", "dw", "dense", 37)]


@pytest.mark.parametrize("c", BF16_DENSE, ids=V.name)
def test_mutant_roundings_differ(c):
    """truncation, round-half-up and a double rounding each store a different tensor than one rounding to nearest even -- and differ from
    one another; each within the 6e-3 of the maximum that used to be the test"""
    out = V.reference(c, V.values(c))["out"]
    right = V.bf16_rne(out)
    wrong = [V.bf16_trunc(out), V.bf16_half_up(out), V.bf16_double(out)]
    for i, m in enumerate(wrong):
        assert not torch.equal(m, right), i
        assert float((m.double() - out).abs().max() / out.abs().max()) < 6e-3
        for m2 in wrong[i + 1:]:
            assert not torch.equal(m, m2)
    ties = (right.double() - out).abs() * 2 == (V.bf16_trunc(out).double() - V.bf16_half_up(out).double()).abs()
    assert int((ties & (right.double() != out)).sum()) > 10 and int((V.bf16_double(out) != right).sum()) > 10


# ------------------------------------------------------------------------------------------------ the other mutants
@pytest.mark.parametrize("N", [3, 37])
def test_mutant_dropped_product_at_a_run_boundary(N):
    c = _case("wgrad_bf16", "dw", "sparse", N)
    o, v = V.operands(c), V.values(c)
    ref = V.wgrad_ref(v["x"], v["dy"])
    right = V.bf16_rne(ref)
    dy, x = v["dy"].view(-1, 64), V.frame(v["x"], 1)
    checked = 0
    for t0, t1 in V.runs("wgrad_bf16", N)[:: max(1, len(V.runs("wgrad_bf16", N)) // 16)]:
        for p in (t0 * 224, t1 * 224 - 1):                                    # first / last pixel of the run
            n, yy, xx = p // 3136, (p % 3136) // 56, p % 56
            co = int(dy[p].nonzero()[0])
            for r, s in ((1, 1), (0, 1), (2, 1), (1, 0), (1, 2)):
                if not (0 <= yy + r - 1 < 56 and 0 <= xx + s - 1 < 56):
                    continue
                mutant = ref.clone()
                mutant[co, r, s, 7] -= dy[p, co] * x[n, yy + r, xx + s, 7]
                assert not torch.equal(V.bf16_rne(mutant), right)
                checked += 1
    assert checked > 100


def test_mutant_mask_greater_or_equal():
    c = _case("c64_f32", "dx_bn", "bn_exact", 1)
    v = V.values(c)
    pre = (v["bn_x"] - v["mean"]) * (v["rstd"] * v["gamma"]) + v["beta"]
    zero = pre == 0
    assert 0.15 < float(zero.float().mean()) < 0.3                              # the planted share lands exactly on 0 ...
    flat = pre.view(-1, 64)
    z = zero.view(-1, 64)
    assert bool(((flat[1:] > 0) & z[:-1]).any()) and bool(((flat[1:] < 0) & z[:-1]).any())        # ... with both signs next to it
    assert bool((pre > 0).any(0).any(0).any(0).all()) and bool((pre < 0).any(0).any(0).any(0).all())
    dx = V.conv_ref(v["dy"], V.rot(v["w"]))
    right = V.reference(c, v)
    g_ge = torch.where(V.bn_mask(v, strict=False), dx, torch.zeros_like(dx))
    assert not torch.equal(g_ge.float(), right["out"].float())
    assert int((zero & (dx != 0)).sum()) > 1000 and bool((right["out"][zero] == 0).all())
    assert not torch.equal(V.bn_partials(g_ge, v), right["stats"])
    assert V.bn_chain_bound(c, v, dx) < V.LIM
    # fma(x - mean, rstd gamma, beta) is exact: fp32 arithmetic reproduces the fp64 value, fused or not
    f = lambda k: v[k].float()
    assert torch.equal(torch.addcmul(f("beta"), f("bn_x") - f("mean"), f("rstd") * f("gamma")).double(), pre)
    # the convention: torch.relu's gradient at an exact zero is 0, like the kernel's `> 0`
    t = torch.tensor([-1.0, -0.0, 0.0, 1.0], requires_grad=True)
    torch.relu(t).sum().backward()
    assert t.grad.tolist() == [0.0, 0.0, 0.0, 1.0]


def test_mutant_activated_pad_column():
    for fam, form in (("bn_exact", "bn"), ("bn_exact_small", "bn_stats")):
        c = _case("c64_bf16", form, fam, 1)
        o, v = V.operands(c), V.values(c)
        assert set(o["scale"].tolist()) == {0.5, -0.5, 1.0, -1.0, 2.0, -2.0} and int(o["shift"].min()) == -2 and int(o["shift"].max()) == 2
        assert int((o["shift"] > 0).sum()) >= 16 and int((o["shift"] < 0).sum()) >= 16
        right = V.reference(c, v)["out"]
        wrong = V.bn_on_load_pad_activated(v, v["w"])
        assert not torch.equal(V.bf16_rne(wrong), V.bf16_rne(right))
        inner = (slice(None), slice(1, 55), slice(1, 55))
        assert torch.equal(wrong[inner], right[inner])                         # the fault lives on the border only
        act = V.bn_on_load(v)
        assert bool((act == 0).any()) and bool((act > 0).any()) and torch.equal(act * 2, (act * 2).round())


def test_mutant_pixel_counted_twice():
    seams = 0
    for c in V.table():
        if "stats" not in c.form or (c.N or 99) > 3 or c.form == "dx_bn":
            continue
        v = V.values(c)
        r = V.reference(c, v)
        y = V.stored(c, r["out"]).double()
        flat = y.view(-1, y.shape[-1])
        tile = {"c64_f32": 112, "c64_bf16": 224, "c128_f32/128": 112, "c128_f32/192": 112}.get(c.kernel, 16)
        for p in (tile - 1, tile, flat.shape[0] - 1):                         # the pixels on both sides of the first tile seam, the last pixel
            twice = r["stats"] + torch.stack((flat[p], flat[p].square()))
            assert not torch.equal(twice[0], r["stats"][0]) and not torch.equal(twice[1], r["stats"][1]), (V.name(c), p)
            assert float(((twice - r["stats"]).abs() / torch.stack((flat.abs().sum(0), flat.square().sum(0))).clamp_min(1)).max()) < 1.0
            seams += 1
    assert seams >= 3 * 20
    c = _case("c64_f32", "dx_bn", "bn_exact", 1)
    v = V.values(c)
    r = V.reference(c, v)
    one = torch.zeros_like(r["out"])
    one[0, 1, 55] = r["out"][0, 1, 55]                                         # the last pixel of the first row pair
    assert bool((V.bn_partials(one, v) != 0).any(1).all())


@pytest.mark.parametrize("kernel,form", [("c64_f32", "dx"), ("c128_f32/128", "dx"), ("c64_bf16", "dx_fn")])
@pytest.mark.parametrize("family", ["impulse", "dense"])
def test_mutant_rotation_without_the_channel_swap(kernel, form, family):
    c = _case(kernel, form, family, 1)
    v = V.values(c)
    right = V.stored(c, V.reference(c, v)["out"])
    for wrong_filter in (V.rot_without_swap(v["w"]), v["w"].permute(3, 1, 2, 0).contiguous(), v["w"]):      # no swap; no rotation; neither
        assert not torch.equal(V.stored(c, V.conv_ref(v["dy"], wrong_filter)), right)


def test_impulse_family_names_tap_and_roles():
    for k, co, ci in ((3, 64, 64), (3, 192, 128), (7, 64, 3), (5, 24, 16)):
        w = V.impulse_filter(co, k, ci)
        assert int(w.min()) >= 1 and int(w.max()) <= 252 and torch.equal(w.double().to(BF).double(), w.double())
        per_pair = w.permute(0, 3, 1, 2).reshape(co * ci, -1)
        assert all(len(set(row.tolist())) == k * k for row in per_pair[:: max(1, co * ci // 200)])      # injective in the tap per (co, ci)
        if co == ci:
            assert not torch.equal(w, w.permute(3, 1, 2, 0))
    c = _case("c64_f32", "fwd", "impulse", 3)
    o, v = V.operands(c), V.values(c)
    assert int(o["x"].sum()) == len(set(V.impulse_positions(3, 56, 56))) and set(o["x"].unique().tolist()) == {0, 1}
    pos = set(V.impulse_positions(3, 56, 56))
    assert {(0, 0), (0, 55), (55, 0), (55, 55)} <= {(y, x) for _, y, x in pos} and {n for n, _, _ in pos} == {0, 1, 2}
    y = V.reference(c, v)["out"]
    n, yy, xx = 2, 30, 30                                                      # an interior impulse: the output around it IS the filter
    k = V.impulse_positions(3, 56, 56).index((n, yy, xx))
    ch = (7 * k + 3) % 64
    for r in range(3):
        for s in range(3):
            assert torch.equal(y[n, yy + 1 - r, xx + 1 - s], v["w"][:, r, s, ch])


def test_table_holds_every_required_cell():
    req = V.required()
    for slots in SLOTS:
        got = V.hit(slots)
        assert got >= req, sorted(req - got)[:8]
    assert len(req) == 2 * sum(len(V.FORMS[k]) for k in V.NS) + 2 * (2 * 4 + 1)
    assert {k for k, _, _ in req} == set(V.GEOM) and len(V.GEOM) == 10          # nine entry points; c128 at both output widths
    forms = {(k, f) for k, f, _ in req}
    for k, f in (("c64_f32", "dx_bn"), ("c64_f32", "dx_res"), ("c64_f32", "fwd_res_stats"), ("c128_f32/192", "fwd_bias_stats"),
                 ("c128_f32/128", "dx"), ("c64_bf16", "bn_stats"), ("c64_bf16", "dx_fn"), ("stem_f32", "refusal")):
        assert (k, f) in forms
    # a device without the wrap size must FAIL the GPU test, not lose the cell silently
    assert ("stem_f32", "fwd_stats", "wrap") not in V.hit(4096)
    for kernel, N, shape in V.REFUSALS:
        assert shape[1] % 2 == 1 and kernel in ("stem_f32", "stem_bf16")
