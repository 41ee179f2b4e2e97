"""The premises of tests/_block_cells.py, without a GPU: the partition mirror against a brute-force walk over the items, the slab mirror
against the figures of the launchers, sum |a| |b| < 2^24 at every stage of every family, the references against int64 / fp64 torch, the
two classes of the gelu_exact family, the tile layouts of the stored dS, and -- per fault class -- that a reference carrying exactly that
fault differs on these operands."""
import itertools

import pytest
import torch

from tests import _block_cells as B
from tests import _gemm_cells as G

F64 = torch.float64
BIG_M = 2735          # stand-in for the device-dependent M of the N = 768 case (43 tiles, ragged)


@pytest.mark.parametrize("grid", (256, 512, 768))
def test_partition_mirror_matches_a_walk_over_the_items(grid):
    seen = set()
    for nchunk, tiles in itertools.product((24, 1, 6, 18, 32), list(range(1, 70)) + [grid // 24 * k + d for k in (1, 2, 3) for d in (-1, 0, 1)]
                                           + [grid + d for d in (-1, 0, 1, 7)]):
        g = min(grid, tiles * nchunk)
        share, mid, cross = B.brute_force(tiles, nchunk, g)
        assert torch.equal(B.sharers(tiles, nchunk, g), share), (tiles, nchunk, g)
        assert B.range_classes(tiles, nchunk, g)[:2] == (mid, cross), (tiles, nchunk, g)
        base, rem = B.split(tiles * nchunk, g)
        assert base * g + rem == tiles * nchunk and sum(B.range_of(b, base, rem)[1] for b in range(g)) == tiles * nchunk
        if nchunk == 24:
            seen |= B.tile_classes(tiles, nchunk, g)
    # every class the GPU cases are built to reach exists at every slot count
    assert {"owner", "two", "all"} <= seen, seen
    # fewer items than slots: one chunk per workgroup, every tile shared by all of its chunks
    assert B.tile_classes(5, 24, 120) == {"all"} and B.range_classes(5, 24, 120) == (True, False, 1)
    # a whole number of tiles per range: nothing is shared and no fix-up runs
    assert B.tile_classes(2 * grid, 24, grid) == {"owner"} and B.range_classes(2 * grid, 24, grid)[:2] == (False, True)


def test_smallest_m_finds_a_two_way_shared_tile_next_to_an_owned_one():
    for slots, rows in ((256, 192), (768, 64)):
        grid_of = lambda M: min(slots, -(-M // rows) * 24)
        want = lambda t, g: {"owner", "two"} <= B.tile_classes(t, 24, g)
        M = B.smallest_m(rows, 24, grid_of, want, ragged=5)
        t = -(-M // rows)
        # (below `slots` tiles base is 23 and the first rem ranges, one item longer, own whole tiles while rem >= 24 - t)
        assert slots * 23 // 24 <= t <= slots + 1 and {"owner", "two"} <= B.tile_classes(t, 24, slots)
        assert not {"owner", "two"} <= B.tile_classes(t - 1, 24, grid_of((t - 1) * rows))
        share = B.brute_force(t, 24, slots)[0]
        assert int((share == 1).sum()) >= 1 and int((share == 2).sum()) >= 1


def test_slab_mirror():
    assert B.dw_slabs(8224, 192, 32) == (129, 2, 1) and B.dw_slabs(2592, 576, 32) == (41, 2, 1) and B.dw_slabs(2080, 768, 32) == (33, 2, 1)
    assert [B.dw_smallest_m(N, 32, 2, 1) for N in B.DW_NS] == [8224, 2592, 2080]
    assert B.dw_slabs(64, 192, 32) == (2, 1, 1) and B.dw_slabs(96, 576, 32) == (3, 1, 1) and B.dw_slabs(160, 768, 32) == (5, 1, 1)
    assert B.dw_slabs(64, 192, 64) == (2, 1, 0)                      # the bf16 kernel at its minimum: an empty second slab
    for N, sr, M in itertools.product(B.DW_NS, (32, 64), (64, 128, 192, 320, 2112, 4160, 8256, 16448, 32832)):
        rows = B.dw_slab_rows(M, N, sr)
        sp, per, last = B.dw_slabs(M, N, sr)
        assert len(rows) == sp >= 2 and rows[0][0] == 0 and rows[-1][1] == M and all(a[1] == b[0] for a, b in zip(rows, rows[1:]))
        assert all(m1 - m0 == per * sr for m0, m1 in rows[:-1]) and rows[-1][1] - rows[-1][0] == last * sr
        assert sp <= 8 * (32 // (N // 192)) or sp == 2               # never more than one round of workgroups
    assert B.dw_slabs(B.dw_smallest_m(192, 32, 3, 1), 192, 32)[1:] == (3, 1)


def _lcases():
    for form, prec in itertools.product(B.LFORMS, (0, 1)):
        if form == "ln":
            continue
        for fam, (M, N) in itertools.product(B.linear_family(form, prec, 0), B.linear_shapes(BIG_M)):
            yield B.LCase(form, M, N, prec, 0, fam)


def test_linear_rows_premises():
    n = 0
    for c in _lcases():
        o = {k: v.double() for k, v in B.linear_operands(c.form, c.fam, c.M, c.N).items()}
        assert B.linear_bound(c, o) < B.LIM, B.lname(c)
        y, pre, cs = B.linear_reference(c, o)
        # the reference is an integer computation: int64 agrees
        oi = B.linear_operands(c.form, c.fam, c.M, c.N)
        xi = G.bf16_round(oi["x"].double()).long() if c.prec == 1 else oi["x"]
        P = xi @ oi["w"].t()
        if c.form == "plain":
            assert torch.equal(y.long(), P) and bool((y == y.round()).all())
        if c.form in ("gelu_pre", "gelu_res"):
            z, s, only = B.gelu_exact_classes(pre)
            assert only and (z >= 0.2 and s >= 0.2 or c.M * c.N < 4096), (B.lname(c), z, s)
            assert float(pre.max()) <= 2040                          # 8 significant bits: a bf16-stored y holds it exactly
            assert torch.equal(pre.long(), P + oi["bias"])
            # fp64 GELU of these values is the identity to within fp32's half ulp
            ex = torch.nn.functional.gelu(pre)
            assert bool(((ex - pre).abs() <= pre.abs() * 2.0 ** -25).all())
        if c.form == "dact_cs":
            z, s, only = B.gelu_exact_classes(o["aux"])
            assert only and (z >= 0.2 and s >= 0.2 or c.M * c.N < 4096) and float(o["aux"].max()) <= 64
            assert bool((2 * y == (2 * y).round()).all()) and cs.shape == (-(-c.M // 64), c.N)
            g = o["aux"].clone().requires_grad_(True)
            torch.nn.functional.gelu(g).sum().backward()
            big = o["aux"] >= 8
            assert bool(((g.grad - 1).abs()[big] < 2.0 ** -25).all()) and bool((g.grad[~big] == 0.5).all())
        n += 1
    assert n > 100


def test_selector_weights_select_one_column_per_unit_and_cover_every_column():
    for M, N in B.linear_shapes(BIG_M):
        o = B.linear_operands("ln", "selector", M, N)
        assert bool(((o["w"] != 0).sum(1) == 1).all())
        if N >= 192:
            assert len(set(o["k"].tolist())) == 192
        xn = torch.randn(M, 192, dtype=F64)
        assert torch.equal(xn @ o["w"].t(), o["wv"] * xn[:, o["k"]])          # one product, exact zeros: exact for ANY activations
        assert bool((o["wv"].abs().log2() == o["wv"].abs().log2().round()).all())


def test_const_rows_give_beta_back():
    """sum of 192 copies of c, times fl(1/192), is c in fp32 for every row constant: x - mean == 0 and the LayerNorm output is beta"""
    for c in B.CONST_ROW_VALUES:
        s = torch.zeros((), dtype=torch.float32)
        for _ in range(192):
            s = s + torch.tensor(float(c), dtype=torch.float32)
        assert float(s * torch.tensor(1.0 / 192, dtype=torch.float32)) == float(c)


def test_mlp_premises():
    for M in (1, 150, 3000):
        o = {k: v.double() for k, v in B.mlp_fwd_operands(M).items()}
        hmax, ymax = B.mlp_fwd_bound(o)
        assert hmax <= 2040 and ymax < B.LIM
        y, hpre, h = B.mlp_fwd_reference(o, M)
        z, s, only = B.gelu_exact_classes(hpre)
        assert only and z >= 0.2 and s >= 0.2, (z, s)
        oi = B.mlp_fwd_operands(M)
        hi = oi["w1"] @ oi["beta"] + oi["b1"]
        assert torch.equal(y[0].long(), oi["w2"] @ hi + oi["b2"] + oi["c"][0])
        ref = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(o["beta"], o["w1"], o["b1"])), o["w2"], o["b2"])
        assert float((ref + o["c"][0] - y[0]).abs().max()) < 1e-3
        # the permuted / chunk-major second weight holds the same numbers
        w2 = o["w2"]
        assert torch.equal(B.second_weight(w2, False)[:, torch.argsort(B.unit_perm())], w2)
        assert torch.equal(B.second_weight(w2, True).permute(1, 0, 2).reshape(192, 768), B.second_weight(w2, False))
        assert sorted(B.unit_perm().tolist()) == list(range(768))
        for prec in (0, 1):
            b = {k: v.double() for k, v in B.mlp_bwd_operands(M).items()}
            dhp, dxn, cp = B.mlp_bwd_reference(b, M, prec)
            z, s, only = B.gelu_exact_classes(B.periodic(b["hpre"], M))
            assert only and z >= 0.2 and s >= 0.2
            d2 = G.bf16_round(dhp) if prec else dhp
            assert float((d2.abs() @ b["w1t"].abs().t()).max()) < B.LIM and float(cp.abs().max()) < B.LIM
            assert float((B.periodic(b["dy"], M).abs() @ b["w2t"].abs().t()).max()) < B.LIM
            assert bool((2 * dhp == (2 * dhp).round()).all()) and bool((2 * dxn == (2 * dxn).round()).all())
    # autograd agrees (fp64, precision 0)
    b = {k: v.double() for k, v in B.mlp_bwd_operands(40).items()}
    hp = b["hpre"].clone().requires_grad_(True)
    xn = torch.zeros(40, 192, dtype=F64, requires_grad=True)
    yy = torch.nn.functional.gelu(hp + xn @ b["w1t"]) @ b["w2t"]
    yy.backward(b["dy"])
    dhp, dxn, _ = B.mlp_bwd_reference(b, 40, 0)
    assert float((hp.grad - dhp).abs().max()) < 1e-3 and float((xn.grad - dxn).abs().max()) < 1e-2


@pytest.mark.parametrize("fam", B.DW_FAMILIES)
def test_dw_premises(fam):
    for N, M in itertools.product(B.DW_NS, (64, 160, 2112)):
        a, b = B.dw_values(fam, M, N)
        ai, bi, ea, eb = B.dw_operands(fam, M, N)
        # (in units of the operands' common power of two, as tests/_gemm_cells.py's magnitude_bound)
        assert B.dw_bound(ai.double(), bi.double()) < B.LIM and B.dw_bound(ai.double(), G.bf16_round(bi.double())) < B.LIM
        slabs = B.dw_reference(a, b, B.dw_slab_rows(M, N, 32))
        assert torch.equal(slabs.sum(0), (ai.t() @ bi).double() * 2.0 ** (ea + eb))
        assert torch.equal(slabs.sum(0), B.dw_reference(a, b, B.dw_slab_rows(M, N, 64)).sum(0))
        if fam == "row_coded":
            assert bool(((a != 0).sum(1) == N // 192).all()) and int(b.min()) >= 1 and int(b.max()) <= 127
        if fam == "sel16":
            assert bool(((a != 0).sum(0) == 1).all())


# ------------------------------------------------------------------------------------------------ the tests bite
def _old_metric(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


def test_fault_row_dropped_from_a_slab():
    M, N = 8224, 192
    rows = B.dw_slab_rows(M, N, 32)
    for fam in ("row_coded", "small_int"):
        a, b = B.dw_values(fam, M, N)
        assert not torch.equal(B.dw_reference(a, b, rows, "row_dropped"), B.dw_reference(a, b, rows))
    # on randn at the size the suite used (ops.linear_dw: M >= 4096; here 73776 tokens) the same fault is inside the bf16 tolerance
    g = torch.Generator().manual_seed(1)
    M = 73776
    a, b = torch.randn(M, N, generator=g, dtype=F64), torch.randn(M, 192, generator=g, dtype=F64)
    assert _old_metric(a.t() @ b - torch.outer(a[0], b[0]), a.t() @ b) < 2e-2


def test_fault_truncation_for_round_to_nearest_even():
    c = B.LCase("plain", 65, 192, 1, 0, "x12")
    o = {k: v.double() for k, v in B.linear_operands(c.form, c.fam, c.M, c.N).items()}
    good, bad = B.linear_reference(c, o)[0], B.linear_reference(c, o, "truncate")[0]
    assert float((good != bad).double().mean()) > 0.9
    g = torch.Generator().manual_seed(2)
    r = dict(x=torch.randn(65, 192, generator=g, dtype=F64), w=torch.randn(192, 192, generator=g, dtype=F64))
    assert _old_metric(B.linear_reference(c, r, "truncate")[0], r["x"] @ r["w"].t()) < 2e-2
    b = {k: v.double() for k, v in B.mlp_bwd_operands(150).items()}
    assert not torch.equal(B.mlp_bwd_reference(b, 150, 1)[1], B.mlp_bwd_reference(b, 150, 1, fault="truncate")[1])


def test_fault_partial_added_twice_and_units_in_the_wrong_order():
    o = {k: v.double() for k, v in B.mlp_fwd_operands(150).items()}
    y = B.mlp_fwd_reference(o, 150)[0]
    for fault in ("partial_twice", "unit_order"):
        assert float((B.mlp_fwd_reference(o, 150, fault)[0] != y).double().mean()) > 0.5, fault
    # a permutation inside a chunk keeps the column sums of w2 and the sum of h: on randn it only moves mass between similar columns
    assert float(B.mlp_fwd_reference(o, 150, "unit_order")[2].sum()) == float(B.mlp_fwd_reference(o, 150)[2].sum())


def test_fault_column_sum_counts_a_row_past_m():
    c = B.LCase("dact_cs", 65, 192, 0, 0, "small_int")
    o = {k: v.double() for k, v in B.linear_operands(c.form, c.fam, c.M, c.N).items()}
    good, bad = B.linear_reference(c, o)[2], B.linear_reference(c, o, "colsum_past_m")[2]
    assert torch.equal(good[0], bad[0]) and float((good[1] != bad[1]).double().mean()) > 0.5


def test_fault_residual_added_before_gelu():
    """GELU(pre + res) instead of GELU(pre) + res: pre + res leaves the family's two exact classes (it goes negative), so the outputs
    differ almost everywhere; the `gelu_res` form of rp_linear_rows192 is the cell that sees it"""
    c = B.LCase("gelu_res", 65, 192, 0, 0, "gelu_exact")
    o = {k: v.double() for k, v in B.linear_operands(c.form, c.fam, c.M, c.N).items()}
    good, bad = B.linear_reference(c, o)[0], B.linear_reference(c, o, "res_before_gelu")[0]
    assert float((good != bad).double().mean()) > 0.3


def test_mlp_selector_family():
    for M, shift in ((1, 0), (150, 1), (3000, 3)):
        o = B.mlp_selector_operands(M, shift)
        assert bool(((o["w1"] != 0).sum(1) == 1).all()) and bool(((o["w2"] != 0).sum(1) == 1).all())
        assert len(set(o["k1"].tolist())) == 192
        xn, h = torch.randn(7, 192, dtype=F64), torch.randn(7, 768, dtype=F64)
        assert torch.equal(xn @ o["w1"].t(), o["wv1"] * xn[:, o["k1"]]) and torch.equal(h @ o["w2"].t(), o["wv2"] * h[:, o["u2"]])
    units = set()
    for shift in range(4):
        units |= set(B.mlp_selector_operands(150, shift)["u2"].tolist())
    assert units == set(range(768))


def test_ds_tile_layouts_and_the_swapped_index_fault():
    for layout in ("acc", "runs"):
        off = B.ds_offsets(layout)
        assert sorted(off.flatten().tolist()) == list(range(576 * 576))            # a bijection onto the image
        assert bool((off // 1024 == (torch.arange(576)[:, None] // 32) * 18 + torch.arange(576)[None, :] // 32).all())
    r, lane = 9, 37                                                                 # the header's formulas, the other way round
    i, j = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), lane & 31
    assert int(B.ds_offsets("acc")[i, j]) == r * 64 + lane and int(B.ds_offsets("runs")[5, 7]) == ((5 >> 2) * 32 + 7) * 4 + (5 & 3)
    Z, H = 2, 3
    ds = B.ds_code(Z * H).double()
    assert not torch.equal(ds, ds.transpose(1, 2)) and not torch.equal(ds[0], ds[1]) and int(ds.abs().max()) == 7
    for bits12 in (False, True):
        b = G.bf16_round(B.ds_b(Z, H, bits12, 1).double())
        unit = 16 if bits12 else 1                  # 12 bits rounded to bf16's 8: every operand, product and sum is a multiple of 16
        assert bool((b % unit == 0).all())
        tot = torch.einsum("zhij,zjhd->zihd", ds.abs().view(Z, H, 576, 576), b.abs().view(Z, 576, H, 64)).reshape(Z * 18, 32, H * 64)
        assert float(tot.sum(1).max()) < B.LIM * unit               # the column sums over 32 rows, hence every out as well
    b = B.ds_b(Z, H, False, 1).double()
    good = B.ds_reference(ds, b, Z, H, 1)[0]
    assert torch.equal(good.long(), B.ds_reference(B.ds_code(Z * H), B.ds_b(Z, H, False, 1), Z, H, 1)[0])      # int64 agrees
    for layout in ("acc", "runs"):
        # what a kernel that swaps (i, j) inside a tile would read from the correctly placed image
        img = B.ds_place(ds, layout)
        seen = img[:, B.ds_offsets(layout, swapped=True).flatten()].view(Z * H, 576, 576)
        assert torch.equal(img[:, B.ds_offsets(layout).flatten()].view(Z * H, 576, 576), ds)
        bad = B.ds_reference(seen, b, Z, H, 1)[0]
        assert float((good != bad).double().mean()) > 0.5
    # on randn the swap is gross too (it is no small-error fault): the old tolerance saw it at the sizes it ran, the new cells see it at
    # every Z, H, b_xor and in the column sums


def test_mlp_bwd_ln_premises():
    for M in (1, 181, 700):
        b = {k: v.double() for k, v in B.mlp_bwd_ln_operands(M).items()}
        xhat = B.periodic(b["xc"], M) * 2.0 ** B.periodic(b["rexp"], M)[:, None]
        assert bool((2 * xhat == (2 * xhat).round()).all()) and float(xhat.abs().max()) <= 4
        for prec in (0, 1):
            dhp, dxn, _ = B.mlp_bwd_reference(b, M, prec)
            terms = torch.cat([dxn * xhat, dxn, B.periodic(b["dy"], M)], 1)
            assert bool((4 * terms == (4 * terms).round()).all())
            T = -(-M // 192)
            pad = torch.zeros(T * 192, 576, dtype=F64)
            pad[:M] = terms.abs()
            assert float(pad.view(T, 192, 576).sum(1).max()) * 4 < B.LIM          # a whole tile's sums, in units of 1/4
            assert float((G.bf16_round(dhp).abs() @ b["w1t"].abs().t()).max()) * 2 < B.LIM
            share = torch.tensor([1] + [2] * (T - 1))
            part = B.ln_part_reference(dxn, xhat, B.periodic(b["dy"], M), share)[0]
            assert part.shape == (4 * T, 576) and torch.equal(part.view(T, 4, 576).sum(1), pad.view(T, 192, 576).sum(1).sign() * 0 + torch.cat(
                [terms, torch.zeros(T * 192 - M, 576, dtype=F64)]).view(T, 192, 576).sum(1))
            assert bool((part[1:4] == 0).all())


def test_dx_lnbwd_premises():
    for M in (53, 187):
        o = {k: v.double() for k, v in B.dx_lnbwd_operands(M).items()}
        assert torch.equal(G.bf16_round(o["dy"]), o["dy"]) and torch.equal(G.bf16_round(o["wt"]), o["wt"])
        dxn = o["dy"] @ o["wt"].t()
        assert torch.equal(dxn.long(), B.dx_lnbwd_operands(M)["dy"] @ B.dx_lnbwd_operands(M)["wt"].t())
        xhat = o["xc"] * 2.0 ** o["rexp"][:, None]
        part = B.dx_lnbwd_part((o["dy"].abs() @ o["wt"].abs().t()), xhat.abs(), o["add"].abs(), 64)
        assert float(part.max()) * 2 < B.LIM and part.shape == (-(-M // 64), 3, 192)
        assert B.dx_lnbwd_part(dxn, xhat, None, 64).shape[1] == 2
