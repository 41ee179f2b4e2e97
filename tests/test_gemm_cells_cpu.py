"""CPU proofs behind tests/test_gpu_gemm_cells.py (no GPU, no library): the operands of tests/_gemm_cells.py really make every partial
sum exact, a float32 matmul that is not ours reproduces the integer reference bit for bit, the Python mirror of rp_gemm's dispatch agrees
with ops.gemm_tile, the case table hits every cell the mirror says each group must hit, and the limb families populate the bf16 limbs they
claim."""
import collections

import pytest
import torch

from tests import _gemm_cells as G


def _distinct_operand_cases():
    seen = {}
    for c in G.table():
        seen.setdefault((c.family, c.M, c.N, c.K, c.batch, G.inexact(c), c.dact == 2, c.prec == 1, c.bias, c.res, c.colsum), c)
    return list(seen.values())


def test_every_partial_sum_is_exact():
    """sum |a| |b| (+ |bias| + |residual|; x M for column sums) on the case's power-of-two grid stays below 2^24: every product, every
    partial sum in any order, every slab, every exact epilogue intermediate and every column sum is an fp32 integer"""
    worst = collections.Counter()
    for c in _distinct_operand_cases():
        w, g = G.magnitude_bound(c)
        assert w < G.LIM, (G.name(c), w, g)
        worst[c.family] = max(worst[c.family], w)
        o = G.operands(c)
        for k in ("A", "B", "bias", "aux", "res"):
            assert int(o[k].abs().max()) < G.LIM
    assert worst["small_int"] >= G.K_LONG * 49           # the long-K case is in the table and is the tightest small_int case
    assert worst["limb_a"] < 1 << 23 and worst["limb_b"] < 1 << 23


def test_small_int_ranges_and_special_aux():
    c = G.mk("epi", "DRELU", 68, 60, 36, (0, 0), 0)
    o, v = G.operands(c), G.values(c)
    assert int(o["A"].min()) == -7 and int(o["A"].max()) == 7 and int(o["B"].min()) == -7 and int(o["B"].max()) == 7
    assert not torch.equal(o["A"][0, :36], o["A"][0, :36].t())
    assert int(o["bias"].abs().max()) <= 64 and int(o["res"].abs().max()) == 64 and int(o["aux"].abs().max()) == 64
    zero = v["aux"] == 0
    neg = zero & torch.signbit(v["aux"])
    assert int(neg.sum()) > 100 and int((zero & ~neg).sum()) > 100 and int((v["aux"] > 0).sum()) > 100
    assert torch.signbit(v["aux"].float())[neg].all() and torch.signbit(v["aux"].to(torch.bfloat16))[neg].all()
    g = G.mk("epi", "BIAS_GELU_PRE", 68, 60, 36, (0, 0), 0)
    pre = G.epilogue(g, G.product(g, G.values(g)), G.values(g), torch.float64)[0]
    assert torch.equal(pre * 64, (pre * 64).round()) and 0.5 < float(pre.std()) < 4.0      # multiples of 1/64 of order 1
    assert torch.equal(pre.float().double(), pre)


@pytest.mark.parametrize("family,prec", [("small_int", 0), ("small_int", 1), ("limb_a", 0), ("limb_a", 1), ("limb_b", 0), ("limb_b", 1),
                                         ("selector", 0)])
def test_plain_float32_matmul_is_exact(family, prec):
    """the premise on an implementation that is not ours: torch's CPU float32 matmul equals the int64 product, and the fp64 product the
    GPU tests use as reference equals it too"""
    for M, N, K in ((68, 60, 64), (64, 68, 64)) + (((68, 60, G.K_LONG),) if family == "small_int" else ()):
        c = G.mk("limb", "RAW", M, N, K, (0, 0), prec)._replace(family=family)
        o, v = G.operands(c), G.values(c)
        A, B = o["A"], o["B"]
        if prec == 1:
            A, B = G.bf16_round(A.double()).long(), G.bf16_round(B.double()).long()
            if family != "small_int":
                assert not (torch.equal(A, o["A"]) and torch.equal(B, o["B"]))                   # the rounding is seen ...
                big = o["B"] if family == "limb_b" else o["A"]
                trunc = (big.abs() >> 12 << 12) * big.sign()
                assert not torch.equal(trunc, B if family == "limb_b" else A)                    # ... and differs from truncation
        want = (A @ B.transpose(1, 2)).double() * 2.0 ** (o["ea"] + o["eb"])
        ref = G.product(c, v)
        assert torch.equal(ref, want)
        Af, Bf = (A.double() * 2.0 ** o["ea"]).float(), (B.double() * 2.0 ** o["eb"]).float()
        assert torch.equal(Af.double(), A.double() * 2.0 ** o["ea"])
        got = Af @ Bf.transpose(1, 2)
        assert got.dtype == torch.float32 and torch.equal(got.double(), want)
        assert torch.equal((Bf @ Af.transpose(1, 2)).transpose(1, 2).double(), want)            # another summation order


def _limbs(x):
    """x (fp32-exact) -> its three bf16 limbs by truncation, as csrc/gemm.hip splits them"""
    out, r = [], x.float()
    for _ in range(3):
        top = (r.view(torch.int32) & -65536).view(torch.float32)
        out.append(top)
        r = r - top
    assert bool((r == 0).all())
    return out


def test_limb_families_populate_their_limbs():
    c = G.mk("limb", "RAW", 68, 60, 64, (0, 0), 3)
    v = G.values(c._replace(family="limb_b"))
    b1, b2, b3 = _limbs(v["B"])
    assert bool((b1 != 0).all()) and float((b2 != 0).float().mean()) > 0.95 and float((b3 != 0).float().mean()) > 0.7
    assert bool((v["B"].abs() >= 2 ** 19).all()) and bool((v["B"].abs() < 2 ** 20).all()) and bool((v["B"].long() & 0xFF != 0).all())
    assert all(bool((_limbs(v["A"])[i] == 0).all()) for i in (1, 2))
    A = v["A"]
    assert bool(((A != 0).sum(-1) == 8).all()) and set(A.unique().tolist()) == {-1.0, 0.0, 1.0}
    used = (A[0] != 0).any(0)
    assert bool(used.all())                                                  # all 32 slots of both k-tiles
    assert bool(((A[0, :, :32] != 0).any(1) & (A[0, :, 32:] != 0).any(1)).float().mean() > 0.9)
    assert len({tuple(r.nonzero().flatten().tolist()) for r in A[0]}) > 60  # positions vary per row
    va = G.values(c._replace(family="limb_a"))
    a1, a2, a3 = _limbs(va["A"])
    assert float((a2 != 0).float().mean()) > 0.95 and float((a3 != 0).float().mean()) > 0.7
    assert bool(((va["B"] != 0).sum(-1) == 8).all()) and bool((va["B"][0] != 0).any(0).all())
    vs = G.values(c._replace(family="selector"))
    nz = vs["A"][0] != 0
    assert bool((nz.sum(1) == 1).all()) and bool(nz.any(0).all())            # one per row, every k hit
    assert torch.equal(nz.float().argmax(1), G.sigma(torch.arange(68), 64))
    for t in (vs["A"][0][nz], vs["B"].flatten()):
        l1, l2, l3 = _limbs(t)
        assert bool((l1 != 0).all()) and bool((l2 != 0).all()) and bool((l3 == 0).all())
        assert bool((l1.abs() >= 2 ** 15).all()) and bool((l2.abs() >= 16).all()) and bool((l2.abs() <= 240).all())
    P = G.product(c._replace(family="selector"), vs)
    assert bool((P != 0).all()) and bool((P.abs() < 2 ** 32).all()) and torch.equal(P.float().double(), P) and bool((P.long() % 256 == 0).all())
    vi = G.values(c)
    assert all(bool((_limbs(vi[k])[i] == 0).all()) for k in ("A", "B") for i in (1, 2))


def test_mirror_agrees_with_gemm_tile():
    from rel_pose_amd import ops
    for c in G.table():
        assert G.tile(c) == ops.gemm_tile(c.M, c.N, c.al, c.bl, G.has_aux(c) or c.res, c.prec), G.name(c)
        assert G.abi_ok(c) is None
    for lay in G.LAYOUTS:
        for p in G.PRECISIONS:
            for M, N, K in G._universe(lay):
                for mode in ("RAW", "RES"):
                    c = G.mk("main", mode, M, N, K, lay, p)
                    assert G.tile(c) == ops.gemm_tile(M, N, lay[0], lay[1], c.res, p)


def test_table_hits_every_required_cell():
    req, got = G.required(), G.hit()
    for group in ("main", "epi", "splitk", "order"):
        assert got[group] == req[group], (group, sorted(req[group] - got[group])[:5], sorted(got[group] - req[group])[:5])
    # listed explicitly: what the mirror reaches
    tiles = {k[2] for k in req["main"]}
    assert tiles == {(1, 1), (1, 2), (2, 1), (1, 3)}                         # (2,2): not reachable without RP_GEMM_TILE
    assert {(k[0], k[1]) for k in req["main"] if k[2] == (1, 3)} == {((0, 1), 0), ((1, 0), 0), ((1, 1), 0), ((1, 1), 1), ((1, 1), 3)}
    assert {k[3] for k in req["main"] if k[1] != 0} == {"reg"} and {k[3] for k in req["main"] if k[1] == 0} == {"reg", "dma"}
    assert len(req["main"]) == 4 * 3 * 2 + 4 * 2 * 3 + 3 * 2 + 2
    modes = {k[3] for k in req["epi"]}
    assert modes == {"RAW", "BIAS", "BIAS_RES", "RES", "BIAS_GELU", "BIAS_GELU_PRE", "BIAS_RELU", "DGELU", "DRELU", "GENERIC"}
    assert {k[4] for k in req["epi"] if k[3] == "GENERIC"} == {"G_RELU_NOBIAS", "G_GELU_RES", "G_DRELU_BIAS", "G_PRE_RELU", "G_PRE"}
    assert all(k[5] == "generic" for k in req["epi"] if k[0] == (1, 1) or k[3] == "GENERIC")
    assert {(k[5]) for k in req["epi"] if k[0] != (1, 1) and k[3] != "GENERIC"} == {"staged", "generic"}     # generic through N % 4 != 0
    assert not any(k[2] == (1, 3) for k in req["epi"] if k[3] in ("BIAS_RES", "RES", "DGELU", "DRELU"))      # aux / residual: TN <= 2
    classes = {(k[2], k[3]) for k in req["splitk"] if k[1] == 0}
    assert classes == {("reg", ("tail", 0)), ("reg", ("tail", 1)), ("reg", ("tail", 2)), ("dma", ("whole", 0)), ("dma", ("short", 0)),
                       ("dma", ("whole", 1)), ("dma", ("whole", 2))}
    assert {k[3] for k in req["splitk"] if k[1] != 0} == {("tail", 0), ("tail", 1), ("tail", 2), ("whole", 0), ("short", 0), ("whole", 1),
                                                         ("whole", 2)}
    assert {(k[2], k[4]) for k in req["order"] if k[1] == 0} == {((1, 3), False), ((2, 1), False), ((2, 1), True)}


def test_main_cells_are_ragged_in_every_direction():
    by = collections.defaultdict(lambda: [False, False, False])
    for c in G.cases_of("main"):
        key = ((c.al, c.bl), c.prec, G.tile(c), G.path(c))
        by[key] = [a or b for a, b in zip(by[key], G.ragged(c))]
    for (lay, p, t, path), (rm, rn, rk) in by.items():
        assert rm, (lay, p, t, path)
        assert rn or t == (1, 3), (lay, p, t, path)
        assert rk == (path == "reg"), (lay, p, t, path)
    long_k = [c for c in G.cases_of("main") if c.K == G.K_LONG]
    assert len(long_k) == 12 and {G.path(c) for c in long_k} == {"dma", "reg"}


def test_other_groups_cover_what_they_state():
    t = lambda g: G.cases_of(g)
    assert {(c.batch, c.M, c.N, c.K, c.mode, (c.al, c.bl)) for c in t("batch")} == {
        (b, M, N, K, m, lay) for b in (2, 5) for M, N, K in G.BATCH_SHAPES for m in ("RAW", "RES") for lay in ((0, 0), (0, 1))}
    cs = t("colsum")
    assert {(G.tile(c), c.mode) for c in cs} == {(tl, m) for tl in ((1, 1), (1, 2), (2, 1)) for m in G.COLSUM_MODES}
    assert all(G.staged(c) and c.M % (64 * G.tile(c)[0]) for c in cs)
    assert all(any(c.M <= (G.colsum_rows(c) - 1) * 32 * G.tile(c)[0] and G.tile(c) == tl for c in cs) for tl in ((1, 1), (1, 2), (2, 1)))
    io = t("iobf16")
    assert {c.io for c in io} == {1, 2, 3, 4, 7} and {G.tile(c) for c in io} == {(1, 1), (2, 1), (1, 2)} and all(c.prec == 1 for c in io)
    assert all(G.staged(c) or not c.io & 6 for c in io) and all(G.ragged(c)[0] and G.ragged(c)[1] for c in io)
    lb = t("limb")
    for lay in G.LAYOUTS:
        tiles3 = {G.tile(c) for c in lb if c.prec == 3 and (c.al, c.bl) == lay}
        assert tiles3 == {(1, 1), (1, 2), (2, 1)} | ({(1, 3)} if lay == (1, 1) else set())
        for tl in tiles3:
            assert {c.family for c in lb if c.prec == 3 and (c.al, c.bl) == lay and G.tile(c) == tl} == {"limb_a", "limb_b", "selector"}
        assert {c.family for c in lb if c.prec == 0 and (c.al, c.bl) == lay} == {"limb_a", "limb_b", "selector"}
        assert {c.family for c in lb if c.prec == 1 and (c.al, c.bl) == lay} == {"limb_a", "limb_b"}
    assert all(c.K == 64 for c in lb)
    for lay in G.LAYOUTS:
        d = G.defer_tasks(lay, 0)
        assert len(d) == 8 and len({(c.M, c.N, c.K, c.split) for c in d}) == 8 and 0 < sum(c.trans_c for c in d) < 8


def test_activation_references_and_bound_rule():
    """the fp32 restatement is a sane yardstick (non-zero error, far below the kernel-visible scale) and a wrong GELU form is outside the rule"""
    from tests import _norm_regimes as R
    for p, mode in ((0, "BIAS_GELU"), (1, "BIAS_GELU"), (0, "DGELU"), (1, "DGELU")):
        c = G.mk("epi", mode, 68, 60, 36, (0, 0), p)
        v = G.values(c)
        P = G.product(c, v)
        want, yard = G.epilogue(c, P, v, torch.float64)[1], G.epilogue(c, P, v, torch.float32)[1]
        other = G.epilogue(c, P, v, torch.float64, "erf" if G.form(c) == "tanh" else "tanh")[1]
        idx = {"all": torch.arange(want.numel())}
        one = torch.ones(want.numel())
        ok = R.judge("elem", yard.flatten(), yard.flatten(), want.flatten(), idx, scale=one)[0]
        bad = R.judge("elem", other.flatten(), yard.flatten(), want.flatten(), idx, scale=one)[0]
        assert ok["of_limit"] <= 1.0 / R.FACTOR + 1e-9 or ok["yard"] * R.FACTOR < R.FLOOR
        assert bad["of_limit"] > 10.0
