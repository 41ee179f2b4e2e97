"""Exact-arithmetic operands, references, a mirror of rp_gemm's dispatch and the case table for the rp_gemm cell tests
(csrc/gemm.hip, gemm_dma.hip, gemm_common.h).  torch only, no GPU and no library at import: tests/test_gemm_cells_cpu.py proves the premises
on the CPU, tests/test_gpu_gemm_cells.py runs the table on the device.

The method.  Operands are chosen so that every product and every partial sum, in ANY summation order, is an integer times one power of
two and below 2^24 in magnitude (bounded through sum |a| |b|).  fp32 accumulation is then exact, and so are the bf16 MFMA's fp32
accumulation, the split-K slabs, the fixed-order reduce and the column sums: the kernel's output must equal the integer reference BIT FOR
BIT (torch.equal), with no tolerance and no yardstick, and a single wrong element anywhere is seen.  Operands are kept as int64 tensors
with a binary exponent (value = int * 2^e); the references multiply them in fp64, where integers of this size are exact (the CPU test
checks that against an int64 matmul).

Families
  small_int   A, B iid integers in [-7, 7]; bias / residual / aux integers in [-64, 64].  Exact in bf16, limbs 2 and 3 are zero: the
              workhorse of every cell at precisions 0, 1 and 3.  ReLU' cells: aux holds exact zeros and -0.0.  GELU / GELU' cells: B is
              scaled by 2^-6 and bias / aux by 2^-4, so the pre-activations are multiples of 1/64 of order 1 (still exact).
  limb_b      A ternary {-1, 0, 1} with exactly 8 non-zeros per row at positions that vary per row and cover all 64 k of two k-tiles;
              B 20-bit integers in [2^19, 2^20) with random sign and a non-zero low byte: limbs of 8 + 8 + 4 bits.  |sums| < 2^23.
              Precision 3 must equal the integer product: pins the limb products (0,0), (0,1), (0,2) and the limb weights.  Precision 1
              must equal the same sum over operand.to(bfloat16): round-to-nearest-even of the operands, not truncation.
  limb_a      the mirror image: A 20-bit, B ternary -- products (0,0), (1,0), (2,0).
  selector    A has one non-zero per row, at k = sigma(m) = (5 m + 3) mod K (M >= K: every k is hit); that value and every entry of B
              are 16-bit integers 2^8 h + 16 l, h in [128, 255], l in [1, 15]: limb 1 = 2^8 h, limb 2 = 16 l, limb 3 = 0.  Each output
              is ONE product, a multiple of 2^8 below 2^32 (24 significant bits, exact), and non-zero in limb product (1,1) -- the one
              the other families cannot see.  Precisions 0 and 3.

Only the pointwise activations are inexact: GELU / GELU' outputs (and the GELU' column sums) are judged element by element against fp64
GELU of the EXACT pre-activation under tests/_norm_regimes.py's bound rule (8 x the error of the plain fp32 torch restatement under
elem_rel with scale 1, floor 4 * 2^-23; a bf16-stored C gets that module's one bf16 rounding on top); erf form for precisions 0 and 3,
sigmoid ("tanh") form for precision 1.  pre_out itself is exact.

Inputs that must not be read: every [rows, cols] operand is stored with ld = cols + 4 (bf16 operands too) and NaN in the pad columns,
batches leave a NaN gap of 8 elements between problems, bias has 4 NaN behind it; C / pre_out / column-sum partials / the workspace are
NaN before the call, ldc = N + 4 (the next multiple of 4 above N when N % 4 != 0) and the pad must still be NaN afterwards.

The mirror (tile, path, epi_mode, staged, order, split_class -> cell) restates the dispatch of rp_gemm in Python; its tile must agree with
ops.gemm_tile.  What the mirror finds, over the extents below:
  * tiles (1,1), (1,2), (2,1) and (1,3) are reachable.  (2,2) is NOT: for M > 64 the selection overrides it with (2,1) or (1,3) at every
    precision; like (2,3) it is reachable only through the once-per-process RP_GEMM_TILE tuning variable and is left out.
  * (1,3) needs N % 192 == 0, so it has no ragged N tile; at precisions 1 and 3 it exists for the [K,M]x[K,N] layout only.
  * the register-staged fp32 loop at K % 32 == 0 is reachable only through RP_GEMM_NO_DMA (left out) or with M < 4 or N < 4 (in the
    table); the same loop runs for every K % 32 != 0 case.
  * the LayerNorm-backward epilogue is inexact by nature and covered by tests/test_gpu_norm_regimes.py.

Groups of the table (table(); required(): what each group must contain, derived from the mirror independently of the table):
  main      split_k = 1, raw: every (layout, precision, tile, path), each with ragged M, ragged N (not (1,3)) and, register path, ragged K;
            one K = 2688 case per (layout, precision).
  epi       every epilogue mode (staged ones, the four documented generic combinations and pre_out alone) on every tile it reaches, also
            through N % 4 != 0 and layout (1,1) (both generic), precisions 0 and 1, register and DMA loops.
  splitk    split_k in {2, 3, 5, 9, 12} x K in {36, 64, 100, 160}: whole splits, a short or ragged last split, one and two-or-more trailing
            empty splits in both loops; raw, two epilogues in the reduce, trans_c; ldc = N + 4.  `defer`: 8 deferred products of different
            shapes finished by one rp_splitk_reduce_multi.
  order     ntm = 17 (the XCD swizzle with an early return) for a (1,3) and a TM = 2 tile, both loops, with and without colsum_part.
  batch     batch in {2, 5}, gapped strides, layouts (0,0) and (0,1), raw and residual.
  colsum    tiles (1,1), (1,2), (2,1), M ragged so that a wave row lies past M; BIAS, DGELU, DRELU, RES.
  iobf16    bits 1, 2, 4, 1|2, 1|2|4 on the staged modes the ABI allows; tiles (1,1), (2,1), (1,2), ragged M and N.
  limb      limb_a, limb_b, selector on every (layout, tile) of precision 3 and one tile per layout at precisions 0 and 1; K = 64."""
import collections
import functools
import itertools

import torch

from tests import _norm_regimes as R

LIM = 1 << 24
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))
PRECISIONS = (0, 1, 3)
MS = (1, 3, 4, 60, 64, 68, 128, 132, 1028, 2052)
NS = (4, 60, 64, 68, 128, 192, 196, 384)
NS_B0 = (1, 3, 5, 7, 70)
KS = (4, 28, 32, 36, 64, 96, 100, 160)
K_LONG = 2688
SPLITS = (2, 3, 5, 9, 12)
SPLIT_KS = (36, 64, 100, 160)
GAP = 8

_FIELDS = dict(group="main", family="small_int", M=0, N=0, K=0, al=0, bl=0, prec=0, bias=False, pre=False, act=0, dact=0, res=False,
               split=1, trans_c=False, batch=1, colsum=False, io=0, mode="RAW")
Case = collections.namedtuple("Case", list(_FIELDS), defaults=list(_FIELDS.values()))

# name -> flags; the first nine are the modes the `if` ladder of rp_gemm names, the G_* ones fall to EPI_GENERIC
MODES = collections.OrderedDict(
    RAW={}, BIAS=dict(bias=True), BIAS_RES=dict(bias=True, res=True), RES=dict(res=True), BIAS_GELU=dict(bias=True, act=1),
    BIAS_GELU_PRE=dict(bias=True, act=1, pre=True), BIAS_RELU=dict(bias=True, act=2), DGELU=dict(dact=1), DRELU=dict(dact=2),
    G_RELU_NOBIAS=dict(act=2), G_GELU_RES=dict(bias=True, act=1, res=True), G_DRELU_BIAS=dict(dact=2, bias=True),
    G_PRE_RELU=dict(bias=True, pre=True, act=2), G_PRE=dict(bias=True, pre=True))


def mk(group, mode, M, N, K, lay, prec, **kw):
    return Case(group=group, mode=mode, M=M, N=N, K=K, al=lay[0], bl=lay[1], prec=prec, **dict(MODES[mode], **kw))


def name(c):
    s = "%s/%s/%s %dx%dx%d lay%d%d p%d" % (c.group, c.family, c.mode, c.M, c.N, c.K, c.al, c.bl, c.prec)
    for k in ("split", "batch", "io"):
        if getattr(c, k) != _FIELDS[k]:
            s += " %s=%d" % (k, getattr(c, k))
    return s + (" trans_c" if c.trans_c else "") + (" colsum" if c.colsum else "")


# ------------------------------------------------------------------------------------------------ the mirror of rp_gemm's dispatch
def has_aux(c):
    return c.dact != 0


def abi_ok(c):
    """the alignment rules of the ABI that a case must respect to be launched at all (None = fine)"""
    if (c.al == 0 or c.bl == 0) and c.K % 4:
        return "K"
    if c.al == 1 and c.M % 4:
        return "M"
    if c.bl == 1 and c.N % 4:
        return "N"
    if c.split > 1 and (c.N % 4 or c.batch > 1):
        return "split"
    return None


def tile(c):
    tm, tn = (1 if c.M <= 64 else 2), (1 if c.N <= 64 else 2)
    reads_mn = has_aux(c) or c.res
    if c.M > 64 and c.prec == 0:
        if c.al == 0 and c.bl == 0:
            tm, tn = 2, 1
        elif c.N % 192 == 0 and not reads_mn:
            tm, tn = 1, 3
        else:
            tm, tn = 2, 1
    if c.M > 64 and c.prec != 0:
        if c.al == 1 and c.bl == 1 and c.N % 192 == 0 and not reads_mn:
            tm, tn = 1, 3
        else:
            tm, tn = 2, 1
    return tm, tn


def k_per_split(c):
    ktiles = (c.K + 31) // 32
    return -(-ktiles // c.split) * 32


def path(c):
    return "dma" if (c.prec == 0 and c.K % 32 == 0 and k_per_split(c) % 32 == 0 and c.M >= 4 and c.N >= 4) else "reg"


def epi_mode(c):
    b, pr, rs = c.bias, c.pre, c.res
    m = "GENERIC"
    if c.dact == 0:
        if c.act == 0 and not pr:
            m = ("BIAS_RES" if rs else "BIAS") if b else ("RES" if rs else "RAW")
        elif c.act == 1 and b and not rs:
            m = "BIAS_GELU_PRE" if pr else "BIAS_GELU"
        elif c.act == 2 and b and not rs and not pr:
            m = "BIAS_RELU"
    elif not b and not pr and not rs and c.act == 0:
        m = "DGELU" if c.dact == 1 else "DRELU"
    return m


def staged(c):
    """the MAIN kernel's store: LDS-staged 16-byte rows or the per-element loop (a split-K main kernel stores raw slabs)"""
    mode = "RAW" if c.split > 1 else epi_mode(c)
    return not (c.al == 1 and c.bl == 1) and c.N % 4 == 0 and mode != "GENERIC"


def ntm(c):
    return -(-c.M // (64 * tile(c)[0]))


def order(c):
    return "split" if c.split > 1 else ("swizzle" if ntm(c) >= 16 else "plain")


def split_lengths(c):
    kps = k_per_split(c)
    return [max(0, min(c.K, (z + 1) * kps) - z * kps) for z in range(c.split)]


def split_class(c):
    """(last live split: whole / short (fewer k-tiles) / tail (K tail inside it), trailing empty splits: 0, 1, 2 = two or more)"""
    if c.split == 1:
        return ("none", 0)
    lens = split_lengths(c)
    live = [n for n in lens if n > 0]
    kind = "tail" if c.K % 32 else ("short" if live[-1] < k_per_split(c) else "whole")
    return (kind, min(len(lens) - len(live), 2))


def cell(c):
    return (c.al, c.bl, c.prec, tile(c), path(c), epi_mode(c), "staged" if staged(c) else "generic", order(c), split_class(c))


def ragged(c):
    tm, tn = tile(c)
    return (c.M % (64 * tm) != 0, c.N % (64 * tn) != 0, c.K % 32 != 0)


def colsum_rows(c):
    return 2 * ntm(c)


def form(c):
    return "tanh" if c.prec == 1 else "erf"


def inexact(c):
    return c.act == 1 or c.dact == 1


# ------------------------------------------------------------------------------------------------ operands
def _gen(*key):
    g = torch.Generator()
    seed = 12345
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    g.manual_seed(seed)
    return g


def _ints(shape, lo, hi, *key):
    return torch.randint(lo, hi + 1, shape, generator=_gen(*key), dtype=torch.int64)


def _sign(shape, *key):
    return _ints(shape, 0, 1, *key) * 2 - 1


def _ternary(b, rows, K, *key):
    t = torch.zeros(b, rows, K, dtype=torch.int64)
    pos = torch.rand(b, rows, K, generator=_gen(*key)).argsort(-1)[..., :8]
    return t.scatter_(-1, pos, _sign((b, rows, 8), 11, *key))


def _bits20(b, rows, K, *key):
    mag = _ints((b, rows, K), 1 << 19, (1 << 20) - 1, *key)
    mag = torch.where(mag & 0xFF == 0, mag | 0x5A, mag)
    return mag * _sign((b, rows, K), 13, *key)


def _sel16(shape, *key):
    return (16 * _ints(shape, 128, 255, *key) + _ints(shape, 1, 15, 17, *key)) * _sign(shape, 19, *key)


def sigma(m, K):
    return (5 * m + 3) % K


@functools.lru_cache(maxsize=None)
def _operands(family, M, N, K, batch, gelu, drelu):
    """int64 tensors and binary exponents: A [b,M,K], B [b,N,K], bias [N], aux / res [b,M,N]; negzero: where aux is -0.0"""
    key = (M, N, K, batch)
    o = dict(ea=0, eb=0, e_bias=0, e_aux=0, e_res=0, negzero=None)
    if family == "small_int":
        o["A"], o["B"] = _ints((batch, M, K), -7, 7, 1, *key), _ints((batch, N, K), -7, 7, 2, *key)
    elif family == "limb_b":
        o["A"], o["B"] = _ternary(batch, M, K, 1, *key), _bits20(batch, N, K, 2, *key)
    elif family == "limb_a":
        o["A"], o["B"] = _bits20(batch, M, K, 1, *key), _ternary(batch, N, K, 2, *key)
    elif family == "selector":
        assert M >= K, "sigma must cover every k"
        A = torch.zeros(batch, M, K, dtype=torch.int64)
        m = torch.arange(M)
        A[:, m, sigma(m, K)] = _sel16((batch, M), 1, *key)
        o["A"], o["B"], o["ea"], o["eb"] = A, _sel16((batch, N, K), 2, *key), 4, 4
    else:
        raise ValueError(family)
    o["bias"] = _ints((N,), -64, 64, 3, *key)
    o["aux"], o["res"] = _ints((batch, M, N), -64, 64, 4, *key), _ints((batch, M, N), -64, 64, 5, *key)
    if gelu:
        o["eb"], o["e_bias"], o["e_aux"] = -6, -4, -4
    if drelu:
        flat = o["aux"].view(-1)
        flat[::5] = 0
        nz = torch.zeros_like(flat, dtype=torch.bool)
        nz[1::7] = True
        flat[nz] = 0
        o["negzero"] = nz.view(batch, M, N)
    return o


def operands(c):
    return _operands(c.family, c.M, c.N, c.K, c.batch, inexact(c), c.dact == 2)


def values(c, device="cpu"):
    """the operands as fp64 values (exact), on `device`: A [b,M,K], B [b,N,K], bias [N], aux / res [b,M,N]"""
    o = operands(c)
    v = {k: (o[k].to(device).double() * 2.0 ** o[e]) for k, e in (("A", "ea"), ("B", "eb"), ("bias", "e_bias"), ("aux", "e_aux"),
                                                                   ("res", "e_res"))}
    if o["negzero"] is not None:
        v["aux"] = torch.where(o["negzero"].to(device), torch.full_like(v["aux"], -0.0), v["aux"])
    return v


def bf16_round(t):
    return t.float().to(torch.bfloat16).double()


def product(c, v):
    """op(A) op(B) in fp64 [b,M,N] -- exact; precision 1 multiplies the operands rounded to bf16 (round to nearest even)"""
    A, B = (bf16_round(v["A"]), bf16_round(v["B"])) if c.prec == 1 else (v["A"], v["B"])
    return A @ B.transpose(1, 2)


def epilogue(c, P, v, dtype, frm=None):
    """(pre, out) of RpGemm's epilogue, in `dtype`, from the exact product P"""
    frm = form(c) if frm is None else frm
    x = P.to(dtype)
    if c.bias:
        x = x + v["bias"].to(dtype)
    pre = x
    if c.act == 1:
        x = R.gelu(x, frm)
    elif c.act == 2:
        x = x.clamp_min(0)
    if c.dact == 1:
        x = x * R.gelu_grad(v["aux"].to(dtype), frm)
    elif c.dact == 2:
        x = torch.where(v["aux"].to(dtype) > 0, x, torch.zeros_like(x))
    if c.res:
        x = x + v["res"].to(dtype)
    return pre, x


def colsum_ref(c, out):
    """[2 ntm, N] column sums of out [M, N] over the 32 TM rows of each (tile, wave row); rows past M contribute nothing"""
    h = 32 * tile(c)[0]
    rows = colsum_rows(c)
    pad = torch.zeros(rows * h, out.shape[1], dtype=out.dtype, device=out.device)
    pad[:c.M] = out
    return pad.view(rows, h, -1).sum(1)


def magnitude_bound(c):
    """(largest |value| any partial sum or exact epilogue intermediate can take, in units of the case's grid; grid exponent).  int64."""
    o = operands(c)
    A, B = o["A"], o["B"]
    if c.prec == 1:      # operands after RNE to bf16 are still integers on the same grid (|x| < 2^8: unchanged; 20 bits: multiples of 2^12)
        A, B = bf16_round(A.double()).long(), bf16_round(B.double()).long()
    es = [o["ea"] + o["eb"]] + ([o["e_bias"]] if c.bias else []) + ([o["e_res"]] if c.res else [])
    g = min(es)
    tot = (A.abs() @ B.abs().transpose(1, 2)) << (o["ea"] + o["eb"] - g)
    if c.bias:
        tot = tot + (o["bias"].abs() << (o["e_bias"] - g))
    if c.res and not inexact(c):
        tot = tot + (o["res"].abs() << (o["e_res"] - g))
    worst = int(tot.max())
    if c.colsum:
        worst *= c.M
    return worst, g


# ------------------------------------------------------------------------------------------------ the table
SHAPES = ((1, 1), (3, 5), (1, 7), (4, 4), (60, 60), (64, 64), (60, 64), (64, 60), (64, 3), (60, 68), (64, 128), (4, 196), (3, 68),
          (64, 70), (60, 384), (68, 60), (128, 64), (132, 196), (68, 7), (132, 70), (128, 128), (68, 4), (68, 192), (128, 192), (132, 384))
K_REG, K_DMA = (4, 28, 36, 100), (32, 64, 96, 160)
EPI_SHAPES = ((60, 60), (60, 68), (68, 60), (132, 196), (68, 192), (60, 70), (68, 7), (3, 5), (4, 7))
SPLIT_SHAPE = (68, 60)
SPLIT_VARIANTS = (("RAW", {}), ("G_SPLIT_BIAS_RELU_RES", None), ("BIAS_GELU_PRE", {}), ("RAW", dict(trans_c=True)))
MODES["G_SPLIT_BIAS_RELU_RES"] = dict(bias=True, act=2, res=True)
ORDER_SHAPES = ((1028, 192), (2052, 60))
BATCH_SHAPES = ((68, 60, 36), (132, 96, 32))
COLSUM_SHAPES = ((60, 60), (20, 60), (60, 68), (20, 68), (68, 60), (132, 60))
COLSUM_MODES = ("BIAS", "DGELU", "DRELU", "RES")
IO_SHAPES = ((60, 60), (68, 60), (60, 68))
IO_MODES = (("RAW", (1, 2, 3)), ("BIAS", (1, 2, 3)), ("BIAS_GELU", (1, 2, 3)), ("BIAS_GELU_PRE", (1, 2, 3)), ("BIAS_RELU", (1, 2, 3)),
            ("DGELU", (1, 2, 4, 3, 7)), ("DRELU", (1, 2, 4, 3, 7)), ("BIAS_RES", (1,)), ("RES", (1,)))
LIMB_SHAPES = ((64, 60), (64, 68), (68, 60), (68, 192))
DEFER_TASKS = ((68, 60, 36, 2, False), (64, 64, 64, 3, True), (60, 128, 100, 5, False), (132, 196, 160, 9, True), (4, 4, 36, 12, False),
               (128, 192, 64, 2, True), (68, 4, 100, 3, False), (60, 384, 160, 5, True))


def _legal(cases):
    return [c for c in cases if abi_ok(c) is None]


def _main():
    out = []
    for lay, p in itertools.product(LAYOUTS, PRECISIONS):
        for i, (M, N) in enumerate(SHAPES):
            ks = [K_REG[i % 4], K_REG[(i + 1) % 4], K_DMA[i % 4], K_DMA[(i + 2) % 4]]
            out += [mk("main", "RAW", M, N, K, lay, p) for K in ks]
        out.append(mk("main", "RAW", 68, 60, K_LONG, lay, p))
    return _legal(out)


def _epi():
    out = []
    for lay, p in itertools.product(LAYOUTS, (0, 1)):
        for (M, N), K, mode in itertools.product(EPI_SHAPES, (36, 64) if p == 0 else (36,), list(MODES)[:14]):
            out.append(mk("epi", mode, M, N, K, lay, p))
    return _legal(out)


def _splitk():
    out = []
    for lay, p in itertools.product(LAYOUTS, PRECISIONS):
        for s, K, (mode, kw) in itertools.product(SPLITS, SPLIT_KS, SPLIT_VARIANTS):
            out.append(mk("splitk", mode, SPLIT_SHAPE[0], SPLIT_SHAPE[1], K, lay, p, split=s, **(kw or {})))
    return _legal(out)


def defer_tasks(lay, p):
    return _legal([mk("defer", "RAW", M, N, K, lay, p, split=s, trans_c=t) for M, N, K, s, t in DEFER_TASKS])


def _order():
    out = []
    for lay, p in itertools.product(LAYOUTS, PRECISIONS):
        for (M, N), K in itertools.product(ORDER_SHAPES, (36, 32)):
            c = mk("order", "RAW", M, N, K, lay, p)
            if order(c) != "swizzle":
                continue
            out.append(c)
            if tile(c)[0] == 2 and lay != (1, 1):
                out.append(c._replace(colsum=True))
    return _legal(out)


def _batch():
    out = []
    for lay, p in itertools.product(((0, 0), (0, 1)), PRECISIONS):
        for (M, N, K), b, mode in itertools.product(BATCH_SHAPES, (2, 5), ("RAW", "RES")):
            out.append(mk("batch", mode, M, N, K, lay, p, batch=b))
    return _legal(out)


def _colsum():
    out = []
    for lay, p in itertools.product(LAYOUTS[:3], PRECISIONS):
        for (M, N), K, mode in itertools.product(COLSUM_SHAPES, (36, 64) if p == 0 else (36,), COLSUM_MODES):
            out.append(mk("colsum", mode, M, N, K, lay, p, colsum=True))
    return _legal(out)


def _iobf16():
    out = []
    for lay in LAYOUTS:
        for (M, N), (mode, bits) in itertools.product(IO_SHAPES, IO_MODES):
            for io in bits:
                if lay == (1, 1) and io & 6:
                    continue
                out.append(mk("iobf16", mode, M, N, 36, lay, 1, io=io))
    return _legal(out)


def _limb():
    out = []
    for lay, p in itertools.product(LAYOUTS, PRECISIONS):
        seen = set()
        for (M, N), fam in itertools.product(LIMB_SHAPES, ("limb_a", "limb_b", "selector")):
            c = mk("limb", "RAW", M, N, 64, lay, p)._replace(family=fam)
            if (fam == "selector" and p == 1) or (p != 3 and seen and tile(c) not in seen):
                continue
            seen.add(tile(c))
            out.append(c)
    return _legal(out)


@functools.lru_cache(maxsize=None)
def table():
    return tuple(_main() + _epi() + _splitk() + _order() + _batch() + _colsum() + _iobf16() + _limb())


def keys():
    """(group, a_layout, b_layout, precision) of the GPU tests, in table order"""
    return list(dict.fromkeys((c.group, c.al, c.bl, c.prec) for c in table()))


def cases_of(group):
    return [c for c in table() if c.group == group]


def cases(group, al, bl, prec):
    return [c for c in table() if (c.group, c.al, c.bl, c.prec) == (group, al, bl, prec)]


# ------------------------------------------------------------------------------------------------ what the table must contain
def _universe(lay, extra_n=True):
    ns = NS + (NS_B0 if lay[1] == 0 and extra_n else ())
    return [(M, N, K) for M, N, K in itertools.product(MS, ns, KS)]


def required():
    """group -> set of cells the group must hit, enumerated from the mirror over the issue's extents -- not from the table"""
    req = collections.defaultdict(set)
    for lay, p in itertools.product(LAYOUTS, PRECISIONS):
        for M, N, K in _universe(lay):
            c = mk("main", "RAW", M, N, K, lay, p)
            if abi_ok(c) is None and order(c) == "plain":
                req["main"].add((lay, p, tile(c), path(c)))
            if abi_ok(c) is None and order(c) == "swizzle" and M in (1028, 2052) and tile(c) in ((1, 3), (2, 1)):
                req["order"].add((lay, p, tile(c), path(c), False))
                if tile(c)[0] == 2 and lay != (1, 1):
                    req["order"].add((lay, p, tile(c), path(c), True))
        for M, N, K in _universe(lay):
            if M > 132 or p == 3:
                continue
            for mode in list(MODES)[:14]:
                c = mk("epi", mode, M, N, K, lay, p)
                if abi_ok(c) is None:
                    req["epi"].add((lay, p, tile(c), epi_mode(c), mode, "staged" if staged(c) else "generic"))
        for s, K in itertools.product(SPLITS, SPLIT_KS):
            for mode, kw in SPLIT_VARIANTS:
                c = mk("splitk", mode, SPLIT_SHAPE[0], SPLIT_SHAPE[1], K, lay, p, split=s, **(kw or {}))
                req["splitk"].add((lay, p, path(c), split_class(c), mode, c.trans_c))
    return req


def hit():
    """group -> the same projections, of the table"""
    got = collections.defaultdict(set)
    for c in table():
        lay = (c.al, c.bl)
        if c.group == "main" and order(c) == "plain":
            got["main"].add((lay, c.prec, tile(c), path(c)))
        elif c.group == "order":
            got["order"].add((lay, c.prec, tile(c), path(c), c.colsum))
        elif c.group == "epi":
            got["epi"].add((lay, c.prec, tile(c), epi_mode(c), c.mode, "staged" if staged(c) else "generic"))
        elif c.group == "splitk":
            got["splitk"].add((lay, c.prec, path(c), split_class(c), c.mode, c.trans_c))
    return got
