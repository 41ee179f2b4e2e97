"""Exact-arithmetic operands, references and a Python mirror of the work partitions for the transformer Block's dense kernels that do not
go through rp_gemm: rp_linear_rows192 (csrc/linear_rows.hip), rp_mlp_fused_fwd / _bwd / _bwd_ln (csrc/mlp_fused.hip), the weight-gradient
kernels rp_dw192_f32 / _split3 / _bf16 (csrc/dw192_*.hip) with rp_splitk_reduce_multi behind them, rp_ds_matmul / rp_ds_matmul_t
(csrc/attention.hip) and rp_dx_lnbwd_bf16 (csrc/dx_lnbwd_bf16.hip).  torch only, no GPU and no library at
import: tests/test_block_cells_cpu.py proves the premises on the CPU, tests/test_gpu_block_cells.py runs the cases through the C ABI.
The generators (_ints, _sign, _bits20, _sel16, _ternary, bf16_round) are tests/_gemm_cells.py's.

The method is that module's: operands for which every product and every partial sum, in ANY order, is an integer times one power of two
below 2^24 (bounded through sum |a| |b|).  Stream-K cuts, the fix-up's sums of partial tiles, split-K slabs, the fixed-order reduce and
the column sums are then exact and the stored value must equal the integer reference BIT FOR BIT.

Families
  small_int    integers in [-7, 7] (activations, gradients, weights), [-64, 64] (bias, residual).
  x12          the operand a precision-1 kernel rounds on chip holds 12-bit integers (odd, |x| in [2^11, 2^12)): the reference multiplies
               round-to-nearest-even(x); truncation differs in about half of the elements.
  gelu_exact   pre-activations in {0} u {8, 16, ...}: non-negative sparse activations x weights in {0, 8, 16} + bias in {0, 8, 16}.
               common.h: gelu_fast(x) = x (1 - e) with e ~ 1e-8 < 2^-25 for x >= 5.7, so GELU(x) = x, and GELU(0) = 0; gelu_bf saturates
               the same way (exp2(-71) vanishes next to 1).  GELU'(x) = 1 for x >= 8 and 0.5 at 0 -- the latter if v_exp_f32(-1) = 0.5
               (erf form) resp. v_rcp_f32(2) = 0.5 (sigmoid form), which the first GPU case of each form reads back.  No negatives:
               x e != 0 there.  Both classes hold at least 20 % of the values of every case (checked on the CPU).
  selector     behind a fused LayerNorm the activations are arbitrary fp32.  The weight has ONE non-zero per output unit, +-2^j at
               k(n) = (5 n + 3 + shift) mod 192 (5 is a unit mod 192: 192 consecutive n hit every k), no bias: each output is one product
               with a power of two plus exact zeros, y[m, n] == +-2^j xn_out[m, k(n)] of the same launch, for ANY activations.  At
               precision 1 the right-hand side is xn_out as stored with io_bf16 bit 3 (the rows the MFMA consumed) -- or the fp32 xn_out
               rounded to nearest even when bit 3 is off.
  const_rows   rp_mlp_fused_fwd: every row of x is a constant c_m (an integer for which sum / 192 == c_m in fp32, checked), so the
               LayerNorm output equals beta bit for bit; beta, w1, b1 from gelu_exact, w2, b2 small_int: the whole chain -- both
               products, bias, GELU, residual, owner epilogue or fix-up -- equals an integer reference.
  row_coded    rp_dw192_*: a[m, n] = +-1 where n == m (mod 192), b[m, k] = 1 + (37 m + 11 k + (m >> 7)) mod 127, a 7-bit code of the token:
               a token row that is dropped, counted twice or shifted changes a stored integer of its slab.
  limb / sel16 rp_dw192_split3 (and the other two): ternary x 20-bit operands reach limb products (0,0), (0,1), (0,2), one 16-bit x 16-bit
               product per output reaches (1,1) (tests/_gemm_cells.py).  rp_dw192_bf16 with an fp32 b must equal the product with
               round-to-nearest-even(b).

  int_xhat     rp_mlp_fused_bwd_ln, rp_dx_lnbwd_bf16: the LayerNorm's x, mean and rstd are inputs, so xhat is made a small multiple of 1/2
               (integer mean, rstd in {1, 1/2}, integer x - mean): the per-block column sums of dxn o xhat, dxn and dy / add are exact.
  ds_code      rp_ds_matmul(_t): ds[i][j] = (3 i + 5 j + 7 zh) mod 15 - 7, placed into the two tile layouts from the header's text.
Outputs that are inexact by nature (GELU of arbitrary values, dx behind a LayerNorm backward) go by tests/_norm_regimes.py's bound rule.

The mirror restates how linear_rows.hip and mlp_fused.hip cut their (row tile) x (chunk) list into G contiguous ranges (G from
rp_linear_rows192_grid / rp_mlp_fused_grid on the device): base, rem, every range, the number of ranges that share a tile (1 = finished by
its owner's epilogue; 2, 3 or all 24 = by the fix-up), whether a range starts inside a tile or runs across a tile boundary; and how the
rp_dw192_* launchers cut M token rows into slabs of whole stages."""
import collections
import functools

import torch

from tests import _gemm_cells as G

LIM = G.LIM
C, HID, CH, NCHUNK = 192, 768, 32, 24
ROWS_LINEAR = 64
PERIOD = 1031          # operands of the large-M cases repeat with this (prime) period of rows


# ------------------------------------------------------------------------------------------------ the mirror: stream-K ranges
def split(items, grid):
    """(base, rem) of `items` work items cut into `grid` contiguous ranges, the first rem of them one item longer"""
    return divmod(items, grid)


def range_of(b, base, rem):
    """(first item, number of items) of range b"""
    return b * base + min(b, rem), base + (1 if b < rem else 0)


def owner(item, base, rem):
    """the range that holds `item` (int or int64 tensor) -- closed form, no enumeration"""
    big = rem * (base + 1)
    if isinstance(item, torch.Tensor):
        lo = torch.div(item, base + 1, rounding_mode="floor")
        hi = rem + torch.div(item - big, max(base, 1), rounding_mode="floor")
        return torch.where(item < big, lo, hi)
    return item // (base + 1) if item < big else rem + (item - big) // base


def sharers(tiles, nchunk, grid):
    """[tiles] int64: how many ranges hold a chunk of each tile (ranges are contiguous: last owner - first owner + 1)"""
    base, rem = split(tiles * nchunk, grid)
    first = torch.arange(tiles, dtype=torch.int64) * nchunk
    return owner(first + nchunk - 1, base, rem) - owner(first, base, rem) + 1


def class_name(n, nchunk):
    return {1: "owner", 2: "two", 3: "three", nchunk: "all"}.get(int(n), "n%d" % int(n))


def tile_classes(tiles, nchunk, grid):
    """the set of classes of a launch's tiles: 'owner' (finished in the main kernel), 'two' / 'three' / 'all' (nchunk one-chunk partials)
    or 'n<k>' -- what finishes each tile"""
    return {class_name(n, nchunk) for n in sharers(tiles, nchunk, grid).unique()}


def range_classes(tiles, nchunk, grid):
    """linear_rows: (some range starts inside a tile, some range runs across a tile boundary, base)"""
    base, rem = split(tiles * nchunk, grid)
    b = torch.arange(grid, dtype=torch.int64)
    start = b * base + torch.clamp(b, max=rem)
    count = base + (b < rem).long()
    mid = bool(((start % nchunk != 0) & (count > 0)).any())
    cross = bool((torch.div(start, nchunk, rounding_mode="floor") != torch.div(start + count - 1, nchunk, rounding_mode="floor")).any())
    return mid, cross, base


def brute_force(tiles, nchunk, grid):
    """the same facts by walking every item of every range: ([tiles] sharers, mid, cross)"""
    base, rem = split(tiles * nchunk, grid)
    who = [set() for _ in range(tiles)]
    mid = cross = False
    nxt = 0
    for b in range(grid):
        start, count = range_of(b, base, rem)
        assert start == nxt
        nxt = start + count
        seen = set()
        for it in range(start, start + count):
            assert owner(it, base, rem) == b
            who[it // nchunk].add(b)
            seen.add(it // nchunk)
        mid |= count > 0 and start % nchunk != 0
        cross |= len(seen) > 1
    assert nxt == tiles * nchunk
    return torch.tensor([len(w) for w in who]), mid, cross


def mlp_rows(backward, prec):
    """rows per tile of the fused MLP (include/relpose_hip.h at rp_mlp_fused_grid): 64 for the fp32 forward, 192 otherwise"""
    return 64 if not backward and prec == 0 else 192


def smallest_m(rows, nchunk, grid_of, want, ragged=0, max_tiles=4096):
    """the smallest M = tiles * rows - ragged for which want(tiles, grid) holds; grid_of(M) asks the library"""
    for t in range(1, max_tiles + 1):
        M = t * rows - ragged
        if M > 0 and want(t, grid_of(M)):
            return M
    raise AssertionError("no M up to %d tiles reaches the class" % max_tiles)


# ------------------------------------------------------------------------------------------------ the mirror: rp_dw192_* slabs
def dw_slabs(M, N, sr):
    """(number of slabs, stages per slab, stages of the last slab) -- rp_dw192_f32_splits (sr = 32) / rp_dw192_bf16_splits (sr = 64).  With
    fewer than two stages the count stays 2 and the second slab is empty (0 stages: zeros)."""
    ntile, stages = N // C, -(-M // sr)
    sp = max(2, min(8 * (32 // ntile), stages))
    per = -(-stages // sp)
    sp = max(2, -(-stages // per))
    return sp, per, stages - (sp - 1) * per


def dw_slab_rows(M, N, sr):
    sp, per, _ = dw_slabs(M, N, sr)
    return [(min(M, s * per * sr), min(M, (s + 1) * per * sr)) for s in range(sp)]


def dw_smallest_m(N, sr, per, last):
    for stages in range(2, 4096):
        if dw_slabs(stages * sr, N, sr)[1:] == (per, last):
            return stages * sr
    raise AssertionError


# ------------------------------------------------------------------------------------------------ generators
def _sparse(rows, K, nnz, lo, hi, *key):
    t = torch.zeros(rows, K, dtype=torch.int64)
    pos = torch.rand(rows, K, generator=G._gen(7, *key)).argsort(-1)[:, :nnz]
    return t.scatter_(-1, pos, G._ints((rows, nnz), lo, hi, 9, *key))


def _w816(rows, K, *key):
    """{0, 8, 16}, non-zero with probability 1 / 12"""
    return (torch.rand(rows, K, generator=G._gen(21, *key)) < 1 / 12).long() * 8 * G._ints((rows, K), 1, 2, 23, *key)


def _b816(n, *key):
    return (torch.rand(n, generator=G._gen(25, *key)) < 0.25).long() * 8 * G._ints((n,), 1, 2, 27, *key)


def preact(rows, cols, *key):
    """a saved pre-activation of the gelu_exact family: 0 (about 40 %) or an integer in [8, 64]"""
    z = torch.rand(rows, cols, generator=G._gen(29, *key)) < 0.4
    return torch.where(z, torch.zeros(rows, cols, dtype=torch.int64), G._ints((rows, cols), 8, 64, 31, *key))


def _x12(rows, K, *key):
    return (G._ints((rows, K), 1 << 10, (1 << 11) - 1, 33, *key) * 2 + 1) * G._sign((rows, K), 35, *key)


def periodic(t, M):
    """[M, ...] from a base of at most PERIOD rows"""
    return t if t.shape[0] == M else t[torch.arange(M, device=t.device) % t.shape[0]]


def base_rows(M):
    return min(M, PERIOD)


def gelu_exact_classes(pre):
    """(share of zeros, share of values >= 8, everything is one of the two)"""
    z, s = (pre == 0), (pre >= 8)
    return float(z.double().mean()), float(s.double().mean()), bool((z | s).all())


def gelu_grad_x(pre):
    return torch.where(pre == 0, torch.full_like(pre, 0.5), torch.ones_like(pre))


# ------------------------------------------------------------------------------------------------ rp_linear_rows192
LFORMS = ("plain", "bias", "bias_res", "gelu_pre", "ln", "dact_cs", "gelu_res")
BIASED = ("bias", "bias_res", "gelu_pre", "gelu_res")
LCase = collections.namedtuple("LCase", "form M N prec io fam")
LINEAR_NS = (192, 576, 768, 32, 1024)
LINEAR_MS = (1, 15, 17, 63, 65)


def lname(c):
    return "linear/%s/%s M=%d N=%d p%d io=%d" % (c.form, c.fam, c.M, c.N, c.prec, c.io)


def linear_io(form, prec):
    """the io_bf16 combinations the ABI admits for a form (bit 0 x bf16: not with a LayerNorm; bit 2: needs dact_aux; bit 3: needs xn_out)"""
    if prec == 0:
        return (0,)
    if form == "ln":
        return (0, 2, 8, 10)
    return (0, 1, 2, 3, 4, 5, 6, 7) if form == "dact_cs" else (0, 1, 2, 3)


def linear_family(form, prec, io):
    if form in ("gelu_pre", "gelu_res"):
        return ("gelu_exact",)
    if form == "ln":
        return ("selector",)
    return ("small_int", "x12") if form == "plain" and prec == 1 and not io & 1 else ("small_int",)


def linear_shapes(big_m):
    """(M, N) of every (form, precision, io): the M list at N = 192, every N at a ragged two-tile and a one-wave M, and the M at which the
    ranges of N = 768 start inside tiles and cross them (from the device)"""
    return [(M, 192) for M in LINEAR_MS] + [(M, N) for N in LINEAR_NS[1:] for M in (17, 65)] + [(big_m, 768)]


@functools.lru_cache(maxsize=None)
def linear_operands(form, fam, M, N):
    """int64 / fp32 operands on the CPU: x [M,192], w [N,192], bias [N], res / aux [M,N] (whatever the form reads)"""
    key = (M, N, LFORMS.index(form))
    o = {}
    if fam == "gelu_exact":
        o["x"], o["w"], o["bias"] = _sparse(M, C, 8, 1, 3, 1, *key), _w816(N, C, 2, *key), _b816(N, 3, *key)
    elif fam == "selector":
        g = G._gen(41, *key)
        rows = torch.randn(M, C, generator=g) * torch.rand(M, 1, generator=g).mul(6).exp2() + torch.randn(M, 1, generator=g) * 8
        n = torch.arange(N)
        o["k"] = (5 * n + 3 + 7 * (M % 5)) % C
        o["wv"] = G._sign((N,), 43, *key).double() * 2.0 ** G._ints((N,), -2, 3, 45, *key).double()
        w = torch.zeros(N, C, dtype=torch.float64)
        w[n, o["k"]] = o["wv"]
        o["x"], o["w"] = rows.float(), w
        o["gamma"] = torch.randn(C, generator=g).float() * 0.5 + 1
        o["beta"] = torch.randn(C, generator=g).float()
        return o
    else:
        o["x"] = _x12(M, C, 1, *key) if fam == "x12" else G._ints((M, C), -7, 7, 1, *key)
        o["w"], o["bias"] = G._ints((N, C), -7, 7, 2, *key), G._ints((N,), -64, 64, 3, *key)
    o["res"] = G._ints((M, N), -64, 64, 4, *key)
    o["aux"] = preact(M, N, 5, *key)
    return o


def linear_reference(c, o, fault=None):
    """fp64 (y, y_pre or None, colsum_part or None) of an exact (non-selector) case; operands `o` as fp64 tensors on any device.
    fault: a reference carrying exactly one fault class (the CPU proof that the family sees it)."""
    x = o["x"]
    if c.prec == 1:
        x = G.bf16_round(x) if fault != "truncate" else truncate_bf16(x)
    y = x @ o["w"].t()
    pre = None
    if c.form in BIASED:
        y = y + o["bias"]
    if fault == "res_before_gelu":                     # act(pre + res) instead of act(pre) + res (pre + res may be negative: the true GELU)
        return torch.nn.functional.gelu(y + o["res"]), y, None
    if c.form in ("gelu_pre", "gelu_res"):
        pre = y                                        # GELU on the gelu_exact family is the identity
    if c.form in ("bias_res", "gelu_res"):
        y = y + o["res"]
    cs = None
    if c.form == "dact_cs":
        y = y * gelu_grad_x(o["aux"])
        tiles = -(-c.M // ROWS_LINEAR)
        pad = torch.zeros(tiles * ROWS_LINEAR, c.N, dtype=y.dtype, device=y.device)
        pad[:c.M] = y
        if fault == "colsum_past_m" and c.M % ROWS_LINEAR:
            pad[c.M] = y[c.M - 1]
        cs = pad.view(tiles, ROWS_LINEAR, c.N).sum(1)
    return y, pre, cs


def truncate_bf16(t):
    """fp64 -> bf16 by TRUNCATION of the fp32 pattern (the fault, not what the kernels do)"""
    bits = t.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).double()


def linear_bound(c, o):
    """largest sum |a| |b| (+ |bias| + |res|), and over a tile's rows for the column sums: must stay below 2^24"""
    x = G.bf16_round(o["x"]) if c.prec == 1 else o["x"]
    tot = x.abs() @ o["w"].abs().t()
    if c.form in BIASED:
        tot = tot + o["bias"].abs()
    if c.form in ("bias_res", "gelu_res"):
        tot = tot + o["res"].abs()
    worst = float(tot.max())
    return worst * (min(c.M, ROWS_LINEAR) if c.form == "dact_cs" else 1)


# ------------------------------------------------------------------------------------------------ rp_mlp_fused_fwd / _bwd
CONST_ROW_VALUES = (0, 1, -2, 3, 8, -16, 40, 64, -5, 12)


@functools.lru_cache(maxsize=None)
def mlp_fwd_operands(M):
    """const_rows: x [P] (the row constants of the base period), beta [192], w1 [768,192], b1 [768], w2 [192,768], b2 [192] -- int64"""
    key = (M, 77)
    P = base_rows(M)
    c = torch.tensor(CONST_ROW_VALUES)[G._ints((P,), 0, len(CONST_ROW_VALUES) - 1, 1, *key)]
    beta = _sparse(1, C, 8, 1, 3, 2, *key)[0]
    return dict(c=c, beta=beta, gamma=G._ints((C,), -7, 7, 6, *key), w1=_w816(HID, C, 3, *key), b1=_b816(HID, 4, *key),
                w2=G._ints((C, HID), -7, 7, 5, *key), b2=G._ints((C,), -64, 64, 7, *key))


def mlp_fwd_reference(o, M, fault=None):
    """fp64: (y [M,192], hpre [768], h [768]) -- every row has the same hidden vector; operands as fp64 tensors on one device"""
    hpre = o["w1"] @ o["beta"] + o["b1"]
    h = hpre                                           # GELU on the gelu_exact family is the identity
    out = o["w2"] @ h + o["b2"]
    if fault == "partial_twice":                       # the first chunk's partial added twice by the fix-up
        out = out + o["w2"][:, :CH] @ h[:CH]
    if fault == "unit_order":                          # the units of chunk 0 in reversed order against w2's columns
        out = out + o["w2"][:, :CH] @ (h[:CH].flip(0) - h[:CH])
    c = periodic(o["c"], M)
    return c[:, None] + out[None, :], hpre, h


@functools.lru_cache(maxsize=None)
def mlp_selector_operands(M, shift):
    """selector family of rp_mlp_fused_fwd: arbitrary fp32 rows (per-row offsets and scales), w1 with one +-2^j per hidden unit u at
    k(u) = (5 u + 3 + shift) mod 192, w2 with one +-2^j per output n at unit u(n) = (4 n + shift) mod 768 (shift = 0..3 selects every
    unit once), b1 = b2 = 0.  fp32 / fp64 tensors on the CPU; x holds the base period of rows."""
    key = (M, shift, 79)
    g = G._gen(41, *key)
    P = base_rows(M)
    x = torch.randn(P, C, generator=g) * torch.rand(P, 1, generator=g).mul(6).exp2() + torch.randn(P, 1, generator=g) * 8
    u, n = torch.arange(HID), torch.arange(C)
    k1, u2 = (5 * u + 3 + shift) % C, (4 * n + shift) % HID
    wv1 = G._sign((HID,), 43, *key).double() * 2.0 ** G._ints((HID,), -2, 2, 45, *key).double()
    wv2 = G._sign((C,), 47, *key).double() * 2.0 ** G._ints((C,), -2, 2, 49, *key).double()
    w1, w2 = torch.zeros(HID, C, dtype=torch.float64), torch.zeros(C, HID, dtype=torch.float64)
    w1[u, k1], w2[n, u2] = wv1, wv2
    return dict(x=x.float(), gamma=(torch.randn(C, generator=g) * 0.5 + 1).float(), beta=torch.randn(C, generator=g).float(), w1=w1, w2=w2,
                k1=k1, u2=u2, wv1=wv1, wv2=wv2)


def mlp_fwd_bound(o):
    hpre = o["w1"].abs() @ o["beta"].abs() + o["b1"].abs()
    return float(hpre.max()), float((o["w2"].abs() @ hpre + o["b2"].abs()).max() + o["c"].abs().max())


@functools.lru_cache(maxsize=None)
def mlp_bwd_operands(M):
    """dy [P,192], hpre [P,768] (gelu_exact), w2t [768,192], w1t [192,768] -- int64, P = the base period"""
    key = (M, 78)
    P = base_rows(M)
    return dict(dy=G._ints((P, C), -7, 7, 1, *key), hpre=preact(P, HID, 2, *key), w2t=G._ints((HID, C), -7, 7, 3, *key),
                w1t=G._ints((C, HID), -7, 7, 4, *key))


def mlp_bwd_reference(o, M, prec, rows=192, fault=None):
    """fp64 (dhp [M,768], dxn [M,192], colpart [tiles,768]); precision 1 packs dhp to bf16 (nearest even) for the second product"""
    dy, hpre = periodic(o["dy"], M), periodic(o["hpre"], M)
    dhp = (dy @ o["w2t"].t()) * gelu_grad_x(hpre)
    d2 = dhp if prec == 0 else (G.bf16_round(dhp) if fault != "truncate" else truncate_bf16(dhp))
    dxn = d2 @ o["w1t"].t()
    tiles = -(-M // rows)
    pad = torch.zeros(tiles * rows, HID, dtype=dhp.dtype, device=dhp.device)
    pad[:M] = dhp
    return dhp, dxn, pad.view(tiles, rows, HID).sum(1)


def unit_perm():
    """order of the hidden units inside every 32-chunk of the precision-1 second weight, from the text at rp_mlp_fused_bwd: position
    8 q + e of chunk c holds unit 32 c + 4 q + e (e < 4) or 32 c + 16 + 4 q + e - 4 (e >= 4)"""
    out = []
    for c in range(NCHUNK):
        for q in range(4):
            for e in range(8):
                out.append(32 * c + (4 * q + e if e < 4 else 16 + 4 * q + e - 4))
    return torch.tensor(out)


def second_weight(w, chunk_major):
    """[192, 768] second weight of a precision-1 launch: permuted units, optionally chunk-major [24][192][32]"""
    p = w[:, unit_perm().to(w.device)]
    return p.view(C, NCHUNK, CH).permute(1, 0, 2).contiguous() if chunk_major else p.contiguous()


# ------------------------------------------------------------------------------------------------ rp_dw192_*
DW_NS = (192, 576, 768)
DW_FAMILIES = ("small_int", "row_coded", "limb", "sel16")


@functools.lru_cache(maxsize=None)
def dw_operands(fam, M, N):
    """(a [M,N], b [M,192]) int64 and their common binary exponent pair (ea, eb)"""
    key = (M, N, DW_FAMILIES.index(fam))
    if fam == "small_int":
        return G._ints((M, N), -7, 7, 1, *key), G._ints((M, C), -7, 7, 2, *key), 0, 0
    m = torch.arange(M)
    if fam == "row_coded":
        a = torch.zeros(M, N, dtype=torch.int64)
        for t in range(N // C):
            a[m, t * C + m % C] = G._sign((M,), 3 + t, *key)
        k = torch.arange(C)
        return a, 1 + (37 * m[:, None] + 11 * k[None, :] + (m[:, None] >> 7)) % 127, 0, 0
    if fam == "limb":                                  # a^T ternary with 8 non-zeros per output row n, b 20-bit
        return G._ternary(1, N, M, 1, *key)[0].t().contiguous(), G._bits20(1, M, C, 2, *key)[0], 0, 0
    if fam == "sel16":                                 # one non-zero per output row n, at token (5 n + 3) mod M
        a = torch.zeros(M, N, dtype=torch.int64)
        n = torch.arange(N)
        a[G.sigma(n, M), n] = G._sel16((N,), 1, *key)
        return a, G._sel16((M, C), 2, *key), 4, 4
    raise ValueError(fam)


def dw_values(fam, M, N, device="cpu"):
    a, b, ea, eb = dw_operands(fam, M, N)
    return a.to(device).double() * 2.0 ** ea, b.to(device).double() * 2.0 ** eb


def dw_reference(a, b, rows, fault=None):
    """fp64 slabs [len(rows)][N][192] of a^T b over the token rows [m0, m1) of each slab (dw_slab_rows: equal slabs, a shorter last)"""
    sp, rps, M = len(rows), rows[0][1] - rows[0][0], a.shape[0]
    assert all(m0 == s * rps for s, (m0, _) in enumerate(rows[:-1])) and rows[-1][1] == M <= sp * rps
    pa, pb = (torch.zeros(sp * rps, t.shape[1], dtype=t.dtype, device=t.device) for t in (a, b))
    pa[:M], pb[:M] = a, b
    if fault == "row_dropped":
        pa[0] = 0
    return pa.view(sp, rps, -1).transpose(1, 2) @ pb.view(sp, rps, -1)


def dw_bound(a, b):
    return float((a.abs().t() @ b.abs()).max())


# ------------------------------------------------------------------------------------------------ rp_ds_matmul / rp_ds_matmul_t
NTOK, TILE = 576, 32


def ds_code(ZH):
    """integer ds [ZH, 576, 576] in [-7, 7]: NOT symmetric in (i, j) and different for every problem zh"""
    i, j, zh = torch.arange(NTOK)[None, :, None], torch.arange(NTOK)[None, None, :], torch.arange(ZH)[:, None, None]
    return (3 * i + 5 * j + 7 * zh) % 15 - 7


def ds_offsets(layout, swapped=False):
    """[576, 576] int64: where element (i, j) of one problem lies in its tiled image, written from the text of include/relpose_hip.h.
    'acc' (rp_attn_bwd_dkdv_ds / rp_emm_grad_ds -> rp_ds_matmul): ds[i >> 5][j >> 5][r][lane], i & 31 = (r & 3) + 8 (r >> 2) + 4 (lane >> 5),
    j & 31 = lane & 31.  'runs' (rp_attn_bwd_dkdv_p -> rp_ds_matmul_t): [i >> 5][j >> 5][1024], element at ((i >> 2) * 32 + j) * 4 + (i & 3)
    inside the tile.  swapped: the fault -- i and j exchanged INSIDE a tile."""
    i, j = torch.arange(NTOK)[:, None].expand(NTOK, NTOK), torch.arange(NTOK)[None, :].expand(NTOK, NTOK)
    ii, jj = (j & 31, i & 31) if swapped else (i & 31, j & 31)
    if layout == "acc":
        r, hi = (ii & 3) + 4 * (ii >> 3), (ii >> 2) & 1
        off = r * 64 + jj + 32 * hi
    else:
        off = ((ii >> 2) * 32 + jj) * 4 + (ii & 3)
    return ((i >> 5) * (NTOK // TILE) + (j >> 5)) * (TILE * TILE) + off


def ds_place(ds, layout, swapped=False):
    """[ZH, 576, 576] -> the flat tiled image [ZH, 576 * 576]"""
    off = ds_offsets(layout, swapped).flatten().to(ds.device)
    out = torch.empty(ds.shape[0], NTOK * NTOK, dtype=ds.dtype, device=ds.device)
    out[:, off] = ds.reshape(ds.shape[0], -1)
    return out


def ds_b(Z, H, bits12, *key):
    """b [Z, 576, H * 64]: small_int, or 12-bit odd integers (the operand the bf16 form rounds on chip)"""
    shape = (Z * NTOK, H * 64)
    return (_x12(*shape, 51, *key) if bits12 else G._ints(shape, -7, 7, 53, *key)).view(Z, NTOK, H * 64)


def ds_reference(ds, b, Z, H, b_xor):
    """fp64 (out [Z * 576, H * 64], colpart [Z * 18, H * 64]): out[z][i][h 64 + d] = sum_j ds[z H + h][i][j] b[z ^ b_xor][j][h 64 + d]"""
    bz = b[torch.arange(Z, device=b.device) ^ b_xor].view(Z, NTOK, H, 64)
    out = torch.einsum("zhij,zjhd->zihd", ds.view(Z, H, NTOK, NTOK), bz).reshape(Z * NTOK, H * 64)
    return out, out.view(Z * NTOK // TILE, TILE, H * 64).sum(1)


# ------------------------------------------------------------------------------------------------ rp_mlp_fused_bwd_ln
LN_SUB = 4


@functools.lru_cache(maxsize=None)
def mlp_bwd_ln_operands(M):
    """rp_mlp_fused_bwd's operands at smaller magnitudes (dy, w1t in [-1, 1], w2t in [-3, 3]) plus a LayerNorm whose xhat is a small
    multiple of 1/2: integer mean in [-8, 8], rstd in {1, 1/2}, x - mean an integer in [-4, 4] (ln_x, ln_mean, ln_rstd are INPUTS).  Then
    dxn o xhat, dxn and dy are multiples of 1/4 and all three thirds of ln_part are exact, which exposes dxn -- it never reaches memory."""
    key = (M, 80)
    P = base_rows(M)
    return dict(dy=G._ints((P, C), -1, 1, 1, *key), hpre=preact(P, HID, 2, *key), w2t=G._ints((HID, C), -3, 3, 3, *key),
                w1t=G._ints((C, HID), -1, 1, 4, *key), xc=G._ints((P, C), -4, 4, 5, *key), mean=G._ints((P,), -8, 8, 6, *key),
                rexp=G._ints((P,), -1, 0, 7, *key), gamma=G._ints((C,), -7, 7, 8, *key))


def ln_part_reference(dxn, xhat, dy, share, rows=192):
    """fp64 ln_part [tiles * 4][3 * 192]: per block of rows / 4 rows the column sums of (dxn o xhat | dxn | dy); a tile its owner finished
    (share == 1) has the whole tile's sums in its first row and zeros in the other three.  Rows past M count nothing."""
    M, T = dxn.shape[0], share.numel()
    cat = torch.zeros(T * rows, 3 * C, dtype=dxn.dtype, device=dxn.device)
    cat[:M] = torch.cat([dxn * xhat, dxn, dy], 1)
    sub = cat.view(T, LN_SUB, rows // LN_SUB, 3 * C).sum(2)
    own = (share == 1).to(dxn.device)
    whole = sub.sum(1)
    sub[own] = 0
    sub[own, 0] = whole[own]
    return sub.view(T * LN_SUB, 3 * C), float(torch.cat([(dxn * xhat).abs(), dxn.abs(), dy.abs()], 1).sum(0).max()) if T == 1 else None


# ------------------------------------------------------------------------------------------------ rp_dx_lnbwd_bf16
@functools.lru_cache(maxsize=None)
def dx_lnbwd_operands(M):
    """dy [M,576] and wt = W^T [192,576] in [-3, 3] (exact in bf16), add in [-64, 64], and the integer-grade LayerNorm of
    mlp_bwd_ln_operands: dxn = dy W is an integer, dxn o xhat a multiple of 1/2, every plane of `part` exact"""
    key = (M, 81)
    return dict(dy=G._ints((M, 576), -3, 3, 1, *key), wt=G._ints((C, 576), -3, 3, 2, *key), add=G._ints((M, C), -64, 64, 3, *key),
                xc=G._ints((M, C), -4, 4, 5, *key), mean=G._ints((M,), -8, 8, 6, *key), rexp=G._ints((M,), -1, 0, 7, *key),
                gamma=G._ints((C,), -7, 7, 8, *key))


def dx_lnbwd_part(dxn, xhat, add, rows):
    """fp64 part [tiles][np][192]: per tile of `rows` rows the column sums of dxn o xhat, dxn and (np = 3) add"""
    planes = [dxn * xhat, dxn] + ([] if add is None else [add])
    M, T = dxn.shape[0], -(-dxn.shape[0] // rows)
    pad = torch.zeros(T * rows, len(planes), C, dtype=dxn.dtype, device=dxn.device)
    pad[:M] = torch.stack(planes, 1)
    return pad.view(T, rows, len(planes), C).sum(1)
