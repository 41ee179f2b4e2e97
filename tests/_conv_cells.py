"""Exact-arithmetic operands, integer references, mutants and the case table for the hand-written convolutions (csrc/conv*.hip: nine
entry points, and the autograd nodes of ops.py that rotate and role-swap their filters).  torch only, no GPU and no library at import:
tests/test_conv_cells_cpu.py proves the premises on the CPU, tests/test_gpu_conv_cells.py runs the table on the device.

The method is tests/_gemm_cells.py's.  Operands are integers times one power of two (kept as int64 tensors with a binary exponent), chosen
so that every product and every partial sum, in ANY order, stays below 2^24 on the case's grid: fp32 and bf16-MFMA accumulation, the
per-workgroup partials, the fixed-order reduces and the double statistics are then exact, and the kernel must equal the reference BIT FOR
BIT (torch.equal).  A bf16-stored output must equal the exact value rounded ONCE to nearest even.  The references are sums of fp64
matmuls, one per filter tap, on NHWC operands (conv_ref / wgrad_ref / rot); the CPU test checks them against fp64 F.conv2d, its autograd
and an int64 unfold-matmul.

Families
  dense        x, dY, res iid integers (|x|, |dY| <= 3; res, bias in [-64, 64]), w iid integers * 2^-3 with |w| <= 7 for the fp32 kernels.
               bf16-STORED outputs take |w| <= 31 (the stem: |x| <= 15 too): the exact values then reach 12 and more significant bits, and
               only from 12 bits on does a double rounding (through 11 bits, as fp16 / tf32 keep) differ from one rounding; with |w| <= 7 the
               3x3 sums stay near 10 bits.  The bounds hold with room: 576 * 3 * 31 = 53 568.
  dense_small  x, w in {-1, 0, 1}: the statistics cases of the kernels whose epilogue sums y and y^2 in fp32 per lane before the double
               (conv3x3_bf16.hip over a workgroup's run, conv_stem*.hip over a wave's tiles): sum y^2 of a whole run must stay below
               2^24 as well (stat_group_bound).  conv3x3_f32.hip / conv3x3_c128_f32.hip sum in double from the first addition and take `dense`.
  sparse       the bf16 weight gradient: dY is zero except at a chosen pixel set (sparse_pixels: the first and last pixel of every
               workgroup's run, the first and last row of every 4-row strip, rows 0 / 55, columns 0 / 55, both ends of the 16-pixel k-steps 3
               and 10 that straddle an image row), +-1 there in 4 of the 64 channels; x is +-1 everywhere (a halo position read where zero
               padding belongs contributes).  Every exact result is an integer of magnitude <= 255: <= 8 significant bits, so dropping any
               single product changes the STORED bf16 value.  (The kernel also runs `dense`: its fp32 partials and reduce are exact
               there too, which pins the ONE rounding of its final store -- the sparse results never round.)
  impulse      x is one-hot at corners, edge mid-points, tile seams and the interior; w[co][r][s][ci] = 1 + tap + taps * ((co + 2 ci) mod M),
               <= 252: injective in the tap per (co, ci) pair and not symmetric in (co, ci), exact in bf16.  The output is the filter laid
               around the impulse and names tap, rotation and channel role-swap when it is wrong.
  bn_exact     BN + ReLU on load (conv3x3_bf16.hip): scale in {+-1/2, +-1, +-2}, integer shifts in [-2, 2] of both signs: max(0, x scale +
               shift) is exact and bf16-representable, a wrongly activated pad position is max(0, shift) > 0 (bn_exact_small: x, w in
               {-1, 0, 1} for the form that also sums the statistics in fp32).  RpBnMask (conv3x3_f32.hip):
               integer mean and beta, rstd and gamma powers of two: fma(x - mean, rstd gamma, beta) is exact; every fifth element lands
               exactly on 0 with values of both signs next to it; the masked gradient and the partial sums of g and g xhat are exact.

The table (table(); required(): the (kernel, form, seam) cells it must hold, derived from FORMS and the seam lists, not from the table).
Fixed-shape kernels: N in {1, 3, 37} ({1, 3, 5} for the stem weight gradients) = runs of at most one tile and runs of several tiles that
start and end inside an image (tiles_of / groups_of mirror the launchers; the GPU test checks the mirror against the library's *_blocks()).
Stem forward: 32 x 32 (OW % 16 == 0), 37 x 44 and 64 x 100 (ragged 16-pixel tile, odd H), and 224 x 224 at the smallest N <= 16 for which
a wave takes more than one tile (wrap_n: decided on the device from rp_conv_stem_blocks)."""
import collections
import functools

import torch

LIM = 1 << 24
NWG = 256
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
EW = -3                                   # binary exponent of the dense filters
WRAP_MAX_N = 16

Case = collections.namedtuple("Case", "kernel form family N H W")

# kernel -> (H, W, input channels, output channels, filter size, stride, tiles per image, bf16-stored output)
GEOM = collections.OrderedDict([
    ("c64_f32", (56, 56, 64, 64, 3, 1, 28, False)), ("c128_f32/128", (28, 28, 128, 128, 3, 1, 7, False)),
    ("c128_f32/192", (28, 28, 128, 192, 3, 1, 7, False)), ("c64_bf16", (56, 56, 64, 64, 3, 1, 14, True)),
    ("wgrad_f32", (56, 56, 64, 64, 3, 1, 56, False)), ("wgrad_bf16", (56, 56, 64, 64, 3, 1, 14, True)),
    ("stem_f32", (None, None, 3, 64, 7, 2, None, False)), ("stem_bf16", (None, None, 3, 64, 7, 2, None, True)),
    ("stem_wgrad_f32", (224, 224, 3, 64, 7, 2, 112, False)), ("stem_wgrad_bf16", (224, 224, 3, 64, 7, 2, 56, False))])

# every epilogue option of every kernel: kernel -> form -> families it runs on
FORMS = collections.OrderedDict([
    ("c64_f32", collections.OrderedDict([("fwd", ("dense", "impulse")), ("fwd_stats", ("dense",)), ("fwd_res_stats", ("dense",)),
                                         ("dx", ("dense", "impulse")), ("dx_res", ("dense",)), ("dx_bn", ("bn_exact",))])),
    ("c128_f32/128", collections.OrderedDict([("fwd", ("dense", "impulse")), ("fwd_stats", ("dense",)), ("fwd_bias_stats", ("dense",)),
                                              ("dx", ("dense", "impulse"))])),
    ("c128_f32/192", collections.OrderedDict([("fwd", ("dense", "impulse")), ("fwd_bias", ("dense",)), ("fwd_bias_stats", ("dense",))])),
    ("c64_bf16", collections.OrderedDict([("plain", ("dense", "impulse")), ("stats", ("dense_small",)), ("bn", ("bn_exact",)),
                                          ("bn_stats", ("bn_exact_small",)), ("dx_fn", ("dense", "impulse"))])),
    ("wgrad_f32", collections.OrderedDict([("dw", ("dense",))])),
    ("wgrad_bf16", collections.OrderedDict([("dw", ("sparse", "dense"))])),
    ("stem_f32", collections.OrderedDict([("fwd", ("dense", "impulse")), ("fwd_stats", ("dense_small",))])),
    ("stem_bf16", collections.OrderedDict([("fwd", ("dense", "impulse")), ("fwd_stats", ("dense_small",))])),
    ("stem_wgrad_f32", collections.OrderedDict([("dw", ("dense",))])),
    ("stem_wgrad_bf16", collections.OrderedDict([("dw", ("dense",))]))])

NS = {k: ((1, 3, 5) if k.startswith("stem_wgrad") else (1, 3, 37)) for k in GEOM if GEOM[k][0] is not None}
STEM_SHAPES = ((1, 32, 32, "aligned"), (2, 37, 44, "ragged"), (3, 64, 100, "ragged"), (None, 224, 224, "wrap"))
STEM_SNW = 8                              # waves of a stem workgroup; a wave walks tile, tile + 8 * blocks, ...
FP32_STATS = ("c64_bf16", "stem_f32", "stem_bf16")      # statistics summed in fp32 per lane before the double


def name(c):
    return "%s/%s/%s N=%s %sx%s" % (c.kernel, c.form, c.family, c.N, c.H, c.W)


# ------------------------------------------------------------------------------------------------ the mirror of the launchers
def tiles_of(kernel, N):
    return N * GEOM[kernel][6]


def groups_of(kernel, N):
    """workgroups (c128: tile chunks) that share the tiles -- rp_*_blocks() of the library"""
    t = tiles_of(kernel, N)
    if kernel.startswith("c128_f32"):
        ncg = GEOM[kernel][3] // 64
        per8 = 32 // ncg
        while per8 > 1 and 8 * (per8 - 1) >= t:
            per8 -= 1
        return 8 * per8
    return min(t, NWG)


def runs(kernel, N):
    """[t0, t1) of every workgroup, as the kernels cut them"""
    t, g = tiles_of(kernel, N), groups_of(kernel, N)
    return [(t * b // g, t * (b + 1) // g) for b in range(g)]


def seam(kernel, N):
    return "multi" if max(t1 - t0 for t0, t1 in runs(kernel, N)) > 1 else "single"


def stem_out(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def stem_tiles(N, H, W):
    oh, ow = stem_out(H, W)
    return N * oh * ((ow + 15) // 16)


def wrap_n(blocks_fn, H=224, W=224):
    """smallest N <= WRAP_MAX_N at which a wave of the stem forward takes a second tile, or None; blocks_fn(N, H, W) = rp_conv_stem*_blocks"""
    for N in range(1, WRAP_MAX_N + 1):
        if stem_tiles(N, H, W) > STEM_SNW * blocks_fn(N, H, W):
            return N
    return None


def stem_path(N, H, W, blocks):
    if stem_tiles(N, H, W) > STEM_SNW * blocks:
        return "wrap"
    return "ragged" if stem_out(H, W)[1] % 16 else "aligned"


# ------------------------------------------------------------------------------------------------ operands
def _gen(*key):
    g = torch.Generator()
    seed = 54321
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    g.manual_seed(seed)
    return g


def _ints(shape, lo, hi, *key):
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(*key), dtype=torch.int64)


def _sign(shape, *key):
    return _ints(shape, 0, 1, *key) * 2 - 1


def amplitude(kernel, family):
    """(max |x| or |dY|, max |w| in units of 2^EW)"""
    if family in ("dense_small", "bn_exact_small"):
        return 1, 1
    if kernel == "stem_bf16":
        return 15, 31
    if kernel == "c64_bf16":
        return 3, 31
    return 3, 7


def impulse_filter(co, k, ci):
    """[co][k][k][ci] int64: 1 + tap + taps * ((co + 2 ci) mod M), at most 252"""
    taps = k * k
    M = 252 // taps - 1
    o, c = torch.arange(co).view(-1, 1, 1, 1), torch.arange(ci).view(1, 1, 1, -1)
    tap = (torch.arange(k).view(1, -1, 1, 1) * k + torch.arange(k).view(1, 1, -1, 1))
    return 1 + tap + taps * ((o + 2 * c) % M)


def impulse_positions(N, H, W):
    """(n, y, x) of the impulses: corners, edge mid-points, the seams of 2-row / 4-row tiles and 16-pixel blocks, the interior"""
    h, w = H - 1, W - 1
    pos = [(0, 0), (0, w), (h, 0), (h, w), (0, w // 2), (h // 2, 0), (h, w // 2 + 1), (h // 2 + 1, w), (1, 15), (2, 16), (3, min(31, w)),
           (4, min(32, w)), (3, w), (4, 0), (H // 2 + 2, W // 2 + 2), (h - 4, w - 8), (h - 3, w - 7)]
    out = [(k % N, y, x) for k, (y, x) in enumerate(pos)] + [(N - 1, h, w), (N - 1, 0, 0), (N // 2, h // 2, 15), (N // 2, h // 2, 16)]
    return [(n, min(max(y, 0), h), min(max(x, 0), w)) for n, y, x in out]


def impulse_tensor(N, H, W, C):
    x = torch.zeros(N, H, W, C, dtype=torch.int64)
    for k, (n, y, xx) in enumerate(impulse_positions(N, H, W)):
        x[n, y, xx, (7 * k + 3) % C] = 1
    return x


STRIP_PIX = (0, 55, 56, 111, 112, 167, 168, 223, 48, 63, 160, 175, 100)      # of a 4 x 56 strip: row ends, k-steps 3 and 10 (48..63, 160..175)


def sparse_pixels(N):
    """flat pixel indices (over [N, 56, 56]) that carry the non-zeros of the sparse dY; a strip tile is 224 consecutive pixels"""
    nt = tiles_of("wgrad_bf16", N)
    P = set()
    for t0, t1 in runs("wgrad_bf16", N):
        if t0 < t1:
            P.update((t0 * 224, t1 * 224 - 1))                    # first and last pixel of the run
    for t in range(nt):
        P.update((t * 224 + (5 * t) % 56, t * 224 + 168 + (11 * t + 7) % 56))      # first and last row of every strip
    for t in sorted({0, 13, nt // 2, nt - 14, nt - 1}):              # strips with image rows 0 and 55; every listed position of a strip
        P.update(t * 224 + p for p in STRIP_PIX)
    return sorted(P)


BN_SCALES = (0.5, -1.0, 2.0, -0.5, 1.0, -2.0)


@functools.lru_cache(maxsize=3)
def _operands(kernel, family, N, H, W):
    """int64 tensors (NHWC; w [co][k][k][ci]) and binary exponents.  `x` is the kernel's streamed operand (dY for the dx forms)."""
    _, _, ci, co, k, stride, _, _ = GEOM[kernel]
    kid = list(GEOM).index(kernel)
    key = (kid, N, H, W)
    o = dict(ex=0, ew=EW, e_dy=0)
    oh, ow = (H, W) if stride == 1 else stem_out(H, W)
    xa, wa = amplitude(kernel, family)
    if family == "impulse":
        o["x"], o["w"], o["ew"] = impulse_tensor(N, H, W, ci), impulse_filter(co, k, ci), 0
        o["dy"] = impulse_tensor(N, oh, ow, co)
    elif family == "sparse":
        o["x"] = _sign((N, H, W, ci), 1, *key)
        dy = torch.zeros(N * H * W, co, dtype=torch.int64)
        P = torch.tensor(sparse_pixels(N))
        cls = torch.arange(len(P)) % 16
        ch = cls.view(-1, 1) + 16 * torch.arange(4).view(1, -1)
        dy[P.view(-1, 1), ch] = _sign(ch.shape, 2, *key)
        o["dy"], o["w"] = dy.view(N, H, W, co), _ints((co, k, k, ci), -wa, wa, 3, *key)
    else:
        o["x"], o["w"] = _ints((N, H, W, ci), -xa, xa, 1, *key), _ints((co, k, k, ci), -wa, wa, 3, *key)
        o["dy"] = _ints((N, oh, ow, co), -3, 3, 2, *key)
    o["bias"] = _ints((co,), -64, 64, 4, *key)
    if kernel == "c64_f32":
        o["res"] = _ints((N, H, W, co), -64, 64, 5, *key)
    if family.startswith("bn_exact") and kernel == "c64_bf16":
        c = torch.arange(ci)
        o["scale"] = torch.tensor(BN_SCALES, dtype=F64)[c % 6]
        o["shift"] = (c * 2 + c // 6) % 5 - 2
    if family == "bn_exact" and kernel == "c64_f32":
        c = torch.arange(co)
        o["mean"], o["beta"] = (c * 3 + c // 5) % 5 - 2, (c * 2 + c // 7) % 5 - 2
        o["rstd"] = torch.tensor((0.5, 0.25), dtype=F64)[c % 2]
        o["gamma"] = torch.tensor((1.0, -2.0, 2.0, -1.0, 1.0), dtype=F64)[c % 5]
        rg = o["rstd"] * o["gamma"]
        x0 = o["mean"].double() - o["beta"].double() / rg                  # fma(x0 - mean, rstd gamma, beta) == 0
        assert torch.equal(x0, x0.round())
        xb = _ints((N * H * W, co), -8, 8, 6, *key)
        i = torch.arange(N * H * W).view(-1, 1) + torch.arange(co).view(1, -1)      # the planted pattern shifts per channel
        xb = torch.where(i % 5 == 0, x0.long().expand_as(xb), xb)
        xb = torch.where(i % 5 == 1, (x0.long() + 1).expand_as(xb), xb)
        xb = torch.where(i % 5 == 2, (x0.long() - 1).expand_as(xb), xb)
        o["bn_x"] = xb.view(N, H, W, co)
    return o


def operands(c):
    return _operands(c.kernel, c.family, c.N, c.H, c.W)


def values(c, device="cpu"):
    """the operands as exact fp64 values on `device`"""
    o = operands(c)
    v = {}
    for k, e in (("x", "ex"), ("w", "ew"), ("dy", "e_dy"), ("bias", None), ("res", None), ("shift", None), ("mean", None), ("beta", None),
                 ("bn_x", None)):
        if k in o:
            v[k] = o[k].to(device).double() * 2.0 ** (o[e] if e else 0)
    for k in ("scale", "rstd", "gamma"):
        if k in o:
            v[k] = o[k].to(device)
    return v


def frame(x, pad=3):
    """[N,H,W,C] -> the image inside a `pad`-pixel zero frame"""
    return torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))


# ------------------------------------------------------------------------------------------------ references (fp64, one matmul per tap)
def conv_ref(x, w, stride=1, pad=1):
    """x [N,H,W,ci], w [co][kh][kw][ci] -> [N,OH,OW,co] = sum over taps of x[n, s oy + r - pad, s ox + q - pad, :] w[:, r, q, :]^T"""
    N, H, W, ci = x.shape
    co, kh, kw, _ = w.shape
    xp = frame(x, pad) if pad else x
    oh, ow = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    y = torch.zeros(N * oh * ow, co, dtype=x.dtype, device=x.device)
    for r in range(kh):
        for q in range(kw):
            xs = xp[:, r:r + stride * (oh - 1) + 1:stride, q:q + stride * (ow - 1) + 1:stride]
            y += xs.reshape(-1, ci) @ w[:, r, q].t()
    return y.view(N, oh, ow, co)


def wgrad_ref(x, dy, k=3, stride=1, pad=1):
    """dW [co][k][k][ci] = sum over pixels of dY[n, oy, ox, co] x[n, s oy + r - pad, s ox + q - pad, ci]"""
    N, oh, ow, co = dy.shape
    xp = frame(x, pad) if pad else x
    dyt = dy.reshape(-1, co).t().contiguous()
    dw = torch.zeros(co, k, k, x.shape[-1], dtype=x.dtype, device=x.device)
    for r in range(k):
        for q in range(k):
            xs = xp[:, r:r + stride * (oh - 1) + 1:stride, q:q + stride * (ow - 1) + 1:stride]
            dw[:, r, q] = dyt @ xs.reshape(-1, x.shape[-1])
    return dw


def rot(w):
    """the input gradient's filter w'[ci][r][s][co] = w[co][2 - r][2 - s][ci] (any odd size)"""
    return w.flip(1, 2).permute(3, 1, 2, 0).contiguous()


def rot_without_swap(w):
    """MUTANT: rotated, channel roles kept (square filters)"""
    return w.flip(1, 2).contiguous()


def stats_ref(y):
    """[2][C]: sums of y and y^2 over all pixels"""
    y2 = y.reshape(-1, y.shape[-1])
    return torch.stack((y2.sum(0), y2.square().sum(0)))


def bn_on_load(v):
    """max(0, x scale + shift) of conv3x3_bf16.hip's operand load; the zero padding is added AFTER it"""
    return (v["x"] * v["scale"] + v["shift"]).clamp_min(0)


def bn_on_load_pad_activated(v, w):
    """MUTANT: the activation also applied to the 58-column halo border"""
    return conv_ref((frame(v["x"], 1) * v["scale"] + v["shift"]).clamp_min(0), w, 1, 0)


def bn_mask(v, strict=True):
    """the ReLU mask of RpBnMask: fma(x - mean, rstd gamma, beta) > 0 (strict=False: the MUTANT >=)"""
    pre = (v["bn_x"] - v["mean"]) * (v["rstd"] * v["gamma"]) + v["beta"]
    return pre > 0 if strict else pre >= 0


def bn_partials(g, v):
    """[2][C]: sums of g and g xhat, xhat = (x - mean) rstd"""
    xh = (v["bn_x"] - v["mean"]) * v["rstd"]
    C = g.shape[-1]
    return torch.stack((g.reshape(-1, C).sum(0), (g * xh).reshape(-1, C).sum(0)))


def reference(c, v):
    """dict of the exact fp64 results of case c: out [, stats [2][C]]"""
    _, _, ci, co, k, stride, _, _ = GEOM[c.kernel]
    f = c.form
    r = {}
    if c.kernel.startswith("stem_wgrad"):
        r["out"] = wgrad_ref(frame(v["x"]), v["dy"], 7, 2, 0)
    elif c.kernel.startswith("wgrad"):
        r["out"] = wgrad_ref(v["x"], v["dy"])
    elif c.kernel.startswith("stem"):
        r["out"] = conv_ref(frame(v["x"]), v["w"], 2, 0)
    elif f.startswith("dx"):
        r["out"] = conv_ref(v["dy"], rot(v["w"]))
    elif f.startswith("bn"):
        r["out"] = conv_ref(bn_on_load(v), v["w"])
    else:
        r["out"] = conv_ref(v["x"], v["w"])
    if "bias" in f:
        r["out"] = r["out"] + v["bias"]
    if "res" in f:
        r["out"] = r["out"] + v["res"]
    if f == "dx_bn":
        r["out"] = torch.where(bn_mask(v), r["out"], torch.zeros_like(r["out"]))
        r["stats"] = bn_partials(r["out"], v)
    elif "stats" in f:
        r["stats"] = stats_ref(stored(c, r["out"]).double())
    return r


# ------------------------------------------------------------------------------------------------ roundings to bf16 (and the wrong ones)
def _bits(t):
    return t.float().contiguous().view(torch.int32)


def _round_bits(t, keep):
    """fp32 -> `keep` significant bits, round to nearest even, in integer arithmetic (finite, far from overflow)"""
    drop = 24 - keep
    b = _bits(t)
    lsb = (b >> drop) & 1
    return ((b + ((1 << (drop - 1)) - 1) + lsb) & ~((1 << drop) - 1)).view(F32)


def bf16_rne(t):
    return t.float().to(BF)


def bf16_rne_int(t):
    return _round_bits(t, 8).to(BF)


def bf16_trunc(t):
    """MUTANT: truncation"""
    return (_bits(t) & -65536).view(F32).to(BF)


def bf16_half_up(t):
    """MUTANT: round half away from zero (add half an ulp to the magnitude, truncate)"""
    return ((_bits(t) + 0x8000) & -65536).view(F32).to(BF)


def bf16_double(t):
    """MUTANT: rounded twice -- to 11 significant bits (what fp16 and tf32 keep), then to bf16"""
    return _round_bits(_round_bits(t, 11), 8).to(BF)


def stored(c, out64):
    """the exact result as the kernel stores it"""
    return bf16_rne(out64) if GEOM[c.kernel][7] else out64.float()


# ------------------------------------------------------------------------------------------------ bounds
def sum_bound(c):
    """largest sum |a| |b| (+ |bias| + |res|) any output element can take, in units of the case's grid: analytic, from the operand ranges"""
    _, _, ci, co, k, stride, _, _ = GEOM[c.kernel]
    o = operands(c)
    unit = min(0, o["ew"])
    if "wgrad" in c.kernel:
        if c.family == "sparse":
            return None                                           # measured: sparse_count
        oh, ow = (c.H, c.W) if stride == 1 else stem_out(c.H, c.W)
        return c.N * oh * ow * int(o["x"].abs().max()) * int(o["dy"].abs().max())
    xmax = int((o["dy"] if c.form.startswith("dx") else o["x"]).abs().max())
    if c.form.startswith("bn"):
        xmax, unit = 2 * (2 * xmax + 2), unit - 1               # max(0, x scale + shift) <= 2 |x| + 2, in halves
    b = k * k * ci * xmax * int(o["w"].abs().max())
    if "bias" in c.form:
        b += 64 << -unit
    if "res" in c.form:
        b += 64 << -unit
    return b


def stat_group_bound(c, y64, blocks=None):
    """kernels of FP32_STATS: the largest sum of y^2 (in units of the result's grid) over the pixels whose values ONE fp32 accumulation
    chain can see -- a workgroup's whole run (conv3x3_bf16.hip) or a wave's tiles (the stems) -- per channel; sum |y| is below it"""
    o = operands(c)
    e = o["ew"] - (1 if c.form.startswith("bn") else 0)
    u = (y64 * 2.0 ** -e)
    assert torch.equal(u, u.round())
    C = u.shape[-1]
    u2 = u.square()
    if c.kernel == "c64_bf16":
        per_tile = u2.reshape(-1, 224, C).sum(1)
        return max(float(per_tile[t0:t1].sum(0).max()) for t0, t1 in runs(c.kernel, c.N) if t0 < t1)
    N, oh, ow, _ = u.shape
    tx = (ow + 15) // 16
    pad = torch.zeros(N, oh, tx * 16, C, dtype=u.dtype, device=u.device)
    pad[:, :, :ow] = u2
    per_tile = pad.view(N * oh * tx, 16, C).sum(1)
    nwaves = STEM_SNW * blocks
    rows = -(-per_tile.shape[0] // nwaves) * nwaves
    full = torch.zeros(rows, C, dtype=u.dtype, device=u.device)
    full[:per_tile.shape[0]] = per_tile
    return float(full.view(-1, nwaves, C).sum(0).max())


def bn_chain_bound(c, v, g64):
    """RpBnMask: conv3x3_f32.hip sums g and g xhat over a tile's seven pixels per lane in fp32 (double above that): 7 max |g| max |xhat| on
    the product's grid"""
    o = operands(c)
    xh = ((v["bn_x"] - v["mean"]) * v["rstd"]).abs().max() * 4          # rstd >= 1/4
    return 7 * float(g64.abs().max() * 2.0 ** -o["ew"]) * float(xh)


# ------------------------------------------------------------------------------------------------ the table
def _fixed_cases():
    out = []
    for kernel, ns in NS.items():
        H, W = GEOM[kernel][:2]
        for N in ns:
            for form, fams in FORMS[kernel].items():
                for fam in fams:
                    if fam == "impulse" and N == 37:
                        continue                                   # the impulse names taps and roles: one multi-image size is enough
                    out.append(Case(kernel, form, fam, N, H, W))
    return out


def _stem_cases():
    out = []
    for kernel in ("stem_f32", "stem_bf16"):
        for N, H, W, _ in STEM_SHAPES:
            for form, fams in FORMS[kernel].items():
                for fam in fams:
                    if fam == "impulse" and N is None:
                        continue
                    out.append(Case(kernel, form, fam, N, H, W))
    return out


@functools.lru_cache(maxsize=None)
def table():
    return tuple(_fixed_cases() + _stem_cases())


def keys():
    """(kernel, N, H, W) of the GPU tests, in table order; N = None: the wrap case, sized on the device"""
    return list(dict.fromkeys((c.kernel, c.N, c.H, c.W) for c in table()))


def cases(kernel, N, H, W):
    return [c for c in table() if (c.kernel, c.N, c.H, c.W) == (kernel, N, H, W)]


STEM_PATHS = ("aligned", "ragged", "ragged_odd_h", "wrap", "odd_w_refused")


def required():
    """the (kernel, form, seam) cells the table must hold: every epilogue option of every kernel at one N with single-tile workgroups and one
    with multi-tile runs; every stem form on every stem path.  Enumerated from FORMS and the launch mirror, not from the table."""
    req = set()
    for kernel, forms in FORMS.items():
        for form in forms:
            if kernel in NS:
                req.update((kernel, form, s) for s in ("single", "multi"))
            else:
                req.update((kernel, form, p) for p in STEM_PATHS[:4])
        if kernel not in NS:
            req.add((kernel, "refusal", "odd_w_refused"))
    return req


def hit(stem_slots=512):
    """the same projection of the table (+ the refusal rows of the GPU test, REFUSALS); the wrap case counts when wrap_n finds an N for a
    device with `stem_slots` resident stem workgroups"""
    got = set()
    for c in table():
        if c.kernel in NS:
            got.add((c.kernel, c.form, seam(c.kernel, c.N)))
            continue
        blocks = lambda N, H, W: min(-(-stem_tiles(N, H, W) // STEM_SNW), stem_slots)
        N = c.N if c.N is not None else wrap_n(blocks, c.H, c.W)
        if N is None:
            continue
        p = stem_path(N, c.H, c.W, blocks(N, c.H, c.W))
        got.add((c.kernel, c.form, p))
        if p == "ragged" and c.H % 2:
            got.add((c.kernel, c.form, "ragged_odd_h"))
    got.update((k, "refusal", "odd_w_refused") for k, _, _ in REFUSALS)
    return got


# odd W: 2 (OW - 1) + 8 > W + 6 -- the last window's pad taps would leave its row -- RP_EBADSHAPE before anything is launched
REFUSALS = (("stem_f32", 2, (32, 33)), ("stem_f32", 1, (37, 43)), ("stem_bf16", 2, (32, 33)), ("stem_bf16", 1, (37, 43)))
