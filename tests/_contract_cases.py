"""Memory-contract cases of the C ABI (include/relpose_hip.h): one table entry per launching entry point.

The header's conventions make the contract testable: the library never allocates, uses no atomics and no memsets, and is
deterministic -- so what an entry point leaves in memory may depend only on its inputs, never on what its outputs or workspace held
before the call.  A case describes ONE direct call (ctypes, through _lib.load(), not through rel_pose_amd/ops.py):

  * every operand with its role -- input (`const` in the header), output, workspace;
  * for every output the columns the header documents as written (`wins`); everything else inside the operand -- the gap columns
    of a row stride larger than the width, the other thirds of a shared dqkv -- must come back untouched;
  * optional checks of the values (documented zero padding, an fp64 reference at the bound of the kernel's own parity test).

Operands are carved from one larger allocation each with a GUARD BAND on both sides: max(1 MiB, 256 rows x ld x element size).  A
whole-tile overrun (a 32- / 64- / 256-row tile past the last row, a 1 KB / 4 KB accumulator run past the end) lands in memory the
test owns and is reported with operand name and offset.  OVERRUNS BEYOND THE GUARD ARE OUT OF REACH of this module: a kernel that
computes a wild address (a wrong image index times the image size) is not caught here.

Guards, gaps and (in the first of the two runs) outputs and workspaces hold a sentinel per element type: fp32 a NaN with payload
0x7FC0DEAD, bf16 0x7FAD, double a NaN with payload 0x7FF8DEADDEADDEAD, bytes 0xA5, int 0x7FC0DEAD.  The second run pre-fills outputs
and workspaces with a finite pattern (12345.0; bytes 0x5A; int 0x12345678) instead.

Importing this module touches neither CUDA nor the library: builders only run when tests/test_gpu_memory_contract.py calls them.
CASES maps an entry point to its builders, UNCOVERED maps the entry points without one to the reason."""
import ctypes
import functools
import math
import struct

import torch

P = ctypes.c_void_p
F32, BF16, F64, U8, I32 = torch.float32, torch.bfloat16, torch.float64, torch.uint8, torch.int32

_BITS = {F32: torch.int32, BF16: torch.int16, F64: torch.int64, U8: torch.uint8, I32: torch.int32}
SENTINEL = {F32: 0x7FC0DEAD, BF16: 0x7FAD, F64: 0x7FF8DEADDEADDEAD, U8: 0xA5, I32: 0x7FC0DEAD}
FINITE = {F32: struct.unpack("<i", struct.pack("<f", 12345.0))[0], BF16: struct.unpack("<i", struct.pack("<f", 12345.0))[0] >> 16,
          F64: struct.unpack("<q", struct.pack("<d", 12345.0))[0], U8: 0x5A, I32: 0x12345678}
GUARD_MIN_BYTES = 1 << 20
GUARD_ROWS = 256

N_TOK, DIM, HEADS, XW, GW, NWG = 576, 192, 3, 96, 224, 6
SCALE = 64 ** -0.5


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    return torch.randn(*shape, generator=g) * scale


class Operand:
    """role 'in' / 'out' / 'ws' / 'inout' (read and updated in place: the running statistics); the operand is [rows, ld] elements of `dtype` (a flat array: rows = 1).
    in : values = {first column: CPU tensor [rows, width]} -- the rest (gaps) holds the sentinel, which a kernel must not use.
    out: wins = {name: (c0, c1)} -- the column windows the call writes in every row; everything else must stay untouched."""

    def __init__(self, name, role, dtype, rows, ld, values=None, wins=None):
        self.name, self.role, self.dtype, self.rows, self.ld = name, role, dtype, int(rows), int(ld)
        self.values, self.wins = values or {}, wins or {}
        self.esize = torch.empty(0, dtype=dtype).element_size()
        g = max(GUARD_MIN_BYTES, GUARD_ROWS * self.ld * self.esize)
        self.guard = -(-g // 256) * 256 // self.esize
        self.n = self.rows * self.ld

    def alloc(self, device, finite):
        bits = _BITS[self.dtype]
        self.arena = torch.full((self.guard + self.n + self.guard,), SENTINEL[self.dtype], dtype=bits, device=device)
        self.region = self.arena[self.guard:self.guard + self.n]
        self.fill = FINITE[self.dtype] if (finite and self.role != "in") else SENTINEL[self.dtype]
        if self.role in ("in", "inout"):
            r2 = self.region.view(self.rows, self.ld)
            for c0, v in self.values.items():
                v = v.to(self.dtype).reshape(self.rows, -1).contiguous()
                r2[:, c0:c0 + v.shape[1]] = v.view(bits).to(device)
        else:
            self.region.fill_(self.fill)
        self.before = self.region.clone() if self.role == "in" else None
        return self

    def addr(self, col=0, row=0):
        return self.region.data_ptr() + (row * self.ld + col) * self.esize

    def logical(self, c0, c1):
        return self.region.view(self.rows, self.ld)[:, c0:c1].clone().view(self.dtype)


def inp(name, t, ld=None, dtype=F32, col=0):
    t = t.reshape(t.shape[0], -1) if t.dim() > 1 else t.reshape(1, -1)
    return Operand(name, "in", dtype, t.shape[0], ld or (col + t.shape[1]), values={col: t})


def inp_multi(name, rows, ld, parts, dtype=F32):
    """one input buffer with several column blocks, e.g. the packed q | k | v"""
    return Operand(name, "in", dtype, rows, ld, values=parts)


def out(name, rows, width, ld=None, dtype=F32, wins=None):
    return Operand(name, "out", dtype, rows, ld or width, wins=wins if wins is not None else {name: (0, width)})


def inout(name, t):
    t = t.reshape(1, -1)
    return Operand(name, "inout", F32, 1, t.shape[1], values={0: t}, wins={name: (0, t.shape[1])})


def flat(name, n, dtype=F32):
    return Operand(name, "out", dtype, 1, n, wins={name: (0, n)})


def work(name, nbytes):
    assert nbytes % 4 == 0, nbytes
    return Operand(name, "ws", F32, 1, max(nbytes // 4, 0))


def a_(A_, n, col=0):
    return P(A_[n].addr(col)) if n in A_ else None


class Case:
    """operands: list of Operand; call(lib, A, st): performs the launch, A[name] is the Operand (A[name].addr(col) a device address);
    check(vals, report): optional value checks on vals[window name] (device tensors), returns a list of error strings;
    ws_probe(lib, A, st): optional, repeats the call with one float less of workspace_bytes (must raise RP_EWORKSPACE);
    sibling: optional builder of the packed-layout case whose windows must be bit-identical to this one's."""

    def __init__(self, operands, call, check=None, ws_probe=None, sibling=None):
        self.operands, self.call, self.check, self.ws_probe, self.sibling = operands, call, check, ws_probe, sibling


CASES = {}


def case(entry, ident):
    def deco(fn):
        fn.entry, fn.ident = entry, ident
        CASES.setdefault(entry, []).append(fn)
        return fn
    return deco


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _bound(errs, what, e, bound):
    if not e < bound:
        errs.append("%s: error %.3e against fp64 exceeds %.1e" % (what, e, bound))
    return e


# ================================================================================================ rp_gemm
def _gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def _gemm_case(M, N, K, ldc_extra=0, al=0, bl=0, bias=False, pre=False, act=0, dact=0, aux=False, residual=False, colsum=False,
               split_k=1, trans_c=False, batch=1, defer=False, bound=2e-6):
    """bound: test_gemm_layouts / test_gemm_epilogues_splitk_batch state 2e-6 of max|ref| for every fp32 rp_gemm form."""
    A, B = rnd(1, batch * M, K), rnd(2, batch * N, K, scale=K ** -0.5)
    Ain = A if al == 0 else A.view(batch, M, K).transpose(1, 2).reshape(batch * K, M)
    Bin = B if bl == 0 else B.view(batch, N, K).transpose(1, 2).reshape(batch * K, N)
    crows, ccols = (N, M) if trans_c else (M, N)
    ldc = ccols + ldc_extra
    ops_ = [inp("A", Ain), inp("B", Bin), out("C", batch * crows, ccols, ldc)]
    bv = rnd(3, N) if bias else None
    xv = rnd(4, M, N) if aux else None
    rv = rnd(5, M, N) if residual else None
    if bias:
        ops_.append(inp("bias", bv))
    if pre:
        ops_.append(out("pre_out", M, N, ldc))
    if aux:
        ops_.append(inp("aux", xv, ld=ldc))
    if residual:
        ops_.append(inp("residual", rv, ld=ldc))
    state = {}

    def sizes(lib):
        from rel_pose_amd import ops
        if colsum and "cs" not in state:
            tm, _ = ops.gemm_tile(M, N, al, bl, aux or residual, 0)
            state["cs"] = 2 * (-(-M // (64 * tm)))
        if split_k > 1 and "ws" not in state:
            state["ws"] = lib.rp_gemm_workspace_bytes(M, N, split_k)
        return state

    def struct_(lib, A_, wsb=None):
        from rel_pose_amd import _lib
        g = _lib.RpGemm()
        g.A, g.B, g.C = A_["A"].addr(), A_["B"].addr(), A_["C"].addr()
        g.M, g.N, g.K = M, N, K
        g.lda, g.ldb, g.ldc = (K if al == 0 else M), (K if bl == 0 else N), ldc
        g.a_layout, g.b_layout, g.batch = al, bl, batch
        g.stride_a, g.stride_b, g.stride_c = M * K, N * K, crows * ldc
        g.split_k = split_k
        if split_k > 1:
            g.workspace, g.workspace_bytes = A_["workspace"].addr(), (state["ws"] if wsb is None else wsb)
        for nm in ("bias", "pre_out", "aux", "residual", "colsum_part"):
            if nm in A_:
                setattr(g, nm, A_[nm].addr())
        g.act, g.dact, g.trans_c, g.precision, g.defer_reduce = act, dact, int(trans_c), 0, int(defer)
        return g

    def late(lib):                      # operands whose size the library reports
        s = sizes(lib)
        extra = []
        if colsum:
            extra.append(out("colsum_part", s["cs"], N))
        if split_k > 1:
            extra.append(work("workspace", s["ws"]))
        return extra

    def call(lib, A_, st):
        lib.rp_gemm(ctypes.byref(struct_(lib, A_)), st)
        if defer:
            from rel_pose_amd import _lib
            arr = (_lib.RpSplitkTask * 1)()
            arr[0].ws, arr[0].C, arr[0].M, arr[0].N, arr[0].ldc, arr[0].split_k, arr[0].trans_c = (
                A_["workspace"].addr(), A_["C"].addr(), M, N, ldc, split_k, int(trans_c))
            lib.rp_splitk_reduce_multi(arr, 1, st)

    def probe(lib, A_, st):
        lib.rp_gemm(ctypes.byref(struct_(lib, A_, state["ws"] - 4)), st)

    def check(v, errs):
        p = (A.double().view(batch, M, K) @ B.double().view(batch, N, K).transpose(1, 2))
        if bias:
            p = p + bv.double()
        e = {}
        if pre:
            e["pre_out"] = _bound(errs, "pre_out", rel(v["pre_out"], p[0]), bound)
        if act == 1:
            p = _gelu64(p)
        if act == 2:
            p = p.clamp_min(0)
        if dact == 1:
            x = xv.double()
            p = p * (0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * math.pi) ** 0.5)
        if dact == 2:
            p = p * (xv > 0)
        if residual:
            p = p + rv.double()
        if trans_c:
            p = p.transpose(1, 2)
        e["C"] = _bound(errs, "C", rel(v["C"], p.reshape(batch * crows, ccols)), bound)
        if colsum:      # test_gemm_epilogue_column_sums: 2e-6 against the sums of the stored values
            e["colsum"] = _bound(errs, "colsum_part", rel(v["colsum_part"].double().sum(0), v["C"].double().sum(0)), 2e-6)
        return e

    c = Case(ops_, call, check, probe if split_k > 1 else None)
    c.late = late
    return c


for _i, (_m, _n, _k) in enumerate([(130, 100, 36), (33, 16, 512), (200, 768, 192)]):
    for _x in (4, 64):
        case("rp_gemm", "%dx%dx%d-ldc+%d" % (_m, _n, _k, _x))(lambda m=_m, n=_n, k=_k, x=_x: _gemm_case(m, n, k, ldc_extra=x))
case("rp_gemm", "130x100x36-bias-gelu-pre-residual-ldc+4")(
    lambda: _gemm_case(130, 100, 36, ldc_extra=4, bias=True, pre=True, act=1, residual=True))
case("rp_gemm", "200x768x192-dgelu-aux-colsum")(lambda: _gemm_case(200, 768, 192, bl=0, dact=1, aux=True, colsum=True, bound=5e-6))
case("rp_gemm", "130x100x36-bias-colsum")(lambda: _gemm_case(130, 100, 36, bias=True, residual=True, colsum=True))
case("rp_gemm", "300x192x768-splitk5-epilogue")(
    lambda: _gemm_case(300, 192, 768, bias=True, act=2, residual=True, split_k=5))
case("rp_gemm", "130x100x36-splitk2-ldc+4")(lambda: _gemm_case(130, 100, 36, ldc_extra=4, split_k=2))
case("rp_gemm", "768x192x1152-dw-splitk6-trans_c")(lambda: _gemm_case(768, 192, 1152, al=1, bl=1, split_k=6, trans_c=True))
case("rp_gemm", "batch6-576x96x96")(lambda: _gemm_case(576, 96, 96, bl=1, batch=6))
case("rp_splitk_reduce_multi", "deferred-192x768x1152-splitk6")(
    lambda: _gemm_case(192, 768, 1152, al=1, bl=1, split_k=6, defer=True))
case("rp_splitk_reduce_multi", "deferred-trans_c-ldc+4")(
    lambda: _gemm_case(768, 192, 1152, al=1, bl=1, split_k=4, defer=True, trans_c=True, ldc_extra=4))


@case("rp_gemm", "ln-epilogue-M1000")
def _gemm_ln():
    """RpGemm.ln_*: C = LayerNorm'(A B^T) + residual at a ragged M; ln_part [ceil(M/64)][3*192].  Bound: the 5e-6 of
    test_gemm_with_fused_layernorm_backward (dx and the three column sums)."""
    M, N, K = 1000, 192, 576
    dy, W, x, g, res = rnd(1, M, K), rnd(2, N, K, scale=K ** -0.5), rnd(3, M, N), 1 + 0.1 * rnd(4, N), rnd(5, M, N)
    mean = x.double().mean(1)
    rstd = (x.double().var(1, unbiased=False) + 1e-6).rsqrt()
    nt = -(-M // 64)
    ops_ = [inp("A", dy), inp("B", W), inp("ln_x", x), inp("ln_mean", mean.float()), inp("ln_rstd", rstd.float()), inp("ln_gamma", g),
            inp("residual", res), out("C", M, N), out("ln_part", nt, 3 * N)]

    def call(lib, A_, st):
        from rel_pose_amd import _lib
        s = _lib.RpGemm()
        s.A, s.B, s.C = A_["A"].addr(), A_["B"].addr(), A_["C"].addr()
        s.M, s.N, s.K, s.lda, s.ldb, s.ldc, s.batch, s.split_k = M, N, K, K, K, N, 1, 1
        s.residual = A_["residual"].addr()
        s.ln_x, s.ln_mean, s.ln_rstd, s.ln_gamma, s.ln_part = (A_[n].addr() for n in ("ln_x", "ln_mean", "ln_rstd", "ln_gamma", "ln_part"))
        lib.rp_gemm(ctypes.byref(s), st)

    def check(v, errs):
        p = dy.double() @ W.double().t()
        xh = (x.double() - mean[:, None]) * rstd[:, None]
        gg = p * g.double()
        ref = rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True)) + res.double()
        sums = v["ln_part"].double().sum(0).cpu()
        return {"C": _bound(errs, "C", rel(v["C"], ref), 5e-6),
                "dgamma": _bound(errs, "ln_part dgamma", rel(sums[:N], (p * xh).sum(0)), 5e-6),
                "dbeta": _bound(errs, "ln_part dbeta", rel(sums[N:2 * N], p.sum(0)), 5e-6),
                "dres": _bound(errs, "ln_part residual", rel(sums[2 * N:], res.double().sum(0)), 5e-6)}
    return Case(ops_, call, check)


@case("rp_transpose_multi", "3-tasks-ragged")
def _transpose_multi():
    shapes = [(192, 768), (130, 36), (33, 100)]
    srcs = [rnd(10 + i, r, c) for i, (r, c) in enumerate(shapes)]
    ops_ = [inp("src%d" % i, s) for i, s in enumerate(srcs)] + [out("dst%d" % i, c, r) for i, (r, c) in enumerate(shapes)]

    def call(lib, A_, st):
        from rel_pose_amd import _lib
        arr = (_lib.RpTransposeTask * len(shapes))()
        for i, (r, c) in enumerate(shapes):
            arr[i].src, arr[i].dst, arr[i].rows, arr[i].cols = A_["src%d" % i].addr(), A_["dst%d" % i].addr(), r, c
        lib.rp_transpose_multi(arr, len(shapes), st)

    def check(v, errs):
        for i, s in enumerate(srcs):
            if not torch.equal(v["dst%d" % i].cpu(), s.t().contiguous()):
                errs.append("dst%d is not the exact transpose" % i)
        return {}
    return Case(ops_, call, check)


# ================================================================================================ row-resident Linear, fused MLP
def _rows_case(M, N, ln=False, act=0, pre=False, residual=False, dact=False, colsum=False):
    """bound 2e-6: test_row_resident_linear_with_fused_layernorm; the GELU' input-gradient form with column sums 3e-6:
    test_row_resident_input_gradient_with_gelu_grad_and_column_sums."""
    x, W, b = rnd(1, M, DIM), rnd(2, N, DIM, scale=DIM ** -0.5), rnd(3, N)
    g, be, res, aux = 1 + 0.1 * rnd(4, DIM), 0.1 * rnd(5, DIM), rnd(6, M, N), rnd(7, M, N)
    ops_ = [inp("x", x), inp("w", W), inp("bias", b), out("y", M, N)]
    if ln:
        ops_ += [inp("ln_gamma", g), inp("ln_beta", be), out("xn_out", M, DIM), flat("mean_out", M), flat("rstd_out", M)]
    if residual:
        ops_.append(inp("residual", res))
    if pre:
        ops_.append(out("y_pre", M, N))
    if dact:
        ops_.append(inp("dact_aux", aux))

    def late(lib):
        return [out("colsum_part", -(-M // lib.rp_linear_rows192_tile_rows()), N)] if colsum else []

    def call(lib, A_, st):
        a = lambda n: P(A_[n].addr()) if n in A_ else None
        lib.rp_linear_rows192(a("x"), a("w"), a("bias"), a("residual"), a("ln_gamma"), a("ln_beta"), 1e-6, a("y"), a("y_pre"),
                              a("xn_out"), a("mean_out"), a("rstd_out"), a("dact_aux"), a("colsum_part"), M, N, DIM, act, 0, 0, st)

    def check(v, errs):
        xd = x.double()
        if ln:
            xd = torch.nn.functional.layer_norm(xd, (DIM,), g.double(), be.double(), 1e-6)
        p = xd @ W.double().t() + b.double()
        y = _gelu64(p) if act else p
        if dact:
            a_ = aux.double().requires_grad_(True)
            _gelu64(a_).sum().backward()
            y = y * a_.grad
        if residual:
            y = y + res.double()
        bound = 3e-6 if dact else 2e-6
        e = {"y": _bound(errs, "y", rel(v["y"], y), bound)}
        if pre:
            e["y_pre"] = _bound(errs, "y_pre", rel(v["y_pre"], p), bound)
        if colsum:
            e["colsum"] = _bound(errs, "colsum_part", rel(v["colsum_part"].double().sum(0), v["y"].double().sum(0)), 3e-6)
        return e
    c = Case(ops_, call, check)
    c.late = late
    return c


for _m in (140, 9216 + 48):
    case("rp_linear_rows192", "M%d-ln-qkv576" % _m)(lambda m=_m: _rows_case(m, 576, ln=True))
    case("rp_linear_rows192", "M%d-proj192-residual" % _m)(lambda m=_m: _rows_case(m, 192, residual=True))
case("rp_linear_rows192", "M140-fc1-gelu-pre")(lambda: _rows_case(140, 768, ln=True, act=1, pre=True))
case("rp_linear_rows192", "M140-dx-dgelu-colsum")(lambda: _rows_case(140, 768, dact=True, colsum=True))


def _mlp_weights():
    return (1 + 0.1 * rnd(2, DIM), 0.1 * rnd(3, DIM), rnd(4, 4 * DIM, DIM, scale=DIM ** -0.5), 0.1 * rnd(5, 4 * DIM),
            rnd(6, DIM, 4 * DIM, scale=(4 * DIM) ** -0.5), 0.1 * rnd(7, DIM))


def _mlp_fwd_case(M, train):
    """bound 2e-6 of max|ref|: test_fused_mlp_inference_kernel (y and, training form, the saved tensors)."""
    x = rnd(1, M, DIM)
    g, be, w1, b1, w2, b2 = _mlp_weights()
    ops_ = [inp("x", x), inp("gamma", g), inp("beta", be), inp("w1", w1), inp("b1", b1), inp("w2", w2), inp("b2", b2), out("y", M, DIM)]
    if train:
        ops_ += [out("xn_out", M, DIM), flat("mean_out", M), flat("rstd_out", M), out("h_out", M, 4 * DIM), out("hpre_out", M, 4 * DIM)]

    def late(lib):
        return [work("workspace", lib.rp_mlp_fused_workspace_bytes(M))]

    def call(lib, A_, st):
        a = lambda n: P(A_[n].addr()) if n in A_ else None
        lib.rp_mlp_fused_fwd(a("x"), a("gamma"), a("beta"), a("w1"), a("b1"), a("w2"), a("b2"), a("y"), a("workspace"), M, DIM, 4 * DIM,
                             1e-6, a("xn_out"), a("mean_out"), a("rstd_out"), a("h_out"), a("hpre_out"), 0, 0, st)

    def check(v, errs):
        xn = torch.nn.functional.layer_norm(x.double(), (DIM,), g.double(), be.double(), 1e-6)
        hp = xn @ w1.double().t() + b1.double()
        h = _gelu64(hp)
        y = x.double() + h @ w2.double().t() + b2.double()
        e = {"y": _bound(errs, "y", rel(v["y"], y), 2e-6)}
        if train:
            for n, r in (("xn_out", xn), ("h_out", h), ("hpre_out", hp)):
                e[n] = _bound(errs, n, rel(v[n], r), 2e-6)
        return e
    c = Case(ops_, call, check)
    c.late = late
    return c


def _mlp_bwd_case(M, ln):
    """bound 3e-6 of max|ref|: test_fused_mlp_backward_data_kernel / test_fused_mlp_backward_with_layernorm_backward_folded_in."""
    dy, hpre = rnd(1, M, DIM), rnd(8, M, 4 * DIM)
    g, _, w1, _, w2, _ = _mlp_weights()
    x = rnd(9, M, DIM)
    mean = x.double().mean(1)
    rstd = (x.double().var(1, unbiased=False) + 1e-6).rsqrt()
    ops_ = [inp("dy", dy), inp("hpre", hpre), inp("w2t", w2.t().contiguous()), inp("w1t", w1.t().contiguous()), out("dhp", M, 4 * DIM),
            out("dx" if ln else "dxn", M, DIM)]
    if ln:
        ops_ += [inp("ln_x", x), inp("ln_gamma", g), inp("ln_mean", mean.float()), inp("ln_rstd", rstd.float())]

    def late(lib):
        e = [out("colpart", -(-M // lib.rp_mlp_fused_bwd_tile_rows()), 4 * DIM), work("workspace", lib.rp_mlp_fused_bwd_workspace_bytes(M))]
        if ln:
            e.append(out("ln_part", lib.rp_mlp_fused_bwd_ln_part_rows(M), 3 * DIM))
        return e

    def call(lib, A_, st):
        a = lambda n: P(A_[n].addr()) if n in A_ else None
        if ln:
            lib.rp_mlp_fused_bwd_ln(a("dy"), a("hpre"), a("w2t"), a("w1t"), a("dhp"), a("dx"), a("colpart"), a("workspace"), M, DIM, 4 * DIM,
                                    0, 0, a("ln_x"), a("ln_gamma"), a("ln_mean"), a("ln_rstd"), a("ln_part"), st)
        else:
            lib.rp_mlp_fused_bwd(a("dy"), a("hpre"), a("w2t"), a("w1t"), a("dhp"), a("dxn"), a("colpart"), a("workspace"), M, DIM, 4 * DIM,
                                 0, 0, st)

    def check(v, errs):
        hp = hpre.double().requires_grad_(True)
        _gelu64(hp).sum().backward()
        dhp = (dy.double() @ w2.double()) * hp.grad
        dxn = dhp @ w1.double()
        e = {"dhp": _bound(errs, "dhp", rel(v["dhp"], dhp), 3e-6),
             "colpart": _bound(errs, "colpart", rel(v["colpart"].double().sum(0), dhp.sum(0)), 3e-6)}
        if ln:
            xh = (x.double() - mean[:, None]) * rstd[:, None]
            gg = dxn * g.double()
            dx = rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True)) + dy.double()
            e["dx"] = _bound(errs, "dx", rel(v["dx"], dx), 3e-6)
            s = v["ln_part"].double().sum(0).cpu()
            e["ln_part"] = _bound(errs, "ln_part", max(rel(s[:DIM], (dxn * xh).sum(0)), rel(s[DIM:2 * DIM], dxn.sum(0)),
                                                       rel(s[2 * DIM:], dy.double().sum(0))), 3e-6)
        else:
            e["dxn"] = _bound(errs, "dxn", rel(v["dxn"], dxn), 3e-6)
        return e
    c = Case(ops_, call, check)
    c.late = late
    return c


for _m in (140, 9216 + 48):
    case("rp_mlp_fused_fwd", "M%d-inference" % _m)(lambda m=_m: _mlp_fwd_case(m, False))
    case("rp_mlp_fused_fwd", "M%d-training" % _m)(lambda m=_m: _mlp_fwd_case(m, True))
    case("rp_mlp_fused_bwd", "M%d" % _m)(lambda m=_m: _mlp_bwd_case(m, False))
    case("rp_mlp_fused_bwd_ln", "M%d" % _m)(lambda m=_m: _mlp_bwd_case(m, True))


# ================================================================================================ LayerNorm, column sums
@case("rp_layernorm_fwd", "rows1000-C192")
def _ln_fwd():
    rows, C = 1000, 192
    x, g, b = rnd(1, rows, C), 1 + 0.1 * rnd(2, C), 0.1 * rnd(3, C)
    ops_ = [inp("x", x), inp("gamma", g), inp("beta", b), out("y", rows, C), flat("mean", rows), flat("rstd", rows)]

    def call(lib, A_, st):
        lib.rp_layernorm_fwd(P(A_["x"].addr()), P(A_["gamma"].addr()), P(A_["beta"].addr()), P(A_["y"].addr()), P(A_["mean"].addr()),
                             P(A_["rstd"].addr()), rows, C, 1e-6, st)

    def check(v, errs):       # test_layernorm_fwd_bwd: 2e-6
        ref = torch.nn.functional.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-6)
        return {"y": _bound(errs, "y", rel(v["y"], ref), 2e-6), "mean": _bound(errs, "mean", rel(v["mean"].view(-1), x.double().mean(1)), 2e-6)}
    return Case(ops_, call, check)


def _ln_bwd_case(add):
    rows, C = 1000, 192
    dy, x, g, ad = rnd(1, rows, C), rnd(2, rows, C), 1 + 0.1 * rnd(3, C), rnd(4, rows, C)
    mean = x.double().mean(1)
    rstd = (x.double().var(1, unbiased=False) + 1e-6).rsqrt()
    np_ = 3 if add else 2
    ops_ = [inp("dy", dy), inp("x", x), inp("gamma", g), inp("mean", mean.float()), inp("rstd", rstd.float()), out("dx", rows, C)]
    if add:
        ops_.append(inp("add", ad))

    def late(lib):
        return [out("dgamma_part", lib.rp_layernorm_bwd_blocks(rows), np_ * C)]

    def call(lib, A_, st):
        a = lambda n: P(A_[n].addr()) if n in A_ else None
        lib.rp_layernorm_bwd(a("dy"), a("x"), a("gamma"), a("mean"), a("rstd"), a("add"), a("dx"), a("dgamma_part"), None, rows, C, st)

    def check(v, errs):       # test_layernorm_fwd_bwd: 5e-6 for the backward
        xh = (x.double() - mean[:, None]) * rstd[:, None]
        gg = dy.double() * g.double()
        dx = rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True)) + (ad.double() if add else 0)
        s = v["dgamma_part"].double().sum(0).cpu()
        return {"dx": _bound(errs, "dx", rel(v["dx"], dx), 5e-6),
                "dgamma": _bound(errs, "dgamma", rel(s[:C], (dy.double() * xh).sum(0)), 5e-6),
                "dbeta": _bound(errs, "dbeta", rel(s[C:2 * C], dy.double().sum(0)), 5e-6)}
    c = Case(ops_, call, check)
    c.late = late
    return c


case("rp_layernorm_bwd", "rows1000")(lambda: _ln_bwd_case(False))
case("rp_layernorm_bwd", "rows1000-add")(lambda: _ln_bwd_case(True))


def _colsum_case(rows, cols, ld):
    t = rnd(1, rows, cols)
    ops_ = [inp("in", t, ld=ld), flat("out", cols)]
    state = {}

    def late(lib):
        state["ws"] = lib.rp_colsum_workspace_bytes(rows, cols)
        return [work("workspace", state["ws"])]

    def call(lib, A_, st, wsb=None):
        lib.rp_colsum(P(A_["in"].addr()), rows, cols, ld, P(A_["out"].addr()), P(A_["workspace"].addr()),
                      state["ws"] if wsb is None else wsb, st)

    def check(v, errs):       # test_colsum: 2e-6
        return {"out": _bound(errs, "out", rel(v["out"].view(-1), t.double().sum(0)), 2e-6)}
    c = Case(ops_, call, check, lambda lib, A_, st: call(lib, A_, st, state["ws"] - 4))
    c.late = late
    c.has_workspace = lambda: state["ws"] > 0          # (few rows: one stage, no workspace, nothing to refuse)
    return c


case("rp_colsum", "1000x576")(lambda: _colsum_case(1000, 576, 576))
case("rp_colsum", "1000x100-ld164")(lambda: _colsum_case(1000, 100, 164))
case("rp_colsum", "37x768-ld772")(lambda: _colsum_case(37, 768, 772))


@case("rp_colsum_multi", "3-tasks")
def _colsum_multi():
    shapes = [(1000, 576, 576), (37, 768, 772), (2304, 192, 192)]
    ts = [rnd(20 + i, r, c) for i, (r, c, _) in enumerate(shapes)]
    ops_ = [inp("in%d" % i, t, ld=shapes[i][2]) for i, t in enumerate(ts)] + [flat("out%d" % i, c) for i, (_, c, _) in enumerate(shapes)]
    state = {}

    def tasks(A_):
        from rel_pose_amd import _lib
        arr = (_lib.RpColsumTask * len(shapes))()
        for i, (r, c, ld) in enumerate(shapes):
            arr[i].in_, arr[i].rows, arr[i].cols, arr[i].ld = (A_["in%d" % i].addr() if A_ else 0), r, c, ld
            arr[i].out = A_["out%d" % i].addr() if A_ else 0
        return arr

    def late(lib):
        state["ws"] = lib.rp_colsum_multi_workspace_bytes(tasks(None), len(shapes))
        return [work("workspace", state["ws"])]

    def call(lib, A_, st, wsb=None):
        lib.rp_colsum_multi(tasks(A_), len(shapes), P(A_["workspace"].addr()), state["ws"] if wsb is None else wsb, st)

    def check(v, errs):
        return {"out%d" % i: _bound(errs, "out%d" % i, rel(v["out%d" % i].view(-1), t.double().sum(0)), 2e-6) for i, t in enumerate(ts)}
    c = Case(ops_, call, check, lambda lib, A_, st: call(lib, A_, st, state["ws"] - 4))
    c.late = late
    return c


# ================================================================================================ attention family
# Layouts: "packed" = the [Z*576, 576] q | k | v buffer every test of tests/test_gpu_kernels.py uses (ldq = ldk = ldv = 576, ldo = 192,
# gradients into one dqkv); "split" = q, k, v in separate buffers of row strides 192 / 256 / 320, o with ldo = 256, dq / dk / dv in
# buffers of strides 200 / 256 / 320, column-sum partials with ldp = 640.  The split case names its packed sibling: same values, same
# tiles, same order -- the results must be the same bits.  Z = 2, 6: one-wave workgroups (Z*H*9 <= 512); Z = 20: the two-wave form
# every full-size batch runs (the launchers read their RP_ATTN_* overrides once per process, so the size is what selects the form here).
LOG2E = 1.4426950408889634


@functools.lru_cache(maxsize=4)
def _qkv(Z):
    qkv = rnd(1, Z * N_TOK, 3 * DIM)
    qkv[:, :2 * DIM] *= 1.7
    qkv[5, :64] *= 6.0
    return qkv


def _heads(t, Z):
    return t.double().view(Z, N_TOK, HEADS, 64).permute(0, 2, 1, 3)


def _swap(t, x):
    return t.view(t.shape[0] // 2, 2, *t.shape[1:]).flip(1).reshape(t.shape) if x else t


def _attn_ref(qkv, Z, q_xor=0, k_xor=0, grad=None):
    """fp64 attention on the CPU: (o [Z*576,192], lse [Z,H,576], p) and, with grad = dO, the gradient of qkv"""
    x = qkv.double().requires_grad_(grad is not None)
    q, k, v = (_heads(x[:, i * DIM:(i + 1) * DIM], Z) for i in range(3))
    q, k, v = _swap(q, q_xor), _swap(k, k_xor & 1), _swap(v, k_xor >> 1)
    s = q @ k.transpose(-1, -2) * SCALE
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = (p @ v).permute(0, 2, 1, 3).reshape(Z * N_TOK, DIM)
    if grad is None:
        return o, lse, p
    (o * grad.double()).sum().backward()
    return o.detach(), lse.detach(), x.grad


def _qkv_in(layout, qkv, Z, need="qkv"):
    """input operands for q / k / v and the function (name -> (address, ld)) over the allocated operands"""
    rows = Z * N_TOK
    if layout == "packed":
        ops_ = [inp_multi("qkv", rows, 3 * DIM, {i * DIM: qkv[:, i * DIM:(i + 1) * DIM] for i, n in enumerate("qkv") if n in need})]
        return ops_, lambda A_, n: (P(A_["qkv"].addr("qkv".index(n) * DIM)), 3 * DIM)
    lds = {"q": 192, "k": 256, "v": 320}
    ops_ = [inp(n, qkv[:, i * DIM:(i + 1) * DIM], ld=lds[n]) for i, n in enumerate("qkv") if n in need]
    return ops_, lambda A_, n: (P(A_[n].addr()), lds[n])


def _dqkv_out(layout, Z, need, parts=False):
    rows = Z * N_TOK
    if layout == "packed":
        ops_ = [out("dqkv", rows, 3 * DIM, wins={"d" + n: ("qkv".index(n) * DIM, "qkv".index(n) * DIM + DIM) for n in need})]
        if parts:
            ops_.append(out("part", Z * 18, 3 * DIM, wins={"p" + n: ("qkv".index(n) * DIM, "qkv".index(n) * DIM + DIM) for n in need}))
        return ops_, (lambda A_, n: (P(A_["dqkv"].addr("qkv".index(n) * DIM)), 3 * DIM)), (
            lambda A_, n: P(A_["part"].addr("qkv".index(n) * DIM)) if parts else None), 3 * DIM
    lds = {"q": 200, "k": 256, "v": 320}
    ops_ = [out("d" + n, rows, DIM, ld=lds[n]) for n in need]
    if parts:
        ops_.append(out("part", Z * 18, 640, wins={"p" + n: ("qkv".index(n) * 200, "qkv".index(n) * 200 + DIM) for n in need}))
    return ops_, (lambda A_, n: (P(A_["d" + n].addr()), lds[n])), (
        lambda A_, n: P(A_["part"].addr("qkv".index(n) * 200)) if parts else None), 640


def _sib(fn, *a, **k):
    return lambda: fn("packed", *a, **k)


def _attn_fwd_case(layout, Z, q_xor=0, k_xor=0, stats_only=False, savep=False):
    """bounds: test_attention_fwd_bwd (o 5e-6, lse 2e-6); stored tiles: test_attention_stored_p_fwd_bwd (5e-6 on the probabilities)"""
    qkv = _qkv(Z)
    ins, ptr = _qkv_in(layout, qkv, Z, "qk" if stats_only else "qkv")
    ldo = DIM if layout == "packed" else 256
    ops_ = ins + [flat("lse", Z * HEADS * N_TOK)]
    if not stats_only:
        ops_.append(out("o", Z * N_TOK, DIM, ld=ldo))
    if savep:
        ops_ += [flat("pst", Z * HEADS * 18 * 18 * 1024), flat("mrun", Z * HEADS * 18 * N_TOK)]

    def call(lib, A_, st):
        (q, ldq), (k, ldk) = ptr(A_, "q"), ptr(A_, "k")
        v, ldv = (None, 4) if stats_only else ptr(A_, "v")
        o = None if stats_only else P(A_["o"].addr())
        if savep:
            lib.rp_attn_fwd_savep(q, k, v, o, P(A_["lse"].addr()), P(A_["pst"].addr()), P(A_["mrun"].addr()), Z, HEADS, ldq, ldk, ldv, ldo,
                                  SCALE, st)
        else:
            lib.rp_attn_fwd(q, k, v, o, P(A_["lse"].addr()), Z, HEADS, ldq, ldk, ldv, ldo, q_xor, k_xor, SCALE, int(stats_only), 0, st)

    def check(v, errs):
        o, lse, _ = _attn_ref(qkv, Z, q_xor, k_xor)
        e = {"lse": _bound(errs, "lse", rel(v["lse"].view(Z, HEADS, N_TOK), lse), 2e-6)}
        if not stats_only:
            e["o"] = _bound(errs, "o", rel(v["o"], o), 5e-6)
        if savep:      # the quantity test_attention_stored_p_fwd_bwd bounds: P = pst * exp2(mrun - lse / ln 2) against softmax(S), 5e-6
            _, _, pn = _attn_ref(qkv, Z)
            fac = torch.exp2(v["mrun"].double().view(Z, HEADS, 18, N_TOK) - v["lse"].double().view(Z, HEADS, 1, N_TOK) / math.log(2.0))
            pst = v["pst"].double().view(Z, HEADS, 18, 18, 8, 32, 4).permute(0, 1, 2, 5, 3, 4, 6).reshape(Z, HEADS, N_TOK, N_TOK)
            e["p"] = _bound(errs, "pst * exp2(mrun - lse2)", rel(pst * fac.permute(0, 1, 3, 2).repeat_interleave(32, dim=3), pn), 5e-6)
        return e
    return Case(ops_, call, check, sibling=None if layout == "packed" else _sib(_attn_fwd_case, Z, q_xor, k_xor, stats_only, savep))


def _tile_runs(t):
    """[..., 576 (a), 576 (b)] -> store_tile_runs' layout [..., 18, 18, 1024]: element (a, b) of a tile at ((b >> 2) * 32 + a) * 4 + (b & 3)"""
    lead = t.shape[:-2]
    x = t.reshape(*lead, 18, 32, 18, 8, 4)                       # ..., at, a, bt, b >> 2, b & 3
    n = len(lead)
    return x.permute(*range(n), n, n + 2, n + 3, n + 1, n + 4).reshape(*lead, 18, 18, 1024)


@functools.lru_cache(maxsize=2)
def _savep_ref(Z):
    qkv = _qkv(Z)
    q, k = _heads(qkv[:, :DIM], Z), _heads(qkv[:, DIM:2 * DIM], Z)
    s2 = q @ k.transpose(-1, -2) * (SCALE * LOG2E)                                     # [Z,H,i,j] in log2 units
    mt = torch.cummax(s2.view(Z, HEADS, N_TOK, 18, 32).amax(-1), -1)[0]               # [Z,H,i,t]
    pst = torch.exp2(s2.view(Z, HEADS, N_TOK, 18, 32) - mt[..., None]).view(Z, HEADS, N_TOK, N_TOK)
    return _tile_runs(pst), mt.permute(0, 1, 3, 2).contiguous()


def _ds_tiles(ds):
    """[Z,H,576 (a),576 (b)] -> the MFMA accumulator image rp_attn_bwd_dkdv_ds / rp_emm_grad_ds store: [.., a >> 5, b >> 5, r, lane],
    a & 31 = (r & 3) + 8 (r >> 2) + 4 (lane >> 5), b & 31 = lane & 31"""
    Z, H = ds.shape[:2]
    x = ds.reshape(Z, H, 18, 4, 2, 4, 18, 32)                    # at, r >> 2, lane >> 5, r & 3, bt, lane & 31
    return x.permute(0, 1, 2, 6, 3, 5, 4, 7).reshape(Z, H, 18, 18, 1024)


@functools.lru_cache(maxsize=8)
def _attn_bwd_data(Z, kv_xor):
    do = rnd(2, Z * N_TOK, DIM)
    o, lse, gref = _attn_ref(_qkv(Z), Z, 0, 3 * kv_xor, grad=do)
    return o, lse, gref, (do.double() * o).view(Z, N_TOK, HEADS, 64).sum(-1).permute(0, 2, 1)


def _attn_bwd_case(layout, Z, entry, kv_xor=0, parts=False):
    """every backward form of the fused attention against fp64 autograd at test_attention_fwd_bwd's 2e-5 (column-sum partials
    against the stored gradients: 2e-6)"""
    qkv, do = _qkv(Z), rnd(2, Z * N_TOK, DIM)
    o, lse, gref, delta = _attn_bwd_data(Z, kv_xor)
    need = {"rp_attn_bwd": "qkv", "rp_attn_bwd_cross": "qkv", "rp_attn_bwd_dkdv": "kv", "rp_attn_bwd_dkdv_ds": "kv", "rp_attn_bwd_dq": "q",
            "rp_attn_bwd_dkdv_p": "kv"}[entry]
    ins, ptr = _qkv_in(layout, qkv, Z, "qv" if entry == "rp_attn_bwd_dkdv_p" else "qkv")
    outs, dptr, pptr, ldp = _dqkv_out(layout, Z, need, parts)
    lddo = DIM if layout == "packed" else 224
    ops_ = ins + outs + [inp("dout", do, ld=lddo), inp("lse", lse.reshape(1, -1).float()), inp("delta", delta.reshape(1, -1).float())]
    if entry in ("rp_attn_bwd_dkdv_ds", "rp_attn_bwd_dkdv_p"):
        ops_.append(flat("ds", Z * HEADS * N_TOK * N_TOK))
    if entry == "rp_attn_bwd_dkdv_p":
        pst, mrun = _savep_ref(Z)
        ops_ += [inp("pst", pst.reshape(1, -1).float()), inp("mrun", mrun.reshape(1, -1).float())]

    def call(lib, A_, st):
        a = lambda n: P(A_[n].addr())
        (q, ldq), (v, ldv) = ptr(A_, "q"), ptr(A_, "v")
        k, ldk = ptr(A_, "k") if entry != "rp_attn_bwd_dkdv_p" else (None, 4)
        d = {n: dptr(A_, n) for n in need}
        if entry == "rp_attn_bwd":
            lib.rp_attn_bwd(q, k, v, a("dout"), a("lse"), a("delta"), d["q"][0], d["k"][0], d["v"][0], Z, HEADS, ldq, ldk, ldv, lddo,
                            d["q"][1], d["k"][1], d["v"][1], SCALE, 0, st)
        elif entry == "rp_attn_bwd_cross":
            lib.rp_attn_bwd_cross(q, k, v, a("dout"), a("lse"), a("delta"), d["q"][0], d["k"][0], d["v"][0], Z, HEADS, ldq, ldk, ldv, lddo,
                                  d["q"][1], d["k"][1], d["v"][1], SCALE, kv_xor, 0, st)
        elif entry == "rp_attn_bwd_dkdv":
            lib.rp_attn_bwd_dkdv(q, k, v, a("dout"), a("lse"), a("delta"), d["k"][0], d["v"][0], Z, HEADS, ldq, ldk, ldv, lddo,
                                 d["k"][1], d["v"][1], SCALE, 0, st)
        elif entry == "rp_attn_bwd_dkdv_ds":
            lib.rp_attn_bwd_dkdv_ds(q, k, v, a("dout"), a("lse"), a("delta"), d["k"][0], d["v"][0], a("ds"), Z, HEADS, ldq, ldk, ldv, lddo,
                                    d["k"][1], d["v"][1], SCALE, 0, pptr(A_, "k"), pptr(A_, "v"), ldp, st)
        elif entry == "rp_attn_bwd_dq":
            lib.rp_attn_bwd_dq(q, k, v, a("dout"), a("lse"), a("delta"), d["q"][0], Z, HEADS, ldq, ldk, ldv, lddo, d["q"][1], SCALE, 0, st)
        else:
            lib.rp_attn_bwd_dkdv_p(q, v, a("dout"), a("lse"), a("delta"), a("pst"), a("mrun"), d["k"][0], d["v"][0], a("ds"), Z, HEADS,
                                   ldq, ldv, lddo, d["k"][1], d["v"][1], SCALE, pptr(A_, "k"), pptr(A_, "v"), ldp, st)

    def check(v, errs):
        e = {}
        for n in need:
            i = "qkv".index(n)
            e["d" + n] = _bound(errs, "d" + n, rel(v["d" + n], gref[:, i * DIM:(i + 1) * DIM]), 2e-5)
            if parts:
                e["p" + n] = _bound(errs, "p" + n, rel(v["p" + n], v["d" + n].double().view(Z * 18, 32, DIM).sum(1)), 2e-6)
        return e
    return Case(ops_, call, check, sibling=None if layout == "packed" else _sib(_attn_bwd_case, Z, entry, kv_xor, parts))


def _delta_case(Z, ld):
    do, o = rnd(2, Z * N_TOK, DIM), rnd(3, Z * N_TOK, DIM)
    ops_ = [inp("dout", do, ld=ld), inp("o", o, ld=ld), flat("delta", Z * HEADS * N_TOK)]

    def call(lib, A_, st):
        lib.rp_attn_bwd_delta(P(A_["dout"].addr()), P(A_["o"].addr()), P(A_["delta"].addr()), Z, HEADS, ld, st)

    def check(v, errs):      # part of test_attention_fwd_bwd's backward (2e-5)
        ref = (do.double() * o.double()).view(Z, N_TOK, HEADS, 64).sum(-1).permute(0, 2, 1)
        return {"delta": _bound(errs, "delta", rel(v["delta"].view(Z, HEADS, N_TOK), ref), 2e-5)}
    return Case(ops_, call, check, sibling=None if ld == DIM else (lambda: _delta_case(Z, DIM)))


def _ds_matmul_case(layout, Z, b_xor, tiled_t, colpart):
    """out = dS b per (image, head) from the tiled dS array (rp_ds_matmul: accumulator-image tiles; rp_ds_matmul_t: 16-byte-run tiles);
    bound: it is the dQ half of test_attention_fwd_bwd's stored-dS backward (2e-5)"""
    ds, b = rnd(4, Z, HEADS, N_TOK, N_TOK, scale=0.05), rnd(5, Z * N_TOK, DIM)
    if tiled_t:       # rp_attn_bwd_dkdv_p's tiles: element (query i, key j) at ((i >> 2) * 32 + j) * 4 + (i & 3) = _tile_runs of dS^T
        tiles = _tile_runs(ds.transpose(-1, -2)).reshape(Z, HEADS, 18, 18, 1024).transpose(2, 3)
    else:
        tiles = _ds_tiles(ds)
    ldb, ldo, ldp = (3 * DIM, 3 * DIM, 3 * DIM) if layout == "packed" else (256, 320, 640)
    ops_ = [inp("ds", tiles.reshape(1, -1)), inp("b", b, ld=ldb), out("out", Z * N_TOK, DIM, ld=ldo)]
    if colpart:
        ops_.append(out("colpart", Z * 18, DIM, ld=ldp))

    def call(lib, A_, st):
        cp = P(A_["colpart"].addr()) if colpart else None
        if tiled_t:
            lib.rp_ds_matmul_t(P(A_["ds"].addr()), P(A_["b"].addr()), P(A_["out"].addr()), Z, HEADS, ldb, ldo, b_xor, cp, ldp, st)
        else:
            lib.rp_ds_matmul(P(A_["ds"].addr()), P(A_["b"].addr()), P(A_["out"].addr()), Z, HEADS, ldb, ldo, b_xor, 0, cp, ldp, st)

    def check(v, errs):
        ref = (ds.double() @ _swap(_heads(b, Z), b_xor)).permute(0, 2, 1, 3).reshape(Z * N_TOK, DIM)
        e = {"out": _bound(errs, "out", rel(v["out"], ref), 2e-5)}
        if colpart:
            e["colpart"] = _bound(errs, "colpart", rel(v["colpart"], v["out"].double().view(Z * 18, 32, DIM).sum(1)), 2e-6)
        return e
    return Case(ops_, call, check, sibling=None if layout == "packed" else _sib(_ds_matmul_case, Z, b_xor, tiled_t, colpart))


for _lay in ("packed", "split"):
    for _z in (2, 6):
        case("rp_attn_fwd", "%s-Z%d" % (_lay, _z))(lambda l=_lay, z=_z: _attn_fwd_case(l, z))
        case("rp_attn_fwd_savep", "%s-Z%d" % (_lay, _z))(lambda l=_lay, z=_z: _attn_fwd_case(l, z, savep=True))
        case("rp_attn_bwd", "%s-Z%d" % (_lay, _z))(lambda l=_lay, z=_z: _attn_bwd_case(l, z, "rp_attn_bwd"))
        case("rp_attn_bwd_dkdv_ds", "%s-Z%d-colparts" % (_lay, _z))(lambda l=_lay, z=_z: _attn_bwd_case(l, z, "rp_attn_bwd_dkdv_ds", parts=True))
        case("rp_attn_bwd_dkdv_p", "%s-Z%d-colparts" % (_lay, _z))(lambda l=_lay, z=_z: _attn_bwd_case(l, z, "rp_attn_bwd_dkdv_p", parts=True))
        case("rp_ds_matmul_t", "%s-Z%d-colpart" % (_lay, _z))(lambda l=_lay, z=_z: _ds_matmul_case(l, z, 0, True, True))
        for _x in (0, 1):
            case("rp_ds_matmul", "%s-Z%d-b_xor%d" % (_lay, _z, _x))(lambda l=_lay, z=_z, x=_x: _ds_matmul_case(l, z, x, False, x == 0))
    case("rp_attn_fwd", "%s-Z6-stats_only-q_xor" % _lay)(lambda l=_lay: _attn_fwd_case(l, 6, q_xor=1, stats_only=True))
    case("rp_attn_fwd", "%s-Z2-stats_only-k_xor1" % _lay)(lambda l=_lay: _attn_fwd_case(l, 2, k_xor=1, stats_only=True))
    case("rp_attn_fwd", "%s-Z6-k_xor3" % _lay)(lambda l=_lay: _attn_fwd_case(l, 6, k_xor=3))
    case("rp_attn_bwd_cross", "%s-Z6-kv_xor" % _lay)(lambda l=_lay: _attn_bwd_case(l, 6, "rp_attn_bwd_cross", kv_xor=1))
    case("rp_attn_bwd_cross", "%s-Z2-kv_xor" % _lay)(lambda l=_lay: _attn_bwd_case(l, 2, "rp_attn_bwd_cross", kv_xor=1))
    case("rp_attn_bwd_dkdv", "%s-Z6" % _lay)(lambda l=_lay: _attn_bwd_case(l, 6, "rp_attn_bwd_dkdv"))
    case("rp_attn_bwd_dkdv", "%s-Z2" % _lay)(lambda l=_lay: _attn_bwd_case(l, 2, "rp_attn_bwd_dkdv"))
    case("rp_attn_bwd_dq", "%s-Z6" % _lay)(lambda l=_lay: _attn_bwd_case(l, 6, "rp_attn_bwd_dq"))
    case("rp_attn_bwd_dq", "%s-Z2" % _lay)(lambda l=_lay: _attn_bwd_case(l, 2, "rp_attn_bwd_dq"))
    case("rp_ds_matmul_t", "%s-Z2-b_xor1" % _lay)(lambda l=_lay: _ds_matmul_case(l, 2, 1, True, False))
case("rp_attn_bwd_delta", "Z2-ld192")(lambda: _delta_case(2, DIM))
case("rp_attn_bwd_delta", "Z6-ld256")(lambda: _delta_case(6, 256))
# the two-wave workgroups (Z*H*9 > 512) in the strided layout
case("rp_attn_fwd", "split-Z20-two-wave")(lambda: _attn_fwd_case("split", 20))
case("rp_attn_fwd_savep", "split-Z20-two-wave")(lambda: _attn_fwd_case("split", 20, savep=True))
case("rp_attn_bwd", "split-Z20-two-wave")(lambda: _attn_bwd_case("split", 20, "rp_attn_bwd"))
case("rp_attn_bwd_dkdv_p", "split-Z20-two-wave-colparts")(lambda: _attn_bwd_case("split", 20, "rp_attn_bwd_dkdv_p", parts=True))
case("rp_attn_bwd_dkdv_ds", "split-Z20-two-wave-colparts")(lambda: _attn_bwd_case("split", 20, "rp_attn_bwd_dkdv_ds", parts=True))
case("rp_attn_bwd_cross", "split-Z20-two-wave-kv_xor")(lambda: _attn_bwd_case("split", 20, "rp_attn_bwd_cross", kv_xor=1))
case("rp_attn_bwd_dkdv", "split-Z20-two-wave")(lambda: _attn_bwd_case("split", 20, "rp_attn_bwd_dkdv"))
case("rp_attn_bwd_dq", "split-Z20-two-wave")(lambda: _attn_bwd_case("split", 20, "rp_attn_bwd_dq"))
case("rp_attn_fwd", "split-Z20-two-wave-k_xor3")(lambda: _attn_fwd_case("split", 20, k_xor=3))


# ================================================================================================ Essential Matrix Module
# ldqkv = 576 (packed, as everywhere in tests/test_gpu_kernels.py) and 640: the 64 columns behind q | k | v hold the sentinel on the way
# in and must come back untouched in dqkv.  References: tests/test_gpu_kernels.py's _emm_ref, restated for the CPU.
@functools.lru_cache(maxsize=4)
def _emm_data(Z):
    qkv = rnd(4, Z * N_TOK, 3 * DIM)
    pos = rnd(5, Z // 2, N_TOK, 6, scale=0.5)
    t = qkv.double().view(Z, N_TOK, 3, HEADS, 64).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    perm = [z ^ 1 for z in range(Z)]
    d = {"qkv": qkv, "pos": pos}
    qk = torch.stack([q[perm], k]).clone().requires_grad_(True)
    s = (qk[0] @ qk[1].transpose(-1, -2)) * SCALE
    d["S2"] = (s * LOG2E).detach()
    d["rlse"], d["clse"] = torch.logsumexp(s, -1).detach(), torch.logsumexp(s, -2).detach()
    a = s.softmax(-1) * s.softmax(-2)
    x = torch.cat([v, pos.double()[[z // 2 for z in range(Z)]].unsqueeze(1).expand(Z, HEADS, N_TOK, 6)], -1)
    x96 = torch.zeros(Z, HEADS, N_TOK, XW, dtype=torch.float64)
    x96[..., :70] = x
    d["x"] = x96
    d["T"], d["U"] = (a @ x96).detach(), (a.transpose(-1, -2) @ x96).detach()
    F = x96.transpose(-1, -2) @ (a @ x96)
    d["F"] = F.detach()
    dF = torch.zeros(Z, HEADS, XW, XW, dtype=torch.float64)
    dF[..., :70, :70] = rnd(6, Z, HEADS, 70, 70).double()
    d["dF"] = dF
    (F * dF).sum().backward()
    d["dq"] = qk.grad[0][perm].permute(0, 2, 1, 3).reshape(Z * N_TOK, DIM)       # gradient of the q columns (rows of image z ^ 1)
    d["dk"] = qk.grad[1].permute(0, 2, 1, 3).reshape(Z * N_TOK, DIM)
    d["w"], d["wp"] = x96 @ dF, x96 @ dF.transpose(-1, -2)
    d["rho"], d["gamma"] = (d["w"] * d["T"]).sum(-1), (d["wp"] * d["U"]).sum(-1)
    # scale * dS (query i of the partner image, key j), what rp_emm_grad_ds stores key-major
    A = a.detach()
    dA = d["w"] @ x96.transpose(-1, -2)
    R, C = s.softmax(-1).detach(), s.softmax(-2).detach()
    d["dS"] = SCALE * (2 * A * dA - R * d["rho"][..., None] - C * d["gamma"][..., None, :])
    return d


def _f32(t):
    return t.float() if t.dtype == torch.float64 else t


def _emm_stats_case(Z, ld, s_out):
    d = _emm_data(Z)
    ops_ = [inp_multi("qkv", Z * N_TOK, ld, {0: d["qkv"][:, :2 * DIM]}), flat("rlse", Z * HEADS * N_TOK), flat("clse", Z * HEADS * N_TOK)]
    if s_out:
        ops_.append(flat("s_out", Z * HEADS * 18 * 18 * 1024))

    def late(lib):
        return [work("workspace", lib.rp_emm_stats_workspace_bytes(Z, HEADS))]

    def call(lib, A_, st):
        lib.rp_emm_stats(P(A_["qkv"].addr()), P(A_["qkv"].addr(DIM)), P(A_["rlse"].addr()), P(A_["clse"].addr()), P(A_["workspace"].addr()),
                         P(A_["s_out"].addr()) if s_out else None, Z, HEADS, ld, ld, SCALE, 0, st)

    def check(v, errs):      # test_attention_stats_partner / test_emm_stored_scores: 2e-6
        e = {"rlse": _bound(errs, "rlse", rel(v["rlse"].view(Z, HEADS, N_TOK), d["rlse"]), 2e-6),
             "clse": _bound(errs, "clse", rel(v["clse"].view(Z, HEADS, N_TOK), d["clse"]), 2e-6)}
        if s_out:
            e["s_out"] = _bound(errs, "s_out", rel(v["s_out"].view(-1), _tile_runs(d["S2"]).reshape(-1)), 2e-6)
        return e
    c = Case(ops_, call, check, sibling=None if ld == 3 * DIM else (lambda: _emm_stats_case(Z, 3 * DIM, s_out)))
    c.late = late
    return c


def _emm_build_x_case(Z, ld, bwd):
    d = _emm_data(Z)
    if bwd:
        dx = rnd(7, Z, HEADS, N_TOK, XW)
        ops_ = [inp("dx", dx.view(-1, XW)), out("dqkv", Z * N_TOK, 3 * DIM, ld=ld, wins={"dv": (2 * DIM, 3 * DIM)})]
    else:
        ops_ = [inp_multi("qkv", Z * N_TOK, ld, {2 * DIM: d["qkv"][:, 2 * DIM:]}), inp("pos", d["pos"].view(-1, 6)), out("x", Z * HEADS * N_TOK, XW)]

    def call(lib, A_, st):
        if bwd:
            lib.rp_emm_build_x_bwd(P(A_["dx"].addr()), P(A_["dqkv"].addr()), Z, HEADS, ld, st)
        else:
            lib.rp_emm_build_x(P(A_["qkv"].addr()), P(A_["pos"].addr()), P(A_["x"].addr()), Z, HEADS, ld, st)

    def check(v, errs):
        if bwd:
            if not torch.equal(v["dv"].cpu(), dx[..., :64].permute(0, 2, 1, 3).reshape(Z * N_TOK, DIM)):
                errs.append("dv columns are not dx[..., :64]")
        else:
            x = v["x"].view(Z, HEADS, N_TOK, XW).cpu()
            if not torch.equal(x[..., :70], d["x"][..., :70].float()):
                errs.append("x[..., :70] is not [v | pos]")
            if float(x[..., 70:].abs().max()) != 0.0 or bool(torch.isnan(x[..., 70:]).any()):
                errs.append("x columns 70..95 are not zero")
        return {}
    return Case(ops_, call, check, sibling=None if ld == 3 * DIM else (lambda: _emm_build_x_case(Z, 3 * DIM, bwd)))


def _emm_apply_case(Z, ld, swap=False, single=False, x_left=False, s_in=False, want_t=True):
    """T = A X (swap: U = A^T X) and the six per-workgroup partials of F; bound 1e-5 over the 70 live columns, rows / columns
    70..95 of F exactly zero (test_emm_forward_pieces)"""
    d = _emm_data(Z)
    ops_ = [inp_multi("qkv", Z * N_TOK, ld, {0: d["qkv"][:, :2 * DIM]}), inp("x", _f32(d["x"]).view(-1, XW)),
            inp("rlse", _f32(d["rlse"]).reshape(1, -1)), inp("clse", _f32(d["clse"]).reshape(1, -1))]
    if x_left:
        ops_.append(inp("x_left", _f32(d["x"]).flip(0).reshape(-1, XW)))
    if s_in:
        ops_.append(inp("s_in", _f32(_tile_runs(d["S2"])).reshape(1, -1)))
    if want_t:
        ops_.append(out("t_out", Z * HEADS * N_TOK, XW))
    if not swap:
        ops_.append(out("f_part", Z * HEADS * NWG * XW, XW))

    def call(lib, A_, st):
        a = lambda n: P(A_[n].addr()) if n in A_ else None
        lib.rp_emm_apply(a("qkv"), ld, a("x"), a("x_left"), a("rlse"), a("clse"), a("s_in"), a("t_out"), a("f_part"), Z, HEADS, SCALE,
                         int(swap), int(single), 0, st)

    def check(v, errs):
        e, ref = {}, not (single or x_left)          # (the ablation forms have no fp64 reference here; the documented zeros hold for all)
        if want_t:
            t = v["t_out"].view(Z, HEADS, N_TOK, XW)
            if not bool((t[..., 70:] == 0).all()):
                errs.append("T columns 70..95 are not exactly zero")
            if ref:
                e["T"] = _bound(errs, "t_out", rel(t[..., :70], (d["U"] if swap else d["T"])[..., :70]), 1e-5)
        if not swap:
            fp = v["f_part"].view(Z, HEADS, NWG, XW, XW)
            if not (bool((fp[..., 70:, :] == 0).all()) and bool((fp[..., :, 70:] == 0).all())):
                errs.append("F rows / columns 70..95 are not exactly zero in every partial")
            if ref:
                e["F"] = _bound(errs, "f_part", rel(fp.double().sum(2)[..., :70, :70], d["F"][..., :70, :70]), 1e-5)
        return e
    return Case(ops_, call, check,
                sibling=None if ld == 3 * DIM else (lambda: _emm_apply_case(Z, 3 * DIM, swap, single, x_left, s_in, want_t)))


def _emm_finalize_case(Z, nparts, entry):
    d = _emm_data(Z)
    if entry == "rp_emm_finalize_bwd":
        dg = torch.zeros(Z * 70, GW)
        dg[:, :210] = rnd(8, Z * 70, 210)
        ops_ = [inp("dg", dg), out("df", Z * HEADS * XW, XW)]
    else:
        fp = torch.zeros(Z, HEADS, nparts, XW, XW)
        fp[..., :70, :70] = rnd(9, Z, HEADS, nparts, 70, 70)
        ops_ = [inp("f_part", fp.view(-1, XW)), out("g", Z * 70, GW)]

    def call(lib, A_, st):
        if entry == "rp_emm_finalize":
            lib.rp_emm_finalize(P(A_["f_part"].addr()), P(A_["g"].addr()), Z, HEADS, GW, st)
        elif entry == "rp_emm_finalize_parts":
            lib.rp_emm_finalize_parts(P(A_["f_part"].addr()), P(A_["g"].addr()), Z, HEADS, GW, nparts, st)
        else:
            lib.rp_emm_finalize_bwd(P(A_["dg"].addr()), P(A_["df"].addr()), Z, HEADS, GW, st)

    def check(v, errs):
        perm = [z ^ 1 for z in range(Z)]
        if entry == "rp_emm_finalize_bwd":       # the transpose of rp_emm_finalize: df[z][h][a][c] = dg[z ^ 1][c][h * 70 + a], zero elsewhere
            ref = torch.zeros(Z, HEADS, XW, XW)
            ref[..., :70, :70] = dg.view(Z, 70, GW)[perm][..., :210].reshape(Z, 70, HEADS, 70).permute(0, 2, 3, 1)
            if not torch.equal(v["df"].view(Z, HEADS, XW, XW).cpu(), ref):
                errs.append("df is not the zero-padded transpose of dg")
            return {}
        F = fp.double().sum(2)[..., :70, :70]                                         # [Z,H,a,c]
        ref = F[perm].reshape(Z, 210, 70).transpose(-1, -2)                            # test_emm_forward_pieces: g[z^1][c][h*70+a], 1e-5
        g = v["g"].view(Z, 70, GW).cpu()
        if float(g[..., 210:].abs().max()) != 0.0 or bool(torch.isnan(g[..., 210:]).any()):
            errs.append("g columns 210..223 are not zero")
        return {"g": _bound(errs, "g", rel(g[..., :210], ref), 1e-5)}
    return Case(ops_, call, check)


@case("rp_rowdot96", "rows-3456")
def _rowdot():
    rows = 2 * HEADS * N_TOK
    a, b = rnd(1, rows, XW), rnd(2, rows, XW)
    ops_ = [inp("a", a), inp("b", b), flat("out", rows)]

    def call(lib, A_, st):
        lib.rp_rowdot96(P(A_["a"].addr()), P(A_["b"].addr()), P(A_["out"].addr()), rows, st)

    def check(v, errs):       # rho / gamma of test_emm_backward (5e-5)
        return {"out": _bound(errs, "out", rel(v["out"].view(-1), (a.double() * b.double()).sum(1)), 5e-5)}
    return Case(ops_, call, check)


def _emm_grad_case(Z, ld, entry, swap=False, s_in=False):
    """dq (swap = 0: the q columns, rows of image z ^ 1) / dk (swap = 1: the k columns) of the EMM against fp64 autograd at
    test_emm_backward's 5e-5; rp_emm_grad_ds also stores scale * dS key-major in rp_ds_matmul's (recompute form) or
    rp_ds_matmul_t's (s_in form) tiles"""
    d = _emm_data(Z)
    win = {"dk": (DIM, 2 * DIM)} if swap else {"dq": (0, DIM)}
    ops_ = [inp_multi("qkv", Z * N_TOK, ld, {0: d["qkv"][:, :2 * DIM]}), inp("x", _f32(d["x"]).view(-1, XW)),
            inp("w", _f32(d["wp"] if swap else d["w"]).view(-1, XW)), inp("rlse", _f32(d["rlse"]).reshape(1, -1)),
            inp("clse", _f32(d["clse"]).reshape(1, -1)), inp("rho", _f32(d["rho"]).reshape(1, -1)),
            inp("gamma", _f32(d["gamma"]).reshape(1, -1)), out("dqkv", Z * N_TOK, 3 * DIM, ld=ld, wins=win)]
    if entry == "rp_emm_grad_ds":
        ops_.append(flat("ds", Z * HEADS * N_TOK * N_TOK))
        if s_in:
            ops_.append(inp("s_in", _f32(_tile_runs(d["S2"])).reshape(1, -1)))

    def call(lib, A_, st):
        a = lambda n: P(A_[n].addr()) if n in A_ else None
        if entry == "rp_emm_grad":
            lib.rp_emm_grad(a("qkv"), ld, a("x"), a("w"), a("rlse"), a("clse"), a("rho"), a("gamma"), a("dqkv"), Z, HEADS, SCALE, int(swap),
                            0, 0, st)
        else:
            lib.rp_emm_grad_ds(a("qkv"), ld, a("x"), a("w"), a("rlse"), a("clse"), a("rho"), a("gamma"), a("s_in"), a("dqkv"), a("ds"), Z,
                               HEADS, SCALE, 0, 0, st)

    def check(v, errs):
        n = "dk" if swap else "dq"
        e = {n: _bound(errs, n, rel(v[n], d[n]), 5e-5)}
        if entry == "rp_emm_grad_ds":
            dst = d["dS"].transpose(-1, -2)                       # key-major: rows = keys j, columns = queries i
            if s_in:      # rp_ds_matmul_t's tiles: element (row a, column b) at ((a >> 2) * 32 + b) * 4 + (a & 3)
                ref = _tile_runs(dst.transpose(-1, -2)).reshape(Z, HEADS, 18, 18, 1024).transpose(2, 3)
            else:
                ref = _ds_tiles(dst)
            e["ds"] = _bound(errs, "ds", rel(v["ds"].view(-1), ref.reshape(-1)), 5e-5)
        return e
    return Case(ops_, call, check, sibling=None if ld == 3 * DIM else (lambda: _emm_grad_case(Z, 3 * DIM, entry, swap, s_in)))


for _z, _ld in ((2, 576), (6, 576), (2, 640), (6, 640)):
    _t = "Z%d-ld%d" % (_z, _ld)
    case("rp_emm_stats", _t)(lambda z=_z, l=_ld: _emm_stats_case(z, l, False))
    case("rp_emm_stats", _t + "-s_out")(lambda z=_z, l=_ld: _emm_stats_case(z, l, True))
    case("rp_emm_build_x", _t)(lambda z=_z, l=_ld: _emm_build_x_case(z, l, False))
    case("rp_emm_build_x_bwd", _t)(lambda z=_z, l=_ld: _emm_build_x_case(z, l, True))
    case("rp_emm_apply", _t)(lambda z=_z, l=_ld: _emm_apply_case(z, l))
    case("rp_emm_apply", _t + "-swap")(lambda z=_z, l=_ld: _emm_apply_case(z, l, swap=True))
    case("rp_emm_grad", _t + "-swap0")(lambda z=_z, l=_ld: _emm_grad_case(z, l, "rp_emm_grad"))
    case("rp_emm_grad", _t + "-swap1")(lambda z=_z, l=_ld: _emm_grad_case(z, l, "rp_emm_grad", swap=True))
    case("rp_emm_grad_ds", _t)(lambda z=_z, l=_ld: _emm_grad_case(z, l, "rp_emm_grad_ds"))
case("rp_emm_apply", "Z2-ld640-single")(lambda: _emm_apply_case(2, 640, single=True))
case("rp_emm_apply", "Z2-ld640-x_left")(lambda: _emm_apply_case(2, 640, x_left=True))
case("rp_emm_apply", "Z6-s_in")(lambda: _emm_apply_case(6, 576, s_in=True))
case("rp_emm_apply", "Z2-s_in-swap")(lambda: _emm_apply_case(2, 576, s_in=True, swap=True))
case("rp_emm_apply", "Z2-f-only")(lambda: _emm_apply_case(2, 576, want_t=False))
case("rp_emm_grad_ds", "Z6-s_in")(lambda: _emm_grad_case(6, 576, "rp_emm_grad_ds", s_in=True))
for _z in (2, 6):
    case("rp_emm_finalize", "Z%d" % _z)(lambda z=_z: _emm_finalize_case(z, NWG, "rp_emm_finalize"))
    case("rp_emm_finalize_parts", "Z%d-nparts1" % _z)(lambda z=_z: _emm_finalize_case(z, 1, "rp_emm_finalize_parts"))
    case("rp_emm_finalize_bwd", "Z%d" % _z)(lambda z=_z: _emm_finalize_case(z, NWG, "rp_emm_finalize_bwd"))
case("rp_emm_finalize_parts", "Z2-nparts6")(lambda: _emm_finalize_case(2, NWG, "rp_emm_finalize_parts"))


# ================================================================================================ weight-gradient products
def _dw192_case(M, N, lda):
    """rp_dw192_f32 leaves rp_dw192_f32_splits(M, N) slabs [split][N][192] in the workspace: here the workspace IS the output (exactly
    rp_dw192_f32_workspace_bytes), its slabs summed against fp64 at test_weight_gradient_output_stationary_fp32's 3e-6"""
    a, b = rnd(1, M, N), rnd(2, M, DIM)
    ops_ = [inp("a", a, ld=lda), inp("b", b)]
    state = {}

    def late(lib):
        state["sk"], state["ws"] = lib.rp_dw192_f32_splits(M, N), lib.rp_dw192_f32_workspace_bytes(M, N)
        assert state["ws"] == state["sk"] * N * DIM * 4, (state, "rp_dw192_f32_workspace_bytes is not splits * N * 192 floats")
        return [out("slabs", state["sk"] * N, DIM)]

    def call(lib, A_, st, wsb=None):
        lib.rp_dw192_f32(P(A_["a"].addr()), lda, P(A_["b"].addr()), M, N, P(A_["slabs"].addr()), state["ws"] if wsb is None else wsb, st)

    def check(v, errs):
        got = v["slabs"].double().view(state["sk"], N, DIM).sum(0)
        return {"dw": _bound(errs, "dw", rel(got, a.double().t() @ b.double()), 3e-6)}
    c = Case(ops_, call, check, lambda lib, A_, st: call(lib, A_, st, state["ws"] - 4),
             sibling=None if lda == N else (lambda: _dw192_case(M, N, N)))
    c.late = late
    return c


case("rp_dw192_f32", "M4736-N576")(lambda: _dw192_case(4096 + 640, 576, 576))
case("rp_dw192_f32", "M4736-N576-lda640")(lambda: _dw192_case(4096 + 640, 576, 640))
case("rp_dw192_f32", "M4736-N192-lda256")(lambda: _dw192_case(4096 + 640, 192, 256))


# ================================================================================================ CNN front-end (fp32 storage)
def _bn_data(shape):
    N, C, H, W = shape
    R = N * H * W
    x, res, dy = rnd(1, R, C) * 2 + 0.5, rnd(2, R, C), rnd(3, R, C)
    g, b = 1 + 0.2 * rnd(4, C), 0.2 * rnd(5, C)
    mean = x.double().mean(0)
    rstd = (x.double().var(0, unbiased=False) + 1e-5).rsqrt()
    return R, C, x, res, dy, g, b, mean, rstd


_BN_SHAPES = [(3, 192, 12, 12), (2, 128, 9, 7)]          # the odd shapes of test_fused_batchnorm_add_relu (bound 5e-6)


def _bn_stats_case(shape, running, from_partials):
    R, C, x, _, _, _, _, mean, rstd = _bn_data(shape)
    ops_ = [flat("mean", C), flat("rstd", C)]
    if running:
        ops_ += [inout("running_mean", torch.zeros(C)), inout("running_var", torch.ones(C))]
    nblk = 3
    if from_partials:
        cuts = [0, R // 3, R // 2, R]
        part = torch.stack([torch.stack([x[a:b].double().sum(0), (x[a:b].double() ** 2).sum(0)]) for a, b in zip(cuts, cuts[1:])])
        ops_ += [inp("partial", part.view(1, -1), dtype=F64), inp("pivot", torch.zeros(C))]
    else:
        ops_.append(inp("x", x))

    def late(lib):
        return [] if from_partials else [work("partial", lib.rp_bn_partial_blocks(R) * 2 * C * 8)]

    def call(lib, A_, st):
        if from_partials:
            lib.rp_bn_stats_from_partials(a_(A_, "partial"), nblk, R, C, a_(A_, "pivot"), a_(A_, "mean"), a_(A_, "rstd"), a_(A_, "running_mean"),
                                          a_(A_, "running_var"), 0.1, 1e-5, st)
        else:
            lib.rp_bn_stats(a_(A_, "x"), R, C, a_(A_, "partial"), a_(A_, "mean"), a_(A_, "rstd"), a_(A_, "running_mean"), a_(A_, "running_var"),
                            0.1, 1e-5, 0, st)

    def check(v, errs):
        e = {"mean": _bound(errs, "mean", rel(v["mean"].view(-1), mean), 5e-6), "rstd": _bound(errs, "rstd", rel(v["rstd"].view(-1), rstd), 5e-6)}
        if running:
            e["running_var"] = _bound(errs, "running_var", rel(v["running_var"].view(-1), 0.9 + 0.1 * x.double().var(0, unbiased=True)), 5e-6)
        return e
    c = Case(ops_, call, check)
    c.late = late
    return c


def _bn_apply_case(shape, with_res, relu):
    R, C, x, res, _, g, b, mean, rstd = _bn_data(shape)
    ops_ = [inp("x", x), inp("mean", mean.float()), inp("rstd", rstd.float()), inp("gamma", g), inp("beta", b), out("y", R, C)]
    if with_res:
        ops_.append(inp("residual", res))

    def call(lib, A_, st):
        lib.rp_bn_apply_fwd(a_(A_, "x"), a_(A_, "mean"), a_(A_, "rstd"), a_(A_, "gamma"), a_(A_, "beta"), a_(A_, "residual"), a_(A_, "y"), R, C,
                            int(relu), 0, st)

    def check(v, errs):
        y = (x.double() - mean) * rstd * g.double() + b.double() + (res.double() if with_res else 0)
        return {"y": _bound(errs, "y", rel(v["y"], y.clamp_min(0) if relu else y), 5e-6)}
    return Case(ops_, call, check)


def _bn_bwd_case(shape, with_res, training, from_partials=False):
    R, C, x, res, dy, g, b, mean, rstd = _bn_data(shape)
    xh = (x.double() - mean) * rstd
    y = (xh * g.double() + b.double() + (res.double() if with_res else 0)).clamp_min(0)
    gm = dy.double() * (y > 0)
    ops_ = [inp("x", x), inp("mean", mean.float()), inp("rstd", rstd.float()), inp("gamma", g), out("dx", R, C), flat("dgamma", C),
            flat("dbeta", C), work("c12", 2 * C * 4)]
    nblk = 2
    if from_partials:
        h = R // 2
        part = torch.stack([torch.stack([gm[a:c].sum(0), (gm[a:c] * xh[a:c]).sum(0)]) for a, c in ((0, h), (h, R))])
        ops_ += [inp("g", gm.float()), inp("partial", part.view(1, -1), dtype=F64)]
    else:
        ops_ += [inp("dy", dy), inp("beta", b)]
        if with_res:
            ops_ += [inp("y", y.float()), out("dres", R, C)]

    def late(lib):
        return [] if from_partials else [work("partial", lib.rp_bn_partial_blocks(R) * 2 * C * 8)]

    def call(lib, A_, st):
        if from_partials:
            lib.rp_bn_bwd_from_partials(a_(A_, "g"), a_(A_, "x"), a_(A_, "mean"), a_(A_, "rstd"), a_(A_, "gamma"), a_(A_, "partial"), nblk,
                                        a_(A_, "dx"), a_(A_, "dgamma"), a_(A_, "dbeta"), a_(A_, "c12"), R, C, st)
        else:
            lib.rp_bn_bwd(a_(A_, "dy"), a_(A_, "y"), a_(A_, "x"), a_(A_, "mean"), a_(A_, "rstd"), a_(A_, "gamma"), a_(A_, "beta"), a_(A_, "dx"),
                          a_(A_, "dres"), a_(A_, "dgamma"), a_(A_, "dbeta"), a_(A_, "partial"), a_(A_, "c12"), R, C, 1, int(training), 0, st)

    def check(v, errs):
        gr = g.double() * rstd
        dx = gr * (gm - gm.mean(0) - xh * (gm * xh).mean(0)) if training else gr * gm
        return {"dx": _bound(errs, "dx", rel(v["dx"], dx), 5e-6),
                "dgamma": _bound(errs, "dgamma", rel(v["dgamma"].view(-1), (gm * xh).sum(0)), 5e-6),
                "dbeta": _bound(errs, "dbeta", rel(v["dbeta"].view(-1), gm.sum(0)), 5e-6)}
    c = Case(ops_, call, check)
    c.late = late
    return c


for _s in _BN_SHAPES:
    _t = "x".join(map(str, _s))
    case("rp_bn_stats", _t + "-running")(lambda s=_s: _bn_stats_case(s, True, False))
    case("rp_bn_stats_from_partials", _t + "-running")(lambda s=_s: _bn_stats_case(s, True, True))
    case("rp_bn_apply_fwd", _t + "-residual-relu")(lambda s=_s: _bn_apply_case(s, True, True))
    case("rp_bn_bwd", _t + "-residual-training")(lambda s=_s: _bn_bwd_case(s, True, True))
    case("rp_bn_bwd_from_partials", _t)(lambda s=_s: _bn_bwd_case(s, False, True, from_partials=True))
case("rp_bn_stats", "2x128x9x7-no-running")(lambda: _bn_stats_case(_BN_SHAPES[1], False, False))
case("rp_bn_apply_fwd", "2x128x9x7-plain")(lambda: _bn_apply_case(_BN_SHAPES[1], False, False))
case("rp_bn_bwd", "2x128x9x7-recomputed-mask-eval")(lambda: _bn_bwd_case(_BN_SHAPES[1], False, False))


def _pool_ref(x_nhwc):
    """torch's MaxPool2d(3, 2, 1) on the CPU and the window position 0..8 of every maximum"""
    N, H, W, C = x_nhwc.shape
    y, flat_ = torch.nn.functional.max_pool2d(x_nhwc.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    OH, OW = y.shape[2:]
    ih, iw = flat_ // W, flat_ % W
    oh, ow = torch.arange(OH).view(1, 1, OH, 1), torch.arange(OW).view(1, 1, 1, OW)
    pos = (ih - (2 * oh - 1)) * 3 + (iw - (2 * ow - 1))
    return y.permute(0, 2, 3, 1).contiguous(), pos.permute(0, 2, 3, 1).contiguous().to(torch.uint8)


def _pool_case(shape, bwd):
    """bit-identical to torch (test_maxpool3x3s2_matches_torch_including_ties)"""
    N, C, H, W = shape
    x = rnd(1, N, H, W, C)
    y, pos = _pool_ref(x)
    OH, OW = y.shape[1:3]
    dy = rnd(2, N, OH, OW, C)
    if bwd:
        ops_ = [inp("dy", dy.view(-1, C)), inp("idx", pos.view(-1, C), dtype=U8), out("dx", N * H * W, C)]
    else:
        ops_ = [inp("x", x.view(-1, C)), out("y", N * OH * OW, C), out("idx", N * OH * OW, C, dtype=U8)]

    def call(lib, A_, st):
        if bwd:
            lib.rp_maxpool3x3s2_bwd(a_(A_, "dy"), a_(A_, "idx"), a_(A_, "dx"), N, H, W, C, 0, st)
        else:
            lib.rp_maxpool3x3s2_fwd(a_(A_, "x"), a_(A_, "y"), a_(A_, "idx"), N, H, W, C, 0, st)

    def check(v, errs):
        if bwd:
            xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
            torch.nn.functional.max_pool2d(xr, 3, 2, 1).backward(dy.permute(0, 3, 1, 2))
            if not torch.equal(v["dx"].cpu().view(N, H, W, C), xr.grad.permute(0, 2, 3, 1)):
                errs.append("dx differs from torch's max-pool backward")
        elif not (torch.equal(v["y"].cpu().view(y.shape), y) and torch.equal(v["idx"].cpu().view(pos.shape), pos)):
            errs.append("y / idx differ from torch's max-pool")
        return {}
    return Case(ops_, call, check)


for _s in [(3, 64, 20, 28), (2, 8, 7, 9), (1, 4, 1, 2)]:
    case("rp_maxpool3x3s2_fwd", "x".join(map(str, _s)))(lambda s=_s: _pool_case(s, False))
    case("rp_maxpool3x3s2_bwd", "x".join(map(str, _s)))(lambda s=_s: _pool_case(s, True))


def _bn_pool_case(shape, training, bwd):
    """the fused stem chain: forward bit-identical to BatchNorm-apply + ReLU + pool, backward to 2e-6
    (test_fused_stem_batchnorm_relu_maxpool_is_bit_identical_to_the_separate_kernels)"""
    N, C, H, W = shape
    R, _, x, _, _, g, b, mean, rstd = _bn_data(shape)
    a = ((x.double() - mean) * rstd * g.double() + b.double()).clamp_min(0).view(N, H, W, C)
    y, pos = _pool_ref(a)
    OH, OW = y.shape[1:3]
    dp = rnd(6, N, OH, OW, C)
    ops_ = [inp("x", x), inp("mean", mean.float()), inp("rstd", rstd.float()), inp("gamma", g), inp("beta", b)]
    if bwd:
        ops_ += [inp("dp", dp.view(-1, C)), inp("idx", pos.view(-1, C), dtype=U8), out("dx", R, C), flat("dgamma", C), flat("dbeta", C),
                 work("c12", 2 * C * 4)]
    else:
        ops_ += [out("y", N * OH * OW, C), out("idx", N * OH * OW, C, dtype=U8)]

    def late(lib):
        return [work("partial", lib.rp_bn_partial_blocks(R) * 2 * C * 8)] if bwd else []

    def call(lib, A_, st):
        if bwd:
            lib.rp_bn_relu_pool_bwd(a_(A_, "dp"), a_(A_, "idx"), a_(A_, "x"), a_(A_, "mean"), a_(A_, "rstd"), a_(A_, "gamma"), a_(A_, "beta"),
                                    a_(A_, "dx"), a_(A_, "dgamma"), a_(A_, "dbeta"), a_(A_, "partial"), a_(A_, "c12"), N, H, W, C,
                                    int(training), 0, st)
        else:
            lib.rp_bn_relu_pool_fwd(a_(A_, "x"), a_(A_, "mean"), a_(A_, "rstd"), a_(A_, "gamma"), a_(A_, "beta"), a_(A_, "y"), a_(A_, "idx"),
                                    N, H, W, C, 0, st)

    def check(v, errs):
        if not bwd:
            return {"y": _bound(errs, "y", rel(v["y"].view(y.shape), y), 2e-6)}
        ar = a.permute(0, 3, 1, 2).clone().requires_grad_(True)
        torch.nn.functional.max_pool2d(ar, 3, 2, 1).backward(dp.double().permute(0, 3, 1, 2))
        gm = (ar.grad.permute(0, 2, 3, 1) * (a > 0)).reshape(R, C)
        xh = (x.double() - mean) * rstd
        gr = g.double() * rstd
        dx = gr * (gm - gm.mean(0) - xh * (gm * xh).mean(0)) if training else gr * gm
        return {"dx": _bound(errs, "dx", rel(v["dx"], dx), 2e-6), "dgamma": _bound(errs, "dgamma", rel(v["dgamma"].view(-1), (gm * xh).sum(0)), 2e-6),
                "dbeta": _bound(errs, "dbeta", rel(v["dbeta"].view(-1), gm.sum(0)), 2e-6)}
    c = Case(ops_, call, check)
    c.late = late
    return c


for _s, _tr in (((3, 8, 9, 11), True), ((2, 16, 10, 7), False)):
    case("rp_bn_relu_pool_fwd", "x".join(map(str, _s)))(lambda s=_s, t=_tr: _bn_pool_case(s, t, False))
    case("rp_bn_relu_pool_bwd", "x".join(map(str, _s)) + ("-training" if _tr else "-eval"))(lambda s=_s, t=_tr: _bn_pool_case(s, t, True))


def _conv64_case(N, igrad=False, res=False, bn=False, stats=False):
    """rp_conv3x3_c64_f32 against fp64 F.conv2d at test_conv3x3_c64_forward_and_input_gradient_exact_fp32's 2e-6 (plain forms)"""
    x, w = rnd(1, N, 56, 56, 64), rnd(2, 64, 3, 3, 64, scale=(64 * 9) ** -0.5)
    r, xb = rnd(3, N * 3136, 64), rnd(4, N * 3136, 64)
    ops_ = [inp("x", x.view(-1, 64)), inp("w", w.view(64, -1)), out("y", N * 3136, 64)]
    if res:
        ops_.append(inp("res", r))
    if bn:
        ops_ += [inp("bn_x", xb), inp("bn_mean", 0.1 * rnd(5, 64)), inp("bn_rstd", 1 + 0.1 * rnd(6, 64).abs()), inp("bn_gamma", 1 + 0.1 * rnd(7, 64)),
                 inp("bn_beta", 0.1 * rnd(8, 64))]

    def late(lib):
        return [out("stats", lib.rp_conv3x3_c64_f32_blocks(N), 128, dtype=F64)] if stats else []

    def call(lib, A_, st):
        m = None
        if bn:
            from rel_pose_amd import _lib
            mk = _lib.RpBnMask()
            mk.x, mk.mean, mk.rstd, mk.gamma, mk.beta = (A_[n].addr() for n in ("bn_x", "bn_mean", "bn_rstd", "bn_gamma", "bn_beta"))
            m = ctypes.byref(mk)
        lib.rp_conv3x3_c64_f32(a_(A_, "x"), a_(A_, "w"), a_(A_, "y"), a_(A_, "stats"), a_(A_, "res"), m, N, 56, 56, int(igrad), st)

    def check(v, errs):
        if bn:
            return {}
        wc = w.double().permute(0, 3, 1, 2)                       # [co, ci, r, s]
        if igrad:
            wc = wc.flip(2, 3).transpose(0, 1)
        ref = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), wc, None, 1, 1).permute(0, 2, 3, 1).reshape(-1, 64)
        ref = ref + (r.double() if res else 0)
        e = {"y": _bound(errs, "y", rel(v["y"], ref), 2e-6)}
        if stats:     # sums of the stored values: 2e-7 in that test
            st_ = v["stats"].view(-1, 2, 64).sum(0).cpu()
            e["sum"] = _bound(errs, "stats", rel(st_[0], v["y"].double().sum(0)), 2e-7)
        return e
    c = Case(ops_, call, check)
    c.late = late
    return c


case("rp_conv3x3_c64_f32", "N1-forward")(lambda: _conv64_case(1))
case("rp_conv3x3_c64_f32", "N3-forward-stats")(lambda: _conv64_case(3, stats=True))
case("rp_conv3x3_c64_f32", "N3-input-gradient-res-stats")(lambda: _conv64_case(3, igrad=True, res=True, stats=True))
case("rp_conv3x3_c64_f32", "N1-input-gradient-bn-stats")(lambda: _conv64_case(1, igrad=True, bn=True, stats=True))
case("rp_conv3x3_c64_f32", "N3-input-gradient-bn-stats")(lambda: _conv64_case(3, igrad=True, bn=True, stats=True))


def _conv128_case(N, CO, igrad=False, bias=False, stats=False):
    """rp_conv3x3_c128_f32 at test_conv3x3_c128_forward_and_input_gradient_exact_fp32's 2e-6"""
    x, w, b = rnd(1, N, 28, 28, 128), rnd(2, CO, 3, 3, 128, scale=(128 * 9) ** -0.5), rnd(3, CO)
    ops_ = [inp("x", x.view(-1, 128)), inp("w", w.view(CO, -1)), out("y", N * 784, CO)]
    if bias:
        ops_.append(inp("bias", b))

    def late(lib):
        return [out("stats", lib.rp_conv3x3_c128_f32_blocks(N, CO) // (CO // 64), 2 * CO, dtype=F64)] if stats else []

    def call(lib, A_, st):
        lib.rp_conv3x3_c128_f32(a_(A_, "x"), a_(A_, "w"), a_(A_, "bias"), a_(A_, "y"), a_(A_, "stats"), N, 28, 28, CO, int(igrad), st)

    def check(v, errs):
        wc = w.double().permute(0, 3, 1, 2)
        if igrad:
            wc = wc.flip(2, 3).transpose(0, 1)
        ref = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), wc, b.double() if bias else None, 1, 1).permute(0, 2, 3, 1).reshape(-1, CO)
        e = {"y": _bound(errs, "y", rel(v["y"], ref), 2e-6)}
        if stats:
            e["sum"] = _bound(errs, "stats", rel(v["stats"].view(-1, 2, CO).sum(0).cpu()[0], v["y"].double().sum(0)), 2e-7)
        return e
    c = Case(ops_, call, check)
    c.late = late
    return c


case("rp_conv3x3_c128_f32", "N1-CO128-stats")(lambda: _conv128_case(1, 128, stats=True))
case("rp_conv3x3_c128_f32", "N3-CO192-bias-stats")(lambda: _conv128_case(3, 192, bias=True, stats=True))
case("rp_conv3x3_c128_f32", "N3-CO128-input-gradient")(lambda: _conv128_case(3, 128, igrad=True))


def _wgrad64_case(N):
    """rp_conv3x3_c64_wgrad_f32 against fp64 autograd at test_conv3x3_c64_weight_gradient_exact_fp32's 3e-6"""
    x, dy = rnd(1, N, 56, 56, 64), rnd(5, N, 56, 56, 64)
    ops_ = [inp("x", x.view(-1, 64)), inp("dy", dy.view(-1, 64)), out("dw", 64, 576)]
    state = {}

    def late(lib):
        state["ws"] = lib.rp_conv3x3_c64_wgrad_f32_workspace_bytes(N)
        return [work("workspace", state["ws"])]

    def call(lib, A_, st, wsb=None):
        lib.rp_conv3x3_c64_wgrad_f32(a_(A_, "x"), a_(A_, "dy"), a_(A_, "dw"), a_(A_, "workspace"), state["ws"] if wsb is None else wsb, N, 56, 56, st)

    def check(v, errs):
        w = torch.zeros(64, 64, 3, 3, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w, None, 1, 1).backward(dy.double().permute(0, 3, 1, 2))
        return {"dw": _bound(errs, "dw", rel(v["dw"].view(64, 3, 3, 64), w.grad.permute(0, 2, 3, 1)), 3e-6)}
    c = Case(ops_, call, check, lambda lib, A_, st: call(lib, A_, st, state["ws"] - 4))
    c.late = late
    return c


case("rp_conv3x3_c64_wgrad_f32", "N1")(lambda: _wgrad64_case(1))
case("rp_conv3x3_c64_wgrad_f32", "N3")(lambda: _wgrad64_case(3))


def _framed(N, H, W):
    x = torch.zeros(N, H + 6, W + 6, 3)
    x[:, 3:-3, 3:-3] = rnd(1, N, H, W, 3)
    return x


def _stem_fwd_case(N, H, W, stats):
    """rp_conv_stem_fwd against fp64 F.conv2d at test_hand_written_stem_convolution's 2e-6"""
    x, w = _framed(N, H, W), rnd(2, 64, 7, 7, 3, scale=147 ** -0.5)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ops_ = [inp("x_padded", x.view(-1, 3)), inp("w", w.view(64, -1)), out("y", N * OH * OW, 64)]

    def late(lib):
        return [out("stats", lib.rp_conv_stem_blocks(N, H, W), 128, dtype=F64)] if stats else []

    def call(lib, A_, st):
        lib.rp_conv_stem_fwd(a_(A_, "x_padded"), a_(A_, "w"), a_(A_, "y"), a_(A_, "stats"), N, H, W, st)

    def check(v, errs):
        ref = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None, 2, 0).permute(0, 2, 3, 1)
        e = {"y": _bound(errs, "y", rel(v["y"], ref.reshape(-1, 64)), 2e-6)}
        if stats:
            e["sum"] = _bound(errs, "stats", rel(v["stats"].view(-1, 2, 64).sum(0).cpu()[0], v["y"].double().sum(0)), 2e-6)
        return e
    c = Case(ops_, call, check)
    c.late = late
    return c


case("rp_conv_stem_fwd", "N1-32x32")(lambda: _stem_fwd_case(1, 32, 32, False))
case("rp_conv_stem_fwd", "N3-64x96-stats")(lambda: _stem_fwd_case(3, 64, 96, True))
case("rp_conv_stem_fwd", "N1-224x224-stats")(lambda: _stem_fwd_case(1, 224, 224, True))


def _stem_wgrad_case(N):
    """rp_conv_stem_wgrad_f32 against fp64 autograd at test_stem_weight_gradient_exact_fp32's 3e-6"""
    x, dy = _framed(N, 224, 224), rnd(3, N, 112, 112, 64)
    ops_ = [inp("x_padded", x.view(-1, 3)), inp("dy", dy.view(-1, 64)), out("dw", 64, 147)]
    state = {}

    def late(lib):
        state["ws"] = lib.rp_conv_stem_wgrad_f32_workspace_bytes(N)
        return [work("workspace", state["ws"])]

    def call(lib, A_, st, wsb=None):
        lib.rp_conv_stem_wgrad_f32(a_(A_, "x_padded"), a_(A_, "dy"), a_(A_, "dw"), a_(A_, "workspace"), state["ws"] if wsb is None else wsb,
                                   N, 224, 224, st)

    def check(v, errs):
        w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w, None, 2, 0).backward(dy.double().permute(0, 3, 1, 2))
        return {"dw": _bound(errs, "dw", rel(v["dw"].view(64, 7, 7, 3), w.grad.permute(0, 2, 3, 1)), 3e-6)}
    c = Case(ops_, call, check, lambda lib, A_, st: call(lib, A_, st, state["ws"] - 4))
    c.late = late
    return c


case("rp_conv_stem_wgrad_f32", "N1")(lambda: _stem_wgrad_case(1))
case("rp_conv_stem_wgrad_f32", "N3")(lambda: _stem_wgrad_case(3))


# ================================================================================================ small kernels
def _tokens_case(entry, Z=2, C=DIM, N=N_TOK):
    """index operations, bit-exact (test_colsum_tokens_posenc_pose)"""
    feat, pe, dx = rnd(1, Z, C, N), rnd(2, N, C), rnd(3, Z, N, C)
    if entry == "rp_tokens_bwd":
        ops_ = [inp("dx", dx.view(-1, C)), out("dfeat", Z * C, N)]
    elif entry == "rp_tokens_fwd":
        ops_ = [inp("feat", feat.view(-1, N)), inp("pos_embed", pe), out("x", Z * N, C)]
    else:
        ops_ = [inp("feat", dx.view(-1, C)), inp("pos_embed", pe), out("x", Z * N, C)]

    def call(lib, A_, st):
        if entry == "rp_tokens_bwd":
            lib.rp_tokens_bwd(a_(A_, "dx"), a_(A_, "dfeat"), Z, C, N, st)
        else:
            getattr(lib, entry)(a_(A_, "feat"), a_(A_, "pos_embed"), a_(A_, "x"), Z, C, N, st)

    def check(v, errs):
        if entry == "rp_tokens_bwd":
            ok = torch.equal(v["dfeat"].cpu().view(Z, C, N), dx.transpose(1, 2).contiguous())
        elif entry == "rp_tokens_fwd":
            ok = torch.equal(v["x"].cpu().view(Z, N, C), feat.transpose(1, 2) + pe)
        else:
            ok = torch.equal(v["x"].cpu().view(Z, N, C), dx + pe)
        if not ok:
            errs.append("not bit-exact")
        return {}
    return Case(ops_, call, check)


for _e in ("rp_tokens_fwd", "rp_tokens_fwd_nhwc", "rp_tokens_bwd"):
    case(_e, "Z2")(lambda e=_e: _tokens_case(e))
    case(_e, "Z3-C64-N96")(lambda e=_e: _tokens_case(e, 3, 64, 96))


def _preprocess_case(Z, H, W, pad):
    img = torch.floor(torch.rand(Z, 3, H, W, generator=torch.Generator().manual_seed(3)) * 256).clamp_max(255)
    S = 224 + 2 * (pad or 0)
    ops_ = [inp("images", img.view(-1, W)), out("out", Z * S * S, 3)]

    def call(lib, A_, st):
        if pad is None:
            lib.rp_preprocess(a_(A_, "images"), a_(A_, "out"), Z, H, W, st)
        else:
            lib.rp_preprocess_padded(a_(A_, "images"), a_(A_, "out"), Z, H, W, pad, st)

    def check(v, errs):
        o = v["out"].cpu().view(Z, S, S, 3)
        if pad:
            frame = o.clone()
            frame[:, pad:-pad, pad:-pad] = 0
            if float(frame.abs().max()) != 0.0 or bool(torch.isnan(frame).any()):
                errs.append("the %d-pixel frame is not zero" % pad)
            o = o[:, pad:-pad, pad:-pad]
        iy = (torch.arange(224) * (H / 224.0)).floor().long()          # nearest resize as F.interpolate(mode="nearest")
        ix = (torch.arange(224) * (W / 224.0)).floor().long()
        src = img[:, [2, 1, 0]][:, :, iy][:, :, :, ix].permute(0, 2, 3, 1).double() / 255.0
        ref = (src - torch.tensor([0.485, 0.456, 0.406], dtype=torch.float64)) / torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64)
        return {"out": _bound(errs, "out", rel(o, ref), 1e-6)}       # (the kernel is bit-exact against the fp32 oracle; fp64 here: one ulp)
    c = Case(ops_, call, check)
    return c


case("rp_preprocess", "Z2-256x320")(lambda: _preprocess_case(2, 256, 320, None))
case("rp_preprocess_padded", "Z2-256x320-pad3")(lambda: _preprocess_case(2, 256, 320, 3))
case("rp_preprocess_padded", "Z3-480x640-pad3")(lambda: _preprocess_case(3, 480, 640, 3))


def _golden():
    import os
    import numpy as np
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_outputs.npz"))


def _posenc_case(B, l1, with_intr):
    """golden: the reference's own positional features for these intrinsics (test_colsum_tokens_posenc_pose: 3e-7; none: bit-exact)"""
    intr = torch.tensor([[32.373, 25.898, 12.0, 12.0], [18.0, 21.0, 12.0, 9.0], [25.0, 25.0, 11.0, 13.0]])[:B, None, :].repeat(1, 2, 1)
    ops_ = [inp("lin24", torch.linspace(-1, 1, steps=24, dtype=torch.float32)), out("pos", B * N_TOK, 6)]
    if with_intr:
        ops_.append(inp("intrinsics", intr.reshape(1, -1)))

    def call(lib, A_, st):
        lib.rp_posenc(a_(A_, "intrinsics"), a_(A_, "lin24"), a_(A_, "pos"), B, int(l1), st)

    def check(v, errs):
        if l1 or B != 2:
            return {}
        pos = v["pos"].cpu().view(B, N_TOK, 6)
        if with_intr:
            return {"pos": _bound(errs, "pos", rel(pos, torch.as_tensor(_golden()["posenc_intr_f32"])), 3e-7)}
        if not torch.equal(pos, torch.as_tensor(_golden()["posenc_none_f32"])):
            errs.append("pos without intrinsics is not bit-exact")
        return {}
    return Case(ops_, call, check)


case("rp_posenc", "B2-intrinsics")(lambda: _posenc_case(2, False, True))
case("rp_posenc", "B2-no-intrinsics")(lambda: _posenc_case(2, False, False))
case("rp_posenc", "B3-l1-intrinsics")(lambda: _posenc_case(3, True, True))


def _unit_poses(seed, B):
    p = rnd(seed, B, 2, 7)
    p[..., 3:] = torch.nn.functional.normalize(p[..., 3:], dim=-1)
    return p


def _pose_norm_case(B, bwd):
    """against the oracle's normalize_preds in fp64 (test_colsum_tokens_posenc_pose: forward 1e-6, slot 0 copied exactly; backward 1e-5)"""
    pred, gs, dout = rnd(1, B, 2, 7), rnd(2, B, 2, 7), rnd(3, B, 2, 7)
    pred[3, 1, 3:] *= 1e-3                                    # exercises the max(|q|, 0.01) clamp
    if bwd:
        ops_ = [inp("pred", pred.view(B, 14)), inp("dout", dout.view(B, 14)), out("dpred", B, 14)]
    else:
        ops_ = [inp("pred", pred.view(B, 14)), inp("gs", gs.view(B, 14)), out("out", B, 14)]

    def call(lib, A_, st):
        if bwd:
            lib.rp_pose_normalize_bwd(a_(A_, "pred"), a_(A_, "dout"), a_(A_, "dpred"), B, st)
        else:
            lib.rp_pose_normalize_fwd(a_(A_, "pred"), a_(A_, "gs"), a_(A_, "out"), B, st)

    def check(v, errs):
        from oracle import relpose_oracle as O
        if bwd:
            p64 = pred.double().requires_grad_(True)
            (O.normalize_preds(gs.double(), p64) * dout.double()).sum().backward()
            return {"dpred": _bound(errs, "dpred", rel(v["dpred"].view(B, 2, 7), p64.grad), 1e-5)}
        o = v["out"].cpu().view(B, 2, 7)
        if not torch.equal(o[:, 0], gs[:, 0]):
            errs.append("slot 0 is not Gs")
        return {"out": _bound(errs, "out", rel(o, O.normalize_preds(gs.double(), pred.double())), 1e-6)}
    return Case(ops_, call, check)


case("rp_pose_normalize_fwd", "B5")(lambda: _pose_norm_case(5, False))
case("rp_pose_normalize_bwd", "B5")(lambda: _pose_norm_case(5, True))


@case("rp_geodesic_loss", "B37")
def _geodesic():
    """against the PyTorch SE(3) formulation in fp64, value 2e-6 and gradient 2e-5 (test_fused_geodesic_loss_matches_se3_autograd, same
    special pairs; pair 0 sits on the singularity of |tau|, |phi| and is only required to be finite there, as in that test)"""
    B = 37
    Ps, Gs = _unit_poses(1, B), _unit_poses(2, B)
    Gs[..., :3] *= 0.7
    ident = torch.tensor([0, 0, 0, 0, 0, 0, 1.0])
    Ps[:, 0], Gs[:, 0] = ident, ident
    Gs[0, 1] = Ps[0, 1]
    Gs[1, 1, 3:] = -Gs[1, 1, 3:]
    Gs[2, 1, 3:] = torch.tensor([0.0, 0.0, 0.96, -0.28])
    ops_ = [inp("Ps", Ps.view(B, 14)), inp("Gs", Gs.view(B, 14)), flat("losses", 2), flat("dmean", 2 * B * 14), work("scratch", 60 * B * 4)]

    def call(lib, A_, st):
        lib.rp_geodesic_loss(a_(A_, "Ps"), a_(A_, "Gs"), a_(A_, "losses"), a_(A_, "dmean"), a_(A_, "scratch"), B, st)

    def check(v, errs):
        from rel_pose_amd.losses import geodesic_loss_tensors_torch
        from rel_pose_amd.se3 import SE3
        e, dm = {}, v["dmean"].cpu().view(2, B, 2, 7)
        if not bool(torch.isfinite(dm).all()):
            errs.append("dmean is not finite")
        for m, name in enumerate(("tr", "rot")):
            Gr = Gs.double().requires_grad_(True)
            loss = geodesic_loss_tensors_torch(SE3(Ps.double()), [SE3(Gr)])[m]
            loss.backward()
            e[name] = _bound(errs, "losses[%d]" % m, rel(v["losses"].view(-1)[m], loss.detach()), 2e-6)
            e["d" + name] = _bound(errs, "dmean[%d]" % m, rel(dm[m, 1:], Gr.grad[1:]), 2e-5)
        return e
    return Case(ops_, call, check)


@case("rp_augment_pairs", "B6-60x80-to-48x64")
def _augment():
    """integer arithmetic, EXACT against RGBDAugmentor.apply + nearest resize (test_fused_augmentation_is_pils_arithmetic_bit_for_bit)"""
    from rel_pose_amd.data_readers.augmentation import RGBDAugmentor
    B, H, W, Ho, Wo = 6, 60, 80, 48, 64
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (B, 2, H, W, 3), generator=g, dtype=torch.uint8)
    params = RGBDAugmentor(reshape_size=[Ho, Wo], generator=g).draw_batch(B).float()
    params[:, 8] = (torch.arange(B) % 2 == 0).float()
    params[-1] = RGBDAugmentor(reshape_size=[Ho, Wo], jitter=False).draw_batch(1)[0]
    ops_ = [inp("images", img.view(-1, W * 3), dtype=U8), inp("params", params), out("out", B * 2 * 3 * Ho, Wo)]

    def late(lib):
        return [work("workspace", B * lib.rp_augment_blocks() * 8)]

    def call(lib, A_, st):
        lib.rp_augment_pairs(a_(A_, "images"), a_(A_, "params"), a_(A_, "out"), a_(A_, "workspace"), B, H, W, Ho, Wo, st)

    def check(v, errs):
        o = v["out"].cpu().view(B, 2, 3, Ho, Wo)
        for b in range(B):
            x = img[b].permute(0, 3, 1, 2).float()
            ref = torch.nn.functional.interpolate(RGBDAugmentor.apply(x, RGBDAugmentor.params_to_dict(params[b])), size=[Ho, Wo])
            if not torch.equal(o[b], ref):
                errs.append("pair %d differs from RGBDAugmentor.apply + nearest resize" % b)
        return {}
    c = Case(ops_, call, check)
    c.late = late
    return c


@functools.lru_cache(maxsize=2)
def _two_view(n, Pn):
    """poses, their essential matrices (LAPACK-side oracle) and Pn points in front of both cameras: test_pose_from_essential_round_trip's setup"""
    from oracle import svd3x3_oracle as SO
    g = torch.Generator().manual_seed(17)
    pose = torch.zeros(n, 7)
    pose[:, :3] = torch.randn(n, 3, generator=g)
    ax = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    half = torch.rand(n, 1, generator=g) * 2.0 - 1.0
    pose[:, 3:6], pose[:, 6:] = ax * torch.sin(half), torch.cos(half)
    R, t = torch.from_numpy(SO.rotation_from_quat(pose[:, 3:].numpy())), pose[:, :3].double()
    X1 = torch.empty(n, Pn, 3, dtype=torch.float64)
    for i in range(n):
        got = 0
        while got < Pn:
            cand = torch.cat([torch.randn(64, 2, generator=g, dtype=torch.float64) * 2.0, torch.rand(64, 1, generator=g, dtype=torch.float64) * 6.0 + 1.0], 1)
            ok = cand[(cand @ R[i].T + t[i])[:, 2] > 0.5]
            k = min(Pn - got, ok.shape[0])
            X1[i, got:got + k] = ok[:k]
            got += k
    X2 = torch.einsum("nij,npj->npi", R, X1) + t[:, None, :]
    E = torch.from_numpy(SO.essential_from_pose(pose.numpy())).float()
    return pose, E, (X1[..., :2] / X1[..., 2:]).float(), (X2[..., :2] / X2[..., 2:]).float()


def _geom_case(entry, n=37, Pn=12):
    pose, E, x1, x2 = _two_view(n, Pn)
    A = rnd(2, n, 9)
    if entry == "rp_essential_from_pose":
        ops_ = [inp("pose", pose), out("E", n, 9)]
    elif entry == "rp_svd3x3":
        ops_ = [inp("A", A), out("U", n, 9), out("S", n, 3), out("V", n, 9)]
    else:
        ops_ = [inp("E", E.reshape(n, 9)), inp("x1", x1.reshape(n, -1)), inp("x2", x2.reshape(n, -1)), out("pose", n, 7), out("count", 1, n, dtype=I32)]

    def call(lib, A_, st):
        if entry == "rp_essential_from_pose":
            lib.rp_essential_from_pose(a_(A_, "pose"), a_(A_, "E"), n, st)
        elif entry == "rp_svd3x3":
            lib.rp_svd3x3(a_(A_, "A"), a_(A_, "U"), a_(A_, "S"), a_(A_, "V"), n, st)
        else:
            lib.rp_pose_from_essential(a_(A_, "E"), a_(A_, "x1"), a_(A_, "x2"), Pn, a_(A_, "pose"), a_(A_, "count"), n, st)

    def check(v, errs):
        if entry == "rp_essential_from_pose":      # test_svd3x3_and_essential_matrix_vs_lapack: 2e-6
            return {"E": _bound(errs, "E", rel(v["E"].view(n, 3, 3), E.double()), 2e-6)}
        if entry == "rp_svd3x3":       # U diag(S) V^T reconstructs A, U and V orthogonal: 3e-6 in that test
            U, S, V = v["U"].double().view(n, 3, 3).cpu(), v["S"].double().cpu(), v["V"].double().view(n, 3, 3).cpu()
            eye = torch.eye(3, dtype=torch.float64)
            return {"usv": _bound(errs, "U S V^T", rel(U @ torch.diag_embed(S) @ V.transpose(1, 2), A.view(n, 3, 3)), 3e-6),
                    "orth": _bound(errs, "U^T U, V^T V", max(float((U.transpose(1, 2) @ U - eye).abs().max()),
                                                            float((V.transpose(1, 2) @ V - eye).abs().max())), 3e-6)}
        # test_pose_from_essential_round_trip: the input pose comes back (angle 2e-3 rad, t direction 1 - 1e-6), every point in front
        o, cnt = v["pose"].double().cpu(), v["count"].cpu().view(-1)
        if not bool((cnt == Pn).all()):
            errs.append("count: not every point is in front of both cameras")
        tn = pose[:, :3].double() / pose[:, :3].double().norm(dim=1, keepdim=True)
        ang = 2.0 * torch.acos((o[:, 3:] * pose[:, 3:].double()).sum(1).abs().clamp(max=1.0))
        cos_t = (o[:, :3] * tn).sum(1)
        if not float(cos_t.min()) > 1.0 - 1e-6:
            errs.append("t direction cosine %.9f" % float(cos_t.min()))
        return {"angle": _bound(errs, "rotation angle", float(ang.max()), 2e-3)}
    return Case(ops_, call, check)


for _e in ("rp_essential_from_pose", "rp_svd3x3", "rp_pose_from_essential"):
    case(_e, "n37")(lambda e=_e: _geom_case(e))
    case(_e, "n300")(lambda e=_e: _geom_case(e, 300))


# ================================================================================================ not covered here
_BF16_PATH = "bf16 data path (BASELINE.json configs[4]): reached at wrapper level by the poisoned-allocator runs of the bf16 configuration"
UNCOVERED = {n: _BF16_PATH for n in (
    "rp_conv_stem_fwd_bf16", "rp_conv_stem_wgrad_bf16", "rp_conv3x3_c64_bf16", "rp_conv3x3_c64_wgrad_bf16", "rp_attn_fwd_bf16",
    "rp_attn_bwd_delta_bf16", "rp_attn_bwd_bf16", "rp_dw192_bf16", "rp_dx_lnbwd_bf16", "rp_emm_build_x_bf16", "rp_emm_apply_bf16",
    "rp_emm_f_bf16", "rp_emm_w_bf16", "rp_emm_dx_bf16", "rp_emm_grad_bf16")}
UNCOVERED["rp_dw192_split3"] = "opt-in kernel (RP_DW_SPLIT3=1), same slabs and arguments as rp_dw192_f32; not on any default path"
