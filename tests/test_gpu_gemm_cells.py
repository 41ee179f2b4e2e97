"""rp_gemm's dispatch table, cell by cell, on operands for which the right answer is exact (tests/_gemm_cells.py: families, references,
the mirror of the dispatch and the case table; tests/test_gemm_cells_cpu.py proves the premises on the CPU).

Cases run through ops.gemm; those it cannot express -- the rows of colsum_part, a private NaN-filled workspace for split-K, defer_reduce --
go through the C structure (ctypes), as tests/_contract_cases.py does.  Every operand is stored with NaN pad columns
and NaN gaps, every output is NaN before the call: the stored values must equal the integer reference BIT FOR BIT (torch.equal; a
bf16-stored C: the reference rounded to nearest even) and the pads must still be NaN.  The only bounded comparisons are the GELU / GELU'
outputs and the GELU' column sums, under tests/_norm_regimes.py's bound rule against fp64 of the exact pre-activation; the worst share of
the limit per test goes to the test report.

test_refusals: one call per `return RP_E*` of rp_gemm and rp_splitk_reduce_multi -- host side only, no kernel runs, the documented status
and an untouched NaN-filled C.  (defer_reduce with an epilogue is refused BEFORE the main kernel is launched.)"""
import ctypes
import re

import pytest
import torch

from tests import _gemm_cells as G
from tests import _norm_regimes as R
from tests.test_gpu_kernels import report

pytestmark = pytest.mark.gpu

NAN = float("nan")
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    return _lib.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ld(cols):
    return cols + 4 if cols % 4 == 0 else (cols // 4 + 1) * 4


class Buf:
    """[batch, rows, cols] inside a NaN-filled flat buffer: row stride ld = cols + 4, batch stride rows * ld + GAP"""

    def __init__(self, batch, rows, cols, dtype, data=None, ld=None):
        self.shape, self.ld = (batch, rows, cols), (_ld(cols) if ld is None else ld)
        self.stride = rows * self.ld + (G.GAP if batch > 1 else 0)
        self.flat = torch.full((batch * self.stride,), NAN, dtype=dtype, device="cuda")
        if data is not None:
            self.view().copy_(data)

    def view(self):
        b, r, c = self.shape
        return self.flat.as_strided((b, r, c), (self.stride, self.ld, 1))

    def ptr(self):
        return self.flat.data_ptr()

    def pads_untouched(self):
        b, r, c = self.shape
        return int(self.flat.isnan().sum()) == self.flat.numel() - b * r * c + int(self.view().isnan().sum())


class Launch:
    def __init__(self, c, lib):
        from rel_pose_amd import _lib
        self.c, self.lib = c, lib
        v = self.v = G.values(c, "cuda")
        b = c.batch
        self.A = Buf(b, *((c.M, c.K) if c.al == 0 else (c.K, c.M)), BF if c.io & 1 else F32, v["A"] if c.al == 0 else v["A"].transpose(1, 2))
        self.B = Buf(b, *((c.N, c.K) if c.bl == 0 else (c.K, c.N)), F32, v["B"] if c.bl == 0 else v["B"].transpose(1, 2))
        crows, ccols = (c.N, c.M) if c.trans_c else (c.M, c.N)
        cdt = BF if c.io & 2 else F32
        self.C = Buf(b, crows, ccols, cdt)
        self.pre = Buf(b, c.M, c.N, cdt) if c.pre else None
        self.bias = Buf(1, 1, c.N, F32, v["bias"].view(1, 1, -1)) if c.bias else None
        self.aux = Buf(b, c.M, c.N, BF if c.io & 4 else F32, v["aux"]) if G.has_aux(c) else None
        self.res = Buf(b, c.M, c.N, F32, v["res"]) if c.res else None
        self.cs = torch.full((G.colsum_rows(c), c.N), NAN, device="cuda") if c.colsum else None
        self.ws = None
        g = self.g = _lib.RpGemm()
        g.A, g.B, g.C = self.A.ptr(), self.B.ptr(), self.C.ptr()
        g.M, g.N, g.K = c.M, c.N, c.K
        g.lda, g.ldb, g.ldc = self.A.ld, self.B.ld, self.C.ld
        g.a_layout, g.b_layout, g.batch = c.al, c.bl, b
        g.stride_a, g.stride_b, g.stride_c = self.A.stride, self.B.stride, self.C.stride
        g.split_k = c.split
        if c.split > 1:
            nbytes = lib.rp_gemm_workspace_bytes(c.M, c.N, c.split)
            assert nbytes == c.split * c.M * c.N * 4
            self.ws = torch.full((nbytes // 4 + 64,), NAN, device="cuda")          # 64 floats of guard behind the slabs
            g.workspace, g.workspace_bytes = self.ws.data_ptr(), nbytes
        for nm, buf in (("bias", self.bias), ("pre_out", self.pre), ("aux", self.aux), ("residual", self.res)):
            if buf is not None:
                setattr(g, nm, buf.ptr())
        if self.cs is not None:
            g.colsum_part = self.cs.data_ptr()
        g.act, g.dact, g.trans_c, g.precision, g.io_bf16 = c.act, c.dact, int(c.trans_c), c.prec, c.io

    def run(self, defer=False):
        c = self.c
        if c.split == 1 and not c.colsum:           # everything ops.gemm can express goes through it (its io_bf16 / stride plumbing too)
            from rel_pose_amd import ops
            flat = lambda b: None if b is None else b.flat
            ops.gemm(self.A.flat, self.B.flat, c.M, c.N, c.K, a_layout=c.al, b_layout=c.bl, lda=self.A.ld, ldb=self.B.ld, out=self.C.flat,
                     ldc=self.C.ld, bias=flat(self.bias), act=c.act, pre_out=flat(self.pre), dact=c.dact, aux=flat(self.aux),
                     residual=flat(self.res), split_k=1, batch=c.batch, strides=(self.A.stride, self.B.stride, self.C.stride),
                     precision=c.prec)
            return self
        self.g.defer_reduce = int(defer)
        self.lib.rp_gemm(ctypes.byref(self.g), _stream())
        return self

    def task(self, t):
        c = self.c
        t.ws, t.C, t.M, t.N, t.ldc, t.split_k, t.trans_c = self.ws.data_ptr(), self.C.ptr(), c.M, c.N, self.C.ld, c.split, int(c.trans_c)


class Judge:
    def __init__(self, key):
        self.key, self.failed, self.worst, self.n = key, [], 0.0, 0

    def fail(self, c, what):
        self.failed.append("%s: %s" % (G.name(c), what))

    def exact(self, c, what, got, want):
        if got.shape != want.shape or not torch.equal(got, want):
            bad = (got.double() != want.double()) | got.isnan()
            at = tuple(int(i) for i in bad.nonzero()[0])
            self.fail(c, "%s: %d of %d elements differ, first at %s: got %r, want %r" % (
                what, int(bad.sum()), bad.numel(), at, float(got[at]), float(want[at])))

    def bounded(self, c, what, got, yard, want, scale=None, extra=0.0):
        if not bool(torch.isfinite(got.float()).all()):
            return self.fail(c, what + ": not finite")
        n = want.numel()
        scale = torch.ones(n, dtype=F64) if scale is None else scale.flatten()
        j = R.judge("elem", got.flatten(), yard.flatten(), want.flatten(), {"all": torch.arange(n)}, scale=scale, extra=extra)[0]
        self.worst = max(self.worst, j["of_limit"])
        if not j["of_limit"] <= 1.0:
            self.fail(c, "%s: %.3e at %d = %.2f x its limit (plain fp32: %.3e)" % (what, j["err"], j["where"], j["of_limit"], j["yard"]))

    def done(self):
        report("gemm_cells.%s.lay%d%d.p%d" % self.key, cases=self.n, worst_activation_of_limit=self.worst)
        assert not self.failed, "%d of %d cases -- " % (len({f.split(":")[0] for f in self.failed}), self.n) + "; ".join(self.failed[:6])


def check(jd, c, L):
    """the outputs of one finished launch against the exact reference"""
    jd.n += 1
    v = L.v
    P = G.product(c, v)
    pre64, out64 = G.epilogue(c, P, v, F64)
    store = (lambda t: t.float().to(BF)) if c.io & 2 else (lambda t: t.float())
    tr = (lambda t: t.transpose(1, 2)) if c.trans_c else (lambda t: t)
    got = L.C.view()
    yard = None
    if G.inexact(c):
        yard = G.epilogue(c, P, v, F32)[1]
        jd.bounded(c, "C", got, yard, out64, extra=R.BF16_STORE if c.io & 2 else 0.0)
    else:
        jd.exact(c, "C", got, store(tr(out64)))
    if not L.C.pads_untouched():
        jd.fail(c, "C: pad columns / gaps written")
    if c.pre:
        jd.exact(c, "pre_out", L.pre.view(), store(pre64))
        if not L.pre.pads_untouched():
            jd.fail(c, "pre_out: pad columns / gaps written")
    if c.colsum:
        if G.inexact(c):
            jd.bounded(c, "colsum_part", L.cs, G.colsum_ref(c, yard[0]), G.colsum_ref(c, out64[0]),
                       scale=G.colsum_ref(c, out64[0].square()).sqrt().cpu())
        else:
            jd.exact(c, "colsum_part", L.cs, G.colsum_ref(c, out64[0]).float())
    if L.ws is not None and not bool(L.ws[-64:].isnan().all()):
        jd.fail(c, "workspace: written past rp_gemm_workspace_bytes")


KEYS = G.keys()


@pytest.mark.parametrize("group,al,bl,prec", KEYS, ids=["%s-lay%d%d-p%d" % k for k in KEYS])
def test_cells(lib, group, al, bl, prec):
    jd = Judge((group, al, bl, prec))
    for c in G.cases(group, al, bl, prec):
        check(jd, c, Launch(c, lib).run())
    jd.done()


@pytest.mark.parametrize("al,bl", G.LAYOUTS, ids=["lay%d%d" % l for l in G.LAYOUTS])
@pytest.mark.parametrize("prec", G.PRECISIONS)
def test_deferred_multi_reduce(lib, al, bl, prec):
    """8 split-K products of different shapes (some trans_c) left in their workspaces and finished by ONE rp_splitk_reduce_multi: exact, and
    bit-equal to the undeferred calls"""
    from rel_pose_amd import _lib
    jd = Judge(("defer", al, bl, prec))
    tasks = G.defer_tasks((al, bl), prec)
    assert len(tasks) == _lib.RP_SPLITK_MAX == 8
    direct = [Launch(c, lib).run() for c in tasks]
    deferred = [Launch(c, lib).run(defer=True) for c in tasks]
    for c, L in zip(tasks, deferred):
        assert bool(L.C.flat.isnan().all()), G.name(c) + ": a deferred call wrote C"
    arr = (_lib.RpSplitkTask * len(tasks))()
    for t, L in zip(arr, deferred):
        L.task(t)
    lib.rp_splitk_reduce_multi(arr, len(tasks), _stream())
    for c, L, D in zip(tasks, deferred, direct):
        check(jd, c, L)
        jd.exact(c, "deferred vs direct", L.C.view(), D.C.view())
    jd.done()


# ------------------------------------------------------------------------------------------------ refusals
OK, EBADSHAPE, EALIGN, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3, -4
BIG = 1 << 18


def _refusal_rows():
    rows = []

    def add(name, code, **kw):
        rows.append((name, code, kw))

    for k in ("M", "N", "K"):
        add(k + "=0", EBADSHAPE, **{k: 0})
    add("a_layout=2", EBADSHAPE, a_layout=2)
    add("b_layout=-1", EBADSHAPE, b_layout=-1)
    add("lda%4", EALIGN, lda=38)
    add("ldb%4", EALIGN, ldb=38)
    add("ldc%4", EALIGN, ldc=62)
    add("K%4 with a K-contiguous operand", EALIGN, K=38, lda=40, ldb=40)
    add("M%4 with a_layout=1", EALIGN, a_layout=1, M=66, lda=68)
    add("N%4 with b_layout=1", EALIGN, b_layout=1, N=62, ldb=64, ldc=64)
    for k in ("A", "B", "C"):
        add(k + " not 16-byte aligned", EALIGN, **{k: ("off", k, 4)})
    add("batch with split", EUNSUPPORTED, batch=2, split_k=2, workspace="ws")
    for k in ("stride_a", "stride_b", "stride_c"):
        add("batch with %s %% 4" % k, EALIGN, batch=2, **{k: 68 * 64 + 2})
    add("split with N%4", EALIGN, split_k=2, workspace="ws", N=62, ldc=64)
    add("split without workspace", EWORKSPACE, split_k=2)
    add("split with a short workspace", EWORKSPACE, split_k=2, workspace="ws", workspace_bytes=2 * 68 * 60 * 4 - 4)
    add("io_bf16 at precision 0", EUNSUPPORTED, io_bf16=1)
    add("io_bf16 with batch", EUNSUPPORTED, io_bf16=1, precision=1, batch=2)
    add("io_bf16 unknown bit", EUNSUPPORTED, io_bf16=8, precision=1)
    add("bf16 C with split", EUNSUPPORTED, io_bf16=2, precision=1, split_k=2, workspace="ws")
    add("bf16 C with residual", EUNSUPPORTED, io_bf16=2, precision=1, residual="res")
    add("bf16 C with N%4", EUNSUPPORTED, io_bf16=2, precision=1, N=62, ldc=64)
    add("bf16 C with layout 11", EUNSUPPORTED, io_bf16=2, precision=1, a_layout=1, b_layout=1, lda=68, ldb=60)
    add("bf16 C with ln_x", EUNSUPPORTED, io_bf16=2, precision=1, ln_x="aux")
    add("bf16 aux without aux", EBADSHAPE, io_bf16=4, precision=1)
    add("bf16 C with a generic epilogue", EUNSUPPORTED, io_bf16=2, precision=1, act=2)
    add("bf16 aux with layout 11", EUNSUPPORTED, io_bf16=4, precision=1, dact=1, aux="aux", a_layout=1, b_layout=1, lda=68, ldb=60)
    add("bf16 aux with split", EUNSUPPORTED, io_bf16=4, precision=1, dact=1, aux="aux", split_k=2, workspace="ws")
    add("ln_x without ln_mean", EBADSHAPE, ln_x="aux", ln_rstd="aux", ln_gamma="aux", ln_part="res")
    ln = dict(ln_x="aux", ln_mean="aux", ln_rstd="aux", ln_gamma="aux", ln_part="res")
    add("ln_* with N != 192", EUNSUPPORTED, **ln)
    add("ln_* with bias", EUNSUPPORTED, N=192, ldc=192, bias="bias", **ln)
    add("ln_* with split", EUNSUPPORTED, N=192, ldc=192, split_k=2, workspace="ws", **ln)
    add("colsum with split", EUNSUPPORTED, colsum_part="res", split_k=2, workspace="ws")
    add("colsum with batch", EUNSUPPORTED, colsum_part="res", batch=2)
    add("colsum with N%4", EUNSUPPORTED, colsum_part="res", N=62, ldc=64)
    add("colsum with layout 11", EUNSUPPORTED, colsum_part="res", a_layout=1, b_layout=1, lda=68, ldb=60)
    add("colsum with a (1,3) tile", EUNSUPPORTED, colsum_part="res", b_layout=1, N=192, ldb=192, ldc=192)
    add("colsum with a generic epilogue", EUNSUPPORTED, colsum_part="res", act=2)
    add("precision 2", EUNSUPPORTED, precision=2)
    add("trans_c without split", EUNSUPPORTED, trans_c=1)
    add("trans_c with bias", EUNSUPPORTED, trans_c=1, split_k=2, workspace="ws", bias="bias")
    add("defer_reduce with an epilogue", EUNSUPPORTED, defer_reduce=1, split_k=2, workspace="ws", bias="bias")
    return rows


REFUSALS = _refusal_rows()


@pytest.fixture(scope="module")
def refusal_bufs(lib):
    b = {k: torch.zeros(BIG, device="cuda") for k in ("A", "B", "aux", "res", "bias", "ws")}
    b["C"] = torch.full((BIG,), NAN, device="cuda")
    return b


def _refused(call, code):
    with pytest.raises(RuntimeError) as e:
        call()
    m = re.search(r"RP error (-?\d+)", str(e.value))
    assert m and int(m.group(1)) == code, str(e.value)


@pytest.mark.parametrize("name,code,kw", REFUSALS, ids=[re.sub(r"\W+", "_", r[0]) for r in REFUSALS])
def test_refusals(lib, refusal_bufs, name, code, kw):
    from rel_pose_amd import _lib
    bufs = refusal_bufs
    g = _lib.RpGemm()
    g.A, g.B, g.C = (bufs[k].data_ptr() for k in "ABC")
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc = 68, 60, 36, 36, 36, 60
    g.batch, g.split_k = 1, 1
    g.stride_a, g.stride_b, g.stride_c = 68 * 64, 64 * 64, 68 * 64
    for k, val in kw.items():
        if isinstance(val, tuple):
            val = bufs[val[1]].data_ptr() + val[2]
        elif isinstance(val, str):
            if k == "workspace" and "workspace_bytes" not in kw:
                g.workspace_bytes = BIG * 4
            val = bufs[val].data_ptr()
        setattr(g, k, val)
    _refused(lambda: lib.rp_gemm(ctypes.byref(g), _stream()), code)
    torch.cuda.synchronize()
    assert bool(bufs["C"].isnan().all()), name + ": C was written by a refused call"


def test_null_struct_is_refused(lib):
    _refused(lambda: lib.rp_gemm(None, _stream()), EBADSHAPE)


REDUCE_REFUSALS = [("no tasks", EBADSHAPE, dict(n=0)), ("too many tasks", EBADSHAPE, dict(n=9)), ("null tasks", EBADSHAPE, dict(null=True)),
                   ("ws null", EBADSHAPE, dict(ws=None)), ("C null", EBADSHAPE, dict(C=None)), ("M=0", EBADSHAPE, dict(M=0)),
                   ("N=0", EBADSHAPE, dict(N=0)), ("N%4", EBADSHAPE, dict(N=62)), ("split_k=1", EBADSHAPE, dict(split_k=1)),
                   ("ldc%4", EALIGN, dict(ldc=62)), ("ws not 16-byte aligned", EALIGN, dict(ws=("off", "ws", 4))),
                   ("C not 16-byte aligned", EALIGN, dict(C=("off", "C", 4)))]


@pytest.mark.parametrize("name,code,kw", REDUCE_REFUSALS, ids=[re.sub(r"\W+", "_", r[0]) for r in REDUCE_REFUSALS])
def test_reduce_multi_refusals(lib, refusal_bufs, name, code, kw):
    from rel_pose_amd import _lib
    bufs = refusal_bufs
    arr = (_lib.RpSplitkTask * 9)()
    for t in arr:
        t.ws, t.C, t.M, t.N, t.ldc, t.split_k, t.trans_c = bufs["ws"].data_ptr(), bufs["C"].data_ptr(), 68, 60, 60, 2, 0
    for k, val in kw.items():
        if k in ("n", "null"):
            continue
        if isinstance(val, tuple):
            val = bufs[val[1]].data_ptr() + val[2]
        setattr(arr[1], k, val)
    _refused(lambda: lib.rp_splitk_reduce_multi(None if kw.get("null") else arr, kw.get("n", 2), _stream()), code)
    torch.cuda.synchronize()
    assert bool(bufs["C"].isnan().all()), name + ": C was written by a refused call"
