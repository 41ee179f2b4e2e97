"""GPU parity tests, kernel by kernel, through the C ABI (ctypes) on a real MI355X.

References: (i) the CPU oracle (oracle/relpose_oracle.py, pinned against the real reference by
tests/test_oracle_golden.py) evaluated in fp64; (ii) for op-level checks at larger sizes, the same op written
in plain PyTorch fp64 on the GPU.  Tolerances are stated per test; index/layout ops are bit-exact.
Measured errors are appended to gpurun_out/test_report.txt.

These tests check VALUES.  Where a kernel writes, that it writes all of its output, and that it does not depend on what its output
held before (guard bands, poisoned outputs, strided layouts) is the memory contract: tests/test_gpu_memory_contract.py over the
case table of tests/_contract_cases.py.  (The attention launchers read their RP_ATTN_FWD / RP_ATTN_NW overrides once per process, so
test_attention_fwd_bwd[2] only selects the two-wave workgroups when it is the first attention launch of the process; the two-wave
forms are reached by size in test_attention_stored_p_fwd_bwd[30], the full-size tests and the Z = 20 cases of the contract table, and
are value-tested by size -- forward, stored-P, recompute and cross backward, per 32-row block and per head against fp64 in peaked, flat,
climbing and large softmax regimes -- by the Z = 20 cases of tests/test_gpu_softmax_regimes.py.)
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def report(name, **kv):
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "test_report.txt"), "a") as f:
        f.write(name + ": " + ", ".join("%s=%.3e" % (k, v) for k, v in kv.items()) + "\n")


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, ops as o
    _lib.load()
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed + int(np.prod(shape)) % 9973)
    return (torch.randn(*shape, generator=g) * scale).cuda()


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("M,N,K", [(128, 192, 192), (1152, 576, 192), (200, 768, 192), (70, 192, 224), (64, 512, 2688),
                                   (33, 16, 512), (1152, 192, 768), (130, 100, 36)])
@pytest.mark.parametrize("al,bl", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("prec", [0, 3])
def test_gemm_layouts(ops, M, N, K, al, bl, prec):
    """both fp32-grade operand precisions (0 = exact fp32 MFMA, the default; 3 = split-bf16 limbs), same tolerance"""
    if (al == 1 and M % 4) or (bl == 1 and N % 4):
        pytest.skip("contiguous extent must be a multiple of 4")
    A = rnd(M, K, seed=1)
    Bm = rnd(N, K, seed=2)
    ref = A.double() @ Bm.double().t()
    Ain = A if al == 0 else A.t().contiguous()
    Bin = Bm if bl == 0 else Bm.t().contiguous()
    out = ops.gemm(Ain, Bin, M, N, K, a_layout=al, b_layout=bl, split_k=1, precision=prec)
    e = rel(out, ref)
    report("gemm[%d,%d,%d|%d%d|p%d]" % (M, N, K, al, bl, prec), rel=e)
    assert e < 2e-6
    # A = I with an asymmetric B catches transposed C writes (exact in both precisions: 1 * b = b1 + b2 + b3)
    if M == K and al == 0 and bl == 0:
        eye = torch.eye(M, device="cuda")
        assert torch.equal(ops.gemm(eye, Bm, M, N, K, split_k=1, precision=prec), Bm.t().contiguous())


def test_gemm_operand_precisions(ops):
    """RpGemm.precision: 3 (three bf16 limbs per operand, six limb products) must be fp32-grade -- no worse than the exact
    fp32 MFMA kernel against fp64, also with a wide dynamic range and cancellation; 1 (bf16 operands) must really be bf16."""
    M, N, K = 1152, 192, 768
    g = torch.Generator(device="cpu").manual_seed(5)
    A = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-12, 12, (M, 1), generator=g).float())).cuda()
    W = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-6, 6, (1, K), generator=g).float())).cuda()
    A[:, 1::2] = -A[:, ::2] * (1 + 1e-3 * torch.randn(M, K // 2, generator=g).cuda())      # pairwise cancellation
    W[:, 1::2] = W[:, ::2]
    ref = A.double() @ W.double().t()
    scale = (A.double().abs() @ W.double().abs().t())          # condition-aware: error relative to sum |a||b| per row

    def err(p):
        c = ops.gemm(A, W, M, N, K, precision=p, split_k=1)
        return float(((c.double() - ref).abs() / scale).max())
    e0, e3, e1 = err(0), err(3), err(1)
    report("gemm_precisions", fp32_mfma=e0, split_bf16x3=e3, bf16=e1)
    assert e0 < 3e-7 and e3 < 3e-7 and e3 < 2 * e0 + 1e-8
    assert 1e-4 < e1 < 1e-2
    with pytest.raises(RuntimeError):
        ops.gemm(A, W, M, N, K, precision=2)
    # very small and huge operands survive the truncation split (bf16 has fp32's exponent range; only below ~1e-33 would
    # the third limb drop into the subnormals)
    tiny = torch.full((64, 32), 3e-30, device="cuda")
    big = torch.full((64, 32), 1e18, device="cuda")
    out = ops.gemm(tiny, big, 64, 64, 32, precision=3, split_k=1)
    assert rel(out, tiny.double() @ big.double().t()) < 1e-6


def test_gemm_epilogues_splitk_batch(ops):
    M, N, K = 300, 192, 768
    A, W, b, R = rnd(M, K, seed=3), rnd(N, K, seed=4, scale=0.05), rnd(N, seed=5), rnd(M, N, seed=6)
    pre_ref = A.double() @ W.double().t() + b.double()
    gelu = lambda x: 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))
    y, pre = ops.linear(A, W, b, act=1, want_pre=True, residual=R)
    assert rel(pre, pre_ref) < 2e-6
    assert rel(y, gelu(pre_ref) + R.double()) < 2e-6
    y2 = ops.linear(A, W, b, act=2)
    assert rel(y2, pre_ref.clamp_min(0)) < 2e-6
    # derivative epilogues
    aux = rnd(M, N, seed=7)
    x64 = aux.double().requires_grad_(True)
    gelu(x64).sum().backward()
    d1 = ops.gemm(A, W, M, N, K, dact=1, aux=aux)
    assert rel(d1, (A.double() @ W.double().t()) * x64.grad) < 2e-6
    d2 = ops.gemm(A, W, M, N, K, dact=2, aux=aux)
    assert rel(d2, (A.double() @ W.double().t()) * (aux > 0)) < 2e-6
    # split-K (deterministic: two runs bit-identical) incl. epilogue in the reduce kernel
    for sk in (2, 5, 24):
        o1 = ops.gemm(A, W, M, N, K, bias=b, act=2, residual=R, split_k=sk)
        o2 = ops.gemm(A, W, M, N, K, bias=b, act=2, residual=R, split_k=sk)
        assert torch.equal(o1, o2)
        assert rel(o1, pre_ref.clamp_min(0) + R.double()) < 2e-6
    # weight-gradient form: dW = dY^T X over many rows, auto split-K
    Mt = 4608
    dY, X = rnd(Mt, 192, seed=8), rnd(Mt, 768, seed=9)
    dw = ops.linear_dw(dY, X)
    e = rel(dw, dY.double().t() @ X.double())
    report("gemm_dw", rel=e)
    assert e < 2e-6
    dw2, db2 = ops.linear_dw_db(dY, X)                    # bias gradient fused into the weight-gradient GEMM
    assert torch.equal(dw2, dw) and rel(db2, dY.double().sum(0)) < 2e-6
    dYs, Xs = rnd(300, 16, seed=15), rnd(300, 512, seed=16)      # small-M path (regressor): no split
    dws, dbs = ops.linear_dw_db(dYs, Xs)
    assert rel(dws, dYs.double().t() @ Xs.double()) < 2e-6 and rel(dbs, dYs.double().sum(0)) < 2e-6
    dx = ops.linear_dx(dY, rnd(192, 768, seed=10))
    assert rel(dx, dY.double() @ rnd(192, 768, seed=10).double()) < 2e-6
    # batched 576x96 @ 96x96 (EMM backward shapes)
    Xb, Db = rnd(2, 3, 576, 96, seed=11), rnd(2, 3, 96, 96, seed=12)
    assert rel(ops._bmm96(Xb, Db, False), Xb.double() @ Db.double()) < 2e-6
    assert rel(ops._bmm96(Xb, Db, True, residual=Xb), Xb.double() @ Db.double().transpose(-1, -2) + Xb.double()) < 2e-6
    # regressor shape: M=2 rows, K=26880, split-K
    F_, W0 = rnd(2, 26880, seed=13), rnd(512, 26880, seed=14, scale=0.01)
    e = rel(ops.linear(F_, W0, act=2), (F_.double() @ W0.double().t()).clamp_min(0))
    report("gemm_regressor", rel=e)
    assert e < 5e-6


@pytest.mark.parametrize("prec", [0, 3])
def test_gemm_epilogue_column_sums(ops, prec):
    """RpGemm.colsum_part: sum_m C[m][n] of the stored (post-epilogue) values from the epilogue itself -- ragged M and N tiles,
    GELU' epilogue (the fc1 bias gradient) and plain bias epilogue"""
    M, N, K = 1000, 200, 192
    dy, W, aux, b = rnd(M, K, seed=31), rnd(K, N, seed=32, scale=0.1), rnd(M, N, seed=33), rnd(N, seed=34)
    out, cs = ops.gemm(dy, W, M, N, K, b_layout=1, dact=1, aux=aux, want_colsum=True, precision=prec, split_k=1)
    x = aux.double()
    ggrad = 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5
    ref = (dy.double() @ W.double()) * ggrad
    assert rel(out, ref) < 5e-6 and rel(cs, ref.sum(0)) < 5e-6
    assert rel(cs, out.double().sum(0)) < 2e-6                 # sums of exactly the values that were stored
    Wt = rnd(N, K, seed=35, scale=0.1)
    out2, cs2 = ops.gemm(dy, Wt, M, N, K, bias=b, want_colsum=True, precision=prec, split_k=1)
    assert rel(cs2, out2.double().sum(0)) < 2e-6
    with pytest.raises(RuntimeError):
        ops.gemm(dy, Wt, M, 192, K, b_layout=0, a_layout=0, want_colsum=True, split_k=2)


def test_gemm_bf16_storage_of_activation_operands(ops):
    """RpGemm.io_bf16 (bf16 configuration, operand precision 1): A / aux read as bf16, C / pre_out written as bf16.  The MFMA operands
    are bf16 in this precision anyway, so with bf16-representable inputs the bf16-stored launch must equal the fp32-stored one BIT FOR
    BIT, and a bf16 output must be the round-to-nearest-even of the fp32 output -- for the K-contiguous and the MN-contiguous A layout,
    the GELU + pre-activation and the GELU' epilogues, and ragged M."""
    bf = torch.bfloat16
    M, K, N = 1000, 192, 768
    x, W, b = rnd(M, K, seed=1).to(bf), rnd(N, K, seed=2) * 0.07, rnd(N, seed=3) * 0.1
    # fc1-like: GELU + pre-activation, outputs in bf16
    pre32 = torch.empty(M, N, device="cuda")
    y32 = ops.gemm(x.float(), W, M, N, K, bias=b, act=1, pre_out=pre32, precision=1)
    pre16 = torch.empty(M, N, device="cuda", dtype=bf)
    y16 = ops.gemm(x, W, M, N, K, bias=b, act=1, pre_out=pre16, precision=1, out_dtype=bf)
    assert y16.dtype == bf and torch.equal(y16, y32.to(bf)) and torch.equal(pre16, pre32.to(bf))
    # fc2-like: A = h (bf16, K-contiguous), fp32 output + residual
    W2, res = rnd(K, N, seed=4) * 0.05, rnd(M, K, seed=5)
    a = ops.gemm(y16, W2, M, K, N, residual=res, precision=1)
    b_ = ops.gemm(y16.float(), W2, M, K, N, residual=res, precision=1)
    assert a.dtype == torch.float32 and torch.equal(a, b_)
    # input gradient with GELU'(aux): aux bf16, output bf16
    dy = rnd(M, K, seed=6)
    d32 = ops.gemm(dy, W2, M, N, K, b_layout=1, dact=1, aux=pre16.float(), precision=1)
    d16 = ops.gemm(dy, W2, M, N, K, b_layout=1, dact=1, aux=pre16, precision=1, out_dtype=bf)
    assert torch.equal(d16, d32.to(bf))
    # weight gradient: A = dh (bf16, MN-contiguous), split-K
    xn = rnd(M, K, seed=7)
    w32 = ops.gemm(d16.float(), xn, N, K, M, a_layout=1, b_layout=1, precision=1, split_k=4)
    w16 = ops.gemm(d16, xn, N, K, M, a_layout=1, b_layout=1, precision=1, split_k=4)
    assert torch.equal(w16, w32)
    assert rel(w16, d16.double().t() @ xn.double()) < 2e-2
    with pytest.raises(RuntimeError):
        ops.gemm(x, W, M, N, K, precision=0)          # bf16-stored operands only exist in the bf16 configuration


def test_gemm_precision1_epilogue_uses_the_bf16_configurations_gelu_pair(ops):
    """at operand precision 1 the BF instantiations of mlp_fused / linear_rows compute the sigmoid ("tanh") GELU and its exact
    derivative; rp_gemm's GELU / GELU' epilogues -- the fallback path (ops.ROWS_LINEAR / ROWS_DX / FUSE_MLP* = False, and every shape the row-resident kernels do not take) -- must be
    the SAME function, or forward and backward of one step disagree.  With bf16-representable operands the products are exact, so the
    epilogue is visible at fp32 accuracy: <= 3e-6 against the tanh form, and measurably (> 1e-4) away from the erf form; precisions 0
    and 3 (the fp32-grade parity modes) keep the reference's erf GELU (vision_transformer.py:397, mlp.py:22)."""
    import torch.nn.functional as F
    bf = torch.bfloat16
    q = lambda t: t.to(bf).float()
    M, K, N = 1152, 192, 768
    x, W, b = q(rnd(M, K, seed=1, scale=2.0)), q(rnd(N, K, seed=2, scale=0.1)), 0.1 * rnd(N, seed=3)
    pre = F.linear(x.double(), W.double(), b.double())
    for prec, approx, other in ((1, "tanh", "none"), (0, "none", "tanh"), (3, "none", "tanh")):      # (the split-bf16 parity mode is pinned to erf too)
        y = ops.gemm(x, W, M, N, K, bias=b, act=1, precision=prec)
        e_same, e_other = rel(y, F.gelu(pre, approximate=approx)), rel(y, F.gelu(pre, approximate=other))
        assert e_same < 3e-6 and e_other > 3e-5, (prec, e_same, e_other)
        # GELU'(aux) epilogue: dx = (dy W2) o GELU'(aux)
        dy, W2 = q(rnd(M, K, seed=6)), q(rnd(K, N, seed=4, scale=0.05))
        aux = q(rnd(M, N, seed=7, scale=1.5))
        a = aux.double().requires_grad_(True)
        F.gelu(a, approximate=approx).sum().backward()
        d = ops.gemm(dy, W2, M, N, K, b_layout=1, dact=1, aux=aux, precision=prec)
        assert rel(d, (dy.double() @ W2.double()) * a.grad) < 5e-6, prec
    # and the row-resident default kernels of the bf16 configuration agree with the rp_gemm fallback to fp32 rounding
    prev = ops.GEMM_PRECISION
    ops.set_gemm_precision(1)
    try:
        xr = q(rnd(M, 192, seed=11))
        h_rows = ops.linear_rows(xr, W, b, act=1)
        h_gemm = ops.gemm(xr, W, M, N, K, bias=b, act=1, precision=1)
        assert rel(h_rows, h_gemm) < 3e-6
    finally:
        ops.set_gemm_precision(prev)


@pytest.mark.parametrize("N", [3, 37, 256])
def test_conv3x3_c64_bf16_forward_fused_forms_and_backward(ops, N):
    """rp_conv3x3_c64_bf16 (csrc/conv3x3_bf16.hip; resnet.layer1's 3x3 / 64 -> 64 convolutions in the bf16 configuration, src/model.py:131)
    against fp64 F.conv2d on the same bf16 operands: plain; with the producing layer's BatchNorm-apply + ReLU folded into the operand
    load (zero padding must stay zero); with the batch statistics of the stored output from the epilogue; ops.Conv3x3C64Fn's input
    gradient (the same kernel on dY with the rotated, transposed filter) and weight gradient against fp64 autograd.  N = 3 / 37: tile
    runs that end inside an image and workgroups with 0-3 tiles; 256: the configs[4] size (first and last images checked).
    Tolerance 6e-3 of the maximum (a bf16 output, 2^-8 relative, of fp32-accumulated exact products); statistics 1e-6.  The weight
    gradient (rp_conv3x3_c64_wgrad_bf16: output-stationary over the pixel stream, transpose reads, fixed-order partial sums) is a bf16
    output of up to 800 k fp32-accumulated products per element: 6e-3 against fp64 (N <= 37) / 1e-2 against MIOpen's bf16 result (256)."""
    import torch.nn.functional as F
    bf, CL = torch.bfloat16, torch.channels_last
    x = rnd(N, 64, 56, 56, seed=1).to(bf).contiguous(memory_format=CL)
    w = rnd(64, 64, 3, 3, seed=2, scale=(64 * 9) ** -0.5).to(bf).contiguous(memory_format=CL)
    scale, shift = 0.5 + rnd(64, seed=3).abs(), 0.3 * rnd(64, seed=4)
    xn, wn = x.permute(0, 2, 3, 1), w.permute(0, 2, 3, 1)
    sel = sorted(set(list(range(min(N, 3))) + [N - 1]))
    ref = F.conv2d(x[sel].double(), w.double(), None, 1, 1).permute(0, 2, 3, 1)
    y, st = ops.conv3x3_c64_bf16(xn, wn, want_stats=True)
    e = dict(plain=rel(y[sel], ref))
    assert torch.equal(y, ops.conv3x3_c64_bf16(xn, wn))                                   # the statistics do not change the output
    yd = y.double()
    e["sum"], e["sumsq"] = rel(st[:, 0].sum(0), yd.sum((0, 1, 2))), rel(st[:, 1].sum(0), (yd * yd).sum((0, 1, 2)))
    xa = torch.relu(x[sel].float() * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).to(bf)
    ref_bn = F.conv2d(xa.double(), w.double(), None, 1, 1).permute(0, 2, 3, 1)
    e["bn_relu_on_load"] = rel(ops.conv3x3_c64_bf16(xn, wn, scale, shift)[sel], ref_bn)
    # autograd Function: forward, dX, dW
    x1, w1 = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    y1 = ops.Conv3x3C64Fn.apply(x1, w1, False)
    dy = rnd(*y1.shape, seed=5).to(bf).contiguous(memory_format=CL)
    y1.backward(dy)
    x64, w64 = x[sel].double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(x64, w64, None, 1, 1).backward(dy[sel].double())
    e["dx"] = rel(x1.grad[sel], x64.grad)
    if N <= 37:                                           # weight gradient (csrc/conv3x3_wgrad_bf16.hip) against fp64 over ALL images
        xa64, wa64 = x.double(), w.double().requires_grad_(True)
        F.conv2d(xa64, wa64, None, 1, 1).backward(dy.double())
        e["dw"] = rel(w1.grad, wa64.grad)
    else:                                                 # N = 256: against MIOpen's backward-weights on the same operands, and twice
        dw_mi = torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])[1]
        e["dw"] = rel(w1.grad, dw_mi.double())
        assert torch.equal(ops.conv3x3_c64_wgrad_bf16(xn, dy.permute(0, 2, 3, 1)), w1.grad.permute(0, 2, 3, 1))      # deterministic
    report("conv3x3_c64_bf16[N=%d]" % N, **e)
    assert max(e["plain"], e["bn_relu_on_load"], e["dx"]) < 6e-3 and e["dw"] < (6e-3 if N <= 37 else 1e-2) and max(e["sum"], e["sumsq"]) < 1e-6, e
    with pytest.raises(RuntimeError):
        ops.conv3x3_c64_bf16(xn.float(), wn)


@pytest.mark.parametrize("N", [1, 3, 37, 128])
def test_conv3x3_c64_weight_gradient_exact_fp32(ops, N):
    """rp_conv3x3_c64_wgrad_f32 (csrc/conv3x3_wgrad_f32.hip: the weight gradient of resnet.layer1's 3x3 / 64 -> 64 convolutions in the
    exact-fp32 configuration, autograd of src/model.py:131) against fp64 autograd of F.conv2d over ALL images (N <= 37) / against
    MIOpen's fp32 backward-weights (N = 128, the headline size): 3e-6 of the maximum (fp32 accumulation of up to 400 k exact products per
    element, in workgroup partials summed in a fixed order) / 2e-5 between the two fp32 results.  N = 1 / 3 / 37: fewer image rows than
    workgroup slots, runs that start and end inside an image (every edge case of the row ring: first / last row of an image in the
    prologue, in the steady state and at a workgroup boundary).  Deterministic; ops.Conv3x3C64F32Fn (MIOpen forward and input gradient,
    this weight gradient) against plain autograd of the module."""
    import torch.nn.functional as F
    CL = torch.channels_last
    x = rnd(N, 64, 56, 56, seed=1).contiguous(memory_format=CL)
    w = rnd(64, 64, 3, 3, seed=2, scale=(64 * 9) ** -0.5).contiguous(memory_format=CL)
    dy = rnd(N, 64, 56, 56, seed=5).contiguous(memory_format=CL)
    dw = ops.conv3x3_c64_wgrad_f32(x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1))
    assert torch.equal(dw, ops.conv3x3_c64_wgrad_f32(x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)))        # deterministic
    if N <= 37:
        w64 = w.double().requires_grad_(True)
        F.conv2d(x.double(), w64, None, 1, 1).backward(dy.double())
        e = rel(dw.permute(0, 3, 1, 2), w64.grad)
        bound = 3e-6
    else:
        ref = torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])[1]
        e = rel(dw.permute(0, 3, 1, 2), ref.double())
        bound = 2e-5
    x1, w1 = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y1 = ops.Conv3x3C64F32Fn.apply(x1, w1, False, False, None)
    y1.backward(dy)
    x2, w2 = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y2 = F.conv2d(x2, w2, None, 1, 1)
    y2.backward(dy)
    e_fn = dict(y=rel(y1, y2.double()), dx=rel(x1.grad, x2.grad.double()), dw=rel(w1.grad, w2.grad.double()))
    report("conv3x3_c64_wgrad_f32[N=%d]" % N, dw=e, **{"fn_" + k: v for k, v in e_fn.items()})
    # (from ops.CONV3X3_F32_MIN_N images up the Fn's forward and input gradient are csrc/conv3x3_f32.hip, below it MIOpen's)
    own = ops.CONV3X3_F32 and N >= ops.CONV3X3_F32_MIN_N
    assert e < bound and (e_fn["y"] < 2e-6 if own else e_fn["y"] == 0.0) and e_fn["dx"] < 2e-6 and e_fn["dw"] < 2e-5, (e, e_fn)
    assert w1.grad.is_contiguous(memory_format=CL) or w1.grad.shape == w2.grad.shape
    with pytest.raises(RuntimeError):
        ops.conv3x3_c64_wgrad_f32(x.permute(0, 2, 3, 1).to(torch.bfloat16), dy.permute(0, 2, 3, 1))


@pytest.mark.parametrize("N", [1, 3, 37, 128])
def test_conv3x3_c64_forward_and_input_gradient_exact_fp32(ops, N):
    """rp_conv3x3_c64_f32 (csrc/conv3x3_f32.hip: resnet.layer1's 3x3 / 64 -> 64 convolutions in the exact-fp32 configuration,
    src/model.py:131, forward and -- on dY with the rotated, channel-swapped filter -- input gradient) against fp64 F.conv2d / its
    autograd on EVERY output element: 2e-6 of the maximum (576 exact fp32 products per element, fp32 accumulation).  N = 1 / 3 / 37:
    fewer row pairs than workgroup slots and runs that start and end inside an image (first / last rows of an image in the prologue,
    in the steady state and at a workgroup boundary: the zero slot above row 0 and below row 55, the ring wrap); N = 128: the headline
    size, checked in chunks.  Deterministic (no atomics, fixed summation order)."""
    import torch.nn.functional as F
    CL = torch.channels_last
    x = rnd(N, 64, 56, 56, seed=11).contiguous(memory_format=CL)
    w = rnd(64, 64, 3, 3, seed=12, scale=(64 * 9) ** -0.5).contiguous(memory_format=CL)
    dy = rnd(N, 64, 56, 56, seed=15).contiguous(memory_format=CL)
    xr, wr, dyr = x.permute(0, 2, 3, 1), w.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)
    assert xr.is_contiguous() and wr.is_contiguous()
    y = ops.conv3x3_c64_f32(xr, wr)
    assert torch.equal(y, ops.conv3x3_c64_f32(xr, wr))
    dx = ops.conv3x3_c64_f32(dyr, wr, input_gradient=True)
    assert torch.equal(dx, ops.conv3x3_c64_f32(dyr, w.flip(2, 3).permute(1, 2, 3, 0).contiguous()))      # = the forward kernel on the rotated, swapped filter
    e_y = e_dx = 0.0
    w64 = w.double()
    for i in range(0, N, 16):
        xs = x[i:i + 16].double().requires_grad_(True)
        ys = F.conv2d(xs, w64, None, 1, 1)
        ys.backward(dy[i:i + 16].double())
        e_y = max(e_y, float((y[i:i + 16].permute(0, 3, 1, 2).double() - ys).abs().max() / ys.abs().max()))
        e_dx = max(e_dx, float((dx[i:i + 16].permute(0, 3, 1, 2).double() - xs.grad).abs().max() / xs.grad.abs().max()))
    # the epilogue's BatchNorm partials: same y, per-channel sums of y and y^2 over all pixels (fp32 over a tile's 7 pixels per lane,
    # double above that: 2e-7 of sum |y| / sum y^2), and the mean / rstd BnActFn derives from them against the statistics pass
    y2, st = ops.conv3x3_c64_f32(xr, wr, want_stats=True)
    yd = y.double().reshape(-1, 64)
    e_s1 = float(((st[:, 0].sum(0) - yd.sum(0)).abs() / yd.abs().sum(0)).max())
    e_s2 = float(((st[:, 1].sum(0) - yd.square().sum(0)).abs() / yd.square().sum(0)).max())
    # the residual epilogue (y = conv + res: one fp32 add per element, so bit-equal to adding afterwards) and the shared-input form of the
    # autograd node: the identity path's gradient is added by the input-gradient kernel
    rres = rnd(N, 56, 56, 64, seed=16)
    assert torch.equal(ops.conv3x3_c64_f32(dyr, wr, input_gradient=True, res=rres), dx + rres)
    xs_, ws_ = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ys_, _, xalias = ops.Conv3x3C64F32Fn.apply(xs_, ws_, True, True, None)
    ((ys_ * dy).sum() + (xalias * rres.permute(0, 3, 1, 2)).sum()).backward()
    xp_, wp_ = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ((F.conv2d(xp_, wp_, None, 1, 1) * dy).sum() + (xp_ * rres.permute(0, 3, 1, 2)).sum()).backward()
    e_sh = rel(xs_.grad, xp_.grad.double())
    assert e_sh < 3e-6 and rel(ws_.grad, wp_.grad.double()) < 2e-5, e_sh
    report("conv3x3_c64_f32[N=%d]" % N, y=e_y, dx=e_dx, stats_sum=e_s1, stats_sumsq=e_s2, shared_input_dx=e_sh)
    assert e_y < 2e-6 and e_dx < 2e-6, (e_y, e_dx)
    assert torch.equal(y2, y) and st.shape[1:] == (2, 64) and e_s1 < 2e-7 and e_s2 < 2e-7, (e_s1, e_s2)
    with pytest.raises(RuntimeError):
        ops.conv3x3_c64_f32(xr.to(torch.bfloat16), wr)
    with pytest.raises(RuntimeError):
        ops.conv3x3_c64_f32(xr[:, :28].contiguous(), wr)


@pytest.mark.parametrize("N", [1, 3, 37, 128])
@pytest.mark.parametrize("CO", [128, 192])
def test_conv3x3_c128_forward_and_input_gradient_exact_fp32(ops, N, CO):
    """rp_conv3x3_c128_f32 (csrc/conv3x3_c128_f32.hip: resnet.layer2's 3x3 / 128 -> 128 convolutions, src/model.py:132, forward and input
    gradient; extractor_final_conv.conv1 3x3 / 128 -> 192 with bias, src/modules/extractor.py:9,51, forward) against fp64 F.conv2d / its
    autograd on EVERY output element: 2e-6 of the maximum (1152 exact fp32 products per element, fp32 accumulation).  N = 1 / 3 / 37: fewer
    tiles than workgroup slots and chunks that start and end inside an image (zero slot above row 0 and below row 27, the ring wrap, the
    two-barrier refill); N = 128: the headline size, checked in chunks.  Deterministic.  ops.Conv3x3C128F32Fn (own forward / square input
    gradient, MIOpen weight and bias gradients) against plain autograd of F.conv2d."""
    import torch.nn.functional as F
    CL = torch.channels_last
    x = rnd(N, 128, 28, 28, seed=21).contiguous(memory_format=CL)
    w = rnd(CO, 128, 3, 3, seed=22, scale=(128 * 9) ** -0.5).contiguous(memory_format=CL)
    b = rnd(CO, seed=23, scale=0.3) if CO == 192 else None
    dy = rnd(N, CO, 28, 28, seed=25).contiguous(memory_format=CL)
    xr, wr, dyr = x.permute(0, 2, 3, 1), w.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)
    assert xr.is_contiguous() and wr.is_contiguous() and dyr.is_contiguous()
    y = ops.conv3x3_c128_f32(xr, wr, b)
    assert torch.equal(y, ops.conv3x3_c128_f32(xr, wr, b))
    dx = None
    if CO == 128:
        dx = ops.conv3x3_c128_f32(dyr, wr, input_gradient=True)
        assert torch.equal(dx, ops.conv3x3_c128_f32(dyr, w.flip(2, 3).permute(1, 2, 3, 0).contiguous()))      # = the forward kernel on the rotated, swapped filter
    e_y = e_dx = 0.0
    w64 = w.double()
    for i in range(0, N, 16):
        xs = x[i:i + 16].double().requires_grad_(True)
        ys = F.conv2d(xs, w64, None if b is None else b.double(), 1, 1)
        ys.backward(dy[i:i + 16].double())
        e_y = max(e_y, float((y[i:i + 16].permute(0, 3, 1, 2).double() - ys).abs().max() / ys.abs().max()))
        if dx is not None:
            e_dx = max(e_dx, float((dx[i:i + 16].permute(0, 3, 1, 2).double() - xs.grad).abs().max() / xs.grad.abs().max()))
    x1, w1 = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    b1 = None if b is None else b.clone().requires_grad_(True)
    ops.Conv3x3C128F32Fn.apply(x1, w1, b1, False).backward(dy)
    x2, w2 = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    b2 = None if b is None else b.clone().requires_grad_(True)
    F.conv2d(x2, w2, b2, 1, 1).backward(dy)
    e_fn = dict(dx=rel(x1.grad, x2.grad.double()), dw=rel(w1.grad, w2.grad.double()), db=0.0 if b is None else rel(b1.grad, b2.grad.double()))
    y2, st = ops.conv3x3_c128_f32(xr, wr, b, want_stats=True)      # the epilogue's BatchNorm partials (see the 64-channel test)
    yd = y.double().reshape(-1, CO)
    e_s1 = float(((st[:, 0].sum(0) - yd.sum(0)).abs() / yd.abs().sum(0)).max())
    e_s2 = float(((st[:, 1].sum(0) - yd.square().sum(0)).abs() / yd.square().sum(0)).max())
    assert torch.equal(y2, y) and st.shape[1:] == (2, CO) and e_s1 < 2e-7 and e_s2 < 2e-7, (e_s1, e_s2)
    report("conv3x3_c128_f32[N=%d,CO=%d]" % (N, CO), y=e_y, dx=e_dx, stats_sum=e_s1, stats_sumsq=e_s2, **{"fn_" + k: v for k, v in e_fn.items()})
    assert e_y < 2e-6 and e_dx < 2e-6 and e_fn["dx"] < 3e-6 and e_fn["dw"] < 2e-5 and e_fn["db"] < 2e-5, (e_y, e_dx, e_fn)
    with pytest.raises(RuntimeError):
        ops.conv3x3_c128_f32(xr.to(torch.bfloat16), wr)
    with pytest.raises(RuntimeError):
        ops.conv3x3_c128_f32(xr[:, :14].contiguous(), wr)
    if CO == 192:
        with pytest.raises(RuntimeError):
            ops.conv3x3_c128_f32(xr, wr, input_gradient=True)


@pytest.mark.parametrize("C,HW,N", [(64, 56, 3), (64, 56, 37), (64, 56, 128)])
def test_batchnorm_backward_first_pass_in_the_convolution_epilogue(ops, C, HW, N, monkeypatch):
    """a = relu(bn1(x1)); y = conv2(a) (torchvision BasicBlock, src/model.py:131-132) in the exact-fp32 configuration: the hand-written
    input-gradient kernel of conv2 masks its result with bn1's ReLU and forms bn1's backward column sums (sum g, sum g * xhat) in its
    epilogue (RpBnMask), rp_bn_bwd_from_partials runs only the second and third pass.  (1) kernel level: g against dX * [fma(x - mean,
    rstd * gamma, beta) > 0] and the partials against fp64 sums of g and g * xhat (2e-7 of the sums of magnitudes); (2) autograd level:
    ops.bn_act + ops.conv2d with the fusion on against the same chain with it off (rp_bn_bwd's three passes): every gradient within 2e-6
    (same arithmetic, another summation order of the column sums)."""
    import torch.nn as nn
    CL = torch.channels_last
    monkeypatch.setattr(ops, "CONV3X3_F32_MIN_N", 0)
    monkeypatch.setattr(ops, "CONV3X3_WGRAD_F32_MIN_N", 0)
    monkeypatch.setattr(ops, "CONV3X3_C128_F32_MIN_N", 0)
    x1 = rnd(N, C, HW, HW, seed=31).contiguous(memory_format=CL)
    dy = rnd(N, C, HW, HW, seed=32).contiguous(memory_format=CL)
    w = rnd(C, C, 3, 3, seed=33, scale=(C * 9) ** -0.5).contiguous(memory_format=CL)
    gamma, beta = 1 + 0.2 * rnd(C, seed=34), 0.2 * rnd(C, seed=35)
    xr, dyr, wr = x1.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1), w.permute(0, 2, 3, 1)
    x2d = xr.reshape(-1, C)
    mean = x2d.mean(0)
    rstd = (x2d.var(0, unbiased=False) + 1e-5).rsqrt()
    conv = ops.conv3x3_c64_f32
    dx_plain = conv(dyr, wr, input_gradient=True)
    g, part = conv(dyr, wr, input_gradient=True, want_stats=True, bn=(xr, mean, rstd, gamma, beta))
    yv = torch.addcmul(beta, xr - mean, rstd * gamma)                 # (two roundings where the kernel has one fma: the sign can differ next to 0)
    sure = yv.abs() > 1e-5
    assert torch.equal(torch.where(sure, g, 0 * g), torch.where(sure & (yv > 0), dx_plain, 0 * g))
    gd = g.double().reshape(-1, C)
    xh = ((x2d - mean) * rstd).double()
    e1 = float(((part[:, 0].sum(0) - gd.sum(0)).abs() / gd.abs().sum(0)).max())
    e2 = float(((part[:, 1].sum(0) - (gd * xh).sum(0)).abs() / (gd * xh).abs().sum(0)).max())
    assert part.dtype == torch.float64 and part.shape[1:] == (2, C) and e1 < 2e-7 and e2 < 2e-7, (e1, e2)
    # autograd level
    grads = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "CONV_F32_BN_BWD", fused)
        bn = nn.BatchNorm2d(C).cuda().train()
        cv = nn.Conv2d(C, C, 3, 1, 1, bias=False).cuda()
        with torch.no_grad():
            bn.weight.copy_(gamma); bn.bias.copy_(beta); cv.weight.copy_(w)
        cv.weight.data = cv.weight.data.contiguous(memory_format=CL)
        xi = x1.clone().requires_grad_(True)
        a = ops.bn_act(bn, xi)
        assert (getattr(a, "_rp_bn", None) is not None) == fused
        y, _ = ops.conv2d(cv, a, want_stats=True)
        y.backward(dy)
        grads[fused] = (xi.grad, bn.weight.grad, bn.bias.grad, cv.weight.grad)
        assert not ops._BN_PENDING
    errs = [rel(u, v) for u, v in zip(grads[True], grads[False])]
    report("bn_bwd_in_conv_epilogue[C=%d,N=%d]" % (C, N), partial_sum=e1, partial_sum_xhat=e2, dx=errs[0], dgamma=errs[1], dbeta=errs[2], dw=errs[3])
    assert max(errs) < 2e-6, errs


@pytest.mark.parametrize("ci,co,k,pad,h", [(128, 192, 5, 0, 28), (192, 192, 5, 0, 28), (64, 96, 3, 1, 20)])
def test_bf16_convolution_input_gradient_as_forward_convolution(ops, ci, co, k, pad, h):
    """ops.ConvBf16Fn (bf16 configuration, the CNN tail's 5x5 valid convolutions, src/modules/extractor.py:51-65): the input gradient
    computed as a FORWARD convolution of dY with the rotated / transposed filter against fp64 autograd of F.conv2d on the same
    bf16-rounded operands: 1e-2 of the maximum (bf16 output of fp32-accumulated exact products) -- like MIOpen's own backward-data;
    weight and bias gradients (MIOpen's backward-weights) likewise."""
    import torch.nn.functional as F
    bf, CL = torch.bfloat16, torch.channels_last
    x = rnd(6, ci, h, h, seed=1).to(bf).contiguous(memory_format=CL).requires_grad_(True)
    w = rnd(co, ci, k, k, seed=2, scale=(ci * k * k) ** -0.5).to(bf).contiguous(memory_format=CL).requires_grad_(True)
    b = rnd(co, seed=3).to(bf).requires_grad_(True)
    y = ops.ConvBf16Fn.apply(x, w, b, (pad, pad))
    dy = rnd(*y.shape, seed=4).to(bf).contiguous(memory_format=CL)
    y.backward(dy)
    x64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (x, w, b))
    F.conv2d(x64, w64, b64, 1, pad).backward(dy.double())
    e = dict(dx=rel(x.grad, x64.grad), dw=rel(w.grad, w64.grad), db=rel(b.grad, b64.grad))
    report("conv_bf16_bwd_as_fwd[%d->%d,k%d]" % (ci, co, k), **e)
    assert max(e.values()) < 1e-2, e
    x2 = x.detach().clone().requires_grad_(True)
    F.conv2d(x2, w.detach(), b.detach(), 1, pad).backward(dy)             # MIOpen's backward-data on the same operands
    assert rel(x.grad, x2.grad) < 1e-2


@pytest.mark.parametrize("N,hw", [(2, 224), (5, 100), (37, 224)])
def test_stem_convolution_bf16_configuration(ops, N, hw):
    """rp_conv_stem_fwd_bf16 (csrc/conv_stem_bf16.hip; resnet.conv1, src/model.py:127, in the bf16 configuration) against fp64 F.conv2d on
    the bf16-rounded image and filter: 6e-3 of the maximum (bf16 output of fp32-accumulated exact products), batch statistics of the
    stored values 1e-6; ops.StemConvBf16Fn's weight gradient against fp64 autograd: at 224 x 224 the hand-written stream
    (csrc/conv_stem_wgrad_bf16.hip: fp32 output of fp32-accumulated exact bf16 products) 1e-4, else MIOpen's bf16 backward-weights 1e-2;
    the hand-written gradient is deterministic and agrees with MIOpen's."""
    import torch.nn.functional as F
    bf, CL = torch.bfloat16, torch.channels_last
    img = rnd(N, 3, hw, hw, seed=1)
    w = rnd(64, 3, 7, 7, seed=2, scale=147 ** -0.5).contiguous(memory_format=CL).requires_grad_(True)
    xp = torch.zeros(N, hw + 6, hw + 6, 3, device="cuda")
    xp[:, 3:-3, 3:-3] = img.permute(0, 2, 3, 1)
    y, st = ops.StemConvBf16Fn.apply(xp, w, True)
    x64, w64 = img.to(bf).double(), w.detach().to(bf).double().requires_grad_(True)
    ref = F.conv2d(x64, w64, None, 2, 3)
    yd = y.double()
    e = dict(y=rel(y, ref), sum=rel(st[:, 0].sum(0), yd.sum((0, 2, 3))), sumsq=rel(st[:, 1].sum(0), (yd * yd).sum((0, 2, 3))))
    assert y.dtype == bf and y.is_contiguous(memory_format=CL)
    assert torch.equal(y, ops.StemConvBf16Fn.apply(xp, w))
    dy = rnd(*y.shape, seed=3).to(bf).contiguous(memory_format=CL)
    y.backward(dy)
    ref.backward(dy.double())
    e["dw"] = rel(w.grad, w64.grad)
    report("conv_stem_bf16[N=%d,%d]" % (N, hw), **e)
    assert e["y"] < 6e-3 and max(e["sum"], e["sumsq"]) < 1e-6 and e["dw"] < (1e-4 if hw == 224 else 1e-2) and w.grad.dtype == torch.float32, e
    if hw == 224:
        d1 = ops.conv_stem_wgrad_bf16(xp, dy.permute(0, 2, 3, 1))
        assert torch.equal(d1, ops.conv_stem_wgrad_bf16(xp, dy.permute(0, 2, 3, 1))) and torch.equal(d1.permute(0, 3, 1, 2), w.grad)
        mi = torch.ops.aten.convolution_backward(dy, xp.to(bf).permute(0, 3, 1, 2), w.detach().to(bf), None, [2, 2], [0, 0], [1, 1], False, [0, 0], 1,
                                                 [False, True, False])[1]
        assert rel(d1.permute(0, 3, 1, 2), mi.double()) < 1e-2


def test_gemm_errors_are_loud(ops):
    A = rnd(64, 30)
    with pytest.raises(RuntimeError):
        ops.gemm(A, rnd(64, 30), 64, 64, 30)          # K % 4 != 0 -> RP_EALIGN
    with pytest.raises(RuntimeError):
        ops.gemm(torch.zeros(64, 32), torch.zeros(64, 32), 64, 64, 32)      # CPU tensors: no fallback


# ------------------------------------------------------------------------------------------------ rowwise
@pytest.mark.parametrize("M,with_add", [(576 * 4, True), (576 * 4, False), (1000, True)])
def test_gemm_with_fused_layernorm_backward(ops, M, with_add):
    """RpGemm.ln_*: the input-gradient GEMM of the Linear behind a LayerNorm applies the LayerNorm backward in its epilogue
    (reference autograd of vision_transformer.py:352-353).  Against fp64 autograd of  LN(x) @ W^T  and against the unfused
    pair of kernels; M = 1000 leaves a ragged last 64-row tile."""
    N = 576
    x, dy, W = rnd(M, 192, seed=31), rnd(M, N, seed=32), rnd(N, 192, seed=33) * 0.07
    gamma, beta = rnd(192, seed=34) * 0.3 + 1.0, rnd(192, seed=35) * 0.1
    add = rnd(M, 192, seed=36) if with_add else None
    xn, mean, rstd = ops.layernorm_fwd(x, gamma, beta)
    x64 = x.double().requires_grad_(True)
    g64 = gamma.double().requires_grad_(True)
    b64 = beta.double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(x64, (192,), g64, b64, 1e-6) @ W.double().t()
    (y * dy.double()).sum().backward()
    ref_dx = x64.grad + (add.double() if with_add else 0.0)
    keep = ops.FUSE_LN_BWD
    try:
        ops.FUSE_LN_BWD = True
        fused = ops.linear_dx_lnbwd(dy, W, x, gamma, mean, rstd, add=add)
        ops.FUSE_LN_BWD = False
        plain = ops.linear_dx_lnbwd(dy, W, x, gamma, mean, rstd, add=add)
    finally:
        ops.FUSE_LN_BWD = keep
    e = [rel(fused[0], ref_dx), rel(fused[1], g64.grad), rel(fused[2], b64.grad)]
    if with_add:
        e.append(rel(fused[3], add.double().sum(0)))
    report("gemm_lnbwd[M=%d,add=%d]" % (M, with_add), dx=e[0], dgamma=e[1], dbeta=e[2], vs_unfused=rel(fused[0], plain[0]))
    assert max(e) < 5e-6
    assert rel(fused[0], plain[0]) < 2e-6 and rel(fused[1], plain[1]) < 2e-6 and rel(fused[2], plain[2]) < 2e-6
    # the bf16 configuration's operand precision (register-staged kernel, same shared epilogue): fused == unfused to fp32 rounding of
    # the SAME bf16-operand product; against fp64 the bf16 operand rounding shows (stated 2e-2)
    keepp = ops.GEMM_PRECISION
    try:
        ops.set_gemm_precision(1)
        ops.FUSE_LN_BWD = True
        fb = ops.linear_dx_lnbwd(dy, W, x, gamma, mean, rstd, add=add)
        ops.FUSE_LN_BWD = False
        pb = ops.linear_dx_lnbwd(dy, W, x, gamma, mean, rstd, add=add)
    finally:
        ops.set_gemm_precision(keepp)
        ops.FUSE_LN_BWD = keep
    report("gemm_lnbwd_bf16[M=%d,add=%d]" % (M, with_add), dx_vs_unfused=rel(fb[0], pb[0]), dx_vs_fp64=rel(fb[0], ref_dx))
    assert rel(fb[0], pb[0]) < 5e-6 and rel(fb[1], pb[1]) < 5e-5 and rel(fb[2], pb[2]) < 5e-5 and rel(fb[0], ref_dx) < 2e-2


def test_layernorm_fwd_bwd(ops):
    rows, C = 1000, 192
    x, g, b, dy, add = rnd(rows, C, seed=1), rnd(C, seed=2) * 0.2 + 1, rnd(C, seed=3), rnd(rows, C, seed=4), rnd(rows, C, seed=5)
    y, mean, rstd = ops.layernorm_fwd(x, g, b)
    x64 = x.double().requires_grad_(True)
    g64, b64 = g.double().requires_grad_(True), b.double().requires_grad_(True)
    y64 = torch.nn.functional.layer_norm(x64, (C,), g64, b64, 1e-6)
    assert rel(y, y64) < 2e-6
    (y64 * dy.double()).sum().backward()
    dx, dg, db, asum = ops.layernorm_bwd(dy, x, g, mean, rstd, add=add)
    e = max(rel(dx, x64.grad + add.double()), rel(dg, g64.grad), rel(db, b64.grad), rel(asum, add.double().sum(0)))
    report("layernorm", rel=e)
    assert e < 5e-6
    dx0, dg0, db0 = ops.layernorm_bwd(dy, x, g, mean, rstd)          # without a residual-branch operand: 3 results
    assert rel(dx0, x64.grad) < 5e-6 and torch.equal(dg0, dg) and torch.equal(db0, db)


def test_colsum_tokens_posenc_pose(ops, golden):
    t = rnd(5000, 576, seed=1)
    assert rel(ops.colsum(t), t.double().sum(0)) < 2e-6
    assert torch.equal(ops.colsum(t), ops.colsum(t))
    # token layout: bit-exact permutation (pos_embed = 0), then the add
    feat = rnd(4, 192, 24, 24, seed=2)
    pe = rnd(576, 192, seed=3)
    tok = ops.TokensFn.apply(feat, torch.zeros_like(pe))
    assert torch.equal(tok, feat.reshape(4, 192, 576).permute(0, 2, 1).contiguous())
    tok2 = ops.TokensFn.apply(feat, pe)
    assert torch.equal(tok2, feat.reshape(4, 192, 576).permute(0, 2, 1) + pe)
    # channels-last map: the permutation is a view; same values, bit-exact
    fcl = feat.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    tok3 = ops.TokensFn.apply(fcl, pe)
    assert torch.equal(tok3, tok2)
    (tok3 * rnd(4, 576, 192, seed=4)).sum().backward()
    assert torch.equal(fcl.grad, rnd(4, 576, 192, seed=4).permute(0, 2, 1).reshape(4, 192, 24, 24))
    f2 = feat.clone().requires_grad_(True)
    p2 = pe.clone().requires_grad_(True)
    cot = rnd(4, 576, 192, seed=4)
    (ops.TokensFn.apply(f2, p2) * cot).sum().backward()
    assert torch.equal(f2.grad, cot.permute(0, 2, 1).reshape(4, 192, 24, 24))
    assert rel(p2.grad, cot.double().sum(0)) < 1e-6
    # positional features vs the reference's own output (golden) and the no-intrinsics case bit-exact
    intr = torch.tensor([[32.373, 25.898, 12.0, 12.0], [18.0, 21.0, 12.0, 9.0]])[:, None, :].repeat(1, 2, 1).contiguous().cuda()
    pos = ops.posenc(intr, 2, intr.device)
    e = rel(pos, torch.as_tensor(golden["posenc_intr_f32"]))
    report("posenc", rel=e)
    assert e < 3e-7
    assert np.array_equal(ops.posenc(None, 2, intr.device).cpu().numpy(), golden["posenc_none_f32"])
    # pose normalisation fwd/bwd
    from oracle import relpose_oracle as O
    pred = rnd(5, 2, 7, seed=5)
    pred[3, 1, 3:] *= 1e-3                                    # exercises the max(|q|, 0.01) clamp
    gs = rnd(5, 2, 7, seed=6)
    ref = O.normalize_preds(gs.cpu().double(), pred.cpu().double())
    out = torch.empty_like(pred)
    from rel_pose_amd import _lib
    lib = _lib.load()
    _lib.check(lib.rp_pose_normalize_fwd(ops._p(pred), ops._p(gs), ops._p(out), 5, ops._st()), "norm")
    assert rel(out, ref) < 1e-6 and torch.equal(out[:, 0], gs[:, 0])
    p64 = pred.cpu().double().requires_grad_(True)
    cot = rnd(5, 2, 7, seed=7)
    (O.normalize_preds(gs.cpu().double(), p64) * cot.cpu().double()).sum().backward()
    dpred = torch.empty_like(pred)
    _lib.check(lib.rp_pose_normalize_bwd(ops._p(pred), ops._p(cot), ops._p(dpred), 5, ops._st()), "normb")
    assert rel(dpred, p64.grad) < 1e-5


# ------------------------------------------------------------------------------------------------ attention
def _attn_ref(qkv, Z):
    q, k, v = qkv.double().view(Z, 576, 3, 3, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 0.125
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(Z * 576, 192)
    return o, torch.logsumexp(s, -1), s


@pytest.mark.parametrize("waves", [None, "2"])
def test_attention_fwd_bwd(ops, waves, monkeypatch):
    """waves=None: the launcher's choice for 4 images (one-wave workgroups, the small-batch form); "2": the two-wave workgroups every
    full-size batch runs (RP_ATTN_FWD / RP_ATTN_NW are the launchers' tuning overrides)."""
    if waves:
        monkeypatch.setenv("RP_ATTN_FWD", waves + "2")
        monkeypatch.setenv("RP_ATTN_NW", waves)
    Z = 4
    qkv = rnd(Z * 576, 576, seed=1)
    qkv[:, :384] *= 1.7          # sharper softmax
    qkv[5, :64] *= 6.0           # one spiky query row (forces a big online-softmax rescale)
    o, lse = ops.attn_fwd(qkv, Z)
    q64 = qkv.double().requires_grad_(True)
    o_ref, lse_ref, _ = _attn_ref(q64, Z)
    e_o, e_l = rel(o, o_ref), rel(lse, lse_ref)
    report("attn_fwd", o=e_o, lse=e_l)
    assert e_o < 5e-6 and e_l < 2e-6
    do = rnd(Z * 576, 192, seed=2)
    (o_ref * do.double()).sum().backward()
    for store_ds in (True, False):          # dQ from the stored dS via a batched GEMM (default) / from the recompute pass
        keep, ops.ATTN_BWD_STORE_DS = ops.ATTN_BWD_STORE_DS, store_ds
        try:
            dqkv = ops.attn_bwd(qkv, o, lse, do, Z)
        finally:
            ops.ATTN_BWD_STORE_DS = keep
        e = [rel(dqkv[:, i * 192:(i + 1) * 192], q64.grad[:, i * 192:(i + 1) * 192]) for i in range(3)]
        report("attn_bwd[store_ds=%d]" % store_ds, dq=e[0], dk=e[1], dv=e[2])
        assert max(e) < 2e-5
    # the stored-dS kernels can also leave the column sums of dq | dk | dv per 32-row block (the qkv bias gradient's partials)
    d2, part = ops.attn_bwd(qkv, o, lse, do, Z, want_bias_partials=True)
    assert part.shape == (Z * 18, 576) and torch.equal(d2, ops.attn_bwd(qkv, o, lse, do, Z))
    blocks = d2.double().view(Z * 18, 32, 576).sum(1)
    assert rel(part, blocks) < 2e-6 and rel(part.double().sum(0), q64.grad.sum(0)) < 2e-5


@pytest.mark.parametrize("Z", [4, 30])
def test_attention_stored_p_fwd_bwd(ops, Z):
    """Stored-P form (rp_attn_fwd_savep + rp_attn_bwd_dkdv_p + rp_ds_matmul; autograd of vision_transformer.py:325-329): the forward's
    o / lse must be BIT-identical to rp_attn_fwd (same arithmetic, only extra stores), the stored tiles must be the un-normalised
    probabilities in the documented layout, and the gradients must match fp64 autograd like the recompute form's.  Z = 4: one-wave
    workgroups; Z = 30 (810 two-wave workgroups): the form every full-size batch runs."""
    qkv = rnd(Z * 576, 576, seed=1)
    qkv[:, :384] *= 1.7
    qkv[5, :64] *= 6.0           # a spiky query row: its running maximum jumps, the per-tile factor must follow it
    o0, lse0 = ops.attn_fwd(qkv, Z)
    o, lse, pst, mrun = ops.attn_fwd(qkv, Z, save_p=True)
    assert torch.equal(o, o0) and torch.equal(lse, lse0)
    # tile layout: element (query i, key j) of tile (qb, t) at float ((j >> 2) * 32 + i) * 4 + (j & 3)
    q64 = qkv.double().requires_grad_(True)
    o_ref, lse_ref, S = _attn_ref(q64, Z)                                           # S [Z,3,576,576], natural-log units
    Pn = torch.exp(S.detach() - lse_ref.detach().view(Z, 3, 576, 1))
    fac = torch.exp2(mrun.double() - lse.double().view(Z, 3, 1, 576) / math.log(2.0))          # [Z,3,18 tiles,576]
    Pst = pst.view(Z, 3, 18, 18, 8, 32, 4).permute(0, 1, 2, 5, 3, 4, 6).reshape(Z, 3, 576, 576).double()   # [z,h,(qb,i),(t,j>>2,j&3)]
    Pback = Pst * fac.permute(0, 1, 3, 2).repeat_interleave(32, dim=3)
    e_p = rel(Pback, Pn)
    report("attn_fwd_savep[Z=%d]" % Z, p=e_p)
    assert e_p < 5e-6
    do = rnd(Z * 576, 192, seed=2)
    (o_ref * do.double()).sum().backward()
    dqkv, part = ops.attn_bwd(qkv, o, lse, do, Z, want_bias_partials=True, saved_p=(pst, mrun))
    e = [rel(dqkv[:, i * 192:(i + 1) * 192], q64.grad[:, i * 192:(i + 1) * 192]) for i in range(3)]
    report("attn_bwd[stored_p, Z=%d]" % Z, dq=e[0], dk=e[1], dv=e[2])
    assert max(e) < 2e-5
    assert torch.equal(dqkv, ops.attn_bwd(qkv, o, lse, do, Z, saved_p=(pst, mrun)))           # deterministic
    blocks = dqkv.double().view(Z * 18, 32, 576).sum(1)
    assert rel(part, blocks) < 2e-6 and rel(part.double().sum(0), q64.grad.sum(0)) < 2e-5
    ref_form = ops.attn_bwd(qkv, o, lse, do, Z)                                                # recompute form: same gradients to rounding
    assert rel(dqkv, ref_form) < 5e-6
    with pytest.raises(RuntimeError):
        ops.attn_fwd(qkv, Z, k_xor=3, save_p=True)


def test_cross_attention_is_attention_on_partner_keys_values(ops):
    """--noess cross attention (vision_transformer.py:239-262): rp_attn_fwd(k_xor=3) / rp_attn_bwd_cross(kv_xor=1) must be
    BIT-identical to the plain kernels run on a copy whose k|v columns are pair-swapped (same tiles, same order)."""
    Z = 6
    qkv = rnd(Z * 576, 576, seed=21)
    sw = qkv.clone().view(Z, 576, 576)
    sw[:, :, 192:] = ops.pair_swap(qkv.view(Z, 576, 576))[:, :, 192:]
    sw = sw.view(Z * 576, 576).contiguous()
    o_x, lse_x = ops.attn_fwd(qkv, Z, k_xor=3)
    o_s, lse_s = ops.attn_fwd(sw, Z)
    assert torch.equal(o_x, o_s) and torch.equal(lse_x, lse_s)
    do = rnd(Z * 576, 192, seed=22)
    d_x = ops.attn_bwd(qkv, o_x, lse_x, do, Z, kv_xor=1).view(Z, 576, 576)
    keep, ops.ATTN_BWD_STORE_DS = ops.ATTN_BWD_STORE_DS, False          # the recompute-based dQ pass, like the cross kernels
    try:
        d_s = ops.attn_bwd(sw, o_s, lse_s, do, Z).view(Z, 576, 576)
    finally:
        ops.ATTN_BWD_STORE_DS = keep
    assert torch.equal(d_x[:, :, :192], d_s[:, :, :192])                                # dq stays with the query image
    assert torch.equal(d_x[:, :, 192:], ops.pair_swap(d_s)[:, :, 192:])                 # dk, dv land on the partner image
    with pytest.raises(RuntimeError):
        ops.attn_fwd(qkv[:5 * 576].contiguous(), 5, k_xor=3)                            # odd image count has no pairs


def test_attention_stats_partner(ops):
    Z = 4
    qkv = rnd(Z * 576, 576, seed=3)
    rlse, clse = ops.emm_stats(qkv, Z)
    t = qkv.double().view(Z, 576, 3, 3, 64).permute(2, 0, 3, 1, 4)
    q, k = t[0], t[1]
    qp = q[[1, 0, 3, 2]]                                    # partner image's queries
    s = (qp @ k.transpose(-1, -2)) * 0.125                  # S_z[i][j]
    assert rel(rlse, torch.logsumexp(s, -1)) < 2e-6
    assert rel(clse, torch.logsumexp(s, -2)) < 2e-6
    # rp_emm_stats (one pass over S: rows online, columns from per-block partials) against the two stats_only passes it replaces
    keep, ops.EMM_STATS_ONE_PASS = ops.EMM_STATS_ONE_PASS, False
    try:
        r2, c2 = ops.emm_stats(qkv, Z)
    finally:
        ops.EMM_STATS_ONE_PASS = keep
    assert ops.EMM_STATS_ONE_PASS and torch.equal(rlse, r2) and rel(clse, c2) < 1e-6
    qs = qkv.clone()
    qs[:576, :64] *= 40.0                                   # one head of one image with scores of magnitude ~1e3: the per-block maxima matter
    r3, c3 = ops.emm_stats(qs, Z)
    t3 = qs.double().view(Z, 576, 3, 3, 64).permute(2, 0, 3, 1, 4)
    s3 = (t3[0][[1, 0, 3, 2]] @ t3[1].transpose(-1, -2)) * 0.125
    assert rel(r3, torch.logsumexp(s3, -1)) < 2e-6 and rel(c3, torch.logsumexp(s3, -2)) < 2e-6
    with pytest.raises(RuntimeError):
        ops.emm_stats(qkv[:3 * 576].contiguous(), 3)          # odd image count has no pairs


# ------------------------------------------------------------------------------------------------ EMM
def _emm_ref(qkv, pos, Z):
    """fp64 F_z = X^T A X, T = A X, U = A^T X per (z,h)."""
    t = qkv.double().view(Z, 576, 3, 3, 64).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    perm = [z ^ 1 for z in range(Z)]
    s = (q[perm] @ k.transpose(-1, -2)) * 0.125
    a = s.softmax(-1) * s.softmax(-2)
    pe = pos.double()[[z // 2 for z in range(Z)]].unsqueeze(1).expand(Z, 3, 576, 6)
    x = torch.cat([v, pe], dim=-1)
    T = a @ x
    return x.transpose(-1, -2) @ T, T, a.transpose(-1, -2) @ x, x, a


def test_emm_forward_pieces(ops):
    Z = 4
    qkv = rnd(Z * 576, 576, seed=4)
    intr = torch.tensor([[30.0, 26.0, 12.0, 12.0], [18.0, 21.0, 12.0, 9.0]])[:, None, :].repeat(1, 2, 1).contiguous().cuda()
    pos = ops.posenc(intr, Z // 2, qkv.device)
    F_ref, T_ref, U_ref, x_ref, _ = _emm_ref(qkv, pos, Z)
    rlse, clse = ops.emm_stats(qkv, Z)
    xa = ops.emm_build_x(qkv, pos, Z)
    assert torch.equal(xa[..., :70].double(), x_ref.float().double()) and float(xa[..., 70:].abs().max()) == 0.0
    t, fpart = ops.emm_apply(qkv, xa, rlse, clse, Z)
    u, _ = ops.emm_apply(qkv, xa, rlse, clse, Z, swap=True, want_f=False)
    F = fpart.double().sum(2)
    e = dict(T=rel(t[..., :70], T_ref), U=rel(u[..., :70], U_ref), F=rel(F[..., :70, :70], F_ref))
    report("emm_fwd", **e)
    assert max(e.values()) < 1e-5
    assert float(F[..., 70:, :].abs().max()) == 0.0 and float(F[..., :, 70:].abs().max()) == 0.0
    g = ops.emm_finalize(fpart, Z)                     # [Z*70, 224]
    g_ref = F_ref[[z ^ 1 for z in range(Z)]].reshape(Z, 210, 70).transpose(-1, -2)      # vision_transformer.py:229-230,238
    assert rel(g.view(Z, 70, 224)[..., :210], g_ref) < 1e-5
    assert float(g.view(Z, 70, 224)[..., 210:].abs().max()) == 0.0


def test_emm_backward(ops):
    Z = 2
    qkv = rnd(Z * 576, 576, seed=5)
    intr = torch.tensor([[30.0, 26.0, 12.0, 12.0]])[:, None, :].repeat(1, 2, 1).contiguous().cuda()
    pos = ops.posenc(intr, 1, qkv.device)
    dF = torch.zeros(Z, 3, 96, 96, device="cuda")
    dF[..., :70, :70] = rnd(Z, 3, 70, 70, seed=6)
    q64 = qkv.double().requires_grad_(True)
    F_ref, _, _, _, _ = _emm_ref(q64, pos, Z)
    (F_ref * dF[..., :70, :70].double()).sum().backward()
    rlse, clse = ops.emm_stats(qkv, Z)
    xa = ops.emm_build_x(qkv, pos, Z)
    t, _ = ops.emm_apply(qkv, xa, rlse, clse, Z)
    dqkv = ops.emm_backward(qkv, xa, t, rlse, clse, dF, Z)
    e = [rel(dqkv[:, i * 192:(i + 1) * 192], q64.grad[:, i * 192:(i + 1) * 192]) for i in range(3)]
    report("emm_bwd", dq=e[0], dk=e[1], dv=e[2])
    assert max(e) < 5e-5


@pytest.mark.parametrize("Z", [2, 6])
def test_emm_stored_scores(ops, Z):
    """Stored-S form of the EMM (rp_emm_stats(s_out) -> rp_emm_apply / rp_emm_grad_ds(s_in); vision_transformer.py:198-223 and its
    autograd): the stored tiles are the scores in log2 units in the documented layout, the statistics are BIT-identical to the pass that
    does not store, and T, F, U and the gradients agree with fp64 like the recompute form's (same bounds) -- and with the recompute
    form itself to fp32 rounding."""
    qkv = rnd(Z * 576, 576, seed=4)
    intr = torch.tensor([[30.0, 26.0, 12.0, 12.0], [18.0, 21.0, 12.0, 9.0], [25.0, 25.0, 11.0, 13.0]])[:Z // 2, None, :].repeat(1, 2, 1).contiguous().cuda()
    pos = ops.posenc(intr, Z // 2, qkv.device)
    q64 = qkv.double().requires_grad_(True)
    F_ref, T_ref, U_ref, _, _ = _emm_ref(q64, pos, Z)
    rlse, clse, sc = ops.emm_stats(qkv, Z, want_s=True)
    r0, c0 = ops.emm_stats(qkv, Z)
    assert sc is not None and torch.equal(rlse, r0) and torch.equal(clse, c0)
    # S_z[i][j] = scale q_{z^1,i} . k_{z,j}; tile (query block, key tile), element (i, j) at float ((j >> 2) * 32 + i) * 4 + (j & 3)
    q3 = qkv.double().view(Z, 576, 3, 3, 64)
    qp = q3[[z ^ 1 for z in range(Z)], :, 0]                                       # [Z,576,3,64] queries of the partner image
    S = torch.einsum("zihd,zjhd->zhij", qp, q3[:, :, 1]) * 0.125 * math.log2(math.e)
    got = sc.view(Z, 3, 18, 18, 8, 32, 4).permute(0, 1, 2, 5, 3, 4, 6).reshape(Z, 3, 576, 576).double()      # [z,h,(qb,i),(t,j>>2,j&3)]
    assert rel(got, S) < 2e-6
    xa = ops.emm_build_x(qkv, pos, Z)
    t, fpart = ops.emm_apply(qkv, xa, rlse, clse, Z, s=sc)
    u, _ = ops.emm_apply(qkv, xa, rlse, clse, Z, swap=True, want_f=False, s=sc)
    F = fpart.double().sum(2)
    e = dict(T=rel(t[..., :70], T_ref), U=rel(u[..., :70], U_ref), F=rel(F[..., :70, :70], F_ref))
    report("emm_fwd_stored_s[Z=%d]" % Z, **e)
    assert max(e.values()) < 1e-5
    t0, f0 = ops.emm_apply(qkv, xa, rlse, clse, Z)
    u0, _ = ops.emm_apply(qkv, xa, rlse, clse, Z, swap=True, want_f=False)
    assert rel(t, t0) < 2e-6 and rel(u, u0) < 2e-6 and rel(fpart, f0) < 2e-6
    dF = torch.zeros(Z, 3, 96, 96, device="cuda")
    dF[..., :70, :70] = rnd(Z, 3, 70, 70, seed=6)
    (F_ref * dF[..., :70, :70].double()).sum().backward()
    dqkv = ops.emm_backward(qkv, xa, t, rlse, clse, dF, Z, s=sc)
    eb = [rel(dqkv[:, i * 192:(i + 1) * 192], q64.grad[:, i * 192:(i + 1) * 192]) for i in range(3)]
    report("emm_bwd_stored_s[Z=%d]" % Z, dq=eb[0], dk=eb[1], dv=eb[2])
    assert max(eb) < 5e-5
    assert torch.equal(dqkv, ops.emm_backward(qkv, xa, t, rlse, clse, dF, Z, s=sc))          # deterministic
    assert rel(dqkv, ops.emm_backward(qkv, xa, t0, rlse, clse, dF, Z)) < 1e-5


@pytest.mark.parametrize("H,W", [(384, 384), (256, 320), (384, 512), (480, 640)])
def test_preprocess_bit_exact(ops, H, W):
    """channel flip, /255, mean/std, nearest resize to 224 -- bit-exact vs the oracle (which is pinned to
    the reference's F.interpolate index maps)."""
    from oracle import relpose_oracle as O
    imgs = O.synthetic_images(2, H, W, key=31)
    ref = O.preprocess(imgs)                                   # [4,3,224,224] CPU
    got = ops.preprocess(imgs.cuda())
    assert got.shape == (4, 3, 224, 224) and got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got.cpu(), ref)


# ------------------------------------------------------------------------------------------------ CNN front-end BatchNorm
@pytest.mark.parametrize("shape", [(4, 64, 28, 28), (3, 192, 12, 12), (2, 128, 9, 7)])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("with_res,relu", [(False, True), (True, True), (False, False)])
def test_fused_batchnorm_add_relu(ops, shape, training, with_res, relu):
    """ops.bn_act (csrc/batchnorm.hip) against torch.nn.BatchNorm2d (+ add + relu) in fp64: output, input / residual /
    affine gradients and the running-statistics update."""
    N, C, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(C + H)
    x = (torch.randn(N, C, H, W, generator=g) * 1.7 + 0.6)
    res = torch.randn(N, C, H, W, generator=g) if with_res else None
    cot = torch.randn(N, C, H, W, generator=g)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    ref_bn = torch.nn.BatchNorm2d(C).double()
    ref_bn.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in bn.state_dict().items()})
    bn = bn.cuda().train(training)
    ref_bn.train(training)
    xr = x.double().requires_grad_(True)
    rr = None if res is None else res.double().requires_grad_(True)
    yr = ref_bn(xr)
    if rr is not None:
        yr = yr + rr
    if relu:
        yr = yr.relu()
    (yr * cot.double()).sum().backward()
    xg = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    rg = None if res is None else res.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.bn_act(bn, xg, residual=rg, relu=relu)
    assert y.is_contiguous(memory_format=torch.channels_last)
    (y * cot.cuda()).sum().backward()
    errs = dict(y=rel(y, yr), dx=rel(xg.grad, xr.grad), dgamma=rel(bn.weight.grad, ref_bn.weight.grad),
                dbeta=rel(bn.bias.grad, ref_bn.bias.grad), rmean=rel(bn.running_mean, ref_bn.running_mean),
                rvar=rel(bn.running_var, ref_bn.running_var))
    if rg is not None:
        errs["dres"] = rel(rg.grad, rr.grad)
    report("bn_act[%s|train=%d|res=%d|relu=%d]" % ("x".join(map(str, shape)), training, with_res, relu), **errs)
    assert max(errs.values()) < 5e-6
    assert int(bn.num_batches_tracked) == (1 if training else 0)


@pytest.mark.parametrize("with_res,relu", [(False, True), (True, True), (True, False)])
def test_fused_batchnorm_bf16_storage(ops, with_res, relu):
    """The bf16 storage mode of csrc/batchnorm.hip (the bf16 configuration keeps the tensors between MIOpen's bf16 convolutions in
    bf16): same kernels, activations widened exactly on load and rounded to nearest-even on store, statistics / arithmetic fp32.
    Against fp64 torch.nn.BatchNorm2d ON THE SAME bf16-rounded inputs: outputs and input gradients agree to bf16 rounding (<= 2^-8
    of the tensor maximum: one rounding on store), the parameter gradients and running statistics -- fp32 outputs of fp32 sums -- to
    1e-5 (training mode; the ReLU mask is taken from the bf16-rounded stored y when a residual was added, like the fp32 path does from
    its y); also the fused stem chain bn -> relu -> maxpool(3,2,1)."""
    N, C, H, W = 6, 64, 28, 28
    bf = torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(11)
    x = (torch.randn(N, C, H, W, generator=g) * 1.7 + 0.6).to(bf)
    res = torch.randn(N, C, H, W, generator=g).to(bf) if with_res else None
    cot = torch.randn(N, C, H, W, generator=g).to(bf)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
    ref_bn = torch.nn.BatchNorm2d(C).double()
    ref_bn.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in bn.state_dict().items()})
    bn = bn.cuda().train()
    xr = x.double().requires_grad_(True)
    rr = None if res is None else res.double().requires_grad_(True)
    yr = ref_bn(xr)
    if rr is not None:
        yr = yr + rr
    if relu:
        yr = yr.relu()
    (yr * cot.double()).sum().backward()
    xg = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    rg = None if res is None else res.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.bn_act(bn, xg, residual=rg, relu=relu)
    assert y.dtype == bf and y.is_contiguous(memory_format=torch.channels_last)
    (y.float() * cot.cuda().float()).sum().backward()
    assert xg.grad.dtype == bf
    errs = dict(y=rel(y.float(), yr), dx=rel(xg.grad.float(), xr.grad), dgamma=rel(bn.weight.grad, ref_bn.weight.grad),
                dbeta=rel(bn.bias.grad, ref_bn.bias.grad), rmean=rel(bn.running_mean, ref_bn.running_mean),
                rvar=rel(bn.running_var, ref_bn.running_var))
    if rg is not None:
        errs["dres"] = rel(rg.grad.float(), rr.grad)
    report("bn_act_bf16[res=%d|relu=%d]" % (with_res, relu), **errs)
    assert max(errs["y"], errs["dx"], errs.get("dres", 0.0)) < 2.0 ** -8
    # dgamma / dbeta sum the MASKED cotangent: a y within bf16 rounding of 0 may take the other side of the ReLU than the fp64 value
    assert max(errs["dgamma"], errs["dbeta"]) < (2e-3 if relu else 1e-5) and max(errs["rmean"], errs["rvar"]) < 1e-5
    if with_res or not relu:
        return
    # fused stem chain bn -> relu -> maxpool in bf16 storage.  Forward: the same pooled values as the separate bf16 kernels, bit for bit
    # (max of rounded values = rounded max).  Backward: the fused kernel takes the arg-max on the fp32 values BEFORE rounding -- like the
    # fp64 reference chain -- while the separate path pools the bf16-rounded tensor, where values within one bf16 ulp tie and the first in
    # scan order wins: gradients are routed to a different pixel of the window there (both are valid roundings of the same chain), so
    # the fused backward is checked against fp64 autograd and the separate path only for how rarely it disagrees.
    pool = torch.nn.MaxPool2d(3, 2, 1)
    bn2 = torch.nn.BatchNorm2d(C).cuda().train()
    bn2.load_state_dict(ref_bn.state_dict())
    bn3 = torch.nn.BatchNorm2d(C).cuda().train()
    bn3.load_state_dict(ref_bn.state_dict())
    ref2 = torch.nn.BatchNorm2d(C).double()
    ref2.load_state_dict(ref_bn.state_dict())
    x1 = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    x2 = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    keep = ops.FUSE_STEM_POOL
    try:
        ops.FUSE_STEM_POOL = True
        ya = ops.bn_relu_maxpool(bn2, pool, x1)
        ops.FUSE_STEM_POOL = False
        yb = ops.bn_relu_maxpool(bn3, pool, x2)
    finally:
        ops.FUSE_STEM_POOL = keep
    assert ya.dtype == bf and torch.equal(ya, yb)
    c2 = torch.randn(ya.shape, generator=g).to(bf)
    (ya.float() * c2.cuda().float()).sum().backward()
    (yb.float() * c2.cuda().float()).sum().backward()
    xr2 = x.double().requires_grad_(True)
    yr2 = pool(ref2(xr2).relu())
    (yr2 * c2.double()).sum().backward()
    e_y, e_dx, e_dg = rel(ya.float(), yr2), rel(x1.grad.float(), xr2.grad), rel(bn2.weight.grad, ref2.weight.grad)
    differ = float(((x1.grad.float() - x2.grad.float()).abs() > 1e-3 * float(x1.grad.float().abs().max())).float().mean())
    report("bn_pool_bf16", y=e_y, dx=e_dx, dgamma=e_dg, separate_path_routes_differently=differ)
    assert e_y < 2.0 ** -8 and e_dx < 2.0 ** -7 and e_dg < 1e-4 and differ < 0.02


def test_fused_geodesic_loss_matches_se3_autograd(ops):
    """csrc/se3loss.hip against the PyTorch SE(3) formulation (rel_pose_amd/se3.py) in fp64, value and gradient, including an
    exact-identity relative pose (zero rotation / translation branches) and a rotation beyond 90 degrees (w < 0 branch)."""
    from rel_pose_amd.losses import geodesic_loss_tensors, geodesic_loss_tensors_torch
    from rel_pose_amd.se3 import SE3
    g = torch.Generator(device="cpu").manual_seed(3)
    B = 37

    def poses(scale):
        q = torch.randn(B, 2, 4, generator=g)
        q = q / q.norm(dim=-1, keepdim=True)
        return torch.cat([torch.randn(B, 2, 3, generator=g) * scale, q], -1)
    Ps, Gs = poses(1.0), poses(0.7)
    Ps[:, 0] = torch.tensor([0, 0, 0, 0, 0, 0, 1.0])
    Gs[:, 0] = torch.tensor([0, 0, 0, 0, 0, 0, 1.0])
    Gs[0, 1] = Ps[0, 1]                                     # prediction == ground truth: d = identity
    Gs[1, 1, 3:] = -Gs[1, 1, 3:]                            # same rotation, opposite quaternion sign
    Gs[2, 1, 3:] = torch.tensor([0.0, 0.0, 0.96, -0.28])    # w < 0
    Gr = Gs.double().requires_grad_(True)
    ltr_r, lrot_r = geodesic_loss_tensors_torch(SE3(Ps.double()), [SE3(Gr)])
    (10.0 * ltr_r + 7.0 * lrot_r).backward()
    Gg = Gs.cuda().requires_grad_(True)
    ltr, lrot = geodesic_loss_tensors(SE3(Ps.cuda()), [SE3(Gg)])
    (10.0 * ltr + 7.0 * lrot).backward()
    # pair 0 sits ON the singularity of |tau|, |phi| (d = identity): its gradient is the unit direction of rounding noise in
    # either implementation -- only required to be finite and bounded like a subgradient; everything else must match
    e = dict(tr=rel(ltr, ltr_r), rot=rel(lrot, lrot_r), grad=rel(Gg.grad[1:], Gr.grad[1:]))
    report("geodesic_loss", **e)
    assert torch.isfinite(Gg.grad).all() and float(Gg.grad[0].abs().max()) < 17.0 / (2 * B) * 4
    assert e["tr"] < 2e-6 and e["rot"] < 2e-6 and e["grad"] < 2e-5


@pytest.mark.parametrize("shape", [(3, 64, 20, 28), (2, 8, 7, 9), (1, 4, 1, 2)])
def test_maxpool3x3s2_matches_torch_including_ties(ops, shape):
    """values, and gradient routing with many exact ties (post-ReLU zeros), bit-identical to torch.nn.MaxPool2d(3, 2, 1)"""
    N, C, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(H * W)
    x = torch.relu(torch.randn(N, C, H, W, generator=g)).round(decimals=1)         # zeros and repeated values
    pool = torch.nn.MaxPool2d(3, 2, 1)
    xr = x.clone().requires_grad_(True)
    yr = pool(xr)
    cot = torch.randn(yr.shape, generator=g)
    (yr * cot).sum().backward()
    xg = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.maxpool3x3s2(pool, xg)
    (y * cot.cuda()).sum().backward()
    assert y.shape == yr.shape and torch.equal(y.cpu(), yr)
    assert torch.equal(xg.grad.cpu(), xr.grad)


def test_fused_batchnorm_statistics_are_cancellation_safe(ops):
    """|mean| >> std (1000 vs 0.01): the column statistics are accumulated about a pivot row, so E[d^2] - E[d]^2 keeps the
    variance; a plain fp32 E[x^2] - mean^2 would return noise here"""
    g = torch.Generator(device="cpu").manual_seed(9)
    x = (1000.0 + 0.01 * torch.randn(16, 64, 24, 24, generator=g))
    bn = torch.nn.BatchNorm2d(64).cuda().train()
    y = ops.bn_act(bn, x.cuda().contiguous(memory_format=torch.channels_last), relu=False)
    xd = x.double()
    ref = (xd - xd.mean((0, 2, 3), keepdim=True)) / torch.sqrt(xd.var((0, 2, 3), unbiased=False, keepdim=True) + 1e-5)
    # x itself only carries ~6e-5 of absolute resolution at 1000, i.e. ~6e-3 of a 0.01 standard deviation
    assert float((y.cpu().double() - ref).abs().max()) < 2e-2
    assert rel(bn.running_var, 0.9 + 0.1 * xd.var((0, 2, 3), unbiased=True)) < 1e-6


def test_unsupported_intrinsics_fail_loudly_without_a_sync(ops):
    """The reference asserts that both images of a pair share their intrinsics (vision_transformer.py:117) and traps when the
    first pair's principal point lies on an axis (:124-126).  Here the check runs inside rp_posenc (no host sync): an offending
    pair's positional encodings are NaN -- which poisons its pose and the batch loss -- while well-formed pairs are untouched."""
    good = torch.tensor([[30.0, 26.0, 12.0, 11.0]]).repeat(3, 2, 1).contiguous().cuda()
    ref = ops.posenc(good, 3, good.device)
    assert torch.isfinite(ref).all()
    bad = good.clone()
    bad[1, 1, 0] = 31.0                                       # pair 1: fx differs between its two images
    pos = ops.posenc(bad, 3, bad.device)
    assert torch.isnan(pos[1, :, 3:5]).all() and torch.equal(pos[0], ref[0]) and torch.equal(pos[2], ref[2])
    origin = good.clone()
    origin[0, :, 2] = 0.0                                     # first pair's cx = 0: the reference drops into pdb for the whole batch
    assert torch.isnan(ops.posenc(origin, 3, origin.device)[..., 3:5]).all()


def test_ds_matmul_bf16_tiles(ops):
    """rp_ds_matmul(ds_bf16 = 1): the stored-dS product of the bf16 configuration (bf16 tiles in the producer's accumulator image,
    v_mfma_f32_32x32x16_bf16, b rounded to bf16 on chip).  With bf16-representable ds AND b every product is exact: fp32-accumulation
    accuracy (3e-6 of the maximum) against fp64 on the de-tiled array, for b of the same image and of the partner image; with a
    general b the stated bf16 tolerance (2e-2); and the fp32-tile launch on the same values agrees."""
    Z = 4
    bf = torch.bfloat16
    tiles = rnd(Z, 3, 576, 576, seed=51).to(bf)                       # the TILED array as a producer would write it
    r_ = torch.arange(16, device="cuda")[:, None]
    l_ = torch.arange(64, device="cuda")[None, :]
    ii = ((r_ & 3) + 8 * (r_ >> 2) + 4 * (l_ >> 5)).reshape(-1)
    jj = (l_ & 31).expand(16, 64).reshape(-1)
    dense = torch.empty(Z, 3, 18, 18, 32, 32, device="cuda", dtype=torch.float64)
    dense[:, :, :, :, ii, jj] = tiles.view(Z, 3, 18, 18, 1024).double()
    dense = dense.permute(0, 1, 2, 4, 3, 5).reshape(Z, 3, 576, 576)
    e = {}
    for name, b in (("exact_operands", rnd(Z * 576, 576, seed=52).to(bf).float()), ("general_b", rnd(Z * 576, 576, seed=53))):
        for b_xor in (0, 1):
            out = torch.zeros(Z * 576, 576, device="cuda")
            ops.ds_matmul(tiles, b.data_ptr() + 4 * 192, 576, out.data_ptr(), 576, Z, b_xor=b_xor)
            bz = b.view(Z, 576, 576)[:, :, 192:384]
            if b_xor:
                bz = bz.view(Z // 2, 2, 576, 192).flip(1).reshape(Z, 576, 192)
            ref = torch.matmul(dense, bz.reshape(Z, 576, 3, 64).permute(0, 2, 1, 3).double()).permute(0, 2, 1, 3).reshape(Z * 576, 192)
            e["%s_xor%d" % (name, b_xor)] = rel(out[:, :192], ref)
            assert float(out[:, 192:].abs().max()) == 0.0             # only the addressed column block is written
            if name == "exact_operands" and not b_xor:
                out32 = torch.zeros_like(out)
                ops.ds_matmul(tiles.float(), b.data_ptr() + 4 * 192, 576, out32.data_ptr(), 576, Z)
                e["vs_fp32_tiles"] = rel(out[:, :192], out32[:, :192])
    report("ds_matmul_bf16", **e)
    assert max(e["exact_operands_xor0"], e["exact_operands_xor1"], e["vs_fp32_tiles"]) < 3e-6, e
    assert max(e["general_b_xor0"], e["general_b_xor1"]) < 2e-2, e


# ------------------------------------------------------------------------------------------------ configs[4]: bf16 MFMA mode
def test_attention_and_emm_bf16_operand_mode(ops):
    """BASELINE.json configs[4] ("bf16 with MFMA bf16 attention GEMMs"): the `bf16` argument of rp_attn_* / rp_emm_* moves the
    QK^T / PV / dS contractions to v_mfma_f32_32x32x16_bf16 (operands rounded to bf16, fp32 accumulate and softmax state).
    Stated tolerance against the fp64 reference: 2e-2 of max|ref| forward, 4e-2 backward (bf16 carries 8 significant bits:
    2^-9 per operand, ~1e-2 after the 64-term dot products and the exp; 6e-2 for the EMM, whose exponent is 2 S); the fp32 mode on the same inputs stays < 2e-5, and
    the flag is process state that is switched back."""
    Z = 4
    qkv = rnd(Z * 576, 576, seed=1)
    qkv[:, :384] *= 1.7
    do = rnd(Z * 576, 192, seed=2)
    q64 = qkv.double().requires_grad_(True)
    o_ref, lse_ref, _ = _attn_ref(q64, Z)
    (o_ref * do.double()).sum().backward()
    pos = rnd(Z // 2, 576, 6, seed=4)
    try:
        ops.set_attention_precision(1)
        o, lse = ops.attn_fwd(qkv, Z)
        e_o, e_l = rel(o, o_ref), rel(lse, lse_ref)
        errs = {}
        for store_ds in (True, False):
            keep, ops.ATTN_BWD_STORE_DS = ops.ATTN_BWD_STORE_DS, store_ds
            try:
                dqkv = ops.attn_bwd(qkv, o, lse, do, Z)
            finally:
                ops.ATTN_BWD_STORE_DS = keep
            errs[store_ds] = max(rel(dqkv[:, i * 192:(i + 1) * 192], q64.grad[:, i * 192:(i + 1) * 192]) for i in range(3))
        x = ops.emm_build_x(qkv, pos, Z)
        rl, cl = ops.emm_stats(qkv, Z)
        t, fpart = ops.emm_apply(qkv, x, rl, cl, Z)
    finally:
        ops.set_attention_precision(0)
    report("attn_bf16", o=e_o, lse=e_l, bwd_ds=errs[True], bwd_recompute=errs[False])
    assert 1e-5 < e_o < 2e-2 and e_l < 2e-2
    assert max(errs.values()) < 4e-2
    # EMM forward pieces against the fp32 kernels (themselves pinned to fp64 at 2e-6 by test_emm_forward_pieces)
    t32, f32 = ops.emm_apply(qkv, x, rl, cl, Z)
    e_t, e_f = rel(t, t32), rel(fpart.sum(2), f32.sum(2))
    report("emm_bf16", T=e_t, F=e_f)
    assert 1e-6 < e_t < 6e-2 and e_f < 6e-2            # the dual softmax exponent is 2 S: twice the score error of plain attention
    o32, _ = ops.attn_fwd(qkv, Z)
    assert rel(o32, o_ref) < 5e-6                       # back on the exact path


# ------------------------------------------------------------------------------------------------ a16: 3x3 SVD auxiliary
def test_svd3x3_and_essential_matrix_vs_lapack(ops):
    """SURVEY row a16 / north_star: one-wavefront Jacobi 3x3 SVD, off the model's output path, pinned against LAPACK.
    E = [t]x R(q) -> SVD round trip: singular values (s, s, 0) and equal to numpy.linalg.svd's (fp64), U S V^T = E,
    U and V orthogonal; plus generic, rank-1 and zero matrices."""
    from oracle import svd3x3_oracle as SO
    from rel_pose_amd import geom
    g = torch.Generator().manual_seed(3)
    n = 1000                                               # not a multiple of 64: ragged last wavefront
    pose = torch.randn(n, 7, generator=g)
    pose[:, 3:] = pose[:, 3:] / pose[:, 3:].norm(dim=1, keepdim=True)
    E = geom.essential_from_pose(pose.cuda())
    E_ref = SO.essential_from_pose(pose.numpy())
    assert rel(E, torch.from_numpy(E_ref)) < 2e-6
    generic = torch.randn(n, 3, 3, generator=g)
    rank1 = torch.randn(n, 3, 1, generator=g) @ torch.randn(n, 1, 3, generator=g)
    zero = torch.zeros(4, 3, 3)
    worst = {}
    for tag, A in (("essential", E.cpu()), ("generic", generic), ("rank1", rank1), ("zero", zero)):
        U, S, V = geom.svd3x3(A.cuda())
        U, S, V = U.cpu().double(), S.cpu().double(), V.cpu().double()
        s_ref = torch.from_numpy(SO.singular_values(A.numpy()))
        scale = s_ref[:, :1].clamp_min(1e-30)
        e_s = float(((S - s_ref).abs() / scale).max()) if tag != "zero" else float(S.abs().max())
        rec = U @ torch.diag_embed(S) @ V.transpose(-1, -2)
        e_rec = float(((rec - A.double()).abs().amax((1, 2)) / scale[:, 0]).max()) if tag != "zero" else float(rec.abs().max())
        eye = torch.eye(3, dtype=torch.float64)
        e_orth = max(float((U.transpose(-1, -2) @ U - eye).abs().max()), float((V.transpose(-1, -2) @ V - eye).abs().max()))
        assert bool((S[:, 0] >= S[:, 1]).all() and (S[:, 1] >= S[:, 2]).all() and (S >= 0).all())
        worst[tag] = max(e_s, e_rec, e_orth)
        assert e_s < 3e-6 and e_rec < 3e-6 and e_orth < 3e-6, (tag, e_s, e_rec, e_orth)
    U, S, V = geom.svd3x3(E)
    assert float(((S[:, 0] - S[:, 1]).abs() / S[:, 0]).max()) < 3e-6 and float((S[:, 2] / S[:, 0]).max()) < 3e-6   # (s, s, 0)
    report("svd3x3", **worst)


def test_pose_from_essential_round_trip(ops):
    """north_star's "per-pair 3x3 SVD ... produce relative R,t" closed as a round trip (no reference row: SURVEY a16, off
    ViTEss.forward's path): pose -> E = [t]x R(q) (rp_essential_from_pose) -> SVD + four candidates + cheirality on synthetic points
    (rp_pose_from_essential) -> the input pose again: rotation angle error <= 2e-3 rad (fp32 SVD of a rank-2 matrix: sqrt(eps)-level
    sensitivity near 180-degree / degenerate configurations, measured ~1e-4), t direction cosine >= 1 - 1e-6 (t is recovered up to
    scale, sign fixed by the points), every synthetic point in front of both cameras; and the same decisions as the LAPACK oracle."""
    from oracle import svd3x3_oracle as SO
    from rel_pose_amd import geom
    g = torch.Generator().manual_seed(17)
    n, P = 300, 12
    pose = torch.zeros(n, 7)
    pose[:, :3] = torch.randn(n, 3, generator=g)
    ax = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    half = (torch.rand(n, 1, generator=g) * 2.0 - 1.0)            # rotation angle within +-2 rad: the two cameras never face away from
    pose[:, 3:6], pose[:, 6:] = ax * torch.sin(half), torch.cos(half)          # each other, so points in front of both always exist
    R = torch.from_numpy(SO.rotation_from_quat(pose[:, 3:].numpy()))
    t = pose[:, :3].double()
    # 3-D points in front of camera 1 whose images in camera 2 are in front as well (rejection sampling, deterministic)
    X1 = torch.empty(n, P, 3, dtype=torch.float64)
    for i in range(n):
        got, tries = 0, 0
        while got < P:
            tries += 1
            assert tries < 500, "rejection sampling of points in front of both cameras does not terminate"
            cand = torch.cat([torch.randn(64, 2, generator=g, dtype=torch.float64) * 2.0, torch.rand(64, 1, generator=g, dtype=torch.float64) * 6.0 + 1.0], 1)
            z2 = (cand @ R[i].T + t[i])[:, 2]
            ok = cand[z2 > 0.5]
            k = min(P - got, ok.shape[0])
            X1[i, got:got + k] = ok[:k]
            got += k
    X2 = torch.einsum("nij,npj->npi", R, X1) + t[:, None, :]
    x1 = (X1[..., :2] / X1[..., 2:]).float()
    x2 = (X2[..., :2] / X2[..., 2:]).float()
    E = geom.essential_from_pose(pose.cuda())
    out, count = geom.pose_from_essential(E, x1.cuda(), x2.cuda())
    out, count = out.cpu().double(), count.cpu()
    assert bool((count == P).all()), count.min()
    tn = t / t.norm(dim=1, keepdim=True)
    cos_t = (out[:, :3] * tn).sum(1)
    qd = (out[:, 3:] * pose[:, 3:].double()).sum(1).abs().clamp(max=1.0)
    ang = 2.0 * torch.acos(qd)
    report("pose_from_essential", max_angle=float(ang.max()), min_cos_t=float(cos_t.min()))
    assert float(ang.max()) < 2e-3 and float(cos_t.min()) > 1.0 - 1e-6
    assert float((out[:, :3].norm(dim=1) - 1).abs().max()) < 1e-5 and bool((out[:, 6] >= 0).all())
    # the LAPACK oracle takes the same decisions on the same E and points
    Ro, to, co = SO.decode_essential(E.cpu().numpy()[:40], x1.numpy()[:40], x2.numpy()[:40])
    Rg = torch.from_numpy(SO.rotation_from_quat(out[:40, 3:].numpy()))
    assert float((Rg - torch.from_numpy(Ro)).abs().max()) < 5e-4 and float((out[:40, :3] - torch.from_numpy(to)).abs().max()) < 5e-4
    assert bool((torch.from_numpy(co) == P).all())


def test_batched_column_sums_equal_individual_ones(ops):
    """rp_colsum_multi: several column sums in one pair of launches give bit-identical results to rp_colsum one by one
    (same stage split, same summation order), incl. a single-stage task, a ragged column count and more than 8 tasks."""
    shapes = [(73728, 576), (1152, 768), (1152, 576), (300, 14), (64, 192), (5000, 100), (1152, 384), (2, 512), (9000, 64), (1, 8)]
    ins = [rnd(r, c, seed=100 + i) for i, (r, c) in enumerate(shapes)]
    ref = [ops.colsum(t) for t in ins]
    with ops.colsum_batch():
        got = [ops.colsum(t) for t in ins]
    for a, b, t in zip(got, ref, ins):
        assert torch.equal(a, b)
        assert rel(a, t.double().sum(0)) < 1e-5


def test_fused_augmentation_is_pils_arithmetic_bit_for_bit(ops):
    """rp_augment_pairs (uint8 BGR pairs -> jittered, resized fp32 model input) against RGBDAugmentor.apply + F.interpolate -- the
    tensor statement of the reference's ToPILImage / ColorJitter / RandomGrayscale / ToTensor / nearest-resize chain
    (src/data_readers/augmentation.py:7-37), which tests/test_data_eval_cpu.py shows equal to Pillow's 8-bit arithmetic on all 2^24
    colours and to the reference's own reader -- with the SAME parameter rows: every op order, grey on and off, skipped ops, the
    corners of the parameter box, flat and saturated regions.  Integer arithmetic: EXACT equality."""
    import itertools
    import torch.nn.functional as F
    from rel_pose_amd.data_readers.augmentation import RGBDAugmentor
    g = torch.Generator().manual_seed(5)
    aug = RGBDAugmentor(reshape_size=[96, 128], generator=g)
    perms = list(itertools.permutations(range(4)))
    B, H, W = len(perms) + 4, 120, 160
    img = torch.randint(0, 256, (B, 2, H, W, 3), generator=g, dtype=torch.uint8)
    img[3, :, :, :40] = img[3, :, :, :1, :1]                      # flat regions: max == min (hue of a grey pixel), saturated colours
    img[4, 0] = 255
    img[4, 1] = 0
    prm = aug.draw_batch(B)
    prm[:len(perms), :4] = torch.tensor(perms, dtype=torch.float32)
    prm[:, 8] = (torch.arange(B) % 5 == 0).float()
    prm[-1] = RGBDAugmentor(reshape_size=[96, 128], jitter=False).draw_batch(1)[0]      # jitter off: the resized input exactly
    prm[-2, 4:8] = torch.tensor([1.25, 0.75, 1.25, 0.4 / 3.14])  # corners of the parameter box
    prm[-3, 4:8] = torch.tensor([0.75, 1.25, 0.75, -0.4 / 3.14])
    prm[-4, :4] = torch.tensor([2.0, -1.0, 3.0, -1.0])           # two ops skipped
    intr = torch.tensor([[517.97, 517.97, 320.0, 240.0]]).repeat(B, 2, 1).cuda()
    out, intr2 = aug.augment_batch_hip(img.cuda(), intr, params=prm)
    assert out.shape == (B, 2, 3, 96, 128) and out.dtype == torch.float32
    assert torch.allclose(intr2[0, 0].cpu(), torch.tensor([517.97 * 128 / 160, 517.97 * 96 / 120, 320.0 * 128 / 160, 240.0 * 96 / 120]))
    for b in range(B):
        x = img[b].permute(0, 3, 1, 2).float()
        ref = F.interpolate(RGBDAugmentor.apply(x, RGBDAugmentor.params_to_dict(prm[b])), size=[96, 128])
        assert torch.equal(out[b].cpu(), ref), b
        assert torch.equal(F.interpolate(RGBDAugmentor.apply(x.cuda(), RGBDAugmentor.params_to_dict(prm[b])), size=[96, 128]).cpu(), ref), b
    assert torch.equal(out[-1].cpu(), F.interpolate(img[-1].permute(0, 3, 1, 2).float(), size=[96, 128]))
    assert torch.equal(out, out.round()) and float(out.min()) >= 0 and float(out.max()) <= 255
    with pytest.raises(ValueError):
        ops.augment_pairs(img.float().cuda(), prm.cuda(), 96, 128)


def test_gpu_input_path_reproduces_the_references_reader(ops, tmp_path):
    """SURVEY 8f row 3 on the device: decode-only readers (raw=True) + rp_augment_pairs against what the REFERENCE's own readers
    produced on the same fake datasets (tests/golden/reference_readers.npz; src/data_readers/base.py:45-97, augmentation.py:19-37):
    with the jitter off and with each fixed ColorJitter / RandomGrayscale draw the image tensor is identical to the last bit, and so
    are the poses and the rescaled intrinsics."""
    import hashlib
    from rel_pose_amd.data_readers.augmentation import RGBDAugmentor
    from rel_pose_amd.data_readers.interiornet import InteriorNet
    from rel_pose_amd.data_readers.matterport import Matterport
    from tests import _eval_cases as EC
    ref = np.load(os.path.join(ROOT, "tests", "golden", "reference_readers.npz"))
    mroot, proot = str(tmp_path / "matterport_fake"), str(tmp_path / "pano_fake")
    EC.write_matterport_train(mroot)
    EC.write_panorama_train(proot, "interiornet", "")

    def check(prefix, db, idx, size, prm_row):
        images, poses, intr = db[idx]                                   # uint8 [2,H,W,3] BGR as decoded, unscaled intrinsics
        aug = RGBDAugmentor(reshape_size=size)
        out, k = aug.augment_batch_hip(images[None].cuda(), intr[None].clone().cuda(), params=prm_row[None])
        a = out[0].cpu().contiguous().numpy()
        assert hashlib.sha256(a.tobytes()).hexdigest() == str(ref[prefix + "_images_sha256"]), prefix
        assert np.array_equal(poses.numpy(), ref[prefix + "_poses"]) and np.array_equal(k[0].cpu().numpy(), ref[prefix + "_intrinsics"]), prefix

    off = RGBDAugmentor([8, 8], jitter=False).draw_batch(1)[0]
    mp = Matterport(datapath=mroot, subepoch=0, raw=True)
    for i in range(len(mp)):
        check("mp_sub0_i%d" % i, mp, i, [96, 128], off)
    check("mp_default_size_i2", mp, 2, [384, 512], off)
    pano = InteriorNet(datapath=proot, subepoch=0, streetlearn_interiornet_type="", raw=True)
    for i in range(4):
        check("interiornet_sub0_i%d" % i, pano, i, [64, 80], off)
    for name, p in EC.FIXED_JITTER.items():
        row = torch.tensor([float(v) for v in p["order"]] + [p["b"], p["c"], p["s"], p["h"], float(p["gray"])])
        check("mp_%s_i3" % name, mp, 3, [96, 128], row)
        check("interiornet_%s_i2" % name, pano, 2, [64, 80], row)


@pytest.mark.parametrize("M", [140, 1152, 8960, 73728 + 48])
def test_fused_mlp_inference_kernel(ops, M):
    """rp_mlp_fused_fwd: y = x + fc2(GELU(fc1(LN(x)))) with the hidden activation on chip (vision_transformer.py:353,
    vit_layers/mlp.py:20-26) against fp64 PyTorch and against the unfused kernel chain it replaces at inference; row counts
    that are not multiples of the 128-row tile (the CrossBlock's 70-token output: 140 rows per pair) and that exercise the
    stream-K split with shared tiles.  Tolerance 2e-6 relative to max|y| (fp32 MFMA accumulation over K = 192 / 768)."""
    import torch.nn.functional as F
    x = rnd(M, 192, seed=1, scale=2.0)
    x[3] = x[3] * 30 + 100                                         # a row with a large mean: centred variance
    g, b = 1 + 0.1 * rnd(192, seed=2), 0.1 * rnd(192, seed=3)
    w1, b1 = rnd(768, 192, seed=4, scale=192 ** -0.5), 0.1 * rnd(768, seed=5)
    w2, b2 = rnd(192, 768, seed=6, scale=768 ** -0.5), 0.1 * rnd(192, seed=7)
    y = ops.mlp_fused(x, g, b, w1, b1, w2, b2)
    xd = x.double()
    ref = xd + F.linear(F.gelu(F.linear(F.layer_norm(xd, (192,), g.double(), b.double(), 1e-6), w1.double(), b1.double())),
                        w2.double(), b2.double())
    e = rel(y, ref)
    xn, _, _ = ops.layernorm_fwd(x, g, b)
    chain = ops.linear(ops.linear(xn, w1, b1, act=1), w2, b2, residual=x)
    e2 = rel(y, chain)
    report("mlp_fused_M%d" % M, vs_fp64=e, vs_unfused_chain=e2, chain_vs_fp64=rel(chain, ref))
    assert e < 2e-6 and e2 < 2e-6
    assert torch.equal(y, ops.mlp_fused(x, g, b, w1, b1, w2, b2))                  # deterministic (fixed-order fix-up)
    # training form: the same launch also stores what the backward needs (its y may differ from the inference launch's in the last
    # bit: the two instantiations' occupancy, hence where the stream-K split cuts a tile's chunk range, can differ)
    yt, xn_t, mean_t, rstd_t, h_t, hpre_t = ops.mlp_fused(x, g, b, w1, b1, w2, b2, train=True)
    xnd = F.layer_norm(xd, (192,), g.double(), b.double(), 1e-6)
    pre_ref = F.linear(xnd, w1.double(), b1.double())
    t = dict(xn=rel(xn_t, xnd), mean=rel(mean_t, xd.mean(1)), rstd=rel(rstd_t, (xd.var(1, unbiased=False) + 1e-6).rsqrt()),
             hpre=rel(hpre_t, pre_ref), h=rel(h_t, F.gelu(pre_ref)))
    t["y_vs_inference_launch"] = rel(yt, y)
    report("mlp_fused_train_M%d" % M, **t)
    assert max(t.values()) < 2e-6 and t["y_vs_inference_launch"] < 5e-7, t
    assert all(torch.equal(a_, b_) for a_, b_ in zip(ops.mlp_fused(x, g, b, w1, b1, w2, b2, train=True), (yt, xn_t, mean_t, rstd_t, h_t, hpre_t)))
    with pytest.raises(RuntimeError):
        ops.mlp_fused(x[:, :128].contiguous(), g[:128], b[:128], w1[:, :128].contiguous(), b1, w2, b2)


@pytest.mark.parametrize("M", [140, 1152, 9216 + 48])
def test_row_resident_linear_with_fused_layernorm(ops, M):
    """rp_linear_rows192 -- the K = 192 Linear layers (qkv, proj, fc1: vision_transformer.py:323,330,352-353, mlp.py:22-23) with the
    preceding LayerNorm fused in -- against fp64 PyTorch: y, pre-activation, normalised rows, mean, rstd; and
    against the generic rp_gemm path it replaces.  Tolerance 2e-6 of max|y| (fp32 accumulation over K = 192)."""
    import torch.nn.functional as F
    x = rnd(M, 192, seed=11, scale=2.0)
    x[5] = x[5] * 20 - 50
    g, b = 1 + 0.1 * rnd(192, seed=12), 0.1 * rnd(192, seed=13)
    xd = x.double()
    xnd = F.layer_norm(xd, (192,), g.double(), b.double(), 1e-6)
    worst = {}
    # qkv: LN fused, training outputs
    w, bias = rnd(576, 192, seed=14, scale=192 ** -0.5), 0.1 * rnd(576, seed=15)
    y, xn, mean, rstd = ops.linear_rows(x, w, bias, ln=(g, b), want_ln_out=True)
    worst["qkv"] = rel(y, F.linear(xnd, w.double(), bias.double()))
    worst["xn"] = rel(xn, xnd)
    worst["mean"] = rel(mean, xd.mean(1))
    worst["rstd"] = rel(rstd, (xd.var(1, unbiased=False) + 1e-6).rsqrt())
    xn_k, m_k, r_k = ops.layernorm_fwd(x, g, b)
    worst["xn_vs_ln_kernel"] = rel(xn, xn_k)
    y_inf = ops.linear_rows(x, w, bias, ln=(g, b))                                      # inference: no side outputs
    assert torch.equal(y_inf, y)
    # proj: no LN, residual
    wp, bp, res = rnd(192, 192, seed=16, scale=192 ** -0.5), 0.1 * rnd(192, seed=17), rnd(M, 192, seed=18)
    worst["proj"] = rel(ops.linear_rows(x, wp, bp, residual=res), res.double() + F.linear(xd, wp.double(), bp.double()))
    # fc1: LN + GELU + pre-activation
    w1, b1 = rnd(768, 192, seed=19, scale=192 ** -0.5), 0.1 * rnd(768, seed=20)
    h, hpre, xn2, _, _ = ops.linear_rows(x, w1, b1, act=1, want_pre=True, ln=(g, b), want_ln_out=True)
    pre_ref = F.linear(xnd, w1.double(), b1.double())
    worst["fc1_pre"] = rel(hpre, pre_ref)
    worst["fc1_gelu"] = rel(h, F.gelu(pre_ref))
    # the generic GEMM path on the same inputs
    old = ops.gemm(xn_k, w1, M, 768, 192, bias=b1, act=1)
    worst["fc1_vs_rp_gemm"] = rel(h, old)
    assert ops.linear(x, wp, bp, residual=res).shape == (M, 192)                          # ops.linear routes here for K = 192
    report("linear_rows_M%d" % M, **worst)
    assert max(worst.values()) < 2e-6, worst
    with pytest.raises(RuntimeError):
        ops.linear_rows(x, rnd(200, 192, seed=1), None)                                    # N % 32 != 0


@pytest.mark.parametrize("M", [140, 9216 + 48])
def test_row_resident_linear_bf16_configuration(ops, M):
    """rp_linear_rows192 at operand precision 1 (the bf16 configuration: v_mfma_f32_16x16x32_bf16, fp32 accumulate; LayerNorm, bias,
    GELU, residual in fp32).  With bf16-REPRESENTABLE operands the products are exact, so the result must match fp64 to fp32
    accumulation accuracy (3e-6 of the maximum); with general operands it is the bf16-operand product (2e-2 relative to fp64, the
    tolerance of the bf16 rp_gemm test).  bf16 storage: y / pre are the round-to-nearest-even of the fp32 outputs BIT FOR BIT, and a
    bf16 aux is read exactly."""
    import torch.nn.functional as F
    bf = torch.bfloat16
    prev = ops.GEMM_PRECISION
    ops.set_gemm_precision(1)
    try:
        q = lambda t: t.to(bf).float()
        x, res = q(rnd(M, 192, seed=31)), rnd(M, 192, seed=32)
        w, bias = q(rnd(576, 192, seed=33, scale=192 ** -0.5)), 0.1 * rnd(576, seed=34)
        e = {}
        e["qkv_exact_operands"] = rel(ops.linear_rows(x, w, bias), F.linear(x.double(), w.double(), bias.double()))
        wp = q(rnd(192, 192, seed=35, scale=192 ** -0.5))
        e["proj_exact_operands"] = rel(ops.linear_rows(x, wp, None, residual=res), res.double() + x.double() @ wp.double().t())
        assert max(e.values()) < 3e-6, e
        # general operands + fused LayerNorm + GELU: bf16-operand accuracy, LayerNorm outputs still fp32-exact
        xg = rnd(M, 192, seed=36, scale=2.0)
        g, b = 1 + 0.1 * rnd(192, seed=37), 0.1 * rnd(192, seed=38)
        w1, b1 = rnd(768, 192, seed=39, scale=192 ** -0.5), 0.1 * rnd(768, seed=40)
        h, hpre, xn, mean, rstd = ops.linear_rows(xg, w1, b1, act=1, want_pre=True, ln=(g, b), want_ln_out=True)
        xnd = F.layer_norm(xg.double(), (192,), g.double(), b.double(), 1e-6)
        pre_ref = F.linear(xnd, w1.double(), b1.double())
        f = dict(xn=rel(xn, xnd), mean=rel(mean, xg.double().mean(1)))
        assert max(f.values()) < 2e-6, f
        f.update(fc1_pre=rel(hpre, pre_ref), fc1_gelu=rel(h, F.gelu(pre_ref)))
        assert max(f.values()) < 2e-2, f
        # bf16 storage of the outputs
        h16, hpre16, _, _, _ = ops.linear_rows(xg, w1, b1, act=1, want_pre=True, ln=(g, b), want_ln_out=True, out_dtype=bf)
        assert h16.dtype == bf and torch.equal(h16, h.to(bf)) and torch.equal(hpre16, hpre.to(bf))
        # input-gradient form with GELU'(aux), aux in bf16, output in bf16, column sums from the fp32 values
        dy, w2 = rnd(M, 192, seed=41), rnd(192, 768, seed=42, scale=768 ** -0.5)
        d32, cs32 = ops.linear_dx(dy, w2, dact=1, aux=hpre16.float(), want_colsum=True)
        d16, cs16 = ops.linear_dx(dy, w2, dact=1, aux=hpre16, want_colsum=True, out_dtype=bf)
        assert d16.dtype == bf and torch.equal(d16, d32.to(bf)) and torch.equal(cs16, cs32)
        a = hpre16.double()
        gp = 0.5 * (1 + torch.erf(a / math.sqrt(2))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2 * math.pi)
        ref = (dy.double() @ w2.double()) * gp
        f.update(dx=rel(d32, ref), colsum=rel(cs32, ref.sum(0)))
        report("linear_rows_bf16_M%d" % M, **e, **f)
        assert f["dx"] < 2e-2 and f["colsum"] < 2e-2, f
    finally:
        ops.set_gemm_precision(prev)
    with pytest.raises(RuntimeError):
        ops.linear_rows(rnd(64, 192), rnd(192, 192), None, out_dtype=bf)             # bf16 storage only in the bf16 configuration


@pytest.mark.parametrize("M", [140, 1152, 9216 + 48])
def test_fused_mlp_backward_data_kernel(ops, M):
    """rp_mlp_fused_bwd: dhp = (dy W2) o GELU'(h_pre), dxn = dhp W1 and the per-tile column sums of dhp (fc1 bias gradient) as one
    kernel, against fp64 autograd of fc2(GELU(fc1(xn))) (vit_layers/mlp.py:20-26).  Tolerance 3e-6 of the maximum."""
    import torch.nn.functional as F
    w1, b1 = rnd(768, 192, seed=4, scale=192 ** -0.5), 0.1 * rnd(768, seed=5)
    w2 = rnd(192, 768, seed=6, scale=768 ** -0.5)
    xn = rnd(M, 192, seed=8).double().requires_grad_(True)
    dy = rnd(M, 192, seed=9)
    hp = F.linear(xn, w1.double(), b1.double())
    hp.retain_grad()
    y = F.linear(F.gelu(hp), w2.double())
    y.backward(dy.double())
    dhp, dxn, part = ops.mlp_fused_bwd(dy, hp.detach().float().contiguous(), w1, w2)
    e = dict(dhp=rel(dhp, hp.grad), dxn=rel(dxn, xn.grad), db1=rel(part.sum(0), hp.grad.sum(0)))
    report("mlp_fused_bwd_M%d" % M, **e)
    assert max(e.values()) < 3e-6, e
    d2, x2, p2 = ops.mlp_fused_bwd(dy, hp.detach().float().contiguous(), w1, w2)
    assert torch.equal(d2, dhp) and torch.equal(x2, dxn) and torch.equal(p2, part)        # deterministic


@pytest.mark.parametrize("M", [140, 9216 + 48])
def test_fused_mlp_forward_bf16_configuration(ops, M):
    """rp_mlp_fused_fwd at operand precision 1 (both products on v_mfma_f32_16x16x32_bf16 from bf16 weight copies; LayerNorm, bias, GELU
    and the residual fp32), inference and training form.  LayerNorm outputs stay fp32-exact (2e-6); the pre-activation, the hidden
    activation and y carry the bf16 operand rounding (2e-2 of the maximum against fp64); with bf16 storage h / hpre are the
    round-to-nearest-even of the fp32-stored ones BIT FOR BIT and y is unchanged; the inference launch gives the training launch's y."""
    import torch.nn.functional as F
    bf = torch.bfloat16
    x = rnd(M, 192, seed=1, scale=2.0)
    g, b = 1 + 0.1 * rnd(192, seed=2), 0.1 * rnd(192, seed=3)
    w1, b1 = rnd(768, 192, seed=4, scale=192 ** -0.5), 0.1 * rnd(768, seed=5)
    w2, b2 = rnd(192, 768, seed=6, scale=768 ** -0.5), 0.1 * rnd(192, seed=7)
    xd = x.double()
    xnd = F.layer_norm(xd, (192,), g.double(), b.double(), 1e-6)
    pre_ref = F.linear(xnd, w1.double(), b1.double())
    ref = xd + F.linear(F.gelu(pre_ref), w2.double(), b2.double())
    prev = ops.GEMM_PRECISION
    ops.set_gemm_precision(1)
    try:
        y, xn, mean, rstd, h, hpre = ops.mlp_fused(x, g, b, w1, b1, w2, b2, train=True)
        e = dict(xn=rel(xn, xnd), mean=rel(mean, xd.mean(1)), rstd=rel(rstd, (xd.var(1, unbiased=False) + 1e-6).rsqrt()))
        assert max(e.values()) < 2e-6, e
        e.update(hpre=rel(hpre, pre_ref), h=rel(h, F.gelu(pre_ref)), y=rel(y, ref))
        # exactness of the SECOND product and of the unit permutation: y against fp64 on the kernel's own bf16-rounded h and weights
        y_chk = xd + F.linear(h.to(bf).double(), w2.to(bf).double(), b2.double())
        e["y_given_h"] = rel(y, y_chk)
        y16, _, _, _, h16, hpre16 = ops.mlp_fused(x, g, b, w1, b1, w2, b2, train=True, out_dtype=bf)
        assert h16.dtype == bf and torch.equal(h16, h.to(bf)) and torch.equal(hpre16, hpre.to(bf)) and torch.equal(y16, y)
        e["y_inference_launch"] = rel(ops.mlp_fused(x, g, b, w1, b1, w2, b2), y)
    finally:
        ops.set_gemm_precision(prev)
    report("mlp_fused_fwd_bf16_M%d" % M, **e)
    assert max(e["hpre"], e["h"], e["y"]) < 2e-2 and e["y_given_h"] < 3e-6 and e["y_inference_launch"] < 5e-7, e
    with pytest.raises(RuntimeError):
        ops.mlp_fused(x, g, b, w1, b1, w2, b2, train=True, out_dtype=bf)          # bf16 storage only in the bf16 configuration


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("M", [140, 1152, 9216 + 48, 73728])
def test_fused_mlp_backward_with_layernorm_backward_folded_in(ops, M, precision):
    """rp_mlp_fused_bwd_ln: the backward of norm2 (Block.forward, vision_transformer.py:353: x + mlp(norm2(x))) on the epilogue of the fused
    MLP backward -- dx = LayerNorm-backward(dxn) + dy, with dgamma / dbeta / colsum(dy) from per-row-block partial sums.  Reference: fp64
    LayerNorm backward of the dxn the SAME kernel writes without the fold (checked against autograd by the tests above), so the bound is
    fp32 rounding (3e-6 of the maximum) in both operand precisions.  The sizes cover tiles finished by one workgroup (epilogue form),
    tiles shared between workgroups (fix-up form: all of M = 1152, a third of 73 728) and a ragged last tile.  Deterministic."""
    bf = torch.bfloat16
    q = (lambda t: t.to(bf).float()) if precision else (lambda t: t)
    w1 = q(rnd(768, 192, seed=4, scale=192 ** -0.5))
    w2 = q(rnd(192, 768, seed=6, scale=768 ** -0.5))
    dy = q(rnd(M, 192, seed=9))
    hp = q(rnd(M, 768, seed=8, scale=1.5))
    x = rnd(M, 192, seed=10) * 2.0 + 0.3
    gamma = 1.0 + 0.2 * rnd(192, seed=11)
    mean = x.mean(1).contiguous()
    rstd = (x.var(1, unbiased=False) + 1e-6).rsqrt().contiguous()
    prev = ops.GEMM_PRECISION
    ops.set_gemm_precision(precision)
    try:
        dhp0, dxn, part0 = ops.mlp_fused_bwd(dy, hp, w1, w2)
        dhp, (dx, dg, db, da), part = ops.mlp_fused_bwd(dy, hp, w1, w2, ln=(x, gamma, mean, rstd))
        dhp2, (dx2, dg2, db2, da2), part2 = ops.mlp_fused_bwd(dy, hp, w1, w2, ln=(x, gamma, mean, rstd))
    finally:
        ops.set_gemm_precision(prev)
    assert torch.equal(dhp, dhp0) and torch.equal(part, part0)                      # the rest of the kernel is untouched
    assert all(torch.equal(a, b) for a, b in ((dx, dx2), (dg, dg2), (db, db2), (da, da2), (dhp, dhp2)))
    d = dxn.double()
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    g = d * gamma.double()
    ref = rstd.double()[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True)) + dy.double()
    e = dict(dx=rel(dx, ref), dgamma=rel(dg, (d * xh).sum(0)), dbeta=rel(db, d.sum(0)), colsum_dy=rel(da, dy.double().sum(0)))
    report("mlp_fused_bwd_ln_M%d_p%d" % (M, precision), **e)
    assert max(e.values()) < 3e-6, e


@pytest.mark.parametrize("M", [140, 9216 + 48])
def test_fused_mlp_backward_bf16_configuration(ops, M):
    """rp_mlp_fused_bwd at operand precision 1 (v_mfma_f32_16x16x32_bf16 from bf16 weight copies, the second one in the kernel's
    chunk-permuted unit order).  With bf16-representable dy and weights the FIRST product is exact: dhp must match fp64 to fp32
    accuracy (5e-6: v_exp_f32 / v_rcp_f32 are 1-ulp instructions); dxn contracts the bf16-rounded dhp -- against the fp64 product of exactly those rounded values also 3e-6, and
    within the stated bf16 tolerance (2e-2) of the unrounded chain.  bf16 storage: a bf16 hpre is read exactly and a bf16 dhp is the
    round-to-nearest-even of the fp32 one BIT FOR BIT; column sums come from the fp32 values."""
    import torch.nn.functional as F
    bf = torch.bfloat16
    q = lambda t: t.to(bf).float()
    w1, b1 = q(rnd(768, 192, seed=4, scale=192 ** -0.5)), 0.1 * rnd(768, seed=5)
    w2 = q(rnd(192, 768, seed=6, scale=768 ** -0.5))
    dy = q(rnd(M, 192, seed=9))
    hp = q(rnd(M, 768, seed=8, scale=1.5))                     # bf16-representable pre-activation: the bf16-stored run reads the same values
    # the bf16 configuration's GELU is torch's approximate='tanh' form (csrc/common.h: gelu_bf, |difference to the erf form| <= 4.8e-4,
    # below the bf16 storage rounding of the typical hidden value); the backward multiplies by ITS exact derivative
    a = hp.double().requires_grad_(True)
    F.gelu(a, approximate="tanh").sum().backward()
    gp = a.grad
    dhp_ref = (dy.double() @ w2.double()) * gp
    prev = ops.GEMM_PRECISION
    ops.set_gemm_precision(1)
    try:
        dhp, dxn, part = ops.mlp_fused_bwd(dy, hp, w1, w2)
        e = dict(dhp=rel(dhp, dhp_ref), db1=rel(part.sum(0), dhp_ref.sum(0)),
                 dxn_of_rounded_dhp=rel(dxn, dhp.to(bf).double() @ w1.double()), dxn=rel(dxn, dhp_ref @ w1.double()))
        d16, x16, p16 = ops.mlp_fused_bwd(dy, hp.to(bf), w1, w2, out_dtype=bf)
        assert d16.dtype == bf and torch.equal(d16, dhp.to(bf)) and torch.equal(x16, dxn) and torch.equal(p16, part)
        d2, x2, p2 = ops.mlp_fused_bwd(dy, hp, w1, w2)
        assert torch.equal(d2, dhp) and torch.equal(x2, dxn) and torch.equal(p2, part)        # deterministic
    finally:
        ops.set_gemm_precision(prev)
    report("mlp_fused_bwd_bf16_M%d" % M, **e)
    assert max(e["dhp"], e["db1"]) < 5e-6 and e["dxn_of_rounded_dhp"] < 3e-6 and e["dxn"] < 2e-2, e
    with pytest.raises(RuntimeError):
        ops.mlp_fused_bwd(dy, hp.to(bf), w1, w2)                  # bf16 storage only in the bf16 configuration


@pytest.mark.parametrize("M", [140, 1152, 9216 + 48])
def test_row_resident_input_gradient_with_gelu_grad_and_column_sums(ops, M):
    """linear_dx for a Linear with 192 outputs (fc2, attention proj) on rp_linear_rows192: dx = (dy W) o GELU'(aux) and the column
    sums of dx (the fc1 bias gradient), against fp64 and against the rp_gemm path.  Tolerance 3e-6 of the maximum."""
    dy, aux = rnd(M, 192, seed=21), rnd(M, 768, seed=22, scale=1.5)
    w2 = rnd(192, 768, seed=23, scale=768 ** -0.5)
    dx, cs = ops.linear_dx(dy, w2, dact=1, aux=aux, want_colsum=True)
    a = aux.double()
    gp = 0.5 * (1 + torch.erf(a / math.sqrt(2))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2 * math.pi)
    ref = (dy.double() @ w2.double()) * gp
    old_dx, old_cs = ops.gemm(dy, w2, M, 768, 192, b_layout=1, dact=1, aux=aux, want_colsum=True)
    wp = rnd(192, 192, seed=24, scale=192 ** -0.5)
    e = dict(dx=rel(dx, ref), colsum=rel(cs, ref.sum(0)), vs_rp_gemm=rel(dx, old_dx), colsum_vs_rp_gemm=rel(cs, old_cs),
             proj_dx=rel(ops.linear_dx(dy, wp), dy.double() @ wp.double()))
    report("linear_rows_dx_M%d" % M, **e)
    assert max(e.values()) < 3e-6, e


@pytest.mark.parametrize("shape,training", [((6, 64, 112, 112), True), ((3, 8, 9, 11), True), ((2, 16, 10, 7), False)])
def test_fused_stem_batchnorm_relu_maxpool_is_bit_identical_to_the_separate_kernels(ops, shape, training):
    """ops.bn_relu_maxpool (rp_bn_relu_pool_fwd / _bwd: the stem's bn1 -> relu -> maxpool, src/model.py:127-130, without the
    full-resolution intermediates) against BnActFn + MaxPool3x3s2Fn: outputs, window positions and running statistics bit-identical
    (same arithmetic), gradients equal to 2e-6 (the fused backward sums window-major; bit-identical in eval mode, where no sums
    enter dx), odd sizes included; and against torch.nn in fp64 (2e-6)."""
    import copy
    N, C, H, W = shape
    torch.manual_seed(3)
    bn = torch.nn.BatchNorm2d(C).cuda()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(C))
        bn.weight[0] = -0.7                                     # a negative scale: relu(bn(.)) is not monotone in x there
        bn.bias.copy_(0.2 * torch.randn(C))
        bn.running_mean.copy_(0.1 * torch.randn(C)); bn.running_var.copy_(0.5 + torch.rand(C))
    bn.train(training)
    pool = torch.nn.MaxPool2d(3, 2, 1)
    x0 = (torch.randn(N, C, H, W, device="cuda") * 1.5 + 0.3).contiguous(memory_format=torch.channels_last)
    x0[0, :, :4, :4] = 0.25                                     # ties inside windows
    cot = None
    res = []
    for fused in (True, False):
        b = copy.deepcopy(bn)
        x = x0.clone().requires_grad_(True)
        prev, ops.FUSE_STEM_POOL = ops.FUSE_STEM_POOL, fused
        try:
            y = ops.bn_relu_maxpool(b, pool, x)
        finally:
            ops.FUSE_STEM_POOL = prev
        if cot is None:
            cot = torch.randn_like(y)
        y.backward(cot)
        res.append((y.detach(), x.grad, b.weight.grad, b.bias.grad, b.running_mean.clone(), b.running_var.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][4], res[1][4]) and torch.equal(res[0][5], res[1][5])
    for a, bb in zip(res[0][1:4], res[1][1:4]):
        assert rel(a, bb) < 2e-6
    if not training:
        assert torch.equal(res[0][1], res[1][1])
    b64 = copy.deepcopy(bn).double()
    x64 = x0.double().requires_grad_(True)
    y64 = pool(torch.relu(b64(x64)))
    y64.backward(cot.double())
    e = dict(y=rel(res[0][0], y64), dx=rel(res[0][1], x64.grad), dgamma=rel(res[0][2], b64.weight.grad), dbeta=rel(res[0][3], b64.bias.grad))
    report("bn_relu_maxpool_%dx%dx%dx%d" % shape, **e)
    assert max(e.values()) < 2e-6, e


@pytest.mark.parametrize("N,H,W", [(4, 224, 224), (2, 64, 96), (1, 32, 32)])
def test_hand_written_stem_convolution(ops, N, H, W):
    """rp_conv_stem_fwd (resnet.conv1: 7x7 / 2, pad 3, 3 -> 64; src/model.py:127) on the zero-framed channels-last image against fp64
    F.conv2d (2e-6 of the maximum; MIOpen's own fp32 result is at 7e-7), its BatchNorm-statistics partials against the sums of the
    output, the framed preprocessing kernel against the plain one (bit-exact interior, zero frame), and the weight gradient of
    StemConvFn against autograd's."""
    import torch.nn.functional as F
    torch.manual_seed(5)
    x = torch.randn(N, 3, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    w = (torch.randn(64, 3, 7, 7, device="cuda") * 0.05).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    xp = F.pad(x.permute(0, 2, 3, 1), (0, 0, 3, 3, 3, 3)).contiguous()
    y, stats = ops.conv_stem_fwd(xp, w.detach(), want_stats=True)
    ref = F.conv2d(x.double(), w.detach().double(), None, 2, 3).permute(0, 2, 3, 1)
    e = dict(y=rel(y, ref), sum=rel(stats[:, 0].sum(0), ref.sum((0, 1, 2))), sumsq=rel(stats[:, 1].sum(0), (ref * ref).sum((0, 1, 2))))
    assert torch.equal(ops.conv_stem_fwd(xp, w.detach()), y)
    out = ops.StemConvFn.apply(xp, w)
    cot = torch.randn_like(out)
    out.backward(cot)
    wd = w.detach().double().requires_grad_(True)
    F.conv2d(x.double(), wd, None, 2, 3).backward(cot.double())
    e["dw"] = rel(w.grad, wd.grad)
    report("conv_stem_%dx%dx%d" % (N, H, W), **e)
    assert max(e.values()) < 2e-6, e
    if (H, W) == (224, 224):
        imgs = torch.floor(torch.rand(2, 2, 3, 96, 128, device="cuda") * 255)
        plain, framed = ops.preprocess(imgs), ops.preprocess(imgs, pad=3)
        assert torch.equal(framed[:, 3:-3, 3:-3, :], plain.permute(0, 2, 3, 1))
        framed[:, 3:-3, 3:-3, :] = 0
        assert float(framed.abs().max()) == 0.0


@pytest.mark.parametrize("N", [1, 3, 128])
def test_stem_weight_gradient_exact_fp32(ops, N):
    """rp_conv_stem_wgrad_f32 (csrc/conv_stem_wgrad_f32.hip: weight gradient of resnet.conv1, 7x7 / 2, pad 3, 3 -> 64, src/model.py:127, in
    the exact-fp32 configuration; space-to-depth + the output-stationary fp32 stream) against fp64 autograd of F.conv2d over ALL images
    (N = 1, 3: fewer / ragged tile runs per workgroup) and against MIOpen's fp32 backward-weights at the headline size (N = 128):
    3e-6 of the maximum (fp32 accumulation of up to 1.6 M exact products per element in per-workgroup partials summed in a fixed order)
    / 2e-5 between the two fp32 results.  Deterministic.  The 8th row / column of the space-to-depth support must not leak into dW."""
    import torch.nn.functional as F
    CL = torch.channels_last
    x = rnd(N, 3, 224, 224, seed=1).contiguous(memory_format=CL)
    dy = rnd(N, 64, 112, 112, seed=2).contiguous(memory_format=CL)
    xp = F.pad(x.permute(0, 2, 3, 1), (0, 0, 3, 3, 3, 3)).contiguous()
    dw = ops.conv_stem_wgrad_f32(xp, dy.permute(0, 2, 3, 1))
    assert torch.equal(dw, ops.conv_stem_wgrad_f32(xp, dy.permute(0, 2, 3, 1)))            # deterministic
    w = rnd(64, 3, 7, 7, seed=3, scale=0.05).contiguous(memory_format=CL)
    if N <= 3:
        w64 = w.double().requires_grad_(True)
        F.conv2d(x.double(), w64, None, 2, 3).backward(dy.double())
        e, bound = rel(dw.permute(0, 3, 1, 2), w64.grad), 3e-6
    else:
        ref = torch.ops.aten.convolution_backward(dy, xp.permute(0, 3, 1, 2), w, None, [2, 2], [0, 0], [1, 1], False, [0, 0], 1,
                                                  [False, True, False])[1]
        e, bound = rel(dw.permute(0, 3, 1, 2), ref.double()), 2e-5
    report("conv_stem_wgrad_f32[N=%d]" % N, dw=e)
    assert e < bound, e
    with pytest.raises(RuntimeError):
        ops.conv_stem_wgrad_f32(xp[:, :100].contiguous(), dy.permute(0, 2, 3, 1))


def test_deferred_splitk_reduces_are_bit_identical(ops):
    """ops.splitk_batch: the weight-gradient GEMMs of a block leave their split-K slabs in a private arena and ONE rp_splitk_reduce_multi
    finishes all of them (incl. the transposed-store form of fc2) -- same sums in the same order as each GEMM's own reduce."""
    M = 9 * 576
    dy1, x1 = rnd(M, 576, seed=1), rnd(M, 192, seed=2)        # qkv-like: [576,192]
    dy2, x2 = rnd(M, 192, seed=3), rnd(M, 768, seed=4)        # fc2-like: wide-K', reduce writes the transpose
    dy3, x3 = rnd(M, 192, seed=5), rnd(M, 192, seed=6)
    keep = ops.SPLITK_BATCHING
    try:
        ops.SPLITK_BATCHING = False
        ref = [ops.linear_dw(dy1, x1), ops.linear_dw(dy2, x2), ops.linear_dw(dy3, x3)]
        ops.SPLITK_BATCHING = True
        with ops.splitk_batch():
            out = [ops.linear_dw(dy1, x1), ops.linear_dw(dy2, x2), ops.linear_dw(dy3, x3)]
    finally:
        ops.SPLITK_BATCHING = keep
    torch.cuda.synchronize()
    for a, b in zip(out, ref):
        assert torch.equal(a, b)
    assert rel(out[0], dy1.double().t() @ x1.double()) < 2e-6


def test_transposed_weight_cache_and_batched_transposes(ops):
    """ops.transposed: W^T of registered weights comes from one rp_transpose_multi launch, is cached on the tensor and follows
    in-place updates and explicit invalidation (a graph replay)."""
    ws = [torch.nn.Parameter(rnd(r, c, seed=10 + i)) for i, (r, c) in enumerate([(768, 192), (192, 768), (192, 192), (70, 33)])]
    ops.register_transposed(*ws)
    t0 = ops.transposed(ws[0])
    assert torch.equal(t0, ws[0].detach().t())
    for w in ws[1:]:                                     # the others were transposed by the same launch
        assert getattr(w, "_rp_t", None) is not None and torch.equal(w._rp_t[3], w.detach().t())
        assert ops.transposed(w) is w._rp_t[3]
    with torch.no_grad():
        ws[2].mul_(2.0)
    assert torch.equal(ops.transposed(ws[2]), ws[2].detach().t())
    stale = ops.transposed(ws[3])
    ops.invalidate_pad_cache()
    fresh = ops.transposed(ws[3])
    assert fresh is not stale and torch.equal(fresh, ws[3].detach().t())


@pytest.mark.parametrize("M,N", [(4096, 192), (4096 + 640, 576), (9 * 4096, 768)])
def test_weight_gradient_output_stationary_fp32(ops, M, N, monkeypatch):
    """rp_dw192_f32 (exact fp32, output-stationary [192 x 192] tiles + the fixed-order split-K reduce) through ops.linear_dw, both
    orientations, against fp64 (3e-6 of max|dW|: fp32 products and sums over ~600-row slabs) and against the rp_gemm split-K form it
    replaces (same arithmetic in another summation order: 3e-6); deterministic; deferred reduce inside ops.splitk_batch gives the
    same bits."""
    wide = rnd(M, N, seed=3)
    nar = rnd(M, 192, seed=4)
    ref = wide.double().t() @ nar.double()
    dw = ops.linear_dw(wide, nar)                      # dy wide: [N,192]
    dw2 = ops.linear_dw(nar, wide)                     # x wide: [192,N] (transposed by the reduce)
    e1, e2 = rel(dw, ref), rel(dw2, ref.t())
    monkeypatch.setattr(ops, "DW192_F32", False)
    old, old2 = ops.linear_dw(wide, nar), ops.linear_dw(nar, wide)
    monkeypatch.setattr(ops, "DW192_F32", True)
    e3 = max(rel(dw, old), rel(dw2, old2))
    report("dw192_f32[M=%d,N=%d]" % (M, N), direct=e1, transposed=e2, vs_rp_gemm=e3)
    assert dw.shape == (N, 192) and dw2.shape == (192, N) and max(e1, e2, e3) < 3e-6
    assert torch.equal(dw, ops.linear_dw(wide, nar))
    with ops.splitk_batch():
        d3, d4 = ops.linear_dw(wide, nar), ops.linear_dw(nar, wide)
    assert torch.equal(d3, dw) and torch.equal(d4, dw2)


@pytest.mark.parametrize("M,N", [(4096, 192), (4096 + 640, 576), (9 * 4096, 768), (128 * 576, 192)])
def test_weight_gradient_split3_is_fp32_grade(ops, M, N, monkeypatch):
    """rp_dw192_split3 (opt-in, RP_DW_SPLIT3=1: fp32 operands split on chip into three round-to-nearest bf16 limbs, six limb products on
    the bf16 matrix pipe, fp32 accumulators) against fp64 and against the exact-fp32 kernel it would replace: the
    SAME bound as test_weight_gradient_output_stationary_fp32 (3e-6 of max|dW|), and its error against fp64 stays within 1.25x of the fp32
    MFMA kernel's own, maximum and rms (measured: maximum equal, rms 1.03-1.16x -- the bf16 MFMA's internal 16-term sum rounds a little
    more than eight 2-term fp32 MFMAs; the gate's "<= the exact kernel's" is therefore MISSED by that margin and the path stays opt-in:
    profiles/r6_split3_gate.txt).  Operands with a wide dynamic range (a column scale 2^-20 .. 2^20) are included: the
    split is per element, so a large column cannot swamp a small one.  Deterministic; same slabs, same deferred reduce."""
    wide = rnd(M, N, seed=3)
    nar = rnd(M, 192, seed=4)
    sc = torch.exp2(torch.linspace(-20, 20, 192, device=nar.device))
    for tag, b in (("plain", nar), ("wide_range", nar * sc)):
        ref = wide.double().t() @ b.double()
        exact = ops.linear_dw(wide, b)
        monkeypatch.setattr(ops, "DW_SPLIT3", True)
        dw = ops.linear_dw(wide, b)                      # dy wide: [N,192]
        dw2 = ops.linear_dw(b, wide)                     # x wide: [192,N] (transposed by the reduce)
        again = ops.linear_dw(wide, b)
        with ops.splitk_batch():
            d3 = ops.linear_dw(wide, b)
        monkeypatch.setattr(ops, "DW_SPLIT3", False)
        # per-column errors (each column of dW has its own scale in the wide-range case)
        den = ref.abs().amax(dim=0, keepdim=True)
        e_split = float(((dw.double() - ref).abs() / den).max())
        e_exact = float(((exact.double() - ref).abs() / den).max())
        e_t = float(((dw2.double().t() - ref).abs() / den).max())
        rms_split = float(((dw.double() - ref) / den).square().mean().sqrt())
        rms_exact = float(((exact.double() - ref) / den).square().mean().sqrt())
        report("dw192_split3[M=%d,N=%d,%s]" % (M, N, tag), split3=e_split, exact_fp32=e_exact, transposed=e_t, rms_split3=rms_split,
               rms_exact_fp32=rms_exact)
        assert dw.shape == (N, 192) and dw2.shape == (192, N) and max(e_split, e_t) < 3e-6
        assert e_split <= 1.25 * e_exact and rms_split <= 1.25 * rms_exact
        assert torch.equal(dw, again) and torch.equal(dw, d3)


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return all(_same(u, v) for u, v in zip(a, b) if u is not None)
    return torch.equal(a, b)


def test_fp32_path_kernels_are_bit_reproducible_at_full_size(ops):
    """The exact-fp32 kernels that stage operands through LDS rings (LDS-DMA, hand-counted waits), at the headline size (128 images,
    M = 73 728 token rows), six launches each on the same inputs: bit-identical outputs.  Companion of
    test_bf16_path_kernels_are_bit_reproducible_at_full_size (round 4 found a ring slot refilled under a slow wave's reads in one of the
    bf16 kernels, visible only under full load)."""
    Z = 128
    M = Z * 576
    x, gm, bt = rnd(M, 192, seed=51), 1 + 0.1 * rnd(192, seed=52), 0.1 * rnd(192, seed=53)
    W = rnd(576, 192, seed=54, scale=0.07)
    dy = rnd(M, 576, seed=55)
    add = rnd(M, 192, seed=56)
    _, mean, rstd = ops.layernorm_fwd(x, gm, bt)
    w1, b1 = rnd(768, 192, seed=57, scale=0.07), 0.1 * rnd(768, seed=58)
    w2, b2 = rnd(192, 768, seed=59, scale=0.04), 0.1 * rnd(192, seed=60)
    qkv = rnd(M, 576, seed=61)
    do = rnd(M, 192, seed=62)
    o, lse = ops.attn_fwd(qkv, Z)
    hpre = ops.mlp_fused(x, gm, bt, w1, b1, w2, b2, train=True)[5]
    cases = {
        "dw192_f32": lambda: ops.linear_dw(dy, x),
        "qkv_dx_lnbwd": lambda: ops.linear_dx_lnbwd(dy, W, x, gm, mean, rstd, add=add),
        "qkv_fwd": lambda: ops.ln_linear(x, gm, bt, W, 0.1 * gm.repeat(3), train=True),
        "proj_fwd": lambda: ops.linear(do, W[:192], gm, residual=x),
        "mlp_fwd": lambda: ops.mlp_fused(x, gm, bt, w1, b1, w2, b2, train=True),
        "mlp_infer": lambda: ops.mlp_fused(x, gm, bt, w1, b1, w2, b2),
        "mlp_bwd": lambda: ops.mlp_fused_bwd(add, hpre, w1, w2),
        "attn_fwd": lambda: ops.attn_fwd(qkv, Z),
        "attn_bwd": lambda: ops.attn_bwd(qkv, o, lse, do, Z),
    }
    bad = {}
    for name, fn in cases.items():
        ref = fn()
        torch.cuda.synchronize()
        n = 0
        for _ in range(6):
            out = fn()
            torch.cuda.synchronize()
            n += 0 if _same(ref, out) else 1
        bad[name] = float(n)
    report("fp32_path_reproducible_128_images", **bad)
    assert not any(bad.values()), bad
