"""rp_conv5x5_dgrad_f32 (librelpose_conv5x5.so, csrc_conv5x5/conv5x5_dgrad_f32.hip): the exact-fp32 input gradient of the two valid 5x5
convolutions of extractor_final_conv (conv2 192 -> 192, downsample.0 128 -> 192; 28 x 28 -> 24 x 24) on a real MI355X.

A workgroup of the kernel owns ONE pixel of dx for a block of 128 images and walks only the taps that fall inside dy, so the cases
are the 81 different tap sets of the 784 pixels (every launch has them all), the image blocks (N = 1, 2, 3: one ragged block;
N = 130: a full block and a ragged one of two images) and both channel counts.  References are fp64 on the CPU
(torch.nn.grad.conv2d_input), computed once per shape."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_kernels import report            # (the measured errors go to the suite's test report)

pytestmark = pytest.mark.gpu

CL = torch.channels_last


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib, ops as o
    _lib.load()
    _lib.load_conv5x5()
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed + int(np.prod(shape)) % 9973)
    return torch.randn(*shape, generator=g) * scale


def ints(*shape, seed=0, lo=-2, hi=2):
    g = torch.Generator(device="cpu").manual_seed(seed + int(np.prod(shape)) % 9973)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def ref64(dy, w):
    """fp64 input gradient on the CPU: dy [N,192,24,24], w [192,CI,5,5] -> [N,CI,28,28]"""
    return torch.nn.grad.conv2d_input((dy.shape[0], w.shape[1], 28, 28), w.double(), dy.double())


def own(ops, dy, w, res=None):
    """the kernel on NCHW-shaped CPU operands -> NCHW-shaped CPU result"""
    dyr = dy.cuda().permute(0, 2, 3, 1).contiguous()
    wr = w.cuda().permute(0, 2, 3, 1).contiguous()
    rr = None if res is None else res.cuda().permute(0, 2, 3, 1).contiguous()
    return ops.conv5x5_dgrad_f32(dyr, wr, rr).permute(0, 3, 1, 2).cpu()


@functools.lru_cache(maxsize=None)
def exact_case(N, CI):
    dy, w = ints(N, 192, 24, 24, seed=31), ints(192, CI, 5, 5, seed=32)
    return dy, w, ref64(dy, w)


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("CI", [128, 192])
def test_exact_arithmetic_bit_for_bit(ops, N, CI):
    """dy and w are integers in -2..2: every partial sum is at most 4800 x 4 in magnitude, exact in fp32, so dx equals the fp64
    reference bit for bit whatever the order of the sum -- every tap, channel chunk and border case is pinned; likewise with a residual
    of small integers."""
    dy, w, ref = exact_case(N, CI)
    dx = own(ops, dy, w)
    assert dx.dtype == torch.float32 and torch.equal(dx.double(), ref)
    res = ints(N, CI, 28, 28, seed=33, lo=-8, hi=8)
    assert torch.equal(own(ops, dy, w, res).double(), ref + res.double())


@pytest.mark.parametrize("CI", [128, 192])
def test_more_than_one_block_of_images(ops, CI):
    """N = 130: a full block of 128 images and a ragged block of two.  The images are independent, so image n of the batch equals the
    same image run alone (bit for bit: the order of its sum does not depend on N); images 0, 127, 128 and 129 also equal fp64."""
    dy, w = ints(130, 192, 24, 24, seed=34), ints(192, CI, 5, 5, seed=32)
    dx = own(ops, dy, w)
    pick = [0, 127, 128, 129]
    assert torch.equal(dx[pick].double(), ref64(dy[pick], w))
    assert torch.equal(dx[:64], own(ops, dy[:64], w)) and torch.equal(dx[64:], own(ops, dy[64:], w))


@pytest.mark.parametrize("CI", [128, 192])
def test_impulses_give_the_flipped_filter(ops, CI):
    """one non-zero of dy at each corner and at an interior pixel, each in an image of its own: its 5 x 5 x CI footprint in dx is the
    filter (dx[y0 + r][x0 + s][ci] = w[co][ci][r][s]), everything else is exactly zero"""
    w = rnd(192, CI, 5, 5, seed=35)
    spots = [(0, 0, 0), (0, 23, 5), (23, 0, 64), (23, 23, 191), (11, 7, 100)]
    dy = torch.zeros(len(spots), 192, 24, 24)
    want = torch.zeros(len(spots), CI, 28, 28)
    for n, (y0, x0, co) in enumerate(spots):
        dy[n, co, y0, x0] = 1.0
        want[n, :, y0:y0 + 5, x0:x0 + 5] = w[co]
    assert torch.equal(own(ops, dy, w), want)


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("CI", [128, 192])
def test_random_operands_against_fp64_and_miopen(ops, N, CI):
    """random operands, filter scale (192 x 25)^-1/2: max error over max |ref| on every element against fp64, for the own kernel and for
    MIOpen's fp32 backward-data on the same operands.  The products are the same 4800 and only the order differs, so the own kernel
    must stay within 2 x MIOpen's error.  Two calls give the same bits."""
    dy = rnd(N, 192, 24, 24, seed=36)
    w = rnd(192, CI, 5, 5, seed=37, scale=(192 * 25) ** -0.5)
    ref = ref64(dy, w)
    dx = own(ops, dy, w)
    assert torch.equal(dx, own(ops, dy, w))
    dyc, wc = dy.cuda().contiguous(memory_format=CL), w.cuda().contiguous(memory_format=CL)
    x0 = torch.empty(N, CI, 28, 28, device="cuda").contiguous(memory_format=CL)
    mi = torch.ops.aten.convolution_backward(dyc, x0, wc, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, [True, False, False])[0].cpu()
    scale = float(ref.abs().max())
    e_own, e_mi = float((dx.double() - ref).abs().max()) / scale, float((mi.double() - ref).abs().max()) / scale
    print("conv5x5_dgrad_f32[N=%d,CI=%d]: own %.3e, MIOpen %.3e" % (N, CI, e_own, e_mi))
    report("conv5x5_dgrad_f32[N=%d,CI=%d]" % (N, CI), own=e_own, miopen=e_mi)
    assert e_own <= 2 * e_mi, (e_own, e_mi)


@pytest.mark.parametrize("N,CI,with_res", [(1, 128, True), (3, 192, True), (2, 192, False)])
def test_memory_contract(ops, N, CI, with_res):
    """NaN-poisoned guard bands around dy, w, res and dx, dx itself poisoned: the inputs and every band are untouched, every element of
    dx is written (none is NaN) and the result is the one of plain tensors"""
    from rel_pose_amd import _lib
    lib = _lib.load_conv5x5()
    G = 4096                                                        # floats of a band: the views stay 16-byte aligned

    def banded(t):
        buf = torch.full((t.numel() + 2 * G,), float("nan"), device="cuda")
        buf[G:G + t.numel()] = t.reshape(-1).cuda()
        return buf, buf[G:G + t.numel()]

    dy = ints(N, 24, 24, 192, seed=38)
    w = ints(192, 5, 5, CI, seed=39)
    res = ints(N, 28, 28, CI, seed=40, lo=-8, hi=8) if with_res else None
    bufs = {k: banded(v) for k, v in (("dy", dy), ("w", w), ("res", res)) if v is not None}
    before = {k: b.clone() for k, (b, _) in bufs.items()}
    out, dx = banded(torch.full((N, 28, 28, CI), float("nan")))
    ptr = lambda t: None if t is None else t.data_ptr()
    lib.rp_conv5x5_dgrad_f32(ptr(bufs["dy"][1]), ptr(bufs["w"][1]), ptr(dx), N, CI, ptr(bufs["res"][1]) if with_res else None,
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k, (b, _) in bufs.items():
        assert torch.equal(b.view(torch.int32), before[k].view(torch.int32)), k + " or its bands were written"
    assert bool(torch.isnan(out[:G]).all()) and bool(torch.isnan(out[-G:]).all()), "dx's bands were written"
    assert not bool(torch.isnan(dx).any()), "an element of dx was not written"
    plain = ops.conv5x5_dgrad_f32(dy.cuda(), w.cuda(), None if res is None else res.cuda())
    assert torch.equal(dx.view(N, 28, 28, CI), plain)


@pytest.mark.parametrize("CI", [128, 192])
def test_autograd_function_against_plain_autograd(ops, CI):
    """ops.Conv5x5ValidF32Fn (MIOpen forward, own input gradient, MIOpen weight and bias gradients) against plain autograd of F.conv2d at
    N = 2: the forward within 1e-5; dx within 2 x plain autograd's own error against fp64; dw and db within 2e-5 of plain autograd's"""
    N = 2
    x = rnd(N, CI, 28, 28, seed=41).cuda().contiguous(memory_format=CL)
    w = rnd(192, CI, 5, 5, seed=37, scale=(192 * 25) ** -0.5)
    b = rnd(192, seed=42, scale=0.3).cuda()
    dy = rnd(N, 192, 24, 24, seed=36)
    wc, dyc = w.cuda().contiguous(memory_format=CL), dy.cuda().contiguous(memory_format=CL)
    x1, w1, b1 = x.clone().requires_grad_(True), wc.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y1 = ops.Conv5x5ValidF32Fn.apply(x1, w1, b1)
    y1.backward(dyc)
    x2, w2, b2 = x.clone().requires_grad_(True), wc.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y2 = F.conv2d(x2, w2, b2)
    y2.backward(dyc)
    # (the same MIOpen call on the same operands; MIOpen may pick another solver from call to call, so not the same bits: two fp32
    # sums of CI x 25 products each within 3e-6 of the exact one)
    assert float((y1 - y2).detach().abs().max() / y2.detach().abs().max()) < 1e-5
    ref = ref64(dy, w)
    scale = float(ref.abs().max())
    e_own, e_mi = float((x1.grad.cpu().double() - ref).abs().max()) / scale, float((x2.grad.cpu().double() - ref).abs().max()) / scale
    rel = lambda a, c: float((a.double() - c.double()).abs().max() / c.double().abs().max())
    e_dw, e_db = rel(w1.grad, w2.grad), rel(b1.grad, b2.grad)
    print("Conv5x5ValidF32Fn[CI=%d]: dx own %.3e, plain %.3e, dw %.3e, db %.3e" % (CI, e_own, e_mi, e_dw, e_db))
    report("Conv5x5ValidF32Fn[CI=%d]" % CI, dx_own=e_own, dx_plain=e_mi, dw=e_dw, db=e_db)
    assert e_own <= 2 * e_mi and e_dw < 2e-5 and e_db < 2e-5, (e_own, e_mi, e_dw, e_db)
    # the dispatch: both layers' shapes from the threshold up, and nothing else
    m = torch.nn.Conv2d(CI, 192, 5).cuda()
    old = ops.CONV5X5_DGRAD_F32_MIN_N
    try:
        ops.CONV5X5_DGRAD_F32_MIN_N = 0
        assert ops.conv5x5_dgrad_f32_ok(m, x1) and not ops.conv5x5_dgrad_f32_ok(m, x1[:, :, :27])
        assert not ops.conv5x5_dgrad_f32_ok(torch.nn.Conv2d(CI, 192, 5, padding=2).cuda(), x1)
        assert not ops.conv5x5_dgrad_f32_ok(torch.nn.Conv2d(CI, 128, 5).cuda(), x1)
        ops.CONV5X5_DGRAD_F32_MIN_N = 3
        assert not ops.conv5x5_dgrad_f32_ok(m, x1)
    finally:
        ops.CONV5X5_DGRAD_F32_MIN_N = old


def test_whole_training_step_with_and_without_the_own_input_gradient(ops):
    """one training step of the product model at 2 pairs with CONV5X5_DGRAD_F32_MIN_N = 0 (both tail convolutions on the own kernel)
    against the same step with the switch off, under the fp32 criteria of test_every_kernel_path_switch_has_a_working_alternative:
    pose within 2e-4, every checked gradient cosine >= 0.9999"""
    import types
    from rel_pose_amd.model import ViTEss
    from tests.test_gpu_entrypoints import _step_outputs
    torch.manual_seed(0)
    args = types.SimpleNamespace(noess="", pool_size=60, fc_hidden_size=512, fusion_transformer=True, transformer_depth=6,
                                 cross_features=False, use_single_softmax=False, no_pos_encoding=False, l1_pos_encoding=False)
    model = ViTEss(args).cuda().train()
    images = torch.floor(torch.rand(2, 2, 3, 384, 384, device="cuda") * 255.0)
    Gs = torch.tensor([0, 0, 0, 0, 0, 0, 1.0]).repeat(2, 2, 1).cuda()
    intr = torch.tensor([[192.0, 192.0, 192.0, 192.0]]).repeat(2, 2, 1).cuda()
    bn = {k: v.clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    old = ops.CONV5X5_DGRAD_F32, ops.CONV5X5_DGRAD_F32_MIN_N
    calls = []
    inner = ops.conv5x5_dgrad_f32
    try:
        ops.CONV5X5_DGRAD_F32, ops.CONV5X5_DGRAD_F32_MIN_N = False, 0
        base_out, base_g = _step_outputs(model, images, Gs, intr)
        model.load_state_dict(bn, strict=False)
        ops.CONV5X5_DGRAD_F32 = True
        ops.conv5x5_dgrad_f32 = lambda *a: (calls.append(a[1].shape[-1]), inner(*a))[1]
        out, g = _step_outputs(model, images, Gs, intr)
    finally:
        ops.CONV5X5_DGRAD_F32, ops.CONV5X5_DGRAD_F32_MIN_N = old
        ops.conv5x5_dgrad_f32 = inner
    assert sorted(calls) == [128, 192], calls                      # both layers took the own kernel, once each
    e_pose = float((out - base_out).abs().max() / base_out.abs().max())
    cs = {k: float(torch.dot(g[k], base_g[k]) / (g[k].norm() * base_g[k].norm()).clamp_min(1e-300)) for k in g}
    print("whole step: pose %.3e, min cosine %.6f" % (e_pose, min(cs.values())))
    report("conv5x5_dgrad_whole_step", pose=e_pose, min_cos=min(cs.values()))
    assert bool(torch.isfinite(out).all()) and e_pose < 2e-4 and all(c >= 0.9999 for c in cs.values()), (e_pose, cs)
