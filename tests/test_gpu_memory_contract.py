"""The memory contract of the C ABI on a real MI355X: where every entry point writes, and that it writes all of its output.

tests/test_gpu_kernels.py checks VALUES; its outputs come from torch.empty, whose caching allocator hands back the block the
previous identical call just freed -- with the right answer already in it -- and nothing there reads the memory next to an output.
This module calls every case of tests/_contract_cases.py straight through the ctypes binding, twice (outputs and workspaces
pre-filled with a NaN sentinel, then with a finite pattern), every operand between guard bands, and asserts

  guards intact          every guard band bit-identical afterwards (operand name + first offset reported);
  untouched intact       gap columns of a strided output, the other thirds of a shared dqkv: bit-identical;
  full coverage          no pre-fill pattern left in the documented written region (documented zero padding exactly zero);
  inputs unchanged       every `const` operand bit-identical to its clone;
  no stale dependence    the two runs' outputs bit-identical;
  workspace honesty      exactly the bytes the *_workspace_bytes function reports; one float less raises RP_EWORKSPACE (an argument
                         check before any launch);
  strides                a split-layout case equals its packed-layout sibling bit for bit;
  values                 where the case carries an fp64 reference: the bound of that kernel's own parity test.

No test here provokes a fault: every stray write these checks can see lands in memory the test owns.  The second half runs whole
model steps with torch.empty / torch.empty_like / ops._empty poisoned (wrappers, workspaces and caches included)."""
import os

import pytest
import torch

from tests import _contract_cases as CC
from tests.test_gpu_kernels import report as _kernel_report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_ALL = [b for name in sorted(CC.CASES) for b in CC.CASES[name]]


def report(line):
    """one line of measured facts into the report file the other GPU tests append to"""
    _kernel_report(line)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from rel_pose_amd import _lib
    return _lib.load()


def _first(mask):
    return int(mask.reshape(-1).nonzero()[0])


def run_case(lib, builder, finite, probe=False):
    """one guarded call of the case; returns (violations, {window: device tensor}, case, operands).  probe: where the case has one,
    first repeat the call with one float less of workspace_bytes -- it must be refused"""
    import ctypes
    c = builder()
    ops_ = list(c.operands) + (c.late(lib) if hasattr(c, "late") else [])
    dev = torch.device("cuda")
    A = {o.name: o.alloc(dev, finite) for o in ops_}
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = []
    if probe and c.ws_probe is not None and (not hasattr(c, "has_workspace") or c.has_workspace()):
        with pytest.raises(RuntimeError, match="workspace too small"):
            c.ws_probe(lib, A, st)
    c.call(lib, A, st)
    torch.cuda.synchronize()
    vals = {}
    for o in ops_:
        s = CC.SENTINEL[o.dtype]
        lo, hi = o.arena[:o.guard] != s, o.arena[o.guard + o.n:] != s
        if bool(lo.any()):
            bad.append("%s: guard below the operand overwritten, first at element %d" % (o.name, _first(lo) - o.guard))
        if bool(hi.any()):
            bad.append("%s: guard above the operand overwritten, first at element %d past its end" % (o.name, _first(hi)))
        if o.role == "in":
            ne = o.region != o.before
            if bool(ne.any()):
                bad.append("%s: const operand modified, first at element %d" % (o.name, _first(ne)))
        elif o.role == "inout":
            vals[o.name] = o.logical(0, o.ld)
        elif o.role == "out":
            r2 = o.region.view(o.rows, o.ld)
            written = torch.zeros(o.rows, o.ld, dtype=torch.bool, device=dev)
            for c0, c1 in o.wins.values():
                written[:, c0:c1] = True
            stale = (r2 == o.fill) & written
            if bool(stale.any()):
                i = _first(stale)
                bad.append("%s: %d documented output elements never written, first at row %d col %d"
                           % (o.name, int(stale.sum()), i // o.ld, i % o.ld))
            touched = (r2 != o.fill) & ~written
            if bool(touched.any()):
                i = _first(touched)
                bad.append("%s: %d elements outside the documented region written, first at row %d col %d"
                           % (o.name, int(touched.sum()), i // o.ld, i % o.ld))
            for w, (c0, c1) in o.wins.items():
                vals[w] = o.logical(c0, c1)
    return bad, vals, c, ops_


@pytest.mark.parametrize("builder", _ALL, ids=["%s[%s]" % (b.entry, b.ident) for b in _ALL])
def test_memory_contract(lib, builder):
    bad_a, va, c, ops_ = run_case(lib, builder, finite=False, probe=True)
    bad_b, vb, _, _ = run_case(lib, builder, finite=True)
    bad = ["NaN-fill run: " + b for b in bad_a] + ["finite-fill run: " + b for b in bad_b]
    for w in va:
        bits = CC._BITS[va[w].dtype]
        if not torch.equal(va[w].view(bits), vb[w].view(bits)):
            ne = va[w].view(bits) != vb[w].view(bits)
            bad.append("%s: result depends on what the output / workspace held before the call (%d elements differ, first at flat %d)"
                       % (w, int(ne.sum()), _first(ne)))
    if c.sibling is not None:          # same values, packed layout: same tiles, same order -> the same bits
        bad_p, vp, _, _ = run_case(lib, c.sibling, finite=False)
        bad += ["packed sibling: " + b for b in bad_p]
        for w in va:
            if w in vp and not torch.equal(va[w].view(CC._BITS[va[w].dtype]), vp[w].view(CC._BITS[vp[w].dtype])):
                bad.append("%s: the strided layout's result differs from the packed layout's" % w)
    errs = {}
    if c.check is not None and not bad_a:
        errs = c.check(va, bad) or {}
    report("memory_contract %s[%s]: %s%s" % (
        builder.entry, builder.ident,
        " ".join("%s(ld=%d,guard=%dB)" % (o.name, o.ld, o.guard * o.esize) for o in ops_ if o.role != "in"),
        "".join(" %s=%.3e" % kv for kv in errs.items())))
    assert not bad, "\n".join(bad)


# ================================================================================================ poisoned-allocator runs of the wrappers
# Every output and workspace of rel_pose_amd/ops.py comes from torch.empty / torch.empty_like / ops._empty; here those return poisoned
# memory (floating point: the NaN sentinel, then 12345.0; bytes 0xA5 / 0x5A) and the cached workspaces are dropped, so a whole model
# step runs with NO stale right answer anywhere.  Output and every parameter gradient must be finite, free of the pattern, and the
# same bits as an unpoisoned run.
class _Poison:
    def __init__(self, monkeypatch):
        from rel_pose_amd import ops
        self.ops, self.mode, self.count = ops, None, 0
        self.empty, self.empty_like = torch.empty, torch.empty_like
        monkeypatch.setattr(torch, "empty", lambda *a, **k: self._fill(self.empty(*a, **k)))
        monkeypatch.setattr(torch, "empty_like", lambda *a, **k: self._fill(self.empty_like(*a, **k)))
        monkeypatch.setattr(ops, "_empty", lambda *shape, like: self._fill(self.empty(shape, device=like.device, dtype=torch.float32)))

    def _fill(self, t):
        if self.mode is None or not t.is_cuda or t.numel() == 0:
            return t
        if t.dtype in (torch.float32, torch.bfloat16, torch.float64):
            t.view(CC._BITS[t.dtype]).fill_((CC.SENTINEL if self.mode == "nan" else CC.FINITE)[t.dtype])
        elif t.dtype == torch.float16:
            t.fill_(float("nan") if self.mode == "nan" else 12345.0)
        elif t.dtype == torch.uint8:
            t.fill_(0xA5 if self.mode == "nan" else 0x5A)
        else:
            return t
        self.count += 1
        return t

    def set(self, mode):
        """None / "nan" / "finite"; drops every cached workspace so that it is allocated again under the new mode"""
        ops = self.ops
        for cache in (ops._WS_CACHE, ops._mlp_ws, ops._ARENA, ops._stats_ws, ops._ZEROS):
            cache.clear()
        ops.invalidate_pad_cache()
        torch.cuda.synchronize()
        self.mode = mode


@pytest.fixture
def poison(monkeypatch):
    p = _Poison(monkeypatch)
    yield p
    p.set(None)


def _same_under_poison(poison, step, tag, miopen=False, after=None):
    """step() -> {name: tensor}; unpoisoned, NaN-filled and finite-filled runs must agree bit for bit.
    miopen: the step goes through MIOpen (convolutions of the CNN front-end, the --noess head), whose solver choice and atomically
    accumulated weight gradients this project does not control: after a warm-up two unpoisoned runs decide -- bit-identical, and
    bit-identity is demanded under poison too; otherwise finite and pattern-free, and after(mode) (the existing test's comparison
    with its reference, run while the model still holds that step's gradients) must pass behind each poisoned step."""
    clone = lambda d: {k: v.detach().clone() for k, v in d.items()}
    poison.set(None)
    same = True
    if miopen:
        step()
        first = clone(step())
    runs = {None: clone(step())}
    if miopen:
        same = all(torch.equal(first[k], runs[None][k]) for k in first)
        report("poisoned_allocator %s: two unpoisoned runs bit-identical=%s" % (tag, same))
    for mode in ("nan", "finite"):
        poison.set(mode)
        before = poison.count
        runs[mode] = clone(step())
        torch.cuda.synchronize()
        # the fixture must have taken effect: a step allocates dozens of outputs and workspaces through the patched functions
        assert poison.count - before >= 10, "only %d allocations of this step were poisoned" % (poison.count - before)
        if after is not None and not same:
            poison.mode = None
            after(mode)
    poison.set(None)
    bad = []
    for mode in ("nan", "finite"):
        for k, v in runs[mode].items():
            if not bool(torch.isfinite(v).all()):
                bad.append("%s fill: %s is not finite (%d elements)" % (mode, k, int((~torch.isfinite(v)).sum())))
            elif mode == "finite" and bool((v == 12345.0).any()):
                bad.append("finite fill: %s holds the fill pattern" % k)
            elif same and not torch.equal(v, runs[None][k]):
                bad.append("%s fill: %s differs from the unpoisoned run (max |diff| %.3e)" % (mode, k, float((v - runs[None][k]).abs().max())))
    report("poisoned_allocator %s: tensors=%d violations=%d" % (tag, len(runs[None]), len(bad)))
    assert len(runs[None]) > 0 and not bad, "\n".join(bad[:20])
    return runs, same


def _grads(m, extra):
    d = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    d.update(extra)
    return d


def _model(**flags):
    from rel_pose_amd.model import ViTEss
    from oracle import relpose_oracle as O
    from tests.test_gpu_model import make_args
    a = make_args()
    a.__dict__.update(flags)
    shapes = dict(O.vit_param_shapes(noess=bool(a.noess)))
    shapes.update(O.cnn_param_shapes())
    m = ViTEss(a)
    m.load_state_dict(O.make_state(shapes, torch.float32), strict=True)
    return m.cuda()


def _token_step(m, B, train, key=None):
    """the test_odd_batch_sizes_fwd_bwd setup: tokens in, <pose, cot> backward"""
    from oracle import relpose_oracle as O
    tok = O.synthetic_tokens(2 * B, key=key if key is not None else 300 + B)
    Gs = torch.tensor([0, 0, 0, 0, 0, 0, 1.0]).repeat(B, 2, 1).cuda()
    intr = torch.tensor([[30.0, 26.0, 12.0, 11.0]]).repeat(B, 2, 1).contiguous().cuda()
    cot = O.closed_form((B, 2, 7), 77, 1.0, dtype=torch.float64).float().cuda()

    def step():
        m.train(train)
        for p in m.parameters():
            p.grad = None
        fmap = tok.permute(0, 2, 1).contiguous().view(2 * B, 192, 24, 24).cuda().requires_grad_(train)
        if not train:
            with torch.no_grad():
                return {"pose": m.forward_tokens(fmap, Gs, intr)}
        out = m.forward_tokens(fmap, Gs, intr)
        (out * cot).sum().backward()
        return _grads(m, {"pose": out, "grad_tokens": fmap.grad})
    return step


@pytest.mark.parametrize("B", [1, 3])
def test_poisoned_training_step_from_tokens(poison, B):
    m = _model()
    try:
        _same_under_poison(poison, _token_step(m, B, True), "train_tokens[B=%d]" % B)
    finally:
        m.eval()


def test_poisoned_inference_forward(poison):
    _same_under_poison(poison, _token_step(_model().eval(), 2, False), "inference_tokens[B=2]")


@pytest.mark.parametrize("train", [False, True])
def test_poisoned_noess_model(poison, train):
    """--noess: the pool_attn head is two 1x1 nn.Conv2d + BatchNorm through MIOpen, not through this library.  Bit-identity with the
    unpoisoned run is therefore demanded only when two warmed-up unpoisoned runs are themselves bit-identical (the MIOpen rule of
    _same_under_poison, which the images-in test uses too): MIOpen's first call of a shape may pick another solver than later
    calls, and the first measured run differed from later ones by 4e-7 in the pose with nothing poisoned.  Otherwise: finite,
    pattern-free, and within the existing test's bounds of the reference; the setup, the reference (the real reference's fp64 golden outputs) and the bounds are test_noess_fwd_bwd_vs_reference's."""
    import numpy as np
    from oracle import relpose_oracle as O
    from tests import test_gpu_model as TM
    golden = np.load(os.path.join(ROOT, "tests", "golden", "reference_outputs_noess.npz"))
    m, tag = TM._noess_model(train), "train" if train else "eval"
    tok = O.synthetic_tokens(4)
    Gs = torch.tensor([0, 0, 0, 0, 0, 0, 1.0]).repeat(2, 2, 1).cuda()
    cot = O.closed_form((2, 7), 993, 1.0, dtype=torch.float64).float().cuda()
    bn = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    last = {}

    def step():
        m.load_state_dict(bn, strict=False)
        for p in m.parameters():
            p.grad = None
        fmap = tok.permute(0, 2, 1).contiguous().view(4, 192, 24, 24).cuda().requires_grad_(True)
        pose = m.forward_tokens(fmap, Gs, TM.intr24().cuda())
        (pose[:, 1] * cot).sum().backward()
        last["pose"], last["fmap"] = pose, fmap
        return _grads(m, {"pose": pose, "grad_tokens": fmap.grad})

    def after(mode):
        t_err, q_err, _ = O.pose_errors(last["pose"].detach().cpu(), torch.from_numpy(golden["noess_pose_from_tokens_%s_f64" % tag]))
        e_g = TM.rel(last["fmap"].grad.view(4, 192, 576).permute(0, 2, 1).reshape(-1)[::37], golden["noess_grad_tokens_sub_%s_f64" % tag])
        ca, errs = m.fusion_transformer.blocks[5].cross_attn, []
        for i, w in enumerate([ca.qkv.weight, ca.proj.weight, m.pool_attn[0].weight, m.pool_attn[4].weight, m.pose_regressor[0].weight]):
            g = w.grad.double().reshape(-1).cpu()
            r = golden["noess_grad_sums_%s_f64" % tag][i]
            errs.append(max(float(np.abs(g[:16].numpy() - r[3:]).max() / np.abs(r[3:]).max()), abs(float(g.abs().sum()) - r[1]) / r[1]))
        report("poisoned_allocator noess[%s] %s fill vs reference: t=%.3e q=%.3e grad_tokens=%.3e grad_params=%.3e"
               % (tag, mode, t_err, q_err, e_g, max(errs)))
        assert max(t_err, q_err) < 1e-4 and e_g < 2.5e-5 and max(errs) < 6e-5
    _same_under_poison(poison, step, "noess[%s]" % tag, miopen=True, after=after)


@pytest.mark.parametrize("tag", ["l1", "single", "cross", "all3"])
def test_poisoned_ablation_variants(poison, tag):
    from tests.test_gpu_model import VARIANTS
    _same_under_poison(poison, _token_step(_model(**VARIANTS[tag]), 2, True), "variant_" + tag)


def _bf16_configuration(on):
    from rel_pose_amd import ops
    ops.set_gemm_precision(1 if on else 0)
    ops.set_attention_precision(1 if on else 0)
    ops.set_cnn_precision(1 if on else 0)


@pytest.mark.parametrize("B", [2, 3])
def test_poisoned_bf16_configuration_from_tokens(poison, B):
    """the bf16 data path (rp_attn_*_bf16, rp_emm_*_bf16, rp_dx_lnbwd_bf16, the io_bf16 forms of the Linear / MLP kernels): the entry
    points tests/_contract_cases.py lists as UNCOVERED are reached here"""
    m = _model()
    _bf16_configuration(True)
    try:
        _same_under_poison(poison, _token_step(m, B, True), "bf16_train_tokens[B=%d]" % B)
    finally:
        _bf16_configuration(False)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_poisoned_training_step_images_in(poison, precision):
    """Images in: the CNN front-end goes through MIOpen, whose weight gradients may be accumulated atomically.  Two unpoisoned runs decide:
    bit-identical -> bit-identity is demanded under poison as well; otherwise finite, pattern-free and, in the exact-fp32 configuration,
    every trainable tensor within test_end_to_end_backward_images_in_vs_oracle's bounds of the fp64 oracle (its own comparison, run
    behind each poisoned step).  The bf16 configuration has no oracle bound for this batch: there the contract itself -- finite,
    pattern-free -- is what is asserted when MIOpen does not repeat itself, and the difference to the unpoisoned run is reported."""
    from oracle import relpose_oracle as O
    from rel_pose_amd.se3 import SE3
    B, H, W = 2, 384, 384
    m = _model()
    imgs = O.synthetic_images(B, H, W, key=77).cuda()
    intr = torch.tensor([[0.9 * W, 0.8 * W, W / 2.0, H / 2.0]]).repeat(B, 2, 1).contiguous().cuda()
    Gs = torch.tensor([0, 0, 0, 0, 0, 0, 1.0]).repeat(B, 2, 1).cuda()
    cot = O.closed_form((B, 2, 7), 7117, 1.0, dtype=torch.float64).float().cuda()
    bn = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}

    def step():
        m.load_state_dict(bn, strict=False)
        m.train()
        for p in m.parameters():
            p.grad = None
        out = m(imgs, SE3(Gs), intrinsics=intr.clone())[0].data
        (out * cot).sum().backward()
        last["pose"] = out
        return _grads(m, {"pose": out})
    after, last = None, {}
    if precision == "fp32":
        from tests import test_gpu_model as TM
        oracle = {}

        def after(mode):
            if not oracle:          # (only needed when MIOpen does not repeat itself: two CPU runs of the whole oracle)
                shapes = dict(O.vit_param_shapes())
                shapes.update(O.cnn_param_shapes())
                sd32, sd64 = O.make_state(shapes, torch.float32), O.make_state(shapes, torch.float64)
                ci, cg, cc = imgs.cpu(), Gs.cpu(), cot.double().cpu()
                oracle["f64"], oracle["pose"] = TM._e2e_oracle_grads(sd64, ci.double(), cg, intr.cpu(), cc, True)
                oracle["f32"] = TM._e2e_oracle_grads(sd32, ci, cg, intr.cpu(), cc, True)[0]
            t_err, q_err, _ = O.pose_errors(last["pose"].detach().cpu(), oracle["pose"])
            assert max(t_err, q_err) < 1e-4, (mode, t_err, q_err)
            TM._compare_all_trainable(m, oracle["f64"], oracle["f32"], 1.0, "poisoned_images_in_%s_fill" % mode)
    _bf16_configuration(precision == "bf16")
    try:
        runs, same = _same_under_poison(poison, step, "images_in[%s]" % precision, miopen=True, after=after)
        if not same:      # (the pose goes through no atomically accumulated sum: report how far the runs are apart)
            worst = max(float((runs[mode]["pose"] - runs[None]["pose"]).abs().max() / runs[None]["pose"].abs().max()) for mode in ("nan", "finite"))
            report("poisoned_allocator images_in[%s]: pose, worst relative difference to the unpoisoned run %.3e" % (precision, worst))
    finally:
        _bf16_configuration(False)
        m.eval()
