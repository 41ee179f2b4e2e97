"""Inputs, fp64 references, fp32 yardsticks and per-block metrics for the softmax-regime tests of the attention and Essential-Matrix-Module
kernels (csrc/attention.hip, csrc/emm.hip).  torch only, no GPU and no library at import: tests/test_softmax_regimes_cpu.py proves every
regime's condition and the gradient yardstick cap on the CPU, tests/test_gpu_softmax_regimes.py runs the kernels.

Regimes.  Each builder returns qkv [Z*576, 576] fp32 (q | k | v, head-major columns of 64) from a fixed seed.  pairing = "self" plants the
structure in q_z against k_z (plain attention, S_z = q_z k_z^T / 8); "cross" plants it in q_{z^1} against k_z (the EMM and the cross attention,
S_z = q_{z^1} k_z^T / 8).
  diffuse      randn: the control.  The largest probability of a row is about 0.02.
  sharp        q[i] = 1.5 k[pi(i)], another random permutation per (image, head): the matched score is 1.5 |k|^2 / 8 ~ 12 over a background
               of standard deviation 1.5, rows and columns: median top probability 0.99, 5 % quantile 0.8.
  onehot       the same with c = 4 (matched score ~ 32): every top probability >= 0.99.  Forward only: with P one-hot P (dP - delta) cancels to
               nothing and plain fp32 is itself wrong by 2e-3 .. 4e-3 per head.
  staircase    a unit vector u per head; 2 (index // 32) u added on the loop axis and 8 u on the other one: the score gains 2 per 32-wide tile
               over noise of standard deviation 1.4, so the running maximum of an online softmax moves at nearly every tile ("up") or sits in
               the first tile and every later tile is scaled far down ("down").  axis = "keys" drives the row-side online softmax, "queries"
               the 18 per-block column partials of rp_emm_stats.
  large(f)     head 0 of image 0: q times f, as tests/test_gpu_kernels.py::test_attention_stats_partner does -- which reaches max |s| = 190 at
               f = 40, not the 1e3 its comment names -- and k of that head in the first pair times LARGE_KEY_GAIN = 4: max |s| = 780 .. 920 at
               f = 40 (the condition is > 500), 160 .. 180 at f = 8, a near one-hot softmax in that head next to five diffuse ones.
  flat         q of image 0 zero, k of image 1 / head 1 zero: lse = ln 576 and o = the column mean of v there.

References (attn_ref, emm_ref) take the dtype to run in: fp64 is the reference, fp32 -- plain PyTorch, torch.softmax, no TF32 -- the YARDSTICK:
the error a straightforward fp32 implementation makes on the same input.  emm_ref follows oracle/relpose_oracle.py cross_attention (pinned to the
real reference, ablation flags included, by tests/test_oracle_golden.py).

Metrics.  block_rel: max |a - b| / max |b| inside each (image, head, 32-row block), the worst block and where it is -- an error confined to
one block, one head or one image of a pair is judged against that block's own values, not against the largest value anywhere.  head_rel: the same
per (image, head), for gradients and F.  lse_err: max over rows of |a - b| / max(1, |b|).

Bound rule.  An asserted error is compared with 8 x the yardstick's error on the same input under the same metric (bound()).  On the existing
attention input the kernels measure 1.3e-6 (o) and 3.3e-6 (dq) where plain fp32 makes 1.0e-6 and 0.9e-6: a ratio of up to 3.6 from another
summation order, up to 18 rescales and the hardware exponential; 8 leaves a factor of two over that.  An index, rescale, normaliser or
half-wave defect produces errors >= 1e-3.  The log-sum-exp's yardstick can be within an ulp of exact, so lse_err has the floor LSE_FLOOR.
One effect is the kernels' own and not the yardstick's -- the normaliser carried as an fp32 log-sum-exp -- and has a derived allowance per
element in the regimes where it shows ("the carried normaliser" below); every other regime and output keeps the plain rule."""
import functools
import math

import numpy as np
import torch

N_TOK, HEADS, HD = 576, 3, 64
SCALE = HD ** -0.5
EPS32 = 2.0 ** -23
FACTOR = 8.0
# lse = (m + log2(l)) ln 2 formed in fp32 has at least four roundings of up to half an ulp of the value each (the score the maximum came
# from, m + log2(l), the product with ln 2, the stored result) and the hardware logarithm's 1 ulp: 3 ulps, and one more for the sum l itself.
# In the metric's units (relative to max(1, |value|)) an ulp is at most 2^-23.
LSE_FLOOR = 4 * EPS32
GRAD_YARDSTICK_CAP = 2e-4


def bound(yard, floor=0.0):
    return max(FACTOR * yard, floor)


# ------------------------------------------------------------------------------------------------ inputs
def _randn(Z, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(Z, N_TOK, 3, HEADS, HD, generator=g), g


def _pack(t):
    return t.reshape(t.shape[0] * N_TOK, 3 * HEADS * HD).contiguous()


def diffuse(Z, pairing="self", seed=101):
    return _pack(_randn(Z, seed)[0])


@functools.lru_cache(maxsize=None)
def _planted(Z, c, pairing, seed):
    t, g = _randn(Z, seed)
    perm = torch.stack([torch.stack([torch.randperm(N_TOK, generator=g) for _ in range(HEADS)]) for _ in range(Z)])      # [Z,H,576]
    for z in range(Z):
        zq = z ^ 1 if pairing == "cross" else z
        for h in range(HEADS):
            t[zq, :, 0, h] = c * t[z, perm[z, h], 1, h]
    return _pack(t), perm


def sharp(Z, pairing="self", c=1.5, seed=102):
    """-> (qkv, perm [Z,H,576]): query i of problem z (its keys are image z's) is planted on key perm[z,h,i]"""
    qkv, perm = _planted(Z, float(c), pairing, seed)
    return qkv.clone(), perm


def onehot(Z, pairing="self", c=4.0, seed=103):
    qkv, perm = _planted(Z, float(c), pairing, seed)
    return qkv.clone(), perm


def staircase(Z, pairing="self", axis="keys", direction="up", seed=104):
    t, g = _randn(Z, seed)
    u = torch.randn(HEADS, HD, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    step = torch.arange(N_TOK) // 32
    if direction == "down":
        step = N_TOK // 32 - 1 - step
    ramp = 2.0 * step.float()[None, :, None, None] * u
    loop, other = (1, 0) if axis == "keys" else (0, 1)
    t[:, :, loop] += ramp
    t[:, :, other] += 8.0 * u
    return _pack(t)


LARGE_KEY_GAIN = 4.0


def large(Z, f, pairing="self", seed=105):
    t, _ = _randn(Z, seed)
    t[0, :, 0, 0] *= float(f)
    t[:2, :, 1, 0] *= LARGE_KEY_GAIN
    return _pack(t)


def flat(Z, pairing="self", seed=106):
    t, _ = _randn(Z, seed)
    t[0, :, 0] = 0.0
    t[1, :, 1, 1] = 0.0
    return _pack(t)


def build(name, Z, pairing):
    """regime by name -> (qkv, perm or None)"""
    if name == "diffuse":
        return diffuse(Z, pairing), None
    if name == "sharp":
        return sharp(Z, pairing)
    if name == "onehot":
        return onehot(Z, pairing)
    if name.startswith("staircase"):
        _, axis, direction = name.split("_")
        return staircase(Z, pairing, axis, direction), None
    if name.startswith("large"):
        return large(Z, int(name[5:]), pairing), None
    if name == "flat":
        return flat(Z, pairing), None
    raise KeyError(name)


FORWARD_SELF = ("diffuse", "sharp", "onehot", "staircase_keys_up", "staircase_keys_down", "large8", "large40", "flat")
GRADIENT_SELF = ("diffuse", "sharp", "staircase_keys_up", "large8", "large40", "flat")
FORWARD_CROSS = ("diffuse", "sharp", "onehot", "staircase_keys_up", "staircase_queries_up", "staircase_queries_down", "large8", "large40", "flat")
GRADIENT_CROSS = ("diffuse", "sharp", "staircase_keys_up", "staircase_queries_up", "large8", "large40", "flat")


def make_pos(Z):
    """positional features [Z/2, 576, 6] fp32 of Z/2 pairs with differing intrinsics (the oracle's closed form, on the CPU)"""
    from oracle import relpose_oracle as O
    rows = torch.tensor([[30.0, 26.0, 12.0, 12.0], [18.0, 21.0, 12.0, 9.0], [25.0, 25.0, 11.0, 13.0]])
    intr = rows[torch.arange(Z // 2) % 3][:, None, :].repeat(1, 2, 1)
    return O.positional_encodings(Z // 2, intr, torch.float32)


# ------------------------------------------------------------------------------------------------ references
def split(qkv, Z):
    """[Z*576, 576] -> q, k, v [Z,H,576,64]"""
    return qkv.view(Z, N_TOK, 3, HEADS, HD).permute(2, 0, 3, 1, 4)


def _partner(Z):
    return [z ^ 1 for z in range(Z)]


def scores(qkv, Z, pairing):
    q, k, _ = split(qkv, Z)
    return ((q[_partner(Z)] if pairing == "cross" else q) @ k.transpose(-1, -2)) * SCALE


def attn_ref(qkv, Z, kv_xor=0, dtype=torch.float64):
    """-> (o [Z*576,192], lse [Z,H,576], s [Z,H,576,576]); kv_xor = 1: keys and values of the partner image (vision_transformer.py:239-262)"""
    assert not torch.backends.cuda.matmul.allow_tf32
    q, k, v = split(qkv.to(dtype), Z)
    if kv_xor:
        k, v = k[_partner(Z)], v[_partner(Z)]
    s = (q @ k.transpose(-1, -2)) * SCALE
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(Z * N_TOK, HEADS * HD)
    return o, torch.logsumexp(s, -1), s


def emm_ref(qkv, pos, Z, single=False, cross=False, dtype=torch.float64):
    """-> (F [Z,H,70,70], T = A X, U = A^T X [Z,H,576,70], X, A) of problem z: S = q_{z^1} k_z^T / 8, A = softmax(S, -1) softmax(S, -2)
    (single: the row softmax only), X = [v | pos], F = X^T A X (cross: X[z^1]^T A X) -- oracle/relpose_oracle.py cross_attention"""
    assert not torch.backends.cuda.matmul.allow_tf32
    q, k, v = split(qkv.to(dtype), Z)
    s = (q[_partner(Z)] @ k.transpose(-1, -2)) * SCALE
    a = torch.softmax(s, -1) if single else torch.softmax(s, -1) * torch.softmax(s, -2)
    pe = pos.to(dtype)[[z // 2 for z in range(Z)]].unsqueeze(1).expand(Z, HEADS, N_TOK, 6)
    x = torch.cat([v, pe], dim=-1)
    T = a @ x
    xl = x[_partner(Z)] if cross else x
    return xl.transpose(-1, -2) @ T, T, a.transpose(-1, -2) @ x, x, a


def emm_stats_ref(qkv, Z, dtype=torch.float64):
    """-> (rlse, clse [Z,H,576], s [Z,H,576,576]) of S_z = q_{z^1} k_z^T / 8"""
    s = scores(qkv.to(dtype), Z, "cross")
    return torch.logsumexp(s, -1), torch.logsumexp(s, -2), s


def grads(fn, qkv, cot, Z, dtype):
    """autograd of sum(fn(qkv) * cot) in `dtype` -> (dq, dk, dv) [Z,H,576,64]"""
    x = qkv.detach().to(dtype, copy=True).requires_grad_(True)
    (fn(x) * cot.to(dtype)).sum().backward()
    return split_grad(x.grad, Z)


def cotangent(shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def split_grad(dqkv, Z):
    return tuple(t for t in split(dqkv, Z))


# ------------------------------------------------------------------------------------------------ metrics
def _worst(err, ref):
    ratio = err / ref.clamp_min(1e-300)
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), tuple(int(n) for n in np.unravel_index(i, tuple(ratio.shape)))


def block_max(t):
    """[Z,H,576,C] -> [Z,H,18]: largest magnitude inside each 32-row block"""
    return t.detach().abs().reshape(t.shape[0], t.shape[1], N_TOK // 32, -1).amax(-1)


def head_max(t):
    """[Z,H,...] -> [Z,H]"""
    return t.detach().abs().reshape(t.shape[0], t.shape[1], -1).amax(-1)


def block_cells(a, b):
    """-> (max |a - b|, max |b|) per (image, head, 32-row block), [Z,H,18] each"""
    a, b = a.detach().double(), b.detach().double().to(a.device)
    return block_max(a - b), block_max(b)


def head_cells(a, b):
    a, b = a.detach().double(), b.detach().double().to(a.device)
    return head_max(a - b), head_max(b)


def global_cells(a, b):
    """the global metric as one cell [1,1]"""
    a, b = a.detach().double(), b.detach().double().to(a.device)
    return (a - b).abs().max().reshape(1, 1), b.abs().max().reshape(1, 1)


CELLS = {"block": block_cells, "head": head_cells, "global": global_cells}


def spread(r, like, kind):
    """a per-cell quantity of `kind` broadcast to the elements of `like` ([Z,H,576,C]; head: [Z,H,...]; global: any)"""
    if kind == "block":
        return r.repeat_interleave(32, dim=2).reshape(*like.shape[:3], *([1] * (like.dim() - 3)))
    return r.reshape(*r.shape, *([1] * (like.dim() - 2))) if kind == "head" else r.reshape([1] * like.dim())


def worst(cells, limit=None):
    """cells = (err, ref) -> (largest err / ref, where); with `limit` (absolute, per cell): (largest err / limit, where)"""
    return _worst(cells[0], cells[1] if limit is None else limit)


def block_rel(a, b):
    """[Z,H,576,C]: max over (image, head, 32-row block) of max |a - b| / max |b| inside the block -> (worst, (image, head, block))"""
    return worst(block_cells(a, b))


def head_rel(a, b):
    """[Z,H,...]: max over (image, head) of max |a - b| / max |b| -> (worst, (image, head))"""
    return worst(head_cells(a, b))


def lse_err(a, b):
    """[Z,H,576]: max over rows of |a - b| / max(1, |b|) -> (worst, (image, head, row))"""
    a, b = a.detach().double(), b.detach().double().to(a.device)
    return _worst((a - b).abs(), b.abs().clamp_min(1.0))


def rel(a, b):
    """the global metric of tests/test_gpu_kernels.py"""
    return worst(global_cells(a, b))[0]


def heads_of(t, Z):
    """[Z*576, 192] -> [Z,H,576,64]"""
    return t.view(Z, N_TOK, HEADS, HD).permute(0, 2, 1, 3)


def top_probabilities(s):
    """largest probability of every row and of every column of softmax(s): ([Z,H,576], [Z,H,576])"""
    return torch.softmax(s, -1).amax(-1), torch.softmax(s, -2).amax(-2)


def running_max_increases(s, axis):
    """how often the running maximum over 32-wide tiles along the loop axis rises, per line: axis "keys" -> per row over key tiles,
    "queries" -> per column over query blocks.  [Z,H,576] of counts in 0..17"""
    if axis == "queries":
        s = s.transpose(-1, -2)
    m = s.reshape(*s.shape[:-1], N_TOK // 32, 32).amax(-1)
    run = torch.cummax(m, -1).values
    return (run[..., 1:] > run[..., :-1]).sum(-1)


LN_NTOK = math.log(N_TOK)


# ------------------------------------------------------------------------------------------------ the carried normaliser
# The yardstick DIVIDES by the sum of exponentials: a probability near 1 is exact to eps32 whatever the size of the scores.  The kernels carry
# the normaliser as an fp32 log-sum-exp and form every probability as exp2(s2 - lse2) (log2 units) -- in the forward's epilogue, in every
# backward pass, in rp_emm_apply and rp_emm_grad.  The exponent has the roundings of s2 (1 ulp of |s2| for the accumulated dot product and the
# scale folded into an operand), of the stored lse (1/2) and of its product with log2 e (1/2): 2 ulps of max(|s2|, |lse2|), so every
# probability has the relative error  eps_c = 2 eps32 max(|s|, |lse|)  (natural units; ln 2 turns the log2 ulps into them) -- 7.6e-6 at
# |lse| = 32 (`onehot`), 1.9e-4 at 800 (`large40`), where the yardstick makes 3e-7.  The dual softmax A = P_row P_col has two such exponents
# (rp_emm_grad: eo el) or one of twice the size (rp_emm_apply: 2 s2 - rlse2 - clse2): 2 eps_c.  Each pass has its own instance of the error: the
# rho / gamma sums come from the T and U that rp_emm_apply left, the softmax factors they are subtracted from in dS = 2 A dA - P_row rho -
# P_col gamma are formed anew in rp_emm_grad -- where autograd reuses ONE stored softmax and its cancellation is exact.  A form that
# recomputes q k^T per pass with the scale on another operand has another ulp of |s2| between its passes: twice eps_c again.
# In the regimes where the largest probabilities are near 1 AND the exponents are large (CARRIED) this, not the summation order, is the
# kernels' error, so there the bound is  8 x yardstick + eps_c x (first-order sensitivity of the output to a relative error of every
# probability), the sensitivity computed in fp64 from the reference (attn_sensitivity, emm_sensitivity), for the outputs that miss the plain rule
# there: the stored probabilities and dv of the attention, T / U / F and the gradients of the EMM.  Every other regime keeps the plain
# 8 x rule.  (An index, rescale or normaliser defect is >= 1e-3 of the block; the largest allowance, `large40`, is 2e-4 x sensitivity.)
CARRIED = ("onehot", "large8", "large40")


def carried_eps(*ts):
    """eps_c per (image, head) [Z,H] from the fp64 scores and log-sum-exps of the problem"""
    return 2 * EPS32 * torch.stack([head_max(t) for t in ts]).amax(0)


def attn_sensitivity(qkv, do, Z, kv_xor=0):
    """fp64 first-order allowances of plain attention: (eps_c [Z,H], P, P^T |do| [Z,H,576,64] -- dv's, on the image the values came from)"""
    q, k, v = split(qkv.double(), Z)
    if kv_xor:
        k, v = k[_partner(Z)], v[_partner(Z)]
    s = (q @ k.transpose(-1, -2)) * SCALE
    P = torch.softmax(s, -1)
    eps = carried_eps(s, torch.logsumexp(s, -1))
    sdv = P.transpose(-1, -2) @ heads_of(do.double(), Z).abs()
    return eps, P, sdv[_partner(Z)] if kv_xor else sdv


def emm_sensitivity(qkv, pos, cot, Z, single=False, cross=False, recomputed=False):
    """fp64 allowances (absolute, eps_c folded in) of the EMM of emm_ref: dict of T, U [Z,H,576,70], F [Z,H,70,70] and, with the cotangent
    `cot` of F, dq, dk, dv [Z,H,576,64] on the images the gradients belong to.  With A' = A (1 + e), |e| <= eps = (1 or 2) eps_c:
      T = A X, U = A^T X_L, F = X_L^T A X      ->  eps A |X|, eps A^T |X_L|, eps |X_L|^T A |X|
      dS = 2 A dA - P_row rho - P_col gamma     ->  eps (2 A |dA| + P_row R + P_col G),  R_i = sum_j A |dA|, G_j = sum_i A |dA|
                                                    (single: dS = A (dA - rho) -> eps (A |dA| + A R)); dq = dS k / 8, dk = dS^T q / 8
      dX = U dF (+ T dF^T for the left operand) ->  eps ((A^T |X_L|) |dF| + (A |X|) |dF|^T); dv = its first 64 columns
    recomputed: the forms that recompute the scores in every pass, twice the eps in the gradients."""
    q, k, v = split(qkv.double(), Z)
    par = _partner(Z)
    qp = q[par]
    s = (qp @ k.transpose(-1, -2)) * SCALE
    prow = torch.softmax(s, -1)
    pcol = torch.ones_like(prow) if single else torch.softmax(s, -2)
    eps = carried_eps(s, torch.logsumexp(s, -1), torch.logsumexp(s, -2))[..., None, None] * (1 if single else 2)
    A = prow * pcol if not single else prow
    pe = pos.double()[[z // 2 for z in range(Z)]].unsqueeze(1).expand(Z, HEADS, N_TOK, 6)
    x = torch.cat([v, pe], dim=-1)
    xl = x[par] if cross else x
    AX, AtXl = A @ x.abs(), A.transpose(-1, -2) @ xl.abs()
    out = dict(T=eps * AX, U=eps * (A.transpose(-1, -2) @ x.abs()), F=eps * (xl.abs().transpose(-1, -2) @ AX))
    if cot is None:
        return out
    dF = cot.double().to(x.device)
    eg = eps * (2 if recomputed else 1)
    AdA = A * ((xl @ dF) @ x.transpose(-1, -2)).abs()
    R, G = AdA.sum(-1, keepdim=True), AdA.sum(-2, keepdim=True)
    dS = eg * (AdA + A * R if single else 2 * AdA + prow * R + pcol * G)
    out["dq"] = ((dS @ k.abs()) * SCALE)[par]                    # the queries are the partner image's
    out["dk"] = (dS.transpose(-1, -2) @ qp.abs()) * SCALE
    dxl, dx = eg * (AX @ dF.abs().transpose(-1, -2)), eg * (AtXl @ dF.abs())
    out["dv"] = (dx + (dxl[par] if cross else dxl))[..., :HD]
    return out
