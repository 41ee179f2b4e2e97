#!/usr/bin/env python3
"""Time rp_emm_submatch next to rp_emm_matches and next to what a user would otherwise write on the same device.

    python tools/submatch_time.py [--calls 100] [--rounds 3] [--out profiles/submatch_time.txt]

At Z = 128 and Z = 12 images with H = 3 heads (packed qkv rows of random values at the scale of the model's, dual softmax, radius 2 and
1): device events around `calls` back-to-back calls of rel_pose_amd.readout.emm_submatch (after a warm-up of the same shape), alternating
with
    rel_pose_amd.readout.emm_matches          the readout whose argmax it localises, on the same inputs (a pass over all 576 x 576 scores)
    the torch composition of the same work    gather of the window's rows by index, the batched dot products, exp, the sums and the vertex
`rounds` repetitions show the spread.  The bytes and multiply-adds per call are computed from the shapes: every owner gathers (2 radius +
1)^2 rows of 256 bytes (fewer at the borders) and reads its own.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [12, 128]
GRID, TOK, HEADS, HD = 24, 576, 3, 64


def torch_composition(qkv, rlse, clse, idx, Z, radius):
    """rp_emm_submatch (swap = 0, dual softmax, valid centres) in plain torch -> (win, quad) [Z,3,576,4]"""
    import torch
    W = 2 * radius + 1
    q = qkv[:, :HEADS * HD].view(Z // 2, 2, TOK, HEADS, HD).flip(1).reshape(Z, TOK, HEADS, HD).permute(0, 2, 1, 3)      # rows: the partner's q
    k = qkv[:, HEADS * HD:2 * HEADS * HD].view(Z, TOK, HEADS, HD).permute(0, 2, 1, 3)                                      # [Z,3,576,64]
    d = torch.arange(W, device=qkv.device) - radius
    x0, y0 = (idx % GRID).long(), (idx // GRID).long()
    x, y = torch.broadcast_tensors(x0[..., None, None] + d[None, :], y0[..., None, None] + d[:, None])                     # [Z,3,576,W,W]
    live = ((x >= 0) & (x < GRID) & (y >= 0) & (y < GRID)).flatten(-2)
    n = (y.clamp(0, GRID - 1) * GRID + x.clamp(0, GRID - 1)).flatten(-2)                                                    # [Z,3,576,W*W]
    rows = torch.gather(k[:, :, None].expand(-1, -1, TOK, -1, -1), 3, n[..., None].expand(-1, -1, -1, -1, HD))            # [Z,3,576,W*W,64]
    e = 2 * HD ** -0.5 * (rows * q[..., None, :]).sum(-1) - rlse[..., None] - torch.gather(clse[:, :, None].expand(-1, -1, TOK, -1), 3, n)
    e = e.masked_fill(~live, float("-inf"))
    u = (e - e.max(-1, keepdim=True).values).exp()
    su = u.sum(-1)
    fx, fy = (x - x0[..., None, None]).flatten(-2).float(), (y - y0[..., None, None]).flatten(-2).float()
    mx, my = (u * fx).sum(-1) / su, (u * fy).sum(-1) / su
    var = (u * ((fx - mx[..., None]) ** 2 + (fy - my[..., None]) ** 2)).sum(-1) / su
    win = torch.stack([x0 + mx, y0 + my, e.exp().sum(-1), var], -1)
    c0 = radius * W + radius

    def vertex(a, b, c, both):
        curv = torch.where(both, (b - a) + (b - c), torch.zeros_like(b))
        off = torch.where(both & (curv > 0), (0.5 * (c - a) / curv).clamp(-0.5, 0.5), torch.zeros_like(b))
        return off, curv
    ox, cx = vertex(e[..., c0 - 1], e[..., c0], e[..., c0 + 1], (x0 > 0) & (x0 < GRID - 1))
    oy, cy = vertex(e[..., c0 - W], e[..., c0], e[..., c0 + W], (y0 > 0) & (y0 < GRID - 1))
    return win, torch.stack([x0 + ox, y0 + oy, cx, cy], -1)


def timed(fn, calls):
    """milliseconds per call: device events around `calls` calls, behind one warm-up call and a synchronise"""
    import torch
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / calls


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline_seconds", type=float, default=4.0, help="cap of one baseline measurement (fewer calls where 100 would not fit)")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("submatch_time needs a GPU")
    from rel_pose_amd import ops, readout
    result = {"calls": args.calls, "device": torch.cuda.get_device_name(0), "rows": []}
    for Z in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(Z)
        qkv = torch.randn(Z * TOK, 3 * HEADS * HD, device="cuda", generator=gen) * 0.5
        rlse, clse = ops.emm_stats(qkv, Z)
        idx, _, _ = readout.emm_matches(qkv, rlse, clse, Z)
        for radius in (2, 1):
            W = 2 * radius + 1
            x0, y0 = idx % GRID, idx // GRID
            span = lambda c: (c + radius).clamp(max=GRID - 1) - (c - radius).clamp(min=0) + 1          # noqa: E731
            slots = int((span(x0) * span(y0)).sum())
            macs, gathered = slots * HD, slots * (HD * 4 + 4) + Z * HEADS * TOK * (HD * 4 + 4 + 4 + 32)

            def own():
                readout.emm_submatch(qkv, rlse, clse, idx, Z, radius=radius)

            def matches():
                readout.emm_matches(qkv, rlse, clse, Z)

            def composed():
                torch_composition(qkv, rlse, clse, idx, Z, radius)
            for rnd in range(args.rounds):
                row = {"Z": Z, "H": HEADS, "radius": radius, "round": rnd, "window_slots": slots, "multiply_adds": macs,
                       "bytes_gathered_and_written": gathered, "rp_emm_submatch_ms": timed(own, args.calls),
                       "rp_emm_matches_ms": timed(matches, args.calls)}
                row["submatch_over_matches"] = row["rp_emm_submatch_ms"] / row["rp_emm_matches_ms"]
                row["gather_GB_per_s"] = gathered / (row["rp_emm_submatch_ms"] * 1e-3) / 1e9
                try:
                    once = timed(composed, 1)
                    calls = int(min(args.calls, args.baseline_seconds * 1e3 / max(once, 1e-3)))
                    row["torch_composition_ms"], row["torch_composition_calls"] = (timed(composed, calls), calls) if calls >= 3 else (once, 1)
                    row["torch_over_own"] = row["torch_composition_ms"] / row["rp_emm_submatch_ms"]
                except RuntimeError as e:                          # (out of memory at the large shape: said, not hidden)
                    row["torch_composition_ms"] = "failed: " + str(e).splitlines()[0]
                    torch.cuda.empty_cache()
                result["rows"].append(row)
                print(json.dumps(row), flush=True)
            # the two compute the same thing
            try:
                win, quad = readout.emm_submatch(qkv, rlse, clse, idx, Z, radius=radius)
                twin, tquad = torch_composition(qkv, rlse, clse, idx, Z, radius)
                result["Z%d_r%d_own_vs_torch" % (Z, radius)] = {"win_xy": float((win[..., :2] - twin[..., :2]).abs().max()),
                                                               "quad_xy": float((quad[..., :2] - tquad[..., :2]).abs().max())}
                del twin, tquad
            except RuntimeError as e:
                result["Z%d_r%d_own_vs_torch" % (Z, radius)] = "failed: " + str(e).splitlines()[0]
            torch.cuda.empty_cache()
            if args.out:                                           # (after every shape: what is measured is kept)
                with open(args.out, "w") as fh:
                    fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))
    return result


if __name__ == "__main__":
    main()
