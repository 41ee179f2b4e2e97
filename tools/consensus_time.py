#!/usr/bin/env python3
"""Time rp_eight_point_consensus next to rp_eight_point and next to what a user would otherwise write on the same device.

    python tools/consensus_time.py [--calls 100] [--rounds 3] [--trace DIR] [--out profiles/consensus_time.txt]

At (n, P, M) = (6, 576, 1024) and (64, 1728, 1024) -- the workload's size --: device events around `calls` back-to-back calls of
rel_pose_amd.consensus.eight_point_consensus (after a warm-up of the same shape), alternating with
    rel_pose_amd.eightpoint.eight_point(iters = 4)   the all-data solve the consensus is put in front of
    the torch composition of the same work on the same inputs and the same samples: gather, Hartley normalisation, batched
    torch.linalg.svd of the [n M, 8, 9] row matrices (full: the ninth right vector), F = T2^T F^ T1, a batched 3 x 3 SVD for the
    projection, the Sampson cost of every hypothesis against every row by broadcasting, argmin
`rounds` repetitions show the spread.  --trace DIR: first, in a child process of its own, `rocprofv3 --kernel-trace --stats` around a
few calls of the two entry points (kernel times; tracing slows the host, so the event timings are taken without it); the kernel rows
of its statistics are appended to the output; if that child does not end with 0 the tool stops there, before it touches the device
itself.  Needs a GPU; there is no fallback."""
import argparse
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(6, 576, 1024), (64, 1728, 1024)]           # the small one first: its rows are out before the large baseline starts
TAU, SEED = 0.01, 1


def trace(out_dir, calls):
    """kernel statistics of a few calls, from a fresh child under rocprofv3 (this process has not touched the device yet)"""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out_dir, "-o", "consensus", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--calls", str(calls), "--kernels_only"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    if r.returncode != 0:                                          # a child that failed on the device: nothing more is started on it
        raise SystemExit("consensus_time: the traced child ended with %d; stopping before this process touches the device\n%s"
                         % (r.returncode, r.stdout[-3000:]))
    rows = []
    for path in sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as fh:
            lines = fh.read().splitlines()
        rows += [lines[0]] + [ln for ln in lines[1:] if any(k in ln for k in ("hypothesis_kernel", "select_kernel", "eight_point_kernel"))]
    return {"command": " ".join(cmd[:cmd.index("--")]), "kernel_stats": rows or ["none found", r.stdout[-800:]]}


def torch_composition(x1, x2, w, tau, samples):
    """the work of rp_eight_point_consensus in plain torch -> (E [n,3,3], best [n], cost [n,M])"""
    import torch
    n, P = w.shape
    M = samples.shape[1]
    idx = samples.long().reshape(n, M * 8, 1).expand(-1, -1, 2)

    def norm(x):
        p = torch.gather(x, 1, idx).reshape(n, M, 8, 2)
        c = p.mean(2, keepdim=True)
        s = 2 ** 0.5 / (p - c).norm(dim=-1).mean(2)
        return (p - c) * s[..., None, None], s, c[:, :, 0]
    (a, s1, c1), (b, s2, c2) = norm(x1), norm(x2)
    one = torch.ones_like(a[..., :1])
    A = (torch.cat([b, one], -1)[..., :, None] * torch.cat([a, one], -1)[..., None, :]).flatten(-2).reshape(n * M, 8, 9)
    f = torch.linalg.svd(A, full_matrices=True).Vh[:, 8].reshape(n, M, 3, 3)

    def T(s, c):
        t = torch.zeros(n, M, 3, 3, device=s.device, dtype=s.dtype)
        t[..., 0, 0] = t[..., 1, 1] = s
        t[..., 0, 2], t[..., 1, 2], t[..., 2, 2] = -s * c[..., 0], -s * c[..., 1], 1
        return t
    F = T(s2, c2).transpose(-1, -2) @ f @ T(s1, c1)
    U, _, Vh = torch.linalg.svd(F)
    E = U[..., :2] @ Vh[..., :2, :]                                                  # [n,M,3,3]
    h1 = torch.cat([x1, torch.ones_like(x1[..., :1])], -1)                           # [n,P,3]
    h2 = torch.cat([x2, torch.ones_like(x2[..., :1])], -1)
    l2 = torch.einsum("nmrc,npc->nmpr", E, h1)
    l1 = torch.einsum("nmrc,npr->nmpc", E, h2)
    r = (l2 * h2[:, None]).sum(-1)
    d = r * r / (l2[..., 0] ** 2 + l2[..., 1] ** 2 + l1[..., 0] ** 2 + l1[..., 1] ** 2)
    t2 = (tau * tau)[:, None, None]
    cost = (w[:, None] * t2 * torch.log1p(d / t2)).sum(-1) / w.sum(-1, keepdim=True)
    best = cost.argmin(-1)
    return E[torch.arange(n, device=E.device), best], best, cost


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
    ap.add_argument("--baseline_seconds", type=float, default=4.0, help="cap of one baseline measurement (fewer calls; a single timed call where three would not fit)")
    ap.add_argument("--trace", default="", metavar="DIR", help="first run rocprofv3 --kernel-trace --stats in a child of its own, output under DIR")
    ap.add_argument("--trace_calls", type=int, default=5)
    ap.add_argument("--kernels_only", action="store_true", help="(the traced child) only the two entry points, no baselines, no output file")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    result = {"calls": args.calls, "tau": TAU, "seed": SEED, "rows": []}
    if args.trace:
        result["rocprofv3"] = trace(args.trace, args.trace_calls)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("consensus_time needs a GPU")
    from rel_pose_amd import consensus, eightpoint
    from tools.eightpoint_time import scenes
    result["device"] = torch.cuda.get_device_name(0)
    for n, P, M in SHAPES:
        x1, x2, w = (t.cuda() for t in scenes(n, P))
        x2[:, ::3] = torch.rand_like(x2[:, ::3]) * 1.2 - 0.6                         # a third of the matches wrong
        tau = torch.full((n,), TAU, device="cuda")
        first = consensus.eight_point_consensus(x1, x2, w, tau=tau, hypotheses=M, seed=SEED, return_samples=True)

        def own():
            consensus.eight_point_consensus(x1, x2, w, tau=tau, hypotheses=M, seed=SEED, return_weights=True)

        def all_data():
            eightpoint.eight_point(x1, x2, w, tau=tau, iters=4)

        def composed():
            torch_composition(x1, x2, w, tau, first.samples)
        if args.kernels_only:
            timed(own, args.calls)
            timed(all_data, args.calls)
            continue
        for rnd in range(args.rounds):
            row = {"n": n, "P": P, "M": M, "round": rnd, "rp_eight_point_consensus_ms": timed(own, args.calls),
                   "rp_eight_point_iters4_ms": timed(all_data, args.calls)}
            try:
                once = timed(composed, 1)
                calls = int(min(args.calls, args.baseline_seconds * 1e3 / max(once, 1e-3)))
                row["torch_composition_ms"], row["torch_composition_calls"] = (timed(composed, calls), calls) if calls >= 3 else (once, 1)
                row["torch_over_own"] = row["torch_composition_ms"] / row["rp_eight_point_consensus_ms"]
            except RuntimeError as e:                              # (a solver library that is not there: said, not hidden)
                row["torch_composition_ms"] = "failed: " + str(e).splitlines()[0]
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
        # the two compute the same thing: the composition's best cost against the kernel's, and the residuals per second the kernel scores
        try:
            _, _, cost = torch_composition(x1, x2, w, tau, first.samples)
            result["n%d_best_cost_own_vs_torch" % n] = [float(first.stat[:, 0].max()), float(cost.min(-1).values.max()),
                                                        float((first.stat[:, 0] - cost.min(-1).values).abs().max())]
        except RuntimeError as e:
            result["n%d_best_cost_own_vs_torch" % n] = "failed: " + str(e).splitlines()[0]
        ms = min(r["rp_eight_point_consensus_ms"] for r in result["rows"] if r["n"] == n)
        result["n%d_sampson_residuals_per_second" % n] = n * M * float((w > 0).sum(-1).float().mean()) / (ms * 1e-3)
        if args.out:                                               # (after every shape: what is measured is kept)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))
    return result


if __name__ == "__main__":
    main()
