#!/usr/bin/env python3
"""Time rp_eight_point next to what a user would otherwise write on the same device.

    python tools/eightpoint_time.py [--n 64] [--P 1728] [--calls 100] [--rounds 3] [--out profiles/eightpoint_time.txt]

For iters = 0 and 4: device events around `calls` back-to-back calls of rel_pose_amd.eightpoint.eight_point (after a warm-up of the same
shape), alternating with the baselines on the same weighted, normalised row matrices A [n,P,9], for the same number of solves
(iters + 1 per call):
    torch.linalg.svd(A, full_matrices=False)         the null vector as the last row of Vh -- the counterpart in accuracy
    torch.linalg.eigh(A^T A)                         the normal equations: cheaper, and what fp32 cannot afford
The baselines only decompose: they leave out the normalisation, the projection and the re-weighting that the kernel's time includes.
`rounds` repetitions of the whole comparison show the spread.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scenes(n, P, seed=0):
    """random two-view geometry, float32 on the CPU: x1, x2 [n,P,2], w [n,P]"""
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.eye(3, dtype=torch.float64) + 0.2 * torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    R = q * torch.sign(torch.linalg.det(q))[:, None, None]
    t = torch.randn(n, 1, 3, generator=g, dtype=torch.float64)
    xy = torch.rand(n, P, 2, generator=g, dtype=torch.float64) * 1.1 - 0.55
    z = torch.rand(n, P, 1, generator=g, dtype=torch.float64) * 6 + 4
    X2 = torch.cat([xy * z, z], -1) @ R.transpose(1, 2) + t
    x2 = X2[..., :2] / X2[..., 2:] + 1e-3 * torch.randn(n, P, 2, generator=g, dtype=torch.float64)
    return xy.float(), x2.float(), torch.rand(n, P, generator=g) * 0.95 + 0.05


def row_matrices(x1, x2, w):
    """the weighted, Hartley-normalised rows sqrt(w) (x2h (x) x1h), [n,P,9] (plain torch)"""
    def norm(x):
        c = (w[..., None] * x).sum(1, keepdim=True) / w.sum(1)[:, None, None]
        m = (w * (x - c).norm(dim=-1)).sum(1) / w.sum(1)
        return (x - c) * (2 ** 0.5 / m)[:, None, None]
    a, b = norm(x1), norm(x2)
    one = torch.ones_like(a[..., :1])
    return w.sqrt()[..., None] * (torch.cat([b, one], -1)[..., :, None] * torch.cat([a, one], -1)[..., None, :]).flatten(-2)


def timed(fn, calls):
    """milliseconds per call: device events around `calls` calls, behind one warm-up call and a synchronise"""
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
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--P", type=int, default=1728)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline_seconds", type=float, default=4.0, help="cap of one baseline measurement (fewer calls, never fewer than 3)")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eightpoint_time needs a GPU")
    from rel_pose_amd import eightpoint
    x1, x2, w = (t.cuda() for t in scenes(args.n, args.P))
    tau = torch.full((args.n,), 0.01, device="cuda")
    A = row_matrices(x1, x2, w).contiguous()
    result = {"n": args.n, "P": args.P, "calls": args.calls, "device": torch.cuda.get_device_name(0), "rows": []}
    for iters in (0, 4):
        solves = iters + 1

        def own():
            eightpoint.eight_point(x1, x2, w, tau=tau, iters=iters)

        def svd():
            for _ in range(solves):
                torch.linalg.svd(A, full_matrices=False)

        def eigh():
            for _ in range(solves):
                torch.linalg.eigh(A.transpose(1, 2) @ A)
        for rnd in range(args.rounds):
            row = {"iters": iters, "solves": solves, "round": rnd, "rp_eight_point_ms": timed(own, args.calls)}
            for name, fn in (("torch_svd_ms", svd), ("torch_gram_eigh_ms", eigh)):
                try:
                    once = timed(fn, 1)
                    calls = int(max(3, min(args.calls, args.baseline_seconds * 1e3 / max(once, 1e-3))))
                    row[name], row[name.replace("_ms", "_calls")] = timed(fn, calls), calls
                except RuntimeError as e:                      # (a solver library that is not there: said, not hidden)
                    row[name] = "failed: " + str(e).splitlines()[0]
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
    # the timed call does solve the problem: the root of the median Sampson distance is at the scale of the noise put in (1e-3)
    from rel_pose_amd import readout
    E = eightpoint.eight_point(x1, x2, w).E
    result["sqrt_median_sampson_of_own_E"] = float(readout.sampson_distance(E, x1, x2).median().sqrt())
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return result


if __name__ == "__main__":
    main()
