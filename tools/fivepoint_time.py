#!/usr/bin/env python3
"""Time rp_five_point_consensus next to rp_eight_point_consensus on the same inputs.

    python tools/fivepoint_time.py [--reps 30] [--warmup 5] [--out profiles/fivepoint_time.txt]

At n = 64 and P = 576 and 1728 (a third of the matches replaced by noise, the scenes of tools/consensus_time.py): the five-point
consensus at M = 256 and at M = 1024 against the eight-point consensus at M = 1024.  After `warmup` calls of the same shape every one
of `reps` calls is timed by a pair of device events of its own; the median is what is quoted, the minimum and the maximum show the
spread.  Also printed: the valid roots per sample (the scoring work grows with it) and the inlier share of the two winners.  No target
is fixed in advance.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(64, 576), (64, 1728)]
TAU, SEED = 0.01, 1


def timed(fn, warmup, reps):
    """milliseconds per call: (median, min, max) over `reps` calls, each between two device events, behind `warmup` calls"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        ms.append(start.elapsed_time(stop))
    return statistics.median(ms), min(ms), max(ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fivepoint_time needs a GPU")
    from rel_pose_amd import consensus, fivepoint
    from tools.eightpoint_time import scenes
    result = {"reps": args.reps, "warmup": args.warmup, "tau": TAU, "seed": SEED, "device": torch.cuda.get_device_name(0), "rows": []}
    for n, P in SHAPES:
        x1, x2, w = (t.cuda() for t in scenes(n, P))
        x2[:, ::3] = torch.rand_like(x2[:, ::3]) * 1.2 - 0.6                         # a third of the matches wrong
        tau = torch.full((n,), TAU, device="cuda")
        row = {"n": n, "P": P}
        for name, fn, M in (("rp_five_point_consensus", fivepoint.five_point_consensus, 256),
                            ("rp_five_point_consensus", fivepoint.five_point_consensus, 1024),
                            ("rp_eight_point_consensus", consensus.eight_point_consensus, 1024)):
            med, lo, hi = timed(lambda: fn(x1, x2, w, tau=tau, hypotheses=M, seed=SEED, return_weights=True), args.warmup, args.reps)
            out = fn(x1, x2, w, tau=tau, hypotheses=M, seed=SEED)
            key = "%s_M%d" % (name, M)
            row[key + "_ms"] = {"median": med, "min": lo, "max": hi}
            row[key + "_valid_per_sample"] = float(out.stat[:, 2].mean()) / M
            row[key + "_inlier_share"] = float(out.stat[:, 1].mean())
        row["five_M1024_over_eight_M1024"] = row["rp_five_point_consensus_M1024_ms"]["median"] / row["rp_eight_point_consensus_M1024_ms"]["median"]
        row["five_M256_over_eight_M1024"] = row["rp_five_point_consensus_M256_ms"]["median"] / row["rp_eight_point_consensus_M1024_ms"]["median"]
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        if args.out:                                               # (after every shape: what is measured is kept)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(result, indent=1) + "\n")
    return result


if __name__ == "__main__":
    main()
