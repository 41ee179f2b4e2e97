#!/usr/bin/env python3
"""Time rp_refine_pose next to the eight-point solve it follows, on the same device and the same matches.

    python tools/refine_time.py [--shapes 64x1728,6x576] [--iters 10] [--calls 100] [--rounds 3] [--out profiles/refine_time.txt]

For every shape n x P: device events around `calls` back-to-back calls (after a warm-up of the same shape) of
    rel_pose_amd.refine.refine_pose(iters = --iters)      about 2 barriers per iteration
    rel_pose_amd.refine.refine_pose(iters = 0)            the scorer
    rel_pose_amd.eightpoint.eight_point(iters = 0)        one solve: about 330 barriers
The start poses are the decoded eight-point poses of the same scenes.  `rounds` repetitions show the spread.  Each call is one kernel
(refine_pose_kernel, eight_point_kernel), so one `rocprofv3 --kernel-trace --stats -- python tools/refine_time.py --rounds 1` run gives
the kernels' own times next to these.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x1728,6x576")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("refine_time needs a GPU")
    from eightpoint_time import scenes, timed
    from rel_pose_amd import eightpoint, geom, refine
    result = {"iters": args.iters, "calls": args.calls, "device": torch.cuda.get_device_name(0), "rows": []}
    for shape in args.shapes.split(","):
        n, P = (int(v) for v in shape.split("x"))
        x1, x2, w = (t.cuda() for t in scenes(n, P))
        tau = torch.full((n,), 0.01, device="cuda")
        pose0, _ = geom.pose_from_essential(eightpoint.eight_point(x1, x2, w).E, x1, x2)
        for rnd in range(args.rounds):
            row = {"n": n, "P": P, "round": rnd,
                   "rp_refine_pose_ms": timed(lambda: refine.refine_pose(pose0, x1, x2, w, tau=tau, iters=args.iters), args.calls),
                   "rp_refine_pose_iters0_ms": timed(lambda: refine.refine_pose(pose0, x1, x2, w, tau=tau, iters=0), args.calls),
                   "rp_eight_point_iters0_ms": timed(lambda: eightpoint.eight_point(x1, x2, w), args.calls)}
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
        # the timed call does refine: the cost falls, and steps are accepted
        r = refine.refine_pose(pose0, x1, x2, w, tau=tau, iters=args.iters)
        result["%dx%d" % (n, P)] = {"cost_start_mean": float(r.stat[:, 0].mean()), "cost_end_mean": float(r.stat[:, 1].mean()),
                                    "accepted_mean": float(r.stat[:, 2].mean())}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return result


if __name__ == "__main__":
    main()
