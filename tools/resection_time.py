#!/usr/bin/env python3
"""Time the two entry points of include/relpose_resection.h next to the rotation library's, in the same run.

    python tools/resection_time.py [--reps 100] [--warmup 10] [--out profiles/resection_time.txt]

At (n, P, M) = (10, 576, 256) and (128, 1728, 256), three-view scenes with noise 1e-3 and a third of the images replaced by noise:
rp_p3p_consensus and rp_pnp_refine (10 iterations, from the consensus winner); alongside, on the same row counts, rp_rotation_consensus
and rp_rotation_refine (10 iterations, from ITS winner) -- they are the comparison, not their recorded figures.

WHERE THE TIME GOES.  A lane of the hypothesis kernel does two things: the fp64 three-point solver, whose cost does not depend on P, and
the walk over the K rows with four running sums.  The ablation the tool offers needs no second build: `solver_only` is the same call on
the first THREE rows of every problem (K = 3: the walk is three rows long, the staging is one round), and `cost_loop` is the difference
to the full call.  After `warmup` calls of the same shape every one of `reps` calls is timed by a pair of device events of its own; the
median is what is quoted, the minimum and the maximum show the spread.  No ratio is promised: what comes out is recorded.  Needs a GPU;
there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(10, 576, 256), (128, 1728, 256)]
TAU, SEED = 0.012, 1


def scenes(n, P, seed=0):
    """float32 on the CPU: points at depth 3 - 9 in front of the hub, a camera rotated by 0.2 rad and moved by 0.5 - 2; the images with
    Gaussian noise 1e-3; also the images under the rotation alone (the rotation library's input)"""
    import torch
    g = torch.Generator().manual_seed(seed)
    axis = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
    k = torch.zeros(n, 3, 3, dtype=torch.float64)
    k[:, 0, 1], k[:, 0, 2], k[:, 1, 0], k[:, 1, 2], k[:, 2, 0], k[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    R = torch.eye(3, dtype=torch.float64) + 0.19866933 * k + (1 - 0.98006658) * (k @ k)
    t = torch.nn.functional.normalize(torch.randn(n, 1, 3, generator=g, dtype=torch.float64), dim=-1) * (torch.rand(n, 1, 1, generator=g, dtype=torch.float64) * 1.5 + 0.5)
    xy = torch.rand(n, P, 2, generator=g, dtype=torch.float64) * 0.576 - 0.288
    X = torch.cat([xy, torch.ones(n, P, 1, dtype=torch.float64)], -1) * (torch.rand(n, P, 1, generator=g, dtype=torch.float64) * 6 + 3)
    m = X @ R.transpose(1, 2) + t
    x = m[..., :2] / m[..., 2:] + 1e-3 * torch.randn(n, P, 2, generator=g, dtype=torch.float64)
    r = torch.cat([xy, torch.ones(n, P, 1, dtype=torch.float64)], -1) @ R.transpose(1, 2)
    return X.float(), x.float(), xy.float(), (r[..., :2] / r[..., 2:]).float(), torch.rand(n, P, generator=g) * 0.95 + 0.05


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("resection_time needs a GPU")
    from rel_pose_amd import resection, rotation
    from tools.fivepoint_time import timed
    result = {"reps": args.reps, "warmup": args.warmup, "tau": TAU, "seed": SEED, "device": torch.cuda.get_device_name(0), "rows": []}
    for n, P, M in SHAPES:
        X, x, x1, x2, w = (t.cuda() for t in scenes(n, P))
        x[:, ::3] = torch.rand_like(x[:, ::3]) * 0.576 - 0.288                       # a third of the images wrong
        x2[:, ::3] = torch.rand_like(x2[:, ::3]) * 0.576 - 0.288
        tau = torch.full((n,), TAU, device="cuda")
        X3, x3, w3 = X[:, :3].contiguous(), x[:, :3].contiguous(), w[:, :3].contiguous()
        c = resection.p3p_consensus(X, x, w, tau=tau, hypotheses=M, seed=SEED)
        r = resection.pnp_refine(X, x, w, c.pose, tau=tau, iters=10)
        rc = rotation.rotation_consensus(x1, x2, w, tau=tau, hypotheses=M, seed=SEED)
        rr = rotation.rotation_refine(x1, x2, w, rc.R, tau=tau, iters=10)
        row = {"n": n, "P": P, "M": M}
        for name, fn in (("rp_p3p_consensus", lambda: resection.p3p_consensus(X, x, w, tau=tau, hypotheses=M, seed=SEED, return_weights=True)),
                         ("rp_p3p_consensus_solver_only", lambda: resection.p3p_consensus(X3, x3, w3, tau=tau, hypotheses=M, seed=SEED, return_weights=True)),
                         ("rp_pnp_refine_10", lambda: resection.pnp_refine(X, x, w, c.pose, tau=tau, iters=10, return_weights=True)),
                         ("rp_rotation_consensus", lambda: rotation.rotation_consensus(x1, x2, w, tau=tau, hypotheses=M, seed=SEED, return_weights=True)),
                         ("rp_rotation_refine_10", lambda: rotation.rotation_refine(x1, x2, w, rc.R, tau=tau, iters=10, return_weights=True))):
            med, lo, hi = timed(fn, args.warmup, args.reps)
            row[name + "_ms"] = {"median": med, "min": lo, "max": hi}
        row["rp_p3p_consensus_cost_loop_ms"] = row["rp_p3p_consensus_ms"]["median"] - row["rp_p3p_consensus_solver_only_ms"]["median"]
        row["p3p_over_rotation_consensus"] = row["rp_p3p_consensus_ms"]["median"] / row["rp_rotation_consensus_ms"]["median"]
        row["pnp_over_rotation_refine_10"] = row["rp_pnp_refine_10_ms"]["median"] / row["rp_rotation_refine_10_ms"]["median"]
        row["resection_inlier_share"], row["rotation_inlier_share"] = float(r.stat[:, 1].mean()), float(rr.stat[:, 1].mean())
        row["mean_solutions_per_sample"] = float(c.hyp_count.float().mean())
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        if args.out:                                                   # (after every shape: what is measured is kept)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(result, indent=1) + "\n")
    return result


if __name__ == "__main__":
    main()
