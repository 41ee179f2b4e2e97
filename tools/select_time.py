#!/usr/bin/env python3
"""Time rp_model_select (include/relpose_select.h) next to the rotation library's scorer, in the same run.

    python tools/select_time.py [--reps 30] [--warmup 5] [--out profiles/select_time.txt]

At (n, P, C) = (10, 576, 5) and (128, 1728, 5), the pure-rotation scenes of tools/rotation_time.py with a third of the matches replaced
by noise and five candidates of the kinds of select.AUTO_KINDS derived from the rotation consensus winner: rp_model_select with and
without its optional outputs; alongside, on the same rows, rp_rotation_refine(iters = 0) -- one pass over the rows with one reduction,
the cheapest kernel of the same layout.  Then, on one pair of images through a randomly initialised model,
ViTEss.auto_pose_from_matches against the three chains it runs.  After `warmup` calls of the same shape every one of `reps` calls is
timed by a pair of device events of its own; the median is what is quoted, the minimum and the maximum show the spread.  No ratio is
promised: what comes out is recorded.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(10, 576, 5), (128, 1728, 5)]
TAU, SEED = 0.01, 1


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("select_time needs a GPU")
    from oracle import relpose_oracle as O
    from rel_pose_amd import rotation, select
    from tests.test_gpu_memory_contract import _model
    from tools.fivepoint_time import timed
    from tools.rotation_time import scenes
    result = {"reps": args.reps, "warmup": args.warmup, "tau": TAU, "seed": SEED, "device": torch.cuda.get_device_name(0), "rows": [], "chains": {}}

    def save():
        if args.out:                                                   # (after every shape: what is measured is kept)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(result, indent=1) + "\n")
    for n, P, C in SHAPES:
        x1, x2, w = (t.cuda() for t in scenes(n, P))
        x2[:, ::3] = torch.rand_like(x2[:, ::3]) * 1.2 - 0.6                         # a third of the matches wrong
        tau = torch.full((n,), TAU, device="cuda")
        R = rotation.rotation_consensus(x1, x2, w, tau=tau, hypotheses=256, seed=SEED).R
        g = torch.Generator(device="cuda").manual_seed(3)
        t = torch.nn.functional.normalize(torch.randn(n, 3, device="cuda", generator=g), dim=-1)
        tx = torch.zeros(n, 3, 3, device="cuda")
        tx[:, 0, 1], tx[:, 0, 2], tx[:, 1, 0], tx[:, 1, 2], tx[:, 2, 0], tx[:, 2, 1] = -t[:, 2], t[:, 1], t[:, 2], -t[:, 0], -t[:, 1], t[:, 0]
        E = tx @ R
        noise = lambda s: s * torch.randn(n, 3, 3, device="cuda", generator=g)      # noqa: E731
        models = torch.stack([E, E + noise(3e-3), E + noise(1e-2), R + noise(1e-3), R], 1).contiguous()
        s = select.model_select(x1, x2, w, models, select.AUTO_KINDS, tau=tau)
        row = {"n": n, "P": P, "C": C, "picks": s.pick.cpu().tolist()[:10], "sigma": float(s.scale[:, 0].mean())}
        for name, fn in (("rp_model_select", lambda: select.model_select(x1, x2, w, models, select.AUTO_KINDS, tau=tau)),
                         ("rp_model_select_all_outputs", lambda: select.model_select(x1, x2, w, models, select.AUTO_KINDS, tau=tau,
                                                                                     return_residuals=True, return_labels=True)),
                         ("rp_rotation_refine_0", lambda: rotation.rotation_refine(x1, x2, w, R, tau=tau, iters=0))):
            med, lo, hi = timed(fn, args.warmup, args.reps)
            row[name + "_ms"] = {"median": med, "min": lo, "max": hi}
        row["select_over_rotation_refine_0"] = row["rp_model_select_ms"]["median"] / row["rp_rotation_refine_0_ms"]["median"]
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        save()
    # the chains, one pair of 384 x 384 images through a randomly initialised model
    m = _model().eval()
    images = O.synthetic_images(1, 384, 384, key=78).cuda()
    intr = torch.tensor([[0.9 * 384, 0.8 * 384, 192.0, 192.0]]).repeat(1, 2, 1).contiguous().cuda()
    for name, fn in (("auto_pose_from_matches", lambda: m.auto_pose_from_matches(images, intr)),
                     ("consensus_pose_from_matches", lambda: m.consensus_pose_from_matches(images, intr)),
                     ("planar_pose_from_matches", lambda: m.planar_pose_from_matches(images, intr)),
                     ("rotation_from_matches", lambda: m.rotation_from_matches(images, intr))):
        med, lo, hi = timed(fn, args.warmup, args.reps)
        result["chains"][name + "_ms"] = {"median": med, "min": lo, "max": hi}
        print(json.dumps({name + "_ms": result["chains"][name + "_ms"]}), flush=True)
        save()
    return result


if __name__ == "__main__":
    main()
