#!/usr/bin/env python3
"""Time rp_emm_guided_matches (include/relpose_guided.h) next to what it stands beside.

    python tools/guided_time.py [--reps 30] [--warmup 5] [--out profiles/guided_time.txt]

At (Z, H) = (128, 3) and (12, 3), on standard-normal q | k at scale 0.125 with the normalisers of rp_emm_stats and the fundamental
matrix of a built scene (tests/_guided_ref.py): rp_emm_guided_matches at band 1.5 and 1e9 (every pair admitted), rows and columns,
beside rp_emm_matches from the unchanged readout library on the same inputs -- the same tiles, the same 33 MFMA steps; what is
added per score is the admission.  Then, on one pair of images through a randomly initialised model, the whole of
guided_pose_from_matches (prior given, and prior = "consensus") beside consensus_pose_from_matches.  After `warmup` calls of the same
shape every one of `reps` calls is timed by a pair of device events of its own; the median is what is quoted, the minimum and the
maximum show the spread.  No target is fixed in advance.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(128, 3), (12, 3)]
BANDS = [1.5, 1e9]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("guided_time needs a GPU")
    from oracle import relpose_oracle as O
    from rel_pose_amd import guided, ops, readout
    from tests import _guided_ref as G
    from tests import _submatch_ref as S
    from tests.test_gpu_memory_contract import _model
    from tools.fivepoint_time import timed
    result = {"reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "rows": [], "chains": {}}

    def save():
        if args.out:                                               # (after every row: what is measured is kept)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(result, indent=1) + "\n")
    F1 = G.grid_F(S.built_inputs(0)).reshape(3, 3)
    for Z, H in SHAPES:
        assert H == ops.HEADS
        qkv = (0.125 * torch.randn(Z * 576, 576, generator=torch.Generator().manual_seed(Z))).cuda()
        rlse, clse = ops.emm_stats(qkv, Z)
        F = torch.from_numpy(np.stack([F1.T.reshape(9), F1.reshape(9)] * (Z // 2)).astype(np.float32)).cuda()
        row = {"Z": Z, "H": H}
        for swap in (False, True):
            tag = "cols" if swap else "rows"
            med, lo, hi = timed(lambda: readout.emm_matches(qkv, rlse, clse, Z, swap=swap), args.warmup, args.reps)
            row["rp_emm_matches_%s_ms" % tag] = {"median": med, "min": lo, "max": hi}
            for band in BANDS:
                bd = torch.full((Z,), band, device="cuda")
                med, lo, hi = timed(lambda: guided.emm_guided_matches(qkv, rlse, clse, F, bd, Z, swap=swap), args.warmup, args.reps)
                row["rp_emm_guided_matches_%s_band%g_ms" % (tag, band)] = {"median": med, "min": lo, "max": hi}
                row["guided_over_matches_%s_band%g" % (tag, band)] = med / row["rp_emm_matches_%s_ms" % tag]["median"]
        idx, stat = guided.emm_guided_matches(qkv, rlse, clse, F, 1.5, Z)
        row["support_band1.5"], row["unmatched_band1.5"] = float(guided.support_of(stat).mean()), float((idx < 0).float().mean())
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        save()
    # the chains, one pair of 384 x 384 images through a randomly initialised model
    m = _model().eval()
    images = O.synthetic_images(1, 384, 384, key=78).cuda()
    intr = torch.tensor([[0.9 * 384, 0.8 * 384, 192.0, 192.0]]).repeat(1, 2, 1).contiguous().cuda()
    pose = m.consensus_pose_from_matches(images, intr).pose
    for name, fn in (("consensus_pose_from_matches", lambda: m.consensus_pose_from_matches(images, intr)),
                     ("guided_pose_from_matches_prior_given", lambda: m.guided_pose_from_matches(images, intr, prior=pose)),
                     ("guided_pose_from_matches_prior_consensus", lambda: m.guided_pose_from_matches(images, intr, prior="consensus")),
                     ("pose_support", lambda: m.pose_support(images, intr, pose)),
                     ("correspondences", lambda: m.correspondences(images))):
        med, lo, hi = timed(fn, args.warmup, args.reps)
        result["chains"][name + "_ms"] = {"median": med, "min": lo, "max": hi}
        print(json.dumps({name + "_ms": result["chains"][name + "_ms"]}), flush=True)
        save()
    return result


if __name__ == "__main__":
    main()
