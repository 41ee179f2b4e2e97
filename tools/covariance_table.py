#!/usr/bin/env python3
"""The CPU-side figures of DESIGN.md 5.13, from the committed reference tests/_covariance_ref.py (numpy, fp64; no GPU, no library).

    python tools/covariance_table.py --table [--trials 200]     the calibration of the sandwich covariance against sigma^2 H^-1
    python tools/covariance_table.py --constants                the worst errors of the float32 restatement over the GPU cases (x 8: the
                                                                constants of tests/test_gpu_covariance.py)
    python tools/covariance_table.py --seeds                    per GPU shape the first batch seed by the rules of the test

--table: every row is one geometry, one P, one share f of wrong matches and one tau / sigma; `trials` fresh draws of noise (sigma = 1e-3)
and wrong matches, refine_ref for 15 iterations from the true pose, the error of the result in the five parameters against the predicted
covariance.  Coverage: the share of draws whose squared Mahalanobis distance is below 11.07, the 95 % point of chi^2_5.  The rows that
tests/test_covariance_cpu.py asserts come first (with its 100 trials); the others are recorded, not asserted."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ASSERTED = [(g, 576, f, ts) for g in (1, 2) for f, ts in ((0.0, 10), (0.3, 10), (0.3, 3))]
RECORDED = ([(g, 576, 0.5, 10) for g in (1, 2, 3)] + [(3, 576, f, ts) for f, ts in ((0.0, 10), (0.3, 10), (0.3, 3))]
            + [(g, P, f, 10) for P in (128, 1728) for g in (1, 2) for f in (0.0, 0.3, 0.5)] + [(g, 576, 0.3, 30) for g in (1, 2)])


def table(trials):
    from tests import _covariance_ref as C
    print("| g | P | f | tau/sigma | trials | coverage | naive coverage | M2/5 | naive M2/5 | sd_rot pred / emp (deg) | sd_dir pred / emp (deg) | status -1 |")
    print("| --- | --- | --- | --- | --- | --- | --- | --- | --- | --- | --- | --- |")
    for rows, k in ((ASSERTED, 100), (RECORDED, trials)):
        for g, P, f, ts in rows:
            r = C.mc_run(g, P, C.SIGMA, f, ts, k)
            print("| %d | %d | %.1f | %d | %d | %.2f | %.2f | %.2f | %.1f | %.3f / %.3f | %.3f / %.3f | %.3f |"
                  % (g, P, f, ts, k, r["coverage"], r["coverage_naive"], r["m2_over_5"], r["m2_over_5_naive"], r["sd_rot_pred"], r["sd_rot_emp"],
                     r["sd_dir_pred"], r["sd_dir_emp"], r["not_determined"]), flush=True)


def batch_ok(C, n, P, seed):
    """the rules of tests/test_gpu_covariance.py for a batch seed, weighted and not: the float32 restatement and fp64 agree on status
    and on the count of negative rows, no row inside the window of u = 1, at least half of the problems with status 1 and a gap
    eig[0] / eig[1] >= GAP_MIN, and no weak vector whose two largest components are within 1 % of each other (the sign rule)"""
    import numpy as np
    for weighted in (False, True):
        a = C.gpu_case(n, P, weighted, seed)
        r64, r32 = C.covariance_ref(*a), C.covariance_f32(*a)
        if not (r64.stat[:, 0] == r32.stat[:, 0]).all() or not (r64.stat[:, 5] == r32.stat[:, 5]).all() or C.window_rows(*a).any():
            return False
        good = (r64.stat[:, 0] == C.OK) & (r64.eig[:, 0] >= C.GAP_MIN * np.maximum(r64.eig[:, 1], 1e-300))
        if 2 * int(good.sum()) < n:
            return False
        mags = np.sort(np.abs(r64.weak[good]), -1)
        if (mags[:, -2] > 0.99 * mags[:, -1]).any():
            return False
    return True


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--constants", action="store_true")
    ap.add_argument("--seeds", action="store_true")
    ap.add_argument("--trials", type=int, default=200)
    args = ap.parse_args(argv)
    from tests import _covariance_ref as C
    if args.seeds:
        for n, P in C.GPU_SHAPES:
            print((n, P), next(s for s in range(100) if batch_ok(C, n, P, s)), flush=True)
    if args.constants:
        import numpy as np
        worst = np.zeros(5)
        for n, P, weighted in C.gpu_cases():
            a = C.gpu_case(n, P, weighted)
            e = C.gpu_errors(C.covariance_f32(*a), C.covariance_ref(*a))
            worst = np.maximum(worst, e)
            print((n, P, weighted), " ".join("%.4g" % v for v in e), flush=True)
        print("worst (normal, cov, eig, weak, cost): %s ; x 8: %s" % (" ".join("%.4g" % v for v in worst), " ".join("%.4g" % (8 * v) for v in worst)))
    if args.table:
        table(args.trials)


if __name__ == "__main__":
    main()
