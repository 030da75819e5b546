#!/usr/bin/env python
"""The image pyramid against the full-size solve on the Teddy and Baby2 pairs (tests/golden), DESIGN.md 6.4: both views
solved coarse to fine (solve_pair_ncc_pyramid) and at full size (solve_pair_ncc) in the same run with the same
iteration budget per solve (max_relgap 0: every solve runs `--maxiter` iterations).

    python examples/example_pyramid.py [--levels 2] [--maxiter 30] [--expand guided] [--kernel 1] [--drop-slice]

Per pair and method it prints the wall time per stage, the kernel family of every solve (TrwsPlan.path(): 2 is the
K <= 64 Pipe family), the energy of the final left map in the full-size model (one dispmap_ncc, set_disparity +
update_energy), the share of consistent pixels at check tolerances 0.5 and 1.0, and the share of pixels where the two
methods' left maps differ by more than 1.  --drop-slice leaves out the coarsest level's last slice where that level has
65 (one past the Pipe family), as a caller who wants the coarse solve in that family would.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = (("teddy", "teddy_pair.npz", 60), ("baby2", "baby2_pair.npz", 86))
UNARY_WEIGHT, TOL = 40.0, 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=2)
    ap.add_argument("--maxiter", type=int, default=30)
    ap.add_argument("--expand", default="guided")
    ap.add_argument("--kernel", type=int, default=1)
    ap.add_argument("--drop-slice", action="store_true")
    args = ap.parse_args()
    import stereo_amd
    from stereo_amd import pyramid
    s = 1 << args.levels
    for name, file, D in PAIRS:
        g = np.load(os.path.join(ROOT, "tests", "golden", file))
        images = [g["im0"].astype(np.float64), g["im1"].astype(np.float64)]
        H, W = images[0].shape[:2]
        disparities = np.arange(D, dtype=np.float64)
        if args.drop_slice and pyramid.level_disparities(disparities, args.levels).shape[0] == 65:
            disparities = disparities[:s * 63 + 1]
        print("%s %d x %d, %d disparities, kernel %d, unary weight %g, tol %g, %d iterations per solve, %d reductions, expand %s"
              % (name, H, W, disparities.shape[0], args.kernel, UNARY_WEIGHT, TOL, args.maxiter, args.levels, args.expand))
        solve_args = (images, disparities, args.kernel, UNARY_WEIGHT, TOL)
        stereo_amd.solve_pair_ncc_pyramid(*solve_args, args.levels, 1, 0.0, expand=args.expand)      # warm-up: code objects
        t0 = time.perf_counter()
        pyr = stereo_amd.solve_pair_ncc_pyramid(*solve_args, args.levels, args.maxiter, 0.0, expand=args.expand)
        t_pyr = time.perf_counter() - t0
        t0 = time.perf_counter()
        full = stereo_amd.solve_pair_ncc(*solve_args, args.maxiter, 0.0)
        t_full = time.perf_counter() - t0

        print("  pyramid: %.3f s in all;  " % t_pyr + "  ".join("%s %.3f s" % kv for kv in pyr.times.items()))
        for l in range(args.levels, -1, -1):
            res = pyr.levels[l]
            h, w = res.left.dispmap.shape
            print("    level %d, %d x %d, %d slices, tol %g, edge weight %g, families %s: " % (
                l, h, w, pyr.disparities[l].shape[0], pyr.tol[l], pyr.smooth_weight[l], res.left.paths)
                + "  ".join("%s %.3f s" % kv for kv in res.times.items()))
            print("      left: energy %s  bound %s  iterations %s" % (
                ["%.3f" % e for e in res.left.energy], ["%.3f" % b for b in res.left.lower_bound], [int(i) for i in res.left.iterations]))
            if l < args.levels:
                share = np.bincount(res.left.expand_source.reshape(-1) + 1, minlength=5) / float(h * w)
                print("      left: expansion's source -1, 0 .. 3: " + " ".join("%.3f" % v for v in share))
        print("  full size: %.3f s in all, family %s;  " % (t_full, full.left.paths) + "  ".join("%s %.3f s" % kv for kv in full.times.items()))
        print("    left: energy %.3f  bound %.3f  iterations %d" % (full.left.energy[0], full.left.lower_bound[0], full.left.iterations[0]))

        dm = stereo_amd.dispmap_ncc(images, disparities, args.kernel, UNARY_WEIGHT, TOL)
        for what, result in (("pyramid", pyr), ("full size", full)):
            dm.set_disparity(result.left.dispmap)
            dm.update_energy()
            line = "  %-9s left map in the full-size model: energy %.3f" % (what, dm.energy())
            for tol in (0.5, 1.0):
                status, _ = stereo_amd.lr_check(result.left.dispmap, result.right.dispmap, 1, tol)
                line += ";  consistent at %.1f: %.4f" % (tol, float((status == 0).mean()))
            print(line)
        diff = np.abs(pyr.left.dispmap - full.left.dispmap)
        print("  left maps differ by more than 1 at %.4f of the pixels, by more than 2 (the band's half-width) at %.4f; median |difference| %.3f"
              % (float((diff > 1.0).mean()), float((diff > 2.0).mean()), float(np.median(diff))))


if __name__ == "__main__":
    main()
