#!/usr/bin/env python
"""Sub-pixel disparities on the Teddy pair (tests/golden/teddy_pair.npz) by band refinement: the
whole-pixel solve of both views as examples/example_consistency.py runs it, then two band levels around each map --
+-1 pixel in steps of 1/4, then +-1/4 in steps of 1/16 -- each a 9-label TRW-S problem built on the device.

    python examples/example_subpixel.py [--disparities 60] [--maxiter 30] [--refine-iters 0] [--save out.npz]

Prints, for the whole-pixel maps and after each level: TRW-S energy and bound of the pass, the reference model's
energy of the left map (set_disparity + update_energy on one dispmap_ncc, so that all passes are measured in one energy
function), and the share of pixels of both views that the left-right check finds consistent at tolerance 1.0 and 0.5.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = (np.arange(-4, 5) / 4.0, np.arange(-4, 5) / 16.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--disparities", type=int, default=60)
    ap.add_argument("--maxiter", type=int, default=30)
    ap.add_argument("--refine-iters", type=int, default=0)
    ap.add_argument("--save", help="write the maps of every pass of both views to this .npz")
    args = ap.parse_args()
    import stereo_amd
    g = np.load(os.path.join(ROOT, "tests", "golden", "teddy_pair.npz"))
    images = [g["im0"].astype(np.float64), g["im1"].astype(np.float64)]
    disparities = np.arange(args.disparities, dtype=np.float64)
    t0 = time.perf_counter()
    out = stereo_amd.solve_pair_ncc(images, disparities, 1, 40.0, 8.0, args.maxiter, 1e-4, check_tol=0.5,
                                    refine_iters=args.refine_iters, band_levels=LEVELS)
    seconds = time.perf_counter() - t0
    model = stereo_amd.dispmap_ncc(images, disparities, 1, 40.0, 8.0)
    names = ["whole pixels"] + (["occlusion refine"] if args.refine_iters > 0 else []) + \
            ["level %d (%+g .. %+g by %g)" % (i + 1, l[0], l[-1], l[1] - l[0]) for i, l in enumerate(LEVELS)]
    for p, name in enumerate(names):
        model.set_disparity(out.left.maps[p])
        print("%-32s left: TRW-S energy %.4f bound %.4f after %d iterations; model energy of the map %.4f"
              % (name, out.left.energy[p], out.left.lower_bound[p], out.left.iterations[p], model.energy()))
        for tol in (1.0, 0.5):
            shares = []
            for ref, other, direction in ((out.left, out.right, 1), (out.right, out.left, -1)):
                status, _ = stereo_amd.lr_check(ref.maps[p], other.maps[p], direction, tol)
                shares.append(float(np.mean(status == 0)))
            print("%-32s consistent at tolerance %.1f: left %.4f right %.4f" % ("", tol, shares[0], shares[1]))
    off_grid = float(np.mean(out.left.dispmap != np.rint(out.left.dispmap)))
    print("share of left pixels off the whole-pixel grid after the levels: %.4f" % off_grid)
    print("stage times: " + "  ".join("%s %.3f s" % kv for kv in out.times.items()))
    print("end to end (both views, volumes to filled sub-pixel maps): %.3f s" % seconds)
    if args.save:
        np.savez_compressed(args.save, **{"%s_pass%d" % (name, p): m for name, view in (("left", out.left), ("right", out.right))
                                          for p, m in enumerate(view.maps)})


if __name__ == "__main__":
    main()
