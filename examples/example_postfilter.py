#!/usr/bin/env python
"""The map filter after check and fill on the Teddy pair (tests/golden/teddy_pair.npz).

    python examples/example_postfilter.py [--disparities 60] [--maxiter 30] [--record out.txt]

Two solves of both views -- (a) solve_pair_ncc, --maxiter iterations, and (b) solve_pair_ncc_scanline alone, 8 directions
-- each checked at tolerance 1 and filled; then, for r = 1, 2 and 4, unguided and guided by the view's own image under
Contrast(2, 0.5, 8, 40), MedianFilter(r) on each view's filled map: only the consistent pixels vote, only the others are
rewritten.  Per solve, filter and view:
  changed      the share of all pixels whose value the filter changed, and the share of the targets
  kept         targets whose window held no voter (they keep the row fill's value)
  energy       scanline.model_energy of the filled and of the filtered map (both lie on the label grid: the filter selects,
               it does not average) under the solve's own model, uniform edge weights 1
and per solve and filter the share of pixels found consistent when the two FILTERED maps are cross-checked against each
other at tolerance 1, next to the same figure for the two filled maps.

There is no ground truth here: the figures are model energy and left-right consistency, not accuracy.  A lower energy
or a higher consistency after the filter says the filtered map is smoother and agrees more with the other view's, not that
it is nearer to the truth.  The output is kept as profiles/map_filter_example.txt; nothing in it is asserted anywhere."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GUIDE = (2.0, 0.5, 8.0, 40.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--disparities", type=int, default=60)
    ap.add_argument("--maxiter", type=int, default=30)
    ap.add_argument("--record", help="write the printed lines to this file")
    args = ap.parse_args()
    import stereo_amd
    from stereo_amd import Contrast, MedianFilter, consistency, scanline, terms as T
    g = np.load(os.path.join(ROOT, "tests", "golden", "teddy_pair.npz"))
    images = [g["im0"].astype(np.float64), g["im1"].astype(np.float64)]
    H, W = images[0].shape[:2]
    disparities = np.arange(args.disparities, dtype=np.float64)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say("example_postfilter.py --disparities %d --maxiter %d   (Teddy, %d x %d; model energy and consistency, not accuracy: "
        "there is no ground truth here)" % (args.disparities, args.maxiter, H, W))
    volumes = consistency.pair_volumes(images, disparities)
    unaries = consistency.pair_unaries(images, disparities, 40.0, volumes)
    conn = T.construct_neighborhood(H, W)
    labels_of = lambda m: np.rint(m).astype(np.int64).T.reshape(-1) + 1             # (disparities are 0 .. D - 1)
    energy = lambda u, m: scanline.model_energy(u, conn, 1.0, disparities, 1, 8.0, labels_of(m))
    solves = [
        ("(a) solve_pair_ncc, %d iterations" % args.maxiter,
         lambda: stereo_amd.solve_pair_ncc(images, disparities, 1, 40.0, 8.0, args.maxiter, 0.0, check_tol=1.0, volumes=volumes)),
        ("(b) solve_pair_ncc_scanline, 8 directions",
         lambda: scanline.solve_pair_ncc_scanline(images, disparities, 1, 40.0, 8.0, check_tol=1.0, volumes=volumes)),
    ]
    for name, run in solves:
        out = run()
        both = [float(np.mean(consistency.lr_check(a.filled, b.filled, s, 1.0, want_residual=False)[0] == 0))
                for a, b, s in ((out.left, out.right, 1), (out.right, out.left, -1))]
        say("%s: targets (status != 0) left %.4f right %.4f of the pixels; filled maps cross-checked: consistent left %.4f right %.4f"
            % (name, np.mean(out.left.status != 0), np.mean(out.right.status != 0), both[0], both[1]))
        for r in (1, 2, 4):
            for guide in (None, Contrast(*GUIDE)):
                f = MedianFilter(r, guide)
                t0 = time.perf_counter()
                res = [f.apply(view.filled, view.status, im) for view, im in zip(out.views, images)]
                seconds = time.perf_counter() - t0
                cross = [float(np.mean(consistency.lr_check(res[i][0], res[1 - i][0], s, 1.0, want_residual=False)[0] == 0))
                         for i, s in ((0, 1), (1, -1))]
                for side, view, u, (filtered, source, kept) in zip(("left", "right"), out.views, unaries, res):
                    changed = filtered != view.filled
                    targets = view.status != 0
                    assert not changed[~targets].any()
                    say("  r = %d %-8s %-5s changed %.4f of the pixels, %.4f of the targets; kept %5d; energy filled %.2f -> "
                        "filtered %.2f" % (r, "guided" if guide else "unguided", side, changed.mean(),
                                           changed[targets].mean() if targets.any() else 0.0, kept, energy(u, view.filled),
                                           energy(u, filtered)))
                say("  r = %d %-8s filtered maps cross-checked: consistent left %.4f right %.4f; both views filtered in %.3f s "
                    "(host arrays, uploads included)" % (r, "guided" if guide else "unguided", cross[0], cross[1], seconds))
    if args.record:
        with open(args.record, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
