#!/usr/bin/env python
"""Both views of the Teddy pair (tests/golden/teddy_pair.npz) with the left-right cross-check, the occlusion map and
the fill: two NCC volumes, two TRW-S problems in one batch, each map checked against the other.

    python examples/example_consistency.py [--disparities 60] [--maxiter 30] [--refine-iters 0] [--save out.npz]

Prints the share of pixels per status for both views and the time of each stage.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("consistent", "occluded", "mismatch", "out of view", "not finite")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--disparities", type=int, default=60)
    ap.add_argument("--maxiter", type=int, default=30)
    ap.add_argument("--refine-iters", type=int, default=0)
    ap.add_argument("--check-tol", type=float, default=1.0)
    ap.add_argument("--save", help="write maps, statuses and filled maps of both views to this .npz")
    args = ap.parse_args()
    import stereo_amd
    g = np.load(os.path.join(ROOT, "tests", "golden", "teddy_pair.npz"))
    images = [g["im0"].astype(np.float64), g["im1"].astype(np.float64)]
    disparities = np.arange(args.disparities, dtype=np.float64)
    out = stereo_amd.solve_pair_ncc(images, disparities, 1, 40.0, 8.0, args.maxiter, 1e-4, check_tol=args.check_tol,
                                    refine_iters=args.refine_iters)
    for name, view in (("left", out.left), ("right", out.right)):
        share = np.bincount(view.status.reshape(-1), minlength=5) / float(view.status.size)
        print("%-5s  " % name + "  ".join("%s %.4f" % (n, s) for n, s in zip(NAMES, share)))
        for p, (e, lb, it) in enumerate(zip(view.energy, view.lower_bound, view.iterations)):
            print("       pass %d: energy %.6f  bound %.6f  after %d iterations" % (p + 1, e, lb, it))
    print("stage times: " + "  ".join("%s %.3f s" % kv for kv in out.times.items()))
    if args.save:
        np.savez_compressed(args.save, **{"%s_%s" % (name, key): getattr(view, key) for name, view in
                                          (("left", out.left), ("right", out.right)) for key in ("dispmap", "status", "filled")})


if __name__ == "__main__":
    main()
