#!/usr/bin/env python
"""Sub-pixel refinement that keeps each pixel's plane, on the Teddy pair (tests/golden/teddy_pair.npz):
a short plane-lattice fusion as in examples/example_ncc.py, then the same two levels -- +-1 pixel in steps of 1/4, then
+-1/4 in steps of 1/16 -- twice from the same start: once with refine_band, which turns every pixel into a
fronto-parallel plane first, once with refine_plane_band, where label k is the pixel's own plane moved
by the offset.

    python examples/example_plane_band.py [--disparities 60] [--maxiter 30]

Prints, for the start and after each level of both refinements, the model energy from update_energy() on one object
(one energy function for every line), the TRW-S energy and bound of the level, and the share of pixels whose plane is
slanted (a or b not zero).
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
    args = ap.parse_args()
    import stereo_amd
    g = np.load(os.path.join(ROOT, "tests", "golden", "teddy_pair.npz"))
    images = [g["im0"].astype(np.float64), g["im1"].astype(np.float64)]
    disparities = np.arange(args.disparities, dtype=np.float64)
    dm = stereo_amd.dispmap_ncc(images, disparities, 1, 40.0, 8.0)
    print("NCC volume + winner-takes-all start: energy %.4f" % dm.energy())
    proposals = dm.generate_plane_lattice(radius=5)
    proposals += [stereo_amd.PlaneProposal([0.0, 0.0, 1.0, -float(d)]) for d in range(0, int(disparities.max()) + 1, 10)]
    for p in proposals:
        dm.binary_fusion(p)
    start = dm.assignment.copy()
    slanted = lambda a: float(np.mean((a[0] != 0) | (a[1] != 0)))

    def report(name, out=None, level=None):
        dm.update_energy()
        line = "%-44s model energy %.4f, slanted pixels %.4f" % (name, dm.energy(), slanted(dm.assignment))
        if out is not None:
            line += "; TRW-S energy %.4f bound %.4f after %d iterations" % (out.energy[level], out.lower_bound[level], out.iterations[level])
        print(line)

    report("binary fusion of %d plane proposals" % len(proposals))
    for name, refine in (("refine_band (fronto-parallel labels)", dm.refine_band),
                         ("refine_plane_band (the pixel's own plane)", dm.refine_plane_band)):
        dm.assignment = start
        t0 = time.perf_counter()
        for i, level in enumerate(LEVELS):
            out = refine([level], maxiter=args.maxiter)
            report("%s, level %d (%+g .. %+g by %g)" % (name.split(" (")[0], i + 1, level[0], level[-1], level[1] - level[0]), out, 0)
        print("%-44s %.3f s for both levels" % (name, time.perf_counter() - t0))


if __name__ == "__main__":
    main()
