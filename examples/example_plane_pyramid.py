#!/usr/bin/env python
"""The plane pyramid on the Teddy pair (tests/golden/teddy_pair.npz), against the two ways to a map it
joins.  Left view, one dispmap_ncc object, three kinds of run:

  1. solve_pyramid with today's propagate=: per level one candidate pass -- offsets -1, 0, 1, the current
     map and the winner-take-all map at the 12 taps 1, 2 and 4 pixels along the rows and the columns -- then the bands;
  2. solve_plane_pyramid with the same pass on planes and a Fit source next to 'base' and 'wta' (K = 3 + 3 * 12 = 39),
     then the plane bands; and the same without the Fit source (K = 27), to see what the fit itself adds;
  3. the full-size plane candidates of examples/example_plane_candidates.py: the plane-lattice fusion, one plane-candidate
     pass ('base' and 'wta', K = 27), then the plane band.

Every run ends in the same bands at full size: +-2 in steps of 1, +-1 in steps of 1/4, +-1/4 in steps of 1/16.

    python examples/example_plane_pyramid.py [--disparities 60] [--maxiter 30] [--levels 2] [--radius 2] [--tau 1.0]

Prints per run the left view's model energy at full size from update_energy() (one energy function for every line), the
share of pixels whose plane is slanted (a or b not zero) and the wall time.  Nothing is asserted; the output of one run
is kept as profiles/plane_pyramid_example.txt.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAPS = [(dy * r, dx * r) for r in (1, 2, 4) for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1))]
SUBPIXEL = [np.arange(-4, 5) / 4.0, np.arange(-4, 5) / 16.0]
BAND = np.arange(-2.0, 3.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--disparities", type=int, default=60)
    ap.add_argument("--maxiter", type=int, default=30)
    ap.add_argument("--levels", type=int, default=2)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--tau", type=float, default=1.0)
    args = ap.parse_args()
    import stereo_amd
    from stereo_amd.plane_candidates import Fit
    g = np.load(os.path.join(ROOT, "tests", "golden", "teddy_pair.npz"))
    images = [g["im0"].astype(np.float64), g["im1"].astype(np.float64)]
    disparities = np.arange(args.disparities, dtype=np.float64)
    L = args.levels
    dm = stereo_amd.dispmap_ncc(images, disparities, 1, 40.0, 8.0)
    bands = [[BAND] + SUBPIXEL] + [[BAND]] * (L - 1)
    recipe = lambda sources: [[dict(offsets=[-1.0, 0.0, 1.0], taps=TAPS, sources=sources)] for _ in range(L)]
    print("teddy %d x %d, %d disparities, kernel 1, unary weight 40, tol 8, %d iterations per solve, %d reductions, expand guided"
          % (tuple(dm.sz) + (args.disparities, args.maxiter, L)))

    def report(name, seconds, out=None):
        dm.update_energy()
        a = dm.assignment
        print("%-72s model energy %.4f, slanted %.4f, %.3f s" % (name, dm.energy(), float(np.mean((a[0] != 0) | (a[1] != 0))), seconds))
        if out is not None:
            for l in range(L, -1, -1):
                print("    level %d: energy %s  bound %s" % (l, ["%.3f" % e for e in out.energy[l]], ["%.3f" % b for b in out.lower_bound[l]]))
            for l in range(L - 1, -1, -1):
                src = out.expand_source[l]
                print("    level %d: expansion's source -1, 0 .. 3: %s" % (l, " ".join("%.3f" % float((src == k).mean()) for k in range(-1, 4))))

    def run(name, solve):
        dm.init_solution()
        t0 = time.perf_counter()
        out = solve()
        report(name, time.perf_counter() - t0, out)

    for _ in range(2):                    # (the first round pays for the code objects and the allocator: read the second)
        run("1. solve_pyramid, propagate 'base' + 'wta' (K = 27), bands",
            lambda: dm.solve_pyramid(L, bands=bands, maxiter=args.maxiter, propagate=recipe(["base", "wta"])))
        run("2. solve_plane_pyramid, Fit(%d, %g) + 'base' + 'wta' (K = 39), plane bands" % (args.radius, args.tau),
            lambda: dm.solve_plane_pyramid(L, bands=bands, maxiter=args.maxiter, propagate=recipe([Fit(args.radius, args.tau), "base", "wta"])))
        run("2b. solve_plane_pyramid, 'base' + 'wta' (K = 27), plane bands",
            lambda: dm.solve_plane_pyramid(L, bands=bands, maxiter=args.maxiter, propagate=recipe(["base", "wta"])))
        run("2c. solve_plane_pyramid without a candidate pass, plane bands",
            lambda: dm.solve_plane_pyramid(L, bands=bands, maxiter=args.maxiter))

        dm.init_solution()
        t0 = time.perf_counter()
        proposals = dm.generate_plane_lattice(radius=5)
        proposals += [stereo_amd.PlaneProposal([0.0, 0.0, 1.0, -float(d)]) for d in range(0, int(disparities.max()) + 1, 10)]
        for p in proposals:
            dm.binary_fusion(p)
        report("3. full size: binary fusion of %d plane proposals" % len(proposals), time.perf_counter() - t0)
        dm.refine_plane_candidates([dict(offsets=[-1.0, 0.0, 1.0], taps=TAPS, sources=["base", "wta"])], maxiter=args.maxiter)
        dm.refine_plane_band([BAND] + SUBPIXEL, maxiter=args.maxiter)
        report("3. ... then plane candidates (K = 27) and the plane bands", time.perf_counter() - t0)
        # and the fit as one more source of that full-size pass
        dm.init_solution()
        t0 = time.perf_counter()
        for p in proposals:
            dm.binary_fusion(p)
        dm.refine_plane_candidates([dict(offsets=[-1.0, 0.0, 1.0], taps=TAPS, sources=[Fit(args.radius, args.tau), "base", "wta"])],
                                   maxiter=args.maxiter)
        dm.refine_plane_band([BAND] + SUBPIXEL, maxiter=args.maxiter)
        report("3b. the same with a Fit(%d, %g) source (K = 39)" % (args.radius, args.tau), time.perf_counter() - t0)
        print()


if __name__ == "__main__":
    main()
