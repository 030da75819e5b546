#!/usr/bin/env python
"""Plane propagation on the Teddy pair (tests/golden/teddy_pair.npz), after the short plane-lattice fusion
of examples/example_plane_band.py.  From that one start, for the left view and its mirrored twin:

  1. refine_plane_band alone: +-1 pixel in steps of 1/4, then +-1/4 in steps of 1/16;
  2. one plane-candidate pass -- the current planes ('base') and the winner-take-all map ('wta') at the 12 taps 1, 2 and 4
     pixels along the rows and the columns, offsets -1, 0, 1: K = 3 + 2 * 12 = 27 -- followed by the same plane band;
  3. refine_candidates with the same recipe (fronto-parallel labels: a copied disparity, not a copied plane), followed by
     the same plane band;
  4. for dispmap_globalstereo on the same pair: the binary fusion of its 14 SegPln proposals, then one plane-candidate
     pass with 'base' and the 14 proposals at the tap (0, 0) -- simultaneous fusion with the band's offsets in one problem.

    python examples/example_plane_candidates.py [--disparities 60] [--maxiter 30]

Prints per run the model energy from update_energy() (one energy function for every line of a class), the share of pixels
whose plane is slanted (a or b not zero), for dispmap_ncc the share of left pixels the left-right check finds consistent
at tolerance 0.5, and the wall time.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BAND = (np.arange(-4, 5) / 4.0, np.arange(-4, 5) / 16.0)
TAPS = [(0, s) for s in (-1, 1, -2, 2, -4, 4)] + [(s, 0) for s in (-1, 1, -2, 2, -4, 4)]
RECIPE = dict(offsets=[-1.0, 0.0, 1.0], taps=TAPS, sources=["base", "wta"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--disparities", type=int, default=60)
    ap.add_argument("--maxiter", type=int, default=30)
    args = ap.parse_args()
    import stereo_amd
    g = np.load(os.path.join(ROOT, "tests", "golden", "teddy_pair.npz"))
    images = [g["im0"].astype(np.float64), g["im1"].astype(np.float64)]
    disparities = np.arange(args.disparities, dtype=np.float64)
    slanted = lambda a: float(np.mean((a[0] != 0) | (a[1] != 0)))

    left = stereo_amd.dispmap_ncc(images, disparities, 1, 40.0, 8.0)
    views = [left, left.mirrored()]
    starts = []
    for dm in views:
        proposals = dm.generate_plane_lattice(radius=5)
        proposals += [stereo_amd.PlaneProposal([0.0, 0.0, 1.0, -float(d)]) for d in range(0, int(disparities.max()) + 1, 10)]
        for p in proposals:
            dm.binary_fusion(p)
        starts.append(dm.assignment.copy())

    def report(name, seconds=None):
        left.update_energy()
        status, _ = stereo_amd.lr_check(views[0].current_dispmap(), views[1].current_dispmap(), 1, 0.5)
        line = "%-58s model energy %.4f, slanted %.4f, consistent at 0.5 %.4f" % (
            name, left.energy(), slanted(left.assignment), float((status == 0).mean()))
        print(line + ("" if seconds is None else ", %.3f s (both views)" % seconds))

    report("dispmap_ncc: binary fusion of %d plane proposals" % len(proposals))
    runs = (("plane band alone", None),
            ("plane candidates (K = 27), then the plane band", lambda dm: dm.refine_plane_candidates([RECIPE], maxiter=args.maxiter)),
            ("candidate band (K = 27), then the plane band", lambda dm: dm.refine_candidates([RECIPE], maxiter=args.maxiter)))
    for name, first in runs:
        t0 = time.perf_counter()
        for dm, start in zip(views, starts):
            dm.assignment = start
            if first is not None:
                out = first(dm)
                if dm is left:
                    note = "TRW-S energy %.4f bound %.4f after %d iterations" % (out.energy[0], out.lower_bound[0], out.iterations[0])
        if first is not None:
            report("  %s: after the pass" % name.split(",")[0], time.perf_counter() - t0)
            print("  %-56s %s" % ("", note))
        for dm in views:
            dm.refine_plane_band(list(BAND), maxiter=args.maxiter)
        report(name, time.perf_counter() - t0)

    # dispmap_globalstereo: its own energy (another unary, segment-weighted edges), so its lines compare with each other only
    P = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))])[:, :, None], (1, 1, 2))
    P[0, 3, 1] = -0.25
    gs = stereo_amd.dispmap_globalstereo(images, P, (0, args.disparities - 1), 4, rng=np.random.default_rng(0))
    N = gs.sz[0] * gs.sz[1]
    proposals = [p.expand(N) if hasattr(p, "expand") else np.asarray(p) for p in gs.segpln(seed=0)]
    for p in proposals:
        gs.binary_fusion(p)
    fused = gs.assignment.copy()

    def report_gs(name, seconds=None, out=None):
        gs.update_energy()
        line = "%-58s model energy %.4f, slanted %.4f" % (name, gs.energy(), slanted(gs.assignment))
        if out is not None:
            line += "; TRW-S energy %.4f bound %.4f after %d iterations" % (out.energy[0], out.lower_bound[0], out.iterations[0])
        print(line + ("" if seconds is None else ", %.3f s" % seconds))

    report_gs("dispmap_globalstereo: binary fusion of %d SegPln proposals" % len(proposals))
    step = 1.0 / (4.0 * gs.d_step)                   # a quarter pixel in the smoothness term's units
    t0 = time.perf_counter()
    out = gs.refine_plane_band([np.arange(-4, 5) * step], maxiter=args.maxiter)
    report_gs("plane band alone (+-1 pixel by 1/4)", time.perf_counter() - t0, out)
    gs.assignment = fused
    t0 = time.perf_counter()
    level = dict(offsets=[-4 * step, 0.0, 4 * step], taps=[(0, 0)], sources=["base"] + proposals)
    out = gs.refine_plane_candidates([level], maxiter=args.maxiter)
    report_gs("plane candidates: base + %d proposals at (0, 0), K = %d" % (len(proposals), 3 + 1 + len(proposals)), time.perf_counter() - t0, out)
    t1 = time.perf_counter()
    out = gs.refine_plane_band([np.arange(-4, 5) * step], maxiter=args.maxiter)
    report_gs("   ... then the plane band", time.perf_counter() - t1, out)


if __name__ == "__main__":
    main()
