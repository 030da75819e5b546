#!/usr/bin/env python
"""Scanline aggregation on the Teddy pair (tests/golden/teddy_pair.npz): both views, four ways to a map.

    python examples/example_scanline.py [--disparities 60] [--maxiter 30] [--smooth-weight 1.0] [--levels trws|scanline|both]
                                        [--record out.txt] [--contrast]

  (a) solve_pair_ncc: the full-range TRW-S solve, --maxiter iterations
  (b) solve_pair_ncc_scanline alone: 8 directions, every direction weighing --smooth-weight
  (c) (b) plus one K = 27 candidate level: offsets -1, 0, 1 and 12 taps on each of the sources 'base' and 'wta'
  (d) (c) plus the two sub-pixel band levels of examples/example_subpixel.py
--levels says how the levels of (c) and (d) are solved: by TRW-S (the default, --maxiter iterations per level), by one
scanline aggregation on the level's own inputs (level_solver="scanline"), or both ways side by side.  The
output of --levels both behind DESIGN.md 6.11 is kept as profiles/scanline_levels_example.txt; whether a scanline level
should become a default anywhere is decided later from that file, not here.

The two NCC volumes are made once and handed to every variant (their time is printed once); each variant runs twice and
the second run's wall time is the one reported, so that no variant pays for code objects and allocator warm-up.  Per
variant: the model energy of the left map (set_disparity + energy() on one dispmap_ncc: one energy function for maps on and
off the label grid), the share of pixels of each view that the left-right check finds consistent at tolerance 0.5 and 1.0,
the share of left pixels further than 2 from (a)'s left map, and the wall time.

--contrast runs another comparison instead: (a), (b) and (c) with uniform weights and with image-guided
weights, once per Contrast setting of SETTINGS (w_high, w_low, g0, g1 in the images' 0 .. 255 units; the first is the one
the example would take by default).  Every map's energy is the energy under ITS OWN model -- uniform weights, or that
setting's contrast weights (dispmap_ncc.set_contrast) -- so energies compare within one model, across (a), (b), (c), not
across models.  The output is kept as profiles/scanline_contrast_example.txt; nothing in it is asserted anywhere."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BANDS = (np.arange(-4, 5) / 4.0, np.arange(-4, 5) / 16.0)         # example_subpixel.py's LEVELS
TAPS = [(0, -1), (0, 1), (-1, 0), (1, 0), (0, -2), (0, 2), (-2, 0), (2, 0), (-1, -1), (-1, 1), (1, -1), (1, 1)]
CANDIDATES = [dict(offsets=[-1.0, 0.0, 1.0], taps=TAPS, sources=["base", "wta"])]                   # K = 3 + 2 * 12 = 27
# the Contrast settings --contrast tries: a ramp around the uniform weight 1, a gentler one, one that only lowers, a step
SETTINGS = [(2.0, 0.5, 8.0, 40.0), (1.5, 0.75, 8.0, 40.0), (1.0, 0.25, 5.0, 25.0), (1.0, 0.25, 16.0, 16.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--disparities", type=int, default=60)
    ap.add_argument("--maxiter", type=int, default=30)
    ap.add_argument("--smooth-weight", type=float, default=1.0)
    ap.add_argument("--levels", choices=["trws", "scanline", "both"], default="trws", help="how the levels of (c) and (d) are solved")
    ap.add_argument("--record", help="write the printed lines to this file")
    ap.add_argument("--contrast", action="store_true", help="uniform against image-guided weights (DESIGN.md 6.12)")
    args = ap.parse_args()
    import stereo_amd
    from stereo_amd import consistency, scanline
    g = np.load(os.path.join(ROOT, "tests", "golden", "teddy_pair.npz"))
    images = [g["im0"].astype(np.float64), g["im1"].astype(np.float64)]
    disparities = np.arange(args.disparities, dtype=np.float64)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say("example_scanline.py --disparities %d --maxiter %d --smooth-weight %g --levels %s"
        % (args.disparities, args.maxiter, args.smooth_weight, args.levels))
    t0 = time.perf_counter()
    volumes = consistency.pair_volumes(images, disparities)
    say("the two NCC volumes (shared by every variant): %.3f s" % (time.perf_counter() - t0))
    model = stereo_amd.dispmap_ncc(images, disparities, 1, 40.0, 8.0)
    if args.contrast:
        contrast_comparison(args, images, disparities, volumes, model, say)
        if args.record:
            with open(args.record, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    common = dict(check_tol=0.5, smooth_weight=args.smooth_weight, maxiter=args.maxiter, max_relgap=0.0, volumes=volumes)
    variants = [
        ("(a) solve_pair_ncc, %d iterations" % args.maxiter,
         lambda: stereo_amd.solve_pair_ncc(images, disparities, 1, 40.0, 8.0, args.maxiter, 0.0, check_tol=0.5, volumes=volumes)),
        ("(b) scanline alone", lambda: scanline.solve_pair_ncc_scanline(images, disparities, 1, 40.0, 8.0, **common)),
    ]
    for solver in (["trws", "scanline"] if args.levels == "both" else [args.levels]):
        tag = "" if args.levels == "trws" else ", levels by %s" % solver
        variants += [
            ("(c) scanline + candidates K = 27" + tag,
             lambda solver=solver: scanline.solve_pair_ncc_scanline(images, disparities, 1, 40.0, 8.0, candidate_levels=CANDIDATES,
                                                                    level_solver=solver, **common)),
            ("(d) (c) + two sub-pixel band levels" + tag,
             lambda solver=solver: scanline.solve_pair_ncc_scanline(images, disparities, 1, 40.0, 8.0, candidate_levels=CANDIDATES,
                                                                    band_levels=BANDS, level_solver=solver, **common)),
        ]
    reference = None
    for name, run in variants:
        run()
        t0 = time.perf_counter()
        out = run()
        seconds = time.perf_counter() - t0
        if reference is None:
            reference = out.left.dispmap
        model.set_disparity(out.left.dispmap)
        shares = []
        for tol in (0.5, 1.0):
            for ref, other, direction in ((out.left, out.right, 1), (out.right, out.left, -1)):
                status, _ = stereo_amd.lr_check(ref.dispmap, other.dispmap, direction, tol, want_residual=False)
                shares.append(float(np.mean(status == 0)))
        far = float(np.mean(np.abs(out.left.dispmap - reference) > 2.0))
        say("%-58s model energy of the left map %.4f; consistent at 0.5: left %.4f right %.4f, at 1.0: left %.4f right %.4f; "
            "left pixels further than 2 from (a): %.4f; wall %.3f s" % (name, model.energy(), shares[0], shares[1], shares[2], shares[3], far, seconds))
        say("%-58s passes: energy %s iterations %s; stages: %s"
            % ("", ["%.4f" % e for e in out.left.energy], [int(i) for i in out.left.iterations],
               "  ".join("%s %.3f s" % kv for kv in out.times.items())))
    if args.record:
        with open(args.record, "w") as f:
            f.write("\n".join(lines) + "\n")


def contrast_comparison(args, images, disparities, volumes, model, say):
    import stereo_amd
    from stereo_amd import Contrast, scanline
    say("Contrast settings tried (w_high, w_low, g0, g1): %s" % SETTINGS)
    uniform = model.smooth_weights.copy()
    for setting in [None] + SETTINGS:
        c = None if setting is None else Contrast(*setting)
        if c is None:
            model.smooth_weights = uniform
            say("uniform weights 1")
        else:
            model.set_contrast(c)
            w = model.smooth_weights
            say("%r: edge weights of the left image: mean %.4f, at w_high %.4f, at w_low %.4f of the edges"
                % (c, w.mean(), np.mean(w == c.w_high), np.mean(w == c.w_low)))
        weights = dict(contrast=c) if c is not None else {}
        common = dict(check_tol=0.5, maxiter=args.maxiter, max_relgap=0.0, volumes=volumes, **weights)
        variants = [
            ("(a) solve_pair_ncc, %d iterations" % args.maxiter,
             lambda: stereo_amd.solve_pair_ncc(images, disparities, 1, 40.0, 8.0, args.maxiter, 0.0, check_tol=0.5, volumes=volumes, **weights)),
            ("(b) scanline alone", lambda: scanline.solve_pair_ncc_scanline(images, disparities, 1, 40.0, 8.0, **common)),
            ("(c) scanline + candidates K = 27",
             lambda: scanline.solve_pair_ncc_scanline(images, disparities, 1, 40.0, 8.0, candidate_levels=CANDIDATES, **common)),
        ]
        for name, run in variants:
            run()
            t0 = time.perf_counter()
            out = run()
            seconds = time.perf_counter() - t0
            model.set_disparity(out.left.dispmap)
            shares = []
            for tol in (0.5, 1.0):
                for ref, other, direction in ((out.left, out.right, 1), (out.right, out.left, -1)):
                    status, _ = stereo_amd.lr_check(ref.dispmap, other.dispmap, direction, tol, want_residual=False)
                    shares.append(float(np.mean(status == 0)))
            say("  %-40s energy of the left map under this model %.4f; consistent at 0.5: left %.4f right %.4f, at 1.0: left %.4f "
                "right %.4f; wall %.3f s" % (name, model.energy(), shares[0], shares[1], shares[2], shares[3], seconds))


if __name__ == "__main__":
    main()
