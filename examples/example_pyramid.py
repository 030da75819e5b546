#!/usr/bin/env python
"""The image pyramid against the full-size solve on the Teddy and Baby2 pairs (tests/golden), DESIGN.md 6.4: both views
solved coarse to fine (solve_pair_ncc_pyramid) and at full size (solve_pair_ncc) in the same run with the same
iteration budget per solve (max_relgap 0: every solve runs `--maxiter` iterations).

    python examples/example_pyramid.py [--levels 2] [--maxiter 30] [--expand guided] [--kernel 1] [--drop-slice]
                                       [--unary images|blocks|both] [--carry] [--record out.txt]
                                       [--propagate] [--propagate-passes 1]

Per pair and method it prints the wall time per stage, the kernel family of every solve (TrwsPlan.path(): 2 is the
K <= 64 Pipe family), the energy of the final left map in the full-size model (one dispmap_ncc, set_disparity +
update_energy), the share of consistent pixels at check tolerances 0.5 and 1.0, and the share of pixels where the two
methods' left maps differ by more than 1.  --unary chooses where a level's volume comes from: the NCC
of the reduced images, the block means of the full-size volume, or both side by side.  --drop-slice leaves out the coarsest level's last slice where that level has
65 (one past the Pipe family), as a caller who wants the coarse solve in that family would.

--propagate adds, next to every pyramid, the same pyramid with candidate passes before each level's bands:
--propagate-passes passes per level, each with the offsets -1, 0, 1 and the current map and the level's winner-take-all
map at the 12 taps 1, 2 and 4 pixels away along the rows and the columns (K = 27).

--carry measures instead what carrying the messages from stage to stage buys.  On the left view with
solo plans, per band of every level, around the map the cold chain produced: the cold band's energy and bound after
--maxiter iterations and, from the carried band's trace, the first iteration at which its energy is at or below the cold
energy and the first at which its bound is at or above the cold bound (the first band of a level carries from the scale
above, the others from the band before).  Then the pair pyramid end to end with max_relgap 1e-4 for carry 'none',
'levels' and 'scales': iterations per pass, the energy of the final left map in the full-size model, wall time.
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


def measure_carry(name, images, disparities, args, say):
    import stereo_amd
    from stereo_amd import band, carry, pyramid, terms as T
    from stereo_amd.trws import TrwsPlan
    NEVER = -1e300
    L = args.levels
    bands = [[np.array(pyramid.DEFAULT_BAND)]] * L
    bands[0] = bands[0] + [np.arange(-4, 5) / 4.0]             # level 0: the band, then a quarter-pixel level
    host, dev = pyramid.reduce_images(images, L)
    disp = [pyramid.level_disparities(disparities, l) for l in range(L + 1)]
    model = [pyramid.level_model(args.kernel, TOL, l) for l in range(L + 1)]
    H, W = host[L][0].shape[:2]
    conn = T.construct_neighborhood(H, W)
    vol = T.ncc_volume(host[L][0], host[L][1], disp[L], 2, layout=1)
    plan = TrwsPlan(args.kernel, disp[L].shape[0], H * W, conn)
    plan.upload(UNARY_WEIGHT * (1.0 - vol), np.ones(conn.shape[1]) * model[L][1], model[L][0], positions=disp[L])
    plan.iterate(args.maxiter, NEVER)
    labels, en, lb, _ = plan.result()
    say("%s level %d (%d x %d, %d slices), left view, %d iterations: energy %.4f bound %.4f" % (name, L, H, W, disp[L].shape[0], args.maxiter, en, lb))
    stage = carry.full_range_stage(plan, disp[L], conn, (H, W))
    plan.close()
    current = disp[L][labels.astype(np.int64) - 1].reshape(W, H).T
    for l in range(L - 1, -1, -1):
        H, W = host[l][0].shape[:2]
        conn = T.construct_neighborhood(H, W)
        expanded, _ = pyramid._expand_view(current, (H, W), pyramid.MODES[args.expand], dev[l][0], dev[l + 1][0])
        vol = T.ncc_volume(host[l][0], host[l][1], disp[l], 2, layout=1)
        alphas = np.ones(conn.shape[1]) * model[l][1]
        cold = band.BandProblem(vol, disp[l], UNARY_WEIGHT, expanded, conn, alphas, layout=1)
        warm = band.BandProblem(vol, disp[l], UNARY_WEIGHT, expanded, conn, alphas, layout=1)
        for b, offsets in enumerate(bands[l]):
            pa, pb = TrwsPlan(args.kernel, len(offsets), H * W, conn), TrwsPlan(args.kernel, len(offsets), H * W, conn)
            cold.build(offsets, pa, model[l][0])
            pa.iterate(args.maxiter, NEVER)
            labels, en, lb, _ = pa.result()
            t0 = time.perf_counter()
            warm.build(offsets, pb, model[l][0], carry=warm.carry_from(stage, scales=b == 0))
            t_build = time.perf_counter() - t0
            first_en = first_lb = None
            trace = []
            for it in range(1, args.maxiter + 1):
                pb.iterate(1, NEVER)
                _, wen, wlb, _ = pb.result(want_labels=False)
                trace.append((wen, wlb))
                if first_en is None and wen <= en:
                    first_en = it
                if first_lb is None and wlb >= lb:
                    first_lb = it
            say("%s level %d band %d (%d x %d, offsets %+g .. %+g by %g): cold after %d iterations energy %.4f bound %.4f"
                % (name, l, b + 1, H, W, offsets[0], offsets[-1], offsets[1] - offsets[0], args.maxiter, en, lb))
            say("%s level %d band %d carried from %s: energy %.4f bound %.4f after 1 iteration, %.4f / %.4f after %d; energy at or "
                "below the cold one first at iteration %s, bound at or above the cold one first at iteration %s (build + transfer "
                "+ load %.3f s)" % (name, l, b + 1, "the scale above" if b == 0 else "the band before", trace[0][0], trace[0][1],
                                    trace[-1][0], trace[-1][1], args.maxiter, first_en, first_lb, t_build))
            stage = cold.stage(pa)                  # both chains go on around the cold chain's map
            current = cold.apply(labels)
            warm.apply(labels)
            pa.close()
            pb.close()
    dm = stereo_amd.dispmap_ncc(images, disparities, args.kernel, UNARY_WEIGHT, TOL)
    solve_args = (images, disparities, args.kernel, UNARY_WEIGHT, TOL, L, args.maxiter, 1e-4)
    for mode in ("none", "levels", "scales", "none", "levels", "scales"):
        t0 = time.perf_counter()
        out = stereo_amd.solve_pair_ncc_pyramid(*solve_args, bands=bands, expand=args.expand, carry=mode)
        seconds = time.perf_counter() - t0
        dm.set_disparity(out.left.dispmap)
        dm.update_energy()
        say("%s pair pyramid, max_relgap 1e-4, carry %-6s: left iterations per level %s; energy of the final left map in the "
            "full-size model %.4f; end to end %.3f s"
            % (name, mode, {l: [int(i) for i in out.levels[l].left.iterations] for l in range(L, -1, -1)}, dm.energy(), seconds))


PROPAGATE_TAPS = [(dy * r, dx * r) for r in (1, 2, 4) for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1))]


def propagate_levels(levels, passes):
    return [[dict(offsets=[-1.0, 0.0, 1.0], taps=PROPAGATE_TAPS, sources=["base", "wta"])] * passes for _ in range(levels)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=2)
    ap.add_argument("--maxiter", type=int, default=30)
    ap.add_argument("--expand", default="guided")
    ap.add_argument("--kernel", type=int, default=1)
    ap.add_argument("--drop-slice", action="store_true")
    ap.add_argument("--carry", action="store_true", help="measure what carried messages buy (DESIGN.md 6.5)")
    ap.add_argument("--record", help="append the printed lines to this file")
    ap.add_argument("--unary", default="images", choices=("images", "blocks", "both"),
                    help="where a level's volume comes from (DESIGN.md 6.6); both: the two choices side by side")
    ap.add_argument("--propagate", action="store_true", help="also run every pyramid with candidate passes (DESIGN.md 6.7)")
    ap.add_argument("--propagate-passes", type=int, default=1, help="candidate passes per level")
    args = ap.parse_args()
    import stereo_amd
    from stereo_amd import pyramid
    s = 1 << args.levels
    unaries = ("images", "blocks") if args.unary == "both" else (args.unary,)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    for name, file, D in PAIRS:
        g = np.load(os.path.join(ROOT, "tests", "golden", file))
        images = [g["im0"].astype(np.float64), g["im1"].astype(np.float64)]
        H, W = images[0].shape[:2]
        disparities = np.arange(D, dtype=np.float64)
        if args.drop_slice and pyramid.level_disparities(disparities, args.levels).shape[0] == 65:
            disparities = disparities[:s * 63 + 1]
        say("%s %d x %d, %d disparities, kernel %d, unary weight %g, tol %g, %d iterations per solve, %d reductions, expand %s"
            % (name, H, W, disparities.shape[0], args.kernel, UNARY_WEIGHT, TOL, args.maxiter, args.levels, args.expand))
        if args.carry:
            carry_lines = []

            def say_carry(line):
                print(line, flush=True)
                carry_lines.append(line)

            say_carry("example_pyramid.py --carry --levels %d --maxiter %d --expand %s --kernel %d%s: %s %d x %d, %d disparities"
                % (args.levels, args.maxiter, args.expand, args.kernel, " --drop-slice" if args.drop_slice else "", name, H, W,
                   disparities.shape[0]))
            measure_carry(name, images, disparities, args, say_carry)
            if args.record:
                with open(args.record, "a") as f:
                    f.write("\n".join(carry_lines) + "\n")
            continue
        solve_args = (images, disparities, args.kernel, UNARY_WEIGHT, TOL)
        pyramids = []
        variants = []
        for unary in unaries:
            variants.append(("pyramid, unary %s" % unary, dict(unary=unary)))
            if args.propagate:
                variants.append(("pyramid, unary %s, propagate x %d" % (unary, args.propagate_passes),
                                 dict(unary=unary, propagate=propagate_levels(args.levels, args.propagate_passes))))
        for what, kw in variants:
            stereo_amd.solve_pair_ncc_pyramid(*solve_args, args.levels, 1, 0.0, expand=args.expand, **kw)   # warm-up: code objects
            t0 = time.perf_counter()
            pyr = stereo_amd.solve_pair_ncc_pyramid(*solve_args, args.levels, args.maxiter, 0.0, expand=args.expand, **kw)
            pyramids.append((what, pyr, time.perf_counter() - t0))
        t0 = time.perf_counter()
        full = stereo_amd.solve_pair_ncc(*solve_args, args.maxiter, 0.0)
        t_full = time.perf_counter() - t0

        for what, pyr, t_pyr in pyramids:
            say("  %s: %.3f s in all;  " % (what, t_pyr) + "  ".join("%s %.3f s" % kv for kv in pyr.times.items()))
            for l in range(args.levels, -1, -1):
                res = pyr.levels[l]
                h, w = res.left.dispmap.shape
                say("    level %d, %d x %d, %d slices, tol %g, edge weight %g, families %s: " % (
                    l, h, w, pyr.disparities[l].shape[0], pyr.tol[l], pyr.smooth_weight[l], res.left.paths)
                    + "  ".join("%s %.3f s" % kv for kv in res.times.items()))
                say("      left: energy %s  bound %s  iterations %s" % (
                    ["%.3f" % e for e in res.left.energy], ["%.3f" % b for b in res.left.lower_bound], [int(i) for i in res.left.iterations]))
                if l < args.levels:
                    share = np.bincount(res.left.expand_source.reshape(-1) + 1, minlength=5) / float(h * w)
                    say("      left: expansion's source -1, 0 .. 3: " + " ".join("%.3f" % v for v in share))
        say("  full size: %.3f s in all, family %s;  " % (t_full, full.left.paths) + "  ".join("%s %.3f s" % kv for kv in full.times.items()))
        say("    left: energy %.3f  bound %.3f  iterations %d" % (full.left.energy[0], full.left.lower_bound[0], full.left.iterations[0]))

        dm = stereo_amd.dispmap_ncc(images, disparities, args.kernel, UNARY_WEIGHT, TOL)
        for what, result in [(w, p) for w, p, _ in pyramids] + [("full size", full)]:
            dm.set_disparity(result.left.dispmap)
            dm.update_energy()
            line = "  %-40s left map in the full-size model: energy %.3f" % (what, dm.energy())
            for tol in (0.5, 1.0):
                status, _ = stereo_amd.lr_check(result.left.dispmap, result.right.dispmap, 1, tol)
                line += ";  consistent at %.1f: %.4f" % (tol, float((status == 0).mean()))
            say(line)
        for what, pyr, _ in pyramids:
            diff = np.abs(pyr.left.dispmap - full.left.dispmap)
            say("  %s: left map differs from the full-size one by more than 1 at %.4f of the pixels, by more than 2 (the band's "
                "half-width) at %.4f; median |difference| %.3f"
                % (what, float((diff > 1.0).mean()), float((diff > 2.0).mean()), float(np.median(diff))))
    if args.record and not args.carry:
        with open(args.record, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
