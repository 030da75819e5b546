#!/usr/bin/env python
"""Sub-pixel disparities on the Teddy pair (tests/golden/teddy_pair.npz) by band refinement: the
whole-pixel solve of both views as examples/example_consistency.py runs it, then two band levels around each map --
+-1 pixel in steps of 1/4, then +-1/4 in steps of 1/16 -- each a 9-label TRW-S problem built on the device.

    python examples/example_subpixel.py [--disparities 60] [--maxiter 30] [--refine-iters 0] [--save out.npz]
                                        [--carry [--record out.txt]]

Prints, for the whole-pixel maps and after each level: TRW-S energy and bound of the pass, the reference model's
energy of the left map (set_disparity + update_energy on one dispmap_ncc, so that all passes are measured in one energy
function), and the share of pixels of both views that the left-right check finds consistent at tolerance 1.0 and 0.5.

--carry measures what carrying the messages from one stage to the next buys, on the left view with solo
plans.  Per level, around the map the cold chain produced: the cold level's energy and bound after --maxiter iterations,
and from the carried level's trace, one iteration at a time, the first iteration at which its energy is at or below
the cold energy and the first at which its bound is at or above the cold bound.  Then the pair solve end to end with
max_relgap 1e-4, without and with carry: iterations per pass, the model energy of the final left map, wall time.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = (np.arange(-4, 5) / 4.0, np.arange(-4, 5) / 16.0)


def measure_carry(images, disparities, maxiter, say):
    import stereo_amd
    from stereo_amd import band, carry, terms as T
    from stereo_amd.trws import TrwsPlan
    NEVER = -1e300
    H, W = images[0].shape[:2]
    N = H * W
    conn = T.construct_neighborhood(H, W)
    vol = T.ncc_volume(images[0], images[1], disparities, 2, layout=1)
    plan = TrwsPlan(1, disparities.shape[0], N, conn)
    plan.upload(40.0 * (1.0 - vol), np.ones(conn.shape[1]), 8.0, positions=disparities)
    plan.iterate(maxiter, NEVER)
    labels, en, lb, _ = plan.result()
    say("whole pixels, left view, %d iterations: energy %.4f bound %.4f" % (maxiter, en, lb))
    stage = carry.full_range_stage(plan, disparities, conn, (H, W))
    plan.close()
    base = disparities[labels.astype(np.int64) - 1].reshape(W, H).T
    cold = band.BandProblem(vol, disparities, 40.0, base, conn, layout=1)
    warm = band.BandProblem(vol, disparities, 40.0, base, conn, layout=1)
    for level, offsets in enumerate(LEVELS, start=1):
        a, b = TrwsPlan(1, len(offsets), N, conn), TrwsPlan(1, len(offsets), N, conn)
        t0 = time.perf_counter()
        cold.build(offsets, a, 8.0)
        a.iterate(maxiter, NEVER)
        labels, en, lb, _ = a.result()
        t_cold = time.perf_counter() - t0
        t0 = time.perf_counter()
        warm.build(offsets, b, 8.0, carry=warm.carry_from(stage))
        t_build = time.perf_counter() - t0
        first_en = first_lb = None
        trace = []
        for it in range(1, maxiter + 1):
            b.iterate(1, NEVER)
            _, wen, wlb, _ = b.result(want_labels=False)
            trace.append((wen, wlb))
            if first_en is None and wen <= en:
                first_en = it
            if first_lb is None and wlb >= lb:
                first_lb = it
        say("level %d (%d offsets %+g .. %+g): cold after %d iterations energy %.4f bound %.4f (build + solve %.3f s)"
            % (level, len(offsets), offsets[0], offsets[-1], maxiter, en, lb, t_cold))
        say("level %d carried from %s: energy %.4f bound %.4f after 1 iteration, %.4f / %.4f after %d; energy at or below "
            "the cold one first at iteration %s, bound at or above the cold one first at iteration %s (build + transfer + "
            "load %.3f s)" % (level, "the whole-pixel solve" if level == 1 else "level %d" % (level - 1), trace[0][0], trace[0][1],
                              trace[-1][0], trace[-1][1], maxiter, first_en, first_lb, t_build))
        stage = cold.stage(a)                       # both chains go on around the cold chain's map
        cold.apply(labels)
        warm.apply(labels)
        a.close()
        b.close()
    model = stereo_amd.dispmap_ncc(images, disparities, 1, 40.0, 8.0)
    for on in (False, True, False, True):
        t0 = time.perf_counter()
        out = stereo_amd.solve_pair_ncc(images, disparities, 1, 40.0, 8.0, maxiter, 1e-4, check_tol=0.5, band_levels=LEVELS, carry=on)
        seconds = time.perf_counter() - t0
        model.set_disparity(out.left.dispmap)
        say("pair solve, max_relgap 1e-4, carry %-5s: iterations per pass left %s right %s; band stages %s; model energy of the "
            "final left map %.4f; end to end %.3f s"
            % (on, [int(i) for i in out.left.iterations], [int(i) for i in out.right.iterations],
               "  ".join("%s %.3f s" % (k, v) for k, v in out.times.items() if k in ("band_1", "band_2")), model.energy(), seconds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--disparities", type=int, default=60)
    ap.add_argument("--maxiter", type=int, default=30)
    ap.add_argument("--refine-iters", type=int, default=0)
    ap.add_argument("--save", help="write the maps of every pass of both views to this .npz")
    ap.add_argument("--carry", action="store_true", help="measure what carried messages buy (DESIGN.md 6.5)")
    ap.add_argument("--record", help="with --carry: append the measurement's lines to this file")
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
    if args.carry:
        lines = []

        def say(line):
            print(line, flush=True)
            lines.append(line)

        say("example_subpixel.py --carry --disparities %d --maxiter %d" % (args.disparities, args.maxiter))
        measure_carry(images, disparities, args.maxiter, say)
        if args.record:
            with open(args.record, "a") as f:
                f.write("\n".join(lines) + "\n")
    if args.save:
        np.savez_compressed(args.save, **{"%s_pass%d" % (name, p): m for name, view in (("left", out.left), ("right", out.right))
                                          for p, m in enumerate(view.maps)})


if __name__ == "__main__":
    main()
