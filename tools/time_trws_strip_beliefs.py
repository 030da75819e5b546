"""Development tool: what node beliefs cost on row strips and in a batch, against another checkout.
usage: time_trws_strip_beliefs.py [--other DIR] [iters=20] [runs=3]

Every run is a fresh child process that imports stereo_amd from one tree -- DIR (a built checkout of the parent commit)
and this one, ALTERNATING, `runs` times each -- and measures, each after two warm-up iterations, `iters` iterations
between device synchronisations:
  strips   the Teddy NCC volume (tests/golden/teddy_pair.npz, 450 x 375 x 60, tol 8, shared positions) as G = 2 and 4
           logical strips: ms per iteration with beliefs off and, where the tree has them on strips, on;
  batch    8 members 128 x 128 x 16 (noise volumes, shared positions), beliefs on: iterations per second summed over the
           members (the parent launches phase 1 once per member, this tree once per batch iteration).
Prints per figure the median and min .. max of each tree's runs; the last line is one JSON object with every run.  The
output behind DESIGN.md's figures is kept as profiles/trws_strip_beliefs_timing.txt (redirect stdout there)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = -1e300


def worker(tree, iters):
    sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT); sys.path.insert(0, tree)
    import numpy as np, torch
    from bench import synthetic_volume
    from helpers import grid_conn
    from stereo_amd import terms as T
    from stereo_amd.strips import TrwsStrips, make_strips
    from stereo_amd.trws import TrwsBatch, TrwsPlan

    def timed(fn):
        torch.cuda.synchronize(); t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    out = {}
    g = np.load(os.path.join(ROOT, "tests", "golden", "teddy_pair.npz"))
    im0, im1 = g["im0"].astype(np.float64), g["im1"].astype(np.float64)
    H, W = im0.shape[:2]
    K = 60
    unary = np.ascontiguousarray(40.0 * (1.0 - T.ncc_volume(im0, im1, np.arange(K, dtype=np.float64), 2, layout=1).T))
    conn = grid_conn(H, W)
    for G in (2, 4):
        for on in (False, True):
            if on and not hasattr(TrwsStrips, "keep_min_marginals"):
                continue
            s = make_strips(1, K, H, W, conn.T, G)
            s.upload(unary.T, np.ones(conn.shape[0]), 8.0, positions=np.arange(K, dtype=np.float64))
            if on:
                s.keep_min_marginals()
            s.iterate(2, NEVER)
            out["strips G=%d beliefs %s ms/iteration" % (G, "on" if on else "off")] = 1e3 * timed(lambda: s.iterate(iters, NEVER)) / iters
            s.close()
    B, Hb, Wb, Kb = 8, 128, 128, 16
    dev = torch.device("cuda", 0)
    conn = grid_conn(Hb, Wb)
    d_alpha = torch.ones(conn.shape[0], dtype=torch.float64, device=dev)
    d_pos = torch.arange(Kb, dtype=torch.float64, device=dev)
    plans = []
    for i in range(B):
        u = torch.from_numpy(synthetic_volume(Hb, Wb, Kb, seed=1 + i)).to(dev)
        p = TrwsPlan(1, Kb, Hb * Wb, conn.T)
        p.bind_device(u.data_ptr(), d_alpha.data_ptr(), 8.0, d_positions=d_pos.data_ptr(), keepalive=(u, d_alpha, d_pos))
        p.keep_min_marginals()
        plans.append(p)
    batch = TrwsBatch(plans)
    batch.iterate(2, NEVER)
    out["batch 8 x 128x128x16 beliefs on iterations/s"] = B * iters / timed(lambda: batch.iterate(iters, NEVER))
    batch.close()
    for p in plans:
        p.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    import numpy as np
    a = sys.argv[1:]
    if a and a[0] == "--worker":
        return worker(a[1], int(a[2]))
    other = None
    if a and a[0] == "--other":
        other, a = os.path.abspath(a[1]), a[2:]
    iters = int(a[0]) if len(a) > 0 else 20
    runs = int(a[1]) if len(a) > 1 else 3
    trees = ([("other", other)] if other else []) + [("this", ROOT)]
    res = {name: {} for name, _ in trees}
    for r in range(runs):
        for name, tree in trees:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, str(iters)], capture_output=True,
                               text=True, timeout=900)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit("run %d of tree %s failed:\n%s\n%s" % (r, tree, p.stdout[-2000:], p.stderr[-2000:]))
            for k, v in json.loads(line[0][7:]).items():
                res[name].setdefault(k, []).append(v)
    for k in sorted({k for v in res.values() for k in v}):
        for name, _ in trees:
            v = res[name].get(k)
            if v:
                print("%-50s %-6s median %9.3f  (%9.3f .. %9.3f)  spread %.1f %%" %
                      (k, name, np.median(v), min(v), max(v), 100 * (max(v) - min(v)) / np.median(v)), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
