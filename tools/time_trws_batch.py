"""Development tool: TRW-S batches against the same plans iterated one after the other.
usage: time_trws_batch.py [iters=10] [runs=3] [sizes=1,2,4,8]
Two volumes: the Teddy NCC volume (tests/golden/teddy_pair.npz, 450 x 375 x 60, tol 8) and a 128 x 128 x 16 noise volume,
shared ascending positions, unit weights.  Per batch size B: B plans, timed `runs` times ALTERNATING between
  sequential   plain TrwsPlan.iterate, member after member (what a caller with B problems had before batches), and
  batch        TrwsBatch.iterate,
each run after a reset and two warm-up iterations, `iters` iterations timed between device synchronisations.  Prints
iterations per second summed over the members (median, min .. max of the runs), the ratio of the medians, and checks
that both ways end with the same energies and bounds.  Last line: one JSON object with every figure.  The output of
the run behind DESIGN.md 4.9's table is kept as profiles/trws_batch_timing.txt (redirect stdout there)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from bench import synthetic_volume
from helpers import grid_conn
from stereo_amd.trws import TrwsPlan, TrwsBatch

a = sys.argv[1:]
iters = int(a[0]) if len(a) > 0 else 10
runs = int(a[1]) if len(a) > 1 else 3
sizes = [int(x) for x in a[2].split(",")] if len(a) > 2 else [1, 2, 4, 8]
dev = torch.device("cuda", 0)
NEVER = -1e300


def volumes():
    g = np.load(os.path.join(ROOT, "tests", "golden", "teddy_pair.npz"))
    im0, im1 = g["im0"].astype(np.float64), g["im1"].astype(np.float64)
    from stereo_amd import terms as T
    H, W = im0.shape[:2]
    ncc = T.ncc_volume(im0, im1, np.arange(60, dtype=np.float64), 2, layout=1)
    # (members are different problems, like the frames of a sequence: the volume plus 1 % of its range in noise per member)
    base = np.ascontiguousarray(40.0 * (1.0 - ncc.T))
    yield "teddy 450x375x60", H, W, 60, 8.0, [base if i == 0 else base + np.random.default_rng(100 + i).uniform(0, 0.4, size=base.shape)
                                             for i in range(max(sizes))]
    yield "noise 128x128x16", 128, 128, 16, 8.0, [synthetic_volume(128, 128, 16, seed=1 + i) for i in range(max(sizes))]


def timed(fn):
    torch.cuda.synchronize(); t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


out = {}
for name, H, W, K, tol, unaries in volumes():
    conn = grid_conn(H, W); E = conn.shape[0]; N = H * W
    d_alpha = torch.ones(E, dtype=torch.float64, device=dev)
    d_pos = torch.arange(K, dtype=torch.float64, device=dev)
    d_un = {}
    for B in sizes:
        plans = []
        for i in range(B):
            if id(unaries[i]) not in d_un:
                d_un[id(unaries[i])] = torch.from_numpy(unaries[i]).to(dev)
            u = d_un[id(unaries[i])]
            p = TrwsPlan(1, K, N, conn.T)
            p.bind_device(u.data_ptr(), d_alpha.data_ptr(), tol, d_positions=d_pos.data_ptr(), keepalive=(u, d_alpha, d_pos))
            plans.append(p)
        batch = TrwsBatch(plans)
        rate = {"sequential": [], "batch": []}
        ends = {}
        for r in range(runs):
            for how in ("sequential", "batch"):
                batch.reset()
                if how == "sequential":
                    for p in plans: p.iterate(2, NEVER)
                    dt = timed(lambda: [p.iterate(iters, NEVER) for p in plans])
                else:
                    batch.iterate(2, NEVER)
                    dt = timed(lambda: batch.iterate(iters, NEVER))
                rate[how].append(B * iters / dt)
                ends[how] = [p.result(want_labels=False)[1:] for p in plans]
        assert ends["sequential"] == ends["batch"], (ends["sequential"], ends["batch"])
        med = {h: float(np.median(v)) for h, v in rate.items()}
        spread = max((max(v) - min(v)) / np.median(v) for v in rate.values())
        st = batch.stats()
        print("%s  B=%d  sequential %.2f it/s (%.2f .. %.2f)  batch %.2f it/s (%.2f .. %.2f)  batch/sequential %.3f  spread %.1f %%  floated %d  path %d"
              % (name, B, med["sequential"], min(rate["sequential"]), max(rate["sequential"]), med["batch"], min(rate["batch"]),
                 max(rate["batch"]), med["batch"] / med["sequential"], 100 * spread, st["floated"], plans[0].path()), flush=True)
        out["%s B=%d" % (name, B)] = dict(rate, ratio=med["batch"] / med["sequential"], spread=spread, capacity=st["capacity"])
        batch.close()
        for p in plans: p.close()
print(json.dumps(out))
