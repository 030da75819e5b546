"""Development tool: randomised parity stress of the large-label kernel (512 < K <= 4096, one shared
strictly ascending positions vector; stereo_trws_plan_path 5) against the CPU oracle, in the style of
stress_trws.py: small graphs, both smoothness kernels, both message modes, node order, integer ties,
flat unaries and out-of-range proposals drawn at random.  The reference's own message classes serve as the
oracle up to K = 1024 where they are built (they re-sort every column: slow beyond), the restatement above.
usage: stress_trws_large.py [seconds=60] [seed=0]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from stereo_amd.trws import TrwsPlan
from helpers import trws_problem
from oracle import pyoracle as po

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
ref_types = po.ref_types() is not None
t0, n, bad, serial, messages = time.time(), 0, 0, 0, 0
modes = {}
while time.time() - t0 < budget:
    K = int(rng.integers(513, 4097))
    H, W = int(rng.integers(1, 6)), int(rng.integers(2, 7))
    kernel = int(rng.choice([1, 1, 2]))
    integer = bool(rng.integers(0, 4) == 0)
    tol = float(rng.choice([0.0, 2.0, 8.0, 40.0, 1e9]))
    iters = int(rng.integers(1, 4))
    seed = int(rng.integers(0, 1 << 30))
    p = trws_problem(seed, H, W, K, kind="fronto", integer=integer)
    look = int(rng.integers(0, 4))
    if look == 1:    # flat: most sources useful
        p["unary"] = p["unary"] * 0.02
    elif look == 2:  # out-of-range plane proposals (dispmap_ncc.m:245)
        p["unary"] = np.where(rng.random(p["unary"].shape) < 0.1, 4e7 + p["unary"], p["unary"])
    kind = int(rng.integers(0, 3))
    if kind == 0:
        pos = np.arange(K, dtype=np.float64)
    elif kind == 1:
        pos = np.arange(K, dtype=np.float64) * float(rng.choice([0.0625, 0.25, 0.5])) - 3.0
    else:
        pos = np.cumsum(rng.uniform(0.05, 2.0, size=K))
    if integer:
        pos = np.arange(K, dtype=np.float64)
    minplus = bool(rng.integers(0, 4) == 0)
    ordering = int(rng.integers(0, 4) == 0)
    q = np.tile(pos, (p["conn"].shape[0], 1))
    ref = po.trws(kernel, p["unary"], p["conn"], q, q, p["alphas"], tol, iters, -1e300, mode=0 if minplus else 1,
                  use_ref_types=ref_types and not minplus and K <= 1024, ordering=ordering)
    plan = TrwsPlan(kernel, K, H * W, p["conn"].T, message_mode=(1 if minplus else 0) | (0x100 if ordering else 0))
    plan.upload(p["unary"].T, p["alphas"], tol, positions=pos)
    plan.iterate(iters, max_relgap=-1e300)
    got = plan.result()
    path = plan.path()
    if not minplus:
        serial += plan.serial_messages()
        messages += p["conn"].shape[0] * (2 * iters + 1)
    plan.close()
    ok = path == 5 and np.array_equal(got[0], ref[0]) and got[1] == ref[1] and got[2] == ref[2] and got[3] == ref[3]
    modes[(kernel, minplus, ordering)] = modes.get((kernel, minplus, ordering), 0) + 1
    n += 1
    if not ok:
        bad += 1
        print("MISMATCH", dict(seed=seed, H=H, W=W, K=K, kernel=kernel, integer=integer, look=look, pos=kind, tol=tol,
                               iters=iters, path=path, minplus=minplus, ordering=ordering))
print("stress_large: %d problems, %d mismatches, %.0f s, oracle %s, serial messages %d of %d exact" % (
    n, bad, time.time() - t0, "reference types (K <= 1024)" if ref_types else "restatement", serial, messages))
print("(kernel, minplus, index order) -> problems:", sorted(modes.items()))
sys.exit(1 if bad else 0)
