"""Development tool: cost of the TRW-S node beliefs on the Teddy NCC volume (450 x 375 x 60, kernel 1,
tol 8, unit weights, fronto-parallel labels; built as tools/time_trws.py ... volume=teddy builds it).
usage: time_trws_min_marginals.py [iters=20] [--profile]
  - iteration time with beliefs off and on, alternating, three runs each (fresh plan per run, two warm-up iterations);
  - the phase-2 call (stereo_trws_plan_min_marginals_device into torch tensors);
  - bytes of both kernels from the shapes and the share of the 8 TB/s HBM peak at the measured times (phase 1: the
    overhead per iteration; phase 2: the call);
  - with --profile, both kernels under rocprofv3 --kernel-trace --stats in a child process of their own (a second
    JSON line; the child's output goes to mm_prof.log in the profile directory).
Prints one JSON line (two with --profile)."""
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from helpers import grid_conn  # noqa: E402
from stereo_amd.trws import TrwsPlan  # noqa: E402

K, TOL, PEAK = 60, 8.0, 8e12


def teddy_volume(dev):
    from stereo_amd import terms as T
    g = np.load(os.path.join(ROOT, "tests", "golden", "teddy_pair.npz"))
    im0, im1 = g["im0"].astype(np.float64), g["im1"].astype(np.float64)
    H, W = im0.shape[:2]
    ncc = T.ncc_volume(im0, im1, np.arange(K, dtype=np.float64), 2, layout=1)
    return H, W, torch.from_numpy(np.ascontiguousarray(40.0 * (1.0 - ncc.T))).to(dev)


def make_plan(H, W, d_unary, dev, beliefs):
    conn = grid_conn(H, W)
    E, N = conn.shape[0], H * W
    plan = TrwsPlan(1, K, N, conn.T)
    d_alpha = torch.ones(E, dtype=torch.float64, device=dev)
    d_pos = torch.arange(K, dtype=torch.float64, device=dev)
    plan.bind_device(d_unary.data_ptr(), d_alpha.data_ptr(), TOL, d_positions=d_pos.data_ptr(), keepalive=(d_unary, d_alpha, d_pos))
    if beliefs:
        plan.keep_min_marginals()
    return plan, N, E


def timed_run(H, W, d_unary, dev, beliefs, iters):
    plan, N, E = make_plan(H, W, d_unary, dev, beliefs)
    plan.iterate(2, max_relgap=-1e300)
    torch.cuda.synchronize(); t = time.perf_counter()
    plan.iterate(iters, max_relgap=-1e300)
    dt = (time.perf_counter() - t) / iters
    _, en, lb, _ = plan.result(want_labels=False)
    phase2 = None
    if beliefs:
        mm = torch.empty((N, K), dtype=torch.float64, device=dev)
        conf = torch.empty(N, dtype=torch.float64, device=dev)
        am = torch.empty(N, dtype=torch.int32, device=dev)
        plan.min_marginals_device(mm.data_ptr(), conf.data_ptr(), am.data_ptr())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(10):
            plan.min_marginals_device(mm.data_ptr(), conf.data_ptr(), am.data_ptr(), torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        phase2 = e0.elapsed_time(e1) / 1e3 / 10
    plan.close()
    return dt, en, lb, phase2, N, E


def profile_child(iters):
    """The kernels under rocprofv3 in a fresh child process; returns {kernel: (calls, average ns)}."""
    out = tempfile.mkdtemp(prefix="mm_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "mm", "--",
           sys.executable, os.path.abspath(__file__), str(iters), "--child"]
    with open(os.path.join(out, "mm_prof.log"), "w") as log:
        rc = subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT, timeout=300).returncode
    res = dict(profile_dir=out, rc=rc)
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        import csv
        for row in csv.DictReader(open(f)):
            for name in ("trws_beliefs_accum_kernel", "trws_beliefs_finish_kernel"):
                if name in row["Name"]:
                    res[name] = (int(row["Calls"]), float(row["AverageNs"]))
    return res


def main():
    a = [x for x in sys.argv[1:] if not x.startswith("--")]
    iters = int(a[0]) if a else 20
    dev = torch.device("cuda", 0)
    H, W, d_unary = teddy_volume(dev)
    if "--child" in sys.argv:   # (the profiled process: a few iterations and phase-2 calls with beliefs on)
        timed_run(H, W, d_unary, dev, True, iters)
        return
    runs = {False: [], True: []}
    ref = {}
    p2 = []
    for _ in range(3):
        for on in (False, True):
            dt, en, lb, phase2, N, E = timed_run(H, W, d_unary, dev, on, iters)
            runs[on].append(dt * 1e3)
            ref.setdefault(on, (en, lb))
            if phase2 is not None:
                p2.append(phase2 * 1e3)
    off, on = float(np.median(runs[False])), float(np.median(runs[True]))
    out = dict(workload="Teddy NCC volume %dx%dx%d, kernel 1, tol %g, %d iterations per run" % (W, H, K, TOL, iters),
               ms_per_iteration_off=runs[False], ms_per_iteration_on=runs[True],
               overhead_ms=on - off, overhead_pct=100.0 * (on - off) / off,
               results_equal=ref[False] == ref[True], phase2_call_ms=p2)
    bytes1 = 8.0 * K * (2 * N + E)
    bytes2 = 8.0 * K * (2 * N + E) + 12.0 * N
    p2m = float(np.median(p2))
    out["phase1_from_overhead"] = dict(bytes=bytes1, hbm_frac=bytes1 / max(on - off, 1e-9) * 1e3 / PEAK)
    out["phase2_from_call"] = dict(bytes=bytes2, hbm_frac=bytes2 / (p2m * 1e-3) / PEAK)
    print(json.dumps(out), flush=True)
    if "--profile" in sys.argv:
        prof = profile_child(5)
        for name, b in (("trws_beliefs_accum_kernel", bytes1), ("trws_beliefs_finish_kernel", bytes2)):
            if name in prof:
                calls, ns = prof[name]
                prof[name] = dict(calls=calls, avg_us=ns / 1e3, bytes=b, hbm_frac=b / (ns * 1e-9) / PEAK)
        print(json.dumps(prof))


if __name__ == "__main__":
    main()
