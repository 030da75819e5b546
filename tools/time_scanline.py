"""Development tool: what the scanline aggregation costs on a device-resident volume.
usage: time_scanline.py [output file] [runs=25] [calls per run=20]

Volumes of 375 x 450 x 60 and 2000 x 3000 x 64 (H x W x D; bench.py's synthetic volume, label fastest), kernel 1, tol 8,
positions 0 .. D - 1, every weight 1.  Per size, between HIP events on one stream, after a warm-up:
  4 directions, 8 directions   stereo_scanline_aggregate_device, the C entry with its arguments built once
  horizontal / vertical / diagonal   one direction of each class alone (the call's reduction to labels, which reads S
                   once more, is included in every figure)
  copy             a device-to-device copy of the bytes ONE direction must move, 8 D N read + 16 D N read and written
                   = 24 D N bytes (12 D N read, 12 D N written); a call of R directions is held against R times that
  TRW-S iteration  one iteration of the same volume on a TrwsPlan bound to the same tensor (grid edges, alphas 1), wall
                   clock around plan.iterate(n) after a warm-up, n = 20 (5 at the large size), median of 5
One run is `calls` calls back to back; the figure is the time per call.  At the large size the runs and calls are cut to
5 and 4 (a call moves 74 GB).  Prints the median and min .. max of the runs in microseconds, the ratios, and as the last line
one JSON object with every run.  The output behind DESIGN.md's figures is kept as profiles/scanline_timing.txt."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HORIZONTAL, VERTICAL, DIAGONAL = (0, 1), (1, 0), (1, 1)


def main():
    import ctypes as C
    import numpy as np, torch
    import stereo_amd
    import bench
    from helpers import grid_conn
    from stereo_amd import _lib, scanline
    from stereo_amd.trws import TrwsPlan
    if stereo_amd.device_count() < 1:
        raise SystemExit("time_scanline.py: no HIP device (timings are taken on the GPU only)")
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    runs0 = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    calls0 = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    stream = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    res, lines = {}, []
    NEVER = -1e300

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def timed(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(calls):
            fn()
        b.record(stream)
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / calls

    def measure(key, fn, runs, calls):
        for _ in range(2):
            timed(fn, calls)                     # warm-up: code objects, the allocator, clocks
        res[key] = [timed(fn, calls) for _ in range(runs)]
        v = sorted(res[key])
        say("%-44s median %12.2f us  (%12.2f .. %12.2f)" % (key, v[len(v) // 2], v[0], v[-1]))
        return v[len(v) // 2]

    for H, W, D in ((375, 450, 60), (2000, 3000, 64)):
        N = H * W
        large = N * D > (1 << 28)
        runs, calls = (min(runs0, 5), min(calls0, 4)) if large else (runs0, calls0)
        who = "%d x %d x %d" % (H, W, D)
        say("%s: %d runs of %d calls" % (who, runs, calls))
        if large:
            d_unary = bench.synthetic_volume_device(H, W, D, 1, dev).reshape(-1).contiguous()
        else:
            d_unary = torch.from_numpy(bench.synthetic_volume(H, W, D, seed=1)).to(dev).reshape(-1).contiguous()
        positions = np.arange(D, dtype=np.float64)
        d_pos = torch.from_numpy(positions).to(dev)
        d_S = torch.empty(D * N, dtype=torch.float64, device=dev)
        d_labels = torch.empty(N, dtype=torch.int32, device=dev)
        d_map = torch.empty((W, H), dtype=torch.float64, device=dev)
        d_conf = torch.empty((W, H), dtype=torch.float64, device=dev)
        src = torch.zeros(12 * D * N, dtype=torch.uint8, device=dev)
        dst = torch.zeros(12 * D * N, dtype=torch.uint8, device=dev)
        t_copy = measure("%s copy 24 D N bytes" % who, lambda: dst.copy_(src), runs, calls)
        del src, dst
        L, err = _lib.lib(), _lib.errbuf()
        vp = lambda t: C.c_void_p(t.data_ptr())
        t_dirs = {}
        for name, dirs in (("4 directions", scanline.DIRECTIONS_4), ("8 directions", scanline.DIRECTIONS_8),
                           ("horizontal (0, 1)", [HORIZONTAL]), ("vertical (1, 0)", [VERTICAL]), ("diagonal (1, 1)", [DIAGONAL])):
            d = np.array(dirs, dtype=np.int32).reshape(-1)
            w = np.ones(len(dirs))
            args = (vp(d_unary), C.c_int(H), C.c_int(W), C.c_int(D), vp(d_pos), C.c_int(1), C.c_double(8.0),
                    d.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(len(dirs)),
                    vp(d_S), vp(d_labels), vp(d_map), vp(d_conf), C.c_void_p(stream.cuda_stream), err, C.c_size_t(len(err)))
            assert L.stereo_scanline_aggregate_device(*args) == 0, err.value
            t_dirs[name] = measure("%s %s" % (who, name), lambda: L.stereo_scanline_aggregate_device(*args), runs, calls)
        # one TRW-S iteration of the same volume
        conn = grid_conn(H, W)
        plan = TrwsPlan(1, D, N, conn.T)
        d_alpha = torch.ones(conn.shape[0], dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        plan.bind_device(d_unary.data_ptr(), d_alpha.data_ptr(), 8.0, d_positions=d_pos.data_ptr(), keepalive=(d_unary, d_alpha, d_pos))
        n = 5 if large else 20
        plan.iterate(3, NEVER)
        t_iter = []
        for _ in range(5):
            t0 = time.perf_counter()
            plan.iterate(n, NEVER)
            t_iter.append(1e6 * (time.perf_counter() - t0) / n)
        plan.close()
        res["%s TRW-S iteration" % who] = t_iter
        v = sorted(t_iter)
        t_trws = v[len(v) // 2]
        say("%-44s median %12.2f us  (%12.2f .. %12.2f)   [wall clock, %d iterations per run]" % ("%s TRW-S iteration" % who, t_trws, v[0], v[-1], n))
        for name, t in t_dirs.items():
            R = 4 if name.startswith("4") else 8 if name.startswith("8") else 1
            say("%s %-20s / (%d x copy) %6.2f    / TRW-S iteration %6.3f" % (who, name, R, t / (R * t_copy), t / t_trws))
        del d_unary, d_S, d_alpha
        torch.cuda.empty_cache()
    say(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
