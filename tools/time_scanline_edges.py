"""Development tool: what scanline aggregation on per-edge positions costs on device-resident inputs.
usage: time_scanline_edges.py [output file] [runs=15] [calls per run=10] [sizes=375x450,2000x3000]

Per size (H x W) and K = 9, 17, 27, 64: bench.py's synthetic volume as the unary (label fastest), the image grid with two
edges per pair (construct_neighborhood, what a level has), q and qprim uniform in [0, 8), alphas 1, tol 2.  Between HIP
events on one stream, after a warm-up, for both kernels:
  (0, 1), (1, 0), 4 directions   stereo_scanline_edges_aggregate_device, the C entry with its arguments built once (the
                   call's reduction to labels, which reads S once more, is included in every figure)
and, with kernel 1, against three things in the same run:
  copy             a device-to-device copy of the bytes ONE direction must move: 8 K N of U, 16 K N of S read and
                   written, 32 K N of the four edge rows per step = 56 K N bytes (28 K N read, 28 K N written)
  shared           stereo_scanline_aggregate_device at D = K on one shared positions vector, the same directions
  TRW-S iteration  one iteration of a TrwsPlan bound to the same unary, q, qprim and alphas, wall clock around
                   plan.iterate(n) after a warm-up, n = 10 (2 at the large size), median of 3
One run is `calls` calls back to back; the figure is the time per call.  At the large size the runs and calls are cut to
3 and 2.  Prints the median and min .. max of the runs in microseconds, the ratios, and as the last line one JSON object
with every run.  The output behind DESIGN.md's figures is kept as profiles/scanline_edges_timing.txt."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = (("(0, 1)", [(0, 1)]), ("(1, 0)", [(1, 0)]), ("4 directions", [(0, 1), (0, -1), (1, 0), (-1, 0)]))


def main():
    import ctypes as C
    import numpy as np, torch
    import stereo_amd
    import bench
    from stereo_amd import _lib, scanline, terms as T
    from stereo_amd.trws import TrwsPlan
    if stereo_amd.device_count() < 1:
        raise SystemExit("time_scanline_edges.py: no HIP device (timings are taken on the GPU only)")
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    runs0 = int(sys.argv[2]) if len(sys.argv) > 2 else 15
    calls0 = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    sizes = [tuple(int(v) for v in s.split("x")) for s in (sys.argv[4] if len(sys.argv) > 4 else "375x450,2000x3000").split(",")]
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
        say("%-52s median %12.2f us  (%12.2f .. %12.2f)" % (key, v[len(v) // 2], v[0], v[-1]))
        return v[len(v) // 2]

    L, err = _lib.lib(), _lib.errbuf()
    vp = lambda t: C.c_void_p(t.data_ptr())
    for H, W in sizes:
        N = H * W
        large = N > (1 << 20)
        runs, calls = (min(runs0, 3), min(calls0, 2)) if large else (runs0, calls0)
        conn = T.construct_neighborhood(H, W)
        E = conn.shape[1]
        d_conn = torch.from_numpy(np.asfortranarray(conn, dtype=np.uint32).reshape(-1, order="F").view(np.int32)).to(dev)
        table, _ = scanline.edge_table_device(d_conn, E, (H, W))
        d_alphas = torch.ones(E, dtype=torch.float64, device=dev)
        for K in (9, 17, 27, 64):
            who = "%d x %d K = %d" % (H, W, K)
            say("%s: E = %d, %d runs of %d calls" % (who, E, runs, calls))
            d_unary = bench.synthetic_volume_device(H, W, K, 1, dev).reshape(-1).contiguous()
            gen = torch.Generator(device=dev).manual_seed(K)
            d_q = torch.rand(K * E, dtype=torch.float64, device=dev, generator=gen) * 8.0
            d_qprim = torch.rand(K * E, dtype=torch.float64, device=dev, generator=gen) * 8.0
            d_S = torch.empty(K * N, dtype=torch.float64, device=dev)
            d_labels = torch.empty(N, dtype=torch.int32, device=dev)
            d_map = torch.empty((W, H), dtype=torch.float64, device=dev)
            d_conf = torch.empty((W, H), dtype=torch.float64, device=dev)
            src = torch.zeros(28 * K * N, dtype=torch.uint8, device=dev)
            dst = torch.zeros(28 * K * N, dtype=torch.uint8, device=dev)
            t_copy = measure("%s copy 56 K N bytes" % who, lambda: dst.copy_(src), runs, calls)
            del src, dst
            d_pos = torch.arange(K, dtype=torch.float64, device=dev)
            t_edges, t_shared = {}, {}
            for name, dirs in SETS:
                d = np.array(dirs, dtype=np.int32).reshape(-1)
                w = np.ones(len(dirs))
                dp = d.ctypes.data_as(C.POINTER(C.c_int32))
                for kernel in (1, 2):
                    args = (C.c_int(kernel), vp(d_unary), C.c_int(H), C.c_int(W), C.c_int(K), C.c_int64(E), vp(table), vp(d_q), vp(d_qprim),
                            vp(d_alphas), C.c_double(2.0), dp, C.c_int(len(dirs)), vp(d_S), vp(d_labels), vp(d_conf),
                            C.c_void_p(stream.cuda_stream), err, C.c_size_t(len(err)))
                    assert L.stereo_scanline_edges_aggregate_device(*args) == 0, err.value
                    t = measure("%s edges kernel %d %s" % (who, kernel, name), lambda: L.stereo_scanline_edges_aggregate_device(*args), runs, calls)
                    if kernel == 1:
                        t_edges[name] = t
                sargs = (vp(d_unary), C.c_int(H), C.c_int(W), C.c_int(K), vp(d_pos), C.c_int(1), C.c_double(2.0), dp,
                         w.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(len(dirs)), vp(d_S), vp(d_labels), vp(d_map), vp(d_conf),
                         C.c_void_p(stream.cuda_stream), err, C.c_size_t(len(err)))
                assert L.stereo_scanline_aggregate_device(*sargs) == 0, err.value
                t_shared[name] = measure("%s shared kernel 1 %s" % (who, name), lambda: L.stereo_scanline_aggregate_device(*sargs), runs, calls)
            plan = TrwsPlan(1, K, N, conn)
            torch.cuda.synchronize()
            plan.bind_device(d_unary.data_ptr(), d_alphas.data_ptr(), 2.0, d_q=d_q.data_ptr(), d_qprim=d_qprim.data_ptr(),
                             keepalive=(d_unary, d_alphas, d_q, d_qprim))
            n = 2 if large else 10
            plan.iterate(1 if large else 3, NEVER)
            t_iter = []
            for _ in range(3):
                t0 = time.perf_counter()
                plan.iterate(n, NEVER)
                t_iter.append(1e6 * (time.perf_counter() - t0) / n)
            plan.close()
            res["%s TRW-S iteration" % who] = t_iter
            v = sorted(t_iter)
            t_trws = v[len(v) // 2]
            say("%-52s median %12.2f us  (%12.2f .. %12.2f)   [wall clock, %d iterations per run]" % ("%s TRW-S iteration" % who, t_trws, v[0], v[-1], n))
            for name, dirs in SETS:
                R = len(dirs)
                say("%s edges %-14s / (%d x copy) %6.2f    / shared %6.2f    / TRW-S iteration %6.3f"
                    % (who, name, R, t_edges[name] / (R * t_copy), t_edges[name] / t_shared[name], t_edges[name] / t_trws))
            del d_unary, d_S, d_q, d_qprim
            torch.cuda.empty_cache()
    say(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
