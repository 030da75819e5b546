"""Development tool: what the weighted scanline aggregation costs next to the unweighted one.
usage: time_scanline_weighted.py [output file] [runs=25] [calls per run=20]

The method is tools/time_scanline.py's: volumes of 375 x 450 x 60 and 2000 x 3000 x 64 (H x W x D; bench.py's synthetic
volume, label fastest), kernel 1, tol 8, positions 0 .. D - 1; between HIP events on one stream, after a warm-up, one run
is `calls` calls back to back and the figure is the time per call (runs and calls cut to 5 and 4 at the large size).
Per size, for 1 (horizontal), 4 and 8 directions, in the same run:
  unweighted       stereo_scanline_aggregate_device, every weight 1
  weighted         stereo_scanline_aggregate_weighted_device with the step weights of a random H x W x 3 image under
                   Contrast(1, 0.25, 0.1, 0.5) (values on the whole ramp, both ends included)
and once per size:
  step weights     stereo_contrast_step_weights_device for the 8 directions (C = 3)
  copy             a device-to-device copy that moves the builder's bytes: 8 (C + R) N = 88 N (44 N read, 44 N written)
Prints the median and min .. max of the runs in microseconds, the ratios weighted / unweighted and builder / copy, and as
the last line one JSON object with every run.  The output behind DESIGN.md's figures is kept as
profiles/scanline_weighted_timing.txt."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import ctypes as C
    import numpy as np, torch
    import stereo_amd
    import bench
    from stereo_amd import _lib, contrast, scanline
    if stereo_amd.device_count() < 1:
        raise SystemExit("time_scanline_weighted.py: no HIP device (timings are taken on the GPU only)")
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    runs0 = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    calls0 = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    stream = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    res, lines = {}, []
    rule = contrast.Contrast(1.0, 0.25, 0.1, 0.5)

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
        say("%-48s median %12.2f us  (%12.2f .. %12.2f)" % (key, v[len(v) // 2], v[0], v[-1]))
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
        gen = torch.Generator(device=dev)
        gen.manual_seed(3)
        d_image = torch.rand(3 * N, dtype=torch.float64, device=dev, generator=gen)
        d_wstep = torch.empty(8 * N, dtype=torch.float64, device=dev)
        L, err = _lib.lib(), _lib.errbuf()
        vp = lambda t: C.c_void_p(t.data_ptr())

        all8 = np.array(scanline.DIRECTIONS_8, dtype=np.int32).reshape(-1)
        par = rule._c()
        build = (vp(d_image), C.c_int(H), C.c_int(W), C.c_int(3), all8.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int(8), C.byref(par),
                 vp(d_wstep), C.c_void_p(stream.cuda_stream), err, C.c_size_t(len(err)))
        assert L.stereo_contrast_step_weights_device(*build) == 0, err.value
        t_build = measure("%s step weights, 8 directions" % who, lambda: L.stereo_contrast_step_weights_device(*build), runs, calls)
        src = torch.zeros(44 * N, dtype=torch.uint8, device=dev)
        dst = torch.zeros(44 * N, dtype=torch.uint8, device=dev)
        t_copy = measure("%s copy 88 N bytes" % who, lambda: dst.copy_(src), runs, calls)
        del src, dst
        say("%s step weights / copy %6.2f" % (who, t_build / t_copy))

        for name, dirs in (("1 direction (0, 1)", [(0, 1)]), ("4 directions", scanline.DIRECTIONS_4), ("8 directions", scanline.DIRECTIONS_8)):
            d = np.array(dirs, dtype=np.int32).reshape(-1)
            w = np.ones(len(dirs))
            # the step weights of exactly these directions, in their order
            d_w = contrast.step_weights_device(d_image, (H, W, 3), dirs, rule)
            head = (vp(d_unary), C.c_int(H), C.c_int(W), C.c_int(D), vp(d_pos), C.c_int(1), C.c_double(8.0),
                    d.ctypes.data_as(C.POINTER(C.c_int32)))
            tail = (C.c_int(len(dirs)), vp(d_S), vp(d_labels), vp(d_map), vp(d_conf), C.c_void_p(stream.cuda_stream), err,
                    C.c_size_t(len(err)))
            plain = head + (w.ctypes.data_as(C.POINTER(C.c_double)),) + tail
            weighted = head + (vp(d_w),) + tail
            assert L.stereo_scanline_aggregate_device(*plain) == 0, err.value
            assert L.stereo_scanline_aggregate_weighted_device(*weighted) == 0, err.value
            t_plain = measure("%s %s unweighted" % (who, name), lambda: L.stereo_scanline_aggregate_device(*plain), runs, calls)
            t_weighted = measure("%s %s weighted" % (who, name), lambda: L.stereo_scanline_aggregate_weighted_device(*weighted), runs, calls)
            say("%s %-20s weighted / unweighted %6.3f    step weights (8 directions) / weighted %6.3f"
                % (who, name, t_weighted / t_plain, t_build / t_weighted))
            del d_w
        del d_unary, d_S, d_image, d_wstep
        torch.cuda.empty_cache()
    say(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
