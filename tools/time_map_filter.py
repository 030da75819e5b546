"""Development tool: what the map filter costs.
usage: time_map_filter.py [output file] [runs=25] [calls per run=20]

The method is tools/time_scanline_weighted.py's: device-resident arrays, between HIP events on one stream, after a warm-up,
one run is `calls` calls of stereo_map_weighted_median_device back to back and the figure is the time per call (runs and
calls cut to 5 and 4 at the large size).  Maps of 375 x 450 and 2000 x 3000 (H x W) of random normal values (no ties: every
comparison decides), for r = 1, 2 and 4:
  unguided           no image, no pixel_weight: the instantiation without a multiply
  guided             a random H x W x 3 image under Contrast(1, 0.25, 0.1, 0.5) (values on the whole ramp)
  weighted           no image, pixel_weight = 1 off the targets and 0 on them: what MedianFilter(r) asks for
each with every pixel a target, with 10 % of the pixels as targets in vertical stripes 4 pixels wide every 40 columns
(Teddy-like: occlusions are slivers beside depth edges; most 64 x 4 tiles hold no target and leave early) and with a
scattered 10 % (every tile holds targets, every wave runs the loop with a tenth of its lanes).  At r = 4, unguided, two more
target sets that keep every wave in the loop with half its lanes: the first 32 lanes of every wave (rows y mod 64 < 32) and
every other lane (even rows).
Once per size: a device-to-device copy of the 16 N bytes the filter must move (8 N read, 8 N written).
Prints the median and min .. max of the runs in microseconds, the ratio to the copy and the time per target and
compare-select-add step, and as the last line one JSON object with every run.  The output behind DESIGN.md's figures is
kept as profiles/map_filter_timing.txt."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import ctypes as C
    import torch
    import stereo_amd
    from stereo_amd import _lib, contrast, mapfilter
    if stereo_amd.device_count() < 1:
        raise SystemExit("time_map_filter.py: no HIP device (timings are taken on the GPU only)")
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    runs0 = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    calls0 = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    stream = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    res, lines = {}, []
    rule = contrast.Contrast(1.0, 0.25, 0.1, 0.5)
    L, err = _lib.lib(), _lib.errbuf()
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

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
        return v[len(v) // 2], v[0], v[-1]

    for H, W in ((375, 450), (2000, 3000)):
        N = H * W
        large = N > (1 << 20)
        runs, calls = (min(runs0, 5), min(calls0, 4)) if large else (runs0, calls0)
        who = "%d x %d" % (H, W)
        say("%s: %d runs of %d calls" % (who, runs, calls))
        gen = torch.Generator(device=dev)
        gen.manual_seed(3)
        d_map = torch.randn((W, H), dtype=torch.float64, device=dev, generator=gen)
        d_image = torch.rand(3 * N, dtype=torch.float64, device=dev, generator=gen)
        d_out = torch.empty((W, H), dtype=torch.float64, device=dev)
        d_source = torch.empty((W, H), dtype=torch.int32, device=dev)
        d_kept = torch.zeros(1, dtype=torch.int32, device=dev)
        stripes = ((torch.arange(W, device=dev) % 40) < 4).to(torch.int32)[:, None].expand(W, H).contiguous()
        scattered = (torch.rand((W, H), device=dev, generator=gen) < 0.1).to(torch.int32)
        src = torch.zeros(8 * N, dtype=torch.uint8, device=dev)
        dst = torch.zeros(8 * N, dtype=torch.uint8, device=dev)
        t_copy, lo, hi = measure("%s copy 16 N bytes" % who, lambda: dst.copy_(src), runs, calls)
        say("%-58s median %12.2f us  (%12.2f .. %12.2f)" % ("%s copy 16 N bytes" % who, t_copy, lo, hi))
        del src, dst
        for r in (1, 2, 4):
            steps = (2 * r + 1) ** 4
            for tname, targets in (("all targets", None), ("10 % in stripes", stripes), ("10 % scattered", scattered)):
                n_targets = N if targets is None else int(targets.sum().item())
                voters = None if targets is None else (targets == 0).to(torch.float64)
                for kind, image, c, pw in (("unguided", None, None, None), ("guided", d_image, rule, None),
                                           ("weighted", None, None, voters)):
                    if kind == "weighted" and targets is None:
                        continue                       # (nobody left to vote)
                    shape = (H, W, 3) if image is not None else (H, W)
                    mapfilter.weighted_median_device(d_map, shape, r, image, c, pw, targets, out=d_out, source=d_source,
                                                     kept=d_kept, stream=stream)          # (the wrapper's checks, once)
                    par = c._c() if c is not None else None
                    args = (vp(d_map), C.c_int(H), C.c_int(W), C.c_int(r), vp(image), C.c_int(3 if image is not None else 0),
                            C.byref(par) if par is not None else None, vp(pw), vp(targets), vp(d_out), vp(d_source),
                            vp(d_kept), C.c_void_p(stream.cuda_stream), err, C.c_size_t(len(err)))
                    fn = lambda: L.stereo_map_weighted_median_device(*args)
                    assert fn() == 0, err.value
                    key = "%s r=%d %-9s %s" % (who, r, kind, tname)
                    t, lo, hi = measure(key, fn, runs, calls)
                    say("%-58s median %12.2f us  (%12.2f .. %12.2f)   / copy %8.1f   %7.2f ns per target, %6.2f ps per step"
                        % (key, t, lo, hi, t / t_copy, 1e3 * t / n_targets, 1e6 * t / n_targets / steps))
        rows = torch.arange(H, device=dev)[None, :].expand(W, H)
        for tname, targets in (("lanes 0 .. 31 of every wave", ((rows % 64) < 32).to(torch.int32).contiguous()),
                               ("every other lane", ((rows % 2) == 0).to(torch.int32).contiguous())):
            args = (vp(d_map), C.c_int(H), C.c_int(W), C.c_int(4), None, C.c_int(0), None, None, vp(targets), vp(d_out),
                    vp(d_source), vp(d_kept), C.c_void_p(stream.cuda_stream), err, C.c_size_t(len(err)))
            fn = lambda: L.stereo_map_weighted_median_device(*args)
            assert fn() == 0, err.value
            key = "%s r=4 unguided  %s" % (who, tname)
            t, lo, hi = measure(key, fn, runs, calls)
            say("%-58s median %12.2f us  (%12.2f .. %12.2f)   / copy %8.1f" % (key, t, lo, hi, t / t_copy))
        del d_map, d_image, d_out, d_source, stripes, scattered, rows
        torch.cuda.empty_cache()
    say(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
