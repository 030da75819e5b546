"""Development tool: what the two pyramid kernels cost on device-resident inputs.
usage: time_pyramid.py [output file] [runs=25] [launches per run=20]

Sizes 375 x 450 x 3 and 2000 x 3000 x 3, a random 0 .. 255 image, its reduction, a whole-pixel coarse map.  Per case,
between HIP events on one stream after a warm-up:
  reduce          stereo_pyramid_reduce_device: reads 8 H W C bytes, writes 8 Hc Wc C
  expand nearest  stereo_pyramid_expand_device, mode 0: reads 8 Hc Wc, writes 12 H W (the map and `source`)
  expand guided   mode 1: reads 8 Hc Wc (1 + C) + 8 H W C, writes 12 H W
  copy            a device-to-device copy that moves the same number of bytes (half of them read, half written)
One run is `launches` launches back to back; the figure is the time per launch: median and min .. max of `runs` runs
in microseconds and the ratio to the copy.  The last line is one JSON object with every run.  The output behind
DESIGN.md's figures is kept as profiles/pyramid_timing.txt."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import ctypes as C
    import torch
    import stereo_amd
    from stereo_amd import _lib, pyramid
    if stereo_amd.device_count() < 1:
        raise SystemExit("time_pyramid.py: no HIP device (timings are taken on the GPU only)")
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    launches = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    stream = torch.cuda.current_stream()
    res, lines = {}, []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(launches):
            fn()
        b.record(stream)
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / launches

    def measure(key, fn):
        for _ in range(3):
            timed(fn)                     # warm-up: code objects, the allocator, clocks
        res[key] = [timed(fn) for _ in range(runs)]
        v = sorted(res[key])
        say("%-44s median %10.2f us  (%10.2f .. %10.2f)" % (key, v[len(v) // 2], v[0], v[-1]))
        return v[len(v) // 2]

    def against_copy(who, what, nbytes, fn):
        half = nbytes // 2
        src = torch.zeros(half, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(half, dtype=torch.uint8, device="cuda")
        t_copy = measure("%s copy of %s's bytes" % (who, what), lambda: dst.copy_(src))
        del src, dst
        t = measure("%s %s" % (who, what), fn)
        say("%s %s / copy %.2f   (%.1f MB, %.0f GB/s of the bytes it must move)" % (who, what, t / t_copy, nbytes / 1e6, nbytes / t / 1e3))

    L, err = _lib.lib(), _lib.errbuf()
    vp = lambda t: C.c_void_p(t.data_ptr())
    tail = (C.c_void_p(stream.cuda_stream), err, C.c_size_t(len(err)))
    say("%d runs of %d launches" % (runs, launches))
    for H, W, Cn in ((375, 450, 3), (2000, 3000, 3)):
        Hc, Wc = pyramid.coarse_size(H, W)
        gen = torch.Generator(device="cuda").manual_seed(H)
        d_im = torch.randint(0, 256, (Cn, W, H), device="cuda", generator=gen).to(torch.float64)
        d_red = pyramid.reduce_device(d_im)
        d_coarse = torch.randint(0, 64, (Wc, Hc), device="cuda", generator=gen).to(torch.float64)
        d_out = torch.empty((W, H), dtype=torch.float64, device="cuda")
        d_src = torch.empty((W, H), dtype=torch.int32, device="cuda")
        who = "%d x %d x %d" % (H, W, Cn)
        sizes = (C.c_int(Hc), C.c_int(Wc), C.c_int(H), C.c_int(W))
        red_args = (vp(d_im), C.c_int(H), C.c_int(W), C.c_int(Cn), vp(d_red)) + tail
        near_args = (vp(d_coarse),) + sizes + (C.c_int(0), None, None, C.c_int(Cn), vp(d_out), vp(d_src)) + tail
        guided_args = (vp(d_coarse),) + sizes + (C.c_int(1), vp(d_im), vp(d_red), C.c_int(Cn), vp(d_out), vp(d_src)) + tail
        for fn, a in ((L.stereo_pyramid_reduce_device, red_args), (L.stereo_pyramid_expand_device, near_args),
                      (L.stereo_pyramid_expand_device, guided_args)):
            assert fn(*a) == 0, err.value
        against_copy(who, "reduce", 8 * Cn * (H * W + Hc * Wc), lambda: L.stereo_pyramid_reduce_device(*red_args))
        against_copy(who, "expand nearest", 8 * Hc * Wc + 12 * H * W, lambda: L.stereo_pyramid_expand_device(*near_args))
        against_copy(who, "expand guided", 8 * Hc * Wc * (1 + Cn) + 8 * H * W * Cn + 12 * H * W,
                     lambda: L.stereo_pyramid_expand_device(*guided_args))
        share = torch.bincount(d_src.reshape(-1) + 1, minlength=5).cpu().numpy() / float(H * W)
        say("%s guided: share of pixels per source -1, 0 .. 3: %s" % (who, " ".join("%.3f" % s for s in share)))
        del d_im, d_red, d_coarse, d_out, d_src
        torch.cuda.empty_cache()
    say(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
