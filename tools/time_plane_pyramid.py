"""Development tool: what the two kernels of the plane pyramid cost on device-resident inputs.
usage: time_plane_pyramid.py [output file] [runs=25] [launches per run=20]

Shapes 375 x 450 and 2000 x 3000, a random 3-channel image; the expansion reads random slanted planes, the fit one
slanted surface with noise below tau (every tap inside the image takes part).  Per case, between HIP events on one
stream after a warm-up:
  expand planes   stereo_pyramid_expand_planes_device, guided (C = 3) and nearest, with `source`, called directly
  fit local       stereo_planes_fit_local_device at radius 2 and 4, tau = 1.5, called directly
  copy            a device-to-device copy of the bytes the kernel must move (half of them read, half written):
                  expand: the coarse planes (32 Nc), in the guided mode the two images (24 N + 24 Nc), the fine planes
                  (32 N) and source (4 N); fit: the planes in and out (64 N) -- the halo a tile reads again is not counted
One run is `launches` launches back to back; the figure is the time per launch: median and min .. max of `runs` runs
in microseconds and the ratio to the copy.  The last line is one JSON object with every run.  The output behind
DESIGN.md's figures is kept as profiles/plane_pyramid_timing.txt."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import ctypes as C
    import torch
    import stereo_amd
    from stereo_amd import _lib, pyramid
    if stereo_amd.device_count() < 1:
        raise SystemExit("time_plane_pyramid.py: no HIP device (timings are taken on the GPU only)")
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
        say("%-60s median %10.2f us  (%10.2f .. %10.2f)" % (key, v[len(v) // 2], v[0], v[-1]))
        return v[len(v) // 2]

    def against_copy(who, what, nbytes, call, elements):
        src = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
        t_copy = measure("%s copy of the bytes of %s" % (who, what), lambda: dst.copy_(src))
        del src, dst
        t = measure("%s %s" % (who, what), call)
        say("%s %s / copy %.2f   (%.1f MB, %.0f GB/s of the bytes it must move; %.1f ps per pixel)"
            % (who, what, t / t_copy, nbytes / 1e6, nbytes / t / 1e3, 1e6 * t / elements))

    L, err = _lib.lib(), _lib.errbuf()
    vp = lambda t: C.c_void_p(t.data_ptr())
    tail = (C.c_void_p(stream.cuda_stream), err, C.c_size_t(len(err)))
    say("%d runs of %d launches" % (runs, launches))
    for H, W in ((375, 450), (2000, 3000)):
        Hc, Wc = pyramid.coarse_size(H, W)
        N, Nc, Cn = H * W, Hc * Wc, 3
        gen = torch.Generator(device="cuda").manual_seed(H)
        rand = lambda *shape: torch.rand(*shape, dtype=torch.float64, device="cuda", generator=gen)

        def planes(n):                    # a, b in +-0.5, c = 1, disparities of a few tens
            p = rand(n, 4) - 0.5
            p[:, 2] = 1.0
            p[:, 3] = -60.0 * rand(n)
            return p.contiguous()

        d_coarse = planes(Nc)
        # the fit's input: one slanted surface with noise below tau, as fronto-parallel planes, so that every tap inside
        # the image takes part (the most work a pixel can have)
        i = torch.arange(N, dtype=torch.float64, device="cuda")
        d_fine_in = torch.zeros((N, 4), dtype=torch.float64, device="cuda")
        d_fine_in[:, 2] = 1.0
        d_fine_in[:, 3] = -(0.01 * torch.floor(i / H) + 0.02 * torch.remainder(i, H) + rand(N) - 0.5)
        d_im, d_red = 255.0 * rand(Cn, W, H), 255.0 * rand(Cn, Wc, Hc)
        d_out = torch.empty((N, 4), dtype=torch.float64, device="cuda")
        d_source = torch.empty((W, H), dtype=torch.int32, device="cuda")
        d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        who = "%d x %d:" % (H, W)
        for mode, name in ((1, "guided"), (0, "nearest")):
            args = (vp(d_coarse), C.c_int(Hc), C.c_int(Wc), C.c_int(H), C.c_int(W), C.c_int(mode), vp(d_im), vp(d_red),
                    C.c_int(Cn), vp(d_out), vp(d_source)) + tail
            assert L.stereo_pyramid_expand_planes_device(*args) == 0, err.value
            nbytes = 32 * Nc + 36 * N + (8 * Cn * (N + Nc) if mode == 1 else 0)
            against_copy(who, "expand planes, %s" % name, nbytes, lambda: L.stereo_pyramid_expand_planes_device(*args), N)
        for radius in (2, 4):
            args = (vp(d_fine_in), C.c_int(H), C.c_int(W), C.c_int(radius), C.c_double(1.5), vp(d_out), vp(d_bad)) + tail
            assert L.stereo_planes_fit_local_device(*args) == 0, err.value
            against_copy(who, "fit local, radius %d" % radius, 64 * N, lambda: L.stereo_planes_fit_local_device(*args), N)
        del d_coarse, d_fine_in, d_im, d_red, d_out, d_source
        torch.cuda.empty_cache()
    say(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
