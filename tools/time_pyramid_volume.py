"""Development tool: what the volume reduction of the image pyramid costs on device-resident inputs.
usage: time_pyramid_volume.py [output file] [runs=25] [launches per run=20]

Shapes 375 x 450 x 60 -> 31 slices and 2000 x 3000 x 256 -> 129 slices (the slices 0 .. D - 1, the next level's slices
and sample positions as level_disparities / level_sample_at give them), a random volume in [-1, 1], both layouts.  Per
case, between HIP events on one stream after a warm-up:
  reduce volume   stereo_pyramid_reduce_volume_device, called directly
  copy            a device-to-device copy of the bytes the kernel must move (half of them read, half written): the
                  lines of the finer volume it touches -- per sample the nearest slice and its two neighbours; layout 0:
                  whole slices, layout 1: the 128-byte lines of every pixel's column that hold one -- plus the output
One run is `launches` launches back to back; the figure is the time per launch: median and min .. max of `runs` runs
in microseconds and the ratio to the copy.  The last line is one JSON object with every run.  The output behind
DESIGN.md's figures is kept as profiles/pyramid_volume_timing.txt."""
import json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def touched_bytes(H, W, slices, sample_at, layout):
    """Bytes of the finer volume in the lines the kernel reads (module docstring)."""
    import numpy as np
    D = slices.shape[0]
    touched = np.zeros(D, bool)
    for d in sample_at:
        dist = np.abs(d - slices)
        t = int(np.flatnonzero(dist <= dist.min())[-1])          # the nearest slice, ties to the larger index
        touched[max(t - 1, 0):min(t + 1, D - 1) + 1] = True
    if layout == 0:
        return 8 * H * W * int(touched.sum())
    period = D * 16 // math.gcd(D, 16)                            # elements after which columns and lines line up again
    lines = np.tile(touched, period // D).reshape(-1, 16).any(axis=1)
    return int(128 * float(lines.sum()) * (float(H) * W * D / period))


def main():
    import ctypes as C
    import numpy as np
    import torch
    import stereo_amd
    from stereo_amd import _lib, pyramid
    if stereo_amd.device_count() < 1:
        raise SystemExit("time_pyramid_volume.py: no HIP device (timings are taken on the GPU only)")
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

    L, err = _lib.lib(), _lib.errbuf()
    vp = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    say("%d runs of %d launches" % (runs, launches))
    for H, W, D in ((375, 450, 60), (2000, 3000, 256)):
        Hc, Wc = pyramid.coarse_size(H, W)
        slices = np.arange(D, dtype=np.float64)
        coarser = pyramid.level_disparities(slices, 1)
        sample_at = np.ascontiguousarray(pyramid.level_sample_at(slices, coarser))
        Kc = sample_at.shape[0]
        gen = torch.Generator(device="cuda").manual_seed(H)
        d_vol = torch.rand(H * W * D, dtype=torch.float64, device="cuda", generator=gen) * 2.0 - 1.0
        d_out = torch.empty(Hc * Wc * Kc, dtype=torch.float64, device="cuda")
        d_slices, d_sample_at = torch.from_numpy(slices).cuda(), torch.from_numpy(sample_at).cuda()
        for layout in (1, 0):
            who = "%d x %d x %d -> %d slices, layout %d:" % (H, W, D, Kc, layout)
            args = (vp(d_vol), C.c_int(H), C.c_int(W), C.c_int(D), C.c_int(layout), hp(slices), vp(d_slices), hp(sample_at),
                    vp(d_sample_at), C.c_int(Kc), vp(d_out), C.c_void_p(stream.cuda_stream), err, C.c_size_t(len(err)))
            assert L.stereo_pyramid_reduce_volume_device(*args) == 0, err.value
            nbytes = touched_bytes(H, W, slices, sample_at, layout) + 8 * Hc * Wc * Kc
            src = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
            dst = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
            t_copy = measure("%s copy of its bytes" % who, lambda: dst.copy_(src))
            del src, dst
            t = measure("%s reduce volume" % who, lambda: L.stereo_pyramid_reduce_volume_device(*args))
            say("%s reduce volume / copy %.2f   (%.1f MB, %.0f GB/s of the bytes it must move; %.1f ps per output element)"
                % (who, t / t_copy, nbytes / 1e6, nbytes / t / 1e3, 1e6 * t / (Hc * Wc * Kc)))
        del d_vol, d_out
        torch.cuda.empty_cache()
    say(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
