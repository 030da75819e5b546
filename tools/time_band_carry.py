"""Development tool: what the transfer of carried messages costs on device-resident inputs.
usage: time_band_carry.py [output file] [runs=25] [launches per run=20]

Sizes 375 x 450 (K 9 -> 9) and 2000 x 3000 (K 9 -> 17), the image grid's 4-neighbourhood in both directions
(E about 4 N), random message rows, quarter-pixel offsets, shifts of up to one pixel, every edge inheriting from
itself (edge_src NULL) and, at the small size, through a permuted edge_src.  Per case, between HIP events on one stream
after a warm-up:
  carry       stereo_band_carry_device: reads 8 K_old E (old rows) + 4 E (receivers; + 4 E with edge_src) + 8 N
              (shifts), writes 8 K_new E
  copy        a device-to-device copy that moves the same number of bytes (half of them read, half written), in the
              same process
One run is `launches` launches back to back; the figure is the time per launch: median and min .. max of `runs` runs in
microseconds and the ratio to the copy.  The last line is one JSON object with every run.  The output behind DESIGN.md's
figures is kept as profiles/band_carry_timing.txt."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import ctypes as C
    import numpy as np, torch
    import stereo_amd
    from stereo_amd import _lib, band, carry, terms as T
    if stereo_amd.device_count() < 1:
        raise SystemExit("time_band_carry.py: no HIP device (timings are taken on the GPU only)")
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
        say("%-62s median %10.2f us  (%10.2f .. %10.2f)" % (key, v[len(v) // 2], v[0], v[-1]))
        return v[len(v) // 2]

    L, err = _lib.lib(), _lib.errbuf()
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    hp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    tail = (C.c_void_p(stream.cuda_stream), err, C.c_size_t(len(err)))
    say("%d runs of %d launches" % (runs, launches))
    for H, W, K_old, K_new, permuted in ((375, 450, 9, 9, False), (375, 450, 9, 9, True), (2000, 3000, 9, 17, False)):
        N = H * W
        conn = T.construct_neighborhood(H, W)
        E = conn.shape[1]
        gen = torch.Generator(device="cuda").manual_seed(H + K_new)
        d_old = torch.rand(E * K_old, dtype=torch.float64, device="cuda", generator=gen) * 40.0
        d_new = torch.empty(E * K_new, dtype=torch.float64, device="cuda")
        d_recv = torch.from_numpy(carry.receivers(N, conn, 1)).cuda()
        d_shift = torch.randint(-4, 5, (N,), device="cuda", generator=gen).to(torch.float64) / 4.0
        d_src = torch.randperm(E, device="cuda", generator=gen).to(torch.int32) if permuted else None
        off_old = (np.arange(K_old, dtype=np.float64) - K_old // 2) / 4.0
        off_new = (np.arange(K_new, dtype=np.float64) - K_new // 2) / 16.0
        d_off_old, d_off_new = band.to_device_vector(off_old), band.to_device_vector(off_new)
        d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        read = 8 * K_old * E + 4 * E * (2 if permuted else 1) + 8 * N
        written = 8 * K_new * E
        who = "%d x %d K %d -> %d%s" % (H, W, K_old, K_new, ", permuted edge_src" if permuted else "")
        say("%s: N %d E %d, reads %.1f MB, writes %.1f MB" % (who, N, E, read / 1e6, written / 1e6))
        half = (written + read) // 2
        src = torch.zeros(half, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(half, dtype=torch.uint8, device="cuda")
        t_copy = measure("%s copy" % who, lambda: dst.copy_(src))
        del src, dst
        args = (vp(d_old), C.c_int64(E), C.c_int(K_old), hp(off_old), vp(d_off_old), vp(d_src), vp(d_recv), C.c_int64(N),
                vp(d_shift), C.c_double(1.0), C.c_double(1.0), hp(off_new), vp(d_off_new), C.c_int(K_new), C.c_int64(E),
                vp(d_new), vp(d_bad)) + tail
        assert L.stereo_band_carry_device(*args) == 0, err.value
        t = measure("%s carry" % who, lambda: L.stereo_band_carry_device(*args))
        assert int(d_bad.item()) == 0
        say("%s carry / copy %.2f   (%.0f GB/s of the bytes it must move)" % (who, t / t_copy, (written + read) / t / 1e3))
        del d_old, d_new
        torch.cuda.empty_cache()
    say(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
