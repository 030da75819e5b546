"""Development tool: what the band builder costs on device-resident inputs, and what a band level costs per TRW-S
iteration.
usage: time_band.py [output file] [runs=25] [launches per run=20]

Builder.  Sizes 375 x 450 with D = 60 slices (K = 9 and 17 offsets, both volume layouts) and 2000 x 3000 with D = 64
(K = 9, the label-fastest volume), a random volume, a whole-pixel base inside the range, quarter-pixel offsets
around 0, the image grid's 4-neighbourhood in both directions (E about 4 N).  Per case, between HIP events on one
stream after a warm-up:
  inputs      stereo_band_inputs_device (both kernels; with E = 0 the unary kernel alone): writes 8 K (N + 2 E) bytes;
              must read 8 N (span + 3) bytes of the volume (span = slices between the smallest and the largest
              offset), 8 N of base and 8 E of conn
  copy        a device-to-device copy that moves the same number of bytes (half of them read, half written)
  apply       stereo_band_apply_device: 20 bytes per pixel
One run is `launches` launches back to back; the figure is the time per launch: median and min .. max of `runs` runs
in microseconds and the ratio to the copy.

Level.  The Teddy pair (tests/golden/teddy_pair.npz), D = 60, the whole-pixel winner-takes-all map as base: milliseconds
per iteration of a K = 9 and a K = 17 band level from plan.stats() (20 iterations after 5), next to the 60-label
problem on the same volume.  The last line is one JSON object with every run.  The output behind DESIGN.md's figures is
kept as profiles/band_timing.txt."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import ctypes as C
    import numpy as np, torch
    import stereo_amd
    from stereo_amd import _lib, band, terms as T
    from stereo_amd.trws import TrwsPlan
    if stereo_amd.device_count() < 1:
        raise SystemExit("time_band.py: no HIP device (timings are taken on the GPU only)")
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
    vp = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    tail = (C.c_void_p(stream.cuda_stream), err, C.c_size_t(len(err)))
    say("%d runs of %d launches" % (runs, launches))
    for H, W, D, K, layout in ((375, 450, 60, 9, 1), (375, 450, 60, 17, 1), (375, 450, 60, 9, 0), (375, 450, 60, 17, 0),
                               (2000, 3000, 64, 9, 1)):
        N = H * W
        gen = torch.Generator(device="cuda").manual_seed(H + K)
        d_ncc = torch.rand(N * D, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        d_base = torch.randint(4, D - 4, (W, H), device="cuda", generator=gen).to(torch.float64)
        conn = T.construct_neighborhood(H, W)
        E = conn.shape[1]
        d_conn = torch.from_numpy(np.asfortranarray(conn, dtype=np.uint32).reshape(-1, order="F").view(np.int32).copy()).cuda()
        disparities = np.arange(D, dtype=np.float64)
        offsets = (np.arange(K, dtype=np.float64) - K // 2) / 4.0
        d_disp, d_off = band.to_device_vector(disparities), band.to_device_vector(offsets)
        d_unary = torch.empty(K * N, dtype=torch.float64, device="cuda")
        d_q, d_qprim = (torch.empty(K * E, dtype=torch.float64, device="cuda") for _ in range(2))
        d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_labels = torch.randint(1, K + 1, (N,), device="cuda", generator=gen).to(torch.int32)
        d_refined = torch.empty((W, H), dtype=torch.float64, device="cuda")
        span = int(round(offsets[-1] - offsets[0]))
        written, read = 8 * K * (N + 2 * E), 8 * N * (span + 3) + 8 * N + 8 * E
        who = "%d x %d D %d K %d layout %d" % (H, W, D, K, layout)
        say("%s: N %d E %d, writes %.1f MB, must read %.1f MB" % (who, N, E, written / 1e6, read / 1e6))
        half = (written + read) // 2
        src = torch.zeros(half, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(half, dtype=torch.uint8, device="cuda")
        t_copy = measure("%s copy" % who, lambda: dst.copy_(src))
        del src, dst
        in_args = (vp(d_ncc), C.c_int(H), C.c_int(W), C.c_int(D), C.c_int(layout), hp(disparities), vp(d_disp), C.c_double(40.0),
                   vp(d_base), hp(offsets), vp(d_off), C.c_int(K), C.c_int64(E), vp(d_conn), vp(d_unary), vp(d_q), vp(d_qprim),
                   vp(d_bad)) + tail
        assert L.stereo_band_inputs_device(*in_args) == 0, err.value
        t_in = measure("%s inputs" % who, lambda: L.stereo_band_inputs_device(*in_args))
        assert int(d_bad.item()) == 0
        un_args = in_args[:12] + (C.c_int64(0), None) + in_args[14:]
        t_un = measure("%s inputs, E = 0 (the unary kernel alone)" % who, lambda: L.stereo_band_inputs_device(*un_args))
        say("%s unary kernel %.2f us for %.1f MB written, positions kernel (the difference) %.2f us for %.1f MB written"
            % (who, t_un, 8 * K * N / 1e6, t_in - t_un, 16 * K * E / 1e6))
        say("%s inputs / copy %.2f   (%.0f GB/s of the bytes it must move)" % (who, t_in / t_copy, (written + read) / t_in / 1e3))
        if layout == 1:
            half = 10 * N
            src = torch.zeros(half, dtype=torch.uint8, device="cuda")
            dst = torch.zeros(half, dtype=torch.uint8, device="cuda")
            t_copy20 = measure("%s copy 20 B/px" % who, lambda: dst.copy_(src))
            del src, dst
            ap_args = (vp(d_base), C.c_int(H), C.c_int(W), vp(d_labels), hp(offsets), vp(d_off), C.c_int(K), vp(d_refined), vp(d_bad)) + tail
            t_ap = measure("%s apply" % who, lambda: L.stereo_band_apply_device(*ap_args))
            say("%s apply / copy %.2f" % (who, t_ap / t_copy20))
        del d_ncc, d_unary, d_q, d_qprim
        torch.cuda.empty_cache()

    # ---- a band level on Teddy, per iteration
    g = np.load(os.path.join(ROOT, "tests", "golden", "teddy_pair.npz"))
    im0, im1 = g["im0"].astype(np.float64), g["im1"].astype(np.float64)
    H, W = im0.shape[:2]
    D = 60
    disparities = np.arange(D, dtype=np.float64)
    vol = T.ncc_volume(im0, im1, disparities, 2, layout=1)
    conn = T.construct_neighborhood(H, W)
    E, N = conn.shape[1], H * W
    NEVER = -1e300

    def per_iteration(plan):
        plan.stats(reset=True)
        plan.iterate(5, NEVER)
        plan.stats(reset=True)
        plan.iterate(20, NEVER)
        ms, _ = plan.stats()
        return ms / 20.0

    plan = TrwsPlan(1, D, N, conn)
    plan.upload(40.0 * (1.0 - vol), np.ones(E), 8.0, positions=disparities)
    res["teddy K 60 ms/iteration"] = per_iteration(plan)
    say("Teddy %d x %d, 60 labels (shared positions, path %d): %.3f ms per iteration" % (H, W, plan.path(), res["teddy K 60 ms/iteration"]))
    plan.close()
    base = disparities[np.argmax(vol, axis=0)].reshape(W, H).T
    for K in (9, 17):
        offsets = (np.arange(K, dtype=np.float64) - K // 2) / 4.0
        prob = band.BandProblem(vol, disparities, 40.0, base, conn, layout=1)
        plan = TrwsPlan(1, K, N, conn)
        prob.build(offsets, plan, 8.0)
        key = "teddy band K %d ms/iteration" % K
        res[key] = per_iteration(plan)
        say("Teddy band level, K %d offsets %g .. %g by 1/4 (positions per edge, path %d): %.3f ms per iteration"
            % (K, offsets[0], offsets[-1], plan.path(), res[key]))
        plan.close()
    say("README's recorded figures for the enlarged label set on this pair: 7.9 ms per iteration at K = 60, 2711 ms at K = 1024 (1/16 pixel)")
    say(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
