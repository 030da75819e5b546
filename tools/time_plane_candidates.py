"""Development tool: what the plane-candidate builder costs on device-resident inputs, next to a device-to-device copy of
its bytes and to the plane band builder at equal K and E.
usage: time_plane_candidates.py [output file] [runs=15] [launches per run=20]

Sizes 375 x 450 with D = 60 slices and 2000 x 3000 with D = 64, K = 9 (3 offsets + the own planes at 6 taps) and K = 17
(5 offsets + two plane maps at 6 taps), for both unary sources: the NCC sampler on a random label-fastest volume and the
photo-consistency term on two random 3-channel images with the projection of example_global.m.  The planes are slanted
(|a|, |b| <= 0.002, c = 1) through whole-pixel disparities inside the range; the image grid's 4-neighbourhood in both
directions (E about 4 N).  Per case, between HIP events on one stream after a warm-up:
  gather      stereo_plane_candidates_gather_device: writes the 32 K N bytes of the table
  inputs      stereo_plane_candidates_inputs_*_device (both kernels; with E = 0 the unary kernel alone): writes
              8 K (N + 2 E) bytes; reads the 32 K N bytes of the table (the positions kernel loads two planes per element:
              64 K E bytes requested, 32 K N distinct), the source's samples and 8 E of conn
  plane band  stereo_plane_band_inputs_*_device at the same K and E (quarter-pixel offsets around 0): the same stores and
              the same sampler chain, its K lanes sharing the 32 N bytes of the planes from cache
  copy        a device-to-device copy that moves the bytes the plane-candidate builder must move (written + 32 K N + conn;
              half of them read, half written)
One run is `launches` launches back to back; the figure is the time per launch: median and min .. max of `runs` runs in
microseconds.  The last line is one JSON object with every run.  The output behind DESIGN.md's figures is kept as
profiles/plane_candidates_timing.txt.  STEREO_HIP_LIB selects another build of the library (the positions kernel's elements
per thread are a compile-time flag, PLANE_CAND_POS_PER_THREAD)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAPS = [(0, -1), (0, 1), (-1, 0), (1, 0), (0, -4), (0, 4)]


def main():
    import ctypes as C
    import numpy as np, torch
    import stereo_amd
    from stereo_amd import _lib, band, candidates, terms as T
    if stereo_amd.device_count() < 1:
        raise SystemExit("time_plane_candidates.py: no HIP device (timings are taken on the GPU only)")
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 15
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
        say("%-74s median %10.2f us  (%10.2f .. %10.2f)" % (key, v[len(v) // 2], v[0], v[-1]))
        return v[len(v) // 2], v[-1] - v[0]

    L, err = _lib.lib(), _lib.errbuf()
    vp = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))
    tail = (C.c_void_p(stream.cuda_stream), err, C.c_size_t(len(err)))
    say("%d runs of %d launches; library %s" % (runs, launches, os.path.basename(_lib.LIB_PATH)))

    def slanted(gen, H, W, D, count):
        """count plane maps as one (count, N, 4) tensor: [a b 1 d] with d = -(base + a x + b y), base whole in 8 .. D - 8"""
        N = H * W
        a = (torch.rand((count, N), dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 0.004
        b = (torch.rand((count, N), dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 0.004
        base = torch.randint(8, D - 8, (count, N), device="cuda", generator=gen).to(torch.float64)
        i = torch.arange(N, device="cuda")
        x, y = (i // H + 1).to(torch.float64), (i % H + 1).to(torch.float64)
        return torch.stack([a, b, torch.ones_like(a), -(base + a * x + b * y)], dim=2).contiguous()

    for H, W, D, Ko, M in ((375, 450, 60, 3, 1), (375, 450, 60, 5, 2), (2000, 3000, 64, 3, 1), (2000, 3000, 64, 5, 2)):
        N = H * W
        taps = np.array(TAPS, dtype=np.int32)
        Tn = taps.shape[0]
        K = Ko + M * Tn
        gen = torch.Generator(device="cuda").manual_seed(H + K)
        d_planes = slanted(gen, H, W, D, 1)[0].contiguous()
        d_src = slanted(gen, H, W, D, M)
        conn = T.construct_neighborhood(H, W)
        E = conn.shape[1]
        d_conn = torch.from_numpy(np.asfortranarray(conn, dtype=np.uint32).reshape(-1, order="F").view(np.int32).copy()).cuda()
        disparities = np.arange(D, dtype=np.float64)
        offsets = (np.arange(Ko, dtype=np.float64) - Ko // 2) / 2.0
        band_offsets = (np.arange(K, dtype=np.float64) - K // 2) / 4.0
        d_disp, d_off, d_boff = (band.to_device_vector(v) for v in (disparities, offsets, band_offsets))
        d_taps = candidates.taps_to_device(taps)
        d_pcand = torch.empty(4 * K * N, dtype=torch.float64, device="cuda")
        d_unary = torch.empty(K * N, dtype=torch.float64, device="cuda")
        d_q, d_qprim = (torch.empty(K * E, dtype=torch.float64, device="cuda") for _ in range(2))
        d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        written, table = 8 * K * (N + 2 * E), 32 * K * N
        who = "%d x %d D %d K %d (%d + %d x %d)" % (H, W, D, K, Ko, M, Tn)
        say("%s: N %d E %d, inputs writes %.1f MB and reads the %.1f MB table" % (who, N, E, written / 1e6, table / 1e6))
        half = (written + table + 8 * E) // 2
        src = torch.zeros(half, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(half, dtype=torch.uint8, device="cuda")
        t_copy, _ = measure("%s copy" % who, lambda: dst.copy_(src))
        del src, dst
        g_args = (vp(d_planes), C.c_int(H), C.c_int(W), hp(offsets), vp(d_off), C.c_int(Ko), vp(d_src), C.c_int(M),
                  hp(taps, C.c_int32), vp(d_taps), C.c_int(Tn), vp(d_pcand), vp(d_bad)) + tail
        assert L.stereo_plane_candidates_gather_device(*g_args) == 0, err.value
        t_g, _ = measure("%s gather" % who, lambda: L.stereo_plane_candidates_gather_device(*g_args))
        assert int(d_bad.item()) == 0
        table_tail = (vp(d_pcand), C.c_int(K), C.c_int64(E), vp(d_conn), vp(d_unary), vp(d_q), vp(d_qprim), vp(d_bad)) + tail
        band_tail = (vp(d_planes), hp(band_offsets), vp(d_boff), C.c_int(K), C.c_int64(E), vp(d_conn), vp(d_unary), vp(d_q),
                     vp(d_qprim), vp(d_bad)) + tail
        for kind in ("ncc", "globalstereo"):
            if kind == "ncc":
                d_data = [torch.rand(N * D, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1]
                head = (vp(d_data[0]), C.c_int(H), C.c_int(W), C.c_int(D), C.c_int(1), hp(disparities), vp(d_disp), C.c_double(40.0))
                fn, band_fn = L.stereo_plane_candidates_inputs_ncc_device, L.stereo_plane_band_inputs_ncc_device
            else:
                d_data = [torch.randint(0, 256, (3 * N,), device="cuda", generator=gen).to(torch.float64) for _ in range(2)]
                P2 = np.zeros((4, 3))
                P2[0, 0] = P2[1, 1] = P2[2, 2] = 1.0
                P2[3, 0] = -0.25
                P2 = np.ascontiguousarray(P2.reshape(-1, order="F"))
                head = (vp(d_data[0]), vp(d_data[1]), C.c_int(H), C.c_int(W), C.c_int(3), hp(P2), C.c_double(0.0), C.c_double(float(D)),
                        C.c_double(30.0))
                fn, band_fn = L.stereo_plane_candidates_inputs_globalstereo_device, L.stereo_plane_band_inputs_globalstereo_device
            me = "%s %s" % (who, kind)
            in_args = head + table_tail
            assert fn(*in_args) == 0, err.value
            t_in, _ = measure("%s inputs" % me, lambda: fn(*in_args))
            assert int(d_bad.item()) == 0
            un_args = head + table_tail[:2] + (C.c_int64(0), None) + table_tail[4:]
            t_un, _ = measure("%s inputs, E = 0 (the unary kernel alone)" % me, lambda: fn(*un_args))
            b_args = head + band_tail
            assert band_fn(*b_args) == 0, err.value
            t_b, spread_b = measure("%s plane band inputs" % me, lambda: band_fn(*b_args))
            assert int(d_bad.item()) == 0
            bu_args = head + band_tail[:4] + (C.c_int64(0), None) + band_tail[6:]
            t_bu, _ = measure("%s plane band inputs, E = 0 (the unary kernel alone)" % me, lambda: band_fn(*bu_args))
            say("%s unary kernel %.2f us (plane band's %.2f: ratio %.2f), positions kernel (the difference) %.2f us (plane band's "
                "%.2f: ratio %.2f; the plane band's inputs figure spreads over %.2f us)"
                % (me, t_un, t_bu, t_un / t_bu, t_in - t_un, t_b - t_bu, (t_in - t_un) / (t_b - t_bu), spread_b))
            say("%s gather + inputs %.2f us: / copy %.2f, / plane band inputs %.2f;  inputs alone: / copy %.2f, / plane band inputs %.2f"
                % (me, t_g + t_in, (t_g + t_in) / t_copy, (t_g + t_in) / t_b, t_in / t_copy, t_in / t_b))
            del d_data
            torch.cuda.empty_cache()
        del d_unary, d_q, d_qprim, d_pcand
        torch.cuda.empty_cache()
    say(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
