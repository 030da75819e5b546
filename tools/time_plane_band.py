"""Development tool: what the plane-band builder costs on device-resident inputs, next to its two yardsticks, and what a
plane-band level costs per TRW-S iteration.
usage: time_plane_band.py [output file] [runs=25] [launches per run=20]

Builder.  The method and the shapes of tools/time_band.py: 375 x 450 with D = 60 slices (K = 9 and 17 offsets) and
2000 x 3000 with D = 64 (K = 9), the label-fastest volume, the image grid's 4-neighbourhood in both directions (E about
4 N), quarter-pixel offsets around 0.  The planes are slightly slanted ([a b 1 d], |a|, |b| <= 1/64) through a whole-pixel
disparity inside the range; the globalstereo source has C = 3 random images, the projection of example_global.m and
d_min = 0, d_step = 4 (D - 1) (the planes' disparities are then four times the NCC case's, so the projected column
moves by the same number of pixels).  Per case, between HIP events on one stream after a warm-up:
  ncc inputs   stereo_plane_band_inputs_ncc_device (both kernels; with E = 0 the unary kernel alone): writes
               8 K (N + 2 E) bytes; must read 8 N (span + 3) bytes of the volume, 32 N of planes in each of its two
               kernels and 8 E of conn
  gs inputs    stereo_plane_band_inputs_globalstereo_device: the same writes; must read 16 N C of the two images, 32 N of
               planes in each kernel and 8 E of conn
  copy         a device-to-device copy that moves the same number of bytes as the ncc builder (half read, half written)
  band inputs  stereo_band_inputs_device, the fronto-parallel builder of DESIGN.md 6.2, on the map of the same planes'
               disparities: the other yardstick (the parent's code, not under test here)
  apply        stereo_plane_band_apply_device: 68 bytes per pixel, next to a copy of as many
One run is `launches` launches back to back; the figure is the time per launch: median and min .. max of `runs` runs
in microseconds.

Level.  The Teddy pair (tests/golden/teddy_pair.npz), D = 60, the planes [0 0 1 -wta] of the whole-pixel winner-takes-all
map: milliseconds per iteration of a K = 9 and a K = 17 plane-band level from plan.stats() (20 iterations after 5).  The
last line is one JSON object with every run.  The output behind DESIGN.md's figures is kept as
profiles/plane_band_timing.txt."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import ctypes as C
    import numpy as np, torch
    import stereo_amd
    from stereo_amd import _lib, band, plane_band, terms as T
    from stereo_amd.trws import TrwsPlan
    if stereo_amd.device_count() < 1:
        raise SystemExit("time_plane_band.py: no HIP device (timings are taken on the GPU only)")
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
        say("%-70s median %10.2f us  (%10.2f .. %10.2f)" % (key, v[len(v) // 2], v[0], v[-1]))
        return v[len(v) // 2]

    def copy_of(key, nbytes):
        src = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
        return measure(key, lambda: dst.copy_(src))

    L, err = _lib.lib(), _lib.errbuf()
    vp = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    tail = (C.c_void_p(stream.cuda_stream), err, C.c_size_t(len(err)))
    say("%d runs of %d launches" % (runs, launches))
    P2 = np.zeros((4, 3)); P2[0, 0] = P2[1, 1] = P2[2, 2] = 1.0; P2[3, 0] = -0.25
    P2 = np.ascontiguousarray(P2.reshape(-1, order="F"))
    for H, W, D, K in ((375, 450, 60, 9), (375, 450, 60, 17), (2000, 3000, 64, 9)):
        N, Cn, layout = H * W, 3, 1
        gen = torch.Generator(device="cuda").manual_seed(H + K)
        d_ncc = torch.rand(N * D, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        d_im0 = torch.rand(N * Cn, dtype=torch.float64, device="cuda", generator=gen) * 255
        d_im1 = torch.rand(N * Cn, dtype=torch.float64, device="cuda", generator=gen) * 255
        d_base = torch.randint(4, D - 4, (W, H), device="cuda", generator=gen).to(torch.float64)
        xs = torch.arange(1, W + 1, device="cuda", dtype=torch.float64)[:, None].expand(W, H)
        ys = torch.arange(1, H + 1, device="cuda", dtype=torch.float64)[None, :].expand(W, H)
        a = torch.randint(-4, 5, (W, H), device="cuda", generator=gen).to(torch.float64) / 256.0
        b = torch.randint(-4, 5, (W, H), device="cuda", generator=gen).to(torch.float64) / 256.0

        def planes_for(scale):          # [a b 1 d] whose disparity at the own point is scale * base
            return torch.stack([a * scale, b * scale, torch.ones_like(a), -(scale * d_base + scale * (a * xs + b * ys))], dim=2).reshape(N, 4).contiguous()

        d_planes, d_planes_gs = planes_for(1.0), planes_for(4.0)
        conn = T.construct_neighborhood(H, W)
        E = conn.shape[1]
        d_conn = torch.from_numpy(np.asfortranarray(conn, dtype=np.uint32).reshape(-1, order="F").view(np.int32).copy()).cuda()
        disparities = np.arange(D, dtype=np.float64)
        offsets = (np.arange(K, dtype=np.float64) - K // 2) / 4.0
        offsets_gs = offsets * 4.0
        d_disp, d_off, d_off_gs = (band.to_device_vector(v) for v in (disparities, offsets, offsets_gs))
        d_unary = torch.empty(K * N, dtype=torch.float64, device="cuda")
        d_q, d_qprim = (torch.empty(K * E, dtype=torch.float64, device="cuda") for _ in range(2))
        d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_labels = torch.randint(1, K + 1, (N,), device="cuda", generator=gen).to(torch.int32)
        d_refined = torch.empty((N, 4), dtype=torch.float64, device="cuda")
        span = int(round(offsets[-1] - offsets[0]))
        written = 8 * K * (N + 2 * E)
        read_ncc = 8 * N * (span + 3) + 2 * 32 * N + 8 * E
        read_gs = 16 * N * Cn + 2 * 32 * N + 8 * E
        read_band = 8 * N * (span + 3) + 8 * N + 8 * E
        who = "%d x %d D %d K %d" % (H, W, D, K)
        say("%s: N %d E %d, writes %.1f MB; must read %.1f MB (ncc), %.1f MB (globalstereo, C = 3), %.1f MB (the fronto-parallel band)"
            % (who, N, E, written / 1e6, read_ncc / 1e6, read_gs / 1e6, read_band / 1e6))
        t_copy = copy_of("%s copy of the ncc builder's bytes" % who, written + read_ncc)
        t_copy_un = copy_of("%s copy of the ncc unary kernel's bytes" % who, 8 * K * N + 8 * N * (span + 3) + 32 * N)
        outs = (vp(d_unary), vp(d_q), vp(d_qprim), vp(d_bad)) + tail
        ncc_head = (vp(d_ncc), C.c_int(H), C.c_int(W), C.c_int(D), C.c_int(layout), hp(disparities), vp(d_disp), C.c_double(40.0),
                    vp(d_planes), hp(offsets), vp(d_off), C.c_int(K))
        gs_head = (vp(d_im0), vp(d_im1), C.c_int(H), C.c_int(W), C.c_int(Cn), hp(P2), C.c_double(0.0), C.c_double(4.0 * (D - 1)),
                   C.c_double(30.0), vp(d_planes_gs), hp(offsets_gs), vp(d_off_gs), C.c_int(K))
        band_head = (vp(d_ncc), C.c_int(H), C.c_int(W), C.c_int(D), C.c_int(layout), hp(disparities), vp(d_disp), C.c_double(40.0),
                     vp(d_base), hp(offsets), vp(d_off), C.c_int(K))
        full, unary_only = (C.c_int64(E), vp(d_conn)), (C.c_int64(0), None)
        t = {}
        for name, fn, head in (("ncc", L.stereo_plane_band_inputs_ncc_device, ncc_head),
                               ("globalstereo", L.stereo_plane_band_inputs_globalstereo_device, gs_head),
                               ("fronto-parallel band", L.stereo_band_inputs_device, band_head)):
            assert fn(*(head + full + outs)) == 0, err.value
            assert int(d_bad.item()) == 0
            t[name] = measure("%s %s inputs" % (who, name), lambda: fn(*(head + full + outs)))
            t[name + " unary"] = measure("%s %s inputs, E = 0 (the unary kernel alone)" % (who, name), lambda: fn(*(head + unary_only + outs)))
        for name, read in (("ncc", read_ncc), ("globalstereo", read_gs), ("fronto-parallel band", read_band)):
            say("%s %s: unary kernel %.2f us for %.1f MB written, positions kernel (the difference) %.2f us for %.1f MB written (%.0f GB/s stored); "
                "inputs / copy %.2f, %.0f GB/s of the bytes it must move" % (
                    who, name, t[name + " unary"], 8 * K * N / 1e6, t[name] - t[name + " unary"], 16 * K * E / 1e6,
                    16 * K * E / (t[name] - t[name + " unary"]) / 1e3, t[name] / t_copy, (written + read) / t[name] / 1e3))
        say("%s ncc unary kernel / copy of its bytes %.2f; plane-band positions / fronto-parallel positions %.2f" % (
            who, t["ncc unary"] / t_copy_un, (t["ncc"] - t["ncc unary"]) / (t["fronto-parallel band"] - t["fronto-parallel band unary"])))
        t_copy68 = copy_of("%s copy 68 B/px" % who, 68 * N)
        ap_args = (vp(d_planes), C.c_int64(N), vp(d_labels), hp(offsets), vp(d_off), C.c_int(K), vp(d_refined), vp(d_bad)) + tail
        assert L.stereo_plane_band_apply_device(*ap_args) == 0, err.value
        t_ap = measure("%s apply" % who, lambda: L.stereo_plane_band_apply_device(*ap_args))
        say("%s apply / copy %.2f" % (who, t_ap / t_copy68))
        del d_ncc, d_im0, d_im1, d_unary, d_q, d_qprim, d_planes, d_planes_gs
        torch.cuda.empty_cache()

    # ---- a plane-band level on Teddy, per iteration
    g = np.load(os.path.join(ROOT, "tests", "golden", "teddy_pair.npz"))
    im0, im1 = g["im0"].astype(np.float64), g["im1"].astype(np.float64)
    H, W = im0.shape[:2]
    D = 60
    disparities = np.arange(D, dtype=np.float64)
    vol = T.ncc_volume(im0, im1, disparities, 2, layout=1)
    conn = T.construct_neighborhood(H, W)
    N = H * W
    NEVER = -1e300

    def per_iteration(plan):
        plan.stats(reset=True)
        plan.iterate(5, NEVER)
        plan.stats(reset=True)
        plan.iterate(20, NEVER)
        ms, _ = plan.stats()
        return ms / 20.0

    planes = np.zeros((4, N), order="F")
    planes[2], planes[3] = 1.0, -disparities[np.argmax(vol, axis=0)]
    source = plane_band.NccSource(vol, disparities, 40.0, layout=1, shape=(H, W))
    for K in (9, 17):
        offsets = (np.arange(K, dtype=np.float64) - K // 2) / 4.0
        prob = plane_band.PlaneBandProblem(source, planes, conn)
        plan = TrwsPlan(1, K, N, conn)
        prob.build(offsets, plan, 8.0)
        key = "teddy plane band K %d ms/iteration" % K
        res[key] = per_iteration(plan)
        say("Teddy plane-band level, K %d offsets %g .. %g by 1/4 (positions per edge, path %d): %.3f ms per iteration"
            % (K, offsets[0], offsets[-1], plan.path(), res[key]))
        plan.close()
    say("profiles/band_timing.txt, the fronto-parallel band level on this pair: 9.359 ms per iteration at K = 9, 12.082 ms at K = 17")
    say(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
