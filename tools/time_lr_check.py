"""Development tool: what the left-right check and the fill cost on device-resident maps.
usage: time_lr_check.py [output file] [runs=25] [launches per run=20]

Maps of 375 x 450 and 2000 x 3000 (H x W): a background plane with boxes in front of it, 4 % of the pixels of each map
replaced by noise, so that the check finds consistent, occluded, mismatched and out-of-view pixels in the proportions of
a real pair.  Per size, between HIP events on one stream, after a warm-up of every shape and chunk count:
  check            stereo_lr_check_device with the residual: 28 bytes per pixel (two maps read, status and residual written)
  fill C=..        stereo_lr_fill_device_chunks for every chunk count C that fits a workgroup; the bytes the fill MUST move are
                   24 per pixel (map and status read, filled and source written)
  copy 28 / 24     a device-to-device copy of the same number of bytes (half of them read, half written)
One run is `launches` launches back to back; the figure is the time per launch.  Prints the median and min .. max of
`runs` runs in microseconds, the ratio to the copy, and as the last line one JSON object with every run.  The output
behind DESIGN.md's figures is kept as profiles/lr_check_timing.txt."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(H, W, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    left = np.full((H, W), 8.0)
    right = np.full((H, W), 8.0)
    for x0 in range(W // 6, W - W // 6, W // 4):      # boxes with d = 24, each over its own band of rows
        y0 = int(rng.integers(0, H // 2))
        left[y0:y0 + H // 2, x0:x0 + W // 8] = 24.0
        right[y0:y0 + H // 2, x0 - 24:x0 + W // 8 - 24] = 24.0
    for m in (left, right):
        noise = rng.random((H, W)) < 0.04
        m[noise] = rng.integers(0, 128, size=int(noise.sum())) / 4.0
    return left, right


def main():
    import numpy as np, torch
    import stereo_amd
    import ctypes as C
    from stereo_amd import _lib, consistency as lr
    if stereo_amd.device_count() < 1:
        raise SystemExit("time_lr_check.py: no HIP device (timings are taken on the GPU only)")
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    launches = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    stream = torch.cuda.current_stream()
    res, lines = {}, []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def timed(fn):
        """microseconds per launch: `launches` launches between two events"""
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
        say("%-34s median %10.2f us  (%10.2f .. %10.2f)" % (key, v[len(v) // 2], v[0], v[-1]))
        return v[len(v) // 2]

    chunk_counts = (1, 2, 4, 8, 16)
    say("chunk count in the library: %d; %d runs of %d launches" % (lr.fill_chunks(), runs, launches))
    for H, W in ((375, 450), (2000, 3000)):
        left, right = scene(H, W, H)
        dev = lambda m: torch.from_numpy(np.ascontiguousarray(m.T)).cuda()
        d_left, d_right = dev(left), dev(right)
        d_status = torch.empty((W, H), dtype=torch.int32, device="cuda")
        d_res = torch.empty((W, H), dtype=torch.float64, device="cuda")
        d_filled = torch.empty((W, H), dtype=torch.float64, device="cuda")
        d_source = torch.empty((W, H), dtype=torch.int32, device="cuda")
        N = H * W
        who = "%d x %d" % (H, W)
        lr.lr_check_device(d_left, d_right, 1, 1.0, status=d_status, residual=d_res)
        torch.cuda.synchronize()
        share = np.bincount(d_status.cpu().numpy().reshape(-1), minlength=5) / float(N)
        say("%s: %d pixels, status shares %s" % (who, N, " ".join("%d: %.3f" % (i, s) for i, s in enumerate(share))))
        copies = {}
        for nbytes in (28, 24):
            src = torch.zeros(nbytes * N // 2, dtype=torch.uint8, device="cuda")
            dst = torch.zeros(nbytes * N // 2, dtype=torch.uint8, device="cuda")
            copies[nbytes] = measure("%s copy %d B/px" % (who, nbytes), lambda: dst.copy_(src))
        # the C entries directly, arguments built once: the interpreter must not be what the events see
        L, err = _lib.lib(), _lib.errbuf()
        vp = lambda t: C.c_void_p(t.data_ptr())
        tail = (C.c_void_p(stream.cuda_stream), err, C.c_size_t(len(err)))
        check_args = (vp(d_left), vp(d_right), C.c_int(H), C.c_int(W), C.c_int(1), C.c_double(1.0), vp(d_status), vp(d_res)) + tail
        t_check = measure("%s check" % who, lambda: L.stereo_lr_check_device(*check_args))
        t_fill = {}
        for c in chunk_counts:
            fill_args = (vp(d_left), vp(d_status), C.c_int(H), C.c_int(W), vp(d_filled), vp(d_source), C.c_int(c)) + tail
            t_fill[c] = measure("%s fill C=%d" % (who, c), lambda: L.stereo_lr_fill_device_chunks(*fill_args))
            want = lr.lr_fill_device(d_left, d_status, chunks=1)
            assert torch.equal(want[1], d_source) and torch.equal(want[0].nan_to_num(-1.0), d_filled.nan_to_num(-1.0))
        say("%s check / copy %.2f   " % (who, t_check / copies[28]) + "   ".join("fill C=%d / copy %.2f" % (c, t_fill[c] / copies[24]) for c in chunk_counts))
    say(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
