"""Development tool: what saving and loading a solver state costs.
usage: time_trws_state.py [runs=3]

The Teddy NCC volume (tests/golden/teddy_pair.npz, 450 x 375 x 60, tol 8, shared positions) as a single plan and as
G = 2 and 4 logical strips, each after three iterations.  Per configuration, `runs` times each, between device
synchronisations:
  save_device / load_device   into / from torch tensors, as GB/s of state bytes moved (8 K E of messages + 4 N of labels,
                              read once and written once), next to a plain device-to-device hipMemcpy of the same byte
                              count timed in the same process.  load_device includes the reset it implies;
  save / load                 the host variants, in seconds.
Prints the median and min .. max of each figure and the ratio of the device figures to the plain copy; the last line is
one JSON object with every run.  The output behind DESIGN.md's figures is kept as profiles/trws_state_timing.txt
(redirect stdout there)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
NEVER = -1e300


def main():
    import numpy as np, torch
    from helpers import grid_conn
    from stereo_amd import terms as T
    from stereo_amd.strips import make_strips
    from stereo_amd.trws import TrwsPlan
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 3

    def timed(fn):
        torch.cuda.synchronize(); t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    g = np.load(os.path.join(ROOT, "tests", "golden", "teddy_pair.npz"))
    im0, im1 = g["im0"].astype(np.float64), g["im1"].astype(np.float64)
    H, W = im0.shape[:2]
    K = 60
    unary = np.ascontiguousarray(40.0 * (1.0 - T.ncc_volume(im0, im1, np.arange(K, dtype=np.float64), 2, layout=1).T))
    conn = grid_conn(H, W)
    N, E = H * W, conn.shape[0]
    nbytes = 8 * K * E + 4 * N
    d_m = torch.zeros((E, K), dtype=torch.float64, device="cuda")
    d_x = torch.zeros(N, dtype=torch.int32, device="cuda")
    src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    res = {}

    def note(key, value):
        res.setdefault(key, []).append(value)

    for G in (1, 2, 4):
        s = TrwsPlan(1, K, N, conn.T) if G == 1 else make_strips(1, K, H, W, conn.T, G)
        s.upload(unary.T, np.ones(E), 8.0, positions=np.arange(K, dtype=np.float64))
        s.iterate(3, NEVER)
        who = "single plan" if G == 1 else "G=%d strips" % G
        st = s.save_state_device(d_m.data_ptr(), d_x.data_ptr())   # (warm-up: code objects, the strips' masks and tables)
        s.load_state_device(st, d_m.data_ptr(), d_x.data_ptr())
        dst.copy_(src)
        for _ in range(runs):
            note("%s save_device GB/s" % who, 2e-9 * nbytes / timed(lambda: s.save_state_device(d_m.data_ptr(), d_x.data_ptr())))
            note("%s load_device GB/s" % who, 2e-9 * nbytes / timed(lambda: s.load_state_device(st, d_m.data_ptr(), d_x.data_ptr())))
            note("%s plain copy GB/s" % who, 2e-9 * nbytes / timed(lambda: dst.copy_(src)))
            host = []
            note("%s save s" % who, timed(lambda: host.append(s.save_state())))
            note("%s load s" % who, timed(lambda: s.load_state(host[0])))
        s.close()
    print("state: %d bytes (E = %d, K = %d, N = %d); GB/s counts them read once and written once" % (nbytes, E, K, N))
    for k in res:
        v = res[k]
        print("%-34s median %10.4f  (%10.4f .. %10.4f)" % (k, np.median(v), min(v), max(v)), flush=True)
    for G in (1, 2, 4):
        who = "single plan" if G == 1 else "G=%d strips" % G
        plain = np.median(res["%s plain copy GB/s" % who])
        print("%-12s save_device / plain copy %.2f   load_device / plain copy %.2f" %
              (who, np.median(res["%s save_device GB/s" % who]) / plain, np.median(res["%s load_device GB/s" % who]) / plain))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
