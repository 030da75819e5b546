"""NumPy restatement of stereo_pyramid_reduce_volume's definition (include/stereo_hip.h): what the
kernels must give, bit for bit.  The sampler is the oracle's restatement of the reference (oracle.terms); the four
clamped reads and their order are the image reduction's (tests/pyramid_restate.py).  Test infrastructure."""
import numpy as np

from oracle import terms as OT


def reduce_volume(ncc, disparities, sample_at):
    """ncc H x W x D with slices at `disparities` -> (H + 1) // 2 x (W + 1) // 2 x len(sample_at)."""
    ncc = np.asarray(ncc, np.float64)
    H, W, _ = ncc.shape
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    out = np.zeros((Hc, Wc, len(sample_at)))
    y0, x0 = 2 * np.arange(Hc), 2 * np.arange(Wc)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    done = {}                                   # (a long sample_at may repeat its values: each is worked out once)
    for j, d in enumerate(np.asarray(sample_at, np.float64)):
        if d.tobytes() not in done:
            with np.errstate(divide="ignore", invalid="ignore"):
                v = OT.sample_ncc_from_disp(ncc, disparities, np.full(H * W, d))
            v00, v10, v01, v11 = v[np.ix_(y0, x0)], v[np.ix_(y1, x0)], v[np.ix_(y0, x1)], v[np.ix_(y1, x1)]
            done[d.tobytes()] = np.float64(0.25) * (((v00 + v10) + v01) + v11)
        out[:, :, j] = done[d.tobytes()]
    return out


def level_sample_at(finer, coarser):
    finer = np.asarray(finer, np.float64)
    return np.clip(np.float64(2.0) * np.asarray(coarser, np.float64), finer.min(), finer.max())


def to_layout(hwd, layout):
    """An H x W x D array as the host forms take it: itself for layout 0, D x N (pixels column major) for layout 1."""
    H, W, D = hwd.shape
    return hwd if layout == 0 else np.asfortranarray(hwd.transpose(2, 0, 1).reshape((D, H * W), order="F"))


def from_layout(a, H, W, layout):
    """The inverse of to_layout -> H x W x D."""
    return np.asarray(a) if layout == 0 else np.asarray(a).reshape((a.shape[0], H, W), order="F").transpose(1, 2, 0)
