"""The reference's answers to one test's calls.  Where oracle/_ref was built they come from the reference's own libraries,
live; elsewhere they are replayed from tests/golden/ref_calls_<name>.npz, which tests/golden/make_golden_ref_calls.py
records from those libraries.  Every replayed call checks a digest of its inputs against the recorded one, so a test whose
inputs change fails until the file is recorded again.  STEREO_RECORD_REF_CALLS=1 (with oracle/_ref present) writes the file."""
import hashlib
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _digest(args, kw):
    h = hashlib.sha1()
    for a in list(args) + [kw[k] for k in sorted(kw)]:
        if isinstance(a, np.ndarray):
            h.update(str(a.dtype).encode() + str(a.shape).encode())
            h.update(np.ascontiguousarray(a).tobytes())
        else:
            h.update(repr(a).encode())
    return h.hexdigest()


class RefCalls:
    def __init__(self, oracle, name, live):
        self.oracle, self.live = oracle, live
        self.path = os.path.join(GOLD, "ref_calls_%s.npz" % name)
        self.record = live and bool(os.environ.get("STEREO_RECORD_REF_CALLS"))
        self.calls = []
        self.n = 0
        if not live:
            assert os.path.exists(self.path), "%s missing and oracle/_ref not built" % self.path
            self.rec = _load(self.path)

    def call(self, fn, *args, **kw):
        """fn(*args, **kw) of the reference (a tuple of arrays / numbers), or its recorded answer."""
        d = _digest(args, kw)
        if self.live:
            out = tuple(fn(*args, **kw))
            if self.record:
                self.calls.append((d, out))
            return out
        i = self.n
        self.n += 1
        digests, outs = self.rec
        assert i < len(digests), "more calls than recorded in %s" % self.path
        assert digests[i] == d[:16], "call %d: inputs differ from the recording %s" % (i, self.path)
        return tuple(o[i] for o in outs)

    def ref_rd(self, *args, **kw):
        return self.call(self.oracle.ref_rd, *args, **kw)

    def update_message(self, *args, **kw):
        return self.call(self.oracle.update_message, *args, **kw)

    def ref_segment_ms(self, *args, **kw):
        return self.call(lambda *a, **k: (self.oracle.ref_segment_ms(*a, **k),), *args, **kw)[0]

    def ref_segment_gb(self, *args, **kw):
        return self.call(lambda *a, **k: (self.oracle.ref_segment_gb(*a, **k),), *args, **kw)[0]

    def finish(self):
        if self.record:
            arrs = {"digests": np.array([d[:16] for d, _ in self.calls])}
            nout = {len(out) for _, out in self.calls}
            assert len(nout) == 1, "calls of one test must return the same number of values"
            for j in range(nout.pop()):
                vals = [np.asarray(out[j]) for _, out in self.calls]
                flat = np.concatenate([v.reshape(-1).astype(np.float64) for v in vals])
                for t in (np.int8, np.int32):      # (label vectors and maps: small integers)
                    if np.array_equal(flat, flat.astype(t)):
                        flat = flat.astype(t)
                        break
                shapes = np.zeros((len(vals), 4), np.int64)
                for k, v in enumerate(vals):
                    shapes[k, 0] = v.ndim
                    shapes[k, 1:1 + v.ndim] = v.shape
                arrs["data_%d" % j], arrs["shapes_%d" % j] = flat, shapes
            np.savez_compressed(self.path, **arrs)
        elif not self.live:
            assert self.n == len(self.rec[0]), "%d calls, %d recorded in %s" % (self.n, len(self.rec[0]), self.path)


def _load(path):
    """(input digests, per output position the list of the calls' values: arrays or numbers)."""
    z = np.load(path)
    digests = [str(d) for d in z["digests"]]
    outs = []
    j = 0
    while "data_%d" % j in z.files:
        flat, shapes = z["data_%d" % j], z["shapes_%d" % j]
        vals, at = [], 0
        for sh in shapes:
            shape = tuple(int(x) for x in sh[1:1 + sh[0]])
            n = int(np.prod(shape)) if shape else 1
            v = flat[at:at + n].reshape(shape)
            vals.append(v if shape else v[()])
            at += n
        outs.append(vals)
        j += 1
    return digests, outs
