"""-m gpu: the tagged-granule row hand-over between ordinary runs (descriptor word 57; trws_pipe.hip).

A row's node takes the rows of the node above as granules {value half, epoch} that the producer's finishing compute
wave publishes as soon as the message is final, instead of behind the storer's completion flag one visit later.  The
granule carries the very 64 bits the flag path loads, so labels, energy, bound and iteration count must be the same
with granules on (the default), off (STEREO_HIP_TRWS_GRANULES=0) and on with development switch 262144 -- a hashed
quarter of the nodes publishes a few microseconds late, so consumers find last sweep's tags and must sweep again.
Heights above 256 rows make runs wait for a workgroup (more runs than resident workgroups)."""
import numpy as np
import pytest

from helpers import grid_conn

pytestmark = pytest.mark.gpu

ENV = ("STEREO_HIP_TRWS_GRANULES", "STEREO_HIP_TRWS_DEBUG", "STEREO_HIP_TRWS_SPEC")


def _solve(monkeypatch, env, kernel, unary, conn, alphas, tol, iters, positions=None, q=None, mode=None):
    from stereo_amd.trws import TrwsPlan, MESSAGES_MINPLUS
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    N, K = unary.shape
    plan = TrwsPlan(kernel, K, N, conn.T, *(() if mode is None else (mode,)))
    if q is None:
        plan.upload(unary.T, alphas, tol, positions=positions)
    else:
        plan.upload(unary.T, alphas, tol, q=q.T, qprim=q.T)
    out = []
    for _ in range(iters):
        plan.iterate(1, max_relgap=-1e300)
        lab, en, lb, it = plan.result()
        out.append((lab.copy(), en, lb, it))
    plan.close()
    return out


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and x[1:] == y[1:] for x, y in zip(a, b))


def _noise(seed, H, W, K, ncc_like=False):
    rng = np.random.default_rng(seed)
    conn = grid_conn(H, W)
    if ncc_like:   # a Teddy-like volume: a planted disparity ramp + noise, masked columns at the left border
        cols = np.repeat(np.arange(W), H)
        truth = (0.25 * K + 0.5 * K * cols / W)[:, None]
        unary = np.minimum(np.abs(np.arange(K)[None, :] - truth) / 4.0, 1.0) * 30.0 + rng.uniform(0, 10, (H * W, K))
        unary[cols < 6, :] = 40.0
    else:
        unary = rng.uniform(0, 40, size=(H * W, K))
    return unary, conn, np.ones(conn.shape[0])


CASES = [
    # id, seed, H, W, K, kernel, tol, positions ("shared" / "edges"), spec, mode, ncc-like, iterations
    ("teddy-crop", 1, 120, 150, 60, 1, 8.0, "shared", True, None, True, 4),
    ("noise-tall", 2, 300, 40, 16, 1, 4.0, "shared", True, None, False, 3),
    ("noise-tall-nospec", 3, 290, 33, 12, 1, 3.0, "shared", False, None, False, 3),
    ("kernel2", 4, 60, 70, 20, 2, 30.0, "shared", False, None, False, 3),
    ("per-edge", 5, 50, 64, 24, 1, 6.0, "edges", False, None, False, 3),
    ("per-edge-k2", 6, 45, 52, 18, 2, 25.0, "edges", False, None, False, 3),
    ("minplus", 7, 40, 48, 16, 1, 4.0, "shared", True, "minplus", False, 3),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_granules_change_nothing(case, hip, monkeypatch):
    from stereo_amd.trws import TrwsPlan, MESSAGES_MINPLUS
    _, seed, H, W, K, kernel, tol, where, spec, mode, ncc, iters = case
    unary, conn, alphas = _noise(seed, H, W, K, ncc)
    pos = np.arange(K, dtype=np.float64)
    kw = dict(positions=pos) if where == "shared" else dict(q=np.tile(np.random.default_rng(seed).permutation(K).astype(np.float64), (conn.shape[0], 1)))
    if mode == "minplus":
        kw["mode"] = MESSAGES_MINPLUS
    base = {} if spec else {"STEREO_HIP_TRWS_SPEC": "0"}
    off = _solve(monkeypatch, dict(base, STEREO_HIP_TRWS_GRANULES="0"), kernel, unary, conn, alphas, tol, iters, **kw)
    on = _solve(monkeypatch, base, kernel, unary, conn, alphas, tol, iters, **kw)
    assert _same(off, on)
    late = _solve(monkeypatch, dict(base, STEREO_HIP_TRWS_DEBUG="262144"), kernel, unary, conn, alphas, tol, iters, **kw)
    assert _same(off, late)


def test_granules_after_a_reset(hip, monkeypatch):
    """Epochs restart when a plan is solved again from zero; the granules' tags must not survive that."""
    from stereo_amd.trws import TrwsPlan, MESSAGES_MINPLUS
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    unary, conn, alphas = _noise(8, 64, 80, 16)
    N, K = unary.shape
    plan = TrwsPlan(1, K, N, conn.T)
    plan.upload(unary.T, alphas, 4.0, positions=np.arange(K, dtype=np.float64))
    plan.iterate(3, max_relgap=-1e300)
    first = plan.result()
    plan.upload(unary.T * 0.5, alphas, 4.0, positions=np.arange(K, dtype=np.float64))
    plan.reset()
    plan.iterate(3, max_relgap=-1e300)
    second = plan.result()
    plan.close()
    monkeypatch.setenv("STEREO_HIP_TRWS_GRANULES", "0")
    ref = TrwsPlan(1, K, N, conn.T)
    ref.upload(unary.T * 0.5, alphas, 4.0, positions=np.arange(K, dtype=np.float64))
    ref.iterate(3, max_relgap=-1e300)
    want = ref.result()
    ref.close()
    assert np.array_equal(second[0], want[0]) and second[1:] == want[1:]
    assert not (np.array_equal(first[0], second[0]) and first[1:] == second[1:])
