"""-m gpu: every path of the K <= 64 message routine that carries the running min-plus minimum m1 (trws_dev.h:
message_regs), in whole solves against the CPU oracle.

m1 is updated by every trip of the compacted pair loop, by the flat path's window loop, by the merge with a twin's
partial minimum (coop_collect) and, on the cold path, replaced by the second look's.  It has to live in registers
(DESIGN.md 4.4 round 13), and a change of how it is kept must not move a bit on any of these paths.  Every case asserts
that labels, energy and lower bound are oracle.pyoracle.trws's bit for bit after each of 1 .. ITERS iterations, on the
default schedule and on the plain one (STEREO_HIP_TRWS_SPEC=0); the 30 x 40 grid, which gets the speculative schedule,
also with development switch 16384 (the runner's rows made wrong: second walks, where the helpers' exchange areas
hold the first walk's partial minima).

Volumes (shared ascending positions 0 .. K - 1, smoothness kernel 1, tol 8: truncation window of 8 entries), one per
path.  "useful" sources of a message are those with h < min h + alpha lambda.  The counts below are those of a NumPy
restatement of the FIRST forward sweep (plain min-plus messages on the oracle's node order, trws_structure) as
minimum / median / maximum of the useful sources per message over K = 60 and 64, 12 x 9 | 30 x 40 (390 | 4660 messages):
  noise      unary uniform(0, 1600): <= 8 useful sources, the eight-entry case of the compacted loop, nothing split
             (1 / 2 / 6 | 1 / 2 / 7);
  sloped     a V of slope 4 around a per-node centre plus uniform(0, 1), equal weights: 9 .. 32 useful sources,
             every pair of pixels a twin pair, so the pair loop is split and merged through coop_collect
             (8 / 16 / 32 | 7 / 17 / 34: at most 4 | 6 messages at 8 or fewer, 0 | 4 above 32);
  flat       uniform(0, 18), equal weights: more than 32 useful sources, the flat path with its helper
             (44 / 60 / 64 | 43 / 60 / 64);
  flat-pair  the same volume with independent weights 0.25 .. 2 per directed edge: no twins; messages with a small
             weight have 9 .. 32 useful sources (the unsplit compacted loop: 33 and 43 | 477 and 434 messages), nearly
             all others more than 32 (the flat path alone: 356 and 343 | 4155 and 4210);
  ties       noise with a block of nodes whose unary is exactly 0 for every label, like the masked columns of an NCC
             volume: exact ties, failed certificates, the second look's rule and the serial construction;
  near-ties  every node's row from tests/adversarial.py's generators (tangent pairs, exact-slope ramps, truncation-level
             hits, plateaus, far cones: within a few delta or ulps of a tie).
serial_messages() must be 0 on the noise volume (continuous noise: a failed certificate there would be a defect of the
certified path, not of the data) and > 0 on the ties volume; where spec_stats() is active it must show commits, and
it must be active on the 30 x 40 grid by default."""
import numpy as np
import pytest

import adversarial
from helpers import grid_conn

pytestmark = pytest.mark.gpu

ENV = ("STEREO_HIP_TRWS_GRANULES", "STEREO_HIP_TRWS_DEBUG", "STEREO_HIP_TRWS_SPEC", "STEREO_HIP_TRWS_ROW_CHUNK", "STEREO_HIP_TRWS_BLOCKS",
       "STEREO_HIP_TRWS_FAST", "STEREO_HIP_GPUS", "STEREO_HIP_TRWS_MESSAGES", "STEREO_HIP_TRWS_CACHE", "STEREO_HIP_TRWS_CERTIFICATE",
       "STEREO_HIP_TRWS_SPEC_SEG")
ITERS = 3
NEVER = -1e300
TOL = 8.0
VOLUMES = ("noise", "sloped", "flat", "flat-pair", "ties", "near-ties")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("STEREO_HIP_TRWS_SPIN_SECONDS", "3")


def volume(name, H, W, K):
    """(unary (N, K), alphas (E,)) of a named volume; node id = column * H + row (helpers.grid_conn)"""
    N, conn = H * W, grid_conn(H, W)
    E = conn.shape[0]
    rng = np.random.default_rng(1000 * H + 10 * W + K + 100000 * VOLUMES.index(name))
    alphas = np.ones(E)
    lab = np.arange(K, dtype=np.float64)
    if name == "noise":
        unary = rng.uniform(0, 1600, size=(N, K))
    elif name == "sloped":
        centre = rng.uniform(0.2 * K, 0.8 * K, size=(N, 1))
        unary = 4.0 * np.abs(lab[None, :] - centre) + rng.uniform(0, 1, size=(N, K))
    elif name in ("flat", "flat-pair"):
        unary = np.random.default_rng(1000 * H + 10 * W + K + 200000).uniform(0, 18, size=(N, K))   # one volume, two weightings
        if name == "flat-pair":
            alphas = rng.uniform(0.25, 2.0, size=E)
            w = {(int(i), int(j)): x for (i, j), x in zip(conn, alphas)}
            assert all(w[(j, i)] != x for (i, j), x in w.items())
    elif name == "ties":
        unary = rng.uniform(0, 40, size=(N, K))
        col = np.arange(N) // H
        unary[(col >= W // 3) & (col < W // 3 + max(2, W // 5))] = 0.0
    else:
        assert name == "near-ties"
        unary = np.stack([adversarial.heights(rng, lab, 1.0, TOL, adversarial.KINDS[n % len(adversarial.KINDS)]) for n in range(N)])
    return np.ascontiguousarray(unary), alphas


_problems, _wanted = {}, {}


def _problem(name, H, W, K):
    """built once per key, never changed"""
    key = (name, H, W, K)
    if key not in _problems:
        conn = grid_conn(H, W)
        unary, alphas = volume(name, H, W, K)
        pos = np.arange(K, dtype=np.float64)
        q = np.tile(pos, (conn.shape[0], 1))
        _problems[key] = dict(key=key, unary=unary, conn=conn, q=q, alphas=alphas, pos=pos)
    return _problems[key]


def _oracle(oracle, p):
    """the oracle's (labels, energy, bound, iterations) after 1 .. ITERS iterations"""
    if p["key"] not in _wanted:
        _wanted[p["key"]] = [oracle.trws(1, p["unary"], p["conn"], p["q"], p["q"], p["alphas"], TOL, n, NEVER, mode=1) for n in range(1, ITERS + 1)]
    return _wanted[p["key"]]


def _walk(monkeypatch, env, p):
    """one plan, one iteration at a time: its results after each, serial_messages() and spec_stats() at the end"""
    from stereo_amd.trws import TrwsPlan
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        N, K = p["unary"].shape
        plan = TrwsPlan(1, K, N, p["conn"].T)
        plan.upload(p["unary"].T, p["alphas"], TOL, positions=p["pos"])
        assert plan.path() == 2, "path %d, expected the K <= 64 kernel" % plan.path()
        plan.serial_messages(reset=True)
        got = []
        for _ in range(ITERS):
            plan.iterate(1, max_relgap=NEVER)
            got.append(plan.result())
        serial, stats = plan.serial_messages(), plan.spec_stats()
        plan.close()
    return got, serial, stats


def _is(got, want, what):
    lab, en, lb, it = got
    assert it == want[3], what
    assert np.array_equal(lab, want[0]), "%s: labels differ at %d of %d nodes" % (what, int((lab != want[0]).sum()), lab.size)
    assert en == want[1] and lb == want[2], (what, (en, lb), want[1:3])


CASES = [(H, W, K, name) for (H, W) in ((12, 9), (30, 40)) for K in (60, 64) for name in VOLUMES]


@pytest.mark.parametrize("H,W,K,name", CASES, ids=["%dx%d-K%d-%s" % c for c in CASES])
def test_message_minimum_paths(H, W, K, name, hip, oracle, monkeypatch):
    p = _problem(name, H, W, K)
    want = _oracle(oracle, p)
    runs = [("default schedule", {}), ("plain schedule", {"STEREO_HIP_TRWS_SPEC": "0"})]
    if (H, W) == (30, 40):
        runs.append(("second walks", {"STEREO_HIP_TRWS_DEBUG": "16384"}))
    for what, env in runs:
        got, serial, st = _walk(monkeypatch, env, p)
        print(what, "serial messages", serial, "spec", st)
        for n in range(ITERS):
            _is(got[n], want[n], "%s, iteration %d" % (what, n + 1))
        if name == "noise":
            assert serial == 0, (what, serial)
        if name == "ties":
            assert serial > 0, what
        if "STEREO_HIP_TRWS_SPEC" in env:
            assert not st["active"] and st["commits"] == 0, (what, st)
        else:
            assert not st["active"] or st["commits"] > 0, (what, st)
            if (H, W) == (30, 40):
                assert st["active"] and st["commits"] > 0, (what, st)
