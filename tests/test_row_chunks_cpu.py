"""Host tests of the sub-row runs (no GPU; trws_graph.h: Sweep::Chunked): the chain schedule with every
ordinary run cut into runs of at most C positions, as the K <= 64 kernel walks it where a sweep has more runs than
resident workgroups.  Through stereo_trws_schedule_chunked, which builds the schedule for a given C and number of resident
workgroups and returns it the way the kernels see it (runs, tickets, and predecessor / dependencies read back from the
descriptors).

Checked on grids 6 x 20, 9 x 33 and 12 x 40 with C in {4, 8, 16} and 2, 3 and 4 resident workgroups, both directions:
runs of at most C positions that partition the nodes in the visit order of the whole rows; a ticket order in which
every dependency of a run lies in an earlier ticket; termination of the protocol model with that many workgroups; C = 0
gives the chain schedule's arrays, descriptors included; and graphs off the image grid, which have fewer runs than a
device has compute units, keep the chain schedule whatever C says."""
import importlib

import numpy as np
import pytest

import graph_families as gf
from helpers import grid_conn

T = importlib.import_module("stereo_amd.trws")

GRIDS = [(6, 20), (9, 33), (12, 40)]
CHUNKS = [4, 8, 16]
WORKGROUPS = [2, 3, 4]
CASES = [(H, W, C, wg, d) for H, W in GRIDS for C in CHUNKS for wg in WORKGROUPS for d in (0, 1)]

_plain, _chunked = {}, {}


def plain(H, W, d):
    if (H, W, d) not in _plain:
        conn = grid_conn(H, W)
        _plain[H, W, d] = (T.schedule(H * W, conn.T, d), T.descriptors(H * W, conn.T, d))
    return _plain[H, W, d]


def chunked(H, W, C, wg, d):
    if (H, W, C, wg, d) not in _chunked:
        _chunked[H, W, C, wg, d] = T.schedule_chunked(H * W, grid_conn(H, W).T, d, C, wg)
    return _chunked[H, W, C, wg, d]


def run_of_rank(s):
    out = np.zeros(len(s["rank_at"]), np.int64)
    for k in range(len(s["run_ptr"]) - 1):
        out[s["rank_at"][s["run_ptr"][k]:s["run_ptr"][k + 1]]] = k
    return out


@pytest.mark.parametrize("H,W,C,wg,d", CASES)
def test_runs_are_pieces_of_the_rows(H, W, C, wg, d):
    s, (p, _) = chunked(H, W, C, wg, d), plain(H, W, d)
    assert s["chunked"] and s["chunk"] == C
    lens = np.diff(s["run_ptr"])
    whole = s["spec_run"] if s["spec_ok"] else -1
    assert all(n <= C for k, n in enumerate(lens) if k != whole) and lens.min() >= 1
    # the same positions in the same order, and no run that crosses the border between two whole runs
    assert np.array_equal(s["rank_at"], p["rank_at"])
    assert s["run_ptr"][0] == 0 and s["run_ptr"][-1] == H * W
    assert set(p["run_ptr"].tolist()) <= set(s["run_ptr"].tolist())
    # every run is drawn once
    assert sorted(s["ticket_run"].tolist()) == list(range(len(lens)))
    # inside a piece the hand-over is the whole row's; a piece's first node takes nothing in LDS and waits for the node
    # in front like for any other
    run = run_of_rank(s)
    for k in range(len(lens)):
        a, b = int(s["run_ptr"][k]), int(s["run_ptr"][k + 1])
        first = int(s["rank_at"][a])
        assert s["pred_rank"][first] == -1
        before = int(p["pred_rank"][first])
        if before >= 0:
            assert before in s["dep_rank"][s["dep_ptr"][first]:s["dep_ptr"][first + 1]].tolist() and run[before] != k
        for pos in range(a + 1, b):
            r = int(s["rank_at"][pos])
            assert s["pred_rank"][r] == p["pred_rank"][r] == s["rank_at"][pos - 1]
            assert np.array_equal(s["dep_rank"][s["dep_ptr"][r]:s["dep_ptr"][r + 1]], p["dep_rank"][p["dep_ptr"][r]:p["dep_ptr"][r + 1]])


@pytest.mark.parametrize("H,W,C,wg,d", CASES)
def test_tickets_extend_the_dependencies(H, W, C, wg, d):
    s = chunked(H, W, C, wg, d)
    run = run_of_rank(s)
    ticket = np.zeros(len(s["ticket_run"]), np.int64)
    ticket[s["ticket_run"]] = np.arange(len(ticket))
    for r in range(H * W):
        for x in s["dep_rank"][s["dep_ptr"][r]:s["dep_ptr"][r + 1]]:
            assert run[x] == run[r] or ticket[run[x]] < ticket[run[r]], (r, int(x))
    # ... and follow the wavefront, not the rows: the pieces of one row are not drawn one behind the other
    rows = [k for k in range(len(ticket) - 1) if s["run_ptr"][k + 1] in set(plain(H, W, d)[0]["run_ptr"].tolist())]
    inner = [k for k in range(len(ticket) - 1) if k not in rows]   # pieces with a piece of the same row behind them
    assert any(ticket[k + 1] != ticket[k] + 1 for k in inner)


@pytest.mark.parametrize("H,W,C,wg,d", CASES)
def test_protocol_model_terminates(H, W, C, wg, d):
    s = chunked(H, W, C, wg, d)
    allowed = T.look_ahead_allowed(s, d)
    # bit 12 of the descriptors is the rule restated on these runs
    bit12 = np.zeros(H * W, bool)
    bit12[s["desc"][:, 1]] = (s["desc"][:, 2] >> 12) & 1
    assert np.array_equal(bit12, allowed)
    assert T.simulate_look_ahead(s, allowed)
    for handover in (0.0, 2.5):
        span, finished = T.simulate_schedule(s, wg, handover=handover)
        assert finished
    # fewer workgroups than the schedule was checked for is outside the promise; more is inside it
    assert T.simulate_schedule(s, wg + 5)[1]


@pytest.mark.parametrize("H,W", GRIDS)
def test_chunk_zero_is_the_chain_schedule(H, W):
    for d in (0, 1):
        p, desc = plain(H, W, d)
        z = T.schedule_chunked(H * W, grid_conn(H, W).T, d, 0, 3)
        assert not z["chunked"]
        for key in ("rank_at", "run_ptr", "ticket_run", "pred_rank", "dep_ptr", "dep_rank"):
            assert np.array_equal(z[key], p[key]), key
        assert np.array_equal(z["desc"], desc)
        # building the pieces leaves the chain schedule's own descriptors alone: a run with as many workgroups as runs
        # is below the gate, and returns them
        big = T.schedule_chunked(H * W, grid_conn(H, W).T, d, 8, len(p["run_ptr"]) - 1)
        assert not big["chunked"] and np.array_equal(big["desc"], desc)


def test_granule_marks_follow_the_pieces():
    """word 57 on the pieces: a piece's first node takes the rows of the node in front as granules (both runs ordinary,
    the producer's ticket earlier), and that node publishes them"""
    H, W, C, d = 9, 33, 8, 0
    s = chunked(H, W, C, 3, d)
    p, _ = plain(H, W, d)
    pos_of = np.zeros(H * W, np.int64)
    pos_of[s["rank_at"]] = np.arange(H * W)
    seen = 0
    for k in range(len(s["run_ptr"]) - 1):
        first = int(s["rank_at"][s["run_ptr"][k]])
        before = int(p["pred_rank"][first])
        if before < 0:
            continue
        D, B = s["desc"][pos_of[first]], s["desc"][pos_of[before]]
        nout, nin = D[2] & 15, (D[2] >> 4) & 15
        rows = [j for j in range(nout, nout + nin) if D[32 + j] == B[0]]
        assert rows and all((D[55] >> j) & 1 for j in rows)          # fetched from memory
        if bin(int(D[55]) & 255).count("1") > 4:                     # (the kernel sweeps at most four granule rows a node)
            assert int(D[57]) & 255 == 0
            continue
        assert all((D[57] >> j) & 1 for j in rows)                   # as granules
        for j in rows:
            out = [i for i in range(B[2] & 15) if B[4 + i] == D[4 + j]]
            assert len(out) == 1 and (B[57] >> (8 + out[0])) & 1 and (B[57] >> 20) & 1
        seen += 1
    assert seen > 10


@pytest.mark.parametrize("name,N,conn", gf.fast_families(), ids=[f[0] for f in gf.fast_families()])
def test_graphs_off_the_grid_keep_their_schedule(name, N, conn):
    for d in (0, 1):
        p = T.schedule(N, conn.T, d)
        s = T.schedule_chunked(N, conn.T, d, 8, 256)
        assert not s["chunked"]
        for key in ("rank_at", "run_ptr", "ticket_run", "pred_rank", "dep_ptr", "dep_rank"):
            assert np.array_equal(s[key], p[key]), key
        assert np.array_equal(s["desc"], T.descriptors(N, conn.T, d))
