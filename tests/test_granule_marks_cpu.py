"""Host marks of the tagged-granule row hand-over (descriptor word 57, trws_graph.h: kDescGran), no device: every marked
incoming row joins two ordinary runs of one sweep whose producer draws the earlier ticket; nothing of the speculative
schedule's cut run (its segments and its runner) is marked; the producer publishes exactly the rows its consumers
take as granules; and a dependency is only dropped from the flag wait when every row it feeds comes as granules."""
import numpy as np
import pytest

from helpers import grid_conn

GRAN = 57


def _random_graph(N, seed):
    # an irregular graph inside the pipelined kernels' range: a path + a few random chords (<= 8 edges per node)
    rng = np.random.default_rng(seed)
    edges = [(i, i + 1) for i in range(N - 1)]
    deg = np.zeros(N, int)
    for a, b in edges:
        deg[a] += 1; deg[b] += 1
    for _ in range(N):
        a, b = rng.integers(0, N, 2)
        if a != b and deg[a] < 3 and deg[b] < 3:
            edges.append((int(a), int(b))); deg[a] += 1; deg[b] += 1
    return np.array(edges, np.int64).T


def _check(N, conn0, expect_marks):
    from stereo_amd.trws import descriptors, schedule, spec_schedule
    marked_total = 0
    for d in (0, 1):
        s = schedule(N, conn0, d)
        sp = spec_schedule(N, conn0, d)
        desc = descriptors(N, conn0, d).astype(np.int64)
        rank_at, run_ptr, ticket_run = s["rank_at"], s["run_ptr"], s["ticket_run"]
        R = len(run_ptr) - 1
        run_of_pos = np.repeat(np.arange(R), np.diff(run_ptr))
        pos_of_rank = np.empty(N, np.int64)
        pos_of_rank[rank_at] = np.arange(N)
        ticket_of = np.empty(R, np.int64)
        ticket_of[ticket_run] = np.arange(R)
        cut = sp["run"] if sp is not None else -1
        published = {}   # producer position -> outgoing slots its consumers take as granules
        for p in range(N):
            D = desc[p]
            w = int(D[GRAN])
            gm, flags = w & 255, (w >> 16) & 15
            nout, nin, nd = D[2] & 15, (D[2] >> 4) & 15, (D[2] >> 8) & 15
            if not gm:
                continue
            marked_total += bin(gm).count("1")
            kr = run_of_pos[p]
            assert kr != cut, "a node of the cut run (a segment of the speculative schedule) takes granules"
            assert gm & ~int(D[55]) == 0, "a granule row that is not a fetched row"
            assert bin(gm).count("1") <= 4
            for k in range(8):
                if not (gm >> k) & 1:
                    continue
                assert nout <= k < nout + nin
                e, other = int(D[4 + k]), int(D[32 + k])
                # the other end, by rank: its position and run
                po = int(np.flatnonzero(desc[:, 0] == other)[0])
                ko = run_of_pos[po]
                assert ko != kr and ko != cut, "granules inside one run or from the cut run"
                assert ticket_of[ko] < ticket_of[kr], "the producer's run draws a later ticket"
                P = desc[po]
                slots = [j for j in range(P[2] & 15) if P[4 + j] == e]
                assert len(slots) == 1
                published.setdefault(po, set()).add(slots[0])
            # dependencies: dropped from the flag wait only when every row they feed is a granule row
            rows_of = {}
            for k in range(nout, nout + nin):
                if (int(D[55]) >> k) & 1:
                    rows_of.setdefault(int(np.flatnonzero(desc[:, 0] == D[32 + k])[0]), []).append(k)
            for q in range(nd):
                dep_pos = pos_of_rank[int(D[20 + q])]
                ks = rows_of.get(int(dep_pos), [])
                covered = bool(ks) and all((gm >> k) & 1 for k in ks)
                assert ((flags >> q) & 1) == (0 if covered else 1)
        # producers: bits 8-15 are exactly the published slots, bit 20 with any of them
        for p in range(N):
            w = int(desc[p, GRAN])
            want = published.get(p, set())
            assert ((w >> 8) & 255) == sum(1 << j for j in want)
            assert ((w >> 20) & 1) == (1 if want else 0)
            if want:
                assert run_of_pos[p] != cut
    assert (marked_total > 0) == expect_marks


@pytest.mark.parametrize("shape", [(12, 17), (30, 40)])
def test_grid_marks(shape):
    H, W = shape
    _check(H * W, grid_conn(H, W).T, True)


def test_teddy_grid_marks():
    # the flagship workload's graph: only the descriptor words are looked at, vectorised where it matters
    from stereo_amd.trws import descriptors, schedule, spec_schedule
    H, W = 375, 450
    N = H * W
    conn0 = grid_conn(H, W).T
    for d in (0, 1):
        s, sp = schedule(N, conn0, d), spec_schedule(N, conn0, d)
        desc = descriptors(N, conn0, d).astype(np.int64)
        run_ptr, ticket_run = s["run_ptr"], s["ticket_run"]
        R = len(run_ptr) - 1
        run_of_pos = np.repeat(np.arange(R), np.diff(run_ptr))
        ticket_of = np.empty(R, np.int64)
        ticket_of[ticket_run] = np.arange(R)
        pos_of_node = np.empty(N, np.int64)
        pos_of_node[desc[:, 0]] = np.arange(N)
        w = desc[:, GRAN]
        gm = w & 255
        cons = np.flatnonzero(gm)
        assert len(cons) > 0.9 * N, "the interior rows take their rows as granules"
        cut_pos = run_of_pos == sp["run"]
        assert not (w[cut_pos] & 0x1fffff).any(), "the border chain (runner and segments) is not marked"
        assert ((gm & ~desc[:, 55]) == 0).all()
        for k in range(8):
            sel = cons[(gm[cons] >> k) & 1 == 1]
            prod = pos_of_node[desc[sel, 32 + k]]
            assert (run_of_pos[prod] != run_of_pos[sel]).all()
            assert not cut_pos[prod].any()
            assert (ticket_of[run_of_pos[prod]] < ticket_of[run_of_pos[sel]]).all()
            # the producer publishes the row under the same edge id
            pub = (w[prod] >> 8) & 255
            hit = np.zeros(len(sel), bool)
            for j in range(8):
                hit |= ((pub >> j) & 1 == 1) & (desc[prod, 4 + j] == desc[sel, 4 + k]) & (j < (desc[prod, 2] & 15))
            assert hit.all()
        # an interior node of a row waits for no flag at all: its only foreign dependency is the node above
        nd = (desc[cons, 2] >> 8) & 15
        flags = (w[cons] >> 16) & 15
        assert ((flags & ~((1 << nd) - 1)) == 0).all()
        assert (flags == 0).mean() > 0.9


def test_non_grid_graph_marks():
    from stereo_amd.trws import descriptors
    N = 300
    conn0 = _random_graph(N, 5)
    desc0 = descriptors(N, conn0, 0)
    # whatever the schedule makes of it, every mark obeys the rule
    marks = int((desc0[:, GRAN] & 255).astype(bool).sum())
    _check(N, conn0, marks > 0)


def test_strips_are_not_marked():
    from stereo_amd.strips import strip_layout_host
    H, W = 40, 30
    conn0 = grid_conn(H, W).T
    owner = (np.arange(H * W) % H >= H // 2).astype(np.int32)   # node id = col * H + row: two row bands
    for d in (0, 1):
        for s in (0, 1):
            L = strip_layout_host(H * W, conn0, owner, 2, s, d)
            assert not L["desc"][:, GRAN].any()
