"""Host tests of the chain schedule OFF the image grid (no GPU): the graph families of graph_families.py through the
checks test_host_graph.py, test_granule_marks_cpu.py and test_spec_cpu.py make on grids, plus the rule that holds
everything together -- the library never hands the descriptor-driven kernels a schedule whose loader protocol its own
host model (trws.simulate_look_ahead) cannot show to terminate.  A graph the model rejects goes to the
generic kernel: stereo_trws_schedule reports it as not eligible."""
import numpy as np
import pytest

import graph_families as gf
from helpers import grid_conn
from test_granule_marks_cpu import _check as check_granule_marks

FAMILIES = gf.fast_families(1)
FAMILIES_BIG = gf.fast_families(2)


def _eligible(N, conn):
    from stereo_amd import StereoHipError
    from stereo_amd.trws import schedule
    try:
        schedule(N, conn.T, 0, 0)
        return True
    except StereoHipError as e:
        assert "not eligible" in str(e)
        return False


def _real_bit12(N, conn, d):
    """Bit 12 of descriptor word 2 by rank, as the kernels read it."""
    from stereo_amd.trws import descriptors
    desc = descriptors(N, conn.T, d)
    bit = np.zeros(N, bool)
    bit[desc[:, 1]] = (desc[:, 2] >> 12) & 1 == 1
    return bit


def _model_terminates(N, conn, capacity=0):
    """The protocol model on the schedule built for `capacity` resident workgroups.  The descriptors' own bit 12 can be
    read for capacity 0 only; a schedule built for a capacity may be another one, and takes the restated rule
    (test_bit12_is_the_restated_rule: the two agree wherever both exist)."""
    from stereo_amd.trws import schedule, simulate_look_ahead, look_ahead_allowed
    for d in (0, 1):
        s = schedule(N, conn.T, d, capacity)
        if not simulate_look_ahead(s, look_ahead_allowed(s, d) if capacity else _real_bit12(N, conn, d)):
            return False
    return True


def _check_schedule_graph(N, conn, capacity):
    """test_host_graph._check_schedule for any connectivity."""
    from stereo_amd.trws import analyze, schedule, simulate_schedule
    a = analyze(N, conn.T)
    rank = a["rank"]
    tail_r, head_r = rank[a["tail"]], rank[a["head"]]
    levels = int(a["level"].max()) + 1
    out = {}
    for d in (0, 1):
        s = schedule(N, conn.T, d, capacity)
        R = len(s["ticket_run"])
        assert sorted(s["rank_at"].tolist()) == list(range(N))            # every node visited once
        assert sorted(s["ticket_run"].tolist()) == list(range(R))         # every run dispensed once
        assert s["run_ptr"][0] == 0 and s["run_ptr"][-1] == N and (np.diff(s["run_ptr"]) > 0).all()
        pos_of = np.empty(N, np.int64); pos_of[s["rank_at"]] = np.arange(N)
        run_of_pos = np.repeat(np.arange(R), np.diff(s["run_ptr"]))
        need = [set() for _ in range(N)]
        src, dst = (tail_r, head_r) if d == 0 else (head_r, tail_r)
        for x, y in zip(src.tolist(), dst.tolist()):
            need[y].add(x)
        for r in range(N):
            listed = s["dep_rank"][s["dep_ptr"][r]:s["dep_ptr"][r + 1]].tolist()
            deps = set(listed)
            assert len(listed) <= 4 and len(deps) == len(listed)
            pr = int(s["pred_rank"][r])
            if pr >= 0:
                # the LDS hand-over comes from the node visited just before in the same run
                assert pos_of[pr] == pos_of[r] - 1 and run_of_pos[pos_of[pr]] == run_of_pos[pos_of[r]]
                deps.add(pr)
            # (the rank-contiguous fallback schedule also hands over from TWO visits back, through the LDS ring that
            #  keeps the last visits' messages: slots 8 .. 15 of descriptor words 12 .. 19)
            for x in need[r] - deps:
                assert pos_of[x] == pos_of[r] - 2 and run_of_pos[pos_of[x]] == run_of_pos[pos_of[r]], (r, x)
                assert (s["rank_at"] == (np.arange(N) if d == 0 else np.arange(N)[::-1])).all(), "ring hand-over outside the fallback"
                deps.add(x)
            assert deps == need[r], (r, deps, need[r])
        # every run resident: the chain schedule (capacity 0) takes exactly the DAG depth -- a node follows the one it
        # hangs on; a schedule built for few workgroups may be the rank-contiguous one, whose runs also string
        # together nodes that do not depend on each other: it must finish, its length is not promised
        mk, ok = simulate_schedule(s, 10 ** 9)
        assert ok and (mk == levels or capacity)
        if capacity:
            mk2, ok2 = simulate_schedule(s, capacity)
            assert ok2, "schedule deadlocks with %d resident workgroups" % capacity
            out[d] = mk2 / levels
    return out


@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_family_schedule(fam):
    name, N, conn = fam
    assert conn.min() >= 0 and conn.max() < N and (conn[:, 0] != conn[:, 1]).all()
    assert np.bincount(conn.ravel(), minlength=N).max() <= 8
    assert _eligible(N, conn), "%s left the descriptor-driven kernels" % name
    for capacity in (0, 2, 3, 16):
        _check_schedule_graph(N, conn, capacity)
        assert _model_terminates(N, conn, capacity)


@pytest.mark.parametrize("fam", FAMILIES_BIG, ids=[f[0] for f in FAMILIES_BIG])
def test_family_schedule_at_parity_size(fam):
    """The graphs the GPU parity tests run (a few thousand nodes), at the capacities a device gives a plan: every run
    resident, one workgroup per CU (256), two per CU."""
    from stereo_amd.trws import schedule, simulate_schedule
    name, N, conn = fam
    assert _eligible(N, conn)
    for capacity in (0, 16, 256, 512):
        assert _model_terminates(N, conn, capacity)
        for d in (0, 1):
            s = schedule(N, conn.T, d, capacity)
            assert sorted(s["rank_at"].tolist()) == list(range(N))
            assert simulate_schedule(s, capacity or 10 ** 9)[1], (name, d, capacity)


def test_masked_image_with_more_runs_than_workgroups():
    """15 % of an image masked out: far more runs than a 256-CU device keeps resident (one workgroup per CU for the
    wide kernel, up to four for the others) -- the case the GPU parity test runs.  Whatever schedule the library
    builds for that capacity must complete in ticket order with that many workgroups, and with far fewer."""
    from stereo_amd.trws import schedule, simulate_schedule
    for (H, W), capacities in (((40, 50), (256, 64, 16)), ((80, 100), (1024, 256))):
        N, conn = gf.masked_grid(H, W, 0.15, 3)
        assert len(schedule(N, conn.T, 0, 0)["ticket_run"]) > capacities[0]
        for capacity in capacities:
            runs = []
            for d in (0, 1):
                s = schedule(N, conn.T, d, capacity)
                runs.append(len(s["ticket_run"]))
                assert simulate_schedule(s, capacity)[1], (d, capacity)
            assert max(runs) > capacity
            assert _model_terminates(N, conn, capacity)


@pytest.mark.parametrize("fam", FAMILIES + FAMILIES_BIG[:7], ids=[f[0] for f in FAMILIES] + [f[0] + "-big" for f in FAMILIES_BIG[:7]])
def test_family_spec_schedule(fam):
    from stereo_amd.trws import schedule, spec_schedule, simulate_spec_schedule
    name, N, conn = fam
    for d in (0, 1):
        sp = spec_schedule(N, conn.T, d)
        if sp is None:
            continue
        s = schedule(N, conn.T, d, 0)
        for wg in (10 ** 9, 16, 3):
            assert simulate_spec_schedule(s, sp, wg)[1], (name, d, wg)


def test_single_edged_grid_gets_a_speculative_schedule():
    from stereo_amd.trws import spec_schedule
    N, conn = gf.single_grid(30, 40)
    for d in (0, 1):
        sp = spec_schedule(N, conn.T, d)
        assert sp is not None and sp["nseg"] == 8


@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_family_granule_marks(fam):
    from stereo_amd.trws import descriptors
    name, N, conn = fam
    marks = sum(int((descriptors(N, conn.T, d)[:, 57] & 255).astype(bool).sum()) for d in (0, 1))
    check_granule_marks(N, conn.T, marks > 0)


def test_bit12_is_the_restated_rule():
    from stereo_amd.trws import schedule, look_ahead_allowed
    for name, N, conn in FAMILIES + FAMILIES_BIG:
        for d in (0, 1):
            assert np.array_equal(_real_bit12(N, conn, d), look_ahead_allowed(schedule(N, conn.T, d, 0), d)), (name, d)


def test_graphs_outside_the_range_are_refused():
    for name, N, conn in gf.slow_families():
        assert not _eligible(N, conn), name
    N8, c8 = gf.star_in_chain(8)
    N9, c9 = gf.star_in_chain(9)
    assert np.bincount(c8.ravel()).max() == 8 and np.bincount(c9.ravel()).max() == 9
    assert _eligible(N8, c8) and not _eligible(N9, c9)


def _spec_terminates(N, conn, workgroups=(10 ** 9, 16, 3)):
    """Whatever speculative schedule the library hands out finishes in its model (trws.simulate_spec_schedule: a node of
    the cut run is visible only once its segment has committed)."""
    from stereo_amd.trws import schedule, spec_schedule, simulate_spec_schedule
    for d in (0, 1):
        sp = spec_schedule(N, conn.T, d)
        if sp is not None:
            s = schedule(N, conn.T, d, 0)
            if not all(simulate_spec_schedule(s, sp, wg)[1] for wg in workgroups):
                return False
    return True


def _would_be_spec(s, L=16):
    """The speculative schedule trws_graph.cpp derives from a chain schedule, restated BEFORE the library judges it:
    the longest run (the first of them) cut into segments of L nodes, the last one taking the remainder; the runner's
    ticket first, the cut run's ticket replaced by its segments'."""
    run_ptr, ticket_run = s["run_ptr"], s["ticket_run"]
    R = len(run_ptr) - 1
    lens = np.diff(run_ptr)
    best = int(np.argmax(lens))
    c0, c1, nseg = int(run_ptr[best]), int(run_ptr[best + 1]), int(lens[best]) // L
    ptr, kind = [], []
    for k in range(R):
        if k == best:
            ptr += [c0 + q * L for q in range(nseg)]; kind += [1 + q for q in range(nseg)]
        else:
            ptr.append(int(run_ptr[k])); kind.append(0)
    ptr.append(int(run_ptr[R]))
    tickets = [-1]
    for k in ticket_run.tolist():
        tickets += [best + q for q in range(nseg)] if k == best else [k if k < best else k + nseg - 1]
    return dict(run=best, c0=c0, c1=c1, seg_len=L, nseg=nseg, run_ptr=np.array(ptr), kind=np.array(kind), ticket_run=np.array(tickets))


def test_would_be_spec_is_the_librarys():
    from stereo_amd.trws import schedule, spec_schedule
    for N, conn in (gf.single_grid(30, 40), gf.row_major_grid(40, 50), gf.permuted_grid(40, 50, 2)):
        for d in (0, 1):
            sp, mine = spec_schedule(N, conn.T, d), _would_be_spec(schedule(N, conn.T, d, 0))
            assert sp is not None
            for key in mine:
                assert np.array_equal(sp[key], mine[key]), key


@pytest.mark.parametrize("which", ["172", "302"])
def test_speculative_schedule_that_cannot_commit_is_dropped(which):
    """A long chain with a short side run: the side run hangs on chain node a and feeds chain node b a few steps on.
    Cut into speculative segments, a and b share a segment; a's flag is held back until that segment commits
    (trws_pipe.hip, storer: `if (!(SPEC && seg >= 0)) st_sc1(p.done ...)`), the side run waits for it, b waits for the
    side run, the segment never finishes its walk.  The plain chain schedule terminates: the graph stays on the
    pipelined kernels WITHOUT a speculative schedule in that direction."""
    from stereo_amd.trws import schedule, spec_schedule, simulate_spec_schedule
    N, conn = (gf.SPEC_DEADLOCK172_N, gf.SPEC_DEADLOCK172) if which == "172" else (gf.SPEC_DEADLOCK302_N, gf.SPEC_DEADLOCK302)
    assert _eligible(N, conn) and _model_terminates(N, conn)
    stuck = []
    for d in (0, 1):
        s = schedule(N, conn.T, d, 0)
        would = _would_be_spec(s)
        assert would["nseg"] >= 8
        if not simulate_spec_schedule(s, would, 10 ** 9)[1]:
            stuck.append(d)
            assert spec_schedule(N, conn.T, d) is None
    assert stuck, "the restated speculative schedule terminates: the regression proves nothing"
    assert _spec_terminates(N, conn)


def test_chains_with_side_runs_never_get_an_unproven_speculative_schedule():
    """300 seeded chains of 130 .. 400 nodes with one to three side runs -- the family in which a run is long enough to
    be cut AND other runs hang on it: every speculative schedule handed out finishes in the model; the search must
    meet both outcomes."""
    from stereo_amd.trws import schedule, spec_schedule, simulate_spec_schedule
    kept = dropped = deserved = 0
    for seed in range(300):
        rng = np.random.default_rng(5000 + seed)
        N, conn = gf.chain_with_side_runs(int(rng.integers(130, 400)), seed, gadgets=int(rng.integers(1, 4)))
        assert _eligible(N, conn), seed
        assert _model_terminates(N, conn), seed
        for d in (0, 1):
            s = schedule(N, conn.T, d, 0)
            sp = spec_schedule(N, conn.T, d)
            if sp is not None:
                kept += 1
                assert simulate_spec_schedule(s, sp, 10 ** 9)[1], (seed, d)   # (built for capacity 0: every task resident)
            else:
                dropped += 1
                would = _would_be_spec(s)
                if would["nseg"] >= 8 and not simulate_spec_schedule(s, would, 10 ** 9)[1]:
                    deserved += 1
    print("chains with side runs: %d speculative schedules kept, %d not built or dropped, %d of them because the model deadlocks"
          % (kept, dropped, deserved))
    assert kept > 0 and deserved > 0


def _chain_schedule_model(N, conn, d):
    """The protocol model on the chain schedule BEFORE the library judges it, restated here from the oriented edges
    (trws_graph.cpp's chain builder: a node extends the run of the node visited two steps or one step earlier that it
    depends on and that still ends its run, two steps first) -- so that a rejected graph can be shown to deserve it."""
    from stereo_amd.trws import analyze, simulate_look_ahead
    a = analyze(N, conn.T)
    rank = a["rank"]
    src, dst = (rank[a["tail"]], rank[a["head"]]) if d == 0 else (rank[a["head"]], rank[a["tail"]])
    need = [[] for _ in range(N)]
    for x, y in zip(src.tolist(), dst.tolist()):
        if x not in need[y]:
            need[y].append(x)
    order = list(range(N)) if d == 0 else list(range(N - 1, -1, -1))
    pos = {r: p for p, r in enumerate(order)}
    run_of, tail_of, runs, pred = {}, [], [], {}
    for p, r in enumerate(order):
        best = None
        for o in need[r]:
            if p - pos[o] in (1, 2) and tail_of[run_of[o]] == o and (best is None or pos[o] < pos[best]):
                best = o
        if best is None:
            run_of[r] = len(runs); runs.append([r]); tail_of.append(r)
        else:
            run_of[r] = run_of[best]; runs[run_of[r]].append(r); tail_of[run_of[r]] = r; pred[r] = best
    rank_at = np.array([r for run in runs for r in run], np.int64)
    run_ptr = np.cumsum([0] + [len(run) for run in runs])
    dep_ptr, dep_rank = [0], []
    for r in range(N):
        dep_rank += [x for x in need[r] if x != pred.get(r)]
        dep_ptr.append(len(dep_rank))
    s = dict(rank_at=rank_at, run_ptr=run_ptr, dep_ptr=np.array(dep_ptr), dep_rank=np.array(dep_rank, np.int64))
    return simulate_look_ahead(s, np.zeros(N, bool))


def test_the_eight_node_deadlock_goes_to_the_generic_kernel():
    """Forward sweep of DEADLOCK8: two runs whose second nodes each wait for the other's first node.  The visit that
    computes a run's first node ends at a barrier its loader reaches only with the second node's dependencies visible,
    and the first node's flag is raised behind that barrier (trws_pipe.hip: wait_for_dependencies_w in the loader's
    visit loop, st_sc1(p.done ...) in the storer's): neither run can move.  The graph is inside the degree limits, and
    the library must refuse it the descriptor-driven kernels."""
    N, conn = gf.DEADLOCK8_N, gf.DEADLOCK8
    assert np.bincount(conn.ravel(), minlength=N).max() <= 4          # degrees alone would admit it
    assert not _chain_schedule_model(N, conn, 0)                      # the restated chain schedule does deadlock
    assert not _eligible(N, conn)
    from stereo_amd import StereoHipError
    from stereo_amd.trws import descriptors
    with pytest.raises(StereoHipError, match="outside the descriptor-driven kernels' range"):
        descriptors(N, conn.T, 0)


def test_no_unproven_schedule_is_ever_handed_out():
    """Over every family and 1200 seeded random sparse graphs (degree <= 4: the degree limits always hold): the
    library either refuses the graph the descriptor kernels -- only where the restated chain schedule's model really
    deadlocks -- or hands out a schedule on which the model terminates with the descriptors' own bit 12."""
    refused = {"small": 0, "isolated": 0, "large": 0}
    count = {"small": 0, "isolated": 0, "large": 0}
    graphs = [(n, N, c, None) for n, N, c in FAMILIES + FAMILIES_BIG]
    for seed in range(1200):
        rng = np.random.default_rng(10_000 + seed)
        if seed < 500:
            kind, (N, c) = "small", gf.random_sparse(int(rng.integers(8, 15)), seed)
        elif seed < 1000:
            kind, (N, c) = "isolated", gf.random_sparse(int(rng.integers(8, 15)), seed, isolated=int(rng.integers(1, 4)))
        else:
            kind, (N, c) = "large", gf.random_sparse(200, seed)
        graphs.append((kind, N, c, kind))
    for name, N, c, kind in graphs:
        if _eligible(N, c):
            assert _model_terminates(N, c), (name, N, c.tolist() if N < 20 else None)
            assert _spec_terminates(N, c, (10 ** 9,) if kind else (10 ** 9, 16, 3)), (name, N, c.tolist() if N < 20 else None)
            if kind is not None:
                assert _chain_schedule_model(N, c, 0) and _chain_schedule_model(N, c, 1)
        else:
            assert kind is not None, "%s fell back to the generic kernel" % name     # the families all stay
            assert not (_chain_schedule_model(N, c, 0) and _chain_schedule_model(N, c, 1)), (name, c.tolist())
            refused[kind] += 1
        if kind is not None:
            count[kind] += 1
    for kind in count:
        print("random sparse graphs (%s): %d of %d go to the generic kernel (%.1f %%)"
              % (kind, refused[kind], count[kind], 100.0 * refused[kind] / count[kind]))
    assert refused["small"] + refused["isolated"] > 0, "the search no longer finds a deadlock: it proves nothing"
    assert sum(refused.values()) < 0.2 * sum(count.values())


def test_grid_tests_still_see_the_grid_unchanged():
    """The check accepts every image grid (nothing may fall back there): spot sizes incl. the degenerate ones."""
    for H, W in [(1, 2), (2, 1), (1, 9), (9, 1), (2, 2), (3, 3), (7, 9), (30, 40), (120, 90)]:
        assert _eligible(H * W, grid_conn(H, W)), (H, W)


def test_grid_derived_families_never_fall_back():
    """Random sizes of every grid-derived family, at the capacities a 256-CU device gives a plan (0: every run resident;
    256: the wide kernel; 1024: four workgroups per CU): none is refused the descriptor-driven kernels, whichever schedule
    the capacity makes the library build."""
    from stereo_amd.trws import schedule
    rng = np.random.default_rng(77)
    for trial in range(40):
        H, W = int(rng.integers(2, 70)), int(rng.integers(2, 70))
        s = int(rng.integers(0, 1 << 30))
        for name, (N, conn) in (("single", gf.single_grid(H, W)), ("shuffled", gf.shuffled_grid(H, W, s)),
                                ("permuted", gf.permuted_grid(H, W, s)), ("row-major", gf.row_major_grid(H, W)),
                                ("masked", gf.masked_grid(H, W, 0.15, s)), ("dropped", gf.dropped_edges_grid(H, W, 0.25, s)),
                                ("two-grids", gf.two_grids(H, W, max(H // 2, 1), W))):
            if len(conn) == 0:
                continue
            for capacity in (0, 256, 1024):
                for d in (0, 1):
                    r = schedule(N, conn.T, d, capacity)      # raises StereoHipError if the graph is not eligible
                    assert len(r["rank_at"]) == N, (name, H, W, s, capacity)
