"""-m gpu: the HIP roof-duality solver against the exact yardsticks of tests/rd_exact.py -- no QPBO library, no
tolerance -- on every arc-list class (at most 4, 5 .. 16, more than 16 distinct neighbours), through every device
path and under every schedule switch.

Y8 (invariance): the bound and the strong part of the labelling are bit-equal across all of them.  On the fixture's
instances that follows from Y3 and Y4, which pin both to the committed LP values on every path; on the 40 x 50
frustrated grid, which is too large to enumerate, every path is pinned to the CPU restatement (integer costs: its
bound is exact, its strong stage gives the strong labels, its final labels the open set).  Weak labels
may differ between paths; each labelling must satisfy Y1, Y2 and Y5 on its own, and WHICH variables stay unlabelled
is fixed by the LP as well (Y9).

The unions have 1,500 to 6,600 variables in shuffled order: 3 to 13 tiles of 512 variables, as many workgroups
per launch (min(2 * CUs, tiles), at most 64 under Improve), grid barriers between them."""
import ctypes

import numpy as np
import pytest

import rd_exact as rx
from helpers import glass_problem

pytestmark = pytest.mark.gpu

SWITCHES = {                      # "a schedule, not an algorithm"
    "tiled0": ("STEREO_HIP_QPBO_TILED", "0"),
    "switch0": ("STEREO_HIP_QPBO_SWITCH", "0"),
    "adaptive0": ("STEREO_HIP_QPBO_ADAPTIVE", "0"),
    "relabel1": ("STEREO_HIP_QPBO_RELABEL_EVERY", "1"),
    "wrap3": ("STEREO_HIP_QPBO_WRAP_AT", "3"),
}
PATHS = ["nocache", "cache", "plan", "plan_grid", "weak_full", "confined1", "confined0"]
ENV = ["STEREO_HIP_RD_CACHE", "STEREO_HIP_QPBO_WEAK_FULL", "STEREO_HIP_QPBO_CONFINED"] + [v for v, _ in SWITCHES.values()]


@pytest.fixture(scope="module")
def fx():
    return rx.fixture()


def _solve(hip, monkeypatch, path, args, conn, N, grid=None):
    """The results of one path: a list of (result, improve, result of the same path without Improve or None)."""
    from stereo_amd.rd import RdPlan
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    srand = ctypes.CDLL(None).srand
    if path in ("nocache", "cache"):
        monkeypatch.setenv("STEREO_HIP_RD_CACHE", "0" if path == "nocache" else "1")
        plain = hip.rd(*args, conn.T + 1, {})
        srand(3)
        return [(plain, False, None), (hip.rd(*args, conn.T + 1, {"improve": True}), True, plain)]
    if path == "weak_full":
        monkeypatch.setenv("STEREO_HIP_QPBO_WEAK_FULL", "1")
    elif path in ("confined1", "confined0"):
        monkeypatch.setenv("STEREO_HIP_QPBO_CONFINED", path[-1])
    elif path in SWITCHES:
        monkeypatch.setenv(*SWITCHES[path])
    plan = RdPlan(N, conn.T, grid=grid if path == "plan_grid" or path in SWITCHES else None)
    try:
        plain = plan.solve(*args)
        out = [(plain, False, None)]
        if path in ("plan", "plan_grid"):
            out.append((plan.solve(*args), False, None))     # on the buffers and marks the first move left behind
        else:
            srand(3)
            out.append((plan.solve(*args, improve=True), True, plain))
            if path != "weak_full":
                out.append((plan.solve(*args), False, None))   # ... and on what Improve left behind
    finally:
        plan.close()
    return out


def _check_all(hip, monkeypatch, path, inst):
    for result, improve, plain in _solve(hip, monkeypatch, path, inst.args(), inst.conn, inst.N, inst.grid):
        try:
            rx.check(inst, result, improve=improve, plain_nu=plain[3] if plain else None)
        except rx.Violation as e:
            raise AssertionError("%s, path %s%s: %s" % (inst.name, path, ", Improve" if improve else "", e))


@pytest.mark.parametrize("path", [p for p in PATHS if p != "plan_grid"])
@pytest.mark.parametrize("cls", rx.CLASSES)
def test_small_instances(cls, path, fx, hip, monkeypatch):
    """36 enumerated instances per class, every cost family: one tile, one workgroup."""
    for inst in fx.small_of(cls):
        _check_all(hip, monkeypatch, path, inst)


UNIONS = ["le4", "le4grid", "mid", "hub", "big"]     # (only le4grid has an image grid behind it)
UNION_CASES = [(n, p) for n in UNIONS for p in PATHS + sorted(SWITCHES) if p != "plan_grid" or n == "le4grid"]


@pytest.mark.parametrize("name,path", UNION_CASES, ids=["%s-%s" % c for c in UNION_CASES])
def test_unions(name, path, fx, hip, monkeypatch):
    """Disjoint unions of enumerable components under shuffled ids: several tiles, workgroups and grid barriers."""
    _check_all(hip, monkeypatch, path, fx.unions[name])


def test_unions_reach_the_paths_they_are_for(fx):
    """The class is decided by the longest arc list of a doubled node, the launch by the number of tiles."""
    want = {"le4": (4, 4, 4), "le4grid": (4, 4, 4), "big": (4, 4, 13), "mid": (5, 16, 3), "hub": (17, 19, 3)}
    for name, (lo, hi, tiles) in want.items():
        u = fx.unions[name]
        assert lo <= u.max_degree() <= hi
        assert (u.N + 511) // 512 == tiles
    H, W = fx.unions["le4grid"].grid     # image-patch tiling: 32 rows x 16 columns per tile
    assert ((H + 31) // 32) * ((W + 15) // 16) == 6


def test_each_class_takes_its_own_path(fx, hip, monkeypatch, capfd):
    """What the solver itself reports (STEREO_HIP_QPBO_VERBOSE) on the three shuffled unions, tiled rounds asked for
    from the first round on: only arc lists of at most 4 get tiled rounds; up to 16 the weak pass runs on the gathered
    free subgraph, above that (or when asked) on the whole residual network."""
    import re
    from stereo_amd.rd import RdPlan
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("STEREO_HIP_QPBO_VERBOSE", "1")
    monkeypatch.setenv("STEREO_HIP_QPBO_SWITCH", "0")
    said = {}
    for name, weak_full in [("le4", False), ("mid", False), ("hub", False), ("mid", True)]:
        if weak_full:
            monkeypatch.setenv("STEREO_HIP_QPBO_WEAK_FULL", "1")
        u = fx.unions[name]
        plan = RdPlan(u.N, u.conn.T)
        capfd.readouterr()
        result = plan.solve(*u.args())
        plan.close()
        err = capfd.readouterr().err
        rx.check(u, result)
        assert result[3] > 0
        said[name, weak_full] = (int(re.search(r"tiled section: [0-9.]+ ms, (\d+) rounds", err).group(1)),
                                 "free variables" in err, "fetch the residual network" in err)
    assert said["le4", False][0] > 0 and said["le4", False][1:] == (True, False)
    assert said["mid", False] == (0, True, False)
    assert said["hub", False] == (0, False, True)
    assert said["mid", True] == (0, False, True)


@pytest.fixture(scope="module")
def glass(hip, oracle):
    """A 40 x 50 frustrated grid with integer costs (every sum exact); the restatement's strong stage says which
    labels are strong."""
    p = glass_problem(77, 40, 50, 3.0, True)
    args = (p["U0"], p["U1"], p["E00"], p["E01"], p["E10"], p["E11"])
    strong = oracle.rd(*args, p["conn"], stage=1)[0]
    assert 0 < np.count_nonzero(strong >= 0) < strong.size
    return p, args, strong


def _energy(p, x):
    i, j = p["conn"][:, 0], p["conn"][:, 1]
    t = np.where(x[i] == 1, np.where(x[j] == 1, p["E11"], p["E10"]), np.where(x[j] == 1, p["E01"], p["E00"]))
    return float(np.where(x == 1, p["U1"], p["U0"]).sum() + t.sum())


@pytest.mark.parametrize("path", PATHS + sorted(SWITCHES))
def test_glass_grid_is_invariant(path, glass, hip, oracle, monkeypatch):
    p, args, strong = glass
    S = strong >= 0
    ref = oracle.rd(*args, p["conn"])
    lb0 = ref[2]                               # integer costs: the restatement's bound is exact too
    for (lab, en, lb, nu), improve, plain in _solve(hip, monkeypatch, path, args, p["conn"], 40 * 50, (40, 50)):
        assert lb == lb0, path                                            # Y8 (and Y3 through the restatement)
        assert np.array_equal(lab[S], strong[S]), path                   # Y8
        assert en == _energy(p, (lab == 1).astype(np.int64)), path       # Y1
        assert en >= lb
        if improve:                                                       # Y2, Y7
            assert set(np.unique(lab)) <= {0.0, 1.0} and nu == plain[3]
            assert en <= _energy(p, (strong == 1).astype(np.int64))
        else:
            assert set(np.unique(lab)) <= {-1.0, 0.0, 1.0} and nu == np.count_nonzero(lab < 0)
            assert np.array_equal(lab < 0, ref[0] < 0), path                # Y9: the open set does not depend on the path
