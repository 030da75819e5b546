"""The exact roof-duality yardsticks (tests/rd_exact.py) against the CPU restatement oracle.rd, the fixture
against its own definitions, and the check against results that are wrong by the smallest possible amount."""
import numpy as np
import pytest

import rd_exact as rx


@pytest.fixture(scope="module")
def fx():
    return rx.fixture()


def _instances(fx, group):
    return fx.small_of(group[6:]) if group.startswith("small-") else [fx.unions[group]]


GROUPS = ["small-" + c for c in rx.CLASSES] + ["le4", "le4grid", "mid", "hub", "big"]


# ------------------------------------------------------------------ the fixture

@pytest.mark.parametrize("cls", rx.CLASSES)
def test_lp_values_rederived(cls, fx):
    """Every stored bound and every stored Y4 label, from the LP again (HiGHS)."""
    pytest.importorskip("scipy")
    import make_golden_rd_exact as mg
    for c in fx.components:
        if c.cls == cls:
            lb, strong = mg.lp_solve(c)
            assert lb == c.lb, c.name
            assert np.array_equal(strong, c.strong), c.name


def test_unmerged_lp_is_looser():
    """The merge is part of the definition: on a multi-edge component the LP with one table per EDGE lies
    strictly below the LP with one table per pair."""
    pytest.importorskip("scipy")
    import make_golden_rd_exact as mg
    looser = 0
    for c in rx.fixture().components:
        if c.family == "multi" and c.cls == "le4":
            raw = mg.lp_unmerged(c)
            assert raw <= c.lb + c.step() / 8, c.name
            looser += raw < c.lb - c.step() / 4
    assert looser > 0


def test_fixture_covers_what_it_claims(fx):
    for c in fx.components:
        d = c.max_degree()
        assert {"le4": d <= 4, "mid": 5 <= d <= 16, "hub": d >= 17}[c.cls], (c.name, d)
        assert c.N <= 20
        if c.family == "huge":
            assert 2 <= np.count_nonzero(c.U == rx.HUGE) <= 3 and c.s == 10
        if c.family == "sub":
            assert c.submodular()
        if c.family == "multi":
            e = {}
            for i, j in c.conn:
                e.setdefault((min(i, j), max(i, j)), []).append(i < j)
            assert any(len(v) > 1 and len(set(v)) == 2 for v in e.values())    # antiparallel
            assert any(v.count(True) > 1 or v.count(False) > 1 for v in e.values())   # parallel
    for cls in rx.CLASSES:
        small = fx.small_of(cls)
        assert len(small) == 36
        assert {i.parts[0][0].family for i in small} == set(rx.FAMILIES)
        assert any(i.parts[0][0].max_degree() == 8 for i in small) or cls != "mid"
    for name, u in fx.unions.items():
        assert u.N >= 3 * 512 - 64, name           # three tiles of 512 variables: several workgroups, grid barriers
        assert {c.family for c, _ in u.parts} == set(rx.FAMILIES), name
        if u.grid is None:    # shuffled ids: the components span the tiles
            spans = sum(len(set(ids // 512)) > 1 for _, ids in u.parts)
            assert spans >= 0.9 * len(u.parts), name
    assert fx.unions["big"].N > 6000
    H, W = fx.unions["le4grid"].grid
    u = fx.unions["le4grid"]
    assert H * W == u.N
    c, r = u.conn // H, u.conn % H
    assert np.all(np.abs(c[:, 0] - c[:, 1]) + np.abs(r[:, 0] - r[:, 1]) == 1)      # edges of the image grid only


def test_every_minimiser_carries_the_strong_labels(fx):
    """Y4 against enumeration, and Y6 on the fixture itself: LP bound <= min E, equal where submodular."""
    for c in fx.components:
        S = c.strong >= 0
        assert np.all(c.minimisers()[:, S] == c.strong[S]), c.name
        assert c.lb <= c.min_energy(), c.name
        if c.submodular():
            assert c.lb == c.min_energy(), c.name
        assert (c.lb * 2 ** (c.s + 1)).is_integer(), c.name


# ------------------------------------------------------------------ the restatement meets the yardsticks

@pytest.mark.parametrize("group", GROUPS)
def test_restatement_meets_the_yardsticks(group, fx, oracle):
    for inst in _instances(fx, group):
        plain = oracle.rd(*inst.args(), inst.conn)
        rx.check(inst, plain)
        improved = oracle.rd(*inst.args(), inst.conn, improve=True, seed=5)
        rx.check(inst, improved, improve=True, plain_nu=plain[3])
        if group.startswith("small-"):   # the strong stage alone gives exactly the Y4 labels
            assert np.array_equal(oracle.rd(*inst.args(), inst.conn, stage=1)[0], np.maximum(inst.strong, -1)), inst.name


def test_instance_mix(fx, oracle):
    """Instances that are decided outright, or not at all, teach little: in every union at least a fifth of
    the components are partially labelled and a tenth fully; at least a fifth of the small instances have both
    strongly persistent and strongly open variables."""
    for name, u in fx.unions.items():
        part, full, none = u.mix(oracle.rd(*u.args(), u.conn)[0])
        assert part + full + none == len(u.parts)
        assert 5 * part >= len(u.parts) and 10 * full >= len(u.parts), (name, part, full, none)
    both = sum(0 < np.count_nonzero(i.strong >= 0) < i.N for i in fx.small)
    assert 5 * both >= len(fx.small), both


# ------------------------------------------------------------------ the check rejects what is barely wrong

def _rule(inst, result, **kw):
    with pytest.raises(rx.Violation) as e:
        rx.check(inst, result, **kw)
    return e.value.rule


def _with_labels(inst, lab, lb, nu):
    return lab, inst.energy(lab == 1), lb, nu


@pytest.mark.parametrize("group", ["small-le4", "small-mid", "small-hub", "mid"])
def test_check_rejects_the_smallest_errors(group, fx, oracle):
    seen = {"Y4": 0, "Y5": 0, "Y7": 0, "Y9": 0}
    for inst in _instances(fx, group):
        lab, en, lb, nu = oracle.rd(*inst.args(), inst.conn)
        step = min(c.step() for c, _ in inst.parts)
        for d in (step / 2, -step / 2):
            assert _rule(inst, (lab, en, lb + d, nu)) == "Y3"     # the bound lives on the half step
        for d in (step, -step):
            assert _rule(inst, (lab, en + d, lb, nu)) == "Y1"
        for d in (1, -1):
            assert _rule(inst, (lab, en, lb, nu + d)) == "Y2"
        S = np.flatnonzero(inst.strong >= 0)
        if S.size:
            bad = lab.copy(); bad[S[len(S) // 2]] = 1 - bad[S[len(S) // 2]]
            assert _rule(inst, _with_labels(inst, bad, lb, nu)) == "Y4"
            seen["Y4"] += 1
        # a label on an open variable that no minimiser carries breaks the autarky
        for v in np.flatnonzero(lab < 0)[:4]:
            for a in (0, 1):
                bad = lab.copy(); bad[v] = a
                try:
                    rx.check(inst, _with_labels(inst, bad, lb, nu - 1))
                except rx.Violation as e:
                    assert e.rule == "Y5"
                    seen["Y5"] += 1
        # the weak labels withheld: the strong labels alone are an autarky too, but decidable variables stay open
        weak = (lab >= 0) & (inst.strong == -1)
        if weak.any():
            bad = lab.copy(); bad[weak] = -1
            assert _rule(inst, _with_labels(inst, bad, lb, nu + np.count_nonzero(weak))) == "Y9"
            seen["Y9"] += 1
        # Improve: worse than the strong labels alone
        imp = oracle.rd(*inst.args(), inst.conn, improve=True, seed=5)
        assert _rule(inst, (imp[0], imp[1], imp[2], nu + 1), improve=True, plain_nu=nu) == "Y2"
        base = (inst.strong == 1).astype(np.float64)
        rng = np.random.default_rng(len(inst.name))
        opened = np.flatnonzero(inst.strong < 0)
        for _ in range(8 if opened.size else 0):
            bad = base.copy(); bad[rng.choice(opened, max(1, opened.size // 3), replace=False)] = 1
            if inst.energy(bad == 1) > inst.energy(base == 1):
                assert _rule(inst, _with_labels(inst, bad, lb, nu), improve=True, plain_nu=nu) == "Y7"
                seen["Y7"] += 1
                break
    assert all(seen.values()), seen
