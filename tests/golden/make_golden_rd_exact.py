"""rd_exact.npz: enumerable roof-duality instances with their LP bounds and strong persistencies.

Needs SciPy (scipy.optimize.linprog, HiGHS); the tests that read the fixture do not.  Nothing here comes
from a QPBO library: the bound is the optimum of the LP relaxation over the local polytope of the merged
function, and a variable is strongly persistent when it takes one value on the whole optimal face.

    python tests/golden/make_golden_rd_exact.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rd_exact as rx  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------ the LP

def lp_terms(c, merge=True):
    """Merged pairs and unaries of a component as the LP sees them.  An out-of-range unary (rd_exact.HUGE) is
    replaced by M = 1 + |U0| + |U1| + sum |incident terms| (the other unary's magnitude included): the variable
    sits at its cheap value in every optimum for that M and any larger one, so the optimum is the same."""
    pairs, tab = c.merged() if merge else (c.conn, c.T)   # (not merged: one table per edge, for comparison only)
    U = c.U.copy()
    for v, k in zip(*np.nonzero(U == rx.HUGE)):
        inc = np.abs(tab[(pairs == v).any(1)]).sum()
        U[v, k] = np.ceil(1 + inc + abs(U[v, 1 - k]))
    return U, pairs, tab


def lp_system(c, merge=True):
    """min cost . z, A z = b, 0 <= z <= 1 with z = (x_1 .. x_N, mu_e(00), mu_e(01), mu_e(10), mu_e(11) ...)."""
    from scipy.sparse import coo_matrix
    U, pairs, tab = lp_terms(c, merge)
    N, P = c.N, len(pairs)
    cost = np.concatenate([U[:, 1] - U[:, 0], tab.ravel()])
    rows, cols, vals = [], [], []
    for e, (i, j) in enumerate(pairs):
        o = N + 4 * e
        rows += [3 * e] * 3 + [3 * e + 1] * 3 + [3 * e + 2] * 4
        cols += [o + 2, o + 3, i, o + 1, o + 3, j, o, o + 1, o + 2, o + 3]
        vals += [1, 1, -1, 1, 1, -1, 1, 1, 1, 1]
    A = coo_matrix((vals, (rows, cols)), shape=(3 * P, N + 4 * P)).tocsr()
    b = np.zeros(3 * P); b[2::3] = 1
    return cost, float(U[:, 0].sum()), A, b


def lp_unmerged(c):
    """The LP optimum with one table per edge: a weaker relaxation wherever two edges share a pair."""
    from scipy.optimize import linprog
    cost, const, A, b = lp_system(c, merge=False)
    r = linprog(cost, A_eq=A, b_eq=b, bounds=[(0, 1)] * cost.size, method="highs")
    assert r.status == 0, r.message
    return r.fun + const


def lp_solve(c):
    """(bound snapped to the half step, Y4 labels: 0 / 1 strong, rd_exact.HALF = 1/2 in every optimum, -1 else).  The raw optimum must lie within a quarter of the half step
    of a grid point.  Vertices of the local polytope are half-integral, so the extreme values of x_i over the
    optimal face are 0, 1/2 or 1: thresholds at 1/4 and 3/4 are safe."""
    from scipy.optimize import linprog
    N = c.N
    half = c.step() / 2
    if c.E == 0:
        d = c.U[:, 1] - c.U[:, 0]
        return float(np.minimum(c.U[:, 0], c.U[:, 1]).sum()), np.where(d > 0, 0, np.where(d < 0, 1, -1)).astype(np.int8)   # (a tie: free, never forced to 1/2)
    cost, const, A, b = lp_system(c)
    bounds = [(0, 1)] * cost.size
    r = linprog(cost, A_eq=A, b_eq=b, bounds=bounds, method="highs")
    assert r.status == 0, r.message
    raw = r.fun + const
    lb = round(raw / half) * half
    assert abs(raw - lb) < half / 4, (c.name, raw, lb)
    face = dict(A_ub=cost[None, :], b_ub=[lb - const + half / 64], A_eq=A, b_eq=b, bounds=bounds, method="highs")
    strong = np.full(N, -1, dtype=np.int8)
    for i in range(N):
        e = np.zeros(cost.size)
        if 0.25 < r.x[i] < 0.75:
            # a vertex of the optimal face has x_i = 1/2: not strong; is it 1/2 on the whole face?
            e[i] = 1
            lo, hi = linprog(e, **face), linprog(-e, **face)
            assert lo.status == 0 and hi.status == 0
            if lo.fun > 0.25 and -hi.fun < 0.75:
                strong[i] = rx.HALF
        elif r.x[i] <= 0.25:    # 0 is attained; can x_i leave it?
            e[i] = -1
            q = linprog(e, **face)
            assert q.status == 0, q.message
            if -q.fun < 0.25:
                strong[i] = 0
        else:
            e[i] = 1
            q = linprog(e, **face)
            assert q.status == 0, q.message
            if q.fun > 0.75:
                strong[i] = 1
    return float(lb), strong


# ------------------------------------------------------------------ the instances

FIELD = {"le4": 0.85, "mid8": 5.0, "mid16": 8.0, "hub": 3.0}
# families of a pool of components, in the proportions of one union
MIX = ["glass"] * 12 + ["mixed"] * 2 + ["sub"] * 2 + ["multi"] * 2 + ["huge"] * 2


def build_components(rng):
    comps = []

    def add(cls, family, conn, field):
        comps.append(rx.make_component(rng, "%s-%s-%d" % (cls, family, len(comps)), cls, family, conn, field))
    for k in range(60):      # at most 4 neighbours: ring plus chords, capped random graphs, two bridged rings
        N = int(rng.integers(12, 21))
        conn = (rx.ring_chords(N), rx.capped_graph(rng, N, 4), rx.two_rings(rng, N))[k % 3]
        add("le4", MIX[k % len(MIX)], conn, FIELD["le4"])
    for k in range(44):      # ... and small grid patches
        h, w = [(3, 4), (4, 4), (3, 5), (4, 5), (2, 8), (3, 6), (2, 5)][k % 7]
        add("le4", MIX[k % len(MIX)], rx.patch_graph(h, w), FIELD["le4"])
    for k in range(100):     # 5 .. 16 neighbours: capped at 8, capped at 16
        N = int(rng.integers(13, 18))
        cap = 8 if k % 2 else 16
        add("mid", MIX[k % len(MIX)], rx.capped_graph(rng, N, cap), FIELD["mid%d" % cap])
    for k in range(84):      # one or two hubs next to 17 or more others
        N = 18 if k % 6 else int(rng.integers(19, 21))
        add("hub", MIX[k % len(MIX)], rx.hub_graph(rng, N, 1 + k % 2), FIELD["hub"])
    return comps


def in_place_patches(rng, comps, H, W):
    """Grid patches left where they are inside an H x W image numbered col * H + row: bands of 3 or 4 rows cut
    into patches 3 to 5 columns wide, no edges between patches.  Appends the patches to comps."""
    bands = [3, 4, 4, 4, 4, 4, 4, 4, 3, 3, 3]     # (a band crosses row 32, where the image-patch tiling cuts)
    assert sum(bands) == H
    comp, ids, r0 = [], [], 0
    for h in bands:
        c0 = 0
        while c0 < W:
            rem = W - c0
            w = rem if rem <= 5 else int(rng.integers(3, 6))
            if rem - w in (1, 2):    # (only when 6 or 7 columns remain: leave 3)
                w = rem - 3
            c = rx.make_component(rng, "le4-inplace-%d" % len(comps), "le4", MIX[len(comps) % len(MIX)],
                                  rx.patch_graph(h, w), FIELD["le4"])
            comp.append(len(comps)); comps.append(c)
            cols, rows = np.divmod(np.arange(h * w), h)
            ids.append((c0 + cols) * H + r0 + rows)
            c0 += w
        r0 += h
    return comp, np.concatenate(ids)


def shuffled_union(rng, comps, members):
    """Disjoint union under shuffled variable ids and edge order: every component spans the tiles."""
    n = sum(comps[k].N for k in members)
    e = sum(comps[k].E for k in members)
    return dict(comp=members, ids=rng.permutation(n), edges=rng.permutation(e))


def build(seed=20260521):
    rng = np.random.default_rng(seed)
    comps = build_components(rng)
    by = {cls: [k for k, c in enumerate(comps) if c.cls == cls] for cls in rx.CLASSES}
    # the small instances: 36 per class, every family among them
    small = by["le4"][:20] + by["le4"][60:76] + by["mid"][:36] + by["hub"][:36]
    unions = {cls: shuffled_union(rng, comps, by[cls]) for cls in rx.CLASSES}
    # about 6,000 variables: the shuffled unions' components four times over, under new ids
    unions["big"] = shuffled_union(rng, comps, (by["le4"] * 4))
    H, W = 40, 40
    members, ids = in_place_patches(rng, comps, H, W)
    e = sum(comps[k].E for k in members)
    unions["le4grid"] = dict(comp=members, ids=ids, edges=rng.permutation(e), grid=(H, W))
    for c in comps:
        c.lb, c.strong = lp_solve(c)
    return comps, unions, small


if __name__ == "__main__":
    comps, unions, small = build()
    np.savez_compressed(os.path.join(HERE, "rd_exact.npz"), **rx.pack(comps, unions, small))
    print("%d components, unions %s" % (len(comps), {k: len(v["ids"]) for k, v in unions.items()}))
