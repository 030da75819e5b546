"""Exact, library-free yardsticks for roof duality (QPBO) -- NumPy only.

All costs of an instance lie on an exact grid, integers times 2**-s, so every sum below is exact in
fp64 and every comparison is `==`: the tolerance is zero by derivation.  For a result
``(lab, en, lb, nu)`` of a problem, `check` applies

  Y1  en  == energy of lab (unlabelled -> 0), evaluated from the caller's tables
  Y2  nu  == count(lab < 0); with Improve lab in {0, 1} and nu is the count of the run without it
  Y3  lb  == optimum of the LP relaxation over the local polytope of the MERGED function (one table per
             unordered pair: parallel and antiparallel edges summed, reversed ones transposed)
  Y4  a variable whose value is the same in every LP optimum carries that value
  Y5  autarky: writing the labelled part of lab into ANY assignment never raises the energy, and some
      global minimiser agrees with lab on the labelled part (by enumeration of all 2**N assignments)
  Y6  lb <= min E; on a submodular component everything is labelled and E(lab) == lb == min E
  Y7  Improve: E(improved) <= E(0 with the strong labels of Y4 written in); strong labels keep their value
  Y9  without Improve, the unlabelled variables are exactly those that are 1/2 in EVERY LP optimum.  (The LP
      optima are the convex hull of the half-integral solutions read off the minimum cuts of the doubled
      network; i and its mate lie on one side of every minimum cut iff they share a strongly connected
      component of the residual network, and those are the variables weak persistency leaves open.)

Roof duality decomposes over connected components, so a union of enumerable components (N <= 20 each)
under shuffled variable ids and edge order is checked component by component: that is how instances of
a few thousand variables -- several tiles, several workgroups, grid barriers -- get an exact yardstick.
The LP values (Y3, Y4) come from tests/golden/rd_exact.npz (make_golden_rd_exact.py: HiGHS, run where
SciPy is available); nothing here reads a QPBO library.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "rd_exact.npz")

HALF = -2            # in the Y4 labels: the variable is 1/2 in EVERY LP optimum (-1: open, but integral in some)
HUGE = 4e7           # an out-of-range plane's unary (dispmap_ncc.m:245)
CLASSES = ("le4", "mid", "hub")   # largest number of distinct neighbours: <= 4, 5 .. 16, >= 17
FAMILIES = ("glass", "mixed", "sub", "multi", "huge")


class Violation(AssertionError):
    def __init__(self, rule, msg):
        AssertionError.__init__(self, "%s: %s" % (rule, msg))
        self.rule = rule


# ------------------------------------------------------------------ components

class Component:
    """One connected, enumerable problem: N <= 20 variables, costs = integers * 2**-s."""

    def __init__(self, name, cls, family, s, U, T, conn, lb=None, strong=None):
        self.name, self.cls, self.family, self.s = name, cls, family, int(s)
        self.U = np.asarray(U, dtype=np.float64).reshape(-1, 2)          # N x 2: U0, U1
        self.T = np.asarray(T, dtype=np.float64).reshape(-1, 4)          # E x 4: E00, E01, E10, E11
        self.conn = np.asarray(conn, dtype=np.int64).reshape(-1, 2)
        self.N, self.E = self.U.shape[0], self.T.shape[0]
        assert self.N <= 20
        self.lb = lb                  # LP optimum (fixture)
        self.strong = strong          # Y4 labels (fixture): 0 / 1 the value in every LP optimum, HALF, -1 otherwise
        self._enum = None             # (min E, indices of the minimisers), filled by the first enumeration
        self._sub = None
        self._y5 = {}                 # labelled part -> None | message

    def step(self):
        return 2.0 ** -self.s

    def neighbours(self):
        nb = [set() for _ in range(self.N)]
        for i, j in self.conn:
            nb[i].add(int(j)); nb[j].add(int(i))
        return nb

    def max_degree(self):
        return max([len(s) for s in self.neighbours()] + [0])

    def merged(self):
        """One table per unordered pair i < j (what group_pairs does on the host)."""
        d = {}
        for (i, j), t in zip(self.conn, self.T):
            if i > j:
                i, j, t = j, i, t[[0, 2, 1, 3]]
            d[(int(i), int(j))] = d.get((int(i), int(j)), 0.0) + t
        keys = sorted(d)
        return np.array(keys, dtype=np.int64).reshape(-1, 2), np.array([d[k] for k in keys]).reshape(-1, 4)

    def submodular(self):
        if self._sub is None:
            _, t = self.merged()
            self._sub = bool(np.all(t[:, 0] + t[:, 3] <= t[:, 1] + t[:, 2]))
        return self._sub

    def energy(self, x):
        x = np.asarray(x, dtype=np.int64)
        i, j = self.conn[:, 0], self.conn[:, 1]
        return float(self.U[np.arange(self.N), x].sum() + self.T[np.arange(self.E), 2 * x[i] + x[j]].sum())

    # -- enumeration: the table of all 2**N energies, built one variable at a time (variables of high degree
    # first, so that a pair costs 2**(position of its later end) additions)
    def energies(self):
        pairs, tab = self.merged()
        deg = np.bincount(pairs.ravel(), minlength=self.N)
        order = np.argsort(-deg, kind="stable")
        pos = np.empty(self.N, dtype=np.int64); pos[order] = np.arange(self.N)
        back = [[] for _ in range(self.N)]          # per position k: (earlier position, 2 x 2 table [x_earlier][x_k])
        for (i, j), t in zip(pairs, tab):
            t = t.reshape(2, 2)
            a, b = pos[i], pos[j]
            if a < b:
                back[b].append((a, t))
            else:
                back[a].append((b, t.T))
        idx = np.arange(1 << max(self.N - 1, 0), dtype=np.int64)
        en = np.zeros(1)
        for k in range(self.N):
            v = order[k]
            lo = en + self.U[v, 0]
            hi = en + self.U[v, 1]
            for a, t in back[k]:
                bit = (idx[:1 << k] >> a) & 1
                lo += np.where(bit == 1, t[1, 0], t[0, 0])
                hi += np.where(bit == 1, t[1, 1], t[0, 1])
            en = np.concatenate([lo, hi])
        return en, pos

    def enumerated(self):
        """(min E, indices of all minimisers, bit position of every variable)."""
        if self._enum is None:
            en, pos = self.energies()
            mn = en.min()
            self._enum = (float(mn), np.flatnonzero(en == mn), pos)
        return self._enum

    def min_energy(self):
        return self.enumerated()[0]

    def autarky(self, lab):
        """Y5 for the labelled part of lab (length N, -1 = unlabelled): None, or what fails."""
        lab = np.asarray(lab).astype(np.int8)
        key = lab.tobytes()
        if key not in self._y5:
            self._y5[key] = self._autarky(lab)
        return self._y5[key]

    def _autarky(self, lab):
        L = np.flatnonzero(lab >= 0)
        if L.size == 0:
            return None
        en, pos = self.energies()
        mn = en.min()
        if self._enum is None:
            self._enum = (float(mn), np.flatnonzero(en == mn), pos)
        mask = int((1 << pos[L]).sum())
        val = int((lab[L].astype(np.int64) << pos[L]).sum())
        idx = np.arange(en.size, dtype=np.int64)
        over = (idx & ~mask) | val
        worse = np.flatnonzero(en[over] > en)
        if worse.size:
            k = worse[0]
            return "overwriting assignment %d raises the energy %r -> %r" % (k, en[k], en[over[k]])
        mins = self._enum[1]
        if not np.any((mins & mask) == val):
            return "no global minimiser agrees with the labelled part"
        return None

    def minimisers(self):
        """All global minimisers, one row each (N columns)."""
        _, mins, pos = self.enumerated()
        return ((mins[:, None] >> pos[None, :]) & 1).astype(np.int8)


# ------------------------------------------------------------------ instances

class Instance:
    """What a solver sees (U0, U1, E00 .. E11, conn) plus its components: `parts` lists, per component,
    (component, global ids of its variables in the component's own order)."""

    def __init__(self, name, cls, N, parts, edge_perm=None, grid=None):
        self.name, self.cls, self.N, self.parts, self.grid = name, cls, int(N), parts, grid
        U = np.zeros((self.N, 2))
        seen = np.zeros(self.N, dtype=bool)
        conn, T = [], []
        for c, ids in parts:
            assert not seen[ids].any()
            seen[ids] = True
            U[ids] = c.U
            conn.append(ids[c.conn]); T.append(c.T)
        assert seen.all()
        conn = np.concatenate(conn).reshape(-1, 2); T = np.concatenate(T).reshape(-1, 4)
        if edge_perm is not None:
            conn, T = conn[edge_perm], T[edge_perm]
        self.U0, self.U1 = U[:, 0].copy(), U[:, 1].copy()
        self.E00, self.E01, self.E10, self.E11 = (np.ascontiguousarray(T[:, k]) for k in range(4))
        self.conn = np.ascontiguousarray(conn)                     # E x 2, zero based
        self.lb = float(sum(c.lb for c, _ in parts)) if all(c.lb is not None for c, _ in parts) else None
        self.strong = np.full(self.N, -1, dtype=np.int8)
        for c, ids in parts:
            if c.strong is not None:
                self.strong[ids] = c.strong

    def args(self):
        return (self.U0, self.U1, self.E00, self.E01, self.E10, self.E11)

    def energy(self, x):
        x = np.asarray(x, dtype=np.int64)
        i, j = self.conn[:, 0], self.conn[:, 1]
        t = np.where(x[i] == 1, np.where(x[j] == 1, self.E11, self.E10), np.where(x[j] == 1, self.E01, self.E00))
        return float(np.where(x == 1, self.U1, self.U0).sum() + t.sum())

    def max_degree(self):
        return max(c.max_degree() for c, _ in self.parts)

    def mix(self, lab):
        """(partially, fully, not at all) labelled components."""
        part = full = none = 0
        for c, ids in self.parts:
            k = int((np.asarray(lab)[ids] < 0).sum())
            part += 0 < k < c.N; full += k == 0; none += k == c.N
        return part, full, none


def single(c):
    return Instance(c.name, c.cls, c.N, [(c, np.arange(c.N))])


# ------------------------------------------------------------------ the check

def check(inst, result, improve=False, plain_nu=None):
    """Y1 .. Y7 and Y9 for one result (lab, en, lb, nu); raises Violation naming the first rule that fails.
    improve: the result of a run with Improve; plain_nu: num_unlabelled of the same problem without it."""
    lab, en, lb, nu = result
    lab = np.asarray(lab)
    if lab.shape != (inst.N,) or not np.all(np.isin(lab, (0, 1) if improve else (-1, 0, 1))):
        raise Violation("Y2", "labels outside the allowed set")
    x = (lab == 1).astype(np.int64)
    # Y3
    if lb != inst.lb:
        raise Violation("Y3", "bound %r, LP optimum %r (difference %r)" % (lb, inst.lb, lb - inst.lb))
    # Y4
    S = inst.strong >= 0
    if not np.array_equal(lab[S], inst.strong[S]):
        bad = np.flatnonzero(S & (lab != inst.strong))
        raise Violation("Y4", "%d strongly persistent variables mislabelled, first %d: %d for %d"
                        % (bad.size, bad[0], lab[bad[0]], inst.strong[bad[0]]))
    # Y1
    e = inst.energy(x)
    if en != e:
        raise Violation("Y1", "energy %r, labelling evaluates to %r (difference %r)" % (en, e, en - e))
    # Y2
    if improve:
        if plain_nu is not None and nu != plain_nu:
            raise Violation("Y2", "num_unlabelled %r with Improve, %r without" % (nu, plain_nu))
    elif nu != np.count_nonzero(lab < 0):
        raise Violation("Y2", "num_unlabelled %r, %d labels are negative" % (nu, np.count_nonzero(lab < 0)))
    # Y6, first half
    mn = float(sum(c.min_energy() for c, _ in inst.parts))
    if not lb <= mn:
        raise Violation("Y6", "bound %r above the minimum energy %r" % (lb, mn))
    for c, ids in inst.parts:
        l = lab[ids]
        if c.submodular():
            if np.any(l < 0):
                raise Violation("Y6", "%s is submodular and has unlabelled variables" % c.name)
            if not (c.energy(l == 1) == c.min_energy() == c.lb):
                raise Violation("Y6", "%s is submodular: E(lab) %r, min E %r, bound %r"
                                % (c.name, c.energy(l == 1), c.min_energy(), c.lb))
        if improve:
            base = c.energy(c.strong == 1)
            if c.energy(l == 1) > base:
                raise Violation("Y7", "%s: improved energy %r above %r of the strong labels alone"
                                % (c.name, c.energy(l == 1), base))
        else:
            msg = c.autarky(l)
            if msg:
                raise Violation("Y5", "%s: %s" % (c.name, msg))
    # Y9
    if not improve and not np.array_equal(lab < 0, inst.strong == HALF):
        bad = np.flatnonzero((lab < 0) != (inst.strong == HALF))
        raise Violation("Y9", "%d variables: unlabelled but integral in some LP optimum, or labelled but 1/2 in all "
                        "(first %d: label %d)" % (bad.size, bad[0], lab[bad[0]]))


# ------------------------------------------------------------------ builders (used by the fixture's generator)

def _on_grid(rng, base, s):
    """Integers `base` moved onto the 2**-s grid: base + jitter / 2**s."""
    base = np.asarray(base, dtype=np.float64)
    if s == 0:
        return base
    q = 1 << s
    return (base * q + rng.integers(-(q // 3), q // 3 + 1, base.shape)) / q


def capped_graph(rng, N, d):
    """Ring plus random chords, no variable with more than d distinct neighbours."""
    nb = [set() for _ in range(N)]

    def add(i, j):
        if i != j and j not in nb[i] and len(nb[i]) < d and len(nb[j]) < d:
            nb[i].add(j); nb[j].add(i)
    for i in range(N):
        add(i, (i + 1) % N)
    for _ in range(40 * N):
        add(int(rng.integers(N)), int(rng.integers(N)))
    return np.array([(i, j) for i in range(N) for j in sorted(nb[i]) if i < j], dtype=np.int64)


def ring_chords(N):
    return np.array([(i, (i + 1) % N) for i in range(N)] + [(i, i + N // 2) for i in range(N // 2)], dtype=np.int64)


def two_rings(rng, N):
    """Two rings with chords, joined by one or two bridges: at most 4 neighbours."""
    n1 = N // 2
    a, b = capped_graph(rng, n1, 3), capped_graph(rng, N - n1, 3) + n1
    bridges = [(0, n1)] + ([(n1 // 2, n1 + (N - n1) // 2)] if rng.random() < 0.5 else [])
    return np.concatenate([a, b, np.array(bridges, dtype=np.int64)])


def patch_graph(h, w):
    """An h x w patch of the 4-connected grid, variable = col * h + row."""
    e = [(c * h + r, c * h + r + 1) for c in range(w) for r in range(h - 1)]
    e += [(c * h + r, (c + 1) * h + r) for c in range(w - 1) for r in range(h)]
    return np.array(e, dtype=np.int64)


def hub_graph(rng, N, hubs):
    """`hubs` variables next to all others; the rest on a ring with a few chords (at most 3 neighbours there:
    dense graphs stay wholly unlabelled and teach little)."""
    e = [(a, v) for a in range(hubs) for v in range(a + 1, N)]
    e += [(int(i) + hubs, int(j) + hubs) for i, j in capped_graph(rng, N - hubs, 3)]
    return np.array(e, dtype=np.int64)


def make_component(rng, name, cls, family, conn, field):
    """Costs of one family on a given graph.  field: width of the random field of the frustrated families."""
    N = int(conn.max()) + 1
    flip = rng.random(len(conn)) < 0.5
    conn = conn.copy(); conn[flip] = conn[flip][:, ::-1]
    s = 10 if family == "huge" else int(rng.choice([0, 0, 1, 3, 10]))
    if family == "multi":   # parallel, antiparallel and duplicated edges: the neighbour sets stay what they were
        k = max(2, len(conn) // 3)
        par, anti, dup = (conn[rng.choice(len(conn), k, replace=False)] for _ in range(3))
        conn = np.concatenate([conn, par, anti[:, ::-1], dup])
    E = len(conn)
    if family == "sub":
        T = rng.integers(0, 5, (E, 4)).astype(np.float64)
        T[:, 1:3] += 5
        U = rng.integers(0, 21, (N, 2)).astype(np.float64)
    elif family in ("glass", "huge") or (family == "multi" and rng.random() < 0.5):
        J = np.round(rng.normal(size=E) * 4)
        T = np.stack([np.zeros(E), J, J, np.zeros(E)], 1)
        # (a strong field on one half of the variables, a weak one on the other: partly labelled outcomes)
        w = np.where(np.arange(N) < rng.integers(N // 3, N - N // 3 + 1), 2.5, 0.4)
        U = np.stack([np.zeros(N), np.round(rng.normal(size=N) * field * 2 * w)], 1)
    else:
        T = np.round(rng.uniform(-6, 6, (E, 4)))
        U = np.round(rng.uniform(-4, 4, (N, 2)) * max(1.0, field / 2))
    T, U = _on_grid(rng, T, s), _on_grid(rng, U, s)
    if family == "multi":
        T[E - k:] = T[conn_index(conn[:E - k], conn[E - k:])]   # the duplicates carry their original's table
    if family == "huge":
        for n_, v in enumerate(rng.choice(N, int(rng.integers(2, 4)), replace=False)):
            U[v, n_ % 2] = HUGE
    return Component(name, cls, family, s, U, T, conn)


def conn_index(conn, rows):
    """Index in conn of the first edge equal to each of rows."""
    return np.array([np.flatnonzero((conn == r).all(1))[0] for r in rows], dtype=np.int64)


# ------------------------------------------------------------------ the fixture

_STEP_BITS = 11   # every stored number is an integer multiple of 2**-11 (s <= 10, bounds on the half step)


def pack(components, unions, small):
    """Everything the tests need, as arrays: the instances themselves, each component's bound and Y4 labels."""
    q = float(1 << _STEP_BITS)

    def ints(a):
        v = np.asarray(a, dtype=np.float64) * q
        assert np.all(v == np.round(v)) and np.all(np.abs(v) < 2.0 ** 52)
        return v.astype(np.int64)
    out = {
        "comp_name": np.array([c.name for c in components]),
        "comp_cls": np.array([c.cls for c in components]),
        "comp_family": np.array([c.family for c in components]),
        "comp_s": np.array([c.s for c in components], dtype=np.int8),
        "comp_N": np.array([c.N for c in components], dtype=np.int16),
        "comp_E": np.array([c.E for c in components], dtype=np.int32),
        "comp_U": ints(np.concatenate([c.U for c in components])),
        "comp_T": ints(np.concatenate([c.T for c in components])),
        "comp_conn": np.concatenate([c.conn for c in components]).astype(np.int8),
        "comp_lb": ints([c.lb for c in components]),
        "comp_strong": np.concatenate([c.strong for c in components]).astype(np.int8),
        "small": np.asarray(small, dtype=np.int32),
        "union_names": np.array(sorted(unions)),
    }
    for name, u in unions.items():
        out["union_%s_comp" % name] = np.asarray(u["comp"], dtype=np.int32)
        out["union_%s_ids" % name] = np.asarray(u["ids"], dtype=np.uint16)
        out["union_%s_edges" % name] = np.asarray(u["edges"], dtype=np.uint16)
        out["union_%s_grid" % name] = np.asarray(u.get("grid") or (0, 0), dtype=np.int32)
    return out


class Fixture:
    def __init__(self, path=FIXTURE):
        g = np.load(path)
        q = float(1 << _STEP_BITS)
        N, E = g["comp_N"].astype(np.int64), g["comp_E"].astype(np.int64)
        no, eo = np.concatenate([[0], np.cumsum(N)]), np.concatenate([[0], np.cumsum(E)])
        U, T, conn, strong = g["comp_U"] / q, g["comp_T"] / q, g["comp_conn"], g["comp_strong"]
        lb = g["comp_lb"] / q
        self.components = [
            Component(str(g["comp_name"][k]), str(g["comp_cls"][k]), str(g["comp_family"][k]), g["comp_s"][k],
                      U[no[k]:no[k + 1]], T[eo[k]:eo[k + 1]], conn[eo[k]:eo[k + 1]], float(lb[k]),
                      strong[no[k]:no[k + 1]].copy())
            for k in range(len(N))]
        self.small = [single(self.components[k]) for k in g["small"]]
        self.unions = {}
        for name in g["union_names"]:
            name = str(name)
            comp = g["union_%s_comp" % name]
            ids = g["union_%s_ids" % name].astype(np.int64)
            parts, o = [], 0
            for k in comp:
                c = self.components[k]
                parts.append((c, ids[o:o + c.N])); o += c.N
            grid = tuple(int(v) for v in g["union_%s_grid" % name])
            cls = parts[0][0].cls
            self.unions[name] = Instance(name, cls, ids.size, parts, g["union_%s_edges" % name].astype(np.int64),
                                         grid if grid[0] > 0 else None)

    def small_of(self, cls):
        return [i for i in self.small if i.cls == cls]


_fixture = None


def fixture():
    """The committed instances, loaded once per process (the enumerations are cached on the components)."""
    global _fixture
    if _fixture is None:
        _fixture = Fixture()
    return _fixture
