"""Seeded generators of graphs that are NOT the reference's image grid (inputs only, no solver code).

Every generator returns ``(N, conn)`` with ``conn`` an (E, 2) int64 array of zero-based directed edges, the
layout of ``helpers.grid_conn``.  The grid-derived families keep the 4-neighbourhood's shape and change what a
caller may legitimately change -- which of a pair's two directed edges are listed, the edge order, the node
numbering, missing pixels, missing edges; the others are sparse graphs inside (or, on purpose, just outside) the
descriptor-driven kernels' range: at most 8 incident edges per node."""
import numpy as np

from helpers import grid_conn

# smallest graph found on which the chain schedule's loader protocol cannot terminate (forward sweep): two runs
# whose second nodes each wait for the other's first node
DEADLOCK8 = np.array([[0, 1], [0, 2], [1, 3], [2, 4], [1, 5], [5, 6], [3, 7], [5, 2], [3, 5], [6, 2]], np.int64)
DEADLOCK8_N = 8


# a long chain with a two-node side run: the chain is cut into speculative segments, the side run hangs on a chain node
# that becomes visible only when its segment commits and feeds a later node of the same segment -- the speculative
# schedule cannot terminate there (forward sweep, 10 segments), the plain chain schedule can
SPEC_DEADLOCK172_N = 172
SPEC_DEADLOCK172 = np.array([[i, i + 1] for i in range(169)] + [[170, 171], [171, 8], [10, 170]], np.int64)
SPEC_DEADLOCK302_N = 302
SPEC_DEADLOCK302 = np.array([[i, i + 1] for i in range(297)] + [[298, 299], [229, 299], [298, 231], [301, 300], [301, 227],
                                                                [300, 229]], np.int64)


def _arr(edges):
    return np.asarray(edges, np.int64).reshape(-1, 2)


def single_grid(H, W):
    """4-neighbourhood, node id = col * H + row like grid_conn, every pair listed ONCE (low id first)."""
    c = grid_conn(H, W)
    return H * W, c[c[:, 0] < c[:, 1]]


def shuffled_grid(H, W, seed):
    c = grid_conn(H, W)
    return H * W, c[np.random.default_rng(seed).permutation(len(c))]


def permuted_grid(H, W, seed):
    perm = np.random.default_rng(seed).permutation(H * W)
    return H * W, perm[grid_conn(H, W)]


def row_major_grid(H, W):
    ids = np.arange(H * W)
    new = (ids % H) * W + ids // H      # col * H + row  ->  row * W + col
    return H * W, new[grid_conn(H, W)]


def masked_grid(H, W, share, seed):
    """grid_conn with `share` of the pixels removed (their edges go, the survivors are renumbered in order); a
    survivor may lose all its neighbours and stay as an isolated node."""
    rng = np.random.default_rng(seed)
    keep = rng.random(H * W) >= share
    keep[rng.integers(0, H * W)] = True
    new = np.cumsum(keep) - 1
    c = grid_conn(H, W)
    c = c[keep[c[:, 0]] & keep[c[:, 1]]]
    return int(keep.sum()), new[c]


def dropped_edges_grid(H, W, share, seed):
    """grid_conn with `share` of the DIRECTED edges dropped: pairs with one edge, pairs with none."""
    c = grid_conn(H, W)
    return H * W, c[np.random.default_rng(seed).random(len(c)) >= share]


def two_grids(H1, W1, H2, W2):
    a, b = grid_conn(H1, W1), grid_conn(H2, W2)
    return H1 * W1 + H2 * W2, np.concatenate([a, b + H1 * W1])


def ring(N):
    i = np.arange(N)
    j = (i + 1) % N
    return N, np.concatenate([np.stack([i, j], 1), np.stack([j, i], 1)])


def chain(N):
    i = np.arange(N - 1)
    return N, np.stack([i, i + 1], 1)


def chain_with_side_runs(n, seed, gadgets=1):
    """A chain of n nodes (long enough: the one run the speculative schedule cuts into segments) and `gadgets` side
    runs of one or two extra nodes, each joined to two chain nodes a few steps apart, edges listed either way round."""
    rng = np.random.default_rng(seed)
    edges = [(i, i + 1) for i in range(n - 1)]
    N = n
    used = np.zeros(n, bool)
    for _ in range(gadgets):
        for _ in range(32):
            a = int(rng.integers(1, n - 10))
            b = a + int(rng.integers(1, 9))
            if not used[a] and not used[b]:
                break
        else:
            continue
        used[a] = used[b] = True
        path = [a] + list(range(N, N + int(rng.integers(1, 3)))) + [b]
        N = max(path[1:-1]) + 1
        for u, v in zip(path[:-1], path[1:]):
            edges.append((u, v) if rng.integers(0, 2) else (v, u))
    return N, _arr(edges)


def random_tree(N, seed, max_degree=4):
    rng = np.random.default_rng(seed)
    deg = np.zeros(N, int)
    edges = []
    for v in range(1, N):
        while True:
            u = int(rng.integers(0, v))
            if deg[u] < max_degree:
                break
        edges.append((u, v) if rng.integers(0, 2) else (v, u))
        deg[u] += 1; deg[v] += 1
    return N, _arr(edges)


def random_sparse(N, seed, extra=None, max_degree=4, isolated=0):
    """Connected graph on N nodes: a random spanning tree plus up to `extra` (default N // 2) random edges, every
    degree <= max_degree; `isolated` more nodes without any edge are appended."""
    rng = np.random.default_rng(seed)
    deg = np.zeros(N, int)
    edges = []
    for v in range(1, N):
        for _ in range(64):
            u = int(rng.integers(0, v))
            if deg[u] < max_degree - 1:
                break
        else:
            u = int(np.flatnonzero(deg[:v] < max_degree)[0])
        edges.append((u, v) if rng.integers(0, 2) else (v, u))
        deg[u] += 1; deg[v] += 1
    have = set(map(frozenset, edges))
    for _ in range(N // 2 if extra is None else extra):
        a, b = (int(x) for x in rng.integers(0, N, 2))
        if a != b and deg[a] < max_degree and deg[b] < max_degree and frozenset((a, b)) not in have:
            edges.append((a, b)); have.add(frozenset((a, b)))
            deg[a] += 1; deg[b] += 1
    return N + isolated, _arr(edges)


def random_multi(N, seed):
    """random_sparse with degree <= 3 in which a third of the pairs are listed twice (either direction) and a few
    three times: parallel edges, at most 8 incident edges per node."""
    rng = np.random.default_rng(seed)
    _, c = random_sparse(N, seed, max_degree=3)
    inc = np.bincount(c.ravel(), minlength=N)
    out = [tuple(e) for e in c]
    for a, b in c[rng.permutation(len(c))]:
        copies = int(rng.choice([0, 0, 1, 1, 2]))
        for _ in range(copies):
            if inc[a] < 8 and inc[b] < 8:
                out.append((a, b) if rng.integers(0, 2) else (b, a))
                inc[a] += 1; inc[b] += 1
    return N, _arr(out)[rng.permutation(len(out))]


def single_grid8(H, W):
    """8-neighbourhood, every pair once: interior degree 8, but more than four foreign dependencies per node --
    outside the descriptor-driven kernels' range."""
    rows, cols = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ids = cols * H + rows
    e = []
    for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
        r0, r1 = max(0, -dr), H - max(0, dr)
        c0, c1 = max(0, -dc), W - max(0, dc)
        a = ids[r0:r1, c0:c1]
        b = ids[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
        e.append(np.stack([a.ravel(), b.ravel()], 1))
    return H * W, np.concatenate(e)


def star_in_chain(degree, tail=20):
    """A chain of `tail` nodes whose node 0 is also the hub of a star of four leaves joined by double edges (in
    both directions): node 0 has exactly `degree` <= 9 incident edges (8: the descriptor kernels' limit; 9: one over)
    but never more than four distinct neighbours on either side of the visiting order."""
    edges = [(i, i + 1) for i in range(tail - 1)]
    edges += [(0, tail + k // 2) if k % 2 else (tail + k // 2, 0) for k in range(degree - 1)]
    return tail + 4, _arr(edges)


def fast_families(scale=1):
    """(name, N, conn) of every family that stays inside the descriptor kernels' range; `scale` 1: a few hundred
    nodes, 2: a few thousand."""
    H, W = (14, 19) if scale == 1 else (40, 50)
    n = 300 if scale == 1 else 2500
    fams = [
        ("single-grid", *single_grid(H, W)),
        ("shuffled-grid", *shuffled_grid(H, W, 1)),
        ("permuted-grid", *permuted_grid(H, W, 2)),
        ("row-major-grid", *row_major_grid(H, W)),
        ("masked-grid", *masked_grid(H, W, 0.15, 3)),
        ("dropped-edges-grid", *dropped_edges_grid(H, W, 0.25, 4)),
        ("two-grids", *two_grids(H, W // 2, H // 2, W)),
        ("ring", *ring(n)),
        ("chain", *chain(n)),
        ("random-tree", *random_tree(n, 5)),
        ("random-sparse", *random_sparse(n, 6)),
        ("random-sparse-isolated", *random_sparse(n, 7, isolated=n // 10)),
        ("random-multi", *random_multi(n, 8)),
        ("degree-8", *star_in_chain(8)),
    ]
    return fams


GRID_DERIVED = ("single-grid", "shuffled-grid", "permuted-grid", "row-major-grid", "masked-grid", "dropped-edges-grid",
                "two-grids")


def slow_families():
    """(name, N, conn) of the graphs the generic kernel must take."""
    return [("single-grid8", *single_grid8(9, 11)), ("degree-9", *star_in_chain(9))]
