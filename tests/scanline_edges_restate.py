"""Scanline aggregation on per-edge positions restated once in NumPy (the definition: include/stereo_hip.h, DESIGN.md
6.11).  Imports nothing from ``stereo_amd/`` or ``oracle/``.

unary: K x N float64, label fastest, N = H * W, pixel id p = y + H * x.  conn: 2 x E zero based.  q, qprim: K x E.
alphas: E.  kernel 1: v(d) = d, 2: v(d) = d * d.  Edge e = (i1, i2) costs
c_e(x_i1, x_i2) = alphas_e * min(v(|qprim(x_i1, e) - q(x_i2, e)|), tol), the product last.  Every line below rounds once
per operation, in the order the definition writes them.
"""
import numpy as np

DIRECTIONS_4 = ((0, 1), (0, -1), (1, 0), (-1, 0))


def edge_table(conn, shape):
    """The 4 N int32 table: table[slot + 2 * (axis + 2 * p)], axis 0 the pair (p - 1, p) in a column, axis 1 the pair
    (p - H, p) in a row, slot 0 the edge oriented from the smaller pixel id to the larger, slot 1 the reverse, -1 where
    there is none.  ValueError, naming the edge, for an edge the grid does not have or has already."""
    H, W = shape
    N = H * W
    conn = np.asarray(conn).astype(np.int64).reshape(2, -1)
    table = np.full(4 * N, -1, np.int32)
    for e in range(conn.shape[1]):
        i1, i2 = int(conn[0, e]), int(conn[1, e])
        if i1 == i2:
            raise ValueError("edge %d is a self-loop" % e)
        if not (0 <= i1 < N and 0 <= i2 < N):
            raise ValueError("edge %d is out of range" % e)
        lo, hi = min(i1, i2), max(i1, i2)
        if hi - lo == 1 and hi % H != 0:            # the same column, rows y - 1 and y
            axis = 0
        elif hi - lo == H:                          # the same row, columns x - 1 and x
            axis = 1
        else:
            raise ValueError("edge %d does not join two 4-neighbours" % e)
        index = (0 if i1 < i2 else 1) + 2 * (axis + 2 * hi)
        if table[index] != -1:
            raise ValueError("edge %d: its slot is taken by edge %d" % (e, table[index]))
        table[index] = e
    return table


def edge_cost(q, qprim, alphas, kernel, tol, e):
    """(K, K): c_e at [x_i1, x_i2]"""
    if kernel not in (1, 2):
        raise ValueError("kernel must be 1 or 2")
    d = np.abs(qprim[:, e][:, None] - q[:, e][None, :])
    with np.errstate(over="ignore"):
        v = d if kernel == 1 else d * d
    return np.float64(alphas[e]) * np.minimum(v, np.float64(tol))


def step_table(table, shape, q, qprim, alphas, kernel, tol, p, pprev):
    """T[k, l] for pixel p with label k and its predecessor pprev with label l: the two slots' costs, each with its
    arguments in its own orientation, added; an absent slot is +0.0."""
    H, _ = shape
    K = q.shape[0]
    lo, hi = min(p, pprev), max(p, pprev)
    axis = 0 if hi - lo == 1 and hi % H != 0 else 1            # (H = 1: a row's neighbours are 1 apart too)
    assert hi - lo == (1 if axis == 0 else H)
    terms = []
    for slot in (0, 1):
        e = int(table[slot + 2 * (axis + 2 * hi)])
        if e < 0:
            terms.append(np.zeros((K, K)))
            continue
        c = edge_cost(q, qprim, alphas, kernel, tol, e)          # [x_i1, x_i2], i1 = lo for slot 0, hi for slot 1
        first = lo if slot == 0 else hi
        terms.append(c.T if first == pprev else c)                 # -> [x_p, x_pprev]
    return terms[0] + terms[1]


def direction_costs(unary, shape, table, q, qprim, alphas, kernel, tol, direction):
    """L_r, K x N."""
    H, W = shape
    dy, dx = direction
    if (dy, dx) not in DIRECTIONS_4:
        raise ValueError("a direction is one of (0, 1), (0, -1), (1, 0), (-1, 0): the model has no diagonal edges")
    U = np.asarray(unary, dtype=np.float64)
    K = U.shape[0]
    assert U.shape == (K, H * W)
    q, qprim = np.asarray(q, dtype=np.float64).reshape(K, -1), np.asarray(qprim, dtype=np.float64).reshape(K, -1)
    L = np.zeros((K, H * W))
    ys = range(H) if dy >= 0 else range(H - 1, -1, -1)      # predecessors first
    xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
    for x in xs:
        for y in ys:
            p = x * H + y
            yp, xp = y - dy, x - dx
            if 0 <= yp < H and 0 <= xp < W:
                pp = xp * H + yp
                T = step_table(table, shape, q, qprim, alphas, kernel, tol, p, pp)
                L[:, p] = U[:, p] + (L[:, pp][None, :] + T).min(axis=1)
            else:
                L[:, p] = U[:, p]
    return L


def aggregate(unary, shape, conn, q, qprim, alphas, kernel, tol, directions=DIRECTIONS_4):
    """-> (S K x N, labels N int32 one based, confidence H x W)"""
    H, W = shape
    directions = list(directions)
    if not 1 <= len(directions) <= 8:
        raise ValueError("1 .. 8 directions")
    table = edge_table(conn, shape)
    S = None
    for direction in directions:
        L = direction_costs(unary, shape, table, q, qprim, alphas, kernel, tol, direction)
        S = L if S is None else S + L
    K = S.shape[0]
    labels = (np.argmin(S, axis=0) + 1).astype(np.int32)               # argmin: the first minimum
    rel = S - S.min(axis=0)[None, :]
    conf = np.sort(rel, axis=0)[1] if K > 1 else np.full(H * W, np.inf)
    return S, labels, conf.reshape(W, H).T
