"""First-principles yardsticks for TRW-S that do not go through the oracle (inputs and exact answers, no solver code).

Nothing here imports ``oracle/`` or ``stereo_amd/`` and nothing restates the solver.  The checks depend only on the
energy model that the C ABI documents (include/stereo_hip.h): for a labelling x, with connectivity row e = (a, b),

    E(x) = sum_i U[i, x_i] + sum_e alpha_e * min(v(|qprim_e[x_a] - q_e[x_b]|), lambda),   v(d) = d (kernel 1), d^2 (kernel 2)

and on two facts about TRW-S that follow from that definition alone:

* on a tree every gamma is 1 and one iteration is exact min-sum dynamic programming: energy == lower bound == OPT, and
  the node beliefs are the true min-marginals minus OPT (chain_dp gives both);
* on any graph the bound is a lower bound of every labelling's energy (so LB <= OPT <= energy), it never decreases from
  one iteration to the next, and the first one is at least sum_i min_k U[i, k] (optimum_exhaustive gives OPT on grids
  small enough to enumerate).

Why the chain checks and the energy identity are bitwise.  dyadic_problem draws every number on a dyadic grid: unaries
and per-edge positions are multiples of 2^-6 (bits = 6; FINE_BITS below is the one exception and has its own
argument), shared positions and alphas multiples of 2^-2.  A difference of two
positions is a multiple of 2^-6, its square of 2^-12, alpha times either of 2^-14; lambda is a dyadic number too or so
large (1e9) that it never cuts.  With the K <= 1024 of this suite every such term is below 2^22.  So every energy, every
message of an exact dynamic programme and every partial sum of either is a sum of at most N + E multiples of 2^-14 that
are below 2^22: below 2^35 for the graphs here, 49 significant bits at the most, and fp64 holds it without rounding in
whatever order it is added up.  Two different such values differ by at least 2^-14 ~ 6e-5.  On loopy graphs gamma can
be 1/3, the messages are rounded, and the bound checks carry SLACK; the reported energy is still the exact energy of a
labelling and is compared without any.
"""
from fractions import Fraction

import numpy as np

# Worst relative violation, over max(1, |OPT|), of LB_t <= OPT and of LB_{t+1} >= LB_t that the CPU oracle itself
# shows on the enumerated grids below (both message routines, 30 iterations): rounding of the gamma = 1/3 messages.
# Measured: excess 2.6e-16, dip 3.8e-16 (test_first_principles_cpu.py measures again and holds the oracle below twice this).
MEASURED_VIOLATION = 3.8e-16
SLACK = 1000 * MEASURED_VIOLATION   # 3.8e-13: eight orders of magnitude below the 2^-14 that separates two dyadic energies

LAMBDAS = (0.5, 2.0, 6.0, 64.0, 1e9)
ALPHAS = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0)


def grid_edges(H, W):
    """(E, 2) zero-based 4-neighbourhood of an H x W grid, node id = col * H + row (tests/helpers.grid_conn's
    convention): vertical edges first, then horizontal ones; dyadic_problem permutes and flips them."""
    ids = np.arange(H * W).reshape(W, H).T          # ids[row, col]
    vert = np.stack([ids[:-1, :].ravel(), ids[1:, :].ravel()], 1)
    horz = np.stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()], 1)
    return np.concatenate([vert, horz]).astype(np.int64)


def _dyadic(rng, shape, top, bits):
    return rng.integers(0, int(top) << bits, size=shape).astype(np.float64) / float(1 << bits)


def dyadic_problem(rng, H, W, K, shared, umax=4, bits=6):
    """One problem on the H x W grid with every number on a dyadic grid (module docstring).  Returns dict(unary (N, K),
    conn (E, 2) zero based, q (E, K), qprim (E, K), alphas (E,), positions (K,) or None, lam).  The edge order is a
    random permutation and about half of the edges have their endpoints swapped.  shared: one strictly ascending
    positions vector stands in every row of q and qprim (and is returned as positions)."""
    N = H * W
    conn = grid_edges(H, W)
    E = conn.shape[0]
    conn = conn[rng.permutation(E)]
    flip = rng.random(E) < 0.5
    conn[flip] = conn[flip][:, ::-1]
    unary = _dyadic(rng, (N, K), umax, bits)
    if shared:
        steps = np.sort(rng.choice(K + K // 2 + 2, size=K, replace=False))
        positions = steps.astype(np.float64) * 0.25
        q = np.tile(positions, (E, 1))
        qprim = q.copy()
    else:
        positions = None
        q = _dyadic(rng, (E, K), 8, bits)
        qprim = _dyadic(rng, (E, K), 8, bits)
    alphas = rng.choice(ALPHAS, size=E, p=(0.1, 0.1, 0.2, 0.3, 0.2, 0.1))
    lam = float(rng.choice(LAMBDAS))
    return dict(unary=unary, conn=conn, q=q, qprim=qprim, alphas=alphas, positions=positions, lam=lam, H=H, W=W)


def _v(kernel):
    if kernel not in (1, 2):
        raise ValueError("kernel must be 1 or 2")
    return (lambda d: d) if kernel == 1 else (lambda d: d * d)


_SHIFT = 80


def _scaled_ints(a):
    """the floats of `a` times 2^80 as Python ints, or None if one of them is no multiple of 2^-80 (scaling a float by a
    power of two is exact, and so is int() of a float that holds an integer)"""
    b = np.asarray(a, dtype=np.float64) * 2.0 ** _SHIFT
    if not (np.isfinite(b).all() and np.array_equal(b, np.rint(b))):
        return None
    return [int(v) for v in b]


def energy_exact_by_terms(p, kernel, lam, x):
    """The energy of the labelling x as a fractions.Fraction, one Fraction per number, term by term from the model in
    the module docstring: the definition (about 10 microseconds per term)."""
    v = _v(kernel)
    lam = Fraction(float(lam))
    x = [int(k) for k in x]
    total = Fraction(0)
    for i, k in enumerate(x):
        total += Fraction(float(p["unary"][i, k]))
    for e, (a, b) in enumerate(p["conn"]):
        d = abs(Fraction(float(p["qprim"][e, x[int(a)]])) - Fraction(float(p["q"][e, x[int(b)]])))
        total += Fraction(float(p["alphas"][e])) * min(v(d), lam)
    return total


def energy_exact(p, kernel, lam, x):
    """The energy of the labelling x (zero based, one label per node) as a fractions.Fraction: exact rational
    arithmetic, no rounding anywhere.  Where every number is a multiple of 2^-80 (all of dyadic_problem's are) the sum
    is formed in Python integers over one power-of-two denominator -- the same terms as energy_exact_by_terms, which
    test_first_principles_cpu.py holds it to -- so that a grid of 10^5 nodes costs a fraction of a second."""
    _v(kernel)
    x = np.asarray(x, dtype=np.int64)
    E = np.arange(len(p["conn"]))
    parts = [_scaled_ints(a) for a in (p["unary"][np.arange(len(x)), x], p["qprim"][E, x[p["conn"][:, 0]]],
                                       p["q"][E, x[p["conn"][:, 1]]], p["alphas"], [lam])]
    if any(a is None for a in parts):
        return energy_exact_by_terms(p, kernel, lam, x)
    u, qa, qb, alphas, (lam_i,) = parts
    one = 1 << _SHIFT
    if kernel == 1:        # alpha * min(d, lam): denominator 2^160
        pair = sum(al * min(abs(s - t), lam_i) for al, s, t in zip(alphas, qa, qb))
        return Fraction(sum(u) * one + pair, one * one)
    pair = sum(al * min((s - t) * (s - t), lam_i * one) for al, s, t in zip(alphas, qa, qb))    # d^2: 2^160, with alpha 2^240
    return Fraction(sum(u) * one * one + pair, one * one * one)


def edge_table(p, kernel, lam, e):
    """(K, K) float64: the cost of edge e = (a, b) at [x_a, x_b]; exact on dyadic inputs."""
    d = np.abs(p["qprim"][e][:, None] - p["q"][e][None, :])
    return p["alphas"][e] * np.minimum(_v(kernel)(d), lam)


def optimum_exhaustive(p, kernel, lam):
    """(OPT, a minimising labelling) over all K^N labellings, K^N <= 4^9.  Vectorised float64: exact on dyadic
    inputs, in any order of summation."""
    N, K = p["unary"].shape
    if K ** N > 4 ** 9:
        raise ValueError("too many labellings to enumerate")
    X = np.stack(np.unravel_index(np.arange(K ** N), (K,) * N), 1)      # (K^N, N)
    en = np.zeros(K ** N)
    for i in range(N):
        en += p["unary"][i, X[:, i]]
    for e, (a, b) in enumerate(p["conn"]):
        en += edge_table(p, kernel, lam, e)[X[:, a], X[:, b]]
    best = int(np.argmin(en))
    return float(en[best]), X[best].copy()


def path_order(N, conn):
    """The nodes of a graph whose edges form one path over all N nodes, from the end with the smaller id, and for every
    step the edge row it uses."""
    if len(conn) != N - 1:
        raise ValueError("not a path: %d edges on %d nodes" % (len(conn), N))
    adj = [[] for _ in range(N)]
    for e, (a, b) in enumerate(conn):
        adj[int(a)].append((int(b), e))
        adj[int(b)].append((int(a), e))
    ends = [i for i in range(N) if len(adj[i]) == 1]
    if N == 1:
        return [0], []
    if len(ends) != 2 or any(len(x) > 2 for x in adj):
        raise ValueError("not a path")
    nodes, edges, prev = [ends[0]], [], -1
    while len(nodes) < N:
        step = [(j, e) for j, e in adj[nodes[-1]] if j != prev]
        if len(step) != 1:
            raise ValueError("not a path")
        prev = nodes[-1]
        nodes.append(step[0][0])
        edges.append(step[0][1])
    return nodes, edges


def chain_dp(p, kernel, lam):
    """Plain O(N K^2) min-sum dynamic programming on a path, whatever the order and orientation of its edge rows.
    Returns (OPT, MM): MM[i, k] = the smallest energy of a labelling with x_i = k (the true min-marginals, (N, K));
    OPT = min_k MM[i, k] at every node.  Exact on dyadic inputs."""
    N, K = p["unary"].shape
    nodes, edges = path_order(N, p["conn"])
    tables = []
    for s, e in enumerate(edges):               # tables[s][x_u, x_v] for the step nodes[s] -> nodes[s + 1]
        t = edge_table(p, kernel, lam, e)
        tables.append(t if int(p["conn"][e][0]) == nodes[s] else t.T)
    F = np.zeros((N, K))                        # F[s]: best cost of everything up to and including nodes[s]
    F[0] = p["unary"][nodes[0]]
    for s in range(1, N):
        F[s] = p["unary"][nodes[s]] + (F[s - 1][:, None] + tables[s - 1]).min(axis=0)
    B = np.zeros((N, K))                        # B[s]: best cost of everything behind nodes[s]
    for s in range(N - 2, -1, -1):
        B[s] = (tables[s] + (p["unary"][nodes[s + 1]] + B[s + 1])[None, :]).min(axis=1)
    MM = np.zeros((N, K))
    MM[nodes] = F + B
    return float(F[N - 1].min()), MM


def sum_min_unary(p):
    return float(p["unary"].min(axis=1).sum())


def check_run(p, kernel, lam, per_iteration_results, opt, slack, tight=True):
    """The properties of one run that follow from the energy alone.  per_iteration_results: one (labels, energy, lb)
    per iteration 1, 2, ... -- labels zero based, or None where the solver does not show them.  opt: the optimum, or
    None where nobody knows it (every reported energy is then the upper bound).  slack is relative to max(1, |opt|)
    and applies to the bound checks only; tight: the last bound must have reached OPT (1 - 1e-9)."""
    _v(kernel)      # (refuses a kernel the model does not have before anything is compared)
    energies = [float(r[1]) for r in per_iteration_results]
    bounds = [float(r[2]) for r in per_iteration_results]
    assert energies, "no iterations"
    scale = max(1.0, abs(opt if opt is not None else min(energies)))
    tol = slack * scale
    for t, (labels, en, lb) in enumerate(per_iteration_results, start=1):
        if labels is not None:
            exact = energy_exact(p, kernel, lam, labels)
            assert Fraction(float(en)) == exact, "iteration %d: energy %r, its labelling costs %r" % (t, en, float(exact))
        if opt is not None:
            assert en >= opt, "iteration %d: energy %r below the optimum %r" % (t, en, opt)
            assert lb <= opt + tol, "iteration %d: bound %r above the optimum %r" % (t, lb, opt)
        for s, other in enumerate(energies, start=1):
            assert lb <= other + tol, "bound %r of iteration %d above the energy %r of iteration %d" % (lb, t, other, s)
        if t > 1:
            assert lb >= bounds[t - 2] - tol, "iteration %d: bound fell from %r to %r" % (t, bounds[t - 2], lb)
    assert bounds[0] >= sum_min_unary(p) - tol, "first bound %r below the sum of the unary minima %r" % (bounds[0], sum_min_unary(p))
    if opt is not None and tight:
        assert bounds[-1] >= opt - 1e-9 * abs(opt), "bound %r has not reached the optimum %r" % (bounds[-1], opt)


def violations(per_iteration_results, opt):
    """(worst excess of a bound over opt, worst dip of the bound), both relative to max(1, |opt|); 0 where none."""
    bounds = [float(r[2]) for r in per_iteration_results]
    scale = max(1.0, abs(opt))
    over = max([0.0] + [(lb - opt) / scale for lb in bounds])
    dip = max([0.0] + [(a - b) / scale for a, b in zip(bounds, bounds[1:])])
    return over, dip


# ---- the instances, shared by test_first_principles_cpu.py (the oracle) and test_first_principles_gpu.py (the device) --

CHAIN_K = (2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024)     # the edges of the five kernel families
# A plan is given N and the connectivity, never H and W: to a plain TrwsPlan 1 x 9 and 9 x 1 are the same path over nodes
# 0 .. 8 (another seed, that is all), walked end to end as ONE run per direction.  The two orientations differ only
# where H and W are handed over: row strips and the gateway.
CHAIN_SHAPES = ((1, 9), (9, 1))
LONG_CHAINS = ((1, 300, 8), (300, 1, 8), (1100, 1, 4))             # one long serial run: hundreds of visits by one workgroup
# Grids whose rows are walked in pieces (sub-row runs), which no chain can be -- a chain is one run:
# (H, W, K, row chunk, resident workgroups).  The small one under STEREO_HIP_TRWS_ROW_CHUNK=8 and STEREO_HIP_TRWS_BLOCKS=3:
# 9 rows become 53 pieces of at most 8 positions in either direction, dispensed to 3 workgroups.  The tall one as a plan
# comes by default: 299 rows are more than the 256 compute units keep resident, so the backward sweep walks them in
# pieces of 112 and the ticket dispenser hands out more runs than there are workgroups.
PIECES_SMALL = (10, 40, 8, 8, 3)
PIECES_TALL = (300, 300, 4, 112, 256)
FEATURE_CHAINS = ((24, 1, 16), (24, 1, 96))
# the other two members of the batch around each feature chain: other lengths and label counts, the same kernel family
BATCH_CHAINS = {16: ((1, 9, 5), (40, 1, 33)), 96: ((1, 9, 70), (13, 1, 128))}
GRID_SHAPES = ((3, 3, 3), (2, 4, 3), (2, 3, 4), (3, 3, 2), (3, 4, 2), (2, 5, 3))
# (H, W, K, kernel, shared): K <= 64, two labels per lane, wide, large -- with exact messages (instance() below)
MIDSIZE = ((24, 20, 16, 1, False), (24, 20, 100, 2, False), (24, 20, 200, 2, True), (24, 20, 600, 1, True))

_problems = {}


def problem(H, W, K, shared, seed=0, bits=6):
    """The one dyadic problem of this shape, kind of positions, seed and grid; built once, never changed."""
    key = (H, W, K, bool(shared), seed, bits)
    if key not in _problems:
        p = dyadic_problem(np.random.default_rng([H, W, K, int(shared), seed]), H, W, K, shared, bits=bits)
        for a in p.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _problems[key] = p
    return _problems[key]


def expected_path(K, shared, minplus, kernel):
    """The kernel family (TrwsPlan.path()) that DESIGN.md 4.8 gives a whole problem on a grid graph, or 0 where no
    family takes it (K > 512 with positions per edge)."""
    if K > 512:
        return 5 if shared else 0
    if K <= 64:
        return 1 if minplus else 2
    if K <= 256 and shared and (kernel == 1 or not minplus):
        return 3
    if K <= 128 and not minplus:
        return 4
    return 1


# The linear kernel with EXACT messages is drawn on a finer grid.  That mode promises the reference's bits, and the
# reference's lower-envelope routine for the linear kernel leaves out a segment that meets the segment before it
# exactly at that segment's root (typeStereoLinear.h:442-449: s <= qj, "numerical stability"), although the new segment
# is the lower one from there on.  Its message is then above the min-plus message: beliefs are off, the bound can
# exceed the optimum and can fall.  Multiples of 2^-6 produce such exact ties all the time (test_first_principles_cpu.py
# keeps one instance that shows it); 24 random bits make one a 2^-24 event per comparison while everything stays exact
# in fp64 (linear terms only: multiples of 2^-26, sums below 2^17).  The min-plus mode and the quadratic kernel are
# exact on the coarse grid and run there.
FINE_BITS = 24


def instance(H, W, K, shared, kernel, minplus, seed=0):
    """The instance of this shape for this kernel and message mode."""
    return problem(H, W, K, shared, seed, FINE_BITS if (kernel == 1 and not minplus) else 6)


def chain_cases(K, kernel):
    """Every (H, W, shared, minplus) the chain test runs at this label count and smoothness kernel."""
    return [(H, W, shared, minplus) for H, W in CHAIN_SHAPES for shared in (True, False) for minplus in (False, True)
            if expected_path(K, shared, minplus, kernel)]


# One seed per enumerated grid instance, in grid_cases() order: seeds on which the CPU oracle's bound reaches the
# optimum within 30 iterations (test_first_principles_cpu.py asserts it; a seed that does not is replaced, not excused).
GRID_SEEDS = tuple(range(100, 148))


def grid_cases():
    """[(H, W, K, kernel, shared, minplus, seed)]: every shape with both kernels, kinds of positions and message modes."""
    combos = [(H, W, K, kernel, shared, minplus) for H, W, K in GRID_SHAPES for kernel in (1, 2) for shared in (True, False)
              for minplus in (False, True)]
    assert len(GRID_SEEDS) == len(combos)
    return [c + (s,) for c, s in zip(combos, GRID_SEEDS)]
