"""CPU restatement of Minimize_TRW_S (cpp/trw-s/minimize.cpp:31-113) that also records node beliefs.

Built on oracle.trws_structure (SetAutomaticOrdering + CompleteGraphConstruction) and oracle.update_message /
oracle.add_column, one node at a time in the reference's order.  After t iterations it runs the forward pass of
iteration t + 1 up to the point where each node has formed its Di (minimize.cpp:38-46) -- sending that node's forward
messages too, since later nodes read them -- and returns those Di: the definition of the plan's min-marginals
(DESIGN.md 4.7).  Small problems only (a Python loop per node and message).
"""
import numpy as np


def default_impl(oracle, minplus=False):
    """Message routine that matches the product: the reference's type classes where oracle/_ref is built, the oracle's
    envelope restatement otherwise; the brute-force definition for the min-plus message mode."""
    if minplus:
        return "brute"
    return "ref" if oracle.have_ref_types() else "envelope"


def oracle_trws(oracle, impl, kernel, p, tol, iters, ordering=0):
    """oracle.trws with the message routine `impl` (fixed iteration count)."""
    kw = dict(mode=0) if impl == "brute" else dict(mode=1, use_ref_types=(impl == "ref"))
    return oracle.trws(kernel, p["unary"], p["conn"], p["q"], p["qprim"], p["alphas"], tol, iters, -1e300,
                       ordering=ordering, **kw)


def _index_order_structure(N, conn):
    """MRFEnergy without SetAutomaticOrdering: nodes in index order (MRFEnergy.cpp:37-76), edges oriented by
    CompleteGraphConstruction (MRFEnergy.cpp:176-222; trws_oracle.c graph_orient)."""
    E = len(conn)
    tail = [int(a) for a, _ in conn]
    head = [int(b) for _, b in conn]
    dirn = [0] * E
    firstF, firstB = [-1] * N, [-1] * N
    nextF, nextB = [-1] * E, [-1] * E
    for e in range(E):   # MRFEnergy.cpp:83-111: prepended
        a, b = tail[e], head[e]
        nextF[e] = firstF[a]; firstF[a] = e
        nextB[e] = firstB[b]; firstB[b] = e
    rank = list(range(N))
    firstB = [-1] * N
    for i in range(N):
        eprev, e = -1, firstF[i]
        while e >= 0:
            j = head[e]
            if rank[i] < rank[j]:
                nextB[e] = firstB[j]; firstB[j] = e
                eprev, e = e, nextF[e]
            else:
                enext = nextF[e]
                dirn[e] = 1 - dirn[e]
                tail[e], head[e] = j, i
                if eprev >= 0:
                    nextF[eprev] = enext
                else:
                    firstF[i] = enext
                nextF[e] = firstF[j]; firstF[j] = e
                nextB[e] = firstB[i]; firstB[i] = e
                e = enext

    def walk(first, nxt, i):
        out, e = [], first[i]
        while e >= 0:
            out.append(e); e = nxt[e]
        return out

    return dict(order=list(range(N)), tail=tail, dir=dirn,
                fwd=[walk(firstF, nextF, i) for i in range(N)], bwd=[walk(firstB, nextB, i) for i in range(N)])


def _structure(oracle, N, conn, ordering):
    if ordering == 1:
        return _index_order_structure(N, conn)
    s = oracle.trws_structure(N, conn)
    fp, fi, bp, bi = s["fwd_ptr"], s["fwd_idx"], s["bwd_ptr"], s["bwd_idx"]
    return dict(order=[int(i) for i in np.argsort(s["rank"], kind="stable")], tail=[int(t) for t in s["tail"]],
                dir=[int(d) for d in s["dir"]],
                fwd=[[int(e) for e in fi[fp[i]:fp[i + 1]]] for i in range(N)],
                bwd=[[int(e) for e in bi[bp[i]:bp[i + 1]]] for i in range(N)])


def trws_beliefs(oracle, impl, kernel, p, tol, iters, ordering=0):
    """t = iters iterations (no stop test), then the beliefs.  p: trws_problem-style dict (unary (N,K), conn (E,2),
    q/qprim (E,K), alphas (E,)).  Returns dict(labels (1-based), energy, lb, iterations, D (N,K) beliefs,
    mm (N,K), confidence (N,), argmin (N,) 0-based)."""
    unary = np.ascontiguousarray(p["unary"], dtype=np.float64)
    q = np.ascontiguousarray(p["q"], dtype=np.float64)
    qp = np.ascontiguousarray(p["qprim"], dtype=np.float64)
    alphas = np.asarray(p["alphas"], dtype=np.float64)
    N, K = unary.shape
    E = len(p["conn"])
    g = _structure(oracle, N, p["conn"], ordering)
    order, fwd, bwd, tail, dirn = g["order"], g["fwd"], g["bwd"], g["tail"], g["dir"]
    gamma = [1.0 / max(len(fwd[i]), len(bwd[i])) if (fwd[i] or bwd[i]) else np.inf for i in range(N)]
    M = np.zeros((E, K))
    col_impl = "ref" if impl == "ref" else "brute"

    def upd(e, Di, i, d):
        m, v = oracle.update_message(kernel, Di, gamma[i], M[e], q[e], qp[e], alphas[e], tol, d, dirn[e], impl=impl)
        M[e] = m
        return v

    def forward(record=None):
        for i in order:
            Di = unary[i].copy()
            for e in fwd[i]:
                Di += M[e]
            for e in bwd[i]:
                Di += M[e]
            if record is not None:
                record[i] = Di
            for e in fwd[i]:
                upd(e, Di, i, 0)

    x = np.zeros(N, np.int64)
    LB = En = 0.0
    for _ in range(iters):
        forward()
        LB = 0.0
        for i in reversed(order):
            Di = unary[i].copy()
            for e in bwd[i]:
                Di += M[e]
            for e in fwd[i]:
                Di += M[e]
            vmin = Di[0]
            for k in range(1, K):
                if vmin > Di[k]:
                    vmin = Di[k]
            Di = Di - vmin
            LB += vmin
            for e in bwd[i]:
                LB += upd(e, Di, i, 1)
        En = 0.0
        for i in order:   # minimize.cpp:223-264
            Db = unary[i].copy()
            for e in bwd[i]:
                Db = oracle.add_column(kernel, q[e], qp[e], alphas[e], tol, x[tail[e]], Db, 0, dirn[e], impl=col_impl)
            Di = Db.copy()
            for e in fwd[i]:
                Di += M[e]
            k = int(np.argmin(Di))    # first minimum (strict '>' of the reference)
            x[i] = k
            En += Db[k]
    D = np.zeros((N, K))
    forward(record=D)
    mn = D.min(axis=1)
    mm = D - mn[:, None]
    conf = np.sort(mm, axis=1)[:, 1] if K > 1 else np.full(N, np.inf)
    return dict(labels=x.astype(np.float64) + 1, energy=En, lb=LB, iterations=float(iters), D=D, mm=mm,
                confidence=conf, argmin=np.argmin(D, axis=1))
