"""Seeded generators shared by tests/test_diag_factored_cpu.py and tests/test_gpu_diag_factored.py: factored blocks in which
some constraints carry a diagonal part, A_k = diag(a_k) + V_k D_k V_k' (an item (V, d, a) of build_factored_model), beside plain
factors and a few stored matrices -- and a NumPy restatement of the formulas the device assembles such a block with, which the
CPU test checks against tr(A_i W A_j W) for every case below: the formulas are right before any kernel computes them.  (The GPU
test does not use this restatement: its references are h_definition from the dense A_k, mode 0 and the stored-matrix route.)"""
import numpy as np
import scipy.sparse as sp

# (msz, nvar, khat, diagonal rows): msz not a multiple of 16 or 64, R = nvar khat not a multiple of 64; one pure trace row,
# three rows (two of them adjacent in H order), the tile edge 63 / 64 / 65, every constraint a sum; msz 13: one partial K step
# of the MFMA kernels (no prefetch of a next step), 66 columns; msz 72: a second tile of 64 whose K range is one partial step
CASES = [(16, 5, 1, 1), (33, 37, 2, 3), (65, 70, 4, 63), (65, 70, 4, 64), (65, 70, 4, 65), (130, 130, 16, 130), (333, 300, 2, 3),
         (13, 33, 2, 1), (72, 70, 1, 65)]


def _factors(m, n, khat, seed):
    """Random signed dense factors of rank 0 .. khat (mixed), as tests/test_gpu_hybrid_factored.py draws them."""
    rng = np.random.default_rng(seed)
    facs = []
    for k in range(n):
        r = int(rng.integers(0, khat + 1)) if k % 4 else khat
        facs.append((rng.standard_normal((m, r)) / np.sqrt(m), rng.choice([-1.0, 1.0], size=r)))
    return facs


def _identity(m, seed):
    return sp.identity(m, format="csc")


def _nine(m, seed):
    """Nine entries: four symmetric off-diagonal pairs and one diagonal entry."""
    rng = np.random.default_rng(seed)
    A = sp.lil_matrix((m, m))
    idx = rng.choice(m, size=8, replace=False)
    for t in range(4):
        A[idx[2 * t], idx[2 * t + 1]] = A[idx[2 * t + 1], idx[2 * t]] = rng.standard_normal()
    A[idx[0], idx[0]] = -1.3
    return A.tocsc()


def _tridiag(m, seed):
    rng = np.random.default_rng(seed)
    off = rng.standard_normal(m - 1)
    return sp.diags([off, rng.standard_normal(m), off], [-1, 0, 1], format="csc")


def _dense_sym(m, seed):
    R = np.random.default_rng(seed).standard_normal((m, m))
    return sp.csc_matrix(0.5 * (R + R.T) / np.sqrt(m))


STORED_KINDS = [_identity, _nine, _tridiag, _dense_sym]


def _diagonal(m, seed):
    """A diagonal part with zeros and negative entries."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(m)
    a[rng.choice(m, size=max(1, m // 3), replace=False)] = 0.0
    a[0] = -abs(a[0]) - 0.5
    return a


def diag_rows(n, count):
    """Indices of the constraints that carry a diagonal part: one (the last), three (1 and 2 are adjacent in H order, and the
    last), `count` leading ones, or all."""
    if count == 1:
        return [n - 1]
    if count == 3:
        return [1, 2, n - 1]
    return list(range(count))


def stored_set(m, n, count, seed):
    """Stored constraints among the ones without a diagonal part: an identity, a 9-entry matrix and a dense matrix (a dense slot
    when the threshold is lowered to msz^2) -- none when every constraint is a sum."""
    free = [k for k in range(n) if k not in diag_rows(n, count)]
    if len(free) < 4:
        return {}
    idx = [free[0], free[len(free) // 2], free[-1]]
    kinds = [_identity, _nine, _dense_sym]
    return {k: kinds[t](m, seed + 10 * k + t) for t, k in enumerate(idx)}


def block_items(m, n, khat, count, seed, stored=True):
    """The items of one block for build_factored_model: (V, d) pairs, (V, d, a) triples at diag_rows (the single row of count 1
    is the pure trace row (None, [], ones)), stored matrices at stored_set."""
    items = list(_factors(m, n, khat, seed))
    for k in diag_rows(n, count):
        V, d = items[k]
        items[k] = (None, [], np.ones(m)) if count == 1 else (V, d, _diagonal(m, seed + 7 * k + 1))
    if stored:
        for k, a in stored_set(m, n, count, seed).items():
            items[k] = a
    return items


def dense_of(item):
    """The constraint matrix of an item, dense, from the definition."""
    if sp.issparse(item):
        return item.toarray()
    if isinstance(item, np.ndarray):
        return item
    V, d = item[0], np.asarray(item[1], float)
    m = len(item[2]) if len(item) == 3 else np.asarray(V).shape[0]
    A = np.zeros((m, m))
    if V is not None and np.asarray(V).size:
        V = np.asarray(V, float).reshape(m, -1)
        A = (V * d) @ V.T
        A = 0.5 * (A + A.T)
    if len(item) == 3:
        A = A + np.diag(np.asarray(item[2], float))
    return A


def diag_as_stored(items):
    """The same block with every (V, d, a) triple given as a stored sparse matrix: the route a diagonal part had to take before."""
    return [sp.csc_matrix(dense_of(it)) if isinstance(it, tuple) and len(it) == 3 else it for it in items]


def h_definition(As, W):
    """H_ij = tr(A_i W A_j W)."""
    A = np.stack(As)
    T = np.matmul(np.matmul(W, A), W)
    n = len(As)
    return A.reshape(n, -1) @ T.reshape(n, -1).T


def spd(m, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    return G @ G.T, G


def sym(m, seed):
    R = np.random.default_rng(seed).standard_normal((m, m))
    return 0.5 * (R + R.T)


def h_formulas(items, W):
    """The Schur matrix of a block the way the device assembles it: stored constraints S, factor parts F (every constraint that
    is not stored; weight 0 where it has no factors), diagonal parts D, with Ad the diagonals as columns and Y = W Vd:
        H_SS, H_FF, H_SF                              as for a hybrid block
        H_DD = Ad' (W o W) Ad
        C    = Ad' (Y o Y), weighted by d and summed per constraint;   H over the factored positions += C + C' (2 C_ss)
        H_sk = a_k' diag(W A_s W)                     stored s, diagonal row k"""
    n, m = len(items), W.shape[0]
    st = {k: dense_of(it) for k, it in enumerate(items) if not isinstance(it, tuple)}
    fac = {k: it for k, it in enumerate(items) if isinstance(it, tuple)}
    dg = {k: np.asarray(it[2], float) for k, it in fac.items() if len(it) == 3}
    H = np.zeros((n, n))
    for s, As in st.items():                                   # H_SS
        for t, At in st.items():
            H[s, t] = np.trace(As @ W @ At @ W)
    Y = {}
    for k, it in fac.items():
        V = np.zeros((m, 0)) if it[0] is None else np.asarray(it[0], float).reshape(m, -1)
        Y[k] = (W @ V, V, np.asarray(it[1], float))
    own = np.concatenate([np.full(v[1].shape[1], k, dtype=np.int64) for k, v in Y.items()])     # factor column -> constraint
    if own.size:                                               # H_FF: sum_pq d_p d_q (u_p' v_q)^2, summed per pair of constraints
        Yall, Vall = np.hstack([v[0] for v in Y.values()]), np.hstack([v[1] for v in Y.values()])
        dall = np.concatenate([v[2] for v in Y.values()])
        P = np.zeros((n, own.size))
        P[own, np.arange(own.size)] = 1.0
        H += P @ ((Yall.T @ Vall) ** 2 * np.outer(dall, dall)) @ P.T
    for j, (Yj, Vj, dj) in Y.items():
        for s, As in st.items():                               # H_SF: sum_p d_p y_p' A_s y_p
            H[s, j] = H[j, s] = float(np.sum(dj * np.sum(Yj * (As @ Yj), axis=0)))
    rows = sorted(dg)
    if rows:
        Ad = np.column_stack([dg[k] for k in rows])
        H[np.ix_(rows, rows)] += Ad.T @ (W * W) @ Ad           # H_DD
        C = np.zeros((len(rows), n))
        for j, (Yj, _, dj) in Y.items():
            C[:, j] = Ad.T @ ((Yj * Yj) @ dj)
        for a, k in enumerate(rows):                           # C + C'
            H[k, :] += C[a]
            H[:, k] += C[a]
        for s, As in st.items():                               # stored rows against diagonal rows
            ts = np.diag(W @ As @ W)
            for a, k in enumerate(rows):
                H[s, k] += Ad[:, a] @ ts
                H[k, s] += Ad[:, a] @ ts
    return H
