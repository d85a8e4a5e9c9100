"""Seeded cases of the rank-class route of the rank-k Schur assembly (library option lowrank_ragged, csrc/raggedops.hip):
factors of mixed ranks, an SPD W with its G (tests/test_gpu_factored.py::_spd), and the reference H_ij = tr(A_i W A_j W) from
the materialised A_k in NumPy.  Shared by tests/test_ragged_cpu.py and tests/test_gpu_ragged.py; everything is cached and
left unchanged.

    R1  16 / 5     ranks 16, 1, 0, 3, 2: classes 16, 1, 4, 2 in single partial tiles, a rank-0 row, a padding column, one K step
    R2  96 / 37    8 x rank 16, the rest cycling 1, 2, 4, 8, mixed signs: class 16 spans two tiles (diagonal + off-diagonal)
    R3  130 / 130  one rank 9, 129 x rank 1: the motivating shape, K tail, a last tile of one column
    R4  257 / 70   33 x rank 2, 37 x rank 5..8, sparse factors: short last tiles both ways, segment starts off 64
    R5  96 + 130 / 37  two blocks, R2's and one of R3's kind (msz 130, one rank 9 among 36 x rank 1), plus C_lin: H in natural
        order, the blocks accumulate into shared entries
    R6  R2 with constraints 0 and 7 stored as sparse matrices and constraint 3 = (None, [], ones): hybrid block + diagonal row
    R7  13 / 33    ranks cycling 2, 1, 4: classes 4, 2, 1 of 11 groups each (Rc = 77, no multiple of 16) in single partial tiles,
        and K = msz = 13: one partial K step, the prefetch of a next step never taken
"""
import functools

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
NAMES = ["R1", "R2", "R3", "R4", "R5", "R6", "R7"]


def spd(m, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    return G @ G.T, G


def _dense_factor(rng, m, r):
    return rng.standard_normal((m, r)) / np.sqrt(m), rng.choice([-1.0, 1.0], size=r)


def _sparse_factor(rng, m, r):
    V = np.zeros((m, r))
    for p in range(r):
        V[rng.choice(m, size=3, replace=False), p] = rng.standard_normal(3)
    return V, rng.choice([-1.0, 1.0], size=r)


def ranks_of(name):
    """The rank list of the single-block cases (H index = constraint number: identity sigmaA of a pure factored block)."""
    if name == "R1":
        return [16, 1, 0, 3, 2]
    if name in ("R2", "R6"):
        r = [16] * 8 + [(1, 2, 4, 8)[k % 4] for k in range(29)]
        if name == "R6":
            for k in (0, 3, 7):
                r[k] = 0
        return r
    if name == "R3":
        return [1] * 64 + [9] + [1] * 65
    if name == "R5b":                                  # the second block of R5
        return [1] * 18 + [9] + [1] * 18
    if name == "R4":
        return [2] * 33 + [5 + k % 4 for k in range(37)]
    if name == "R7":
        return [(2, 1, 4)[k % 3] for k in range(33)]
    raise KeyError(name)


SIZES = {"R1": (16, 5), "R2": (96, 37), "R3": (130, 130), "R4": (257, 70), "R5b": (130, 37), "R6": (96, 37), "R7": (13, 33)}
SEEDS = {"R1": 101, "R2": 102, "R3": 103, "R4": 104, "R5b": 105, "R6": 102, "R7": 107}


@functools.lru_cache(maxsize=None)
def factors(name):
    """[(V, d)] of a single-block case; R6: the factors of R2 (the entries of constraints 0, 3, 7 are replaced in `items`)."""
    m, n = SIZES[name]
    rng = np.random.default_rng(SEEDS[name])
    ranks = ranks_of("R2" if name == "R6" else name)
    make = _sparse_factor if name == "R4" else _dense_factor
    return [make(rng, m, r) for r in ranks]


@functools.lru_cache(maxsize=None)
def stored_rows(m, seed=7):
    """Two sparse symmetric matrices (the stored constraints of R6)."""
    out = []
    for s in (seed, seed + 1):
        a = sp.random(m, m, density=0.02, random_state=s, format="csr")
        out.append(sp.csc_matrix(a + a.T + sp.diags(np.random.default_rng(s).standard_normal(m) * (np.arange(m) % 5 == 0))))
    return out


def blocks(name):
    """The `factors` argument of build_factored_model / load_factored_model: one list per block."""
    if name == "R5":
        return [list(factors("R2")), list(factors("R5b"))]
    items = list(factors(name))
    if name == "R6":
        m = SIZES["R6"][0]
        s0, s7 = stored_rows(m)
        items[0], items[7] = s0, s7
        items[3] = (None, [], np.ones(m))
    return [items]


def nvar(name):
    return SIZES["R2"][1] if name == "R5" else SIZES[name][1]


def msizes(name):
    return [SIZES["R2"][0], SIZES["R5b"][0]] if name == "R5" else [SIZES[name][0]]


def c_lin(name):
    if name != "R5":
        return None
    return sp.random(nvar(name), 6, density=0.3, random_state=3, format="csr")


def materialise(item, m):
    """A_k (dense) of one entry of `blocks`: a pair (V, d), a triple (V, d, a) or a stored matrix."""
    if sp.issparse(item):
        return item.toarray()
    if len(item) == 3:
        V, d, a = item
        A = np.diag(np.asarray(a, float))
        if V is not None and np.size(d):
            A = A + (np.asarray(V) * np.asarray(d)) @ np.asarray(V).T
        return A
    V, d = item
    a = (V * d) @ V.T
    return 0.5 * (a + a.T)


@functools.lru_cache(maxsize=None)
def scaling(name):
    """[(W, G)] per block."""
    return [spd(m, 1000 + 10 * i + m) for i, m in enumerate(msizes(name))]


def _h_block(As, W, dtype):
    W = W.astype(dtype)
    T = [W @ a.astype(dtype) @ W for a in As]
    n = len(As)
    H = np.zeros((n, n), dtype=dtype)
    for i in range(n):
        for j in range(i + 1):
            H[i, j] = H[j, i] = np.sum(T[i] * As[j].astype(dtype))
    return H


@functools.lru_cache(maxsize=None)
def reference(name, dtype=np.float64):
    """H_ij = sum over blocks of tr(A_i W A_j W) from the materialised A_k (+ C_lin diag(X_lin ./ S_lin) C_lin' with unit
    X_lin, S_lin_inv for R5), natural order."""
    n = nvar(name)
    H = np.zeros((n, n), dtype=dtype)
    for items, m, (W, _) in zip(blocks(name), msizes(name), scaling(name)):
        H += _h_block([materialise(it, m) for it in items], W, dtype)
    C = c_lin(name)
    if C is not None:
        Cd = C.toarray().astype(dtype)
        H += Cd @ Cd.T
    return H


def relerr(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.sqrt(np.sum((a - b) ** 2)) / max(np.sqrt(np.sum(b * b)), LD(1e-300)))


def model(name):
    from loraine_jl_amd.model import build_factored_model
    n = nvar(name)
    C = c_lin(name)
    F0 = [-np.eye(m) for m in msizes(name)]
    return build_factored_model(F0, blocks(name), np.zeros(n), 0.0, None if C is None else np.ones(C.shape[1]), C,
                                factored_form=1)


def block_ranks(fm, i):
    """Ranks per constraint of block i as the library counts them: weighted factor columns of the padded upload."""
    _, d, khat = fm.lowrank[i]
    return np.count_nonzero(np.asarray(d).reshape(-1, khat), axis=1).tolist()


# ---------------------------------------------------------------------------------------------- the planted solve
class Planted:
    """max b'y s.t. C - sum_k y_k M_k >= 0, M_k = -A_k, A_k = V_k diag(d_k) V_k' of mixed ranks: msz 40 / nvar 60 with 58 rank-1
    constraints and two of rank 6, planted as loraine_jl_amd.synthetic.FactoredLowRankProblem plants its own: X* = Q diag(lam)
    Q' of rank 2, S* = I - Q Q', y* ~ 0.1 N(0, 1), b_k = <M_k, X*>, C = S* + sum_k y*_k M_k; optimum b'y*."""

    def __init__(self, m=40, n=60, seed=17):
        rng = np.random.default_rng(seed)
        self.m, self.n = m, n
        self.ranks = [6 if k in (11, 42) else 1 for k in range(n)]
        self.facs = [_dense_factor(rng, m, r) for r in self.ranks]
        Q, _ = np.linalg.qr(rng.standard_normal((m, 2)))
        lam = np.array([1.0, 1.5])
        lam *= np.sqrt(m) / lam.sum()
        X = (Q * lam) @ Q.T
        As = [materialise(f, m) for f in self.facs]
        self.b = -np.array([np.sum(a * X) for a in As])
        self.ystar = 0.1 * rng.standard_normal(n)
        C = np.eye(m) - Q @ Q.T - sum(y * a for y, a in zip(self.ystar, As))
        self.C = 0.5 * (C + C.T)
        self.optimum = float(self.b @ self.ystar)

    def F0(self):
        return [-self.C]

    def factors(self):
        return [list(self.facs)]
