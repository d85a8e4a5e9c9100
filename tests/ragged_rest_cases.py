"""Seeded cases of what else runs on the compacted columns of a mixed-rank factored block (library options ragged_cross and
ragged_ts; csrc/fac_cols.h, csrc/schur_factored.hip, csrc/facops.hip, csrc/diagops.hip, csrc/prec.hip): the cross terms of the mode-1 assembly with stored
constraints and diagonal parts, and ts of H_alpha.  Shared by tests/test_ragged_rest_cpu.py and tests/test_gpu_ragged_rest.py;
everything is cached and left unchanged, nothing is committed as a fixture.

    X1  ragged_cases R6 (96 / 37): two sparse stored rows and one purely diagonal row among the classes 16, 8, 4, 2, 1
    X2  msz 70 / nvar 90, rank of constraint k = (1, 2, 3, 5, 9, 16)[k % 6]: all five classes, segments starting at 0, 480, 600,
        660, 690 (Rc = 705 of R = 1440) as drawn; then constraints 0 and 31 become sparse stored matrices, constraint 5 a full
        symmetric one (a dense slot), constraint 13 the trace row (None, [], ones), and twenty others keep their factors and get
        a diagonal part (V, d, a).  What the device sees: 86 groups, segments at 0, 464, 584, 644, 670, Rc = 684 -- none but the
        first a multiple of 64 --, a K tail (70 = 4 x 16 + 6), 21 diagonal rows
    T1  msz 70 / nvar 65, ranks cycling 1, 2, 3, 5, 9 (khat 16, all five classes), built as cg_lowrank_cases.build_case builds its
        cases: constraints 0 and 64 stored, constraint 1 with a diagonal part beside its factors, constraint 63 purely diagonal --
        rows without a group at the first row of a 64-row tile of ts, at its last row and in the tile of one row

The reference of H is ragged_cases' tr(A_i W A_j W) from the materialised matrices in np.longdouble; that of H_alpha is
oracle/cg_reference.py on the oracle model of the materialised data.  compact / h_by_group / ts_by_group restate the compacted
algebra of the device in NumPy float64 from the padded upload and the index maps of loraine_jl_amd.model.ragged_columns."""
import functools
import types

import numpy as np
import scipy.sparse as sp

import ragged_cases as rc
from oracle import cg_reference as cr
from oracle import loraine_oracle as lo

LD = np.longdouble
NAMES = ["X1", "X2", "T1"]
X2_RANKS = (1, 2, 3, 5, 9, 16)
X2_STORED, X2_DENSE, X2_TRACE = (0, 31), 5, 13
X2_DIAG = [k for k in range(1, 90) if k not in (5, 13, 31)][::4][:20]
T1_RANKS = (1, 2, 3, 5, 9)
T1_STORED, T1_DIAG, T1_PURE = (0, 64), 1, 63


def _sym_sparse(m, seed):
    a = sp.random(m, m, density=0.03, random_state=seed, format="csr")
    return sp.csc_matrix(a + a.T + sp.diags(np.random.default_rng(seed).standard_normal(m) * (np.arange(m) % 7 == 0)))


def _diag_part(rng, m):
    a = rng.standard_normal(m) / np.sqrt(m)
    a[rng.random(m) < 0.25] = 0.0
    return a


@functools.lru_cache(maxsize=None)
def items(name):
    """The constraint list of the one block, as build_factored_model takes it."""
    if name == "X1":
        return tuple(rc.blocks("R6")[0])
    if name == "X2":
        m, n = 70, 90
        rng = np.random.default_rng(2001)
        out = [rc._dense_factor(rng, m, X2_RANKS[k % 6]) for k in range(n)]
        for i, k in enumerate(X2_STORED):
            out[k] = _sym_sparse(m, 40 + i)
        full = rng.standard_normal((m, m)) / m
        out[X2_DENSE] = sp.csc_matrix(full + full.T)
        out[X2_TRACE] = (None, [], np.ones(m))
        for k in X2_DIAG:
            out[k] = (out[k][0], out[k][1], _diag_part(rng, m))
        return tuple(out)
    if name == "T1":
        m, n = 70, 65
        rng = np.random.default_rng(2002)
        out = [rc._dense_factor(rng, m, T1_RANKS[k % 5]) for k in range(n)]
        for k in T1_STORED:
            out[k] = sp.csc_matrix(rc.materialise(out[k], m))
        out[T1_DIAG] = (out[T1_DIAG][0], out[T1_DIAG][1], _diag_part(rng, m))
        out[T1_PURE] = (None, [], _diag_part(rng, m))
        return tuple(out)
    raise KeyError(name)


def sizes(name):
    return {"X1": rc.SIZES["R6"], "X2": (70, 90), "T1": (70, 65)}[name]


def stored_rows(name):
    return sorted(k for k, it in enumerate(items(name)) if sp.issparse(it))


def diag_rows(name):
    return sorted(k for k, it in enumerate(items(name)) if not sp.issparse(it) and len(it) == 3)


def cross_rows(name):
    """Constraints whose rows and columns of H hold cross terms: the stored and the diagonal ones."""
    return sorted(stored_rows(name) + diag_rows(name))


@functools.lru_cache(maxsize=None)
def matrices(name):
    m, _ = sizes(name)
    return tuple(rc.materialise(it, m) for it in items(name))


@functools.lru_cache(maxsize=None)
def case(name):
    """model (oracle MyModel of the materialised data), W, G (lists), X_lin, S_lin_inv (empty), x -- what oracle/cg_reference.py
    reads.  X1, X2: W, G of ragged_cases.spd; T1: the spectrum of the CG cases."""
    m, n = sizes(name)
    rng = np.random.default_rng(3000 + n)
    C0 = rng.standard_normal((m, m))
    A = [[sp.csc_matrix(-(C0 + C0.T) / 2)] + [sp.csc_matrix(a) for a in matrices(name)]]
    model = lo.make_model(A, rng.standard_normal(n), 0.0, None, None)
    if name == "X1":
        W, G = rc.scaling("R6")[0]
    elif name == "X2":
        W, G = rc.spd(m, 1000 + m)
    else:
        W, G = cr.scaling_from_spectrum(cr.spectrum(m, top=4), rng)
    return types.SimpleNamespace(name=name, model=model, W=[W], G=[G], X_lin=np.zeros(0), S_lin_inv=np.zeros(0),
                                 x=rng.standard_normal(n))


@functools.lru_cache(maxsize=None)
def factored_model(name):
    from loraine_jl_amd.model import build_factored_model
    m, n = sizes(name)
    c = case(name)
    fm = build_factored_model([sp.csc_matrix(c.model.A[0][0])], [list(items(name))], np.asarray(c.model.b, float), 0.0, None,
                              None, factored_form=1)
    assert fm.factored and sorted(fm.stored[0]) == stored_rows(name) and sorted(fm.diag[0]) == diag_rows(name)
    return fm


@functools.lru_cache(maxsize=None)
def reference_h(name):
    """H_ij = tr(A_i W A_j W) in np.longdouble (ragged_cases' reference on this case's matrices)."""
    return rc._h_block(list(matrices(name)), case(name).W[0], LD)


def block_ranks(name):
    return rc.block_ranks(factored_model(name), 0)


# ---------------------------------------------------------------------------------------------- the compacted algebra in NumPy
def compact(name):
    """(plan, Vc, wc) from the padded upload of the block by the index maps of ragged_columns (natural constraint order)."""
    from loraine_jl_amd.model import ragged_columns
    V, d, khat = factored_model(name).lowrank[0]
    n = sizes(name)[1]
    Vp = np.asarray(V.todense()).reshape(n, khat, -1)
    d = np.asarray(d, float).reshape(n, khat)
    p = ragged_columns(np.count_nonzero(d, axis=1).tolist())
    Vc, wc = np.zeros((Vp.shape[2], p["Rc"])), np.zeros(p["Rc"])
    for col in range(p["Rc"]):
        if p["wc"][col] < 0:
            continue
        h = p["gh"][p["cg"][col]]
        q = np.flatnonzero(d[h])[p["wc"][col]]
        Vc[:, col], wc[col] = Vp[h, q], d[h, q]
    return p, Vc, wc


def h_by_group(name):
    """H of mode 1 as the device forms it under lowrank_ragged + ragged_cross, float64: H_FF = the weighted squares of Yc' Vc
    summed by group pair; stored x stored from the matrices; stored x factored H_sj = sum_{c in group j} wc_c y_c' A_s y_c;
    diagonal parts H_DD = Ad' (W o W) Ad, C = Ad' (Yc o Yc) weighted and summed class by class and stored through gh (a
    constraint of rank 0 keeps its zero), H += C + C'; stored x diagonal a_k' diag(W A_s W)."""
    m, n = sizes(name)
    fm = factored_model(name)
    W = case(name).W[0]
    p, Vc, wc = compact(name)
    gh = np.asarray(p["gh"], int)
    Yc = W @ Vc
    H = np.zeros((n, n))
    S = (Yc.T @ Vc) ** 2 * np.outer(wc, wc)
    cg = np.asarray(p["cg"], int)
    ng = len(gh)
    B = np.zeros((p["Rc"], ng))
    B[np.arange(p["Rc"]), cg] = 1.0
    H[np.ix_(gh, gh)] += B.T @ S @ B
    st = stored_rows(name)
    As = {k: np.asarray(fm.stored[0][k].todense()) for k in st}
    for s in st:
        WAW = W @ As[s] @ W
        for t in st:
            H[s, t] += np.sum(WAW * As[t])
        q = wc * np.einsum("ic,ic->c", As[s] @ Yc, Yc)
        for g in range(ng):
            v = q[p["start"][g]:p["start"][g] + p["size"][g]].sum()
            H[s, gh[g]] += v
            H[gh[g], s] += v
    rows = diag_rows(name)
    if rows:
        Ad = np.column_stack([fm.diag[0][k] for k in rows])
        H[np.ix_(rows, rows)] += Ad.T @ (W * W) @ Ad
        C = np.zeros((len(rows), n))
        g = 0
        while g < ng:                                      # one product per class segment
            c = p["size"][g]
            g1 = g
            while g1 < ng and p["size"][g1] == c:
                g1 += 1
            c0, c1 = p["start"][g], p["start"][g] + c * (g1 - g)
            part = (Ad.T @ (Yc[:, c0:c1] ** 2)) * wc[c0:c1]
            C[:, gh[g:g1]] = part.reshape(len(rows), g1 - g, c).sum(axis=2)
            g = g1
        for i, k in enumerate(rows):
            H[k, :] += C[i]
            H[:, k] += C[i]
        for s in st:
            ts = np.diag(W @ As[s] @ W)
            for i, k in enumerate(rows):
                v = float(ts @ Ad[:, i])
                H[s, k] += v
                H[k, s] += v
    return H


def ts_by_group(name, erank, aamat=1):
    """M_alpha = AAAATtau + t t' with t as the device forms it under ragged_ts, float64 (cg_diag_cases.ts_formula on the
    compacted columns): Pc = L' Vc, Tc = Vc' Um, t[j, a m + r] = -sum_{c in group hg[j]} wc_c Tc[c, a] Pc[r, c], zero where
    hg[j] < 0; the diagonal term and the stored rows as there."""
    m, n = sizes(name)
    fm = factored_model(name)
    W = case(name).W[0]
    p, Vc, wc = compact(name)
    k = erank
    lam, Q = np.linalg.eigh(W)
    tau = lo._tau(lam[: m - k], aamat)
    Um = Q[:, m - k:] * np.sqrt(lam[m - k:] - tau)[None, :]
    L = np.linalg.cholesky(2.0 * W - Um @ Um.T)
    Pc, Tc = L.T @ Vc, Vc.T @ Um
    t = np.zeros((n, k * m))
    for a in range(k):
        u = Um[:, a]
        for j in range(n):
            g = p["hg"][j]
            row = np.zeros(m)
            if g >= 0:
                for c in range(p["start"][g], p["start"][g] + p["size"][g]):
                    if wc[c] != 0.0:
                        row -= wc[c] * Tc[c, a] * Pc[:, c]
            if j in fm.diag[0]:
                au = fm.diag[0][j] * u
                row = row - np.array([au[r:] @ L[r:, r] for r in range(m)])
            if j in fm.stored[0]:
                assert g < 0
                row = -(L.T @ (np.asarray(fm.stored[0][j].todense()) @ u))
            t[j, a * m:(a + 1) * m] = row
    dsum = tau * tau if aamat < 3 else 0.0
    return dsum * np.eye(n) + t @ t.T


# ---------------------------------------------------------------------------------------------- the planted solve
class PlantedTrace(rc.Planted):
    """ragged_cases.Planted with the trace row tr X added as the purely diagonal constraint (None, [], ones): A = I, y*_tr =
    0.05, b_tr = <M_tr, X*> = -tr X*, C less y*_tr I -- S* and X* are those of the parent, the optimum moves by b_tr y*_tr."""

    def __init__(self, m=40, n=60, seed=17):
        super().__init__(m, n, seed)
        rng = np.random.default_rng(seed)                  # the parent's draws again, up to X*
        facs = [rc._dense_factor(rng, m, r) for r in self.ranks]
        assert all(np.array_equal(a[0], b[0]) for a, b in zip(facs, self.facs))
        Q, _ = np.linalg.qr(rng.standard_normal((m, 2)))
        lam = np.array([1.0, 1.5])
        lam *= np.sqrt(m) / lam.sum()
        X = (Q * lam) @ Q.T
        ytr = 0.05
        self.facs = list(self.facs) + [(None, [], np.ones(m))]
        self.b = np.append(self.b, -np.trace(X))
        self.ystar = np.append(self.ystar, ytr)
        self.C = self.C - ytr * np.eye(m)
        self.n = n + 1
        self.optimum = float(self.b @ self.ystar)
