"""Inputs of tests/test_cg_diag_cpu.py and tests/test_gpu_cg_diag.py: the models of tests/cg_lowrank_cases.py with DIAGONAL PARTS
added to some constraints, A_k = diag(a_k) + V_k D_k V_k'.  Each case exists twice: as a factored model (the (V, d, a) triples
of build_factored_model, some constraints of D1h as matrices) and materialised, as the oracle model whose np.longdouble
cr.dense_operator / cr.reference_run is the reference.  Nothing is committed as a fixture.

Recipe: the case is drawn exactly as lc.build_case draws it, with the same rng order; before the matrices are formed
drng = default_rng(seed_d), and for each block in order, for each listed row in ascending order,
    a = drng.standard_normal(m) / sqrt(m);  a[drng.random(m) < 0.25] = 0;  A_k += diag(a).

  D1   L1 (msz 37, nvar 130, khat 4)           rows {0, 1, 2, 64, 129}              seed_d 7321   K = 7, 7, 10, 12 per lc.PRECS
  D1a  L1                                      all 130 rows (tiles of 64 + 64 + 2)  seed_d 7321   K = 6, 6, 11, 10
  D1h  D1 with constraints {7, 100} as matrices: a hybrid block with diagonal rows -- the data and the reference of D1
  D2   L2 (33 + 18, nvar 257, 5 linear rows)   block 0 {3, 64, 65, 256}, block 1 every even row   seed_d 7322   K = 7, 7, 10, 10
  D3   L3 (msz 70, nvar 65, khat 1)            rows 0 .. 16 (K start of the second 64-column tile)   seed_d 7314   K = 8, 10, 12, 12

K is what cr.choose_K returned where this file was written (the last K in 3 .. 12 with a gap and a drift of the float64 dense
recurrence below cr.DRIFT_MAX; the drift is a rounding-level quantity, so K is recorded, not asserted: the tests take run.K).

The seeds matter: with them cr.reference_run meets its gap and drift conditions for all four lc.PRECS, and a float64 recurrence
in the device's algebra (DiagFactorOperator) reaches the reference's exits within 5 x the oracle's distance (worst ratios
measured: D1 1.39, D1a 1.26, D1h 0.80, D2 1.42, D3 1.82).  For D3, seed_d = 7313 gives a ratio of 3.2 and seed_d = 7315 loses
the reference's gap under the two diagonal preconditioners."""
import functools
import types

import numpy as np
import scipy.sparse as sp

import cg_lowrank_cases as lc
from oracle import cg_reference as cr
from oracle import loraine_oracle as lo

# name -> (case of cg_lowrank_cases, diagonal rows per block, seed_d, stored constraints per block)
CASES = {
    "D1": ("L1", [(0, 1, 2, 64, 129)], 7321, [()]),
    "D1a": ("L1", [tuple(range(130))], 7321, [()]),
    "D1h": ("L1", [(0, 1, 2, 64, 129)], 7321, [(7, 100)]),
    "D2": ("L2", [(3, 64, 65, 256), tuple(range(0, 257, 2))], 7322, [(), ()]),
    "D3": ("L3", [tuple(range(17))], 7314, [()]),
}
NAMES = list(CASES)


def base(name):
    return CASES[name][0]


def data_name(name):
    """The case whose materialised data (and so whose reference) `name` shares: D1h is D1 given differently."""
    return "D1" if name == "D1h" else name


def diag_sets(name):
    return [tuple(s) for s in CASES[name][1]]


def stored_sets(name):
    return [tuple(s) for s in CASES[name][3]]


def n_diag(name):
    return sum(len(s) for s in CASES[name][1])


def n_stored(name):
    return sum(len(s) for s in CASES[name][3])


def n_blocks(name):
    return len(CASES[name][1])


def build_case(name):
    """lc.build_case with the diagonal parts added (the draws of `rng` in its order): model (oracle MyModel of the
    materialised data), factors (per block [(V, d)]), diag (per block {k: a}), W, G, X_lin, S_lin_inv, h, x."""
    lname, rows, seed_d, _ = CASES[name]
    msizes, nvar, kmax, nlin, seed = lc.SHAPES[lname]
    rng = np.random.default_rng(seed)
    factors = [lc._block_factors(m, nvar, k, rng) for m, k in zip(msizes, kmax)]
    drng = np.random.default_rng(seed_d)
    diag = []
    for m, rws in zip(msizes, rows):
        dg = {}
        for k in sorted(rws):
            a = drng.standard_normal(m) / np.sqrt(m)
            a[drng.random(m) < 0.25] = 0.0
            dg[k] = a
        diag.append(dg)
    A = []
    for m, facs, dg in zip(msizes, factors, diag):
        C0 = rng.standard_normal((m, m))
        mats = lc._matrices(facs)
        for k, a in dg.items():
            mats[k] = sp.csc_matrix(mats[k] + sp.diags(a, format="csc"))
        A.append([sp.csc_matrix(-(C0 + C0.T) / 2)] + mats)
    C_lin = d_lin = None
    if nlin > 0:
        C_lin = sp.csr_matrix(sp.random(nvar, nlin, density=0.06, random_state=rng, data_rvs=rng.standard_normal))
        d_lin = rng.standard_normal(nlin)
    model = lo.make_model(A, rng.standard_normal(nvar), 0.0, d_lin, C_lin)
    rng = np.random.default_rng(seed + 1000)
    W, G = [], []
    for m in msizes:
        Wb, Gb = cr.scaling_from_spectrum(cr.spectrum(m, top=min(4, m - 1)), rng)
        W.append(Wb)
        G.append(Gb)
    X_lin = np.exp(rng.uniform(-1.0, 1.0, model.nlin))
    S_lin_inv = np.exp(rng.uniform(-1.0, 1.0, model.nlin))
    x = rng.standard_normal(nvar)
    case = types.SimpleNamespace(name=name, model=model, factors=factors, diag=diag, W=W, G=G, X_lin=X_lin,
                                 S_lin_inv=S_lin_inv, h=None, x=x)
    h = np.zeros(nvar)
    lo.MyA(W, model.AA, model.nlin, model.C_lin, X_lin, S_lin_inv)(h, rng.standard_normal(nvar))
    case.h = h
    return case


@functools.lru_cache(maxsize=None)
def _inputs(dname):
    return build_case(dname)


def case_inputs(name):
    """Built once per process, shared by every test that needs it, never modified (D1h: the object of D1)."""
    return _inputs(data_name(name))


@functools.lru_cache(maxsize=None)
def _data(dname):
    case = _inputs(dname)
    return case, cr.dense_operator(case.model, case.W, case.X_lin, case.S_lin_inv)


def case_data(name):
    """(case, dense longdouble H of the materialised model)."""
    return _data(data_name(name))


@functools.lru_cache(maxsize=None)
def _run(dname, prec, erank):
    case, H = _data(dname)
    return cr.reference_run(case, H, prec, erank)


def case_run(name, prec, erank):
    return _run(data_name(name), prec, erank)


def block_items(name):
    """Per block the items of build_factored_model: (V, d), (V, d, a) at the diagonal rows, the matrix at the stored ones."""
    case = case_inputs(name)
    m = case.model
    blocks = []
    for i, (facs, dg, st) in enumerate(zip(case.factors, case.diag, stored_sets(name))):
        blk = list(facs)
        for k, a in dg.items():
            blk[k] = (facs[k][0], facs[k][1], a)
        for k in st:
            assert k not in dg
            blk[k] = sp.csc_matrix(m.A[i][k + 1])
        blocks.append(blk)
    return blocks


@functools.lru_cache(maxsize=None)
def factored_model(name):
    """The factored model of case `name`, built once per process and never modified."""
    from loraine_jl_amd.model import build_factored_model
    case = case_inputs(name)
    m = case.model
    F0 = [sp.csc_matrix(m.A[i][0]) for i in range(m.nlmi)]
    fm = build_factored_model(F0, block_items(name), np.asarray(m.b, float), 0.0, m.d_lin if m.nlin else None,
                              m.C_lin if m.nlin else None, factored_form=1)
    assert fm.factored and all(fm.factored_blocks)
    assert [sorted(s) for s in fm.stored] == [sorted(s) for s in stored_sets(name)]
    assert [sorted(d) for d in fm.diag] == [sorted(s) for s in diag_sets(name)]
    return fm


class DiagFactorOperator:
    """MyA in float64 in the algebra of the device under cg_factored + cg_diag (the composition; the scaled-factor form is not
    taken for a block with diagonal rows): per block M = -V diag(d o x) V' (lower triangle, mirrored) minus diag(Ad x_rows),
    minus x_k A_k for the stored constraints; Z = (W M) W; (Ax)_k = -sum_p d_kp v_kp' Z v_kp - a_k' diag(Z), and -<A_s, Z> for
    a stored constraint."""

    def __init__(self, case, stored):
        self.case, self.blocks = case, []
        n = case.model.n
        for i, facs in enumerate(case.factors):
            st = sorted(stored[i])
            keep = [k for k in range(n) if k not in st]
            V = np.concatenate([facs[k][0] for k in keep], axis=1)
            d = np.concatenate([facs[k][1] for k in keep])
            own = np.repeat(np.asarray(keep), [facs[k][0].shape[1] for k in keep])
            As = [np.asarray(case.model.A[i][k + 1].todense()) for k in st]
            rows = sorted(case.diag[i])
            Ad = np.column_stack([case.diag[i][k] for k in rows]) if rows else np.zeros((V.shape[0], 0))
            self.blocks.append((V, d, own, case.W[i], st, As, np.asarray(rows, dtype=np.int64), Ad))

    def __call__(self, Ax, x):
        y = np.zeros_like(x)
        for V, d, own, W, st, As, rows, Ad in self.blocks:
            M = -(V * (d * x[own])) @ V.T
            M = np.tril(M) + np.tril(M, -1).T
            M[np.diag_indices_from(M)] -= Ad @ x[rows]
            for k, A in zip(st, As):
                M = M - x[k] * A
            Z = (W @ M) @ W
            np.add.at(y, own, -d * np.einsum("ij,ij->j", Z @ V, V))
            y[rows] -= Ad.T @ np.diag(Z)
            for k, A in zip(st, As):
                y[k] -= float(np.sum(A * Z))
        m = self.case.model
        if m.nlin > 0:
            y += m.C_lin @ ((self.case.X_lin * self.case.S_lin_inv) * (m.C_lin.T @ x))
        Ax[:] = y


def ts_formula(case, stored, erank, aamat=1):
    """H_alpha of the materialised model as the DEVICE forms it, in NumPy float64: per block the eigenpairs of W, tau and
    Um = v_l sqrt(lambda_l - tau), L = chol(2 W - Um Um') (lower), and
        t[j, a m + r] = -[ sum_p d_jp (v_jp' u_a) (L' v_jp)[r]           factor term (P = L' Vd, T = Vd' Um)
                           + sum_{i >= r} a_ji u_a[i] L[i, r]             diagonal term (ts_diag_mfma_kernel)
                           + (L' A_j u_a)[r] for a stored constraint ]    stored rows, from the entries
    (the device keeps ts = D^-1/2 t; the scaling cancels in the matrix).  Returns M_alpha = AAAATtau + t t' -- the matrix
    cr.prec_alpha_matrix forms from the dense A_k."""
    model = case.model
    n, k = model.n, erank
    dsum, cols = 0.0, []
    for i, facs in enumerate(case.factors):
        m = int(model.msizes[i])
        W = case.W[i]
        lam, Q = np.linalg.eigh(W)
        tau = lo._tau(lam[: m - k], aamat)
        if aamat < 3:
            dsum += tau * tau
        Um = Q[:, m - k:] * np.sqrt(lam[m - k:] - tau)[None, :]
        L = np.linalg.cholesky(2.0 * W - Um @ Um.T)
        st = set(stored[i])
        t = np.zeros((n, k * m))
        for a in range(k):
            u = Um[:, a]
            for j in range(n):
                if j in st:
                    t[j, a * m:(a + 1) * m] = -(L.T @ (np.asarray(model.A[i][j + 1].todense()) @ u))
                    continue
                V, d = facs[j]
                row = -((L.T @ V) @ (d * (V.T @ u)))
                if j in case.diag[i]:
                    au = case.diag[i][j] * u
                    row = row - np.array([au[r:] @ L[r:, r] for r in range(m)])
                t[j, a * m:(a + 1) * m] = row
        cols.append(t)
    t = np.concatenate(cols, axis=1)
    M = dsum * np.eye(n) + t @ t.T
    if model.nlin > 0:
        Cl = model.C_lin.toarray()
        M += (Cl * (case.X_lin * case.S_lin_inv)[None, :]) @ Cl.T
    return M
