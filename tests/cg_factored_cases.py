"""Inputs of tests/test_cg_factored_cpu.py and tests/test_gpu_cg_factored.py: the models of tests/cg_lowrank_cases.py loaded as
FACTORED models (build_factored_model(..., factored_form=1) from case.factors), some constraints given as matrices instead --
hybrid blocks.  The data is the data of the materialised model, so its longdouble H, case_run and the oracle are the
reference; nothing new is computed here but the NumPy float64 operators in the algebra the device uses.

  F1   L1 (msz 37, nvar 130, khat 4)            pure
  F1h  L1 with constraints {0, 7, 129} stored   hybrid: a dense slot candidate (0), a sparse one (7), the last dense one
  F2   L2 (33 + 18, nvar 257, 5 linear rows)    block 0 hybrid {3, 64, 256}, block 1 pure
  F3   L3 (msz 70, nvar 65, khat 1)             {0, 64} stored
"""
import functools

import numpy as np
import scipy.sparse as sp

import cg_lowrank_cases as lc

# name -> (case of cg_lowrank_cases, stored constraints per block)
CASES = {
    "F1": ("L1", [()]),
    "F1h": ("L1", [(0, 7, 129)]),
    "F2": ("L2", [(3, 64, 256), ()]),
    "F3": ("L3", [(0, 64)]),
}


def base(name):
    return CASES[name][0]


def stored_sets(name):
    return [tuple(s) for s in CASES[name][1]]


def n_stored(name):
    return sum(len(s) for s in CASES[name][1])


def n_pure(name):
    return sum(1 for s in CASES[name][1] if not s)


def n_blocks(name):
    return len(CASES[name][1])


@functools.lru_cache(maxsize=None)
def factored_model(name):
    """The factored model of case `name`, built once per process and never modified."""
    from loraine_jl_amd.model import build_factored_model
    case = lc.case_inputs(base(name))
    m = case.model
    blocks = []
    for i, (facs, st) in enumerate(zip(case.factors, stored_sets(name))):
        blk = list(facs)
        for k in st:
            blk[k] = sp.csc_matrix(m.A[i][k + 1])
        blocks.append(blk)
    F0 = [sp.csc_matrix(m.A[i][0]) for i in range(m.nlmi)]
    fm = build_factored_model(F0, blocks, np.asarray(m.b, float), 0.0, m.d_lin if m.nlin else None,
                              m.C_lin if m.nlin else None, factored_form=1)
    assert fm.factored and all(fm.factored_blocks)
    assert [sorted(s) for s in fm.stored] == [sorted(s) for s in stored_sets(name)]
    return fm


class ScaledFactorOperator:
    """MyA in float64 in the algebra of the device under cg_factored: per block Y = W V once, then
    N = -Y diag(d o x) Y' (lower triangle, mirrored) = W mat(AA' x) W and (Ax)_k = -sum_p d_kp v_kp' N v_kp (scaled = True, a
    pure block), or M = -V diag(d o x) V', Z = (W M) W and the same quadratic forms (the composition).  A stored constraint
    (hybrid block) has no factor column: its part of M comes from its entries, added to the ONE matrix Z is formed from,
    and its row of the result is <A_s, Z> over the entries."""

    def __init__(self, case, stored, scaled):
        self.case, self.blocks = case, []
        n = case.model.n
        for i, facs in enumerate(case.factors):
            st = sorted(stored[i])
            keep = [k for k in range(n) if k not in st]
            V = np.concatenate([facs[k][0] for k in keep], axis=1)
            d = np.concatenate([facs[k][1] for k in keep])
            own = np.repeat(np.asarray(keep), [facs[k][0].shape[1] for k in keep])
            As = [np.asarray(case.model.A[i][k + 1].todense()) for k in st]
            W = case.W[i]
            self.blocks.append((V, d, own, W, st, As, (W @ V) if (scaled and not st) else None))

    def __call__(self, Ax, x):
        y = np.zeros_like(x)
        for V, d, own, W, st, As, Y in self.blocks:
            if Y is not None:
                Z = -(Y * (d * x[own])) @ Y.T
                Z = np.tril(Z) + np.tril(Z, -1).T
            else:
                M = -(V * (d * x[own])) @ V.T
                M = np.tril(M) + np.tril(M, -1).T
                for k, A in zip(st, As):
                    M = M - x[k] * A
                Z = (W @ M) @ W
            np.add.at(y, own, -d * np.einsum("ij,ij->j", Z @ V, V))
            for k, A in zip(st, As):
                y[k] -= float(np.sum(A * Z))
        m = self.case.model
        if m.nlin > 0:
            y += m.C_lin @ ((self.case.X_lin * self.case.S_lin_inv) * (m.C_lin.T @ x))
        Ax[:] = y
