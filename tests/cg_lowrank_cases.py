"""Seeded inputs of tests/test_cg_lowrank_cpu.py and tests/test_gpu_cg_lowrank.py: models whose constraints are BUILT from
rank-k factors, A_k = (V_k d_k) V_k', so that the CG path can run from the factors (option cg_lowrank) and from the entries
of the same AA.  One function for both files, nothing committed as a fixture; the reference is oracle/cg_reference.py
as it stands.

Per block the ranks cycle through 1 .. kmax (padding columns of weight 0 exist whenever kmax is no power of two or a
constraint has a lower rank), the signs are +-1 at random.  Three constraints of four have a dense V scaled by 1/sqrt(m):
m^2 entries, dense slots.  Every fourth has a V supported on two rows, rank 1 or 2, on an index pair of its own: four
entries, sparse slots -- so sigmaA is not the identity.  (Repeated index pairs make such constraints nearly dependent:
cond(H) goes to 1e10, where a float64 CG says nothing.)

  L1  msz 37, nvar 130, kmax 3 -> khat 4                 one block, position space
  L2  msz 33 + 18, nvar 257, khat 2 and 1, 5 linear rows  two blocks, has_LD, two CG workgroups
  L3  msz 70, nvar 65, khat 1                             tile edges just past 64 in both directions of the transpose
"""
import functools
import types

import numpy as np
import scipy.sparse as sp

from oracle import cg_reference as cr
from oracle import loraine_oracle as lo

# name -> (msizes, nvar, kmax per block, nlin, seed)
SHAPES = {
    "L1": ([37], 130, [3], 0, 321),                  # (seed 311: the factor-form float64 recurrence is 24 x the oracle's distance)
    "L2": ([33, 18], 257, [2, 1], 5, 322),           # (seed 312: no gap with a well-determined iterate under H_alpha, erank 1)
    "L3": ([70], 65, [1], 0, 313),
}
PRECS = [(0, 1), (2, 1), (1, 1), (1, 2)]


def _block_factors(m, nvar, kmax, rng):
    """[(V (m x r), d (r))] * nvar as the module docstring describes."""
    iu, ju = np.triu_indices(m, 1)
    pairs = rng.permutation(iu.size)
    assert pairs.size >= (nvar + 3) // 4                       # pairwise distinct index pairs
    facs = []
    for j in range(nvar):
        if j % 4 == 3:
            r = min(kmax, 1 + (j // 4) % 2)
            V = np.zeros((m, r))
            q = pairs[j // 4]
            M = rng.uniform(0.5, 1.5, (2, r))
            if r == 2:
                M[1, 1] = -M[1, 1]                             # (det < 0: two independent columns on the two rows)
            V[[iu[q], ju[q]], :] = M * rng.choice([-1.0, 1.0], (1, r))
        else:
            r = 1 + j % kmax
            V = rng.standard_normal((m, r)) / np.sqrt(m)
        facs.append((V, rng.choice([-1.0, 1.0], size=r)))
    return facs


def _matrices(facs):
    out = []
    for V, d in facs:
        a = (V * d) @ V.T
        out.append(sp.csc_matrix(0.5 * (a + a.T)))
    return out


def build_case(name, seed=None):
    """model (oracle MyModel), factors (per block [(V, d)]), lowrank (per block (V, d, khat) as Device.upload_lowrank takes
    them, from the host's own factor check), W, G, X_lin, S_lin_inv, right-hand side h, a vector x."""
    from loraine_jl_amd.model import user_factors
    msizes, nvar, kmax, nlin, seed0 = SHAPES[name]
    seed = seed0 if seed is None else seed
    rng = np.random.default_rng(seed)
    factors = [_block_factors(m, nvar, k, rng) for m, k in zip(msizes, kmax)]
    A = []
    for m, facs in zip(msizes, factors):
        C0 = rng.standard_normal((m, m))
        A.append([sp.csc_matrix(-(C0 + C0.T) / 2)] + _matrices(facs))
    C_lin = d_lin = None
    if nlin > 0:
        C_lin = sp.csr_matrix(sp.random(nvar, nlin, density=0.06, random_state=rng, data_rvs=rng.standard_normal))
        d_lin = rng.standard_normal(nlin)
    model = lo.make_model(A, rng.standard_normal(nvar), 0.0, d_lin, C_lin)
    lowrank = user_factors(model.A, nvar, factors)            # raises ValueError for a factor that misses its A_k
    rng = np.random.default_rng(seed + 1000)
    W, G = [], []
    for m in msizes:
        Wb, Gb = cr.scaling_from_spectrum(cr.spectrum(m, top=min(4, m - 1)), rng)
        W.append(Wb)
        G.append(Gb)
    X_lin = np.exp(rng.uniform(-1.0, 1.0, model.nlin))
    S_lin_inv = np.exp(rng.uniform(-1.0, 1.0, model.nlin))
    x = rng.standard_normal(nvar)
    case = types.SimpleNamespace(name=name, model=model, factors=factors, lowrank=lowrank, W=W, G=G, X_lin=X_lin,
                                 S_lin_inv=S_lin_inv, h=None, x=x)
    h = np.zeros(nvar)                                        # h = H v: in the range of the large eigenvalues, as in cr.build_case
    lo.MyA(W, model.AA, model.nlin, model.C_lin, X_lin, S_lin_inv)(h, rng.standard_normal(nvar))
    case.h = h
    return case


class FactorFormOperator:
    """MyA in float64 with the ALGEBRA of the factor form (NumPy, no device): M = -V diag(d o x) V' (lower triangle,
    mirrored), Z = W M W, (Ax)_k = -sum_p d_kp v_kp' Z v_kp, plus the linear term.  Its factors are not bit for bit the
    entries of AA (A_k was rounded after the product), and its sums run in another order than lo.MyA's: how far a float64
    recurrence moves with it is what the factor form costs on an input, whatever device runs it."""

    def __init__(self, case):
        self.case, self.blocks = case, []
        for i, facs in enumerate(case.factors):
            V = np.concatenate([v for v, _ in facs], axis=1)
            d = np.concatenate([dd for _, dd in facs])
            own = np.repeat(np.arange(case.model.n), [v.shape[1] for v, _ in facs])
            self.blocks.append((V, d, own, case.W[i]))

    def __call__(self, Ax, x):
        y = np.zeros_like(x)
        for V, d, own, W in self.blocks:
            M = -(V * (d * x[own])) @ V.T
            M = np.tril(M) + np.tril(M, -1).T
            Q = ((W @ M) @ W) @ V
            np.add.at(y, own, -d * np.einsum("ij,ij->j", Q, V))
        m = self.case.model
        if m.nlin > 0:
            y += m.C_lin @ ((self.case.X_lin * self.case.S_lin_inv) * (m.C_lin.T @ x))
        Ax[:] = y


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """Built once per process, shared by every test that needs it, never modified."""
    return build_case(name)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(case, dense longdouble H)."""
    case = case_inputs(name)
    return case, cr.dense_operator(case.model, case.W, case.X_lin, case.S_lin_inv)


@functools.lru_cache(maxsize=None)
def case_run(name, prec, erank):
    """History of the longdouble recurrence, the iteration K the tests stop in and its tolerance (cr.reference_run:
    pcg_history twice, choose_K with drift <= cr.DRIFT_MAX, pick_tol)."""
    case, H = case_data(name)
    return cr.reference_run(case, H, prec, erank)
