"""Inputs of tests/test_model_layout_cpu.py (and of the upload tests of tests/test_gpu_failure_paths.py): the arguments of
lrn_upload_model, lrn_upload_lowrank and lrn_upload_diag for blocks small enough to check by eye, each built for one branch
of the layout planner (csrc/model_layout.h) that no golden file reaches.

block(name) is (m, AA, sigma, nvar): AA a scipy CSC matrix nvar x m^2 whose STORED entries are the input (an explicit zero
stays stored), sigma 0-based and sorted by decreasing count of non-zeros as lrn_upload_model demands.

  zero        a stored explicit zero: dropped from nnz, ent_* and cq_*
  empty       a constraint with no entry: npos_nz < nvar
  wave45      nnz 5, 5, 4, 4, 1: the q_wave boundary lies between 5 and 4
  unsym       an entry (1, 0) without (0, 1): sp_ok false
  cross       constraint 0 holds (2, 0) only, constraint 1 holds (0, 2) only: sp_ok true, pc_t points across
  long66      side 66: pattern column 0 has 65 stored rows, column 1 has 64 (and their transposes): sp_long_cols = [0]
  two_block   side 5, six constraints, two blocks, constraint 4 of block 0 empty (the GPU upload tests)
"""
import numpy as np
import scipy.sparse as sp


def aa_from(m, nvar, entries):
    """entries: (constraint, row, col, value of AA) -- stored as given, an explicit zero included"""
    k, r, c, v = (np.array(x) for x in zip(*entries))
    A = sp.coo_matrix((v.astype(float), (k, r + c * m)), shape=(nvar, m * m)).tocsc()      # (keeps stored zeros)
    A.sort_indices()
    return A


def sigma_for(AA):
    """a valid sigmaA: constraints by decreasing number of non-zero entries, ties by number"""
    R = sp.csr_matrix(AA)
    cnt = np.array([np.count_nonzero(R.data[R.indptr[i]:R.indptr[i + 1]]) for i in range(R.shape[0])])
    return np.argsort(-cnt, kind="stable").astype(np.int64)


def sym(k, r, c, v):
    return [(k, r, c, v)] + ([(k, c, r, v)] if r != c else [])


def block(name):
    if name == "zero":
        m, nvar = 4, 3
        e = sym(0, 0, 0, 1.5) + sym(0, 2, 1, -2.0) + sym(1, 3, 3, 0.5) + [(1, 1, 1, 0.0)] + sym(2, 3, 0, 4.0) + sym(2, 2, 2, -1.0)
    elif name == "empty":
        m, nvar = 3, 4
        e = sym(0, 0, 0, 1.0) + sym(0, 1, 0, 2.0) + sym(3, 2, 2, -3.0)
    elif name == "wave45":
        m, nvar = 5, 5
        e = []
        for k, n in enumerate([4, 5, 1, 5, 4]):      # diagonal entries; a count of 5 is three of them and one symmetric pair
            e += [(k, i, i, 1.0 + k + i) for i in range(3 if n == 5 else n)]
            if n == 5:
                e += sym(k, 4, k % 3, -0.25 * (k + 1))
    elif name == "unsym":
        m, nvar = 3, 2
        e = [(0, 1, 0, 2.0), (0, 0, 0, 1.0), (1, 2, 2, 3.0)]
    elif name == "cross":
        m, nvar = 3, 2
        e = [(0, 2, 0, 1.25), (0, 1, 1, 1.0), (1, 0, 2, -0.75)]
    elif name == "long66":
        m, nvar = 66, 8
        e = []
        for r in range(1, 66):                         # column 0: rows 1 .. 65 (65 entries); its transposes in row 0
            e += sym(r % nvar, r, 0, 1.0 + r)
        for r in range(2, 65):                         # column 1: rows 0 (above) and 2 .. 64 = 64 entries
            e += sym((r + 3) % nvar, r, 1, -1.0 - r)
    else:
        raise KeyError(name)
    AA = aa_from(m, nvar, e)
    return m, AA, sigma_for(AA), nvar


BLOCKS = ["zero", "empty", "wave45", "unsym", "cross", "long66"]


def two_block():
    """side 5, six constraints, two blocks; block 0: constraints of 9, 7, 5, 3, 0 (number 4) and 1 entries, symmetric;
    block 1: three entries each.  With dense_threshold = 5 block 0 stores positions 0 .. 2 dense (0 < nd = 3 < npos_nz = 5)"""
    m, nvar = 5, 6
    rng = np.random.default_rng(11)
    e0 = []
    for k, n in zip(range(6), [9, 7, 5, 3, 0, 1]):
        e0 += [(k, i, i, float(rng.integers(1, 9))) for i in range(1 if n else 0)]
        pairs = [(1, 0), (2, 0), (3, 1), (4, 2)][:(n - 1) // 2] if n else []
        for r, c in pairs:
            e0 += sym(k, r, c, float(rng.integers(-9, 0)))
    e1 = []
    for k in range(6):
        e1 += [(k, k % 5, k % 5, 2.0 + k)] + sym(k, (k + 1) % 5, (k + 3) % 5, -1.0 - k)
    AA = [aa_from(m, nvar, e0), aa_from(m, nvar, e1)]
    sigma = np.stack([sigma_for(a) for a in AA], axis=1)
    qA = np.array([[nvar, nvar], [0, 0]], dtype=np.int64)
    return AA, sigma, qA, [m, m]


def lowrank_case(nvar, m, khat, seed, zero_weight=1):
    """V ((nvar khat) x m, about half full), d = +-1 with the columns of constraint `zero_weight` all of weight 0"""
    rng = np.random.default_rng(seed)
    V = sp.random(nvar * khat, m, density=0.5, random_state=rng, data_rvs=lambda n: rng.integers(1, 8, n).astype(float)).tocsc()
    d = rng.choice([-1.0, 1.0], nvar * khat)
    d[zero_weight * khat:(zero_weight + 1) * khat] = 0.0
    return V, d


def linear_case(nvar, nlin, seed):
    rng = np.random.default_rng(seed)
    C = sp.random(nvar, nlin, density=0.5, random_state=rng, data_rvs=lambda n: rng.integers(1, 8, n) / 4.0).tocsc()
    C.sort_indices()
    return C
