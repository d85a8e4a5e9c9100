"""Factored constraints with a diagonal part on the host (no GPU): parsing of the (V, d, a) items of build_factored_model and
every ValueError, ||AA_i||_F against the dense norm, the materialised fallback against the definition (and its weight-0
factor columns), the kit = 1 refusal -- and the NumPy restatement of the device's formulas (tests/diag_factored_cases.py)
against tr(A_i W A_j W) for every generator case: the formulas the kernels implement are checked apart from the kernels (the GPU
test compares the device with the definition, mode 0 and the stored-matrix route, not with this restatement)."""
import numpy as np
import pytest
import scipy.sparse as sp

import diag_factored_cases as dc
from loraine_jl_amd.model import build_factored_model, build_model, check_diag_kit
from loraine_jl_amd.optimizer import Optimizer
from loraine_jl_amd.solvers import _fro


def relerr(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _materialised(F0, blocks, n, kappa=8):
    A = [[sp.csc_matrix(F)] + [sp.csc_matrix(dc.dense_of(it)) for it in blk] for F, blk in zip(F0, blocks)]
    return build_model(A, np.zeros(n), kappa=kappa)


def test_items_are_parsed():
    m, n = 12, 6
    rng = np.random.default_rng(1)
    V = rng.standard_normal((m, 2))
    d = np.array([1.0, -1.0])
    a = dc._diagonal(m, 3)
    items = [(V, d, a), (None, [], np.ones(m)), (V, d), (V[:, 0], [1.0], np.zeros(m)), sp.identity(m, format="csc"),
             (sp.csc_matrix(V), d, sp.csc_matrix(a.reshape(-1, 1)))]
    fm = build_factored_model([-np.eye(m)], [items], np.zeros(n), factored_form=1)
    assert fm.factored and fm.factored_blocks == [True] and sorted(fm.stored[0]) == [4]
    assert sorted(fm.diag[0]) == [0, 1, 5]                      # (an all-zero diagonal is the pair (V, d))
    assert np.array_equal(fm.diag[0][0], a) and np.array_equal(fm.diag[0][1], np.ones(m)) and np.array_equal(fm.diag[0][5], a)
    Vp, dp, kh = fm.lowrank[0]
    assert kh == 2 and list(dp) == [1, -1, 0, 0, 1, -1, 1, 0, 0, 0, 1, -1]
    assert Vp[2:4].nnz == 0 and np.array_equal(Vp[0:2].toarray(), V.T) and np.array_equal(Vp[6].toarray().ravel(), V[:, 0])
    # the layout of a model without diagonal parts does not move
    plain = build_factored_model([-np.eye(m)], [[(V, d)] * n], np.zeros(n), factored_form=1)
    assert plain.diag == [{}] and plain.stored == [{}]


def test_bad_items_raise():
    m, n = 10, 3
    facs = dc._factors(m, n, 2, 3)
    F0 = [-np.eye(m)]

    def build(item, at=1):
        blk = list(facs)
        blk[at] = item
        return build_factored_model(F0, [blk], np.zeros(n))

    V, d = facs[0]
    with pytest.raises(ValueError, match=r"block 1, constraint 2: the diagonal part has 9 entries"):
        build((V, d, np.ones(m - 1)))
    with pytest.raises(ValueError, match=r"block 1, constraint 3: the diagonal part has a non-finite"):
        build((V, d, np.r_[np.ones(m - 1), np.nan]), at=2)
    with pytest.raises(ValueError, match=r"block 1, constraint 2: the diagonal part has a non-finite"):
        build((None, [], np.r_[np.inf, np.ones(m - 1)]))
    with pytest.raises(ValueError, match="factor columns"):
        build((None, [1.0], np.ones(m)))                       # weights without columns
    with pytest.raises(ValueError, match="side"):
        build((np.ones((m + 1, 1)), [1.0], np.ones(m)))
    with pytest.raises(ValueError, match="2-D"):                # a bare vector is not a diagonal part
        build(np.ones(m))


@pytest.mark.parametrize("m,n,khat,count", dc.CASES)
def test_aa_fro_is_the_dense_norm(m, n, khat, count):
    items = dc.block_items(m, n, khat, count, 100 * m + n)
    fm = build_factored_model([-np.eye(m)], [items], np.zeros(n), factored_form=1)
    assert fm.factored and sorted(fm.diag[0]) == dc.diag_rows(n, count)
    ref = np.sqrt(sum(np.sum(dc.dense_of(it) ** 2) for it in items))
    assert fm.aa_fro[0] == pytest.approx(ref, rel=1e-12)


def test_materialised_fallback_is_the_definition():
    """Unit-vector factors with diagonal parts of a few entries: the auto rule materialises the block; the constraints are the
    sparse sums, the sum rows have weight-0 factor columns (their entries carry them whole) and the model has no diag."""
    m = n = 24
    rng = np.random.default_rng(5)
    items = [(np.eye(m)[:, [k]], np.ones(1)) for k in range(n)]
    sparse_a = np.zeros(m)
    sparse_a[[2, 7]] = [1.5, -0.5]
    items[3] = (np.eye(m)[:, [3]], -np.ones(1), sparse_a)
    items[9] = (None, [], np.r_[np.ones(3), np.zeros(m - 3)])
    items[20] = sp.identity(m, format="csc")
    F0 = [-np.eye(m)]
    fm = build_factored_model(F0, [items], np.ones(n))
    mm = _materialised(F0, [items], n)
    assert not fm.factored and fm.factored_blocks == [False] and fm.diag == [{}] and fm.stored == [{}]
    assert (fm.AA[0] != mm.AA[0]).nnz == 0 and np.array_equal(fm.sigmaA, mm.sigmaA) and np.array_equal(fm.qA, mm.qA)
    for k in range(n + 1):
        assert (fm.A[0][k] != mm.A[0][k]).nnz == 0
    assert fm.aa_fro[0] == pytest.approx(_fro(mm.AA[0]), rel=1e-12)
    V, d, kh = fm.lowrank[0]
    for k in (3, 9, 20):
        assert not d[k * kh:(k + 1) * kh].any() and V[k * kh:(k + 1) * kh].nnz == 0
    assert all(d[k * kh] == 1.0 for k in range(n) if k not in (3, 9, 20))
    check_diag_kit(fm, 1)                                       # nothing to refuse: the entries hold the diagonal parts
    # the count: nnz(a) joins sum nnz(V_k V_k'); a dense diagonal part on every constraint keeps the block factored
    dense = [(np.eye(m)[:, [k]], np.ones(1), rng.standard_normal(m)) for k in range(n)]
    fd = build_factored_model(F0, [dense], np.ones(n))
    assert fd.factored and sorted(fd.diag[0]) == list(range(n))
    # forced: factored, with the parts in diag
    ff = build_factored_model(F0, [items], np.ones(n), factored_form=1)
    assert ff.factored and sorted(ff.diag[0]) == [3, 9] and sorted(ff.stored[0]) == [20]
    assert ff.aa_fro[0] == pytest.approx(_fro(mm.AA[0]), rel=1e-12)


def test_kit_1_raises_before_a_device_is_opened():
    m, n = 12, 7
    items = list(dc._factors(m, n, 2, 9))
    items[4] = (None, [], np.ones(m))
    for cg in (False, True):
        o = Optimizer()
        o.set_silent(True)
        o.set_attribute("kit", 1)
        o.load_factored_model([-np.eye(m)], [items], np.ones(n), factored_form=1, cg=cg)
        with pytest.raises(ValueError, match="diagonal parts" if cg else "kit = 0"):
            o.optimize()
        assert o.solver is None
    fm = build_factored_model([-np.eye(m)], [items], np.ones(n), factored_form=1)
    fm.factored_cg = True
    with pytest.raises(ValueError, match="diagonal parts"):
        check_diag_kit(fm, 1)
    check_diag_kit(fm, 0)


@pytest.mark.parametrize("stored", [True, False])
@pytest.mark.parametrize("m,n,khat,count", dc.CASES)
def test_device_formulas_against_the_definition(m, n, khat, count, stored):
    items = dc.block_items(m, n, khat, count, 100 * m + n, stored=stored)
    assert sum(1 for it in items if isinstance(it, tuple) and len(it) == 3) == count
    W, _ = dc.spd(m, 6 + m)
    Hdef = dc.h_definition([dc.dense_of(it) for it in items], W)
    assert relerr(dc.h_formulas(items, W), Hdef) < 1e-12
    # the stored-matrix route of the same data is the same matrix
    again = dc.diag_as_stored(items)
    assert all(not (isinstance(it, tuple) and len(it) == 3) for it in again)
    assert relerr(dc.h_definition([dc.dense_of(it) for it in again], W), Hdef) < 1e-14


def test_data_operators_against_the_definition():
    """y_k = -<A_k, Z> and M = -sum_k x_k A_k split as the device splits them: factor form, stored rows, diagonal parts."""
    m, n, khat, count = 33, 37, 2, 3
    items = dc.block_items(m, n, khat, count, 7)
    Z = dc.sym(m, 1)
    x = np.random.default_rng(2).standard_normal(n)
    As = [dc.dense_of(it) for it in items]
    y = np.zeros(n)
    M = np.zeros((m, m))
    for k, it in enumerate(items):
        if not isinstance(it, tuple):
            y[k] -= np.sum(it.toarray() * Z)
            M -= x[k] * it.toarray()
            continue
        if it[0] is not None:
            V, d = it[0], np.asarray(it[1])
            y[k] -= np.sum(d * np.einsum("ip,ij,jp->p", V, Z, V))
            M -= x[k] * (V * d) @ V.T
        if len(it) == 3:
            y[k] -= it[2] @ np.diag(Z)
            M[np.diag_indices(m)] -= x[k] * it[2]
    assert relerr(y, -np.array([np.sum(a * Z) for a in As])) < 1e-13
    assert relerr(M, -sum(xk * a for xk, a in zip(x, As))) < 1e-13
