"""Factor-only models on the host (no GPU): build_factored_model -- AA without entries, identity sigmaA, the same padded
factors build_model(..., factors=) produces -- the factor formula for ||AA_i||_F, input checks, the auto rule that
materialises tiny factors, and the ValueErrors of kit = 1 / resident=False (raised before any device is opened)."""
import numpy as np
import pytest
import scipy.sparse as sp

from loraine_jl_amd.model import build_factored_model, build_model, factors_fro
from loraine_jl_amd.optimizer import Optimizer
from loraine_jl_amd.solvers import _dense, _fro


def _factors(m, n, khat, seed, sparse=False):
    """Random signed factors of rank 0 .. khat (mixed), sparse (3 entries per column) or dense."""
    rng = np.random.default_rng(seed)
    facs = []
    for k in range(n):
        r = int(rng.integers(0, khat + 1)) if k % 4 else khat
        if sparse:
            V = np.zeros((m, r))
            for p in range(r):
                V[rng.choice(m, size=min(3, m), replace=False), p] = rng.standard_normal(min(3, m))
        else:
            V = rng.standard_normal((m, r)) / np.sqrt(m)
        facs.append((V, rng.choice([-1.0, 1.0], size=r)))
    return facs


def _materialised(F0, blocks, n):
    A = []
    for F, facs in zip(F0, blocks):
        blk = [sp.csc_matrix(F)]
        for V, d in facs:
            a = (V * d) @ V.T
            blk.append(sp.csc_matrix(0.5 * (a + a.T)))
        A.append(blk)
    return build_model(A, np.zeros(n), factors=blocks)


@pytest.mark.parametrize("m,n,khat,sparse", [(12, 9, 1, False), (20, 13, 4, False), (33, 10, 16, False), (25, 17, 2, True)])
def test_factored_model_layout_and_norm(m, n, khat, sparse):
    facs = _factors(m, n, khat, 7 * m + n, sparse)
    F0 = [-np.eye(m)]
    fm = build_factored_model(F0, [facs], np.zeros(n), factored_form=1)
    mm = _materialised(F0, [facs], n)
    assert fm.factored and fm.from_factors and fm.factored_blocks == [True]
    assert fm.nlmi == 1 and fm.n == n and list(fm.msizes) == [m]
    assert fm.AA[0].shape == (n, m * m) and fm.AA[0].nnz == 0
    assert not fm.nzA.any()
    assert np.array_equal(fm.sigmaA[:, 0], np.arange(n))
    assert len(fm.A[0]) == 1                                   # F_0 only
    assert np.array_equal(_dense(fm.C[0]), mm.C[0].toarray())
    V, d, kh = fm.lowrank[0]
    Vm, dm, khm = mm.lowrank[0]
    assert kh == khm == khat
    assert np.array_equal(d, dm) and (V != Vm).nnz == 0
    # ||AA_i||_F from the khat x khat Gram matrices against the materialised rows
    ref = _fro(mm.AA[0])
    assert fm.aa_fro[0] == pytest.approx(ref, rel=1e-12)
    assert factors_fro(V, d, kh, n, chunk=4) == pytest.approx(ref, rel=1e-12)


def test_sparse_factor_input_and_two_blocks():
    n = 11
    b0, b1 = _factors(14, n, 2, 1), _factors(9, n, 4, 2, sparse=True)
    b1s = [(sp.csc_matrix(V), d) for V, d in b1]
    F0 = [-np.eye(14), sp.csc_matrix(-2.0 * np.eye(9))]
    C_lin = sp.random(n, 3, density=0.5, random_state=4, format="csr")
    fm = build_factored_model(F0, [b0, b1s], np.arange(n, dtype=float), 1.5, np.ones(3), C_lin, factored_form=1)
    mm = _materialised(F0, [b0, b1], n)
    assert fm.factored_blocks == [True, True] and fm.nlin == 3 and fm.b_const == 1.5
    for i in range(2):
        assert (fm.lowrank[i][0] != mm.lowrank[i][0]).nnz == 0
        assert fm.aa_fro[i] == pytest.approx(_fro(mm.AA[i]), rel=1e-12)
    assert np.array_equal(fm.qA, np.zeros((2, 2), dtype=np.int64))


def test_bad_input_raises():
    m, n = 10, 6
    facs = _factors(m, n, 2, 3)
    F0 = [-np.eye(m)]
    with pytest.raises(ValueError, match="constraints"):
        build_factored_model(F0, [facs[:-1]], np.zeros(n))
    with pytest.raises(ValueError, match="LMI blocks"):
        build_factored_model(F0, [facs, facs], np.zeros(n))
    wide = list(facs)
    wide[2] = (np.ones((m, 17)), np.ones(17))
    with pytest.raises(ValueError, match="at most 16"):
        build_factored_model(F0, [wide], np.zeros(n))
    short = list(facs)
    short[1] = (np.ones((m, 2)), np.ones(3))
    with pytest.raises(ValueError, match="weights"):
        build_factored_model(F0, [short], np.zeros(n))
    tall = list(facs)
    tall[0] = (np.ones((m + 1, 1)), np.ones(1))
    with pytest.raises(ValueError, match="side"):
        build_factored_model(F0, [tall], np.zeros(n))
    with pytest.raises(ValueError, match="factored_form"):
        build_factored_model(F0, [facs], np.zeros(n), factored_form=0)


def test_auto_rule_materialises_unit_vectors_and_keeps_dense_factors():
    """maxG11-like data, A_k = e_k e_k' (one entry each): the sparse path serves it -- the block is materialised and
    equals what build_model makes of the matrices; dense factors stay factored."""
    m = n = 30
    unit = [(np.eye(m)[:, [k]], np.ones(1)) for k in range(n)]
    F0 = [sp.random(m, m, density=0.1, random_state=1)]
    F0 = [sp.csc_matrix(F0[0] + F0[0].T)]
    fm = build_factored_model(F0, [unit], np.ones(n))
    assert not fm.factored and fm.from_factors and fm.factored_blocks == [False]
    mm = _materialised(F0, [unit], n)
    assert (fm.AA[0] != mm.AA[0]).nnz == 0 and fm.AA[0].nnz == n
    assert np.array_equal(fm.nzA, mm.nzA) and np.array_equal(fm.sigmaA, mm.sigmaA) and np.array_equal(fm.qA, mm.qA)
    assert len(fm.A[0]) == n + 1
    assert (fm.lowrank[0][0] != mm.lowrank[0][0]).nnz == 0
    # forced
    ff = build_factored_model(F0, [unit], np.ones(n), factored_form=1)
    assert ff.factored and ff.AA[0].nnz == 0
    # dense factors: m^2 entries per constraint, far above datasparsity
    dense = _factors(m, n, 2, 5)
    fd = build_factored_model(F0, [dense], np.ones(n))
    assert fd.factored and fd.factored_blocks == [True] and fd.AA[0].nnz == 0
    # mixed model: one block of each kind
    fx = build_factored_model([F0[0], F0[0]], [unit, dense], np.ones(n))
    assert fx.factored and fx.factored_blocks == [False, True]
    assert fx.AA[0].nnz == n and fx.AA[1].nnz == 0


def test_kit_1_and_host_loop_raise_before_a_device_is_needed():
    m, n = 12, 7
    facs = _factors(m, n, 2, 9)
    with pytest.raises(ValueError, match="resident"):
        Optimizer(resident=False).load_factored_model([-np.eye(m)], [facs], np.ones(n))
    o = Optimizer()
    o.set_silent(True)
    o.set_attribute("kit", 1)
    o.load_factored_model([-np.eye(m)], [facs], np.ones(n), factored_form=1)
    with pytest.raises(ValueError, match="kit = 0"):
        o.optimize()
    assert o.solver is None
