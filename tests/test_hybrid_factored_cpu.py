"""Hybrid factored blocks on the host (no GPU): build_factored_model with a few STORED constraints among the factors -- rows
of AA for the stored constraints only, stored positions first in sigmaA, weight-0 padding, ||AA_i||_F of both parts --, a
model without stored entries field by field, input checks, the auto rule on a hybrid block, kit = 1, and the generator's
stored= argument against brute force."""
import numpy as np
import pytest
import scipy.sparse as sp

from loraine_jl_amd.model import build_factored_model, build_model, factors_fro, pad_factors
from loraine_jl_amd.optimizer import Optimizer
from loraine_jl_amd.solvers import _dense, _fro
from loraine_jl_amd.synthetic import FactoredLowRankProblem


def _factors(m, n, khat, seed):
    rng = np.random.default_rng(seed)
    facs = []
    for k in range(n):
        r = int(rng.integers(0, khat + 1)) if k % 4 else khat
        facs.append((rng.standard_normal((m, r)) / np.sqrt(m), rng.choice([-1.0, 1.0], size=r)))
    return facs


def _tridiag(m):
    return sp.diags([np.ones(m - 1), 2.0 * np.ones(m), np.ones(m - 1)], [-1, 0, 1], format="csc")


def _few(m):
    A = sp.lil_matrix((m, m))
    A[1, 3] = A[3, 1] = 0.5
    A[2, 2] = -1.5
    return A.tocsc()


def _dense_sym(m, seed):
    R = np.random.default_rng(seed).standard_normal((m, m))
    return 0.5 * (R + R.T)


def _matrix(item):
    if sp.issparse(item):
        return sp.csc_matrix(item)
    if isinstance(item, np.ndarray):
        return sp.csc_matrix(item)
    V, d = item
    a = (V * d) @ V.T
    return sp.csc_matrix(0.5 * (a + a.T))


def _materialised(F0, blocks, n, kappa=8):
    A = [[sp.csc_matrix(F)] + [_matrix(it) for it in blk] for F, blk in zip(F0, blocks)]
    return build_model(A, np.zeros(n), kappa=kappa)


def test_hybrid_layout_and_norm():
    m, n, khat = 20, 13, 4
    mixed = list(_factors(m, n, khat, 5))
    stored = {0: sp.identity(m, format="csc"), 6: _few(m), 9: _dense_sym(m, 1), 12: _tridiag(m)}
    for k, a in stored.items():
        mixed[k] = a
    F0 = [-np.eye(m)]
    fm = build_factored_model(F0, [mixed], np.zeros(n), factored_form=1)
    mm = _materialised(F0, [mixed], n)
    assert fm.factored and fm.from_factors and fm.factored_blocks == [True]
    assert len(fm.A[0]) == 1 and sorted(fm.stored[0]) == sorted(stored)
    for k, a in stored.items():
        assert (fm.stored[0][k] != sp.csc_matrix(a)).nnz == 0
    # rows of AA for the stored constraints only, each -vec(A) as in the materialised model
    AA = fm.AA[0].tocsr()
    assert AA.shape == (n, m * m)
    for k in range(n):
        if k in stored:
            assert (AA[k] != mm.AA[0].tocsr()[k]).nnz == 0 and AA[k].nnz == sp.csc_matrix(stored[k]).nnz
        else:
            assert AA[k].nnz == 0
    assert np.array_equal(fm.nzA[:, 0], [sp.csc_matrix(stored[k]).nnz if k in stored else 0 for k in range(n)])
    # stable sort by nnz, descending: stored positions first (dense, tridiagonal, identity, the small one), then the
    # factored constraints in their natural order
    assert list(fm.sigmaA[:4, 0]) == [9, 12, 0, 6]
    assert list(fm.sigmaA[4:, 0]) == [k for k in range(n) if k not in stored]
    assert fm.qA[0, 0] == fm.qA[1, 0] == 3                  # kappa = 8: the first position with nnz <= 8 is the small matrix
    # weight-0 padding for the stored constraints, the factors of the others untouched
    V, d, kh = fm.lowrank[0]
    assert kh == khat
    ref = [(np.zeros((m, 0)), np.zeros(0)) if k in stored else it for k, it in enumerate(mixed)]
    Vr, dr, _ = pad_factors(ref, n, m)
    assert np.array_equal(d, dr) and (V != Vr).nnz == 0
    for k in stored:
        assert not d[k * kh:(k + 1) * kh].any() and V[k * kh:(k + 1) * kh].nnz == 0
    assert fm.aa_fro[0] == pytest.approx(_fro(mm.AA[0]), rel=1e-12)
    assert np.array_equal(_dense(fm.C[0]), np.eye(m))


def test_model_without_stored_entries_is_unchanged():
    n = 11
    b0, b1 = _factors(14, n, 2, 1), _factors(9, n, 4, 2)
    F0 = [-np.eye(14), sp.csc_matrix(-2.0 * np.eye(9))]
    C_lin = sp.random(n, 3, density=0.5, random_state=4, format="csr")
    fm = build_factored_model(F0, [b0, b1], np.arange(n, dtype=float), 1.5, np.ones(3), C_lin, factored_form=1)
    assert fm.factored and fm.from_factors and fm.factored_blocks == [True, True] and fm.stored == [{}, {}]
    assert fm.nlmi == 2 and fm.n == n and fm.nlin == 3 and fm.b_const == 1.5 and list(fm.msizes) == [14, 9]
    assert np.array_equal(fm.b, np.arange(n, dtype=float)) and np.array_equal(fm.d_lin, np.ones(3))
    assert (fm.C_lin != C_lin).nnz == 0 and fm.B == [] and fm.lowrank_note == ""
    assert not fm.nzA.any() and fm.nzA.dtype == np.int64
    assert np.array_equal(fm.qA, np.zeros((2, 2), dtype=np.int64))
    for i, (m, facs) in enumerate(((14, b0), (9, b1))):
        assert fm.AA[i].shape == (n, m * m) and fm.AA[i].nnz == 0 and len(fm.A[i]) == 1
        assert np.array_equal(fm.sigmaA[:, i], np.arange(n))
        V, d, kh = fm.lowrank[i]
        Vr, dr, khr = pad_factors(facs, n, m)
        assert kh == khr and np.array_equal(d, dr) and (V != Vr).nnz == 0
        assert fm.aa_fro[i] == factors_fro(Vr, dr, khr, n)
    assert np.array_equal(fm.C[0], np.eye(14)) and (fm.C[1] != sp.csc_matrix(2.0 * np.eye(9))).nnz == 0


def test_bad_stored_input_raises():
    m, n = 10, 6
    facs = _factors(m, n, 2, 3)
    F0 = [-np.eye(m)]
    wrong = list(facs)
    wrong[2] = sp.identity(m + 1, format="csc")
    with pytest.raises(ValueError, match="side"):
        build_factored_model(F0, [wrong], np.zeros(n))
    wrong[2] = np.ones((m, m - 1))
    with pytest.raises(ValueError, match="side"):
        build_factored_model(F0, [wrong], np.zeros(n))
    skew = list(facs)
    a = np.zeros((m, m))
    a[1, 4] = 1.0
    skew[0] = a
    with pytest.raises(ValueError, match="symmetric"):
        build_factored_model(F0, [skew], np.zeros(n))
    skew[0] = sp.csc_matrix(a)
    with pytest.raises(ValueError, match="symmetric"):
        build_factored_model(F0, [skew], np.zeros(n), factored_form=1)
    flat = list(facs)
    flat[1] = np.ones(m)
    with pytest.raises(ValueError, match="2-D"):
        build_factored_model(F0, [flat], np.zeros(n))


def test_auto_rule_materialises_a_hybrid_block_of_unit_vectors():
    m = n = 30
    mixed = [(np.eye(m)[:, [k]], np.ones(1)) for k in range(n)]
    mixed[0] = sp.identity(m, format="csc")
    mixed[11] = _tridiag(m)
    mixed[29] = _dense_sym(m, 2)
    F0 = [sp.csc_matrix(_tridiag(m))]
    fm = build_factored_model(F0, [mixed], np.ones(n))
    mm = _materialised(F0, [mixed], n)
    assert not fm.factored and fm.from_factors and fm.factored_blocks == [False] and fm.stored == [{}]
    assert (fm.AA[0] != mm.AA[0]).nnz == 0
    assert np.array_equal(fm.nzA, mm.nzA) and np.array_equal(fm.sigmaA, mm.sigmaA) and np.array_equal(fm.qA, mm.qA)
    assert len(fm.A[0]) == n + 1
    for k in range(n + 1):
        assert (fm.A[0][k] != mm.A[0][k]).nnz == 0
    assert (fm.C[0] != mm.C[0]).nnz == 0
    assert fm.aa_fro[0] == pytest.approx(_fro(mm.AA[0]), rel=1e-12)
    # forced: hybrid
    ff = build_factored_model(F0, [mixed], np.ones(n), factored_form=1)
    assert ff.factored and sorted(ff.stored[0]) == [0, 11, 29] and ff.AA[0].nnz == m + (3 * m - 2) + m * m
    # dense factors beside the stored matrices stay factored under the auto rule
    dense = list(_factors(m, n, 2, 5))
    dense[3] = sp.identity(m, format="csc")
    fd = build_factored_model(F0, [dense], np.ones(n))
    assert fd.factored and sorted(fd.stored[0]) == [3] and fd.AA[0].nnz == m


def test_kit_1_still_raises_for_a_hybrid_model():
    m, n = 12, 7
    mixed = list(_factors(m, n, 2, 9))
    mixed[4] = sp.identity(m, format="csc")
    with pytest.raises(ValueError, match="resident"):
        Optimizer(resident=False).load_factored_model([-np.eye(m)], [mixed], np.ones(n))
    o = Optimizer()
    o.set_silent(True)
    o.set_attribute("kit", 1)
    o.load_factored_model([-np.eye(m)], [mixed], np.ones(n), factored_form=1)
    with pytest.raises(ValueError, match="kit = 0"):
        o.optimize()
    assert o.solver is None


def test_generator_with_stored_constraints_against_brute_force():
    m, n = 20, 15
    stored = [(0, sp.identity(m, format="csc")), (7, _few(m)), (14, _tridiag(m))]
    P0 = FactoredLowRankProblem(m, n, 2, 3, seed=4)
    P = FactoredLowRankProblem(m, n, 2, 3, seed=4, stored=stored)
    # the draws do not depend on the argument
    for name in ("V", "d", "Q", "lam", "ystar"):
        assert np.array_equal(getattr(P, name), getattr(P0, name)), name
    keep = [k for k in range(n) if k not in (0, 7, 14)]
    assert np.array_equal(P.b[keep], P0.b[keep])
    # b and C from the definition
    X = (P.Q * P.lam) @ P.Q.T
    A = [P.constraint(k) for k in range(n)]
    for k, a in stored:
        assert np.array_equal(A[k], a.toarray())
    b = -np.array([np.sum(a * X) for a in A])
    assert np.allclose(P.b, b, rtol=1e-12, atol=1e-14)
    C = np.eye(m) - P.Q @ P.Q.T - sum(y * a for y, a in zip(P.ystar, A))
    assert np.allclose(P.C_dense(), C, rtol=1e-12, atol=1e-14)
    assert np.array_equal(P.F0()[0], -P.C_dense())
    assert P.optimum == pytest.approx(float(b @ P.ystar), rel=1e-12)
    fac = P.factors()[0]
    assert len(fac) == n and all(sp.issparse(fac[k]) for k in (0, 7, 14)) and all(isinstance(fac[k], tuple) for k in keep)
    fm = build_factored_model(P.F0(), P.factors(), P.b)
    assert fm.factored and sorted(fm.stored[0]) == [0, 7, 14]
    # without the argument nothing moves: the numbers tests/test_gpu_factored.py solves for
    Q0 = FactoredLowRankProblem(m, n, 2, 3, seed=4, stored=None)
    assert np.array_equal(Q0.b, P0.b) and Q0.optimum == P0.optimum and np.array_equal(Q0.C_dense(), P0.C_dense())
    assert all(isinstance(f, tuple) for f in Q0.factors()[0])
    assert P0.optimum == pytest.approx(0.06902829094129755, rel=1e-12)       # (recorded before the argument existed)
