"""Rank-k constraint data (datarank = k >= 1) on the host: factor detection A_k = V_k diag(d_k) V_k', the padding to khat
columns, the fallback of a model without such a form, and the check of user-supplied factors.  No GPU."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import loraine_jl_amd  # noqa: F401  (alias module for the `loraine.jl_amd/` package)
from loraine_jl_amd import model as lm

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _signed(m, r, signs, seed):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((m, r))
    d = np.asarray(signs, dtype=float)
    A = (V * d) @ V.T
    return 0.5 * (A + A.T)


@pytest.mark.parametrize("r,signs", [(1, [1]), (1, [-1]), (2, [1, -1]), (3, [1, -1, -1]), (3, [1, 1, 1])])
def test_detection_reproduces_the_constraint(r, signs):
    m = 23
    A = _signed(m, r, signs, 7 + r)
    f = lm.lowrank_factor(sp.csc_matrix(A), m, 4)
    assert f is not None
    V, d = f
    assert V.shape == (m, r)
    assert sorted(d.tolist()) == sorted(float(s) for s in signs)
    assert np.linalg.norm(A - (V * d) @ V.T) <= lm.LOWRANK_TOL


def test_detection_rejects_a_rank_above_the_limit():
    m = 17
    A = _signed(m, 3, [1, -1, 1], 3)
    assert lm.lowrank_factor(sp.csc_matrix(A), m, 2) is None
    assert lm.lowrank_factor(sp.csc_matrix(A), m, 3) is not None


def test_theta_constraint_has_two_signed_factors():
    """e_i e_j' + e_j e_i' (matrix completion, theta constraints): rank 2 with one positive, one negative eigenvalue."""
    m, i, j = 11, 2, 7
    A = sp.csc_matrix(([1.0, 1.0], ([i, j], [j, i])), shape=(m, m))
    V, d = lm.lowrank_factor(A, m, 2)
    assert sorted(d.tolist()) == [-1.0, 1.0]
    assert np.count_nonzero(np.any(V != 0.0, axis=1)) == 2          # the factors live on the support {i, j}
    assert np.linalg.norm(A.toarray() - (V * d) @ V.T) <= 1e-14
    assert lm.lowrank_factor(A, m, 1) is None


def test_empty_constraint_has_rank_zero():
    V, d = lm.lowrank_factor(sp.csc_matrix((5, 5)), 5, 1)
    assert V.shape == (5, 0) and d.size == 0


def test_padding_to_a_power_of_two():
    m = 9
    rng = np.random.default_rng(1)
    ranks = [1, 3, 0, 2]
    facs = [(rng.standard_normal((m, r)), np.where(np.arange(r) % 2 == 0, 1.0, -1.0)) for r in ranks]
    V, d, khat = lm.pad_factors(facs, len(ranks), m)
    assert khat == 4
    assert V.shape == (len(ranks) * khat, m)
    Vd = V.toarray()
    for k, (Vk, dk) in enumerate(facs):
        r = Vk.shape[1]
        blk = Vd[k * khat:(k + 1) * khat]
        assert np.array_equal(blk[:r], Vk.T)
        assert not blk[r:].any()                                  # padding columns are zero ...
        assert np.array_equal(d[k * khat:k * khat + r], dk)
        assert not d[k * khat + r:(k + 1) * khat].any()           # ... with weight 0
    assert [lm.padded_rank(r) for r in (0, 1, 2, 3, 5, 8, 9, 16)] == [1, 1, 2, 4, 8, 8, 16, 16]


def test_maxG11_datarank_1_is_rank_one():
    model = lm.model_from_sdpa(os.path.join(GOLD, "maxG11.dat-s"), datarank=1)
    assert len(model.lowrank) == 1 and model.lowrank_note == ""
    V, d, khat = model.lowrank[0]
    m = int(model.msizes[0])
    assert khat == 1 and V.shape == (model.n, m)
    for k in range(0, model.n, 97):
        Ak = model.A[0][k + 1].toarray()
        vk = V[k].toarray().ravel()
        assert np.linalg.norm(Ak - d[k] * np.outer(vk, vk)) <= lm.LOWRANK_TOL


def test_theta1_datarank_2_falls_back():
    """The trace constraint I of theta1 has full rank: no rank-2 form, the whole model takes the general path."""
    model = lm.model_from_sdpa(os.path.join(GOLD, "theta1.dat-s"), datarank=2)
    assert model.lowrank == []
    assert "not of rank <= 2" in model.lowrank_note
    plain = lm.model_from_sdpa(os.path.join(GOLD, "theta1.dat-s"), datarank=0)
    assert plain.lowrank == [] and plain.lowrank_note == ""
    for a, b in zip(model.AA, plain.AA):
        assert (a != b).nnz == 0


def test_datarank_above_16_falls_back():
    model = lm.model_from_sdpa(os.path.join(GOLD, "theta1.dat-s"), datarank=17)
    assert model.lowrank == [] and "> 16" in model.lowrank_note


def _small_problem(m=8, n=4, seed=0):
    rng = np.random.default_rng(seed)
    facs, A = [], [sp.csc_matrix(-np.eye(m))]
    for k in range(n):
        r = 1 + k % 3
        V = rng.standard_normal((m, r))
        d = np.where(np.arange(r) % 2 == 0, 1.0, -1.0)
        A.append(sp.csc_matrix(0.5 * ((V * d) @ V.T + ((V * d) @ V.T).T)))
        facs.append((V, d))
    return [A], rng.standard_normal(n), [facs]


def test_user_factors_are_checked_and_padded():
    A, b, facs = _small_problem()
    model = lm.build_model(A, b, factors=facs)
    V, d, khat = model.lowrank[0]
    assert khat == 4 and V.shape == (4 * khat, 8)
    assert np.count_nonzero(d) == sum(f[0].shape[1] for f in facs[0])


def test_user_factors_that_do_not_match_are_rejected():
    A, b, facs = _small_problem()
    V, d = facs[0][2]
    facs[0][2] = (V, -d)
    with pytest.raises(ValueError, match="constraint 3"):
        lm.build_model(A, b, factors=facs)
    A, b, facs = _small_problem()
    V, d = facs[0][1]
    facs[0][1] = (V * (1.0 + 1e-4), d)
    with pytest.raises(ValueError):
        lm.build_model(A, b, factors=facs)
    A, b, facs = _small_problem()
    with pytest.raises(ValueError):
        lm.build_model(A, b, factors=[facs[0][:3]])


def test_optimizer_takes_factors():
    from loraine_jl_amd.optimizer import Optimizer
    A, b, facs = _small_problem()
    o = Optimizer()
    o.load_model(A, b, factors=facs)
    assert o._pending[1][-1] is facs
