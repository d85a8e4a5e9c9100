"""The inputs of tests/test_gpu_cg_lowrank.py (tests/cg_lowrank_cases.py) are fair -- asserted on the CPU, with the
functions of oracle/cg_reference.py as they stand.

The GPU tests run the CG path from the rank-k factors of the data (option cg_lowrank) and ask for the reference's exact
iteration count and for results within a small multiple of the float64 oracle's own error.  That needs inputs whose
constraints really ARE their factors (the host's check accepts every one), which reach the branches they are built for
(dense and sparse slots, a permutation sigmaA, padding columns, two blocks with linear rows, tiles just past 64), whose H
is far from singular (cond <= 1e7: a float64 CG says nothing near 1e10) and whose residual history has a gap at an
iterate that rounding does not move (drift <= cr.DRIFT_MAX).

One more condition belongs to the factor form.  The GPU test takes the float64 oracle's distance from the reference as
"what float64 costs on this input" and grants the device 20 x that.  The oracle works on the entries of AA; the factor
form is another float64 algebra (lc.FactorFormOperator: the same map from V and d).  Early iterates (K = 5 .. 7, errors
of 1e-15 .. 1e-14) sit at the rounding floor, where one of the two can be an order of magnitude luckier than the other
-- L1 with seed 311: oracle 2.7e-15, factor form 6.5e-14 in NumPy, on the H-weighted distance -- and then the oracle's
distance is not the cost of float64 on that input.  Inputs are kept where the NumPy factor-form recurrence stays within
5 x the oracle's distances: the device, with yet another summation order, keeps a factor 4 of the 20."""
import numpy as np
import pytest

import cg_lowrank_cases as lc
from oracle import cg_reference as cr
from oracle import loraine_oracle as lo

NAMES = ["L1", "L2", "L3"]


def _ids(p):
    return "prec%d-erank%d" % p


@pytest.mark.parametrize("name", NAMES)
def test_host_factor_check_accepts_every_constraint(name):
    """build_case went through model.user_factors (ValueError on a miss); here each residual by itself, and the padded
    arrays against the factors they came from."""
    from loraine_jl_amd.model import LOWRANK_TOL, _factor_residual, padded_rank, user_factors
    case = lc.case_inputs(name)
    model = case.model
    for i, facs in enumerate(case.factors):
        m = int(model.msizes[i])
        assert len(facs) == model.n
        for k, (V, d) in enumerate(facs):
            assert _factor_residual(model.A[i][k + 1], V, d) <= LOWRANK_TOL
        Vp, dp, khat = case.lowrank[i]
        assert khat == padded_rank(lc.SHAPES[name][2][i]) and Vp.shape == (model.n * khat, m) and dp.size == model.n * khat
        ranks = np.count_nonzero(dp.reshape(model.n, khat), axis=1)
        assert ranks.tolist() == [V.shape[1] for V, _ in facs]
    bad = [list(f) for f in case.factors]
    V, d = bad[0][1]
    bad[0][1] = (V, -d)
    with pytest.raises(ValueError):
        user_factors(model.A, model.n, bad)


def test_inputs_reach_the_branches_they_are_for():
    L1, L2, L3 = (lc.case_inputs(n) for n in NAMES)
    assert [l[2] for l in L1.lowrank] == [4] and [l[2] for l in L2.lowrank] == [2, 1] and [l[2] for l in L3.lowrank] == [1]
    assert [int(m) for m in L1.model.msizes] == [37] and L1.model.n == 130 and L1.model.nlin == 0
    assert [int(m) for m in L2.model.msizes] == [33, 18] and L2.model.n == 257 and L2.model.nlin == 5
    assert L2.model.C_lin.nnz > 0
    assert [int(m) for m in L3.model.msizes] == [70] and L3.model.n == 65          # 64 + 6 rows, 64 + 1 constraints
    assert (L2.model.n + 255) // 256 == 2                                          # two workgroups of the CG recurrence
    for case in (L1, L2, L3):
        model = case.model
        for i in range(model.nlmi):
            n, q = model.n, int(model.qA[0, i])
            assert q == n - n // 4                                                 # dense slots, then the sparse ones
            assert not np.array_equal(model.sigmaA[:, i], np.arange(n))
            assert sorted(model.sigmaA[:, i].tolist()) == list(range(n))
            nz = model.nzA[:, i]
            assert (nz[3::4] == 4).all() and (np.delete(nz, np.s_[3::4]) == int(model.msizes[i]) ** 2).all()
            d = case.lowrank[i][1]
            assert (d == 1.0).any() and (d == -1.0).any()
    # padding columns of weight 0: khat 4 for ranks 1..3 (L1), rank-1 constraints under khat 2 (L2, block 1)
    assert (L1.lowrank[0][1].reshape(-1, 4) == 0.0).any(axis=1).all()
    assert (L2.lowrank[0][1].reshape(-1, 2) == 0.0).any()
    # the sparse constraints sit on pairwise distinct index pairs
    for case in (L1, L2, L3):
        for i, facs in enumerate(case.factors):
            pairs = [tuple(np.nonzero(np.any(V != 0.0, axis=1))[0]) for V, _ in facs[3::4]]
            assert all(len(p) == 2 for p in pairs) and len(set(pairs)) == len(pairs)


@pytest.mark.parametrize("name", NAMES)
def test_eigenvalues_are_separated_and_H_is_well_conditioned(name):
    case, H = lc.case_data(name)
    for W in case.W:
        lam = np.linalg.eigvalsh(W)
        assert lam[0] > 0 and 5e2 < lam[-1] / lam[0] < 2e3
        for i in range(1, 4):                                                      # erank <= 2 is what the GPU tests use
            assert lam[-i] / lam[-i - 1] >= 1.5
    ev = np.linalg.eigvalsh(H.astype(np.float64))
    print("CGLR %s cond(H) = %.3e" % (name, ev[-1] / ev[0]))
    assert ev[0] > 0 and ev[-1] / ev[0] <= 1e7


@pytest.mark.parametrize("name", NAMES)
def test_reference_operator_is_the_oracles(name):
    """dense_operator on the AA built from the factors against MyA, and against the factors themselves:
    H_ij = sum_pq d_ip d_jq (v_ip' W v_jq)^2."""
    case, H = lc.case_data(name)
    y = np.zeros(case.model.n)
    lo.MyA(case.W, case.model.AA, case.model.nlin, case.model.C_lin, case.X_lin, case.S_lin_inv)(y, case.x)
    assert cr.relerr(y, H @ case.x.astype(cr.LD)) < 1e-13
    Hf = np.zeros((case.model.n, case.model.n), dtype=cr.LD)
    for i, facs in enumerate(case.factors):
        Wl = case.W[i].astype(cr.LD)
        Vall = np.concatenate([V for V, _ in facs], axis=1).astype(cr.LD)
        dall = np.concatenate([d for _, d in facs]).astype(cr.LD)
        own = np.repeat(np.arange(case.model.n), [V.shape[1] for V, _ in facs])
        T = (Vall.T @ Wl @ Vall) ** 2 * np.outer(dall, dall)
        S = np.zeros((case.model.n, T.shape[1]), dtype=cr.LD)
        np.add.at(S, own, T)
        Hb = np.zeros_like(Hf)
        np.add.at(Hb.T, own, S.T)
        Hf += Hb
    if case.model.nlin:
        Cl = case.model.C_lin.toarray().astype(cr.LD)
        Hf += (Cl * (case.X_lin * case.S_lin_inv).astype(cr.LD)[None, :]) @ Cl.T
    assert cr.relerr(Hf, H) < 1e-15


@pytest.mark.parametrize("prec,erank", lc.PRECS, ids=[_ids(p) for p in lc.PRECS])
@pytest.mark.parametrize("name", ["L1", "L2"])
def test_inputs_have_a_gap_at_K_and_the_oracle_stops_there(name, prec, erank):
    case, H = lc.case_data(name)
    run = lc.case_run(name, prec, erank)
    K, rho = run.K, run.hist.rho
    assert 3 <= K <= 12
    assert rho[K - 1] / rho[K] >= 1.5
    assert run.tol == cr.pick_tol(rho, K)
    assert all(r > run.tol * 1.2 for r in rho[:K]) and rho[K] < run.tol / 1.2
    assert max(run.drift[K - 1], run.drift[K]) <= cr.DRIFT_MAX
    Ao, Mo = cr.oracle_state(case, prec, erank)
    xo, ec, it = lo.cg(Ao, case.h, tol=run.tol, maxIter=10000, precon=Mo)
    assert (ec, it) == (30, K)
    assert cr.relerr(xo, run.hist.x[K]) < 5e-8                # 20 x this stays under the 1e-6 the GPU test never exceeds
    xo, ec, it = lo.cg(Ao, case.h, tol=run.tol, maxIter=K - 1, precon=Mo)
    assert (ec, it) == (-2, K - 1)
    assert cr.relerr(xo, run.hist.x[K - 1]) < 5e-8


@pytest.mark.parametrize("erank", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_reference_preconditioner_is_the_oracles(name, erank):
    """prec_alpha_matrix (solved with in longdouble) against the float64 MyM on these inputs: the distance the GPU test
    multiplies by 20 is small enough to mean something."""
    case = lc.case_inputs(name)
    ref = cr.reference_solver(case, 1, erank)(case.x)
    _, Mo = cr.oracle_state(case, 1, erank)
    z = np.zeros(case.model.n)
    Mo(z, case.x)
    assert cr.relerr(z, ref) < 5e-11                          # 20 x this stays under the 1e-9 cap of the apply


def _herr(H, x, xref, h):
    d = H @ (np.asarray(x, dtype=cr.LD) - np.asarray(xref, dtype=cr.LD))
    h = np.asarray(h, dtype=cr.LD)
    return float(np.sqrt(np.sum(d * d)) / np.sqrt(np.sum(h * h)))


@pytest.mark.parametrize("prec,erank", lc.PRECS, ids=[_ids(p) for p in lc.PRECS])
@pytest.mark.parametrize("name", ["L1", "L2"])
def test_factor_form_in_float64_costs_what_the_oracle_costs(name, prec, erank):
    """lo.cg with the NumPy factor-form operator: the same exits and counts, x and H dx within 5 x the oracle's."""
    case, H = lc.case_data(name)
    run = lc.case_run(name, prec, erank)
    Ao, Mo = cr.oracle_state(case, prec, erank)
    Af = lc.FactorFormOperator(case)
    y, yf = np.zeros(case.model.n), np.zeros(case.model.n)
    Ao(y, case.x)
    Af(yf, case.x)
    assert cr.relerr(yf, y) < 1e-14
    for maxit, want in ((10000, (30, run.K)), (run.K - 1, (-2, run.K - 1))):
        xo, ec, it = lo.cg(Ao, case.h, tol=run.tol, maxIter=maxit, precon=Mo)
        xf, ecf, itf = lo.cg(Af, case.h, tol=run.tol, maxIter=maxit, precon=Mo)
        assert (ec, it) == (ecf, itf) == want
        xref = run.hist.x[it]
        ex_o, ex_f = cr.relerr(xo, xref), cr.relerr(xf, xref)
        er_o, er_f = _herr(H, xo, xref, case.h), _herr(H, xf, xref, case.h)
        print("CGLR float64 %s prec=%d erank=%d it=%d | x: oracle %.2e factor form %.2e | H dx: oracle %.2e factor form %.2e"
              % (name, prec, erank, it, ex_o, ex_f, er_o, er_f))
        assert ex_f <= 5.0 * ex_o and er_f <= 5.0 * er_o
