"""The extended-precision PCG reference (oracle/cg_reference.py) against the float64 oracle, and the conditions that the
inputs of tests/test_gpu_pcg_reference.py have to meet -- all of it on the CPU.

The GPU tests ask the device for an EXACT iteration count and for iterates within a small multiple of the float64
oracle's own error.  That is only a fair question where the answer is determined: the tolerance sits in a gap of the
residual history, the iterates around it are not ill-conditioned functions of the data, the -13 exit is not a near-zero
p'Ap, and the eigenvectors H_alpha is built from belong to separated eigenvalues.  Those are properties of the inputs;
they are asserted here, where no device is involved."""
import numpy as np
import pytest

from oracle import cg_reference as cr
from oracle import loraine_oracle as lo

PRECS = [(0, 1), (2, 1), (1, 1), (1, 3)]
GPU_CASES = ["A", "B", "C", "D"]


def _ids(p):
    return "prec%d-erank%d" % p


def test_longdouble_is_wider_than_double():
    """The whole module rests on it (x86-64: 64-bit mantissa)."""
    assert np.finfo(cr.LD).eps < 1e-18


def test_eig_ld_is_accurate_beyond_double():
    rng = np.random.default_rng(0)
    W, _ = cr.scaling_from_spectrum(cr.spectrum(33), rng)
    lam, V = cr.eig_ld(W)
    Wl = W.astype(cr.LD)
    assert float(np.abs(V.T @ V - np.eye(33)).max()) < 1e-17
    assert float(np.abs(Wl @ V - V * lam[None, :]).max()) < 1e-17 * 1e3
    assert np.allclose(lam.astype(float), np.linalg.eigvalsh(W), rtol=1e-12)


def test_spd_solver_refines_below_double():
    rng = np.random.default_rng(1)
    B = rng.standard_normal((60, 60))
    M = (B @ B.T + 60 * np.eye(60)).astype(cr.LD)
    x = rng.standard_normal(60).astype(cr.LD)
    y = cr.spd_solver(M)(x)
    assert cr.relerr(M @ y, x) < 1e-17
    assert cr.relerr(cr.spd_solver(M, refine=False)(x), y) < 1e-13


def test_pick_tol_wants_a_gap():
    rho = [1.0, 0.5, 0.4, 0.1, 0.09]
    assert cr.pick_tol(rho, 3) == pytest.approx(0.2)
    with pytest.raises(AssertionError):
        cr.pick_tol(rho, 2)                      # 0.5 / 0.4 < 1.5
    with pytest.raises(AssertionError):
        cr.pick_tol([1.0, 0.11, 0.3, 0.1], 3)    # an earlier residual sits next to the tolerance
    assert cr.choose_K(rho, [0.0] * 5, kmin=1) == 3
    with pytest.raises(AssertionError):
        cr.choose_K(rho, [0.0, 0.0, 1e-3, 1e-3, 0.0], kmin=2)     # the iterates at the gap are not determined


def test_pcg_history_trivial_exits():
    H = np.eye(3)
    assert cr.pcg_history(H, cr.identity_solver(), np.zeros(3), 1e-6, 5)[4:] == (1, 0)
    assert cr.pcg_history(H, cr.identity_solver(), 1e-9 * np.ones(3), 1e-6, 5)[4:] == (2, 0)
    h = cr.pcg_history(np.diag([1.0, 2.0, 3.0]), cr.identity_solver(), np.ones(3), 1e-12, 10)
    assert (h.code, h.it) == (30, 3) and cr.relerr(h.x[3], [1.0, 0.5, cr.LD(1) / 3]) < 1e-18


@pytest.mark.parametrize("prec,erank", PRECS, ids=[_ids(p) for p in PRECS])
@pytest.mark.parametrize("name", ["D", "T"])
def test_reference_operator_and_preconditioners_agree_with_the_oracle(name, prec, erank):
    """theta1 and tru3 (72 linear rows): H against MyA, M^-1 against MyM / MyM_beta."""
    case, H = cr.case_data(name)
    n = case.model.n
    Ao, Mo = cr.oracle_state(case, prec, erank)
    y = np.zeros(n)
    Ao(y, case.x)
    assert cr.relerr(y, H @ case.x.astype(cr.LD)) < 1e-13
    z = np.zeros(n)
    Mo(z, case.x)
    assert cr.relerr(z, cr.reference_solver(case, prec, erank)(case.x)) < 1e-10


# tru3 with H_alpha is left to the apply check above: cond(M_alpha) = 1e5 (erank 1) and 1.5e6 (erank 3) there, MyM itself
# is 4e-13 off the reference, CG turns that into 2e-11 after ONE step and 2e-10 after four, and with erank 1 the residual
# stays within 0.8 .. 1 for thirteen steps (no gap to put a tolerance in).  x to 1e-10 would test the oracle's float64
# Woodbury formula, not the reference.
@pytest.mark.parametrize("name,prec,erank", [("D", p, e) for p, e in PRECS] + [("T", 0, 1), ("T", 2, 1)])
def test_reference_recurrence_agrees_with_the_oracle(name, prec, erank):
    """Same exit and count as loraine_oracle.cg, x to 1e-10 -- at the first iteration K >= 2 with a gap that float64
    rounding moves by < 1e-13 (CG iterates lose about a digit per step on these systems, see choose_K)."""
    case, H = cr.case_data(name)
    Ao, Mo = cr.oracle_state(case, prec, erank)
    run = cr.case_run(name, prec, erank, 1e-13, 2, False)
    K, tol = run.K, run.tol
    xo, ec, it = lo.cg(Ao, case.h, tol=tol, maxIter=10000, precon=Mo)
    assert (ec, it) == (30, K)
    assert cr.relerr(xo, run.hist.x[K]) < 1e-10
    xo, ec, it = lo.cg(Ao, case.h, tol=tol, maxIter=K - 1, precon=Mo)
    assert (ec, it) == (-2, K - 1)
    assert cr.relerr(xo, run.hist.x[K - 1]) < 1e-10
    full = cr.pcg_history(H, run.solve, case.h, tol, 10000)
    assert (full.code, full.it) == (30, K) and cr.relerr(full.x[K], run.hist.x[K]) == 0.0


@pytest.mark.parametrize("name", GPU_CASES + ["E"])
def test_inputs_eigenvalues_are_separated_and_H_is_definite(name):
    """The top erank + 1 <= 4 eigenvalues of every W are separated by factors >= 1.5 (Jacobi, Lanczos and the reference
    then mean the same eigenvectors), cond(W) is about 1e3, the constraints are independent."""
    case = cr.case_inputs(name)
    for W in case.W:
        lam = np.linalg.eigvalsh(W)
        assert lam[0] > 0 and 5e2 < lam[-1] / lam[0] < 2e3
        for i in range(1, 5):
            assert lam[-i] / lam[-i - 1] >= 1.5
    assert sum(int(m) * (int(m) + 1) // 2 for m in case.model.msizes) >= case.model.n
    if name != "E":                                             # (E serves the preconditioner apply only)
        ev = np.linalg.eigvalsh(cr.case_data(name)[1].astype(np.float64))
        assert ev[0] > 0 and ev[-1] / ev[0] < 1e7


def test_inputs_reach_the_branches_they_are_for():
    """Workgroup slices of lrn_pcg (nwg = ceil(nvar / 256) <= 256, per = ceil(nvar / nwg)), ksz off the multiples of 16
    and 32, both kinds of constraint slot, linear rows."""
    def slices(n):
        nwg = max(1, min(256, (n + 255) // 256))
        per = (n + nwg - 1) // nwg
        return nwg, per, n - (nwg - 1) * per
    shape = {name: slices(cr.case_data(name)[0].model.n) for name in GPU_CASES}
    assert shape == {"A": (2, 129, 128), "B": (3, 172, 170), "C": (2, 150, 150), "D": (1, 104, 104)}
    B = cr.case_data("B")[0].model
    assert [e * int(B.msizes[0]) for e in (1, 3)] == [33, 99]
    C = cr.case_data("C")[0].model
    assert [int(m) for m in C.msizes] == [25, 17] and C.nlin == 5 and C.C_lin.nnz > 0
    E = cr.case_inputs("E").model
    assert 3 * int(E.msizes[0]) == 270 and E.n == 300
    for model in (B, C):
        for i in range(model.nlmi):
            assert 0 < int(model.qA[0, i]) < model.n           # dense slots and sparse slots


@pytest.mark.parametrize("prec,erank", PRECS, ids=[_ids(p) for p in PRECS])
@pytest.mark.parametrize("name", GPU_CASES)
def test_inputs_have_a_gap_at_K_and_the_oracle_stops_there(name, prec, erank):
    case, H = cr.case_data(name)
    run = cr.case_run(name, prec, erank)
    K, rho = run.K, run.hist.rho
    assert 3 <= K <= 12
    assert rho[K - 1] / rho[K] >= 1.5
    assert run.tol == cr.pick_tol(rho, K)
    assert all(r > run.tol * 1.2 for r in rho[:K]) and rho[K] < run.tol / 1.2
    assert max(run.drift[K - 1], run.drift[K]) <= 1e-9
    Ao, Mo = cr.oracle_state(case, prec, erank)
    xo, ec, it = lo.cg(Ao, case.h, tol=run.tol, maxIter=10000, precon=Mo)
    assert (ec, it) == (30, K)
    assert cr.relerr(xo, run.hist.x[K]) < 5e-8                # 20 x this stays under the 1e-6 the GPU test never exceeds
    xo, ec, it = lo.cg(Ao, case.h, tol=run.tol, maxIter=K - 1, precon=Mo)
    assert (ec, it) == (-2, K - 1)
    assert cr.relerr(xo, run.hist.x[K - 1]) < 5e-8


def test_indefinite_seed_gives_a_clear_alpha_invalid_exit():
    """W with two negative eigenvalues: the reference leaves with (-13, it), 2 <= it <= 10, p'Ap clearly negative there
    (|p'Ap| >= 1e-3 ||p|| ||Ap||) and at least as clearly positive in every step before; float64 agrees."""
    case, H = cr.case_data("A-indefinite")
    lam = np.linalg.eigvalsh(case.W[0])
    assert (lam < 0).sum() == 2 and lam[0] < -1.0
    assert np.linalg.eigvalsh(H.astype(np.float64))[0] < 0
    hist = cr.pcg_history(H, cr.identity_solver(), case.h, 0.0, 50)
    assert hist.code == -13 and 2 <= hist.it <= 10
    it = hist.it
    assert len(hist.x) == it and len(hist.pAp) == it          # x[it - 1] is the last iterate
    assert hist.pAp[it - 1] < 0 and hist.clear[it - 1] >= 1e-3
    assert all(hist.pAp[k] > 0 and hist.clear[k] >= hist.clear[it - 1] for k in range(it - 1))
    Ao, Mo = cr.oracle_state(case, 0, 1)
    xo, ec, ito = lo.cg(Ao, case.h, tol=0.0, maxIter=50, precon=Mo)
    assert (ec, ito) == (-13, it)
    assert cr.relerr(xo, hist.x[it - 1]) < 1e-12
