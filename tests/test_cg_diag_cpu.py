"""The CG path on factored blocks with diagonal parts (library option cg_diag, Optimizer.load_factored_model(..., cg="diag")),
the parts that need no GPU.

1. The conditions the GPU test rests on, asserted: on the inputs of tests/cg_diag_cases.py cr.reference_run meets its gap and
   drift conditions for every (prec, erank) of lc.PRECS (K recorded there); the device's algebra in NumPy float64
   (DiagFactorOperator: the composition with the diagonal terms, stored rows by their entries) is within 1e-14 of the longdouble
   operator, drives lo.cg to the reference's exits (30, K) and (-2, K - 1) exactly, with x and H dx within 5 x the oracle's
   distance from the reference -- the bound of tests/test_cg_factored_cpu.py.
2. The ts formula: factor term + diagonal term + stored rows in NumPy (cg_diag_cases.ts_formula), H_alpha formed from it,
   against cr.prec_alpha_matrix of the materialised model, every case, erank 1 and 2 -- the formula apart from the kernel.
   Bound 1e-12 relative (Frobenius): both sides sum at most nvar khat msz products of float64 data with cond(W) = 1e3, the
   project's bound for one formulation against another.
3. The host opt-in: cg="diag" sets both flags and kit = 1 passes check_diag_kit before a device is opened; cg=True still raises
   with "diagonal parts"."""
import numpy as np
import pytest

import cg_diag_cases as dc
import cg_lowrank_cases as lc
from oracle import cg_reference as cr
from oracle import loraine_oracle as lo


def _herr(H, x, xref, h):
    d = H @ (np.asarray(x, dtype=cr.LD) - np.asarray(xref, dtype=cr.LD))
    h = np.asarray(h, dtype=cr.LD)
    return float(np.sqrt(np.sum(d * d)) / np.sqrt(np.sum(h * h)))


@pytest.mark.parametrize("prec,erank", lc.PRECS, ids=["prec%d-erank%d" % p for p in lc.PRECS])
@pytest.mark.parametrize("name", dc.NAMES)
def test_device_algebra_in_float64_costs_what_the_oracle_costs(name, prec, erank):
    case, H = dc.case_data(dc.data_name(name))
    run = dc.case_run(name, prec, erank)                       # (asserts the gap and the drift bound itself)
    assert 3 <= run.K <= 12 and max(run.drift[run.K - 1], run.drift[run.K]) <= cr.DRIFT_MAX
    Ao, Mo = cr.oracle_state(case, prec, erank)
    Af = dc.DiagFactorOperator(case, dc.stored_sets(name))
    yf = np.zeros(case.model.n)
    Af(yf, case.x)
    err_op = cr.relerr(yf, H @ case.x.astype(cr.LD))
    print("CGDIAG float64 %s operator %.2e from the reference" % (name, err_op))
    assert err_op < 1e-14
    for maxit, want in ((10000, (30, run.K)), (run.K - 1, (-2, run.K - 1))):
        xo, ec, it = lo.cg(Ao, case.h, tol=run.tol, maxIter=maxit, precon=Mo)
        xf, ecf, itf = lo.cg(Af, case.h, tol=run.tol, maxIter=maxit, precon=Mo)
        assert (ec, it) == (ecf, itf) == want
        xref = run.hist.x[it]
        ex_o, ex_f = cr.relerr(xo, xref), cr.relerr(xf, xref)
        er_o, er_f = _herr(H, xo, xref, case.h), _herr(H, xf, xref, case.h)
        print("CGDIAG float64 %s prec=%d erank=%d it=%d | x: oracle %.2e this form %.2e (ratio %.2f) | H dx: oracle %.2e this "
              "form %.2e (ratio %.2f)" % (name, prec, erank, it, ex_o, ex_f, ex_f / ex_o, er_o, er_f, er_f / er_o))
        assert ex_f <= 5.0 * ex_o and er_f <= 5.0 * er_o


@pytest.mark.parametrize("erank", [1, 2])
@pytest.mark.parametrize("name", dc.NAMES)
def test_ts_formula_gives_the_reference_h_alpha(name, erank):
    case = dc.case_inputs(name)
    ref = cr.prec_alpha_matrix(case.model, case.W, erank, 1, case.X_lin, case.S_lin_inv)
    M = dc.ts_formula(case, dc.stored_sets(name), erank)
    err = cr.relerr(M.ravel(), ref.ravel())
    # without the diagonal term the formula is NOT the reference's matrix: the term is what the test is about
    bare = dc.ts_formula(case_without_diag(case), dc.stored_sets(name), erank)
    miss = cr.relerr(bare.ravel(), ref.ravel())
    print("CGDIAG ts formula %s erank=%d | H_alpha vs prec_alpha_matrix %.2e | without the diagonal term %.2e" % (name, erank, err, miss))
    assert err < 1e-12
    assert miss > 1e-6


def test_the_cases_are_the_ones_the_gpu_test_counts_on():
    """Rows per case (prec_ts_diag_rows, prec_ts_stored_rows of the GPU test) and the factored models themselves: diagonal rows
    in `diag`, the stored constraints of D1h in AA, nothing else there."""
    assert [dc.n_diag(n) for n in dc.NAMES] == [5, 130, 5, 4 + 129, 17] and dc.n_stored("D1h") == 2
    for name in dc.NAMES:
        fm = dc.factored_model(name)
        case = dc.case_inputs(name)
        for i, st in enumerate(dc.stored_sets(name)):
            assert fm.AA[i].nnz == sum(case.model.A[i][k + 1].nnz for k in st)
            for k, a in fm.diag[i].items():
                assert np.array_equal(a, case.diag[i][k])


def case_without_diag(case):
    import types
    c = types.SimpleNamespace(**vars(case))
    c.diag = [{} for _ in case.diag]
    return c


def test_host_opt_in():
    from loraine_jl_amd.model import build_factored_model, check_diag_kit, check_factored_kit
    from loraine_jl_amd.optimizer import Optimizer
    m, n = 12, 7
    rng = np.random.default_rng(9)
    items = [(rng.standard_normal((m, 2)) / np.sqrt(m), np.array([1.0, -1.0])) for _ in range(n)]
    items[4] = (None, [], np.ones(m))
    F0 = [-np.eye(m)]
    # the model flag alone decides, before any device exists
    fm = build_factored_model(F0, [items], np.ones(n), factored_form=1)
    assert fm.factored and sorted(fm.diag[0]) == [4] and not fm.factored_cg and not fm.factored_cg_diag
    fm.factored_cg = True
    with pytest.raises(ValueError, match="diagonal parts"):
        check_diag_kit(fm, 1)
    fm.factored_cg_diag = True
    check_factored_kit(fm, 1)
    check_diag_kit(fm, 1)
    check_diag_kit(fm, 0)
    # through the Optimizer: cg="diag" sets both flags and kit = 1 passes both checks; stop before a device is opened
    class NoDevice:
        """Stands where the device would: the first call the solver makes on it ends the test (both checks lie before it)."""
        calls = []

        def __getattr__(self, name):
            NoDevice.calls.append(name)
            raise RuntimeError("stop before a device is used: " + name)

    o = Optimizer(device=NoDevice())
    o.set_silent(True)
    o.set_attribute("kit", 1)
    o.load_factored_model(F0, [items], np.ones(n), factored_form=1, cg="diag")
    with pytest.raises(RuntimeError, match="stop before a device is used: upload_model"):
        o.optimize()
    assert o.solver is None and NoDevice.calls == ["upload_model"]
    # cg=True keeps the refusal and its text, cg=False the older one; any other string is an error of its own
    for cg, text in ((True, "diagonal parts"), (False, "kit = 0")):
        o.load_factored_model(F0, [items], np.ones(n), factored_form=1, cg=cg)
        with pytest.raises(ValueError, match=text):
            o.optimize()
        assert o.solver is None
    with pytest.raises(ValueError, match="cg is False, True"):
        o.load_factored_model(F0, [items], np.ones(n), factored_form=1, cg="yes")
    # kit = 0 is untouched by the flag
    o.load_factored_model(F0, [items], np.ones(n), factored_form=1, cg="diag")
    assert o._pending[1][-1] is True
