"""The CG path on factored and hybrid models (library option cg_factored, Optimizer.load_factored_model(..., cg=True)), the
parts that need no GPU.

1. What the algebra costs: tests/test_gpu_cg_factored.py asks the device for the reference's exact exit and count.  Here the
   same operators in NumPy float64 -- the scaled-factor form N = -Y diag(d o x) Y' with Y = W V, and the hybrid form (stored
   rows by their entries, one Z) -- drive lo.cg on the inputs of tests/cg_lowrank_cases.py: the same exits and counts as the
   oracle, x and H dx within 5 x the oracle's distance from the longdouble reference (the condition of
   tests/test_cg_lowrank_cpu.py::test_factor_form_in_float64_costs_what_the_oracle_costs).  Measured with the committed
   seeds: worst ratio 1.73 for the scaled form, 2.33 for the stored sets; the operators are 2.4e-16 .. 6.3e-16 from the
   reference.
2. The host check: kit = 1 on a factored model still raises "kit = 0" by default, and passes with cg=True -- before any
   device exists."""
import numpy as np
import pytest

import cg_factored_cases as fc
import cg_lowrank_cases as lc
from oracle import cg_reference as cr
from oracle import loraine_oracle as lo

# (id, case of cg_lowrank_cases, stored constraints per block)
FORMS = [("L1-scaled", "L1", [()]), ("L2-scaled", "L2", [(), ()]),
         ("L1-stored", "L1", fc.stored_sets("F1h")), ("L2-stored", "L2", fc.stored_sets("F2"))]


def _herr(H, x, xref, h):
    d = H @ (np.asarray(x, dtype=cr.LD) - np.asarray(xref, dtype=cr.LD))
    h = np.asarray(h, dtype=cr.LD)
    return float(np.sqrt(np.sum(d * d)) / np.sqrt(np.sum(h * h)))


@pytest.mark.parametrize("prec,erank", lc.PRECS, ids=["prec%d-erank%d" % p for p in lc.PRECS])
@pytest.mark.parametrize("tag,name,stored", FORMS, ids=[f[0] for f in FORMS])
def test_scaled_and_hybrid_forms_in_float64_cost_what_the_oracle_costs(tag, name, stored, prec, erank):
    case, H = lc.case_data(name)
    run = lc.case_run(name, prec, erank)
    Ao, Mo = cr.oracle_state(case, prec, erank)
    Af = fc.ScaledFactorOperator(case, stored, scaled=True)
    yf = np.zeros(case.model.n)
    Af(yf, case.x)
    err_op = cr.relerr(yf, H @ case.x.astype(cr.LD))
    print("CGFAC float64 %s operator %.2e from the reference" % (tag, err_op))
    assert err_op < 1e-14
    for maxit, want in ((10000, (30, run.K)), (run.K - 1, (-2, run.K - 1))):
        xo, ec, it = lo.cg(Ao, case.h, tol=run.tol, maxIter=maxit, precon=Mo)
        xf, ecf, itf = lo.cg(Af, case.h, tol=run.tol, maxIter=maxit, precon=Mo)
        assert (ec, it) == (ecf, itf) == want
        xref = run.hist.x[it]
        ex_o, ex_f = cr.relerr(xo, xref), cr.relerr(xf, xref)
        er_o, er_f = _herr(H, xo, xref, case.h), _herr(H, xf, xref, case.h)
        print("CGFAC float64 %s prec=%d erank=%d it=%d | x: oracle %.2e this form %.2e | H dx: oracle %.2e this form %.2e"
              % (tag, prec, erank, it, ex_o, ex_f, er_o, er_f))
        assert ex_f <= 5.0 * ex_o and er_f <= 5.0 * er_o


def test_kit_1_needs_cg_true_and_the_default_text_stays():
    from loraine_jl_amd.model import check_factored_kit
    from loraine_jl_amd.optimizer import Optimizer
    fm = fc.factored_model("F1")
    assert fm.factored and not fm.factored_cg
    check_factored_kit(fm, 0)
    with pytest.raises(ValueError, match="kit = 0"):
        check_factored_kit(fm, 1)
    import dataclasses
    fmc = dataclasses.replace(fm, factored_cg=True)
    check_factored_kit(fmc, 1)                                   # passes: no device was needed to say so
    check_factored_kit(fmc, 0)
    # through the Optimizer: the default raises before a device is opened, as it always has
    case = lc.case_inputs("L1")
    F0 = [-np.eye(37)]
    o = Optimizer()
    o.set_silent(True)
    o.set_attribute("kit", 1)
    o.load_factored_model(F0, [case.factors[0]], np.ones(case.model.n), factored_form=1)
    with pytest.raises(ValueError, match="kit = 0"):
        o.optimize()
    assert o.solver is None
    o.load_factored_model(F0, [case.factors[0]], np.ones(case.model.n), factored_form=1, cg=True)
    assert o._pending[1][-1] is True


def test_sharding_refuses_a_factored_model_under_kit_1():
    import types
    from loraine_jl_amd.sharding import DistributedHotPath
    solver = types.SimpleNamespace(kit=1, model=fc.factored_model("F1"), dist=None)
    with pytest.raises(ValueError, match="one GPU"):
        DistributedHotPath(solver, 0, 2)
    assert solver.dist is None
