"""GPU: the CG path from the rank-k factors of the data (option cg_lowrank; csrc/hop.hip: H of the assembled-matrix operator
in mode 1, csrc/dataops.hip: the matrix-free operator in factor form, csrc/prec.hip, csrc/facops.hip: ts of H_alpha by fac_ts_kernel)
against the extended-precision reference of oracle/cg_reference.py.

The inputs are those of tests/cg_lowrank_cases.py (constraints built from their factors; L1 one block in position space,
L2 two blocks + linear rows, L3 tiles just past 64); tests/test_cg_lowrank_cpu.py asserts on the CPU that they are fair.

Bounds follow the rule of tests/test_gpu_pcg_reference.py: the float64 oracle (lo.MyA, lo.MyM, lo.cg) runs on the same
inputs against the longdouble reference, the device gets 20 x the oracle's distance -- a different summation order moves
rounding by a small multiple -- and never more than the caps that file uses: 1e-6 on x, 2 tol on the true residual,
1e-9 on the apply (Jacobi eigenvectors).  Every test prints the oracle's and the device's distance."""
import contextlib
import functools

import numpy as np
import pytest

import cg_lowrank_cases as lc
from oracle import cg_reference as cr
from oracle import loraine_oracle as lo

pytestmark = pytest.mark.gpu

DEFAULTS = dict(prec_eig=0, matvec_h=0, prec_inv=-1, prec_dense=0, cg_lowrank=0)
FACTOR = 20.0
NEW_COUNTERS = ("hop_assemble_lowrank", "op_factored_cg", "prec_ts_factored")
FORMS = [(0, 1), (1, 1), (1, 2)]       # (prec_inv, prec_dense): triangular solves, explicit inverse, one dense matrix


@pytest.fixture(scope="module")
def dev():
    import loraine_jl_amd
    d = loraine_jl_amd.Device(0)
    yield d
    d.close()


@contextlib.contextmanager
def options(dev, **kw):
    try:
        for k, v in kw.items():
            dev.set_option(k, v)
        yield
    finally:
        for k in kw:
            dev.set_option(k, DEFAULTS[k])


def _upload(dev, case, with_G=True, factors=True, drop=None):
    """drop = k: the factor columns of constraint k of block 0 get weight 0 -- a constraint with entries and no weighted
    factor column, so the factors do not cover the block (v_partial)."""
    m = case.model
    dev.upload_model(m.AA, m.sigmaA, m.qA, m.msizes, C_lin=m.C_lin if m.nlin else None)
    if factors:
        for i, (V, d, khat) in enumerate(case.lowrank):
            d = d.copy()
            if drop is not None and i == 0:
                d[drop * khat:(drop + 1) * khat] = 0.0
            dev.upload_lowrank(i, khat, V, d)
    for i in range(m.nlmi):
        dev.set_scaling(i, case.W[i], case.G[i] if with_G else None)
    if m.nlin:
        dev.set_lin(case.X_lin, case.S_lin_inv)


def _counts(dev):
    return {k: dev.count(k) for k in NEW_COUNTERS}


def _herr(H, x, xref, h):
    """||H (x - xref)|| / ||h|| in longdouble."""
    d = H @ (np.asarray(x, dtype=cr.LD) - np.asarray(xref, dtype=cr.LD))
    h = np.asarray(h, dtype=cr.LD)
    return float(np.sqrt(np.sum(d * d)) / np.sqrt(np.sum(h * h)))


# ---------------------------------------------------------------------------------------------- what float64 costs
@functools.lru_cache(maxsize=None)
def _oracle_operator(name):
    case, H = lc.case_data(name)
    ref = H @ case.x.astype(cr.LD)
    y = np.zeros(case.model.n)
    lo.MyA(case.W, case.model.AA, case.model.nlin, case.model.C_lin, case.X_lin, case.S_lin_inv)(y, case.x)
    return ref, cr.relerr(y, ref)


@functools.lru_cache(maxsize=None)
def _oracle_apply(name, erank):
    case = lc.case_inputs(name)
    ref = cr.reference_solver(case, 1, erank)(case.x)
    _, Mo = cr.oracle_state(case, 1, erank)
    z = np.zeros(case.model.n)
    Mo(z, case.x)
    return ref, cr.relerr(z, ref)


@functools.lru_cache(maxsize=None)
def _oracle_pcg(name, prec, erank):
    case, H = lc.case_data(name)
    run = lc.case_run(name, prec, erank)
    Ao, Mo = cr.oracle_state(case, prec, erank)
    out = []
    for maxit in (10000, run.K - 1):
        xo, ec, it = lo.cg(Ao, case.h, tol=run.tol, maxIter=maxit, precon=Mo)
        out.append(((ec, it), cr.relerr(xo, run.hist.x[it]), _herr(H, xo, run.hist.x[it], case.h)))
    return out


# ---------------------------------------------------------------------------------------------- the three checks
def _check_operator(dev, name, mh, tag):
    """dev.matvec(x) twice under matvec_h = mh against H x of the reference -> the counter deltas."""
    case, _ = lc.case_data(name)
    ref, err_o = _oracle_operator(name)
    with options(dev, matvec_h=mh):
        c0 = _counts(dev)
        y1 = dev.matvec(case.x)
        y2 = dev.matvec(case.x)
        c1 = _counts(dev)
    err = cr.relerr(y1, ref)
    print("CGLR operator %s %s mh=%d | oracle %.2e bound %.2e | device %.2e" % (name, tag, mh, err_o, FACTOR * err_o, err))
    assert err <= FACTOR * err_o, (err, err_o)
    assert np.array_equal(y1, y2)
    return {k: c1[k] - c0[k] for k in c0}


def _check_apply(dev, name, erank, tag, want_factored):
    case = lc.case_inputs(name)
    ref, err_o = _oracle_apply(name, erank)
    bound = min(FACTOR * err_o, 1e-9)
    lin = case.model.nlin > 0
    res = []
    with options(dev, prec_eig=1):
        for inv, dense in FORMS:
            with options(dev, prec_inv=inv, prec_dense=dense):
                assert dev.prec_setup(1, erank, 1) == 0
                assert dev.count("prec_ts_factored") == want_factored
                b0 = dev.count("prec_dense_build")
                res.append((dev.prec_apply(case.x), dev.count("prec_dense_build") - b0))
    errs = [cr.relerr(y, ref) for y, _ in res]
    print("CGLR apply %s %s erank=%d | oracle %.2e bound %.2e | device potrs %.2e inverse %.2e dense %.2e"
          % (name, tag, erank, err_o, bound, errs[0], errs[1], errs[2]))
    # the dense form exists without linear rows from nvar 256 on (prec.hip::prec_dense_worthwhile)
    assert [b for _, b in res] == [0, 0, 1 if (not lin and case.model.n >= 256) else 0]
    for e in errs:
        assert e <= bound, (errs, bound)


def _check_pcg(dev, name, prec, erank, mh, tag):
    case, H = lc.case_data(name)
    run = lc.case_run(name, prec, erank)
    K, tol = run.K, run.tol
    orc = _oracle_pcg(name, prec, erank)
    assert orc[0][0] == (30, K) and orc[1][0] == (-2, K - 1)
    with options(dev, prec_eig=1, matvec_h=mh):
        assert dev.prec_setup(prec, erank, 1) == 0
        c0 = _counts(dev)
        got = [dev.pcg(case.h, tol, 10000), dev.pcg(case.h, tol, K - 1)]
        c1 = _counts(dev)
    checks = []
    for (x, ec, it), want, (_, ex_o, er_o) in zip(got, ((30, K), (-2, K - 1)), orc):
        xref = run.hist.x[want[1]]
        ex, er = cr.relerr(x, xref), _herr(H, x, xref, case.h)
        res = cr.true_residual(H, x, case.h)
        print("CGLR pcg %s %s prec=%d erank=%d mh=%d K=%d tol=%.3e exit=(%d,%d) want=(%d,%d) | x: oracle %.2e device %.2e | "
              "H dx: oracle %.2e device %.2e | true residual %.4e"
              % (name, tag, prec, erank, mh, K, tol, ec, it, want[0], want[1], ex_o, ex, er_o, er, res))
        checks.append(((ec, it), want, ex, min(FACTOR * ex_o, 1e-6), er, FACTOR * er_o, res))
    for got_exit, want, ex, bx, er, br, res in checks:
        assert got_exit == want
        assert ex <= bx, (ex, bx)
        assert er <= br, (er, br)
        if want[0] == 30:
            assert res <= 2.0 * tol
    return {k: c1[k] - c0[k] for k in ("hop_assemble_lowrank", "op_factored_cg")}, c1["prec_ts_factored"]


# ---------------------------------------------------------------------------------------------- 1-3: from the factors
@pytest.mark.parametrize("name", ["L1", "L2", "L3"])
def test_operator_from_factors(dev, name):
    """matvec_h = 1: mat(AA' x) and AA vec(W M W) of every block in factor form; matvec_h = 2: y = H x with H assembled in
    mode 1, once for the two calls."""
    case = lc.case_inputs(name)
    _upload(dev, case)
    with options(dev, cg_lowrank=1):
        d1 = _check_operator(dev, name, 1, "factors")
        d2 = _check_operator(dev, name, 2, "factors")
    assert d1 == dict(hop_assemble_lowrank=0, op_factored_cg=2 * case.model.nlmi, prec_ts_factored=0)
    assert d2 == dict(hop_assemble_lowrank=1, op_factored_cg=0, prec_ts_factored=0)


@pytest.mark.parametrize("with_G", [True, False], ids=["G", "W-only"])
@pytest.mark.parametrize("erank", [1, 2])
@pytest.mark.parametrize("name", ["L1", "L2", "L3"])
def test_halpha_apply_with_ts_from_factors(dev, name, erank, with_G):
    """prec_setup forms ts as P = L' Vd, T = Vd' Um and fac_ts_kernel for every block; the apply in its three forms against
    the reference solve with prec_alpha_matrix.  W-only: eig(W) from W itself, the same reference."""
    case = lc.case_inputs(name)
    _upload(dev, case, with_G=with_G)
    with options(dev, cg_lowrank=1):
        _check_apply(dev, name, erank, "factors" + ("" if with_G else " W-only"), case.model.nlmi)


@pytest.mark.parametrize("mh", [1, 2], ids=["matrixfree", "assembledH"])
@pytest.mark.parametrize("prec,erank", lc.PRECS, ids=["prec%d-erank%d" % p for p in lc.PRECS])
@pytest.mark.parametrize("name", ["L1", "L2"])
def test_pcg_from_factors(dev, name, prec, erank, mh):
    """(30, K) exactly at the tolerance in the gap, (-2, K - 1) at maxit = K - 1, x and the true residual those of the
    reference -- with the operator and, under H_alpha, ts taken from the factors."""
    case = lc.case_inputs(name)
    _upload(dev, case)
    with options(dev, cg_lowrank=1):
        delta, tsf = _check_pcg(dev, name, prec, erank, mh, "factors")
    assert (delta["op_factored_cg"] > 0) == (mh == 1)
    assert delta["hop_assemble_lowrank"] == (1 if mh == 2 else 0)
    assert tsf == (case.model.nlmi if prec == 1 else 0)


# ---------------------------------------------------------------------------------------------- 4: default untouched
def test_default_option_leaves_every_bit_alone():
    """The same model with and without uploaded factors, default options (cg_lowrank = 0), a fresh context each so that both
    see the same history: matvec, prec_setup + prec_apply and pcg give identical bits, the new counters stay 0."""
    import loraine_jl_amd
    case = lc.case_inputs("L1")
    run = lc.case_run("L1", 1, 1)
    out = []
    for factors in (False, True):
        d = loraine_jl_amd.Device(0)
        try:
            _upload(d, case, factors=factors)
            y = d.matvec(case.x)
            assert d.prec_setup(1, 1, 1) == 0
            z = d.prec_apply(case.x)
            x, ec, it = d.pcg(case.h, run.tol, 10000)
            out.append((y, z, x, ec, it))
            assert _counts(d) == dict.fromkeys(NEW_COUNTERS, 0)
        finally:
            d.close()
    for a, b in zip(out[0][:3], out[1][:3]):
        assert np.array_equal(a, b)
    assert out[0][3:] == out[1][3:]


# ---------------------------------------------------------------------------------------------- 5: not covered
def test_block_the_factors_do_not_cover_stays_on_the_entries(dev):
    """Constraint 5 of L1 has entries and only weight-0 factor columns: the factors are not the whole block (v_partial).
    cg_lowrank = 1 must leave it on the entry routes -- counters at 0, the bounds of the tests above."""
    case = lc.case_inputs("L1")
    _upload(dev, case, drop=5)
    with options(dev, cg_lowrank=1):
        c0 = _counts(dev)
        _check_operator(dev, "L1", 1, "not covered")
        _check_operator(dev, "L1", 2, "not covered")
        _check_apply(dev, "L1", 2, "not covered", 0)
        for mh in (1, 2):
            _check_pcg(dev, "L1", 1, 1, mh, "not covered")
        c1 = _counts(dev)
    assert c1["hop_assemble_lowrank"] == c0["hop_assemble_lowrank"] and c1["op_factored_cg"] == c0["op_factored_cg"]
    assert c1["prec_ts_factored"] == 0
    assert dev.count("lowrank_from_entries") == 0          # (H of the operator was assembled in mode 0, not mode 1's fallback)


# ---------------------------------------------------------------------------------------------- 6: solve
def _solve(P, force=None, **attrs):
    from loraine_jl_amd import solvers
    from loraine_jl_amd.optimizer import Optimizer
    import scipy.sparse as sp
    o = Optimizer()
    o.set_silent(True)
    for k, v in attrs.items():
        o.set_attribute(k, v)
    A = [sp.csc_matrix(P.F0()[0])] + [sp.csc_matrix(P.constraint(k)) for k in range(P.nvar)]
    o.load_model([A], P.b, max_sense=True)
    o._copy_to()                                   # (optimize() is these two steps; the option goes in between)
    o.solver.dev.set_option("reset_timing", 1)
    if force is not None:
        o.solver.dev.set_option("cg_lowrank", force)
    solvers.solve(o.solver, o.halpha)
    return o


def test_kit1_solve_with_datarank_2():
    """A planted problem with a rank-2 solution and rank-2 data (msz 40, nvar 60): kit = 1 with H_alpha and datarank = 2
    uploads the factors and lets the cost model route the CG path; forced (cg_lowrank = 1) every piece comes from them.
    Both end at the optimum of the datarank = 0 run and of the direct solver, within what the termination test pins."""
    from loraine_jl_amd.synthetic import FactoredLowRankProblem
    P = FactoredLowRankProblem(40, 60, krank=2, xrank=2, seed=11)
    edimacs = 1e-7
    base = dict(preconditioner=1, eDIMACS=edimacs)
    o0 = _solve(P, kit=1, datarank=0, **base)
    od = _solve(P, kit=0, datarank=0, **base)
    oa = _solve(P, kit=1, datarank=2, **base)
    of = _solve(P, force=1, kit=1, datarank=2, **base)
    assert not o0.solver.lowrank and o0.solver.dev.count("hop_assemble_lowrank") + o0.solver.dev.count("op_factored_cg") == 0
    for o, tag in ((oa, "auto"), (of, "forced")):
        s = o.solver
        used = s.dev.count("hop_assemble_lowrank") + s.dev.count("op_factored_cg")
        print("CGLR solve %s: status %d, %d iterations, %d CG iterations, objective %.10f dual %.10f | H in mode 1 %d, "
              "operator blocks in factor form %d, ts blocks from factors (last setup) %d | datarank 0: %.10f / %.10f, "
              "kit 0: %.10f / %.10f, planted %.10f"
              % (tag, s.status, s.iter, s.cg_iter_tot, o.objective_value(), o.dual_objective_value(),
                 s.dev.count("hop_assemble_lowrank"), s.dev.count("op_factored_cg"), s.dev.count("prec_ts_factored"),
                 o0.objective_value(), o0.dual_objective_value(), od.objective_value(), od.dual_objective_value(), P.optimum))
        assert s.lowrank and s.datarank == 2 and s.kit == 1
        assert used > 0
        assert s.status == 1 and o.termination_status() == "OPTIMAL"
        for ref in (o0, od):
            assert ref.solver.status == 1
            assert o.objective_value() == pytest.approx(ref.objective_value(), rel=2.5 * edimacs)
            assert o.dual_objective_value() == pytest.approx(ref.dual_objective_value(), rel=2.5 * edimacs)
    assert of.solver.dev.count("prec_ts_factored") > 0
