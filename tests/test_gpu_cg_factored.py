"""GPU: the CG path on factored and hybrid models (library option cg_factored; csrc/cgops.hip: the guard, csrc/prec.hip: the stored rows of
ts, csrc/hop.hip: H in mode 1 and its memory budget, csrc/dataops.hip: the scaled-factor operator, csrc/facops.hip: the fused
quadratic form) against the extended-precision reference of oracle/cg_reference.py.

The inputs are those of tests/cg_lowrank_cases.py loaded as factored models (tests/cg_factored_cases.py: F1 pure, F1h / F2 / F3
with a few stored constraints); the reference H, case_run and the oracle are those of the materialised model.
tests/test_cg_factored_cpu.py asserts on the CPU that the algebra itself costs what the oracle costs.

Bounds are those of tests/test_gpu_cg_lowrank.py: 20 x the oracle's distance from the longdouble reference, never more than
1e-6 on x, 2 tol on the true residual, 1e-9 on the apply; 1e-12 relative for one formulation against another (the fused
kernel against NumPy from the factors).  Every test prints the oracle's and the device's distance."""
import contextlib
import functools

import numpy as np
import pytest

import cg_factored_cases as fc
import cg_lowrank_cases as lc
from oracle import cg_reference as cr
from oracle import loraine_oracle as lo

pytestmark = pytest.mark.gpu

DEFAULTS = dict(prec_eig=0, matvec_h=0, prec_inv=-1, prec_dense=0, cg_factored=0, fac_op_scaled=-1, fac_quadform=-1,
                hop_max_mb=-1)
FACTOR = 20.0
FORMS = [(0, 1), (1, 1), (1, 2)]       # (prec_inv, prec_dense): triangular solves, explicit inverse, one dense matrix
COUNTERS = ("op_factored_scaled", "op_quadform_fused", "hop_assemble", "hop_assemble_lowrank", "hop_over_budget", "hop_matvec",
            "matvec")
NAMES = ["F1", "F1h", "F2", "F3"]


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


def _scale(dev, case, with_G=True):
    """(Again: a new NT scaling, so that the operator choice and H are taken anew.)"""
    for i in range(case.model.nlmi):
        dev.set_scaling(i, case.W[i], case.G[i] if with_G else None)
    if case.model.nlin:
        dev.set_lin(case.X_lin, case.S_lin_inv)


def _upload(dev, name, with_G=True):
    fm = fc.factored_model(name)
    case = lc.case_inputs(fc.base(name))
    dev.upload_model(fm.AA, fm.sigmaA, fm.qA, fm.msizes, C_lin=fm.C_lin if fm.nlin else None)
    for i, (V, d, khat) in enumerate(fm.lowrank):
        dev.upload_lowrank(i, khat, V, d)
        dev.set_factored(i)
    _scale(dev, case, with_G)
    return case


def _counts(dev):
    return {k: dev.count(k) for k in COUNTERS}


def _delta(c0, c1):
    return {k: c1[k] - c0[k] for k in c0}


def _herr(H, x, xref, h):
    d = H @ (np.asarray(x, dtype=cr.LD) - np.asarray(xref, dtype=cr.LD))
    h = np.asarray(h, dtype=cr.LD)
    return float(np.sqrt(np.sum(d * d)) / np.sqrt(np.sum(h * h)))


# ---------------------------------------------------------------------------------------------- what float64 costs
@functools.lru_cache(maxsize=None)
def _oracle_operator(lname):
    case, H = lc.case_data(lname)
    ref = H @ case.x.astype(cr.LD)
    y = np.zeros(case.model.n)
    lo.MyA(case.W, case.model.AA, case.model.nlin, case.model.C_lin, case.X_lin, case.S_lin_inv)(y, case.x)
    return ref, cr.relerr(y, ref)


@functools.lru_cache(maxsize=None)
def _oracle_apply(lname, erank):
    case = lc.case_inputs(lname)
    ref = cr.reference_solver(case, 1, erank)(case.x)
    _, Mo = cr.oracle_state(case, 1, erank)
    z = np.zeros(case.model.n)
    Mo(z, case.x)
    return ref, cr.relerr(z, ref)


@functools.lru_cache(maxsize=None)
def _oracle_pcg(lname, prec, erank):
    case, H = lc.case_data(lname)
    run = lc.case_run(lname, prec, erank)
    Ao, Mo = cr.oracle_state(case, prec, erank)
    out = []
    for maxit in (10000, run.K - 1):
        xo, ec, it = lo.cg(Ao, case.h, tol=run.tol, maxIter=maxit, precon=Mo)
        out.append(((ec, it), cr.relerr(xo, run.hist.x[it]), _herr(H, xo, run.hist.x[it], case.h)))
    return out


# ---------------------------------------------------------------------------------------------- 1: the operator
def _operator_twice(dev, name, tag):
    """A new scaling, dev.matvec(x) twice against H x of the reference -> the counter deltas of the two calls."""
    case = lc.case_inputs(fc.base(name))
    ref, err_o = _oracle_operator(fc.base(name))
    _scale(dev, case)
    c0 = _counts(dev)
    y1 = dev.matvec(case.x)
    y2 = dev.matvec(case.x)
    d = _delta(c0, _counts(dev))
    err = cr.relerr(y1, ref)
    print("CGFAC operator %s %s | oracle %.2e bound %.2e | device %.2e" % (name, tag, err_o, FACTOR * err_o, err))
    assert err <= FACTOR * err_o, (err, err_o)
    assert np.array_equal(y1, y2)
    return d


@pytest.mark.parametrize("name", NAMES)
def test_operator_on_factored_and_hybrid_blocks(dev, name):
    """matvec_h = 1: the matrix-free operator, the factor part of every block in factor form -- the composition or Y = W Vd
    (pure blocks only), Q + column dots or the fused quadratic form; matvec_h = 2: y = H x with H assembled in mode 1, once for
    the two calls.  The route is read off the counters."""
    _upload(dev, name)
    nb, npure = fc.n_blocks(name), fc.n_pure(name)
    with options(dev, cg_factored=1):
        for mh in (1, 2):
            for scaled in (0, 1):
                for quad in (0, 1):
                    with options(dev, matvec_h=mh, fac_op_scaled=scaled, fac_quadform=quad):
                        d = _operator_twice(dev, name, "mh=%d scaled=%d quadform=%d" % (mh, scaled, quad))
                    if mh == 1:
                        assert d["op_factored_scaled"] == 2 * npure * scaled
                        assert d["op_quadform_fused"] == 2 * nb * quad
                        assert d["hop_assemble"] == d["hop_matvec"] == 0
                    else:
                        assert d["hop_assemble_lowrank"] == d["hop_assemble"] == 1 and d["hop_matvec"] == 2
                        assert d["op_factored_scaled"] == d["op_quadform_fused"] == 0
                    assert d["hop_over_budget"] == 0
        # no room for H: the forced assembled-matrix operator steps back to the matrix-free one instead of assembling
        with options(dev, matvec_h=2, hop_max_mb=0):
            d = _operator_twice(dev, name, "mh=2 hop_max_mb=0")
        assert d["hop_assemble"] == 0 and d["hop_matvec"] == 0 and d["hop_over_budget"] >= 1


# ---------------------------------------------------------------------------------------------- 2: the fused kernel alone
SHAPES = [  # msz, nvar, khat, sparse factors: tests/test_gpu_factored.py::CASES
    (16, 5, 1, False), (16, 37, 16, False), (96, 37, 2, True), (96, 130, 4, False), (130, 37, 8, True),
    (130, 130, 16, False), (257, 5, 4, True), (257, 130, 1, True), (333, 37, 8, False), (333, 300, 2, False),
    (257, 300, 1, False), (130, 300, 16, True), (333, 130, 4, True), (96, 5, 8, False),
    # the K range of the tile: one partial step, two steps and a tail of 8, a second row strip of 8 rows
    (13, 33, 2, False), (40, 37, 4, True), (72, 33, 16, False)]


def _factors(m, n, khat, seed, sparse):
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


def _matvec_numpy(facs, W, x):
    """AA vec(W mat(AA' x) W) straight from the factors."""
    m = W.shape[0]
    M = np.zeros((m, m))
    for k, (V, d) in enumerate(facs):
        M -= x[k] * (V * d) @ V.T
    Z = W @ M @ W
    return np.array([-float(np.sum(d * np.einsum("mp,mq,qp->p", V, Z, V))) for V, d in facs])


@pytest.mark.parametrize("m,n,khat,sparse", SHAPES)
def test_fused_quadratic_form_against_numpy(dev, m, n, khat, sparse):
    """fac_quadform_kernel + fac_quadform_reduce_kernel inside matvec: ranks 0 .. khat mixed (weight-0 columns), khat up to 16,
    msz and R off and on the tile of 64, one strip and six, msz 13 / 40 / 72 for the K range of the tile (one partial step; two
    steps and a tail; a second strip of eight rows), under both operator forms; twice for the bits."""
    from loraine_jl_amd.model import build_factored_model
    facs = _factors(m, n, khat, 1000 * m + n + khat, sparse)
    fm = build_factored_model([-np.eye(m)], [facs], np.zeros(n), factored_form=1)
    rng = np.random.default_rng(m + n)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    W = G @ G.T
    x = rng.standard_normal(n)
    ref = _matvec_numpy(facs, W, x)
    dev.upload_model(fm.AA, fm.sigmaA, fm.qA, fm.msizes)
    V, d, kh = fm.lowrank[0]
    dev.upload_lowrank(0, kh, V, d)
    dev.set_factored(0)
    dev.set_scaling(0, W, G)
    with options(dev, cg_factored=1, matvec_h=1, fac_quadform=1):
        for scaled in (0, 1):
            with options(dev, fac_op_scaled=scaled):
                f0 = dev.count("op_quadform_fused")
                y1 = dev.matvec(x)
                y2 = dev.matvec(x)
                assert dev.count("op_quadform_fused") - f0 == 2
            err = np.linalg.norm(y1 - ref) / np.linalg.norm(ref)
            print("CGFAC fused m=%d n=%d khat=%d sparse=%d scaled=%d | %.2e" % (m, n, khat, sparse, scaled, err))
            assert err < 1e-12
            assert np.array_equal(y1, y2)


# ---------------------------------------------------------------------------------------------- 3: H_alpha
@pytest.mark.parametrize("with_G", [True, False], ids=["G", "W-only"])
@pytest.mark.parametrize("erank", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_halpha_apply_with_stored_rows_from_the_entries(dev, name, erank, with_G):
    """ts of every block from its factors (fac_ts_kernel), the rows of the stored constraints of a hybrid block from their
    entries on a compact buffer; the apply in its three forms against the reference solve with prec_alpha_matrix."""
    case = _upload(dev, name, with_G=with_G)
    lname = fc.base(name)
    ref, err_o = _oracle_apply(lname, erank)
    bound = min(FACTOR * err_o, 1e-9)
    lin = case.model.nlin > 0
    res = []
    with options(dev, cg_factored=1, prec_eig=1):
        for inv, dense in FORMS:
            with options(dev, prec_inv=inv, prec_dense=dense):
                assert dev.prec_setup(1, erank, 1) == 0
                assert dev.count("prec_ts_factored") == fc.n_blocks(name)
                assert dev.count("prec_ts_stored_rows") == fc.n_stored(name)
                b0 = dev.count("prec_dense_build")
                z = dev.prec_apply(case.x)
                built = dev.count("prec_dense_build") - b0
                assert dev.prec_setup(1, erank, 1) == 0                      # a second setup: the same bits
                assert np.array_equal(z, dev.prec_apply(case.x))
                res.append((z, built))
    errs = [cr.relerr(y, ref) for y, _ in res]
    print("CGFAC apply %s erank=%d %s | oracle %.2e bound %.2e | device potrs %.2e inverse %.2e dense %.2e"
          % (name, erank, "G" if with_G else "W-only", err_o, bound, errs[0], errs[1], errs[2]))
    assert [b for _, b in res] == [0, 0, 1 if (not lin and case.model.n >= 256) else 0]
    for e in errs:
        assert e <= bound, (errs, bound)


# ---------------------------------------------------------------------------------------------- 4: lrn_pcg
@pytest.mark.parametrize("mh", [1, 2], ids=["matrixfree", "assembledH"])
@pytest.mark.parametrize("prec,erank", lc.PRECS, ids=["prec%d-erank%d" % p for p in lc.PRECS])
@pytest.mark.parametrize("name", ["F1", "F1h", "F2"])
def test_pcg_on_factored_models(dev, name, prec, erank, mh):
    """(30, K) exactly at the tolerance in the gap, (-2, K - 1) at maxit = K - 1, x and the true residual those of the
    reference."""
    lname = fc.base(name)
    case, H = lc.case_data(lname)
    _upload(dev, name)
    run = lc.case_run(lname, prec, erank)
    K, tol = run.K, run.tol
    orc = _oracle_pcg(lname, prec, erank)
    assert orc[0][0] == (30, K) and orc[1][0] == (-2, K - 1)
    with options(dev, cg_factored=1, prec_eig=1, matvec_h=mh):
        assert dev.prec_setup(prec, erank, 1) == 0
        c0 = _counts(dev)
        got = [dev.pcg(case.h, tol, 10000), dev.pcg(case.h, tol, K - 1)]
        d = _delta(c0, _counts(dev))
        tsf = dev.count("prec_ts_factored")
    checks = []
    for (x, ec, it), want, (_, ex_o, er_o) in zip(got, ((30, K), (-2, K - 1)), orc):
        xref = run.hist.x[want[1]]
        ex, er = cr.relerr(x, xref), _herr(H, x, xref, case.h)
        res = cr.true_residual(H, x, case.h)
        print("CGFAC pcg %s prec=%d erank=%d mh=%d K=%d tol=%.3e exit=(%d,%d) want=(%d,%d) | x: oracle %.2e device %.2e | "
              "H dx: oracle %.2e device %.2e | true residual %.4e"
              % (name, prec, erank, mh, K, tol, ec, it, want[0], want[1], ex_o, ex, er_o, er, res))
        checks.append(((ec, it), want, ex, min(FACTOR * ex_o, 1e-6), er, FACTOR * er_o, res))
    for got_exit, want, ex, bx, er, br, res in checks:
        assert got_exit == want
        assert ex <= bx, (ex, bx)
        assert er <= br, (er, br)
        if want[0] == 30:
            assert res <= 2.0 * tol
    assert d["hop_assemble_lowrank"] == (1 if mh == 2 else 0) and (d["hop_matvec"] > 0) == (mh == 2)
    assert tsf == (fc.n_blocks(name) if prec == 1 else 0)


@pytest.mark.parametrize("prec,erank", lc.PRECS, ids=["prec%d-erank%d" % p for p in lc.PRECS])
@pytest.mark.parametrize("name", ["F1", "F2"])
def test_pcg_matrix_free_through_the_scaled_factors_and_the_fused_form(dev, name, prec, erank):
    """The same exits and counts with both routes of the matrix-free operator forced on (the cost model leaves them off at
    these sizes): tests/test_cg_factored_cpu.py shows that the scaled-factor algebra in float64 keeps them."""
    lname = fc.base(name)
    case, H = lc.case_data(lname)
    _upload(dev, name)
    run = lc.case_run(lname, prec, erank)
    K, tol = run.K, run.tol
    orc = _oracle_pcg(lname, prec, erank)
    with options(dev, cg_factored=1, prec_eig=1, matvec_h=1, fac_op_scaled=1, fac_quadform=1):
        assert dev.prec_setup(prec, erank, 1) == 0
        c0 = _counts(dev)
        got = [dev.pcg(case.h, tol, 10000), dev.pcg(case.h, tol, K - 1)]
        d = _delta(c0, _counts(dev))
    for (x, ec, it), want, (_, ex_o, er_o) in zip(got, ((30, K), (-2, K - 1)), orc):
        xref = run.hist.x[want[1]]
        ex, er = cr.relerr(x, xref), _herr(H, x, xref, case.h)
        print("CGFAC pcg forced routes %s prec=%d erank=%d exit=(%d,%d) want=(%d,%d) | x: oracle %.2e device %.2e | "
              "H dx: oracle %.2e device %.2e" % (name, prec, erank, ec, it, want[0], want[1], ex_o, ex, er_o, er))
        assert (ec, it) == want
        assert ex <= min(FACTOR * ex_o, 1e-6) and er <= FACTOR * er_o
    napp = d["matvec"]                     # (operator applications queued: the iterations and the look-ahead beyond the exit)
    assert napp >= 2 * K - 1
    assert d["op_factored_scaled"] == napp * fc.n_pure(name) and d["op_quadform_fused"] == napp * fc.n_blocks(name)


# ---------------------------------------------------------------------------------------------- 5: solve
@pytest.mark.parametrize("hybrid", [False, True], ids=["pure", "hybrid"])
def test_kit1_solve_of_a_factored_model(hybrid):
    """The planted msz 40 / nvar 60 / rank-2 problem given by its factors alone, load_factored_model(..., cg=True), kit = 1 with
    H_alpha and erank 1; the second run has a trace row and a sparse row stored (a hybrid block)."""
    import scipy.sparse as sp
    from loraine_jl_amd._capi import LoraineHipError
    from loraine_jl_amd.optimizer import Optimizer
    from loraine_jl_amd.synthetic import FactoredLowRankProblem
    m = 40
    stored = None
    if hybrid:
        row = sp.lil_matrix((m, m))
        row[3, 3], row[10, 10] = 1.0, -1.0
        row[3, 25] = row[25, 3] = 0.5
        stored = [(0, sp.identity(m, format="csc")), (37, row.tocsc())]
    P = FactoredLowRankProblem(m, 60, krank=2, xrank=2, seed=11, stored=stored)
    o = Optimizer()
    o.set_silent(True)
    for k, v in dict(kit=1, preconditioner=1, erank=1).items():
        o.set_attribute(k, v)
    o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True, factored_form=1, cg=True)
    o.optimize()
    s = o.solver
    print("CGFAC solve %s: status %d, %d iterations, %d CG iterations, objective %.10f planted %.10f | H in mode 1 %d, "
          "over budget %d, ts blocks from factors %d, stored rows %d"
          % ("hybrid" if hybrid else "pure", s.status, s.iter, s.cg_iter_tot, o.objective_value(), P.optimum,
             s.dev.count("hop_assemble_lowrank"), s.dev.count("hop_over_budget"), s.dev.count("prec_ts_factored"),
             s.dev.count("prec_ts_stored_rows")))
    assert s.model.factored and s.model.factored_cg and s.kit == 1
    assert s.status == 1 and o.termination_status() == "OPTIMAL"
    assert abs(o.objective_value() - P.optimum) <= 1e-6 * (1 + abs(P.optimum))
    assert s.cg_iter_tot > 0
    assert s.dev.count("prec_ts_factored") == 1 and s.dev.count("prec_ts_stored_rows") == (2 if hybrid else 0)
    assert "hop_over_budget" in s.trace[-1] and "op_quadform_fused" in s.trace[-1]
    # no row of AA for a factored constraint, on the host or on the device
    assert s.model.AA[0].nnz == (sum(a.nnz for _, a in stored) if hybrid else 0)
    for k in (1, 36, 59):
        with pytest.raises(LoraineHipError, match="factored"):
            s.dev.get_constraint(0, k)


# ---------------------------------------------------------------------------------------------- 6: defaults
def _refused(dev, n):
    from loraine_jl_amd._capi import LoraineHipError
    with pytest.raises(LoraineHipError, match="factored"):
        dev.matvec(np.ones(n))
    with pytest.raises(LoraineHipError, match="factored"):
        dev.prec_setup(1, 1, 1)
    with pytest.raises(LoraineHipError, match="factored"):
        dev.pcg(np.ones(n), 1e-6)


@pytest.mark.parametrize("name", ["F1", "F1h"])
def test_default_option_still_refuses(dev, name):
    case = _upload(dev, name)
    n = case.model.n
    _refused(dev, n)
    with options(dev, cg_factored=1):
        dev.matvec(np.ones(n))
        assert dev.prec_setup(1, 1, 1) == 0
        dev.pcg(case.h, 1e-3, 5)
    _refused(dev, n)
