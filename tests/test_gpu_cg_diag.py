"""GPU: the CG path on factored blocks with diagonal parts, A_k = diag(a_k) + V_k D_k V_k' (library option cg_diag beside
cg_factored; csrc/cgops.hip: the guard no_diag, csrc/prec.hip: the call in prec_setup, csrc/diagops.hip: ts_diag_mfma_kernel, csrc/hop.hip:
the mode-1 terms of the cost model and the budget) against the extended-precision reference of oracle/cg_reference.py.

The inputs are those of tests/cg_diag_cases.py (D1, D1a, D1h, D2, D3: the models of tests/cg_lowrank_cases.py with diagonal
parts) loaded as factored models; the reference H, case_run and the oracle are those of the materialised model.
tests/test_cg_diag_cpu.py asserts on the CPU that the algebra itself costs what the oracle costs, and checks the ts formula
apart from the kernel.

Bounds are those of tests/test_gpu_cg_factored.py: 20 x the oracle's distance from the longdouble reference, never more than
1e-6 on x, 2 tol on the true residual, 1e-9 on the apply.  Every test prints the oracle's and the device's distance."""
import contextlib
import functools
import types

import numpy as np
import pytest
import scipy.sparse as sp

import cg_diag_cases as dg
import cg_factored_cases as fc
import cg_lowrank_cases as lc
import diag_factored_cases as dfc
from oracle import cg_reference as cr
from oracle import loraine_oracle as lo

pytestmark = pytest.mark.gpu

DEFAULTS = dict(prec_eig=0, matvec_h=0, prec_inv=-1, prec_dense=0, cg_factored=0, cg_diag=0, fac_op_scaled=-1, fac_quadform=-1,
                hop_max_mb=-1)
FACTOR = 20.0
FORMS = [(0, 1), (1, 1), (1, 2)]       # (prec_inv, prec_dense): triangular solves, explicit inverse, one dense matrix
COUNTERS = ("op_factored_scaled", "op_quadform_fused", "op_diag", "hop_assemble", "hop_assemble_lowrank", "hop_over_budget",
            "hop_matvec", "matvec", "schur_diag")
NAMES = dg.NAMES


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


def _upload_model(dev, fm, dense_threshold=None):
    """What ResidentSolver does with a factored model: entries of the stored rows, factors, the declaration, the diagonal parts."""
    if dense_threshold is not None:
        dev.set_option("dense_threshold", dense_threshold)
    try:
        dev.upload_model(fm.AA, fm.sigmaA, fm.qA, fm.msizes, C_lin=fm.C_lin if fm.nlin else None)
    finally:
        dev.set_option("dense_threshold", -1.0)
    for i, (V, d, khat) in enumerate(fm.lowrank):
        dev.upload_lowrank(i, khat, V, d)
        dev.set_factored(i)
        if fm.diag[i]:
            rows = sorted(fm.diag[i])
            dev.upload_diag(i, rows, np.column_stack([fm.diag[i][k] for k in rows]))


def _upload(dev, name, with_G=True):
    case = dg.case_inputs(name)
    _upload_model(dev, dg.factored_model(name))
    assert dev.count("diag_rows") == dg.n_diag(name)
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
def _oracle_operator(dname):
    case, H = dg.case_data(dname)
    ref = H @ case.x.astype(cr.LD)
    y = np.zeros(case.model.n)
    lo.MyA(case.W, case.model.AA, case.model.nlin, case.model.C_lin, case.X_lin, case.S_lin_inv)(y, case.x)
    return ref, cr.relerr(y, ref)


def _apply_reference(case, erank, x):
    """(reference M_alpha^-1 x in longdouble, the float64 oracle's distance from it)."""
    ref = cr.reference_solver(case, 1, erank)(x)
    _, Mo = cr.oracle_state(case, 1, erank)
    z = np.zeros(case.model.n)
    Mo(z, x)
    return ref, cr.relerr(z, ref)


@functools.lru_cache(maxsize=None)
def _oracle_apply(dname, erank):
    case = dg.case_inputs(dname)
    return _apply_reference(case, erank, case.x)


@functools.lru_cache(maxsize=None)
def _oracle_pcg(dname, prec, erank):
    case, H = dg.case_data(dname)
    run = dg.case_run(dname, prec, erank)
    Ao, Mo = cr.oracle_state(case, prec, erank)
    out = []
    for maxit in (10000, run.K - 1):
        xo, ec, it = lo.cg(Ao, case.h, tol=run.tol, maxIter=maxit, precon=Mo)
        out.append(((ec, it), cr.relerr(xo, run.hist.x[it]), _herr(H, xo, run.hist.x[it], case.h)))
    return out


# ---------------------------------------------------------------------------------------------- 1: the operator
def _operator_twice(dev, name, tag):
    """A new scaling, dev.matvec(x) twice against H x of the reference -> the counter deltas of the two calls."""
    case = dg.case_inputs(name)
    ref, err_o = _oracle_operator(dg.data_name(name))
    _scale(dev, case)
    c0 = _counts(dev)
    y1 = dev.matvec(case.x)
    y2 = dev.matvec(case.x)
    d = _delta(c0, _counts(dev))
    err = cr.relerr(y1, ref)
    print("CGDIAG operator %s %s | oracle %.2e bound %.2e | device %.2e" % (name, tag, err_o, FACTOR * err_o, err))
    assert err <= FACTOR * err_o, (err, err_o)
    assert np.array_equal(y1, y2)
    return d


@pytest.mark.parametrize("name", NAMES)
def test_operator_with_diagonal_parts(dev, name):
    """matvec_h = 1: the matrix-free composition, with Q + column dots or the fused quadratic form for the factor part, the
    diagonal terms after it (op_diag: two per block and application); the scaled-factor form is never taken for a block with
    diagonal rows, also when it is forced.  matvec_h = 2: y = H x with H assembled in mode 1 (assemble_diag), once for the two
    calls.  hop_max_mb = 0: no room for H, the matrix-free operator runs."""
    _upload(dev, name)
    nb = dg.n_blocks(name)
    with options(dev, cg_factored=1, cg_diag=1):
        for mh in (1, 2):
            for scaled in (0, 1):
                for quad in (0, 1):
                    with options(dev, matvec_h=mh, fac_op_scaled=scaled, fac_quadform=quad):
                        d = _operator_twice(dev, name, "mh=%d scaled=%d quadform=%d" % (mh, scaled, quad))
                    assert d["op_factored_scaled"] == 0
                    if mh == 1:
                        assert d["op_diag"] == 2 * 2 * nb
                        assert d["op_quadform_fused"] == 2 * nb * quad
                        assert d["hop_assemble"] == d["hop_matvec"] == d["schur_diag"] == 0
                    else:
                        assert d["hop_assemble_lowrank"] == d["hop_assemble"] == 1 and d["hop_matvec"] == 2
                        assert d["schur_diag"] == nb and d["op_diag"] == 0 and d["op_quadform_fused"] == 0
                    assert d["hop_over_budget"] == 0
        with options(dev, matvec_h=2, hop_max_mb=0):
            d = _operator_twice(dev, name, "mh=2 hop_max_mb=0")
        assert d["hop_assemble"] == 0 and d["hop_matvec"] == 0 and d["hop_over_budget"] >= 1 and d["op_diag"] == 2 * 2 * nb


# ---------------------------------------------------------------------------------------------- 2: H_alpha
@pytest.mark.parametrize("with_G", [True, False], ids=["G", "W-only"])
@pytest.mark.parametrize("erank", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_halpha_apply_with_the_diagonal_rows_in_ts(dev, name, erank, with_G):
    """ts of every block from its factors (fac_ts_kernel), the stored rows of D1h from their entries, the term of the diagonal
    rows added by ts_diag_mfma_kernel; the apply in its three forms against the reference solve with prec_alpha_matrix of the
    materialised model."""
    case = _upload(dev, name, with_G=with_G)
    ref, err_o = _oracle_apply(dg.data_name(name), erank)
    bound = min(FACTOR * err_o, 1e-9)
    lin = case.model.nlin > 0
    res = []
    with options(dev, cg_factored=1, cg_diag=1, prec_eig=1):
        for inv, dense in FORMS:
            with options(dev, prec_inv=inv, prec_dense=dense):
                assert dev.prec_setup(1, erank, 1) == 0
                assert dev.count("prec_ts_factored") == dg.n_blocks(name)
                assert dev.count("prec_ts_stored_rows") == dg.n_stored(name)
                assert dev.count("prec_ts_diag_rows") == dg.n_diag(name)
                b0 = dev.count("prec_dense_build")
                z = dev.prec_apply(case.x)
                built = dev.count("prec_dense_build") - b0
                assert dev.prec_setup(1, erank, 1) == 0                      # a second setup: the same bits
                assert dev.count("prec_ts_diag_rows") == dg.n_diag(name)
                assert np.array_equal(z, dev.prec_apply(case.x))
                res.append((z, built))
    errs = [cr.relerr(y, ref) for y, _ in res]
    print("CGDIAG apply %s erank=%d %s | oracle %.2e bound %.2e | device potrs %.2e inverse %.2e dense %.2e"
          % (name, erank, "G" if with_G else "W-only", err_o, bound, errs[0], errs[1], errs[2]))
    assert [b for _, b in res] == [0, 0, 1 if (not lin and case.model.n >= 256) else 0]
    for e in errs:
        assert e <= bound, (errs, bound)


# ---------------------------------------------------------------------------------------------- 3: the kernel's edges
@functools.lru_cache(maxsize=None)
def _edge_case(m, n, khat, count):
    """A block of tests/diag_factored_cases.py (stored rows included) as a factored model and materialised, W with the spectrum
    of the other cases, a vector x."""
    from loraine_jl_amd.model import build_factored_model
    items = dfc.block_items(m, n, khat, count, 100 * m + n)
    F0 = -np.eye(m)
    fm = build_factored_model([F0], [items], np.zeros(n), factored_form=1)
    assert fm.factored and sorted(fm.diag[0]) == dfc.diag_rows(n, count)
    A = [[sp.csc_matrix(F0)] + [sp.csc_matrix(dfc.dense_of(it)) for it in items]]
    model = lo.make_model(A, np.zeros(n), 0.0, None, None)
    rng = np.random.default_rng(1000 * m + n + count)
    W, G = cr.scaling_from_spectrum(cr.spectrum(m, top=min(4, m - 1)), rng)
    case = types.SimpleNamespace(name="edge", model=model, W=[W], G=[G], X_lin=np.zeros(0), S_lin_inv=np.zeros(0),
                                 x=rng.standard_normal(n))
    return fm, case


_EIG = {}


@contextlib.contextmanager
def _eig_ld_once():
    """cr.prec_alpha_matrix computes cr.eig_ld(W) anew for every erank -- six seconds at msz 333, the whole cost of the reference
    there.  Inside this block the same function runs once per matrix and process and its result is shared (never modified)."""
    import hashlib
    orig = cr.eig_ld

    def once(W):
        key = (W.shape, hashlib.sha1(np.ascontiguousarray(W).tobytes()).hexdigest())
        if key not in _EIG:
            _EIG[key] = orig(W)
        return _EIG[key]

    cr.eig_ld = once
    try:
        yield
    finally:
        cr.eig_ld = orig


@pytest.mark.parametrize("erank", [1, 2])
@pytest.mark.parametrize("m,n,khat,count", dfc.CASES)
def test_ts_kernel_at_its_edges(dev, m, n, khat, count, erank):
    """msz 13 (one partial K step), 16 (one K step), 33, 65 (the second tile of columns of L starts at K = 64 and has one
    column), 72 (it has eight, and a second tile of 65 diagonal rows beside it), 130, 333 (six tiles, K starts 0 .. 320); 1, 3,
    63 / 64 / 65, 130 diagonal rows; with the stored rows of the generator (an identity, a 9-entry
    matrix, a dense slot).  The apply against the longdouble H_alpha of the materialised model."""
    fm, case = _edge_case(m, n, khat, count)
    with _eig_ld_once():
        ref, err_o = _apply_reference(case, erank, case.x)
    bound = min(FACTOR * err_o, 1e-9)
    _upload_model(dev, fm, float(m * m))
    _scale(dev, case)
    with options(dev, cg_factored=1, cg_diag=1, prec_eig=1):
        assert dev.prec_setup(1, erank, 1) == 0
        assert dev.count("prec_ts_diag_rows") == count and dev.count("prec_ts_stored_rows") == len(fm.stored[0])
        z = dev.prec_apply(case.x)
        assert dev.prec_setup(1, erank, 1) == 0
        assert np.array_equal(z, dev.prec_apply(case.x))
    err = cr.relerr(z, ref)
    print("CGDIAG edges m=%d n=%d khat=%d rows=%d erank=%d | oracle %.2e bound %.2e | device %.2e"
          % (m, n, khat, count, erank, err_o, bound, err))
    assert err <= bound, (err, bound)


# ---------------------------------------------------------------------------------------------- 4: lrn_pcg
@pytest.mark.parametrize("mh", [1, 2], ids=["matrixfree", "assembledH"])
@pytest.mark.parametrize("prec,erank", lc.PRECS, ids=["prec%d-erank%d" % p for p in lc.PRECS])
@pytest.mark.parametrize("name", ["D1", "D1h", "D2"])
def test_pcg_on_models_with_diagonal_parts(dev, name, prec, erank, mh):
    """(30, K) exactly at the tolerance in the gap, (-2, K - 1) at maxit = K - 1, x and the true residual those of the
    reference."""
    case, H = dg.case_data(name)
    _upload(dev, name)
    run = dg.case_run(name, prec, erank)
    K, tol = run.K, run.tol
    orc = _oracle_pcg(dg.data_name(name), prec, erank)
    assert orc[0][0] == (30, K) and orc[1][0] == (-2, K - 1)
    with options(dev, cg_factored=1, cg_diag=1, prec_eig=1, matvec_h=mh):
        assert dev.prec_setup(prec, erank, 1) == 0
        c0 = _counts(dev)
        got = [dev.pcg(case.h, tol, 10000), dev.pcg(case.h, tol, K - 1)]
        d = _delta(c0, _counts(dev))
        tsf, tsd = dev.count("prec_ts_factored"), dev.count("prec_ts_diag_rows")
    checks = []
    for (x, ec, it), want, (_, ex_o, er_o) in zip(got, ((30, K), (-2, K - 1)), orc):
        xref = run.hist.x[want[1]]
        ex, er = cr.relerr(x, xref), _herr(H, x, xref, case.h)
        res = cr.true_residual(H, x, case.h)
        print("CGDIAG pcg %s prec=%d erank=%d mh=%d K=%d tol=%.3e exit=(%d,%d) want=(%d,%d) | x: oracle %.2e device %.2e | "
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
    assert (d["op_diag"] > 0) == (mh == 1) and d["op_factored_scaled"] == 0
    assert tsf == (dg.n_blocks(name) if prec == 1 else 0) and tsd == (dg.n_diag(name) if prec == 1 else 0)


# ---------------------------------------------------------------------------------------------- 5: solve
def test_kit1_solve_with_the_trace_row_as_a_diagonal_part():
    """The planted msz 40 / nvar 60 / rank-2 problem of tests/test_gpu_cg_factored.py::test_kit1_solve_of_a_factored_model (seed
    11, the sparse row at 37 stored) with the trace row given as (None, [], ones): load_factored_model(..., cg="diag"), kit = 1,
    H_alpha, erank 1.  No entry of the identity exists anywhere."""
    from loraine_jl_amd.optimizer import Optimizer
    from loraine_jl_amd.synthetic import FactoredLowRankProblem
    m = 40
    row = sp.lil_matrix((m, m))
    row[3, 3], row[10, 10] = 1.0, -1.0
    row[3, 25] = row[25, 3] = 0.5
    P = FactoredLowRankProblem(m, 60, krank=2, xrank=2, seed=11, stored=[(0, sp.identity(m, format="csc")), (37, row.tocsc())])
    factors = P.factors()
    factors = [[(None, [], np.ones(m))] + factors[0][1:]]
    o = Optimizer()
    o.set_silent(True)
    for k, v in dict(kit=1, preconditioner=1, erank=1).items():
        o.set_attribute(k, v)
    o.load_factored_model(P.F0(), factors, P.b, max_sense=True, factored_form=1, cg="diag")
    try:
        o.optimize()
        s = o.solver
        print("CGDIAG solve: status %d, %d iterations, %d CG iterations, objective %.10f planted %.10f | H in mode 1 %d, over "
              "budget %d, ts blocks from factors %d, stored rows %d, diagonal rows %d"
              % (s.status, s.iter, s.cg_iter_tot, o.objective_value(), P.optimum, s.dev.count("hop_assemble_lowrank"),
                 s.dev.count("hop_over_budget"), s.dev.count("prec_ts_factored"), s.dev.count("prec_ts_stored_rows"),
                 s.dev.count("prec_ts_diag_rows")))
        assert s.model.factored and s.model.factored_cg and s.model.factored_cg_diag and s.kit == 1
        assert sorted(s.model.diag[0]) == [0] and sorted(s.model.stored[0]) == [37]
        assert s.status == 1 and o.termination_status() == "OPTIMAL"
        assert abs(o.objective_value() - P.optimum) <= 1e-6 * (1 + abs(P.optimum))
        assert s.cg_iter_tot > 0
        assert s.dev.count("diag_rows") == 1 and s.dev.count("prec_ts_factored") == 1
        assert s.dev.count("prec_ts_diag_rows") == 1 and s.dev.count("prec_ts_stored_rows") == 1
        assert "prec_ts_diag_rows" in s.trace[-1]
        assert s.model.AA[0].nnz == row.tocsc().nnz                 # no entry of the identity in AA
    finally:
        if o.solver is not None:                                    # (the device may serve another solve: the defaults again)
            o.solver.dev.set_option("cg_diag", 0)
            o.solver.dev.set_option("cg_factored", 0)


# ---------------------------------------------------------------------------------------------- 6: defaults and refusals
def _refused(dev, n, text):
    from loraine_jl_amd._capi import LoraineHipError
    with pytest.raises(LoraineHipError, match="lrn_matvec: .*diagonal parts.*" + text):
        dev.matvec(np.ones(n))
    with pytest.raises(LoraineHipError, match="lrn_prec_setup: .*diagonal parts.*" + text):
        dev.prec_setup(1, 1, 1)
    with pytest.raises(LoraineHipError, match="lrn_prec_apply: .*diagonal parts.*" + text):
        dev.prec_apply(np.ones(n))
    with pytest.raises(LoraineHipError, match="lrn_pcg: .*diagonal parts.*" + text):
        dev.pcg(np.ones(n), 1e-6)


def _partial_refused(dev, n):
    from loraine_jl_amd._capi import ptr
    x, out = np.ones(n), np.zeros(n)
    assert dev.lib.lrn_matvec_partial(dev.h, ptr(x), ptr(out)) != 0
    msg = dev.lib.lrn_last_error(dev.h).decode()
    assert "lrn_matvec_partial" in msg and "diagonal parts" in msg


def test_defaults_and_refusals(dev):
    case = _upload(dev, "D1")
    n = case.model.n
    parent = "the CG path does not hold them, such a model is solved with kit = 0"
    for cgf in (0, 1):                                   # cg_diag = 0: the text the library has always had, whatever cg_factored says
        with options(dev, cg_factored=cgf):
            _refused(dev, n, parent)
            _partial_refused(dev, n)
    with options(dev, cg_diag=1):                        # cg_diag alone opens nothing
        _refused(dev, n, parent)
        _partial_refused(dev, n)
    with options(dev, cg_factored=1, cg_diag=1):
        dev.matvec(np.ones(n))
        assert dev.prec_setup(1, 1, 1) == 0
        dev.prec_apply(np.ones(n))
        dev.pcg(case.h, 1e-3, 5)
        _partial_refused(dev, n)                         # not sharded: the partial mat-vec and world > 1 stay refused
        dev.set_shard(0, 2)
        try:
            _refused(dev, n, "one GPU")
            _partial_refused(dev, n)
        finally:
            dev.set_shard(0, 1)
    _refused(dev, n, parent)


def test_a_model_without_diagonal_rows_keeps_its_routes_under_cg_diag(dev):
    """F1h of tests/cg_factored_cases.py under cg_factored = 1 and cg_diag = 1: the counters of tests/test_gpu_cg_factored.py, no
    counter of the diagonal parts moves, and the results are those of cg_diag = 0 bit for bit."""
    name = "F1h"
    fm = fc.factored_model(name)
    case = lc.case_inputs(fc.base(name))
    out = {}
    for cgd in (0, 1):
        dev.upload_model(fm.AA, fm.sigmaA, fm.qA, fm.msizes)
        for i, (V, d, khat) in enumerate(fm.lowrank):
            dev.upload_lowrank(i, khat, V, d)
            dev.set_factored(i)
        assert dev.count("diag_rows") == 0
        with options(dev, cg_factored=1, cg_diag=cgd, prec_eig=1):
            ys = []
            for mh in (1, 2):
                with options(dev, matvec_h=mh, fac_op_scaled=1, fac_quadform=1):
                    _scale(dev, case)
                    c0 = _counts(dev)
                    ys.append(dev.matvec(case.x))
                    ys.append(dev.matvec(case.x))
                    d = _delta(c0, _counts(dev))
                assert d["op_diag"] == d["schur_diag"] == 0 and d["hop_over_budget"] == 0
                if mh == 1:
                    assert d["op_factored_scaled"] == 2 * fc.n_pure(name) and d["op_quadform_fused"] == 2 * fc.n_blocks(name)
                    assert d["hop_assemble"] == d["hop_matvec"] == 0
                else:
                    assert d["hop_assemble_lowrank"] == d["hop_assemble"] == 1 and d["hop_matvec"] == 2
            assert dev.prec_setup(1, 2, 1) == 0
            assert dev.count("prec_ts_factored") == fc.n_blocks(name) and dev.count("prec_ts_stored_rows") == fc.n_stored(name)
            assert dev.count("prec_ts_diag_rows") == 0
            out[cgd] = ys + [dev.prec_apply(case.x)]
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
