"""GPU: the device PCG (csrc/cgops.hip: the two-launch recurrence, the host look-ahead; csrc/prec.hip: the H_alpha / H_beta setup
and the SMW apply in its three forms) against the extended-precision reference of oracle/cg_reference.py.

The inputs come from seeds (cr.build_case); tests/test_cg_reference_cpu.py asserts on the CPU that they are fair: the
tolerance lies in a gap of the reference's residual history (so the iteration count is determined: the device has to
return it EXACTLY), the iterates around it are well-conditioned functions of the data, the -13 exit is a clearly negative
p'Ap, the eigenvalues H_alpha is built from are separated.

Shapes (the smallest that reach each branch of pcg_dev: nwg = ceil(nvar / 256), per = ceil(nvar / nwg)):
  A  nvar 257, msz 23           2 workgroups, per 129, last slice 128
  B  nvar 514, msz 33           3 workgroups, per 172, last slice 170; ksz 33 / 99 (off the multiples of 16 and 32)
  C  nvar 300, msz 25 + 17, 5 linear rows      has_LD, second eigenvector pass, lin_diag for H_beta
  D  theta1 (nvar 104, msz 50)  one workgroup, the link to tests/test_gpu_scaling_cg.py
  E  nvar 300, msz 90           ksz 270: prec_inv = -1 takes the explicit inverse by itself

Bounds are not fixed in advance: the float64 oracle (loraine_oracle.cg, MyM) runs on the same inputs, its distance from
the reference is what float64 costs on this input, and the device gets 20 x that -- another summation order over <= 3
workgroups and 256 lanes moves rounding by a small multiple, not by orders of magnitude -- and never more than the
bounds tests/test_gpu_scaling_cg.py already grants (1e-6 on x, 2 tol on the residual, 1e-9 / 1e-7 on the apply)."""
import contextlib
import functools

import numpy as np
import pytest

from oracle import cg_reference as cr
from oracle import loraine_oracle as lo

pytestmark = pytest.mark.gpu

PRECS = [(0, 1), (2, 1), (1, 1), (1, 3)]
DEFAULTS = dict(prec_eig=0, matvec_h=0, pcg_lookahead=2, prec_inv=-1, prec_dense=0, schur_chol=-1)
FACTOR = 20.0


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


def _upload(dev, case, with_G=True):
    m = case.model
    dev.upload_model(m.AA, m.sigmaA, m.qA, m.msizes, C_lin=m.C_lin if m.nlin else None)
    for i in range(m.nlmi):
        dev.set_scaling(i, case.W[i], case.G[i] if with_G else None)
    if m.nlin:
        dev.set_lin(case.X_lin, case.S_lin_inv)


def _herr(H, x, xref, h):
    """||H (x - xref)|| / ||h||: the distance of the true residuals h - H x and h - H xref, in longdouble."""
    d = H @ (np.asarray(x, dtype=cr.LD) - np.asarray(xref, dtype=cr.LD))
    h = np.asarray(h, dtype=cr.LD)
    return float(np.sqrt(np.sum(d * d)) / np.sqrt(np.sum(h * h)))


@functools.lru_cache(maxsize=None)
def _oracle_pcg(name, prec, erank):
    """What float64 costs on this input: loraine_oracle.cg at (tol, maxit large) and at maxit = K - 1 against the
    reference -- ((exit, iterations), error of x, distance of the true residual) for each."""
    case, H = cr.case_data(name)
    run = cr.case_run(name, prec, erank)
    Ao, Mo = cr.oracle_state(case, prec, erank)
    out = []
    for maxit in (10000, run.K - 1):
        xo, ec, it = lo.cg(Ao, case.h, tol=run.tol, maxIter=maxit, precon=Mo)
        out.append(((ec, it), cr.relerr(xo, run.hist.x[it]), _herr(H, xo, run.hist.x[it], case.h)))
    return out


@pytest.mark.parametrize("mh", [1, 2], ids=["matrixfree", "assembledH"])
@pytest.mark.parametrize("prec,erank", PRECS, ids=["prec%d-erank%d" % p for p in PRECS])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_exit_count_and_iterate(dev, name, prec, erank, mh):
    """tol in the gap below rho[K-1]: (30, K) exactly; maxit = K - 1: (-2, K - 1); x is the reference's x_K / x_{K-1} and
    the true residual (longdouble) that of the reference, within 20 x the oracle's own error.  matvec_h = 2 applies the
    assembled H, whose reduction leaves the partial sums of p'Ap (qpart) to cg_b_kernel."""
    case, H = cr.case_data(name)
    run = cr.case_run(name, prec, erank)
    K, tol = run.K, run.tol
    orc = _oracle_pcg(name, prec, erank)
    assert orc[0][0] == (30, K) and orc[1][0] == (-2, K - 1)
    _upload(dev, case)
    with options(dev, prec_eig=1, matvec_h=mh):
        assert dev.prec_setup(prec, erank, 1) == 0
        n0 = dev.count("hop_matvec")
        got = [dev.pcg(case.h, tol, 10000), dev.pcg(case.h, tol, K - 1)]
        hops = dev.count("hop_matvec") - n0
    checks = []
    for (x, ec, it), want, (_, ex_o, er_o) in zip(got, ((30, K), (-2, K - 1)), orc):
        xref = run.hist.x[want[1]]
        ex, er = cr.relerr(x, xref), _herr(H, x, xref, case.h)
        res = cr.true_residual(H, x, case.h)
        print("PCGREF %s prec=%d erank=%d mh=%d K=%d tol=%.3e exit=(%d,%d) want=(%d,%d) | x: oracle %.2e device %.2e | "
              "H dx: oracle %.2e device %.2e | true residual %.4e (reference %.4e)"
              % (name, prec, erank, mh, K, tol, ec, it, want[0], want[1], ex_o, ex, er_o, er, res,
                 cr.true_residual(H, xref, case.h)))
        checks.append(((ec, it), want, ex, min(FACTOR * ex_o, 1e-6), er, FACTOR * er_o, res))
    for got_exit, want, ex, bx, er, br, res in checks:
        assert got_exit == want
        assert ex <= bx, (ex, bx)
        assert er <= br, (er, br)
        if want[0] == 30:
            assert res <= 2.0 * tol
    assert (hops > 0) == (mh == 2)


@functools.lru_cache(maxsize=None)
def _indefinite():
    case, H = cr.case_data("A-indefinite")
    hist = cr.pcg_history(H, cr.identity_solver(), case.h, 0.0, 50)
    Ao, Mo = cr.oracle_state(case, 0, 1)
    xo, ec, it = lo.cg(Ao, case.h, tol=0.0, maxIter=50, precon=Mo)
    assert hist.code == -13 and (ec, it) == (-13, hist.it)
    return case, hist, cr.relerr(xo, hist.x[hist.it - 1])


@pytest.mark.parametrize("mh", [1, 2], ids=["matrixfree", "assembledH"])
def test_alpha_invalid_exit(dev, mh):
    """W with two negative eigenvalues (set through set_scaling, no G): H is indefinite, p'Ap < 0 in iteration 5 of the
    reference.  The device leaves with the same (-13, it) and x = x_{it-1}: the step with the invalid alpha is not
    taken.  An ordinary numerical exit.  schur_chol = 0: the assembled H is formed from W itself, nothing factors W."""
    case, hist, ex_o = _indefinite()
    _upload(dev, case, with_G=False)
    with options(dev, matvec_h=mh, schur_chol=0):
        assert dev.prec_setup(0, 1, 1) == 0
        n0 = dev.count("hop_matvec")
        x, ec, it = dev.pcg(case.h, 0.0, 10000)
        hops = dev.count("hop_matvec") - n0
    ex = cr.relerr(x, hist.x[hist.it - 1])
    print("PCGREF A-indefinite mh=%d exit=(%d,%d) want=(-13,%d) | x: oracle %.2e device %.2e" % (mh, ec, it, hist.it, ex_o, ex))
    assert (ec, it) == (-13, hist.it)
    assert ex <= min(FACTOR * ex_o, 1e-6), (ex, ex_o)
    assert (hops > 0) == (mh == 2)


def _lookahead_runs(dev, h, runs):
    """Every (tol, maxit) of `runs` under pcg_lookahead 0, 1, 2, 8 and 99 (clamped to 8): [(x, exit, iterations), ...]"""
    out = {}
    try:
        for la in (0, 1, 2, 8, 99):
            dev.set_option("pcg_lookahead", la)
            out[la] = [dev.pcg(h, tol, maxit) for tol, maxit in runs]
    finally:
        dev.set_option("pcg_lookahead", 2)
    return out


def _assert_identical(out, wants):
    base = out[0]
    for (x, ec, it), want in zip(base, wants):
        assert (ec, it) == want
    for la, res in out.items():
        for (x, ec, it), (x0, ec0, it0) in zip(res, base):
            assert (ec, it) == (ec0, it0), (la, ec, it, ec0, it0)
            assert np.array_equal(x, x0), (la, float(np.abs(x - x0).max()))


@pytest.mark.parametrize("mh", [1, 2], ids=["matrixfree", "assembledH"])
@pytest.mark.parametrize("prec,erank", [(0, 1), (2, 1), (1, 1)], ids=["prec0", "prec2", "prec1"])
@pytest.mark.parametrize("name", ["B", "C"])
def test_lookahead_changes_neither_count_nor_result(dev, name, prec, erank, mh):
    """The host queues up to 8 iterations beyond the convergence test it has read; kernels queued beyond the last
    iteration must find the exit flag and leave x alone.  Same (code, iterations), bit-identical x, at convergence and
    at the maxit exit."""
    case, _ = cr.case_data(name)
    run = cr.case_run(name, prec, erank)
    _upload(dev, case)
    with options(dev, prec_eig=1, matvec_h=mh):
        assert dev.prec_setup(prec, erank, 1) == 0
        out = _lookahead_runs(dev, case.h, [(run.tol, 10000), (run.tol, run.K - 1)])
    _assert_identical(out, [(30, run.K), (-2, run.K - 1)])


def test_lookahead_changes_neither_count_nor_result_at_alpha_invalid(dev):
    case, hist, _ = _indefinite()
    _upload(dev, case, with_G=False)
    with options(dev, matvec_h=1):
        assert dev.prec_setup(0, 1, 1) == 0
        out = _lookahead_runs(dev, case.h, [(0.0, 10000)])
    _assert_identical(out, [(-13, hist.it)])


@functools.lru_cache(maxsize=None)
def _apply_reference(name, erank):
    """M_alpha^-1 x of the reference and the distance of the float64 MyM from it."""
    case = cr.case_inputs(name)
    ref = cr.reference_solver(case, 1, erank)(case.x)
    _, Mo = cr.oracle_state(case, 1, erank)
    z = np.zeros(case.model.n)
    Mo(z, case.x)
    return ref, cr.relerr(z, ref)


def _apply_bound(err_oracle, eig):
    """20 x the float64 MyM's own error, never looser than the bounds of test_preconditioner_apply_and_pcg: 1e-9 with
    the Jacobi eigendecomposition, 1e-7 with Lanczos (the project's bound for Ritz vectors, not re-derived here)."""
    return min(FACTOR * err_oracle, 1e-9 if eig == 1 else 1e-7)


def _apply_forms(dev, case, erank, forms):
    """prec_setup + prec_apply under each (prec_inv, prec_dense) of `forms`: [(M^-1 x, dense builds, dense applies), ...]"""
    out = []
    for inv, dense in forms:
        with options(dev, prec_inv=inv, prec_dense=dense):
            assert dev.prec_setup(1, erank, 1) == 0
            b0, a0 = dev.count("prec_dense_build"), dev.count("prec_dense_apply")
            y = dev.prec_apply(case.x)
            out.append((y, dev.count("prec_dense_build") - b0, dev.count("prec_dense_apply") - a0))
    return out


@pytest.mark.parametrize("eig", [1, 2], ids=["jacobi", "lanczos"])
@pytest.mark.parametrize("erank", [1, 3])
@pytest.mark.parametrize("name", ["B", "C"])
def test_smw_cores_and_dense_form_against_the_reference(dev, name, erank, eig):
    """prec_apply against M_alpha^-1 x with the SMW core as two triangular solves (prec_inv 0), as an explicit inverse
    with one refinement step (prec_inv 1) and, without linear rows, the whole preconditioner as one dense matrix
    (prec_dense 2, which exists only on top of the inverse form).  The route is read off the counters: a dense build
    happens exactly when the inverse form is in place, nvar >= 256 and AAAATtau is diagonal -- so prec_dense = 2 with
    prec_inv = 0, or with prec_inv = -1 at ksz < 256, must NOT build."""
    case = cr.case_inputs(name)
    ref, err_o = _apply_reference(name, erank)
    bound = _apply_bound(err_o, eig)
    lin = case.model.nlin > 0
    forms = [(0, 1), (1, 1), (1, 2), (0, 2), (-1, 2)]
    _upload(dev, case)
    with options(dev, prec_eig=eig):
        res = _apply_forms(dev, case, erank, forms)
    errs = [cr.relerr(y, ref) for y, _, _ in res]
    print("PCGREF apply %s erank=%d eig=%d | oracle %.2e bound %.2e | device potrs %.2e inverse %.2e dense %.2e"
          % (name, erank, eig, err_o, bound, errs[0], errs[1], errs[2]))
    routes = [(b, a) for _, b, a in res]
    assert routes == [(0, 0), (0, 0), (0, 0) if lin else (1, 1), (0, 0), (0, 0)]
    for e in errs:
        assert e <= bound, (errs, bound)
    for i in range(3):
        for j in range(i):
            assert cr.relerr(res[i][0], res[j][0]) <= bound


def test_inverse_form_is_taken_by_itself_at_ksz_270(dev):
    """msz 90, erank 3: ksz = 270 >= 256, prec_inv = -1 forms (S + I)^-1 (seen through the dense build it allows); the
    triangular solves at this ksz (above the 150 of the other tests) give the same M^-1 x."""
    case = cr.case_inputs("E")
    ref, err_o = _apply_reference("E", 3)
    bound = _apply_bound(err_o, 1)
    _upload(dev, case)
    with options(dev, prec_eig=1):
        res = _apply_forms(dev, case, 3, [(-1, 1), (-1, 2), (0, 1), (0, 2)])
    errs = [cr.relerr(y, ref) for y, _, _ in res]
    print("PCGREF apply E erank=3 eig=1 | oracle %.2e bound %.2e | device auto %.2e auto+dense %.2e potrs %.2e"
          % (err_o, bound, errs[0], errs[1], errs[2]))
    assert [(b, a) for _, b, a in res] == [(0, 0), (1, 1), (0, 0), (0, 0)]
    for e in errs:
        assert e <= bound, (errs, bound)
    for i in range(3):
        for j in range(i):
            assert cr.relerr(res[i][0], res[j][0]) <= bound


def test_halpha_setup_from_W_alone(dev):
    """set_scaling(W, None): the setup takes eig(W) from W itself (fromW: its singular values are its eigenvalues, the
    columns of the Jacobi factor are sigma u).  Same reference, same bound."""
    case = cr.case_inputs("B")
    ref, err_o = _apply_reference("B", 3)
    bound = _apply_bound(err_o, 1)
    _upload(dev, case, with_G=False)
    with options(dev, prec_eig=1):
        assert dev.prec_setup(1, 3, 1) == 0
        y = dev.prec_apply(case.x)
    err = cr.relerr(y, ref)
    print("PCGREF apply B erank=3 from W alone | oracle %.2e bound %.2e | device %.2e" % (err_o, bound, err))
    assert err <= bound, (err, bound)


def test_z_factorisation_exit_leaves_counters_and_context_clean(dev):
    """H_alpha on the indefinite W of the -13 case (from W alone, Jacobi route): 2W - Um Um' <= 2W has a negative
    eigenvalue and the largest shift of the retry ladder is 1e-9 of the mean |lambda|, so all four attempts at
    Z = chol(2W - Um Um') fail -- info != 0, three shifted retries counted, no part of ts reported.  An ordinary
    numerical exit out of the middle of the setup: the same context then sets up case A and applies H_alpha with the
    bits of a fresh context."""
    import loraine_jl_amd
    bad, good = cr.case_inputs("A-indefinite"), cr.case_inputs("A")
    ts_keys = ("prec_ts_factored", "prec_ts_stored_rows", "prec_ts_diag_rows", "prec_ts_ragged")
    _upload(dev, bad, with_G=False)
    with options(dev, prec_eig=1):
        z0 = dev.count("prec_z_shift")
        info = dev.prec_setup(1, 1, 1)
        shifts = dev.count("prec_z_shift") - z0
        ts_counts = [dev.count(k) for k in ts_keys]
        _upload(dev, good)
        info_good = dev.prec_setup(1, 1, 1)
        y = dev.prec_apply(good.x)
    fresh = loraine_jl_amd.Device(0)
    try:
        _upload(fresh, good)
        fresh.set_option("prec_eig", 1)
        assert fresh.prec_setup(1, 1, 1) == 0
        y_fresh = fresh.prec_apply(good.x)
    finally:
        fresh.close()
    print("PCGREF A-indefinite prec=1 info=%d z_shifts=%d ts counters %s | then A: info=%d, max |y - y_fresh| %.2e"
          % (info, shifts, ts_counts, info_good, float(np.abs(y - y_fresh).max())))
    assert info != 0
    assert shifts == 3
    assert ts_counts == [0, 0, 0, 0]
    assert info_good == 0
    assert np.array_equal(y, y_fresh)
