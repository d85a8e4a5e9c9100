"""GPU: what else runs on the compacted columns of a mixed-rank factored block -- Y = W V with the cross terms of the stored
constraints and of the diagonal parts in the mode-1 assembly (library option ragged_cross; csrc/schur_factored.hip::factored_y,
fac_cross_kernel and fac_cross_coldot_kernel on the compacted layout of csrc/fac_cols.h, csrc/diagops.hip: the store map of
diag_sq) and ts of H_alpha (library option ragged_ts; csrc/prec.hip::prec_setup, csrc/facops.hip: fac_ts_kernel on that layout).

Cases: tests/ragged_rest_cases.py (X1, X2, T1) and the mixed-rank CG cases of tests/cg_factored_cases.py (F1, F1h, F2) and
tests/cg_diag_cases.py (D1, D1h, D2) as they are.  The fallback: D3 and L3 as a pure block (khat 1, a factor column for every
constraint, Rc = R).  F3 is no fallback case -- its two stored rows have no factor column, Rc = 63 of R = 65, the route
condition holds -- and runs with the compacted cases.  tests/test_ragged_rest_cpu.py asserts the algebra on the CPU.

Bounds are the project's own and are measured against the references, never against the padded route, whose figures are
printed beside: H -- 1e-12 relative Frobenius against the np.longdouble H (tests/test_gpu_ragged.py), over all of H and over
the rows and columns of the stored and diagonal constraints alone; the H_alpha apply -- min(20 x the oracle's float64 distance
from the longdouble solve, 1e-9) (tests/test_gpu_cg_diag.py); lrn_pcg -- exit code and iteration count of the longdouble
reference run; solves -- status 1 and 1e-6 against the planted optimum."""
import contextlib
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import cg_diag_cases as dg
import cg_factored_cases as fc
import cg_lowrank_cases as lc
import ragged_cases as rc
import ragged_rest_cases as rr
from loraine_jl_amd.model import ragged_plan
from oracle import cg_reference as cr

pytestmark = pytest.mark.gpu

TOL = 1e-12
FACTOR = 20.0
FORMS = [(0, 1), (1, 1), (1, 2)]       # (prec_inv, prec_dense): triangular solves, explicit inverse, one dense matrix
DEFAULTS = dict(lowrank_ragged=0, ragged_ops=0, ragged_cross=0, ragged_ts=0, cg_factored=0, cg_diag=0, matvec_h=0, prec_eig=0,
                prec_inv=-1, prec_dense=0, fac_cross_lds=-1, diag_sq_mfma=-1)
CROSS = ("schur_cross_ragged", "ragged_cross_fallback", "ragged_y_reused", "hybrid_cross_lds", "hybrid_cross_global",
         "hybrid_cross_dense", "diag_sq_rows", "diag_sq_mfma", "schur_ragged", "schur_diag")
TS = ("prec_ts_factored", "prec_ts_stored_rows", "prec_ts_diag_rows", "prec_ts_ragged")
CG_NAMES = ["T1", "F1", "F1h", "F2", "F3", "D1", "D1h", "D2"]      # (F3: khat 1, but its two stored rows have no column -- Rc = 63 of 65)


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


def _upload_fm(dev, fm, dense_threshold=None):
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


def _scale(dev, case, with_G=True):
    for i in range(case.model.nlmi):
        dev.set_scaling(i, case.W[i], case.G[i] if with_G else None)
    if case.model.nlin:
        dev.set_lin(case.X_lin, case.S_lin_inv)


def _counts(dev, keys):
    return {k: dev.count(k) for k in keys}


def _delta(c0, c1):
    return {k: c1[k] - c0[k] for k in c0}


# ---------------------------------------------------------------------------------------------- the mode-1 assembly
def _load_x(dev, name, with_G=True):
    m = rr.sizes(name)[0]
    _upload_fm(dev, rr.factored_model(name), float(m * m) if name == "X2" else None)      # (X2: constraint 5 in a dense slot)
    _scale(dev, rr.case(name), with_G)


def _h_errors(name, H):
    """(relative Frobenius error over all of H, over the rows and columns of the stored and diagonal constraints alone)."""
    ref = rr.reference_h(name)
    mask = np.zeros(ref.shape, dtype=bool)
    rows = rr.cross_rows(name)
    mask[rows, :] = True
    mask[:, rows] = True
    return rc.relerr(H, ref), rc.relerr(H[mask], ref[mask])


@pytest.mark.parametrize("lr", [0, 1], ids=["FF-padded", "FF-ragged"])
@pytest.mark.parametrize("with_G", [True, False], ids=["G", "W-only"])
@pytest.mark.parametrize("name", ["X1", "X2"])
def test_mode_1_cross_terms_on_the_compacted_columns(dev, name, with_G, lr):
    _load_x(dev, name, with_G)
    with options(dev, lowrank_ragged=lr):
        H0 = dev.schur_assemble(1, want_H=True)                  # the padded cross terms, against the same reference
        c0 = _counts(dev, CROSS)
        with options(dev, ragged_cross=1):
            H1 = dev.schur_assemble(1, want_H=True)
            d = _delta(c0, _counts(dev, CROSS))
            H2 = dev.schur_assemble(1, want_H=True)
    e0, e1 = _h_errors(name, H0), _h_errors(name, H1)
    print("RAGGED-REST H %s %s lowrank_ragged=%d | padded %.2e (cross rows %.2e) compacted %.2e (cross rows %.2e) | %s"
          % (name, "G" if with_G else "W-only", lr, e0[0], e0[1], e1[0], e1[1], d))
    assert max(e1) < TOL
    assert max(e0) < TOL
    assert d["schur_cross_ragged"] == 1 and d["ragged_cross_fallback"] == 0
    assert d["schur_ragged"] == lr and d["schur_diag"] == 1
    if name == "X2":
        assert d["hybrid_cross_dense"] == 1 and d["hybrid_cross_lds"] + d["hybrid_cross_global"] == 1
    # with W only the rank-class assembly has left W Vc in its workspace: hybrid_y forms no product of its own
    assert d["ragged_y_reused"] == (1 if (lr and not with_G) else 0)
    assert np.array_equal(H1, H2)                                # one writer per entry, fixed order: the same bits
    assert np.array_equal(H1, H1.T)


@pytest.mark.parametrize("mfma", [0, 1], ids=["diag_sq-rows", "diag_sq-mfma"])
@pytest.mark.parametrize("lds", [0, 1], ids=["gather-global", "gather-lds"])
def test_both_gathers_and_both_forms_of_diag_sq(dev, lds, mfma):
    """X2: the global-memory gather and the LDS one, the rows form and the MFMA form of diag_sq at the class sizes 16 .. 1 (one
    launch per class, after the one of H_DD)."""
    _load_x(dev, "X2")
    with options(dev, lowrank_ragged=1, ragged_cross=1, fac_cross_lds=lds, diag_sq_mfma=mfma):
        c0 = _counts(dev, CROSS)
        H = dev.schur_assemble(1, want_H=True)
        d = _delta(c0, _counts(dev, CROSS))
    e = _h_errors("X2", H)
    print("RAGGED-REST H X2 fac_cross_lds=%d diag_sq_mfma=%d | %.2e (cross rows %.2e) | %s" % (lds, mfma, e[0], e[1], d))
    assert max(e) < TOL
    assert d["hybrid_cross_lds" if lds else "hybrid_cross_global"] == 1
    assert d["hybrid_cross_global" if lds else "hybrid_cross_lds"] == 0
    ncls = ragged_plan(rr.block_ranks("X2"))["ncls"]
    assert d["diag_sq_mfma" if mfma else "diag_sq_rows"] == 1 + ncls and d["diag_sq_rows" if mfma else "diag_sq_mfma"] == 0


# ---------------------------------------------------------------------------------------------- H_alpha
def _cg_case(name):
    """(case, factored model) of a CG case."""
    if name == "T1":
        return rr.case(name), rr.factored_model(name)
    if name == "L3p":
        return lc.case_inputs("L3"), _pure_l3()
    if name.startswith("F"):
        return lc.case_inputs(fc.base(name)), fc.factored_model(name)
    return dg.case_inputs(name), dg.factored_model(name)


@functools.lru_cache(maxsize=None)
def _pure_l3():
    """L3 of tests/cg_lowrank_cases.py (msz 70 / nvar 65, every constraint of rank 1) as a pure factored model: Rc = R."""
    from loraine_jl_amd.model import build_factored_model
    case = lc.case_inputs("L3")
    m = case.model
    fm = build_factored_model([sp.csc_matrix(m.A[0][0])], [list(case.factors[0])], np.asarray(m.b, float), factored_form=1)
    assert fm.factored and not fm.stored[0] and not fm.diag[0]
    return fm


def _n_ragged(fm):
    """Blocks the compaction drops columns of: 0 < Rc < R."""
    out = 0
    for i, (_, _, khat) in enumerate(fm.lowrank):
        Rc = ragged_plan(rc.block_ranks(fm, i))["Rc"]
        out += 0 < Rc < fm.n * khat
    return out


@functools.lru_cache(maxsize=None)
def _apply_reference(name, erank):
    """(reference M_alpha^-1 x in longdouble, the float64 oracle's distance from it); D1h shares D1's data, F1h F1's."""
    case, _ = _cg_case(name)
    ref = cr.reference_solver(case, 1, erank)(case.x)
    _, Mo = cr.oracle_state(case, 1, erank)
    z = np.zeros(case.model.n)
    Mo(z, case.x)
    return ref, cr.relerr(z, ref)


def _ref_name(name):
    return {"D1h": "D1", "F1h": "F1"}.get(name, name)


@pytest.mark.parametrize("erank", [1, 2])
@pytest.mark.parametrize("name", CG_NAMES)
def test_halpha_apply_with_ts_from_the_compacted_columns(dev, name, erank):
    case, fm = _cg_case(name)
    nb, nr = fm.nlmi, _n_ragged(fm)
    assert nr == 1                                               # (F2, D2: the second block has uniform rank 1)
    _upload_fm(dev, fm)
    _scale(dev, case)
    ref, err_o = _apply_reference(_ref_name(name), erank)
    bound = min(FACTOR * err_o, 1e-9)
    out = []
    with options(dev, cg_factored=1, cg_diag=1, prec_eig=1):
        for inv, dense in FORMS:
            with options(dev, prec_inv=inv, prec_dense=dense):
                assert dev.prec_setup(1, erank, 1) == 0          # the padded route
                cp = _counts(dev, TS)
                zp = dev.prec_apply(case.x)
                with options(dev, ragged_ts=1):
                    f0 = dev.count("ragged_ts_fallback")
                    assert dev.prec_setup(1, erank, 1) == 0
                    cr_ = _counts(dev, TS)
                    fb = dev.count("ragged_ts_fallback") - f0
                    z = dev.prec_apply(case.x)
                    assert dev.prec_setup(1, erank, 1) == 0      # a second setup: the same bits
                    assert np.array_equal(z, dev.prec_apply(case.x))
                assert cp["prec_ts_ragged"] == 0 and cr_["prec_ts_ragged"] == nr and fb == nb - nr
                assert cr_["prec_ts_factored"] == cp["prec_ts_factored"] == nb
                assert cr_["prec_ts_stored_rows"] == cp["prec_ts_stored_rows"]
                assert cr_["prec_ts_diag_rows"] == cp["prec_ts_diag_rows"]
                out.append((cr.relerr(zp, ref), cr.relerr(z, ref)))
    print("RAGGED-REST apply %s erank=%d | oracle %.2e bound %.2e | (padded, compacted) potrs %.2e %.2e inverse %.2e %.2e dense "
          "%.2e %.2e" % (name, erank, err_o, bound, out[0][0], out[0][1], out[1][0], out[1][1], out[2][0], out[2][1]))
    for _, e in out:
        assert e <= bound, (out, bound)


# ---------------------------------------------------------------------------------------------- lrn_pcg
@pytest.mark.parametrize("mh", [1, 2], ids=["matrixfree", "assembledH"])
@pytest.mark.parametrize("prec,erank", [(1, 1), (1, 2)], ids=["prec1-erank1", "prec1-erank2"])
@pytest.mark.parametrize("name", ["D1h", "F2"])
def test_pcg_with_all_four_options(dev, name, prec, erank, mh):
    """(30, K) exactly at the tolerance in the gap, (-2, K - 1) at maxit = K - 1: the exits of the longdouble reference run."""
    case, fm = _cg_case(name)
    run = dg.case_run(name, prec, erank) if name.startswith("D") else lc.case_run(fc.base(name), prec, erank)
    K, tol = run.K, run.tol
    _upload_fm(dev, fm)
    _scale(dev, case)
    with options(dev, cg_factored=1, cg_diag=1, prec_eig=1, matvec_h=mh, lowrank_ragged=1, ragged_ops=1, ragged_cross=1,
                 ragged_ts=1):
        assert dev.prec_setup(prec, erank, 1) == 0
        c0 = _counts(dev, ("schur_ragged", "schur_cross_ragged", "op_ragged"))
        got = [dev.pcg(case.h, tol, 10000), dev.pcg(case.h, tol, K - 1)]
        d = _delta(c0, _counts(dev, c0))
        tsr = dev.count("prec_ts_ragged")
    print("RAGGED-REST pcg %s prec=%d erank=%d mh=%d K=%d tol=%.3e | exits (%d, %d) (%d, %d) | %s"
          % (name, prec, erank, mh, K, tol, got[0][1], got[0][2], got[1][1], got[1][2], d))
    assert (got[0][1], got[0][2]) == (30, K)
    assert (got[1][1], got[1][2]) == (-2, K - 1)
    assert tsr == 1
    if mh == 2:
        assert d["schur_ragged"] == 1 and d["schur_cross_ragged"] == 1 and d["op_ragged"] == 0
    else:
        assert d["schur_ragged"] == 0 and d["op_ragged"] > 0


# ---------------------------------------------------------------------------------------------- fallbacks and off-switches
@pytest.mark.parametrize("name", ["L3p", "D3"])
def test_a_uniform_block_keeps_the_padded_bits(dev, name):
    """khat 1 and a factor column for every constraint, Rc = R: L3 as a pure block (no Y is formed for it: the fallback of the
    cross terms has nothing to count) and D3, whose seventeen diagonal rows keep their factors."""
    case, fm = _cg_case(name)
    assert _n_ragged(fm) == 0
    _upload_fm(dev, fm)
    _scale(dev, case)
    with options(dev, cg_factored=1, cg_diag=1, prec_eig=1):
        H0 = dev.schur_assemble(1, want_H=True)
        assert dev.prec_setup(1, 1, 1) == 0
        z0 = dev.prec_apply(case.x)
        c0 = _counts(dev, ("ragged_cross_fallback", "ragged_ts_fallback", "schur_cross_ragged"))
        with options(dev, ragged_cross=1, ragged_ts=1):
            H1 = dev.schur_assemble(1, want_H=True)
            assert dev.prec_setup(1, 1, 1) == 0
            assert dev.count("prec_ts_ragged") == 0 and dev.count("prec_ts_factored") == 1
            z1 = dev.prec_apply(case.x)
        d = _delta(c0, _counts(dev, c0))
    assert d == dict(ragged_cross_fallback=1 if name == "D3" else 0, ragged_ts_fallback=1, schur_cross_ragged=0)
    assert np.array_equal(H1, H0)
    assert np.array_equal(z1, z0)


def _h_and_apply(dev, name):
    """H of mode 1, and for a CG case the H_alpha apply, with the options as they stand."""
    if name == "X1":
        _load_x(dev, name)
        return [dev.schur_assemble(1, want_H=True)]
    case, fm = _cg_case(name)
    _upload_fm(dev, fm)
    _scale(dev, case)
    with options(dev, cg_factored=1, cg_diag=1, prec_eig=1):
        H = dev.schur_assemble(1, want_H=True)
        assert dev.prec_setup(1, 1, 1) == 0
        return [H, dev.prec_apply(case.x)]


@pytest.mark.parametrize("name", ["X1", "D1h"])
def test_options_0_after_1_are_a_fresh_context(dev, name):
    import loraine_jl_amd
    with options(dev, ragged_cross=1, ragged_ts=1):
        _h_and_apply(dev, name)
        assert dev.count("schur_cross_ragged") > 0
    got = _h_and_apply(dev, name)
    fresh = loraine_jl_amd.Device(0)
    try:
        want = _h_and_apply(fresh, name)
        for k in ("schur_cross_ragged", "ragged_cross_fallback", "prec_ts_ragged", "ragged_ts_fallback", "ragged_y_reused"):
            assert fresh.count(k) == 0
    finally:
        fresh.close()
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_the_first_call_of_each_route_builds_the_plan():
    """A context no other rank-class route has touched (lowrank_ragged = 0, ragged_ops = 0): the cross terms on X1, ts on T1."""
    import loraine_jl_amd
    fresh = loraine_jl_amd.Device(0)
    try:
        _load_x(fresh, "X1")
        fresh.set_option("ragged_cross", 1)
        H = fresh.schur_assemble(1, want_H=True)
        assert fresh.count("schur_cross_ragged") == 1 and fresh.count("schur_ragged") == 0
        assert max(_h_errors("X1", H)) < TOL
        fresh.set_option("ragged_cross", 0)
        case, fm = _cg_case("T1")
        _upload_fm(fresh, fm)                                     # (a new upload drops the plan)
        _scale(fresh, case)
        for k, v in dict(cg_factored=1, cg_diag=1, prec_eig=1, ragged_ts=1).items():
            fresh.set_option(k, v)
        assert fresh.prec_setup(1, 1, 1) == 0
        assert fresh.count("prec_ts_ragged") == 1 and fresh.count("op_ragged") == 0
        ref, err_o = _apply_reference("T1", 1)
        assert cr.relerr(fresh.prec_apply(case.x), ref) <= min(FACTOR * err_o, 1e-9)
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------- solves
def _solve(P, ragged, **attrs):
    from loraine_jl_amd.optimizer import Optimizer
    o = Optimizer()
    o.set_silent(True)
    for k, v in attrs.items():
        o.set_attribute(k, v)
    o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True, factored_form=1, ragged=ragged,
                          cg="diag" if attrs.get("kit") == 1 else False)
    try:
        o.optimize()
        s = o.solver
        return dict(status=s.status, iters=s.iter, cg=getattr(s, "cg_iter_tot", 0), obj=o.objective_value(),
                    cross=s.dev.count("schur_cross_ragged"), ts=s.dev.count("prec_ts_ragged"), ragged=s.model.ragged)
    finally:
        if o.solver is not None:                                 # (the device may serve another solve: the defaults again)
            for k in ("ragged_cross", "ragged_ts", "ragged_ops", "lowrank_ragged", "cg_diag", "cg_factored"):
                o.solver.dev.set_option(k, 0)


@pytest.mark.parametrize("kit", [0, 1])
def test_planted_solve_with_a_trace_row(kit):
    """ragged_cases.Planted (msz 40 / nvar 60, two constraints of rank 6 among rank 1) with tr X as (None, [], ones)."""
    P = rr.PlantedTrace()
    attrs = dict(kit=0) if kit == 0 else dict(kit=1, preconditioner=1, erank=1)
    a = _solve(P, "ops", **attrs)
    b = _solve(P, "all", **attrs)
    print("RAGGED-REST solve kit %d | ops: status %d, %d iterations, %d CG, objective %.10f | all: status %d, %d iterations, %d CG, "
          "objective %.10f | planted %.10f | cross-term assemblies by group %d, ts blocks from the compacted columns %d"
          % (kit, a["status"], a["iters"], a["cg"], a["obj"], b["status"], b["iters"], b["cg"], b["obj"], P.optimum, b["cross"],
             b["ts"]))
    assert a["ragged"] == "ops" and b["ragged"] == "all"
    assert b["status"] == 1 and a["status"] == 1
    assert abs(b["obj"] - P.optimum) <= 1e-6 * (1 + abs(P.optimum))
    assert abs(a["obj"] - P.optimum) <= 1e-6 * (1 + abs(P.optimum))
    if kit == 0:
        assert b["cross"] > 0
    else:
        assert b["ts"] == 1
