"""GPU: the data operators of a mixed-rank factored block on the compacted columns of its rank classes (library options ragged_ops
and ragged_ops_split; csrc/raggedops.hip, csrc/ragged_plan.h) through Device / the C ABI, on the cases R1 .. R6 of
tests/ragged_cases.py:

    the resident operators AA vec(X) and Rd = mat(AA' y) (C = S = 0, as tests/test_gpu_hybrid_factored.py::_operators) under
    option 0 and option 1 against NumPy from the materialised constraints, symmetry, reproducibility, the counters;
    forced K-splits of the syrk (ragged_ops_split) on R3 and R4;
    the CG operator (cg_factored = 1, matvec_h = 1) in its four forms fac_op_scaled x fac_quadform against NumPy;
    the fallbacks (uniform block, lrn_set_shard(0, 2)), option 0 after option 1, the plan built by the first operator call;
    solves of the planted problem through Optimizer.load_factored_model(ragged="ops").

Bounds: 1e-12 relative (2-norm of a vector, Frobenius norm of a matrix), the suite's own for a product against another
formulation; tests/test_ragged_ops_cpu.py shows that a float64 evaluation of the same algebra on these inputs stays inside it.
Solves: rel 1e-8 between two solves of one problem, 1e-6 against the planted optimum in the form tests/test_gpu_ragged.py uses
for the same problem.  Every comparison prints its figure before it asserts."""
import contextlib

import numpy as np
import pytest

import ragged_cases as rc
from loraine_jl_amd.model import ragged_chunks, ragged_plan

pytestmark = pytest.mark.gpu

TOL = 1e-12
DEFAULTS = dict(ragged_ops=0, ragged_ops_split=0, lowrank_ragged=0, cg_factored=0, cg_diag=0, cg_lowrank=0, matvec_h=0,
                fac_op_scaled=-1, fac_quadform=-1)
COUNTERS = ("op_ragged", "ragged_ops_fallback", "op_factored", "op_quadform_fused", "op_factored_scaled", "schur_ragged")
OUT_R6 = [0, 3, 7]          # R6: stored rows 0, 7 and the purely diagonal row 3 -- no factor column, no group


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


def _upload(dev, fm):
    dev.upload_model(fm.AA, fm.sigmaA, fm.qA, fm.msizes, C_lin=fm.C_lin if fm.nlin else None)
    for i, (V, d, khat) in enumerate(fm.lowrank):
        dev.upload_lowrank(i, khat, V, d)
        dev.set_factored(i)
        dg = fm.diag[i] if getattr(fm, "diag", None) else {}
        if dg:
            rows = sorted(dg)
            dev.upload_diag(i, rows, np.column_stack([dg[k] for k in rows]))


def _sym(m, seed):
    R = np.random.default_rng(seed).standard_normal((m, m))
    return 0.5 * (R + R.T)


def _inputs(name):
    n = rc.nvar(name)
    Xs = [_sym(m, 40 + m + i) for i, m in enumerate(rc.msizes(name))]
    return Xs, np.random.default_rng(n + 1).standard_normal(n)


def _materialised(name):
    return [[rc.materialise(it, m) for it in items] for items, m in zip(rc.blocks(name), rc.msizes(name))]


def _reference(name):
    """AA vec(X) = -sum over blocks of <A_k, X_i>, Rd_i = sum_k y_k A_i,k (C = S = 0), float64 from the materialised constraints."""
    Xs, y = _inputs(name)
    aax = np.zeros(rc.nvar(name))
    Rd = []
    for As, X in zip(_materialised(name), Xs):
        aax -= np.array([np.sum(a * X) for a in As])
        Rd.append(sum(yk * a for yk, a in zip(y, As)))
    return aax, Rd


def _operators(dev, name):
    """AA vec(X) and Rd through the resident entry points on the model as uploaded -> (aax, [Rd], counter deltas)."""
    Xs, y = _inputs(name)
    for i, X in enumerate(Xs):
        dev.ip_set_c(i, np.zeros_like(X))
        dev.ip_set_iterate(i, X, np.zeros_like(X))
    c0 = {k: dev.count(k) for k in COUNTERS}
    aax = dev.ip_aa_x()
    dev.ip_residual_d(y)
    Rd = [dev.dbg_get_block(i, "Rd")[0] for i in range(len(Xs))]
    return aax, Rd, {k: dev.count(k) - c0[k] for k in COUNTERS}


def _errors(name, aax, Rd):
    aref, Rref = _reference(name)
    return rc.relerr(aax, aref), max(rc.relerr(a, b) for a, b in zip(Rd, Rref))


# ---------------------------------------------------------------------------------------------- resident operators
@pytest.mark.parametrize("name", rc.NAMES)
def test_resident_operators_on_the_compacted_columns(dev, name):
    fm = rc.model(name)
    _upload(dev, fm)
    a0, R0, d0 = _operators(dev, name)
    with options(dev, ragged_ops=1):
        a1, R1, d1 = _operators(dev, name)
        a2, R2, _ = _operators(dev, name)
    e0, e1 = _errors(name, a0, R0), _errors(name, a1, R1)
    print("RAGGED-OPS %s | AA vec(X): padded %.2e ragged %.2e | Rd: padded %.2e ragged %.2e" % (name, e0[0], e1[0], e0[1], e1[1]))
    assert max(e1) < TOL
    assert max(e0) < TOL
    for a, b in zip(R1, R2):
        assert np.array_equal(a, a.T)                      # exactly symmetric
        assert np.array_equal(a, b)                        # fixed order, no atomics: the same bits
    assert np.array_equal(a1, a2)
    # one call of each operator per block by the new route, none fell back, op_factored counts as before
    assert d1["op_ragged"] == 2 * fm.nlmi and d1["ragged_ops_fallback"] == 0 and d1["op_factored"] == d0["op_factored"]
    assert d0["op_ragged"] == 0 and d0["ragged_ops_fallback"] == 0
    assert d1["schur_ragged"] == 0
    if name == "R1":                                       # the rank-0 row receives nothing from the factors
        assert a1[2] == 0.0
    if name == "R6":                                       # ... the stored and diagonal rows only their own terms
        aref, _ = _reference(name)
        assert rc.relerr(a1[OUT_R6], aref[OUT_R6]) < TOL


@pytest.mark.parametrize("split", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("name", ["R3", "R4"])
def test_forced_splits_of_the_syrk(dev, name, split):
    fm = rc.model(name)
    _upload(dev, fm)
    Rc = ragged_plan(rc.block_ranks(fm, 0))["Rc"]
    with options(dev, ragged_ops=1, ragged_ops_split=split):
        a1, R1, d1 = _operators(dev, name)
        chunks = dev.count("ragged_ops_chunks")
        dev.reset_timing()
        assert dev.count("ragged_ops_chunks") == chunks    # state: survives reset_timing
        a2, R2, _ = _operators(dev, name)
    e = _errors(name, a1, R1)
    print("RAGGED-OPS split %s ks=%d (clamped %d, Rc %d) | AA vec(X) %.2e Rd %.2e" % (name, split, chunks, Rc, e[0], e[1]))
    assert chunks == ragged_chunks(Rc, split)[0]
    assert max(e) < TOL
    assert np.array_equal(R1[0], R1[0].T)
    assert np.array_equal(R1[0], R2[0]) and np.array_equal(a1, a2)
    assert d1["op_ragged"] == 2 and d1["ragged_ops_fallback"] == 0


# ---------------------------------------------------------------------------------------------- CG operator
def _matvec_numpy(name, x):
    """AA vec(W mat(AA' x) W) as tests/test_gpu_cg_factored.py::_matvec_numpy forms it -- M = -sum_k x_k A_k, Z = W M W, y_k =
    -<A_k, Z> -- with A_k the materialised constraint, so that the stored and diagonal rows of R6 are included."""
    y = np.zeros(rc.nvar(name))
    for As, (W, _) in zip(_materialised(name), rc.scaling(name)):
        M = -sum(xk * a for xk, a in zip(x, As))
        Z = W @ M @ W
        y -= np.array([np.sum(a * Z) for a in As])
    return y


@pytest.mark.parametrize("name", ["R2", "R3", "R4", "R6"])
def test_cg_operator_in_its_four_forms(dev, name):
    fm = rc.model(name)
    _upload(dev, fm)
    n = rc.nvar(name)
    x = np.random.default_rng(77 + n).standard_normal(n)
    ref = _matvec_numpy(name, x)
    pure = 0 if name == "R6" else 1                        # (fac_op_scaled serves pure blocks without diagonal parts only)
    with options(dev, cg_factored=1, cg_diag=1, matvec_h=1):
        for scaled in (0, 1):
            for quad in (0, 1):
                for i, (W, G) in enumerate(rc.scaling(name)):      # (a new scaling: the operator choice is taken anew)
                    dev.set_scaling(i, W, G)
                with options(dev, fac_op_scaled=scaled, fac_quadform=quad):
                    yp = dev.matvec(x)
                    with options(dev, ragged_ops=1):
                        c0 = {k: dev.count(k) for k in COUNTERS}
                        y1 = dev.matvec(x)
                        y2 = dev.matvec(x)
                        d = {k: dev.count(k) - c0[k] for k in COUNTERS}
                ep, e1 = rc.relerr(yp, ref), rc.relerr(y1, ref)
                print("RAGGED-OPS matvec %s scaled=%d quadform=%d | padded %.2e ragged %.2e" % (name, scaled, quad, ep, e1))
                assert e1 < TOL
                assert ep < TOL
                assert np.array_equal(y1, y2)
                assert d["op_quadform_fused"] == 2 * quad and d["op_factored_scaled"] == 2 * pure * scaled
                assert d["op_ragged"] == 4 and d["ragged_ops_fallback"] == 0


def test_cg_operator_of_a_covered_materialised_block(dev):
    """R2's data as a materialised model with covering factors (build_model(..., factors=)), cg_lowrank = 1: the matrix-free
    operator goes through the factors of the block, and under ragged_ops through their compacted columns."""
    import scipy.sparse as sp
    from loraine_jl_amd.model import build_model
    m, n = rc.SIZES["R2"]
    facs = rc.factors("R2")
    A = [[sp.csc_matrix(-np.eye(m))] + [sp.csc_matrix(rc.materialise(f, m)) for f in facs]]
    mm = build_model(A, np.zeros(n), factors=[list(facs)])
    dev.upload_model(mm.AA, mm.sigmaA, mm.qA, mm.msizes)
    V, d, khat = mm.lowrank[0]
    dev.upload_lowrank(0, khat, V, d)
    W, G = rc.scaling("R2")[0]
    dev.set_scaling(0, W, G)
    x = np.random.default_rng(78).standard_normal(n)
    ref = _matvec_numpy("R2", x)
    with options(dev, cg_lowrank=1, matvec_h=1):
        yp = dev.matvec(x)
        with options(dev, ragged_ops=1):
            c0 = {k: dev.count(k) for k in COUNTERS}
            y1 = dev.matvec(x)
            y2 = dev.matvec(x)
            d1 = {k: dev.count(k) - c0[k] for k in COUNTERS}
    ep, e1 = rc.relerr(yp, ref), rc.relerr(y1, ref)
    print("RAGGED-OPS matvec covered R2 | padded %.2e ragged %.2e" % (ep, e1))
    assert e1 < TOL
    assert ep < TOL
    assert np.array_equal(y1, y2)
    assert d1["op_ragged"] == 4 and d1["ragged_ops_fallback"] == 0


# ---------------------------------------------------------------------------------------------- fallbacks and hygiene
def test_a_uniform_block_keeps_the_padded_bits(dev):
    from loraine_jl_amd.model import build_factored_model
    m, n = rc.SIZES["R3"]
    rng = np.random.default_rng(31)
    facs = [(rng.standard_normal((m, 1)) / np.sqrt(m), rng.choice([-1.0, 1.0], size=1)) for _ in range(n)]
    fm = build_factored_model([-np.eye(m)], [facs], np.zeros(n), factored_form=1)
    _upload(dev, fm)
    a0, R0, _ = _operators(dev, "R3")
    with options(dev, ragged_ops=1):
        a1, R1, d1 = _operators(dev, "R3")
    assert d1["ragged_ops_fallback"] == 2 and d1["op_ragged"] == 0
    assert np.array_equal(a0, a1) and np.array_equal(R0[0], R1[0])


def test_a_sharded_run_keeps_the_padded_bits(dev):
    _upload(dev, rc.model("R3"))
    dev.set_shard(0, 2)
    try:
        a0, R0, _ = _operators(dev, "R3")
        with options(dev, ragged_ops=1):
            a1, R1, d1 = _operators(dev, "R3")
    finally:
        dev.set_shard(0, 1)
    assert d1["ragged_ops_fallback"] == 2 and d1["op_ragged"] == 0
    assert np.array_equal(a0, a1) and np.array_equal(R0[0], R1[0])


@pytest.mark.parametrize("name", ["R2", "R6"])
def test_option_0_after_option_1_is_a_fresh_context(dev, name):
    import loraine_jl_amd
    fm = rc.model(name)
    _upload(dev, fm)
    with options(dev, ragged_ops=1, ragged_ops_split=3):
        _, _, d1 = _operators(dev, name)
        assert d1["op_ragged"] == 2
    a, R, d = _operators(dev, name)
    assert d["op_ragged"] == 0 and d["ragged_ops_fallback"] == 0
    fresh = loraine_jl_amd.Device(0)
    try:
        _upload(fresh, fm)
        af, Rf, df = _operators(fresh, name)
        assert df["op_ragged"] == 0 and fresh.count("ragged_ops_chunks") == 0
    finally:
        fresh.close()
    assert np.array_equal(a, af) and np.array_equal(R[0], Rf[0])


def test_the_first_operator_call_builds_the_plan():
    """ragged_ops = 1 with lowrank_ragged = 0 on a fresh context and a fresh upload: no assembly has run, the operator builds the
    plan and Vc itself."""
    import loraine_jl_amd
    d = loraine_jl_amd.Device(0)
    try:
        _upload(d, rc.model("R2"))
        d.set_option("ragged_ops", 1)
        a1, R1, d1 = _operators(d, "R2")
        assert d1["op_ragged"] == 2 and d1["schur_ragged"] == 0 and d.count("ragged_cols") == 0
    finally:
        d.close()
    e = _errors("R2", a1, R1)
    print("RAGGED-OPS first call R2 | AA vec(X) %.2e Rd %.2e" % e)
    assert max(e) < TOL


# ---------------------------------------------------------------------------------------------- solves
def _opt(**attrs):
    from loraine_jl_amd.optimizer import Optimizer
    o = Optimizer()
    o.set_silent(True)
    for k, v in attrs.items():
        o.set_attribute(k, v)
    return o


def test_planted_solve_kit_0():
    P = rc.Planted()
    runs = {}
    for ragged in (True, "ops"):
        o = _opt(kit=0)
        o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True, factored_form=1, ragged=ragged)
        o.optimize()
        runs[ragged] = o
        assert o.solver.model.ragged == ragged
        assert o.solver.dev.count("schur_ragged") > 0
        assert (o.solver.dev.count("op_ragged") > 0) == (ragged == "ops")
        assert o.solver.dev.count("ragged_ops_fallback") == 0
    a, b = runs[True], runs["ops"]
    print("RAGGED-OPS solve kit 0 | ragged=True: status %d, %d iterations, objective %.12e | ragged=\"ops\": status %d, %d "
          "iterations, objective %.12e | planted %.12e" % (a.solver.status, a.solver.iter, a.objective_value(), b.solver.status,
                                                            b.solver.iter, b.objective_value(), P.optimum))
    assert b.solver.status == 1 and a.solver.status == 1
    assert b.objective_value() == pytest.approx(a.objective_value(), rel=1e-8)


def test_planted_solve_kit_1():
    P = rc.Planted()
    o = _opt(kit=1, preconditioner=1, erank=1)
    o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True, factored_form=1, cg=True, ragged="ops")
    o.optimize()
    s = o.solver
    print("RAGGED-OPS solve kit 1 | status %d, %d iterations, %d CG iterations, objective %.10f planted %.10f | operator calls by "
          "rank class %d, fallbacks %d" % (s.status, s.iter, s.cg_iter_tot, o.objective_value(), P.optimum,
                                           s.dev.count("op_ragged"), s.dev.count("ragged_ops_fallback")))
    assert s.model.ragged == "ops" and s.model.factored_cg and s.kit == 1
    assert s.dev.count("op_ragged") > 0 and s.dev.count("ragged_ops_fallback") == 0
    assert s.status == 1
    assert abs(o.objective_value() - P.optimum) <= 1e-6 * (1 + abs(P.optimum))
