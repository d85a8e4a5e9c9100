"""GPU: factored constraints of rank 17 .. 64 (library option lowrank_wide; csrc/ragged_plan.h with seven classes,
csrc/raggedops.hip::ragged_wide_epilogue, the routing of csrc/schur_factored.hip::assemble_lowrank) through Device / the C ABI and
through Optimizer.load_factored_model(..., wide=True), on the cases of tests/wide_cases.py.

Bounds are the project's own: H -- 1e-12 relative Frobenius against the np.longdouble H (tests/test_gpu_ragged.py; tests/
test_wide_cpu.py shows a float64 evaluation in the device's order at 1e-16 on these inputs and every single fault above 1e-9); the
data operators -- 1e-12 relative (tests/test_gpu_ragged_ops.py), against np.longdouble; the H_alpha apply -- min(20 x the oracle's
float64 distance from the longdouble solve, 1e-9), lrn_pcg -- exit code and iteration count of the longdouble reference run (tests/
test_gpu_ragged_rest.py); solves -- rel 1e-8 between two solves of one problem, 1e-6 (1 + |optimum|) against the planted optimum.
Every comparison prints its figure before it asserts."""
import contextlib
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import ragged_cases as rc
import wide_cases as wc
from loraine_jl_amd.model import ragged_plan
from oracle import cg_reference as cr

pytestmark = pytest.mark.gpu

TOL = 1e-12
FACTOR = 20.0
LD = np.longdouble
DEFAULTS = dict(lowrank_wide=0, lowrank_ragged=0, ragged_ops=0, ragged_cross=0, ragged_ts=0, cg_factored=0, cg_diag=0, matvec_h=0,
                prec_eig=0, prec_inv=-1, prec_dense=0)
STATE = ("ragged_cols", "ragged_classes", "ragged_tiles")
ROUTES = ("schur_ragged", "schur_wide", "ragged_fallback")


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


def _counts(dev, keys):
    return {k: dev.count(k) for k in keys}


def _delta(c0, c1):
    return {k: c1[k] - c0[k] for k in c0}


def _upload(dev, fm, dense=False):
    """The model with its factors; dense: a full stored matrix goes to a dense slot (V3's constraint 1)."""
    if dense:
        dev.set_option("dense_threshold", float(int(fm.msizes[0]) ** 2))
    try:
        dev.upload_model(fm.AA, fm.sigmaA, fm.qA, fm.msizes, C_lin=fm.C_lin if fm.nlin else None)
    finally:
        dev.set_option("dense_threshold", -1.0)
    with options(dev, lowrank_wide=1):
        for i, (V, d, khat) in enumerate(fm.lowrank):
            dev.upload_lowrank(i, khat, V, d)
            dev.set_factored(i)


def _load(dev, name, with_G=True):
    fm = wc.model(name)
    _upload(dev, fm, dense=name == "V3")
    for i, (W, G) in enumerate(wc.scaling(name)):
        dev.set_scaling(i, W, G if with_G else None)
    if fm.nlin:
        dev.set_lin(np.ones(fm.nlin), np.ones(fm.nlin))
    return fm


def _plans(fm):
    return [ragged_plan(rc.block_ranks(fm, i), max_rank=64) for i in range(fm.nlmi)]


# ---------------------------------------------------------------------------------------------- mode 1
@pytest.mark.parametrize("with_G", [True, False], ids=["G", "W-only"])
@pytest.mark.parametrize("name", wc.NAMES)
def test_mode_1_of_a_wide_block(dev, name, with_G):
    fm = _load(dev, name, with_G)
    ref = wc.reference(name)
    plans = _plans(fm)
    nwide = sum(lr[2] > 16 for lr in fm.lowrank)
    nnarrow = fm.nlmi - nwide
    c0 = _counts(dev, ROUTES)
    H0 = dev.schur_assemble(1, want_H=True)                  # lowrank_ragged = 0: the wide block by rank class all the same
    d0 = _delta(c0, _counts(dev, ROUTES))
    state0 = _counts(dev, STATE)
    with options(dev, lowrank_ragged=1):
        c1 = _counts(dev, ROUTES)
        H1 = dev.schur_assemble(1, want_H=True)
        d1 = _delta(c1, _counts(dev, ROUTES))
        state1 = _counts(dev, STATE)
        H2 = dev.schur_assemble(1, want_H=True)
    e0, e1 = rc.relerr(H0, ref), rc.relerr(H1, ref)
    print("WIDE %s %s | lowrank_ragged 0: %.2e 1: %.2e | Rc %d of %d, classes %d, tiles %d | %s %s"
          % (name, "G" if with_G else "W-only", e0, e1, plans[0]["Rc"], fm.n * fm.lowrank[0][2], plans[0]["ncls"],
             plans[0]["tiles"], d0, d1))
    assert e0 < TOL
    assert e1 < TOL
    assert d0 == dict(schur_ragged=nwide, schur_wide=nwide, ragged_fallback=0)      # (a narrow block: the padded route)
    assert d1 == dict(schur_ragged=fm.nlmi, schur_wide=nwide, ragged_fallback=0)
    wide_plan = plans[0]                                     # (V4: block 0 is the wide one)
    assert state0 == dict(ragged_cols=wide_plan["Rc"], ragged_classes=wide_plan["ncls"], ragged_tiles=wide_plan["tiles"])
    last = plans[-1]                                         # the state counters are those of the last block assembled that way
    assert state1 == dict(ragged_cols=last["Rc"], ragged_classes=last["ncls"], ragged_tiles=last["tiles"])
    assert np.array_equal(H1, H2)                            # one writer per entry, fixed order: the same bits
    assert np.array_equal(H1, H1.T) and np.array_equal(H0, H0.T)
    if nnarrow == 0:
        assert np.array_equal(H0, H1)                        # the route of a wide block is forced: the option changes nothing
    if name == "V2":
        assert np.all(H1[15, :] == 0.0) and np.all(H1[:, 15] == 0.0)      # the rank-0 row


def _alone(dev, name, with_G, ragged):
    """H of one block of V4 as a model of its own, under lowrank_ragged = ragged."""
    _upload(dev, wc.block_model(name))
    W, G = wc.scaling("V4")[0 if name == "V1" else 1]
    dev.set_scaling(0, W, G if with_G else None)
    with options(dev, lowrank_ragged=ragged):
        return dev.schur_assemble(1, want_H=True)


@pytest.mark.parametrize("ragged", [0, 1])
@pytest.mark.parametrize("with_G", [True, False], ids=["G", "W-only"])
def test_the_narrow_block_beside_a_wide_one_keeps_its_bits(dev, with_G, ragged):
    """V4 = V1's block + a block of khat 2: H accumulates block 0 then block 1 into zeros, one rounding per entry -- so the bits of
    the narrow block's own assembly under the same option value are in it."""
    Hw = _alone(dev, "V1", with_G, ragged)
    c0 = _counts(dev, ROUTES)
    Hn = _alone(dev, "V4b", with_G, ragged)
    dn = _delta(c0, _counts(dev, ROUTES))
    assert dn == dict(schur_ragged=ragged, schur_wide=0, ragged_fallback=0)
    _load(dev, "V4", with_G)
    with options(dev, lowrank_ragged=ragged):
        H = dev.schur_assemble(1, want_H=True)
    assert np.array_equal(H, Hw + Hn)


def test_a_wide_block_without_a_weighted_column_adds_nothing(dev):
    """khat 32 and every weight 0 (Rc = 0): the assembly counts the wide block, launches no tile and leaves H zero."""
    m, n = wc.SIZES["V1"]
    fm = wc.block_model("V1")
    dev.upload_model(fm.AA, fm.sigmaA, fm.qA, fm.msizes)
    with options(dev, lowrank_wide=1):
        dev.upload_lowrank(0, 32, sp.csr_matrix((n * 32, m)), np.zeros(n * 32))
        dev.set_factored(0)
    W, G = wc.scaling("V1")[0]
    dev.set_scaling(0, W, G)
    for ragged in (0, 1):
        with options(dev, lowrank_ragged=ragged):
            c0 = _counts(dev, ROUTES)
            H = dev.schur_assemble(1, want_H=True)
            assert _delta(c0, _counts(dev, ROUTES)) == dict(schur_ragged=0, schur_wide=1, ragged_fallback=0)
        assert np.all(H == 0.0)


# ---------------------------------------------------------------------------------------------- data operators
def _sym(m, seed):
    R = np.random.default_rng(seed).standard_normal((m, m))
    return 0.5 * (R + R.T)


@functools.lru_cache(maxsize=None)
def _op_inputs(name):
    m, n = wc.SIZES[name]
    return _sym(m, 40 + m), np.random.default_rng(n + 1).standard_normal(n)


@functools.lru_cache(maxsize=None)
def _op_reference(name):
    """AA vec(X) = -<A_k, X> and Rd = sum_k y_k A_k (C = S = 0) in np.longdouble from the materialised constraints."""
    X, y = _op_inputs(name)
    As = [a.astype(LD) for a in wc.matrices(name)[0]]
    return -np.array([np.sum(a * X.astype(LD)) for a in As]), sum(LD(yk) * a for yk, a in zip(y, As))


def _operators(dev, name):
    X, y = _op_inputs(name)
    dev.ip_set_c(0, np.zeros_like(X))
    dev.ip_set_iterate(0, X, np.zeros_like(X))
    keys = ("op_ragged", "ragged_ops_fallback", "op_factored")
    c0 = _counts(dev, keys)
    aax = dev.ip_aa_x()
    dev.ip_residual_d(y)
    return aax, dev.dbg_get_block(0, "Rd")[0], _delta(c0, _counts(dev, keys))


@pytest.mark.parametrize("name", ["V2", "V3"])
def test_data_operators_padded_and_compacted(dev, name):
    _upload(dev, wc.model(name), dense=name == "V3")
    aref, Rref = _op_reference(name)
    a0, R0, d0 = _operators(dev, name)                       # the padded forms at khat 64
    with options(dev, ragged_ops=1):
        a1, R1, d1 = _operators(dev, name)
        a2, R2, _ = _operators(dev, name)
    e0 = (rc.relerr(a0, aref), rc.relerr(R0, Rref))
    e1 = (rc.relerr(a1, aref), rc.relerr(R1, Rref))
    print("WIDE ops %s | AA vec(X): padded %.2e compacted %.2e | Rd: padded %.2e compacted %.2e" % (name, e0[0], e1[0], e0[1], e1[1]))
    assert max(e0) < TOL
    assert max(e1) < TOL
    assert d0["op_ragged"] == 0 and d0["ragged_ops_fallback"] == 0
    assert d1["op_ragged"] == 2 and d1["ragged_ops_fallback"] == 0 and d1["op_factored"] == d0["op_factored"]
    assert np.array_equal(R1, R1.T) and np.array_equal(R1, R2) and np.array_equal(a1, a2)
    if name == "V2":
        assert a1[15] == 0.0 and a0[15] == 0.0               # the rank-0 row


# ---------------------------------------------------------------------------------------------- cross terms
@pytest.mark.parametrize("cross", [0, 1], ids=["cross-padded", "cross-compacted"])
@pytest.mark.parametrize("with_G", [True, False], ids=["G", "W-only"])
def test_cross_terms_of_the_hybrid_block(dev, with_G, cross):
    _load(dev, "V3", with_G)
    ref = wc.reference("V3")
    keys = ("schur_cross_ragged", "ragged_cross_fallback", "ragged_y_reused", "hybrid_cross_dense", "schur_wide")
    with options(dev, ragged_cross=cross):
        c0 = _counts(dev, keys)
        H1 = dev.schur_assemble(1, want_H=True)
        d = _delta(c0, _counts(dev, keys))
        H2 = dev.schur_assemble(1, want_H=True)
    rows = [wc.V3_TRACE, wc.V3_DENSE]
    mask = np.zeros(ref.shape, dtype=bool)
    mask[rows, :] = True
    mask[:, rows] = True
    e = (rc.relerr(H1, ref), rc.relerr(H1[mask], ref[mask]))
    print("WIDE cross V3 %s ragged_cross=%d | %.2e (stored rows %.2e) | %s" % ("G" if with_G else "W-only", cross, e[0], e[1], d))
    assert max(e) < TOL
    assert d["schur_wide"] == 1 and d["schur_cross_ragged"] == cross and d["ragged_cross_fallback"] == 0
    assert d["hybrid_cross_dense"] == 1
    assert d["ragged_y_reused"] == (1 if cross and not with_G else 0)
    assert np.array_equal(H1, H2) and np.array_equal(H1, H1.T)


# ---------------------------------------------------------------------------------------------- H_alpha and lrn_pcg
def _load_cg(dev):
    case, fm = wc.cg_case(), wc.cg_model()
    _upload(dev, fm, dense=True)
    dev.set_scaling(0, case.W[0], case.G[0])
    dev.set_lin(case.X_lin, case.S_lin_inv)
    return case


@functools.lru_cache(maxsize=None)
def _apply_reference(erank):
    case = wc.cg_case()
    ref = cr.reference_solver(case, 1, erank)(case.x)
    _, Mo = cr.oracle_state(case, 1, erank)
    z = np.zeros(case.model.n)
    Mo(z, case.x)
    return ref, cr.relerr(z, ref)


@pytest.mark.parametrize("erank", [1, 2])
def test_halpha_apply_with_ts_padded_and_compacted(dev, erank):
    case = _load_cg(dev)
    ref, err_o = _apply_reference(erank)
    bound = min(FACTOR * err_o, 1e-9)
    keys = ("prec_ts_factored", "prec_ts_stored_rows", "prec_ts_ragged")
    out = []
    with options(dev, cg_factored=1, prec_eig=1):
        for inv, dense in [(0, 1), (1, 1), (1, 2)]:
            with options(dev, prec_inv=inv, prec_dense=dense):
                assert dev.prec_setup(1, erank, 1) == 0      # ts on the padded columns, khat 64
                cp = _counts(dev, keys)
                zp = dev.prec_apply(case.x)
                with options(dev, ragged_ts=1):
                    assert dev.prec_setup(1, erank, 1) == 0
                    cc = _counts(dev, keys)
                    z = dev.prec_apply(case.x)
                    assert dev.prec_setup(1, erank, 1) == 0
                    assert np.array_equal(z, dev.prec_apply(case.x))
                assert cp["prec_ts_ragged"] == 0 and cc["prec_ts_ragged"] == 1
                assert cp["prec_ts_factored"] == cc["prec_ts_factored"] == 1
                assert cp["prec_ts_stored_rows"] == cc["prec_ts_stored_rows"]
                out.append((cr.relerr(zp, ref), cr.relerr(z, ref)))
    print("WIDE apply V3 erank=%d | oracle %.2e bound %.2e | (padded, compacted) potrs %.2e %.2e inverse %.2e %.2e dense %.2e %.2e"
          % (erank, err_o, bound, out[0][0], out[0][1], out[1][0], out[1][1], out[2][0], out[2][1]))
    for ep, e in out:
        assert ep <= bound and e <= bound, (out, bound)


@pytest.mark.parametrize("rest", [0, 1], ids=["padded", "compacted"])
@pytest.mark.parametrize("mh", [1, 2], ids=["matrixfree", "assembledH"])
def test_pcg_against_the_reference_run(dev, mh, rest):
    """(30, K) exactly at the tolerance in the gap, (-2, K - 1) at maxit = K - 1: the exits of the longdouble reference run."""
    case = _load_cg(dev)
    H = cr.dense_operator(case.model, case.W, case.X_lin, case.S_lin_inv)
    run = cr.reference_run(case, H, 1, 1)
    K, tol = run.K, run.tol
    with options(dev, cg_factored=1, prec_eig=1, matvec_h=mh, ragged_ops=rest, ragged_cross=rest, ragged_ts=rest):
        assert dev.prec_setup(1, 1, 1) == 0
        c0 = _counts(dev, ("schur_wide", "schur_ragged", "op_ragged"))
        got = [dev.pcg(case.h, tol, 10000), dev.pcg(case.h, tol, K - 1)]
        d = _delta(c0, _counts(dev, c0))
    print("WIDE pcg V3 mh=%d compacted=%d K=%d tol=%.3e | exits (%d, %d) (%d, %d) | %s"
          % (mh, rest, K, tol, got[0][1], got[0][2], got[1][1], got[1][2], d))
    assert (got[0][1], got[0][2]) == (30, K)
    assert (got[1][1], got[1][2]) == (-2, K - 1)
    if mh == 2:
        assert d["schur_wide"] == 1 and d["schur_ragged"] == 1 and d["op_ragged"] == 0
    else:
        assert d["schur_wide"] == 0 and (d["op_ragged"] > 0) == bool(rest)


# ---------------------------------------------------------------------------------------------- refusals
def _refused(dev, call, text):
    """The call fails with LRN_ERR_ARG (-1) and a text; no route counter moves."""
    import loraine_jl_amd
    keys = ROUTES + ("hybrid_cross_dense", "schur_diag")
    c0 = _counts(dev, keys)
    with pytest.raises(loraine_jl_amd.LoraineHipError) as ei:
        call()
    msg = str(ei.value)
    print("WIDE refusal |", msg)
    assert "(-1)" in msg and text in msg
    assert _counts(dev, keys) == c0


def test_refusals_leave_the_context_usable(dev):
    fm = _load(dev, "V1")
    V, d, khat = fm.lowrank[0]
    H = dev.schur_assemble(1, want_H=True)
    m, n = wc.SIZES["V1"]
    # khat 32 without the option: the text the library has always had
    _refused(dev, lambda: dev.upload_lowrank(0, khat, V, d), "khat = 32 (1, 2, 4, 8 or 16)")
    # no power of two up to 64, with the option on
    with options(dev, lowrank_wide=1):
        for bad in (48, 128):
            _refused(dev, lambda: dev.upload_lowrank(0, bad, sp.csr_matrix((n * bad, m)), np.zeros(n * bad)), "khat = %d" % bad)
    # a diagonal part on a wide block
    _refused(dev, lambda: dev.upload_diag(0, [1], np.ones((m, 1))), "wide")
    # the assembly of a wide block in a sharded run
    dev.set_shard(0, 2)
    try:
        _refused(dev, lambda: dev.schur_assemble(1), "one GPU")
    finally:
        dev.set_shard(0, 1)
    assert np.array_equal(dev.schur_assemble(1, want_H=True), H)      # every refusal left the block as it was


def test_wide_factors_on_a_block_with_diagonal_parts_are_refused(dev):
    """The reverse order: a narrow factored block with a diagonal row first, then a wide upload."""
    from loraine_jl_amd.model import build_factored_model
    m, n = wc.SIZES["V4b"]
    items = list(wc.items("V4b"))
    items[0] = (items[0][0], items[0][1], np.ones(m))
    fm = build_factored_model([-np.eye(m)], [items], np.zeros(n), factored_form=1)
    dev.upload_model(fm.AA, fm.sigmaA, fm.qA, fm.msizes)
    V, d, khat = fm.lowrank[0]
    dev.upload_lowrank(0, khat, V, d)
    dev.set_factored(0)
    dev.upload_diag(0, [0], np.ones((m, 1)))
    W, G = rc.spd(m, 3)
    dev.set_scaling(0, W, G)
    H = dev.schur_assemble(1, want_H=True)
    with options(dev, lowrank_wide=1):
        _refused(dev, lambda: dev.upload_lowrank(0, 32, sp.csr_matrix((n * 32, m)), np.zeros(n * 32)), "diagonal parts")
    assert dev.count("diag_rows") == 1
    assert np.array_equal(dev.schur_assemble(1, want_H=True), H)


# ---------------------------------------------------------------------------------------------- solves
def _solve(P, factors, **kw):
    from loraine_jl_amd.optimizer import Optimizer
    o = Optimizer()
    o.set_silent(True)
    attrs = kw.pop("attrs")
    for k, v in attrs.items():
        o.set_attribute(k, v)
    o.load_factored_model(P.F0(), factors, P.b, max_sense=True, factored_form=1, **kw)
    try:
        o.optimize()
        s = o.solver
        return dict(status=s.status, iters=s.iter, cg=getattr(s, "cg_iter_tot", 0), obj=o.objective_value(),
                    wide=s.dev.count("schur_wide"), ragged=s.dev.count("schur_ragged"), ts=s.dev.count("prec_ts_ragged"),
                    model_wide=s.model.wide)
    finally:
        if o.solver is not None:                             # (the device may serve another solve: the defaults again)
            for k in ("lowrank_wide", "ragged_cross", "ragged_ts", "ragged_ops", "lowrank_ragged", "cg_factored"):
                o.solver.dev.set_option(k, 0)


def test_planted_solve_kit_0():
    P = wc.PlantedWide()
    bound = 1e-6 * (1 + abs(P.optimum))
    a = _solve(P, P.factors(), attrs=dict(kit=0), wide=True, ragged=False)
    b = _solve(P, P.factors(), attrs=dict(kit=0), wide=True, ragged="all")
    s = _solve(P, P.stored_factors(), attrs=dict(kit=0))    # the three wide constraints as stored dense matrices
    print("WIDE solve kit 0 | wide: status %d, %d iterations, objective %.12e | wide + ragged=\"all\": status %d, %d iterations, "
          "objective %.12e | stored: status %d, %d iterations, objective %.12e | planted %.12e"
          % (a["status"], a["iters"], a["obj"], b["status"], b["iters"], b["obj"], s["status"], s["iters"], s["obj"], P.optimum))
    assert a["model_wide"] and b["model_wide"] and not s["model_wide"]
    assert a["wide"] > 0 and a["ragged"] == a["wide"] and b["wide"] > 0 and s["wide"] == 0
    assert a["status"] == b["status"] == 1
    assert a["iters"] == b["iters"]
    assert b["obj"] == pytest.approx(a["obj"], rel=1e-8)
    assert abs(a["obj"] - P.optimum) <= bound and abs(b["obj"] - P.optimum) <= bound
    assert s["status"] == 1 and abs(s["obj"] - P.optimum) <= bound


@pytest.mark.parametrize("ragged", [False, "all"])
def test_planted_solve_kit_1(ragged):
    P = wc.PlantedWide()
    r = _solve(P, P.factors(), attrs=dict(kit=1, preconditioner=1, erank=1), wide=True, ragged=ragged, cg=True)
    print("WIDE solve kit 1 ragged=%r | status %d, %d iterations, %d CG iterations, objective %.10f planted %.10f | assemblies of "
          "the wide block %d, ts blocks from the compacted columns %d" % (ragged, r["status"], r["iters"], r["cg"], r["obj"],
                                                                        P.optimum, r["wide"], r["ts"]))
    assert r["model_wide"]
    assert r["status"] == 1
    assert abs(r["obj"] - P.optimum) <= 1e-6 * (1 + abs(P.optimum))
    assert r["ts"] == (1 if ragged == "all" else 0)
