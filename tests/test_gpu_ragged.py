"""GPU: the rank-class route of the rank-k Schur assembly (library option lowrank_ragged; csrc/raggedops.hip, csrc/ragged_plan.h)
through Device / the C ABI: H of mode 1 against H_ij = tr(A_i W A_j W) from the materialised constraints (tests/ragged_cases.py)
for the cases R1 .. R6 with G and with W only, the counters against the Python planner, reproducibility and symmetry, the
fallbacks (uniform block, sharded run), option 0 after option 1, a materialised model with covering factors, kit = 1 through
the assembled H, and solves through Optimizer.load_factored_model(ragged=True).

The bound is the suite's own for a product against another formulation (tests/test_gpu_lowrank.py, test_gpu_factored.py):
1e-12 relative Frobenius; the padded route (option 0) is measured against the same reference in the same test and both
figures are printed.  The operator bound is that of tests/test_gpu_cg_factored.py: 20 x the oracle's distance from the
longdouble reference.  Solves: rel 1e-8 between two solves of one problem, 1e-6 against the planted optimum."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp

import ragged_cases as rc
from loraine_jl_amd.model import ragged_plan
from oracle import loraine_oracle as lo

pytestmark = pytest.mark.gpu

TOL = 1e-12
DEFAULTS = dict(lowrank_ragged=0, cg_factored=0, cg_diag=0, matvec_h=0)
STATE = ("ragged_cols", "ragged_classes", "ragged_tiles")


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


def _upload(dev, fm, factored=True):
    dev.upload_model(fm.AA, fm.sigmaA, fm.qA, fm.msizes, C_lin=fm.C_lin if fm.nlin else None)
    for i, (V, d, khat) in enumerate(fm.lowrank):
        dev.upload_lowrank(i, khat, V, d)
        if factored:
            dev.set_factored(i)
            dg = fm.diag[i] if getattr(fm, "diag", None) else {}
            if dg:
                rows = sorted(dg)
                dev.upload_diag(i, rows, np.column_stack([dg[k] for k in rows]))


def _scale(dev, name, fm, with_G):
    for i, (W, G) in enumerate(rc.scaling(name)):
        dev.set_scaling(i, W, G if with_G else None)
    if fm.nlin:
        dev.set_lin(np.ones(fm.nlin), np.ones(fm.nlin))


def _load(dev, name, with_G):
    fm = rc.model(name)
    _upload(dev, fm)
    _scale(dev, name, fm, with_G)
    return fm


@pytest.mark.parametrize("with_G", [True, False], ids=["G", "W-only"])
@pytest.mark.parametrize("name", rc.NAMES)
def test_mode_1_by_rank_class(dev, name, with_G):
    fm = _load(dev, name, with_G)
    ref = rc.reference(name)
    plans = [ragged_plan(rc.block_ranks(fm, i)) for i in range(fm.nlmi)]
    H0 = dev.schur_assemble(1, want_H=True)                  # the padded route, against the same reference
    c0 = {k: dev.count(k) for k in ("schur_ragged", "ragged_fallback")}
    with options(dev, lowrank_ragged=1):
        H1 = dev.schur_assemble(1, want_H=True)
        state = {k: dev.count(k) for k in STATE}
        H2 = dev.schur_assemble(1, want_H=True)
        c1 = {k: dev.count(k) for k in c0}
    H0b = dev.schur_assemble(1, want_H=True)
    e0, e1 = rc.relerr(H0, ref), rc.relerr(H1, ref)
    print("RAGGED %s %s | padded %.2e ragged %.2e | Rc %d of %d, classes %d, tiles %d"
          % (name, "G" if with_G else "W-only", e0, e1, state["ragged_cols"], fm.n * fm.lowrank[-1][2], state["ragged_classes"],
             state["ragged_tiles"]))
    assert e1 < TOL
    assert e0 < TOL
    assert c1["schur_ragged"] - c0["schur_ragged"] == 2 * fm.nlmi and c1["ragged_fallback"] == c0["ragged_fallback"]
    last = plans[-1]                                         # the state counters are those of the last block assembled
    assert state == dict(ragged_cols=last["Rc"], ragged_classes=last["ncls"], ragged_tiles=last["tiles"])
    assert np.array_equal(H1, H2)                            # one writer per entry, fixed order: the same bits
    assert np.array_equal(H1, H1.T)
    assert np.array_equal(H0, H0b)                           # option 0 after option 1: the padded route's bits
    if name == "R1":
        assert np.all(H1[2, :] == 0.0) and np.all(H1[:, 2] == 0.0)      # the rank-0 row


def test_a_uniform_block_keeps_the_padded_route(dev):
    from loraine_jl_amd.model import build_factored_model
    m, n = rc.SIZES["R3"]
    rng = np.random.default_rng(31)
    facs = [(rng.standard_normal((m, 1)) / np.sqrt(m), rng.choice([-1.0, 1.0], size=1)) for _ in range(n)]
    fm = build_factored_model([-np.eye(m)], [facs], np.zeros(n), factored_form=1)
    _upload(dev, fm)
    W, G = rc.spd(m, 5)
    dev.set_scaling(0, W, G)
    H0 = dev.schur_assemble(1, want_H=True)
    c0 = {k: dev.count(k) for k in ("schur_ragged", "ragged_fallback")}
    with options(dev, lowrank_ragged=1):
        H1 = dev.schur_assemble(1, want_H=True)
        assert dev.count("ragged_fallback") - c0["ragged_fallback"] == 1
        assert dev.count("schur_ragged") == c0["schur_ragged"]
    assert np.array_equal(H1, H0)


@pytest.mark.parametrize("name", ["R2", "R6"])
def test_option_0_after_option_1_is_a_fresh_context(dev, name):
    import loraine_jl_amd
    _load(dev, name, False)
    with options(dev, lowrank_ragged=1):
        dev.schur_assemble(1)
        assert dev.count("schur_ragged") > 0
    H = dev.schur_assemble(1, want_H=True)
    fresh = loraine_jl_amd.Device(0)
    try:
        _load(fresh, name, False)
        Hf = fresh.schur_assemble(1, want_H=True)
        assert fresh.count("schur_ragged") == 0 and fresh.count("ragged_fallback") == 0
    finally:
        fresh.close()
    assert np.array_equal(H, Hf)


def test_materialised_model_with_covering_factors(dev):
    from loraine_jl_amd.model import build_model
    m, n = rc.SIZES["R2"]
    facs = rc.factors("R2")
    A = [[sp.csc_matrix(-np.eye(m))] + [sp.csc_matrix(rc.materialise(f, m)) for f in facs]]
    mm = build_model(A, np.zeros(n), factors=[list(facs)])
    _upload(dev, mm, factored=False)
    W, G = rc.scaling("R2")[0]
    dev.set_scaling(0, W, G)
    ref = rc.reference("R2")
    Hm0 = dev.schur_assemble(0, want_H=True)
    with options(dev, lowrank_ragged=1):
        c0 = dev.count("schur_ragged")
        H1 = dev.schur_assemble(1, want_H=True)
        assert dev.count("schur_ragged") - c0 == 1
    print("RAGGED covered R2 | mode 1 ragged %.2e, against mode 0 %.2e" % (rc.relerr(H1, ref), rc.relerr(H1, Hm0)))
    assert rc.relerr(H1, ref) < TOL
    assert rc.relerr(H1, Hm0) < TOL


def test_kit_1_operator_through_the_assembled_matrix(dev):
    """R2 as a factored model, cg_factored = 1, the operator forced through H (matvec_h = 2): H comes from the rank-class route."""
    from loraine_jl_amd.model import build_model
    m, n = rc.SIZES["R2"]
    facs = rc.factors("R2")
    Href = rc.reference("R2", rc.LD)
    x = np.random.default_rng(77).standard_normal(n)
    ref = Href @ x.astype(rc.LD)
    W, G = rc.scaling("R2")[0]
    # what float64 costs: the oracle's operator on the materialised model
    A = [[sp.csc_matrix(-np.eye(m))] + [sp.csc_matrix(rc.materialise(f, m)) for f in facs]]
    mm = build_model(A, np.zeros(n))
    yo = np.zeros(n)
    lo.MyA([W], mm.AA, 0, mm.C_lin, np.zeros(0), np.zeros(0))(yo, x)
    err_o = rc.relerr(yo, ref)
    _load(dev, "R2", True)
    with options(dev, cg_factored=1, matvec_h=2, lowrank_ragged=1):
        c0 = {k: dev.count(k) for k in ("schur_ragged", "hop_assemble_lowrank", "hop_matvec")}
        y1 = dev.matvec(x)
        y2 = dev.matvec(x)
        d = {k: dev.count(k) - c0[k] for k in c0}
    err = rc.relerr(y1, ref)
    print("RAGGED operator R2 | oracle %.2e bound %.2e | device %.2e" % (err_o, 20.0 * err_o, err))
    assert d == dict(schur_ragged=1, hop_assemble_lowrank=1, hop_matvec=2)
    assert err <= 20.0 * err_o, (err, err_o)
    assert np.array_equal(y1, y2)


def test_sharded_run_keeps_the_padded_route(dev):
    """lrn_set_shard(0, 2) without a second GPU: the padded, sharded route assembles this rank's column blocks."""
    _load(dev, "R3", True)
    ref = rc.reference("R3")
    dev.set_shard(0, 2)
    try:
        bs = dev.shard_bs()
        H0 = dev.schur_assemble(1, want_H=True)
        with options(dev, lowrank_ragged=1):
            c0 = {k: dev.count(k) for k in ("schur_ragged", "ragged_fallback")}
            H1 = dev.schur_assemble(1, want_H=True)
            assert dev.count("ragged_fallback") - c0["ragged_fallback"] == 1 and dev.count("schur_ragged") == c0["schur_ragged"]
    finally:
        dev.set_shard(0, 1)
    assert np.array_equal(H1, H0)
    own = np.tril(H1)[:, :bs]                                  # rank 0 owns the first column block
    assert rc.relerr(own, np.tril(ref)[:, :bs]) < TOL


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
    for ragged in (False, True):
        o = _opt(kit=0)
        o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True, factored_form=1, ragged=ragged)
        o.optimize()
        runs[ragged] = o
        assert o.solver.model.ragged is ragged
        assert (o.solver.dev.count("schur_ragged") > 0) == ragged
    a, b = runs[False], runs[True]
    print("RAGGED solve kit 0 | padded: status %d, %d iterations, objective %.12e | ragged: status %d, %d iterations, objective "
          "%.12e | planted %.12e" % (a.solver.status, a.solver.iter, a.objective_value(), b.solver.status, b.solver.iter,
                                     b.objective_value(), P.optimum))
    assert b.solver.status == a.solver.status == 1
    assert b.solver.iter == a.solver.iter
    assert b.objective_value() == pytest.approx(a.objective_value(), rel=1e-8)


def test_planted_solve_kit_1():
    P = rc.Planted()
    o = _opt(kit=1, preconditioner=1, erank=1)
    o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True, factored_form=1, cg=True, ragged=True)
    o.optimize()
    s = o.solver
    print("RAGGED solve kit 1 | status %d, %d iterations, %d CG iterations, objective %.10f planted %.10f | H by rank class %d"
          % (s.status, s.iter, s.cg_iter_tot, o.objective_value(), P.optimum, s.dev.count("schur_ragged")))
    assert s.model.ragged and s.model.factored_cg and s.kit == 1
    assert s.status == 1
    assert abs(o.objective_value() - P.optimum) <= 1e-6 * (1 + abs(P.optimum))
