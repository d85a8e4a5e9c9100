"""Factored constraints with a diagonal part on the MI355X: A_k = diag(a_k) + V_k D_k V_k' (items (V, d, a) of
build_factored_model, lrn_upload_diag).  The data operators and the mode-1 Schur matrix (csrc/diagops.hip: H_DD, the cross terms
with the factors and with the stored rows of the same block) against NumPy from the dense A_k, against mode 0 of the materialised
model and against the same model with every diagonal part given as a stored sparse matrix (the hybrid route); both forms of the
squared-operand product, G given or W only, bit-reproducibility, exact symmetry, counters; two blocks with C_lin rows; error
paths; the unchanged default; solves.

All comparisons are relative Frobenius < 1e-12, the bound tests/test_gpu_hybrid_factored.py uses for the same quantities;
rel = 1e-8 between two solves."""
import numpy as np
import pytest
import scipy.sparse as sp

import diag_factored_cases as dc
from oracle import loraine_oracle as lo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import loraine_jl_amd
    d = loraine_jl_amd.Device(0)
    yield d
    d.close()


def relerr(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _models(blocks, n, C_lin=None, factored=None):
    """(factored model, the same data fully materialised); factored: which blocks stay factored (default all)."""
    from loraine_jl_amd.model import build_factored_model, build_model
    F0 = [-np.eye(dc.dense_of(b[0]).shape[0]) for b in blocks]
    d_lin = None if C_lin is None else np.ones(C_lin.shape[1])
    fm = build_factored_model(F0, blocks, np.zeros(n), 0.0, d_lin, C_lin, factored_form=1)
    A = [[sp.csc_matrix(F)] + [sp.csc_matrix(dc.dense_of(it)) for it in b] for F, b in zip(F0, blocks)]
    mm = build_model(A, np.zeros(n), 0.0, d_lin, C_lin)
    if factored is not None:
        for i, f in enumerate(factored):
            if not f:
                fm.AA[i], fm.sigmaA[:, i], fm.qA[:, i], fm.nzA[:, i] = mm.AA[i], mm.sigmaA[:, i], mm.qA[:, i], mm.nzA[:, i]
                fm.factored_blocks[i] = False
    return fm, mm


def _upload(dev, model, dense_threshold=None):
    """What ResidentSolver does with a model: entries, factors, the declaration, the diagonal parts."""
    if dense_threshold is not None:
        dev.set_option("dense_threshold", dense_threshold)
    try:
        dev.upload_model(model.AA, model.sigmaA, model.qA, model.msizes, C_lin=model.C_lin if model.nlin else None)
    finally:
        dev.set_option("dense_threshold", -1.0)
    if getattr(model, "from_factors", False):
        for i, (V, d, khat) in enumerate(model.lowrank):
            dev.upload_lowrank(i, khat, V, d)
            if model.factored_blocks[i]:
                dev.set_factored(i)
                if model.diag[i]:
                    rows = sorted(model.diag[i])
                    dev.upload_diag(i, rows, np.column_stack([model.diag[i][k] for k in rows]))


def _operators(dev, model, Xs, y, dense_threshold=None):
    """AA vec(X) and Rd = C - S - mat(AA'y) with C = S = 0 through the resident entry points."""
    _upload(dev, model, dense_threshold)
    for i, X in enumerate(Xs):
        dev.ip_set_c(i, np.zeros_like(X))
        dev.ip_set_iterate(i, X, np.zeros_like(X))
    dev.reset_timing()
    aax = dev.ip_aa_x()
    dev.ip_residual_d(y)
    Rd = [dev.dbg_get_block(i, "Rd")[0] for i in range(len(Xs))]
    counts = {k: dev.count(k) for k in ("op_factored", "op_dense", "op_sparse", "op_diag", "diag_rows")}
    return aax, Rd, counts


@pytest.mark.parametrize("m,n,khat,count", dc.CASES)
def test_operators_and_schur_matrix_with_diagonal_parts(dev, m, n, khat, count):
    items = dc.block_items(m, n, khat, count, 100 * m + n)
    stored = {k: it for k, it in enumerate(items) if sp.issparse(it)}
    assert sum(1 for it in items if isinstance(it, tuple) and len(it) == 3) == count
    assert bool(stored) == (count < n) and (not stored or sorted(a.nnz for a in stored.values()) == [9, m, m * m])
    fm, mm = _models([items], n)
    assert fm.factored and sorted(fm.diag[0]) == dc.diag_rows(n, count) and sorted(fm.stored[0]) == sorted(stored)
    thr = float(m * m)                                    # the dense stored matrix goes to a dense slot
    As = [dc.dense_of(it) for it in items]
    X = dc.sym(m, m + n)
    y = np.random.default_rng(n).standard_normal(n)
    # ---- data operators
    aax, Rd, cnt = _operators(dev, fm, [X], y, thr)
    assert cnt["diag_rows"] == count and cnt["op_diag"] == 2 and cnt["op_factored"] == 2
    assert cnt["op_dense"] == cnt["op_sparse"] == (2 if stored else 0)
    aax2, Rd2, _ = _operators(dev, fm, [X], y, thr)
    assert np.array_equal(aax, aax2) and np.array_equal(Rd[0], Rd2[0])          # fixed summation order: identical bits
    assert np.array_equal(Rd[0], Rd[0].T)
    aax_np, Rd_np = -np.array([np.sum(a * X) for a in As]), sum(yk * a for yk, a in zip(y, As))
    print(f"aa_times vs NumPy {relerr(aax, aax_np):.2e}, aat_to_mat vs NumPy {relerr(Rd[0], Rd_np):.2e}")
    assert relerr(aax, aax_np) < 1e-12
    assert relerr(Rd[0], Rd_np) < 1e-12
    aax_m, Rd_m, cnt_m = _operators(dev, mm, [X], y)
    assert cnt_m["op_factored"] == 0 and cnt_m["op_diag"] == 0 and cnt_m["diag_rows"] == 0
    assert relerr(aax, aax_m) < 1e-12 and relerr(Rd[0], Rd_m[0]) < 1e-12
    sm, _ = _models([dc.diag_as_stored(items)], n)          # every diagonal part as a stored sparse matrix: the hybrid route
    assert sm.factored and sm.diag == [{}] and len(sm.stored[0]) == len(stored) + count
    aax_s, Rd_s, cnt_s = _operators(dev, sm, [X], y, thr)
    assert cnt_s["op_diag"] == 0 and cnt_s["diag_rows"] == 0
    assert relerr(aax, aax_s) < 1e-12 and relerr(Rd[0], Rd_s[0]) < 1e-12
    # ---- mode 1, both forms of the squared-operand product, G given and W only
    W, G = dc.spd(m, 6 + m)
    Hnp = dc.h_definition(As, W)
    _upload(dev, mm)
    dev.set_scaling(0, W, G)
    H0 = dev.schur_assemble(0, want_H=True)
    _upload(dev, sm, thr)
    dev.set_scaling(0, W, G)
    Hs = dev.schur_assemble(1, want_H=True)
    assert dev.count("diag_rows") == 0
    _upload(dev, fm, thr)
    H = {}
    try:
        for form in (0, 1):
            dev.set_option("diag_sq_mfma", form)
            for with_g in (True, False):
                dev.set_scaling(0, W, G if with_g else None)
                dev.reset_timing()
                Hf = dev.schur_assemble(1, want_H=True)
                assert dev.count("schur_diag") == 1 and dev.count("diag_stored_cross") == (1 if stored else 0)
                assert dev.count("diag_sq_mfma" if form else "diag_sq_rows") == 2
                assert dev.count("diag_sq_rows" if form else "diag_sq_mfma") == 0
                assert dev.count("lowrank") == 1
                assert np.array_equal(Hf, dev.schur_assemble(1, want_H=True))     # two assemblies: the same bits
                assert np.array_equal(Hf, Hf.T)
                errs = [relerr(Hf, ref) for ref in (Hnp, H0, Hs)]
                print(f"form {form} G {with_g}: H vs NumPy {errs[0]:.2e}, vs mode 0 {errs[1]:.2e}, vs stored route {errs[2]:.2e}")
                assert max(errs) < 1e-12
                H[form, with_g] = Hf
        dev.set_option("diag_sq_mfma", -1)                 # auto: the threshold between the forms is 16 rows
        dev.reset_timing()
        Ha = dev.schur_assemble(1, want_H=True)
        assert dev.count("diag_sq_mfma" if count >= 16 else "diag_sq_rows") == 2
        assert np.array_equal(Ha, H[1 if count >= 16 else 0, False])
    finally:
        dev.set_option("diag_sq_mfma", -1)
    assert relerr(H[0, True], H[1, True]) < 1e-12


@pytest.mark.parametrize("count", [15, 16])
def test_auto_rule_switches_forms_at_16_rows(dev, count):
    """Option diag_sq_mfma = -1 on both sides of the threshold: the form taken, and H of the definition either way."""
    m, n, khat = 33, 37, 2
    items = dc.block_items(m, n, khat, count, 77)
    fm, _ = _models([items], n)
    assert len(fm.diag[0]) == count and len(fm.stored[0]) == 3
    W, G = dc.spd(m, 9)
    _upload(dev, fm, float(m * m))
    dev.set_scaling(0, W, G)
    dev.reset_timing()
    H = dev.schur_assemble(1, want_H=True)
    assert dev.count("diag_sq_mfma") == (2 if count >= 16 else 0) and dev.count("diag_sq_rows") == (0 if count >= 16 else 2)
    assert relerr(H, dc.h_definition([dc.dense_of(it) for it in items], W)) < 1e-12


def _rhs_sequence(dev, model, Xs, Ss, Cs, y, dely, ab=None):
    """One predictor / corrector round of right-hand sides with every input given (no solve in between)."""
    _upload(dev, model)
    nl = len(Xs)
    for i in range(nl):
        dev.ip_set_c(i, Cs[i])
        dev.ip_set_iterate(i, Xs[i], Ss[i])
        assert dev.ip_prepare_w(i) == 0
    if model.nlin:
        dev.set_lin(np.ones(model.nlin), np.ones(model.nlin))
    dev.reset_timing()
    dev.ip_residual_d(y)
    aax, rhs = dev.ip_rhs_pred2()
    a, b = dev.ip_find_step(True, 0.0, 0.95, dely)
    if ab is None:
        ab = (a.copy(), b.copy())
    dev.ip_update(True, ab[0], ab[1])
    corr = dev.ip_rhs_corr(0.3)
    H = dev.schur_assemble(1 if getattr(model, "from_factors", False) else 0, want_H=True)
    return dict(aax=aax, rhs=rhs, a=a, b=b, corr=corr, H=H, diag=dev.count("op_diag"), schur=dev.count("schur_diag")), ab


def _iterate(ms, seed):
    rng = np.random.default_rng(seed)
    Xs, Ss, Cs = [], [], []
    for m in ms:
        Q = rng.standard_normal((m, m)) / np.sqrt(m)
        Xs.append(np.eye(m) + 0.3 * Q @ Q.T)
        Q = rng.standard_normal((m, m)) / np.sqrt(m)
        Ss.append(np.eye(m) + 0.3 * Q @ Q.T)
        Cs.append(dc.sym(m, seed + m) / np.sqrt(m))
    return Xs, Ss, Cs


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_two_blocks_with_linear_rows(dev, order):
    """A block with diagonal rows (and stored rows) beside an un-factored dense block, C_lin present, either order: H lives in
    natural index space; H and the right-hand-side sequence against the materialised model."""
    n = 37
    with_diag = dc.block_items(33, n, 2, 3, 5)
    plain = [dc._dense_sym(20, 40 + k) for k in range(n)]
    blocks = [(with_diag, plain)[k] for k in order]
    ms = tuple((33, 20)[k] for k in order)
    C_lin = sp.random(n, 6, density=0.3, random_state=3, format="csr")
    fm, mm = _models(blocks, n, C_lin=C_lin, factored=[k == 0 for k in order])
    assert [bool(d) for d in fm.diag] == [k == 0 for k in order]
    Xp, Sp, Cp = _iterate(ms, 11)
    y = np.random.default_rng(8).standard_normal(n) * 0.1
    dely = np.random.default_rng(9).standard_normal(n) * 0.1
    ref, ab = _rhs_sequence(dev, mm, Xp, Sp, Cp, y, dely)
    got, _ = _rhs_sequence(dev, fm, Xp, Sp, Cp, y, dely, ab)
    assert got["diag"] > 0 and got["schur"] == 1 and ref["diag"] == 0 and ref["schur"] == 0
    for key in ("aax", "rhs", "corr", "H"):
        print(key, relerr(got[key], ref[key]))
        assert relerr(got[key], ref[key]) < 1e-12, key
    for i in range(2):
        assert got["a"][i] == pytest.approx(ref["a"][i], rel=1e-8) and got["b"][i] == pytest.approx(ref["b"][i], rel=1e-8)


def test_errors_are_returned(dev):
    from loraine_jl_amd._capi import LoraineHipError
    m, n, khat = 20, 12, 2
    items = list(dc._factors(m, n, khat, 13))
    items[0] = sp.identity(m, format="csc")
    items[5] = (items[5][0], items[5][1], dc._diagonal(m, 1))
    items[6] = (None, [], np.ones(m))
    fm, mm = _models([items], n)
    a2 = np.column_stack([fm.diag[0][5], fm.diag[0][6]])
    # the block must be factored
    _upload(dev, mm)
    with pytest.raises(LoraineHipError, match="not factored"):
        dev.upload_diag(0, [5, 6], a2)
    dev.upload_model(fm.AA, fm.sigmaA, fm.qA, fm.msizes)
    dev.upload_lowrank(0, fm.lowrank[0][2], fm.lowrank[0][0], fm.lowrank[0][1])
    with pytest.raises(LoraineHipError, match="not factored"):
        dev.upload_diag(0, [5, 6], a2)
    dev.set_factored(0)
    # argument errors
    with pytest.raises(LoraineHipError, match="out of range"):
        dev.upload_diag(0, [5, n], a2)
    with pytest.raises(LoraineHipError, match="out of range"):
        dev.upload_diag(0, [-1, 6], a2)
    with pytest.raises(LoraineHipError, match="listed twice"):
        dev.upload_diag(0, [5, 5], a2)
    with pytest.raises(LoraineHipError, match="block 3"):
        dev.upload_diag(3, [5, 6], a2)
    with pytest.raises(LoraineHipError, match="is stored"):
        dev.upload_diag(0, [0, 6], a2)
    assert dev.count("diag_rows") == 0                          # (a refused upload leaves nothing behind)
    dev.upload_diag(0, [5, 6], a2)
    assert dev.count("diag_rows") == 2
    # refusals of the CG entry points, with and without cg_factored; modes 0 and -1
    W, G = dc.spd(m, 6)
    dev.set_scaling(0, W, G)
    try:
        for cgf in (0, 1):
            dev.set_option("cg_factored", cgf)
            with pytest.raises(LoraineHipError, match="lrn_matvec: .*diagonal parts"):
                dev.matvec(np.ones(n))
            with pytest.raises(LoraineHipError, match="lrn_prec_setup: .*diagonal parts"):
                dev.prec_setup(1, 1, 1)
            with pytest.raises(LoraineHipError, match="lrn_prec_apply: .*diagonal parts"):
                dev.prec_apply(np.ones(n))
            with pytest.raises(LoraineHipError, match="lrn_pcg: .*diagonal parts"):
                dev.pcg(np.ones(n), 1e-6)
            x = np.ones(n)
            out = np.zeros(n)
            from loraine_jl_amd._capi import ptr
            assert dev.lib.lrn_matvec_partial(dev.h, ptr(x), ptr(out)) != 0
            msg = dev.lib.lrn_last_error(dev.h).decode()
            assert "lrn_matvec_partial" in msg and "diagonal parts" in msg
    finally:
        dev.set_option("cg_factored", 0)
    with pytest.raises(LoraineHipError, match="factored"):
        dev.schur_assemble(0)
    with pytest.raises(LoraineHipError, match="factored"):
        dev.schur_assemble(-1)
    As = [dc.dense_of(it) for it in items]
    H1 = dev.schur_assemble(1, want_H=True)
    assert relerr(H1, dc.h_definition(As, W)) < 1e-12
    # a refused upload leaves the parts that are there
    with pytest.raises(LoraineHipError, match="listed twice"):
        dev.upload_diag(0, [6, 6], a2)
    assert dev.count("diag_rows") == 2 and np.array_equal(dev.schur_assemble(1, want_H=True), H1)
    # world > 1: mode 1 of such a block is not sharded
    dev.set_shard(0, 2)
    try:
        with pytest.raises(LoraineHipError, match="one GPU"):
            dev.schur_assemble(1)
    finally:
        dev.set_shard(0, 1)
    # new factors keep the parts; nrows = 0 clears them: the block assembles as the hybrid block without them
    dev.upload_lowrank(0, fm.lowrank[0][2], fm.lowrank[0][0], fm.lowrank[0][1])
    assert dev.count("diag_rows") == 2
    assert np.array_equal(dev.schur_assemble(1, want_H=True), H1)
    dev.upload_diag(0, [], None)
    assert dev.count("diag_rows") == 0
    dev.reset_timing()
    Hp = dev.schur_assemble(1, want_H=True)
    assert dev.count("schur_diag") == 0 and dev.count("diag_sq_rows") == dev.count("diag_sq_mfma") == 0
    bare = list(items)
    bare[5] = items[5][:2]
    bare[6] = (np.zeros((m, 0)), np.zeros(0))
    bm, _ = _models([bare], n)
    _upload(dev, bm)
    dev.set_scaling(0, W, G)
    assert np.array_equal(Hp, dev.schur_assemble(1, want_H=True))
    assert relerr(Hp, dc.h_definition([dc.dense_of(it) for it in bare], W)) < 1e-12
    # lrn_set_factored(0) and a new model drop the parts
    _upload(dev, fm)
    assert dev.count("diag_rows") == 2
    dev.set_factored(0, False)
    assert dev.count("diag_rows") == 0
    _upload(dev, fm)
    assert dev.count("diag_rows") == 2
    _upload(dev, mm)
    assert dev.count("diag_rows") == 0


def test_models_without_diagonal_parts_take_the_routes_they_took(dev):
    """A pure and a hybrid block without diagonal parts: no counter of this feature moves, the route counters are those
    tests/test_gpu_hybrid_factored.py expects, and H is the matrix of the definition."""
    m, n, khat = 33, 37, 2
    W, G = dc.spd(m, 6 + m)
    X = dc.sym(m, 3)
    y = np.random.default_rng(n).standard_normal(n)
    pure = dc._factors(m, n, khat, 21)
    hyb = list(pure)
    hyb[0], hyb[n // 2] = dc._identity(m, 0), dc._nine(m, 1)
    for items, ns in ((pure, 0), (hyb, 2)):
        fm, _ = _models([items], n)
        assert fm.diag == [{}]
        _, _, cnt = _operators(dev, fm, [X], y)
        assert cnt["op_factored"] == 2 and cnt["op_diag"] == 0 and cnt["diag_rows"] == 0
        assert cnt["op_dense"] == 0 and cnt["op_sparse"] == (2 if ns else 0)
        dev.set_scaling(0, W, G)
        dev.reset_timing()
        H = dev.schur_assemble(1, want_H=True)
        assert dev.count("schur_diag") == 0 and dev.count("diag_sq_rows") == dev.count("diag_sq_mfma") == 0
        assert dev.count("diag_stored_cross") == 0 and dev.count("lowrank") == 1
        assert dev.count("hybrid_cross_lds") == (1 if ns else 0) and dev.count("hybrid_cross_global") == 0
        assert relerr(H, dc.h_definition([dc.dense_of(it) for it in items], W)) < 1e-12


# ---------------------------------------------------------------------------------------------- solves
def _opt(**attrs):
    from loraine_jl_amd.optimizer import Optimizer
    o = Optimizer()
    o.set_silent(True)
    o.set_attribute("kit", 0)
    for k, v in attrs.items():
        o.set_attribute(k, v)
    return o


def test_trace_row_as_a_diagonal_part_and_as_a_stored_identity():
    """Planted msz 60 / nvar 80 / rank 2 (synthetic.FactoredLowRankProblem, optimum b'y*) with constraint 0 the trace row: given
    as the diagonal part (None, [], ones) and as a stored identity.  Status 1 both times, objectives within 1e-8 of the planted
    value and of each other, iteration counts within +-1 (rounding: DESIGN section 11 records such a shift)."""
    from loraine_jl_amd.synthetic import FactoredLowRankProblem
    m, n = 60, 80
    P = FactoredLowRankProblem(m, n, 2, 4, seed=2, stored=[(0, sp.identity(m, format="csc"))])
    as_stored = P.factors()
    as_diag = [[(None, [], np.ones(m))] + as_stored[0][1:]]
    od = _opt()
    od.load_factored_model(P.F0(), as_diag, P.b, max_sense=True, factored_form=1)
    od.optimize()
    s = od.solver
    assert s.model.factored and sorted(s.model.diag[0]) == [0] and s.model.stored == [{}]
    assert s.dev.count("diag_rows") == 1 and s.dev.count("op_diag") > 0 and s.dev.count("schur_diag") > 0
    assert s.dev.count("diag_sq_rows") > 0 and s.dev.count("op_sparse") == 0 and s.dev.count("op_dense") == 0
    os_ = _opt()
    os_.load_factored_model(P.F0(), as_stored, P.b, max_sense=True, factored_form=1)
    os_.optimize()
    t = os_.solver
    assert sorted(t.model.stored[0]) == [0] and t.dev.count("diag_rows") == 0 and t.dev.count("op_sparse") > 0
    print("iterations", s.iter, t.iter, "objectives", od.objective_value(), os_.objective_value(), "planted", P.optimum,
          "differences", od.objective_value() - P.optimum, os_.objective_value() - P.optimum,
          od.objective_value() - os_.objective_value())
    assert s.status == 1 and t.status == 1
    assert od.termination_status() == os_.termination_status() == "OPTIMAL"
    assert abs(s.iter - t.iter) <= 1
    assert abs(od.objective_value() - P.optimum) <= 1e-8
    assert abs(os_.objective_value() - P.optimum) <= 1e-8
    assert abs(od.objective_value() - os_.objective_value()) <= 1e-8


def test_every_constraint_a_sum_against_the_oracle():
    """A model in which every constraint is diag(a) + V D V': against the oracle on the materialised data."""
    m, n, seed = 40, 50, 7
    rng = np.random.default_rng(seed)
    items = [(rng.standard_normal((m, 2)) / np.sqrt(m), rng.choice([-1.0, 1.0], size=2), dc._diagonal(m, 50 + k) / 2.0)
             for k in range(n)]
    Q = rng.standard_normal((m, m))
    X0 = np.eye(m) + Q @ Q.T / m
    y0 = rng.standard_normal(n) / np.sqrt(n)
    As = [dc.dense_of(it) for it in items]
    b = -np.array([np.sum(a * X0) for a in As])
    F0 = -(np.eye(m) - sum(y * a for y, a in zip(y0, As)))
    ref = lo.MySolver(lo.make_model([[F0.copy()] + [a.copy() for a in As]], b.copy(), 0.0, None, None), dict(kit=0, verb=0))
    lo.solve(ref)
    om = _opt()
    om.load_model([[sp.csc_matrix(F0)] + [sp.csc_matrix(a) for a in As]], b)
    om.optimize()
    of = _opt()
    of.load_factored_model([F0], [items], b)              # factored_form = -1: dense parts, the block stays factored
    of.optimize()
    s = of.solver
    assert s.model.factored and sorted(s.model.diag[0]) == list(range(n)) and s.datarank == 2
    assert s.dev.count("diag_rows") == n and s.dev.count("diag_sq_mfma") > 0 and s.dev.count("diag_sq_rows") == 0
    assert ref.status == 1 and of.termination_status() == om.termination_status() == "OPTIMAL"
    print("iterations", s.iter, om.solver.iter, ref.iter)
    assert of.objective_value() == pytest.approx(lo.objective_value(ref), rel=1e-8)
    assert of.objective_value() == pytest.approx(om.objective_value(), rel=1e-8)
