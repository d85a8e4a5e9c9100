"""Hybrid factored blocks on the MI355X: most constraints of a block are factors, a few are stored matrices (identity, a
handful of entries, tridiagonal, dense).  The data operators and the mode-1 Schur matrix (H_FF + H_SS + the cross terms of
schur_factored.hip::fac_cross_kernel) against the same data fully materialised (mode 0) and against NumPy from the definition;
bit-reproducibility, exact symmetry, both forms of the cross kernel, G given or W only; two blocks with C_lin rows; error
paths; planted solves through Optimizer.load_factored_model against load_model and the oracle.

Tolerances are those of tests/test_gpu_factored.py for the same comparisons: 1e-12 relative Frobenius against another
formulation, rel=1e-8 between two solves, rel=1e-6 against a planted optimum."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import loraine_oracle as lo

pytestmark = pytest.mark.gpu

SHAPES = [(16, 5, 1), (33, 37, 2), (70, 45, 4), (130, 130, 16), (257, 60, 8), (333, 300, 2)]


@pytest.fixture(scope="module")
def dev():
    import loraine_jl_amd
    d = loraine_jl_amd.Device(0)
    yield d
    d.close()


def relerr(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _factors(m, n, khat, seed):
    """Random signed dense factors of rank 0 .. khat (mixed)."""
    rng = np.random.default_rng(seed)
    facs = []
    for k in range(n):
        r = int(rng.integers(0, khat + 1)) if k % 4 else khat
        facs.append((rng.standard_normal((m, r)) / np.sqrt(m), rng.choice([-1.0, 1.0], size=r)))
    return facs


def _identity(m, seed):
    return sp.identity(m, format="csc")


def _few(m, seed):
    """At most 4 entries: one symmetric off-diagonal pair and one diagonal entry (the thread tier)."""
    rng = np.random.default_rng(seed)
    i, j = rng.choice(m, size=2, replace=False)
    A = sp.lil_matrix((m, m))
    A[i, j] = A[j, i] = 0.7
    A[i, i] = -1.3
    return A.tocsc()


def _tridiag(m, seed):
    rng = np.random.default_rng(seed)
    off = rng.standard_normal(m - 1)
    return sp.diags([off, rng.standard_normal(m), off], [-1, 0, 1], format="csc")


def _dense_sym(m, seed):
    R = np.random.default_rng(seed).standard_normal((m, m))
    return sp.csc_matrix(0.5 * (R + R.T) / np.sqrt(m))


KINDS = [_identity, _few, _tridiag, _dense_sym]


def _stored_set(m, n, count, rot):
    """`count` stored constraints at the first, middle and last indices (one: rotating among the three), kinds rotating."""
    if count == 1:
        idx = [[0], [n // 2], [n - 1]][rot % 3]
    elif count == 3:
        idx = [0, n // 2, n - 1]
    else:
        idx = sorted({0, n // 4, n // 2, (3 * n) // 4, n - 1})
    return {k: KINDS[(rot + t) % 4](m, 10 * k + t) for t, k in enumerate(idx)}


def _mixed(m, n, khat, seed, stored):
    mixed = list(_factors(m, n, khat, seed))
    for k, a in stored.items():
        mixed[k] = a
    return mixed


def _dense_of(item):
    if sp.issparse(item):
        return item.toarray()
    V, d = item
    a = (V * d) @ V.T
    return 0.5 * (a + a.T)


def _models(blocks, n, C_lin=None, factored=None):
    """(hybrid / factored model, the same data fully materialised); factored: which blocks stay factored (default all)."""
    from loraine_jl_amd.model import build_factored_model, build_model
    F0 = [-np.eye(_dense_of(b[0]).shape[0]) for b in blocks]
    d_lin = None if C_lin is None else np.ones(C_lin.shape[1])
    fm = build_factored_model(F0, blocks, np.zeros(n), 0.0, d_lin, C_lin, factored_form=1)
    A = [[sp.csc_matrix(F)] + [sp.csc_matrix(_dense_of(it)) for it in b] for F, b in zip(F0, blocks)]
    mm = build_model(A, np.zeros(n), 0.0, d_lin, C_lin)
    if factored is not None:
        for i, f in enumerate(factored):
            if not f:
                fm.AA[i], fm.sigmaA[:, i], fm.qA[:, i], fm.nzA[:, i] = mm.AA[i], mm.sigmaA[:, i], mm.qA[:, i], mm.nzA[:, i]
                fm.factored_blocks[i] = False
    return fm, mm


def _upload(dev, model, dense_threshold=None):
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
    counts = {k: dev.count(k) for k in ("op_factored", "op_dense", "op_sparse")}
    return aax, Rd, counts


def _sym(m, seed):
    R = np.random.default_rng(seed).standard_normal((m, m))
    return 0.5 * (R + R.T)


def _spd(m, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    return G @ G.T, G


def _h_numpy(As, W):
    """H_ij = tr(A_i W A_j W) from the definition."""
    A = np.stack(As)
    T = np.matmul(np.matmul(W, A), W)
    n = len(As)
    return A.reshape(n, -1) @ T.reshape(n, -1).T


@pytest.mark.parametrize("count", [1, 3, 5])
@pytest.mark.parametrize("m,n,khat", SHAPES)
def test_operators_and_schur_matrix_of_a_hybrid_block(dev, m, n, khat, count):
    rot = SHAPES.index((m, n, khat)) + count
    stored = _stored_set(m, n, count, rot)
    mixed = _mixed(m, n, khat, 1000 * m + n + khat, stored)
    fm, mm = _models([mixed], n)
    ns = len(stored)
    assert fm.factored and sorted(fm.stored[0]) == sorted(stored) and fm.AA[0].nnz == sum(a.nnz for a in stored.values())
    # a fully dense stored matrix goes to a dense slot when the threshold is lowered to msz^2 (counts 1 and 5); with the
    # threshold out of reach (count 3 up to msz 70, and every set without a dense matrix) everything stays in the sparse tier, wave or
    # thread by its length -- the cost model would decide by the shape
    has_dense = any(a.nnz == m * m for a in stored.values())
    all_dense = all(a.nnz == m * m for a in stored.values())
    slot = has_dense and (count != 3 or m > 70)      # (msz^2 entries against msz^2 entries in one wave: small blocks only)
    thr = float(m * m) if slot else 1e18
    As = [_dense_of(it) for it in mixed]
    X = _sym(m, m + n)
    y = np.random.default_rng(n).standard_normal(n)
    aax, Rd, cnt = _operators(dev, fm, [X], y, thr)
    assert cnt["op_factored"] == 2
    if not slot:
        assert cnt["op_dense"] == 0 and cnt["op_sparse"] == 2
    else:
        assert cnt["op_dense"] == 2 and cnt["op_sparse"] == (0 if all_dense else 2)
    aax2, Rd2, _ = _operators(dev, fm, [X], y, thr)
    assert np.array_equal(aax, aax2) and np.array_equal(Rd[0], Rd2[0])          # fixed summation order: identical bits
    assert np.array_equal(Rd[0], Rd[0].T)
    assert relerr(aax, -np.array([np.sum(a * X) for a in As])) < 1e-12
    assert relerr(Rd[0], sum(yk * a for yk, a in zip(y, As))) < 1e-12
    aax_m, Rd_m, cnt_m = _operators(dev, mm, [X], y)
    assert cnt_m["op_factored"] == 0
    assert relerr(aax, aax_m) < 1e-12
    assert relerr(Rd[0], Rd_m[0]) < 1e-12
    # mode 1: H_FF + H_SS + cross terms
    W, G = _spd(m, 6 + m)
    _upload(dev, fm, thr)
    for k in stored:
        assert np.array_equal(dev.get_constraint(0, k), stored[k].toarray())
    dev.set_scaling(0, W, G)
    H = dev.schur_assemble(1, want_H=True)
    assert np.array_equal(H, dev.schur_assemble(1, want_H=True))
    assert np.array_equal(H, H.T)
    forms = {}
    try:
        for form in (0, 1):
            dev.set_option("fac_cross_lds", form)
            dev.reset_timing()
            forms[form] = dev.schur_assemble(1, want_H=True)
            if ns < n and not (slot and all_dense):       # (factored positions and a sparse-tier stored row exist)
                assert dev.count("hybrid_cross_lds" if form else "hybrid_cross_global") == 1
    finally:
        dev.set_option("fac_cross_lds", -1)
    assert np.array_equal(forms[0], forms[1]) and np.array_equal(forms[0], H)
    dev.set_scaling(0, W)                                  # W only: U of the rank-k product already is Y
    Hw = dev.schur_assemble(1, want_H=True)
    assert relerr(Hw, H) < 1e-12
    assert np.array_equal(Hw, dev.schur_assemble(1, want_H=True))
    Hnp = _h_numpy(As, W)
    assert relerr(H, Hnp) < 1e-12
    _upload(dev, mm)
    dev.set_scaling(0, W, G)
    H0 = dev.schur_assemble(0, want_H=True)
    assert relerr(H, H0) < 1e-12


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
    return dict(aax=aax, rhs=rhs, a=a, b=b, corr=corr, H=H, factored=dev.count("op_factored")), ab


def _iterate(ms, seed):
    rng = np.random.default_rng(seed)
    Xs, Ss, Cs = [], [], []
    for m in ms:
        Q = rng.standard_normal((m, m)) / np.sqrt(m)
        Xs.append(np.eye(m) + 0.3 * Q @ Q.T)
        Q = rng.standard_normal((m, m)) / np.sqrt(m)
        Ss.append(np.eye(m) + 0.3 * Q @ Q.T)
        Cs.append(_sym(m, seed + m) / np.sqrt(m))
    return Xs, Ss, Cs


@pytest.mark.parametrize("plain", ["factored", "materialised"])
@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_two_blocks_with_linear_rows(dev, order, plain):
    """A hybrid block beside a plain one -- pure factored, or materialised with its factors uploaded for mode 1 -- in either
    order: H in natural index space, C_lin term included."""
    n = 45
    hyb = _mixed(70, n, 4, 5, {0: _identity(70, 0), 9: _few(70, 1), 22: _tridiag(70, 2), 44: _dense_sym(70, 3)})
    pure = _factors(33, n, 2, 6)
    blocks = [(hyb, pure)[k] for k in order]
    ms = tuple((70, 33)[k] for k in order)
    C_lin = sp.random(n, 6, density=0.3, random_state=3, format="csr")
    fm, mm = _models(blocks, n, C_lin=C_lin, factored=[k == 0 or plain == "factored" for k in order])
    assert [bool(s) for s in fm.stored] == [k == 0 for k in order]
    Xp, Sp, Cp = _iterate(ms, 11)
    y = np.random.default_rng(8).standard_normal(n) * 0.1
    dely = np.random.default_rng(9).standard_normal(n) * 0.1
    ref, ab = _rhs_sequence(dev, mm, Xp, Sp, Cp, y, dely)
    got, _ = _rhs_sequence(dev, fm, Xp, Sp, Cp, y, dely, ab)
    assert got["factored"] > 0 and ref["factored"] == 0
    for key in ("aax", "rhs", "corr", "H"):
        assert relerr(got[key], ref[key]) < 1e-12, key
    for i in range(2):
        assert got["a"][i] == pytest.approx(ref["a"][i], rel=1e-8) and got["b"][i] == pytest.approx(ref["b"][i], rel=1e-8)


def test_errors_are_returned(dev):
    from loraine_jl_amd._capi import LoraineHipError
    from loraine_jl_amd.model import build_model
    n, m = 12, 20
    stored = {0: _identity(m, 0), 7: _tridiag(m, 1)}
    mixed = _mixed(m, n, 2, 13, stored)
    fm, mm = _models([mixed], n)
    V, d, khat = fm.lowrank[0]
    # a constraint with both a stored row and factors: the materialised rows of every constraint + all the factors
    full = build_model([[sp.csc_matrix(-np.eye(m))] + [sp.csc_matrix(_dense_of(it)) for it in _factors(m, n, 2, 13)]],
                       np.zeros(n), factors=[_factors(m, n, 2, 13)])
    dev.upload_model(full.AA, full.sigmaA, full.qA, full.msizes)
    dev.upload_lowrank(0, full.lowrank[0][2], full.lowrank[0][0], full.lowrank[0][1])
    with pytest.raises(LoraineHipError, match="has entries"):
        dev.set_factored(0)
    # ... and one overlapping constraint is enough: the two stored rows of the hybrid model under factors of every constraint
    dev.upload_model(fm.AA, fm.sigmaA, fm.qA, fm.msizes)
    dev.upload_lowrank(0, full.lowrank[0][2], full.lowrank[0][0], full.lowrank[0][1])
    with pytest.raises(LoraineHipError, match="has entries"):
        dev.set_factored(0)
    _upload(dev, fm)
    W, G = _spd(m, 6)
    dev.set_scaling(0, W, G)
    with pytest.raises(LoraineHipError, match="factored"):
        dev.schur_assemble(0)
    with pytest.raises(LoraineHipError, match="factored"):
        dev.schur_assemble(-1)
    with pytest.raises(LoraineHipError, match="factored"):
        dev.matvec(np.ones(n))
    with pytest.raises(LoraineHipError, match="factored"):
        dev.prec_setup(1, 1, 1)
    with pytest.raises(LoraineHipError, match="factored"):
        dev.pcg(np.ones(n), 1e-6)
    for k in range(n):
        if k in stored:
            assert np.array_equal(dev.get_constraint(0, k), stored[k].toarray())
        else:
            with pytest.raises(LoraineHipError, match="factored"):
                dev.get_constraint(0, k)
    H1 = dev.schur_assemble(1, want_H=True)
    assert relerr(H1, _h_numpy([_dense_of(it) for it in mixed], W)) < 1e-12


# ---------------------------------------------------------------------------------------------- the auto rule
def _auto_materialised(m=30, seed=4):
    """Unit-vector factors e_k e_k' with a trace row, a tridiagonal and a dense matrix among them: the auto rule materialises
    the block, and its factors then cover the factored constraints only.  Planted strictly feasible as _planted_hybrid."""
    rng = np.random.default_rng(seed)
    n = m
    mixed = [(np.eye(m)[:, [k]], np.ones(1)) for k in range(n)]
    mixed[0] = sp.identity(m, format="csc")
    mixed[11] = sp.diags([np.ones(m - 1), np.ones(m), np.ones(m - 1)], [-1, 0, 1], format="csc") / 3.0
    R = rng.standard_normal((m, m))
    mixed[n - 1] = sp.csc_matrix(0.5 * (R + R.T) / (2.0 * np.sqrt(m)))
    As = [_dense_of(it) for it in mixed]
    Q = rng.standard_normal((m, m))
    X0 = np.eye(m) + Q @ Q.T / m
    b = -np.array([np.sum(a * X0) for a in As])
    y0 = rng.standard_normal(n) / np.sqrt(n)
    C = np.eye(m) - sum(y * a for y, a in zip(y0, As))
    return [-C] + As, b, mixed


def test_auto_materialised_hybrid_block_assembles_from_its_entries(dev):
    """factored_form = -1 on tiny factors plus stored matrices: the block is materialised, the solver still assembles with mode 1
    (datarank from the factors) -- and the factors do not hold the stored constraints.  Mode 1 of such a block must be the
    general assembly over its entries: H against mode 0 of build_model of the same matrices and against NumPy."""
    from loraine_jl_amd.model import build_factored_model, build_model
    A, b, mixed = _auto_materialised()
    m, n = A[0].shape[0], len(b)
    fm = build_factored_model([A[0]], [mixed], b)
    assert not fm.factored and fm.factored_blocks == [False] and fm.AA[0].nnz > 0
    mm = build_model([[sp.csc_matrix(x) for x in A]], b)
    W, G = _spd(m, 3)
    _upload(dev, fm)
    dev.set_scaling(0, W, G)
    dev.reset_timing()
    H1 = dev.schur_assemble(1, want_H=True)
    assert dev.count("lowrank_from_entries") == 1
    _upload(dev, mm)
    dev.set_scaling(0, W, G)
    H0 = dev.schur_assemble(0, want_H=True)
    assert relerr(H1, H0) < 1e-12
    assert relerr(H1, _h_numpy(A[1:], W)) < 1e-12
    # factors of every constraint of a materialised block: mode 1 stays the product of the factors
    unit = [(np.eye(m)[:, [k]], np.ones(1)) for k in range(n)]
    fu = build_factored_model([A[0]], [unit], b)
    assert not fu.factored
    _upload(dev, fu)
    dev.set_scaling(0, W, G)
    dev.reset_timing()
    Hu = dev.schur_assemble(1, want_H=True)
    assert dev.count("lowrank_from_entries") == 0 and dev.count("lowrank") == 1
    assert relerr(Hu, W * W) < 1e-12


def test_auto_materialised_hybrid_model_solves_as_load_model():
    A, b, mixed = _auto_materialised()
    ref = lo.MySolver(lo.make_model([[x.copy() for x in A]], b.copy(), 0.0, None, None), dict(kit=0, verb=0))
    lo.solve(ref)
    om = _opt()
    om.load_model([[sp.csc_matrix(x) for x in A]], b)
    om.optimize()
    of = _opt()
    of.load_factored_model([A[0]], [mixed], b)            # factored_form = -1, the default
    of.optimize()
    s = of.solver
    assert not s.model.factored and s.lowrank and s.dev.count("op_factored") == 0
    assert ref.status == 1
    assert of.termination_status() == om.termination_status() == "OPTIMAL"
    assert s.iter == om.solver.iter == ref.iter
    assert of.objective_value() == pytest.approx(om.objective_value(), rel=1e-8)
    assert of.objective_value() == pytest.approx(lo.objective_value(ref), rel=1e-8)
    assert of.dual_objective_value() == pytest.approx(om.dual_objective_value(), rel=1e-6)


# ---------------------------------------------------------------------------------------------- solves
def _planted_hybrid(m=60, n=80, seed=3):
    """The planted problem of tests/test_gpu_factored.py::_planted (same seed, same draws for the factored constraints) with
    four stored constraints inserted at indices 0, 17, 41 and 83 of the final list: the identity, four symmetric off-diagonal
    pairs plus one diagonal entry, a tridiagonal matrix / 3, a dense symmetric Gaussian / (2 sqrt m)."""
    rng = np.random.default_rng(seed)
    facs = []
    for k in range(n):
        r = 1 + k % 3
        facs.append((rng.standard_normal((m, r)) / np.sqrt(m), rng.choice([-1.0, 1.0], size=r)))
    Q = rng.standard_normal((m, m))
    X0 = np.eye(m) + Q @ Q.T / m
    y0 = list(rng.standard_normal(n) / np.sqrt(n))
    rs = np.random.default_rng(seed + 1000)
    pairs = sp.lil_matrix((m, m))
    for i, j in ((1, 5), (2, 40), (13, 14), (30, 59)):
        pairs[i, j] = pairs[j, i] = rs.standard_normal()
    pairs[7, 7] = 1.0
    R = rs.standard_normal((m, m))
    extra = [(0, sp.identity(m, format="csc")), (17, pairs.tocsc()),
             (41, sp.diags([np.ones(m - 1), np.ones(m), np.ones(m - 1)], [-1, 0, 1], format="csc") / 3.0),
             (83, sp.csc_matrix(0.5 * (R + R.T) / (2.0 * np.sqrt(m))))]
    mixed = list(facs)
    for k, a in extra:                               # (ascending: each index is the position in the final list)
        mixed.insert(k, a)
        y0.insert(k, float(rs.standard_normal() / np.sqrt(n)))
    As = [_dense_of(it) for it in mixed]
    b = -np.array([np.sum(a * X0) for a in As])
    C = np.eye(m) - sum(y * a for y, a in zip(y0, As))
    return [-C] + As, b, mixed


def _opt(**attrs):
    from loraine_jl_amd.optimizer import Optimizer
    o = Optimizer()
    o.set_silent(True)
    o.set_attribute("kit", 0)
    for k, v in attrs.items():
        o.set_attribute(k, v)
    return o


@pytest.mark.parametrize("initpoint", [0, 1])      # 1: the heuristic reads ||AA_i||_F -- factors and stored rows together
def test_planted_solve_of_a_hybrid_model(initpoint):
    A, b, mixed = _planted_hybrid()
    assert len(mixed) == 84 and [k for k, it in enumerate(mixed) if sp.issparse(it)] == [0, 17, 41, 83]
    ref = lo.MySolver(lo.make_model([[x.copy() for x in A]], b.copy(), 0.0, None, None),
                      dict(kit=0, verb=0, initpoint=initpoint))
    lo.solve(ref)
    om = _opt(initpoint=initpoint)
    om.load_model([[sp.csc_matrix(x) for x in A]], b)
    om.optimize()
    of = _opt(initpoint=initpoint)
    of.load_factored_model([A[0]], [mixed], b, factored_form=1)
    of.optimize()
    s = of.solver
    assert s.model.factored and sorted(s.model.stored[0]) == [0, 17, 41, 83] and s.datarank == 3 and s.lowrank
    assert s.dev.count("op_factored") > 0 and s.dev.count("op_sparse") > 0
    assert s.dev.count("hybrid_cross_lds") > 0
    assert ref.status == 1
    assert of.termination_status() == om.termination_status() == "OPTIMAL"
    assert s.iter == om.solver.iter == ref.iter
    assert of.objective_value() == pytest.approx(om.objective_value(), rel=1e-8)
    assert of.objective_value() == pytest.approx(lo.objective_value(ref), rel=1e-8)
    assert of.dual_objective_value() == pytest.approx(om.dual_objective_value(), rel=1e-6)


def test_planted_generator_with_stored_constraints_against_the_oracle():
    """tests/test_gpu_factored.py::test_planted_generator_against_the_oracle with a trace row and one sparse row stored."""
    from loraine_jl_amd.synthetic import FactoredLowRankProblem
    m = 100
    row = sp.lil_matrix((m, m))
    row[3, 3], row[10, 10] = 1.0, -1.0
    row[3, 50] = row[50, 3] = 0.5
    P = FactoredLowRankProblem(m, 200, 2, 4, seed=2, stored=[(0, sp.identity(m, format="csc")), (120, row.tocsc())])
    A = [P.F0()[0]] + [P.constraint(k) for k in range(P.nvar)]
    ref = lo.MySolver(lo.make_model([A], P.b.copy(), 0.0, None, None), dict(kit=0, verb=0))
    lo.solve(ref)
    of = _opt()
    of.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True)
    of.optimize()
    assert of.solver.model.factored and sorted(of.solver.model.stored[0]) == [0, 120]
    assert of.solver.dev.count("op_factored") > 0 and of.solver.dev.count("op_sparse") > 0
    assert of.termination_status() == "OPTIMAL" and ref.status == 1
    assert of.solver.iter == ref.iter
    assert of.objective_value() == pytest.approx(-lo.objective_value(ref), rel=1e-8)
    assert abs(of.objective_value() - P.optimum) <= 1e-6 * (1 + abs(P.optimum))
