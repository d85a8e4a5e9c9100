"""Factor-only models on the MI355X (lrn_set_factored): the factor form of AA vec(.) and mat(AA' .) through the resident
entry points against NumPy straight from the factors and against the same model uploaded with its materialised AA,
symmetry / reproducibility / route counters, blocks + C_lin, error paths, the pattern route, and solves through
Optimizer.load_factored_model (planted problems against datarank = k and the oracle, maxG11 from unit vectors, and the
full size msz 2000 / nvar 4000, which cannot be loaded as matrices at all).

Tolerances are the suite's own for the same kind of comparison (tests/test_gpu_lowrank.py): 1e-12 relative Frobenius for
a product against another formulation, rel=1e-8 between two solves of one problem, rel=1e-6 against a known optimum,
1e-11 for products at full size (tests/test_gpu_fullsize.py)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import loraine_oracle as lo

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")

CASES = [  # msz, nvar, khat, sparse factors: the shape grid of tests/test_gpu_lowrank.py::CASES
    (16, 5, 1, False), (16, 37, 16, False), (96, 37, 2, True), (96, 130, 4, False), (130, 37, 8, True),
    (130, 130, 16, False), (257, 5, 4, True), (257, 130, 1, True), (333, 37, 8, False), (333, 300, 2, False),
    (257, 300, 1, False), (130, 300, 16, True), (333, 130, 4, True), (96, 5, 8, False)]


@pytest.fixture(scope="module")
def dev():
    import loraine_jl_amd
    d = loraine_jl_amd.Device(0)
    yield d
    d.close()


def relerr(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


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


def _A(facs):
    out = []
    for V, d in facs:
        a = (V * d) @ V.T
        out.append(sp.csc_matrix(0.5 * (a + a.T)))
    return out


def _sym(m, seed):
    R = np.random.default_rng(seed).standard_normal((m, m))
    return 0.5 * (R + R.T)                       # symmetric, NOT definite


def _spd(m, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    return G @ G.T, G


def _models(blocks, n, C_lin=None, factored=None):
    """(factored model, materialised model) of the same data; factored: which blocks stay factored (default all)."""
    from loraine_jl_amd.model import build_factored_model, build_model
    F0 = [-np.eye(b[0][0].shape[0]) for b in blocks]
    d_lin = None if C_lin is None else np.ones(C_lin.shape[1])
    fm = build_factored_model(F0, blocks, np.zeros(n), 0.0, d_lin, C_lin, factored_form=1)
    A = [[sp.csc_matrix(F)] + _A(b) for F, b in zip(F0, blocks)]
    mm = build_model(A, np.zeros(n), 0.0, d_lin, C_lin, factors=blocks)
    if factored is not None:                     # a mixed upload: the un-factored blocks carry their materialised AA
        for i, f in enumerate(factored):
            if not f:
                fm.AA[i], fm.sigmaA[:, i], fm.qA[:, i], fm.nzA[:, i] = mm.AA[i], mm.sigmaA[:, i], mm.qA[:, i], mm.nzA[:, i]
                fm.factored_blocks[i] = False
    return fm, mm


def _upload(dev, model):
    dev.upload_model(model.AA, model.sigmaA, model.qA, model.msizes, C_lin=model.C_lin if model.nlin else None)
    for i, (V, d, khat) in enumerate(model.lowrank):
        dev.upload_lowrank(i, khat, V, d)
        if getattr(model, "factored", False) and model.factored_blocks[i]:
            dev.set_factored(i)


def _aa_x_numpy(blocks, Xs):
    """(AA vec(X))_k = -sum_i sum_p d_p v_p' X_i v_p, straight from the factors."""
    n = len(blocks[0])
    y = np.zeros(n)
    for facs, X in zip(blocks, Xs):
        for k, (V, d) in enumerate(facs):
            y[k] -= float(np.sum(d * np.einsum("mp,mq,qp->p", V, X, V)))
    return y


def _aat_numpy(facs, x):
    """mat(AA' x) = -sum_k x_k V_k D_k V_k'."""
    m = facs[0][0].shape[0]
    M = np.zeros((m, m))
    for k, (V, d) in enumerate(facs):
        M -= x[k] * (V * d) @ V.T
    return M


def _operators(dev, model, Xs, y):
    """AA vec(X) and Rd = C - S - mat(AA'y) with C = S = 0 through the resident entry points."""
    _upload(dev, model)
    for i, X in enumerate(Xs):
        dev.ip_set_c(i, np.zeros_like(X))
        dev.ip_set_iterate(i, X, np.zeros_like(X))
    dev.reset_timing()
    aax = dev.ip_aa_x()
    dev.ip_residual_d(y)
    Rd = [dev.dbg_get_block(i, "Rd")[0] for i in range(len(Xs))]
    counts = {k: dev.count(k) for k in ("op_factored", "op_dense", "op_sparse")}
    return aax, Rd, counts


@pytest.mark.parametrize("m,n,khat,sparse", CASES)
def test_operators_match_numpy_and_the_materialised_model(dev, m, n, khat, sparse):
    facs = _factors(m, n, khat, 1000 * m + n + khat, sparse)
    fm, mm = _models([facs], n)
    assert fm.lowrank[0][2] == khat and fm.AA[0].nnz == 0
    X = _sym(m, m + n)
    y = np.random.default_rng(n).standard_normal(n)
    aax, Rd, cnt = _operators(dev, fm, [X], y)
    assert cnt["op_factored"] == 2 and cnt["op_dense"] == 0 and cnt["op_sparse"] == 0
    aax2, Rd2, _ = _operators(dev, fm, [X], y)
    assert np.array_equal(aax, aax2) and np.array_equal(Rd[0], Rd2[0])          # fixed summation order: identical bits
    assert np.array_equal(Rd[0], Rd[0].T)
    assert relerr(aax, _aa_x_numpy([facs], [X])) < 1e-12
    assert relerr(-Rd[0], _aat_numpy(facs, y)) < 1e-12
    aax_m, Rd_m, cnt_m = _operators(dev, mm, [X], y)
    assert cnt_m["op_factored"] == 0 and cnt_m["op_dense"] + cnt_m["op_sparse"] > 0
    assert relerr(aax, aax_m) < 1e-12
    assert relerr(Rd[0], Rd_m[0]) < 1e-12


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
    H = dev.schur_assemble(1, want_H=True)
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


@pytest.mark.parametrize("factored", [(True, False), (False, True), (True, True)])
def test_two_blocks_with_linear_rows(dev, factored):
    n = 45
    blocks = [_factors(70, n, 4, 5, False), _factors(33, n, 2, 6, True)]
    C_lin = sp.random(n, 6, density=0.3, random_state=3, format="csr")
    fm, mm = _models(blocks, n, C_lin=C_lin, factored=factored)
    Xs = [_sym(70, 1), _sym(33, 2)]
    y = np.random.default_rng(8).standard_normal(n)
    aax, Rd, cnt = _operators(dev, fm, Xs, y)
    assert cnt["op_factored"] == 2 * sum(factored)
    assert relerr(aax, _aa_x_numpy(blocks, Xs)) < 1e-12
    aax_m, Rd_m, _ = _operators(dev, mm, Xs, y)
    assert relerr(aax, aax_m) < 1e-12
    for i in range(2):
        assert np.array_equal(Rd[i], Rd[i].T)
        assert relerr(-Rd[i], _aat_numpy(blocks[i], y)) < 1e-12
        assert relerr(Rd[i], Rd_m[i]) < 1e-12
    # the right-hand sides and the mode-1 Schur matrix (C_lin term included) of one iterate
    Xp, Sp, Cp = _iterate((70, 33), 11)
    dely = np.random.default_rng(9).standard_normal(n) * 0.1
    ref, ab = _rhs_sequence(dev, mm, Xp, Sp, Cp, y * 0.1, dely)
    got, _ = _rhs_sequence(dev, fm, Xp, Sp, Cp, y * 0.1, dely, ab)
    assert got["factored"] > 0 and ref["factored"] == 0
    for key in ("aax", "rhs", "corr", "H"):
        assert relerr(got[key], ref[key]) < 1e-12, key


def test_pattern_route_is_not_taken_by_a_factored_block(dev):
    """From msz = wmw_pattern_min on, right-hand sides of blocks whose constraints are all sparse go through the pattern of
    AA -- empty for a factored block.  The option is lowered instead of growing the problem."""
    m, n = 96, 60
    facs = _factors(m, n, 2, 21, True)
    fm, mm = _models([facs], n)
    Xp, Sp, Cp = _iterate((m,), 12)
    y = np.random.default_rng(1).standard_normal(n) * 0.1
    dely = np.random.default_rng(2).standard_normal(n) * 0.1
    ref, ab = _rhs_sequence(dev, mm, Xp, Sp, Cp, y, dely)
    dev.set_option("wmw_pattern_min", 8)
    try:
        got, _ = _rhs_sequence(dev, fm, Xp, Sp, Cp, y, dely, ab)
    finally:
        dev.set_option("wmw_pattern_min", 1500)
    assert np.linalg.norm(ref["rhs"]) > 0 and np.linalg.norm(ref["corr"]) > 0
    for key in ("aax", "rhs", "corr"):
        assert relerr(got[key], ref[key]) < 1e-12, key
    assert got["a"][0] == pytest.approx(ref["a"][0], rel=1e-8) and got["b"][0] == pytest.approx(ref["b"][0], rel=1e-8)


def test_errors_are_returned(dev):
    from loraine_jl_amd._capi import LoraineHipError
    n, m = 12, 20
    facs = _factors(m, n, 2, 13, False)
    fm, mm = _models([facs], n)
    V, d, khat = fm.lowrank[0]
    dev.upload_model(fm.AA, fm.sigmaA, fm.qA, fm.msizes)
    with pytest.raises(LoraineHipError, match="no factors"):
        dev.set_factored(0)
    dev.upload_model(mm.AA, mm.sigmaA, mm.qA, mm.msizes)
    dev.upload_lowrank(0, khat, V, d)
    with pytest.raises(LoraineHipError, match="has entries"):
        dev.set_factored(0)
    with pytest.raises(LoraineHipError, match="block"):
        dev.set_factored(3)
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
    with pytest.raises(LoraineHipError, match="factored"):
        dev.get_constraint(0, 0)
    # mode 1 is the assembly of a factored block: H, hidx / ipos (identity sigmaA) and the export are those of the data
    H1 = dev.schur_assemble(1, want_H=True)
    As = [a.toarray() for a in _A(facs)]
    Href = np.array([[np.sum((W @ ai @ W) * aj) for aj in As] for ai in As])
    assert relerr(H1, Href) < 1e-12
    dev.set_factored(0, False)                   # taken back: an empty AA again
    assert np.array_equal(dev.schur_assemble(0, want_H=True), np.zeros((n, n)))


# ---------------------------------------------------------------------------------------------- solves
def _planted(m=60, n=80, seed=3):
    """The planted problem of tests/test_gpu_lowrank.py::_planted (same seed, same draws), factors kept."""
    rng = np.random.default_rng(seed)
    facs = []
    for k in range(n):
        r = 1 + k % 3
        facs.append((rng.standard_normal((m, r)) / np.sqrt(m), rng.choice([-1.0, 1.0], size=r)))
    As = [a.toarray() for a in _A(facs)]
    Q = rng.standard_normal((m, m))
    X0 = np.eye(m) + Q @ Q.T / m
    b = -np.array([np.sum(a * X0) for a in As])
    y0 = rng.standard_normal(n) / np.sqrt(n)
    C = np.eye(m) - sum(y * a for y, a in zip(y0, As))
    return [-C] + As, b, facs


def _opt(**attrs):
    from loraine_jl_amd.optimizer import Optimizer
    o = Optimizer()
    o.set_silent(True)
    o.set_attribute("kit", 0)
    for k, v in attrs.items():
        o.set_attribute(k, v)
    return o


@pytest.mark.parametrize("initpoint", [0, 1])      # 1: the heuristic reads ||AA_i||_F -- of a factored block from its factors
def test_planted_solve_from_factors(initpoint):
    A, b, facs = _planted()
    ref = lo.MySolver(lo.make_model([[x.copy() for x in A]], b.copy(), 0.0, None, None),
                      dict(kit=0, verb=0, initpoint=initpoint))
    lo.solve(ref)
    o3 = _opt(datarank=3, initpoint=initpoint)
    o3.load_model([[sp.csc_matrix(x) for x in A]], b)
    o3.optimize()
    of = _opt(initpoint=initpoint)
    of.load_factored_model([A[0]], [facs], b, factored_form=1)
    of.optimize()
    s = of.solver
    assert s.model.factored and s.model.AA[0].nnz == 0 and s.datarank == 3 and s.lowrank
    assert s.dev.count("op_factored") > 0 and s.dev.count("op_dense") == 0 and s.dev.count("op_sparse") == 0
    assert s.dev.count("adense_bytes") == 0
    assert of.termination_status() == o3.termination_status() == "OPTIMAL"
    assert s.iter == o3.solver.iter == ref.iter
    assert of.objective_value() == pytest.approx(o3.objective_value(), rel=1e-8)
    assert of.objective_value() == pytest.approx(lo.objective_value(ref), rel=1e-8)
    assert of.dual_objective_value() == pytest.approx(o3.dual_objective_value(), rel=1e-6)


def test_planted_generator_against_the_oracle():
    """The full-size generator at (100, 200, rank X* 4): against the oracle's solve of the materialised model, so that a
    miss at full size can be told from a wrong generator."""
    from loraine_jl_amd.synthetic import FactoredLowRankProblem
    P = FactoredLowRankProblem(100, 200, 2, 4, seed=2)
    A = [P.F0()[0]] + [P.constraint(k) for k in range(P.nvar)]
    ref = lo.MySolver(lo.make_model([A], P.b.copy(), 0.0, None, None), dict(kit=0, verb=0))
    lo.solve(ref)
    of = _opt()
    of.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True)
    of.optimize()
    assert of.solver.model.factored                                # dense factors: the auto rule keeps them factored
    assert of.termination_status() == "OPTIMAL" and ref.status == 1
    assert of.solver.iter == ref.iter
    assert of.objective_value() == pytest.approx(-lo.objective_value(ref), rel=1e-8)
    assert abs(of.objective_value() - P.optimum) <= 1e-6 * (1 + abs(P.optimum))


@pytest.mark.parametrize("form", [-1, 1])
def test_maxG11_from_unit_vectors(form):
    """maxG11 as F_0 + factors e_k: through the auto rule (materialised: the sparse path) and forced factored."""
    from loraine_jl_amd.model import lowrank_factor, model_from_sdpa
    m0 = model_from_sdpa(os.path.join(GOLD, "maxG11.dat-s"))
    msz = int(m0.msizes[0])
    facs = [lowrank_factor(m0.A[0][k + 1], msz, 1) for k in range(m0.n)]
    assert all(f is not None and f[0].shape[1] == 1 for f in facs)
    o = _opt()
    o.load_factored_model([m0.A[0][0]], [facs], m0.b, m0.b_const, factored_form=form)
    o.optimize()
    s = o.solver
    assert s.model.factored == (form == 1)
    if form == 1:
        assert s.dev.count("op_factored") > 0 and s.dev.count("op_sparse") == 0
    else:
        assert s.dev.count("op_factored") == 0 and s.dev.count("op_sparse") > 0
    assert s.dev.count("lowrank") > 0
    assert o.termination_status() == "OPTIMAL"
    assert o.objective_value() == pytest.approx(629.1648, rel=1e-6)


# ---------------------------------------------------------------------------------------------- full size
MSZ, NVAR = 2000, 4000


@pytest.mark.timeout(300)      # sized from the first run: 5.1 s for the whole test on one MI355X
def test_fullsize_factored_solve():
    """msz 2000, nvar 4000, dense factors of rank 2 with a planted optimum: as matrices this model is 128 GB on the host and
    on the device and cannot be loaded; from the factors it is 128 MB."""
    from loraine_jl_amd.optimizer import Optimizer
    from loraine_jl_amd.synthetic import FactoredLowRankProblem
    P = FactoredLowRankProblem(MSZ, NVAR, 2, 4)
    o = Optimizer()
    o.set_silent(True)
    o.set_attribute("kit", 0)
    o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True)
    o._copy_to()                                                   # upload; the solve follows the operator check
    s = o.solver
    dev = s.dev
    assert s.model.factored and s.datarank == 2
    # the operator at this size: AA vec(X) of a random symmetric X on 64 sampled constraints
    X = _sym(MSZ, 5)
    dev.ip_set_iterate(0, X, np.eye(MSZ))
    aax = dev.ip_aa_x()
    idx = np.random.default_rng(6).choice(NVAR, size=64, replace=False)
    ref = np.array([-np.sum(P.d[k] * np.einsum("mp,mq,qp->p", P.V[k], X, P.V[k])) for k in idx])
    print("full size: |aa_x - numpy| / |numpy| on 64 constraints =", relerr(aax[idx], ref))
    assert relerr(aax[idx], ref) < 1e-11
    # ... and mat(AA'y): Rd = C - S - mat(AA'y) with C = S = 0 is sum_k y_k A_k = Vall diag(y (x) d) Vall', one host product
    y = np.random.default_rng(7).standard_normal(NVAR)
    dev.ip_set_c(0, np.zeros((MSZ, MSZ)))
    dev.ip_set_iterate(0, X, np.zeros((MSZ, MSZ)))
    dev.ip_residual_d(y)
    Rd = dev.dbg_get_block(0, "Rd")[0]
    Vall = P.V.transpose(1, 0, 2).reshape(MSZ, -1)
    Rref = (Vall * (y[:, None] * P.d).ravel()) @ Vall.T
    print("full size: |Rd - numpy| / |numpy| =", relerr(Rd, Rref))
    assert np.array_equal(Rd, Rd.T)
    assert relerr(Rd, Rref) < 1e-11
    dev.ip_set_c(0, P.C_dense())
    from loraine_jl_amd import solvers
    solvers.solve(s, o.halpha)
    gap = abs(o.objective_value() - P.optimum)
    print(f"full size: status {o.termination_status()}, {s.iter} iterations, objective {o.objective_value():.12e}, planted "
          f"{P.optimum:.12e}, |diff| / (1 + |b'y*|) = {gap / (1 + abs(P.optimum)):.3e}, DIMACS {s.DIMACS_error:.3e}, "
          f"device bytes at most {dev.count('device_bytes_peak') / 1e9:.2f} GB")
    assert o.termination_status() == "OPTIMAL"
    assert gap <= 1e-6 * (1 + abs(P.optimum))
    # the device never held the dense data (it would be 128 GB)
    assert dev.count("op_factored") > 0 and dev.count("op_dense") == 0 and dev.count("op_sparse") == 0
    assert dev.count("adense_bytes") == 0
    assert 0 < dev.count("device_bytes_peak") < 16e9
