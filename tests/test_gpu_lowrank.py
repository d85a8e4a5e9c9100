"""Schur assembly from rank-k constraint factors (lrn_upload_lowrank, lrn_schur_assemble mode 1) on the MI355X: against
the general path (mode 0) and the oracle's makeBBBBs, blocks + C_lin, shards, reproducibility, error paths and full
solves with datarank = k."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import loraine_oracle as lo

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def dev():
    import loraine_jl_amd
    d = loraine_jl_amd.Device(0)
    yield d
    d.close()


def relerr(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _spd(m, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    return G @ G.T, G


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


def _model(blocks, n, C_lin=None, factors=True):
    from loraine_jl_amd.model import build_model
    A = [[sp.csc_matrix(-np.eye(V[0][0].shape[0]))] + _A(V) for V in blocks]
    d_lin = None if C_lin is None else np.ones(C_lin.shape[1])
    return build_model(A, np.zeros(n), 0.0, d_lin, C_lin, factors=blocks if factors else None)


def _upload(dev, model):
    dev.upload_model(model.AA, model.sigmaA, model.qA, model.msizes, C_lin=model.C_lin if model.nlin else None)
    for i, (V, d, khat) in enumerate(model.lowrank):
        dev.upload_lowrank(i, khat, V, d)


CASES = [  # msz, nvar, khat, sparse factors, form (-1 auto, 0 gather, 1 dense product), G given
    (16, 5, 1, False, -1, True), (16, 37, 16, False, 1, False), (96, 37, 2, True, 0, True), (96, 130, 4, False, 1, True),
    (130, 37, 8, True, 0, False), (130, 130, 16, False, -1, True), (257, 5, 4, True, -1, False),
    (257, 130, 1, True, 1, False), (333, 37, 8, False, 1, False), (333, 300, 2, False, 0, True),
    (257, 300, 1, False, -1, True), (130, 300, 16, True, 0, True), (333, 130, 4, True, 1, True),
    (96, 5, 8, False, 0, False)]


@pytest.mark.parametrize("m,n,khat,sparse,form,withG", CASES)
def test_lowrank_matches_general_path(dev, m, n, khat, sparse, form, withG):
    facs = _factors(m, n, khat, 1000 * m + n + khat, sparse)
    model = _model([facs], n)
    assert model.lowrank[0][2] == khat
    _upload(dev, model)
    W, G = _spd(m, m + n)
    dev.set_scaling(0, W, G if withG else None)
    H0 = dev.schur_assemble(0, want_H=True)
    dev.set_option("lowrank_form", form)
    try:
        H1 = dev.schur_assemble(1, want_H=True)
    finally:
        dev.set_option("lowrank_form", -1)
    assert relerr(H1, H0) < 1e-12
    assert np.array_equal(H1, H1.T)
    if m <= 130 and n <= 130:      # the oracle's makeBBBBs (the reference's loops) on the same data
        om = lo.make_model([[-np.eye(m)] + [a.toarray() for a in _A(facs)]], np.zeros(n), 0.0, None, None)
        Hr = lo.makeBBBBs(om.n, om.nlmi, om.A, om.AA, [W], om.qA, om.sigmaA)
        Hr = np.tril(Hr) + np.tril(Hr, -1).T
        assert relerr(H1, Hr) < 1e-12


def test_blocks_and_linear_rows(dev):
    n = 45
    blocks = [_factors(70, n, 4, 5, False), _factors(33, n, 2, 6, True)]
    rng = np.random.default_rng(2)
    C_lin = sp.random(n, 6, density=0.3, random_state=3, format="csr")
    model = _model(blocks, n, C_lin=C_lin)
    _upload(dev, model)
    for i, m in enumerate((70, 33)):
        W, G = _spd(m, 20 + i)
        dev.set_scaling(i, W, G if i == 0 else None)
    dev.set_lin(rng.random(6) + 0.5, rng.random(6) + 0.5)
    H0 = dev.schur_assemble(0, want_H=True)
    H1 = dev.schur_assemble(1, want_H=True)
    assert relerr(H1, H0) < 1e-12


def test_sharded_columns(dev):
    """world = 3 column ownership: the union of the shards is the full mode-1 matrix."""
    import torch
    n, m = 300, 96
    model = _model([_factors(m, n, 4, 9, False)], n)
    _upload(dev, model)
    W, G = _spd(m, 4)
    dev.set_scaling(0, W, G)
    Hfull = dev.schur_assemble(1, want_H=True)
    assert dev.schur_plan(1) == 0          # column blocks + all-gather
    parts = []
    for r in range(3):
        dev.set_shard(r, 3)
        dev.schur_assemble(1)
        buf = torch.zeros(dev.shard_doubles(), dtype=torch.float64, device="cuda")
        dev.schur_export_shard(buf)
        parts.append(buf)
    dev.schur_import_all(torch.cat(parts))
    H2 = dev.schur_get()
    dev.set_shard(0, 1)
    assert relerr(H2, Hfull) < 1e-15


def test_bitwise_reproducible_and_route_counted(dev):
    n, m = 130, 257
    model = _model([_factors(m, n, 8, 11, False)], n)
    _upload(dev, model)
    W, G = _spd(m, 5)
    dev.set_scaling(0, W, G)
    dev.set_option("profile", 1)
    dev.set_option("reset_timing", 1)
    try:
        Ha = dev.schur_assemble(1, want_H=True)
        Hb = dev.schur_assemble(1, want_H=True)
        assert dev.count("lowrank") > 0
        assert dev.timing("lowrank") > 0.0
    finally:
        dev.set_option("profile", 0)
    assert np.array_equal(Ha, Hb)


def test_errors_are_returned(dev):
    from loraine_jl_amd._capi import LoraineHipError
    n, m = 12, 20
    model = _model([_factors(m, n, 2, 13, False)], n)
    dev.upload_model(model.AA, model.sigmaA, model.qA, model.msizes)
    W, G = _spd(m, 6)
    dev.set_scaling(0, W, G)
    with pytest.raises(LoraineHipError, match="no factors"):
        dev.schur_assemble(1)
    V, d, khat = model.lowrank[0]
    for bad in (0, 3, 32):
        with pytest.raises(LoraineHipError, match="khat"):
            dev.upload_lowrank(0, bad, sp.csr_matrix((n * bad, m)) if bad else sp.csr_matrix((0, m)), np.zeros(n * bad))
    dev.upload_lowrank(0, khat, V, d)
    H1 = dev.schur_assemble(1, want_H=True)
    assert relerr(H1, dev.schur_assemble(0, want_H=True)) < 1e-12
    # after a fresh model without a scaling: neither G nor W
    dev.upload_model(model.AA, model.sigmaA, model.qA, model.msizes)
    dev.upload_lowrank(0, khat, V, d)
    with pytest.raises(LoraineHipError, match="G or W"):
        dev.schur_assemble(1)


def _planted(m=60, n=80, seed=3):
    """Strictly feasible SDP with rank <= 3 signed dense factors, in the convention of lrn_synthetic_dense_problem (AA = -A):
    X0 = I + QQ'/m, b = AA vec(X0) = -<A_k, X0>, S0 = I, C = S0 + mat(AA' y0) = S0 - sum y0_k A_k; F_0 = -C."""
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
    return [-C] + As, b


def _solve(A, b, resident, datarank):
    from loraine_jl_amd.optimizer import Optimizer
    o = Optimizer(resident=resident)
    o.set_silent(True)
    o.set_attribute("kit", 0)
    o.set_attribute("datarank", datarank)
    o.load_model([[sp.csc_matrix(x) for x in A]], b)
    o.optimize()
    return o


@pytest.mark.parametrize("resident", [True, False])
def test_planted_solve(resident):
    A, b = _planted()
    ref = lo.MySolver(lo.make_model([[x.copy() for x in A]], b.copy(), 0.0, None, None), dict(kit=0, verb=0))
    lo.solve(ref)
    o0 = _solve(A, b, resident, 0)
    assert o0.solver.dev.count("lowrank") == 0
    o3 = _solve(A, b, resident, 3)
    assert o3.solver.datarank == 3 and o3.solver.lowrank
    assert o3.solver.dev.count("lowrank") > 0
    assert o3.termination_status() == o0.termination_status() == "OPTIMAL"
    assert o3.solver.iter == o0.solver.iter == ref.iter
    assert o3.objective_value() == pytest.approx(o0.objective_value(), rel=1e-8)
    assert o3.objective_value() == pytest.approx(lo.objective_value(ref), rel=1e-8)


def _sdpa(name, **opts):
    from loraine_jl_amd.optimizer import Optimizer
    o = Optimizer(resident=False)
    o.set_silent(True)
    for k, v in opts.items():
        o.set_attribute(k, v)
    o.read_from_file(os.path.join(GOLD, name))
    o.optimize()
    return o


def test_maxG11_datarank_1():
    o1 = _sdpa("maxG11.dat-s", kit=0, datarank=1)
    assert o1.solver.dev.count("lowrank") > 0
    assert o1.termination_status() == "OPTIMAL"
    assert o1.objective_value() == pytest.approx(629.1648, rel=1e-6)
    om = _sdpa("maxG11.dat-s", kit=0, datarank=-1)
    assert o1.solver.iter == om.solver.iter


def test_theta1_fallback_is_the_general_path():
    o2 = _sdpa("theta1.dat-s", kit=0, datarank=2)
    assert o2.solver.datarank == 0 and not o2.solver.lowrank
    assert o2.solver.dev.count("lowrank") == 0
    o0 = _sdpa("theta1.dat-s", kit=0, datarank=0)
    assert o2.solver.iter == o0.solver.iter
    keys = ("iter", "primal_obj", "dual_obj", "dimacs", "errs", "mu", "sigma")
    assert [[t[k] for k in keys] for t in o2.solver.trace] == [[t[k] for k in keys] for t in o0.solver.trace]
    assert np.array_equal(o2.solver.y, o0.solver.y)
