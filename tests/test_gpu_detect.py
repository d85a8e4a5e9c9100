"""Low-rank detection on the device (csrc/detect.hip, lrn_lowrank_detect) on the seeded cases of tests/detect_cases.py --
ranks, inertia, residuals against an independent long-double evaluation, exact zeros in the padding, the same bits whatever
else is in the chunk -- and planted solves through Optimizer.load_detected_model against load_model.

Tolerances: the residual the device reports agrees with the long-double evaluation of ||A - V D V'||_F from the returned V, d
within  gamma_(kmax + 4) || |A| + |V| |V|' ||_F  (the entries: kmax products accumulated in the MFMA, one subtraction, with
slack)  +  gamma_L resid,  L = 16 + 6 + 4 + ntiles + 2: the longest addition chain of the kernel's fixed-order sum -- 16 terms
per lane, 6 butterfly steps, 4 waves, the tiles of the matrix in order -- and the rounding of a square and of the root.
Observed err / bound: 0.035 at the most (kmax 16), 0.018 (kmax 64).  Solves: rel=1e-8 between two solves, 1e-6 for the dual objective
(tests/test_gpu_factored.py)."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def gamma(n):
    return n * U / (1.0 - n * U)


@pytest.fixture(scope="module")
def dev():
    import loraine_jl_amd
    d = loraine_jl_amd.Device(0)
    yield d
    d.close()


_RUNS = {}


def run_all(dev, kmax):
    """Every case of this kmax through the C ABI, batched by side; computed once, shared, left unchanged."""
    if kmax not in _RUNS:
        out = {}
        by_m = {}
        for n in dc.cases_for(kmax):
            by_m.setdefault(dc.CASES[n].m, []).append(n)
        for m, names in sorted(by_m.items()):
            rank, resid, V, d = dev.lowrank_detect(dc.batch(names), kmax, tol=dc.TOL, rank_rtol=dc.RANK_RTOL,
                                                   omega=dc.omega_for(m, kmax))
            for i, n in enumerate(names):
                out[n] = (int(rank[i]), float(resid[i]), V[i].copy(), d[i].copy())
        _RUNS[kmax] = out
    return _RUNS[kmax]


def test_symbol_and_argument_checks(dev):
    assert hasattr(dev.lib, "lrn_lowrank_detect")
    from loraine_jl_amd import LoraineHipError
    a = np.eye(4)[None]
    with pytest.raises(LoraineHipError, match="kmax = 32"):
        dev.lowrank_detect(a, 32, omega=np.ones((4, 40)))
    with pytest.raises(ValueError, match="omega"):
        dev.lowrank_detect(a, 16, omega=np.ones((4, 23)))
    dev.lowrank_detect(a, 16)
    held = dev.count("device_bytes")
    dev.set_option("detect_release", 0)                                      # 0 does nothing
    assert held > 0 and dev.count("device_bytes") == held
    dev.set_option("detect_release", 1)
    assert dev.count("device_bytes") < held


@pytest.mark.parametrize("kmax", [16, 64])
def test_rank_inertia_residual_padding(dev, kmax):
    runs = run_all(dev, kmax)
    worst = 0.0
    for name, (rank, resid, V, d) in runs.items():
        c = dc.CASES[name]
        assert rank == (c.rank if c.rank <= kmax else -1), name
        assert np.isfinite(resid), name
        r = max(rank, 0)
        assert not V[:, r:].any() and not d[r:].any(), name                  # exact zeros in the padding
        assert set(np.unique(d[:r])) <= {-1.0, 1.0}, name
        if rank >= 0:
            assert (int(np.sum(d > 0)), int(np.sum(d < 0))) == c.inertia, name
        Al, Vl = c.A.astype(np.longdouble), V.astype(np.longdouble)
        ind = float(np.sqrt(np.sum((Al - (Vl * d.astype(np.longdouble)) @ Vl.T) ** 2)))
        if rank >= 0:
            assert ind <= dc.TOL, (name, ind)
        ntile = ((c.m + 63) // 64) * ((c.m + 63) // 64 + 1) // 2
        L = 16 + 6 + 4 + ntile + 2
        bound = gamma(kmax + 4) * float(np.linalg.norm(np.abs(c.A) + np.abs(V) @ np.abs(V).T)) + gamma(L) * ind
        print(f"kmax {kmax} {name}: rank {rank} resid {resid:.3e} long double {ind:.3e} err/bound "
              f"{abs(resid - ind) / bound if bound else 0.0:.3f}")
        assert abs(resid - ind) <= bound, (name, resid, ind, bound)
        worst = max(worst, abs(resid - ind) / bound if bound else 0.0)
    print(f"kmax {kmax}: largest err / bound {worst:.3f}")


def _same(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("kmax", [16, 64])
def test_same_bits_alone_in_a_batch_and_again(dev, kmax):
    runs = run_all(dev, kmax)
    for name, ref in runs.items():
        c = dc.CASES[name]
        om = dc.omega_for(c.m, kmax)
        for _ in range(2):                                                   # alone, and on a repeated call
            rank, resid, V, d = dev.lowrank_detect(c.A[None], kmax, tol=dc.TOL, rank_rtol=dc.RANK_RTOL, omega=om)
            assert _same((int(rank[0]), float(resid[0]), V[0], d[0]), ref), name
    names70 = dc.batch70()
    base = dc.batch(names70)
    om = dc.omega_for(200, kmax)
    for name in sorted(set(names70)):
        for pos in (0, 35, 69):                                              # first, middle, last of 70
            mats = base.copy()
            mats[pos] = dc.CASES[name].A
            rank, resid, V, d = dev.lowrank_detect(mats, kmax, tol=dc.TOL, rank_rtol=dc.RANK_RTOL, omega=om)
            assert _same((int(rank[pos]), float(resid[pos]), V[pos], d[pos]), runs[name]), (name, pos)


@pytest.mark.parametrize("kmax", [16, 64])
@pytest.mark.parametrize("m", [65, 200])
def test_same_bits_in_a_mixed_batch_of_3(dev, m, kmax):
    """A batch of exactly 3, accepted and rejected constraints side by side, in every rotation: each case first, middle
    and last."""
    runs = run_all(dev, kmax)
    names = dc.batch3(m)
    om = dc.omega_for(m, kmax)
    for rot in range(3):
        order = names[rot:] + names[:rot]
        rank, resid, V, d = dev.lowrank_detect(dc.batch(order), kmax, tol=dc.TOL, rank_rtol=dc.RANK_RTOL, omega=om)
        assert len(rank) == 3
        for pos, name in enumerate(order):
            assert _same((int(rank[pos]), float(resid[pos]), V[pos], d[pos]), runs[name]), (name, pos)
    verdicts = {runs[n][0] >= 0 for n in names}
    assert verdicts == ({True, False} if kmax == 16 or m == 65 else {True})      # (rank 17 is accepted at kmax 64)


@pytest.mark.parametrize("kmax", [16, 64])
def test_detect_factors_gives_the_same_bits_for_1_2_and_7_chunks(dev, kmax):
    from loraine_jl_amd import detect
    runs = run_all(dev, kmax)
    names70 = dc.batch70()
    A = [[sp.identity(200, format="csc")] + [sp.csc_matrix(dc.CASES[n].A) for n in names70]]
    one = 200 * 200 * 8 / 2 ** 20
    for budget, chunks in ((70 * one, 1), (35 * one, 2), (10 * one, 7)):
        items, rep = detect.detect_factors(A, 70, kmax, dev, budget_mb=budget, seed=0, datasparsity=-1, host_side=-1)   # (all 70 to the device)
        assert rep["chunks"] == chunks and rep["counters"]["detect_calls"] == chunks
        acc = sum(1 for n in names70 if runs[n][0] >= 0)
        assert rep["counters"]["detect_accepted"] == acc == rep["accepted"] and rep["counters"]["detect_rejected"] == 70 - acc
        for k, n in enumerate(names70):
            rank, _, V, d = runs[n]
            if rank < 0:
                assert sp.issparse(items[0][k]), n
            else:
                assert np.array_equal(items[0][k][0], V[:, :rank]) and np.array_equal(items[0][k][1], d[:rank]), (n, chunks)
    assert dev.count("device_bytes") < 200 * 200 * 8                         # the chunk workspace was released


@pytest.mark.parametrize("kmax", [16, 64])
def test_sweeps_within_two_of_the_restatement(dev, kmax):
    for name in dc.cases_for(kmax):                                          # every case, at both kmax
        c = dc.CASES[name]
        om = dc.omega_for(c.m, kmax)
        dev.reset_timing()
        dev.lowrank_detect(c.A[None], kmax, tol=dc.TOL, rank_rtol=dc.RANK_RTOL, omega=om)
        want = dc.restate(c.A, om, kmax)["sweeps"]
        got = dev.count("detect_sweeps_max")
        assert 1 <= got <= want + 2, (name, got, want)
        assert dev.count("detect_calls") == 1 and dev.count("detect_accepted") + dev.count("detect_rejected") == 1


# ---------------------------------------------------------------------------------------------- end to end
def _planted(m=40, n=30, seed=11, full=1, rank40=False):
    """Planted strictly feasible SDP given as matrices: dense constraints of rank 1 / 2 / 9, a trace row at index 5 and `full`
    dense full-rank constraints at the indices 6 .. 5 + full; rank40: one more constraint, of rank 40 = m, appended."""
    rng = np.random.default_rng(seed)
    As = []
    special = {5: "trace"}
    for j in range(full):
        special[6 + j] = "full"
    for k in range(n):
        if special.get(k) == "trace":
            As.append(np.eye(m))
        elif special.get(k) == "full":
            R = rng.standard_normal((m, m))
            As.append(0.5 * (R + R.T) / (2.0 * np.sqrt(m)))
        else:
            r = (1, 2, 9)[k % 3]
            V = rng.standard_normal((m, r)) / np.sqrt(m)
            As.append((V * rng.choice([-1.0, 1.0], size=r)) @ V.T)
    if rank40:
        V = rng.standard_normal((m, m)) / np.sqrt(m)
        As.append((V * rng.choice([-1.0, 1.0], size=m)) @ V.T)
    As = [0.5 * (a + a.T) for a in As]
    Q = rng.standard_normal((m, m))
    X0 = np.eye(m) + Q @ Q.T / m
    y0 = rng.standard_normal(len(As)) / np.sqrt(len(As))
    b = -np.array([np.sum(a * X0) for a in As])
    C = np.eye(m) - sum(y * a for y, a in zip(y0, As))
    return [sp.csc_matrix(-C)] + [sp.csc_matrix(a) for a in As], b


def _opt(**attrs):
    from loraine_jl_amd.optimizer import Optimizer
    o = Optimizer()
    o.set_silent(True)
    o.set_attribute("kit", 0)
    for k, v in attrs.items():
        o.set_attribute(k, v)
    return o


def _copy(A):
    return [[x.copy() for x in A]]


def test_planted_solve_hybrid_after_detection():
    A, b = _planted()
    om = _opt()
    om.load_model(_copy(A), b)
    om.optimize()
    od = _opt()
    od.load_detected_model(_copy(A), b, host_side=0)                         # (side 40: the host's eigh would take them all)
    od.optimize()
    s, rep = od.solver, od.detect_report
    assert rep["route"] == "factored" and rep["counters"]["detect_accepted"] == 28 and rep["counters"]["detect_rejected"] == 2
    assert s.model.factored and sorted(s.model.stored[0]) == [5, 6] and s.lowrank and s.datarank == 9
    assert sorted(a.nnz for a in s.model.stored[0].values()) == [40, 1600]   # the trace row and one stored dense row
    assert s.dev.count("op_factored") > 0
    assert "28 constraints as factors" in s.model.lowrank_note
    assert od.termination_status() == om.termination_status() == "OPTIMAL"
    assert od.objective_value() == pytest.approx(om.objective_value(), rel=1e-8)
    assert od.dual_objective_value() == pytest.approx(om.dual_objective_value(), rel=1e-6)
    # the host route (the default for a side of 40) finds the same factors' ranks and leads to the same optimum
    oh = _opt()
    oh.load_detected_model(_copy(A), b)
    oh.optimize()
    assert oh.detect_report["blocks"][0]["host_accepted"] == 28 and oh.detect_report["counters"]["detect_calls"] == 0
    assert oh.objective_value() == pytest.approx(om.objective_value(), rel=1e-8)


def test_planted_solve_wide_after_detection():
    A, b = _planted(rank40=True)
    om = _opt()
    om.load_model(_copy(A), b)
    om.optimize()
    od = _opt()
    od.load_detected_model(_copy(A), b, kmax=64, host_side=0)
    od.optimize()
    s = od.solver
    assert s.model.factored and s.model.wide and s.datarank == 40
    assert od.detect_report["blocks"][0]["ranks"][40] >= 1
    assert od.termination_status() == om.termination_status() == "OPTIMAL"
    assert od.objective_value() == pytest.approx(om.objective_value(), rel=1e-8)
    assert od.dual_objective_value() == pytest.approx(om.dual_objective_value(), rel=1e-6)


def test_seventeen_dense_rows_fall_back_to_the_general_path_bit_for_bit():
    A, b = _planted(full=17)
    om = _opt()
    om.load_model(_copy(A), b)
    om.optimize()
    od = _opt()
    od.load_detected_model(_copy(A), b, host_side=0)
    od.optimize()
    rep = od.detect_report
    assert rep["route"] == "general" and "max_stored = 16" in rep["reason"] and "18 stored" in rep["reason"]
    assert not getattr(od.solver.model, "factored", False)
    assert "general path" in od.solver.model.lowrank_note and "max_stored = 16" in od.solver.model.lowrank_note
    assert od.solver.iter == om.solver.iter
    assert np.array_equal(od.variable_primal(), om.variable_primal())
    assert od.objective_value() == om.objective_value() and od.dual_objective_value() == om.dual_objective_value()
    # 16 kept dense rows (15 full + the trace row) stay below the edge
    A16, b16 = _planted(full=15)
    o16 = _opt()
    o16.load_detected_model(_copy(A16), b16, host_side=0)
    o16._copy_to()
    assert o16.detect_report["route"] == "factored" and len(o16.solver.model.stored[0]) == 16


def test_kit_1_needs_cg_and_solves_with_it():
    A, b = _planted()
    bad = _opt(kit=1)
    bad.load_detected_model(_copy(A), b, host_side=0)
    with pytest.raises(ValueError, match=r"a factored model \(load_factored_model\) needs kit = 0: the CG path reads the constraint "
                                         "matrices, which do not exist"):
        bad.optimize()
    om = _opt()
    om.load_model(_copy(A), b)
    om.optimize()
    oc = _opt(kit=1)
    oc.load_detected_model(_copy(A), b, cg=True, host_side=0)
    oc.optimize()
    assert oc.solver.model.factored and oc.termination_status() == "OPTIMAL"
    # both solves stop on DIMACS errors below eDIMACS = 1e-7, the relative gap among them: each objective is within a few
    # 1e-7 (1 + |optimum|) of the optimum (the bound of tests/test_gpu_cg_factored.py against a planted optimum)
    assert abs(oc.objective_value() - om.objective_value()) <= 1e-6 * (1 + abs(om.objective_value()))
