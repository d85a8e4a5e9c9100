"""The inputs of the low-rank detection are clear cases, its NumPy restatement agrees with model.lowrank_factor on all of
them, single planted faults show, and the pure host side (detect.plan, the fallback rule, the argument checks of
load_detected_model) does what it says -- all without a device.  The cases and the restatement: tests/detect_cases.py."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_cases as dc  # noqa: E402
from loraine_jl_amd import detect  # noqa: E402
from loraine_jl_amd import model as lm  # noqa: E402
from loraine_jl_amd.optimizer import Optimizer  # noqa: E402

KMAXES = (16, 64)
_RESTATED = {}


def restated(name, kmax):
    """The restatement of one case, computed once and shared."""
    if (name, kmax) not in _RESTATED:
        c = dc.CASES[name]
        _RESTATED[name, kmax] = dc.restate(c.A, dc.omega_for(c.m, kmax), kmax)
    return _RESTATED[name, kmax]


def test_the_constants_are_the_models():
    assert dc.TOL == lm.LOWRANK_TOL and dc.RANK_RTOL == detect.RANK_RTOL
    assert np.array_equal(dc.omega_for(37, 16, 3), detect.sketch_matrix(37, 16, 3))


def test_the_case_list_is_covered():
    sides = {c.m for c in dc.CASES.values()}
    assert {1, 5, 23, 24, 25, 37, 63, 64, 65, 129, 200, 71, 72, 73} <= sides
    assert {dc.CASES[n].m for n in dc.cases_for(64)} >= {5, 71, 72, 73, 200}
    ranks = {c.rank for c in dc.CASES.values() if c.m == 200}
    assert {0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65} <= ranks
    assert dc.CASES["identity129"].rank == 129 and dc.CASES["spd65"].rank == 65
    inert = [c.inertia for c in dc.CASES.values() if c.rank]
    assert any(q == 0 for _, q in inert) and any(p == 0 for p, _ in inert) and any(p and q for p, q in inert)
    g = np.abs(dc.CASES["graded_r12"].lam)
    assert g.max() / g.min() == pytest.approx(1e6)
    assert np.linalg.norm(dc.CASES["scaled_1e3_r4"].A) > 1e3 and np.linalg.norm(dc.CASES["scaled_1e-3_r4"].A) < 3e-3
    assert np.count_nonzero(np.any(dc.CASES["support3_r2"].A != 0, axis=1)) == 3
    assert len(dc.batch70()) == 70 and len(set(dc.batch70())) >= 12
    for m in (65, 200):                                      # batches of 1 (every case alone), 3 and 70
        b3 = dc.batch3(m)
        assert len(b3) == len(set(b3)) == 3 and dc.batch(b3).shape == (3, m, m)
        assert {dc.CASES[n].accepted(16) for n in b3} == {True, False}          # mixed verdicts in one batch
    for c in dc.CASES.values():
        assert np.array_equal(c.A, c.A.T)
        assert np.linalg.matrix_rank(c.A, tol=1e-9 * max(1.0, np.abs(c.lam).max(initial=0.0))) == c.rank


@pytest.mark.parametrize("kmax", KMAXES)
def test_clear_cases_only(kmax):
    """Accepted: the restatement's residual is <= 1e-3 tol.  Rejected: the best rank-kmax error, by eigh, is >= 1e3 tol.
    Nothing in between, where the verdict may turn on rounding."""
    for name in dc.cases_for(kmax):
        c = dc.CASES[name]
        if c.accepted(kmax):
            out = restated(name, kmax)
            assert out["rank"] == c.rank, name
            assert out["resid"] <= 1e-3 * dc.TOL, (name, out["resid"])
            d = out["d"][:c.rank]
            assert (int(np.sum(d > 0)), int(np.sum(d < 0))) == c.inertia, name
            assert not out["V"][:, c.rank:].any() and not out["d"][c.rank:].any()
        else:
            lam = np.sort(np.abs(np.linalg.eigvalsh(c.A)))[::-1]
            best = float(np.linalg.norm(lam[kmax:]))
            assert best >= 1e3 * dc.TOL, (name, best)
            assert best == pytest.approx(c.beyond(kmax), rel=1e-9)
            assert restated(name, kmax)["rank"] == -1, name


@pytest.mark.parametrize("kmax", KMAXES)
def test_restatement_agrees_with_lowrank_factor(kmax):
    for name in dc.cases_for(kmax):
        c = dc.CASES[name]
        f = lm.lowrank_factor(sp.csc_matrix(c.A), c.m, kmax)
        got = restated(name, kmax)["rank"]
        assert got == (-1 if f is None else f[0].shape[1]), name


def test_sweeps_stay_far_below_the_limit():
    assert max(restated(n, k)["sweeps"] for k in KMAXES for n in dc.cases_for(k)) <= dc.MAX_SWEEPS // 2


def test_round_robin_meets_every_pair_once():
    for l in (24, 72):
        seen = set()
        for s in range(l - 1):
            pairs = dc.round_robin(l, s)
            assert len({i for p in pairs for i in p}) == l          # disjoint
            seen |= set(pairs)
        assert len(seen) == l * (l - 1) // 2


# ---------------------------------------------------------------------------------------------- planted faults
FAULT_CASES = {
    "sign": [("m200_rank2", 16), ("graded_r12", 16), ("m73_r40", 64)],
    "inverse": [("m200_rank2", 16), ("scaled_1e3_r4", 16), ("m73_r40", 64)],
    "unsym": [("m200_rank2", 16), ("graded_r12", 16), ("graded_r16", 16), ("scaled_1e3_r4", 16), ("m73_r40", 64)],
    "skip": [("m200_rank1", 16), ("graded_r12", 16), ("m200_rank64", 64)],
    "once": [("m200_rank17", 16), ("identity129", 16), ("m200_rank65", 64)],
    "cut": [("m200_rank2", 16), ("m200_rank16", 16), ("m72_r40", 64)],
}


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_planted_fault_shows(fault):
    """One fault in the restatement -- a wrong sign in d, |Lambda|^-1 for |Lambda|^-1/2, an unsymmetrised C (the triangle the
    core step forms, never mirrored), one pair never rotated, off-diagonal tiles counted once, the rank cut on lambda instead
    of |lambda| -- flips a verdict, or moves the reported residual off an independent evaluation of ||A - V D V'||_F by 1e3
    times the bound the clean run keeps."""
    shown = False
    for name, kmax in FAULT_CASES[fault]:
        c = dc.CASES[name]
        clean = restated(name, kmax)
        bad = dc.restate(c.A, dc.omega_for(c.m, kmax), kmax, fault=fault)
        flips = bad["rank"] != clean["rank"]
        # the residual bound of the clean run: reported = independent evaluation to 1e-12 relative (+ 1e-3 tol absolute)
        ind = float(np.linalg.norm(c.A - (bad["V"] * bad["d"]) @ bad["V"].T))
        bound = 1e-12 * ind + 1e-3 * dc.TOL
        breaks = abs(bad["resid"] - ind) > 1e3 * bound or (clean["rank"] >= 0 and bad["resid"] > 1e3 * 1e-3 * dc.TOL)
        ind0 = float(np.linalg.norm(c.A - (clean["V"] * clean["d"]) @ clean["V"].T))
        assert abs(clean["resid"] - ind0) <= 1e-12 * ind0 + 1e-3 * dc.TOL, name
        shown = shown or flips or breaks
    assert shown, fault


# ---------------------------------------------------------------------------------------------- detect.plan
def _blocks(m, nnz, support):
    return [(m, nnz, support)]


def test_plan_routes_by_nnz_and_support():
    nnz = [0, 8, 9, 400, 96 * 96, 97 * 97, 40000]
    sup = [0, 3, 3, 20, 96, 97, 200]
    p = detect.plan(_blocks(200, nnz, sup), 16, 10 * 200 * 200 * 8)
    assert p["stored"] == [[0, 1]]                  # nnz <= datasparsity: no look
    assert p["host"] == [[2, 3, 4]]                 # support side <= 96
    assert p["device"] == [[5, 6]]
    assert p["chunks"] == [(0, [5, 6])]
    p = detect.plan(_blocks(200, nnz, sup), 16, 10 * 200 * 200 * 8, datasparsity=9, host_side=0)
    assert p["stored"] == [[0, 1, 2]] and p["host"] == [[]] and p["device"] == [[3, 4, 5, 6]]
    assert sorted(p["stored"][0] + p["host"][0] + p["device"][0]) == list(range(7))


def test_plan_chunks_one_many_ragged():
    m, n = 200, 70
    one = m * m * 8
    blocks = [(m, [m * m] * n, [m] * n), (100, [10000] * 5, [100] * 5)]
    p = detect.plan(blocks, 64, 70 * one)
    assert p["chunks"] == [(0, list(range(70))), (1, list(range(5)))]
    p = detect.plan(blocks, 64, 35 * one)
    assert [len(ks) for i, ks in p["chunks"] if i == 0] == [35, 35]
    p = detect.plan(blocks, 64, 10 * one + one - 1)
    assert [len(ks) for i, ks in p["chunks"] if i == 0] == [10] * 7
    p = detect.plan(blocks, 64, 16 * one)
    sizes = [len(ks) for i, ks in p["chunks"] if i == 0]
    assert sizes == [16, 16, 16, 16, 6]             # a ragged last chunk
    assert sum((ks for i, ks in p["chunks"] if i == 0), []) == list(range(70))
    for i, ks in p["chunks"]:
        assert len(ks) * blocks[i][0] ** 2 * 8 <= 16 * one
    assert all(i in (0, 1) for i, _ in p["chunks"]) and [ks for i, ks in p["chunks"] if i == 1] == [[0, 1, 2, 3, 4]]
    with pytest.raises(ValueError, match="budget"):
        detect.plan(blocks, 64, one - 1)
    with pytest.raises(ValueError, match="kmax"):
        detect.plan(blocks, 32, one)


def test_fallback_rule_and_max_stored_at_its_edge():
    assert detect.fallback_reason(0, [[]]) == "no constraint has a factor of rank <= kmax"
    assert detect.fallback_reason(5, [[1600] * 16 + [3, 8]]) == ""             # 16 kept -> hybrid
    why = detect.fallback_reason(5, [[4], [1600] * 17])                          # 17 -> general path
    assert "block 2" in why and "17 stored" in why and "max_stored = 16" in why
    assert detect.fallback_reason(5, [[1600] * 17], max_stored=17) == ""
    assert detect.fallback_reason(5, [[9] * 3], max_stored=2, datasparsity=9) == ""
    assert detect.fallback_reason(5, [[10] * 3], max_stored=2, datasparsity=9) != ""


# ---------------------------------------------------------------------------------------------- load_detected_model
def _tiny():
    A = [[sp.identity(3, format="csc")] + [sp.csc_matrix(np.ones((3, 3)))] * 2]
    return A, np.ones(2)


def test_load_detected_model_argument_checks():
    A, b = _tiny()
    with pytest.raises(ValueError, match="needs the resident solver"):
        Optimizer(device=object(), resident=False).load_detected_model(A, b)
    opt = Optimizer(device=object())
    for kmax in (0, 8, 32, True, "16"):
        with pytest.raises(ValueError, match="kmax is 16 or 64"):
            opt.load_detected_model(A, b, kmax=kmax)
    for ms in (-1, 2.5, True, None):
        with pytest.raises(ValueError, match="max_stored is a count"):
            opt.load_detected_model(A, b, max_stored=ms)
    with pytest.raises(ValueError, match=r'cg is False, True or "diag"'):
        opt.load_detected_model(A, b, cg="yes")
    with pytest.raises(ValueError, match=r'ragged is False, True, "ops" or "all"'):
        opt.load_detected_model(A, b, ragged="some")
    with pytest.raises(ValueError, match="factored_form = 0"):
        opt.load_detected_model(A, b, factored_form=0)
    with pytest.raises(ValueError, match="budget_mb"):
        opt.load_detected_model(A, b, budget_mb=0)
    for hs in ("96", 2.5, True, [0]):
        with pytest.raises(ValueError, match="host_side is a whole number"):
            opt.load_detected_model(A, b, host_side=hs)
    with pytest.raises(ValueError, match="seed is a whole number"):
        opt.load_detected_model(A, b, seed="x")
    assert opt.load_detected_model(A, b, kmax=64, max_stored=0, cg="diag", ragged="all") is opt
    assert opt._pending[0] == "detected" and opt._pending[1][1]["kmax"] == 64
    with pytest.raises(ValueError, match="detect_kmax is None, 16 or 64"):
        opt.read_from_file("x.dat-s", detect_kmax=8)
    assert opt.read_from_file("x.dat-s")._pending == ("sdpa", "x.dat-s")
    assert opt.read_from_file("x.dat-s", detect_kmax=64)._pending[0] == "sdpa_detected"


class _FakeDevice:
    """Stands in for the device in detect_factors: answers with the restatement."""

    def __init__(self):
        self.calls = []

    def lowrank_detect(self, mats, kmax, tol=None, rank_rtol=1e-12, omega=None):
        self.calls.append(len(mats))
        outs = [dc.restate(a, omega, kmax, tol, rank_rtol) for a in mats]
        return (np.array([o["rank"] for o in outs], dtype=np.int32), np.array([o["resid"] for o in outs]),
                np.stack([o["V"] for o in outs]), np.stack([o["d"] for o in outs]))

    def set_option(self, key, value):
        pass

    def count(self, key):
        return 0


def test_detected_model_routes_without_a_device():
    """Optimizer._detected_model with the restatement standing in for the device: the factored route, both fallbacks and
    their notes, the kit check with the text load_factored_model gives, and the SDPA entry."""
    m, n = 30, 6
    rng = np.random.default_rng(2)
    low = []
    for k in range(n):
        V = rng.standard_normal((m, 1 + k % 2))
        low.append(sp.csc_matrix(V @ V.T))
    R = rng.standard_normal((m, m))
    full = sp.csc_matrix(R + R.T)
    F0 = sp.identity(m, format="csc")
    b = np.ones(n)

    def model_of(A, **kw):
        opt = Optimizer(device=_FakeDevice())
        for k, v in kw.pop("attrs", {}).items():
            opt.set_attribute(k, v)
        opt.load_detected_model(A, b, host_side=-1, **kw)
        _, (arrays, o) = opt._pending
        return opt, opt._detected_model(arrays, o, 0, 8)

    opt, mdl = model_of([[F0] + low[:5] + [full]])
    assert mdl.factored and sorted(mdl.stored[0]) == [5] and opt.detect_report["route"] == "factored"
    assert opt.detect_report["accepted"] == 5 and "5 constraints as factors" in mdl.lowrank_note
    assert not mdl.factored_cg and mdl.ragged is False
    opt, mdl = model_of([[F0] + [full] * n])
    assert not mdl.factored and opt.detect_report["route"] == "general"
    assert "no constraint has a factor" in mdl.lowrank_note and mdl.lowrank == []
    ref = lm.build_model([[F0] + [full] * n], b)
    assert all(abs(x - y).nnz == 0 for x, y in zip(mdl.AA, ref.AA)) and np.array_equal(mdl.sigmaA, ref.sigmaA)
    opt, mdl = model_of([[F0] + low[:4] + [full] * 2], max_stored=1)
    assert not mdl.factored and "max_stored = 1" in mdl.lowrank_note and "2 stored" in opt.detect_report["reason"]
    opt, mdl = model_of([[F0] + low[:4] + [full] * 2], max_stored=2, cg=True, ragged="ops", attrs=dict(kit=1))
    assert mdl.factored and mdl.factored_cg and mdl.ragged == "ops"
    with pytest.raises(ValueError, match=r"a factored model \(load_factored_model\) needs kit = 0"):
        model_of([[F0] + low[:5] + [full]], attrs=dict(kit=1))
    # an SDPA file whose constraints are all sparse: nothing to detect, the general path
    opt = Optimizer(device=_FakeDevice())
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "theta1.dat-s")
    opt.read_from_file(path, detect_kmax=16)
    kind, (p, o) = opt._pending
    general = lm.model_from_sdpa(p)
    mdl = opt._detected_model((general.A, general.b, general.b_const, general.d_lin, general.C_lin, False), o, 0, 8)
    assert not mdl.factored and opt.detect_report["route"] == "general" and opt.detect_report["chunks"] == 0


def test_detect_factors_items_and_report():
    m, n = 100, 6
    names = ["r1", "r2", "full", "sparse", "small", "r1b"]
    rng = np.random.default_rng(5)
    u = rng.standard_normal((m, 2))
    small = np.zeros((m, m))
    small[:4, :4] = np.outer(np.arange(1.0, 5.0), np.arange(1.0, 5.0))
    sparse = np.zeros((m, m))
    sparse[[1, 2, 2], [2, 1, 2]] = 1.0
    mats = [np.outer(u[:, 0], u[:, 0]), u @ np.diag([1.0, -1.0]) @ u.T, np.eye(m) + np.outer(u[:, 1], u[:, 1]), sparse,
            small, -np.outer(u[:, 1], u[:, 1])]
    A = [[sp.identity(m, format="csc")] + [sp.csc_matrix(a) for a in mats]]
    fake = _FakeDevice()
    items, rep = detect.detect_factors(A, n, 16, fake, budget_mb=2 * m * m * 8 / 2 ** 20)
    assert fake.calls == [2, 2]                                  # r1, r2 | full, r1b: two chunks of two
    rb = rep["blocks"][0]
    assert (rb["device_accepted"], rb["device_rejected"], rb["host_accepted"], rb["host_rejected"], rb["stored"]) == (3, 1, 1, 0, 1)
    assert rb["ranks"] == {1: 3, 2: 1} and 0 <= rb["max_accepted_resid"] <= 1e-3 * dc.TOL and rep["accepted"] == 4
    assert rep["kept_nnz"] == [[m * m, 3]] and rep["chunks"] == 2
    for k, name in enumerate(names):
        if name in ("full", "sparse"):
            assert sp.issparse(items[0][k]) and abs(items[0][k] - A[0][k + 1]).nnz == 0
        else:
            V, d = items[0][k]
            assert V.shape == (m, d.size) and np.linalg.norm(mats[k] - (V * d) @ V.T) <= dc.TOL
    assert detect.fallback_reason(rep["accepted"], rep["kept_nnz"]) == ""
    bad = [[A[0][0]] + [sp.csc_matrix(np.triu(mats[2]))] + A[0][2:]]
    with pytest.raises(ValueError, match="not symmetric"):
        detect.detect_factors(bad, n, 16, fake)
    mdl = lm.build_factored_model([A[0][0]], items, np.ones(n))
    assert mdl.factored and sorted(mdl.stored[0]) == [2, 3]
