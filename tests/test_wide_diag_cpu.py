"""CPU: diagonal parts on wide factored blocks (load_factored_model(..., wide="diag"), library option wide_diag) without a GPU --
the input conditions of the cases of tests/wide_diag_cases.py, a NumPy float64 restatement of the device formulas with C = Ad' (Y o Y)
summed in the order of the wide epilogue of csrc/diagops.hip (blocks of 16 by balanced trees, accumulator 0 + 1, wave 0 + 1; padded
and per class through the group map) against H_ij = tr(A_i W A_j W) from the materialised constraints in np.longdouble, single
faults planted in that restatement, and the host interface.

Bounds.  The restatement stays below 1e-12 relative Frobenius, the bound of tests/test_gpu_diag_factored.py and
tests/test_gpu_wide.py for the same quantity (observed 1.4e-16 .. 2.9e-16 on these cases, cond(W) 4e2 .. 5e3).  Every single fault
must miss 1e-12 by at least 1e3 (observed 2.2e-2 .. 8.9e-1): a GPU test at 1e-12 on these cases sees each."""
import dataclasses

import numpy as np
import pytest
import scipy.sparse as sp

import ragged_cases as rc
import wide_cases as wc
import wide_diag_cases as wd
from loraine_jl_amd.model import build_factored_model
from oracle import cg_reference as cr

TOL = 1e-12


# ---------------------------------------------------------------------------------------------- input conditions
@pytest.mark.parametrize("name", wd.NAMES)
def test_the_reference_is_well_conditioned(name):
    """H of every case is symmetric positive definite, and cond(W) lies in the range of the cases on which the bound 1e-12 was set
    (tests/wide_cases.py, tests/diag_factored_cases.py: ragged_cases.spd scalings below 1e4).  H is assembled, never inverted, in
    these tests: cond(H) is printed, not bounded."""
    H = np.asarray(wd.reference(name), dtype=np.float64)
    lam = np.linalg.eigvalsh(H)
    cw = max(np.linalg.cond(W) for W, _ in wd.scaling(name))
    print("WDIAG cpu input %s | eig(H) %.2e .. %.2e cond %.1e | cond(W) %.1e" % (name, lam[0], lam[-1], lam[-1] / lam[0], cw))
    assert np.array_equal(H, H.T)
    assert lam[0] > 0
    assert cw < 1e4


def test_the_cases_reach_the_edges_they_name():
    from loraine_jl_amd.model import ragged_plan
    fm = wd.model("D32")
    assert fm.lowrank[0][2] == 32 and sorted(fm.diag[0]) == list(range(5)) and fm.n * 32 == 160
    fm = wd.model("D64")
    assert fm.lowrank[0][2] == 64 and sorted(fm.diag[0]) == sorted(wd.D64_DIAG + (wd.D64_TRACE,))
    p = ragged_plan(rc.block_ranks(fm, 0), max_rank=64)
    assert p["seg"][64] == (0, 192) and p["seg"][32] == (192, 288)      # three groups each: a half-full tile of class 32
    assert rc.block_ranks(fm, 0)[wd.D64_TRACE] == 0
    for cnt in (63, 64, 65):
        fm = wd.model("DE%d" % cnt)
        assert fm.lowrank[0][2] == 32 and sorted(fm.diag[0]) == list(range(cnt))
        assert max(rc.block_ranks(fm, 0)) == 32 and min(rc.block_ranks(fm, 0)) == 0
    fm = wd.model("DH")
    assert fm.lowrank[0][2] == 64 and sorted(fm.stored[0]) == [wc.V3_TRACE, wc.V3_DENSE] and fm.nlin == 2
    assert sorted(fm.diag[0]) == sorted(wd.DH_DIAG + (wd.DH_TRACE,))
    fm = wd.model("D2B")
    assert [lr[2] for lr in fm.lowrank] == [32, 2] and sorted(fm.diag[1]) == list(wd.D2B_NARROW_DIAG)


@pytest.mark.parametrize("name", wd.CG_NAMES)
def test_the_pcg_reference_is_stable_under_a_perturbation_of_the_size_of_the_bound(name):
    """The condition tests/cg_diag_cases.py states for its seeds: the longdouble run has a gap of 1.5 at K and a float64 drift below
    cr.DRIFT_MAX (cr.reference_run asserts both) -- and, directly, H perturbed entrywise by 1e-9 relative (far above the 1e-12 of
    the assembled H, the size of the apply's bound) leaves the exits (30, K) and (-2, K - 1) where they are."""
    case, H = wd.cg_data(name)
    lam = np.linalg.eigvalsh(np.asarray(H, dtype=np.float64))
    assert lam[0] > 0
    run = wd.cg_run(name)
    K, tol = run.K, run.tol
    rho = run.hist.rho
    print("WDIAG cpu pcg %s | cond(H) %.1e | K %d tol %.3e | rho[K-1] %.3e rho[K] %.3e | drift %.1e %.1e"
          % (name, lam[-1] / lam[0], K, tol, rho[K - 1], rho[K], run.drift[K - 1], run.drift[K]))
    assert rho[K - 1] / rho[K] >= cr.GAP and max(run.drift[K - 1], run.drift[K]) <= cr.DRIFT_MAX
    rng = np.random.default_rng(5)
    E = rng.uniform(-1.0, 1.0, H.shape)
    Hp = H * (1 + cr.LD(1e-9) * ((E + E.T) / 2))
    for maxit, want in ((10000, (30, K)), (K - 1, (-2, K - 1))):
        for Hx in (H, Hp):
            h = cr.pcg_history(Hx, run.solve, case.h, tol, maxit)
            assert (h.code, h.it) == want


# ---------------------------------------------------------------------------------------------- the device formulas in NumPy
@pytest.mark.parametrize("layout", ["padded", "class"])
@pytest.mark.parametrize("name", wd.NAMES)
def test_the_device_formulas_in_the_epilogue_order_match_the_reference(name, layout):
    H = wd.h_device_order(name, layout)
    err = rc.relerr(H, wd.reference(name))
    print("WDIAG cpu %s %s | %.2e" % (name, layout, err))
    assert np.array_equal(H, H.T) or rc.relerr(H, H.T) < 1e-15
    assert err < TOL


def test_group_sums_are_the_plain_sums():
    S = np.random.default_rng(4).standard_normal((7, 64)) ** 2
    for cs in wc.WIDE_CLASSES:
        got = wd._group_sum(S[:, :cs])
        assert got.shape == (7,) and np.allclose(got, S[:, :cs].sum(axis=1), rtol=1e-14, atol=0.0), cs
    # a group of 32: ((tree of 16) + (tree of 16)); of 64: two of those
    x = S[:1]
    t = lambda a: wc._tree(a, 1)
    assert wd._group_sum(x[:, :32])[0] == (t(x[:, :16]) + t(x[:, 16:32]))[0]
    assert wd._group_sum(x)[0] == ((t(x[:, :16]) + t(x[:, 16:32])) + (t(x[:, 32:48]) + t(x[:, 48:])))[0]


FAULTS = [("acc", "D32", "padded"), ("acc", "D64", "class"), ("acc", "DE64", "padded"), ("wave", "D64", "padded"),
          ("wave", "D64", "class"), ("wave", "DH", "class"), ("pad", "D64", "padded"), ("pad", "D64", "class"),
          ("pad", "DH", "padded"), ("half", "D32", "padded"), ("hmap", "D64", "class"), ("hmap", "DE65", "class")]


@pytest.mark.parametrize("fault,name,layout", FAULTS)
def test_a_single_fault_breaks_the_bound(fault, name, layout):
    """acc: the second accumulator of a group of 32 dropped; wave: the second wave of a group of 64; pad: a padding column with
    weight 1 and a non-zero operand; half: the missing group of a half-full tile written (at kh 32 without a map its address is
    the first column of the next row); hmap: the group map of class 32 shifted by one group.  Each must miss 1e-12 by at least 1e3."""
    H = wd.h_device_order(name, layout, fault=fault)
    err = rc.relerr(H, wd.reference(name))
    print("WDIAG cpu fault %s on %s %s | %.2e" % (fault, name, layout, err))
    assert err >= 1e3 * TOL


# ---------------------------------------------------------------------------------------------- host interface
def _fac(m, r, seed=0):
    return rc._dense_factor(np.random.default_rng(seed), m, r)


def test_build_factored_model_with_wide_diag():
    m = 40
    V, d = _fac(m, 20)
    psi = np.abs(np.random.default_rng(1).standard_normal(m)) + 0.1
    trace = (None, [], np.ones(m))
    blk = [[(V, d, psi), trace, _fac(m, 3, 2)]]
    fm = build_factored_model([-np.eye(m)], blk, np.zeros(3), factored_form=1, max_rank=64, wide_diag=True)
    assert fm.wide and fm.wide_diag and fm.factored and fm.lowrank[0][2] == 32
    assert sorted(fm.diag[0]) == [0, 1] and np.array_equal(fm.diag[0][0], psi) and np.array_equal(fm.diag[0][1], np.ones(m))
    assert rc.block_ranks(fm, 0) == [20, 0, 3]
    assert [f.name for f in dataclasses.fields(fm)][-1] == "ragged"      # (`wide_diag` is read off lowrank and diag: no new field)
    # the default: the refusal, text unchanged
    with pytest.raises(ValueError, match=r"constraint 1 has 20 factor columns .* constraint 1 a diagonal part .* sparse matrix"):
        build_factored_model([-np.eye(m)], blk, np.zeros(3), factored_form=1, max_rank=64)
    with pytest.raises(ValueError, match="wide_diag = True needs max_rank = 64"):
        build_factored_model([-np.eye(m)], blk, np.zeros(3), factored_form=1, wide_diag=True)
    with pytest.raises(ValueError, match="wide_diag is False or True"):
        build_factored_model([-np.eye(m)], blk, np.zeros(3), factored_form=1, max_rank=64, wide_diag="yes")
    # wide without diagonal parts, diagonal parts without wide ranks, and the two in different blocks: not wide_diag
    a = build_factored_model([-np.eye(m)], [[(V, d), _fac(m, 3, 2)]], np.zeros(2), factored_form=1, max_rank=64, wide_diag=True)
    b = build_factored_model([-np.eye(m)], [[_fac(m, 16), trace]], np.zeros(2), factored_form=1, max_rank=64, wide_diag=True)
    c = build_factored_model([-np.eye(m), -np.eye(m)], [[(V, d), _fac(m, 3, 2)], [_fac(m, 16), trace]], np.zeros(2),
                             factored_form=1, max_rank=64, wide_diag=True)
    assert a.wide and not a.wide_diag and not b.wide and not b.wide_diag and c.wide and not c.wide_diag
    for name in wd.NAMES:
        assert wd.model(name).wide_diag
    for name in wc.NAMES:
        assert not wc.model(name).wide_diag


class _Stop(RuntimeError):
    pass


class _RecordingDevice:
    """Stands where the device would: records options and uploads in their order; stop_at = "set_factored" ends the run there (the
    device of tests/test_wide_cpu.py), "upload_diag" after the first upload of diagonal parts, "end" after the last option."""

    def __init__(self, stop_at):
        self.log, self.stop_at = [], stop_at

    def set_option(self, key, value):
        self.log.append((key, value))
        if self.stop_at == "end" and key == "ragged_ts":
            raise _Stop()

    def upload_lowrank(self, i, khat, V, d):
        self.log.append(("upload_lowrank", khat))

    def set_factored(self, i):
        if self.stop_at == "set_factored":
            raise _Stop()
        self.log.append(("set_factored", i))

    def upload_diag(self, i, rows, a):
        self.log.append(("upload_diag", list(rows)))
        if self.stop_at == "upload_diag":
            raise _Stop()

    def __getattr__(self, name):
        if name == "upload_model":
            return lambda *a, **k: None
        raise AttributeError(name)


def _run(P, factors, stop_at, attrs=None, **kw):
    from loraine_jl_amd.optimizer import Optimizer
    dev = _RecordingDevice(stop_at)
    o = Optimizer(device=dev)
    o.set_silent(True)
    for k, v in (attrs or {}).items():
        o.set_attribute(k, v)
    o.load_factored_model(P.F0(), factors, P.b, max_sense=True, factored_form=1, **kw)
    with pytest.raises(_Stop):
        o.optimize()
    return dev.log, o


def test_host_opt_in_order_of_options_and_uploads():
    P = wd.PlantedWideDiag()
    log, o = _run(P, P.factors(), "upload_diag", wide="diag")
    assert log == [("lowrank_wide", 1), ("upload_lowrank", 64), ("set_factored", 0), ("wide_diag", 1), ("upload_diag", [0])]
    # up to the first set_factored: the sequence tests/test_wide_cpu.py::test_host_opt_in pins
    log, _ = _run(P, P.factors(), "set_factored", wide="diag")
    assert log == [("lowrank_wide", 1), ("upload_lowrank", 64)]
    # wide=True (the trace row stored): wide_diag = 0, so that a device another solve used is reset
    log, o = _run(P, P.stored_trace_factors(), "end", wide=True)
    assert log[:4] == [("lowrank_wide", 1), ("upload_lowrank", 64), ("set_factored", 0), ("wide_diag", 0)]
    assert not any(k == "upload_diag" for k, _ in log)
    # a narrow model: 0 as well
    R = rc.Planted()
    log, _ = _run(R, R.factors(), "end")
    assert log[:4] == [("lowrank_wide", 0), ("upload_lowrank", 8), ("set_factored", 0), ("wide_diag", 0)]
    # combines with ragged= and cg= as wide=True does
    log, o = _run(P, P.factors(), "end", attrs=dict(kit=1), wide="diag", ragged="all", cg="diag")
    assert log[:5] == [("lowrank_wide", 1), ("upload_lowrank", 64), ("set_factored", 0), ("wide_diag", 1), ("upload_diag", [0])]
    assert dict(log[5:]) == dict(cg_factored=1, cg_diag=1, lowrank_ragged=1, ragged_ops=1, ragged_cross=1, ragged_ts=1)
    assert o._pending[1][-1] is True


def test_wide_true_still_refuses_a_diagonal_part():
    from loraine_jl_amd.optimizer import Optimizer
    P = wd.PlantedWideDiag()
    o = Optimizer(device=_RecordingDevice("end"))
    o.set_silent(True)
    o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True, factored_form=1, wide=True)
    with pytest.raises(ValueError, match="carries no diagonal part -- store that row as a sparse matrix instead"):
        o.optimize()


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 64, "Diag", "all"])
def test_bad_values_of_wide(bad):
    from loraine_jl_amd.optimizer import Optimizer
    P = rc.Planted()
    with pytest.raises(ValueError, match="wide is False or True"):
        Optimizer(device=_RecordingDevice("end")).load_factored_model(P.F0(), P.factors(), P.b, wide=bad)


@pytest.mark.parametrize("cg", [False, True])
def test_kit_1_needs_cg_diag(cg):
    from loraine_jl_amd.optimizer import Optimizer
    P = wd.PlantedWideDiag()
    o = Optimizer(device=_RecordingDevice("end"))
    o.set_silent(True)
    o.set_attribute("kit", 1)
    o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True, factored_form=1, wide="diag", cg=cg)
    with pytest.raises(ValueError, match="needs kit = 0"):
        o.optimize()


def test_the_header_and_the_bindings_name_the_option():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert '"wide_diag"' in open(os.path.join(root, "include", "loraine_hip.h")).read()
    assert '"wide_diag"' in open(os.path.join(root, "julia", "LoraineHIP.jl")).read()
    # (no new C function: tests/test_bindings_match_header_cpu.py compares the declarations and stays as it is)
    assert "wide_diag" not in open(os.path.join(root, "loraine.jl_amd", "_capi.py")).read()
