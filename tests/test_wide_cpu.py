"""CPU: factored constraints of rank 17 .. 64 (load_factored_model(..., wide=True), library option lowrank_wide) without a GPU --
the wide plan of loraine_jl_amd.model.ragged_plan(max_rank=64) (csrc/ragged_plan.h is the same function) against the layouts
written out in tests/wide_cases.py, the host interface, and a NumPy float64 restatement of the rank-class route in the device's
summation order (16 x 16 accumulator blocks, then accumulator pairs, then wave pairs: wide_cases.device_order) against H_ij =
tr(A_i W A_j W) from the materialised constraints in np.longdouble.

Bounds.  The restatement stays below 1e-13 relative Frobenius: observed 0.9e-16 .. 1.8e-16 on these three rank lists with
ragged_cases.spd scalings (cond(W) 4e2 .. 5e3), so the GPU bound 1e-12 of tests/test_gpu_ragged.py has three orders of margin.
Every single fault planted in the restatement must miss 1e-12 by at least 1e3 -- a test at 1e-12 on these cases sees each
(observed 7e-3 .. 6e-1)."""
import dataclasses

import numpy as np
import pytest
import scipy.sparse as sp

import ragged_cases as rc
import wide_cases as wc
from loraine_jl_amd.model import (RAGGED_CLASSES, RAGGED_CLASSES_WIDE, build_factored_model, ragged_columns, ragged_plan)

# ---------------------------------------------------------------------------------------------- plan layout
EXPECT = {
    # name: (segments by class 64, 32, 16, 8, 4, 2, 1, classes present, tiles, gh)
    "V1": ([(0, 0), (0, 160), (160, 160), (160, 160), (160, 160), (160, 160), (160, 160)], 1, 6, [0, 1, 2, 3, 4]),
    "V2": ([(0, 192), (192, 288), (288, 320), (320, 336), (336, 344), (344, 346), (346, 348)], 7,
           6 + 3 * (2 + 5) + 3 + 2 * 5 + 15, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14]),
    "V3": ([(0, 64), (64, 96), (96, 112), (112, 112), (112, 112), (112, 114), (114, 120)], 5, 15,
           [2, 3, 4, 5, 6, 7, 8, 9, 10, 11]),
}


def test_wide_classes_extend_the_narrow_ones():
    assert RAGGED_CLASSES == (16, 8, 4, 2, 1)
    assert RAGGED_CLASSES_WIDE == (64, 32) + RAGGED_CLASSES == wc.WIDE_CLASSES


@pytest.mark.parametrize("name", list(EXPECT))
def test_wide_plan_against_the_layouts_written_out(name):
    ranks = wc.RANKS[name]
    p = ragged_plan(ranks, max_rank=64)
    seg, ncls, ntiles, gh = EXPECT[name]
    assert [p["seg"][c] for c in RAGGED_CLASSES_WIDE] == seg
    assert p["Rc"] == seg[-1][1] and p["ncls"] == ncls and p["tiles"] == ntiles and p["gh"] == gh
    assert p["classes"] == [0 if r == 0 else min(c for c in RAGGED_CLASSES_WIDE if c >= r) for r in ranks]
    assert len(wc.tiles(p)) == ntiles
    fm = wc.model(name)                                      # the ranks the padded upload shows the library
    assert rc.block_ranks(fm, 0) == ranks
    cols = ragged_columns(ranks, max_rank=64)
    hg = [-1] * len(ranks)
    for g, h in enumerate(gh):
        hg[h] = g
    assert cols["gh"] == gh and cols["hg"] == hg and cols["Rc"] == p["Rc"]
    want_cg = [g for g, h in enumerate(gh) for _ in range(p["classes"][h])]
    assert cols["cg"] == want_cg and cols["size"] == [p["classes"][h] for h in gh]
    for g, h in enumerate(gh):                               # weighted columns first, in their order, then padding
        c0 = cols["start"][g]
        assert cols["wc"][c0:c0 + cols["size"][g]] == list(range(ranks[h])) + [-1] * (cols["size"][g] - ranks[h])


@pytest.mark.parametrize("name", list(EXPECT))
def test_every_pair_of_groups_has_exactly_one_tile_block(name):
    p = ragged_plan(wc.RANKS[name], max_rank=64)
    ng = len(p["gh"])
    seen = {}
    for r0, r1, c0, c1, gi0, gj0, ka, kb, diag in wc.tiles(p):
        assert 0 < r1 - r0 <= 64 and 0 < c1 - c0 <= 64 and (r1 - r0) % ka == 0 and (c1 - c0) % kb == 0 and ka >= kb
        for bi in range((r1 - r0) // ka):
            for bj in range((c1 - c0) // kb):
                gi, gj = gi0 + bi, gj0 + bj
                if diag and gi < gj:
                    continue
                key = (max(gi, gj), min(gi, gj))
                seen[key] = seen.get(key, 0) + 1
    assert len(seen) == ng * (ng + 1) // 2 and set(seen.values()) == {1}


@pytest.mark.parametrize("name", ["R1", "R2", "R3", "R4", "R6"])
def test_the_default_plan_is_unchanged(name):
    """Without the keyword: the five keys, and inside a wide plan of the same ranks the same columns, groups and tile count."""
    ranks = rc.ranks_of(name)
    p, pw = ragged_plan(ranks), ragged_plan(ranks, max_rank=64)
    assert list(p["seg"]) == list(RAGGED_CLASSES) and p == ragged_plan(ranks, 16)
    assert pw["seg"][64] == pw["seg"][32] == (0, 0)
    assert {c: pw["seg"][c] for c in RAGGED_CLASSES} == p["seg"]
    assert (pw["Rc"], pw["ncls"], pw["gh"], pw["tiles"], pw["classes"]) == (p["Rc"], p["ncls"], p["gh"], p["tiles"], p["classes"])
    assert wc.tiles(pw) == wc.tiles(p, RAGGED_CLASSES)
    assert ragged_columns(ranks) == ragged_columns(ranks, max_rank=64)


def test_rank_limits_of_the_plan():
    with pytest.raises(ValueError, match=r"ranks must lie in 0 \.\. 16"):
        ragged_plan([17])
    with pytest.raises(ValueError, match=r"ranks must lie in 0 \.\. 16"):
        ragged_columns([17])
    assert ragged_plan([17], max_rank=64)["seg"][32] == (0, 32)
    assert ragged_plan([64, 33], max_rank=64)["Rc"] == 128
    with pytest.raises(ValueError, match=r"ranks must lie in 0 \.\. 64"):
        ragged_plan([65], max_rank=64)
    with pytest.raises(ValueError):
        ragged_plan([3], max_rank=32)


# ---------------------------------------------------------------------------------------------- host interface
def _fac(m, r, seed=0):
    return rc._dense_factor(np.random.default_rng(seed), m, r)


def test_build_factored_model_rank_limits():
    m = 70
    with pytest.raises(ValueError, match=r"17 factor columns, 17 weights \(at most 16\)"):
        build_factored_model([-np.eye(m)], [[_fac(m, 17)]], np.zeros(1), factored_form=1)
    fm = build_factored_model([-np.eye(m)], [[_fac(m, 64), _fac(m, 3, 1)]], np.zeros(2), factored_form=1, max_rank=64)
    assert fm.lowrank[0][2] == 64 and fm.wide and fm.factored
    with pytest.raises(ValueError, match=r"65 factor columns, 65 weights \(at most 64\)"):
        build_factored_model([-np.eye(m)], [[_fac(m, 65)]], np.zeros(1), factored_form=1, max_rank=64)
    with pytest.raises(ValueError, match="max_rank"):
        build_factored_model([-np.eye(m)], [[_fac(m, 3)]], np.zeros(1), factored_form=1, max_rank=48)
    narrow = build_factored_model([-np.eye(m)], [[_fac(m, 16)]], np.zeros(1), factored_form=1, max_rank=64)
    assert narrow.lowrank[0][2] == 16 and not narrow.wide


@pytest.mark.parametrize("name,khat", [("V1", [32]), ("V2", [64]), ("V3", [64]), ("V4", [32, 2])])
def test_padded_rank_of_the_cases(name, khat):
    fm = wc.model(name)
    assert [lr[2] for lr in fm.lowrank] == khat and fm.wide
    assert [f.name for f in dataclasses.fields(fm)][-1] == "ragged"      # (`wide` is read off lowrank: no new field)


def test_a_diagonal_part_beside_a_wide_rank_is_refused():
    m = 40
    V, d = _fac(m, 20)
    trace = (None, [], np.ones(m))
    with pytest.raises(ValueError, match=r"constraint 1 has 20 factor columns .* constraint 2 a diagonal part .* sparse matrix"):
        build_factored_model([-np.eye(m)], [[(V, d), trace]], np.zeros(2), factored_form=1, max_rank=64)
    # the hybrid form goes in: the trace row as a stored sparse matrix
    fm = build_factored_model([-np.eye(m)], [[(V, d), sp.identity(m, format="csc")]], np.zeros(2), factored_form=1, max_rank=64)
    assert fm.wide and sorted(fm.stored[0]) == [1] and not fm.diag[0]
    # ... and a diagonal part beside ranks up to 16 stays what it was, under either limit
    V, d = _fac(m, 16)
    for kw in ({}, dict(max_rank=64)):
        fm = build_factored_model([-np.eye(m)], [[(V, d), trace]], np.zeros(2), factored_form=1, **kw)
        assert sorted(fm.diag[0]) == [1] and not fm.wide


class _Stop(RuntimeError):
    pass


class _RecordingDevice:
    """Stands where the device would: records options and uploads in their order and ends the run at the first set_factored."""

    def __init__(self):
        self.log = []

    def set_option(self, key, value):
        self.log.append((key, value))

    def upload_lowrank(self, i, khat, V, d):
        self.log.append(("upload_lowrank", khat))

    def set_factored(self, i):
        raise _Stop()

    def __getattr__(self, name):
        if name in ("upload_model", "upload_diag"):
            return lambda *a, **k: None
        raise AttributeError(name)


@pytest.mark.parametrize("wide", [None, False, True])
def test_host_opt_in(wide):
    from loraine_jl_amd.optimizer import Optimizer
    P = rc.Planted() if not wide else wc.PlantedWide()
    dev = _RecordingDevice()
    o = Optimizer(device=dev)
    o.set_silent(True)
    kw = {} if wide is None else dict(wide=wide)
    o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True, factored_form=1, **kw)
    with pytest.raises(_Stop):
        o.optimize()
    assert dev.log == [("lowrank_wide", 1 if wide else 0), ("upload_lowrank", 64 if wide else 8)]


def test_wide_constraints_need_the_opt_in():
    from loraine_jl_amd.optimizer import Optimizer
    P = wc.PlantedWide()
    o = Optimizer(device=_RecordingDevice())
    o.set_silent(True)
    o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True, factored_form=1)
    with pytest.raises(ValueError, match=r"\(at most 16\)"):
        o.optimize()


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 64])
def test_wide_is_a_bool(bad):
    from loraine_jl_amd.optimizer import Optimizer
    P = rc.Planted()
    with pytest.raises(ValueError, match="wide is False or True"):
        Optimizer(device=_RecordingDevice()).load_factored_model(P.F0(), P.factors(), P.b, wide=bad)


def test_wide_combines_with_ragged_and_cg():
    from loraine_jl_amd.optimizer import Optimizer
    P = wc.PlantedWide()
    dev = _RecordingDevice()
    o = Optimizer(device=dev)
    o.set_silent(True)
    o.set_attribute("kit", 1)
    o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True, factored_form=1, wide=True, ragged="all", cg=True)
    assert o._pending[1][-1] is True                                 # (cg stays the last word of the pending load)
    with pytest.raises(_Stop):
        o.optimize()
    assert dev.log[0] == ("lowrank_wide", 1)


def test_more_than_one_gpu_is_refused():
    import types
    from loraine_jl_amd.sharding import DistributedHotPath
    solver = types.SimpleNamespace(kit=0, model=wc.model("V1"), dist=None)
    with pytest.raises(ValueError, match="wide=True.*one GPU"):
        DistributedHotPath(solver, 0, 2)


# ---------------------------------------------------------------------------------------------- the epilogue's order in NumPy
def _facs(name):
    return list(wc.items(name))


@pytest.mark.parametrize("with_G", [True, False], ids=["G", "W-only"])
@pytest.mark.parametrize("name", ["V1", "V2", "V3"])
def test_the_device_order_matches_the_reference(name, with_G):
    m, n = wc.SIZES[name]
    W, G = wc.scaling(name)[0]
    H, pairs, ng = wc.device_order(_facs(name), m, W, G if with_G else None, n)
    assert len(pairs) == ng * (ng + 1) // 2 and set(pairs.values()) == {1}
    err = rc.relerr(H, wc.reference(name, True))
    print("WIDE cpu %s %s | cond(W) %.1e | %.2e" % (name, "G" if with_G else "W-only", np.linalg.cond(W), err))
    assert err < 1e-13
    out = [k for k, r in enumerate(wc.RANKS[name]) if r == 0]
    assert np.all(H[out, :] == 0.0) and np.all(H[:, out] == 0.0)


def test_block_sums_of_a_tile_are_the_plain_sums():
    """tile_blocks against S.reshape(...).sum for every class pair the tiles of a wide block can have."""
    S = np.random.default_rng(4).standard_normal((64, 64)) ** 2
    for ka in wc.WIDE_CLASSES:
        for kb in wc.WIDE_CLASSES:
            want = S.reshape(64 // ka, ka, 64 // kb, kb).sum(axis=(1, 3))
            got = wc.tile_blocks(S, ka, kb)
            assert got.shape == want.shape and np.allclose(got, want, rtol=1e-14, atol=0.0), (ka, kb)


FAULTS = [("drop16", "V1"), ("drop16", "V2"), ("drop16", "V3"), ("acc", "V1"), ("acc", "V2"), ("acc", "V3"), ("wave", "V2"),
          ("wave", "V3"), ("noskip", "V1"), ("noskip", "V2"), ("pad", "V2"), ("pad", "V3")]


@pytest.mark.parametrize("fault,name", FAULTS)
def test_a_single_fault_breaks_the_bound(fault, name):
    """drop16: one 16 x 16 sub-block of a wide diagonal block left out; acc: the second accumulator; wave: the second wave; noskip:
    gi < gj not skipped in a class-32 diagonal tile; pad: weight 1 and a non-zero operand on the padding columns of a constraint of
    rank 33 .. 63.  Each must miss 1e-12 by at least 1e3."""
    m, n = wc.SIZES[name]
    W, G = wc.scaling(name)[0]
    H, _, _ = wc.device_order(_facs(name), m, W, G, n, fault=fault)
    err = rc.relerr(H, wc.reference(name, True))
    print("WIDE cpu fault %s on %s | %.2e" % (fault, name, err))
    assert err >= 1e-9
