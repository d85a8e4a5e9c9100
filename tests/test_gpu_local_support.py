"""The local route of the Schur assembly on the device (option pair_local, csrc/localops.hip): every pair it computes against
the definition tr(A_i W A_j W) in np.longdouble, componentwise within gamma_96 B_ij (local_support_cases), for a benign and
a graded W; every other entry of H, and all of H where the route is not taken, bit for bit what the option-off assembly
gives; counters from the lists; one planted solve through Optimizer.load_model(local_support=True).

Every test here sets pair_local or local_support: none passes on a library without the route."""
import os

import numpy as np
import pytest

import local_support_cases as lc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROUTED = ["sizes", "front33", "mid33", "edge", "single", "prefix", "blocks"]
COUNTERS = ("pair_local_owners", "pair_local_pairs", "pair_local_skipped")


@pytest.fixture(scope="module")
def dev():
    import loraine_jl_amd
    d = loraine_jl_amd.Device(0)
    yield d
    d.set_option("pair_local", 0)
    d.set_option("pair_lanes", 0)
    d.set_option("dense_threshold", -1.0)
    d.close()


def upload(dev, case, wname):
    dev.set_option("dense_threshold", case.dense_threshold)
    dev.upload_model(case.AA, case.sigmaA, case.qA, case.msizes, C_lin=case.C_lin)
    for ib in range(case.nlmi):
        dev.set_scaling(ib, case.W[wname][ib])
    if case.nlin:
        dev.set_lin(case.X_lin, case.S_lin_inv)


def assemble(dev, local, lanes=0):
    dev.set_option("pair_local", local)
    dev.set_option("pair_lanes", lanes)
    dev.reset_timing()
    H = dev.schur_assemble(0, want_H=True)
    return H, {k: dev.count(k) for k in COUNTERS}


_RUNS = {}


def runs(dev, name, wname):
    """off, on, off, on on one uploaded model: computed once, shared, never modified"""
    if (name, wname) not in _RUNS:
        upload(dev, lc.build_case(name), wname)
        _RUNS[(name, wname)] = [assemble(dev, local) for local in (0, 1, 0, 1)]
    return _RUNS[(name, wname)]


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("wname", ["benign", "graded"])
@pytest.mark.parametrize("name", ROUTED)
def test_local_pairs_against_the_definition(dev, name, wname):
    case = lc.build_case(name)
    spec = lc.spec_local(case)
    (_, _), (H, cnt), _, _ = runs(dev, name, wname)
    Href, Btot = lc.reference(name, wname)
    assert cnt == {"pair_local_owners": spec.owners, "pair_local_pairs": spec.pairs, "pair_local_skipped": case.nlmi - 1}
    worst = 0.0
    for (k, l) in lc.local_pairs(case, spec):
        Bp = lc.pair_bound(case, spec, wname, k, l)
        # the pair itself within gamma_96; what else lands on the entry (case 'blocks': a pair of the tiny block, at most four
        # products of three factors, and the linear term, at most three) within gamma_16 of its own absolute sum
        bound = lc.gamma(lc.DEPTH) * Bp + lc.gamma(16) * max(0.0, float(Btot[k, l]) - Bp)
        assert H[k, l] == H[l, k]
        worst = max(worst, float(abs(lc.LD(H[k, l]) - Href[k, l])) / bound)
    print(name, wname, "pairs", spec.pairs, "worst error / bound", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("name", ROUTED)
def test_bits_off_on_off_on_and_outside_the_route(dev, name):
    case = lc.build_case(name)
    spec = lc.spec_local(case)
    (off, c0), (on, _), (off2, c2), (on2, _) = runs(dev, name, "benign")
    assert same_bits(off, off2) and same_bits(on, on2)
    assert c0 == c2 == dict.fromkeys(COUNTERS, 0)
    local = np.zeros(off.shape, dtype=bool)
    for (k, l) in lc.local_pairs(case, spec):
        local[k, l] = local[l, k] = True
    assert local.any() and not local.all()
    # every entry another route computes: the column of an s = 33 owner in front of the range, dense x local, tiny x tiny
    assert same_bits(on[~local], off[~local])
    assert not same_bits(on[local], off[local])          # (the route is another order of summation: it did run)


def test_the_route_leaves_the_s33_and_dense_owners_alone(dev):
    for name, pos in (("front33", 0), ("mid33", None), ("prefix", 0)):
        case = lc.build_case(name)
        spec = lc.spec_local(case)
        (off, _), (on, _), _, _ = runs(dev, name, "benign")
        pos = spec.loc_lo - 1 if pos is None else pos
        assert spec.s[pos] == 33 or pos < spec.nd
        k = int(case.sigmaA[pos, 0])
        below = [int(case.sigmaA[p, 0]) for p in range(pos, case.nvar)]
        assert same_bits(on[below, k], off[below, k])


def test_lists_go_to_the_device_with_the_first_use(dev):
    case = lc.build_case("sizes")
    spec = lc.spec_local(case)
    upload(dev, case, "graded")
    assemble(dev, 0)
    assemble(dev, 0)
    held = dev.count("device_bytes")                     # a model that never takes the route holds no copy of the lists ...
    assemble(dev, 1)
    assert dev.count("device_bytes") - held >= 8 * spec.loc_a.size + 4 * spec.loc_sup.size + 16 * (case.nvar + 1)
    upload(dev, case, "graded")                          # ... and a new upload drops the copies
    assemble(dev, 0)
    assert dev.count("device_bytes") == held


def test_pair_lanes_do_not_reach_the_local_columns(dev):
    case = lc.build_case("sizes")
    spec = lc.spec_local(case)
    upload(dev, case, "graded")
    H16, _ = assemble(dev, 1, lanes=16)
    H64, _ = assemble(dev, 1, lanes=64)
    idx = tuple(np.array(lc.local_pairs(case, spec)).T)
    assert same_bits(H16[idx], H64[idx])
    assert same_bits(H16[idx], runs(dev, "sizes", "graded")[1][0][idx])


@pytest.mark.parametrize("name", ["tiny", "tail33", "tail35"])
def test_empty_range_is_the_parent_bit_for_bit(dev, name):
    (off, _), (on, cnt), _, _ = runs(dev, name, "benign")
    assert same_bits(off, on)
    assert cnt == {"pair_local_owners": 0, "pair_local_pairs": 0, "pair_local_skipped": 1}


def test_tru3_is_unchanged(dev):
    from loraine_jl_amd.model import model_from_sdpa
    model = model_from_sdpa(os.path.join(GOLDEN, "tru3.dat-s"), datarank=0)
    dev.set_option("dense_threshold", -1.0)
    dev.upload_model(model.AA, model.sigmaA, model.qA, model.msizes, C_lin=model.C_lin if model.nlin else None)
    rng = np.random.default_rng(3)
    m = int(model.msizes[0])
    Gm = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    dev.set_scaling(0, Gm @ Gm.T)
    if model.nlin:
        dev.set_lin(np.exp(rng.uniform(-1, 1, model.nlin)), np.exp(rng.uniform(-1, 1, model.nlin)))
    off, _ = assemble(dev, 0)
    on, cnt = assemble(dev, 1)
    assert same_bits(off, on) and np.abs(off).max() > 0
    assert cnt == {"pair_local_owners": 0, "pair_local_pairs": 0, "pair_local_skipped": 1}


def test_pair_local_takes_0_or_1(dev):
    from loraine_jl_amd.device import LoraineHipError
    for bad in (2, -1, 0.5):
        with pytest.raises(LoraineHipError, match=r"\(-1\).*pair_local"):
            dev.set_option("pair_local", bad)
    with pytest.raises(LoraineHipError, match=r"\(-1\).*pair_local_min"):
        dev.set_option("pair_local_min", 0)
    dev.set_option("pair_local", 0)


@pytest.mark.parametrize("kit", [0, 1])
def test_planted_q4_model_solves_both_ways(kit):
    from loraine_jl_amd.optimizer import Optimizer
    A, b = lc.q4_model()
    out = {}
    for local in (True, False):
        o = Optimizer()
        o.set_silent(True)
        o.set_attribute("kit", kit)
        o.set_attribute("eDIMACS", 1e-7)
        o.load_model(A, b, local_support=local)
        o.optimize()
        out[local] = (o.termination_status(), o.objective_value(), o.solver.dev.count("pair_local_pairs"), o.solver.iter)
        o.solver.dev.close()
    print("kit", kit, out)
    assert out[True][0] == out[False][0] == "OPTIMAL"
    assert abs(out[True][1] - out[False][1]) <= 1e-6 * abs(out[False][1])
    assert out[False][2] == 0
    if kit == 0:
        assert out[True][2] > 0
