"""The local route of the Schur assembly (option pair_local, csrc/localops.hip) as far as it goes without a GPU:

  * the lists of csrc/model_layout.h::block_local through lrn_dbg_model_layout -- loc_lo, loc_hi, loc_sptr, loc_sup, loc_aptr,
    loc_a -- against the NumPy statement local_support_cases.spec_local, exactly, on every case of that file;
  * the identity tr(A_i W A_j W) = <Ah_i Wij Ah_j, Wij>_F in the kernel's own order of summation, restated in float64
    (local_support_cases.pair_value), against the definition in np.longdouble: within gamma_96 B_ij on every local pair of
    every case, for a benign and a graded W -- and six single faults, each of which misses that bound by 10^3 or a counter;
  * tru3.dat-s has an empty local range (its constraints have at most 16 entries);
  * the argument check of Optimizer.load_model / read_from_file(local_support=...)."""
import ctypes as C
import os

import numpy as np
import pytest

import loraine_jl_amd
from loraine_jl_amd.model import model_from_sdpa
from loraine_jl_amd.optimizer import Optimizer
import local_support_cases as lc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["loc_lo", "loc_hi", "loc_sptr", "loc_sup", "loc_aptr", "loc_a"]


def layout(name, m, AA, sigma, qA, pos_space, dense_threshold):
    """one array of lrn_dbg_model_layout by name (one call for the length, one for the elements)"""
    lib = loraine_jl_amd.load_library()
    M = AA.tocsc()
    M.sort_indices()
    cp, rv = M.indptr.astype(np.int64) + 1, M.indices.astype(np.int64) + 1
    nz = np.ascontiguousarray(M.data, dtype=np.float64)
    sig = np.asarray(sigma, dtype=np.int64) + 1
    p = lambda a: C.c_void_p(a.ctypes.data)
    args = (m, len(sig), p(cp), p(rv), p(nz), p(sig), int(qA), int(pos_space), float(dense_threshold), 1 << 40,
            None, None, None, 0, None, None, None)
    cnt, msg = C.c_int64(0), C.create_string_buffer(1024)
    rc = lib.lrn_dbg_model_layout(name.encode(), *args, C.byref(cnt), None, None, msg, len(msg))
    assert rc == 0, msg.value.decode()
    real = name == "loc_a"
    out = np.zeros(cnt.value, dtype=np.float64 if real else np.int64)
    rc = lib.lrn_dbg_model_layout(name.encode(), *args, C.byref(cnt), *((None, p(out)) if real else (p(out), None)), msg, len(msg))
    assert rc == 0 and cnt.value == out.size
    return out


def case_layout(case, name, ib=0):
    return layout(name, int(case.msizes[ib]), case.AA[ib], case.sigmaA[:, ib], case.qA[0, ib], case.nlmi == 1, case.dense_threshold)


# ---------------------------------------------------------------------------------------------- the lists
@pytest.mark.parametrize("name", lc.NAMES)
def test_lists_against_the_numpy_statement(name):
    case = lc.build_case(name)
    for ib in range(case.nlmi):
        spec = lc.spec_local(case, ib)
        for key in ("nd", "q_wave", "npos_nz"):
            assert case_layout(case, key, ib)[0] == getattr(spec, key), key
        for key in NAMES:
            got, want = case_layout(case, key, ib), np.atleast_1d(getattr(spec, key))
            assert got.shape == want.shape and (got == want).all(), (name, ib, key)


def test_the_cases_have_what_they_were_built_for():
    sizes = lc.spec_local(lc.build_case("sizes"))
    own = set(sizes.s[sizes.loc_lo:sizes.loc_hi].tolist())
    assert sizes.loc_lo == 0 and {15, 16, 17, 31, 32} <= own and {1, 2, 5, 15} <= set(sizes.s[sizes.loc_hi:sizes.npos_nz].tolist())
    assert sizes.npos_nz == lc.build_case("sizes").nvar - 1                       # the empty constraint is the last position
    assert (sizes.npos_nz - sizes.loc_lo) % 4 != 0                                # partners: no multiple of the waves a workgroup
    # a one-tile owner meets a two-tile partner and the other way round
    tiles = (sizes.s + 15) // 16
    combos = {(int(tiles[i]), int(tiles[j])) for i in range(sizes.loc_lo, sizes.loc_hi) for j in range(i, sizes.npos_nz)}
    assert combos == {(1, 1), (1, 2), (2, 1), (2, 2)}
    A12 = sizes.mats[int(np.nonzero(sizes.s == 12)[0][0])]
    assert not (A12 == A12.T).all()                                               # the unsymmetric Ah
    front = lc.spec_local(lc.build_case("front33"))
    assert front.s[0] == 33 and (front.loc_lo, front.nd) == (1, 0) and front.loc_hi == sizes.loc_hi + 1
    mid = lc.spec_local(lc.build_case("mid33"))
    assert mid.s[mid.loc_lo - 1] == 33 and mid.loc_lo > 3 and mid.loc_hi > mid.loc_lo + 3
    edge = lc.spec_local(lc.build_case("edge"))
    assert edge.nnz[:5].tolist() == [37, 36, 36, 35, 35] and (edge.loc_lo, edge.loc_hi) == (0, 3)
    tiny = lc.spec_local(lc.build_case("tiny"))
    assert tiny.nnz[0] == lc.LOCAL_MIN - 1 and tiny.loc_lo == tiny.loc_hi == 0 and tiny.loc_sup.size == 0 and tiny.loc_a.size == 0
    tail = lc.spec_local(lc.build_case("tail33"))                                 # 20 entries without twins: s = 40 behind loc_hi
    assert tail.nnz[:2].tolist() == [64, 20] and tail.s[1] == 40 and tail.loc_lo == tail.loc_hi == 1 and tail.loc_sup.size == 0
    tail = lc.spec_local(lc.build_case("tail35"))                                 # symmetric, below pair_local_min, and yet s > 32
    assert tail.nnz[:2].tolist() == [64, 35] and tail.s[1] == 35 and tail.loc_lo == tail.loc_hi == 1 and tail.loc_sup.size == 0
    single = lc.spec_local(lc.build_case("single"))
    assert (single.loc_lo, single.loc_hi, single.owners) == (0, 1, 1)
    prefix = lc.spec_local(lc.build_case("prefix"))
    assert prefix.nd == 3 and prefix.loc_lo == 3 and prefix.loc_hi == sizes.loc_hi
    blocks = lc.build_case("blocks")
    assert blocks.nlmi == 2 and blocks.nlin == 4
    assert lc.spec_local(blocks, 0).owners == sizes.owners and lc.spec_local(blocks, 1).owners == 0


def test_tru3_has_no_local_range():
    model = model_from_sdpa(os.path.join(GOLDEN, "tru3.dat-s"), datarank=0)
    m = int(model.msizes[0])
    args = (m, model.AA[0], np.asarray(model.sigmaA)[:, 0], np.asarray(model.qA)[0, 0], model.nlmi == 1, -1.0)
    nnz = layout("nnz", *args)
    assert nnz.max() <= 16 < lc.LOCAL_MIN
    assert layout("loc_lo", *args)[0] == layout("loc_hi", *args)[0] == layout("nd", *args)[0]
    assert layout("loc_sup", *args).size == 0 and layout("loc_a", *args).size == 0


# ---------------------------------------------------------------------------------------------- the algebra
def worst(case, wname, fault=None):
    """largest |route - definition| / (gamma_96 B_ij) over the local pairs of block 0, and the counters"""
    spec = lc.spec_local(case)
    H, _ = lc.reference(case.name, wname)
    got, owners, pairs = lc.route(case, wname, fault=fault)
    ratio = 0.0
    for (k, l) in lc.local_pairs(case, spec):
        v = got.get((k, l), 0.0)                        # (a pair the faulty route left out left its zero in H)
        ratio = max(ratio, float(abs(lc.LD(v) - H[k, l])) / (lc.gamma(lc.DEPTH) * lc.pair_bound(case, spec, wname, k, l)))
    return ratio, owners == spec.owners and pairs == spec.pairs


@pytest.mark.parametrize("wname", ["benign", "graded"])
@pytest.mark.parametrize("name", ["sizes", "front33", "mid33", "edge", "single", "prefix"])
def test_identity_in_kernel_order_meets_the_bound(name, wname):
    ratio, counters = worst(lc.build_case(name), wname)
    print(name, wname, "worst error / bound", ratio)
    assert ratio <= 1.0 and counters


@pytest.mark.parametrize("fault", ["transposed", "wji", "unsorted", "diagonal", "padding", "range"])
def test_single_faults_are_seen(fault):
    case = lc.build_case("mid33" if fault == "range" else "sizes")
    ratio, counters = worst(case, "benign", fault)
    print(fault, "worst error / bound", ratio, "counters", counters)
    assert ratio >= 1.0e3 or not counters
    if fault != "range":
        assert ratio >= 1.0e3                           # (these five are faults of the arithmetic)


# ---------------------------------------------------------------------------------------------- the host argument
@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0])
def test_local_support_is_a_bool(bad):
    o = Optimizer()
    A, b = lc.q4_model(3)
    with pytest.raises(ValueError, match="local_support"):
        o.load_model(A, b, local_support=bad)
    with pytest.raises(ValueError, match="local_support"):
        o.read_from_file(os.path.join(GOLDEN, "tru3.dat-s"), local_support=bad)
    with pytest.raises(ValueError, match="local_support"):
        o.read_from_file(os.path.join(GOLDEN, "tru3.dat-s"), detect_kmax=16, local_support=True)
    o.load_model(A, b, local_support=True)
    assert o._local_support is True
    o.load_model(A, b)
    assert o._local_support is False


class _Stop(RuntimeError):
    pass


class _RecordingDevice:
    """Stands where the device would: records the options set and ends the run at the first call after the upload."""

    def __init__(self):
        self.log = []

    def set_option(self, key, value):
        self.log.append((key, value))

    def upload_model(self, *a, **k):
        self.log.append(("upload_model",))

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def stop(*a, **k):
            raise _Stop(name)
        return stop


def test_host_sets_the_option_after_the_upload_and_resets_a_used_device():
    A, b = lc.q4_model(3)
    dev = _RecordingDevice()

    def run(local):
        o = Optimizer(device=dev)
        o.set_silent(True)
        o.load_model(A, b, local_support=local)
        del dev.log[:]
        with pytest.raises(_Stop):
            o.optimize()
        return [e for e in dev.log if e[0] in ("upload_model", "pair_local")]

    assert run(False) == [("upload_model",)]                                   # the library's default: nothing to set
    assert run(True) == [("upload_model",), ("pair_local", 1)]
    assert run(False) == [("upload_model",), ("pair_local", 0)]                # the device was left at 1
    assert run(False) == [("upload_model",)]
