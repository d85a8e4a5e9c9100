"""The long route of the Schur assembly (option pair_long, csrc/longops.hip) as far as it goes without a GPU:

  * the lists of csrc/model_layout.h::block_long through lrn_dbg_model_layout -- lg_hi, lg_rptr, lg_rows, lg_eptr, lg_ec, lg_ev --
    against the NumPy statement long_rows_cases.spec_long, exactly, on every case of that file;
  * both kernels' orders of summation restated in float64 (long_rows_cases.route) against the definition in np.longdouble:
    within gamma_L B_ij on every routed pair of every case, for a benign and a graded W, with the MFMA form on and off and with
    one slice and many -- and eight single faults, each of which misses that bound by 10^3 or changes a counter;
  * the conditions the cases promise;
  * the argument checks of the long_rows opt-in of the four loaders, and what the solver sets on the device."""
import ctypes as C
import os

import numpy as np
import pytest

import loraine_jl_amd
from loraine_jl_amd.optimizer import Optimizer
import local_support_cases as lc
import long_rows_cases as lr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["lg_hi", "lg_rptr", "lg_rows", "lg_eptr", "lg_ec", "lg_ev"]


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
    real = name == "lg_ev"
    out = np.zeros(cnt.value, dtype=np.float64 if real else np.int64)
    rc = lib.lrn_dbg_model_layout(name.encode(), *args, C.byref(cnt), *((None, p(out)) if real else (p(out), None)), msg, len(msg))
    assert rc == 0 and cnt.value == out.size
    return out


def case_layout(case, name, ib=0):
    return layout(name, int(case.msizes[ib]), case.AA[ib], case.sigmaA[:, ib], case.qA[0, ib], case.nlmi == 1, case.dense_threshold)


# ---------------------------------------------------------------------------------------------- the lists
@pytest.mark.parametrize("name", lr.NAMES)
def test_lists_against_the_numpy_statement(name):
    case = lr.build_case(name)
    for ib in range(case.nlmi):
        spec = lr.spec_long(name, ib, lr.LONG_MIN)           # (the debug entry point plans with the default of pair_long_min)
        for key in ("nd", "q_wave", "npos_nz"):
            assert case_layout(case, key, ib)[0] == getattr(spec, key), key
        for key in NAMES:
            got, want = case_layout(case, key, ib), np.atleast_1d(getattr(spec, key))
            assert got.shape == want.shape and (got == want).all(), (name, ib, key)


def test_the_cases_have_what_they_were_built_for():
    tr = lr.spec_long("trace")
    loc = tr.loc
    assert tr.nnz[:12].tolist() == [1024, 961, 300, 289, 256, 225, 144, 94, 91, 64, 64, 49]
    assert (tr.nd, tr.lg_hi, loc.loc_lo, loc.loc_hi) == (0, 11, 3, 12)
    ident = tr.mats[2]
    assert (ident == np.eye(300)).all() and len(tr.R[2]) == 300                 # rho = 300: two stripes, ld = 320
    assert {int(v) for v in loc.s[3:tr.npos_nz]} >= {1, 2, 8, 12, 15, 16, 17, 31, 32}     # one and two tiles on the MFMA side
    assert tr.npos_nz == lr.build_case("trace").nvar - 1                       # the empty constraint is the last position
    A12 = tr.mats[6]
    assert loc.s[6] == 12 and not (A12 == A12.T).all()                          # the unsymmetric element
    lone = [p for p in range(tr.npos_nz) if tr.nnz[p] == 1 and loc.s[p] == 2]
    assert lone                                                                 # an off-diagonal entry without its twin
    pl, lg_end = lr.plan(tr, local=1)
    assert lg_end == 3 and lr.plan(tr, local=0)[1] == 11
    assert lr.slices(1024, 32, 512) == (64, 16) and lr.slices(300, 300, 512)[0] == 60 and lr.slices(300, 300, lr.LONG_SPLIT)[0] == 3
    rows = lr.spec_long("rows")
    assert rows.nnz[:7].tolist() == [769, 769, 456, 257, 256, 255, 65] and rows.lg_hi == 7 and rows.loc.loc_hi == rows.loc.loc_lo
    assert sorted(len(R) for R in rows.R) == [65, 255, 256, 256, 257, 257, 257]
    bidiag = rows.mats[2]
    assert (np.triu(bidiag) == bidiag).all() and not (bidiag != 0).any(axis=1)[256] and (bidiag != 0).any(axis=0)[256]
    assert all(p[2] == "entry" for p in lr.plan(rows)[0])
    edge = lr.spec_long("edge")
    assert edge.nnz[:5].tolist() == [41, 40, 40, 39, 39] and edge.lg_hi == 3 and lr.spec_long("edge", 0, lr.LONG_MIN).lg_hi == 0
    e64 = lr.spec_long("edge64")
    assert e64.nnz[:5].tolist() == [65, 64, 64, 63, 63] and e64.lg_hi == 3
    prefix = lr.spec_long("prefix")
    assert prefix.nd == 3 and prefix.lg_hi == 11 and lr.plan(prefix, local=1)[1] == 3      # local on: nothing left for the long route
    ov = lr.spec_long("overlap")
    assert ov.nnz[0] == 1024 and ov.loc.s[0] == 32 and (ov.loc.loc_lo, ov.loc.loc_hi, ov.lg_hi) == (0, 4, 3)
    assert lr.plan(ov, local=1)[1] == 0 and lr.plan(ov, local=0)[1] == 3
    assert all(p[2] == "mfma" for p in lr.plan(ov, local=0)[0])
    blocks = lr.build_case("blocks")
    assert blocks.nlmi == 2 and blocks.nlin == 4 and lr.spec_long("blocks", 1).lg_hi == 0
    none = lr.spec_long("none")
    assert none.lg_hi == none.nd == 0 and none.lg_rptr.size == 0 and none.lg_ev.size == 0


# ---------------------------------------------------------------------------------------------- the algebra
CONFIGS = {"mfma": dict(mfma=1, split=lr.LONG_SPLIT), "entry_sliced": dict(mfma=0, split=512)}


def ratio_of(name, wname, local=0, mfma=1, split=lr.LONG_SPLIT, fault=None, fault_pair=None):
    spec = lr.spec_long(name)
    pl, lg_end = lr.plan(spec, local, mfma, split)
    got, cnt = lr.route(name, wname, local, mfma, split, fault, fault_pair)
    return lr.worst(name, wname, got, pl, spec), cnt == lr.counters(pl, lg_end, spec)


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("wname", ["benign", "graded"])
@pytest.mark.parametrize("name", ["trace", "rows", "edge", "prefix", "overlap"])
def test_kernel_orders_meet_the_bound(name, wname, config):
    ratio, same = ratio_of(name, wname, **CONFIGS[config])
    print(name, wname, config, "worst error / bound", ratio)
    assert ratio <= 1.0 and same


def test_kernel_orders_meet_the_bound_beside_the_local_route():
    ratio, same = ratio_of("trace", "graded", local=1)
    assert ratio <= 1.0 and same


FAULTS = {
    # fault: (case, configuration, the pair of positions it is planted on or None)
    "owner_transposed": ("rows", CONFIGS["entry_sliced"], (2, 2)),      # A_i' for A_i on the unsymmetric row
    "pq": ("rows", CONFIGS["entry_sliced"], "lone"),                    # p and q exchanged on the partner without twin (owner: the
                                                                        # unsymmetric row -- a symmetric owner cannot tell)
    "stripe": ("trace", CONFIGS["entry_sliced"], (2, 2)),               # the last thread stripe (a >= 256) dropped
    "ktail": ("trace", CONFIGS["mfma"], (2, 3)),                        # the K tail (a >= 256 of 300) dropped
    "slice": ("trace", CONFIGS["entry_sliced"], (0, 0)),                # one slice dropped
    "self_doubled": ("rows", CONFIGS["entry_sliced"], None),            # the self pair doubled
    "ah_transposed": ("trace", CONFIGS["mfma"], (6, 6)),                # Ah_j' for Ah_j on the unsymmetric element (its self pair)
    "range": ("trace", CONFIGS["mfma"], None),                          # the range off by one
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_single_faults_are_seen(fault):
    name, cfg, pair = FAULTS[fault]
    if pair == "lone":
        spec = lr.spec_long(name)
        pj = [p for p in range(spec.npos_nz) if spec.nnz[p] == 1 and spec.loc.s[p] == 2][0]
        pair = (2, pj)
    ratio, same = ratio_of(name, "benign", fault=fault, fault_pair=pair, **cfg)
    print(fault, "worst error / bound", ratio, "counters equal", same)
    assert ratio >= 1.0e3 or not same
    if fault != "range":
        assert ratio >= 1.0e3                               # (these seven are faults of the arithmetic)


# ---------------------------------------------------------------------------------------------- the host argument
@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0])
def test_long_rows_is_a_bool(bad):
    o = Optimizer()
    A, b = lr.trace_model(24)
    tru3 = os.path.join(GOLDEN, "tru3.dat-s")
    with pytest.raises(ValueError, match="long_rows"):
        o.load_model(A, b, long_rows=bad)
    with pytest.raises(ValueError, match="long_rows"):
        o.read_from_file(tru3, long_rows=bad)
    with pytest.raises(ValueError, match="long_rows"):
        o.load_factored_model([A[0][0]], [[]], b, long_rows=bad)
    with pytest.raises(ValueError, match="long_rows"):
        o.load_detected_model(A, b, long_rows=bad)
    o.load_model(A, b, long_rows=True, local_support=True)
    assert o._long_rows is True and o._local_support is True
    o.load_model(A, b)
    assert o._long_rows is False
    o.read_from_file(tru3, long_rows=True)
    assert o._long_rows is True


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
    A, b = lr.trace_model(24)
    dev = _RecordingDevice()

    def run(long_rows, local=False):
        o = Optimizer(device=dev)
        o.set_silent(True)
        o.load_model(A, b, long_rows=long_rows, local_support=local)
        del dev.log[:]
        with pytest.raises(_Stop):
            o.optimize()
        return [e for e in dev.log if e[0] in ("upload_model", "pair_local", "pair_long")]

    assert run(False) == [("upload_model",)]                                   # the library's default: nothing to set
    assert run(True) == [("upload_model",), ("pair_long", 1)]
    assert run(True, True) == [("upload_model",), ("pair_local", 1), ("pair_long", 1)]
    assert run(False) == [("upload_model",), ("pair_local", 0), ("pair_long", 0)]      # the device was left at 1, 1
    assert run(False) == [("upload_model",)]
