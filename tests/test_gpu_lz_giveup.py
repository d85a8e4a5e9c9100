"""GPU: the give-up and restart path of the resident Lanczos launches (csrc/lz.hip).

A resident launch whose workgroups wait for each other longer than "lz_res_limit" raises its abort word, every workgroup
returns, and the host repeats the run from the start vector with one launch per step (lz_fetch -> lz_record_give_up ->
lz_collect / lanczos_ends / lanczos_extremes_plain).  The test hook "lz_test_withhold" makes ONE workgroup of ONE run keep
ONE step's publication to itself in the k-th resident launch, which is exactly what an unscheduled peer looks like to the
others; the limit is set to 1 ms, so a provoked wait costs a millisecond and the kernel returns normally.

Reference of every case: the launched form (lz_resident = 0) on a context that never gave up -- pinned to LAPACK / NumPy
by test_lanczos_eigmin / test_lanczos_extremes and to the resident form bit for bit by
test_resident_lanczos_steps_are_the_launched_ones.  The restart repeats the run from the same start vector with the
launched form's arithmetic: the agreement asked for is bit for bit, not a tolerance.

`lz_no_persist` is sticky: every test creates its own contexts and closes them.
"""
import contextlib
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")

# 1 ms of the 100 MHz wall clock: healthy steps take 2-5 us (README.md, profiles/r04_xcd_barrier.txt), a > 200-fold margin
# against a spurious give-up
LIMIT = 100000
FIRST, MIDDLE, LAST = 0, 1, 2          # step of the launch
WG0, WGLAST = 0, 1                     # workgroup 0 (also writes for the host) / nwg - 1 (the ragged one)
COMBOS = [(FIRST, WG0), (FIRST, WGLAST), (MIDDLE, WG0), (MIDDLE, WGLAST), (LAST, WG0), (LAST, WGLAST)]


def withhold_code(k, run=0, step=FIRST, wg=WG0):
    """Value of option "lz_test_withhold" (include/loraine_hip.h)."""
    assert 1 <= k < 100000
    return k + 100000 * (run + 2 * (step + 3 * wg))


@contextlib.contextmanager
def device(resident, **opts):
    import loraine_jl_amd
    d = loraine_jl_amd.Device(0)
    try:
        d.set_option("lz_resident", resident)
        for key, v in opts.items():
            d.set_option(key, v)
        yield d
    finally:
        d.close()


def arm(d, k, run=0, step=FIRST, wg=WG0):
    d.set_option("lz_res_limit", LIMIT)
    d.set_option("lz_test_withhold", withhold_code(k, run, step, wg))
    assert d.count("lz_test_withheld") == 0 and d.count("lz_persist_abort") == 0 and d.count("lz_no_persist") == 0


def assert_gave_up_once(d):
    assert d.count("lz_test_withheld") == 1          # the hook fired: the case is not vacuous
    assert d.count("lz_persist_abort") == 1
    assert d.count("lz_no_persist") == 1


def assert_launched_from_now_on(d, call, ref, eq=None):
    """A second call on a context that gave up: its own reference, no resident launch, no second give-up."""
    launches, aborts = d.count("lz_resident_launches"), d.count("lz_persist_abort")
    got = call(d)
    assert (eq(got, ref) if eq else got == ref), (got, ref)
    assert d.count("lz_resident_launches") == launches
    assert d.count("lz_persist_abort") == aborts
    assert d.count("lz_test_withheld") == 1


def sym(Q, lam):
    M = (Q * lam) @ Q.T
    return (M + M.T) / 2


def clustered(n, seed):
    """The clustered spectrum of test_resident_lanczos_steps_are_the_launched_ones: -1, a cluster of n / 4 values within
    1e-3 above it, the rest spread over [0.5, 40]."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.concatenate([[-1.0], -1.0 + 1e-3 * rng.random(n // 4), np.linspace(0.5, 40.0, n - 1 - n // 4)])
    return sym(Q, lam)


def gaussian(n, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return sym(Q, rng.standard_normal(n))


# ---- a. single run

def _single_run_case(M, M2, ref, ref2, k, step, wg):
    with device(1) as d:
        arm(d, k, 0, step, wg)
        got = d.dbg_eigmin(M)
        assert_gave_up_once(d)
        assert got == ref, (k, step, wg, got, ref)          # Ritz value and step count, bit for bit
        assert_launched_from_now_on(d, lambda dd: dd.dbg_eigmin(M2), ref2)


def test_single_run_every_launch_of_the_run():
    """n = 333, every resident launch of the run in turn: the first batch, batches after several looks at T (have_prev,
    theta_prev, last_move, err_prev / err_last, scale set), and batches queued ahead of a look (lanczos_ahead > 0)."""
    n = 333
    # (seed 7 n as in test_resident_lanczos_steps_are_the_launched_ones; on the MI355X the reference run queues batches
    # ahead with it -- asserted below, change the seed if a change of the look-ahead rule makes it fail)
    M, M2 = clustered(n, 7 * n), gaussian(n, n + 1)
    with device(0) as r:
        ref = r.dbg_eigmin(M)
        assert r.count("lanczos_ahead") > 0
        ref2 = r.dbg_eigmin(M2)
        assert r.count("lz_resident_launches") == 0 and r.count("lz_no_persist") == 0
    print(f"n={n}: reference {ref}, second {ref2}")
    assert ref[1] >= 64
    nlaunch = math.ceil(ref[1] / 16)
    for k in range(1, nlaunch + 1):
        step, wg = COMBOS[(k - 1) % len(COMBOS)]
        _single_run_case(M, M2, ref, ref2, k, step, wg)


@pytest.mark.parametrize("n,k,step,wg", [(1024, 1, LAST, WGLAST), (1024, 3, LAST, WG0), (32, 1, MIDDLE, WGLAST), (32, 2, MIDDLE, WG0)])
def test_single_run_smallest_and_largest_size(n, k, step, wg):
    """n = 32: two workgroups, the `t < nwg` load of the partial sums nearly empty; n = 1024: 64 workgroups, all 16 rows
    per lane in use."""
    M, M2 = clustered(n, 7 * n), gaussian(n, n + 1)
    with device(0) as r:
        ref, ref2 = r.dbg_eigmin(M), r.dbg_eigmin(M2)
    print(f"n={n}: reference {ref}, second {ref2}")
    if n == 1024:
        assert ref[1] >= 64
    assert ref[1] > 16 * (k - 1)          # launch k exists
    _single_run_case(M, M2, ref, ref2, k, step, wg)


# ---- b. certified value

def wide_spectrum(n, hi):
    """test_certified_eigmin_on_wide_spectra"""
    rng = np.random.default_rng(n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.concatenate([[-1.005], -np.exp(rng.uniform(np.log(1e-3), np.log(0.9), 5)),
                          np.exp(rng.uniform(np.log(1e-3), np.log(hi), n - 6))])
    M = (Q * lam) @ Q.T
    return 0.5 * (M + M.T)


def test_certified_value_after_a_give_up():
    n, hi = 145, 1e10
    M, M2 = wide_spectrum(n, hi), wide_spectrum(60, 1e2)
    exact = np.linalg.eigvalsh(M)[0]
    with device(0) as r:
        ref, ref2 = r.dbg_eigmin(M, certified=True), r.dbg_eigmin(M2, certified=True)
        plain = r.dbg_eigmin(M)
    assert plain[1] > 16          # launch 2 exists
    with device(1) as d:
        arm(d, 2, 0, MIDDLE, WGLAST)
        got = d.dbg_eigmin(M, certified=True)
        assert_gave_up_once(d)
        assert got == ref, (got, ref)
        assert got[0] <= exact + 1e-6 * abs(exact)
        assert got[0] == pytest.approx(exact, rel=1e-6, abs=1e-6 * hi * 1e-9)
        assert_launched_from_now_on(d, lambda dd: dd.dbg_eigmin(M2, certified=True), ref2)


# ---- c, d, f: a one-block model

def one_block(d, n):
    import scipy.sparse as sp
    nvar = 4
    AA = sp.csc_matrix((np.ones(nvar), (np.arange(nvar), np.arange(nvar) * (n + 1))), shape=(nvar, n * n))
    d.upload_model([AA], np.arange(nvar, dtype=np.int64).reshape(-1, 1), np.zeros((2, 1), dtype=np.int64), [n])
    d.ip_set_c(0, np.eye(n))
    return nvar


def _stats(d, X, S):
    d.ip_set_iterate(0, X, S)
    return d.ip_stats()


@pytest.mark.parametrize("pair", [2, 1, 0])
@pytest.mark.parametrize("n", [333, 801])
def test_two_runs_side_by_side(n, pair):
    """eigmin_certified_pair through ip_stats (nt_mode = 0: no Cholesky shortcut): X takes several times the batches S does,
    so the pair goes in lock-step first and the longer run goes on alone.  eigmin_pair = 2: one grid for both runs -- only
    one of them gives up, both are repeated; 1: two streams, one resident run each -- the other run finishes resident;
    0: one run after the other."""
    X, S = clustered(n, 7 * n), gaussian(n, 3 * n + 1)
    X2, S2 = gaussian(n, 5 * n + 2), clustered(n, 11 * n)
    opts = dict(nt_mode=0, eigmin_pair=pair)
    with device(0, **opts) as r:
        one_block(r, n)
        ref, ref2 = _stats(r, X, S), _stats(r, X2, S2)
        sx, ss = r.dbg_eigmin(X)[1], r.dbg_eigmin(S)[1]
        assert r.count("lz_resident_launches") == 0
    print(f"n={n} pair={pair}: steps X {sx}, S {ss}; reference {ref.tolist()}")
    assert sx >= ss + 64          # different batches: the longer run goes on alone for at least four
    # where the launches of a healthy resident call fall (a probe, not a reference)
    with device(1, **opts) as p:
        one_block(p, n)
        got = _stats(p, X, S)
        launches, pair_batches = p.count("lz_resident_launches"), p.count("lanczos_resident_batches")
        assert p.count("lz_persist_abort") == 0 and p.count("lz_no_persist") == 0
        assert np.array_equal(got, ref)
    print(f"   healthy resident call: {launches} launches, {pair_batches} batches of the pair")
    if pair == 2:
        assert pair_batches > 0
        alone = pair_batches + 2          # (the pair has at most one launch more than looks: a batch queued ahead)
        assert launches > alone
        cases = [(1, 0, FIRST, WG0), (1, 1, LAST, WGLAST), (alone, 0, MIDDLE, WGLAST), (alone, 1, FIRST, WGLAST)]
    elif pair == 1:
        # launches alternate between the streams while both runs live (1 = run 0, 2 = run 1, no batch queued ahead):
        # launch 2 ss / 16 is the last one of S
        alone = 2 * (ss // 16) + 3
        assert launches > alone
        cases = [(1, 0, MIDDLE, WG0), (2, 0, FIRST, WGLAST), (alone, 0, LAST, WG0)]
    else:
        cases = [(1, 0, LAST, WGLAST), (2, 0, MIDDLE, WG0)]          # (the run of X; the run of S is then a launched one)
    for k, run, step, wg in cases:
        with device(1, **opts) as d:
            one_block(d, n)
            arm(d, k, run, step, wg)
            got = _stats(d, X, S)
            assert_gave_up_once(d)
            assert np.array_equal(got, ref), (k, run, step, wg, got.tolist(), ref.tolist())
            assert_launched_from_now_on(d, lambda dd: _stats(dd, X2, S2), ref2, eq=np.array_equal)


def spd(n, rng):
    Mx = rng.standard_normal((n, n + 7)) / np.sqrt(n)
    return Mx @ Mx.T + 0.05 * np.eye(n)


@pytest.mark.parametrize("n,run", [(333, 0), (801, 1)])
def test_find_step_after_a_give_up(n, run):
    """ip_find_step after ip_prepare_w with a seeded dely: the give-up falls into the first launch of the predictor's pair
    of runs; the corrector call that follows is healthy."""
    rng = np.random.default_rng(n)
    X, S = spd(n, rng), spd(n, rng)
    y, dely = rng.standard_normal(4), rng.standard_normal(4)

    def prepare(d):
        one_block(d, n)
        d.ip_set_iterate(0, X, S)
        d.ip_residual_d(y)
        assert d.ip_prepare_w(0) == 0

    def predictor(d):
        a, b = d.ip_find_step(1, 0.0, 0.9, dely)
        return float(a[0]), float(b[0])

    def corrector(d):
        d.ip_update(1, 0.5, 0.5)
        a, b = d.ip_find_step(0, 0.1, 0.9, 0.5 * dely)
        return float(a[0]), float(b[0])

    with device(0) as r:
        prepare(r)
        ref, ref2 = predictor(r), corrector(r)
        assert r.count("lz_resident_launches") == 0
    print(f"n={n}: predictor {ref}, corrector {ref2}")
    with device(1) as d:
        prepare(d)
        assert d.count("lz_resident_launches") == 0          # (ns_lanczos_min = 1500: prepare_w takes none at this size)
        arm(d, 1, run, MIDDLE, WG0 if run else WGLAST)
        got = predictor(d)
        assert_gave_up_once(d)
        assert got == ref, (got, ref)
        assert_launched_from_now_on(d, corrector, ref2)


def test_lanczos_ends_with_the_second_launch_queued_behind():
    """The scale of the Newton-Schulz iteration: 24 steps as two resident launches queued at once.  The first gives up, the
    second runs with the abort word already raised."""
    n = 640
    rng = np.random.default_rng(n)
    X, S, X2, S2 = spd(n, rng), spd(n, rng), spd(n, rng), spd(n, rng)

    def scaling(d, X=X, S=S):
        one_block(d, n)
        d.ip_set_iterate(0, X, S)
        assert d.ip_prepare_w(0) == 0
        out = [d.dbg_get_block(0, name)[0] for name in ("W", "Yh", "Zh")]
        assert d.dbg_get_block(0, "W")[1] == 1          # eigen-free scaling
        assert d.count("ns_fallback") == 0
        return out + [d.timing("ns_c")]

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]

    opts = dict(ns_lanczos_min=8, nt_mode=1)
    with device(0, **opts) as r:
        ref = scaling(r)
        assert r.count("lanczos_ends_steps") == 24 and r.count("lz_resident_launches") == 0
        ref2 = scaling(r, X2, S2)
    with device(1, **opts) as p:          # (probe: the healthy call is two resident launches)
        assert same(scaling(p), ref)
        assert p.count("lz_resident_launches") == 2 and p.count("lz_no_persist") == 0
    with device(1, **opts) as d:
        arm(d, 1, 0, LAST, WGLAST)
        got = scaling(d)
        assert_gave_up_once(d)
        assert d.count("lz_resident_launches") == 2
        assert same(got, ref)
        assert_launched_from_now_on(d, lambda dd: scaling(dd, X2, S2), ref2, eq=same)


# ---- e. H_alpha set-up

def _extreme_spectra(n):
    """test_lanczos_extremes_resident_steps_are_the_launched_ones"""
    rng = np.random.default_rng(n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lams = (np.concatenate([np.exp(rng.uniform(np.log(1e-3), np.log(1.0), n - 1)), [2.0e4]]),
            np.concatenate([0.0132 * (1.0 + 3e-4 * np.arange(n // 3)), np.exp(rng.standard_normal(n - n // 3 - 2)) * 0.3, [39.3, 33694.0]]))
    out = []
    for lam in lams:
        W = (Q * lam) @ Q.T
        out.append(0.5 * (W + W.T))
    return out


def _same_extremes(a, b):
    (lt0, U0, lmin0, tr0, st0), (lt1, U1, lmin1, tr1, st1) = a, b
    return st0 == st1 and lmin0 == lmin1 and tr0 == tr1 and np.array_equal(lt0, lt1) and np.array_equal(U0, U1)


@pytest.mark.parametrize("which,k", [(0, 1), (1, 1), (1, 4)])
def test_h_alpha_setup_hands_over_to_the_full_version(which, k):
    """dbg_lanczos(W, 1), n = 600, resident launches of 24 steps.  A give-up hands the set-up to the fully re-orthogonalised
    version -- different arithmetic: the bounds are those of test_lanczos_extremes against numpy.linalg.eigh.  Launch 4 is
    the first one the plain route can queue ahead of a look (two looks must have been taken)."""
    n = 600
    Ws = _extreme_spectra(n)
    W, W2 = Ws[which], Ws[1 - which]
    with device(0) as r:
        ref = r.dbg_lanczos(W, 1)
        ahead = r.count("lanczos_plain_ahead")
        ref2 = r.dbg_lanczos(W2, 1)
        assert r.count("lanczos_plain") == 2 and r.count("lz_resident_launches") == 0
    print(f"spectrum {which}: reference {ref[4]} steps, {ahead} batches queued ahead")
    assert ref[4] > 24 * (k - 1)
    if k > 1:
        assert ahead > 0
    ev, V = np.linalg.eigh(W)
    with device(1) as d:
        arm(d, k, 0, MIDDLE if k == 1 else FIRST, WGLAST if which else WG0)
        lt, U, lmin, tr, steps = d.dbg_lanczos(W, 1)
        assert_gave_up_once(d)
        assert d.count("lanczos_plain") == 0          # the plain route did not deliver this one
        assert steps <= n
        assert np.allclose(lt, ev[-1:], rtol=1e-9)
        assert abs(tr - np.trace(W)) <= 1e-11 * abs(np.trace(W))
        assert ev[0] - 1e-9 * ev[-1] <= lmin <= ev[0] + (1e-12 if n == steps else 5e-2)
        assert np.allclose(np.abs(np.sum(U * V[:, -1:], axis=0)), 1.0, atol=1e-8)
        assert np.allclose(U.T @ U, np.eye(1), atol=1e-10)
        assert_launched_from_now_on(d, lambda dd: dd.dbg_lanczos(W2, 1), ref2, eq=_same_extremes)
        assert d.count("lanczos_plain") == 1          # the second call: the plain route, launched steps


# ---- g. a whole solve

def _solve(d):
    from loraine_jl_amd.optimizer import Optimizer
    o = Optimizer(resident=True, device=d)
    o.set_silent(True)
    o.set_attribute("kit", 0)
    o.set_attribute("datarank", -1)
    o.read_from_file(os.path.join(GOLD, "maxG11.dat-s"))
    o.optimize()
    assert o.termination_status() == "OPTIMAL"
    return o.solver.trace


def test_give_up_in_the_middle_of_a_solve():
    """maxG11 with a resident launch in the middle of the solve giving up: the same iterates as the launched form, bit for
    bit; resident launches before the give-up, none after it."""
    def objectives(trace):
        return [(t["primal_obj"], t["dual_obj"], t["dimacs"]) for t in trace]

    with device(0) as r:
        ref = objectives(_solve(r))
        assert r.count("lz_no_persist") == 0
    with device(1) as p:          # where the launches of a healthy solve fall (a probe, not a reference)
        trace = _solve(p)
        assert objectives(trace) == ref and p.count("lz_no_persist") == 0
        per_it = [t["lz_resident_launches"] for t in trace]
        assert all(t["lanczos_resident_batches"] > 0 for t in trace) and sum(t["lz_persist_abort"] for t in trace) == 0
    print(f"resident launches per iteration: {per_it}")
    assert len(per_it) >= 8
    k = sum(per_it[:5]) + per_it[5] // 2 + 1          # the middle of the sixth iteration
    with device(1) as d:
        arm(d, k, 1, MIDDLE, WGLAST)
        trace = _solve(d)
        assert d.count("lz_test_withheld") == 1 and d.count("lz_no_persist") == 1
        assert objectives(trace) == ref
        aborts = [t["lz_persist_abort"] for t in trace]
        assert sum(aborts) == 1
        it = aborts.index(1)
        print(f"launch {k}: gave up in iteration {it} of {len(trace)}")
        assert 3 <= it < len(trace) - 1
        assert all(t["lanczos_resident_batches"] > 0 for t in trace[:it])
        assert all(t["lanczos_resident_batches"] == 0 and t["lz_resident_launches"] == 0 for t in trace[it + 1:])


# ---- h. the limit

def test_wait_limit_is_clamped_and_healthy_runs_stay_below_it():
    with device(1) as d:
        assert d.count("lz_res_limit") == 2000000          # the default: 20 ms
        d.set_option("lz_res_limit", 1e12)
        assert d.count("lz_res_limit") == 2000000          # an option never lengthens the wait
        d.set_option("lz_res_limit", 1)
        assert d.count("lz_res_limit") == 1000
        d.reset_timing()
        assert d.count("lz_res_limit") == 1000             # state, not a counter
    with device(1) as d:          # default limit, no hook
        n = 801
        rng = np.random.default_rng(n)
        A = rng.standard_normal((n, n))
        lam, steps = d.dbg_eigmin((A + A.T) / 2)
        assert steps >= 16 and d.count("lz_resident_launches") >= steps // 16
        assert d.count("lz_persist_abort") == 0 and d.count("lz_no_persist") == 0 and d.count("lz_test_withheld") == 0
        assert lam == pytest.approx(np.linalg.eigvalsh((A + A.T) / 2)[0], rel=1e-9)
