"""The conditions that tests/test_gpu_chol.py rests on, checked without a GPU (tests/chol_cases.py):
  * the designed inputs are what they are said to be: the conditioning of the SPD matrices, exact pivots, the pivot
    ratios of every boosting case far from the threshold, cond_2(H_RR) <= 1e4;
  * a float64 NumPy restatement of the algorithm, column by column with no blocking, meets every bound that the GPU test
    asserts, against the same longdouble references -- so the bounds hold for an honest implementation;
  * single planted faults in that restatement each break a bound (by a factor of at least 1e3) or a count."""
import numpy as np
import pytest

import chol_cases as cc


# ------------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("n", cc.SIZES)
def test_spd_conditioning_windows(n):
    A = cc.spd(n, "benign")
    assert np.array_equal(A, A.T) and np.linalg.cond(A) <= 1e6 and np.linalg.eigvalsh(A).min() > 0
    A, d = cc.spd(n, "graded"), cc.spd_scaling(n, "graded")
    assert np.array_equal(A, A.T)
    cond, minpiv = cc.core_condition(n, "graded")
    assert minpiv > 0
    if n == 1:
        assert cond == pytest.approx(1.0)
        return
    assert 1e11 <= cond <= 1e13, cond
    assert d.max() / d.min() == pytest.approx(1e6, rel=1e-9)
    rows = np.sqrt(np.diag(A))                                     # the small rows a norm-wise check is blind to
    assert rows.max() / rows.min() >= (1e5 if n > 9 else 1e3)


def test_nan_fills_the_strict_upper_triangle_only():
    A = cc.with_nan_upper(cc.spd(9, "graded"))
    assert np.isnan(A[np.triu_indices(9, 1)]).all() and np.array_equal(np.tril(A), np.tril(cc.spd(9, "graded")))


def test_exact_matmul_is_exact_up_to_what_it_reports():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((70, 90)) * 10.0 ** rng.uniform(-8, 8, (70, 1))
    B = rng.standard_normal((90, 33)) * 10.0 ** rng.uniform(-8, 8, (1, 33))
    C, left = cc.exact_matmul(A, B)
    ref = A.astype(cc.LD) @ B.astype(cc.LD)
    bound = np.abs(A).astype(cc.LD) @ np.abs(B).astype(cc.LD)
    assert (np.abs(C - ref) <= left + 2.0 ** -60 * bound).all()     # (the plain longdouble product carries 2^-64 per term)
    assert (left <= 1e-15 * bound).all()


@pytest.mark.parametrize("name", cc.BOOST_NAMES)
def test_boost_cases_are_decided_far_from_the_threshold(name):
    case = cc.boost_case(name)
    assert np.array_equal(case.H, case.H.T, equal_nan=True)
    r = case.ref.ratios[np.isfinite(case.ref.ratios)]
    assert r.size > 0 and not ((r >= 1e-2) & (r <= 1e2)).any()
    want = [] if case.code == "kept" else case.cols
    if name == "neg9":                                             # abandoned at the ninth: the strict factorisation decides
        assert (case.ref.info, case.ref.count, case.ref.boosted) == (case.cols[0] + 1, 0, [])
    elif name in ("zero_row", "nan_diag"):
        assert (case.ref.info, case.ref.count) == (case.cols[0] + 1, 0)
    else:
        assert (case.ref.info, case.ref.count, case.ref.boosted) == (0, len(want), want)
        k = cc.kept_reference(name)
        assert cc.kept_condition(name) <= 1e4
        # boosted rows of the reference itself: 1e-40 relative, ten orders inside the limit
        b = np.array(case.ref.boosted, dtype=np.int64)
        assert b.size == 0 or float(np.abs(case.ref.x[b]).max()) <= 1e-38 * float(np.abs(k.x).max())
        assert float(np.abs(case.ref.x[k.R] - k.x).max()) <= 1e-17 * float(np.abs(k.x).max())
    # the strict result: the first column whose exact pivot is not positive
    bad = [j for j in case.cols if case.code in ("0", "-1e-8", "noise", "neg", "zero_row", "nan_diag")]
    assert case.strict.info == (bad[0] + 1 if bad else 0) and case.strict.count == 0
    assert case.shifted.info == (0 if name == "zero_row" else case.strict.info)


def test_boost_positions_cover_the_code_paths():
    n, cols = zip(*cc._POS.values())
    flat = {c for cs in cols for c in cs}
    assert {1, 5, 63, 64, 70, 72, 79, 450, 530, 20} == flat and 72 % 8 == 0 and 79 % 8 == 7
    assert cc.max_boost(200) == 8 and cc.max_boost(577) == 9 and len(cc.SPECIAL["neg9"][1]) == 9


# ------------------------------------------------------------------------------------------------ the honest restatement
@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("n", cc.SIZES)
def test_float64_restatement_meets_the_potrf_and_potrs_bounds(n, kind):
    A = cc.with_nan_upper(cc.spd(n, kind))
    info, _, L = cc.f64_factor(A)
    assert info == 0
    assert cc.check_potrf(L, A) <= cc.limit(n, "potrf")
    b = cc.rhs(n)
    x = cc.f64_trsm(L, cc.f64_trsm(L, b, False), True)
    assert cc.check_potrs(L, x[:, 0], b[:, 0]) <= cc.limit(n, "potrs")


@pytest.mark.parametrize("n", cc.TRSM_N)
def test_float64_restatement_meets_the_trsm_bound(n):
    A = cc.with_nan_upper(cc.spd(n, "graded"))
    _, _, L = cc.f64_factor(A)
    for trans in (False, True):
        for nrhs in cc.NRHS:
            B = cc.rhs(n, nrhs)
            assert cc.check_trsm(L, cc.f64_trsm(L, B, trans), B, trans) <= cc.limit(n, "trsm")


@pytest.mark.parametrize("name", cc.BOOST_NAMES)
def test_float64_restatement_meets_the_boosting_assertions(name):
    case = cc.boost_case(name)
    info, count, x = cc.f64_schur(case.H, case.boost)
    assert (info, count) == (case.ref.info, case.ref.count)
    if info == 0:
        rb, rk = cc.check_boost_solve(name, x)
        assert rb <= 1.0 and rk <= 1.0
    info, count, _ = cc.f64_schur(case.H, 0.0)
    assert count == 0 and (info == case.strict.info or (case.code in ("0", "noise") and info == 0))


# ------------------------------------------------------------------------------------------------ planted faults
def _boost_outcome(name, fault):
    """(info, count) match the reference and the solve is within its bounds; -> (matches, worst ratio)"""
    case = cc.boost_case(name)
    with np.errstate(all="ignore"):
        info, count, x = cc.f64_schur(case.H, case.boost, fault)
    same = (info, count) == (case.ref.info, case.ref.count)
    worst = np.inf if not same else (max(cc.check_boost_solve(name, x)) if info == 0 else 0.0)
    return same, worst


@pytest.mark.parametrize("fault,name", [
    ("running_diagonal", "c70/1e-8"),      # threshold against the running diagonal: a positive pivot is never boosted
    ("running_diagonal", "q0q7/0"),
    ("boost_empty_row", "zero_row"),       # d0 = 0 boosted: info 0 where the row must fail
    ("boost_nan", "nan_diag"),
    ("limit_off_by_one", "neg8"),          # the eighth boosted pivot already abandons the attempt
    ("limit_off_by_one", "neg9_577"),
    ("column_not_dropped", "neg8"),        # the boosted column goes on into the later updates
])
def test_planted_boosting_faults_are_caught(fault, name):
    assert _boost_outcome(name, None) == (True, pytest.approx(0.0, abs=1.0))
    same, worst = _boost_outcome(name, fault)
    assert (not same) or worst >= 1e3, (same, worst)


def test_planted_fault_strict_less_is_caught_where_the_pivot_equals_the_threshold():
    """piv == boost d0 exactly (H = [[1, 1], [1, 2]] in a corner of an identity, boost = 1/2: piv = 2 - 1 = 1/2 * 2): `<=`
    boosts it, `<` does not.  Only here: on the device such an equality would hang on the last bit of a square root."""
    H = np.eye(12)
    H[4, 3] = H[3, 4] = 1.0
    H[4, 4] = 2.0
    assert cc.ref_factor(H, 0.5, 8)[:2] == (0, [4])
    assert cc.f64_factor(H, 0.5, 8)[:2] == (0, 1)
    assert cc.f64_factor(H, 0.5, 8, "strict_less")[:2] == (0, 0)
    # ... and an exact zero pivot with d0 > 0 is below the threshold under both
    case = cc.boost_case("c70/0")
    assert cc.f64_schur(case.H, case.boost, "strict_less")[:2] == (0, 1)


@pytest.mark.parametrize("fault", ["skip_block", "drop_fma"])
@pytest.mark.parametrize("kind", cc.KINDS)
def test_planted_update_faults_break_the_potrf_bound(fault, kind):
    n = 129
    A = cc.with_nan_upper(cc.spd(n, kind))
    info, _, L = cc.f64_factor(A, fault=fault)
    assert info != 0 or cc.check_potrf(L, A) >= 1e3 * cc.limit(n, "potrf")


def test_a_single_wrong_entry_passes_a_normwise_check_and_breaks_the_componentwise_one():
    """Why entry by entry: one entry of a small row of the graded factor off by a relative 1e-6 leaves the norm-wise
    residual of tests/test_gpu_blocks.py at rounding level."""
    n = 129
    A = cc.spd(n, "graded")
    _, _, L = cc.f64_factor(A)
    L = np.tril(L)
    i = int(np.argmin(np.diag(A)))
    j = 0 if i > 0 else 1
    i, j = max(i, j), min(i, j)
    L[i, j] *= 1.0 + 1e-6
    assert np.linalg.norm(L @ L.T - A) / np.linalg.norm(A) < 1e-11
    assert cc.check_potrf(L, A) >= 1e3 * cc.limit(n, "potrf")


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("fault", ["upper_read", "last_rhs"])
def test_planted_trsm_faults_break_the_bound(fault, trans):
    n, nrhs = 65, 17
    A = cc.with_nan_upper(cc.spd(n, "graded"))
    L = cc.with_nan_upper(cc.f64_factor(A)[2])                      # (strict upper: scratch, as the device holds it)
    B = cc.rhs(n, nrhs)
    assert cc.check_trsm(L, cc.f64_trsm(L, B, trans), B, trans) <= cc.limit(n, "trsm")
    assert cc.check_trsm(L, cc.f64_trsm(L, B, trans, fault), B, trans) >= 1e3 * cc.limit(n, "trsm")
