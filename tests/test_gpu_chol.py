"""GPU: the Cholesky factorisation, its pivot boosting and the triangular solves of csrc/chol.hip, entry by entry, against
the longdouble references of tests/chol_cases.py (whose conditions tests/test_chol_cases_cpu.py checks without a GPU).

Every bound is componentwise, in units of u = 2^-53, gamma_k = k u / (1 - k u) with k = n + 8 (Higham, Accuracy and
Stability, Thm 10.3, 8.5, 10.4; the 8 for square roots and reciprocals of a few ulp and the MFMA's summation order):
  potrf   |L L' - A| <= gamma |L||L'| on the lower triangle, info = 0; the input's strict upper triangle holds NaN
  trsm    |op(L) X - B| <= gamma |op(L)||X| with L read back from the device; nrhs 1 .. 257, both `trans`
  potrs   |b - L L' x| <= (2 gamma + gamma^2) |L||L'||x|
  boost   info and chol_boosted equal the reference's; boosted rows of the solve below 1e-30 max(|h|, |x_ref|), kept
          rows within 2 gamma_{3n+8} |H_RR^-1||L_ref||L_ref'||x_ref| of H_RR^-1 h_R; three repeats give the same bits;
          pivot_boost = 0 and lrn_schur_add_diag give the strict result and count nothing
Each test prints its largest err / (u B) (lines CHOL); these figures are information, the limit is gamma / u ~ n + 8.

Observed on an MI355X, largest err / (u B), benign / graded (limit):
  potrf 12.3 at n = 512 (520) / 10.4 at n = 129 (137); n = 1025: 11.7 / 5.4 (1033)
  trsm  5.4 / 7.2 at n = 451, nrhs = 257 (459); the one-thread-per-column kernel (nrhs 1, 2, 15) at most 5.3
  potrs 1.4 at n = 512 (1040) / 1.3 at n = 1 (18)
  boosting: kept rows at most 0.008 of their bound, boosted rows at most 1.7e-10 of theirs."""
import numpy as np
import pytest
import scipy.sparse as sp

import chol_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import loraine_jl_amd
    d = loraine_jl_amd.Device(0)
    yield d
    d.close()


def _report(tag, ratio, lim):
    print("CHOL %-44s max err/(u B) = %10.3f   limit %.1f" % (tag, ratio, lim))
    assert ratio <= lim, (tag, ratio, lim)


def _factor(dev, n, kind):
    """the device's factor of spd(n, kind), its strict upper triangle NaN on the way in"""
    A = cc.with_nan_upper(cc.spd(n, kind))
    L, info = dev.dbg_potrf(A)
    assert info == 0
    assert np.isfinite(L).all()
    return A, L


@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("n", cc.SIZES)
def test_potrf_and_potrs_entrywise(dev, n, kind):
    A, L = _factor(dev, n, kind)
    _report("potrf n=%d %s" % (n, kind), cc.check_potrf(L, A), cc.limit(n, "potrf"))
    b = cc.rhs(n)[:, 0]
    x, info = dev.dbg_potrs(A, b)
    assert info == 0
    _report("potrs n=%d %s" % (n, kind), cc.check_potrs(L, x, b), cc.limit(n, "potrs"))


@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("n", [512, 513])
def test_potrs_on_both_sides_of_the_single_workgroup_limit(dev, n, kind):
    """n = 512: potrs_small_kernel with its right-hand side filling the LDS array; 513: three super-blocks, the last of one
    row.  Right-hand sides that single out the first and the last row, and one graded like the matrix."""
    A, L = _factor(dev, n, kind)
    rng = np.random.default_rng(n)
    worst = 0.0
    for b in (np.ones(n), np.eye(n)[:, 0].copy(), np.eye(n)[:, n - 1].copy(),
              rng.standard_normal(n) * cc.spd_scaling(n, "graded")):
        x, info = dev.dbg_potrs(A, b)
        assert info == 0
        worst = max(worst, cc.check_potrs(L, x, b))
    _report("potrs n=%d %s, four right-hand sides" % (n, kind), worst, cc.limit(n, "potrs"))


@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("n", cc.TRSM_N)
def test_trsm_entrywise(dev, n, kind):
    A, L = _factor(dev, n, kind)
    L2, _ = dev.dbg_potrf(A)
    assert np.array_equal(L, L2)                                   # deterministic: the factor dbg_trsm solves with
    lim = cc.limit(n, "trsm")
    for trans in (False, True):
        worst, X1 = {}, None
        for nrhs in cc.NRHS:
            B = cc.rhs(n, nrhs)
            X, info = dev.dbg_trsm(A, B, trans)
            assert info == 0 and X.shape == B.shape
            worst[nrhs] = cc.check_trsm(L, X, B, trans)
            if nrhs == 1:
                X1 = X
            if nrhs == 2:
                # one right-hand side alone and as column 0 of two: the same system, so op(L) (x1 - x2) is within the
                # two residual bounds (not the same bits: other kernels from nrhs = 16 on, another GEMM shape before)
                same = cc.check_same_solution(L, X1[:, 0], X[:, 0], trans)
                assert same <= lim, (n, kind, trans, same)
        tag = "trsm n=%d %s trans=%d nrhs " % (n, kind, trans) + "/".join(str(k) for k in cc.NRHS)
        print("CHOL %s: %s" % (tag, " ".join("%.2f" % worst[k] for k in cc.NRHS)))
        _report("trsm n=%d %s trans=%d" % (n, kind, trans), max(worst.values()), lim)


# ------------------------------------------------------------------------------------------------ pivot boosting
def _schur_of_side(dev, n):
    """A tiny model with nvar = n (one block of side 8, one diagonal entry per constraint), assembled once so that H exists;
    -> pos, the position of variable i in the factorisation's order, read off an imported diag(1 .. n)."""
    AA = sp.csc_matrix((np.ones(n), (np.arange(n), (np.arange(n) % 8) * 9)), shape=(n, 64))
    dev.upload_model([AA], np.arange(n, dtype=np.int64).reshape(-1, 1), np.zeros((2, 1), dtype=np.int64), [8])
    dev.set_scaling(0, np.eye(8), np.eye(8))
    dev.schur_assemble(0)
    dev.schur_import_full(np.asfortranarray(np.diag(np.arange(1.0, n + 1))))
    pos = np.rint(np.diag(dev.schur_get())).astype(np.int64) - 1
    assert np.array_equal(np.sort(pos), np.arange(n))
    return pos


def _factor_imported(dev, H, boost, shift=None):
    dev.set_option("pivot_boost", boost)
    dev.schur_import_full(np.asfortranarray(np.array(H, dtype=np.float64)))
    if shift is not None:
        dev.schur_add_diag(shift)
    info = dev.schur_factor()
    return info, dev.count("chol_boosted")


def _solve_ones(dev, pos):
    x = np.empty(pos.size)
    x[pos] = dev.schur_solve(np.ones(pos.size))                    # (h = 1 is the same vector in either order)
    return x


def _strict_ok(dev, case, info):
    """the strict result: the reference's first bad column -- or, where that pivot is rounding noise on the device (an exact
    zero in the reference), a tiny diagonal there instead, as tests/test_gpu_blocks.py words it"""
    want = case.shifted.info if info[1] else case.strict.info
    if info[0] == want:
        return True
    if case.code not in ("0", "noise"):
        return False
    later = [c + 1 for c in case.cols if c + 1 > want]
    if info[0] in later:
        return True
    if info[0] != 0:
        return False
    L, i0 = dev.dbg_potrf(case.H)
    dg = np.abs(np.diag(L))
    return i0 == 0 and all(dg[c] < 1e-6 * dg.max() for c in case.cols)


_UPLOADED = {}                                                       # the side of the model the device holds -> pos


@pytest.mark.parametrize("name", cc.BOOST_NAMES)
def test_pivot_boosting_follows_its_rules(dev, name):
    n = cc.BOOST_N[name]
    if n not in _UPLOADED:
        _UPLOADED.clear()
        _UPLOADED[n] = _schur_of_side(dev, n)
    pos = _UPLOADED[n]
    case = cc.boost_case(name)
    try:
        runs = []
        for _ in range(3):
            info, count = _factor_imported(dev, case.H, case.boost)
            runs.append((info, count, _solve_ones(dev, pos) if info == 0 else None))
        info, count, x = runs[0]
        assert (info, count) == (case.ref.info, case.ref.count), (name, info, count, case.ref.info, case.ref.count)
        for i2, c2, x2 in runs[1:]:
            assert (i2, c2) == (info, count) and (x is None or np.array_equal(x, x2)), name
        if info == 0:
            rb, rk = cc.check_boost_solve(name, x)
            print("CHOL boost %-14s n=%d boosted %-28s |x_b| / limit = %9.2e   kept err / bound = %8.4f"
                  % (name, n, case.ref.boosted, rb, rk))
            assert rb <= 1.0 and rk <= 1.0, (name, rb, rk)
        # the strict factorisation: asked for, and after the caller has shifted the diagonal
        for boost, shift in ((0.0, None), (case.boost, cc.SHIFT)):
            si, sc = _factor_imported(dev, case.H, boost, shift)
            assert sc == 0, (name, boost, shift, sc)
            assert _strict_ok(dev, case, (si, shift is not None)), (name, boost, shift, si, case.strict.info)
    finally:
        dev.set_option("pivot_boost", cc.BOOST_DEFAULT)
