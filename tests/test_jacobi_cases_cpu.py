"""CPU: the inputs, the reference and the bounds of tests/jacobi_cases.py, which tests/test_gpu_jacobi.py applies to the device.

  * the conditions of the inputs: kappa_2 of the column-normalised graded matrices <= 15 (10.0 to 10.1), the grading span,
    the cluster widths, exact orthogonality of the permutation cases in integers, exact dependence of the planted columns;
  * the longdouble reference against itself: a column permutation of the input gives the same sorted singular values to
    1e-17 n relative;
  * a float64 restatement of both device algorithms (jc.f64_small, jc.f64_blocked) meets every bound on every case of the
    GPU test -- its sweep counts are the ones the GPU test compares the device's with;
  * eight single faults planted in the blocked restatement each break a bound by a factor of 1e3 or an exact assertion.
The last test prints the restatement's worst ratio to each bound per code path."""
import numpy as np
import pytest

import jacobi_cases as jc

LD = jc.LD
INPUTS = sorted({c[:3] for c in jc.CASES}, key=str)
WORST = {}


@pytest.mark.parametrize("inp", INPUTS, ids=lambda c: "-".join(str(x) for x in c if x is not None))
def test_input_conditions(inp):
    family, n, param = inp
    case = jc.make(family, n, param)
    A = case.A
    assert A.flags.f_contiguous and np.isfinite(A).all()
    assert case.kB <= 15.0 + (1e-9 if family == "cluster" else 0.0), case.kB
    norms = np.sqrt((A.astype(LD) ** 2).sum(axis=0))
    if family in ("graded", "scaled", "orth"):
        g = {"graded": -12 if param in ("desc", "asc") else param, "scaled": -8, "orth": -12}[family]
        scale = {"up": LD(2) ** 150, "down": LD(2) ** -150}.get(param, LD(1))
        assert np.allclose((norms / scale).astype(np.float64), np.abs(case.D), rtol=1e-14, atol=0)
        if n > 1:
            assert np.isclose(float(norms.max() / norms.min()), 10.0 ** -g, rtol=1e-12)
        if param == "desc":
            assert (np.diff(case.D) < 0).all()
        if param == "asc":
            assert (np.diff(case.D) > 0).all()
        if family == "graded" and n >= 64 and param not in ("desc", "asc"):
            for b in range(0, n - 15, 16):                           # every 16-column panel mixes magnitudes
                assert case.D[b:b + 16].max() / case.D[b:b + 16].min() > 10.0 ** (-g / 4.0)
        if family == "graded":
            assert 9.5 <= case.kB <= 10.2 or n < 17, case.kB
    if family == "scaled":
        tiny = np.finfo(np.float64).tiny
        nz = np.abs(A[A != 0])
        assert nz.min() > tiny * 2.0 ** 60 and np.array_equal(A, np.ldexp(jc.make("graded", n, -8).A, 150 if param == "up" else -150))
        # the squares the kernels form stay normal: Gram entries and r2 = d^2 + 4 ga^2 of jrot, tol^2 al be
        assert float(norms.max()) ** 4 < 1e300 and jc.tol_of(n) ** 2 * float(norms.min()) ** 4 > 1e-290
    if family == "cluster":
        q = n // 4
        d = np.sort(case.d)
        for centre in (0.2, 1.0, 3.0):
            near = d[np.abs(d / centre - 1.0) < 1e-3]
            assert near.size == q and np.isclose((near.max() - near.min()) / centre, param, rtol=1e-6), (centre, near.size)
        assert d.min() >= 0.2 and d.max() <= 3.0
        sref = jc.reference_sigma(family, n, param)
        assert float(np.abs(sref - d[::-1].astype(LD)).max()) < 64 * jc.EPS        # the clusters survive the product in float64
    if family == "orth":
        M = (A != 0).astype(np.int64)
        assert np.array_equal(M.T @ M, np.eye(n, dtype=np.int64)) and np.array_equal(M @ M.T, np.eye(n, dtype=np.int64))
    if family == "rankdef":
        z, (dup, src), (comb, j, k) = jc.rankdef_columns(n)
        assert len({z, dup, src, comb, j, k}) == 6
        assert not A[:, z].any() and np.array_equal(A[:, dup], A[:, src])
        assert np.array_equal(A[:, comb].astype(LD), LD(0.5) * A[:, j].astype(LD) - A[:, k].astype(LD))     # exact
        sref = jc.reference_sigma(family, n, param)
        assert sref[-1] == 0 and sref[-3] < 1e-18 * sref[0] and sref[-4] > 1e-8 * sref[0]


@pytest.mark.parametrize("inp", [("graded", 17, -12), ("graded", 97, -16), ("cluster", 64, 1e-6), ("scaled", 96, "down")],
                         ids=lambda c: "-".join(str(x) for x in c))
def test_reference_is_invariant_under_a_column_permutation(inp):
    family, n, param = inp
    A = jc.make(family, n, param).A
    perm = np.random.default_rng(5).permutation(n)
    s2 = np.sort(jc.jacobi_cyclic(A[:, perm], LD)[2])[::-1]
    sref = jc.reference_sigma(family, n, param)
    assert float((np.abs(s2 - sref) / sref).max()) <= 1e-17 * n


@pytest.mark.parametrize("param", ["up", "down"])
def test_reference_of_a_scaled_case_is_the_scaled_reference(param):
    """jc.reference_sigma takes the scaled cases' values from the unscaled one: the same bits as running the method on them"""
    direct = np.sort(jc.jacobi_cyclic(jc.make("scaled", 96, param).A, LD)[2])[::-1]
    assert np.array_equal(direct, jc.reference_sigma("scaled", 96, param))


def _path(case):
    return {0: "small", 16: "16-column", 32: "32-column"}[case[3]]


@pytest.mark.parametrize("case", jc.CASES, ids=jc.case_id)
def test_float64_restatement_meets_every_bound(case):
    US, V, s, sweeps = jc.restated(case)
    r = jc.judge(case, US, V, s, sweeps, "f64")
    w = WORST.setdefault(_path(case), {})
    for k, x in r.items():
        w[k] = max(w.get(k, 0.0), float(x))


@pytest.mark.parametrize("case", [("graded", 96, -12, 0, ()), ("graded", 161, -12, 16, ()), ("graded", 161, -12, 32, ())],
                         ids=jc.case_id)
def test_restatement_without_vectors_is_the_same(case):
    US, V, s, sweeps = jc.restated(case)
    US2, V2, s2, sweeps2 = jc.restated(case, False)
    assert V2 is None and np.array_equal(US, US2) and np.array_equal(s, s2) and sweeps == sweeps2


def test_chunk_plan_of_the_option_cases():
    """jacobi_wgs = 1 is one row chunk, 4096 is ceil(n / 64) chunks, the default lies between at these sizes"""
    assert jc.chunk_plan(161, 16, 1) == (192, 1) and jc.chunk_plan(161, 16, 4096) == (64, 3)
    assert jc.chunk_plan(194, 32, 1) == (256, 1) and jc.chunk_plan(194, 32, 4096) == (64, 4)
    assert [jc.chunk_plan(n, 16)[1] for n in (97, 128, 129, 161, 257)] == [2, 2, 3, 3, 5]


FAULT_CASE = ("graded", 113, -12, 16, (("jacobi_early", 0.0),))


@pytest.mark.parametrize("fault", jc.FAULTS)
def test_planted_fault_breaks_a_bound(fault):
    """n = 113 in 16-column blocks: a ragged last block of one column and a ragged last row chunk; jacobi_early = 0, so that
    the cosine bound is the sharp one.  Each fault breaks a bound by 1e3 or the sweep limit."""
    family, n, param, jb, opts = FAULT_CASE
    inp = jc.make(family, n, param)
    US, V, s, sweeps = jc.f64_blocked(inp.A, jb, True, 0.0, fault=fault)
    m = jc.measure(inp.A, US, V, s, jc.reference_sigma(family, n, param))
    r = jc.ratios(m, jc.limits(n, inp.kB, True, 0.0))
    print("JACOBI fault %-18s sweeps %2d  " % (fault, sweeps) + "  ".join("%s %.2e" % kv for kv in r.items()))
    assert not 0 < sweeps < jc.MAX_SWEEPS or max(r.values()) >= 1e3, (fault, sweeps, r)


def test_zz_worst_ratios_of_the_restatement():
    for path, w in sorted(WORST.items()):
        print("JACOBI f64 worst measured / bound, %-9s: " % path + "  ".join("%s %.3f" % kv for kv in sorted(w.items())))
    assert all(x <= 1.0 for w in WORST.values() for x in w.values())
