"""GPU: the one-sided Jacobi SVD of csrc/jacobi.hip column by column, against the np.longdouble reference and the derived
bounds of tests/jacobi_cases.py (whose inputs, reference and bounds tests/test_jacobi_cases_cpu.py checks without a GPU).

Paths: the one-workgroup kernel (n <= 96), the 16-column block kernels (default from n = 97: odd and even numbers of blocks,
ragged last blocks of 1 and 15 columns, two to five row chunks) and the 32-column block kernels (option jacobi_block: even
n takes the 16-byte loads of the Gram kernel with a scalar tail, odd n scalar loads throughout); options jacobi_wgs = 1 and
4096 (one row chunk, ceil(n / 64) chunks), jacobi_cross = 0, jacobi_inner = 2, jacobi_early = 3e-8 and 0.
Families: graded over 1e8, 1e12, 1e16 (permuted, ascending, descending), clusters of relative width 1e-9 ... 1e-4, rank
deficient (a zero, a duplicate and an exactly dependent column), exactly orthogonal, scaled by 2^+-150.

With u = 2^-53, eps = 2u, tol = eps sqrt(max(n, 4)), kB = kappa_2 of the column-scaled input, beta = n eps kB:
  sig    |s_j - sref_j| <= beta sref_j after sorting        res    ||A v_j - (US)_j|| <= beta s_j for every column
  vorth  max |V'V - I| <= beta                               cos    largest cosine of two columns of US <= 4 tol after a
  sweep that rotated nothing (one-workgroup kernel; jacobi_early = 0), <= 2n 1e-2 early under the early stop (a cap)
  sweeps at most the float64 restatement's (jc.f64_small, jc.f64_blocked) plus 2
  rank deficient: zero column exactly zero, dependent directions and every error below n eps s_max; exactly orthogonal:
  nothing changes, bit for bit; V == NULL (what the solver's own calls pass): US, s and sweeps bit for bit those with V.
Every case prints its figures (lines JACOBI); the last test prints the worst ratio to each bound per path.

Observed on an MI355X, worst measured / bound, one-workgroup / 16-column / 32-column kernels: sig 0.080 / 0.069 / 0.049,
res 0.078 / 0.060 / 0.048, vorth 0.161 / 0.137 / 0.097, cos after a confirming sweep 0.253 / 0.251 / 0.251 (under the early
stop at most 2.0e-14 against a cap of 1e-7), rank deficient |s - sref| / (n eps s_max) 0.515 / 0.180 / 0.187; sweeps within
one of the float64 restatement's on every case (6 to 8 graded, 15 to 21 clustered, 10 to 14 rank deficient)."""
import numpy as np
import pytest

import jacobi_cases as jc

pytestmark = pytest.mark.gpu
WORST = {}


@pytest.fixture(scope="module")
def dev():
    import loraine_jl_amd
    d = loraine_jl_amd.Device(0)
    yield d
    d.close()


def _svd(dev, case, vectors=True):
    family, n, param, jb, opts = case
    assert (jb == 0) == (n <= jc.JAC_SMALL)
    settings = dict(opts)
    if jb == 32:
        settings["jacobi_block"] = 32
    try:
        for k, val in settings.items():
            dev.set_option(k, val)
        return dev.dbg_svd_jacobi(jc.make(family, n, param).A, vectors)
    finally:
        for k in settings:
            dev.set_option(k, jc.DEFAULTS[k])


@pytest.mark.parametrize("case", jc.CASES, ids=jc.case_id)
def test_jacobi_svd_within_the_derived_bounds(dev, case):
    US, s, V, sweeps = _svd(dev, case)
    r = jc.judge(case, US, V, s, sweeps, "device")
    ref_sweeps = jc.restated(case, False)[3]
    print("JACOBI device   %-44s sweeps %d, float64 restatement %d" % (jc.case_id(case), sweeps, ref_sweeps))
    assert sweeps <= ref_sweeps + 2, (jc.case_id(case), sweeps, ref_sweeps)
    w = WORST.setdefault({0: "small", 16: "16-column", 32: "32-column"}[case[3]], {})
    for k, x in r.items():
        w[k] = max(w.get(k, 0.0), float(x))


def test_one_by_one(dev):
    for a in (-3.5, 1e-100):
        A = np.array([[a]])
        US, s, V, sweeps = dev.dbg_svd_jacobi(A)
        assert np.array_equal(US, A) and np.array_equal(V, [[1.0]]) and s[0] == abs(a) and sweeps == 1


@pytest.mark.parametrize("n,jb", [(161, 16), (194, 32)])
def test_one_row_chunk_and_the_default_agree(dev, n, jb):
    """jacobi_wgs = 1 sums the Gram matrices in one chunk, the default in several: other bits, the same singular values
    to within beta"""
    inp = jc.make("graded", n, -12)
    s_one = _svd(dev, ("graded", n, -12, jb, (("jacobi_wgs", 1),)))[1]
    s_def = _svd(dev, ("graded", n, -12, jb, ()))[1]
    a, b = np.sort(s_one.astype(jc.LD)), np.sort(s_def.astype(jc.LD))
    d = float((np.abs(a - b) / b).max())
    print("JACOBI device   n=%d jb=%d wgs=1 against the default: %.2e (beta %.2e)" % (n, jb, d, n * jc.EPS * inp.kB))
    assert d <= n * jc.EPS * inp.kB


@pytest.mark.parametrize("case", [("graded", 96, -12, 0, ()), ("graded", 161, -12, 16, ()), ("graded", 161, -12, 32, ())],
                         ids=jc.case_id)
def test_without_vectors_the_rotations_are_the_same(dev, case):
    """V == NULL is what prepare_W and the preconditioner setup pass: the rotations depend on A alone"""
    US, s, V, sweeps = _svd(dev, case)
    US0, s0, V0, sweeps0 = _svd(dev, case, vectors=False)
    assert V0 is None and sweeps0 == sweeps
    assert np.array_equal(US0, US) and np.array_equal(s0, s)


def test_zz_worst_ratios_on_the_device():
    for path, w in sorted(WORST.items()):
        print("JACOBI device worst measured / bound, %-9s: " % path + "  ".join("%s %.3f" % kv for kv in sorted(w.items())))
    assert all(x <= 1.0 for w in WORST.values() for x in w.values())
