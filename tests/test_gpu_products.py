"""The n x n product layer (csrc/products.hip, symadd of csrc/matops.hip) and the triangular-K ranges of the GEMM
(GEMM_KFROM_M/_N, GEMM_KTO_M/_N, GEMM_C_MIRROR) by themselves, through lrn_dbg_gemm and lrn_dbg_product.

Why the inputs are integers.  Operands hold integers from {-3 .. 3} and alpha is 1 or 0.5, so with K <= 1502 every partial
sum of a product is an integer (or half of one) far below 2^53 in whatever order a kernel adds it: the float64 product NumPy
forms on the host is THE result, and the assertions are np.array_equal, not a tolerance.  A 16 x 16 block that is misplaced,
skipped or added twice, or one element read from the wrong side of a tile boundary, cannot hide behind round-off.  A
triangular operand has stored zeros in its other triangle -- the contract of the K-range flags: a K-step that is computed
early multiplies stored zeros.  One case per entry point runs standard-normal operands against a np.longdouble product
(side 300 only: such a product at 1500 takes minutes).

Why the slab buffer is overwritten first.  A product of side 256 .. 1499 comes back as split-K slabs in ONE cached buffer
per stream that every product reuses, and a symmetric product writes only its lower 64-tiles there: what lies above them is
legitimately stale.  Before every such case a full product of the same side on operands scaled by 2^40 (still exact) fills
the buffer with values around 2^80, so a consumer that reads one stale element is wrong by thirty orders of magnitude
rather than by whatever the previous test happened to leave behind.

Which kernel and how many slabs every shape here takes is pinned without a GPU in tests/test_gemm_plan_cpu.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KFROM_N, KFROM_M, KTO_N, KTO_M = 64, 128, 1024, 2048
BIG_TILE_MIN_N = 1500          # csrc/ops.h
# split factor of the full product (flags = 0) at the sides of the kind 3 cases: tests/test_gemm_plan_cpu.py pins them
FULL_SPLIT = {255: 1, 256: 2, 300: 3, 385: 4, 650: 4, 1300: 1}


@pytest.fixture(scope="module")
def dev():
    import loraine_jl_amd
    d = loraine_jl_amd.Device(0)
    yield d
    d.close()


def ints(rng, *shape):
    return rng.integers(-3, 4, size=shape).astype(np.float64)


def relerr(a, b):
    a = np.asarray(a, dtype=np.longdouble); b = np.asarray(b, dtype=np.longdouble)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def tiles128(n):
    t = np.arange(n) // 128
    return t[:, None] > t[None, :], t[:, None] == t[None, :], t[:, None] < t[None, :]      # below, diagonal, above


# ================================================================== 1. GEMM flags through lrn_dbg_gemm
# NT layout, C = alpha A B' (A: M x K, B: N x K).  op(A)[m][k] = A[m, k], op(B)[k][n] = B[n, k]:
#   KFROM_M: A zero for k < m (upper triangular)     KTO_M: A zero for k > m (lower triangular)
#   KFROM_N: B zero for k < n (upper triangular)     KTO_N: B zero for k > n (lower triangular)
def _operands(rng, M, N, K, flag):
    A = ints(rng, M, K); B = ints(rng, N, K)
    if flag == KFROM_M: A = np.triu(A)
    if flag == KTO_M: A = np.tril(A)
    if flag == KFROM_N: B = np.triu(B)
    if flag == KTO_N: B = np.tril(B)
    return A, B


def _both_mask_forms(dev, A, B, alpha, flags, Cin=None):
    """The product with the straight-line pattern loops and with the branch-per-block body: identical bits."""
    from loraine_jl_amd import _capi
    C0 = dev.dbg_gemm(A, B, False, True, alpha=alpha, Cin=Cin, flags=flags)
    C1 = dev.dbg_gemm(A, B, False, True, alpha=alpha, Cin=Cin, flags=flags | _capi.GEMM_DYN_MASKS)
    assert np.array_equal(C0, C1)
    return C0


# 300 / 385 / 400: direct-to-LDS 128-tile kernel, 3-4 tiles, partial last tile, K % 16 = 12 / 1 / 0, 385 an odd leading
# dimension; 130: register-staged 128-tile kernel (K < 256); (300, 140, 300): the triangular operand spans K, the other
# dimension is narrower
_FLAG_IDS = {KFROM_M: "kfrom_m", KTO_M: "kto_m", KFROM_N: "kfrom_n", KTO_N: "kto_n"}
_ALONE = [(n, n, n, f) for n in (300, 385, 400, 130) for f in (KFROM_M, KTO_M, KFROM_N, KTO_N)] + \
         [(300, 140, 300, f) for f in (KFROM_M, KTO_M)]


@pytest.mark.parametrize("M,N,K,flag", _ALONE, ids=[f"{m}-{n}-{k}-{_FLAG_IDS[f]}" for m, n, k, f in _ALONE])
def test_gemm_k_range_flag_alone(dev, M, N, K, flag):
    """Every tile is computed, every K loop cut down to where the triangular operand is not zero: C is the exact product."""
    rng = np.random.default_rng(M * 11 + N * 5 + flag)
    A, B = _operands(rng, M, N, K, flag)
    ref = A @ B.T
    for alpha in (1.0, 0.5):
        Cm = _both_mask_forms(dev, A, B, alpha, flag)
        assert np.array_equal(Cm, alpha * ref)


@pytest.mark.parametrize("flag", [KFROM_N, KTO_N], ids=["kfrom_n", "kto_n"])
@pytest.mark.parametrize("n", [300, 385, 400, 130])
def test_gemm_k_range_lower_tiles_mirrored(dev, n, flag):
    """K range | TRI_LOWER | C_MIRROR on a product that is NOT symmetric: which side every 128-tile came from."""
    from loraine_jl_amd import _capi
    rng = np.random.default_rng(n * 13 + flag)
    A, B = _operands(rng, n, n, n, flag)
    ref = A @ B.T
    below, dia, above = tiles128(n)
    sentinel = np.full((n, n), -7.25)
    for alpha in (1.0, 0.5):
        Cm = _both_mask_forms(dev, A, B, alpha, flag | _capi.GEMM_TRI_LOWER | _capi.GEMM_C_MIRROR, Cin=sentinel)
        assert np.array_equal(Cm[below], alpha * ref[below])
        assert np.array_equal(Cm[dia], alpha * ref[dia])                 # diagonal tiles: both triangles as computed
        assert np.array_equal(Cm[above], alpha * ref.T[above])           # = the transpose of the lower tiles


@pytest.mark.parametrize("n", [300, 385, 400, 130])
def test_gemm_kfrom_m_lower_tiles(dev, n):
    """KFROM_M | TRI_LOWER (GEMM2' without its packed store): lower tiles exact, the tiles above keep Cin bit for bit."""
    from loraine_jl_amd import _capi
    rng = np.random.default_rng(n * 17)
    A, B = _operands(rng, n, n, n, KFROM_M)
    ref = A @ B.T
    below, dia, above = tiles128(n)
    sentinel = np.full((n, n), -7.25)
    for alpha in (1.0, 0.5):
        Cm = _both_mask_forms(dev, A, B, alpha, KFROM_M | _capi.GEMM_TRI_LOWER, Cin=sentinel)
        assert np.array_equal(Cm[below | dia], alpha * ref[below | dia])
        assert np.array_equal(Cm[above], sentinel[above])


@pytest.mark.parametrize("M,N,K,flags,beta,ksplit", [
    (300, 300, 200, KFROM_N, 0.0, 1),               # KFROM_N with N > K
    (300, 300, 200, KTO_M, 0.0, 1),                 # KTO_M with M > K
    (300, 300, 300, KFROM_M, 0.0, 3),               # a K range cannot be split
    (300, 300, 300, KTO_N, 0.0, 3),
    (300, 300, 300, 4096, 0.0, 1),                  # C_MIRROR without a TRI flag
    (300, 300, 300, 4096 | 1, 0.5, 1),              # C_MIRROR with beta != 0
], ids=["kfrom_n_N_gt_K", "kto_m_M_gt_K", "kfrom_m_ksplit3", "kto_n_ksplit3", "mirror_without_tri", "mirror_beta"])
def test_gemm_refuses(dev, M, N, K, flags, beta, ksplit):
    """LRN_ERR_ARG from the planner, nothing launched: C comes back as it went in."""
    from loraine_jl_amd import _capi
    rng = np.random.default_rng(3)
    A = _capi.f64(ints(rng, M, K)); B = _capi.f64(ints(rng, N, K))
    Cm = np.full((M, N), -7.25, order="F")
    rc = dev.lib.lrn_dbg_gemm(dev.h, 0, 1, M, N, K, 1.0, _capi.ptr(A), M, _capi.ptr(B), N, beta, _capi.ptr(Cm), M, flags, ksplit)
    assert rc == -1
    assert np.all(Cm == -7.25)


# ================================================================== 2. the product layer through lrn_dbg_product
def poison_slabs(dev, A, Bm):
    """Stale-slab guard (module docstring).  At 1300 the full product is not split (tests/test_gemm_plan_cpu.py) while the
    lower tiles come as 2 slabs of 1300^2 doubles: the three slabs of a product of side 1100 cover those (3 x 1100^2 >
    2 x 1300^2), and the buffer is not reallocated in between (it only grows)."""
    n = A.shape[0]
    if not 256 <= n < BIG_TILE_MIN_N:
        return
    for m in ((n, 1100) if n == 1300 else (n,)):
        dev.dbg_product(3, np.ldexp(A[:m, :m], 40), np.ldexp(Bm[:m, :m], 40))


@pytest.mark.parametrize("n", [33, 64, 130, 255, 256, 300, 385, 481, 650, 1300, 1500, 1501, 1502])
def test_sym_product(dev, n):
    """pgemm_nt_sym: one product + slabs_sym_kernel (n < 256), lower slabs + slabs_symlow_kernel (256 .. 1499),
    TRI_LOWER | C_MIRROR + mirror_diag_tiles_kernel (from 1500)."""
    A = ints(np.random.default_rng(n), n, n)
    poison_slabs(dev, A, A)
    out0, _, _ = dev.dbg_product(1, A, A, alpha=0.5)
    assert np.array_equal(out0, out0.T)
    assert np.array_equal(out0, 0.5 * (A @ A.T))


@pytest.mark.parametrize("tri", [KTO_N, KFROM_N], ids=["kto_n", "kfrom_n"])
@pytest.mark.parametrize("n", [1500, 1501, 1502])
def test_sym_product_triangular_operand(dev, n, tri):
    """What W = Pm L_X' relies on: A dense, Bm triangular with the hint -- the lower triangle of the product, mirrored.  At
    1501 (odd) the hint is dropped and the same call gives the same answer."""
    rng = np.random.default_rng(n + tri)
    A = ints(rng, n, n)
    Bm = np.tril(ints(rng, n, n)) if tri == KTO_N else np.triu(ints(rng, n, n))
    ref = 0.5 * (A @ Bm.T)
    out0, _, _ = dev.dbg_product(1, A, Bm, alpha=0.5, tri=tri)
    assert np.array_equal(np.tril(out0), np.tril(ref))
    assert np.array_equal(out0, out0.T)
    if n & 1:
        plain, _, _ = dev.dbg_product(1, A, Bm, alpha=0.5)
        assert np.array_equal(out0, plain)


@pytest.mark.parametrize("with_ct", [False, True], ids=["c", "c_ct"])
@pytest.mark.parametrize("n", [100, 300, 801, 1500, 1501, 1502])
def test_plain_product(dev, n, with_ct):
    """pgemm_nt with and without its transposed copy."""
    rng = np.random.default_rng(n * 3 + with_ct)
    A = ints(rng, n, n); Bm = ints(rng, n, n)
    poison_slabs(dev, A, Bm)
    out0, out1, _ = dev.dbg_product(0, A, Bm, alpha=0.5, want_out1=with_ct)
    assert np.array_equal(out0, 0.5 * (A @ Bm.T))
    if with_ct:
        assert np.array_equal(out1, out0.T)
    else:
        assert out1 is None


@pytest.mark.parametrize("with_ct", [False, True], ids=["c", "c_ct"])
@pytest.mark.parametrize("tri", [KFROM_M, KTO_M], ids=["kfrom_m", "kto_m"])
@pytest.mark.parametrize("n", [1500, 1502])
def test_plain_product_triangular_operand(dev, n, tri, with_ct):
    rng = np.random.default_rng(n * 5 + tri)
    A = np.triu(ints(rng, n, n)) if tri == KFROM_M else np.tril(ints(rng, n, n))
    Bm = ints(rng, n, n)
    out0, out1, _ = dev.dbg_product(0, A, Bm, tri=tri, want_out1=with_ct)
    assert np.array_equal(out0, A @ Bm.T)
    if with_ct:
        assert np.array_equal(out1, out0.T)


@pytest.mark.parametrize("tri", [KFROM_M, KTO_M], ids=["kfrom_m", "kto_m"])
def test_plain_product_ignores_the_hint_below_the_border(dev, tri):
    n = 300
    rng = np.random.default_rng(tri)
    A = np.triu(ints(rng, n, n)) if tri == KFROM_M else np.tril(ints(rng, n, n))
    Bm = ints(rng, n, n)
    poison_slabs(dev, A, Bm)
    hinted, hinted_t, _ = dev.dbg_product(0, A, Bm, tri=tri)
    plain, plain_t, _ = dev.dbg_product(0, A, Bm)
    assert np.array_equal(hinted, A @ Bm.T)
    assert np.array_equal(hinted, plain) and np.array_equal(hinted_t, plain_t)


@pytest.mark.parametrize("n", sorted(FULL_SPLIT))
def test_slabs_to_c_and_ct(dev, n):
    """gemm_nt_slabs + slabs_to_c_and_ct; *scalar proves the slab route ran (1 at 255 and at 1300: C in place)."""
    rng = np.random.default_rng(n * 7)
    A = ints(rng, n, n); Bm = ints(rng, n, n)
    poison_slabs(dev, A, Bm)
    out0, out1, nslab = dev.dbg_product(3, A, Bm, alpha=0.5)
    assert nslab == FULL_SPLIT[n]
    assert np.array_equal(out0, 0.5 * (A @ Bm.T))
    assert np.array_equal(out1, out0.T)


def ulps(x, ref):
    """|x - ref| in units of the spacing of float64 at ref (ref: np.longdouble)"""
    r64 = ref.astype(np.float64)
    return np.max(np.abs(x.astype(np.longdouble) - ref) / np.spacing(np.maximum(np.abs(r64), np.finfo(np.float64).tiny)))


def ns_formulas(P, a):
    """T = a (3 I - a^2 P) / 2 and ||I - P||_F^2 in np.longdouble"""
    P = P.astype(np.longdouble)
    a = np.longdouble(a)
    I = np.eye(P.shape[0], dtype=np.longdouble)
    return 1.5 * a * I - 0.5 * a * a * a * P, ((I - P) ** 2).sum()


@pytest.mark.parametrize("n", [64, 255, 256, 300, 385, 481, 650])
def test_newton_schulz_pass(dev, n):
    """gemm_nt_sym_ns (C == nullptr): T and ||I - P||_F^2 fused into the slab addition.  P = A A' is an integer matrix:
    with a = 1 every term of both is exact; a = 0.8125 = 13 / 16 within 2 ulp (the device may or may not contract the
    multiply-subtract)."""
    A = ints(np.random.default_rng(n * 19), n, n)
    P = A @ A.T
    poison_slabs(dev, A, A)
    T, _, res = dev.dbg_product(2, A, A, a=1.0)
    assert np.array_equal(T, 1.5 * np.eye(n) - 0.5 * P)
    assert res == ((np.eye(n) - P) ** 2).sum()
    poison_slabs(dev, A, A)
    T, _, res = dev.dbg_product(2, A, A, a=0.8125)
    Tref, _ = ns_formulas(P, 0.8125)
    assert ulps(T, Tref) <= 2
    assert res == ((np.eye(n) - P) ** 2).sum()


def test_newton_schulz_pass_realistic(dev):
    """A = Z, Bm = Y' with Z Y ~ I (the inverse square root and square root of a random SPD matrix): T and the residual
    against the formulas applied to pgemm_nt_sym's product of the same operands.  a = 13 / 16: 1.5 a and a^3 / 2 are exact in
    float64, what is left is the rounding of one multiply-subtract (2 ulp); the residual is a sum of n^2 non-negative
    terms, so any order agrees to n^2 2^-53 relative."""
    n = 300
    rng = np.random.default_rng(300)
    G = rng.standard_normal((n, n + 20))
    lam, V = np.linalg.eigh(G @ G.T / n + 0.1 * np.eye(n))
    Z = (V / np.sqrt(lam)) @ V.T
    Y = (V * np.sqrt(lam)) @ V.T
    poison_slabs(dev, Z, Y.T)
    P, _, _ = dev.dbg_product(1, Z, Y.T)
    assert np.array_equal(P, P.T) and relerr(P, np.eye(n)) < 1e-12
    poison_slabs(dev, Z, Y.T)
    T, _, res = dev.dbg_product(2, Z, Y.T, a=0.8125)
    Tref, res_ref = ns_formulas(P, 0.8125)
    assert ulps(T, Tref) <= 2
    assert abs(np.longdouble(res) - res_ref) <= n * n * 2.0 ** -53 * res_ref


@pytest.mark.parametrize("a", [0.5, 1.0])
@pytest.mark.parametrize("n", [100, 300, 650, 1100])
def test_symadd_of_a_product(dev, n, a):
    """prod_slabs + symadd_kernel with its fused <p, Ap> partials; 1100: 35^2 = 1225 tile pairs on 1024 workgroups (the
    grid-stride loop) over three slabs."""
    rng = np.random.default_rng(n * 23)
    A = ints(rng, n, n); Bm = ints(rng, n, n)
    poison_slabs(dev, A, Bm)
    out0, _, dot = dev.dbg_product(4, A, Bm, a=a)
    P = A @ Bm.T
    ref = a * (P + P.T)
    assert np.array_equal(out0, out0.T)
    assert np.array_equal(out0, ref)
    assert dot == (A * ref).sum()


# ---- round-off: standard-normal operands at side 300 against np.longdouble products, with the bound the GEMM tests of
# test_gpu_blocks.py use for these kernels
@pytest.fixture(scope="module")
def normal300():
    n = 300
    rng = np.random.default_rng(2024)
    A = rng.standard_normal((n, n)); Bm = rng.standard_normal((n, n))
    Al = A.astype(np.longdouble)
    PL = Al @ Bm.astype(np.longdouble).T          # A Bm'
    PS = Al @ Al.T                                # A A': symmetric in exact arithmetic
    for x in (A, Bm, PL, PS):
        x.setflags(write=False)
    return A, Bm, PL, PS


BOUND300 = 1e-14 * max(8, np.sqrt(300))


def test_roundoff_plain_product(dev, normal300):
    A, Bm, PL, _ = normal300
    poison_slabs(dev, A, Bm)
    out0, out1, _ = dev.dbg_product(0, A, Bm, alpha=0.75)
    assert relerr(out0, 0.75 * PL) < BOUND300
    assert np.array_equal(out1, out0.T)


def test_roundoff_sym_product(dev, normal300):
    A, _, _, PS = normal300
    poison_slabs(dev, A, A)
    out0, _, _ = dev.dbg_product(1, A, A, alpha=0.75)
    assert np.array_equal(out0, out0.T)
    assert relerr(out0, 0.75 * PS) < BOUND300


def test_roundoff_newton_schulz_pass(dev, normal300):
    """T inherits the relative error of P; the residual s = ||I - P||_F^2 moves by 2 ||I - P|| ||dP||, twice the relative
    error of P (||I - P|| ~ ||P|| here), plus at most n^2 2^-53 from adding its n^2 non-negative terms in any order."""
    A, _, _, PS = normal300
    n = A.shape[0]
    poison_slabs(dev, A, A)
    T, _, res = dev.dbg_product(2, A, A, a=0.8125)
    Tref, res_ref = ns_formulas(PS, 0.8125)
    assert relerr(T, Tref) < BOUND300
    assert abs(np.longdouble(res) - res_ref) < (2 * BOUND300 + n * n * 2.0 ** -53) * res_ref


def test_roundoff_slabs_to_c_and_ct(dev, normal300):
    A, Bm, PL, _ = normal300
    poison_slabs(dev, A, Bm)
    out0, out1, nslab = dev.dbg_product(3, A, Bm, alpha=0.75)
    assert nslab == FULL_SPLIT[300]
    assert relerr(out0, 0.75 * PL) < BOUND300
    assert np.array_equal(out1, out0.T)


def test_roundoff_symadd_of_a_product(dev, normal300):
    """The dot product <A, out0> is a signed sum: its error is measured against sum |A| |out0| -- the error out0 carries
    plus at most n^2 2^-53 from the order of the additions."""
    A, Bm, PL, _ = normal300
    n = A.shape[0]
    poison_slabs(dev, A, Bm)
    out0, _, dot = dev.dbg_product(4, A, Bm, a=0.5)
    ref = 0.5 * (PL + PL.T)
    assert np.array_equal(out0, out0.T)
    assert relerr(out0, ref) < BOUND300
    Al = A.astype(np.longdouble)
    assert abs(np.longdouble(dot) - (Al * ref).sum()) < (BOUND300 + n * n * 2.0 ** -53) * (np.abs(Al) * np.abs(ref)).sum()


def test_product_entry_refuses_bad_arguments(dev):
    from loraine_jl_amd import _capi
    n = 40
    A = _capi.f64(np.eye(n)); out = np.zeros((n, n), order="F"); s = C.c_double(0.0)
    p = _capi.ptr

    def call(kind=0, n=n, A=A, Bm=A, tri=0, out0=out, out1=out, scalar=C.byref(s)):
        return dev.lib.lrn_dbg_product(dev.h, kind, n, p(A), p(Bm), 1.0, 1.0, tri, p(out0), p(out1), scalar)

    assert call() == 0
    assert call(kind=5) == -1 and call(kind=-1) == -1
    assert call(n=0) == -1
    assert call(A=None) == -1 and call(Bm=None) == -1 and call(out0=None) == -1
    assert call(kind=3, out1=None) == -1
    assert call(kind=2, scalar=None) == -1
    assert call(tri=1) == -1 and call(tri=KFROM_M | KTO_M) == -1 and call(tri=4096) == -1
    for tri in (KFROM_M, KFROM_N, KTO_M, KTO_N):
        assert call(tri=tri) == 0
