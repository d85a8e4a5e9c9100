"""Seeded, designed inputs of tests/test_chol_cases_cpu.py and tests/test_gpu_chol.py, and their np.longdouble references:
the Cholesky factorisation, its pivot boosting and the triangular solves of csrc/chol.hip, entry by entry.

(a) spd(n, kind), n in SIZES -- the edges of the code, not of the workload: one diagonal launch (n <= 64), the first and
    last column of an 8-column panel, ragged last blocks of 1, 3 and 8 columns, both sides of POTRS_SMALL = 512, a full, a
    64-aligned and a ragged last 256-row super-block.  "benign": M M' / n + 1e-3 I.  "graded": D Q Lambda Q' D, Q a dense
    random orthogonal matrix, Lambda log-spaced over 1e12, D log-spaced over 1e6 in random order.  with_nan_upper() fills
    the strict upper triangle, which the library documents as scratch, with NaN: a read of it that reaches an output shows.
    The condition number that decides how hard a Cholesky factorisation is, is the one after the diagonal scaling is taken
    out (van der Sluis; Higham, Thm 10.5 ff.): core_condition() is cond_2 of D^-1 A D^-1 from the float64 entries of A, and
    lies in [1e11, 1e13].  cond_2 of A itself is beyond 1e18 for a dense Q (the scaling alone, D^2, spans 1e12) and is no
    number longdouble can measure.  Every exact pivot is positive.
(b) trsm: TRSM_N x NRHS x both `trans`: the one-thread-per-column kernel up to its limit (nrhs 1, 2, 15), the first MFMA
    strip (16), a ragged strip (17), a ragged 64-group (63, 65), a second workgroup (257), a ragged last diagonal block.
(c) boosting: boost_case(name).  H = L0 diag(D) L0' with L0 unit lower triangular, entries of a few bits, so that H is
    exact in float64 and pivot j of an unboosted elimination is D_j.  A planted row j has sum_k l_jk^2 D_k = s_j, so
    d0 = H_jj = s_j + D_j and the ratio piv / d0 is D_j / (s_j + D_j):
      kept   D_j = 2^-10 s_j   (ratio 1e-3 at pivot_boost = 1e-6: a thousand times the threshold)
      1e-8   D_j = 2^-27 s_j   (7.5e-9: boosted)        0   D_j = 0        -1e-8   D_j = -2^-27 s_j
      noise  D_j = 0 with row j of L0 D^1/2 a copy of an earlier row, at the default pivot_boost = 1e-12: H has a
             repeated row, the device's pivot is rounding noise, at most 2 gamma_n d0 < 1e-12 d0 for n <= 577
    (the kept ratio is 2^-10 and not 1e-4: a pivot of r d0 makes cond_2(H_RR) >= 4 / r whatever the rest of the matrix,
    and the error bound of the solve below is derived for cond_2(H_RR) <= 1e4).
    Column 0 cannot be boosted under the rules (its pivot is its d0); case c0 plants column 1, whose row hangs on column 0.

References, all np.longdouble from the float64 inputs: ref_factor() restates the pivot rules from the comment block at the
head of csrc/chol.hip and of schur_factor (csrc/schur.hip) -- boosted when piv <= boost d0, only where d0 > 0, never a
NaN, replaced by 1e40 max(|d0|, 1), counted, abandoned beyond max(8, n / 64) for the strict factorisation to decide.
Matrix products go through exact_matmul (float64 slices whose products are exact, added in longdouble; what it leaves
out is returned and counted as error).  Bounds are componentwise, gamma_k = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and
Stability, Thm 8.5, 10.3, 10.4), with k = n + 8: the 8 for v_rsq-based square roots and reciprocals of a few ulp and
the summation order of the MFMA.
"""
import functools
import types

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
SIZES = [1, 8, 9, 63, 64, 65, 72, 128, 129, 451, 512, 513, 577, 768, 769, 1025]
KINDS = ["benign", "graded"]
TRSM_N = [1, 63, 64, 65, 130, 451]
NRHS = [1, 2, 15, 16, 17, 63, 64, 65, 257]


def gamma(k):
    k = LD(k)
    return k * U / (1 - k * U)


# ------------------------------------------------------------------------------------------------ (a) SPD matrices
@functools.lru_cache(maxsize=None)
def _spd(n, kind):
    rng = np.random.default_rng(7000 + n + (50000 if kind == "graded" else 0))
    if kind == "benign":
        M = rng.standard_normal((n, n + 3))
        A = M @ M.T / n + 1e-3 * np.eye(n)
        d = np.ones(n)
    else:
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        lam = 10.0 ** (-12.0 * np.arange(n) / max(n - 1, 1))
        d = 10.0 ** (-3.0 + 6.0 * rng.permutation(n) / max(n - 1, 1))
        B = (Q * lam) @ Q.T
        A = d[:, None] * B * d[None, :]
    A = np.tril(A) + np.tril(A, -1).T                              # exactly symmetric, whatever the BLAS does
    A.setflags(write=False)
    d.setflags(write=False)
    return A, d


def spd(n, kind):
    """The float64 matrix (symmetric, full; shared, read-only)."""
    return _spd(n, kind)[0]


def spd_scaling(n, kind):
    return _spd(n, kind)[1]


def with_nan_upper(A):
    A = np.array(A, dtype=np.float64, order="F")
    A[np.triu_indices(A.shape[0], 1)] = np.nan
    return A


@functools.lru_cache(maxsize=None)
def rhs(n, nrhs=1):
    B = np.random.default_rng(9000 + n).standard_normal((n, max(NRHS)))[:, :nrhs].copy(order="F")
    B.setflags(write=False)
    return B


# ------------------------------------------------------------------------------------------------ longdouble tools
def chol_ld(A):
    """Lower Cholesky factor of the lower triangle of A in longdouble, column by column (left-looking); -> (L, pivots);
    a pivot that is not positive ends it (the columns from there on stay zero)."""
    A = np.asarray(A)
    n = A.shape[0]
    Al = A.astype(LD)
    L = np.zeros((n, n), dtype=LD)
    piv = np.full(n, np.nan, dtype=LD)
    for j in range(n):
        c = Al[j:, j] - L[j:, :j] @ L[j, :j]
        piv[j] = c[0]
        if not c[0] > 0:
            break
        s = np.sqrt(c[0])
        L[j:, j] = c / s
        L[j, j] = s
    return L, piv


def solve_ld(L, b, trans=None):
    """L'\\(L\\b) in longdouble (trans False / True: only L\\b / L'\\b)."""
    n = L.shape[0]
    x = np.array(b, dtype=LD)
    if trans in (None, False):
        for i in range(n):
            x[i] = (x[i] - L[i, :i] @ x[:i]) / L[i, i]
    if trans in (None, True):
        for i in range(n - 1, -1, -1):
            x[i] = (x[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def cond_ld(A):
    """cond_2 of a symmetric positive definite matrix (lower triangle) in longdouble: power iteration for the largest
    eigenvalue, inverse iteration through the longdouble factor for the smallest; -> (cond, smallest pivot)."""
    n = A.shape[0]
    Al = np.tril(A).astype(LD)
    Al = Al + np.tril(Al, -1).T
    L, piv = chol_ld(Al)
    if not (piv > 0).all():
        return np.inf, float(np.nanmin(piv))
    rng = np.random.default_rng(1)
    v, A64, lmax = rng.standard_normal(n), Al.astype(np.float64), 0.0
    for _ in range(300):                                           # (float64 is enough for the largest eigenvalue)
        v = A64 @ v
        lmax = np.sqrt(v @ v)
        v /= lmax
    lmax = LD(lmax)
    w = rng.standard_normal(n).astype(LD)
    mu = LD(0)
    for _ in range(12):
        w = solve_ld(L, w)
        mu = np.sqrt(w @ w)
        w /= mu
    return float(lmax * mu), float(piv.min())


def core_condition(n, kind):
    """(cond_2 of D^-1 A D^-1, smallest exact pivot of A), from the float64 entries of A, in longdouble."""
    A, d = _spd(n, kind)
    dl = d.astype(LD)
    core = A.astype(LD) / dl[:, None] / dl[None, :]
    return cond_ld(core)[0], float(chol_ld(A)[1].min())


def exact_matmul(A, B, nbits=20, slices=5, balance=False):
    """(A @ B in longdouble, what was left out), as exact_matmul of tests/sparse_ops_cases.py: rows of A and columns of B
    cut into slices of nbits bits below the row's (column's) largest power of two; every product of two slices is exact in
    float64 for K < 2^(52 - 2 nbits); those with i + j < slices are added in longdouble, smallest first.  Left out: the
    pairs with i + j >= slices and the remainders, below 16 K 2^(-nbits slices) rowscale colscale.  balance: the inner
    index is first scaled by the power of two at each row's largest entry of B (exact: A S times S^-1 B), so that what is
    left out is small against sum_k |a_ik| max_j |b_kj| -- for the solution of a graded triangular system, whose entries
    span many orders down one column."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    K = A.shape[1]
    if balance and B.size:
        mx = np.abs(B).max(axis=1)
        s = 2.0 ** np.ceil(np.log2(np.where(mx > 0, mx, 1.0)))
        A, B = A * s[None, :], B / s[:, None]
    assert K * 2.0 ** (2 * nbits + 2) <= 2.0 ** 53

    def cut(X, axis):
        mx = np.abs(X).max(axis=axis, keepdims=True) if X.size else np.ones((1, 1))
        scale = 2.0 ** np.ceil(np.log2(np.where(mx > 0, mx, 1.0)))
        out, r = [], X.copy()
        for i in range(slices):
            unit = scale * 2.0 ** (-nbits * (i + 1))
            hi = np.rint(r / unit) * unit
            out.append(hi)
            r = r - hi
        return out, scale

    (As, sa), (Bs, sb) = cut(A, 1), cut(B, 0)
    C = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for s in range(slices - 1, -1, -1):
        for i in range(s + 1):
            C += (As[i] @ Bs[s - i]).astype(LD)
    left = (sa.astype(LD) * sb.astype(LD)) * LD(16 * K) * LD(2.0) ** (-nbits * slices)
    return C, left


def _worst(err, bound):
    """largest err / bound (inf where a bound of 0 is exceeded or something is not finite)"""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    if err.size == 0:
        return 0.0
    if not (np.isfinite(err).all() and np.isfinite(bound).all()):
        return np.inf
    pos = bound > 0
    if (err[~pos] > 0).any():
        return np.inf
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


# ------------------------------------------------------------------------------------------------ the checks
# Each returns err / (u B) at its worst component, B the absolute-value product of the bound: the assertion is
#   ratio <= limit(n), with gamma_{n+8} / u for potrf and trsm and (2 gamma + gamma^2) / u for potrs.
def limit(n, op):
    g = gamma(n + 8)
    return float((2 * g + g * g) / U) if op == "potrs" else float(g / U)


def check_potrf(Lh, A):
    """|L L' - A| <= gamma_{n+8} |L||L'| on the lower triangle (Thm 10.3); -> worst err / (u |L||L'|)"""
    Lh = np.asarray(Lh)
    if not np.isfinite(Lh).all():
        return np.inf
    Lh = np.tril(Lh)
    P, left = exact_matmul(Lh, Lh.T)
    Bd, _ = exact_matmul(np.abs(Lh), np.abs(Lh.T))
    il = np.tril_indices(Lh.shape[0])
    Al = np.tril(np.nan_to_num(np.asarray(A, dtype=np.float64), nan=0.0)).astype(LD)
    err = (np.abs(np.tril(P) - Al) + np.tril(left))[il]
    return _worst(err, U * Bd[il])


def check_trsm(Lh, X, B, trans):
    """|op(L) X - B| <= gamma_{n+8} |op(L)||X| (Thm 8.5); -> worst err / (u |op(L)||X|)"""
    X = np.asarray(X)
    if not np.isfinite(X).all():
        return np.inf
    T = np.tril(Lh).T if trans else np.tril(Lh)
    P, left = exact_matmul(T, X, balance=True)
    Bd, _ = exact_matmul(np.abs(T), np.abs(X), balance=True)
    return _worst(np.abs(P - np.asarray(B).astype(LD)) + left, U * Bd)


def check_same_solution(Lh, x1, x2, trans):
    """Two computed solutions of the same triangular system, each within the bound of check_trsm:
    |op(L)(x1 - x2)| <= gamma_{n+8} |op(L)|(|x1| + |x2|); -> worst err / (u |op(L)|(|x1| + |x2|))"""
    T = (np.tril(Lh).T if trans else np.tril(Lh)).astype(LD)
    x1, x2 = np.asarray(x1).astype(LD), np.asarray(x2).astype(LD)
    if not (np.isfinite(x1).all() and np.isfinite(x2).all()):
        return np.inf
    return _worst(np.abs(T @ (x1 - x2)), U * (np.abs(T) @ (np.abs(x1) + np.abs(x2))))


def check_potrs(Lh, x, b):
    """|b - L L' x| <= (2 gamma_{n+8} + gamma_{n+8}^2) |L||L'||x| (Thm 10.4's backward error, as a residual);
    -> worst err / (u |L||L'||x|)"""
    x = np.asarray(x)
    if not np.isfinite(x).all():
        return np.inf
    Ll = np.tril(Lh).astype(LD)
    xl = x.astype(LD)
    r = np.asarray(b).astype(LD) - Ll @ (Ll.T @ xl)
    Bd = np.abs(Ll) @ (np.abs(Ll.T) @ np.abs(xl))
    return _worst(np.abs(r), U * Bd)


# ------------------------------------------------------------------------------------------------ (c) boosting
BOOST_PLANTED = 1e-6
BOOST_DEFAULT = 1e-12
_POS = {                                                             # name -> (n, planted columns)
    "c0": (130, [1]), "c5": (130, [5]), "c63": (130, [63]), "c64": (130, [64]), "c70": (130, [70]),
    "q0": (130, [72]), "q7": (130, [79]), "q0q7": (130, [72, 79]),
    "ragged": (451, [450]), "single": (40, [20]), "super": (577, [530]),
}
VARIANTS = ["kept", "1e-8", "0", "-1e-8", "noise"]
_NEG200 = [3, 40, 63, 64, 100, 127, 130, 190, 199]
_NEG577 = [3, 63, 64, 130, 255, 256, 400, 520, 576]
SPECIAL = {"neg8": (200, _NEG200[:8]), "neg9": (200, _NEG200), "neg9_577": (577, _NEG577),
           "zero_row": (130, [70]), "nan_diag": (130, [70])}
BOOST_NAMES = ["%s/%s" % (p, v) for p in _POS for v in VARIANTS] + list(SPECIAL)
BOOST_N = {name: (SPECIAL[name][0] if name in SPECIAL else _POS[name.split("/")[0]][0]) for name in BOOST_NAMES}


def max_boost(n):
    return max(8, n // 64)


def _ldl(n, planted, code, seed):
    """H = L0 diag(D) L0' exactly in float64; planted: columns, code: what D_j is there.  Generic rows: two entries of
    +-1/8 in earlier columns; a planted row: four entries of +-1/2 (one entry of 1 where fewer than four columns come
    before it) in generic columns, none in planted ones; the six rows after a planted column hold an entry in it."""
    rng = np.random.default_rng(seed)
    pl = set(planted)
    L0 = np.eye(n)
    D = rng.choice([1.0, 2.0], n)
    for i in range(1, n):
        gen = [k for k in range(i) if k not in pl]
        if i in pl:
            ks = rng.choice(gen, 4, replace=False) if len(gen) >= 4 else [gen[-1]]
            for k in ks:
                L0[i, k] = (0.5 if len(gen) >= 4 else 1.0) * rng.choice([-1.0, 1.0])
        else:
            for k in rng.choice(i, min(2, i), replace=False):
                L0[i, k] = 0.125 * rng.choice([-1.0, 1.0])
            for j in planted:
                if j < i <= j + 6:
                    L0[i, j] = 0.125 * rng.choice([-1.0, 1.0])
    for j in planted:
        if code == "noise":                                        # row j of L0 D^1/2 = row i of it, i generic
            i = max(k for k in range(j) if k not in pl)
            L0[j, :] = 0.0
            L0[j, :i + 1] = L0[i, :i + 1]
            L0[j, j] = 1.0
        if code == "zero_row":
            L0[j, :j] = 0.0
            L0[j + 1:, j] = 0.0
        s = float((L0[j, :j] ** 2) @ D[:j])
        D[j] = {"kept": 2.0 ** -10 * s, "1e-8": 2.0 ** -27 * s, "0": 0.0, "-1e-8": -2.0 ** -27 * s, "noise": 0.0,
                "neg": -0.25 * s, "zero_row": 0.0, "nan_diag": 1.0}[code]
    H = (L0 * D) @ L0.T
    Hx = ((L0.astype(LD) * D.astype(LD)) @ L0.T.astype(LD))
    assert (Hx == H.astype(LD)).all()                              # exact in float64
    if code == "nan_diag":
        for j in planted:
            H[j, j] = np.nan
    return H


@functools.lru_cache(maxsize=None)
def boost_case(name):
    """Built once per process, shared, never modified: H (float64, full, symmetric), boost, the planted columns, and the
    reference results `ref` (with boosting), `strict` (pivot_boost = 0) and `shifted` (after lrn_schur_add_diag(SHIFT))."""
    if name in SPECIAL:
        n, cols = SPECIAL[name]
        code, boost = ("neg" if name.startswith("neg") else name), BOOST_DEFAULT
    else:
        pos, code = name.split("/")
        n, cols = _POS[pos]
        boost = BOOST_DEFAULT if code == "noise" else BOOST_PLANTED
    H = _ldl(n, cols, code, 100 + BOOST_NAMES.index(name))
    H.setflags(write=False)
    Hs = H + SHIFT * np.eye(n)
    return types.SimpleNamespace(name=name, n=n, H=H, boost=boost, cols=list(cols), code=code,
                                 ref=ref_schur(H, boost), strict=ref_schur(H, 0.0), shifted=ref_schur(Hs, 0.0))


SHIFT = 1e-300                                                       # changes no entry of H but an exact zero


def ref_factor(H, boost, limit_boost):
    """One factorisation attempt in longdouble, by the rules quoted above.  -> (info, boosted columns, L, ratios) with
    ratios[j] = piv / (boost d0) where the rule looks at it (boost > 0, d0 > 0), else NaN."""
    H = np.asarray(H)
    n = H.shape[0]
    A = np.tril(H).astype(LD)
    d0 = np.diag(H).astype(LD)
    L = np.zeros((n, n), dtype=LD)
    boosted, ratios = [], np.full(n, np.nan)
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        piv = c[0]
        if boost > 0 and d0[j] > 0:
            ratios[j] = float(piv / (LD(boost) * d0[j]))
            if piv <= LD(boost) * d0[j]:                           # (false for a NaN)
                boosted.append(j)
                if len(boosted) > limit_boost:
                    return j + 1, boosted, L, ratios
                piv = LD(1e40) * max(abs(d0[j]), LD(1))
        if not piv > 0:                                            # also a NaN
            return j + 1, boosted, L, ratios
        s = np.sqrt(piv)
        L[j:, j] = c / s
        L[j, j] = s
    return 0, boosted, L, ratios


def ref_schur(H, boost, h=None):
    """lrn_schur_factor and lrn_schur_solve: the attempt with boosting where boost > 0; if it fails, the strict
    factorisation decides (and nothing is counted).  -> info, count, boosted, ratios, x = (L L')^-1 h (h: all ones)."""
    n = H.shape[0]
    info, boosted, L, ratios = 1, [], None, np.full(n, np.nan)
    if boost > 0:
        info, boosted, L, ratios = ref_factor(H, boost, max_boost(n))
    if info != 0:
        info, boosted, L, _ = ref_factor(H, 0.0, 0)                # (boosts nothing)
    x = solve_ld(L, np.ones(n) if h is None else h) if info == 0 else None
    return types.SimpleNamespace(info=info, count=len(boosted), boosted=list(boosted), ratios=ratios, x=x)


@functools.lru_cache(maxsize=None)
def kept_reference(name):
    """For a case that factors: R (kept rows), x_ref = H_RR^-1 1 and the componentwise bound of Thm 10.4 to first order,
    2 gamma_{3n+8} |H_RR^-1| |L_ref||L_ref'||x_ref|, L_ref the longdouble factor of H_RR.  (|H_RR^-1| from a float64
    inverse: at cond <= 1e4 good to 1e-11, far inside the factor 2.)"""
    case = boost_case(name)
    assert case.ref.info == 0
    R = np.array([j for j in range(case.n) if j not in set(case.ref.boosted)])
    HRR = case.H[np.ix_(R, R)]
    L, piv = chol_ld(HRR)
    assert (piv > 0).all()
    x = solve_ld(L, np.ones(R.size))
    inv = np.abs(np.linalg.inv(HRR)).astype(LD)
    bound = 2 * gamma(3 * case.n + 8) * (inv @ (np.abs(L) @ (np.abs(L.T) @ np.abs(x))))
    return types.SimpleNamespace(R=R, x=x, bound=bound, HRR=HRR)


def kept_condition(name):
    """cond_2(H_RR) in longdouble"""
    return cond_ld(kept_reference(name).HRR)[0]


def check_boost_solve(name, x):
    """The solve with h = 1 of a case that factors: boosted rows |x_j| <= 1e-30 max(|h|_inf, |x_ref|_inf), kept rows within
    the bound of kept_reference; -> (largest |x_j| / that limit over the boosted rows, largest err / bound over the kept)"""
    case, k = boost_case(name), kept_reference(name)
    x = np.asarray(x)
    if not np.isfinite(x).all():
        return np.inf, np.inf
    small = LD(1e-30) * max(LD(1), np.abs(k.x).max())
    b = np.array(case.ref.boosted, dtype=np.int64)
    rb = float((np.abs(x[b].astype(LD)) / small).max()) if b.size else 0.0
    return rb, _worst(np.abs(x[k.R].astype(LD) - k.x), k.bound)


# ------------------------------------------------------------------------------------------------ float64 restatement
def f64_factor(H, boost=0.0, limit_boost=0, fault=None):
    """The same algorithm in float64, column by column, no blocking (right-looking), for tests/test_chol_cases_cpu.py: an
    honest implementation must meet every bound, and each planted `fault` must break one.  -> (info, count, L)"""
    H = np.asarray(H, dtype=np.float64)
    n = H.shape[0]
    A = np.tril(H).copy()
    d0 = np.diag(H).copy()
    count = 0
    for j in range(n):
        piv = A[j, j]
        dropped = False
        ref_d = piv if fault == "running_diagonal" else d0[j]
        if boost > 0:
            low = piv < boost * ref_d if fault == "strict_less" else piv <= boost * ref_d
            eligible = ref_d > 0 or (fault == "boost_empty_row" and ref_d == 0)
            if (eligible and low) or (fault == "boost_nan" and piv != piv):
                count += 1
                if count > limit_boost - (1 if fault == "limit_off_by_one" else 0):
                    return j + 1, count, A
                piv = 1e40 * max(abs(d0[j]), 1.0) if d0[j] == d0[j] else 1e40
                dropped = True
        if not piv > 0:
            return j + 1, count, A
        s = np.sqrt(piv)
        col = A[j + 1:, j] / (1.0 if (dropped and fault == "column_not_dropped") else s)
        A[j, j] = s
        A[j + 1:, j] = col
        upd = np.tril(np.outer(col, col))
        if fault == "skip_block" and j < 8 and n > 48:              # rows and columns 32 .. 47 miss the first panel
            upd[31 - j:47 - j, 31 - j:47 - j] = 0.0
        if fault == "drop_fma" and j == 6 and n > 8:                # column 7 misses column 6 (q = 7 of the first panel)
            upd[:, 0] = 0.0
        A[j + 1:, j + 1:] -= upd
    return 0, count, A


def f64_trsm(L, B, trans, fault=None):
    """op(L) X = B by substitution in float64, one right-hand side per column; L as the device holds it (strict upper: NaN)"""
    n = L.shape[0]
    X = np.array(B, dtype=np.float64)
    T = np.array(L, dtype=np.float64) if fault == "upper_read" else np.tril(L)
    order = range(n - 1, -1, -1) if trans else range(n)
    ncol = X.shape[1] - (1 if fault == "last_rhs" else 0)
    for i in order:
        acc = T[i + 1:, i] @ X[i + 1:, :ncol] if trans else T[i, :i] @ X[:i, :ncol]
        if fault == "upper_read":                                   # the mirror entries too, with weight 0
            acc = acc + 0.0 * (T[:i, i].sum() if trans else T[i, i + 1:].sum())
        X[i, :ncol] = (X[i, :ncol] - acc) / T[i, i]
    return X


def f64_schur(H, boost, fault=None):
    """f64_factor as lrn_schur_factor runs it (attempt, then strict) and the solve with h = 1; -> (info, count, x)"""
    n = H.shape[0]
    info, count, L = f64_factor(H, boost, max_boost(n), fault) if boost > 0 else (1, 0, None)
    if boost <= 0 or info != 0:
        info, count, L = f64_factor(H, 0.0, 0, None)
    if info != 0:
        return info, count, None
    L = np.tril(L)
    with np.errstate(all="ignore"):
        x = f64_trsm(L, f64_trsm(L, np.ones((n, 1)), False), True)[:, 0]
    return info, count, x
