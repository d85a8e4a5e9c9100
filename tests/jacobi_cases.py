"""Seeded inputs, the np.longdouble reference, the bounds and a float64 restatement of csrc/jacobi.hip, for
tests/test_jacobi_cases_cpu.py and tests/test_gpu_jacobi.py: the one-sided Jacobi SVD column by column.

Inputs (make(family, n, param); all from np.random.default_rng, built once per process, read-only):
  graded   A = B diag(D): B = Q diag(logspace(0, -1, n)) Q2' with unit columns, D = logspace(0, g, n), g = -8, -12, -16, in a
           random permutation (every 16-, 32- or 64-column panel mixes magnitudes), or sorted ("desc", "asc", g = -12).
           kB = kappa_2 of the column-normalised input is 10.0 to 10.1.
  cluster  A = Q diag(d) Q2', d = three clusters of n/4 values at 1, 3 and 0.2 of relative width w, the rest spread over
           (0.2, 3); w = 1e-9 ... 1e-4.  Rotation angles inside a cluster are O(1) while the cosines are O(w): widths of
           1e-6 to 1e-5 sit just under the `s*s > 1e-4` flag of the early stop.  The bound of Demmel and Veselic holds
           for every column scaling A = B D; here kB is taken at D = I, kappa_2(A) = 15 (unit columns would give 17).
  rankdef  graded (g = -6) with one zero column, one exact duplicate and one column 0.5 a_j - a_k that is exact in float64
           (the two columns are first rounded to a common grid).
  orth     A = P diag(D), P a permutation matrix, D graded (g = -12) with random signs: orthogonal in exact arithmetic.
           (A QR factor is not: its cosines reach eps sqrt(n) at n ~ 100.)
  scaled   graded (g = -8) times 2^150 ("up") and 2^-150 ("down"), by np.ldexp: exact.

Reference: jacobi_cyclic(A, LD): a plain cyclic one-sided Jacobi with the rotation formula of jacobi_small_kernel in
np.longdouble, run until a sweep rotates nothing at its own threshold eps_ld sqrt(n); every round of the round-robin
ordering (n/2 disjoint pairs) at once.  Singular values are the final column norms (reference_sigma, cached).

Bounds (measure / limits), from the device's US, V, s and the input, all in longdouble.  u = 2^-53, eps = 2u,
tol = eps sqrt(max(n, 4)) (the documented threshold), kB = kappa_2(B), beta = n eps kB:
  sig    max_j |s_j - sref_j| / sref_j <= beta after sorting (Demmel and Veselic, Jacobi's method is more accurate than QR,
         1992: the relative error of one-sided Jacobi is governed by kappa(B), not kappa(A); dimensional factor n)
  res    ||A v_j - (US)_j||_2 <= beta s_j for every column j -- relative to that column's singular value, not to ||A||
  vorth  max |V'V - I| <= beta
  cos    the largest cosine between two columns of US: <= 4 tol when the last sweep rotated nothing (one-workgroup kernel
         always; blocked kernels under jacobi_early = 0): every pair passed |ga| <= tol sqrt(al be) on a freshly computed
         Gram matrix, whose own rounding is about tol.  Under the default jacobi_early = 3e-8 the cap is 2n 1e-2 early: in
         the last sweep every rotation has an angle of at most 1e-2 and every cosine is at most early, and an annihilated
         pair is re-perturbed by at most 2n later rotations.
  rankdef: 0 < sweeps < 40, the zero column exactly zero with s = 0.0, the two dependent directions s <= n eps s_max, every
         other s within n eps s_max of the reference (absolute: kB is infinite), vorth with kB of the case before planting.
  orth:  sweeps = 1, US = A, V = I and s = |D| bit for bit.

Float64 restatement: f64_small (= jacobi_cyclic in float64 at the device's threshold) and f64_blocked (panel Gram by row
chunks, jrot as written, full schedule in round 0 and cross pairs after it, R accumulated, panel times R, both stopping
rules, the driver's chunking).  An honest restatement must meet every bound on every case; each of FAULTS must break one.
"""
import functools
import types

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
JAC_SMALL = 96
MAX_SWEEPS = 40
EARLY = 3e-8
WIDTHS = [1e-9, 1e-7, 1e-6, 3e-6, 1e-5, 1e-4]
GRADES = [-8, -12, -16, "desc", "asc"]


def tol_of(n):
    return EPS * np.sqrt(float(max(n, 4)))


def rr_pairs(npl, rnd):
    """pairs (p < q) of round rnd of the round-robin tournament on npl (even) players, as rr_pair of csrc/jacobi.hip"""
    m = npl - 1
    k = np.arange(npl // 2)
    a = (rnd + k) % m
    b = (rnd - k + m) % m
    a[0], b[0] = m, rnd
    return np.minimum(a, b), np.maximum(a, b)


# ------------------------------------------------------------------------------------------------ inputs
def _orthogonal(rng, n):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return Q


def _unit_columns(B):
    return B / np.sqrt((B * B).sum(axis=0))[None, :]


def kappa_cols(A):
    """kappa_2 of A with its columns scaled to unit length (float64 SVD: the value is about 10)"""
    nz = np.abs(A).max(axis=0) > 0
    M = A[:, nz]
    e = np.floor(np.log2(np.abs(M).max(axis=0)))
    M = np.ldexp(M, -e.astype(np.int64)[None, :])                    # exact: keeps the scaled cases in range
    s = np.linalg.svd(_unit_columns(M), compute_uv=False)
    return float(s[0] / s[-1])


def _graded(n, g, seed):
    rng = np.random.default_rng(seed)
    B = _unit_columns((_orthogonal(rng, n) * np.logspace(0, -1, n)) @ _orthogonal(rng, n).T)
    perm = rng.permutation(n)
    if g == "desc":
        D = np.logspace(0, -12, n)
    elif g == "asc":
        D = np.logspace(0, -12, n)[::-1].copy()
    else:
        D = np.logspace(0, g, n)[perm]
    return B * D[None, :], D


def cluster_values(n, w, rng):
    """three clusters of n // 4 values of relative width w: around 1, below 3 and above 0.2 (so that max / min <= 15 at
    every width), and n - 3 (n // 4) values between them"""
    q = n // 4
    off = np.linspace(0.0, 1.0, q) if q > 1 else np.zeros(q)
    d = np.concatenate([1.0 + w * (off - 0.5), 3.0 * (1.0 - w * off), 0.2 * (1.0 + w * off),
                        np.geomspace(0.25, 2.5, n - 3 * q)])
    return d[rng.permutation(n)]


def rankdef_columns(n):
    """(zero column, (duplicate, its source), (combination, j, k)): column `combination` = 0.5 a_j - a_k"""
    return n // 3, (n - 1, 1), (n // 2, 2, n - 3)


@functools.lru_cache(maxsize=None)
def make(family, n, param=None):
    """-> namespace(A, kB, D, d): the float64 input (column-major, read-only) and kappa_2 of its column-normalised form"""
    out = types.SimpleNamespace(family=family, n=n, param=param, D=None, d=None)
    if family == "graded":
        A, out.D = _graded(n, param, 1000 + n + 7919 * GRADES.index(param))
        out.kB = kappa_cols(A)
    elif family == "scaled":
        A, out.D = _graded(n, -8, 1000 + n)
        out.kB = kappa_cols(A)
        A = np.ldexp(A, 150 if param == "up" else -150)
    elif family == "cluster":
        rng = np.random.default_rng(2000 + n + 7919 * WIDTHS.index(param))
        out.d = cluster_values(n, param, rng)
        A = (_orthogonal(rng, n) * out.d) @ _orthogonal(rng, n).T
        sv = np.linalg.svd(A, compute_uv=False)
        out.kB = float(sv[0] / sv[-1])                               # the scaling D = I: 15 (unit columns give 17)
    elif family == "rankdef":
        A, out.D = _graded(n, -6, 3000 + n)
        out.kB = kappa_cols(A)                                       # before the columns are planted
        z, (dup, src), (comb, j, k) = rankdef_columns(n)
        grid = 2.0 ** (np.floor(np.log2(min(np.abs(A[:, j]).max(), np.abs(A[:, k]).max()))) - 26)
        A[:, j] = np.rint(A[:, j] / grid) * grid
        A[:, k] = np.rint(A[:, k] / grid) * grid
        A[:, z] = 0.0
        A[:, dup] = A[:, src]
        A[:, comb] = 0.5 * A[:, j] - A[:, k]
    elif family == "orth":
        rng = np.random.default_rng(4000 + n)
        out.D = np.logspace(0, -12, n)[rng.permutation(n)] * rng.choice([-1.0, 1.0], n)
        out.perm = rng.permutation(n)
        A = np.zeros((n, n))
        A[out.perm, np.arange(n)] = out.D
        out.kB = 1.0
    else:
        raise ValueError(family)
    out.A = np.asfortranarray(A)
    out.A.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ cyclic Jacobi
def jacobi_cyclic(A, dtype=LD, tol=None, vectors=False, max_sweeps=200):
    """One-sided cyclic Jacobi in `dtype`, pairs in the round-robin order and the rotation formula of jacobi_small_kernel
    (zeta = (be - al) / (2 ga), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), c = 1 / sqrt(1 + t^2), s = c t); a round's
    disjoint pairs at once.  -> (US, V or None, column norms, sweeps); sweeps counts the last one, which rotated nothing."""
    A = np.asarray(A)
    n = A.shape[0]
    npl = n + (n & 1)
    a = np.zeros((npl, n), dtype=dtype)                              # row j = column j (a padding column is zero: it never
    a[:n] = A.T                                                      # rotates)
    v = np.eye(npl, dtype=dtype) if vectors else None
    if tol is None:
        tol = np.finfo(dtype).eps * np.sqrt(dtype(n))
    tol = dtype(tol)
    one, two = dtype(1), dtype(2)
    sweeps = 0
    with np.errstate(all="ignore"):
        while sweeps < max_sweeps:
            sweeps += 1
            rotated = False
            for rnd in range(npl - 1):
                p, q = rr_pairs(npl, rnd)
                x, y = a[p], a[q]
                al, be, ga = (x * x).sum(axis=1), (y * y).sum(axis=1), (x * y).sum(axis=1)
                rot = np.abs(ga) > tol * np.sqrt(al * be)
                if not rot.any():
                    continue
                rotated = True
                p, q, x, y, al, be, ga = p[rot], q[rot], x[rot], y[rot], al[rot], be[rot], ga[rot]
                zeta = (be - al) / (two * ga)
                t = np.where(zeta >= 0, one, -one) / (np.abs(zeta) + np.sqrt(one + zeta * zeta))
                c = one / np.sqrt(one + t * t)
                s = (c * t)[:, None]
                c = c[:, None]
                a[p], a[q] = c * x - s * y, s * x + c * y
                if vectors:
                    x, y = v[p], v[q]
                    v[p], v[q] = c * x - s * y, s * x + c * y
            if not rotated:
                break
    a = a[:n].T
    return a, (v[:n, :n].T if vectors else None), np.sqrt((a * a).sum(axis=0)), sweeps


@functools.lru_cache(maxsize=None)
def reference_sigma(family, n, param=None):
    """singular values of make(family, n, param).A by the longdouble Jacobi, sorted descending (longdouble, read-only).
    A power of two commutes with every operation of the method (far from over- and underflow), so the scaled cases take
    the values of the graded one times 2^+-150 -- tests/test_jacobi_cases_cpu.py checks that this is exact."""
    if family == "scaled":
        s = np.ldexp(reference_sigma("graded", n, -8), 150 if param == "up" else -150)
    else:
        s = np.sort(jacobi_cyclic(make(family, n, param).A, LD)[2])[::-1].copy()
    s.setflags(write=False)
    return s


# ------------------------------------------------------------------------------------------------ the bounds
def measure(A, US, V, s, sref=None):
    """-> namespace(sig, res, vorth, cos) in longdouble arithmetic (see the head of this file); an entry that cannot be
    measured (no V, no reference) is None, anything not finite gives inf."""
    A, US, s = np.asarray(A), np.asarray(US), np.asarray(s)
    out = types.SimpleNamespace(sig=None, res=None, vorth=None, cos=0.0)
    if not (np.isfinite(US).all() and np.isfinite(s).all() and (V is None or np.isfinite(V).all())):
        return types.SimpleNamespace(sig=np.inf, res=np.inf, vorth=np.inf, cos=np.inf)
    n = A.shape[0]
    Ul, sl = US.astype(LD), s.astype(LD)
    if sref is not None:
        ss = np.sort(sl)[::-1]
        out.sig = float((np.abs(ss - sref) / sref).max())
    if V is not None:
        Vl = np.asarray(V).astype(LD)
        r = np.sqrt(((A.astype(LD) @ Vl - Ul) ** 2).sum(axis=0))
        pos = sl > 0
        out.res = float((r[pos] / sl[pos]).max()) if pos.any() else 0.0
        if (r[~pos] > 0).any():
            out.res = np.inf
        out.vorth = float(np.abs(Vl.T @ Vl - np.eye(n, dtype=LD)).max())
    nrm = np.sqrt((Ul * Ul).sum(axis=0))
    keep = nrm > 0
    if keep.sum() > 1:
        Un = Ul[:, keep] / nrm[keep][None, :]
        G = np.abs(Un.T @ Un)
        np.fill_diagonal(G, 0)
        out.cos = float(G.max())
    return out


def limits(n, kB, confirmed, early=EARLY):
    """the bounds: beta for sig, res and vorth; for cos 4 tol after a sweep that rotated nothing (`confirmed`), else the
    cap of the early stop"""
    beta = n * EPS * kB
    return types.SimpleNamespace(sig=beta, res=beta, vorth=beta, beta=beta,
                                 cos=4 * tol_of(n) if confirmed else 2 * n * 1e-2 * early)


def ratios(m, lim):
    """measured / bound for every measured quantity"""
    return {k: getattr(m, k) / getattr(lim, k) for k in ("sig", "res", "vorth", "cos") if getattr(m, k) is not None}


def check_rankdef(n, US, V, s, sweeps, sref, kB):
    """the assertions of the rank-deficient case; -> (largest |s - sref| / (n eps s_max), max |V'V - I| / beta)"""
    z = rankdef_columns(n)[0]
    assert 0 < sweeps < MAX_SWEEPS, sweeps
    assert np.isfinite(US).all() and np.isfinite(s).all()
    assert not US[:, z].any() and s[z] == 0.0, (np.abs(US[:, z]).max(), s[z])
    ss = np.sort(s.astype(LD))[::-1]
    lim = n * EPS * float(sref[0])
    assert ss[-1] == 0 and (ss[-3:] <= lim).all(), (ss[-3:], lim)
    assert ss[-4] > 1e3 * lim                                        # (the rank is n - 3, not less)
    err = float(np.abs(ss - sref).max() / lim)
    vr = None
    if V is not None:
        Vl = V.astype(LD)
        vr = float(np.abs(Vl.T @ Vl - np.eye(n, dtype=LD)).max() / (n * EPS * kB))
    return err, vr


def check_orth(case, US, V, s, sweeps):
    """exactly orthogonal columns: nothing may change"""
    assert sweeps == 1, sweeps
    assert np.array_equal(US, case.A)
    assert V is None or np.array_equal(V, np.eye(case.n))
    assert np.array_equal(s, np.abs(case.D))


# ------------------------------------------------------------------------------------------------ float64 restatement
FAULTS = ["rsqrt_1e-9", "threshold_max", "gram_last_chunk", "gram_untransposed", "last_rotation", "cross_in_round0",
          "padding_ones", "v_skipped"]


def f64_small(A, vectors=True):
    """jacobi_small_kernel: the cyclic sweep in float64 at the device's threshold, at most 40 sweeps"""
    return jacobi_cyclic(A, np.float64, tol_of(A.shape[0]), vectors, MAX_SWEEPS)


def chunk_plan(n, jb, wgs=0):
    """(rows per chunk, chunks) of the Gram and apply launches, as jacobi_svd sizes them"""
    nbk = (n + jb - 1) // jb
    npair = ((nbk + 1) & ~1) // 2
    target = wgs if wgs > 0 else (1536 if jb == 32 else (256 if n < 1500 else 512))
    nchunk = max(1, min((target + npair - 1) // npair, (n + 63) // 64))
    RC = ((((n + nchunk - 1) // nchunk) + 63) // 64) * 64
    return RC, (n + RC - 1) // RC


def _jrot(al, be, ga, tol, fault):
    """jrot of csrc/jacobi.hip as written, elementwise; -> (c, s, rotated)"""
    if fault == "threshold_max":
        rot = np.abs(ga) > tol * np.maximum(al, be)
    else:
        rot = ga * ga > tol * tol * al * be
    d, g2 = be - al, 2.0 * ga
    r2 = np.where(rot, d * d + g2 * g2, 1.0)
    ir = 1.0 / np.sqrt(r2)
    c2 = 0.5 + 0.5 * np.abs(d) * ir
    ic = 1.0 / np.sqrt(c2)
    if fault == "rsqrt_1e-9":                                        # v_rsq_f64 with one Newton step: both carry an error
        ir, ic = ir * (1.0 + 1e-9), ic * (1.0 - 0.7e-9)
    c = c2 * ic
    s = np.where(d >= 0.0, ga, -ga) * ir * ic
    return np.where(rot, c, 1.0), np.where(rot, s, 0.0), rot


def _gram_sweep(G, tol, big2, inner, full, fault):
    """j*_rotate_kernel on a batch of Gram matrices G (m, w, w): `inner` sweeps of the full (w - 1 steps) or the
    cross-pair schedule (w / 2 steps); -> (R, any rotation, any rotation above the early-stop level) per matrix"""
    m, w = G.shape[0], G.shape[1]
    h = w // 2
    R = np.broadcast_to(np.eye(w), (m, w, w)).copy()
    anyrot, anybig = np.zeros(m, dtype=bool), np.zeros(m, dtype=bool)
    nsteps = w - 1 if full else h
    k = np.arange(h)
    for istep in range(nsteps * inner):
        step = istep % nsteps
        if full:
            p, q = rr_pairs(w, step)
        else:
            p, q = k, h + (k + step) % h
        al, be, ga = G[:, p, p], G[:, q, q], G[:, p, q]
        c, s, rot = _jrot(al, be, ga, tol, fault)
        anyrot |= rot.any(axis=1)
        anybig |= ((ga * ga > big2 * al * be) | (s * s > 1e-4)).any(axis=1)
        J = np.zeros((m, w, w))
        J[:, p, p], J[:, q, q], J[:, p, q], J[:, q, p] = c, c, s, -s
        G = J.transpose(0, 2, 1) @ (G @ J)
        if not (fault == "last_rotation" and istep == nsteps * inner - 1):
            R = R @ J
    return R, anyrot, anybig


def f64_blocked(A, jb=16, vectors=True, early=EARLY, wgs=0, cross=1, inner=1, fault=None):
    """The blocked scheme of jacobi_svd in float64: per round, for every block pair (I, J), the Gram matrix of the panel
    [A_I A_J] as a sum over row chunks, one Gram sweep, the panel (and V's) times R; a sweep ends the SVD when no pair
    rotated or none rotated above the early-stop level.  -> (US, V or None, column norms, sweeps)"""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    a = A.copy(order="F")
    v = np.eye(n) if vectors else None
    tol, big2 = tol_of(n), (early * early if early > 0 else 0.0)
    nbk = (n + jb - 1) // jb
    nbk2 = (nbk + 1) & ~1
    RC, nchunk = chunk_plan(n, jb, wgs)
    w = 2 * jb
    sweeps = 0
    with np.errstate(all="ignore"):
        while sweeps < MAX_SWEEPS:
            h0 = h1 = 0
            for rnd in range(nbk2 - 1):
                I, J = rr_pairs(nbk2, rnd)
                idx = np.concatenate([I[:, None] * jb + np.arange(jb)[None, :], J[:, None] * jb + np.arange(jb)[None, :]],
                                     axis=1)                          # (pairs, w)
                ok = idx < n
                safe = np.where(ok, idx, 0)
                P = np.where(ok[:, None, :], a[:, safe].transpose(1, 0, 2), 0.0)       # (pairs, n, w)
                Pg = np.where(ok[:, None, :], P, 1.0) if fault == "padding_ones" else P
                G = np.zeros((P.shape[0], w, w))
                for ch in range(nchunk):
                    r0, r1 = ch * RC, min(n, (ch + 1) * RC)
                    if fault == "gram_last_chunk" and ch == nchunk - 1 and r1 - r0 < RC:
                        continue
                    G += Pg[:, r0:r1, :].transpose(0, 2, 1) @ Pg[:, r0:r1, :]
                if fault == "gram_untransposed":
                    G[:, jb:, :jb] = G[:, :jb, jb:]
                full = rnd == 0 or cross == 0
                if fault == "cross_in_round0":
                    full = cross == 0
                R, anyrot, anybig = _gram_sweep(G, tol, big2, inner, full, fault)
                h0 += int(anyrot.sum())
                h1 += int(anybig.sum())
                for k in np.nonzero(anyrot)[0]:
                    cols = idx[k][ok[k]]
                    a[:, cols] = (P[k] @ R[k])[:, ok[k]]
                    if vectors and not (fault == "v_skipped" and rnd == 1 and k == 0):
                        Pv = np.where(ok[k][None, :], v[:, safe[k]], 0.0)
                        v[:, cols] = (Pv @ R[k])[:, ok[k]]
            sweeps += 1
            if h0 == 0 or h1 == 0:
                break
    return a, v, np.sqrt((a * a).sum(axis=0)), sweeps


# ------------------------------------------------------------------------------------------------ the cases
# (family, n, param, block, options): block 0 = the one-workgroup kernel (n <= 96), 16 / 32 = the blocked kernels
# (16 is the default from n = 97, 32 is option jacobi_block); options: a tuple of (option, value)
def _cases():
    out = []
    for n in (1, 2, 3, 17, 64, 95, 96):
        out += [("graded", n, -12, 0, ()), ("orth", n, None, 0, ())]
    for n in (64, 96):
        out += [("cluster", n, 1e-6, 0, ()), ("rankdef", n, None, 0, ())]
    for n in (97, 112, 113, 128, 129, 161, 257):
        out.append(("graded", n, -12, 16, ()))
    for n in (97, 129, 130, 161, 194, 257):
        out.append(("graded", n, -12, 32, ()))
    for n, jb in ((113, 16), (161, 16), (130, 32), (161, 32)):
        out += [("cluster", n, 1e-6, jb, ()), ("rankdef", n, None, jb, ()), ("orth", n, None, jb, ())]
    for n, jb in ((96, 0), (161, 16), (161, 32)):
        out += [("graded", n, g, jb, ()) for g in GRADES if g != -12]
        out += [("scaled", n, "up", jb, ()), ("scaled", n, "down", jb, ())]
    for opt in (("jacobi_wgs", 1), ("jacobi_wgs", 4096), ("jacobi_cross", 0), ("jacobi_inner", 2)):
        out.append(("graded", 161, -12, 16, (opt,)))
    for opt in (("jacobi_wgs", 1), ("jacobi_wgs", 4096)):
        out.append(("graded", 194, -12, 32, (opt,)))
    for wd in WIDTHS:
        out += [("cluster", 120, wd, 16, (("jacobi_early", early),)) for early in (EARLY, 0.0)]
    out += [("cluster", 96, 1e-6, 0, (("jacobi_early", early),)) for early in (EARLY, 0.0)]
    # (the sharp cosine bound on the 32-column kernels too)
    out += [(family, 161, param, 32, (("jacobi_early", 0.0),)) for family, param in (("graded", -12), ("cluster", 1e-6))]
    return out


CASES = _cases()
DEFAULTS = {"jacobi_block": 0, "jacobi_wgs": 0, "jacobi_cross": 1, "jacobi_inner": 0, "jacobi_early": EARLY}


def case_id(case):
    family, n, param, jb, opts = case
    return "-".join([family, "n%d" % n] + ([str(param)] if param is not None else []) + ["jb%d" % jb] +
                    ["%s=%g" % (k.replace("jacobi_", ""), val) for k, val in opts])


@functools.lru_cache(maxsize=None)
def restated(case, vectors=True):
    """the float64 restatement's result on a case: (US, V, s, sweeps)"""
    family, n, param, jb, opts = case
    A = make(family, n, param).A
    if jb == 0:
        return f64_small(A, vectors)
    o = dict(opts)
    return f64_blocked(A, jb, vectors, o.get("jacobi_early", EARLY), o.get("jacobi_wgs", 0), o.get("jacobi_cross", 1),
                       max(1, o.get("jacobi_inner", 1)))


def judge(case, US, V, s, sweeps, tag):
    """Every assertion of a case on a result (the device's or the restatement's); prints the figures, -> {bound: ratio}"""
    family, n, param, jb, opts = case
    inp = make(family, n, param)
    if family == "orth":
        check_orth(inp, US, V, s, sweeps)
        print("JACOBI %-8s %-44s unchanged, sweeps %d" % (tag, case_id(case), sweeps))
        return {}
    sref = reference_sigma(family, n, param)
    if family == "rankdef":
        err, vr = check_rankdef(n, US, V, s, sweeps, sref, inp.kB)
        print("JACOBI %-8s %-44s |s - sref| = %.3f n eps s_max, |V'V - I| = %s beta, sweeps %d"
              % (tag, case_id(case), err, "-" if vr is None else "%.3f" % vr, sweeps))
        assert err <= 1.0 and (vr is None or vr <= 1.0), (case_id(case), err, vr)
        return {"rankdef_sig": err, "rankdef_vorth": vr or 0.0}
    early = dict(opts).get("jacobi_early", EARLY)
    lim = limits(n, inp.kB, jb == 0 or early == 0.0, early)
    m = measure(inp.A, US, V, s, sref)
    r = ratios(m, lim)
    f = lambda x: "-" if x is None else "%.2e" % x                   # noqa: E731
    print("JACOBI %-8s %-44s sig %s res %s vorth %s (beta %.2e)  cos %s (cap %.2e)  sweeps %d"
          % (tag, case_id(case), f(m.sig), f(m.res), f(m.vorth), lim.beta, f(m.cos), lim.cos, sweeps))
    assert 0 < sweeps < MAX_SWEEPS, (case_id(case), sweeps)
    assert all(x <= 1.0 for x in r.values()), (case_id(case), r)
    return r
