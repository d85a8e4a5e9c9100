"""Extended-precision reference for the device PCG and its preconditioners (plain numpy, no GPU).

`loraine_oracle` restates the reference solver in float64, which is also the precision of the device code: where the two
disagree nobody knows which one is right.  This module forms the same objects as dense matrices in `np.longdouble`
(64-bit mantissa on x86-64) straight from their definitions:

  operator        H = sum_b AA_b (W_b (x) W_b) AA_b' + C_lin diag(X_lin .* S_lin_inv) C_lin'   (MyA, Solvers.jl:572-614)
  H_beta          M_beta  = diag(d), d = sum_b tau_b^2 + diag(C_lin diag(xs) C_lin')           (Solvers.jl:624-672)
  H_alpha         M_alpha = AAAATtau + t t', t = [AU_a Z]                                      (Solvers.jl:674-904)

MyM applies the Woodbury formula of exactly this M_alpha (AAAATtau^-1 - AAAATtau^-1 t (I + t' AAAATtau^-1 t)^-1 t'
AAAATtau^-1); here the matrix itself is formed and solved with.  Z only enters through Z Z' = 2 W - Umat Umat'.  The
eigenpairs of W are those of numpy polished by Jacobi rotations in longdouble, so the reference does not share the
rounding of the float64 eigenvectors with the code it judges.

`pcg_history` is the recurrence of `loraine_oracle.cg` in longdouble with every iterate kept, `pick_tol` places a
tolerance in a gap of the residual history so that the iteration count of a correct float64 recurrence is determined.

The second half builds the inputs of tests/test_cg_reference_cpu.py and tests/test_gpu_pcg_reference.py from seeds
(`build_case`): one function for both, nothing committed as a fixture.
"""
import functools
import math
import os
import types
from collections import namedtuple

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from . import loraine_oracle as lo

LD = np.longdouble
GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def relerr(a, b):
    """||a - b|| / ||b|| formed in longdouble, returned as a float."""
    a = np.asarray(a, dtype=LD)
    b = np.asarray(b, dtype=LD)
    return float(np.sqrt(np.sum((a - b) ** 2)) / max(np.sqrt(np.sum(b * b)), LD(1e-300)))


# --------------------------------------------------------------------------------------
# eigenpairs of W in longdouble
# --------------------------------------------------------------------------------------
def eig_ld(W):
    """Eigenvalues (ascending) and eigenvectors of the symmetric float64 matrix W to longdouble accuracy: numpy's
    eigenvectors, orthonormalised in longdouble, then cyclic Jacobi sweeps on V' W V (which is diagonal up to 1e-16 ||W||,
    so two or three sweeps finish; clusters are no difficulty for Jacobi)."""
    Wl = np.asarray(W, dtype=LD)
    m = Wl.shape[0]
    _, V0 = np.linalg.eigh(np.asarray(W, dtype=np.float64))
    V = V0.astype(LD)
    for _ in range(2):                                   # Newton step to V'V = I
        V = V @ (LD(1.5) * np.eye(m, dtype=LD) - LD(0.5) * (V.T @ V))
    T = V.T @ Wl @ V
    T = (T + T.T) / LD(2)
    eps = np.finfo(LD).eps
    for _sweep in range(12):
        d = np.abs(np.diag(T))
        off = np.abs(T - np.diag(np.diag(T)))
        thresh = eps * np.sqrt(np.outer(d, d)) * LD(0.25) + np.finfo(LD).tiny
        todo = np.argwhere(np.triu(off > thresh, 1))
        if todo.shape[0] == 0:
            break
        for p, q in todo:
            apq = T[p, q]
            if abs(apq) <= thresh[p, q]:
                continue
            theta = (T[q, q] - T[p, p]) / (LD(2) * apq)
            t = np.sign(theta) / (abs(theta) + np.sqrt(theta * theta + LD(1))) if theta != 0 else LD(1)
            c = LD(1) / np.sqrt(t * t + LD(1))
            s = t * c
            Tp, Tq = T[:, p].copy(), T[:, q].copy()
            T[:, p], T[:, q] = c * Tp - s * Tq, s * Tp + c * Tq
            Tp, Tq = T[p, :].copy(), T[q, :].copy()
            T[p, :], T[q, :] = c * Tp - s * Tq, s * Tp + c * Tq
            Vp, Vq = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = c * Vp - s * Vq, s * Vp + c * Vq
    lam = np.diag(T).copy()
    order = np.argsort(lam, kind="stable")
    return lam[order], V[:, order]


def _tau_ld(lam_s, aamat):
    """Solvers.jl:646-650 / :715-719 (loraine_oracle._tau) in longdouble."""
    if aamat == 0:
        return lam_s.min()
    return (lam_s.min() + lam_s.sum() / LD(lam_s.size)) / LD(2) - LD(1.0e-14)


# --------------------------------------------------------------------------------------
# the dense operator and the matrices the preconditioners invert
# --------------------------------------------------------------------------------------
def _constraints_ld(AAb, m):
    """(nvar, m, m) longdouble: matrix j is mat(AA_b[j, :]) = -A_j (column-major vec)."""
    n = AAb.shape[0]
    return AAb.toarray().astype(LD).reshape(n, m, m).transpose(0, 2, 1)


def _lin_term_ld(model, xs):
    Cl = model.C_lin.toarray().astype(LD)
    return (Cl * np.asarray(xs, dtype=LD)[None, :]) @ Cl.T


def dense_operator(model, W, X_lin=None, S_lin_inv=None):
    """H of MyA, every product in longdouble, formed per constraint as W A_j W."""
    n = model.n
    H = np.zeros((n, n), dtype=LD)
    for b in range(model.nlmi):
        m = int(model.msizes[b])
        Wl = np.asarray(W[b], dtype=LD)
        A = _constraints_ld(model.AA[b], m)
        A = (A + A.transpose(0, 2, 1)) / LD(2)           # mat() symmetrises (kron_etc.jl:13-18)
        T = np.matmul(np.matmul(Wl, A), Wl)
        H += A.reshape(n, m * m) @ T.reshape(n, m * m).T
    if model.nlin > 0:
        H += _lin_term_ld(model, np.asarray(X_lin, dtype=LD) * np.asarray(S_lin_inv, dtype=LD))
    return (H + H.T) / LD(2)


def prec_beta_diag(model, W, erank, aamat=1, X_lin=None, S_lin_inv=None):
    """d of M_beta = diag(d)  (Prec_for_CG_beta)."""
    d = np.zeros(model.n, dtype=LD)
    for b in range(model.nlmi):
        lam, _ = eig_ld(W[b])
        tau = _tau_ld(lam[: lam.size - erank], aamat)
        if aamat < 3:
            d += tau * tau
    if model.nlmi > 0 and model.nlin > 0:
        d += np.diag(_lin_term_ld(model, np.asarray(X_lin, dtype=LD) * np.asarray(S_lin_inv, dtype=LD)))
    return d


def prec_alpha_matrix(model, W, erank, aamat=1, X_lin=None, S_lin_inv=None):
    """M_alpha = AAAATtau + t t' with t = [AU_a Z] as Prec_for_CG_tilS_prep defines it: AU_a[j, :] = mat(AA[j, :]) Umat[:, a],
    Umat = v_l sqrt(lambda_l - tau), Z Z' = 2 W0 + Umat Umat' = 2 W - Umat Umat'."""
    n, k = model.n, erank
    M = np.zeros((n, n), dtype=LD)
    dsum = LD(0)
    for b in range(model.nlmi):
        m = int(model.msizes[b])
        Wl = np.asarray(W[b], dtype=LD)
        lam, V = eig_ld(W[b])
        tau = _tau_ld(lam[: m - k], aamat)
        if aamat < 3:
            dsum += tau * tau
        U = V[:, m - k:] * np.sqrt(lam[m - k:] - tau)[None, :]
        ZZ = LD(2) * Wl - U @ U.T
        A = _constraints_ld(model.AA[b], m)
        for a in range(k):
            AU = np.matmul(A, U[:, a])                   # (nvar, m)
            M += AU @ ZZ @ AU.T
    M += dsum * np.eye(n, dtype=LD)
    if model.nlin > 0:
        M += _lin_term_ld(model, np.asarray(X_lin, dtype=LD) * np.asarray(S_lin_inv, dtype=LD))
    return (M + M.T) / LD(2)


def spd_solver(M, refine=True):
    """x -> M^-1 x for a symmetric positive definite longdouble M: float64 Cholesky factor, refinement on the longdouble
    residual until it stalls (refine = False: the plain float64 solve)."""
    M = np.asarray(M, dtype=LD)
    cf = sla.cho_factor(M.astype(np.float64), lower=True)
    if not refine:
        return lambda x: sla.cho_solve(cf, np.asarray(x, dtype=np.float64))

    def solve(x):
        x = np.asarray(x, dtype=LD)
        y = sla.cho_solve(cf, x.astype(np.float64)).astype(LD)
        best = None
        for _ in range(12):
            r = x - M @ y
            nr = float(np.sqrt(np.sum(r * r)))
            if best is not None and nr >= 0.5 * best:
                if nr < best:
                    y = y + sla.cho_solve(cf, r.astype(np.float64)).astype(LD)
                break
            best = nr
            y = y + sla.cho_solve(cf, r.astype(np.float64)).astype(LD)
        return y

    return solve


def diag_solver(d):
    d = np.asarray(d, dtype=LD)
    return lambda x: np.asarray(x, dtype=LD) / d


def identity_solver():
    return lambda x: np.asarray(x, dtype=LD).copy()


# --------------------------------------------------------------------------------------
# the recurrence
# --------------------------------------------------------------------------------------
History = namedtuple("History", "x rho pAp clear code it")


def pcg_history(H, M_solve, b, tol, maxit, dtype=LD):
    """`loraine_oracle.cg` (ConjugateGradients.jl 0.1) in longdouble (dtype = np.float64: the same dense recurrence in
    the precision of the oracle and the device, to see how far rounding alone moves an iterate).  x[k], rho[k]: iterate and relative residual after k
    iterations (x[0] = 0, rho[0] = 1); pAp[k - 1], clear[k - 1]: p'Ap of iteration k and |p'Ap| / (||p|| ||Ap||); (code, it):
    the exit -- (30, it) converged, (-13, it) alpha negative or infinite in iteration it (x[it - 1] is returned by cg),
    (-2, maxit), (1, 0) for b = 0, (2, 0) for ||b|| <= tol."""
    H = np.asarray(H, dtype=dtype)
    b = np.asarray(b, dtype=dtype)
    n = b.shape[0]
    x = np.zeros(n, dtype=dtype)
    xs, rho, pAps, clear = [x.copy()], [1.0], [], []
    nb = np.sqrt(np.sum(b * b))
    if nb == 0:
        return History(xs, rho, pAps, clear, 1, 0)
    r = b.copy()
    res0 = nb
    if res0 <= tol:
        return History(xs, rho, pAps, clear, 2, 0)
    z = np.asarray(M_solve(r), dtype=dtype)
    p = z.copy()
    for it in range(1, maxit + 1):
        Ap = H @ p
        gamma = np.sum(r * z)
        pAp = np.sum(p * Ap)
        pAps.append(float(pAp))
        clear.append(float(abs(pAp) / (np.sqrt(np.sum(p * p)) * np.sqrt(np.sum(Ap * Ap)))))
        alpha = gamma / pAp if pAp != 0 else dtype(math.inf)
        if np.isinf(alpha) or alpha < 0:
            return History(xs, rho, pAps, clear, -13, it)
        x = x + alpha * p
        r = r - alpha * Ap
        xs.append(x.copy())
        res = np.sqrt(np.sum(r * r)) / res0
        rho.append(float(res))
        if res <= tol:
            return History(xs, rho, pAps, clear, 30, it)
        z = np.asarray(M_solve(r), dtype=dtype)
        beta = np.sum(z * r) / gamma
        p = z + beta * p
    return History(xs, rho, pAps, clear, -2, maxit)


GAP = 1.5


def _gap_ok(rho, K):
    return rho[K - 1] / rho[K] >= GAP and min(rho[:K]) ** 2 >= GAP * rho[K - 1] * rho[K]


def pick_tol(rho, K):
    """The tolerance at which a correct recurrence stops in iteration K and in no other: sqrt(rho[K-1] rho[K]), the
    geometric middle of a gap of at least 1.5 below rho[K-1].  rho[K] lies a factor sqrt(1.5) or more below it, and so
    does every earlier residual above it (the residual norm of CG is not monotone) -- orders of magnitude more than
    rounding moves a float64 residual norm by."""
    assert 1 <= K < len(rho)
    assert rho[K - 1] / rho[K] >= GAP, (K, rho[K - 1], rho[K])
    assert _gap_ok(rho, K), (K, min(rho[:K]), rho[K - 1], rho[K])
    return math.sqrt(rho[K - 1] * rho[K])


DRIFT_MAX = 1.0e-9


def choose_K(rho, drift, kmin=3, kmax=12, drift_max=DRIFT_MAX, last=True):
    """The last (last = False: first) K in [kmin, kmax] at which pick_tol's condition holds and the iterates K - 1 and K are well determined:
    drift[k] = relative distance of iterate k of the float64 dense recurrence from the longdouble one.  An iterate of CG
    next to a peak of the residual norm is an ill-conditioned function of the data (on case D rounding alone moves
    iterate 8 by 0.1 and iterate 11 by 4e-10), and once Ritz values have converged a float64 recurrence leaves the exact
    one for good: such iterates cannot be compared between two precisions."""
    Ks = range(min(kmax, len(rho) - 1, len(drift) - 1), kmin - 1, -1)
    for K in (Ks if last else reversed(Ks)):
        if _gap_ok(rho, K) and max(drift[K - 1], drift[K]) <= drift_max:
            return K
    raise AssertionError("no gap of %g at a well-determined iterate" % GAP)


def drift_of(hist, hist64):
    n = min(len(hist.x), len(hist64.x))
    return [relerr(hist64.x[k], hist.x[k]) if k else 0.0 for k in range(n)]


def true_residual(H, x, b):
    """||H x - b|| / ||b|| in longdouble."""
    H = np.asarray(H, dtype=LD)
    b = np.asarray(b, dtype=LD)
    r = H @ np.asarray(x, dtype=LD) - b
    return float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(b * b)))


# --------------------------------------------------------------------------------------
# inputs of the tests, from seeds
# --------------------------------------------------------------------------------------
def spectrum(m, cond=1.0e3, top=4, sep=1.7):
    """Eigenvalues of a test W, ascending: the `top` largest cond, cond / sep, cond / sep^2, ... (each separated from
    the next one below by a factor >= 1.5), the others spread logarithmically from 1 up to 1 / sep of the smallest of those."""
    hi = cond / sep ** np.arange(top)[::-1]
    lo_ = np.logspace(0.0, np.log10(hi[0] / sep), m - top)
    return np.concatenate([lo_, hi])


def scaling_from_spectrum(lam, rng):
    """W = Q diag(lam) Q' (symmetric to the last bit) and a G with G G' = W whose columns are not orthogonal (G = Q
    diag(sqrt|lam|) R with R orthogonal; only meaningful for lam > 0)."""
    m = lam.size
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    R, _ = np.linalg.qr(rng.standard_normal((m, m)))
    W = (Q * lam[None, :]) @ Q.T
    W = (W + W.T) / 2.0
    G = (Q * np.sqrt(np.abs(lam))[None, :]) @ R
    return W, G


def _random_block(m, nvar, rng):
    """Sparse symmetric constraints: a random sparse part as tests/test_gpu_nt_functions.py::_random_model builds it
    (density 0.08: above the kappa = 8 entries of the dense/sparse split of model.jl:153-174), scaled by 0.05, plus one
    entry of size 1..2 at a position (i <= j) of its own.  nvar is close to m (m + 1) / 2 in the shapes below; without
    the entries of their own the constraints are nearly dependent and cond(H) ~ 1e10, where the iterates of a float64
    CG say nothing.  Every third constraint has two or three entries only, so both kinds of slot exist."""
    iu, ju = np.triu_indices(m)
    own = np.resize(rng.permutation(iu.size), nvar)      # (a block with fewer positions than constraints repeats them)
    A = [sp.csc_matrix((m, m))]
    for j in range(nvar):
        if j % 3 == 2:
            M = np.zeros((m, m))
            for _ in range(1 + int(rng.integers(0, 2))):
                M[int(rng.integers(0, m)), int(rng.integers(0, m))] = 0.05 * rng.standard_normal()
        else:
            M = 0.05 * sp.random(m, m, density=0.08, random_state=rng, data_rvs=rng.standard_normal).toarray()
        v = rng.uniform(1.0, 2.0) * (1.0 if rng.random() < 0.5 else -1.0)
        M[iu[own[j]], ju[own[j]]] += v if iu[own[j]] != ju[own[j]] else v / 2
        A.append(sp.csc_matrix((M + M.T) / 2))
    C0 = rng.standard_normal((m, m))
    A[0] = sp.csc_matrix(-(C0 + C0.T) / 2)
    return A


def random_model(msizes, nvar, nlin, seed):
    rng = np.random.default_rng(seed)
    A = [_random_block(int(m), nvar, rng) for m in msizes]
    C_lin = d_lin = None
    if nlin > 0:
        C_lin = sp.csr_matrix(sp.random(nvar, nlin, density=0.06, random_state=rng, data_rvs=rng.standard_normal))
        d_lin = rng.standard_normal(nlin)
    return lo.make_model(A, rng.standard_normal(nvar), 0.0, d_lin, C_lin)


# name -> (msizes, nvar, nlin, seed); msz (msz + 1) / 2 summed over the blocks >= nvar, so H is positive definite
SHAPES = {
    "A": ([23], 257, 0, 201),          # 2 workgroups, per = 129, last slice 128
    "B": ([33], 514, 0, 208),          # 3 workgroups, per = 172, ragged 170; ksz 33 / 99
    "C": ([25, 17], 300, 5, 206),      # two blocks of different size plus linear rows
    "D": ([50], 104, 0, 203),          # theta1: one workgroup
    "E": ([90], 300, 0, 105),          # ksz = 270 at erank 3: the inverse form by itself
    "T": ([13], 36, 72, 205),          # tru3 (CPU only: the linear rows of a real problem)
}
INDEFINITE_SEED = 1                    # W of the -13 case (shape A), see build_indefinite


def build_case(name):
    """model, W, G (lists per block), X_lin, S_lin_inv, right-hand side h and a vector x for the preconditioner apply."""
    msizes, nvar, nlin, seed = SHAPES[name]
    if name == "D":
        model = lo.model_from_sdpa(os.path.join(GOLD, "theta1.dat-s"))
    elif name == "T":
        model = lo.model_from_sdpa(os.path.join(GOLD, "tru3.dat-s"))
    else:
        model = random_model(msizes, nvar, nlin, seed)
    rng = np.random.default_rng(seed + 1000)
    W, G = [], []
    for m in model.msizes:
        m = int(m)
        Wb, Gb = scaling_from_spectrum(spectrum(m, top=min(4, m - 1)), rng)
        W.append(Wb)
        G.append(Gb)
    X_lin = np.exp(rng.uniform(-1.0, 1.0, model.nlin))
    S_lin_inv = np.exp(rng.uniform(-1.0, 1.0, model.nlin))
    x = rng.standard_normal(model.n)
    case = types.SimpleNamespace(name=name, model=model, W=W, G=G, X_lin=X_lin, S_lin_inv=S_lin_inv, h=None, x=x)
    case.h = _image(case, rng.standard_normal(model.n))
    return case


def _image(case, v):
    """h = H v (float64): a right-hand side in the range of the large eigenvalues of H, as the Schur systems of an IP
    iteration are -- the residual of CG then falls from the first steps on, and its history has gaps to place tol in."""
    h = np.zeros(case.model.n)
    lo.MyA(case.W, case.model.AA, case.model.nlin, case.model.C_lin, case.X_lin, case.S_lin_inv)(h, v)
    return h


def build_indefinite(seed=INDEFINITE_SEED):
    """Shape A with W = Q diag(+-lam) Q', two of the 23 eigenvalues negative: H = AA (W (x) W) AA' is indefinite and the
    unpreconditioned recurrence meets p'Ap < 0 after a few steps.  The seed is chosen so that this is iteration 5 and
    p'Ap is nowhere near zero on the way (tests/test_cg_reference_cpu.py asserts it)."""
    case = build_case("A")
    rng = np.random.default_rng(seed)
    m = int(case.model.msizes[0])
    lam = spectrum(m, cond=30.0)
    lam[rng.permutation(m)[:2]] *= -1.0
    W, _ = scaling_from_spectrum(lam, rng)
    case.name = "A-indefinite"
    case.W, case.G = [W], [None]
    case.h = rng.standard_normal(case.model.n)
    return case


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """Built once per process, shared by every test that needs it, never modified."""
    return build_indefinite() if name == "A-indefinite" else build_case(name)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(case, dense longdouble H), once per process as well."""
    case = case_inputs(name)
    return case, dense_operator(case.model, case.W, case.X_lin, case.S_lin_inv)


@functools.lru_cache(maxsize=None)
def case_run(name, prec, erank, drift_max=DRIFT_MAX, kmin=3, last=True):
    case, H = case_data(name)
    return reference_run(case, H, prec, erank, drift_max, kmin, last)


def oracle_state(case, prec, erank, aamat=1):
    """The float64 oracle's operator and preconditioner on the inputs of `case` (what the existing GPU tests compare to)."""
    model = case.model
    s = types.SimpleNamespace(model=model, W=case.W, X_lin=case.X_lin, S_lin_inv=case.S_lin_inv, erank=erank, aamat=aamat)
    ha = lo.Halpha(1)
    if prec == 1:
        lo.Prec_for_CG_tilS_prep(s, ha)
        Mo = lo.MyM(model.AA, ha.AAAATtau, ha.Umat, ha.Z, ha.cholS)
    elif prec == 2:
        lo.Prec_for_CG_beta(s, ha)
        Mo = lo.MyM_beta(model.AA, ha.AAAATtau)
    else:
        Mo = lo.MyM_no()
    Ao = lo.MyA(case.W, model.AA, model.nlin, model.C_lin, case.X_lin, case.S_lin_inv)
    return Ao, Mo


def reference_solvers(case, prec, erank, aamat=1):
    """M^-1 of the reference for the same (prec, erank): (longdouble solve, plain float64 solve of the same matrix)."""
    if prec == 1:
        M = prec_alpha_matrix(case.model, case.W, erank, aamat, case.X_lin, case.S_lin_inv)
        return spd_solver(M), spd_solver(M, refine=False)
    if prec == 2:
        d = prec_beta_diag(case.model, case.W, erank, aamat, case.X_lin, case.S_lin_inv)
        return diag_solver(d), diag_solver(d)
    return identity_solver(), identity_solver()


def reference_solver(case, prec, erank, aamat=1):
    return reference_solvers(case, prec, erank, aamat)[0]


HISTORY_LEN = 14


def reference_run(case, H, prec, erank, drift_max=DRIFT_MAX, kmin=3, last=True):
    """The history of the reference on `case`, the iteration K the tests stop in and its tolerance."""
    solve, solve64 = reference_solvers(case, prec, erank)
    hist = pcg_history(H, solve, case.h, 0.0, HISTORY_LEN)
    hist64 = pcg_history(H, solve64, case.h, 0.0, HISTORY_LEN, dtype=np.float64)
    drift = drift_of(hist, hist64)
    K = choose_K(hist.rho, drift, kmin=kmin, drift_max=drift_max, last=last)
    return types.SimpleNamespace(solve=solve, hist=hist, drift=drift, K=K, tol=pick_tol(hist.rho, K))
