"""Seeded, designed inputs of tests/test_local_support_cpu.py and tests/test_gpu_local_support.py, and their references: blocks
of stored constraints that are dense (or banded) on a small support S -- element matrices -- beside tiny ones, built so that
the local route of the Schur assembly (csrc/localops.hip, option pair_local; the lists: csrc/model_layout.h::block_local) meets
every edge it has: supports of 1, 5, 15, 16, 17, 31, 32 as owner and as partner in both tile combinations, a support of 33
in front of and inside the sparse range, nnz exactly pair_local_min and one below, tiny partners, an entry without its twin,
an unsymmetric A[S, S], an empty constraint, a dense prefix, two blocks with linear rows.

  sizes     msz 96    the support sizes, banded two-tile partners behind one-tile owners, tiny partners       range [0, hi)
  front33   msz 96    'sizes' with a dense s = 33 owner in front                                               range [1, hi)
  mid33     msz 96    'sizes' with a banded s = 33 owner (99 entries) in the middle                             range behind it
  edge      msz 40    constraints of 37, 36 and 35 entries                                                      loc_hi between
  tiny      msz 40    constraints below 36 entries only                                                         empty range
  tail33    msz 60    one owner; a partner of 20 entries without twins, s = 40                                  empty range
  tail35    msz 60    one owner; a diagonal partner of 35 entries, one below the default pair_local_min, s = 35     empty range
  single    msz 40    one owner (s = 8) and eleven tiny partners                                                range [0, 1)
  prefix    msz 96    'sizes' with qA = nvar and dense_threshold 900: the three largest are stored dense         range [nd, hi)
  blocks    msz 96+12 'sizes' beside a block of tiny constraints, four linear rows (natural order of H)

A constraint is its entry list (rows, cols, values of A; AA = -A as the reader stores it).  The reference is the definition
tr(A_i W A_j W) in np.longdouble from the float64 inputs, through the non-zero rows and columns of each matrix -- not
through the union S the route uses.  The bound of the route (issue: gamma_L B_ij, L = 96):
    B_ij = sum (|Ah_i| |W_ij|) o (|W_ij| |Ah_j'|),   Ah = A[S, S],  W_ij = W[S_i, S_j]
L = 96: at most 32 terms in each of the two products, at most 16 accumulator values a lane, 6 shuffle steps, 2
multiplications; the rest is margin."""
import functools
import types

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = 2.0 ** -53
DEPTH = 96
SMAX = 32                  # LOCAL_SUPPORT_MAX of csrc/model_layout.h
LOCAL_MIN = 36             # PAIR_LOCAL_MIN, the default of option pair_local_min
NAMES = ["sizes", "front33", "mid33", "edge", "tiny", "tail33", "single", "prefix", "blocks", "tail35"]


def gamma(L):
    return L * U / (1.0 - L * U)


# ---------------------------------------------------------------------------------------------- constraints
def _val(rng, shape=None):
    return rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)


def _support(rng, m, s, run):
    """s indices below m, ascending: a run of `run` consecutive ones, the others scattered"""
    start = int(rng.integers(0, m - run + 1))
    S = set(range(start, start + run))
    rest = [v for v in rng.permutation(m) if v not in S]
    S |= {int(v) for v in rest[:s - run]}
    return np.array(sorted(S))


def _on(S, rng, sym=True, band=None):
    """entries of a matrix on S x S: dense, or the band |a - b| <= band of the support's own numbering"""
    s = len(S)
    M = _val(rng, (s, s))
    if sym:
        M = np.tril(M) + np.tril(M, -1).T
    a, b = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
    keep = np.ones((s, s), bool) if band is None else np.abs(a - b) <= band
    return S[a[keep]], S[b[keep]], M[keep]


def _sym_count(S, rng, n):
    """exactly n entries on S x S, symmetric pattern: the diagonal first, then pairs (n - len(S) even or a diagonal dropped)"""
    s = len(S)
    nd_ = s if (n - s) % 2 == 0 else s - 1
    r, c = list(S[:nd_]), list(S[:nd_])
    pairs = [(a, b) for a in range(s) for b in range(a)]
    for k in rng.permutation(len(pairs))[:(n - nd_) // 2]:
        a, b = pairs[k]
        r += [S[a], S[b]]
        c += [S[b], S[a]]
    assert len(r) == n
    v = _val(rng, n)
    return np.array(r), np.array(c), v


def _tiny(rng, m, kind):
    i, j = sorted(int(v) for v in rng.choice(m, 2, replace=False))
    if kind == "diag":                                   # one entry, s = 1
        return np.array([i]), np.array([i]), _val(rng, 1)
    if kind == "pair":                                   # two entries, s = 2
        v = float(_val(rng))
        return np.array([i, j]), np.array([j, i]), np.array([v, v])
    if kind == "lone":                                   # an off-diagonal entry without its twin: one entry, s = 2
        return np.array([j]), np.array([i]), _val(rng, 1)
    return np.zeros(0, int), np.zeros(0, int), np.zeros(0)       # "empty"


def _sizes(rng, m):
    cons = []
    for s in (32, 31, 17, 16, 15):
        cons.append(_on(_support(rng, m, s, s // 2), rng))
    cons.append(_on(np.arange(40, 72), rng))                              # s = 32, one run
    cons.append(_on(_support(rng, m, 12, 4), rng, sym=False))             # unsymmetric Ah, 144 entries
    cons.append(_on(_support(rng, m, 32, 8), rng, band=1))                # two tiles, 94 entries: partner of the one-tile owners
    cons.append(_on(_support(rng, m, 20, 5), rng, band=1))                # two tiles, 58 entries
    cons.append(_on(_support(rng, m, 17, 17), rng, band=1))               # two tiles, 49 entries
    for s in (8, 8, 6):                                                   # one tile, 64 and 36 entries
        cons.append(_on(_support(rng, m, s, s // 2), rng))
    cons.append(_on(_support(rng, m, 5, 2), rng))                         # 25 entries: a partner in the wave range, s = 5
    cons.append(_on(_support(rng, m, 15, 3), rng, band=0))                # 15 entries: diagonal, s = 15
    cons.append(_on(_support(rng, m, 3, 1), rng, sym=False))              # 9 entries
    for kind in ("diag", "pair", "lone", "empty", "pair", "diag", "lone"):
        cons.append(_tiny(rng, m, kind))
    return cons


def _rows(cons, m, nvar=None, where=None):
    """AA (nvar x m^2, CSR) = -A, entry (r, c) of constraint k in column r + c m of row where[k]"""
    nvar = len(cons) if nvar is None else nvar
    r = np.concatenate([np.full(len(c[0]), k if where is None else where[k]) for k, c in enumerate(cons)]).astype(np.int64)
    key = np.concatenate([np.asarray(c[1], np.int64) * m + np.asarray(c[0], np.int64) for c in cons])
    v = np.concatenate([-np.asarray(c[2], float) for c in cons])
    A = sp.csr_matrix((v, (r, key)), shape=(nvar, m * m))
    A.sort_indices()
    return A


def _benign(m, rng):
    Gm = rng.standard_normal((m, m)) / np.sqrt(m) + np.diag(np.exp(rng.uniform(-1, 1, m)))
    W = Gm @ Gm.T
    return (W + W.T) / 2


def _graded(m, rng):
    """D Q Lambda Q' D, D graded over 1e6"""
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    D = 10.0 ** rng.permutation(np.linspace(-3.0, 3.0, m))
    W = D[:, None] * ((Q * np.exp(rng.uniform(-1, 1, m))) @ Q.T) * D[None, :]
    return (W + W.T) / 2


@functools.lru_cache(maxsize=None)
def build_case(name):
    """Built once per process, shared by every test that needs it, never modified."""
    seed = 9100 + NAMES.index(name)
    rng = np.random.default_rng(seed)
    qA_all, dense_threshold, C_lin = False, 1.0e9, None
    if name in ("sizes", "front33", "mid33", "prefix", "blocks"):
        m = 96
        cons = _sizes(np.random.default_rng(9100), m)
        if name == "front33":
            cons.append(_on(_support(rng, m, 33, 10), rng))                   # 1089 entries: the first position
        if name == "mid33":
            cons.append(_on(_support(rng, m, 33, 33), rng, band=1))           # 99 entries: behind the dense 12, before the banded 32
        if name == "prefix":
            qA_all, dense_threshold = True, 900.0
    elif name == "edge":
        m = 40
        cons = [_sym_count(_support(rng, m, 8, 3), rng, n) for n in (37, 36, 36, 35, 35)] + [_tiny(rng, m, "pair")]
    elif name == "tiny":
        m = 40
        cons = [_sym_count(_support(rng, m, 8, 3), rng, n) for n in (35, 24, 9)] + [_tiny(rng, m, k) for k in ("pair", "diag", "empty")]
    elif name == "tail33":
        m = 60
        perm = rng.permutation(m)
        cons = [_on(_support(rng, m, 8, 4), rng), (perm[:20], perm[20:40], _val(rng, 20)), _tiny(rng, m, "pair")]
    elif name == "tail35":
        m = 60
        cons = [_on(_support(rng, m, 8, 4), rng), _on(_support(rng, m, 35, 9), rng, band=0), _tiny(rng, m, "pair")]
    else:                                                                      # "single"
        m = 40
        cons = [_on(_support(rng, m, 8, 4), rng)] + [_tiny(rng, m, k) for k in ("pair", "diag", "lone") * 3 + ("pair", "empty")]
    order = rng.permutation(len(cons))                                         # the natural numbering is not the sorted one
    cons = [cons[k] for k in order]
    nvar = len(cons)
    AA, msizes = [_rows(cons, m)], [m]
    if name == "blocks":
        m2 = 12
        cons2 = [_tiny(rng, m2, k) for k in ("pair", "diag", "lone", "pair", "diag", "pair")]
        AA.append(_rows(cons2, m2, nvar, rng.choice(nvar, len(cons2), replace=False)))
        msizes.append(m2)
        nlin = 4
        lr = rng.choice(nvar, 3 * nlin, replace=False)
        C_lin = sp.csr_matrix((_val(rng, 3 * nlin), (lr, np.repeat(np.arange(nlin), 3))), shape=(nvar, nlin))
    sigma = np.stack([np.argsort(-np.diff(A.indptr), kind="stable") for A in AA], axis=1).astype(np.int64)
    qA = np.zeros((2, len(AA)), dtype=np.int64)
    if qA_all:
        qA[0, :] = nvar
    wr = np.random.default_rng(seed + 500)
    nlin = 0 if C_lin is None else C_lin.shape[1]
    return types.SimpleNamespace(
        name=name, AA=AA, msizes=np.array(msizes, dtype=np.int64), nvar=nvar, nlmi=len(AA), sigmaA=sigma, qA=qA, C_lin=C_lin,
        nlin=nlin, dense_threshold=dense_threshold, W={"benign": [_benign(k, wr) for k in msizes], "graded": [_graded(k, wr) for k in msizes]},
        X_lin=np.exp(wr.uniform(-1.0, 1.0, nlin)), S_lin_inv=np.exp(wr.uniform(-1.0, 1.0, nlin)))


# ---------------------------------------------------------------------------------------------- the lists, as NumPy states them
def matrix(case, ib, k):
    """A_k of block ib, dense msz x msz (the reader's AA = -A, column-major keys)"""
    m = int(case.msizes[ib])
    return -np.asarray(case.AA[ib][k].todense()).reshape(m, m, order="F")


def spec_local(case, ib=0, local_min=LOCAL_MIN):
    """What block_local is to produce for block ib: nd, q_wave, npos_nz, loc_lo, loc_hi, and per position the support (the
    ascending union of the non-zero rows and columns) and A[S, S] column by column -- for the positions from loc_lo on of a
    non-empty range, empty lists elsewhere."""
    m, sigma = int(case.msizes[ib]), case.sigmaA[:, ib]
    nvar = case.nvar
    mats = [matrix(case, ib, k) for k in sigma]
    nnz = np.array([np.count_nonzero(M) for M in mats])
    npos_nz = int(np.count_nonzero(nnz))
    dense = nnz >= case.dense_threshold
    nd = min(int(np.argmin(np.append(dense, False))), int(min(max(case.qA[0, ib], 0), nvar)), npos_nz)
    q_wave = max(nd, min(npos_nz, int(np.count_nonzero(nnz > 4))))
    sup = [np.nonzero((M != 0).any(axis=0) | (M != 0).any(axis=1))[0] for M in mats]
    s = np.array([len(x) for x in sup])
    hi = nd + int(np.count_nonzero(nnz[nd:q_wave] >= local_min))
    lo = hi
    if (s[hi:npos_nz] <= SMAX).all():
        while lo > nd and s[lo - 1] <= SMAX:
            lo -= 1
    listed = [p >= lo and p < npos_nz and lo < hi for p in range(nvar)]
    S = [sup[p] if listed[p] else np.zeros(0, np.int64) for p in range(nvar)]
    Ah = [mats[p][np.ix_(S[p], S[p])].ravel(order="F") for p in range(nvar)]
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return types.SimpleNamespace(
        nd=nd, q_wave=q_wave, npos_nz=npos_nz, nnz=nnz, s=s, loc_lo=lo, loc_hi=hi, S=S, Ah=Ah, sup_all=sup, mats=mats,
        loc_sptr=np.concatenate([[0], np.cumsum([len(x) for x in S])]), loc_sup=cat(S, np.int64),
        loc_aptr=np.concatenate([[0], np.cumsum([len(x) for x in Ah])]), loc_a=cat(Ah, np.float64),
        owners=hi - lo, pairs=int(sum(npos_nz - p for p in range(lo, hi))))


# ---------------------------------------------------------------------------------------------- reference, np.longdouble
@functools.lru_cache(maxsize=None)
def reference(name, wname):
    """(H, B) in the natural numbering, longdouble: H_kl = sum over the blocks of tr(A_k W A_l W) + (C_lin diag(xs) C_lin')_kl
    and the same chain on absolute values.  T_l = W A_l W through the non-zero rows R and columns C of A_l."""
    case = build_case(name)
    n = case.nvar
    H, B = np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=LD)
    for ib in range(case.nlmi):
        m = int(case.msizes[ib])
        for absolute, out in ((False, H), (True, B)):
            Wl = case.W[wname][ib].astype(LD)
            if absolute:
                Wl = np.abs(Wl)
            mats = [matrix(case, ib, k).astype(LD) for k in range(n)]
            if absolute:
                mats = [np.abs(M) for M in mats]
            ent = [np.nonzero(M) for M in mats]
            for l in range(n):
                R, Cc = np.unique(ent[l][0]), np.unique(ent[l][1])
                if R.size == 0:
                    continue
                T = Wl[:, R] @ (mats[l][np.ix_(R, Cc)] @ Wl[Cc, :])              # W A_l W
                for k in range(n):
                    r, c = ent[k]
                    if r.size:
                        out[k, l] += (mats[k][r, c] * T[c, r]).sum()            # tr(A_k T) = sum a_rc T[c, r]
    if case.nlin:
        Cl = case.C_lin.toarray().astype(LD)
        xs = case.X_lin.astype(LD) * case.S_lin_inv.astype(LD)
        H += (Cl * xs) @ Cl.T
        B += (np.abs(Cl) * xs) @ np.abs(Cl).T
    return H, B


def local_pairs(case, spec, ib=0):
    """the pairs (k, l) of natural numbers the local route computes in block ib: owner positions [loc_lo, loc_hi), partners up"""
    sigma = case.sigmaA[:, ib]
    return [(int(sigma[pi]), int(sigma[pj])) for pi in range(spec.loc_lo, spec.loc_hi) for pj in range(pi, spec.npos_nz)]


# ---------------------------------------------------------------------------------------------- the route restated in float64
def _tiles(s):
    return (s + 15) // 16


def pair_value(Si, Ahi, Sj, Ahj, W, fault=None):
    """One pair as local_pair_kernel sums it, in float64: the zero-padded tile Wt of W[S_i, S_j], per output tile (tj, ti) the two
    products in K-steps of 4 up to s_i and s_j, the entrywise product summed per lane (column ci = lane & 15, rows kq + 4 r with
    kq = lane >> 4), the shuffle tree with offsets 32 .. 1.  fault: one deliberate mistake (test_local_support_cpu.py)."""
    si, sj = len(Si), len(Sj)
    Ri, Rj = 16 * _tiles(si), 16 * _tiles(sj)
    pad = 1.0 if fault == "padding" else 0.0
    Gi = Si[::-1] if fault == "unsorted" else Si
    Wt = np.full((Ri, Rj), pad)
    if fault == "wji":                                       # W[S_j, S_i] read where W[S_i, S_j] belongs
        Wt[:si, :sj] = W[np.ix_(Sj[np.arange(si) % sj], Si[np.arange(sj) % si])]
    else:
        Wt[:si, :sj] = W[np.ix_(Gi, Sj)]
    Ai = np.full((Ri, Ri), pad)
    Ai[:si, :si] = np.asarray(Ahi).reshape(si, si, order="F")
    Aj = np.full((Rj, Rj), pad)
    Aj[:sj, :sj] = np.asarray(Ahj).reshape(sj, sj, order="F")
    Bj = Aj if fault == "transposed" else Aj.T               # Q = Wt Ah_j'
    lanes = np.zeros(64)
    ci, kq = np.arange(64) & 15, np.arange(64) >> 4
    for tj in range(Rj // 16):
        for ti in range(Ri // 16):
            P, Q = np.zeros((16, 16)), np.zeros((16, 16))
            for k0 in range(0, si, 4):
                P = P + Ai[16 * ti:16 * ti + 16, k0:k0 + 4] @ Wt[k0:k0 + 4, 16 * tj:16 * tj + 16]
            for k0 in range(0, sj, 4):
                Q = Q + Wt[16 * ti:16 * ti + 16, k0:k0 + 4] @ Bj[k0:k0 + 4, 16 * tj:16 * tj + 16]
            t = np.zeros(64)
            for r in range(4):
                t = t + P[kq + 4 * r, ci] * Q[kq + 4 * r, ci]
            lanes = lanes + t
    for off in (32, 16, 8, 4, 2, 1):
        lanes[:64 - off] = lanes[:64 - off] + lanes[off:]
    return float(lanes[0])


def route(case, wname, ib=0, fault=None):
    """The local pairs of block ib by pair_value, from the lists of spec_local: ({(k, l): value}, owners, pairs)."""
    sp_ = spec_local(case, ib)
    lo, hi = sp_.loc_lo, sp_.loc_hi
    S, Ah = sp_.S, sp_.Ah
    if fault == "range":                                     # one owner too many at the front, or one too few at the end
        if lo > sp_.nd:
            lo -= 1
        else:
            hi -= 1
        S =[sp_.sup_all[p] for p in range(case.nvar)]
        Ah = [sp_.mats[p][np.ix_(S[p], S[p])].ravel(order="F") for p in range(case.nvar)]
    sigma, W = case.sigmaA[:, ib], case.W[wname][ib]
    out, pairs = {}, 0
    for pi in range(lo, hi):
        for pj in range(pi, sp_.npos_nz):
            if fault == "diagonal" and pj == pi:
                continue
            pairs += 1
            if max(len(S[pi]), len(S[pj])) <= SMAX:
                out[(int(sigma[pi]), int(sigma[pj]))] = pair_value(S[pi], Ah[pi], S[pj], Ah[pj], W, fault)
    return out, hi - lo, pairs


def pair_bound(case, spec, wname, k, l, ib=0):
    """B_kl of the issue from the supports (float64 on absolute values; its own rounding is far inside the margin of L)"""
    ipos = np.argsort(case.sigmaA[:, ib])
    Si, Sj = spec.sup_all[ipos[k]], spec.sup_all[ipos[l]]
    Ai, Aj = np.abs(spec.mats[ipos[k]][np.ix_(Si, Si)]), np.abs(spec.mats[ipos[l]][np.ix_(Sj, Sj)])
    Wa = np.abs(case.W[wname][ib][np.ix_(Si, Sj)])
    return float(((Ai @ Wa) * (Wa @ Aj.T)).sum())


# ---------------------------------------------------------------------------------------------- the planted solve
def q4_model(nx=6, seed=77):
    """Q4-like elements on an nx x nx node grid, 2 degrees of freedom a node: element e touches its four nodes (s = 8) with
    Ah_e = G G' (8 x 8, positive semidefinite, full rank).  The problem of load_model, sum_e y_e A_e - C >= 0, with a feasible
    interior point planted on both sides: X0 > 0 any, b_e = -<A_e, X0>; y0 > 0, C = sum y0_e A_e - S0 with S0 > 0.
    -> (A = [[C, A_1, ..., A_n]], b) in the form of Optimizer.load_model."""
    rng = np.random.default_rng(seed)
    m = 2 * nx * nx
    els = []
    for ey in range(nx - 1):
        for ex in range(nx - 1):
            nodes = [ey * nx + ex, ey * nx + ex + 1, (ey + 1) * nx + ex, (ey + 1) * nx + ex + 1]
            S = np.array(sorted(2 * v + d for v in nodes for d in (0, 1)))
            Gm = rng.standard_normal((8, 8)) / np.sqrt(8.0)
            A = np.zeros((m, m))
            A[np.ix_(S, S)] = Gm @ Gm.T
            els.append(sp.csr_matrix((A + A.T) / 2))
    y0 = rng.uniform(0.5, 1.5, len(els))
    S0 = np.eye(m) * 0.5
    X0 = np.eye(m) + 0.1 * np.ones((m, m)) / m
    Cm = sum(y * A for y, A in zip(y0, els)).toarray() - S0
    b = -np.array([float((A.multiply(X0)).sum()) for A in els])
    return [[sp.csr_matrix((Cm + Cm.T) / 2)] + els], b
