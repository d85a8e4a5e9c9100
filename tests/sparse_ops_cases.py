"""Seeded, designed inputs of tests/test_sparse_ops_cpu.py and tests/test_gpu_sparse_ops.py, and their reference: models
whose constraints are stored entries only, built so that the stored-entry ("sparse") kernels of csrc/dataops.hip meet
every edge they have -- unrolled column walks with tails, the 64-entry hand-over to the long-column kernel, more than 64
sharers of a position, entry lists past 64, diagonal entries, empty columns, an empty constraint, short last tiles --
in both size regimes (msz < 1500: one wave per stored entry; from 1500 on: q-tiles dealt to the XCDs).

  S     msz 259           six pattern columns above 64: the automatic rule keeps the dense route
  S4    msz 259           three such columns and 12 ncq < msz^2: the automatic rule takes the pattern route
  L     msz 1500          the large regime: 94 row tiles (the last 12 rows), 24 q-tiles (the last 28 columns), an arrow constraint
  L64   msz 1536          the same on a side that is a multiple of 64 and 16
  A-S, A-L                S4 / L with a tenth of the off-diagonal positions changed below the diagonal only
  P     msz 259           S4 with one stored position whose twin is absent: no pattern route (sp_ok false)
  B2    msz 1500 + 40     two blocks and five linear rows

AA is built directly as scipy.sparse rows (a constraint of the A- cases is not symmetric), sigmaA sorted by decreasing
nnz as lrn_upload_model demands.  The reference works in np.longdouble from the float64 inputs, on the pattern only:
O(ncq msz).  Its bound is the same chain on absolute values; with gamma_L = L u / (1 - L u), u = 2^-53, any order of
the sums of products of depth L stays within gamma_L times that bound of the exact value.
"""
import functools
import types

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = 2.0 ** -53
NAMES = ["S", "S4", "L", "L64", "A-S", "A-L", "P", "B2"]
# the features a block is built to have (asserted from AA in tests/test_sparse_ops_cpu.py)
COUNTS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 63, 64, 65, 66, 130]      # pattern column counts
LONG_EXTRA = [70, 90, 100]                                          # case S: three more columns above 64
LISTS = [1, 2, 3, 4, 5, 64, 65, 129]                                # entry-list lengths
SHARED_OFF, SHARED_DIAG = 130, 65                                   # constraints sharing one off-diagonal pair / one diagonal entry


def gamma(L):
    return L * U / (1.0 - L * U)


def _scaling(m, rng):
    """W = G G', cond ~ 1e4 (as _scaling of tests/test_gpu_hop.py)."""
    Gm = rng.standard_normal((m, m)) / np.sqrt(m) + np.diag(np.exp(rng.uniform(-2, 2, m)))
    return Gm @ Gm.T, Gm


def _val(rng, n=None):
    return rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)


def _block(m, rng, counts, arrow, nfill, empty_cols, nloops):
    """Constraints of one block as lists of undirected edges [(i, j, v)], i <= j (a loop i == j is a diagonal entry, an
    edge the two entries (i, j) and (j, i)), and what was designed: targets (column -> count), the shared positions."""
    tail = list(range(m - 3, m))
    a = 5 if arrow else None                                       # the arrow's column: every row stored
    reserved = set(empty_cols) | set(tail) | ({a} if arrow else set())
    pool = np.array([v for v in range(m) if v not in reserved])
    rng.shuffle(pool)
    targets, fillers = pool[:len(counts)], pool[len(counts):]
    assert fillers.size > max(counts) + 2
    edges, loops = set(), set()
    design = {}
    for t, d in zip(targets, counts):
        t = int(t)
        design[t] = d
        need = d - (1 if arrow else 0)                             # (the arrow's entry (a, t) is in column t already)
        if need >= 2 and (d % 2 == 0 or d == 65):
            loops.add(t)
            need -= 1
        for f in rng.choice(fillers, need, replace=False):
            edges.add((min(t, int(f)), max(t, int(f))))
    edges |= {(m - 3, m - 1), (m - 2, m - 1)}                      # the last q-tile / row group is not empty
    loops |= {m - 1}
    while len(edges) < nfill + sum(counts):
        i, j = (int(v) for v in rng.choice(fillers, 2, replace=False))
        edges.add((min(i, j), max(i, j)))
    loops |= {int(v) for v in rng.choice(fillers, nloops, replace=False)}
    # the shared positions: a fresh pair and a fresh diagonal entry
    while True:
        i, j = sorted(int(v) for v in rng.choice(fillers, 2, replace=False))
        if (i, j) not in edges:
            break
    dstar = int(next(v for v in fillers if int(v) not in loops))
    edges, loops = [e for e in sorted(edges)], sorted(loops)
    rng.shuffle(edges)
    rng.shuffle(loops)
    cons = []

    def take(nl, ne):
        c = [(loops.pop(), None) for _ in range(nl)] + [edges.pop() for _ in range(ne)]
        cons.append([(p, p if q is None else q, float(_val(rng))) for p, q in c])

    for n in LISTS:
        take(n % 2, n // 2)
    first_plain = len(cons)
    while edges or loops:
        ne = min(len(edges), int(rng.integers(0, 4)))
        nl = min(len(loops), 1 if (ne == 0 or rng.random() < 0.15) else 0)
        if ne + nl:
            take(nl, ne)
    plain = np.arange(first_plain, len(cons))
    assert plain.size >= SHARED_OFF
    for k in rng.choice(plain, SHARED_OFF, replace=False):
        cons[k].append((i, j, float(_val(rng))))
    for k in rng.choice(plain, SHARED_DIAG, replace=False):
        cons[k].append((dstar, dstar, float(_val(rng))))
    cons.insert(len(LISTS), [])                                    # a constraint without an entry
    if arrow:                                                      # column a and row a in full, as thetaG11's last constraint
        cons.append([(min(a, r), max(a, r), float(_val(rng))) for r in range(m)])
    return cons, types.SimpleNamespace(targets=design, shared_off=(i, j), shared_diag=dstar, arrow=a, empty_cols=list(empty_cols))


def _rows(cons, m, nvar, where=None):
    """AA (nvar x m^2, CSR) of one block from the edge lists; constraint c goes to row where[c]."""
    r, k, v = [], [], []
    for c, lst in enumerate(cons):
        row = c if where is None else int(where[c])
        for i, j, val in lst:
            r.append(row); k.append(j * m + i); v.append(val)
            if i != j:
                r.append(row); k.append(i * m + j); v.append(val)
    A = sp.csr_matrix((v, (r, k)), shape=(nvar, m * m))
    A.sort_indices()
    return A


def _sigma(AA):
    return np.stack([np.argsort(-np.diff(A.indptr), kind="stable") for A in AA], axis=1).astype(np.int64)


def _finish(name, AA, msizes, design, seed, C_lin=None):
    rng = np.random.default_rng(seed + 500)
    nvar = AA[0].shape[0]
    W, G = zip(*[_scaling(m, rng) for m in msizes])
    xs = [rng.standard_normal(nvar), np.eye(nvar)[:, nvar - 1].copy(), np.ones(nvar)]
    nlin = 0 if C_lin is None else C_lin.shape[1]
    e_max = max(int(np.diff(A.indptr).max()) for A in AA)
    return types.SimpleNamespace(
        name=name, AA=AA, msizes=np.array(msizes, dtype=np.int64), nvar=nvar, nlmi=len(AA), sigmaA=_sigma(AA),
        qA=np.zeros((2, len(AA)), dtype=np.int64), C_lin=C_lin, nlin=nlin,
        X_lin=np.exp(rng.uniform(-1.0, 1.0, nlin)), S_lin_inv=np.exp(rng.uniform(-1.0, 1.0, nlin)),
        W=list(W), G=list(G), xs=xs, design=design, dense_threshold=float(e_max + 1))


def _asymmetric(A, m, rng):
    """About a tenth of the off-diagonal stored positions get other values below the diagonal (every entry there)."""
    A = A.copy()
    keys = np.unique(A.indices)
    low = keys[(keys % m) > (keys // m)]
    pick = rng.choice(low, max(1, low.size // 10), replace=False)
    hit = np.isin(A.indices, pick)
    A.data[hit] *= rng.uniform(0.3, 3.0, int(hit.sum())) * rng.choice([-1.0, 1.0], int(hit.sum()))
    return A


def _without_twin(A, m):
    """Drop one entry below the diagonal whose position no other constraint stores."""
    A = A.tocoo()
    keys, cnt = np.unique(A.col, return_counts=True)
    lone = keys[(cnt == 1) & ((keys % m) > (keys // m))]
    key = int(lone[lone.size // 2])
    keep = A.col != key
    B = sp.csr_matrix((A.data[keep], (A.row[keep], A.col[keep])), shape=A.shape)
    B.sort_indices()
    return B, key


@functools.lru_cache(maxsize=None)
def build_case(name):
    """Built once per process, shared by every test that needs it, never modified."""
    base = {"A-S": "S4", "A-L": "L", "P": "S4"}.get(name, name)
    seed = {"S": 4101, "S4": 4102, "L": 4103, "L64": 4104, "B2": 4105}[base]
    rng = np.random.default_rng(seed)
    if base in ("S", "S4"):
        m = 259
        counts = COUNTS + (LONG_EXTRA if base == "S" else [])
        cons, d = _block(m, rng, counts, False, 300, [0, 7, 100], 40)
        AA, msizes, design, C_lin = [_rows(cons, m, len(cons))], [m], [d], None
    elif base in ("L", "L64"):
        m = 1500 if base == "L" else 1536
        cons, d = _block(m, rng, COUNTS, True, 5000, [], 150)
        AA, msizes, design, C_lin = [_rows(cons, m, len(cons))], [m], [d], None
    else:
        cons1, d1 = _block(1500, rng, COUNTS, True, 3000, [], 100)
        nvar = len(cons1)
        m2 = 40
        cons2 = []
        for _ in range(60):                                        # a small sparse block; most constraints have no entry in it
            i, j = sorted(int(v) for v in rng.choice(m2, 2, replace=False))
            c = [(i, j, float(_val(rng)))]
            if rng.random() < 0.5:
                c.append((i, i, float(_val(rng))))
            cons2.append(c)
        where = rng.choice(nvar, len(cons2), replace=False)
        nlin = 5
        lr = rng.choice(nvar, 3 * nlin, replace=False)              # three entries per column, one per row
        C_lin = sp.csr_matrix((_val(rng, 3 * nlin), (lr, np.repeat(np.arange(nlin), 3))), shape=(nvar, nlin))
        AA, msizes = [_rows(cons1, 1500, nvar), _rows(cons2, m2, nvar, where)], [1500, m2]
        design = [d1, types.SimpleNamespace(targets={}, shared_off=None, shared_diag=None, arrow=None, empty_cols=[])]
    if name.startswith("A-"):
        AA = [_asymmetric(AA[0], msizes[0], np.random.default_rng(seed + 77))]
    if name == "P":
        A, key = _without_twin(AA[0], msizes[0])
        AA = [A]
        design[0] = types.SimpleNamespace(**vars(design[0]), lone_key=key)
    return _finish(name, AA, msizes, design, seed, C_lin)


# ---------------------------------------------------------------------------------------------- what a block contains
def features(case, ib=0):
    """From AA alone: pattern column counts (msz), sharers per stored position (dict key -> count), entry-list lengths,
    whether the pattern is symmetric, ncq, s_max, e_max."""
    A, m = case.AA[ib], int(case.msizes[ib])
    keys, sharers = np.unique(A.indices[A.data != 0.0], return_counts=True)
    colcount = np.bincount(keys // m, minlength=m)
    twins = (keys % m) * m + keys // m
    return types.SimpleNamespace(keys=keys, sharers=dict(zip(keys.tolist(), sharers.tolist())), colcount=colcount,
                                 lists=np.diff(A.indptr), symmetric=bool(np.isin(twins, keys).all()), ncq=int(keys.size),
                                 s_max=int(sharers.max()), e_max=int(np.diff(A.indptr).max()))


def depth(case):
    """L of the operator's bound: s_max + 2 msz + e_max + 8.  Pattern route: a gather of at most s_max products, one
    addition of the twins (the halving is exact), a column walk of at most c_max <= msz products, a dot of msz, a list of
    at most e_max, and the additions into y (one per block, the linear term, its own two short sums): within 8.  Dense
    route: the same gather and list around two products of K = msz."""
    f = [features(case, ib) for ib in range(case.nlmi)]
    return max(x.s_max for x in f) + 2 * int(max(case.msizes)) + max(x.e_max for x in f) + 8


def depth_mat(case):
    """mat(AA'x) and Rd = C - S - mat(AA'x): s_max products summed, the twins added, two more additions, within 4."""
    return max(features(case, ib).s_max for ib in range(case.nlmi)) + 4


def depth_aa(case):
    """AA vec(Z): e_max products summed, one addition into y per block, within 4."""
    return max(features(case, ib).e_max for ib in range(case.nlmi)) + 4


# ---------------------------------------------------------------------------------------------- reference, np.longdouble
def _entries(A):
    A = A.tocoo()
    nz = A.data != 0.0
    return A.row[nz].astype(np.int64), A.col[nz].astype(np.int64), A.data[nz].astype(LD)


def _sym_pattern(case, ib, x, absolute):
    """mat(AA'x) = (M + M')/2 as (keys, values) on the stored positions and their twins, keys ascending."""
    m = int(case.msizes[ib])
    ek, ekey, ev = _entries(case.AA[ib])
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    if absolute:
        ev, xl = np.abs(ev), np.abs(xl)
    ukeys, inv = np.unique(ekey, return_inverse=True)
    raw = np.zeros(ukeys.size, dtype=LD)
    np.add.at(raw, inv, ev * xl[ek])
    tkeys = (ukeys % m) * m + ukeys // m
    allkeys = np.union1d(ukeys, tkeys)
    Mv = np.zeros(allkeys.size, dtype=LD)
    Mv[np.searchsorted(allkeys, ukeys)] += raw / 2
    Mv[np.searchsorted(allkeys, tkeys)] += raw / 2
    return allkeys, Mv


def ref_mat(case, y, ib=0, absolute=False):
    """mat(AA'y) of block ib, dense msz x msz longdouble (absolute: the bound, from |AA| and |y|)."""
    m = int(case.msizes[ib])
    keys, Mv = _sym_pattern(case, ib, y, absolute)
    M = np.zeros((m, m), dtype=LD)
    M[keys % m, keys // m] = Mv
    return M


_Z_CACHE = {}


def _ref_Z(case, ib, W, x, absolute):
    """Z = W mat(AA'x) W on the stored positions of block ib: (entry rows, entry keys, entry values, Z at each entry)."""
    ck = (case.name, ib, absolute, np.asarray(x).tobytes(), id(W))
    if ck in _Z_CACHE:
        return _Z_CACHE[ck]
    m = int(case.msizes[ib])
    Wl = np.asarray(W, dtype=np.float64).astype(LD)
    if absolute:
        Wl = np.abs(Wl)
    keys, Mv = _sym_pattern(case, ib, x, absolute)
    T = np.zeros((m, m), dtype=LD)                                 # T = M W, row a from the stored entries of column a of M (M symmetric)
    col = keys // m
    start = np.searchsorted(col, np.arange(m + 1))
    for a in range(m):
        s, e = start[a], start[a + 1]
        if e > s:
            T[a, :] = Mv[s:e] @ Wl[keys[s:e] % m, :]
    ek, ekey, ev = _entries(case.AA[ib])
    if absolute:
        ev = np.abs(ev)
    ukeys, inv = np.unique(ekey, return_inverse=True)
    Zu = np.zeros(ukeys.size, dtype=LD)
    Tt = np.ascontiguousarray(T.T)
    for s in range(0, ukeys.size, 2000):
        kk = ukeys[s:s + 2000]
        Zu[s:s + 2000] = np.einsum("ij,ij->i", Wl[kk % m, :], Tt[kk // m, :])
    out = (ek, ekey, ev, Zu[inv])
    if len(_Z_CACHE) > 24:
        _Z_CACHE.clear()
    _Z_CACHE[ck] = out
    return out


def _ranges(case, spec):
    if spec is None:
        return [None] * case.nlmi
    assert len(spec) == case.nlmi
    return list(spec)


def ref_operator(case, W, x, cols=None, rows=None, lin=True, absolute=False):
    """y = sum over the blocks of AA vec(W mat(AA'x) W) (+ C_lin diag(X_lin S_lin_inv) C_lin' x when lin), longdouble.
    cols / rows: per block (lo, hi) or None -- only the entries with column (row) in [lo, hi), the share of one rank under
    the pattern route (the dense route); a block takes one of the two.  absolute: the bound B."""
    y = np.zeros(case.nvar, dtype=LD)
    cols, rows = _ranges(case, cols), _ranges(case, rows)
    for ib in range(case.nlmi):
        m = int(case.msizes[ib])
        ek, ekey, ev, Ze = _ref_Z(case, ib, W[ib], x, absolute)
        keep = np.ones(ek.size, dtype=bool)
        if cols[ib] is not None:
            keep &= (ekey // m >= cols[ib][0]) & (ekey // m < cols[ib][1])
        if rows[ib] is not None:
            keep &= (ekey % m >= rows[ib][0]) & (ekey % m < rows[ib][1])
        np.add.at(y, ek[keep], (ev * Ze)[keep])
    if lin and case.nlin > 0:
        Cl = case.C_lin.toarray().astype(LD)
        xs = case.X_lin.astype(LD) * case.S_lin_inv.astype(LD)
        xl = np.asarray(x, dtype=np.float64).astype(LD)
        if absolute:
            Cl, xl = np.abs(Cl), np.abs(xl)
        y += Cl @ (xs * (Cl.T @ xl))
    return y


def ref_bound(case, W, x, cols=None, rows=None, lin=True):
    """B_k = sum_e |AA[k, e]| (|W| Mbar |W|)[e], Mbar from |AA| and |x| (+ the linear term on absolute values)."""
    return ref_operator(case, W, x, cols, rows, lin, absolute=True)


def ref_aa_times(case, Z, absolute=False):
    """sum over the blocks of AA vec(Z_b), longdouble (absolute: the bound, |AA| |Z|)."""
    y = np.zeros(case.nvar, dtype=LD)
    for ib in range(case.nlmi):
        m = int(case.msizes[ib])
        ek, ekey, ev = _entries(case.AA[ib])
        z = np.asarray(Z[ib], dtype=np.float64)[ekey % m, ekey // m].astype(LD)
        np.add.at(y, ek, np.abs(ev) * np.abs(z) if absolute else ev * z)
    return y


def shard_range(m, rank, world):
    """[r0, r1) of rank `rank` of `world` on a side m (matvec_partial_dev)."""
    per = (m + world - 1) // world
    r0 = min(m, rank * per)
    return r0, min(m, r0 + per)


def exact_matmul(A, B, nbits=20, slices=4):
    """A @ B in longdouble through float64 products that are exact: the rows of A and the columns of B are cut into slices
    of nbits bits below the row's (column's) largest power of two, so that every product of two slices is a sum of K
    integers below 2^(2 nbits + 1) -- exact in float64 for K < 2^(52 - 2 nbits) -- and the slice products with
    i + j < slices are added in longdouble.  What is left out is below 2^(-nbits slices) K rowmax colmax."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    assert A.shape[1] * 2.0 ** (2 * nbits + 2) <= 2.0 ** 53

    def cut(X, axis):
        mx = np.abs(X).max(axis=axis, keepdims=True)
        scale = 2.0 ** np.ceil(np.log2(np.where(mx > 0, mx, 1.0)))
        out, r = [], X.copy()
        for i in range(slices):
            unit = scale * 2.0 ** (-nbits * (i + 1))
            hi = np.rint(r / unit) * unit
            out.append(hi)
            r = r - hi
        return out

    As, Bs = cut(A, 1), cut(B, 0)
    C = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for s in range(slices - 1, -1, -1):                            # smallest terms first
        for i in range(s + 1):
            C += (As[i] @ Bs[s - i]).astype(LD)
    return C
