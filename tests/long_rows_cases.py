"""Seeded, designed inputs of tests/test_long_rows_cpu.py and tests/test_gpu_long_rows.py, and their references: blocks with LONG
SPARSE stored constraints -- a trace row, diag(a), a tridiagonal, an arrow -- beside element matrices and tiny constraints, built
so that the long route of the Schur assembly (csrc/longops.hip, option pair_long; the lists: csrc/model_layout.h::block_long)
meets every edge it has.

  trace    msz 300     identity row; 12 element matrices, s = 1, 8, 8, 12 (unsymmetric), 15, 16, 17, 31, 32 dense and 17, 31, 32
                       banded; tiny partners (one entry, a pair, an entry without its twin, an empty constraint)
                       -> rho = 300: two thread stripes, five 64-chunks with a tail of 44, ld = 320; every tile count of the MFMA kernel
  rows     msz 257     diag(a) on 257, 256, 255 and on 65 scattered rows; a tridiagonal and an arrow (769 entries each: a tie); an
                       upper-bidiagonal list without twins (unsymmetric, rows != columns); tiny partners
                       -> stripe and chunk edges 255 / 256 / 257 and 64 / 65; long x long and self pairs; Z from A, not A'
  edge     msz 96      constraints of 41, 40 and 39 entries: lg_hi between them with pair_long_min = 40
  edge64   msz 96      the same at 65, 64, 63: the default of pair_long_min, which lrn_dbg_model_layout uses
  prefix   msz 300     'trace' with qA = nvar and dense_threshold 300: the identity and two elements stored dense, range behind nd
  overlap  msz 96      a 32 x 32 dense element (1024 entries) in front of smaller elements: local owner under pair_local = 1, long
                       owner under 0
  blocks   msz 300+12  'trace' beside a block of tiny constraints, four linear rows (natural order of H, hidx)
  none     msz 96      tiny constraints only: empty range

A constraint is its entry list (rows, cols, values of A; AA = -A as the reader stores it).

Reference: the definition  tr(A_i W A_j W) = sum_e sum_f a_e b_f W[c_e, p_f] W[r_e, q_f]  in np.longdouble from the float64 inputs,
through each matrix's own non-zeros -- no Z, no row lists.  Bound of a routed pair: gamma_L B_ij,
    B_ij = sum_f |b_f| sum_a (sum_{e in row a} |a_e| |W[c_e, p_f]|) |W[R[a], q_f]|      (= the same double sum on absolute values)
L = the longest chain of roundings of the order built, plus 8.  With e_row = the most entries in a row of the owner:
  entry kernel  Z[a, x]: e_row products added in order (e_row).  A thread adds per = ceil(nnz_j / slices) entries times
                ceil(rho_i / 256) stripes, each term two multiplications (the 3 with the add into H); 6 shuffle steps; 3 adds over
                the waves; slices adds in long_reduce_kernel (slices - 1, and 1 into H):
                    L = e_row + per * ceil(rho_i / 256) + 6 + 3 + slices + 3 + 8
  MFMA kernel   Z as above.  A wave's accumulator takes 4 products a K-step over its chunks -- at most rho_i non-zero terms in all,
                the zero padding adds exactly --; 3 adds over the waves; the product with Ah and 15 adds per lane (16); 6 shuffle
                steps; the 3 as above:
                    L = e_row + rho_i + 16 + 3 + 6 + 3 + 8
The order built is the one the issue describes, so these are its formulas."""
import functools
import types

import numpy as np
import scipy.sparse as sp

import local_support_cases as lc

LD = lc.LD
gamma = lc.gamma
LONG_MIN = 64              # PAIR_LONG_MIN of csrc/model_layout.h
LONG_SPLIT = 1 << 15       # PAIR_LONG_SPLIT
SLICES_MAX = 64            # LONG_SLICES_MAX
NAMES = ["trace", "rows", "edge", "edge64", "prefix", "overlap", "blocks", "none"]


# ---------------------------------------------------------------------------------------------- constraints
def _diag_on(rows, rng):
    rows = np.asarray(rows)
    return rows, rows, lc._val(rng, len(rows))


def _trace_cons(rng, m):
    cons = [(np.arange(m), np.arange(m), np.ones(m))]                          # tr X
    for s in (32, 31, 17, 16, 15, 8, 8):
        cons.append(lc._on(lc._support(rng, m, s, s // 2), rng))
    cons.append(lc._on(lc._support(rng, m, 12, 4), rng, sym=False))            # unsymmetric Ah, 144 entries
    for s in (32, 31, 17):
        cons.append(lc._on(lc._support(rng, m, s, 8), rng, band=1))            # two tiles, 94 / 91 / 49 entries
    cons.append(lc._tiny(rng, m, "diag"))                                      # the element with s = 1
    for kind in ("diag", "pair", "lone", "empty"):
        cons.append(lc._tiny(rng, m, kind))
    return cons


def _count_cons(rng, m, counts):
    """symmetric constraints of exactly these entry counts on supports of 12, and a pair"""
    return [lc._sym_count(lc._support(rng, m, 12, 4), rng, n) for n in counts] + [lc._tiny(rng, m, "pair")]


@functools.lru_cache(maxsize=None)
def build_case(name):
    """Built once per process, shared by every test that needs it, never modified."""
    seed = 9300 + NAMES.index(name)
    rng = np.random.default_rng(seed)
    qA_all, dense_threshold, C_lin, long_min = False, 1.0e9, None, LONG_MIN
    if name in ("trace", "prefix", "blocks"):
        m = 300
        cons = _trace_cons(np.random.default_rng(9300), m)
        if name == "prefix":
            qA_all, dense_threshold = True, 300.0
    elif name == "rows":
        m = 257
        i = np.arange(m)
        tri = (np.concatenate([i, i[1:], i[:-1]]), np.concatenate([i, i[:-1], i[1:]]), None)
        arrow = (np.concatenate([i, i[1:], np.zeros(m - 1, int)]), np.concatenate([i, np.zeros(m - 1, int), i[1:]]), None)
        sym = lambda r, c: (r, c, (lambda M: M[r, c])(np.tril(lc._val(rng, (m, m))) + np.tril(lc._val(rng, (m, m)), -1).T))
        bidiag = (np.concatenate([i[:200], i[:-1]]), np.concatenate([i[:200], i[1:]]), lc._val(rng, 200 + m - 1))
        cons = [_diag_on(i, rng), _diag_on(i[:256], rng), _diag_on(np.sort(rng.choice(m, 255, replace=False)), rng),
                _diag_on(np.sort(rng.choice(m, 65, replace=False)), rng), sym(*tri[:2]), sym(*arrow[:2]), bidiag,
                lc._tiny(rng, m, "pair"), lc._tiny(rng, m, "lone"), lc._tiny(rng, m, "diag")]
    elif name in ("edge", "edge64"):
        m = 96
        long_min = 40 if name == "edge" else LONG_MIN
        cons = _count_cons(rng, m, (long_min + 1, long_min, long_min, long_min - 1, long_min - 1))
    elif name == "overlap":
        m = 96
        cons = [lc._on(lc._support(rng, m, 32, 8), rng)] + [lc._on(lc._support(rng, m, s, s // 2), rng) for s in (8, 8, 6, 5)]
        cons += [lc._tiny(rng, m, k) for k in ("pair", "diag", "lone")]
    else:                                                                      # "none"
        m = 96
        cons = [lc._sym_count(lc._support(rng, m, 6, 3), rng, n) for n in (20, 9)] + [lc._tiny(rng, m, k) for k in ("pair", "diag", "lone", "empty")]
    order = rng.permutation(len(cons))                                         # the natural numbering is not the sorted one
    cons = [cons[k] for k in order]
    nvar = len(cons)
    AA, msizes = [lc._rows(cons, m)], [m]
    if name == "blocks":
        m2 = 12
        cons2 = [lc._tiny(rng, m2, k) for k in ("pair", "diag", "lone", "pair", "diag", "pair")]
        AA.append(lc._rows(cons2, m2, nvar, rng.choice(nvar, len(cons2), replace=False)))
        msizes.append(m2)
        nlin = 4
        lr = rng.choice(nvar, 3 * nlin, replace=False)
        C_lin = sp.csr_matrix((lc._val(rng, 3 * nlin), (lr, np.repeat(np.arange(nlin), 3))), shape=(nvar, nlin))
    sigma = np.stack([np.argsort(-np.diff(A.indptr), kind="stable") for A in AA], axis=1).astype(np.int64)
    qA = np.zeros((2, len(AA)), dtype=np.int64)
    if qA_all:
        qA[0, :] = nvar
    wr = np.random.default_rng(seed + 500)
    nlin = 0 if C_lin is None else C_lin.shape[1]
    return types.SimpleNamespace(
        name=name, AA=AA, msizes=np.array(msizes, dtype=np.int64), nvar=nvar, nlmi=len(AA), sigmaA=sigma, qA=qA, C_lin=C_lin,
        nlin=nlin, dense_threshold=dense_threshold, long_min=long_min,
        W={"benign": [lc._benign(k, wr) for k in msizes], "graded": [lc._graded(k, wr) for k in msizes]},
        X_lin=np.exp(wr.uniform(-1.0, 1.0, nlin)), S_lin_inv=np.exp(wr.uniform(-1.0, 1.0, nlin)))


# ---------------------------------------------------------------------------------------------- the lists, as NumPy states them
def entries(M):
    """the non-zeros of a dense matrix in the order of the device lists: by column, then by row"""
    c, r = np.nonzero(M.T)
    return r, c, M[r, c]


@functools.lru_cache(maxsize=None)
def spec_long(name, ib=0, long_min=None):
    """What block_long is to produce for block ib: lg_hi and, for the positions [nd, lg_hi), the ascending distinct rows R_p and per
    row its entries in ascending column order; all five lists empty when the range is.  Beside them what block_local produces
    (local_support_cases.spec_local): the two ranges decide together which kernel takes a pair."""
    case = build_case(name)
    long_min = case.long_min if long_min is None else long_min
    loc = lc.spec_local(case, ib)
    nd = loc.nd
    hi = nd + int(np.count_nonzero(loc.nnz[nd:loc.q_wave] >= long_min))
    R, rptr, eptr, ec, ev = [], [0], [0], [], []
    for p in range(nd, hi):
        M = loc.mats[p]
        rows = np.nonzero((M != 0).any(axis=1))[0]
        R.append(rows)
        for r in rows:
            cols = np.nonzero(M[r])[0]
            ec.append(cols)
            ev.append(M[r, cols])
            eptr.append(eptr[-1] + len(cols))
        rptr.append(rptr[-1] + len(rows))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    empty = hi == nd
    return types.SimpleNamespace(
        loc=loc, nd=nd, q_wave=loc.q_wave, npos_nz=loc.npos_nz, nnz=loc.nnz, mats=loc.mats, lg_hi=hi, R=R,
        lg_rptr=np.zeros(0, np.int64) if empty else np.array(rptr), lg_rows=cat(R, np.int64),
        lg_eptr=np.zeros(0, np.int64) if empty else np.array(eptr), lg_ec=cat(ec, np.int64), lg_ev=cat(ev, np.float64))


def slices(nnz_j, rho_i, split):
    """model_layout.h::long_slices: (slices, entries per slice)"""
    work = nnz_j * rho_i
    ns = max(1, min(-(-work // split), SLICES_MAX, nnz_j))
    per = -(-nnz_j // ns)
    return -(-nnz_j // per), per


def plan(spec, local=0, mfma=1, split=LONG_SPLIT, shift=0):
    """The pairs the route takes, as assemble_sparse and long_plan decide: [(pi, pj, 'mfma' or 'entry', slices, per)], lg_end.
    shift: the range off by one (a fault of test_long_rows_cpu.py)."""
    loc = spec.loc
    local_on = bool(local) and loc.loc_hi > loc.loc_lo
    lg_end = (min(spec.lg_hi, loc.loc_lo) if local_on else spec.lg_hi) + shift
    use_mfma = bool(mfma) and loc.loc_hi > loc.loc_lo
    out = []
    for pi in range(spec.nd, lg_end):
        rho = len(np.nonzero((spec.mats[pi] != 0).any(axis=1))[0])
        for pj in range(pi, spec.npos_nz):
            if use_mfma and pj >= loc.loc_lo:
                out.append((pi, pj, "mfma", 0, 0))
            else:
                out.append((pi, pj, "entry") + slices(int(spec.nnz[pj]), rho, split))
    return out, lg_end


def counters(pl, lg_end, spec):
    return {"pair_long_owners": lg_end - spec.nd, "pair_long_pairs": len(pl),
            "pair_long_mfma_pairs": sum(1 for p in pl if p[2] == "mfma"), "pair_long_slices": sum(p[3] for p in pl)}


def depth(spec, pi, pj, kind, ns, per):
    """L of the bound (module docstring)"""
    M = spec.mats[pi]
    e_row = int((M != 0).sum(axis=1).max())
    rho = int((M != 0).any(axis=1).sum())
    if kind == "mfma":
        return e_row + rho + 16 + 3 + 6 + 3 + 8
    return e_row + per * -(-rho // 256) + 6 + 3 + ns + 3 + 8


# ---------------------------------------------------------------------------------------------- reference, np.longdouble
def _pair_sum(Mi, Mj, W):
    """sum_e sum_f a_e b_f W[c_e, p_f] W[r_e, q_f] over the non-zeros of both, in the dtype of W"""
    r, c, a = entries(Mi)
    p, q, b = entries(Mj)
    if r.size == 0 or p.size == 0:
        return W.dtype.type(0)
    return ((a[:, None] * W[np.ix_(c, p)]) * (W[np.ix_(r, q)] * b[None, :])).sum()


_REF = {}


def reference(name, wname, k, l, ib=0):
    """(H_kl, B_kl) of block ib for the natural numbers k, l: the definition in longdouble, and the same sum on absolute values"""
    key = (name, wname, k, l, ib)
    if key not in _REF:
        case = build_case(name)
        Mi, Mj = lc.matrix(case, ib, k), lc.matrix(case, ib, l)
        W = case.W[wname][ib]
        _REF[key] = (_pair_sum(Mi.astype(LD), Mj.astype(LD), W.astype(LD)), float(_pair_sum(np.abs(Mi), np.abs(Mj), np.abs(W))))
    return _REF[key]


def others(name, wname, k, l):
    """what else lands on H_kl of a case with several blocks and linear rows: (value, absolute sum), longdouble"""
    case = build_case(name)
    v, a = LD(0), 0.0
    for ib in range(1, case.nlmi):
        h, b = reference(name, wname, k, l, ib)
        v, a = v + h, a + b
    if case.nlin:
        Cl = case.C_lin.toarray().astype(LD)
        xs = case.X_lin.astype(LD) * case.S_lin_inv.astype(LD)
        v += (Cl[k] * xs * Cl[l]).sum()
        a += float((np.abs(Cl[k]) * xs * np.abs(Cl[l])).sum())
    return v, a


# ---------------------------------------------------------------------------------------------- the route restated in float64
def _tree(v):
    v = v.copy()
    for off in (32, 16, 8, 4, 2, 1):
        v[:64 - off] = v[:64 - off] + v[off:]
    return v[0]


def z_of(M, W, fault=None):
    """long_z_kernel: (R, Zc) with Zc[a, x] = the sum over the entries of row R[a] in ascending column order, zero rows up to ld"""
    if fault == "owner_transposed":
        M = M.T
    R = np.nonzero((M != 0).any(axis=1))[0]
    ld = -(-len(R) // 64) * 64
    Z = np.zeros((ld, W.shape[0]))
    for a, r in enumerate(R):
        for c in np.nonzero(M[r])[0]:
            Z[a] = Z[a] + M[r, c] * W[:, c]                  # W[x + c msz]: column c
    return R, Z


def entry_value(R, Z, Mj, W, ns, per, fault=None):
    """long_entry_kernel and long_reduce_kernel: per slice 256 threads over f in list order and a = t, t + 256, ...; the shuffle
    tree, the waves in order; the slices in ascending order"""
    p, q, b = entries(Mj)
    if fault == "pq":
        p, q = q, p
    rho, t = len(R), np.arange(256)
    total = None
    for s in range(ns):
        if fault == "slice" and s == ns - 1 and ns > 1:
            continue
        acc = np.zeros(256)
        for f in range(s * per, min((s + 1) * per, len(b))):
            for a0 in range(0, rho, 256):
                if fault == "stripe" and a0 >= 256:
                    continue
                a = a0 + t
                ok = a < rho
                a = a[ok]
                acc[ok] = acc[ok] + (b[f] * Z[a, p[f]]) * W[R[a], q[f]]
        w = [_tree(acc[64 * k:64 * k + 64]) for k in range(4)]
        part = ((w[0] + w[1]) + w[2]) + w[3]
        total = part if total is None else total + part
    return 0.0 if total is None else float(total)


def mfma_value(R, Z, Sj, Ahj, W, fault=None):
    """long_local_kernel: wave w takes the K-chunks w, w + 4, ... of 32 rows, 8 K-steps of 4 each; the waves in order; the product
    with Ah_j in the accumulator layout, per lane over (ti, tj, v); the shuffle tree"""
    sj, rho, ld = len(Sj), len(R), Z.shape[0]
    Rj = 16 * ((sj + 15) // 16)
    ZS, WS = np.zeros((ld, Rj)), np.zeros((ld, Rj))
    ZS[:, :sj] = Z[:, Sj]
    WS[:rho, :sj] = W[np.ix_(R, Sj)]
    if fault == "ktail":
        ZS[256:] = 0.0
    Aj = np.zeros((Rj, Rj))
    Aj[:sj, :sj] = np.asarray(Ahj).reshape(sj, sj, order="F")
    if fault == "ah_transposed":
        Aj = Aj.T
    acc = np.zeros((4, Rj, Rj))
    for ch in range(ld // 32):
        for k0 in range(32 * ch, 32 * ch + 32, 4):
            acc[ch % 4] = acc[ch % 4] + ZS[k0:k0 + 4].T @ WS[k0:k0 + 4]
    M = ((acc[0] + acc[1]) + acc[2]) + acc[3]
    lane = np.arange(64)
    ci, kq = lane & 15, lane >> 4
    s = np.zeros(64)
    for ti in range(Rj // 16):
        for tj in range(Rj // 16):
            for v in range(4):
                u, vv = 16 * ti + kq + 4 * v, 16 * tj + ci
                s = s + Aj[u, vv] * M[u, vv]
    return float(_tree(s))


def route(name, wname, local=0, mfma=1, split=LONG_SPLIT, fault=None, fault_pair=None):
    """Every pair of block 0 the route takes, in float64 in the kernels' order: ({(k, l): value}, counters).  fault: one deliberate
    mistake, applied to the pair fault_pair = (pi, pj) of positions (every pair when None)."""
    case = build_case(name)
    spec = spec_long(name)
    loc = spec.loc
    pl, lg_end = plan(spec, local, mfma, split, shift=-1 if fault == "range" else 0)
    sigma, W = case.sigmaA[:, 0], case.W[wname][0]
    out, zs = {}, {}
    for (pi, pj, kind, ns, per) in pl:
        f = fault if fault_pair in (None, (pi, pj)) else None
        zkey = (pi, f == "owner_transposed")
        if zkey not in zs:
            zs[zkey] = z_of(spec.mats[pi], W, f)
        R, Z = zs[zkey]
        if kind == "mfma":
            v = mfma_value(R, Z, loc.S[pj], loc.Ah[pj], W, f)
        else:
            v = entry_value(R, Z, spec.mats[pj], W, ns, per, f)
        if f == "self_doubled" and pi == pj:
            v = 2.0 * v
        out[(int(sigma[pi]), int(sigma[pj]))] = v
    return out, counters(pl, lg_end, spec)


def worst(name, wname, got, pl, spec):
    """largest |got - definition| / (gamma_L B_ij) over the pairs of the plan; got: {(k, l): value} or a matrix in natural order"""
    sigma = build_case(name).sigmaA[:, 0]
    ratio = 0.0
    for (pi, pj, kind, ns, per) in pl:
        k, l = int(sigma[pi]), int(sigma[pj])
        v = got.get((k, l), 0.0) if isinstance(got, dict) else got[k, l]
        h, b = reference(name, wname, k, l)
        oh, ob = others(name, wname, k, l)
        bound = gamma(depth(spec, pi, pj, kind, ns, per)) * b + gamma(16) * ob
        ratio = max(ratio, float(abs(LD(v) - (h + oh))) / bound)
    return ratio


# ---------------------------------------------------------------------------------------------- planted solves
def planted(cons_mats, seed=5):
    """sum_k y_k A_k - C >= 0 with an interior point planted on both sides (as local_support_cases.q4_model):
    -> (A = [[C, A_1, ..., A_n]], b) in the form of Optimizer.load_model"""
    rng = np.random.default_rng(seed)
    m = cons_mats[0].shape[0]
    y0 = rng.uniform(0.5, 1.5, len(cons_mats))
    X0 = np.eye(m) + 0.1 * np.ones((m, m)) / m
    Cm = sum(y * A for y, A in zip(y0, cons_mats)) - 0.5 * np.eye(m)
    b = -np.array([float((A * X0).sum()) for A in cons_mats])
    return [[sp.csr_matrix((Cm + Cm.T) / 2)] + [sp.csr_matrix(A) for A in cons_mats]], b


def trace_model(m=96, seed=11):
    """a trace row beside positive semidefinite elements (s = 8) and diagonal rows: the model of the planted solves"""
    rng = np.random.default_rng(seed)
    mats = [np.eye(m)]
    for e in range(14):
        S = lc._support(rng, m, 8, 4)
        G = rng.standard_normal((8, 8)) / np.sqrt(8.0)
        A = np.zeros((m, m))
        A[np.ix_(S, S)] = G @ G.T
        mats.append((A + A.T) / 2)
    for e in range(6):
        A = np.zeros((m, m))
        i = rng.choice(m, 3, replace=False)
        A[i, i] = rng.uniform(0.5, 1.5, 3)
        mats.append(A)
    return planted(mats)


def hybrid_model(m=96, n=40, seed=21):
    """a small hybrid block: 40 constraints as factors of rank 2, a stored identity and one stored row of 9 entries, planted as
    tests/test_gpu_hybrid_factored.py plants its model -> (F0, items, b) in the form of Optimizer.load_factored_model"""
    rng = np.random.default_rng(seed)
    items = [(rng.standard_normal((m, 2)) / np.sqrt(m), rng.choice([-1.0, 1.0], size=2)) for _ in range(n)]
    nine = sp.lil_matrix((m, m))
    for i, j in ((1, 5), (2, 40), (13, 14), (30, 59)):
        nine[i, j] = nine[j, i] = rng.standard_normal()
    nine[7, 7] = 1.0
    items.insert(0, sp.identity(m, format="csc"))
    items.insert(17, nine.tocsc())
    dense = [it.toarray() if sp.issparse(it) else (it[0] * it[1]) @ it[0].T for it in items]
    Q = rng.standard_normal((m, m))
    X0 = np.eye(m) + Q @ Q.T / m
    y0 = rng.standard_normal(len(items)) / np.sqrt(len(items))
    b = -np.array([np.sum(a * X0) for a in dense])
    Cm = np.eye(m) - sum(y * a for y, a in zip(y0, dense))
    return -Cm, items, b
