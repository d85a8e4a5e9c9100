"""Static problem data in the reference's layout (`MyModel`, reference src/model.jl:34-87) and
its construction: SDPA sparse files -> MOI-equivalent sign mapping (src/MOI_wrapper.jl:142-232)
-> `_prepare_A` (src/model.jl:120-229).  Host-side, one-time; the arrays built here are what
`Device.upload_model` hands to the GPU library.

    max  b'y - b_const   s.t.  sum_j y_j A_ij <= C_i  (i = 1..nlmi),   C_lin' y <= d_lin
"""
from dataclasses import dataclass, field
from typing import List, Union

import numpy as np
import scipy.sparse as sp


@dataclass
class MyModel:
    A: List[list]           # A[i][k], k = 0..n : F_0, F_1..F_n of block i (csc, both triangles)
    AA: List[sp.csr_matrix]  # AA[i] (n x m_i^2), row j = -vec(A[i][j+1])
    B: List[sp.csr_matrix]   # rank-one factors (datarank = -1) or []
    C: List[sp.csc_matrix]   # C[i] = -A[i][0]
    nzA: np.ndarray
    sigmaA: np.ndarray       # 0-based here; the C ABI receives it 1-based
    qA: np.ndarray
    b: np.ndarray
    b_const: float
    d_lin: np.ndarray
    C_lin: sp.csr_matrix
    n: int
    msizes: np.ndarray
    nlin: int
    nlmi: int
    # rank-k factors (datarank = k >= 1): per block (V, d, khat), V (n * khat x m_i) sparse with row k * khat + p = column p
    # of V_k, d the weights +-1 (0 in the padding), A_k = V_k diag(d_k) V_k'; [] when the data has no such form
    lowrank: list = field(default_factory=list)
    lowrank_note: str = ""     # why datarank >= 1 found no factors (the solver prints it and falls back to datarank = 0)
    # factored model (build_factored_model): the constraints of a factored block exist as `lowrank` only -- its AA has no
    # entry, its A holds F_0 alone.  factored = any block is; factored_blocks[i] per block; aa_fro[i] = ||AA_i||_F from the
    # factors (what the initpoint = 1 heuristic reads from AA otherwise)
    factored: bool = False
    from_factors: bool = False     # built by build_factored_model (some or all blocks may have been materialised)
    factored_blocks: list = field(default_factory=list)
    aa_fro: list = field(default_factory=list)
    # hybrid factored block: a few constraints are STORED matrices instead of factors -- stored[i] = {k: A_i,k+1 (csc)} (0-based
    # k; {} for a pure or a materialised block).  AA[i] then holds the rows of the stored constraints only, lowrank[i]
    # weight-0 columns for them, aa_fro[i] both parts; A[i] stays [F_0]
    stored: list = field(default_factory=list)
    # Optimizer.load_factored_model(..., cg=True): the CG path (kit = 1) is allowed on this factored model -- the solver sets
    # the library option cg_factored = 1 (operator in factor form or through H of mode 1, ts of H_alpha from the factors)
    factored_cg: bool = False
    # Optimizer.load_factored_model(..., cg="diag"): ... also when factored blocks carry diagonal parts (`diag` below) -- the solver
    # sets the library option cg_diag = 1 beside cg_factored (ts of H_alpha gets the term of the diagonal rows)
    factored_cg_diag: bool = False
    # diagonal parts of factored blocks: diag[i] = {k: a (length m_i)} -- constraint k (0-based) of block i is
    # diag(a) + V diag(d) V' with its factors in `lowrank` (none for a purely diagonal constraint, e.g. a trace row).  {} for a
    # block without them and for a materialised block, whose entries hold the diagonal
    diag: list = field(default_factory=list)
    # Optimizer.load_model(..., local_support=True) / long_rows=True of the loaders: stored constraints with a small support are
    # assembled from A[S, S], long sparse ones from Z = (A W) on their rows -- the solver sets the library options pair_local /
    # pair_long = 1 after the upload (routes.py)
    local_support: bool = False
    long_rows: bool = False
    # Optimizer.load_factored_model(..., ragged=True): mode 1 assembles a block of mixed ranks by rank class (ragged_plan below) --
    # the solver sets the library option lowrank_ragged = 1.  ragged="ops": the data operators of such a block run on the
    # compacted columns as well (ragged_columns below) -- library option ragged_ops = 1 beside it.  ragged="all": so do the cross
    # terms of the assembly (stored rows, diagonal parts) and ts of H_alpha -- ragged_cross = 1 and ragged_ts = 1 beside the two
    ragged: Union[bool, str] = False      # False, True, "ops" or "all"

    @property
    def wide(self):
        """Optimizer.load_factored_model(..., wide=True): some block holds a constraint of rank 17 .. 64 (its khat is 32 or 64) --
        the solver sets the library option lowrank_wide = 1 before it uploads the factors; such a block is always assembled by
        rank class.  Read off `lowrank`: no field of its own."""
        return any(lr[2] > LOWRANK_MAX for lr in self.lowrank)

    @property
    def wide_diag(self):
        """Optimizer.load_factored_model(..., wide="diag"): some wide block (khat 32 or 64) carries diagonal parts -- the solver
        sets the library option wide_diag = 1 before it uploads them.  Read off `lowrank` and `diag` of the same block: no field
        of its own."""
        return any(lr[2] > LOWRANK_MAX and bool(dg) for lr, dg in zip(self.lowrank, self.diag))


RAGGED_CLASSES = (16, 8, 4, 2, 1)     # layout order of the rank classes
RAGGED_CLASSES_WIDE = (64, 32) + RAGGED_CLASSES      # ... of a wide block (load_factored_model(..., wide=True): ranks up to 64)
RAGGED_TILE = 64                      # tile side of the rank-class kernel: every class size divides it


def _ragged_classes(max_rank, who):
    if max_rank not in (LOWRANK_MAX, LOWRANK_MAX_WIDE):
        raise ValueError(f"{who}: max_rank is {LOWRANK_MAX} or {LOWRANK_MAX_WIDE}, not {max_rank!r}")
    return RAGGED_CLASSES if max_rank == LOWRANK_MAX else RAGGED_CLASSES_WIDE


def ragged_plan(ranks, max_rank=16):
    """The rank-class plan of one block (library option lowrank_ragged; csrc/ragged_plan.h is the same function of the factor
    weights).  ranks[h] = number of weighted factor columns of the constraint with H index h.  Class of a constraint = the
    smallest of 1, 2, 4, 8, 16 that is >= its rank; rank 0 has no group.  Classes are laid out 16, 8, 4, 2, 1, the groups of a
    class in increasing H index, each on `class` compacted columns.  Tiles: 64 x 64, anchored at the segment starts; for every
    class pair (A, B), A at or before B, all tiles of seg_A x seg_B when A != B and those with tile row >= tile column when
    A == B.  -> dict(classes = class per constraint (0: none), seg = {class: (seg0, seg1)}, Rc, ncls = classes present, gh =
    H index per group, tiles = tile count).
    max_rank=64 (a wide block): ranks up to 64, the classes 64 and 32 laid out in front of the five, the same tile rule; seg
    then has the seven keys.  An empty class has an empty segment and no tile."""
    ranks = [int(r) for r in ranks]
    layout = _ragged_classes(max_rank, "ragged_plan")
    if any(r < 0 or r > max_rank for r in ranks):
        raise ValueError(f"ragged_plan: ranks must lie in 0 .. {max_rank}")
    classes = [0 if r == 0 else padded_rank(r) for r in ranks]
    seg, gh, col = {}, [], 0
    for c in layout:
        members = [h for h, ch in enumerate(classes) if ch == c]
        seg[c] = (col, col + c * len(members))
        col += c * len(members)
        gh += members
    nt = {c: -(-(s1 - s0) // RAGGED_TILE) for c, (s0, s1) in seg.items()}
    tiles = 0
    for i, a in enumerate(layout):
        tiles += nt[a] * (nt[a] + 1) // 2
        for b in layout[i + 1:]:
            tiles += nt[a] * nt[b]
    return dict(classes=classes, seg=seg, Rc=col, ncls=sum(1 for c in layout if seg[c][1] > seg[c][0]), gh=gh,
                tiles=tiles)


RAGGED_KSTEP = 16                     # K step of the operator kernels on the compacted columns
RAGGED_MAX_CHUNKS = 16


def ragged_chunks(Rc, ks):
    """The K-chunks of the column range [0, Rc) (csrc/ragged_plan.h::ragged_chunk_cols): nsteps = ceil(Rc / 16), ks clamped to
    [1, min(16, nsteps)], chunk s = the steps [s nsteps / ks, (s + 1) nsteps / ks) -- uneven where ks does not divide nsteps,
    the last step a tail.  -> (clamped ks, [(first column, end column)] per chunk)."""
    Rc, ks = int(Rc), int(ks)
    nsteps = -(-Rc // RAGGED_KSTEP)
    ks = max(1, min(ks, RAGGED_MAX_CHUNKS, nsteps))
    return ks, [(s * nsteps // ks * RAGGED_KSTEP, min((s + 1) * nsteps // ks * RAGGED_KSTEP, Rc)) for s in range(ks)]


def ragged_columns(ranks, ks=1, max_rank=16):
    """The compacted column layout the data operators walk under the library option ragged_ops (csrc/ragged_plan.h: cg, the
    weight pattern and the chunks; ragged_plan above keeps what it returns).  -> dict(Rc, gh = H index per group, start = first
    column per group, size = class size per group, cg = group per compacted column, wc = per compacted column the index p of
    the weighted factor column of its constraint it holds (the p-th weighted one, in their original order) or -1 for padding,
    ks = clamped chunk count, chunks = [(first column, end column)], hg = group per H index, -1 for a constraint of rank 0 --
    the inverse of gh that the cross terms and ts of H_alpha walk under the library options ragged_cross and ragged_ts).
    max_rank=64: the layout of a wide block, as in ragged_plan."""
    p = ragged_plan(ranks, max_rank)
    start, size, cg, wc = [], [], [], []
    for c in _ragged_classes(max_rank, "ragged_columns"):
        s0, s1 = p["seg"][c]
        for g in range((s1 - s0) // c):
            h = p["gh"][len(start)]
            cg += [len(start)] * c
            wc += [q if q < int(ranks[h]) else -1 for q in range(c)]
            start.append(s0 + g * c)
            size.append(c)
    ks, chunks = ragged_chunks(p["Rc"], ks)
    hg = [-1] * len(p["classes"])
    for g, h in enumerate(p["gh"]):
        hg[h] = g
    return dict(Rc=p["Rc"], gh=p["gh"], start=start, size=size, cg=cg, wc=wc, ks=ks, chunks=chunks, hg=hg)


def check_factored_kit(model, kit):
    """The host's check of kit against a factored model, callable before any device exists: kit = 1 needs the model to say so
    (load_factored_model(..., cg=True)); ValueError otherwise, with the text the default has always had."""
    if getattr(model, "factored", False) and int(kit) != 0 and not getattr(model, "factored_cg", False):
        raise ValueError("a factored model (load_factored_model) needs kit = 0: the CG path reads the constraint "
                         "matrices, which do not exist")


def check_diag_kit(model, kit):
    """kit = 1 against a factored model with diagonal parts, before any device exists: the CG path (also under
    load_factored_model(..., cg=True)) builds ts of H_alpha from the factors and the stored rows and would miss them -- unless the
    model was loaded with cg="diag" (factored_cg_diag): then the library adds their term (option cg_diag)."""
    if getattr(model, "factored_cg_diag", False):
        return
    if int(kit) != 0 and getattr(model, "factored", False) and any(getattr(model, "diag", None) or []):
        raise ValueError("a factored model with diagonal parts (a constraint given as (V, d, a)) needs kit = 0: the CG path "
                         "does not hold the diagonal parts")


def _rank_one_rows(blockA, n):
    """prep_B, src/model.jl:176-197: A_k = b_k b_k' on the support of A_k, or an error."""
    m = blockA[0].shape[0]
    out = sp.lil_matrix((n, m))
    for k in range(n):
        Ak = blockA[k + 1].tocsc()
        if Ak.nnz == 0:
            continue
        support = list(dict.fromkeys(Ak.indices.tolist()))
        sub = Ak[support, :][:, support].toarray()
        _, vecs = np.linalg.eigh(0.5 * (sub + sub.T))
        with np.errstate(invalid="ignore"):
            bk = np.sign(vecs[:, -1]) * np.sqrt(np.diag(sub))
        miss = np.linalg.norm(sub - np.outer(bk, bk))
        if not miss <= 5.0e-6:
            raise ValueError(f"Obtained an error of `{miss} > 5e-6` when converting matrix into rank `1`, "
                             "use `datarank = 0` to disable the rank-1 conversion.")
        out[k, support] = bk
    return out.tocsr()


LOWRANK_TOL = 5.0e-6          # ||A_k - V_k D_k V_k'||_F, the limit prep_B applies to the rank-one form (src/model.jl:189)
LOWRANK_MAX = 16              # largest padded rank of the rank-k assembly
LOWRANK_MAX_WIDE = 64         # ... of a wide factored block (build_factored_model(..., max_rank=64), library option lowrank_wide)


def padded_rank(r):
    """khat: the power of two >= r (at least 1)."""
    k = 1
    while k < r:
        k *= 2
    return k


def _factor_residual(Ak, V, d):
    """||A_k - V diag(d) V'||_F on the union of the supports of A_k and of the rows of V (dense m x r V)."""
    Ak = sp.csc_matrix(Ak)
    rows = np.union1d(np.unique(Ak.indices), np.nonzero(np.any(V != 0.0, axis=1))[0]).astype(np.int64)
    if rows.size == 0:
        return 0.0
    sub = Ak[rows, :][:, rows].toarray()
    Vs = V[rows, :]
    return float(np.linalg.norm(sub - (Vs * d) @ Vs.T))


def lowrank_factor(Ak, m, kmax):
    """A_k = V diag(d) V' from eigh on the support of A_k: eigenpairs with |lam| > 1e-12 max|lam|, v = u sqrt|lam|,
    d = sign(lam).  -> (V (m x r dense), d) or None when the rank exceeds kmax or the residual LOWRANK_TOL."""
    Ak = sp.csc_matrix(Ak)
    if Ak.nnz == 0:
        return np.zeros((m, 0)), np.zeros(0)
    support = np.unique(np.concatenate([Ak.indices, np.repeat(np.arange(m), np.diff(Ak.indptr))]))
    sub = Ak[support, :][:, support].toarray()
    lam, vecs = np.linalg.eigh(0.5 * (sub + sub.T))
    big = np.abs(lam) > 1e-12 * np.max(np.abs(lam)) if lam.size else np.zeros(0, bool)
    if int(big.sum()) > kmax:
        return None
    V = np.zeros((m, int(big.sum())))
    V[support, :] = vecs[:, big] * np.sqrt(np.abs(lam[big]))
    d = np.sign(lam[big])
    if not _factor_residual(Ak, V, d) <= LOWRANK_TOL:
        return None
    return V, d


def pad_factors(facs, n, m):
    """[(V_k (m x r_k), d_k)] * n -> (V (n * khat x m) csr, d (n * khat), khat): zero columns of weight 0 in the padding."""
    khat = padded_rank(max([f[0].shape[1] for f in facs] + [1]))
    rr, cc, vv = [], [], []
    d = np.zeros(n * khat)
    for k, (Vk, dk) in enumerate(facs):
        r = Vk.shape[1]
        if r == 0:
            continue
        q, p = np.nonzero(Vk)
        rr.append(k * khat + p)
        cc.append(q)
        vv.append(Vk[q, p])
        d[k * khat:k * khat + r] = dk
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
    V = sp.csr_matrix((cat(vv, float), (cat(rr, np.int64), cat(cc, np.int64))), shape=(n * khat, m))
    return V, d, khat


def lowrank_factors(A, n, k):
    """Rank-k factors of every constraint of every block (datarank = k) -> (list of (V, d, khat) per block, "") or
    ([], reason) when a constraint has no such form: then the whole model takes the general path."""
    if k > LOWRANK_MAX:
        return [], f"datarank = {k} > {LOWRANK_MAX}"
    out = []
    for i, blk in enumerate(A):
        m = blk[0].shape[0]
        facs = []
        for j in range(n):
            f = lowrank_factor(blk[j + 1], m, k)
            if f is None:
                return [], f"constraint {j + 1} of LMI block {i + 1} is not of rank <= {k}"
            facs.append(f)
        out.append(pad_factors(facs, n, m))
    return out, ""


def user_factors(A, n, factors):
    """factors[i][k] = (V, d) for constraint k + 1 (A[i][k + 1]) -> per block (V, d, khat); a factor that does not
    reproduce its A_k within LOWRANK_TOL raises ValueError."""
    if len(factors) != len(A):
        raise ValueError(f"factors for {len(factors)} LMI blocks, the model has {len(A)}")
    out = []
    for i, blk in enumerate(A):
        m = blk[0].shape[0]
        if len(factors[i]) != n:
            raise ValueError(f"block {i + 1}: factors of {len(factors[i])} constraints, the model has {n}")
        facs = []
        for j, (V, d) in enumerate(factors[i]):
            V = np.asarray(V.toarray() if sp.issparse(V) else V, dtype=np.float64).reshape(m, -1)
            d = np.asarray(d, dtype=np.float64).ravel()
            if d.size != V.shape[1] or V.shape[1] > LOWRANK_MAX:
                raise ValueError(f"block {i + 1}, constraint {j + 1}: {V.shape[1]} factor columns, {d.size} weights "
                                 f"(at most {LOWRANK_MAX})")
            miss = _factor_residual(blk[j + 1], V, d)
            if not miss <= LOWRANK_TOL:
                raise ValueError(f"block {i + 1}, constraint {j + 1}: ||A - V D V'||_F = {miss:.3e} > {LOWRANK_TOL}")
            facs.append((V, d))
        out.append(pad_factors(facs, n, m))
    return out


def _prepare_A(A, datarank, kappa, n):
    """src/model.jl:120-150: AA (prep_AA!), B (prep_B), C, nzA, sigmaA, qA (prep_sparse!)."""
    nlmi = len(A)
    AA, B, C = [], [], []
    nzA = np.zeros((n, nlmi), dtype=np.int64)
    sigmaA = np.zeros((n, nlmi), dtype=np.int64)
    qA = np.zeros((2, nlmi), dtype=np.int64)
    for i, blk in enumerate(A):
        m = blk[0].shape[0]
        C.append(sp.csc_matrix(-blk[0]))
        rr, cc, vv = [], [], []
        for j in range(n):
            co = blk[j + 1].tocoo()
            nzA[j, i] = co.nnz
            rr.append(np.full(co.nnz, j, dtype=np.int64))
            cc.append(co.col.astype(np.int64) * m + co.row)
            vv.append(-co.data)
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
        AA.append(sp.csr_matrix((cat(vv, float), (cat(rr, np.int64), cat(cc, np.int64))), shape=(n, m * m)))
        if datarank == -1:
            B.append(_rank_one_rows(blk, n))
        order = np.argsort(-nzA[:, i], kind="stable")       # sortperm(rev=true) is stable
        sigmaA[:, i] = order
        below = np.nonzero(nzA[order, i] <= kappa)[0]
        qA[:, i] = below[0] if below.size else n
    return AA, B, C, nzA, sigmaA, qA


def build_model(A, b, b_const=0.0, d_lin=None, C_lin=None, datarank=0, kappa=8, factors=None) -> MyModel:
    n = len(b)
    for blk in A:
        for k in range(len(blk)):
            blk[k] = sp.csc_matrix(blk[k])
            blk[k].eliminate_zeros()
    AA, B, C, nzA, sigmaA, qA = _prepare_A(A, datarank, kappa, n)
    if C_lin is None or C_lin.shape[1] == 0:
        C_lin = sp.csr_matrix((n, 0))
        d_lin = np.zeros(0)
    msizes = np.array([blk[0].shape[0] for blk in A], dtype=np.int64)
    lowrank, note = [], ""
    if factors is not None:
        lowrank = user_factors(A, n, factors)
    elif datarank >= 1 and len(A) > 0:
        lowrank, note = lowrank_factors(A, n, datarank)
    return MyModel(A, AA, B, C, nzA, sigmaA, qA, np.asarray(b, float), float(b_const), np.asarray(d_lin, float),
                   sp.csr_matrix(C_lin), n, msizes, int(C_lin.shape[1]), len(A), lowrank, note)


def factors_fro(V, d, khat, n, chunk=256):
    """||AA_i||_F from the padded factors of one block: ||V_k D_k V_k'||_F^2 = sum_pq d_p d_q (v_p' v_q)^2, a khat x khat
    Gram matrix per constraint -- no msz x msz matrix is formed."""
    V = sp.csr_matrix(V)
    d = np.asarray(d, float).reshape(n, khat)
    tot = 0.0
    for k0 in range(0, n, chunk):
        k1 = min(n, k0 + chunk)
        Vk = V[k0 * khat:k1 * khat].toarray().reshape(k1 - k0, khat, -1)
        G = np.einsum("kpm,kqm->kpq", Vk, Vk)
        tot += float(np.einsum("kp,kq,kpq->", d[k0:k1], d[k0:k1], G * G))
    return float(np.sqrt(max(tot, 0.0)))


def _stored_matrix(item, m, where):
    """A stored constraint: symmetric m x m, SciPy sparse or a 2-D array -> csc without explicit zeros, or ValueError."""
    if not sp.issparse(item):
        item = np.asarray(item, dtype=np.float64)
        if item.ndim != 2:
            raise ValueError(f"{where}: a stored constraint is a 2-D matrix, got {item.ndim} dimension(s)")
    if item.shape != (m, m):
        raise ValueError(f"{where}: stored matrix is {item.shape}, the block has side {m}")
    A = sp.csc_matrix(item, dtype=np.float64)
    A.eliminate_zeros()
    skew = abs(A - A.T)
    if skew.nnz and skew.max() > 1e-12 * abs(A).max():
        raise ValueError(f"{where}: stored matrix is not symmetric (max |A - A'| = {skew.max():.3e})")
    return A


def diag_fro_sq(V, d, a):
    """||diag(a) + V diag(d) V'||_F^2 - ||V diag(d) V'||_F^2 = 2 sum_p d_p sum_i a_i v_ip^2 + ||a||^2 (no m x m matrix)."""
    return float(2.0 * np.sum(d * (a @ (V * V))) + a @ a)


def _check_factors(F0, factors, n, max_rank=LOWRANK_MAX, wide_diag=False):
    """factors[i][k] = (V, d) -> dense (m x r) V and d per constraint, or a symmetric m x m matrix (a stored constraint) -> csc,
    or (V, d, a) -> (V, d) and the diagonal part a (V may be None: a purely diagonal constraint); ValueError otherwise.
    -> (items per block, {k: a} per block); an all-zero a is the pair (V, d).  max_rank: the most factor columns of one
    constraint; a block that holds a constraint of more than 16 (a wide block) carries no diagonal part unless wide_diag."""
    if len(factors) != len(F0):
        raise ValueError(f"factors for {len(factors)} LMI blocks, F0 has {len(F0)}")
    out, diags = [], []
    for i, blk in enumerate(factors):
        m = F0[i].shape[0]
        if F0[i].shape != (m, m):
            raise ValueError(f"block {i + 1}: F0 is {F0[i].shape}, not square")
        if len(blk) != n:
            raise ValueError(f"block {i + 1}: factors of {len(blk)} constraints, b has {n} entries")
        facs, dg = [], {}
        for j, item in enumerate(blk):
            if sp.issparse(item) or isinstance(item, np.ndarray):
                facs.append(_stored_matrix(item, m, f"block {i + 1}, constraint {j + 1}"))
                continue
            if len(item) == 3:
                V, d, a = item
                a = np.asarray(a.toarray() if sp.issparse(a) else a, dtype=np.float64).ravel()
                if a.size != m:
                    raise ValueError(f"block {i + 1}, constraint {j + 1}: the diagonal part has {a.size} entries, the block "
                                     f"has side {m}")
                if not np.all(np.isfinite(a)):
                    raise ValueError(f"block {i + 1}, constraint {j + 1}: the diagonal part has a non-finite entry")
                if V is None:
                    V = np.zeros((m, 0))
                if a.any():
                    dg[j] = a.copy()
            else:
                V, d = item
            V = np.asarray(V.toarray() if sp.issparse(V) else V, dtype=np.float64)
            if V.ndim == 1:
                V = V.reshape(-1, 1)
            d = np.asarray(d, dtype=np.float64).ravel()
            if V.ndim != 2 or V.shape[0] != m:
                raise ValueError(f"block {i + 1}, constraint {j + 1}: V is {V.shape}, the block has side {m}")
            if d.size != V.shape[1] or V.shape[1] > max_rank:
                raise ValueError(f"block {i + 1}, constraint {j + 1}: {V.shape[1]} factor columns, {d.size} weights "
                                 f"(at most {max_rank})")
            facs.append((V, d))
        wide = [j for j, f in enumerate(facs) if not sp.issparse(f) and f[0].shape[1] > LOWRANK_MAX]
        if wide and dg and not wide_diag:
            raise ValueError(f"block {i + 1}: constraint {wide[0] + 1} has {facs[wide[0]][0].shape[1]} factor columns (more than "
                             f"{LOWRANK_MAX}) and constraint {min(dg) + 1} a diagonal part (V, d, a): a block with ranks above "
                             f"{LOWRANK_MAX} carries no diagonal part -- store that row as a sparse matrix instead")
        out.append(facs)
        diags.append(dg)
    return out, diags


def build_factored_model(F0, factors, b, b_const=0.0, d_lin=None, C_lin=None, kappa=8, factored_form=-1,
                         max_rank=LOWRANK_MAX, wide_diag=False) -> MyModel:
    """A model given by F_0 (per block), b, optional linear rows and the factors alone: A_ik = V diag(d) V' with
    factors[i][k] = (V (m_i x r, r <= max_rank, dense or sparse), d (+-1)).  No A_ik is formed for a factored block: its AA is
    an n x m^2 matrix without entries (nzA = 0, identity sigmaA) and `lowrank` carries the data.
    max_rank: 16, or 64 for wide blocks (Optimizer.load_factored_model(..., wide=True)) -- a block with a constraint of rank
    above 16 is padded to khat 32 or 64 and carries no diagonal part (V, d, a); `wide` of the model says that one exists.
    wide_diag=True (with max_rank=64; Optimizer.load_factored_model(..., wide="diag")): a wide block may hold (V, d, a) items --
    a factor-model covariance B S B' + diag(psi) with 17 .. 64 factors; `diag[i]` is filled as for a narrow block, `wide_diag` of
    the model says that such a block exists (library option wide_diag).
    factors[i][k] may instead be a symmetric m_i x m_i matrix (SciPy sparse or a 2-D array): constraint k of block i is
    STORED.  A block with both kinds is hybrid: its AA holds the rows -vec(A) of the stored constraints only, nzA / sigmaA /
    qA follow the rule of _prepare_A (stable sort by nnz, descending: the stored constraints take the first positions, the
    factored ones follow in their natural order), `lowrank` pads the stored constraints with weight-0 columns, `stored`
    keeps the matrices.
    factors[i][k] may also be a triple (V, d, a): A_ik = V diag(d) V' + diag(a) with a of length m_i (V = None and d = [] for a
    purely diagonal constraint: a trace row is (None, [], ones)).  The diagonal parts of a factored block go to `diag[i]`; a
    bare 1-D array stays an error, a triple whose a is all zero is the pair (V, d).
    factored_form: 1 = every block factored; -1 = a block whose factors are so small that the sparse path serves it --
    sum_k nnz(V_k V_k') <= kappa * (number of factored constraints), i.e. on average at most `datasparsity` entries per
    constraint, the count below which the reference treats a constraint as sparse -- is materialised (sparse AA built from
    the factors, stored matrices taken as they are, the existing path) and stays un-factored.  A diagonal part counts nnz(a)
    entries towards that sum; in a materialised block the constraint is the sparse sum, and one with a diagonal part gets
    weight-0 factor columns in `lowrank` -- its entries carry it whole, as those of a stored matrix do."""
    n = len(b)
    if factored_form not in (-1, 1):
        raise ValueError(f"factored_form = {factored_form} (-1 auto, 1 always factored)")
    if max_rank not in (LOWRANK_MAX, LOWRANK_MAX_WIDE):
        raise ValueError(f"max_rank = {max_rank!r} ({LOWRANK_MAX}, or {LOWRANK_MAX_WIDE} for wide blocks)")
    if wide_diag not in (False, True):
        raise ValueError(f"wide_diag is False or True, not {wide_diag!r}")
    if wide_diag and max_rank != LOWRANK_MAX_WIDE:
        raise ValueError(f"wide_diag = True needs max_rank = {LOWRANK_MAX_WIDE} (diagonal parts on wide blocks), not {max_rank!r}")
    items_all, diags_all = _check_factors(F0, factors, n, max_rank, bool(wide_diag))
    nlmi = len(F0)
    A, AA, C, lowrank, fblocks, aa_fro, stored, diag = [], [], [], [], [], [], [], []
    nzA = np.zeros((n, nlmi), dtype=np.int64)
    sigmaA = np.zeros((n, nlmi), dtype=np.int64)
    qA = np.zeros((2, nlmi), dtype=np.int64)
    for i, items in enumerate(items_all):
        if sp.issparse(F0[i]):
            F = sp.csc_matrix(F0[i])
            F.eliminate_zeros()
        else:
            F = np.asarray(F0[i], dtype=np.float64)            # (a dense F_0 stays dense: C is then a dense array too)
        m = F.shape[0]
        st = {k: it for k, it in enumerate(items) if sp.issparse(it)}
        none = (np.zeros((m, 0)), np.zeros(0))                 # a stored constraint has no factor column
        facs = [none if k in st else it for k, it in enumerate(items)]
        dg = diags_all[i]
        lr = pad_factors(facs, n, m)
        supp = [int(np.count_nonzero(np.any(V != 0.0, axis=1))) for V, _ in facs]
        small = sum(s * s for s in supp) + sum(int(np.count_nonzero(a)) for a in dg.values()) <= kappa * (n - len(st))
        fro_dg = sum(diag_fro_sq(*facs[k], a) for k, a in dg.items())       # (what the diagonal parts add to ||.||_F^2)
        if factored_form == -1 and small and dg:
            lr = pad_factors([none if k in dg else f for k, f in enumerate(facs)], n, m)
        lowrank.append(lr)
        if factored_form == -1 and small:
            blk = [sp.csc_matrix(F)]
            for k, ((V, d), s) in enumerate(zip(facs, supp)):
                if k in st:
                    blk.append(st[k])
                    continue
                rows = np.nonzero(np.any(V != 0.0, axis=1))[0]
                sub = (V[rows] * d) @ V[rows].T
                Ak = sp.coo_matrix((sub.ravel(), (np.repeat(rows, s), np.tile(rows, s))), shape=(m, m)).tocsc()
                if k in dg:
                    Ak = (Ak + sp.diags(dg[k], format="csc")).tocsc()
                Ak.eliminate_zeros()
                blk.append(Ak)
            AAi, _, Ci, nz, sg, q = _prepare_A([blk], 0, kappa, n)
            A.append(blk); AA.append(AAi[0]); C.append(Ci[0])
            nzA[:, i], sigmaA[:, i], qA[:, i] = nz[:, 0], sg[:, 0], q[:, 0]
            fblocks.append(False)
            aa_fro.append(float(sp.linalg.norm(AAi[0])))
            stored.append({})
            diag.append({})
        elif st:
            empty = sp.csc_matrix((m, m))
            AAi, _, _, nz, sg, q = _prepare_A([[empty] + [st.get(k, empty) for k in range(n)]], 0, kappa, n)
            A.append([F])
            AA.append(AAi[0])
            C.append(sp.csc_matrix(-F) if sp.issparse(F) else -F)
            nzA[:, i], sigmaA[:, i], qA[:, i] = nz[:, 0], sg[:, 0], q[:, 0]
            fblocks.append(True)
            fro = factors_fro(*lr, n)
            if dg:
                fro = float(np.sqrt(max(fro * fro + fro_dg, 0.0)))
            aa_fro.append(float(np.hypot(fro, sp.linalg.norm(AAi[0]))))
            stored.append(st)
            diag.append(dg)
        else:
            A.append([F])
            AA.append(sp.csr_matrix((n, m * m)))
            C.append(sp.csc_matrix(-F) if sp.issparse(F) else -F)
            sigmaA[:, i] = np.arange(n)
            fblocks.append(True)
            fro = factors_fro(*lr, n)
            aa_fro.append(float(np.sqrt(max(fro * fro + fro_dg, 0.0))) if dg else fro)
            stored.append({})
            diag.append(dg)
    if C_lin is None or C_lin.shape[1] == 0:
        C_lin = sp.csr_matrix((n, 0))
        d_lin = np.zeros(0)
    msizes = np.array([blk[0].shape[0] for blk in A], dtype=np.int64)
    return MyModel(A, AA, [], C, nzA, sigmaA, qA, np.asarray(b, float), float(b_const), np.asarray(d_lin, float),
                   sp.csr_matrix(C_lin), n, msizes, int(C_lin.shape[1]), nlmi, lowrank, "",
                   any(fblocks), True, fblocks, aa_fro, stored, diag=diag)


def _tokens(line):
    for ch in "{}(),":
        line = line.replace(ch, " ")
    return line.split()


def read_sdpa(path):
    """SDPA sparse format: nvar / nblocks / block sizes / c / (mat blk i j val) lines."""
    rows = [ln.strip() for ln in open(path)]
    rows = [ln for ln in rows if ln and ln[0] not in '*"']
    nvar = int(_tokens(rows[0])[0])
    nblk = int(_tokens(rows[1])[0])
    sizes = [int(float(t)) for t in _tokens(rows[2])[:nblk]]
    c, at = [], 3
    while len(c) < nvar:
        c += [float(t) for t in _tokens(rows[at])]
        at += 1
    ent = []
    for ln in rows[at:]:
        t = _tokens(ln)
        if len(t) >= 5:
            ent.append((int(t[0]), int(t[1]), int(t[2]), int(t[3]), float(t[4])))
    return nvar, sizes, np.array(c[:nvar]), ent


def model_from_sdpa(path, datarank=0, kappa=8) -> MyModel:
    """min c'x, sum F_k x_k - F_0 >= 0  ->  A[lmi][0] = F_0, A[lmi][k] = F_k, b = -c;
    diagonal blocks (negative size) -> rows of C_lin = -coef', d_lin = -F_0[ii]
    (src/MOI_wrapper.jl:145-149,179-217)."""
    nvar, sizes, c, ent = read_sdpa(path)
    psd = [k for k, s in enumerate(sizes) if s > 0]
    lmi_id = {blk: i for i, blk in enumerate(psd)}
    lin_base, nlin = {}, 0
    for k, s in enumerate(sizes):
        if s < 0:
            lin_base[k] = nlin
            nlin += -s
    trip = [[([], [], []) for _ in range(nvar + 1)] for _ in psd]
    lr, lc, lv = [], [], []
    d_lin = np.zeros(nlin)
    for mat, blk, i, j, v in ent:
        if v == 0.0:
            continue
        blk -= 1
        if sizes[blk] > 0:
            I, J, V = trip[lmi_id[blk]][mat]
            I.append(i - 1); J.append(j - 1); V.append(v)
            if i != j:
                I.append(j - 1); J.append(i - 1); V.append(v)
        else:
            r = lin_base[blk] + i - 1
            if mat == 0:
                d_lin[r] -= v
            else:
                lr.append(mat - 1); lc.append(r); lv.append(-v)
    A = [[sp.csc_matrix((V, (I, J)), shape=(sizes[blk], sizes[blk])) for (I, J, V) in trip[i]]
         for i, blk in enumerate(psd)]
    C_lin = sp.csr_matrix((lv, (lr, lc)), shape=(nvar, nlin))
    return build_model(A, -c, 0.0, d_lin, C_lin, datarank, kappa)
