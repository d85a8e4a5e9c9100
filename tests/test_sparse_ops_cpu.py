"""The designed inputs of tests/sparse_ops_cases.py hold what they are built for, and a float64 NumPy restatement of the
pattern route (the tables of csrc/model_layout.h, the walks of csrc/dataops.hip, both size regimes, whole and column-sharded)
agrees with the longdouble reference within its bound -- and stops doing so, by a factor of 1e3 at least, under each of
the single faults the inputs are meant to expose.  No device."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparse_ops_cases as sc

SP_LONG = 64
PATTERN_CASES = [n for n in sc.NAMES if n != "P"]


# ---------------------------------------------------------------------------------------------- the restatement
class Tables:
    """What lrn_upload_model builds for one block with nd = 0 (csrc/model_layout.h): stored columns of AA (cq_*), the pattern
    by columns (pc_ptr, pc_r), the twin of every stored position (pc_t), the entry lists in position order (ent_*)."""

    def __init__(self, A, m, sigma):
        A = sp.csr_matrix(A).copy()
        A.eliminate_zeros()
        A.sort_indices()
        Ac = A.tocsc()
        Ac.sort_indices()
        self.m, self.nvar = m, A.shape[0]
        cnt = np.diff(Ac.indptr)
        self.cq_q = np.nonzero(cnt)[0].astype(np.int64)
        self.cq_ptr = np.concatenate([[0], np.cumsum(cnt[self.cq_q])]).astype(np.int64)
        self.cq_j, self.cq_v = Ac.indices.astype(np.int64), Ac.data.copy()
        self.ncq = self.cq_q.size
        self.pc_r = self.cq_q % m
        self.pc_c = self.cq_q // m
        self.pc_ptr = np.concatenate([[0], np.cumsum(np.bincount(self.pc_c, minlength=m))]).astype(np.int64)
        twin = self.pc_c + self.pc_r * m
        pos = np.minimum(np.searchsorted(self.cq_q, twin), self.ncq - 1)
        self.sp_ok = bool((self.cq_q[pos] == twin).all())
        self.pc_t = pos
        nnz = np.diff(A.indptr)[sigma]
        assert (np.diff(nnz) <= 0).all()                            # sigmaA sorted by decreasing nnz
        self.sigma = np.asarray(sigma, dtype=np.int64)
        self.npos_nz = int((nnz > 0).sum())
        self.ent_ptr = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int64)
        idx = np.concatenate([np.arange(A.indptr[s], A.indptr[s + 1]) for s in sigma[:self.npos_nz]])
        key = A.indices[idx].astype(np.int64)
        self.ent_r, self.ent_c, self.ent_v = key % m, key // m, -A.data[idx]
        self.ent_t = np.searchsorted(self.cq_q, key)
        self.long_cols = np.nonzero(np.diff(self.pc_ptr) > SP_LONG)[0]

    def auto_pattern(self):
        """use_sparse_matvec under matvec_sparse = 0"""
        if not self.sp_ok:
            return False
        if self.m < 1500:
            return self.m >= 256 and self.ncq * 12.0 < float(self.m) ** 2 and self.long_cols.size <= 4
        return self.ncq * 60.0 < float(self.m) ** 2


def _within(ptr):
    """index of every element inside its segment"""
    n = np.diff(ptr)
    return np.arange(ptr[-1]) - np.repeat(ptr[:-1], n)


class PatternRoute:
    """matvec_sparse_block in float64: the buffers Mv, N and Zs persist between calls as on the device.  fault: one of
    FAULTS, a single deliberate error."""

    def __init__(self, tab, W):
        self.t, self.W = tab, np.asarray(W)
        m = tab.m
        self.small = m < 1500
        self.N = np.zeros((m, m))                                   # N[r, q]
        self.Zs = np.zeros(tab.ncq)
        self.Mv = np.zeros(tab.ncq)

    def apply(self, x, y, q_lo, q_hi, mirror, fault=None):
        t, W, m = self.t, self.W, self.t.m
        # sp_gather_kernel / sp_gather_sym_kernel: lanes stride the sharers of a position
        prod = t.cq_v * x[t.cq_j]
        if fault == "sharer65":
            prod = prod * (_within(t.cq_ptr) < 64)
        raw = np.add.reduceat(prod, t.cq_ptr[:-1])
        self.Mv = raw.copy() if fault == "nosym" else (raw + raw[t.pc_t]) / 2.0
        if q_hi <= q_lo:
            return
        # sp_wm_small_kernel (q-tiles of 256, row groups of 4, walks 8 deep) / sp_wm_xcd_kernel (64, 16, 4 deep)
        tq, rg, deep = (256, 4, 8) if self.small else (64, 16, 4)
        ntile = (q_hi - q_lo + tq - 1) // tq
        if fault == "qtile":
            ntile -= 1
        qs = np.arange(q_lo, min(q_hi, q_lo + ntile * tq))
        cnt = np.diff(t.pc_ptr)
        use = np.ones(t.ncq, dtype=bool)
        if fault == "tail":
            use = _within(t.pc_ptr) < np.repeat((cnt // deep) * deep, cnt)
        Msp = sp.csr_matrix((self.Mv * use, (t.pc_c, t.pc_r)), shape=(m, m))
        rows = np.ones(m, dtype=bool)
        if self.small:
            rows[t.long_cols] = False
        if fault == "rowtile" and m % rg:
            rows[(m // rg) * rg:] = False
        if qs.size:
            full = Msp @ W[qs, :].T                                 # N[r, q] = sum_t Mv[t] W[q, row(t)]
            self.N[np.ix_(rows, qs)] = full[rows]
        if self.small and fault != "long" and t.long_cols.size:     # sp_wm_long_kernel: one launch per long column, every q
            Mfull = sp.csr_matrix((self.Mv, (t.pc_c, t.pc_r)), shape=(m, m))
            self.N[t.long_cols, q_lo:q_hi] = (Mfull[t.long_cols] @ W[:, q_lo:q_hi])
        # sp_dot_wave_kernel
        sel = np.nonzero((t.pc_c >= q_lo) & (t.pc_c < q_hi) & ((t.pc_r <= t.pc_c) | (not mirror)))[0]
        for s in range(0, sel.size, 4000):
            k = sel[s:s + 4000]
            self.Zs[k] = np.einsum("ij,ij->i", W[:, t.pc_r[k]].T, self.N[:, t.pc_c[k]].T)
        if mirror and fault != "nomirror":
            off = sel[t.pc_r[sel] != t.pc_c[sel]]
            self.Zs[t.pc_t[off]] = self.Zs[off]
        # sp_aa_times_kernel: lanes stride the entry list of a position
        term = t.ent_v * self.Zs[t.ent_t]
        if fault != "stale":
            term = term * ((t.ent_c >= q_lo) & (t.ent_c < q_hi))
        if fault == "entry65":
            term = term * (_within(t.ent_ptr) < 64)
        y[t.sigma[:t.npos_nz]] -= np.add.reduceat(term, t.ent_ptr[:t.npos_nz])


class Restatement:
    """matvec_dev / matvec_partial_dev with every block on the pattern route (matvec_sparse = 2)."""

    def __init__(self, case):
        self.case = case
        self.tabs = [Tables(case.AA[ib], int(case.msizes[ib]), case.sigmaA[:, ib]) for ib in range(case.nlmi)]
        self.routes = [PatternRoute(t, case.W[ib]) for ib, t in enumerate(self.tabs)]

    def _lin(self, x, y):
        c = self.case
        if c.nlin > 0:
            y += c.C_lin @ ((c.X_lin * c.S_lin_inv) * (c.C_lin.T @ x))

    def matvec(self, x, fault=None, only=None):
        y = np.zeros(self.case.nvar)
        for ib, r in enumerate(self.routes):
            r.apply(x, y, 0, r.t.m, True, fault if only in (None, ib) else None)
        self._lin(x, y)
        return y

    def partial(self, x, rank, world, fault=None, only=None):
        y = np.zeros(self.case.nvar)
        for ib, r in enumerate(self.routes):
            r0, r1 = sc.shard_range(r.t.m, rank, world)
            if r1 > r0:
                r.apply(x, y, r0, r1, False, fault if only in (None, ib) else None)
        if rank == 0:
            self._lin(x, y)
        return y


def _ratio(got, ref, bound):
    """largest err_k / (u B_k); a component with B_k = 0 must be exact"""
    err = np.abs(np.asarray(got).astype(sc.LD) - ref)
    assert not np.isnan(err.astype(float)).any()
    zero = bound == 0
    assert (err[zero] == 0).all()
    return float((err[~zero] / (sc.U * bound[~zero])).max()) if (~zero).any() else 0.0


def _worlds(case):
    return (2, 3, 7) if int(case.msizes[0]) >= 1500 else (3, 5)


# ---------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", sc.NAMES)
def test_case_contains_what_it_is_built_for(name):
    case = sc.build_case(name)
    f = sc.features(case)
    m = int(case.msizes[0])
    tab = Tables(case.AA[0], m, case.sigmaA[:, 0])
    d = case.design[0]
    assert f.ncq <= 25000 and f.ncq == tab.ncq
    assert case.dense_threshold > f.e_max                           # nd = 0
    assert tab.sp_ok == f.symmetric == (name != "P")
    counts = set(f.colcount.tolist())
    lists = set(f.lists.tolist())
    sharers = set(f.sharers.values())
    if name == "P":
        i, j = d.lone_key % m, d.lone_key // m
        assert i != j and d.lone_key not in f.sharers and (j + i * m) in f.sharers
        return
    assert set(sc.COUNTS) <= counts
    for col, cnt in d.targets.items():
        assert f.colcount[col] == cnt
    assert set(sc.LISTS) <= lists and 0 in lists
    i, j = d.shared_off
    assert i != j and f.sharers[j * m + i] == sc.SHARED_OFF and f.sharers[i * m + j] == sc.SHARED_OFF
    assert f.sharers[d.shared_diag * (m + 1)] == sc.SHARED_DIAG
    assert {sc.SHARED_OFF, sc.SHARED_DIAG} <= sharers and f.s_max == sc.SHARED_OFF
    assert any(k % m == k // m and f.lists[r] == 1 for r in np.nonzero(f.lists == 1)[0] for k in case.AA[0][r].indices)
    nlong = int((f.colcount > SP_LONG).sum())
    assert f.colcount[m - 3:].min() > 0                             # the last q-tile and row group hold entries
    if m < 1500:
        assert m == 259 and f.colcount[0] == 0 and (f.colcount == 0).sum() >= 3
        assert 12 * f.ncq < m * m
        assert nlong >= 6 if name == "S" else nlong <= 4
        assert tab.auto_pattern() == (name != "S")
    else:
        assert f.colcount[d.arrow] == m and f.colcount.min() >= 1 and f.lists.max() == 2 * m - 1
        assert case.xs[1][int(np.argmax(f.lists))] == 1.0           # e_{nvar-1} is the arrow constraint
        assert tab.auto_pattern()
        assert (m % 16 == 12 and m % 64 == 28) if m == 1500 else (m % 64 == 0)
    if name.startswith("A-"):
        A = case.AA[0].tocoo()
        B = sp.csr_matrix((A.data, (A.row, (A.col % m) * m + A.col // m)), shape=A.shape)
        diff = (case.AA[0] - B).tocoo()
        changed = np.unique(diff.col[diff.data != 0])
        off = f.keys[f.keys % m != f.keys // m]
        assert 0.08 < changed.size / off.size < 0.12                # a tenth of the off-diagonal positions differ from their twin
    if name == "B2":
        f2 = sc.features(case, 1)
        t2 = Tables(case.AA[1], 40, case.sigmaA[:, 1])
        assert case.nlin == 5 and t2.sp_ok and not t2.auto_pattern() and (f2.lists == 0).sum() > case.nvar // 2


def test_exact_matmul_is_exact():
    rng = np.random.default_rng(1)
    A = rng.standard_normal((23, 300)) * np.exp(rng.uniform(-8, 8, (23, 300)))
    B = rng.standard_normal((300, 17)) * np.exp(rng.uniform(-8, 8, (300, 17)))
    ref = A.astype(sc.LD) @ B.astype(sc.LD)
    bound = np.abs(A).astype(sc.LD) @ np.abs(B).astype(sc.LD)
    assert (np.abs(sc.exact_matmul(A, B) - ref) <= 2.0 ** -60 * bound).all()
    assert (np.abs(A @ B - ref) > 2.0 ** -56 * bound).any()         # (float64 alone is not)


@pytest.mark.parametrize("name", ["S", "L"])
def test_reference_agrees_with_dense_float64(name):
    case = sc.build_case(name)
    m = int(case.msizes[0])
    for x in case.xs:
        M = (case.AA[0].T @ x).reshape(m, m, order="F")
        M = 0.5 * (M + M.T)
        dense = case.AA[0] @ (case.W[0] @ M @ case.W[0]).reshape(-1, order="F")
        ref = sc.ref_operator(case, case.W, x).astype(float)
        assert np.linalg.norm(dense - ref) <= 1e-12 * np.linalg.norm(ref)
        assert np.allclose(sc.ref_mat(case, x).astype(float), M, rtol=0, atol=1e-13 * np.abs(M).max())


@pytest.mark.parametrize("name", PATTERN_CASES)
def test_restatement_within_the_bound_whole_and_sharded(name):
    case = sc.build_case(name)
    rs = Restatement(case)
    g = sc.gamma(sc.depth(case)) / sc.U
    worst = 0.0
    for x in case.xs:
        ref, B = sc.ref_operator(case, case.W, x), sc.ref_bound(case, case.W, x)
        y = rs.matvec(x)
        worst = max(worst, _ratio(y, ref, B))
        assert np.array_equal(y, rs.matvec(x))
    x = case.xs[0]
    for world in _worlds(case):
        acc = np.zeros(case.nvar, dtype=sc.LD)                      # (the ranks' vectors added in longdouble: every share is within gamma_L B_r, and the B_r add up to B)
        for rank in range(world):
            cols = [sc.shard_range(int(m), rank, world) for m in case.msizes]
            part = rs.partial(x, rank, world)
            worst = max(worst, _ratio(part, sc.ref_operator(case, case.W, x, cols=cols, lin=rank == 0),
                                      sc.ref_bound(case, case.W, x, cols=cols, lin=rank == 0)))
            acc += part
        worst = max(worst, _ratio(acc, sc.ref_operator(case, case.W, x), sc.ref_bound(case, case.W, x)))
    print("SPOPS-CPU %s restatement max err/(u B) = %.2f of %.0f (L = %d)" % (name, worst, g, sc.depth(case)))
    assert worst <= g


def test_rows_and_columns_of_a_shard_add_up():
    """the reference restricted to the rows (dense route) or the columns (pattern route) of the ranks sums to the whole"""
    case = sc.build_case("S4")
    x, m = case.xs[0], int(case.msizes[0])
    whole = sc.ref_operator(case, case.W, x)
    for kw in ("cols", "rows"):
        acc = sum(sc.ref_operator(case, case.W, x, **{kw: [sc.shard_range(m, r, 5)]}) for r in range(5))
        assert float(np.abs(acc - whole).max()) <= 1e-17 * float(np.abs(whole).max())


# ---------------------------------------------------------------------------------------------- sensitivity
# fault -> (regime it exists in: "small", "large" or None for both; whole / sharded; cases it does not apply to)
FAULTS = {
    "tail": (None, "both"),            # the tail of a column walk dropped (count no multiple of 8 / of 4)
    "long": ("small", "both"),         # the > 64 column skipped
    "nosym": (None, "both"),           # pc_t ignored
    "sharer65": (None, "both"),        # the 65th sharer of a position dropped
    "entry65": (None, "both"),         # the 65th entry of a list dropped
    "qtile": (None, "both"),           # the last q-tile of a range dropped
    "rowtile": (None, "both"),         # the last short row tile dropped
    "nomirror": (None, "whole"),       # mirror copies omitted
    "stale": (None, "sharded"),        # an out-of-range column's stale Zs read
}


def _applies(fault, name, m):
    regime, _ = FAULTS[fault]
    if regime == "small" and m >= 1500:
        return False
    if fault == "nosym":
        return name.startswith("A-")
    if fault == "rowtile":
        return m % (4 if m < 1500 else 16) != 0
    return True


@pytest.mark.parametrize("fault", list(FAULTS))
@pytest.mark.parametrize("name", PATTERN_CASES)
def test_single_fault_breaks_the_bound(name, fault):
    case = sc.build_case(name)
    m = int(case.msizes[0])
    if not _applies(fault, name, m):
        return
    rs = Restatement(case)
    x, prime = case.xs[0], case.xs[2] + 0.5 * case.xs[0]
    g = sc.gamma(sc.depth(case))
    rs.matvec(prime)                                                # N and Zs hold another vector's values
    world = _worlds(case)[0]
    found = 0.0
    if FAULTS[fault][1] in ("both", "whole"):
        ref, B = sc.ref_operator(case, case.W, x), sc.ref_bound(case, case.W, x)
        err = np.abs(rs.matvec(x, fault, only=0).astype(sc.LD) - ref)
        found = float((err[B > 0] / (g * B[B > 0])).max())
        if FAULTS[fault][1] == "both":
            assert found >= 1e3, (name, fault, "whole", found)
    if FAULTS[fault][1] in ("both", "sharded"):
        rs.matvec(prime)
        worst = 0.0
        for rank in range(world):
            cols = [sc.shard_range(int(mm), rank, world) for mm in case.msizes]
            ref = sc.ref_operator(case, case.W, x, cols=cols, lin=rank == 0)
            B = sc.ref_bound(case, case.W, x, cols=cols, lin=rank == 0)
            err = np.abs(rs.partial(x, rank, world, fault, only=0).astype(sc.LD) - ref)
            worst = max(worst, float((err[B > 0] / (g * B[B > 0])).max()))
        found = max(found, worst) if FAULTS[fault][1] != "both" else min(found, worst)
    print("SPOPS-CPU %s fault %s: err / (gamma_L B) = %.1e" % (name, fault, found))
    assert found >= 1e3, (name, fault, found)
