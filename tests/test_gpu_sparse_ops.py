"""GPU: the stored-entry data operators of csrc/dataops.hip against the longdouble reference of tests/sparse_ops_cases.py,
in both size regimes (msz 259: sp_gather_sym / sp_wm_small / sp_wm_long; msz 1500 and 1536: sp_gather / sp_symmetrize /
sp_wm_xcd), whole and sharded, with the route that ran read off the counters op_sparse_pattern and op_wmw_pattern.

Every comparison is per component: |y_k - ref_k| <= gamma_L B_k, B the reference's chain on absolute values, L the depth of
the nest of sums (sc.depth: s_max + 2 msz + e_max + 8 for the operator).  The largest observed err_k / (u B_k) is printed
per case and route (lines SPOPS); these figures are information, the bound is gamma_L / u ~ L.

Observed on an MI355X, largest err / (u B) over the three x, dense / pattern route (L):
  S 8.9 / 4.0 (785)   S4 3.7 / 3.4 (785)   L 39.6 / 7.6 (6137)   L64 33.1 / 6.0 (6281)   A-S 6.4 / 3.2 (785)
  A-L 40.8 / 5.3 (6137)   P 3.7 / - (785)   B2 41.3 / 4.9 (6137);  a rank's share: at most 20.9 / 7.6;
  mat(AA'x) at most 1.8 (L = 134), AA vec(X) at most 2.0 (L = e_max + 4);
  resident right-hand side on L: 11.9 by two products, 5.9 on the pattern (L = 6003)."""
import numpy as np
import pytest

import sparse_ops_cases as sc

pytestmark = pytest.mark.gpu

# auto route (matvec_sparse = 0): pattern blocks per application
AUTO = {"S": 0, "S4": 1, "L": 1, "L64": 1, "A-S": 1, "A-L": 1, "P": 0, "B2": 1}
FORCED = {"S": 1, "S4": 1, "L": 1, "L64": 1, "A-S": 1, "A-L": 1, "P": 0, "B2": 2}
WORLDS = {"L": (2, 3, 7), "L64": (2, 3, 7), "A-L": (2, 3, 7), "B2": (2, 3, 7), "S4": (3, 5), "A-S": (3, 5), "S": (3, 5)}


@pytest.fixture(scope="module")
def dev():
    import loraine_jl_amd
    d = loraine_jl_amd.Device(0)
    yield d
    d.close()


def _upload(dev, case):
    """every constraint stored by its entries (nd = 0): the threshold of the dense slots above the longest list"""
    dev.set_option("dense_threshold", case.dense_threshold)
    try:
        dev.upload_model(case.AA, case.sigmaA, case.qA, case.msizes, C_lin=case.C_lin)
    finally:
        dev.set_option("dense_threshold", -1)
    for ib in range(case.nlmi):
        dev.set_scaling(ib, case.W[ib], case.G[ib])
    if case.nlin:
        dev.set_lin(case.X_lin, case.S_lin_inv)


def _check(tag, got, ref, B, L):
    """|got - ref| <= gamma_L B per component (exact where B = 0); -> the largest err / (u B)"""
    got = np.asarray(got)
    assert np.isfinite(got).all(), tag
    err = np.abs(got.astype(sc.LD) - ref)
    pos = B > 0
    ratio = float((err[pos] / (sc.U * B[pos])).max()) if pos.any() else 0.0
    print("SPOPS %-40s max err/(u B) = %8.2f   L = %d" % (tag, ratio, L))
    assert (err[~pos] == 0).all(), tag
    assert (err <= sc.gamma(L) * B).all(), (tag, ratio, L)
    return ratio


def _sym(m, rng):
    A = rng.standard_normal((m, m))
    return (A + A.T) / 2


def _gram(m, rng):
    Q = rng.standard_normal((m, m)) / np.sqrt(m)
    A = Q @ Q.T
    return (A + A.T) / 2                                            # (exactly symmetric, whatever the BLAS does)


def _shards(case, rank, world):
    return [sc.shard_range(int(m), rank, world) for m in case.msizes]


@pytest.mark.parametrize("name", sc.NAMES)
def test_mat_of_AAt_x_and_AA_times(dev, name):
    """mat(AA'y) through Rd = C - S - mat(AA'y) (aat_gather_kernel; symmetrize_kernel at msz 259 and 40,
    symmetrize_tiled_kernel with edge tiles at 1500) and AA vec(X) (aa_times_kernel: lists of 1 to 2 msz - 1 entries, the
    empty constraint exactly 0), X not symmetric."""
    case = sc.build_case(name)
    rng = np.random.default_rng(7)
    _upload(dev, case)
    Cs = [_sym(int(m), rng) for m in case.msizes]
    Ss = [_sym(int(m), rng) for m in case.msizes]
    Xs = [rng.standard_normal((int(m), int(m))) for m in case.msizes]
    for ib in range(case.nlmi):
        dev.ip_set_c(ib, Cs[ib])
        dev.ip_set_iterate(ib, Xs[ib], Ss[ib])
    for ix, y in enumerate(case.xs):
        dev.ip_residual_d(y)
        for ib in range(case.nlmi):
            Rd = dev.dbg_get_block(ib, "Rd")[0]
            assert np.array_equal(Rd, Rd.T)
            ref = Cs[ib].astype(sc.LD) - Ss[ib].astype(sc.LD) - sc.ref_mat(case, y, ib)
            B = np.abs(Cs[ib]).astype(sc.LD) + np.abs(Ss[ib]).astype(sc.LD) + sc.ref_mat(case, y, ib, absolute=True)
            _check("%s mat x%d block %d" % (name, ix, ib), Rd, ref, B, sc.depth_mat(case))
    aax = dev.ip_aa_x()
    assert np.array_equal(aax, dev.ip_aa_x())
    _check("%s aa_times" % name, aax, sc.ref_aa_times(case, Xs), sc.ref_aa_times(case, Xs, absolute=True), sc.depth_aa(case))
    lists = sum(np.diff(A.indptr) for A in case.AA)
    assert (lists == 0).any() and (aax[lists == 0] == 0).all()


@pytest.mark.parametrize("name", sc.NAMES)
def test_operator_by_every_route(dev, name):
    """dense route (matvec_sparse = 1), forced pattern route (2), automatic (0): each within the bound, and the route that
    ran is the one use_sparse_matvec prescribes (counter op_sparse_pattern, +1 per pattern block and application)."""
    case = sc.build_case(name)
    _upload(dev, case)
    L = sc.depth(case)
    try:
        dev.set_option("matvec_h", 1)
        for ix, x in enumerate(case.xs):
            ref, B = sc.ref_operator(case, case.W, x), sc.ref_bound(case, case.W, x)
            for mode, route, want in ((1, "dense", 0), (2, "pattern", FORCED[name]), (0, "auto", AUTO[name])):
                dev.set_option("matvec_sparse", mode)
                n0 = dev.count("op_sparse_pattern")
                y = dev.matvec(x)
                assert dev.count("op_sparse_pattern") == n0 + want, (name, route)
                _check("%s x%d %s" % (name, ix, route), y, ref, B, L)
    finally:
        dev.set_option("matvec_sparse", 0)
        dev.set_option("matvec_h", 0)


@pytest.mark.parametrize("name", list(WORLDS))
def test_shards_by_columns_and_by_rows(dev, name):
    """set_shard + matvec_partial: under the pattern route a rank owns the pattern columns [r0, r1) of Z (q ranges of less
    than one sweep of 8 q-tiles at world 7, a half-filled second sweep at world 2), under the dense route the rows
    (aa_times_rows_kernel); the linear term comes from rank 0; the shares add up to the whole."""
    case = sc.build_case(name)
    _upload(dev, case)
    L = sc.depth(case)
    x = case.xs[0]
    whole, wholeB = sc.ref_operator(case, case.W, x), sc.ref_bound(case, case.W, x)
    modes = [(2, "pattern"), (1, "dense")] + ([(0, "auto")] if name == "B2" else [])
    plans = [(w, range(w)) for w in WORLDS[name]]
    if name == "S4":
        m = int(case.msizes[0])
        plans.append((m + 5, (0, m - 1, m, m + 4)))                 # one column per rank; the last five own nothing
    try:
        dev.set_option("matvec_h", 1)
        for mode, route in modes:
            dev.set_option("matvec_sparse", mode)
            for world, ranks in plans:
                acc = np.zeros(case.nvar, dtype=sc.LD)
                worst = 0.0
                for rank in ranks:
                    dev.set_shard(rank, world)
                    n0 = dev.count("op_sparse_pattern")
                    part = dev.matvec_partial(x)
                    owns = [r1 > r0 for r0, r1 in _shards(case, rank, world)]
                    pattern = [route == "pattern" or (route == "auto" and ib == 0) for ib in range(case.nlmi)]
                    assert dev.count("op_sparse_pattern") == n0 + sum(o and p for o, p in zip(owns, pattern))
                    sh = _shards(case, rank, world)
                    cols = [s if p else None for s, p in zip(sh, pattern)]
                    rows = [None if p else s for s, p in zip(sh, pattern)]
                    ref = sc.ref_operator(case, case.W, x, cols=cols, rows=rows, lin=rank == 0)
                    B = sc.ref_bound(case, case.W, x, cols=cols, rows=rows, lin=rank == 0)
                    if not any(owns) and not (rank == 0 and case.nlin):
                        assert not part.any()
                    err = np.abs(part.astype(sc.LD) - ref)
                    assert (err <= sc.gamma(L) * B).all(), (name, route, world, rank)
                    pos = B > 0
                    if pos.any():
                        worst = max(worst, float((err[pos] / (sc.U * B[pos])).max()))
                    acc += part
                print("SPOPS %-40s max err/(u B) = %8.2f   L = %d" % ("%s shards %s world %d" % (name, route, world), worst, L))
                if len(ranks) == world:                             # (the ranks' vectors added in longdouble: the B_r add up to B)
                    _check("%s sum %s world %d" % (name, route, world), acc, whole, wholeB, L)
    finally:
        dev.set_shard(0, 1)
        dev.set_option("matvec_sparse", 0)
        dev.set_option("matvec_h", 0)


@pytest.mark.parametrize("name", ["S", "S4", "L", "L64", "A-L", "B2"])
def test_same_bits_whatever_ran_before(dev, name):
    """No atomics, and no stale column of N or entry of Zs is read: the same call twice gives the same bits, and the whole
    operator gives the same bits after a run of partials and after a dense-route application of another vector."""
    case = sc.build_case(name)
    _upload(dev, case)
    x, other = case.xs[0], case.xs[2] + 0.5 * case.xs[0]
    world = WORLDS[name][-1]
    try:
        dev.set_option("matvec_h", 1)
        dev.set_option("matvec_sparse", 2)
        y0 = dev.matvec(x)
        assert np.array_equal(y0, dev.matvec(x))
        parts = []
        for rank in range(world):
            dev.set_shard(rank, world)
            parts.append(dev.matvec_partial(other))
            assert np.array_equal(parts[-1], dev.matvec_partial(other))
        dev.set_shard(0, 1)
        assert np.array_equal(y0, dev.matvec(x))
        dev.set_option("matvec_sparse", 1)
        d0 = dev.matvec(other)
        assert np.array_equal(d0, dev.matvec(other))
        dev.set_option("matvec_sparse", 2)
        assert np.array_equal(y0, dev.matvec(x))
        for rank in range(world):                                   # ... and the partials after a whole application
            dev.set_shard(rank, world)
            assert np.array_equal(parts[rank], dev.matvec_partial(other))
    finally:
        dev.set_shard(0, 1)
        dev.set_option("matvec_sparse", 0)
        dev.set_option("matvec_h", 0)


def test_resident_right_hand_side_on_the_pattern(dev):
    """AA vec(W (Rd + S) W) of the resident loop on L: one product and dots on the pattern (aa_times_wmw_pattern, counter
    op_wmw_pattern) at the default wmw_pattern_min, two products with wmw_pattern_min above msz; both against the
    reference built from the device's own W and Rd.  lrn_ip_rhs_pred2 is the entry point that takes the pattern form;
    lrn_ip_rhs_pred always runs both products and is held to the same bound."""
    case = sc.build_case("L")
    m = int(case.msizes[0])
    rng = np.random.default_rng(11)
    _upload(dev, case)
    X = np.eye(m) + 0.3 * _gram(m, rng)
    S = np.eye(m) + 0.3 * _gram(m, rng)
    dev.ip_set_c(0, _sym(m, rng) / np.sqrt(m))
    dev.ip_set_iterate(0, X, S)
    assert dev.ip_prepare_w(0) == 0
    dev.ip_residual_d(0.1 * case.xs[0])
    try:
        n0 = dev.count("op_wmw_pattern")
        _, by_pattern = dev.ip_rhs_pred2()
        assert dev.count("op_wmw_pattern") == n0 + 1
        dev.set_option("wmw_pattern_min", m + 1)
        _, by_products = dev.ip_rhs_pred2()
        single = dev.ip_rhs_pred()
        assert dev.count("op_wmw_pattern") == n0 + 1
    finally:
        dev.set_option("wmw_pattern_min", 1500)
    W = dev.dbg_get_block(0, "W")[0]
    Rd = dev.dbg_get_block(0, "Rd")[0]
    assert np.array_equal(W, W.T) and np.array_equal(Rd, Rd.T)
    Mhi = Rd + S                                                    # Rd + S = Mhi + Mlo exactly (two-sum)
    bb = Mhi - Rd
    Mlo = (Rd - (Mhi - bb)) + (S - bb)
    N = sc.exact_matmul(Mhi, W) + (Mlo @ W).astype(sc.LD)
    Nbar = (np.abs(Mhi) @ np.abs(W)).astype(sc.LD)
    A = case.AA[0].tocoo()
    p, q = A.col % m, A.col // m
    Wl, Wa = W.astype(sc.LD), np.abs(W).astype(sc.LD)
    ukeys, inv = np.unique(A.col, return_inverse=True)
    Zu, Zb = np.zeros(ukeys.size, dtype=sc.LD), np.zeros(ukeys.size, dtype=sc.LD)
    Nt, Nbt = np.ascontiguousarray(N.T), np.ascontiguousarray(Nbar.T)
    for s in range(0, ukeys.size, 2000):
        kk = ukeys[s:s + 2000]
        Zu[s:s + 2000] = np.einsum("ij,ij->i", Wl[kk % m, :], Nt[kk // m, :])
        Zb[s:s + 2000] = np.einsum("ij,ij->i", Wa[kk % m, :], Nbt[kk // m, :])
    ref, B = np.zeros(case.nvar, dtype=sc.LD), np.zeros(case.nvar, dtype=sc.LD)
    np.add.at(ref, A.row, A.data.astype(sc.LD) * Zu[inv])
    np.add.at(B, A.row, np.abs(A.data).astype(sc.LD) * Zb[inv])
    L = 2 * m + sc.features(case).e_max + 4
    _check("L rhs pattern", by_pattern, ref, B, L)
    _check("L rhs two products", by_products, ref, B, L)
    _check("L rhs ip_rhs_pred", single, ref, B, L)
