"""What lrn_upload_model, lrn_upload_lowrank and lrn_upload_diag put on the device, pinned without one.  Every kernel reads
the arrays laid out by csrc/model_layout.h; the GPU tests only see numbers computed from them, and a wrong pc_t, ent_t,
q_wave or sp_long_cols that merely picks a slower or differently rounded route would pass them all.  lrn_dbg_model_layout and
lrn_dbg_factor_layout run the planner on caller arrays and hand back any array by name.

The reference is a NumPy / SciPy statement of the definitions in the comments of csrc/ctx.h (sorting, masking, searchsorted
on whole matrices), not a port of the planner's loops.  Everything is compared exactly: integers, values that are copies or
negations, and the lp_w products, each one multiplication of the same two doubles.

Golden models through model_from_sdpa with datarank = -1 where the data has rank-one form (tru3, maxG11: the rank-one
layout) and 0 where the reader refuses it (theta1, control1, vib3); control1 and vib3 have two blocks (natural order of
hidx, hrow, cl_row), tru3 and vib3 a linear block of 72 columns."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import loraine_jl_amd
from loraine_jl_amd.model import model_from_sdpa
import model_layout_cases as mc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REAL = {"ent_v", "cq_v", "b_val", "lp_w", "cr_val", "v_val", "v_w"}
BIG = 1 << 40


# ---------------------------------------------------------------------------------------------- the two entry points
def _csc(M):
    """(colptr, rowval, nzval) of a scipy CSC matrix as it stands, 1-based int64"""
    if M is None:
        return None, None, None
    return (M.indptr.astype(np.int64) + 1, M.indices.astype(np.int64) + 1, np.ascontiguousarray(M.data, dtype=np.float64))


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _fetch(fn, name, args):
    """(rc, message, array): one call for the length, one for the elements"""
    cnt = C.c_int64(0)
    msg = C.create_string_buffer(1024)
    rc = fn(name.encode(), *args, C.byref(cnt), None, None, msg, len(msg))
    if rc != 0:
        return rc, msg.value.decode(), None
    out = np.zeros(cnt.value, dtype=np.float64 if name in REAL else np.int64)
    rc = fn(name.encode(), *args, C.byref(cnt), *((None, _p(out)) if name in REAL else (_p(out), None)), msg, len(msg))
    assert rc == 0 and cnt.value == out.size
    return rc, "", out


def model_layout(name, m, AA, sigma, qA, pos_space=True, dense_threshold=-1.0, free_bytes=BIG, B=None, Clin=None, raw=False):
    lib = loraine_jl_amd.load_library()
    cp, rv, nz = AA if isinstance(AA, tuple) else _csc(AA)
    nvar = len(sigma)
    sig = np.asarray(sigma, dtype=np.int64) + 1
    bc, br, bv = _csc(B)
    lc, lr, lv = Clin if isinstance(Clin, tuple) else _csc(Clin)
    nlin = 0 if lc is None else len(lc) - 1
    args = (m, nvar, _p(cp), _p(rv), _p(nz), _p(sig), int(qA), int(pos_space), float(dense_threshold), int(free_bytes),
            _p(bc), _p(br), _p(bv), nlin, _p(lc), _p(lr), _p(lv))
    rc, msg, out = _fetch(lib.lrn_dbg_model_layout, name, args)
    if raw:
        return rc, msg
    assert rc == 0, msg
    return out


def factor_layout(name, m, ipos, npos_nz, pos_space, khat=0, V=None, d=None, rows=None, raw=False):
    lib = loraine_jl_amd.load_library()
    ip = np.asarray(ipos, dtype=np.int64)
    vc, vr, vv = V if isinstance(V, tuple) else _csc(V)
    dd = None if d is None else np.ascontiguousarray(d, dtype=np.float64)
    rw = None if rows is None else np.asarray(rows, dtype=np.int64)
    args = (m, len(ip), _p(ip), int(npos_nz), int(pos_space), int(khat), _p(vc), _p(vr), _p(vv), _p(dd),
            0 if rw is None else len(rw), _p(rw))
    rc, msg, out = _fetch(lib.lrn_dbg_factor_layout, name, args)
    if raw:
        return rc, msg
    assert rc == 0, msg
    return out


# ---------------------------------------------------------------------------------------------- the specification
def spec_block(m, AA, sigma, qA, pos_space, dense_threshold, free_bytes):
    """ctx.h, LmiBlock: position p <-> constraint sigma[p]; entry lists in position order with the value of A = -AA; the
    dense prefix [0, nd), the wave range [nd, q_wave); the stored columns of AA over the non-dense constraints; the pattern of
    mat(AA'x) when nothing is dense and the pattern is symmetric."""
    R = sp.csr_matrix(AA).copy()
    R.eliminate_zeros()
    R.sort_indices()
    nvar = R.shape[0]
    sigma = np.asarray(sigma)
    s = {"sigma": sigma, "ipos": np.argsort(sigma), "hidx": np.arange(nvar) if pos_space else sigma}
    nnz = np.diff(R.indptr)[sigma]
    s["nnz"], s["qA"], s["npos_nz"] = nnz, min(max(int(qA), 0), nvar), int(np.count_nonzero(nnz))
    P = R[sigma]                                                       # rows in position order
    s["ent_ptr"] = P.indptr
    s["ent_r"], s["ent_c"], s["ent_v"] = P.indices % m, P.indices // m, -P.data
    # dense prefix: the leading run of dense positions below qA and npos_nz, at most 0.55 free_bytes of matrices
    suffix = np.concatenate([np.cumsum(nnz[::-1])[::-1], [0]]).astype(float)
    if dense_threshold >= 0:
        dense = nnz.astype(float) >= dense_threshold
    else:
        p = np.arange(nvar)
        dense = nnz * suffix[:-1] / 1.0e11 > 3.0 * m * m * m / 2.0e13 + (nvar - p) * float(m) * m / 2.0e13 + 2e-5
    lim = min(s["qA"], s["npos_nz"], int(free_bytes * 0.55 / (m * m * 8.0)))
    run = int(np.argmin(np.append(dense, False)))                      # first position that is not dense
    s["nd"] = nd = min(run, lim)
    s["q_wave"] = max(nd, min(s["npos_nz"], int(np.count_nonzero(nnz > 4))))
    # stored columns of the non-dense constraints, rows (natural numbers) ascending, the value of AA
    keep = sp.diags((s["ipos"] >= nd).astype(float)) @ R
    Kc = sp.csc_matrix(keep)
    Kc.eliminate_zeros()
    Kc.sort_indices()
    cnt = np.diff(Kc.indptr)
    cq_q = np.nonzero(cnt)[0]
    s["cq_q"], s["cq_ptr"], s["cq_j"], s["cq_v"] = cq_q, np.concatenate([[0], np.cumsum(cnt[cq_q])]), Kc.indices, Kc.data
    twin = cq_q // m + (cq_q % m) * m
    s["sp_ok"] = int(nd == 0 and cq_q.size > 0 and bool(np.isin(twin, cq_q).all()))
    if s["sp_ok"]:
        s["pc_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(cq_q // m, minlength=m))])
        s["pc_r"], s["pc_t"] = cq_q % m, np.searchsorted(cq_q, twin)
        s["ent_t"] = np.searchsorted(cq_q, P.indices)
        s["sp_long_cols"] = np.nonzero(np.diff(s["pc_ptr"]) > 64)[0]
    else:
        for k in ("pc_ptr", "pc_r", "pc_t", "ent_t", "sp_long_cols"):
            s[k] = np.zeros(0, dtype=np.int64)
    return s


def spec_rank_one(B, sigma, pos_space):
    """CSR by H index: row h is the factor of constraint sigma[h] in position space, of constraint h otherwise"""
    Bh = sp.csr_matrix(B)[np.asarray(sigma)] if pos_space else sp.csr_matrix(B).copy()
    Bh.sort_indices()
    return {"b_ptr": Bh.indptr, "b_col": Bh.indices, "b_val": Bh.data}


def spec_linear(Clin, ipos, pos_space):
    """ctx.h, lrn_ctx: C_lin by linear constraint with Schur-matrix and natural rows; every lower-triangle target of
    C_lin diag(xs) C_lin' with its (l, C_il C_jl); C_lin by natural rows"""
    Cc = sp.csc_matrix(Clin).copy()
    Cc.sort_indices()
    nvar, nlin = Cc.shape
    hrow = np.asarray(ipos) if pos_space else np.arange(nvar)
    s = {"cl_ptr": Cc.indptr, "cl_rown": Cc.indices, "cl_row": hrow[Cc.indices]}
    Ch = np.zeros((nvar, nlin))
    Ch[hrow[Cc.indices], np.repeat(np.arange(nlin), np.diff(Cc.indptr))] = Cc.data
    T = {}                                                             # (c, r) -> [(l, w)], l ascending
    for l in range(nlin):
        rows = np.nonzero(Ch[:, l])[0]
        for r in rows:
            for c in rows[rows <= r]:
                T.setdefault((int(c), int(r)), []).append((l, Ch[r, l] * Ch[c, l]))
    keys = sorted(T)
    s["lp_c"], s["lp_r"] = np.array([k[0] for k in keys], dtype=int), np.array([k[1] for k in keys], dtype=int)
    s["lp_ptr"] = np.concatenate([[0], np.cumsum([len(T[k]) for k in keys])]).astype(int)
    s["lp_l"] = np.array([l for k in keys for l, _ in T[k]], dtype=int)
    s["lp_w"] = np.array([w for k in keys for _, w in T[k]], dtype=float)
    Cr = sp.csr_matrix(Cc)
    Cr.sort_indices()
    s["cr_ptr"], s["cr_col"], s["cr_val"] = Cr.indptr, Cr.indices, Cr.data
    return s


def spec_lowrank(V, d, khat, ipos, pos_space):
    """CSR by factor column h khat + p in H index order (h = position of the constraint in position space), weights alike"""
    nvar = len(ipos)
    hrow = np.asarray(ipos) if pos_space else np.arange(nvar)
    src = np.empty(nvar * khat, dtype=int)                             # U column -> row of V
    src[(hrow[:, None] * khat + np.arange(khat)).ravel()] = np.arange(nvar * khat)
    Vh = sp.csr_matrix(V)[src]
    Vh.sort_indices()
    return {"v_ptr": Vh.indptr, "v_col": Vh.indices, "v_val": Vh.data, "v_w": np.asarray(d, dtype=float)[src]}


BLOCK_NAMES = ["sigma", "ipos", "nnz", "qA", "npos_nz", "nd", "q_wave", "ent_ptr", "ent_r", "ent_c", "ent_v", "hidx", "cq_q",
               "cq_ptr", "cq_j", "cq_v", "sp_ok", "pc_ptr", "pc_r", "pc_t", "ent_t", "sp_long_cols"]


def same(got, want, what):
    want = np.atleast_1d(np.asarray(want))
    assert got.shape == want.shape and np.array_equal(got, want.astype(got.dtype)), (what, got[:12], want[:12])


def check_block(m, AA, sigma, qA, pos_space=True, dense_threshold=-1.0, free_bytes=BIG):
    s = spec_block(m, AA, sigma, qA, pos_space, dense_threshold, free_bytes)
    g = {n: model_layout(n, m, AA, sigma, qA, pos_space, dense_threshold, free_bytes) for n in BLOCK_NAMES}
    for n in BLOCK_NAMES:
        same(g[n], s[n], n)
    # invariants
    assert np.array_equal(g["ent_ptr"], np.concatenate([[0], np.cumsum(g["nnz"])]))
    assert np.array_equal(g["ipos"][g["sigma"]], np.arange(len(sigma)))
    assert (np.diff(g["cq_q"]) > 0).all()
    if g["sp_ok"][0]:
        assert np.array_equal(g["pc_t"][g["pc_t"]], np.arange(g["pc_t"].size))
    return {k: (v[0] if k in ("qA", "npos_nz", "nd", "q_wave", "sp_ok") else v) for k, v in g.items()}


def check_linear(m, AA, sigma, pos_space, Clin):
    s = spec_linear(Clin, np.argsort(sigma), pos_space)
    g = {n: model_layout(n, m, AA, sigma, 0, pos_space, Clin=Clin) for n in s}
    for n in s:
        same(g[n], s[n], n)
    tgt = np.stack([g["lp_c"], g["lp_r"]], axis=1)
    assert (g["lp_r"] >= g["lp_c"]).all() and len({tuple(t) for t in tgt}) == len(tgt)
    assert [tuple(t) for t in tgt] == sorted(tuple(t) for t in tgt)                        # by (column, row)
    return g


# ---------------------------------------------------------------------------------------------- golden models
@pytest.fixture(scope="module", params=["theta1", "control1", "tru3", "vib3", "maxG11"])
def golden(request):
    name = request.param
    return name, model_from_sdpa(os.path.join(GOLDEN, name + ".dat-s"), datarank=-1 if name in ("tru3", "maxG11") else 0)


def test_golden_models(golden):
    name, mdl = golden
    pos_space = mdl.nlmi == 1
    assert (mdl.nlmi > 1) == (name in ("control1", "vib3")) and (mdl.nlin > 0) == (name in ("tru3", "vib3"))
    for il in range(mdl.nlmi):
        m, AA, sigma = int(mdl.msizes[il]), sp.csc_matrix(mdl.AA[il]), mdl.sigmaA[:, il]
        AA.sort_indices()
        g = check_block(m, AA, sigma, mdl.qA[0, il], pos_space)
        same(g["hidx"], np.arange(mdl.n) if pos_space else sigma, "hidx")
        if len(mdl.B):
            B = sp.csc_matrix(mdl.B[il])
            B.sort_indices()
            s = spec_rank_one(B, sigma, pos_space)
            for n in s:
                same(model_layout(n, m, AA, sigma, 0, pos_space, B=B), s[n], n)
    if mdl.nlin:
        C_lin = sp.csc_matrix(mdl.C_lin)
        C_lin.sort_indices()
        g = check_linear(int(mdl.msizes[0]), sp.csc_matrix(mdl.AA[0]), mdl.sigmaA[:, 0], pos_space, C_lin)
        if not pos_space:
            same(g["cl_row"], g["cl_rown"], "cl_row in the natural order")


# ---------------------------------------------------------------------------------------------- hand-made blocks
@pytest.mark.parametrize("name", mc.BLOCKS)
@pytest.mark.parametrize("pos_space", [True, False])
def test_hand_made_blocks(name, pos_space):
    m, AA, sigma, nvar = mc.block(name)
    g = check_block(m, AA, sigma, nvar, pos_space)
    if name == "zero":
        assert AA.nnz == 8 and g["nnz"].sum() == 7 and g["ent_v"].size == 7 and g["cq_v"].size == 7 and (g["cq_v"] != 0).all()
    if name == "empty":
        assert g["npos_nz"] == 2 < nvar
    if name == "wave45":
        assert list(g["nnz"]) == [5, 5, 4, 4, 1] and g["nd"] == 0 and g["q_wave"] == 2
    if name == "unsym":
        assert g["sp_ok"] == 0 and g["pc_t"].size == 0
    if name == "cross":
        # (2, 0) is stored for constraint 0 alone, (0, 2) for constraint 1 alone: each is the other's transposed position
        t20, t02 = list(g["cq_q"]).index(2), list(g["cq_q"]).index(6)
        assert g["sp_ok"] == 1 and g["pc_t"][t20] == t02 and g["pc_t"][t02] == t20
        assert list(g["cq_j"][g["cq_ptr"][t20]:g["cq_ptr"][t20 + 1]]) == [0] and list(g["cq_j"][g["cq_ptr"][t02]:g["cq_ptr"][t02 + 1]]) == [1]
    if name == "long66":
        cnt = np.diff(g["pc_ptr"])
        assert g["sp_ok"] == 1 and cnt[0] == 65 and cnt[1] == 64 and list(g["sp_long_cols"]) == [0]


@pytest.mark.parametrize("qA,want", [(-3, 0), (0, 0), (2, 2), (5, 5), (9, 5)])
def test_qA_is_clamped_and_bounds_the_dense_prefix(qA, want):
    m, AA, sigma, nvar = mc.block("wave45")
    g = check_block(m, AA, sigma, qA, dense_threshold=1.0)             # every constraint with an entry counts as dense
    assert g["qA"] == want and g["nd"] == want and g["q_wave"] == max(want, 2)


def test_dense_prefix_by_threshold_excludes_the_dense_positions_from_the_stored_columns():
    m, AA, sigma, nvar = mc.block("wave45")
    g = check_block(m, AA, sigma, nvar, dense_threshold=5.0)
    assert g["nd"] == 2 and g["q_wave"] == 2 and g["sp_ok"] == 0 and g["pc_ptr"].size == 0
    assert not np.isin(g["cq_j"], sigma[:2]).any() and g["cq_v"].size == g["nnz"][2:].sum()


@pytest.mark.parametrize("free_bytes,nd", [(0, 0), (5 * 5 * 8, 0), (int(5 * 5 * 8 / 0.55) + 1, 1), (3 * int(5 * 5 * 8 / 0.55) + 3, 3),
                                           (BIG, 5)])
def test_memory_cap_ends_the_dense_prefix(free_bytes, nd):
    """threshold 1 calls all five constraints dense: 0.55 free_bytes / (8 m^2) matrices fit -- none, one, three, all"""
    m, AA, sigma, nvar = mc.block("wave45")
    assert check_block(m, AA, sigma, nvar, dense_threshold=1.0, free_bytes=free_bytes)["nd"] == nd


def test_two_block_model_of_the_gpu_upload_test():
    AA, sigma, qA, ms = mc.two_block()
    g = check_block(ms[0], AA[0], sigma[:, 0], qA[0, 0], False, dense_threshold=5.0)
    assert g["nd"] == 3 and g["npos_nz"] == 5 and g["nnz"][5] == 0
    check_block(ms[1], AA[1], sigma[:, 1], qA[0, 1], False, dense_threshold=5.0)


@pytest.mark.parametrize("pos_space", [True, False])
def test_linear_layout_of_a_generated_block(pos_space):
    m, AA, sigma, nvar = mc.block("wave45")
    check_linear(m, AA, sigma, pos_space, mc.linear_case(nvar, 7, seed=3))


@pytest.mark.parametrize("khat", [1, 4])
@pytest.mark.parametrize("pos_space", [True, False])
def test_rank_k_layout(khat, pos_space):
    m, nvar = 6, 5
    ipos = np.array([2, 0, 4, 1, 3])
    V, d = mc.lowrank_case(nvar, m, khat, seed=khat, zero_weight=1)
    s = spec_lowrank(V, d, khat, ipos, pos_space)
    for n in s:
        same(factor_layout(n, m, ipos, 0, pos_space, khat, V, d), s[n], n)
    h = ipos[1] if pos_space else 1                                    # the all-zero-weight constraint, in H order
    assert not s["v_w"][h * khat:(h + 1) * khat].any() and np.count_nonzero(s["v_w"]) == (nvar - 1) * khat
    # stored positions [0, 2) = constraints 1 and 3: constraint 1 has no weighted column, constraint 3 has
    assert factor_layout("v_partial", m, ipos, 2, pos_space, khat, V, d)[0] == 1
    assert factor_layout("stored_and_factored", m, ipos, 2, pos_space, khat, V, d)[0] == 1
    assert factor_layout("stored_and_factored", m, ipos, 1, pos_space, khat, V, d)[0] == -1
    assert factor_layout("v_partial", m, ipos, 0, pos_space, khat, V, d)[0] == 0


@pytest.mark.parametrize("pos_space", [True, False])
def test_rank_k_layout_of_an_empty_V(pos_space):
    m, nvar, khat = 4, 3, 2
    V = (np.ones(m + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
    ipos = np.array([1, 2, 0])
    d = np.array([1.0, -1.0, 0.0, 0.0, 1.0, 1.0])
    same(factor_layout("v_ptr", m, ipos, 0, pos_space, khat, V, d), np.zeros(nvar * khat + 1), "v_ptr")
    assert factor_layout("v_col", m, ipos, 0, pos_space, khat, V, d).size == 0
    same(factor_layout("v_w", m, ipos, 0, pos_space, khat, V, d), d.reshape(3, 2)[np.argsort(ipos)].ravel() if pos_space else d, "v_w")


@pytest.mark.parametrize("pos_space", [True, False])
def test_diagonal_rows(pos_space):
    m, nvar, npos_nz = 4, 6, 2
    ipos = np.array([3, 0, 5, 1, 2, 4])                                # constraints 1 and 3 are stored
    rows = [4, 0, 2]
    same(factor_layout("dg_nat", m, ipos, npos_nz, pos_space, rows=rows), rows, "dg_nat")
    same(factor_layout("dg_h", m, ipos, npos_nz, pos_space, rows=rows), ipos[rows] if pos_space else rows, "dg_h")
    of_pos = -np.ones(nvar, dtype=int)
    of_pos[ipos[rows]] = np.arange(3)
    same(factor_layout("dg_of_pos", m, ipos, npos_nz, pos_space, rows=rows), of_pos, "dg_of_pos")
    assert factor_layout("dg_h", m, ipos, npos_nz, pos_space, rows=[4, 6], raw=True) == (-1, "lrn_upload_diag: row 6 out of range (0 .. 5)")
    assert factor_layout("dg_h", m, ipos, npos_nz, pos_space, rows=[-1], raw=True) == (-1, "lrn_upload_diag: row -1 out of range (0 .. 5)")
    assert factor_layout("dg_h", m, ipos, npos_nz, pos_space, rows=[4, 0, 4], raw=True) == (-1, "lrn_upload_diag: row 4 is listed twice")
    assert factor_layout("dg_h", m, ipos, npos_nz, pos_space, rows=[4, 3], raw=True) == (
        -3, "lrn_upload_diag: constraint 3 of block 0 is stored (it has entries): its diagonal belongs into the stored matrix")


# ---------------------------------------------------------------------------------------------- error cases
def test_upload_model_errors_keep_their_code_and_text():
    m, AA, sigma, nvar = mc.block("wave45")
    cp, rv, nz = _csc(AA)
    for bad in (0, nvar + 1):
        rv2 = rv.copy()
        rv2[3] = bad
        assert model_layout("nd", m, (cp, rv2, nz), sigma, nvar, raw=True) == (-1, "AA rowval out of range")
    for sg in ([1, 3, 0, 4, 4], [1, 3, 0, 4, 5], [1, 3, 0, 4, -1]):
        assert model_layout("nd", m, AA, np.array(sg), nvar, raw=True) == (-1, "sigmaA is not a permutation")
    assert model_layout("nd", m, AA, np.array([1, 0, 3, 4, 2]), nvar, raw=True) == (
        -1, "sigmaA is not sorted by decreasing nnz (model.jl:159)")
    lc, lr, lv = _csc(mc.linear_case(nvar, 4, seed=5))
    for bad in (0, nvar + 1):
        lr2 = lr.copy()
        lr2[-1] = bad
        assert model_layout("cl_ptr", m, AA, sigma, nvar, Clin=(lc, lr2, lv), raw=True) == (-1, "C_lin rowval out of range")
    assert model_layout("no_such_array", m, AA, sigma, nvar, raw=True) == (-1, "unknown layout array no_such_array")


def test_upload_lowrank_errors_keep_their_code_and_text():
    m, nvar, khat = 6, 5, 2
    ipos = np.arange(nvar)
    V, d = mc.lowrank_case(nvar, m, khat, seed=9)
    cp, rv, nz = _csc(V)
    for bad in (0, nvar * khat + 1):
        rv2 = rv.copy()
        rv2[2] = bad
        assert factor_layout("v_ptr", m, ipos, 0, True, khat, (cp, rv2, nz), d, raw=True) == (
            -1, f"lrn_upload_lowrank: rowval {bad} out of range")
    assert factor_layout("v_ptr", m, ipos, 0, True, khat, (cp - 1, rv, nz), d, raw=True) == (
        -1, "lrn_upload_lowrank: colptr must start at 1 and not decrease")
    cp2 = cp.copy()
    cp2[3] = cp2[2] - 1
    assert factor_layout("v_ptr", m, ipos, 0, True, khat, (cp2, rv, nz), d, raw=True) == (
        -1, "lrn_upload_lowrank: colptr decreases at column 2")
