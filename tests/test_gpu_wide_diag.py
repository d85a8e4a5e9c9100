"""GPU: diagonal parts on wide factored blocks, A_k = diag(a_k) + V_k D_k V_k' with up to 64 factor columns (library option
wide_diag beside lowrank_wide; csrc/diagops.hip::diag_sq_wide_mfma_kernel, the gates of csrc/model_factored.hip) through Device / the C ABI
and through Optimizer.load_factored_model(..., wide="diag"), on the cases of tests/wide_diag_cases.py.

Bounds are the project's own: H and the data operators -- 1e-12 relative Frobenius against np.longdouble from the materialised
constraints (tests/test_gpu_diag_factored.py, tests/test_gpu_wide.py; tests/test_wide_diag_cpu.py shows a float64 evaluation in the
device's order at 3e-16 on these inputs and every single fault above 1e-9); the operator H x -- 20 x the float64 oracle's distance
from the longdouble product, the H_alpha apply -- min(20 x the oracle's distance from the longdouble solve, 1e-9), lrn_pcg -- exit
code and iteration count of the longdouble reference run (tests/test_gpu_cg_diag.py, tests/test_gpu_wide.py); solves -- rel 1e-8
between two solves of one problem, 1e-6 (1 + |optimum|) against the planted optimum.  Every comparison prints its figure before it
asserts."""
import contextlib
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import diag_factored_cases as dfc
import ragged_cases as rc
import wide_cases as wc
import wide_diag_cases as wd
from loraine_jl_amd.model import ragged_plan
from oracle import cg_reference as cr
from oracle import loraine_oracle as lo

pytestmark = pytest.mark.gpu

TOL = 1e-12
FACTOR = 20.0
LD = np.longdouble
DEFAULTS = dict(lowrank_wide=0, wide_diag=0, lowrank_ragged=0, ragged_ops=0, ragged_cross=0, ragged_ts=0, cg_factored=0, cg_diag=0,
                matvec_h=0, prec_eig=0, prec_inv=-1, prec_dense=0, diag_sq_mfma=-1)
ROUTES = ("diag_sq_mfma", "diag_sq_rows", "schur_diag", "schur_wide", "diag_stored_cross")
MFMA_MIN = 16          # csrc/diagops.hip: DG_MFMA_MIN


@pytest.fixture(scope="module")
def dev():
    import loraine_jl_amd
    d = loraine_jl_amd.Device(0)
    yield d
    d.close()


@contextlib.contextmanager
def options(dev, **kw):
    try:
        for k, v in kw.items():
            dev.set_option(k, v)
        yield
    finally:
        for k in kw:
            dev.set_option(k, DEFAULTS[k])


def _counts(dev, keys=ROUTES):
    return {k: dev.count(k) for k in keys}


def _delta(c0, c1):
    return {k: c1[k] - c0[k] for k in c0}


def _upload(dev, fm, dense=False, wide=1, wide_diag=1):
    """What the solver does with a factored model: entries of the stored rows, factors, the declaration, the diagonal parts; dense:
    a full stored matrix goes to a dense slot."""
    if dense:
        dev.set_option("dense_threshold", float(int(fm.msizes[0]) ** 2))
    try:
        dev.upload_model(fm.AA, fm.sigmaA, fm.qA, fm.msizes, C_lin=fm.C_lin if fm.nlin else None)
    finally:
        dev.set_option("dense_threshold", -1.0)
    with options(dev, lowrank_wide=wide, wide_diag=wide_diag):
        for i, (V, d, khat) in enumerate(fm.lowrank):
            dev.upload_lowrank(i, khat, V, d)
            dev.set_factored(i)
            if fm.diag[i]:
                rows = sorted(fm.diag[i])
                dev.upload_diag(i, rows, np.column_stack([fm.diag[i][k] for k in rows]))


def _scale(dev, name, with_G=True):
    for i, (W, G) in enumerate(wd.scaling(name)):
        dev.set_scaling(i, W, G if with_G else None)


def _load(dev, name, with_G=True):
    fm = wd.model(name)
    _upload(dev, fm, dense=name == "DH")
    assert dev.count("diag_rows") == sum(len(d) for d in fm.diag)
    _scale(dev, name, with_G)
    if fm.nlin:
        dev.set_lin(np.ones(fm.nlin), np.ones(fm.nlin))
    return fm


def _sq_calls(fm, cross):
    """Launches of diag_sq per assembly and block: one for P of H_DD (kh 1) and, for C, one on the padded layout or one per
    non-empty class where ragged_cross takes the block (0 < Rc < nvar khat) -> [(diagonal rows, launches)] per block."""
    out = []
    for i, (_, _, khat) in enumerate(fm.lowrank):
        p = ragged_plan(rc.block_ranks(fm, i), max_rank=64)
        by_class = cross and 0 < p["Rc"] < fm.n * khat
        out.append((len(fm.diag[i]), 1 + (p["ncls"] if by_class else 1)))
    return out


# ---------------------------------------------------------------------------------------------- data operators
def _sym(m, seed):
    R = np.random.default_rng(seed).standard_normal((m, m))
    return 0.5 * (R + R.T)


@functools.lru_cache(maxsize=None)
def _op_inputs(name):
    m, n = wd.SIZES[name]
    return _sym(m, 40 + m), np.random.default_rng(n + 1).standard_normal(n)


@functools.lru_cache(maxsize=None)
def _op_reference(name):
    """AA vec(X) = -<A_k, X> and Rd = sum_k y_k A_k (C = S = 0) in np.longdouble from the materialised constraints."""
    X, y = _op_inputs(name)
    As = [a.astype(LD) for a in wd.matrices(name)[0]]
    return -np.array([np.sum(a * X.astype(LD)) for a in As]), sum(LD(yk) * a for yk, a in zip(y, As))


def _operators(dev, name):
    X, y = _op_inputs(name)
    dev.ip_set_c(0, np.zeros_like(X))
    dev.ip_set_iterate(0, X, np.zeros_like(X))
    keys = ("op_ragged", "ragged_ops_fallback", "op_diag")
    c0 = _counts(dev, keys)
    aax = dev.ip_aa_x()
    dev.ip_residual_d(y)
    return aax, dev.dbg_get_block(0, "Rd")[0], _delta(c0, _counts(dev, keys))


@pytest.mark.parametrize("name", ["D64", "DH"])
def test_data_operators_padded_and_compacted(dev, name):
    _load(dev, name)
    aref, Rref = _op_reference(name)
    a0, R0, d0 = _operators(dev, name)
    with options(dev, ragged_ops=1):
        a1, R1, d1 = _operators(dev, name)
        a2, R2, _ = _operators(dev, name)
    e0 = (rc.relerr(a0, aref), rc.relerr(R0, Rref))
    e1 = (rc.relerr(a1, aref), rc.relerr(R1, Rref))
    print("WDIAG ops %s | AA vec(X): padded %.2e compacted %.2e | Rd: padded %.2e compacted %.2e | %s %s"
          % (name, e0[0], e1[0], e0[1], e1[1], d0, d1))
    assert max(e0) < TOL
    assert max(e1) < TOL
    assert d0["op_ragged"] == 0 and d1["op_ragged"] == 2 and d1["ragged_ops_fallback"] == 0
    assert d0["op_diag"] == d1["op_diag"] == 2           # the diagonal term of each operator, after the factor form
    assert np.array_equal(R1, R1.T) and np.array_equal(R1, R2) and np.array_equal(a1, a2)


# ---------------------------------------------------------------------------------------------- mode 1
@pytest.mark.parametrize("with_G", [True, False], ids=["G", "W-only"])
@pytest.mark.parametrize("name", wd.NAMES)
def test_mode_1_of_a_wide_block_with_diagonal_parts(dev, name, with_G):
    fm = _load(dev, name, with_G)
    ref = wd.reference(name)
    nwide = sum(lr[2] > 16 for lr in fm.lowrank)
    nstored = sum(1 for i in range(fm.nlmi) if fm.stored[i] and fm.diag[i])
    worst = 0.0
    for cross in (0, 1):
        calls = _sq_calls(fm, cross)
        for mfma in (0, 1, -1):
            with options(dev, wide_diag=1, diag_sq_mfma=mfma, ragged_cross=cross):
                c0 = _counts(dev)
                H1 = dev.schur_assemble(1, want_H=True)
                d = _delta(c0, _counts(dev))
                H2 = dev.schur_assemble(1, want_H=True)
            e = rc.relerr(H1, ref)
            worst = max(worst, e)
            print("WDIAG mode 1 %s %s ragged_cross=%d diag_sq_mfma=%d | %.2e | %s"
                  % (name, "G" if with_G else "W-only", cross, mfma, e, d))
            assert e < TOL
            want_mfma = sum(k for ns, k in calls if mfma == 1 or (mfma < 0 and ns >= MFMA_MIN))
            assert d == dict(diag_sq_mfma=want_mfma, diag_sq_rows=sum(k for _, k in calls) - want_mfma, schur_diag=fm.nlmi,
                             schur_wide=nwide, diag_stored_cross=nstored)
            assert np.array_equal(H1, H2)                    # one writer per element, fixed order: the same bits
            assert np.array_equal(H1, H1.T)
    print("WDIAG mode 1 %s %s | worst %.2e" % (name, "G" if with_G else "W-only", worst))


def _alone(dev, name, with_G, mfma, cross, wide_diag=1):
    """H of one block of D2B as a model of its own.  wide_diag = 0 (the narrow block only): uploaded and assembled with the option
    off, the route before the option existed."""
    _upload(dev, wd.block_model(name), wide_diag=wide_diag)
    W, G = wd.scaling("D2B")[0 if name == "D32" else 1]
    dev.set_scaling(0, W, G if with_G else None)
    with options(dev, diag_sq_mfma=mfma, ragged_cross=cross, wide_diag=wide_diag):
        return dev.schur_assemble(1, want_H=True)


@pytest.mark.parametrize("cross", [0, 1], ids=["cross-padded", "cross-compacted"])
@pytest.mark.parametrize("mfma", [0, 1])
def test_the_narrow_block_beside_a_wide_one_keeps_its_bits(dev, mfma, cross):
    """D2B = D32's block + a block of khat 2 with diagonal rows.  The narrow block assembled by itself has the bits of its assembly
    with wide_diag = 0, the route before the option.  (Inside D2B its terms -- H_FF, H_DD, C -- are added one after the other to
    what block 0 left, so H of D2B is the sum of the two within rounding, not bit for bit.)"""
    Hw = _alone(dev, "D32", True, mfma, cross)
    Hn = _alone(dev, "D2Bn", True, mfma, cross)
    Hn0 = _alone(dev, "D2Bn", True, mfma, cross, wide_diag=0)
    assert np.array_equal(Hn, Hn0)
    _load(dev, "D2B")
    with options(dev, diag_sq_mfma=mfma, ragged_cross=cross, wide_diag=1):
        H = dev.schur_assemble(1, want_H=True)
    e = rc.relerr(H, Hw + Hn)
    print("WDIAG D2B diag_sq_mfma=%d ragged_cross=%d | against the sum of its blocks' own assemblies %.2e" % (mfma, cross, e))
    assert e < TOL


@pytest.mark.parametrize("m,n,khat,count", [(33, 37, 2, 3), (65, 70, 4, 64)])
def test_a_narrow_case_gives_equal_bits_with_the_option_on_and_off(dev, m, n, khat, count):
    """Two blocks of tests/diag_factored_cases.py (stored rows included) under wide_diag 0 and 1, both forms, both layouts."""
    from loraine_jl_amd.model import build_factored_model
    items = dfc.block_items(m, n, khat, count, 100 * m + n)
    fm = build_factored_model([-np.eye(m)], [items], np.zeros(n), factored_form=1)
    W, G = dfc.spd(m, 5)
    out = {}
    for wdg in (0, 1):
        _upload(dev, fm, dense=True, wide=0, wide_diag=wdg)
        dev.set_scaling(0, W, G)
        with options(dev, wide_diag=wdg):
            for mfma in (0, 1):
                for cross in (0, 1):
                    with options(dev, diag_sq_mfma=mfma, ragged_cross=cross):
                        c0 = _counts(dev)
                        out[wdg, mfma, cross] = dev.schur_assemble(1, want_H=True)
                        d = _delta(c0, _counts(dev))
                    assert d["schur_diag"] == 1 and d["schur_wide"] == 0 and (d["diag_sq_rows"] == 0) == bool(mfma)
    for key, H in out.items():
        if key[0] == 1:
            assert np.array_equal(H, out[(0,) + key[1:]]), key


# ---------------------------------------------------------------------------------------------- the other form of the same model
@pytest.mark.parametrize("name", ["D64", "DH"])
def test_against_the_diagonal_parts_as_stored_matrices(dev, name):
    """The same constraints with every (V, d, a) item as a stored sparse matrix beside wide=True (wide_diag = 0): the only form
    the model had before the option."""
    sm = wd.stored_model(name)
    assert not sm.wide_diag and not any(sm.diag)
    assert sm.wide == (name == "D64")                        # (DH: the ranks 48 and 20 are the stored ones, khat 16 is left)
    _upload(dev, sm, dense=True, wide_diag=0)
    _scale(dev, name)
    if sm.nlin:
        dev.set_lin(np.ones(sm.nlin), np.ones(sm.nlin))
    c0 = _counts(dev)
    Hs = dev.schur_assemble(1, want_H=True)
    ds = _delta(c0, _counts(dev))
    _load(dev, name)
    with options(dev, wide_diag=1):
        Hd = dev.schur_assemble(1, want_H=True)
    ref = wd.reference(name)
    e = rc.relerr(Hd, Hs)
    print("WDIAG forms %s | diagonal parts against stored matrices %.2e | against longdouble: %.2e and %.2e"
          % (name, e, rc.relerr(Hd, ref), rc.relerr(Hs, ref)))
    assert ds["schur_diag"] == 0 and ds["schur_wide"] == int(sm.wide)
    assert e < TOL


# ---------------------------------------------------------------------------------------------- the CG path
def _load_cg(dev, name):
    case, fm = wd.cg_case(name), wd.cg_model(name)
    _upload(dev, fm, dense=name == "DH")
    _rescale(dev, case)
    return case


def _rescale(dev, case):
    """(Again: a new NT scaling, so that the operator choice and H are taken anew.)"""
    dev.set_scaling(0, case.W[0], case.G[0])
    if case.model.nlin:
        dev.set_lin(case.X_lin, case.S_lin_inv)


@functools.lru_cache(maxsize=None)
def _oracle_operator(name):
    case, H = wd.cg_data(name)
    ref = H @ case.x.astype(LD)
    y = np.zeros(case.model.n)
    lo.MyA(case.W, case.model.AA, case.model.nlin, case.model.C_lin, case.X_lin, case.S_lin_inv)(y, case.x)
    return ref, cr.relerr(y, ref)


@pytest.mark.parametrize("name", wd.CG_NAMES)
def test_operator_by_every_route(dev, name):
    """lrn_matvec matrix-free (the composition with the diagonal terms after the factor form, padded and on the compacted columns)
    and through H assembled in mode 1 (assemble_diag at kh 64, padded and per class)."""
    case = _load_cg(dev, name)
    ref, err_o = _oracle_operator(name)
    keys = ("op_diag", "hop_assemble_lowrank", "hop_matvec", "schur_diag", "schur_wide", "op_ragged")
    with options(dev, cg_factored=1, cg_diag=1, wide_diag=1):
        for mh in (1, 2):
            for rest in (0, 1):
                with options(dev, matvec_h=mh, ragged_ops=rest, ragged_cross=rest):
                    _rescale(dev, case)
                    c0 = _counts(dev, keys)
                    y1 = dev.matvec(case.x)
                    y2 = dev.matvec(case.x)
                    d = _delta(c0, _counts(dev, keys))
                err = cr.relerr(y1, ref)
                print("WDIAG operator %s mh=%d compacted=%d | oracle %.2e bound %.2e | device %.2e | %s"
                      % (name, mh, rest, err_o, FACTOR * err_o, err, d))
                assert err <= FACTOR * err_o, (err, err_o)
                assert np.array_equal(y1, y2)
                if mh == 1:
                    assert d["op_diag"] == 4 and d["hop_matvec"] == 0 and d["schur_diag"] == 0
                    assert (d["op_ragged"] > 0) == bool(rest)
                else:
                    assert d["hop_assemble_lowrank"] == 1 and d["hop_matvec"] == 2 and d["op_diag"] == 0
                    assert d["schur_diag"] == 1 and d["schur_wide"] == 1


@functools.lru_cache(maxsize=None)
def _apply_reference(name, erank):
    case = wd.cg_case(name)
    ref = cr.reference_solver(case, 1, erank)(case.x)
    _, Mo = cr.oracle_state(case, 1, erank)
    z = np.zeros(case.model.n)
    Mo(z, case.x)
    return ref, cr.relerr(z, ref)


@pytest.mark.parametrize("erank", [1, 2])
@pytest.mark.parametrize("name", wd.CG_NAMES)
def test_halpha_apply_in_its_three_forms(dev, name, erank):
    case = _load_cg(dev, name)
    ref, err_o = _apply_reference(name, erank)
    bound = min(FACTOR * err_o, 1e-9)
    ndiag = len(wd.cg_model(name).diag[0])
    out = []
    with options(dev, cg_factored=1, cg_diag=1, wide_diag=1, prec_eig=1):
        for inv, dense in [(0, 1), (1, 1), (1, 2)]:
            with options(dev, prec_inv=inv, prec_dense=dense):
                assert dev.prec_setup(1, erank, 1) == 0      # ts on the padded columns, khat 64
                assert dev.count("prec_ts_diag_rows") == ndiag and dev.count("prec_ts_factored") == 1
                zp = dev.prec_apply(case.x)
                with options(dev, ragged_ts=1):
                    assert dev.prec_setup(1, erank, 1) == 0
                    assert dev.count("prec_ts_diag_rows") == ndiag and dev.count("prec_ts_ragged") == 1
                    z = dev.prec_apply(case.x)
                    assert dev.prec_setup(1, erank, 1) == 0
                    assert np.array_equal(z, dev.prec_apply(case.x))
                out.append((cr.relerr(zp, ref), cr.relerr(z, ref)))
    print("WDIAG apply %s erank=%d | oracle %.2e bound %.2e | (padded, compacted) potrs %.2e %.2e inverse %.2e %.2e dense %.2e %.2e"
          % (name, erank, err_o, bound, out[0][0], out[0][1], out[1][0], out[1][1], out[2][0], out[2][1]))
    for ep, e in out:
        assert ep <= bound and e <= bound, (out, bound)


@pytest.mark.parametrize("rest", [0, 1], ids=["padded", "compacted"])
@pytest.mark.parametrize("mh", [1, 2], ids=["matrixfree", "assembledH"])
@pytest.mark.parametrize("name", wd.CG_NAMES)
def test_pcg_against_the_reference_run(dev, name, mh, rest):
    """(30, K) exactly at the tolerance in the gap, (-2, K - 1) at maxit = K - 1: the exits of the longdouble reference run."""
    case = _load_cg(dev, name)
    run = wd.cg_run(name)
    K, tol = run.K, run.tol
    keys = ("schur_wide", "schur_diag", "op_diag", "op_ragged")
    with options(dev, cg_factored=1, cg_diag=1, wide_diag=1, prec_eig=1, matvec_h=mh, lowrank_ragged=rest, ragged_ops=rest,
                 ragged_cross=rest, ragged_ts=rest):
        assert dev.prec_setup(1, 1, 1) == 0
        c0 = _counts(dev, keys)
        got = [dev.pcg(case.h, tol, 10000), dev.pcg(case.h, tol, K - 1)]
        d = _delta(c0, _counts(dev, keys))
    print("WDIAG pcg %s mh=%d compacted=%d K=%d tol=%.3e | exits (%d, %d) (%d, %d) | %s"
          % (name, mh, rest, K, tol, got[0][1], got[0][2], got[1][1], got[1][2], d))
    assert (got[0][1], got[0][2]) == (30, K)
    assert (got[1][1], got[1][2]) == (-2, K - 1)
    if mh == 2:
        assert d["schur_wide"] == 1 and d["schur_diag"] == 1 and d["op_diag"] == 0
    else:
        assert d["schur_wide"] == 0 and d["op_diag"] > 0 and (d["op_ragged"] > 0) == bool(rest)


# ---------------------------------------------------------------------------------------------- refusals
def _refused(dev, call, text, code="(-1)"):
    """The call fails with the code and a text; no route counter moves."""
    import loraine_jl_amd
    c0 = _counts(dev)
    with pytest.raises(loraine_jl_amd.LoraineHipError) as ei:
        call()
    msg = str(ei.value)
    print("WDIAG refusal |", msg)
    assert code in msg and text in msg
    return _delta(c0, _counts(dev))


def test_with_the_option_off_the_refusals_keep_their_texts(dev):
    none = dict.fromkeys(ROUTES, 0)
    m, n = wd.SIZES["D32"]
    fm = wd.model("D32")
    # lrn_upload_diag on a wide block
    dev.upload_model(fm.AA, fm.sigmaA, fm.qA, fm.msizes)
    V, d, khat = fm.lowrank[0]
    with options(dev, lowrank_wide=1):
        dev.upload_lowrank(0, khat, V, d)
        dev.set_factored(0)
    assert _refused(dev, lambda: dev.upload_diag(0, [1], np.ones((m, 1))),
                    "lrn_upload_diag: block 0 is wide (khat = 32 > 16): a wide block carries no diagonal part -- store such a "
                    "constraint as a matrix") == none
    assert dev.count("diag_rows") == 0
    # a wide lrn_upload_lowrank on a block that holds diagonal rows
    nm = wd.block_model("D2Bn")
    mn, nn = wd.SIZES["D2Bn"]
    _upload(dev, nm, wide=0, wide_diag=0)
    with options(dev, lowrank_wide=1):
        assert _refused(dev, lambda: dev.upload_lowrank(0, 32, sp.csr_matrix((nn * 32, mn)), np.zeros(nn * 32)),
                        "lrn_upload_lowrank: khat = 32 on block 0, which holds diagonal parts (lrn_upload_diag): a wide block "
                        "carries none -- store such a constraint as a matrix") == none
    assert dev.count("diag_rows") == len(wd.D2B_NARROW_DIAG)
    # the MFMA form of the squared-operand product at khat 32: a block uploaded under the option, assembled without it
    _load(dev, "D32")
    with options(dev, diag_sq_mfma=1):
        d = _refused(dev, lambda: dev.schur_assemble(1), "diag_sq: the MFMA form needs khat in 1, 2, 4, 8, 16, not 32")
    assert d["schur_diag"] == 0 and d["diag_sq_rows"] == 0
    with options(dev, diag_sq_mfma=1, wide_diag=1):          # ... and with it the context is usable as before
        assert rc.relerr(dev.schur_assemble(1, want_H=True), wd.reference("D32")) < TOL
    # the option itself is known, and resets to 0
    dev.set_option("wide_diag", 1)
    dev.set_option("wide_diag", 0)


def test_with_the_option_on_the_other_refusals_stay(dev):
    from loraine_jl_amd._capi import LoraineHipError, ptr
    fm = _load(dev, "DH")
    n, m = fm.n, int(fm.msizes[0])
    H = dev.schur_assemble(1, want_H=True)
    with options(dev, wide_diag=1, lowrank_wide=1):
        # a stored constraint carries its diagonal in its entries
        with pytest.raises(LoraineHipError, match=r"lrn_upload_diag: constraint 0 of block 0 is stored"):
            dev.upload_diag(0, [wc.V3_TRACE], np.ones((m, 1)))
        assert dev.count("diag_rows") == len(fm.diag[0])
        # one GPU
        dev.set_shard(0, 2)
        try:
            with pytest.raises(LoraineHipError, match="one GPU"):
                dev.schur_assemble(1)
        finally:
            dev.set_shard(0, 1)
        # the CG calls need cg_diag beside cg_factored; lrn_matvec_partial stays refused with both
        x, out = np.ones(n), np.zeros(n)
        for cgf in (0, 1):
            with options(dev, cg_factored=cgf):
                for call in (lambda: dev.matvec(x), lambda: dev.prec_setup(1, 1, 1), lambda: dev.prec_apply(x),
                             lambda: dev.pcg(x, 1e-6)):
                    with pytest.raises(LoraineHipError, match="diagonal parts.*the CG path does not hold them"):
                        call()
        with options(dev, cg_factored=1, cg_diag=1):
            dev.matvec(x)
            assert dev.lib.lrn_matvec_partial(dev.h, ptr(x), ptr(out)) != 0
            msg = dev.lib.lrn_last_error(dev.h).decode()
            assert "lrn_matvec_partial" in msg and "diagonal parts" in msg
        assert np.array_equal(dev.schur_assemble(1, want_H=True), H)      # every refusal left the block as it was


def test_a_wide_re_upload_keeps_the_diagonal_rows(dev):
    """wide_diag = 1: new wide factors on a block that holds diagonal rows -- the rows stay, as under a narrow re-upload."""
    fm = _load(dev, "D32")
    H = dev.schur_assemble(1, want_H=True)
    V, d, khat = fm.lowrank[0]
    with options(dev, lowrank_wide=1, wide_diag=1):
        dev.upload_lowrank(0, khat, V, d)
    assert dev.count("diag_rows") == len(fm.diag[0])
    _scale(dev, "D32")
    assert np.array_equal(dev.schur_assemble(1, want_H=True), H)


# ---------------------------------------------------------------------------------------------- solves
OPTION_KEYS = ("lowrank_wide", "wide_diag", "ragged_cross", "ragged_ts", "ragged_ops", "lowrank_ragged", "cg_diag", "cg_factored")


def _solve(P, factors, **kw):
    from loraine_jl_amd.optimizer import Optimizer
    o = Optimizer()
    o.set_silent(True)
    attrs = kw.pop("attrs")
    for k, v in attrs.items():
        o.set_attribute(k, v)
    o.load_factored_model(P.F0(), factors, P.b, max_sense=True, factored_form=1, **kw)
    try:
        o.optimize()
        s = o.solver
        return dict(status=s.status, iters=s.iter, cg=getattr(s, "cg_iter_tot", 0), obj=o.objective_value(),
                    wide=s.dev.count("schur_wide"), diag=s.dev.count("schur_diag"), rows=s.dev.count("diag_rows"),
                    tsd=s.dev.count("prec_ts_diag_rows"), ts=s.dev.count("prec_ts_ragged"), model_wide_diag=s.model.wide_diag,
                    stored=len(s.model.stored[0]))
    finally:
        if o.solver is not None:                             # (the device may serve another solve: the defaults again)
            for k in OPTION_KEYS:
                o.solver.dev.set_option(k, 0)


def test_planted_solve_kit_0():
    P = wd.PlantedWideDiag()
    bound = 1e-6 * (1 + abs(P.optimum))
    a = _solve(P, P.factors(), attrs=dict(kit=0), wide="diag", ragged=False)
    b = _solve(P, P.factors(), attrs=dict(kit=0), wide="diag", ragged="all")
    s = _solve(P, P.stored_trace_factors(), attrs=dict(kit=0), wide=True)      # the trace row as a stored sparse identity
    print("WDIAG solve kit 0 | wide=\"diag\": status %d, %d iterations, objective %.12e | + ragged=\"all\": status %d, %d iterations, "
          "objective %.12e | trace row stored, wide=True: status %d, %d iterations, objective %.12e | planted %.12e"
          % (a["status"], a["iters"], a["obj"], b["status"], b["iters"], b["obj"], s["status"], s["iters"], s["obj"], P.optimum))
    assert a["model_wide_diag"] and b["model_wide_diag"] and not s["model_wide_diag"]
    assert a["rows"] == b["rows"] == 1 and a["stored"] == 0 and s["rows"] == 0 and s["stored"] == 1
    assert a["wide"] > 0 and a["diag"] == a["wide"] and b["diag"] == b["wide"] > 0 and s["diag"] == 0 and s["wide"] > 0
    assert a["status"] == b["status"] == s["status"] == 1
    assert a["iters"] == b["iters"] == s["iters"]
    assert a["obj"] == pytest.approx(s["obj"], rel=1e-8) and b["obj"] == pytest.approx(s["obj"], rel=1e-8)
    for r in (a, b, s):
        assert abs(r["obj"] - P.optimum) <= bound


@pytest.mark.parametrize("ragged", [False, "all"])
def test_planted_solve_kit_1(ragged):
    P = wd.PlantedWideDiag()
    r = _solve(P, P.factors(), attrs=dict(kit=1, preconditioner=1, erank=1), wide="diag", ragged=ragged, cg="diag")
    print("WDIAG solve kit 1 ragged=%r | status %d, %d iterations, %d CG iterations, objective %.10f planted %.10f | assemblies of "
          "the wide block %d (with diagonal parts %d), diagonal rows in ts %d, ts blocks from the compacted columns %d"
          % (ragged, r["status"], r["iters"], r["cg"], r["obj"], P.optimum, r["wide"], r["diag"], r["tsd"], r["ts"]))
    assert r["model_wide_diag"] and r["rows"] == 1
    assert r["status"] == 1
    assert abs(r["obj"] - P.optimum) <= 1e-6 * (1 + abs(P.optimum))
    assert r["cg"] > 0 and r["tsd"] == 1
    assert r["ts"] == (1 if ragged == "all" else 0)
