"""CPU: the data operators of a mixed-rank factored block on the compacted columns (library option ragged_ops) without a GPU --
the Python restatement of the column plan (loraine_jl_amd.model.ragged_columns / ragged_chunks; csrc/ragged_plan.h holds the
same functions) against hand-written expectations, a NumPy float64 restatement of both operators on the compacted layout
(column dots summed by group through gh; the syrk by K-chunks added in order, then mirrored) against AA vec(Z) and mat(AA' x)
from the materialised constraints, and the host opt-in.  The restatement checks the algebra and the index maps, not the kernels.

The bound is the suite's own for a product against another formulation: 1e-12 relative (2-norm for the vector, Frobenius for
the matrix)."""
import dataclasses

import numpy as np
import pytest

import ragged_cases as rc
from loraine_jl_amd.model import RAGGED_CLASSES, ragged_chunks, ragged_columns, ragged_plan

TOL = 1e-12


# ---------------------------------------------------------------------------------------------- planner
def _r4_wc():
    out = []
    for g in range(37):
        r = 5 + g % 4
        out += list(range(r)) + [-1] * (8 - r)
    return out + [0, 1] * 33


EXPECT = {
    # name: (Rc, gh, start, size, cg, wc)
    "R1": (23, [0, 3, 4, 1], [0, 16, 20, 22], [16, 4, 2, 1], [0] * 16 + [1] * 4 + [2] * 2 + [3],
           list(range(16)) + [0, 1, 2, -1] + [0, 1] + [0]),
    "R3": (145, [64] + list(range(64)) + list(range(65, 130)), [0] + [16 + k for k in range(129)], [16] + [1] * 129,
           [0] * 16 + list(range(1, 130)), list(range(9)) + [-1] * 7 + [0] * 129),
    "R4": (362, list(range(33, 70)) + list(range(33)), [8 * g for g in range(37)] + [296 + 2 * g for g in range(33)],
           [8] * 37 + [2] * 33, [g for g in range(37) for _ in range(8)] + [37 + g for g in range(33) for _ in range(2)],
           _r4_wc()),
    "equal": (10, [0, 1, 2, 3, 4], [0, 2, 4, 6, 8], [2] * 5, [0, 0, 1, 1, 2, 2, 3, 3, 4, 4], [0, 1] * 5),
    "zero": (0, [], [], [], [], []),
    "single": (16, [0], [0], [16], [0] * 16, list(range(9)) + [-1] * 7),
}
LISTS = {"equal": [2] * 5, "zero": [0] * 4, "single": [9]}


@pytest.mark.parametrize("name", list(EXPECT))
def test_columns_against_hand_written_expectations(name):
    ranks = LISTS[name] if name in LISTS else rc.ranks_of(name)
    p = ragged_columns(ranks)
    Rc, gh, start, size, cg, wc = EXPECT[name]
    assert (p["Rc"], p["gh"], p["start"], p["size"], p["cg"], p["wc"]) == (Rc, gh, start, size, cg, wc)
    assert p["ks"] == 1 and p["chunks"] == [(0, Rc)]
    q = ragged_plan(ranks)                         # (the plan of the assembly is untouched and agrees)
    assert sorted(q) == ["Rc", "classes", "gh", "ncls", "seg", "tiles"]
    assert q["Rc"] == Rc and q["gh"] == gh
    for g, (s, c) in enumerate(zip(start, size)):  # every group lies in the segment of its class
        assert q["seg"][c][0] <= s and s + c <= q["seg"][c][1]
        assert q["classes"][gh[g]] == c


CHUNKS = {
    (23, 1): (1, [(0, 23)]),
    (145, 2): (2, [(0, 80), (80, 145)]),
    (145, 3): (3, [(0, 48), (48, 96), (96, 145)]),
    (145, 5): (5, [(0, 32), (32, 64), (64, 96), (96, 128), (128, 145)]),
    (145, 16): (10, [(16 * s, min(16 * s + 16, 145)) for s in range(10)]),
    (362, 8): (8, [(0, 32), (32, 80), (80, 128), (128, 176), (176, 224), (224, 272), (272, 320), (320, 362)]),
}


@pytest.mark.parametrize("Rc,ks", list(CHUNKS))
def test_chunks_cover_every_step_exactly_once(Rc, ks):
    got_ks, chunks = ragged_chunks(Rc, ks)
    assert (got_ks, chunks) == CHUNKS[(Rc, ks)]
    steps = []
    for c0, c1 in chunks:
        assert c0 % 16 == 0 and c0 < c1 <= Rc
        steps += list(range(c0 // 16, -(-c1 // 16)))
    assert steps == list(range(-(-Rc // 16)))
    name = {23: "R1", 145: "R3", 362: "R4"}[Rc]
    p = ragged_columns(rc.ranks_of(name), ks)
    assert p["Rc"] == Rc and (p["ks"], p["chunks"]) == CHUNKS[(Rc, ks)]


def test_chunks_of_degenerate_ranges():
    assert ragged_chunks(0, 4) == (1, [(0, 0)])
    assert ragged_chunks(5, 0) == (1, [(0, 5)])
    assert ragged_chunks(4015, 99)[0] == 16


# ---------------------------------------------------------------------------------------------- algebra
def compact(V, d, khat, n, ks=1):
    """(plan, Vc, wc) of one block from its padded upload (V: n khat x msz, d: n khat), by the index maps of ragged_columns."""
    Vp = np.asarray(V.todense()).reshape(n, khat, -1)
    d = np.asarray(d, float).reshape(n, khat)
    p = ragged_columns(np.count_nonzero(d, axis=1).tolist(), ks)
    Vc, wc = np.zeros((Vp.shape[2], p["Rc"])), np.zeros(p["Rc"])
    for col in range(p["Rc"]):
        g = p["cg"][col]
        assert p["start"][g] <= col < p["start"][g] + p["size"][g]
        if p["wc"][col] < 0:
            continue
        h = p["gh"][g]
        q = np.flatnonzero(d[h])[p["wc"][col]]                 # the wc-th weighted column of the constraint, original order
        Vc[:, col], wc[col] = Vp[h, q], d[h, q]
    return p, Vc, wc


def aa_times_numpy(p, Vc, wc, Z, out):
    """out[gh[g]] -= sum over the columns of group g of wc <(Z Vc)(:, c), Vc(:, c)>, columns in order, zero weights skipped."""
    Q = Z @ Vc
    for g, (s, c) in enumerate(zip(p["start"], p["size"])):
        acc = 0.0
        for col in range(s, s + c):
            if wc[col] != 0.0:
                acc += wc[col] * float(Q[:, col] @ Vc[:, col])
        out[p["gh"][g]] -= acc


def aat_to_mat_numpy(p, F, wc, x):
    """M = -sum_c s_c f_c f_c', s_c = wc[c] x[gh[cg[c]]]: the lower triangle by K-chunks added in the order 0 .. ks - 1, then
    mirrored."""
    s = -(wc * np.asarray(x)[np.asarray(p["gh"], int)[np.asarray(p["cg"], int)]]) if p["Rc"] else np.zeros(0)
    m = F.shape[0]
    M = np.zeros((m, m))
    for c0, c1 in p["chunks"]:
        M += np.tril((F[:, c0:c1] * s[c0:c1]) @ F[:, c0:c1].T)
    return np.tril(M) + np.tril(M, -1).T


def factor_constraints(name):
    """Per block the materialised constraints with the rows the factor part does not serve zeroed (R6: the stored rows 0, 7 and
    the diagonal row 3)."""
    out = []
    for items, m in zip(rc.blocks(name), rc.msizes(name)):
        As = [rc.materialise(it, m) for it in items]
        if name == "R6":
            for k in (0, 3, 7):
                As[k] = np.zeros((m, m))
        out.append(As)
    return out


def sym(m, seed):
    R = np.random.default_rng(seed).standard_normal((m, m))
    return 0.5 * (R + R.T)


@pytest.mark.parametrize("ks", [1, 3, 16])
@pytest.mark.parametrize("name", rc.NAMES)
def test_algebra_of_both_operators_matches_the_materialised_constraints(name, ks):
    fm = rc.model(name)
    n = rc.nvar(name)
    x = np.random.default_rng(n).standard_normal(n)
    got = np.zeros(n)
    ref = np.zeros(n)
    for i, ((V, d, khat), As) in enumerate(zip(fm.lowrank, factor_constraints(name))):
        m = rc.msizes(name)[i]
        p, Vc, wc = compact(V, d, khat, n, ks)
        Z = sym(m, 50 + m + i)
        aa_times_numpy(p, Vc, wc, Z, got)
        ref -= np.array([np.sum(a * Z) for a in As])
        M = aat_to_mat_numpy(p, Vc, wc, x)
        Mref = -sum(xk * a for xk, a in zip(x, As))
        err = rc.relerr(M, Mref)
        print("RAGGED-OPS cpu %s block %d ks %d (clamped %d) | mat(AA'x) %.2e" % (name, i, ks, p["ks"], err))
        assert np.array_equal(M, M.T)
        assert err < TOL
        # the scaled form: F = Yc = W Vc gives W mat(AA' x) W
        W = rc.scaling(name)[i][0]
        errw = rc.relerr(aat_to_mat_numpy(p, W @ Vc, wc, x), W @ Mref @ W)
        assert errw < TOL
    err = rc.relerr(got, ref)
    print("RAGGED-OPS cpu %s | AA vec(Z) %.2e" % (name, err))
    assert err < TOL
    if name == "R1":
        assert got[2] == 0.0                       # the rank-0 row has no group
    if name == "R6":
        assert np.all(got[[0, 3, 7]] == 0.0)


# ---------------------------------------------------------------------------------------------- host opt-in
PARENT_FIELDS = ["A", "AA", "B", "C", "nzA", "sigmaA", "qA", "b", "b_const", "d_lin", "C_lin", "n", "msizes", "nlin", "nlmi",
                 "lowrank", "lowrank_note", "factored", "from_factors", "factored_blocks", "aa_fro", "stored", "factored_cg",
                 "factored_cg_diag", "diag", "local_support", "long_rows", "ragged"]


class _Stop(RuntimeError):
    pass


class _RecordingDevice:
    """Stands where the device would: takes the uploads, records the options and ends the run once ragged_ops is set."""

    def __init__(self):
        self.options = {}

    def set_option(self, key, value):
        self.options[key] = value
        if key == "ragged_ops":
            raise _Stop(key)

    def __getattr__(self, name):
        if name in ("upload_model", "upload_lowrank", "set_factored", "upload_diag"):
            return lambda *a, **k: None
        raise AttributeError(name)


@pytest.mark.parametrize("ragged,want", [(None, (0, 0)), (False, (0, 0)), (True, (1, 0)), ("ops", (1, 1))],
                         ids=["default", "False", "True", "ops"])
def test_host_opt_in(ragged, want):
    from loraine_jl_amd.optimizer import Optimizer
    P = rc.Planted()
    dev = _RecordingDevice()
    o = Optimizer(device=dev)
    o.set_silent(True)
    kw = {} if ragged is None else dict(ragged=ragged)
    o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True, factored_form=1, **kw)
    with pytest.raises(_Stop):
        o.optimize()
    assert (dev.options["lowrank_ragged"], dev.options["ragged_ops"]) == want
    with pytest.raises(ValueError):
        o.load_factored_model(P.F0(), P.factors(), P.b, ragged="columns")


def test_model_fields_are_unchanged():
    fm = rc.model("R2")
    assert [f.name for f in dataclasses.fields(fm)] == PARENT_FIELDS
    assert fm.ragged is False and fm.local_support is False and fm.long_rows is False
    assert RAGGED_CLASSES == (16, 8, 4, 2, 1)
