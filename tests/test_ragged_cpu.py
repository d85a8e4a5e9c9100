"""CPU: the rank-class route of the rank-k Schur assembly (library option lowrank_ragged) without a GPU -- the Python restatement
of the planner (loraine_jl_amd.model.ragged_plan; csrc/ragged_plan.h is the same function) against hand-written expectations,
a NumPy float64 restatement of the whole route (class sort, compaction, T = U_c' B_c, weighted squares, block sums, scatter
through gh into the lower triangle, tile by tile as the kernel walks them) against H_ij = tr(A_i W A_j W) from the materialised
constraints, and the host opt-in.  The restatement checks the algebra and the tile list, not the kernel."""
import dataclasses

import numpy as np
import pytest

import ragged_cases as rc
from loraine_jl_amd.model import RAGGED_CLASSES, RAGGED_TILE, ragged_plan


# ---------------------------------------------------------------------------------------------- planner
def _cyc(rank):
    """H indices of R2's constraints 8 .. 36 of the given rank (they cycle 1, 2, 4, 8)."""
    return [8 + k for k in range(29) if (1, 2, 4, 8)[k % 4] == rank]


EXPECT = {
    # name: (segments by class 16, 8, 4, 2, 1, classes present, tiles, gh)
    "R1": ([(0, 16), (16, 16), (16, 20), (20, 22), (22, 23)], 4, 10, [0, 3, 4, 1]),
    "R2": ([(0, 128), (128, 184), (184, 212), (212, 226), (226, 234)], 5, 21,
           list(range(8)) + _cyc(8) + _cyc(4) + _cyc(2) + _cyc(1)),
    "R3": ([(0, 16), (16, 16), (16, 16), (16, 16), (16, 145)], 2, 10, [64] + list(range(64)) + list(range(65, 130))),
    "R4": ([(0, 0), (0, 296), (296, 296), (296, 362), (362, 362)], 2, 28, list(range(33, 70)) + list(range(33))),
    "R6": ([(0, 80), (80, 136), (136, 164), (164, 178), (178, 186)], 5, 21,
           [1, 2, 4, 5, 6] + _cyc(8) + _cyc(4) + _cyc(2) + _cyc(1)),
    # degenerate lists: all equal, all zero, a single constraint
    "equal": ([(0, 0), (0, 0), (0, 0), (0, 10), (10, 10)], 1, 1, [0, 1, 2, 3, 4]),
    "zero": ([(0, 0)] * 5, 0, 0, []),
    "single": ([(0, 16), (16, 16), (16, 16), (16, 16), (16, 16)], 1, 1, [0]),
}
LISTS = {"equal": [2] * 5, "zero": [0] * 4, "single": [9]}


@pytest.mark.parametrize("name", list(EXPECT))
def test_planner_against_hand_written_expectations(name):
    ranks = LISTS[name] if name in LISTS else rc.ranks_of(name)
    p = ragged_plan(ranks)
    seg, ncls, tiles, gh = EXPECT[name]
    assert [p["seg"][c] for c in RAGGED_CLASSES] == seg
    assert p["Rc"] == seg[-1][1] and p["ncls"] == ncls and p["tiles"] == tiles and p["gh"] == gh
    want = [0 if r == 0 else min(c for c in RAGGED_CLASSES if c >= r) for r in ranks]
    assert p["classes"] == want
    if name in rc.SIZES:      # the ranks the padded upload shows the library are those of the case
        fm = rc.model(name)
        assert rc.block_ranks(fm, 0) == ranks


def test_planner_of_the_motivating_shape():
    """3999 rank-1 constraints and one of rank 9: khat = 16 pads to 64000 columns, the classes keep 4015."""
    p = ragged_plan([1] * 3999 + [9])
    assert p["Rc"] == 4015 and p["ncls"] == 2 and p["gh"][0] == 3999
    nt1 = -(-3999 // RAGGED_TILE)
    assert p["tiles"] == 1 + nt1 + nt1 * (nt1 + 1) // 2
    with pytest.raises(ValueError):
        ragged_plan([17])


# ---------------------------------------------------------------------------------------------- algebra
def _tiles(p):
    """The tile list of csrc/ragged_plan.h::plan_ragged: (r0, r1, c0, c1, gi0, gj0, ka, kb, diag)."""
    grp0, g = {}, 0
    for c in RAGGED_CLASSES:
        grp0[c] = g
        g += (p["seg"][c][1] - p["seg"][c][0]) // c
    out = []
    for ia, a in enumerate(RAGGED_CLASSES):
        for b in RAGGED_CLASSES[ia:]:
            (a0, a1), (b0, b1) = p["seg"][a], p["seg"][b]
            ta, tb = -(-(a1 - a0) // RAGGED_TILE), -(-(b1 - b0) // RAGGED_TILE)
            for ti in range(ta):
                for tj in range(ti + 1 if a == b else tb):
                    r0, c0 = a0 + ti * RAGGED_TILE, b0 + tj * RAGGED_TILE
                    out.append((r0, min(r0 + RAGGED_TILE, a1), c0, min(c0 + RAGGED_TILE, b1), grp0[a] + ti * RAGGED_TILE // a,
                                grp0[b] + tj * RAGGED_TILE // b, a, b, a == b and ti == tj))
    return out


def _route_numpy(V, d, khat, W, G, n, H, pairs):
    """H += the rank-class route of one block, in float64; pairs[(gi, gj)] counts the writers of every pair of groups."""
    Vp = np.asarray(V.todense()).reshape(n, khat, -1)            # constraint, column, msz
    d = np.asarray(d, float).reshape(n, khat)
    ranks = np.count_nonzero(d, axis=1).tolist()
    p = ragged_plan(ranks)
    m = W.shape[0]
    Vc, wc = np.zeros((m, p["Rc"])), np.zeros(p["Rc"])
    col = 0
    for h, c in zip(p["gh"], [c for c in RAGGED_CLASSES for _ in range((p["seg"][c][1] - p["seg"][c][0]) // c)]):
        assert p["seg"][c][0] <= col < p["seg"][c][1]
        k = col
        for q in range(khat):
            if d[h, q] != 0.0:
                Vc[:, k], wc[k] = Vp[h, q], d[h, q]
                k += 1
        col += c
    assert col == p["Rc"]
    Uc = G.T @ Vc if G is not None else W @ Vc
    Bc = Uc if G is not None else Vc
    tiles = _tiles(p)
    assert len(tiles) == p["tiles"]
    for r0, r1, c0, c1, gi0, gj0, ka, kb, diag in tiles:
        T = Uc[:, r0:r1].T @ Bc[:, c0:c1]
        S = T * T * np.outer(wc[r0:r1], wc[c0:c1])
        for bi in range((r1 - r0) // ka):
            for bj in range((c1 - c0) // kb):
                gi, gj = gi0 + bi, gj0 + bj
                if diag and gi < gj:
                    continue
                hi, hj = p["gh"][gi], p["gh"][gj]
                H[max(hi, hj), min(hi, hj)] += S[bi * ka:(bi + 1) * ka, bj * kb:(bj + 1) * kb].sum()
                key = (max(gi, gj), min(gi, gj))
                pairs[key] = pairs.get(key, 0) + 1
    return len(p["gh"])


@pytest.mark.parametrize("with_G", [True, False], ids=["G", "W-only"])
@pytest.mark.parametrize("name", rc.NAMES)
def test_algebra_of_the_route_matches_the_reference(name, with_G):
    fm = rc.model(name)
    n = rc.nvar(name)
    H = np.zeros((n, n))
    for i, ((V, d, khat), (W, G)) in enumerate(zip(fm.lowrank, rc.scaling(name))):
        pairs = {}
        ng = _route_numpy(V, d, khat, W, G if with_G else None, n, H, pairs)
        # every unordered pair of groups, the diagonal included, exactly once
        assert len(pairs) == ng * (ng + 1) // 2 and set(pairs.values()) <= {1}
    H = np.tril(H) + np.tril(H, -1).T
    ref = rc.reference(name).copy()
    if name == "R5":
        C = rc.c_lin(name).toarray()
        ref -= C @ C.T                         # (the route is H_FF of the LMI blocks)
    if name == "R6":                           # ... and of the factored constraints: stored and diagonal rows get nothing
        out = [0, 3, 7]
        assert np.all(H[out, :] == 0.0) and np.all(H[:, out] == 0.0)
        ref[out, :] = 0.0
        ref[:, out] = 0.0
    err = rc.relerr(H, ref)
    print("RAGGED cpu %s %s | %.2e" % (name, "G" if with_G else "W-only", err))
    assert err < 1e-12


# ---------------------------------------------------------------------------------------------- host opt-in
PARENT_FIELDS = ["A", "AA", "B", "C", "nzA", "sigmaA", "qA", "b", "b_const", "d_lin", "C_lin", "n", "msizes", "nlin", "nlmi",
                 "lowrank", "lowrank_note", "factored", "from_factors", "factored_blocks", "aa_fro", "stored", "factored_cg",
                 "factored_cg_diag", "diag"]


class _Stop(RuntimeError):
    pass


class _RecordingDevice:
    """Stands where the device would: takes the uploads, records the options and ends the run once lowrank_ragged is set."""

    def __init__(self):
        self.options = {}

    def set_option(self, key, value):
        self.options[key] = value
        if key == "lowrank_ragged":
            raise _Stop(key)

    def __getattr__(self, name):
        if name in ("upload_model", "upload_lowrank", "set_factored", "upload_diag"):
            return lambda *a, **k: None
        raise AttributeError(name)


@pytest.mark.parametrize("ragged", [None, False, True])
def test_host_opt_in(ragged):
    from loraine_jl_amd.optimizer import Optimizer
    P = rc.Planted()
    dev = _RecordingDevice()
    o = Optimizer(device=dev)
    o.set_silent(True)
    kw = {} if ragged is None else dict(ragged=ragged)
    o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True, factored_form=1, **kw)
    assert o._pending[1][-1] is False                                # (cg stays the last word of the pending load)
    with pytest.raises(_Stop):
        o.optimize()
    assert dev.options["lowrank_ragged"] == (1 if ragged else 0)
    assert dev.options["cg_factored"] == 0 and dev.options["cg_diag"] == 0


def test_default_model_is_the_parents():
    fm = rc.model("R2")
    names = [f.name for f in dataclasses.fields(fm)]
    assert names == PARENT_FIELDS + ["local_support", "long_rows", "ragged"]      # (the two opt-ins of the stored routes: declared, off)
    assert fm.ragged is False and fm.local_support is False and fm.long_rows is False
    fm2 = dataclasses.replace(fm, ragged=True)
    for f in PARENT_FIELDS:
        assert getattr(fm2, f) is getattr(fm, f)
