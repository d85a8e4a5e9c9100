"""CPU: the cross terms of the mode-1 assembly and ts of H_alpha of a mixed-rank factored block on the compacted columns (library
options ragged_cross and ragged_ts) without a GPU.

1. hg, the H index -> group map (loraine_jl_amd.model.ragged_columns; csrc/ragged_plan.h fills the same map in plan_ragged): the
   inverse of gh on the groups, -1 exactly on the constraints of rank 0, for every case of tests/ragged_cases.py and of
   tests/ragged_rest_cases.py.
2. The compacted algebra in NumPy float64 (ragged_rest_cases.h_by_group, ts_by_group: cross terms by group, C of the diagonal
   parts by class, ts by group) against the np.longdouble reference H and against cr.prec_alpha_matrix of the materialised
   model, for X1, X2, T1.  Bounds of the sibling CPU tests: 1e-12 relative Frobenius for H (tests/test_ragged_cpu.py) and for
   H_alpha from the ts formula (tests/test_cg_diag_cpu.py).
3. The host opt-in: load_factored_model(ragged="all") is accepted and sets the four library options, "ops" / True / False set
   the two new ones to 0, another string is refused with a text that names the accepted values."""
import numpy as np
import pytest

import ragged_cases as rc
import ragged_rest_cases as rr
from loraine_jl_amd.model import ragged_columns, ragged_plan
from oracle import cg_reference as cr

TOL = 1e-12
RANK_LISTS = {name: rc.ranks_of(name) for name in ("R1", "R2", "R3", "R4", "R5b", "R6")}


def _ranks(name):
    return RANK_LISTS[name] if name in RANK_LISTS else rr.block_ranks(name)


@pytest.mark.parametrize("name", list(RANK_LISTS) + rr.NAMES)
def test_hg_is_the_inverse_of_gh(name):
    ranks = _ranks(name)
    p = ragged_columns(ranks)
    hg, gh = p["hg"], p["gh"]
    assert len(hg) == len(ranks)
    assert [hg[h] for h in gh] == list(range(len(gh)))                       # inverse on the groups
    assert [h for h, g in enumerate(hg) if g < 0] == [h for h, r in enumerate(ranks) if r == 0]
    assert all(gh[g] == h for h, g in enumerate(hg) if g >= 0)
    assert set(ragged_plan(ranks)) == {"classes", "seg", "Rc", "ncls", "gh", "tiles"}      # ragged_plan returns what it returned


def test_the_cases_are_the_ones_the_gpu_test_counts_on():
    assert rr.block_ranks("X1") == rc.ranks_of("R6")
    assert rr.stored_rows("X1") == [0, 7] and rr.diag_rows("X1") == [3]
    p = ragged_plan([rr.X2_RANKS[k % 6] for k in range(90)])                 # X2 as drawn
    assert [p["seg"][c][0] for c in (16, 8, 4, 2, 1)] == [0, 480, 600, 660, 690] and p["Rc"] == 705
    p = ragged_plan(rr.block_ranks("X2"))                                    # ... and as the device sees it
    assert [p["seg"][c][0] for c in (16, 8, 4, 2, 1)] == [0, 464, 584, 644, 670] and p["Rc"] == 684 and p["ncls"] == 5
    assert rr.factored_model("X2").lowrank[0][2] == 16
    assert rr.stored_rows("X2") == [0, 5, 31] and len(rr.diag_rows("X2")) == 21 and rr.X2_TRACE in rr.diag_rows("X2")
    assert {rr.block_ranks("X2")[k] for k in rr.X2_DIAG} == {1, 2, 3, 5, 9, 16}        # diagonal parts in every class
    p = ragged_plan(rr.block_ranks("T1"))
    assert p["ncls"] == 5 and rr.factored_model("T1").lowrank[0][2] == 16 and p["Rc"] < 65 * 16
    assert [h for h, r in enumerate(rr.block_ranks("T1")) if r == 0] == [0, 63, 64]
    assert rr.stored_rows("T1") == [0, 64] and rr.diag_rows("T1") == [1, 63]


@pytest.mark.parametrize("name", rr.NAMES)
def test_h_by_group_is_the_reference_h(name):
    ref = rr.reference_h(name)
    H = rr.h_by_group(name)
    rows = rr.cross_rows(name)
    err, errx = rc.relerr(H, ref), rc.relerr(H[rows, :], ref[rows, :])
    print("RAGGED-REST cpu %s | H %.2e, rows of the stored and diagonal constraints %.2e" % (name, err, errx))
    assert err < TOL
    assert errx < TOL


@pytest.mark.parametrize("erank", [1, 2])
@pytest.mark.parametrize("name", rr.NAMES)
def test_ts_by_group_gives_the_reference_h_alpha(name, erank):
    c = rr.case(name)
    ref = cr.prec_alpha_matrix(c.model, c.W, erank, 1, c.X_lin, c.S_lin_inv)
    M = rr.ts_by_group(name, erank)
    err = cr.relerr(M.ravel(), ref.ravel())
    print("RAGGED-REST cpu ts %s erank=%d | H_alpha vs prec_alpha_matrix %.2e" % (name, erank, err))
    assert err < 1e-12


# ---------------------------------------------------------------------------------------------- host opt-in
OPTIONS = ("lowrank_ragged", "ragged_ops", "ragged_cross", "ragged_ts")


class _Stop(RuntimeError):
    pass


class _RecordingDevice:
    """Stands where the device would: takes the uploads, records the options and ends the run at the option set after the four."""

    def __init__(self):
        self.options = {}

    def set_option(self, key, value):
        if key not in OPTIONS and all(k in self.options for k in OPTIONS[:2]):
            raise _Stop(key)
        self.options[key] = value

    def __getattr__(self, name):
        if name in ("upload_model", "upload_lowrank", "set_factored", "upload_diag"):
            return lambda *a, **k: None
        raise _Stop(name)


@pytest.mark.parametrize("ragged,want", [(None, (0, 0, 0, 0)), (False, (0, 0, 0, 0)), (True, (1, 0, 0, 0)), ("ops", (1, 1, 0, 0)),
                                         ("all", (1, 1, 1, 1))], ids=["default", "False", "True", "ops", "all"])
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
    assert tuple(dev.options[k] for k in OPTIONS) == want
    if ragged is not None:
        assert o.solver is None or o.solver.model.ragged == ragged


def test_a_bad_string_is_refused_with_the_accepted_values():
    from loraine_jl_amd.optimizer import Optimizer
    P = rc.Planted()
    o = Optimizer(device=_RecordingDevice())
    with pytest.raises(ValueError, match=r'ragged is False, True, "ops" or "all", not \'columns\''):
        o.load_factored_model(P.F0(), P.factors(), P.b, ragged="columns")
