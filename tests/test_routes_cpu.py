"""The host's set-up of a solve sends the device what it always sent: for the grid of loader calls of route_cases.py the whole
log of a recording device -- option and upload calls in order, printed lines with verb = 1 -- equals
tests/golden/route_sequences.json, recorded before loraine_jl_amd/routes.py existed.  routes.resolve is also called by itself,
on the models alone.  No GPU."""
import pytest

import route_cases as rt
from loraine_jl_amd import routes
from loraine_jl_amd.model import MyModel

GOLD = rt.load()
CASES = rt.cases()


def test_the_grid_is_the_recorded_one():
    assert list(CASES) == list(GOLD)
    assert len(CASES) == 4 + 3 * 4 * 3 * 2 + 4 + 3


@pytest.mark.parametrize("name", list(GOLD))
def test_the_device_sees_the_recorded_sequence(name):
    assert CASES[name](rt.RecordingDevice()) == GOLD[name]


def test_the_grid_reaches_every_option_and_both_states():
    seen = {(e[1], e[2]) for log in GOLD.values() for run in (log if isinstance(log[0][0], list) else [log]) for e in run
            if e[0] == "set_option"}
    keys = ("pair_local", "pair_long", "lowrank_wide", "wide_diag", "cg_factored", "cg_diag", "lowrank_ragged", "ragged_ops",
            "ragged_cross", "ragged_ts")
    assert seen == {(k, v) for k in keys for v in (0, 1)} | {("cg_lowrank", -1)}
    refused = [name for name, log in GOLD.items() if log[-1][0] == "ValueError"]
    assert refused and all("kit=1" in name for name in refused)              # (the loaders refuse kit = 1 without the cg opt-in)


# ---------------------------------------------------------------------------------------------- resolve by itself
def _built(wide, **fields):
    """the model load_factored_model builds for the planted problem, without an Optimizer or a device"""
    from loraine_jl_amd.model import build_factored_model
    P, factors = rt.planted(wide)
    m = build_factored_model(P.F0(), factors, P.b, factored_form=1, max_rank=64 if wide else 16, wide_diag=wide == "diag")
    for k, v in fields.items():
        setattr(m, k, v)
    return m


def _sets(steps):
    return [(s.key, s.value) for s in steps]


def test_resolve_needs_no_device():
    m = _built("diag", ragged="all", factored_cg=True, factored_cg_diag=True, long_rows=True)
    assert isinstance(m, MyModel) and m.wide and m.wide_diag and m.local_support is False
    p = routes.resolve(m, 1, 64)
    assert _sets(p.after_upload) == [("pair_local", 0), ("pair_long", 1)] and all(s.sticky for s in p.after_upload)
    assert p.after_upload[0].line is None and "pair_long = 1" in p.after_upload[1].line
    assert _sets(p.before_lowrank) == [("lowrank_wide", 1)] and _sets(p.first_factored) == [("wide_diag", 1)]
    assert _sets(p.after_factored) == [("cg_factored", 1), ("cg_diag", 1), ("lowrank_ragged", 1), ("ragged_ops", 1),
                                       ("ragged_cross", 1), ("ragged_ts", 1)]
    assert [s.line is not None for s in p.after_factored] == [True, True, False, False, False, True]
    assert _sets(p.kit1) == [("cg_lowrank", -1)] and "rank-64" in p.kit1[0].line
    assert not any(s.sticky for stage in p[1:] for s in stage)
    # kit = 0: the CG options go back to the default, nothing under kit = 1
    p0 = routes.resolve(m, 0, 64)
    assert _sets(p0.after_factored)[:2] == [("cg_factored", 0), ("cg_diag", 0)] and p0.kit1 == ()
    assert all(s.line is None for s in p0.after_factored[:2])
    # a narrow model with ragged="ops"
    n = _built(False, ragged="ops")
    pn = routes.resolve(n, 0, 8)
    assert _sets(pn.before_lowrank) == [("lowrank_wide", 0)] and _sets(pn.first_factored) == [("wide_diag", 0)]
    assert _sets(pn.after_factored)[2:] == [("lowrank_ragged", 1), ("ragged_ops", 1), ("ragged_cross", 0), ("ragged_ts", 0)]
    assert all(s.line is None for s in pn.before_lowrank + pn.first_factored)


def test_resolve_on_a_model_that_is_not_a_mymodel():
    from loraine_jl_amd.synthetic import SyntheticDenseModel
    import numpy as np
    s = SyntheticDenseModel(8, 4, np.zeros(4), 1.0, np.zeros(4))
    p = routes.resolve(s, 0, 0)
    assert _sets(p.after_upload) == [("pair_local", 0), ("pair_long", 0)] and p.after_factored == () and p.kit1 == ()


def test_sticky_options_are_sent_when_on_or_left_on():
    dev, said = rt.RecordingDevice(), []
    on = (routes.Step("pair_local", 1, "a line", sticky=True), routes.Step("pair_long", 0, None, sticky=True))
    off = (routes.Step("pair_local", 0, None, sticky=True), routes.Step("pair_long", 0, None, sticky=True))
    routes.apply(dev, off, said.append)
    assert dev.log == [] and said == []                                        # never on: the library's default stands
    routes.apply(dev, on, said.append)
    routes.apply(dev, off, said.append)
    routes.apply(dev, off, said.append)
    assert dev.log == [["set_option", "pair_local", 1], ["set_option", "pair_local", 0]] and said == ["a line"]
    other = rt.RecordingDevice()
    routes.apply(dev, on, said.append)
    routes.apply(other, off, said.append)                                      # what one device was left at says nothing about another
    assert other.log == []
