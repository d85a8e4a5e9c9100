"""Which library options a model's opt-in routes need, decided in one place and without a device.

`resolve(model, kit, datarank)` reads the model once and returns a `Plan`: per stage of the set-up in `MySolver.__init__` the
options to set, in order, each with the line the solver prints after it.  `apply` sends one stage to a device.  A new route
is one more `Step` here (and one line in the option table of csrc/options.h).

Every option is sent in both states, so that a device an earlier solve used comes back to the library's default -- except the
sticky ones, which are sent only when they are turned on, or when an earlier solve left them on for that device: a solve
that never asked for them sends nothing."""
import weakref
from typing import NamedTuple, Optional, Tuple


class Step(NamedTuple):
    key: str
    value: int
    line: Optional[str] = None      # printed (verb > 0) after the option is set
    sticky: bool = False


class Plan(NamedTuple):
    after_upload: Tuple[Step, ...]       # after upload_model
    before_lowrank: Tuple[Step, ...]     # before the first upload_lowrank
    first_factored: Tuple[Step, ...]     # after the first set_factored, before any upload_diag
    after_factored: Tuple[Step, ...]     # after the last block's factors (a factored model only)
    kit1: Tuple[Step, ...]               # the CG path from the factors (kit = 1 only)


# device -> the sticky keys an earlier solve left on
_LEFT_ON = weakref.WeakKeyDictionary()


def resolve(model, kit, datarank) -> Plan:
    def get(name, default=False):         # (synthetic.SyntheticDenseModel is not a MyModel and has none of these)
        return getattr(model, name, default)

    # load_model(..., local_support=True): stored constraints with a small support through A[S, S]
    # long_rows=True of the loaders: long sparse stored constraints from Z = (A W) on their rows
    local, long_rows = bool(get("local_support")), bool(get("long_rows"))
    after_upload = (
        Step("pair_local", int(local), " ---Stored constraints with a support of at most 32 are assembled from A[S, S] "
                                       "(pair_local = 1)" if local else None, sticky=True),
        Step("pair_long", int(long_rows), " ---Long sparse stored constraints are assembled from Z = (A W) on their rows "
                                          "(pair_long = 1)" if long_rows else None, sticky=True))
    # load_factored_model(..., wide=True): constraints of rank 17 .. 64, khat 32 or 64
    wide = bool(get("wide"))
    before_lowrank = (
        Step("lowrank_wide", int(wide), " ---Factored constraints carry up to 64 factor columns; their blocks are assembled by "
                                        "rank class (lowrank_wide = 1)" if wide else None),)
    # load_factored_model(..., wide="diag"): diagonal parts on a wide block.  Set where it is first needed, before any upload_diag;
    # upload_model has cleared the diagonal rows of a used block, so no wide upload_lowrank before it met any
    wide_diag = bool(get("wide_diag"))
    first_factored = (
        Step("wide_diag", int(wide_diag), " ---Wide factored blocks carry diagonal parts (wide_diag = 1)" if wide_diag else None),)
    after_factored = ()
    if get("factored"):
        # kit = 1 on a factored model: check_factored_kit has passed, the model was loaded with cg=True
        # ... with diagonal parts only when it was loaded with cg="diag" (check_diag_kit)
        cg = kit == 1
        cg_diag = cg and bool(get("factored_cg_diag"))
        # load_factored_model(..., ragged=True): blocks of mixed ranks are assembled by rank class
        # ... ragged="ops": and their two data operators run on the same compacted columns
        # ... ragged="all": and the cross terms of the assembly and ts of H_alpha
        rg = get("ragged")
        rest = isinstance(rg, str) and rg == "all"
        ragged, ops = bool(rg), rest or (isinstance(rg, str) and rg == "ops")
        if rest:
            line = (" ---The Schur assembly with its cross terms, the data operators and H_alpha group the factored "
                    "constraints by rank class (lowrank_ragged = 1, ragged_ops = 1, ragged_cross = 1, ragged_ts = 1)")
        elif ops:
            line = (" ---The Schur assembly and the data operators group the factored constraints by rank class "
                    "(lowrank_ragged = 1, ragged_ops = 1)")
        elif ragged:
            line = " ---The Schur assembly groups the factored constraints by rank class (lowrank_ragged = 1)"
        else:
            line = None
        after_factored = (
            Step("cg_factored", int(cg), " ---The CG path runs from the factors of the factored blocks (cg_factored = 1)" if cg else None),
            Step("cg_diag", int(cg_diag), " ---The CG path holds the diagonal parts of the factored blocks (cg_diag = 1)" if cg_diag else None),
            Step("lowrank_ragged", int(ragged)), Step("ragged_ops", int(ops)), Step("ragged_cross", int(rest)),
            Step("ragged_ts", int(rest), line))
    # kit = 1 with rank-k factors: the CG path from them wherever the library's cost model finds that cheaper
    kit1 = (Step("cg_lowrank", -1, f" ---The CG path uses the rank-{datarank} factors of the data (cg_lowrank = -1)"),) if kit == 1 else ()
    return Plan(after_upload, before_lowrank, first_factored, after_factored, kit1)


def apply(dev, steps, say):
    """Sends one stage of a plan to dev; say(line) prints."""
    for s in steps:
        if s.sticky:
            left_on = _LEFT_ON[dev] if dev in _LEFT_ON else ()
            if not s.value and s.key not in left_on:
                continue                   # never on for this device: it is at the library's default
        dev.set_option(s.key, s.value)
        if s.sticky and s.value:
            _LEFT_ON.setdefault(dev, set()).add(s.key)
        elif s.sticky:
            _LEFT_ON[dev].discard(s.key)
        if s.line:
            say(s.line)
