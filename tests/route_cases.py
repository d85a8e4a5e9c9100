"""What the host sends to the device while a solver is set up: every option and upload call in order, and the lines it prints
with verb = 1, for a grid of loader calls.  A recording device stands where the device would and ends the run at the first call
that is neither an option nor an upload (the first call of the solve).

tests/golden/route_sequences.json was recorded with this module on the commit before loraine_jl_amd/routes.py existed, when
MySolver.__init__ decided the options in line; `python tests/route_cases.py` records it again -- the file must come out
unchanged."""
import io
import itertools
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_sequences.json")


class Stop(RuntimeError):
    pass


class RecordingDevice:
    """records (call, arguments that matter) and the printed lines, in one log"""

    def __init__(self):
        self.log = []

    def set_option(self, key, value):
        self.log.append(["set_option", key, value])

    def upload_model(self, *a, **k):
        self.log.append(["upload_model"])

    def upload_lowrank(self, i, khat, V, d):
        self.log.append(["upload_lowrank", int(i), int(khat)])

    def set_factored(self, i):
        self.log.append(["set_factored", int(i)])

    def upload_diag(self, i, rows, a):
        self.log.append(["upload_diag", int(i), [int(r) for r in rows]])

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def stop(*a, **k):
            raise Stop(name)
        return stop


class _Lines(io.TextIOBase):
    """stdout into the device's log, line by line"""

    def __init__(self, log):
        self.log, self.part = log, ""

    def write(self, s):
        self.part += s
        while "\n" in self.part:
            line, self.part = self.part.split("\n", 1)
            self.log.append(["print", line])
        return len(s)


def run(dev, load, attrs=None):
    """load(optimizer) names the model; -> the log of this run on dev (an earlier run's entries are dropped).  A ValueError of the
    loader or of the set-up is the last entry"""
    from loraine_jl_amd.optimizer import Optimizer
    del dev.log[:]
    o = Optimizer(device=dev)
    for k, v in (attrs or {}).items():
        o.set_attribute(k, v)
    out, sys.stdout = sys.stdout, _Lines(dev.log)
    try:
        load(o)
        o.optimize()
        raise AssertionError("the recording device did not end the run")
    except Stop as e:
        dev.log.append(["stop", str(e)])
    except ValueError as e:
        dev.log.append(["ValueError", str(e)])
    finally:
        sys.stdout = out
    return [list(e) for e in dev.log]


# ---------------------------------------------------------------------------------------------- the models
def stored_model():
    import long_rows_cases as lr
    return lr.trace_model(24)


def rank2_model(m=8, n=5, seed=3):
    """constraints of rank 2, A_k = v v' - w w', for datarank = 2"""
    rng = np.random.default_rng(seed)
    mats = [-np.eye(m)]
    for _ in range(n):
        v, w = rng.standard_normal((2, m))
        mats.append(np.outer(v, v) - np.outer(w, w))
    return [mats], np.ones(n)


def planted(wide):
    import ragged_cases as rc
    import wide_diag_cases as wd
    if wide is False:
        P = rc.Planted()
        return P, P.factors()
    P = wd.PlantedWideDiag()
    return P, (P.factors() if wide == "diag" else P.stored_trace_factors())


CG, RAGGED, WIDE, KIT = (False, True, "diag"), (False, True, "ops", "all"), (False, True, "diag"), (0, 1)


def cases():
    """name -> function of a device that returns the log (or the list of logs of a sequence on that one device)"""
    out = {}
    A, b = stored_model()
    for local, long_rows in itertools.product((False, True), repeat=2):
        out[f"load_model local_support={local} long_rows={long_rows}"] = (
            lambda dev, local=local, long_rows=long_rows: run(dev, lambda o: o.load_model(A, b, local_support=local, long_rows=long_rows)))
    for cg, ragged, wide, kit in itertools.product(CG, RAGGED, WIDE, KIT):
        def one(dev, cg=cg, ragged=ragged, wide=wide, kit=kit):
            P, factors = planted(wide)
            return run(dev, lambda o: o.load_factored_model(P.F0(), factors, P.b, max_sense=True, factored_form=1, cg=cg,
                                                            ragged=ragged, wide=wide), dict(kit=kit))
        out[f"load_factored_model cg={cg!r} ragged={ragged!r} wide={wide!r} kit={kit}"] = one
    A2, b2 = rank2_model()
    for kit in KIT:
        out[f"load_model datarank=2 kit={kit}"] = lambda dev, kit=kit: run(dev, lambda o: o.load_model(A2, b2), dict(datarank=2, kit=kit))
        out[f"load_model datarank=2 kit={kit} no factors"] = lambda dev, kit=kit: run(dev, lambda o: o.load_model(A, b),
                                                                                       dict(datarank=2, kit=kit))
    # a device an earlier solve used: on -> off -> off
    for name, on in (("pair_local", dict(local_support=True)), ("pair_long", dict(long_rows=True)),
                     ("pair_local and pair_long", dict(local_support=True, long_rows=True))):
        out[f"used device {name}: on, off, off"] = lambda dev, on=on: [run(dev, lambda o, kw=kw: o.load_model(A, b, **kw))
                                                                       for kw in (on, {}, {})]
    return out


def record():
    return {name: fn(RecordingDevice()) for name, fn in cases().items()}


def dump(data, path):
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in data.items()) + "\n}\n")


def load():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import loraine_jl_amd  # noqa: F401
    dump(record(), sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
