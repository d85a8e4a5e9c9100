"""lrn_set_option on a real context (theta1 uploaded): every key is accepted with the value the golden file of
tests/test_options_cpu.py recorded as accepted, every recorded reject comes back with its code and text, an option that
invalidates the operator choice has lrn_matvec decide again, and a round trip through the defaults leaves the mode-0 assembly
bit for bit what it was."""
import os

import numpy as np
import pytest

import option_cases as oc
from oracle import loraine_oracle as lo

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_every_key_on_a_real_context():
    import loraine_jl_amd
    gold = oc.load()
    dev = loraine_jl_amd.Device(0)              # a context of its own: no error text from an earlier test
    try:
        lib, h = dev.lib, dev.h
        keys = oc.enumerated_keys(lib)
        assert sorted(keys) == sorted(list(gold["keys"]) + gold["skipped"])
        model = lo.model_from_sdpa(os.path.join(GOLD, "theta1.dat-s"))
        rng = np.random.default_rng(0)
        m = int(model.msizes[0])
        Gm = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
        W = Gm @ Gm.T
        dev.upload_model(model.AA, model.sigmaA, model.qA, model.msizes)
        dev.set_scaling(0, W, Gm)
        H0 = dev.schur_assemble(0, want_H=True).copy()

        # the rejects: those without a text first (they leave the text of the last error as it was: none so far)
        rejects = [(key, float(r[0]), r[1], r[2]) for key, e in gold["keys"].items() for r in e["records"] if r[1] != 0]
        assert len(rejects) >= 30
        for key, value, rc, text in sorted(rejects, key=lambda t: t[3] != ""):
            assert lib.lrn_set_option(h, key.encode(), value) == rc, (key, value)
            assert lib.lrn_last_error(h).decode() == text, (key, value)
        assert lib.lrn_set_option(h, b"no_such_option", 1.0) == -1
        assert lib.lrn_last_error(h).decode() == "unknown option no_such_option"

        # every key that is no test hook: an accepted value, then the default again
        plain = [k for k in keys if k not in gold["test_hooks"]]
        assert len(plain) == len(keys) - 2
        for key in plain:
            value = gold["keys"][key]["accepted"] if key in gold["keys"] else 1.0      # (detect_release: nothing to release)
            assert lib.lrn_set_option(h, key.encode(), value) == 0, (key, value)
        for key in plain:
            default = gold["keys"][key]["default"] if key in gold["keys"] else None
            if default is not None:
                assert lib.lrn_set_option(h, key.encode(), default) == 0, (key, default)
        H1 = dev.schur_assemble(0, want_H=True)
        assert H1.tobytes() == H0.tobytes()

        # matvec_h invalidates the operator choice: forced through H once, then "never" -- lrn_matvec must not go on with the
        # choice it had taken for this scaling
        x = rng.standard_normal(model.n)
        dev.set_option("matvec_h", 2)
        n0 = dev.count("hop_matvec")
        by_h = dev.matvec(x)
        assert dev.count("hop_matvec") == n0 + 1
        dev.set_option("matvec_h", 1)
        free = dev.matvec(x)
        assert dev.count("hop_matvec") == n0 + 1
        assert np.linalg.norm(by_h - free) <= 1e-12 * np.linalg.norm(free)
        dev.set_option("matvec_h", 0)
    finally:
        dev.close()
