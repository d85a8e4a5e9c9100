"""bench.py end to end on a small instance: a plain run prints the headline line only and `--dump-outputs` writes what
the last timed step computed (both solves against the dumped Schur matrix); `--full` adds the per-kernel, alongside
and cross-rank figures, and the same arguments give the same outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSZ, NVAR, SEED = 256, 300, 20250614
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "phase_ms_per_step", "dely_checksum", "alongside")


def _bench(out_dir, *extra):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--msz", str(MSZ),
        "--nvar", str(NVAR), "--seed", str(SEED), "--dump-outputs", str(out_dir), *extra]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l_ for l_ in p.stdout.splitlines() if l_.startswith("{")][-1]
    return json.loads(line)


def _dumped(out_dir):
    d = {n: np.load(os.path.join(out_dir, n + ".npy")) for n in ("dely_predictor", "dely_corrector", "schur_H_sample")}
    assert all(a.dtype == np.float64 for a in d.values())
    return d


def test_bench_plain_and_full_runs_dump_the_last_step(tmp_path):
    plain = _bench(tmp_path / "plain")
    for k in HEADLINE:
        assert k in plain
    assert plain["steps"] == 3 and plain["value"] == plain["ms_per_step"] > 0
    assert plain["unit"] == "ms" and plain["higher_is_better"] is False and plain["dtype"] == "f64"
    assert not any(k in plain for k in FULL_ONLY + ("cpu_baseline",))
    d = _dumped(tmp_path / "plain")
    assert d["dely_predictor"].shape == d["dely_corrector"].shape == (NVAR,)
    H = d["schur_H_sample"].reshape(NVAR, NVAR, order="F")          # all of H at this size
    assert np.array_equal(H, H.T)
    rng = np.random.default_rng(SEED + 2)                           # bench.py's right-hand sides
    h_pred, h_corr = rng.standard_normal(NVAR), rng.standard_normal(NVAR)
    for h, x in ((h_pred, d["dely_predictor"]), (h_corr, d["dely_corrector"])):
        x_ref = np.linalg.solve(H, h)
        assert np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref) < 1e-9

    full = _bench(tmp_path / "full", "--full", "--no-cpu-baseline")
    for k in HEADLINE + FULL_ONLY:
        assert k in full
    assert full["roofline"]["achieved"] > 0 and full["phase_ms_per_step"]["assemble"] > 0
    e = _dumped(tmp_path / "full")
    x = e["dely_corrector"]
    assert abs(full["dely_checksum"] - x.sum()) <= 1e-12 * np.abs(x).sum()
    for n in d:                                                     # same arguments -> same inputs -> same outputs
        assert np.allclose(e[n], d[n], rtol=1e-12, atol=1e-14 * np.abs(d[n]).max())
