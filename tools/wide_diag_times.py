"""Times of the mode-1 Schur assembly of a WIDE factored block with diagonal parts, A_k = V_k D_k V_k' + diag(a_k) with up to 64
factor columns (library option wide_diag beside lowrank_wide; csrc/diagops.hip::diag_sq_wide_mfma_kernel), at msz 2000 / nvar
4000 with dense random factors and dense diagonals.

Timed with the library's device events (option "profile") as the median of --reps runs after a warm-up: "assemble" = the whole
lrn_schur_assemble, "diag_cross" = C = Ad' (Y o Y) and its scatter, "diag_dd" = H_DD.  One process and one context per
configuration: the driver (no --config) starts `python tools/wide_diag_times.py --config X` for every X under a time limit of its
own and collects the JSON line each prints; a configuration that fails or runs out of time is recorded as such and the others go
on being measured only if it ended by itself (a time limit or a signal ends the driver: nothing more is started on the GPU).
    a      3990 x rank 1 and ten x (rank 40 + dense diagonal): khat 64, ten diagonal rows, padded and under ragged="all"
    a0     the same model the only way it could be said before: the ten as stored dense matrices in a hybrid block of khat 1
    b      a with constraint 10 the trace row (None, [], ones): eleven diagonal rows
    b0     a0 with the trace row as a stored sparse identity
    c      every constraint rank 32 + a dense diagonal: khat 32, 4000 diagonal rows (Rc = R: ragged_cross keeps the padded layout).
           No baseline: as stored matrices the constraints are 4000 x 2000^2 x 8 bytes = 128 GB.  In the same context then
    d32    diag_sq at kh 32 with 1, 16, 64, 4000 diagonal rows in both forms ("diag_cross")
    d64    every constraint rank 64: diag_sq at kh 64, the same sweep
device_bytes / device_bytes_peak are what the context holds after / held at most during its assemblies.

    python tools/wide_diag_times.py --out profiles/wide_diag_times.json
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEYS = ("assemble", "diag_cross", "diag_dd", "diag_stored", "ragged", "hybrid_cross")
CONFIGS = ("a", "a0", "b", "b0", "c", "d64")
LIMITS = dict(a=240, a0=240, b=240, b0=240, c=420, d64=600)       # seconds per configuration (its own process)
RAGGED = ("lowrank_ragged", "ragged_ops", "ragged_cross", "ragged_ts")
SWEEP = (1, 16, 64, 4000)


def upload_factors(dev, m, n, kh, ranks, V, d):
    """V (m x sum ranks, the weighted columns constraint by constraint), d their weights -> lrn_upload_lowrank at khat = kh; the
    padding columns have no entry and weight 0."""
    from loraine_jl_amd._capi import ptr
    rows = np.concatenate([k * kh + np.arange(r) for k, r in enumerate(ranks)]).astype(np.int64) + 1
    nl = rows.size
    cp = np.arange(m + 1, dtype=np.int64) * nl + 1
    rv = np.tile(rows, m)
    w = np.zeros(n * kh)
    w[rows - 1] = d
    nz = np.ascontiguousarray(V).ravel()
    dev._chk(dev.lib.lrn_upload_lowrank(dev.h, 0, kh, ptr(cp), ptr(rv), ptr(nz), ptr(w)), "lrn_upload_lowrank")


def timed(dev, reps):
    dev.schur_assemble(1)                                    # warm-up (dense copies of V, the plan, workspaces)
    runs = {k: [] for k in KEYS}
    for _ in range(reps):
        dev.set_option("reset_timing", 1)
        dev.schur_assemble(1)
        for k in KEYS:
            runs[k].append(dev.timing(k))
    out = {k + "_ms": float(np.median(v)) for k, v in runs.items()}
    out["assemble_runs_ms"] = runs["assemble"]
    return out


def both_layouts(dev, reps):
    """Padded, then under the four options of ragged="all"."""
    e = dict(padded=timed(dev, reps))
    for k in RAGGED:
        dev.set_option(k, 1)
    e["ragged_all"] = timed(dev, reps)
    e["ragged_all"]["diag_cross_by_class"] = dev.count("ragged_cross_fallback") == 0
    for k in RAGGED:
        dev.set_option(k, 0)
    return e


def sweep(dev, m, n, kh, reps, rng):
    """diag_sq at kh with 1 .. 4000 diagonal rows in both forms: "diag_cross" of the assembly (C and its scatter)."""
    out = {}
    for ns in SWEEP:
        ns = min(ns, n)
        dev.upload_diag(0, list(range(ns)), rng.standard_normal((m, ns)))
        e = {}
        for form, key in ((0, "rows"), (1, "mfma")):
            dev.set_option("diag_sq_mfma", form)
            t = timed(dev, reps)
            used = (dev.count("diag_sq_rows"), dev.count("diag_sq_mfma"))      # (of the last assembly: reset_timing clears them)
            assert (used[1] == 0) if form == 0 else (used[0] == 0), used
            e[key + "_diag_cross_ms"] = t["diag_cross_ms"]
            e[key + "_diag_dd_ms"] = t["diag_dd_ms"]
        dev.set_option("diag_sq_mfma", -1)
        e["rows_over_mfma"] = e["rows_diag_cross_ms"] / e["mfma_diag_cross_ms"]
        out[str(ns)] = e
    return dict(khat=kh, rows=out)


def run_config(cfg, m, n, reps):
    import scipy.sparse as sp

    import loraine_jl_amd

    rng = np.random.default_rng(0)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    W = G @ G.T
    ident = np.arange(n, dtype=np.int64)[:, None]
    dev = loraine_jl_amd.Device(0)
    dev.set_option("profile", 1)
    dev.set_option("lowrank_wide", 1)
    dev.set_option("wide_diag", 1)
    nwide = min(10, n)
    trace = cfg in ("b", "b0")
    if cfg in ("a", "a0", "b", "b0"):
        ranks = np.ones(n, dtype=np.int64)
        ranks[:nwide] = 40
        if trace:
            ranks[nwide] = 0
        rows = list(range(nwide)) + ([nwide] if trace else [])
    else:
        kh = 32 if cfg == "c" else 64
        ranks = np.full(n, kh, dtype=np.int64)
        rows = list(range(n))
    nl = int(ranks.sum())
    V = rng.standard_normal((m, nl)) / np.sqrt(m)
    d = rng.choice([-1.0, 1.0], size=nl)
    Ad = rng.standard_normal((m, len(rows)))
    if trace:
        Ad[:, -1] = 1.0
    e = dict(config=cfg, msz=m, nvar=n, reps=reps, diag_rows=len(rows))
    if cfg in ("a", "b", "c", "d64"):
        kh = 32 if ranks.max() <= 32 else 64
        dev.upload_model([sp.csr_matrix((n, m * m))], ident, np.zeros((2, 1), dtype=np.int64), np.array([m], dtype=np.int64))
        upload_factors(dev, m, n, kh, ranks, V, d)
        dev.set_factored(0)
        dev.set_scaling(0, W, G)
        e["khat"] = kh
        if cfg != "d64":
            dev.upload_diag(0, rows, Ad)
            e.update(both_layouts(dev, reps))
            assert dev.count("schur_wide") > 0 and dev.count("schur_diag") > 0 and dev.count("diag_rows") == len(rows)
            e["device_bytes"], e["device_bytes_peak"] = dev.count("device_bytes"), dev.count("device_bytes_peak")
            if cfg in ("a", "b"):
                e["H_fro"] = float(np.linalg.norm(dev.schur_assemble(1, want_H=True)))
        if cfg in ("c", "d64"):
            e["diag_sq_sweep"] = sweep(dev, m, n, kh, reps, rng)
    else:
        # the form before wide_diag: the ten constraints V D V' + diag(a) as stored dense matrices (positions 0 .. 9, dense slots),
        # the trace row as a stored sparse identity, every other constraint at khat 1
        c0 = np.concatenate([[0], np.cumsum(ranks)])
        rr, cc, vv = [], [], []
        for k in range(nwide):
            Vk = V[:, c0[k]:c0[k + 1]]
            A = (Vk * d[c0[k]:c0[k + 1]]) @ Vk.T
            A = 0.5 * (A + A.T) + np.diag(Ad[:, k])
            rr.append(np.full(m * m, k, dtype=np.int64))
            cc.append(np.arange(m * m, dtype=np.int64))
            vv.append(-A.ravel())
        nst = nwide
        if trace:
            rr.append(np.full(m, nwide, dtype=np.int64))
            cc.append(np.arange(m, dtype=np.int64) * (m + 1))
            vv.append(-np.ones(m))
            nst += 1
        AA = sp.csr_matrix((np.concatenate(vv), (np.concatenate(rr), np.concatenate(cc))), shape=(n, m * m))
        del rr, cc, vv
        r1 = ranks.copy()
        r1[:nwide] = 0
        dev.set_option("dense_threshold", float(m * m))      # (full matrices: dense slots)
        dev.upload_model([AA], ident, np.full((2, 1), nst, dtype=np.int64), np.array([m], dtype=np.int64))
        dev.set_option("dense_threshold", -1.0)
        upload_factors(dev, m, n, 1, r1, V[:, c0[nwide]:], d[c0[nwide]:])
        dev.set_factored(0)
        dev.set_scaling(0, W, G)
        e["khat"] = 1
        e.update(both_layouts(dev, reps))
        assert dev.count("adense_bytes") == nwide * m * m * 8 and dev.count("schur_diag") == 0
        e["device_bytes"], e["device_bytes_peak"] = dev.count("device_bytes"), dev.count("device_bytes_peak")
        e["adense_bytes"] = dev.count("adense_bytes")
        e["H_fro"] = float(np.linalg.norm(dev.schur_assemble(1, want_H=True)))
    dev.close()
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msz", type=int, default=2000)
    ap.add_argument("--nvar", type=int, default=4000)
    ap.add_argument("--configs", type=str, default=",".join(CONFIGS))
    ap.add_argument("--config", type=str, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.config:
        print("RESULT " + json.dumps(run_config(a.config, a.msz, a.nvar, a.reps)), flush=True)
        return
    rec = dict(msz=a.msz, nvar=a.nvar, reps=a.reps, configs={})

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(rec, f, indent=1)

    for cfg in a.configs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--config", cfg, "--msz", str(a.msz), "--nvar", str(a.nvar),
               "--reps", str(a.reps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[cfg])
        except subprocess.TimeoutExpired:
            rec["configs"][cfg] = dict(failed="time limit of %d s" % LIMITS[cfg])
            save()
            print("%s: time limit -- nothing more is started" % cfg, flush=True)
            sys.exit(1)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            rec["configs"][cfg] = dict(failed="exit status %d" % p.returncode, stderr=p.stderr[-2000:])
            save()
            print("%s: exit status %d\n%s" % (cfg, p.returncode, p.stderr[-2000:]), flush=True)
            if p.returncode < 0 or p.returncode in (124, 134, 137, 139):      # a signal: nothing more is started on the GPU
                sys.exit(1)
            continue
        rec["configs"][cfg] = json.loads(line[0][len("RESULT "):])
        print(cfg, json.dumps(rec["configs"][cfg]), flush=True)
        save()
    c = rec["configs"]
    for x, x0 in (("a", "a0"), ("b", "b0")):
        if "padded" in c.get(x, {}) and "padded" in c.get(x0, {}):
            c[x]["baseline_over_this_assemble"] = {k: c[x0][k]["assemble_ms"] / c[x][k]["assemble_ms"] for k in ("padded", "ragged_all")}
            c[x]["baseline_over_this_device_bytes"] = c[x0]["device_bytes"] / c[x]["device_bytes"]
            c[x]["H_fro_rel_diff"] = abs(c[x]["H_fro"] - c[x0]["H_fro"]) / c[x0]["H_fro"]
    save()


if __name__ == "__main__":
    main()
