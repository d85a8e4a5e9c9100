"""Times of the mode-1 Schur assembly of a factored block with constraints of rank 17 .. 64 (library option lowrank_wide:
khat 32 / 64, the classes 64 and 32 of csrc/ragged_plan.h, the wide epilogue of csrc/raggedops.hip) at msz 2000 / nvar 4000, in
one process.

A factored block with random dense factors and a random SPD scaling W = G G'.  Timed with the library's device events (option
"profile") as the median of --reps runs after a warm-up: "lowrank_u" = U_c = G' Vc alone, "ragged" = U_c and the tile launch from
the same start, "assemble" = the whole lrn_schur_assemble.  Shapes:
    a  uniform rank 16, uploaded at khat 32 so that the block is wide and goes by class (Rc = 64 000 of R = 128 000): the tiles
       are those of class 16 alone, the narrow epilogue -- the rate baseline of the K loop
    b  uniform rank 32 (Rc = R = 128 000): every tile takes the wide epilogue
    c  3990 x rank 1 and 10 x rank 40 (khat 64, Rc = 4630 of R = 256 000) -- against the same model with the ten constraints as
       stored dense matrices in a hybrid block of khat 1 (what a model without `wide` can say), "assemble" of both, H compared
    d  ranks uniform in 1 .. 64
Useful flop of the tile launch: Rc^2 msz for the lower triangle of T on the compacted columns; the fraction of the 78.6 TFLOP/s
FP64 matrix peak is quoted for that count.  Every configuration runs in a context of its own: device_bytes / device_bytes_peak
are what that context holds after / held at most during its assemblies.

    python tools/wide_rank_times.py --out profiles/wide_rank_times.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 78.6
KEYS = ("lowrank_u", "ragged", "assemble", "hybrid_y", "hybrid_cross")


def shape_ranks(shape, n, rng):
    if shape == "a":
        return np.full(n, 16, dtype=np.int64)
    if shape == "b":
        return np.full(n, 32, dtype=np.int64)
    if shape == "c":
        r = np.ones(n, dtype=np.int64)
        r[:10] = 40
        return r
    if shape == "d":
        return rng.integers(1, 65, size=n)
    raise ValueError(shape)


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
    return {k: float(np.median(v)) for k, v in runs.items()}, runs["assemble"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msz", type=int, default=2000)
    ap.add_argument("--nvar", type=int, default=4000)
    ap.add_argument("--shapes", type=str, default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import scipy.sparse as sp

    import loraine_jl_amd
    from loraine_jl_amd.model import ragged_plan

    m, n = a.msz, a.nvar
    empty = [sp.csr_matrix((n, m * m))]
    ident = np.arange(n, dtype=np.int64)[:, None]
    rng = np.random.default_rng(0)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    W = G @ G.T

    def fresh():      # a context of its own per configuration: device_bytes is that configuration's
        dev = loraine_jl_amd.Device(0)
        dev.set_option("profile", 1)
        dev.set_option("lowrank_wide", 1)
        return dev

    rec = dict(msz=m, nvar=n, reps=a.reps, peak_tflops=PEAK_TF, shapes={})
    for shape in a.shapes.split(","):
        ranks = shape_ranks(shape, n, rng)
        kh = 32 if shape == "a" else (32 if ranks.max() <= 32 else 64)
        plan = ragged_plan(ranks.tolist(), max_rank=64)
        nl = int(ranks.sum())
        V = rng.standard_normal((m, nl)) / np.sqrt(m)
        d = rng.choice([-1.0, 1.0], size=nl)
        dev = fresh()
        dev.upload_model(empty, ident, np.zeros((2, 1), dtype=np.int64), np.array([m], dtype=np.int64))
        upload_factors(dev, m, n, kh, ranks, V, d)
        dev.set_factored(0)
        dev.set_scaling(0, W, G)
        t, runs = timed(dev, a.reps)
        assert dev.count("schur_wide") > 0 and dev.count("ragged_cols") == plan["Rc"]
        prod = t["ragged"] - t["lowrank_u"]
        e = dict(khat=kh, R=n * kh, Rc=plan["Rc"], classes=plan["ncls"], tiles=plan["tiles"], u_ms=t["lowrank_u"], t_ms=prod,
                 total_ms=t["ragged"], assemble_ms=t["assemble"], assemble_runs_ms=runs,
                 t_tflops=float(plan["Rc"]) ** 2 * m / prod * 1e-9,
                 t_frac_peak=float(plan["Rc"]) ** 2 * m / prod * 1e-9 / PEAK_TF,
                 device_bytes=dev.count("device_bytes"), device_bytes_peak=dev.count("device_bytes_peak"))
        if shape == "c":
            # the baseline: the ten rank-40 constraints as stored dense matrices (positions 0 .. 9, dense slots), the others at khat 1
            Hw = dev.schur_assemble(1, want_H=True)
            c0 = np.concatenate([[0], np.cumsum(ranks)])
            rr, vv = [], []
            for k in range(10):
                Vk = V[:, c0[k]:c0[k + 1]]
                A = (Vk * d[c0[k]:c0[k + 1]]) @ Vk.T
                rr.append(np.full(m * m, k, dtype=np.int64))
                vv.append(-(0.5 * (A + A.T)).ravel())
            AA = sp.csr_matrix((np.concatenate(vv), (np.concatenate(rr), np.tile(np.arange(m * m, dtype=np.int64), 10))),
                               shape=(n, m * m))
            del rr, vv
            r1 = ranks.copy()
            r1[:10] = 0
            dev.close()
            dev = fresh()
            dev.set_option("dense_threshold", float(m * m))      # (full matrices: dense slots)
            dev.upload_model([AA], ident, np.full((2, 1), 10, dtype=np.int64), np.array([m], dtype=np.int64))
            dev.set_option("dense_threshold", -1.0)
            upload_factors(dev, m, n, 1, r1, V[:, c0[10]:], d[c0[10]:])
            dev.set_factored(0)
            dev.set_scaling(0, W, G)
            tb, runs_b = timed(dev, a.reps)
            Hb = dev.schur_assemble(1, want_H=True)
            assert dev.count("adense_bytes") == 10 * m * m * 8
            e["hybrid_baseline"] = dict(khat=1, dense_slots=10, assemble_ms=tb["assemble"], assemble_runs_ms=runs_b,
                                        hybrid_y_ms=tb["hybrid_y"], hybrid_cross_ms=tb["hybrid_cross"],
                                        device_bytes=dev.count("device_bytes"), adense_bytes=dev.count("adense_bytes"))
            e["baseline_over_wide_assemble"] = tb["assemble"] / t["assemble"]
            e["wide_against_baseline_relerr"] = float(np.linalg.norm(Hw - Hb) / np.linalg.norm(Hb))
            del Hw, Hb, AA
        del V
        dev.close()
        rec["shapes"][shape] = e
        print(json.dumps(e), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
