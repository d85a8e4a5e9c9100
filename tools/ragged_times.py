"""Times of the mode-1 Schur assembly of a factored block of MIXED ranks at msz 2000 / nvar 4000: the padded route (library
option lowrank_ragged = 0, every constraint on khat columns) against the rank-class route (1, csrc/raggedops.hip), in one
process on the same uploaded factors.

A pure factored block (empty AA) with random dense factors and a random SPD scaling W = G G'.  Both routes are timed with the
library's device events (option "profile") as the median of --reps runs after a warm-up: "lowrank_u" = U = G' V alone on either
route, "lowrank" (padded) / "ragged" (rank classes) = U and the blocked product from the same start.  Shapes:
    a  all rank 1                       (the rank-class route falls back: the reference point)
    b  3999 x rank 1, one rank 9        (khat 16: the motivating shape)
    c  half rank 1, half rank 2
    d  ranks uniform in 1 .. 16
Useful flop of the blocked product: Rc^2 msz for the lower triangle of T on the compacted columns (what the rank-class route
computes up to its diagonal tiles); the fraction of the 78.6 TFLOP/s FP64 matrix peak is quoted for that count.

    python tools/ragged_times.py --out profiles/ragged_times.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 78.6


def shape_ranks(shape, n, rng):
    if shape == "a":
        return np.ones(n, dtype=np.int64)
    if shape == "b":
        r = np.ones(n, dtype=np.int64)
        r[n // 2] = 9
        return r
    if shape == "c":
        return np.where(np.arange(n) % 2 == 0, 1, 2).astype(np.int64)
    if shape == "d":
        return rng.integers(1, 17, size=n)
    raise ValueError(shape)


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
    from loraine_jl_amd._capi import ptr
    from loraine_jl_amd.model import padded_rank, ragged_plan

    m, n = a.msz, a.nvar
    dev = loraine_jl_amd.Device(0)
    dev.upload_model([sp.csr_matrix((n, m * m))], np.arange(n, dtype=np.int64)[:, None], np.zeros((2, 1), dtype=np.int64),
                     np.array([m], dtype=np.int64))
    rng = np.random.default_rng(0)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    W = G @ G.T
    dev.set_option("profile", 1)
    rec = dict(msz=m, nvar=n, reps=a.reps, peak_tflops=PEAK_TF, shapes={})
    for shape in a.shapes.split(","):
        ranks = shape_ranks(shape, n, rng)
        kh = padded_rank(int(ranks.max()))
        R = n * kh
        plan = ragged_plan(ranks.tolist())
        # dense factors in the upload's own CSC form (row k khat + p = column p of V_k); padding columns are zero, weight 0
        live = (np.arange(kh)[None, :] < ranks[:, None]).ravel()
        cp = (np.arange(m + 1, dtype=np.int64) * R + 1)
        rv = np.tile(np.arange(1, R + 1, dtype=np.int64), m)
        nz = (rng.standard_normal((m, R)) / np.sqrt(m) * live[None, :]).ravel()
        d = rng.choice([-1.0, 1.0], size=R) * live
        dev._chk(dev.lib.lrn_upload_lowrank(dev.h, 0, kh, ptr(cp), ptr(rv), ptr(nz), ptr(d)), "lrn_upload_lowrank")
        del rv, nz
        dev.set_factored(0)
        dev.set_scaling(0, W, G)
        e = dict(khat=kh, R=R, Rc=plan["Rc"], classes=plan["ncls"], tiles=plan["tiles"])
        for opt, key in ((0, "lowrank"), (1, "ragged")):
            dev.set_option("lowrank_ragged", opt)
            dev.schur_assemble(1)                        # warm-up (dense copies of V, the plan, workspaces)
            tu, tt, took = [], [], key
            for _ in range(a.reps):
                dev.set_option("reset_timing", 1)
                dev.schur_assemble(1)
                if opt == 1 and dev.count("schur_ragged") == 0:
                    took = "lowrank"                     # (the fallback of a uniform block)
                tu.append(dev.timing("lowrank_u"))
                tt.append(dev.timing(took))
            u_ms, all_ms = float(np.median(tu)), float(np.median(tt))
            cols = plan["Rc"] if took == "ragged" else R
            e["ragged" if opt else "padded"] = dict(route=took, u_ms=u_ms, t_ms=all_ms - u_ms, total_ms=all_ms, runs_ms=tt,
                                                    t_tflops=float(cols) * cols * m / (all_ms - u_ms) * 1e-9)
        dev.set_option("lowrank_ragged", 0)
        rg, pd = e["ragged"], e["padded"]
        e["padded_over_ragged_t"] = pd["t_ms"] / rg["t_ms"]
        e["padded_over_ragged_total"] = pd["total_ms"] / rg["total_ms"]
        # the useful work on either route is that of the compacted columns
        e["ragged_t_frac_peak"] = float(plan["Rc"]) ** 2 * m / rg["t_ms"] * 1e-9 / PEAK_TF
        rec["shapes"][shape] = e
        print(json.dumps(e), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
