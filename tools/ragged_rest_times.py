"""Times of what the library options ragged_cross and ragged_ts move to the compacted columns of a factored block of MIXED ranks
at msz 2000 / nvar 4000: Y = W V with the cross terms of the mode-1 assembly, and ts of H_alpha.  Options 1 then 0 on one upload
in one process; the rank-class assembly of H_FF (lowrank_ragged = 1) runs under both, so the difference is these two options
alone.  The shapes of tools/ragged_times.py:
    a  all rank 1     b  3999 x rank 1, one rank 9 (khat 16: the motivating shape)     c  half rank 1, half rank 2
    d  ranks uniform in 1 .. 16
each in three variants:
    trace   constraint 0 is the trace row (None, [], ones): no factor column, one diagonal row
    stored  constraints 0 .. 15 are sparse stored matrices (a diagonal and one off-diagonal band, 3 msz - 2 entries each)
    diag    every constraint carries a dense diagonal part beside its factors
Library events (option "profile"; "prec_ts_p" under option "profile_ops"), median of --reps runs after a warm-up:
"hybrid_y", "hybrid_cross", "diag_cross", "assemble" of lrn_schur_assemble(1); "prec_ts_p" and the whole "prec_setup" of
lrn_prec_setup(1, erank, 1) at erank 1 and 3 under cg_factored = 1, cg_diag = 1.  The scaling is set anew before every timed
assembly (Yc = W Vc is cached per scaling: a repeated assembly would not pay for it).  A context per variant, options 1 first:
device_bytes_peak after the option-1 passes and after the padded ones.

    python tools/ragged_rest_times.py --out profiles/ragged_rest_times.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ASSEMBLY_KEYS = ("hybrid_y", "hybrid_cross", "diag_cross", "assemble")
COUNTERS = ("schur_ragged", "schur_cross_ragged", "ragged_cross_fallback", "ragged_y_reused", "hybrid_cross_lds",
            "hybrid_cross_global", "hybrid_cross_dense", "diag_sq_rows", "diag_sq_mfma", "prec_ts_ragged", "ragged_ts_fallback")
NSTORED = 16


def _medians(dev, keys, call, reps, pre=None):
    call()                                            # warm-up (plan, dense copies, workspaces)
    runs = {k: [] for k in keys}
    for _ in range(reps):
        if pre:
            pre()
        dev.set_option("reset_timing", 1)
        call()
        for k in keys:
            runs[k].append(dev.timing(k))
    return {k: dict(ms=float(np.median(v)), runs_ms=v) for k, v in runs.items()}


def _stored_rows(m, n, rng):
    """AA (n x m^2, rows 0 .. NSTORED - 1 = -vec(A_s)) of NSTORED symmetric matrices: a diagonal and one band at distance s + 1."""
    import scipy.sparse as sp
    rows, cols, vals = [], [], []
    for s in range(NSTORED):
        i = np.arange(m)
        j = np.arange(m - s - 1)
        r = np.concatenate([i, j, j + s + 1])
        c = np.concatenate([i, j + s + 1, j])
        off = rng.standard_normal(m - s - 1)
        v = np.concatenate([rng.standard_normal(m), off, off])
        rows.append(np.full(r.size, s))
        cols.append(r + c * m)
        vals.append(-v)
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, m * m))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msz", type=int, default=2000)
    ap.add_argument("--nvar", type=int, default=4000)
    ap.add_argument("--shapes", type=str, default="a,b,c,d")
    ap.add_argument("--variants", type=str, default="trace,stored,diag")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import scipy.sparse as sp

    import loraine_jl_amd
    from loraine_jl_amd._capi import ptr
    from loraine_jl_amd.model import padded_rank, ragged_plan
    from ragged_times import shape_ranks

    m, n = a.msz, a.nvar
    rng = np.random.default_rng(0)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    W = G @ G.T
    rec = dict(msz=m, nvar=n, reps=a.reps, lowrank_ragged=1, shapes={})
    if a.out and os.path.exists(a.out):               # (shapes measured by an earlier call are kept)
        with open(a.out) as f:
            rec["shapes"] = json.load(f).get("shapes", {})
    for shape in a.shapes.split(","):
        base = shape_ranks(shape, n, rng)
        kh = padded_rank(int(base.max()))
        R = n * kh
        cp = (np.arange(m + 1, dtype=np.int64) * R + 1)
        rv = np.tile(np.arange(1, R + 1, dtype=np.int64), m)
        nz0 = rng.standard_normal((m, R)) / np.sqrt(m)
        sign = rng.choice([-1.0, 1.0], size=R)
        rec["shapes"].setdefault(shape, {})
        for variant in a.variants.split(","):
            ranks = base.copy()
            if variant == "trace":
                ranks[0] = 0
            elif variant == "stored":
                ranks[:NSTORED] = 0
            plan = ragged_plan(ranks.tolist())
            live = (np.arange(kh)[None, :] < ranks[:, None]).ravel()
            AA = _stored_rows(m, n, rng) if variant == "stored" else sp.csr_matrix((n, m * m))
            q = NSTORED if variant == "stored" else 0
            dev = loraine_jl_amd.Device(0)
            dev.upload_model([AA], np.arange(n, dtype=np.int64)[:, None], np.full((2, 1), q, dtype=np.int64),
                             np.array([m], dtype=np.int64))
            nz = (nz0 * live[None, :]).ravel()
            d = sign * live
            dev._chk(dev.lib.lrn_upload_lowrank(dev.h, 0, kh, ptr(cp), ptr(rv), ptr(nz), ptr(d)), "lrn_upload_lowrank")
            del nz
            dev.set_factored(0)
            if variant == "trace":
                dev.upload_diag(0, [0], np.ones((m, 1)))
            elif variant == "diag":
                dev.upload_diag(0, np.arange(n), rng.standard_normal((m, n)) / np.sqrt(m))
            dev.set_scaling(0, W, G)
            for k, v in dict(profile=1, lowrank_ragged=1, cg_factored=1, cg_diag=1).items():
                dev.set_option(k, v)
            e = dict(khat=kh, R=R, Rc=plan["Rc"], column_ratio=R / max(1, plan["Rc"]))
            for opt in (1, 0):
                dev.set_option("ragged_cross", opt)
                dev.set_option("ragged_ts", opt)
                dev.set_option("reset_timing", 1)
                # (a new scaling before every timed assembly, as in a solve: Yc = W Vc is cached per scaling and would cost nothing)
                p = _medians(dev, ASSEMBLY_KEYS, lambda: dev.schur_assemble(1), a.reps, pre=lambda: dev.set_scaling(0, W, G))
                dev.set_option("profile_ops", 1)
                for erank in (1, 3):
                    t = _medians(dev, ("prec_ts_p", "prec_setup"), lambda: dev.prec_setup(1, erank, 1), a.reps)
                    p["prec_ts_p_erank%d" % erank] = t["prec_ts_p"]
                    p["prec_setup_erank%d" % erank] = t["prec_setup"]
                dev.set_option("profile_ops", 0)
                dev.set_option("reset_timing", 1)
                dev.schur_assemble(1)
                dev.prec_setup(1, 1, 1)
                p["counters"] = {k: dev.count(k) for k in COUNTERS}
                p["device_bytes_peak"] = dev.count("device_bytes_peak")
                e["option%d" % opt] = p
            e["padded_over_compacted"] = {k: e["option0"][k]["ms"] / max(e["option1"][k]["ms"], 1e-9) for k in e["option0"]
                                          if isinstance(e["option0"][k], dict) and "ms" in e["option0"][k]}
            rec["shapes"][shape][variant] = e
            print(json.dumps({shape + "/" + variant: e}), flush=True)
            dev.close()
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
