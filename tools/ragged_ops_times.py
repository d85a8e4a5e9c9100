"""Times of the two data operators of a factored block of MIXED ranks at msz 2000 / nvar 4000: the padded layout (library option
ragged_ops = 0, every constraint on khat columns) against the compacted columns of the rank classes (1, csrc/raggedops.hip), in
one process on the same uploaded factors -- the shapes of tools/ragged_times.py:
    a  all rank 1                       (option 1 falls back: the reference point)
    b  3999 x rank 1, one rank 9        (khat 16: the motivating shape)
    c  half rank 1, half rank 2
    d  ranks uniform in 1 .. 16
AA vec(X), both products of lrn_ip_rhs_pred2 and mat(AA' y) through the resident entry points, each timed by itself with device
events inside the library (option "profile_ops": keys "aa_times", "aa_times2", "aat_to_mat"); one lrn_matvec under cg_factored
= 1, matvec_h = 1 in its four forms fac_op_scaled x fac_quadform (key "matvec" of option "profile"; Y = W V of the scaled form
is built by the warm-up call).  Median of --reps runs after a warm-up.  Under option 1 the K-split of the syrk is swept
(ragged_ops_split = 1, 2, 4, 8, 16; 0 = the auto rule, whose choice "ragged_ops_chunks" is recorded).  A context per shape,
option 1 first: device_bytes_peak after the option-1 passes and after the padded ones.

    python tools/ragged_ops_times.py --out profiles/ragged_ops_times.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
FORMS = [(0, 0), (0, 1), (1, 0), (1, 1)]       # (fac_op_scaled, fac_quadform)
SPLITS = [1, 2, 4, 8, 16]


def _median(dev, key, call, reps, by_count=True):
    call()                                            # warm-up (plan, dense copies, workspaces, Y of the scaled form)
    ts = []
    for _ in range(reps):
        dev.set_option("reset_timing", 1)
        call()
        ts.append(dev.timing(key) / (max(1, dev.count(key)) if by_count else 1))
    return dict(ms=float(np.median(ts)), runs_ms=ts)


def _passes(dev, n, reps, y, x):
    out = {}
    dev.set_option("profile_ops", 1)
    for key, call in (("aa_times", dev.ip_aa_x), ("aa_times2", dev.ip_rhs_pred2), ("aat_to_mat", lambda: dev.ip_residual_d(y))):
        out[key] = _median(dev, key, call, reps)
    dev.set_option("profile_ops", 0)
    dev.set_option("cg_factored", 1)
    dev.set_option("matvec_h", 1)
    for scaled, quad in FORMS:
        dev.set_option("fac_op_scaled", scaled)
        dev.set_option("fac_quadform", quad)
        out["matvec_scaled%d_fused%d" % (scaled, quad)] = _median(dev, "matvec", lambda: dev.matvec(x), reps, by_count=False)
    dev.set_option("fac_op_scaled", -1)
    dev.set_option("fac_quadform", -1)
    dev.set_option("matvec_h", 0)
    dev.set_option("cg_factored", 0)
    return out


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
    from ragged_times import shape_ranks

    m, n = a.msz, a.nvar
    rng = np.random.default_rng(0)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    W = G @ G.T
    R0 = rng.standard_normal((m, m))
    X = 0.5 * (R0 + R0.T)
    y, x = rng.standard_normal(n), rng.standard_normal(n)
    rec = dict(msz=m, nvar=n, reps=a.reps, shapes={})
    for shape in a.shapes.split(","):
        ranks = shape_ranks(shape, n, rng)
        kh = padded_rank(int(ranks.max()))
        R = n * kh
        plan = ragged_plan(ranks.tolist())
        dev = loraine_jl_amd.Device(0)
        dev.upload_model([sp.csr_matrix((n, m * m))], np.arange(n, dtype=np.int64)[:, None], np.zeros((2, 1), dtype=np.int64),
                         np.array([m], dtype=np.int64))
        live = (np.arange(kh)[None, :] < ranks[:, None]).ravel()
        cp = (np.arange(m + 1, dtype=np.int64) * R + 1)
        rv = np.tile(np.arange(1, R + 1, dtype=np.int64), m)
        nz = (rng.standard_normal((m, R)) / np.sqrt(m) * live[None, :]).ravel()
        d = rng.choice([-1.0, 1.0], size=R) * live
        dev._chk(dev.lib.lrn_upload_lowrank(dev.h, 0, kh, ptr(cp), ptr(rv), ptr(nz), ptr(d)), "lrn_upload_lowrank")
        del rv, nz
        dev.set_factored(0)
        dev.set_scaling(0, W, G)
        dev.ip_set_c(0, np.zeros((m, m)))
        dev.ip_set_iterate(0, X, np.eye(m))
        dev.set_option("profile", 1)
        e = dict(khat=kh, R=R, Rc=plan["Rc"], column_ratio=R / max(1, plan["Rc"]))
        for opt in (1, 0):
            dev.set_option("ragged_ops", opt)
            dev.set_option("reset_timing", 1)
            p = _passes(dev, n, a.reps, y, x)
            p["route"] = "ragged" if dev.count("op_ragged") > 0 else "padded"
            p["device_bytes_peak"] = dev.count("device_bytes_peak")
            if opt == 1 and p["route"] == "ragged":
                p["auto_chunks"] = dev.count("ragged_ops_chunks")
                dev.set_option("profile_ops", 1)
                sweep = {}
                for ks in SPLITS:
                    dev.set_option("ragged_ops_split", ks)
                    t = _median(dev, "aat_to_mat", lambda: dev.ip_residual_d(y), a.reps)
                    t["chunks"] = dev.count("ragged_ops_chunks")
                    sweep[str(ks)] = t
                dev.set_option("ragged_ops_split", 0)
                dev.set_option("profile_ops", 0)
                p["split_sweep"] = sweep
            e["option%d" % opt] = p
        dev.set_option("ragged_ops", 0)
        e["padded_over_ragged"] = {k: e["option0"][k]["ms"] / e["option1"][k]["ms"] for k in e["option0"]
                                   if isinstance(e["option0"][k], dict) and "ms" in e["option0"][k]}
        rec["shapes"][shape] = e
        print(json.dumps(e), flush=True)
        dev.close()
    if "a" in rec["shapes"]:      # every option-1 time over the padded time of the all-rank-1 shape
        base = rec["shapes"]["a"]["option0"]
        for shape, e in rec["shapes"].items():
            e["ragged_over_shape_a_padded"] = {k: e["option1"][k]["ms"] / base[k]["ms"] for k in base
                                               if isinstance(base[k], dict) and "ms" in base[k]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
