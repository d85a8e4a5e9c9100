"""Times of the data operators in factor form (factored blocks, lrn_set_factored) at msz 2000 / nvar 4000, beside the
passes over dense constraint data of the same shape, in one process on one device.

    dense:     lrn_synthetic_dense_model (128 GB of constraint matrices in HBM); AA vec(X) through lrn_ip_aa_x, both
               products of lrn_ip_rhs_pred2 and mat(AA'y) through lrn_ip_residual_d
    factored:  an AA without entries + random dense factors with khat in {1, 2, 4, 8, 16}; the same three entry points

Every operator is timed by itself with device events inside the library (option "profile_ops": keys "aa_times",
"aa_times2", "aat_to_mat"), median of --reps runs after a warm-up.  Useful flop: 2 msz^2 R per product Q = Z Vd
(R = nvar khat; aa_times2 does two), msz^2 R for the lower triangle of Vs Vd'.  --solve adds the full-size planted solve
(synthetic.FactoredLowRankProblem, rank 2) with ms per IP iteration (mean over iterations 2 .. end) and its phases.

    python tools/factored_pass_times.py --out profiles/factored_pass_times.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 78.6


def _passes(dev, n, reps, rng):
    """median ms of (aa_times, aa_times2, aat_to_mat) through the resident entry points."""
    y = rng.standard_normal(n)
    out = {}
    for key, call in (("aa_times", dev.ip_aa_x), ("aat_to_mat", lambda: dev.ip_residual_d(y)),
                      ("aa_times2", dev.ip_rhs_pred2)):
        call()                                            # warm-up (workspaces)
        ts = []
        for _ in range(reps):
            dev.set_option("reset_timing", 1)
            call()
            ts.append(dev.timing(key) / max(1, dev.count(key)))
        out[key] = dict(ms=float(np.median(ts)), runs_ms=ts)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msz", type=int, default=2000)
    ap.add_argument("--nvar", type=int, default=4000)
    ap.add_argument("--khat", type=str, default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import loraine_jl_amd
    from loraine_jl_amd._capi import ptr

    m, n = a.msz, a.nvar
    dev = loraine_jl_amd.Device(0)
    rng = np.random.default_rng(0)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    W = G @ G.T
    R0 = rng.standard_normal((m, m))
    X = 0.5 * (R0 + R0.T)
    rec = dict(msz=m, nvar=n, peak_tflops=PEAK_TF, factored={})

    def prepare():
        dev.set_scaling(0, W, G)
        dev.ip_set_c(0, np.zeros((m, m)))
        dev.ip_set_iterate(0, X, np.eye(m))
        dev.set_option("profile_ops", 1)

    if not a.no_dense:
        dev.synthetic_dense_model(m, n, 7)
        prepare()
        rec["dense"] = _passes(dev, n, a.reps, rng)
        print(json.dumps(dict(dense=rec["dense"])), flush=True)
    # the factored model of the same shape: an AA without entries (this also frees the dense data)
    empty = sp.csr_matrix((n, m * m))
    sig = np.arange(n, dtype=np.int64).reshape(n, 1)
    for kh in [int(x) for x in a.khat.split(",")]:
        R = n * kh
        dev.set_option("profile_ops", 0)
        dev.upload_model([empty], sig, np.zeros((2, 1), dtype=np.int64), [m])
        cp = (np.arange(m + 1, dtype=np.int64) * R + 1)
        rv = np.tile(np.arange(1, R + 1, dtype=np.int64), m)
        nz = rng.standard_normal(R * m) / np.sqrt(m)
        d = rng.choice([-1.0, 1.0], size=R)
        dev._chk(dev.lib.lrn_upload_lowrank(dev.h, 0, kh, ptr(cp), ptr(rv), ptr(nz), ptr(d)), "lrn_upload_lowrank")
        del rv, nz
        dev.set_factored(0)
        prepare()
        e = _passes(dev, n, a.reps, rng)
        flop = dict(aa_times=2.0 * m * m * R, aa_times2=4.0 * m * m * R, aat_to_mat=1.0 * m * m * R)
        for key, f in flop.items():
            e[key]["flop"] = f
            e[key]["tflops"] = f / e[key]["ms"] * 1e-9
            e[key]["frac_peak"] = e[key]["tflops"] / PEAK_TF
            if "dense" in rec:
                e[key]["dense_over_factored"] = rec["dense"][key]["ms"] / e[key]["ms"]
        e.update(khat=kh, R=R, device_gb=dev.count("device_bytes") / 1e9)
        rec["factored"][f"khat{kh}"] = e
        print(json.dumps(e), flush=True)
    dev.set_option("profile_ops", 0)
    if a.solve:
        from loraine_jl_amd import solvers
        from loraine_jl_amd.optimizer import Optimizer
        from loraine_jl_amd.synthetic import FactoredLowRankProblem
        t0 = time.perf_counter()
        P = FactoredLowRankProblem(m, n, 2, 4)
        o = Optimizer(device=dev)
        o.set_silent(True)
        o.set_attribute("kit", 0)
        o.load_factored_model(P.F0(), P.factors(), P.b, max_sense=True)
        o._copy_to()
        t1 = time.perf_counter()
        solvers.solve(o.solver, o.halpha)
        s = o.solver
        tr = s.trace[1:] if len(s.trace) > 1 else s.trace
        mean = lambda f: float(np.mean([f(t) for t in tr]))
        rec["solve"] = dict(
            status=o.termination_status(), iterations=s.iter, objective=o.objective_value(), planted=P.optimum,
            rel_gap=abs(o.objective_value() - P.optimum) / (1 + abs(P.optimum)), dimacs=s.DIMACS_error,
            setup_s=t1 - t0, solve_s=s.tottime, ms_per_iteration=1e3 * mean(lambda t: t["itertime"]),
            phases_ms={k: mean(lambda t, k=k: t["gpu_ms"][k]) for k in ("prepare_w", "assemble", "factor", "solve")},
            rhs_ms=mean(lambda t: t["rhs_ms"]), residual_d_ms=mean(lambda t: t["residual_d_ms"]),
            find_step_ms=mean(lambda t: t["find_step_ms"]), stats_ms=mean(lambda t: t["stats_ms"]),
            device_gb_peak=dev.count("device_bytes_peak") / 1e9)
        print(json.dumps(rec["solve"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
