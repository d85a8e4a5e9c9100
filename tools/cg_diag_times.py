"""Times of the CG path (kit = 1) on a factored block WITH DIAGONAL PARTS (library options cg_factored = 1 and cg_diag = 1),
A_k = diag(a_k) + V_k D_k V_k', at msz 2000 / nvar 4000 / khat 2 (dense random factors, random signs), in one process.

Cases (the data of tools/diag_factored_times.py):
  pure                  no diagonal part: the yardstick (cg_diag has nothing to do)
  trace_diagonal_part   constraint 0 is the trace row (None, [], ones)
  sum_rows4000          every constraint carries a dense random diagonal part beside its rank-2 factors

Per case, median of --reps runs after a warm-up, device events of the library (option "profile"):
  prec_setup_erank{1,3}_ms     lrn_prec_setup of H_alpha (the whole call)
  ts_diag_erank{1,3}_ms        ts_diag_mfma_kernel alone, and ts_p_erank{1,3}_ms: the product P = L' Vd of the same setup (option
                               profile_ops, a run of its own: the two keys synchronise)
  operator_ms                  one application of the matrix-free operator (lrn_matvec under matvec_h = 1, the composition)
  assemble_ms, h_operator_ms   H in mode 1 (a fresh scaling per run) and one y = H x (matvec_h = 2)

    python tools/cg_diag_times.py --out profiles/cg_diag_times.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(dev, keys, run, reps):
    run()                                                    # warm-up: workspaces
    out = {k: [] for k in keys}
    for _ in range(reps):
        dev.set_option("reset_timing", 1)
        run()
        for k in keys:
            out[k].append(dev.timing(k))
    return {k: (float(np.median(v)), v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msz", type=int, default=2000)
    ap.add_argument("--nvar", type=int, default=4000)
    ap.add_argument("--khat", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import loraine_jl_amd
    from loraine_jl_amd.model import build_factored_model

    m, n, kh = a.msz, a.nvar, a.khat
    rng = np.random.default_rng(0)
    V = rng.standard_normal((n, m, kh)) / np.sqrt(m)
    d = rng.choice([-1.0, 1.0], size=(n, kh))
    Ad = rng.standard_normal((n, m)) / np.sqrt(m)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    W = G @ G.T
    x = rng.standard_normal(n)
    dev = loraine_jl_amd.Device(0)
    dev.set_option("profile", 1)
    rec = dict(msz=m, nvar=n, khat=kh, reps=a.reps, cases={})
    F0 = [-np.eye(m)]
    pure = [(V[k], d[k]) for k in range(n)]
    cases = [("pure", pure), ("trace_diagonal_part", [(None, [], np.ones(m))] + pure[1:]),
             ("sum_rows%d" % n, [(V[k], d[k], Ad[k]) for k in range(n)])]
    for name, items in cases:
        model = build_factored_model(F0, [items], np.zeros(n), factored_form=1)
        dev.upload_model(model.AA, model.sigmaA, model.qA, model.msizes)
        Vp, dp, khat = model.lowrank[0]
        dev.upload_lowrank(0, khat, Vp, dp)
        dev.set_factored(0)
        if model.diag[0]:
            rows = sorted(model.diag[0])
            dev.upload_diag(0, rows, np.column_stack([model.diag[0][k] for k in rows]))
        r = dict(diag_rows=len(model.diag[0]))
        dev.set_option("cg_factored", 1)
        dev.set_option("cg_diag", 1)
        dev.set_scaling(0, W, G)
        dev.set_option("matvec_h", 1)
        dev.set_option("fac_op_scaled", 0)
        dev.set_option("fac_quadform", 0)
        t = median_ms(dev, ["matvec"], lambda: dev.matvec(x), a.reps)
        r["operator_ms"], r["operator_runs"] = t["matvec"]

        def assemble():
            dev.set_scaling(0, W, G)                         # (a new scaling: H is assembled again)
            dev.matvec(x)
        dev.set_option("matvec_h", 2)
        t = median_ms(dev, ["assemble"], assemble, a.reps)
        r["assemble_ms"], r["assemble_runs"] = t["assemble"]
        t = median_ms(dev, ["matvec"], lambda: dev.matvec(x), a.reps)
        r["h_operator_ms"], r["h_operator_runs"] = t["matvec"]
        dev.set_option("matvec_h", 1)
        for erank in (1, 3):
            t = median_ms(dev, ["prec_setup"], lambda: dev.prec_setup(1, erank, 1), a.reps)
            r["prec_setup_erank%d_ms" % erank], r["prec_setup_erank%d_runs" % erank] = t["prec_setup"]
            r["prec_ts_diag_rows"] = dev.count("prec_ts_diag_rows")
            dev.set_option("profile_ops", 1)
            t = median_ms(dev, ["prec_ts_p", "prec_ts_diag"], lambda: dev.prec_setup(1, erank, 1), a.reps)
            dev.set_option("profile_ops", 0)
            r["ts_p_erank%d_ms" % erank], r["ts_p_erank%d_runs" % erank] = t["prec_ts_p"]
            r["ts_diag_erank%d_ms" % erank], r["ts_diag_erank%d_runs" % erank] = t["prec_ts_diag"]
        for k, v in dict(matvec_h=0, fac_op_scaled=-1, fac_quadform=-1, cg_diag=0, cg_factored=0).items():
            dev.set_option(k, v)
        rec["cases"][name] = r
        print(name, json.dumps(r), flush=True)
        if a.out:                                            # (after every case: a later one may not fit the time)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(rec, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
