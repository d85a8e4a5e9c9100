"""Times of the mode-1 Schur assembly and of the two data operators of a factored block with diagonal parts,
A_k = diag(a_k) + V_k D_k V_k', at msz 2000 / nvar 4000 / khat 2 (dense random factors, random signs), in one process:

  * the trace row tr X given as a STORED identity (the hybrid route, H_SS under "sparse") and as a diagonal part (None, [], ones);
  * 1 / 16 / 64 / nvar constraints with a dense random diagonal part, under both forms of the squared-operand product
    (option "diag_sq_mfma" = 0 rows form, 1 MFMA form) -- the crossover between the forms is read off this table;
  * the pure block (no diagonal part) as the yardstick, and the two data operators beside it.

Method of tools/hybrid_assembly_times.py: device events of option "profile" ("assemble", "lowrank", "hybrid_y", "hybrid_cross",
"sparse", "diag_dd", "diag_cross", "diag_stored"), median of --reps runs after a warm-up assembly; the operators under
"profile_ops".

    python tools/diag_factored_times.py --out profiles/diag_factored_times.json
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("assemble", "lowrank", "hybrid_y", "hybrid_cross", "sparse", "diag_dd", "diag_cross", "diag_stored")


def _load(dev, model):
    dev.upload_model(model.AA, model.sigmaA, model.qA, model.msizes)
    Vp, dp, khat = model.lowrank[0]
    dev.upload_lowrank(0, khat, Vp, dp)
    dev.set_factored(0)
    if model.diag[0]:
        rows = sorted(model.diag[0])
        dev.upload_diag(0, rows, np.column_stack([model.diag[0][k] for k in rows]))


def _assembly(dev, W, G, reps):
    out = {}
    for label, Gs in (("G", G), ("W_only", None)):
        dev.set_scaling(0, W, Gs)
        dev.schur_assemble(1)                            # warm-up: workspaces
        runs = {k: [] for k in KEYS}
        for _ in range(reps):
            dev.reset_timing()
            dev.schur_assemble(1)
            for k in KEYS:
                runs[k].append(dev.timing(k))
        out[label] = {k + "_ms": float(np.median(v)) for k, v in runs.items()}
        out[label]["assemble_runs_ms"] = runs["assemble"]
    return out


def _operators(dev, X, y, reps):
    m = X.shape[0]
    dev.set_option("profile_ops", 1)
    dev.ip_set_c(0, np.zeros((m, m)))
    dev.ip_set_iterate(0, X, np.zeros((m, m)))
    dev.ip_aa_x()
    dev.ip_residual_d(y)                                 # warm-up
    ta, tm = [], []
    for _ in range(reps):
        dev.reset_timing()
        dev.ip_aa_x()
        dev.ip_residual_d(y)
        ta.append(dev.timing("aa_times"))
        tm.append(dev.timing("aat_to_mat"))
    dev.set_option("profile_ops", 0)
    return dict(aa_times_ms=float(np.median(ta)), aat_to_mat_ms=float(np.median(tm)), aa_times_runs_ms=ta, aat_to_mat_runs_ms=tm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msz", type=int, default=2000)
    ap.add_argument("--nvar", type=int, default=4000)
    ap.add_argument("--khat", type=int, default=2)
    ap.add_argument("--rows", type=str, default="1,16,64,-1", help="numbers of diagonal rows (-1: every constraint)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import loraine_jl_amd
    from loraine_jl_amd.model import build_factored_model

    m, n, kh = a.msz, a.nvar, a.khat
    rng = np.random.default_rng(0)
    V = rng.standard_normal((n, m, kh)) / np.sqrt(m)
    d = rng.choice([-1.0, 1.0], size=(n, kh))
    Ad = rng.standard_normal((n, m)) / np.sqrt(m)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    W = G @ G.T
    X = rng.standard_normal((m, m))
    X = 0.5 * (X + X.T)
    y = rng.standard_normal(n)
    dev = loraine_jl_amd.Device(0)
    dev.set_option("profile", 1)
    rec = dict(msz=m, nvar=n, khat=kh, reps=a.reps, cases={})
    F0 = [-np.eye(m)]

    def run(name, items, forms=(-1,)):
        model = build_factored_model(F0, [items], np.zeros(n), factored_form=1)
        _load(dev, model)
        e = dict(diag_rows=len(model.diag[0]), stored_nnz=int(model.AA[0].nnz))
        for form in forms:
            dev.set_option("diag_sq_mfma", form)
            key = {-1: "auto", 0: "rows_form", 1: "mfma_form"}[form]
            e[key] = _assembly(dev, W, G, a.reps)
        dev.set_option("diag_sq_mfma", -1)
        e.update(_operators(dev, X, y, a.reps))
        rec["cases"][name] = e
        print(name, json.dumps(e), flush=True)

    pure = [(V[k], d[k]) for k in range(n)]
    run("pure", pure)
    run("trace_stored_identity", [sp.identity(m, format="csc")] + pure[1:])
    run("trace_diagonal_part", [(None, [], np.ones(m))] + pure[1:], forms=(0, 1))
    for nr in [int(x) for x in a.rows.split(",")]:
        nr = n if nr < 0 else nr
        pick = set(np.linspace(0, n - 1, nr).astype(int).tolist())
        items = [(V[k], d[k], Ad[k]) if k in pick else (V[k], d[k]) for k in range(n)]
        run(f"sum_rows{nr}", items, forms=(0, 1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
