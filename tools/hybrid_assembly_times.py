"""Times of the mode-1 Schur assembly and of the two data operators of a hybrid factored block at msz 2000 / nvar 4000 /
khat 2: dense random factors (random signs) with 0, 1, 4 and 16 of the constraints replaced by stored sparse matrices --
alternately the identity and a symmetric matrix of 9 entries (a 3 x 3 principal block).  0 stored is the pure factored
block, the yardstick against the commit before the hybrid path (which can run that case only: --stored 0).

Per case, after one warm-up assembly, the median of --reps runs of the device-event times (option "profile"):
"assemble" (all of mode 1), "lowrank" (U and the blocked product, H_FF), "hybrid_y" (Y = W Vd, zero when only W exists and
U already is Y), "hybrid_cross" (the cross kernel), "sparse" (H_SS over the stored rows); with G given and with W only.
The data operators (option "profile_ops"): one AA vec(X) and one mat(AA' y) through the resident entry points, median too.

    python tools/hybrid_assembly_times.py --out profiles/hybrid_assembly_times.json
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stored(m, t, rng):
    if t % 2 == 0:
        return sp.identity(m, format="csc")
    ii = rng.choice(m, size=3, replace=False)
    B = rng.standard_normal((3, 3))
    B = 0.5 * (B + B.T)
    return sp.csc_matrix((B.ravel(), (np.repeat(ii, 3), np.tile(ii, 3))), shape=(m, m))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msz", type=int, default=2000)
    ap.add_argument("--nvar", type=int, default=4000)
    ap.add_argument("--khat", type=int, default=2)
    ap.add_argument("--stored", type=str, default="0,1,4,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--root", type=str, default=ROOT, help="tree whose package is timed (another checkout of this project)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import loraine_jl_amd
    from loraine_jl_amd.model import build_factored_model

    m, n, kh = a.msz, a.nvar, a.khat
    rng = np.random.default_rng(0)
    V = rng.standard_normal((n, m, kh)) / np.sqrt(m)
    d = rng.choice([-1.0, 1.0], size=(n, kh))
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    W = G @ G.T
    X = rng.standard_normal((m, m))
    X = 0.5 * (X + X.T)
    y = rng.standard_normal(n)
    dev = loraine_jl_amd.Device(0)
    dev.set_option("profile", 1)
    rec = dict(msz=m, nvar=n, khat=kh, reps=a.reps, root=os.path.basename(os.path.abspath(a.root)), cases={})
    keys = ("assemble", "lowrank", "lowrank_u", "hybrid_y", "hybrid_cross", "sparse")
    for ns in [int(x) for x in a.stored.split(",")]:
        items = [(V[k], d[k]) for k in range(n)]
        srng = np.random.default_rng(100 + ns)
        for t, k in enumerate(np.linspace(0, n - 1, ns).astype(int) if ns else []):
            items[int(k)] = _stored(m, t, srng)
        model = build_factored_model([-np.eye(m)], [items], np.zeros(n), factored_form=1)
        dev.upload_model(model.AA, model.sigmaA, model.qA, model.msizes)
        Vp, dp, khat = model.lowrank[0]
        dev.upload_lowrank(0, khat, Vp, dp)
        dev.set_factored(0)
        e = dict(stored=ns, stored_nnz=int(model.AA[0].nnz))
        for label, Gs in (("G", G), ("W_only", None)):
            dev.set_scaling(0, W, Gs)
            dev.schur_assemble(1)                        # warm-up: workspaces
            runs = {k: [] for k in keys}
            for _ in range(a.reps):
                dev.reset_timing()
                dev.schur_assemble(1)
                for k in keys:
                    runs[k].append(dev.timing(k))
            e[label] = {k + "_ms": float(np.median(v)) for k, v in runs.items()}
            e[label]["assemble_runs_ms"] = runs["assemble"]
        # the data operators, each timed by itself
        dev.set_option("profile_ops", 1)
        dev.ip_set_c(0, np.zeros((m, m)))
        dev.ip_set_iterate(0, X, np.zeros((m, m)))
        dev.ip_aa_x()
        dev.ip_residual_d(y)                             # warm-up
        ta, tm = [], []
        for _ in range(a.reps):
            dev.reset_timing()
            dev.ip_aa_x()
            dev.ip_residual_d(y)
            ta.append(dev.timing("aa_times"))
            tm.append(dev.timing("aat_to_mat"))
        dev.set_option("profile_ops", 0)
        e["aa_times_ms"], e["aat_to_mat_ms"] = float(np.median(ta)), float(np.median(tm))
        e["aa_times_runs_ms"], e["aat_to_mat_runs_ms"] = ta, tm
        rec["cases"][f"stored{ns}"] = e
        print(json.dumps(e), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
