"""Schur assembly with LONG SPARSE stored constraints: the long route (pair_long = 1) against the pair kernels and
against the default cost model of the dense prefix, on seeded models:

  hex+tr    9^3 nodes x 3 dof (msz 2187), 512 hex elements (s = 24) and one stored trace row     (section 25's model)
  theta     msz 2000, a trace row and 4000 constraints of two entries
  tridiag   msz 2000, a tridiagonal row beside 400 constraints of two entries
  hybrid    msz 2000 / nvar 4000 / rank 2 factored block with one stored identity, mode 1          (section 12's model)

Arms, each on the library of this tree: P pair kernels (pair_long = 0, dense_threshold = 1e18), D the default cost model
(pair_long = 0, dense_threshold = -1, qA = nvar), L the long route (dense_threshold = 1e18), L+ the long route with pair_local = 1
where elements exist.  The arms alternate in one call, REPEATS repeats after a warm-up: median and spread (max - min) of the phase
timer "assemble", with "long" and "sparse" beside it.  Then the two sweeps that set the defaults: diag(a) rows of 32 ... 4096
entries beside 400 tiny partners at msz 4096 (pair_long_min = 1), L against P; pair_long_split 2^14 ... 2^22 on the identity
self pair at msz 2000.  lrn_mfma_f64_peak and the copy bandwidth are probed in the same call.

    python tools/long_rows_times.py [--out profiles/long_rows_times.json] [--quick] [--no-hybrid]
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loraine_jl_amd  # noqa: E402
from local_support_times import grid_model, stats  # noqa: E402

REPEATS = 5
KEYS = ("assemble", "long", "sparse", "local")


def rows_model(m, long_rows, ntiny, seed=3):
    """AA (n x m^2 CSR, = -A): the given long rows (lists of (r, c, v)) and ntiny symmetric constraints of two entries"""
    rng = np.random.default_rng(seed)
    r, k, v = [], [], []
    for e, (rr, cc, vv) in enumerate(long_rows):
        r.append(np.full(len(rr), e)); k.append(np.asarray(cc, np.int64) * m + np.asarray(rr, np.int64)); v.append(-np.asarray(vv, float))
    n0 = len(long_rows)
    i = rng.integers(0, m - 1, ntiny)
    j = i + 1 + rng.integers(0, m - 1 - i)
    w = rng.uniform(0.5, 1.5, ntiny)
    for a, b in ((i, j), (j, i)):
        r.append(n0 + np.arange(ntiny)); k.append(b.astype(np.int64) * m + a); v.append(-w)
    n = n0 + ntiny
    return sp.csr_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(k))), shape=(n, m * m))


def scaling(m, seed=5):
    rng = np.random.default_rng(seed)
    Gm = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    W = Gm @ Gm.T
    return (W + W.T) / 2


def context(m, AA, default_model, long_min=None):
    dev = loraine_jl_amd.Device(0)
    n = AA.shape[0]
    dev.set_option("profile", 1)
    dev.set_option("dense_threshold", -1.0 if default_model else 1.0e18)
    if long_min is not None:
        dev.set_option("pair_long_min", long_min)
    sigma = np.argsort(-np.diff(AA.indptr), kind="stable").astype(np.int64).reshape(-1, 1)
    qA = np.array([[n if default_model else 0], [0]], dtype=np.int64)
    dev.upload_model([AA], sigma, qA, [m])
    dev.set_scaling(0, scaling(m))
    return dev


def timed(dev, long, local=0, mode=0, split=None):
    dev.set_option("pair_long", long)
    dev.set_option("pair_local", local)
    if split is not None:
        dev.set_option("pair_long_split", split)
    dev.reset_timing()
    dev.schur_assemble(mode)
    return {k: dev.timing(k) for k in KEYS}


def alternate(arms, repeats):
    """arms: {name: callable -> timings}; the first pass warms every arm up and is dropped"""
    runs = {a: {k: [] for k in KEYS} for a in arms}
    for rep in range(repeats + 1):
        for a, f in arms.items():
            t = f()
            if rep:
                for k in KEYS:
                    runs[a][k].append(t[k])
    return {a: {k: stats(v) for k, v in runs[a].items()} for a in arms}


def verdict(out, new_arms, old_arms):
    best_new = min(new_arms, key=lambda a: out[a]["assemble"]["median_ms"])
    t = out[best_new]["assemble"]
    out["best_long_arm"] = best_new
    out["wins_by_more_than_both_spreads"] = bool(all(
        out[o]["assemble"]["median_ms"] - t["median_ms"] > max(out[o]["assemble"]["spread_ms"], t["spread_ms"]) for o in old_arms))


def compare(m, AA, repeats, with_local, long_min=None):
    sparse_dev, model_dev = context(m, AA, False, long_min), context(m, AA, True, long_min)
    arms = {"P": lambda: timed(sparse_dev, 0), "D": lambda: timed(model_dev, 0), "L": lambda: timed(sparse_dev, 1)}
    if with_local:
        arms["L+"] = lambda: timed(sparse_dev, 1, local=1)
    out = alternate(arms, repeats)
    H1 = (timed(sparse_dev, 1), sparse_dev.schur_get())[1]
    H0 = (timed(sparse_dev, 0), sparse_dev.schur_get())[1]
    out["rel_diff_long_vs_pair"] = float(np.abs(H1 - H0).max() / np.abs(H0).max())
    out["long_pairs"] = int((timed(sparse_dev, 1), sparse_dev.count("pair_long_pairs"))[1])
    verdict(out, ["L", "L+"] if with_local else ["L"], ["P", "D"])
    sparse_dev.close()
    model_dev.close()
    return out


def hybrid(repeats, m=2000, n=4000, kh=2):
    """section 12's block: factors of rank 2 and one stored identity, mode 1"""
    from loraine_jl_amd.model import build_factored_model
    rng = np.random.default_rng(0)
    V = rng.standard_normal((n, m, kh)) / np.sqrt(m)
    d = rng.choice([-1.0, 1.0], size=(n, kh))
    items = [(V[k], d[k]) for k in range(n)]
    items[0] = sp.identity(m, format="csc")
    model = build_factored_model([-np.eye(m)], [items], np.zeros(n), factored_form=1)
    dev = loraine_jl_amd.Device(0)
    dev.set_option("profile", 1)
    dev.upload_model(model.AA, model.sigmaA, model.qA, model.msizes)
    Vp, dp, khat = model.lowrank[0]
    dev.upload_lowrank(0, khat, Vp, dp)
    dev.set_factored(0)
    dev.set_scaling(0, scaling(m))
    out = alternate({"P": lambda: timed(dev, 0, mode=1), "L": lambda: timed(dev, 1, mode=1)}, repeats)
    out["note"] = "the upload's default cost model keeps the identity sparse: arm D is arm P"
    verdict(out, ["L"], ["P"])
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "long_rows_times.json"))
    ap.add_argument("--quick", action="store_true", help="three repeats, short sweeps")
    ap.add_argument("--no-hybrid", action="store_true")
    a = ap.parse_args()
    rep = 3 if a.quick else REPEATS
    res = {"repeats": rep, "models": {}, "sweep_min": {}, "sweep_split": {}}
    probe = loraine_jl_amd.Device(0)
    res["mfma_f64_peak_tflops"] = probe.mfma_f64_peak()
    res["hbm_copy_peak"] = probe.hbm_copy_peak()
    probe.close()

    def save():
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    show = lambda r: json.dumps({k: (v["assemble"] if isinstance(v, dict) and "assemble" in v else v) for k, v in r.items()})

    d2 = np.arange(2000)
    tri = (np.concatenate([d2, d2[1:], d2[:-1]]), np.concatenate([d2, d2[:-1], d2[1:]]), np.concatenate([2.0 * np.ones(2000), -np.ones(3998)]))
    models = {"hex+tr": lambda: grid_model("hex+tr")[:2] + (True,),
              "theta": lambda: (2000, rows_model(2000, [(d2, d2, np.ones(2000))], 4000), False),
              "tridiag": lambda: (2000, rows_model(2000, [tri], 400), False)}
    for name, make in models.items():
        m, AA, with_local = make()
        r = compare(m, AA, rep, with_local)
        r["msz"], r["constraints"] = m, AA.shape[0]
        res["models"][name] = r
        print(name, show(r), flush=True)
        save()
    if not a.no_hybrid:
        res["models"]["hybrid"] = hybrid(rep)
        print("hybrid", show(res["models"]["hybrid"]), flush=True)
        save()

    # pair_long_min: the smallest swept count from which L wins by more than both spreads
    m = 4096
    rng = np.random.default_rng(9)
    for cnt in ((64, 512, 4096) if a.quick else (32, 64, 128, 256, 512, 1024, 2048, 4096)):
        rows = np.sort(rng.choice(m, cnt, replace=False))
        AA = rows_model(m, [(rows, rows, rng.uniform(0.5, 1.5, cnt))], 400)
        dev = context(m, AA, False, long_min=1)
        r = alternate({"P": lambda: timed(dev, 0), "L": lambda: timed(dev, 1)}, rep)
        verdict(r, ["L"], ["P"])
        dev.close()
        res["sweep_min"][str(cnt)] = r
        print("sweep_min", cnt, show(r), flush=True)
        save()
    won = sorted(int(k) for k, r in res["sweep_min"].items() if r["wins_by_more_than_both_spreads"])
    swept = sorted(int(k) for k in res["sweep_min"])
    tail = [c for c in swept if all(x in won for x in swept if x >= c)]
    res["pair_long_min_measured"] = min(tail) if tail else None

    # pair_long_split: the identity self pair at msz 2000
    AA = rows_model(2000, [(d2, d2, np.ones(2000))], 0)
    dev = context(2000, AA, False)
    splits = [1 << e for e in ((14, 18, 22) if a.quick else range(14, 23))]
    r = alternate({str(s): (lambda s=s: timed(dev, 1, split=s)) for s in splits}, rep)
    dev.close()
    res["sweep_split"] = r
    res["pair_long_split_measured"] = int(min(r, key=lambda s: r[s]["long"]["median_ms"]))
    for s in r:
        print("sweep_split", s, json.dumps(r[s]["long"]), flush=True)
    print("pair_long_min", res["pair_long_min_measured"], "pair_long_split", res["pair_long_split_measured"], flush=True)
    save()


if __name__ == "__main__":
    main()
