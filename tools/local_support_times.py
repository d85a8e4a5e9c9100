"""Schur assembly of finite-element-like stored constraints three ways: the local route (pair_local = 1), the
pair kernels (pair_local = 0) and all constraints stored dense (dense_threshold = 0), on three seeded models:

  q4      31 x 31 nodes x 2 dof (msz 1922), 900 Q4 elements, s = 8
  hex     9^3 nodes x 3 dof (msz 2187), 512 hex elements, s = 24
  hex+tr  the same with one stored trace row: an s = msz owner, which stays on the old routes

Each model is uploaded twice (stored sparse, stored dense; two contexts) and the three arms are timed in one call, alternating,
REPEATS times each: phase timer "assemble" of lrn_schur_assemble mode 0, with "local" and "sparse" beside it.  Reported per
arm: median and spread (max - min).  Then the sweep s = 4, 6, 8, 12, 16, 24, 32 at fixed msz with pair_local_min = 1: local
against pair, the smallest s at which local wins beyond the pair arm's spread.  The flop rate of the local kernel,
sum over its pairs of 2 s_i s_j (s_i + s_j) / time of "local", stands beside lrn_mfma_f64_peak of the same call.

    python tools/local_support_times.py [--out profiles/local_support_times.json] [--quick]
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import loraine_jl_amd  # noqa: E402

REPEATS = 5


def element_rows(m, supports, rng):
    """AA (n x m^2 CSR, = -A) of constraints dense and symmetric on their supports, A[S, S] = G G'"""
    r, k, v = [], [], []
    for e, S in enumerate(supports):
        s = len(S)
        Gm = rng.standard_normal((s, s)) / np.sqrt(s)
        Ah = Gm @ Gm.T
        a, b = np.meshgrid(S, S, indexing="ij")
        r.append(np.full(s * s, e)); k.append((b * m + a).ravel()); v.append(-Ah.ravel())
    return r, k, v


def grid_model(kind, seed=1):
    rng = np.random.default_rng(seed)
    if kind == "q4":
        nx, dof = 31, 2
        node = lambda i, j: i * nx + j
        els = [[node(i, j), node(i, j + 1), node(i + 1, j), node(i + 1, j + 1)] for i in range(nx - 1) for j in range(nx - 1)]
        m = nx * nx * dof
    else:
        nx, dof = 9, 3
        node = lambda i, j, l: (i * nx + j) * nx + l
        els = [[node(i + a, j + b, l + c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
               for i in range(nx - 1) for j in range(nx - 1) for l in range(nx - 1)]
        m = nx ** 3 * dof
    supports = [np.array(sorted(dof * v + d for v in el for d in range(dof))) for el in els]
    r, k, v = element_rows(m, supports, rng)
    n = len(supports)
    if kind == "hex+tr":
        d = np.arange(m)
        r.append(np.full(m, n)); k.append(d * m + d); v.append(-np.ones(m))
        n += 1
    AA = sp.csr_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(k))), shape=(n, m * m))
    return m, AA, supports


def sweep_model(s, m=2000, n=400, seed=2):
    rng = np.random.default_rng(seed + s)
    supports = [np.array(sorted(2 * v + d for v in rng.choice(m // 2, s // 2, replace=False) for d in (0, 1))) for _ in range(n)]
    r, k, v = element_rows(m, supports, rng)
    return m, sp.csr_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(k))), shape=(n, m * m)), supports


def context(m, AA, dense, local_min=None, seed=5):
    dev = loraine_jl_amd.Device(0)
    n = AA.shape[0]
    dev.set_option("profile", 1)
    dev.set_option("dense_threshold", 0.0 if dense else 1.0e18)
    if local_min is not None:
        dev.set_option("pair_local_min", local_min)
    sigma = np.argsort(-np.diff(AA.indptr), kind="stable").astype(np.int64).reshape(-1, 1)
    qA = np.array([[n if dense else 0], [0]], dtype=np.int64)
    dev.upload_model([AA], sigma, qA, [m])
    rng = np.random.default_rng(seed)
    Gm = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    W = Gm @ Gm.T
    dev.set_scaling(0, (W + W.T) / 2)
    return dev


def timed(dev, local):
    dev.set_option("pair_local", local)
    dev.reset_timing()
    dev.schur_assemble(0)
    return {k: dev.timing(k) for k in ("assemble", "local", "sparse")}, dev.count("pair_local_pairs")


def stats(xs):
    return {"median_ms": float(np.median(xs)), "spread_ms": float(max(xs) - min(xs)), "all_ms": [float(x) for x in xs]}


def compare(m, AA, supports, with_dense, local_min=None, repeats=REPEATS):
    sparse_dev = context(m, AA, False, local_min)
    dense_dev = context(m, AA, True) if with_dense else None
    arms = {"local": [], "pair": [], "dense": [], "local_kernel": []}
    pairs = 0
    for rep in range(repeats + 1):                       # (the first pass warms every arm up and is dropped)
        t1, pairs = timed(sparse_dev, 1)
        t0, _ = timed(sparse_dev, 0)
        td = timed(dense_dev, 0)[0] if dense_dev else None
        if rep == 0:
            continue
        arms["local"].append(t1["assemble"]); arms["local_kernel"].append(t1["local"]); arms["pair"].append(t0["assemble"])
        if td:
            arms["dense"].append(td["assemble"])
    H1 = (timed(sparse_dev, 1), sparse_dev.schur_get())[1]
    H0 = (timed(sparse_dev, 0), sparse_dev.schur_get())[1]
    s = np.array([len(x) for x in supports])
    out = {k: stats(v) for k, v in arms.items() if v}
    out["pairs"] = int(pairs)
    out["rel_diff_local_vs_pair"] = float(np.abs(H1 - H0).max() / np.abs(H0).max())
    n = len(supports)                                    # the elements by themselves (the trace row is no local owner)
    out["local_flop"] = float(2.0 * (s[:, None] * s[None, :] * (s[:, None] + s[None, :]))[np.triu_indices(n)].sum())
    out["local_tflops"] = out["local_flop"] / (out["local_kernel"]["median_ms"] * 1e-3) / 1e12
    sparse_dev.close()
    if dense_dev:
        dense_dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "local_support_times.json"))
    ap.add_argument("--quick", action="store_true", help="the hex model and the sweep only, three repeats")
    a = ap.parse_args()
    rep = 3 if a.quick else REPEATS
    res = {"repeats": rep, "models": {}, "sweep": {}}
    probe = loraine_jl_amd.Device(0)
    res["mfma_f64_peak_tflops"] = probe.mfma_f64_peak()
    probe.close()
    for kind in (["hex"] if a.quick else ["q4", "hex", "hex+tr"]):
        m, AA, supports = grid_model(kind)
        r = compare(m, AA, supports, True, repeats=rep)
        r["msz"], r["constraints"] = m, AA.shape[0]
        best = min(("pair", "dense"), key=lambda k: r[k]["median_ms"])
        r["best_existing"] = best
        r["wins_by_more_than_spread"] = bool(r[best]["median_ms"] - r["local"]["median_ms"] > r[best]["spread_ms"])
        res["models"][kind] = r
        print(kind, json.dumps({k: r[k] for k in ("local", "pair", "dense", "local_kernel", "best_existing",
                                                  "wins_by_more_than_spread", "local_tflops", "rel_diff_local_vs_pair")}), flush=True)
    for s in (4, 6, 8, 12, 16, 24, 32):
        m, AA, supports = sweep_model(s)
        r = compare(m, AA, supports, False, local_min=1, repeats=rep)
        r["wins"] = bool(r["pair"]["median_ms"] - r["local"]["median_ms"] > r["pair"]["spread_ms"])
        res["sweep"][str(s)] = r
        print("sweep s", s, "entries", s * s, json.dumps({k: r[k] for k in ("local", "pair", "wins", "local_tflops")}), flush=True)
    won = [int(s) for s, r in res["sweep"].items() if r["wins"]]
    res["crossover_s"] = min(won) if won else None
    print("crossover s", res["crossover_s"], "peak probe", res["mfma_f64_peak_tflops"], flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
