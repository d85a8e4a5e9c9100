"""Times of the low-rank detection (lrn_lowrank_detect, csrc/detect.hip) against the host route it replaces.

One chunk of dense constraints of rank 1, 2, 16 and 40 in equal parts at side --msz (2000), as many as fit the default budget of
detect.detect_factors (1024 MiB: 32 matrices of side 2000), at kmax 16 (rank 40 is rejected there) and 64.  Per kmax:
    steps      milliseconds per constraint of sketch, core, eig, factor, residual: the library's device events (option "profile")
               with the chunk already on the device, medians of --reps calls after 3 warm-ups
    hbm        the sketch pass reads cnt m^2 8 bytes, the residual pass the 64 x 64 tiles on and below the diagonal; their rates
               as a fraction of the copy rate lrn_hbm_copy_peak measures in the same process
    from_host  the whole call from a host pointer (the upload of the chunk included), host clock around the call (it ends in a
               device synchronise), median
    host_route model.lowrank_factor (numpy.linalg.eigh on the support) on 8 of the same constraints, host clock, scaled to
               --nvar (4000) constraints -- the yardstick
--small (64): the same at a side where the host route is the cheaper one (detect.plan sends supports of side <= 96 there).

    python tools/detect_times.py --out profiles/detect_times.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("detect_sketch", "detect_core", "detect_eig", "detect_factor", "detect_resid", "detect")
RANKS = (1, 2, 16, 40)


def make_chunk(m, cnt, seed=0):
    rng = np.random.default_rng(seed)
    mats = np.empty((cnt, m, m))
    ranks = []
    for k in range(cnt):
        r = min(RANKS[k % len(RANKS)], m)
        V = rng.standard_normal((m, r)) / np.sqrt(m)
        mats[k] = (V * rng.choice([-1.0, 1.0], size=r)) @ V.T
        mats[k] = 0.5 * (mats[k] + mats[k].T)
        ranks.append(r)
    return mats, ranks


def measure(dev, m, cnt, kmax, reps, warm, copy_gbps, nvar, host_n):
    import scipy.sparse as sp
    import torch

    from loraine_jl_amd import detect, model
    from loraine_jl_amd._capi import ptr

    mats, ranks = make_chunk(m, cnt)
    om = detect.sketch_matrix(m, kmax, 0)
    om_f = np.asfortranarray(om)
    A_dev = torch.from_numpy(mats).to("cuda:0")
    torch.cuda.synchronize()
    rank = np.zeros(cnt, dtype=np.int32)
    resid = np.zeros(cnt)
    V = np.zeros((cnt, kmax, m))
    d = np.zeros((cnt, kmax))

    def call(src):
        dev._chk(dev.lib.lrn_lowrank_detect(dev.h, m, cnt, ptr(src), kmax, model.LOWRANK_TOL, detect.RANK_RTOL, ptr(om_f),
                                            ptr(rank), ptr(resid), ptr(V), ptr(d)), "lrn_lowrank_detect")

    for _ in range(warm):
        call(A_dev)
    runs = {k: [] for k in STEPS}
    for _ in range(reps):
        dev.reset_timing()
        call(A_dev)
        for k in STEPS:
            runs[k].append(dev.timing(k))
    want = [r if r <= kmax else -1 for r in ranks]
    assert list(rank) == want, (list(rank), want)
    e = dict(msz=m, cnt=cnt, kmax=kmax, ranks=sorted(set(ranks)), accepted=int(np.sum(rank >= 0)),
             sweeps_max=dev.count("detect_sweeps_max"), max_accepted_resid=float(np.max(resid[rank >= 0], initial=0.0)))
    e["ms_per_constraint"] = {k: float(np.median(v)) / cnt for k, v in runs.items()}
    e["chunk_ms_runs"] = runs["detect"]
    nt = (m + 63) // 64
    sk_bytes = cnt * m * m * 8.0
    rs_bytes = cnt * (nt * (nt + 1) // 2) * 64 * 64 * 8.0
    e["sketch_gbps"] = sk_bytes / (np.median(runs["detect_sketch"]) * 1e-3) / 1e9
    e["resid_gbps"] = rs_bytes / (np.median(runs["detect_resid"]) * 1e-3) / 1e9
    e["copy_peak_gbps"] = copy_gbps
    e["sketch_over_copy_peak"] = e["sketch_gbps"] / copy_gbps
    e["resid_over_copy_peak"] = e["resid_gbps"] / copy_gbps
    for _ in range(warm):
        call(mats)
    hs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call(mats)
        hs.append((time.perf_counter() - t0) * 1e3)
    e["from_host_ms_per_constraint"] = float(np.median(hs)) / cnt
    del A_dev
    ht = []
    for k in range(min(host_n, cnt)):
        Ak = sp.csc_matrix(mats[k])
        t0 = time.perf_counter()
        f = model.lowrank_factor(Ak, m, kmax)
        ht.append((time.perf_counter() - t0) * 1e3)
        assert (f is None) == (ranks[k] > kmax)
    e["host_route_ms_per_constraint"] = float(np.median(ht))
    e["host_route_runs_ms"] = ht
    e["nvar"] = nvar
    e["host_route_s_at_nvar"] = e["host_route_ms_per_constraint"] * nvar / 1e3
    e["device_s_at_nvar"] = e["from_host_ms_per_constraint"] * nvar / 1e3
    e["host_over_device"] = e["host_route_ms_per_constraint"] / e["from_host_ms_per_constraint"]
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msz", type=int, default=2000)
    ap.add_argument("--small", type=int, default=64)
    ap.add_argument("--nvar", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-n", type=int, default=8)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()

    import loraine_jl_amd
    from loraine_jl_amd import detect

    dev = loraine_jl_amd.Device(0)
    dev.set_option("profile", 1)
    copy_gbps = dev.hbm_copy_peak()
    rec = dict(reps=a.reps, warmups=3, budget_mb=detect.DEFAULT_BUDGET_MB, runs=[])
    for m in (a.msz, a.small):
        cnt = max(4, min(4000, detect.DEFAULT_BUDGET_MB * 2 ** 20 // (8 * m * m)) // 4 * 4)
        for kmax in (16, 64):
            e = measure(dev, m, cnt, kmax, a.reps, 3, copy_gbps, a.nvar, a.host_n)
            rec["runs"].append(e)
            print(json.dumps(e), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(rec, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
