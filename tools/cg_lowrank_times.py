"""Times of the CG path (kit = 1) through the entries of AA and from the rank-k factors (option cg_lowrank 0 / 1).

Data: a planted problem with dense factors (synthetic.FactoredLowRankProblem: V_k msz x rank, N(0, 1/msz), d = +-1) of
rank 2 and of rank 1, MATERIALISED on the host -- AA holds -vec(V_k D_k V_k') for every constraint, all in dense slots
-- with the factors uploaded beside it, so that both routes see the same constraints.  Default size msz 320 / nvar 640:
the host builds and converts that AA (6.6e7 entries) in about 10 s per upload, and the model is uploaded six times
(--msz / --nvar for a larger one; host time grows with msz^2 nvar).

Per rank and per value of cg_lowrank (0 = the entry routes, the baseline; 1 = every piece from the factors), median of
--reps runs after a warm-up, one process, device events of the library (option "profile"):
  assemble_ms      H of the assembled-matrix operator (hop_prepare: mode 0 / mode 1), a fresh scaling per run
  operator_ms      one application of the matrix-free operator (lrn_matvec under matvec_h = 1)
  prec_setup_ms    lrn_prec_setup of H_alpha at erank 1 and 3 (the whole call: eigenvectors, ts, S, its factorisation)
  ip_iteration_ms  wall time of a kit = 1 solve (H_alpha, erank 1) divided by its IP iterations, with the CG iterations

    python tools/cg_lowrank_times.py --out profiles/cg_lowrank_times.json
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


def materialised_model(P):
    """MyModel of the planted problem with every constraint stored: AA row k = -vec(A_k) (dense), factors beside it."""
    from loraine_jl_amd.model import MyModel, pad_factors
    m, n = P.msz, P.nvar
    A = np.einsum("kip,kp,kjp->kij", P.V, P.d, P.V)
    A = 0.5 * (A + A.transpose(0, 2, 1))
    AA = sp.csr_matrix(-A.reshape(n, m * m))
    nzA = np.full((n, 1), m * m, dtype=np.int64)
    sigmaA = np.arange(n, dtype=np.int64).reshape(n, 1)
    qA = np.full((2, 1), n, dtype=np.int64)                  # every constraint above the sparsity limit: dense slots
    lowrank = [pad_factors([(P.V[k], P.d[k]) for k in range(n)], n, m)]
    return MyModel(None, [AA], [], [P.C_dense()], nzA, sigmaA, qA, P.b.copy(), 0.0, np.zeros(0), sp.csr_matrix((n, 0)),
                   n, np.array([m], dtype=np.int64), 0, 1, lowrank, "")


def median_ms(dev, key, run, reps):
    run()                                                    # warm-up: workspaces, the dense copy of the factors
    out = []
    for _ in range(reps):
        dev.set_option("reset_timing", 1)
        run()
        out.append(dev.timing(key))
    return float(np.median(out)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msz", type=int, default=320)
    ap.add_argument("--nvar", type=int, default=640)
    ap.add_argument("--ranks", type=str, default="2,1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import loraine_jl_amd
    from loraine_jl_amd import resident, solvers
    from loraine_jl_amd.synthetic import FactoredLowRankProblem

    m, n = a.msz, a.nvar
    dev = loraine_jl_amd.Device(0)
    dev.set_option("profile", 1)
    rng = np.random.default_rng(0)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    W = G @ G.T
    x = rng.standard_normal(n)
    rec = dict(msz=m, nvar=n, reps=a.reps, ranks={})
    for rank in [int(r) for r in a.ranks.split(",")]:
        t0 = time.time()
        P = FactoredLowRankProblem(m, n, krank=rank, xrank=4, seed=20250700 + rank)
        model = materialised_model(P)
        e = dict(rank=rank, khat=model.lowrank[0][2], host_build_s=time.time() - t0, routes={})
        for opt in (0, 1):
            dev.upload_model(model.AA, model.sigmaA, model.qA, model.msizes)      # (the solve below uploads its own copy)
            V, d, khat = model.lowrank[0]
            dev.upload_lowrank(0, khat, V, d)
            dev.set_option("cg_lowrank", opt)
            r = {}

            def assemble():
                dev.set_scaling(0, W, G)                     # (a new scaling: H is assembled again)
                dev.matvec(x)
            dev.set_option("matvec_h", 2)
            r["assemble_ms"], r["assemble_runs"] = median_ms(dev, "assemble", assemble, a.reps)
            r["hop_assemble_lowrank"] = dev.count("hop_assemble_lowrank")
            dev.set_option("matvec_h", 1)
            r["operator_ms"], r["operator_runs"] = median_ms(dev, "matvec", lambda: dev.matvec(x), a.reps)
            r["op_factored_cg"] = dev.count("op_factored_cg")
            for erank in (1, 3):
                key = "prec_setup_erank%d_ms" % erank
                r[key], r[key[:-3] + "_runs"] = median_ms(dev, "prec_setup", lambda: dev.prec_setup(1, erank, 1), a.reps)
                r["prec_ts_factored_erank%d" % erank] = dev.count("prec_ts_factored")
            dev.set_option("matvec_h", 0)
            if not a.no_solve:
                s, ha = resident.load(model, dict(kit=1, preconditioner=1, erank=1, datarank=rank, verb=0), device=dev)
                dev.set_option("cg_lowrank", opt)            # (the solver asked for -1, the cost model; here the route is forced)
                dev.set_option("reset_timing", 1)
                t1 = time.time()
                solvers.solve(s, ha)
                wall = time.time() - t1
                r.update(solve_status=int(s.status), ip_iterations=int(s.iter), cg_iterations=int(s.cg_iter_tot),
                         solve_s=wall, ip_iteration_ms=1e3 * wall / max(1, int(s.iter)),
                         solve_hop_assemble=dev.count("hop_assemble"), solve_hop_assemble_lowrank=dev.count("hop_assemble_lowrank"),
                         solve_op_factored_cg=dev.count("op_factored_cg"))
            dev.set_option("cg_lowrank", 0)
            e["routes"]["cg_lowrank_%d" % opt] = r
            print(json.dumps(dict(rank=rank, cg_lowrank=opt, **r)), flush=True)
        rec["ranks"]["rank%d" % rank] = e
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
