"""Times of the CG path (kit = 1) on a FACTORED model (library option cg_factored = 1): the constraints exist as factors only.

Data: synthetic.FactoredLowRankProblem (V_k msz x rank dense, N(0, 1/msz), d = +-1) loaded through build_factored_model(...,
factored_form=1) -- no row of AA anywhere.  Shapes (--shapes msz:nvar:rank,...): 320:640:2 (comparable with the table of
DESIGN.md section 14), 2000:4000:2 (section 11's shape), 256:32768:1 (the regime of the fused quadratic form; H is 8.6 GB).

Per shape, median of --reps runs after a warm-up, one process, device events of the library (option "profile"):
  operator_ms[sS_qQ]   one application of the matrix-free operator (lrn_matvec under matvec_h = 1) with fac_op_scaled = S and
                       fac_quadform = Q; s0_q0 is the parent's composition mat(AA' x) -> W M W -> Q = Z Vd -> column dots
  scaled_y_ms          Y = W Vd, once per NT scaling (option profile_ops; its own run)
  assemble_ms, h_operator_ms   H in mode 1 (a fresh scaling per run) and one y = H x (matvec_h = 2); --no-h skips both
  prec_setup_erank{1,3}_ms     lrn_prec_setup of H_alpha (the whole call)
  ip_iteration_ms      wall time of a kit = 1 solve (H_alpha, erank 1; --solve-maxit caps the IP iterations) per IP iteration

    python tools/cg_factored_times.py --out profiles/cg_factored_times.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(dev, key, run, reps):
    run()                                                    # warm-up: workspaces
    out = []
    for _ in range(reps):
        dev.set_option("reset_timing", 1)
        run()
        out.append(dev.timing(key))
    return float(np.median(out)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, default="320:640:2,2000:4000:2,256:32768:1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--no-h", action="store_true")
    ap.add_argument("--solve-maxit", type=int, default=0, help="cap of the IP iterations of the solve (0: run to the end)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import loraine_jl_amd
    from loraine_jl_amd import resident, solvers
    from loraine_jl_amd.model import build_factored_model
    from loraine_jl_amd.synthetic import FactoredLowRankProblem

    dev = loraine_jl_amd.Device(0)
    dev.set_option("profile", 1)
    rec = dict(reps=a.reps, shapes={})
    for shape in a.shapes.split(","):
        m, n, rank = (int(v) for v in shape.split(":"))
        t0 = time.time()
        P = FactoredLowRankProblem(m, n, krank=rank, xrank=4, seed=20250800 + rank)
        model = build_factored_model(P.F0(), P.factors(), P.b, factored_form=1)
        model.factored_cg = True
        rng = np.random.default_rng(0)
        G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
        W = G @ G.T
        x = rng.standard_normal(n)
        r = dict(msz=m, nvar=n, rank=rank, khat=model.lowrank[0][2], host_build_s=time.time() - t0)
        dev.upload_model(model.AA, model.sigmaA, model.qA, model.msizes)
        V, d, khat = model.lowrank[0]
        dev.upload_lowrank(0, khat, V, d)
        dev.set_factored(0)
        dev.set_option("cg_factored", 1)
        dev.set_scaling(0, W, G)
        dev.set_option("matvec_h", 1)
        for scaled in (0, 1):
            for quad in (0, 1):
                dev.set_option("fac_op_scaled", scaled)
                dev.set_option("fac_quadform", quad)
                key = "operator_ms_s%d_q%d" % (scaled, quad)
                r[key], r[key + "_runs"] = median_ms(dev, "matvec", lambda: dev.matvec(x), a.reps)
        dev.set_option("fac_quadform", 0)
        dev.set_option("fac_op_scaled", 1)
        dev.set_option("profile_ops", 1)

        def scaled_y():
            dev.set_scaling(0, W, G)                         # (a new scaling: Y is formed again)
            dev.matvec(x)
        r["scaled_y_ms"], r["scaled_y_runs"] = median_ms(dev, "fac_scaled_y", scaled_y, a.reps)
        dev.set_option("profile_ops", 0)
        dev.set_option("fac_op_scaled", -1)
        dev.set_option("fac_quadform", -1)
        if not a.no_h:
            def assemble():
                dev.set_scaling(0, W, G)                     # (a new scaling: H is assembled again)
                dev.matvec(x)
            dev.set_option("matvec_h", 2)
            r["assemble_ms"], r["assemble_runs"] = median_ms(dev, "assemble", assemble, a.reps)
            r["h_operator_ms"], r["h_operator_runs"] = median_ms(dev, "matvec", lambda: dev.matvec(x), a.reps)
        dev.set_option("matvec_h", 1)
        for erank in (1, 3):
            key = "prec_setup_erank%d_ms" % erank
            r[key], r[key[:-3] + "_runs"] = median_ms(dev, "prec_setup", lambda: dev.prec_setup(1, erank, 1), a.reps)
        dev.set_option("matvec_h", 0)
        if not a.no_solve:
            opts = dict(kit=1, preconditioner=1, erank=1, verb=0)
            if a.solve_maxit > 0:
                opts["maxit"] = a.solve_maxit
            s, ha = resident.load(model, opts, device=dev)
            dev.set_option("reset_timing", 1)
            t1 = time.time()
            solvers.solve(s, ha)
            wall = time.time() - t1
            r.update(solve_status=int(s.status), ip_iterations=int(s.iter), cg_iterations=int(s.cg_iter_tot), solve_s=wall,
                     ip_iteration_ms=1e3 * wall / max(1, int(s.iter)), solve_hop_assemble=dev.count("hop_assemble"),
                     solve_hop_over_budget=dev.count("hop_over_budget"),
                     solve_op_factored_scaled=dev.count("op_factored_scaled"),
                     solve_op_quadform_fused=dev.count("op_quadform_fused"))
        dev.set_option("cg_factored", 0)
        rec["shapes"][shape] = r
        print(json.dumps(r), flush=True)
        if a.out:                                            # (after every shape: a later one may not fit the time)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(rec, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
