"""Times of the rank-k Schur assembly (lrn_schur_assemble mode 1) at msz 2000 / nvar 4000.

The synthetic dense model (lrn_synthetic_dense_model) only provides a context of that shape; random dense factors
with khat in {1, 2, 4, 8, 16} (random signs) and a random SPD scaling W = G G' are uploaded on top of it.  Mode 1 is
timed with device events (option "profile": "lowrank_u" = U = G'V, "lowrank" = U and the blocked product) after a
warm-up, mode 0 (the general path on the synthetic data) once after a cold call.  For khat = 1 the existing rank-one product of the same
shape -- (U'U).^2, GEMM_SQUARE, lower tiles -- runs through lrn_dbg_gemm (LRN_DBG_GEMM_REPS: back-to-back products timed
with events inside the library).  Useful flop: 2 R msz^2 for U, R^2 msz for the lower triangle of T (R = nvar khat).

    python tools/lowrank_assembly_times.py --out profiles/lowrank_assembly_times.json
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- \
        python tools/lowrank_assembly_times.py --khat 1 --no-mode0 --reps 2
"""
import argparse
import json
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 78.6


def _captured_stderr(fn):
    """Run fn() with file descriptor 2 redirected to a temporary file; -> (result, text the library printed)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            res = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return res, tmp.read().decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msz", type=int, default=2000)
    ap.add_argument("--nvar", type=int, default=4000)
    ap.add_argument("--khat", type=str, default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-mode0", action="store_true")
    ap.add_argument("--no-rank1", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    os.environ.setdefault("LRN_DBG_GEMM_REPS", str(max(1, a.reps)))     # (read by the library at its first dbg_gemm)
    import loraine_jl_amd
    from loraine_jl_amd._capi import GEMM_SQUARE, GEMM_TRI_LOWER, ptr

    m, n = a.msz, a.nvar
    dev = loraine_jl_amd.Device(0)
    dev.synthetic_dense_model(m, n, 7)
    rng = np.random.default_rng(0)
    G = rng.standard_normal((m, m)) / np.sqrt(m) + np.eye(m)
    W = G @ G.T
    dev.set_scaling(0, W, G)
    dev.set_option("profile", 1)
    rec = dict(msz=m, nvar=n, peak_tflops=PEAK_TF, modes={})
    for kh in [int(x) for x in a.khat.split(",")]:
        R = n * kh
        cp = (np.arange(m + 1, dtype=np.int64) * R + 1)
        rv = np.tile(np.arange(1, R + 1, dtype=np.int64), m)
        nz = rng.standard_normal(R * m) / np.sqrt(m)
        d = rng.choice([-1.0, 1.0], size=R)
        dev._chk(dev.lib.lrn_upload_lowrank(dev.h, 0, kh, ptr(cp), ptr(rv), ptr(nz), ptr(d)), "lrn_upload_lowrank")
        del rv, nz
        dev.schur_assemble(1)                            # warm-up (dense copy of V, workspaces)
        tu, tt = [], []
        for _ in range(a.reps):
            dev.set_option("reset_timing", 1)
            dev.schur_assemble(1)
            tu.append(dev.timing("lowrank_u"))
            tt.append(dev.timing("lowrank"))
        u_ms, all_ms = float(np.median(tu)), float(np.median(tt))
        fu, ft = 2.0 * R * m * m, float(R) * R * m
        e = dict(khat=kh, R=R, u_ms=u_ms, t_ms=all_ms - u_ms, lowrank_ms=all_ms, runs_ms=tt,
                 u_tflops=fu / u_ms * 1e-9, t_tflops=ft / (all_ms - u_ms) * 1e-9, tflops=(fu + ft) / all_ms * 1e-9)
        e["frac_peak"] = e["tflops"] / PEAK_TF
        e["t_frac_peak"] = e["t_tflops"] / PEAK_TF
        rec["modes"][f"khat{kh}"] = e
        print(json.dumps(e), flush=True)
        if kh == 1 and not a.no_rank1:
            # the existing rank-one product of the same shape: (U'U).^2, lower tiles, U msz x nvar (host operands)
            U = rng.standard_normal((m, n)) / np.sqrt(m)
            _, txt = _captured_stderr(lambda: dev.dbg_gemm(U, U, transA=True, flags=GEMM_TRI_LOWER | GEMM_SQUARE))
            us = [float(x) for x in re.findall(r"([0-9.]+) us per product", txt)]
            if us:
                r1 = dict(square_ms=us[-1] * 1e-3, line=txt.strip())
                r1["fused_over_square"] = e["t_ms"] / r1["square_ms"]
                rec["rank1_gemm_square"] = r1
                print(json.dumps(r1), flush=True)
    if not a.no_mode0:
        dev.set_option("reset_timing", 1)
        dev.schur_assemble(0)                            # cold: factor of W, workspaces (64 GB of packed L'A_kL)
        rec["mode0_cold_ms"] = dev.timing("assemble")
        dev.set_option("reset_timing", 1)
        dev.schur_assemble(0)
        rec["mode0_ms"] = dev.timing("assemble")
        print(json.dumps(dict(mode0_cold_ms=rec["mode0_cold_ms"], mode0_ms=rec["mode0_ms"])), flush=True)
        for k, e in rec["modes"].items():
            e["mode0_over_mode1"] = rec["mode0_ms"] / e["lowrank_ms"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
