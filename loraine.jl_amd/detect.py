"""From constraint matrices to factors: which A_ik of a model given as matrices (load_model, an SDPA file) are
V diag(d) V' of rank <= kmax, found on the device (Device.lowrank_detect, csrc/detect.hip) and handed to the loaders of factored
and hybrid models (model.build_factored_model) -- what `datarank = -1` does in the reference's prep_B, for ranks up to 64 and
without giving up on the whole model when one constraint has no such form.

plan()             pure: who looks at which constraint, and the device chunks -- no device, no matrix
detect_factors()   the items load_factored_model accepts, per block, and a report
fallback_reason()  pure: the rule that sends the whole model to the general path after all"""
import time

import numpy as np
import scipy.sparse as sp

from .model import LOWRANK_MAX, LOWRANK_MAX_WIDE, LOWRANK_TOL, _stored_matrix, lowrank_factor

HOST_SIDE = 96             # a support of at most this side goes to the host's eigh (lowrank_factor): it costs nothing there
DEFAULT_BUDGET_MB = 1024   # device chunk of detect_factors: cnt m^2 8 bytes at most this
RANK_RTOL = 1e-12          # the relative rank cut of lowrank_factor


def sketch_matrix(m, kmax, seed=0):
    """Omega of one block: m x (kmax + 8) standard normals from Philox(seed)."""
    return np.random.Generator(np.random.Philox(seed)).standard_normal((int(m), int(kmax) + 8))


def plan(blocks, kmax, budget_bytes, datasparsity=8, host_side=HOST_SIDE):
    """blocks[i] = (m, nnz, support): the side of LMI block i and, per constraint, its number of non-zeros and the side of
    its support (rows that hold a non-zero).  -> dict with, per block, the disjoint index lists
      stored[i]   nnz <= datasparsity: sparse enough to stay a stored matrix without a look
      host[i]     support side <= host_side: model.lowrank_factor on the host
      device[i]   the others
    and chunks = [(i, [k, ...]), ...]: the device constraints of one block in order, cnt m^2 8 <= budget_bytes each (the last
    chunk of a block may be ragged).  A budget below one matrix of a block that needs the device is a ValueError."""
    if kmax not in (LOWRANK_MAX, LOWRANK_MAX_WIDE):
        raise ValueError(f"kmax is {LOWRANK_MAX} or {LOWRANK_MAX_WIDE}, not {kmax!r}")
    out = dict(stored=[], host=[], device=[], chunks=[])
    for i, (m, nnz, support) in enumerate(blocks):
        nnz, support = np.asarray(nnz, dtype=np.int64), np.asarray(support, dtype=np.int64)
        if nnz.shape != support.shape:
            raise ValueError(f"block {i + 1}: {nnz.size} nnz counts, {support.size} support sides")
        st, ho, de = [], [], []
        for k in range(nnz.size):
            (st if nnz[k] <= datasparsity else ho if support[k] <= host_side else de).append(k)
        out["stored"].append(st)
        out["host"].append(ho)
        out["device"].append(de)
        if not de:
            continue
        per = int(budget_bytes) // (8 * int(m) * int(m))
        if per < 1:
            raise ValueError(f"block {i + 1}: one {m} x {m} matrix is {8 * m * m} bytes, the budget {int(budget_bytes)}")
        per = min(per, 65535)                      # (grid limit of the batched launches)
        for c0 in range(0, len(de), per):
            out["chunks"].append((i, de[c0:c0 + per]))
    return out


def fallback_reason(accepted, kept_nnz, max_stored=16, datasparsity=8):
    """Why a detected model takes the general path after all, or "".  accepted: constraints that became factors (all blocks);
    kept_nnz[i]: the nnz of every constraint of block i that stays a stored matrix.  The rule: nothing accepted, or a block
    that would keep more than max_stored stored constraints with more than datasparsity non-zeros."""
    if accepted == 0:
        return "no constraint has a factor of rank <= kmax"
    for i, nz in enumerate(kept_nnz):
        dense = int(np.count_nonzero(np.asarray(nz, dtype=np.int64) > datasparsity))
        if dense > max_stored:
            return (f"LMI block {i + 1} would keep {dense} stored constraints with more than {datasparsity} non-zeros "
                    f"(max_stored = {max_stored})")
    return ""


def _support_side(A):
    return int(np.count_nonzero(np.diff(A.indptr)))      # (symmetric: rows with an entry = columns with an entry)


def detect_factors(A, n, kmax, device, budget_mb=None, seed=0, datasparsity=8, host_side=HOST_SIDE):
    """A[i] = [F_0, F_1, ..., F_n] as load_model takes it -> (items, report): items[i][k] is what load_factored_model accepts
    for constraint k + 1 of block i -- (V, d) with V trimmed to its r columns, or the stored matrix itself (csc) --, report a
    dict with, per block, the counts by verdict, the largest accepted residual, the histogram of ranks and the seconds.
    Asymmetric input is a ValueError.  The device sees dense chunks of at most budget_mb MiB; its verdicts depend on the
    matrix and the seed only, not on the budget."""
    budget = int((DEFAULT_BUDGET_MB if budget_mb is None else budget_mb) * 2 ** 20)
    mats, blocks = [], []
    for i, blk in enumerate(A):
        m = blk[0].shape[0]
        if len(blk) != n + 1:
            raise ValueError(f"block {i + 1}: {len(blk) - 1} constraint matrices, b has {n} entries")
        ms = [_stored_matrix(blk[k + 1], m, f"block {i + 1}, constraint {k + 1}") for k in range(n)]
        mats.append(ms)
        blocks.append((m, [a.nnz for a in ms], [_support_side(a) for a in ms]))
    pl = plan(blocks, kmax, budget, datasparsity, host_side)
    items = [list(ms) for ms in mats]
    report = dict(kmax=int(kmax), seed=int(seed), budget_bytes=budget, chunks=len(pl["chunks"]), blocks=[])
    for i, (m, nnz, _) in enumerate(blocks):
        report["blocks"].append(dict(m=int(m), stored=len(pl["stored"][i]), host_accepted=0, host_rejected=0, device_accepted=0,
                                     device_rejected=0, max_accepted_resid=0.0, ranks={}, seconds=0.0))
    def accept(i, k, V, d, resid, who):
        rb = report["blocks"][i]
        items[i][k] = (V, d)
        rb[who + "_accepted"] += 1
        rb["max_accepted_resid"] = max(rb["max_accepted_resid"], float(resid))
        rb["ranks"][int(V.shape[1])] = rb["ranks"].get(int(V.shape[1]), 0) + 1
    for i, (m, _, _) in enumerate(blocks):
        t0 = time.perf_counter()
        for k in pl["host"][i]:
            f = lowrank_factor(mats[i][k], m, kmax)
            if f is None:
                report["blocks"][i]["host_rejected"] += 1
            else:
                sub = mats[i][k].toarray()
                accept(i, k, f[0], f[1], np.linalg.norm(sub - (f[0] * f[1]) @ f[0].T), "host")
        report["blocks"][i]["seconds"] += time.perf_counter() - t0
    omegas = {}
    keys = ("detect_calls", "detect_accepted", "detect_rejected")
    before = {k: device.count(k) for k in keys}
    for i, ks in pl["chunks"]:
        t0 = time.perf_counter()
        m = blocks[i][0]
        if i not in omegas:
            omegas[i] = sketch_matrix(m, kmax, seed)
        dense = np.empty((len(ks), m, m))
        for s, k in enumerate(ks):
            dense[s] = mats[i][k].toarray()
        rank, resid, V, d = device.lowrank_detect(dense, kmax, tol=LOWRANK_TOL, rank_rtol=RANK_RTOL, omega=omegas[i])
        for s, k in enumerate(ks):
            r = int(rank[s])
            if r < 0:
                report["blocks"][i]["device_rejected"] += 1
            else:
                accept(i, k, np.ascontiguousarray(V[s][:, :r]), d[s, :r].copy(), resid[s], "device")
        report["blocks"][i]["seconds"] += time.perf_counter() - t0
    # the library's own counters of these calls (lrn_get_count; a solve resets them at every iteration)
    report["counters"] = {k: device.count(k) - before[k] for k in keys}
    report["counters"]["detect_sweeps_max"] = device.count("detect_sweeps_max")
    if pl["chunks"]:
        device.set_option("detect_release", 1)      # the chunk workspace does not stay beside the model
    report["accepted"] = sum(b["host_accepted"] + b["device_accepted"] for b in report["blocks"])
    report["kept_nnz"] = [[int(a.nnz) for a in its if sp.issparse(a)] for its in items]
    return items, report
