"""Seeded cases of factored constraints of rank 17 .. 64 (library option lowrank_wide, load_factored_model(..., wide=True);
csrc/ragged_plan.h, csrc/raggedops.hip: ragged_wide_epilogue), built on the helpers of tests/ragged_cases.py.  Shared by
tests/test_wide_cpu.py and tests/test_gpu_wide.py; everything is cached and left unchanged.  Weights are +-1, mixed.

    V1  37 / 5     all rank 32: Rc = R = 160, 2.5 tiles of class 32 (the last diagonal tile half full), K = 2 steps + a tail of
                   5 -- the shape the gate Rc < R would have sent to the padded product
    V2  70 / 16    ranks 64, 40, 33, 32, 17, 25, 16, 9, 8, 5, 4, 3, 2, 1, 1, 0: all seven classes; class 64 three groups (two
                   tile rows, padding columns inside groups), class 32 three groups on 96 columns (a partial tile of one group),
                   segment starts 0, 192, 288, 320, 336, 344, 346, Rc = 348; one rank-0 row; K tail of 6
    V3  45 / 12    hybrid: constraint 0 a stored sparse trace row, constraint 1 a stored full matrix (a dense slot), then ranks
                   48, 20, 16, 2 and six of rank 1; two linear rows -- the cross terms, ts of H_alpha and lrn_pcg
    V4  37 + 20 / 5  two blocks: V1's beside a narrow one of khat 2 with ranks 1, 2, 1, 2, 1
    PlantedWide    ragged_cases.Planted (msz 40 / nvar 60) with two constraints of rank 24 and one of rank 40 among rank 1

device_order() restates the rank-class route with the summation order of the device epilogue in NumPy float64: the 16 x 16
accumulator blocks by register sums and balanced trees (the lane butterflies), then the two accumulators of a wave in a direction of
size >= 32 (rows first), then the two waves in a direction of size 64 -- and plants single faults on request."""
import functools
import types

import numpy as np
import scipy.sparse as sp

import ragged_cases as rc

LD = np.longdouble
NAMES = ["V1", "V2", "V3", "V4"]
RANKS = {
    "V1": [32] * 5,
    "V2": [64, 40, 33, 32, 17, 25, 16, 9, 8, 5, 4, 3, 2, 1, 1, 0],
    "V3": [0, 0, 48, 20, 16, 2, 1, 1, 1, 1, 1, 1],
    "V4b": [1, 2, 1, 2, 1],
}
SIZES = {"V1": (37, 5), "V2": (70, 16), "V3": (45, 12), "V4b": (20, 5)}
SEEDS = {"V1": 201, "V2": 202, "V3": 203, "V4b": 204}
V3_TRACE, V3_DENSE = 0, 1
WIDE_CLASSES = (64, 32, 16, 8, 4, 2, 1)


@functools.lru_cache(maxsize=None)
def factors(name):
    m, _ = SIZES[name]
    rng = np.random.default_rng(SEEDS[name])
    return tuple(rc._dense_factor(rng, m, r) for r in RANKS[name])


@functools.lru_cache(maxsize=None)
def items(name):
    """The constraint list of a single block, as build_factored_model takes it."""
    out = list(factors(name))
    if name == "V3":
        m = SIZES[name][0]
        full = np.random.default_rng(77).standard_normal((m, m)) / m
        out[V3_TRACE] = sp.identity(m, format="csc")
        out[V3_DENSE] = sp.csc_matrix(full + full.T)
    return tuple(out)


def blocks(name):
    return [list(items("V1")), list(items("V4b"))] if name == "V4" else [list(items(name))]


def nvar(name):
    return SIZES["V1" if name == "V4" else name][1]


def msizes(name):
    return [SIZES["V1"][0], SIZES["V4b"][0]] if name == "V4" else [SIZES[name][0]]


@functools.lru_cache(maxsize=None)
def c_lin(name):
    if name != "V3":
        return None
    return sp.csr_matrix(sp.random(nvar(name), 2, density=0.5, random_state=5, format="csr"))


@functools.lru_cache(maxsize=None)
def scaling(name):
    """[(W, G)] per block: ragged_cases.spd."""
    return [rc.spd(m, 2000 + 10 * i + m) for i, m in enumerate(msizes(name))]


@functools.lru_cache(maxsize=None)
def matrices(name):
    """Materialised constraints per block."""
    return [[rc.materialise(it, m) for it in blk] for blk, m in zip(blocks(name), msizes(name))]


@functools.lru_cache(maxsize=None)
def reference(name, factored_only=False):
    """H_ij = sum over blocks of tr(A_i W A_j W) in np.longdouble (+ C_lin C_lin' for V3: unit X_lin, S_lin_inv), natural order.
    factored_only: the stored rows and the linear term left out -- H_FF, what the rank-class route alone forms."""
    n = nvar(name)
    H = np.zeros((n, n), dtype=LD)
    for As, (W, _) in zip(matrices(name), scaling(name)):
        H += rc._h_block(As, W, LD)
    if factored_only:
        out = [k for k, r in enumerate(RANKS[name]) if r == 0] if name != "V4" else []
        H[out, :] = 0
        H[:, out] = 0
        return H
    C = c_lin(name)
    if C is not None:
        Cd = C.toarray().astype(LD)
        H += Cd @ Cd.T
    return H


@functools.lru_cache(maxsize=None)
def model(name):
    from loraine_jl_amd.model import build_factored_model
    n = nvar(name)
    C = c_lin(name)
    F0 = [-np.eye(m) for m in msizes(name)]
    return build_factored_model(F0, blocks(name), np.zeros(n), 0.0, None if C is None else np.ones(C.shape[1]), C,
                                factored_form=1, max_rank=64)


def block_model(name):
    """One block of V4 as a model of its own ("V1" or "V4b")."""
    from loraine_jl_amd.model import build_factored_model
    m, n = SIZES[name]
    return build_factored_model([-np.eye(m)], [list(items(name))], np.zeros(n), factored_form=1, max_rank=64)


# ---------------------------------------------------------------------------------------------- the plan in Python
def tiles(p, layout=WIDE_CLASSES):
    """The tile list of csrc/ragged_plan.h::plan_ragged from a plan of loraine_jl_amd.model.ragged_plan: (r0, r1, c0, c1, gi0,
    gj0, ka, kb, diag)."""
    grp0, g = {}, 0
    for c in layout:
        grp0[c] = g
        g += (p["seg"][c][1] - p["seg"][c][0]) // c
    out = []
    for ia, a in enumerate(layout):
        for b in layout[ia:]:
            (a0, a1), (b0, b1) = p["seg"][a], p["seg"][b]
            ta, tb = -(-(a1 - a0) // 64), -(-(b1 - b0) // 64)
            for ti in range(ta):
                for tj in range(ti + 1 if a == b else tb):
                    r0, c0 = a0 + ti * 64, b0 + tj * 64
                    out.append((r0, min(r0 + 64, a1), c0, min(c0 + 64, b1), grp0[a] + ti * 64 // a, grp0[b] + tj * 64 // b, a, b,
                                a == b and ti == tj))
    return out


def compact(facs, m):
    """(columns, Vc, wc) of one block from its factor list [(V, d)] (a stored row: no column) by ragged_columns(max_rank=64)."""
    from loraine_jl_amd.model import ragged_columns
    ranks = [0 if sp.issparse(f) else int(np.count_nonzero(f[1])) for f in facs]
    p = ragged_columns(ranks, max_rank=64)
    Vc, wc = np.zeros((m, p["Rc"])), np.zeros(p["Rc"])
    for col in range(p["Rc"]):
        if p["wc"][col] < 0:
            continue
        V, d = facs[p["gh"][p["cg"][col]]]
        q = np.flatnonzero(d)[p["wc"][col]]
        Vc[:, col], wc[col] = V[:, q], d[q]
    return p, Vc, wc


# ---------------------------------------------------------------------------------------------- the device's order in NumPy
def _tree(x, axis):
    """Balanced pairwise sum along an axis of power-of-two length: the grouping of an xor butterfly."""
    x = np.moveaxis(x, axis, 0)
    while x.shape[0] > 1:
        x = x[0::2] + x[1::2]
    return x[0]


def _block16(S, ka, kb):
    """The ka x kb block sums (ka, kb | 16) of one 16 x 16 accumulator block in the order of the epilogue: element (row kq + 4 r,
    column ci); registers r first (from ka = 8 on), then the columns over neighbouring lanes, then the rows over the lane
    quarters kq.  -> (16 / ka) x (16 / kb)."""
    x = S.reshape(4, 4, 16)                                  # [r][kq][ci]
    if ka >= 8:
        x = np.stack([x[0] + x[1], x[2] + x[3]])
    if ka >= 16:
        x = (x[0] + x[1])[None]
    x = _tree(x.reshape(x.shape[0], 4, 16 // kb, kb), 3)     # [r'][kq][column block]
    kqr = min(ka, 4)
    x = _tree(x.reshape(x.shape[0], 4 // kqr, kqr, 16 // kb), 2)
    return x.reshape(16 // ka, 16 // kb)


def tile_blocks(S, ka, kb, fault=None):
    """Block sums of one 64 x 64 tile of weighted squares (zero beyond the segment ends) in the device's order -> (64 / ka) x
    (64 / kb).  fault: "drop16" leaves out accumulator (1, 1) of wave (0, 0), "acc" the second accumulator of a direction of size
    >= 32, "wave" the second wave of a direction of size 64."""
    ka16, kb16 = min(ka, 16), min(kb, 16)
    kaw, kbw = min(ka, 32), min(kb, 32)
    wave = {}
    for wr in range(2):
        for wn in range(2):
            v = [[None, None], [None, None]]
            for ib in range(2):
                for jb in range(2):
                    r, c = 32 * wr + 16 * ib, 32 * wn + 16 * jb
                    blk = _block16(S[r:r + 16, c:c + 16], ka16, kb16)
                    if fault == "drop16" and (wr, wn, ib, jb) == (0, 0, 1, 1):
                        blk = np.zeros_like(blk)
                    v[ib][jb] = blk
            if ka >= 32:
                v = [[v[0][jb] + (0.0 if fault == "acc" else v[1][jb]) for jb in range(2)]]
            if kb >= 32:
                v = [[row[0] + (0.0 if fault == "acc" else row[1])] for row in v]
            wave[wr, wn] = np.block(v)                       # (32 / kaw) x (32 / kbw)
    if ka == 64:
        wave = {(0, wn): wave[0, wn] + (0.0 if fault == "wave" else wave[1, wn]) for wn in range(2)}
    if kb == 64:
        wave = {(wr, 0): wave[wr, 0] + (0.0 if fault == "wave" else wave[wr, 1]) for wr in range(2) if (wr, 0) in wave}
    rows = sorted({k[0] for k in wave})
    cols = sorted({k[1] for k in wave})
    return np.block([[wave[r, c] for c in cols] for r in rows])


def device_order(facs, m, W, G, n, fault=None):
    """H_FF (n x n, symmetric) of one block by the rank-class route in the device's summation order, float64; pairs counted.
    fault: see tile_blocks; "noskip" adds the blocks gi < gj of the class-32 diagonal tiles as well; "pad" gives the padding
    columns of the first constraint of rank 33 .. 63 non-zero operands and weight 1.  A fault of tile_blocks is planted in the
    first diagonal tile of a wide class."""
    from loraine_jl_amd.model import ragged_plan
    p, Vc, wc = compact(facs, m)
    if fault == "pad":
        g = next(g for g, h in enumerate(p["gh"]) if 32 < np.count_nonzero(facs[h][1]) < 64)
        cols = [c for c in range(p["start"][g], p["start"][g] + p["size"][g]) if p["wc"][c] < 0]
        Vc[:, cols] = np.random.default_rng(9).standard_normal((m, len(cols))) / np.sqrt(m)
        wc[cols] = 1.0
    plan = ragged_plan([0 if sp.issparse(f) else int(np.count_nonzero(f[1])) for f in facs], max_rank=64)
    assert plan["gh"] == p["gh"] and plan["Rc"] == p["Rc"]
    Uc = G.T @ Vc if G is not None else W @ Vc
    Bc = Uc if G is not None else Vc
    H = np.zeros((n, n))
    pairs = {}
    planted = fault in (None, "noskip", "pad")
    for r0, r1, c0, c1, gi0, gj0, ka, kb, diag in tiles(plan):
        S = np.zeros((64, 64))
        T = Uc[:, r0:r1].T @ Bc[:, c0:c1]
        S[:r1 - r0, :c1 - c0] = T * T * np.outer(wc[r0:r1], wc[c0:c1])
        here = None
        if not planted and diag and ka >= (64 if fault == "wave" else 32):
            here, planted = fault, True
        B = tile_blocks(S, ka, kb, here)
        for bi in range((r1 - r0) // ka):
            for bj in range((c1 - c0) // kb):
                gi, gj = gi0 + bi, gj0 + bj
                if diag and gi < gj and not (fault == "noskip" and ka == 32):
                    continue
                hi, hj = p["gh"][gi], p["gh"][gj]
                H[max(hi, hj), min(hi, hj)] += B[bi, bj]
                key = (max(gi, gj), min(gi, gj))
                pairs[key] = pairs.get(key, 0) + 1
    assert planted, "no tile of this case takes the fault %r" % (fault,)
    return np.tril(H) + np.tril(H, -1).T, pairs, len(p["gh"])


# ---------------------------------------------------------------------------------------------- V3 as a CG case
@functools.lru_cache(maxsize=None)
def cg_case():
    """V3 with the spectrum of the CG cases (tests/cg_lowrank_cases.py::build_case): model (oracle MyModel of the materialised
    data), W, G, X_lin, S_lin_inv, right-hand side h = H v, a vector x -- what oracle/cg_reference.py reads."""
    from oracle import cg_reference as cr
    from oracle import loraine_oracle as lo
    m, n = SIZES["V3"]
    rng = np.random.default_rng(3203)
    C0 = rng.standard_normal((m, m))
    A = [[sp.csc_matrix(-(C0 + C0.T) / 2)] + [sp.csc_matrix(a) for a in matrices("V3")[0]]]
    C = c_lin("V3")
    mdl = lo.make_model(A, rng.standard_normal(n), 0.0, rng.standard_normal(C.shape[1]), C)
    W, G = cr.scaling_from_spectrum(cr.spectrum(m, top=4), rng)
    X_lin = np.exp(rng.uniform(-1.0, 1.0, mdl.nlin))
    S_lin_inv = np.exp(rng.uniform(-1.0, 1.0, mdl.nlin))
    case = types.SimpleNamespace(name="V3", model=mdl, W=[W], G=[G], X_lin=X_lin, S_lin_inv=S_lin_inv, h=None,
                                 x=rng.standard_normal(n))
    h = np.zeros(n)
    lo.MyA([W], mdl.AA, mdl.nlin, mdl.C_lin, X_lin, S_lin_inv)(h, rng.standard_normal(n))
    case.h = h
    return case


@functools.lru_cache(maxsize=None)
def cg_model():
    from loraine_jl_amd.model import build_factored_model
    c = cg_case()
    return build_factored_model([sp.csc_matrix(c.model.A[0][0])], [list(items("V3"))], np.asarray(c.model.b, float), 0.0,
                                np.asarray(c.model.d_lin, float), c.model.C_lin, factored_form=1, max_rank=64)


# ---------------------------------------------------------------------------------------------- the planted solve
class PlantedWide(rc.Planted):
    """ragged_cases.Planted with constraints 11 and 42 of rank 24 and constraint 30 of rank 40 among rank 1."""
    WIDE = {11: 24, 42: 24, 30: 40}

    def __init__(self, m=40, n=60, seed=23):
        rng = np.random.default_rng(seed)
        self.m, self.n = m, n
        self.ranks = [self.WIDE.get(k, 1) for k in range(n)]
        self.facs = [rc._dense_factor(rng, m, r) for r in self.ranks]
        Q, _ = np.linalg.qr(rng.standard_normal((m, 2)))
        lam = np.array([1.0, 1.5])
        lam *= np.sqrt(m) / lam.sum()
        X = (Q * lam) @ Q.T
        As = [rc.materialise(f, m) for f in self.facs]
        self.b = -np.array([np.sum(a * X) for a in As])
        self.ystar = 0.1 * rng.standard_normal(n)
        C = np.eye(m) - Q @ Q.T - sum(y * a for y, a in zip(self.ystar, As))
        self.C = 0.5 * (C + C.T)
        self.optimum = float(self.b @ self.ystar)

    def stored_factors(self):
        """The same model with the three wide constraints as stored dense matrices: what a model without `wide` can say."""
        out = list(self.facs)
        for k in self.WIDE:
            out[k] = rc.materialise(self.facs[k], self.m)
        return [out]
