"""Seeded cases of WIDE factored blocks (constraints of rank 17 .. 64, khat 32 or 64) that carry diagonal parts, A_k = diag(a_k) +
V_k D_k V_k' (library option wide_diag beside lowrank_wide, load_factored_model(..., wide="diag"); csrc/diagops.hip:
diag_sq_wide_mfma_kernel), built on tests/wide_cases.py, tests/ragged_cases.py and tests/diag_factored_cases.py.  Shared by
tests/test_wide_diag_cpu.py and tests/test_gpu_wide_diag.py; everything is cached and left unchanged.

    D32   37 / 5     V1's factors (all rank 32), a diagonal part (dfc._diagonal: zeros and negatives) on every constraint: kh 32,
                     nc = 160 = 2.5 tiles (the last one half full), K tail of 5, 5 rows (below the auto threshold of the MFMA form)
    D64   70 / 16    V2's ranks 64, 40, 33, 32, 17, 25, 16, 9, 8, 5, 4, 3, 2, 1, 1, 0; diagonal parts on the constraints of rank 64,
                     33, 17 and one of rank 1 (13); constraint 15 (rank 0) is the pure trace row (None, [], ones): kh 64 padded; by
                     class under ragged_cross: class 64 three groups, class 32 three groups on 96 columns (a half-full tile, stored
                     through hmap), the narrow classes beside them; K tail of 6
    DE63 / DE64 / DE65   65 / 70, khat 32: 63, 64, 65 leading diagonal rows (the row-tile edge of diag_factored_cases.CASES (65,
                     70, 4, .)), ranks 0 .. 32 mixed, every fourth constraint of rank 32: the MFMA form by the auto rule
    DH    45 / 12    V3: a stored sparse trace row, a stored full matrix (a dense slot), two linear rows; diagonal parts on the
                     constraints of rank 48 (2) and 20 (3); the rank-1 constraint 7 replaced by (None, [], ones): the stored x
                     diagonal term, the cross terms, the CG path
    D2B   37 + 20 / 5   D32 beside V4b's block of khat 2 with diagonal parts on its constraints 1 and 4: kh per block
    PlantedWideDiag  msz 40 / nvar 60: wide_cases.PlantedWide with constraint 0 replaced by the trace row (None, [], ones)

c_device_order() restates C = Ad' (Y o Y) with the summation order of the wide epilogue in NumPy float64 -- blocks of 16 columns
by balanced trees (the lane butterfly), then accumulator 0 + 1 of the wave, then wave 0 + 1 for a group of 64 --, padded (kh 32 /
64) and per class (class sizes 64 .. 1 through the group map), and plants single faults on request."""
import functools
import types

import numpy as np
import scipy.sparse as sp

import diag_factored_cases as dfc
import ragged_cases as rc
import wide_cases as wc

LD = np.longdouble
NAMES = ["D32", "D64", "DE63", "DE64", "DE65", "DH", "D2B"]
SINGLE = ["D32", "D64", "DE63", "DE64", "DE65", "DH"]
DE_SHAPE = (65, 70, 32)
SIZES = {"D32": wc.SIZES["V1"], "D64": wc.SIZES["V2"], "DH": wc.SIZES["V3"], "D2Bn": wc.SIZES["V4b"],
         "DE63": DE_SHAPE[:2], "DE64": DE_SHAPE[:2], "DE65": DE_SHAPE[:2]}
D64_DIAG = (0, 2, 4, 13)          # ranks 64, 33, 17, 1
D64_TRACE = 15                    # rank 0
DH_DIAG = (2, 3)                  # ranks 48, 20
DH_TRACE = 7                      # a rank-1 constraint
D2B_NARROW_DIAG = (1, 4)


@functools.lru_cache(maxsize=None)
def items(name):
    """The constraint list of a single block, as build_factored_model takes it."""
    if name == "D32":
        m = SIZES[name][0]
        return tuple((V, d, dfc._diagonal(m, 3200 + k)) for k, (V, d) in enumerate(wc.items("V1")))
    if name == "D64":
        m = SIZES[name][0]
        out = list(wc.items("V2"))
        for k in D64_DIAG:
            out[k] = (out[k][0], out[k][1], dfc._diagonal(m, 6400 + k))
        out[D64_TRACE] = (None, [], np.ones(m))
        return tuple(out)
    if name.startswith("DE"):
        m, n, khat = DE_SHAPE
        out = list(dfc._factors(m, n, khat, 6570))
        for k in range(int(name[2:])):
            out[k] = (out[k][0], out[k][1], dfc._diagonal(m, 6570 + 7 * k + 1))
        return tuple(out)
    if name == "DH":
        m = SIZES[name][0]
        out = list(wc.items("V3"))
        for k in DH_DIAG:
            out[k] = (out[k][0], out[k][1], dfc._diagonal(m, 4500 + k))
        out[DH_TRACE] = (None, [], np.ones(m))
        return tuple(out)
    if name == "D2Bn":
        m = SIZES[name][0]
        out = list(wc.items("V4b"))
        for k in D2B_NARROW_DIAG:
            out[k] = (out[k][0], out[k][1], dfc._diagonal(m, 2000 + k))
        return tuple(out)
    raise KeyError(name)


def blocks(name):
    return [list(items("D32")), list(items("D2Bn"))] if name == "D2B" else [list(items(name))]


def nvar(name):
    return SIZES["D32" if name == "D2B" else name][1]


def msizes(name):
    return [SIZES["D32"][0], SIZES["D2Bn"][0]] if name == "D2B" else [SIZES[name][0]]


def c_lin(name):
    return wc.c_lin("V3") if name == "DH" else None


def diag_rows(name):
    """Per block the sorted constraints with a diagonal part."""
    return [sorted(k for k, it in enumerate(blk) if isinstance(it, tuple) and len(it) == 3) for blk in blocks(name)]


@functools.lru_cache(maxsize=None)
def scaling(name):
    """[(W, G)] per block: ragged_cases.spd with the seeds of wide_cases.scaling (D32, D64, DH, D2B: the W of V1, V2, V3, V4,
    cond 4e2 .. 5e3); DE: seed 6570 (cond 4.9e3 -- seed 2065 of that rule gives 8.8e4, outside the range the other cases keep)."""
    if name.startswith("DE"):
        return [rc.spd(DE_SHAPE[0], 6570)]
    return [rc.spd(m, 2000 + 10 * i + m) for i, m in enumerate(msizes(name))]


@functools.lru_cache(maxsize=None)
def matrices(name):
    """Materialised constraints per block."""
    return [[rc.materialise(it, m) for it in blk] for blk, m in zip(blocks(name), msizes(name))]


@functools.lru_cache(maxsize=None)
def reference(name):
    """H_ij = sum over blocks of tr(A_i W A_j W) in np.longdouble (+ C_lin C_lin' for DH: unit X_lin, S_lin_inv), natural order."""
    n = nvar(name)
    H = np.zeros((n, n), dtype=LD)
    for As, (W, _) in zip(matrices(name), scaling(name)):
        H += rc._h_block(As, W, LD)
    C = c_lin(name)
    if C is not None:
        Cd = C.toarray().astype(LD)
        H += Cd @ Cd.T
    return H


def _build(blks, ms, n, C=None, F0=None, b=None, d_lin=None, **kw):
    from loraine_jl_amd.model import build_factored_model
    F0 = [-np.eye(m) for m in ms] if F0 is None else F0
    if C is not None and d_lin is None:
        d_lin = np.ones(C.shape[1])
    return build_factored_model(F0, blks, np.zeros(n) if b is None else b, 0.0, d_lin, C, factored_form=1, **kw)


@functools.lru_cache(maxsize=None)
def model(name):
    return _build(blocks(name), msizes(name), nvar(name), c_lin(name), max_rank=64, wide_diag=True)


@functools.lru_cache(maxsize=None)
def block_model(name):
    """One block of D2B as a model of its own ("D32" or "D2Bn")."""
    return _build([list(items(name))], [SIZES[name][0]], SIZES[name][1], max_rank=64, wide_diag=True)


@functools.lru_cache(maxsize=None)
def stored_model(name):
    """The same constraints with every (V, d, a) item as a stored sparse matrix beside wide=True: the only form the model had
    before wide_diag."""
    return _build([dfc.diag_as_stored(blk) for blk in blocks(name)], msizes(name), nvar(name), c_lin(name), max_rank=64)


# ---------------------------------------------------------------------------------------------- the device's order in NumPy
def _group_sum(x, fault=None):
    """Sum of the weighted columns of one group (rows x size, size a class size) in the order of the epilogue: size <= 16 one
    balanced tree (the butterfly over size neighbouring lanes); 32: two blocks of 16, accumulator 0 + 1; 64: two waves of 32,
    wave 0 + 1.  fault "acc": the second accumulator of a 32 dropped, "wave": the second wave of a 64."""
    size = x.shape[1]
    if size <= 16:
        return wc._tree(x, 1)
    if size == 32:
        a0, a1 = wc._tree(x[:, :16], 1), wc._tree(x[:, 16:], 1)
        return a0 if fault == "acc" else a0 + a1
    w0, w1 = _group_sum(x[:, :32]), _group_sum(x[:, 32:])
    return w0 if fault == "wave" else w0 + w1


def _fac_pairs(blk, m):
    """[(V, d)] per constraint: a stored constraint and a purely diagonal one have no column."""
    out = []
    for it in blk:
        if not isinstance(it, tuple) or it[0] is None:
            out.append((np.zeros((m, 0)), np.zeros(0)))
        else:
            out.append((np.asarray(it[0], float).reshape(m, -1), np.asarray(it[1], float)))
    return out


def c_device_order(blk, m, W, layout, fault=None):
    """C[s, h] = sum_p d_hp sum_i a_si Y[i, hp]^2 of one block (rows = its diagonal rows in ascending order, h = constraint) in
    float64 with the device's summation order over a column group.  layout "padded": every constraint on khat columns, khat the
    power of two >= the largest rank (32 or 64 here: the wide kernel; the narrow kernel's butterfly for <= 16); "class": the
    compacted columns of ragged_columns(max_rank=64), one launch per class, stored through the group map gh.
    fault: "acc" / "wave" -- the first group of size 32 / 64 loses its second accumulator / wave; "pad" -- the padding columns
    of the first group that has some get weight 1 and a non-zero operand; "half" -- the group behind the last one of a half-full
    tile (a class-32 segment, or the padded layout at kh 32, of an odd number of groups) is written with its zero sum, at the
    address the kernel would compute; "hmap" -- the group map of class 32 shifted by one group."""
    from loraine_jl_amd.model import padded_rank, ragged_columns
    n = len(blk)
    rows = [k for k, it in enumerate(blk) if isinstance(it, tuple) and len(it) == 3]
    Ad = np.column_stack([np.asarray(blk[k][2], float) for k in rows])
    facs = _fac_pairs(blk, m)
    ranks = [int(np.count_nonzero(d)) for _, d in facs]
    C = np.zeros((len(rows), n))
    planted = fault is None
    rng = np.random.default_rng(9)
    if layout == "padded":
        kh = padded_rank(max(max(ranks), 1))
        groups = []
        for h, (V, d) in enumerate(facs):
            Vp, wp = np.zeros((m, kh)), np.zeros(kh)
            Vp[:, :V.shape[1]], wp[:d.size] = V, d
            groups.append((h, Vp, wp))
        segs = [(kh, groups, list(range(n)))]
    else:
        p = ragged_columns(ranks, max_rank=64)
        segs = []
        for cs in wc.WIDE_CLASSES:
            gs = [g for g in range(len(p["gh"])) if p["size"][g] == cs]
            groups = []
            for g in gs:
                h = p["gh"][g]
                V, d = facs[h]
                q = np.flatnonzero(d)
                Vp, wp = np.zeros((m, cs)), np.zeros(cs)
                Vp[:, :q.size], wp[:q.size] = V[:, q], d[q]
                groups.append((h, Vp, wp))
            if groups:
                segs.append((cs, groups, p["gh"]))
    flat = C.reshape(-1)                                     # C as the device addresses it: row s at s * n
    for cs, groups, hmap_all in segs:
        hmap = [h for h, _, _ in groups]
        if fault == "hmap" and cs == 32 and not planted:
            hmap = hmap[1:] + hmap[:1]
            planted = True
        for g, (h, Vp, wp) in enumerate(groups):
            here = None
            if not planted and fault == "pad" and np.any(wp == 0.0) and cs >= 32:
                pad = np.flatnonzero(wp == 0.0)
                Vp, wp = Vp.copy(), wp.copy()
                Vp[:, pad] = rng.standard_normal((m, pad.size)) / np.sqrt(m)
                wp[pad] = 1.0
                planted = True
            if not planted and ((fault == "acc" and cs == 32) or (fault == "wave" and cs == 64)):
                here, planted = fault, True
            Y = W @ Vp
            S = (Ad.T @ (Y * Y)) * wp[None, :]               # rows x cs: the weighted accumulator elements
            C[:, hmap[g]] = _group_sum(S, here)
        if fault == "half" and not planted and cs == 32 and len(groups) % 2 == 1:
            # the wave wc = 1 of the last tile holds group len(groups): its store goes to D[s ldd + (hmap ? hmap[g] : g)]
            g = len(groups)
            if layout == "padded":
                tgt = g                                      # (no map: column n of row s = column 0 of row s + 1)
            else:
                at = hmap_all.index(hmap[-1]) + 1            # the map is read one behind the class: the next class's first group
                tgt = hmap_all[at] if at < len(hmap_all) else n
            for s in range(len(rows)):
                if s * n + tgt < flat.size:
                    flat[s * n + tgt] = 0.0
            planted = True
    assert planted, "no group of this case takes the fault %r" % (fault,)
    return rows, Ad, C


def h_device_order(name, layout, fault=None):
    """H (natural order, symmetric) of a case by the formulas of the device: H_SS, H_FF and the cross terms of the stored rows as
    dfc.h_formulas forms them from the items without their diagonal parts; H_DD = Ad' (W o W) Ad; C + C' with C from
    c_device_order (the fault, if any, in block 0); stored rows against diagonal rows a_k' diag(W A_s W); + C_lin C_lin'."""
    n = nvar(name)
    H = np.zeros((n, n))
    for ib, (blk, m, (W, _)) in enumerate(zip(blocks(name), msizes(name), scaling(name))):
        bare = [(np.zeros((m, 0)) if it[0] is None else it[0], it[1]) if isinstance(it, tuple) and len(it) == 3 else it
                for it in blk]
        H += dfc.h_formulas(bare, W)
        rows, Ad, C = c_device_order(blk, m, W, layout, fault if ib == 0 else None)
        H[np.ix_(rows, rows)] += Ad.T @ (W * W) @ Ad
        for a, k in enumerate(rows):
            H[k, :] += C[a]
            H[:, k] += C[a]
        for s, it in enumerate(blk):
            if isinstance(it, tuple):
                continue
            ts = np.diag(W @ dfc.dense_of(it) @ W)
            for a, k in enumerate(rows):
                H[s, k] += Ad[:, a] @ ts
                H[k, s] += Ad[:, a] @ ts
    Cl = c_lin(name)
    if Cl is not None:
        Cd = Cl.toarray()
        H += Cd @ Cd.T
    return H


# ---------------------------------------------------------------------------------------------- CG cases: DH and D64
CG_NAMES = ["DH", "D64"]
CG_SEEDS = {"DH": 4503, "D64": 7003}


@functools.lru_cache(maxsize=None)
def cg_case(name):
    """DH / D64 with the spectrum of the CG cases (wide_cases.cg_case): the oracle MyModel of the materialised data, W, G, X_lin,
    S_lin_inv, right-hand side h = H v, a vector x -- what oracle/cg_reference.py reads."""
    from oracle import cg_reference as cr
    from oracle import loraine_oracle as lo
    m, n = SIZES[name]
    rng = np.random.default_rng(CG_SEEDS[name])
    C0 = rng.standard_normal((m, m))
    A = [[sp.csc_matrix(-(C0 + C0.T) / 2)] + [sp.csc_matrix(a) for a in matrices(name)[0]]]
    C = c_lin(name)
    mdl = lo.make_model(A, rng.standard_normal(n), 0.0, None if C is None else rng.standard_normal(C.shape[1]), C)
    W, G = cr.scaling_from_spectrum(cr.spectrum(m, top=4), rng)
    X_lin = np.exp(rng.uniform(-1.0, 1.0, mdl.nlin))
    S_lin_inv = np.exp(rng.uniform(-1.0, 1.0, mdl.nlin))
    case = types.SimpleNamespace(name=name, model=mdl, W=[W], G=[G], X_lin=X_lin, S_lin_inv=S_lin_inv, h=None,
                                 x=rng.standard_normal(n))
    h = np.zeros(n)
    lo.MyA([W], mdl.AA, mdl.nlin, mdl.C_lin, X_lin, S_lin_inv)(h, rng.standard_normal(n))
    case.h = h
    return case


@functools.lru_cache(maxsize=None)
def cg_data(name):
    """(case, dense longdouble H of the materialised model)."""
    from oracle import cg_reference as cr
    case = cg_case(name)
    return case, cr.dense_operator(case.model, case.W, case.X_lin, case.S_lin_inv)


@functools.lru_cache(maxsize=None)
def cg_run(name):
    """The reference run with H_alpha, erank 1: history, the iteration K the tests stop in and its tolerance."""
    from oracle import cg_reference as cr
    case, H = cg_data(name)
    return cr.reference_run(case, H, 1, 1)


@functools.lru_cache(maxsize=None)
def cg_model(name):
    c = cg_case(name)
    return _build([list(items(name))], [SIZES[name][0]], SIZES[name][1], c.model.C_lin if c.model.nlin else None,
                  F0=[sp.csc_matrix(c.model.A[0][0])], b=np.asarray(c.model.b, float),
                  d_lin=np.asarray(c.model.d_lin, float) if c.model.nlin else None, max_rank=64, wide_diag=True)


# ---------------------------------------------------------------------------------------------- the planted solve
class PlantedWideDiag(wc.PlantedWide):
    """wide_cases.PlantedWide with constraint 0 replaced by the trace row, given as (None, [], ones): tr X* = sqrt(msz) fixes b_0."""
    TRACE = 0

    def __init__(self, m=40, n=60, seed=23):
        rng = np.random.default_rng(seed)
        self.m, self.n = m, n
        self.ranks = [self.WIDE.get(k, 1) for k in range(n)]
        self.facs = [rc._dense_factor(rng, m, r) for r in self.ranks]
        self.ranks[self.TRACE] = 0
        self.facs[self.TRACE] = (None, [], np.ones(m))
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

    def stored_trace_factors(self):
        """The same model with the trace row as a stored sparse identity: what wide=True alone can say."""
        out = list(self.facs)
        out[self.TRACE] = sp.identity(self.m, format="csc")
        return [out]
