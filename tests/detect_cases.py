"""Seeded inputs of the low-rank detection (csrc/detect.hip, loraine.jl_amd/detect.py) and a float64 NumPy restatement of
its steps.  Not a test module: tests/test_detect_cases_cpu.py checks the cases themselves, tests/test_gpu_detect.py runs them
through the C ABI.

A case is A = Q diag(lam) Q' (Q from a QR, symmetrised), so its exact rank, its inertia and the Frobenius norm of what lies
beyond its kmax largest |lam| are known without an eigensolver."""
import numpy as np

TOL = 5.0e-6            # model.LOWRANK_TOL
RANK_RTOL = 1.0e-12     # the relative cut of model.lowrank_factor
MAX_SWEEPS = 30         # csrc/detect.hip DET_MAX_SWEEPS
ROT_FLOOR = 2.0 ** -60  # csrc/detect.hip: an off-diagonal entry below ROT_FLOOR ||C||_F is left alone
ROT_EPS = 2.0 ** -53    # ... and one below ROT_EPS sqrt|c_pp c_qq| as well


def sketch_width(kmax):
    return kmax + 8


def omega_for(m, kmax, seed=0):
    """The sketch matrix detect.detect_factors draws: m x (kmax + 8) standard normals from Philox(seed)."""
    return np.random.Generator(np.random.Philox(seed)).standard_normal((m, sketch_width(kmax)))


class Case:
    def __init__(self, name, m, lam, seed, rows=None, A=None):
        self.name, self.m = name, m
        lam = np.asarray(lam, dtype=np.float64)
        self.lam = lam
        rng = np.random.default_rng(seed)
        if A is not None:
            self.A = A
        else:
            r = lam.size
            supp = m if rows is None else len(rows)
            Q, _ = np.linalg.qr(rng.standard_normal((supp, r))) if r else (np.zeros((supp, 0)), None)
            sub = (Q * lam) @ Q.T
            sub = 0.5 * (sub + sub.T)
            if rows is None:
                self.A = sub
            else:
                self.A = np.zeros((m, m))
                self.A[np.ix_(rows, rows)] = sub
        self.rank = int(np.count_nonzero(lam))
        self.inertia = (int(np.sum(lam > 0)), int(np.sum(lam < 0)))

    def beyond(self, kmax):
        """Frobenius norm of the part of A beyond its kmax largest |lam|: the best rank-kmax error."""
        a = np.sort(np.abs(self.lam))[::-1]
        return float(np.linalg.norm(a[kmax:]))

    def accepted(self, kmax):
        return self.rank <= kmax


def _signs(r, kind, rng):
    if kind == "pos":
        return np.ones(r)
    if kind == "neg":
        return -np.ones(r)
    s = np.where(np.arange(r) % 2 == 0, 1.0, -1.0)
    return s if r > 1 else np.ones(r)


def _lam(r, kind, rng, lo=0.5, hi=2.0):
    return _signs(r, kind, rng) * rng.uniform(lo, hi, r)


def build_cases():
    """Every case, by name.  Eigenvalues are O(1) (0.5 .. 2) unless the name says otherwise, so a case of
    rank > kmax misses the best rank-kmax approximation by >= 0.5, five orders above TOL."""
    rng = np.random.default_rng(20240)
    cs = []
    kinds = ["pos", "neg", "mixed"]
    # sizes below, at and above l = 24, and one, exactly one and ragged 64-tiles of the residual kernel
    for i, m in enumerate([1, 5, 23, 24, 25, 37, 63, 64, 65, 129, 200]):
        r = min(m, [1, 2, 3][i % 3])
        cs.append(Case(f"m{m}_r{r}", m, _lam(r, kinds[i % 3], rng), 100 + i))
    # sizes around l = 72 for kmax = 64
    for i, m in enumerate([71, 72, 73]):
        cs.append(Case(f"m{m}_r40", m, _lam(40, kinds[i % 3], rng), 120 + i))
    # ranks at m = 200 (and full rank)
    for i, r in enumerate([0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65]):
        cs.append(Case(f"m200_rank{r}", 200, _lam(r, kinds[i % 3], rng), 200 + i))
    cs.append(Case("identity129", 129, np.ones(129), 0, A=np.eye(129)))
    G = np.random.default_rng(7).standard_normal((65, 65))
    spd = G @ G.T / 65 + np.eye(65)
    cs.append(Case("spd65", 65, np.linalg.eigvalsh(spd), 0, A=0.5 * (spd + spd.T)))
    # inputs
    cs.append(Case("graded_r12", 200, _signs(12, "mixed", rng) * np.logspace(0, -6, 12), 300))
    cs.append(Case("graded_r16", 129, np.logspace(0, -6, 16), 301))
    cs.append(Case("scaled_1e3_r4", 200, 1e3 * _lam(4, "mixed", rng), 302))
    cs.append(Case("scaled_1e-3_r4", 200, 1e-3 * _lam(4, "mixed", rng), 303))
    cs.append(Case("repeated_r6", 65, np.array([1.5, 1.5, 1.5, -0.75, -0.75, 1.0]), 304))
    cs.append(Case("support3_r2", 200, np.array([1.25, -0.8]), 305, rows=[7, 64, 199]))
    return {c.name: c for c in cs}


CASES = build_cases()


def cases_for(kmax):
    """Names of the cases run at this kmax: all of them at 16 but the ones of side 71 .. 73, which exist for l = 72; at 64
    the sides 5, 71, 72, 73 and 200 (below, around and above l = 72) and the rank / input cases of side 65 and 129."""
    if kmax == 16:
        return [n for n, c in CASES.items() if c.m not in (71, 72, 73)]
    return [n for n, c in CASES.items() if c.m in (5, 71, 72, 73, 200) or n in ("identity129", "spd65", "graded_r16",
                                                                              "repeated_r6", "m65_r3")]


def batch(names):
    """Cases of one side stacked as the C ABI takes them: cnt x m x m (every matrix symmetric: row- or column-major alike)."""
    return np.stack([CASES[n].A for n in names])


BATCH3 = {200: ("graded_r12", "m200_rank17", "m200_rank1"), 65: ("spd65", "m65_r3", "repeated_r6")}


def batch3(m):
    """A mixed batch of exactly 3 constraints of side m (200: graded and accepted, rank 17, rank 1; 65: full rank, rank 3 with
    mixed signs, a repeated eigenvalue), as names."""
    return list(BATCH3[m])


def batch70():
    """70 constraints of side 200 mixing all kinds (names repeat)."""
    pool = [n for n, c in CASES.items() if c.m == 200]
    return [pool[(3 * i + i // 7) % len(pool)] for i in range(70)]


# ---------------------------------------------------------------------------------------------- the restatement
def round_robin(l, step):
    """The l / 2 disjoint pairs of step `step` (0 .. l - 2) of the tournament ordering, l even (csrc/detect.hip::rr_pair)."""
    pairs = [(l - 1, step)]
    for k in range(1, l // 2):
        pairs.append(((step + k) % (l - 1), (step - k) % (l - 1)))
    return [(min(p, q), max(p, q)) for p, q in pairs]


def jacobi_eig(C, skip_pair=None):
    """Cyclic two-sided Jacobi, round-robin ordering, as the device kernel runs it -> (lam, U, sweeps)."""
    C = C.copy()
    l = C.shape[0]
    U = np.eye(l)
    floor = ROT_FLOOR * np.linalg.norm(C)
    sweeps = 0
    while sweeps < MAX_SWEEPS:
        rotated = 0
        for step in range(l - 1):
            J = np.eye(l)
            done = []
            for p, q in round_robin(l, step):
                if (p, q) == skip_pair:
                    continue
                x = C[p, q]
                if not (abs(x) > floor and abs(x) > ROT_EPS * np.sqrt(abs(C[p, p]) * abs(C[q, q]))):
                    continue
                tau = (C[q, q] - C[p, p]) / (2.0 * x)
                t = (1.0 if tau >= 0 else -1.0) / (abs(tau) + np.hypot(1.0, tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                J[p, p] = J[q, q] = c
                J[p, q], J[q, p] = s, -s
                done.append((p, q))
            if done:
                C = J.T @ C @ J
                U = U @ J
                for p, q in done:
                    C[p, q] = C[q, p] = 0.0
                rotated += len(done)
        sweeps += 1
        if rotated == 0:
            break
    return np.diag(C).copy(), U, sweeps


def tile_residual(A, V, d, once=False):
    """||A - V D V'||_F summed as the residual kernel does: 64 x 64 tiles on and below the diagonal, off-diagonal tiles
    twice (once=True plants the fault that counts them once)."""
    m = A.shape[0]
    R = A - (V * d) @ V.T
    nt = (m + 63) // 64
    tot = 0.0
    for ti in range(nt):
        for tj in range(ti + 1):
            s = float(np.sum(R[64 * ti:64 * ti + 64, 64 * tj:64 * tj + 64] ** 2))
            tot += s if (ti == tj or once) else 2.0 * s
    return float(np.sqrt(tot))


def restate(A, omega, kmax, tol=TOL, rank_rtol=RANK_RTOL, fault=None):
    """The Nystrom steps of csrc/detect.hip in float64 NumPy -> dict(rank, resid, V (m x kmax), d (kmax), sweeps).
    fault: None, or one of "sign", "inverse", "unsym", "skip", "once", "cut" (tests/test_detect_cases_cpu.py)."""
    m = A.shape[0]
    Y = A @ omega
    C = np.tril(omega.T @ Y)              # the core step forms the entries on and below the diagonal only
    if fault != "unsym":
        C = C + np.tril(C, -1).T          # ... and the eigensolver mirrors them
    lam, U, sweeps = jacobi_eig(C, skip_pair=(0, 1) if fault == "skip" else None)
    mx = float(np.max(np.abs(lam))) if lam.size else 0.0
    big = (lam > rank_rtol * mx) if fault == "cut" else (np.abs(lam) > rank_rtol * mx)
    r = int(np.count_nonzero(big))
    V = np.zeros((m, kmax))
    d = np.zeros(kmax)
    if r > kmax:
        return dict(rank=-1, resid=tile_residual(A, V, d, once=fault == "once"), V=V, d=d, sweeps=sweeps)
    idx = np.nonzero(big)[0]
    scale = 1.0 / np.abs(lam[idx]) if fault == "inverse" else 1.0 / np.sqrt(np.abs(lam[idx]))
    V[:, :r] = Y @ (U[:, idx] * scale)
    d[:r] = np.sign(lam[idx])
    if fault == "sign" and r:
        d[0] = -d[0]
    resid = tile_residual(A, V, d, once=fault == "once")
    return dict(rank=r if resid <= tol else -1, resid=resid, V=V, d=d, sweeps=sweeps)
