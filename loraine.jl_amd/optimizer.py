"""`Optimizer`: the user-facing surface of the reference (`Loraine.Optimizer`,
src/MOI_wrapper.jl:42-354) with the same 15 raw attribute names, status mapping and getters,
driving the MI355X hot path.  MathOptInterface itself is a Julia package; this mirrors the
calls a JuMP user makes:

    set_optimizer(model, Loraine.Optimizer)      ->  opt = Optimizer()
    set_attribute(model, "kit", 0)               ->  opt.set_attribute("kit", 0)
    read_from_file(".../theta1.dat-s")           ->  opt.read_from_file(path)
    optimize!(model)                             ->  opt.optimize()
    objective_value(model)                       ->  opt.objective_value()
"""
import numpy as np

from . import solvers
from .model import MyModel, build_factored_model, build_model, check_diag_kit, check_factored_kit, model_from_sdpa

# MOI.TerminationStatus values used by the reference (MOI_wrapper.jl:252-265)
OPTIMIZE_NOT_CALLED = "OPTIMIZE_NOT_CALLED"
OPTIMAL = "OPTIMAL"
INFEASIBLE = "INFEASIBLE"
INFEASIBLE_OR_UNBOUNDED = "INFEASIBLE_OR_UNBOUNDED"
ITERATION_LIMIT = "ITERATION_LIMIT"
FEASIBLE_POINT, INFEASIBLE_POINT, UNKNOWN_RESULT_STATUS, NO_SOLUTION = (
    "FEASIBLE_POINT", "INFEASIBLE_POINT", "UNKNOWN_RESULT_STATUS", "NO_SOLUTION")


class UnsupportedAttribute(KeyError):
    """MOI.UnsupportedAttribute (MOI_wrapper.jl:90-94)."""


class Optimizer:
    def __init__(self, device=None, device_index=0, resident=True, exact_regularised_solve=False):
        # resident=True: X, S and all msz x msz work stay on the device (resident.ResidentSolver);
        # resident=False: step-length search / convergence test in host NumPy (solvers.MySolver)
        self.resident = resident
        # False (default): regularised iterations solve twice, like the reference (src/predictor_corrector.jl:85,90);
        # True: (H + d I)^-1 h.  Not one of the reference's 15 options -- a constructor argument.
        self.exact_regularised_solve = bool(exact_regularised_solve)
        self.solver = None
        self.halpha = None
        self.max_sense = False
        self.silent = False
        self.options = dict(solvers.DEFAULT_OPTIONS)
        self._device = device
        self._device_index = device_index
        self._pending = None
        self._local_support = False
        self._long_rows = False

    # ---- MOI.RawOptimizerAttribute (MOI_wrapper.jl:86-103)
    def supports(self, name):
        return name in solvers.DEFAULT_OPTIONS

    def set_attribute(self, name, value):
        if not self.supports(name):
            raise UnsupportedAttribute(name)
        self.options[name] = value

    def get_attribute(self, name):
        if not self.supports(name):
            raise UnsupportedAttribute(name)
        return self.options[name]

    def set_silent(self, flag=True):          # MOI.Silent (:107-114)
        self.silent = bool(flag)

    def solver_name(self):
        return "Loraine"

    # ---- model input (copy_to, :142-232): options are frozen here, like in the reference (:224)
    def read_from_file(self, path, detect_kmax=None, local_support=False, long_rows=False):
        """detect_kmax = 16 or 64: the constraint matrices of the file go through load_detected_model(kmax=detect_kmax) with
        its defaults; None (default): the file is loaded as it always was.
        local_support: as in load_model (the file loaded as it always was: detect_kmax=None).
        long_rows: as in load_model, with either way of loading the file."""
        self._local_support = self._check_flag("read_from_file", "local_support", local_support)
        self._long_rows = self._check_flag("read_from_file", "long_rows", long_rows)
        if detect_kmax is None:
            self._pending = ("sdpa", path)
            return self
        if self._local_support:
            raise ValueError("read_from_file: local_support=True goes with detect_kmax=None (stored constraints)")
        if not self.resident:
            raise ValueError(self._NEEDS_RESIDENT)
        if isinstance(detect_kmax, bool) or detect_kmax not in (16, 64):
            raise ValueError(f"read_from_file: detect_kmax is None, 16 or 64, not {detect_kmax!r}")
        self._pending = ("sdpa_detected", (path, dict(self._DETECT_DEFAULTS, kmax=int(detect_kmax))))
        return self

    @staticmethod
    def _check_flag(who, name, value):
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError(f"{who}: {name} is False or True, not {value!r}")
        return bool(value)

    @staticmethod
    def _check_cg_ragged(who, cg, ragged):
        """cg: False, True or "diag"; ragged: False, True, "ops" or "all" -> (cg_diag, ragged as the model holds it)"""
        cg_diag = isinstance(cg, str) and cg == "diag"
        if isinstance(cg, str) and not cg_diag:
            raise ValueError(f"{who}: cg is False, True or \"diag\", not {cg!r}")
        if isinstance(ragged, str) and ragged not in ("ops", "all"):
            raise ValueError(f"{who}: ragged is False, True, \"ops\" or \"all\", not {ragged!r}")
        return cg_diag, ragged if isinstance(ragged, str) else bool(ragged)

    def load_model(self, A, b, b_const=0.0, d_lin=None, C_lin=None, max_sense=False, factors=None, local_support=False,
                   long_rows=False):
        """Problem in the reference's own form: max/min over y with LMIs sum_j y_j A_ij - A_i0 >= 0
        given as A[i] = [F_0, F_1, ..., F_n] and rows  C_lin' y <= d_lin.
        factors (optional): factors[i][k] = (V, d) with A[i][k + 1] = V diag(d) V' (V msz x r, r <= 16, d = +-1), used
        instead of the factors datarank >= 1 would compute; checked against A (||A - V D V'||_F <= 5e-6, else ValueError).
        local_support=True (opt-in): stored constraints that touch at most 32 rows and columns and are dense there -- element
        matrices of a finite-element model -- are assembled from A[S, S] on their supports S instead of entry pair by entry
        pair (library option pair_local); one GPU, kit = 0 and kit = 1 (where the CG operator goes through the assembled
        Schur matrix).  Every other constraint keeps its route.
        long_rows=True (opt-in): long sparse stored constraints -- a trace row, a weighted-trace row diag(a), a band: hundreds of
        entries on up to msz rows, kept sparse -- are assembled from Z = (A W) on their rows, sliced over workgroups, instead of
        on one wavefront per pair (library option pair_long); one GPU, kit = 0 and kit = 1.  Independent of local_support: both
        may be on, and where both could take a constraint local_support keeps it."""
        self._local_support = self._check_flag("load_model", "local_support", local_support)
        self._long_rows = self._check_flag("load_model", "long_rows", long_rows)
        self._pending = ("arrays", (A, np.asarray(b, float), float(b_const), d_lin, C_lin, bool(max_sense), factors))
        return self

    def load_factored_model(self, F0, factors, b, b_const=0.0, d_lin=None, C_lin=None, max_sense=False, factored_form=-1,
                            cg=False, ragged=False, wide=False, long_rows=False):
        """The same problem given by its factors alone: F0[i] the constant matrix of block i (the A[i][0] of load_model),
        factors[i][k] = (V, d) with A_i,k+1 = V diag(d) V' (V msz x r, r <= 16 -- r <= 64 with wide=True --, d = +-1, dense or
        sparse).  No A_ik, no row of AA and no dense constraint slab is ever formed, on the host or on the device; implies datarank = the
        largest rank (at least 1) and needs kit = 0 and the resident solver (ValueError otherwise).
        cg=True admits kit = 1 as well (opt-in): the CG operator runs from the factors or through H assembled from them, ts of
        H_alpha comes from the factors (library option cg_factored); one GPU only.
        factors[i][k] may instead be a symmetric msz x msz matrix (SciPy sparse or a 2-D array): that constraint is stored
        as a matrix -- a trace row, a few sparse side constraints among thousands of factored ones (a hybrid block; the
        others stay factors, nothing else is materialised).
        factors[i][k] may also be a triple (V, d, a): A_i,k+1 = V diag(d) V' + diag(a), a of length msz (V = None, d = [] for a
        purely diagonal constraint -- the trace row tr X = 1 is (None, [], ones(msz))).  No entry list is formed for it; needs
        kit = 0, also with cg=True (ValueError otherwise).  cg="diag" is cg=True and admits kit = 1 on such a model as well
        (opt-in: library option cg_diag beside cg_factored -- ts of H_alpha gets the term of the diagonal parts); one GPU only.
        ragged=True (opt-in): the Schur assembly groups the constraints of a factored block by rank class instead of padding all
        of them to the largest rank (library option lowrank_ragged) -- for blocks of mixed ranks, a few constraints of rank 9
        beside thousands of rank 1; a block of uniform rank and a sharded run keep the padded route.
        ragged="ops" is ragged=True and moves the two data operators of such a block, AA vec(.) and mat(AA' .), to the same
        compacted columns (library option ragged_ops beside lowrank_ragged).
        ragged="all" is ragged="ops" and moves what else walked the padded columns there too: Y = W V with the cross terms of
        stored constraints and diagonal parts in the assembly, and ts of H_alpha (library options ragged_cross and ragged_ts).
        wide=True (opt-in): a constraint may carry up to 64 weighted factor columns -- factor-model covariances with 20 to 60
        factors -- instead of going in as a stored matrix (library option lowrank_wide).  A block that holds a constraint of
        rank above 16 is padded to 32 or 64 columns and is always assembled by rank class, whatever `ragged` says; it carries no
        diagonal part (V, d, a) (ValueError: store that row as a sparse matrix instead); one GPU only.  Combines freely with
        ragged= and cg=.
        wide="diag" (opt-in) is wide=True and lifts that refusal: a wide block may hold (V, d, a) items, so B S B' + diag(psi)
        with 17 .. 64 factors and a trace row (None, [], ones) beside it go in as factors and diagonal rows (library option
        wide_diag beside lowrank_wide).  Combines with ragged= and cg= as wide=True does; kit = 1 on such a model needs cg="diag".
        factored_form: -1 (auto) materialises a block whose factors are tiny -- sum_k nnz(V_k V_k') at most datasparsity
        times the number of constraints -- as sparse AA, the existing path; 1 keeps every block factored.
        long_rows=True (opt-in): as in load_model, for the stored matrices of a hybrid block (H_SS of a stored trace row)."""
        self._long_rows = self._check_flag("load_factored_model", "long_rows", long_rows)
        if not isinstance(wide, bool) and not (isinstance(wide, str) and wide == "diag"):
            raise ValueError(f"load_factored_model: wide is False or True (or \"diag\"), not {wide!r}")
        if not self.resident:
            raise ValueError(self._NEEDS_RESIDENT)
        cg_diag, ragged = self._check_cg_ragged("load_factored_model", cg, ragged)
        self._pending = ("factored", (F0, factors, np.asarray(b, float), float(b_const), d_lin, C_lin, bool(max_sense),
                                      int(factored_form), ragged, wide, cg_diag, bool(cg)))
        return self

    _NEEDS_RESIDENT = ("a factored model needs the resident solver (Optimizer(resident=True)): the NumPy host loop "
                       "multiplies by AA")
    _DETECT_DEFAULTS = dict(kmax=16, max_stored=16, cg=False, cg_diag=False, ragged=False, factored_form=-1, budget_mb=None,
                            seed=0, host_side=None)

    def load_detected_model(self, A, b, b_const=0.0, d_lin=None, C_lin=None, max_sense=False, kmax=16, max_stored=16,
                            cg=False, ragged=False, factored_form=-1, budget_mb=None, seed=0, host_side=None, long_rows=False):
        """The problem of load_model, given as matrices, solved as load_factored_model would solve it: every constraint matrix
        that is V diag(d) V' with at most kmax columns becomes a factor, the others stay stored matrices beside them (hybrid
        blocks).  The factors are found when the model goes to the device (detect.detect_factors: the device for dense
        constraints, batched in chunks of budget_mb MiB; the host's eigh for supports of side <= host_side, default 96;
        constraints of at most `datasparsity` non-zeros stay stored without a look), never by an eigh per dense constraint.
        kmax: 16, or 64 (implies wide=True of load_factored_model: ranks 17 .. 64 become factors too).
        cg, ragged, factored_form: as in load_factored_model, with the same checks (kit = 1 needs cg=True).
        Fallback: the whole model takes the general path -- build_model, bit for bit what load_model does -- when no constraint
        was accepted, or when some block would keep more than max_stored stored constraints with more than `datasparsity`
        non-zeros; `detect_report` of the optimizer and `lowrank_note` of the model say which route was taken and why.
        long_rows=True (opt-in): as in load_model, for the constraints that stay stored matrices."""
        self._long_rows = self._check_flag("load_detected_model", "long_rows", long_rows)
        if not self.resident:
            raise ValueError(self._NEEDS_RESIDENT)
        if isinstance(kmax, bool) or kmax not in (16, 64):
            raise ValueError(f"load_detected_model: kmax is 16 or 64, not {kmax!r}")
        if isinstance(max_stored, bool) or not isinstance(max_stored, (int, np.integer)) or max_stored < 0:
            raise ValueError(f"load_detected_model: max_stored is a count >= 0, not {max_stored!r}")
        cg_diag, ragged = self._check_cg_ragged("load_detected_model", cg, ragged)
        if factored_form not in (-1, 1):
            raise ValueError(f"factored_form = {factored_form} (-1 auto, 1 always factored)")
        if budget_mb is not None and not budget_mb > 0:
            raise ValueError(f"load_detected_model: budget_mb is a size in MiB > 0 (or None), not {budget_mb!r}")
        for name, v in (("host_side", host_side), ("seed", seed)):
            if (v is not None or name == "seed") and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
                raise ValueError(f"load_detected_model: {name} is a whole number{' (or None)' if name == 'host_side' else ''}, "
                                 f"not {v!r}")
        opts = dict(kmax=int(kmax), max_stored=int(max_stored), cg=bool(cg), cg_diag=cg_diag, ragged=ragged,
                    factored_form=int(factored_form), budget_mb=budget_mb, seed=int(seed), host_side=host_side)
        self._pending = ("detected", ((A, np.asarray(b, float), float(b_const), d_lin, C_lin, bool(max_sense)), opts))
        return self

    def _detected_model(self, arrays, o, drank, kappa):
        """Detection on the device, then build_factored_model exactly as load_factored_model would call it -- or build_model,
        when the fallback rule says so."""
        from . import detect
        from .device import Device
        A, b, b_const, d_lin, C_lin, max_sense = arrays
        self.max_sense = max_sense
        if self._device is None:
            self._device = Device(self._device_index)
        hs = detect.HOST_SIDE if o["host_side"] is None else int(o["host_side"])
        items, report = detect.detect_factors(A, len(b), o["kmax"], self._device, budget_mb=o["budget_mb"], seed=o["seed"],
                                              datasparsity=kappa, host_side=hs)
        reason = detect.fallback_reason(report["accepted"], report["kept_nnz"], o["max_stored"], kappa)
        report["route"] = "general" if reason else "factored"
        report["reason"] = reason
        self.detect_report = report
        if reason:
            model = build_model(A, b, b_const, d_lin, C_lin, datarank=drank, kappa=kappa)
            note = f"load_detected_model: general path, {reason}"
            model.lowrank_note = f"{model.lowrank_note}; {note}" if model.lowrank_note else note
            return model
        wide = o["kmax"] == 64
        model = build_factored_model([blk[0] for blk in A], items, b, b_const, d_lin, C_lin, kappa=kappa,
                                     factored_form=o["factored_form"], max_rank=64 if wide else 16, wide_diag=False)
        model.factored_cg = o["cg"] and model.factored
        model.factored_cg_diag = o["cg_diag"] and model.factored
        model.ragged = o["ragged"] if model.factored else False
        model.lowrank_note = (f"load_detected_model: {report['accepted']} constraints as factors of rank <= {o['kmax']}, "
                              f"{sum(len(k) for k in report['kept_nnz'])} stored")
        check_factored_kit(model, self.options.get("kit", 0))
        check_diag_kit(model, self.options.get("kit", 0))
        return model

    def _copy_to(self):
        kind, payload = self._pending
        drank = int(self.options.get("datarank", 0))
        kappa = int(self.options.get("datasparsity", 8))
        if kind == "sdpa":
            model = model_from_sdpa(payload, datarank=drank, kappa=kappa)
            self.max_sense = False
        elif kind == "sdpa_detected":
            general = model_from_sdpa(payload[0], datarank=0, kappa=kappa)      # (the file's A, b, linear rows)
            model = self._detected_model((general.A, general.b, general.b_const, general.d_lin, general.C_lin, False),
                                         payload[1], drank, kappa)
        elif kind == "detected":
            model = self._detected_model(payload[0], payload[1], drank, kappa)
        elif kind == "factored":
            F0, factors, b, b_const, d_lin, C_lin, max_sense, form, ragged, wide, cg_diag, cg = payload
            self.max_sense = max_sense
            model = build_factored_model(F0, factors, b, b_const, d_lin, C_lin, kappa=kappa, factored_form=form,
                                         max_rank=64 if wide else 16, wide_diag=wide == "diag")      # (wide: False, True or "diag")
            model.factored_cg = bool(cg) and model.factored
            model.factored_cg_diag = cg_diag and model.factored
            model.ragged = ragged if model.factored else False      # (False, True, "ops" or "all")
            check_factored_kit(model, self.options.get("kit", 0))
            check_diag_kit(model, self.options.get("kit", 0))
        else:
            A, b, b_const, d_lin, C_lin, max_sense, factors = payload
            self.max_sense = max_sense
            model = build_model(A, b, b_const, d_lin, C_lin, datarank=drank, kappa=kappa, factors=factors)
        model.local_support = self._local_support and kind in ("sdpa", "arrays")
        model.long_rows = self._long_rows
        opts = dict(self.options)
        if self.silent:
            opts["verb"] = 0
        if self._device is None:
            from .device import Device
            self._device = Device(self._device_index)
        if self.resident:
            from . import resident
            self.solver, self.halpha = resident.load(model, opts, device=self._device)
        else:
            self.solver, self.halpha = solvers.load(model, opts, device=self._device)
        self.solver.exact_regularised_solve = self.exact_regularised_solve

    def optimize(self):                        # MOI.optimize! (:136-140)
        if self._pending is None:
            raise RuntimeError("no model loaded")
        self._copy_to()
        solvers.solve(self.solver, self.halpha)
        return self

    # ---- results (MOI_wrapper.jl:241-354)
    def termination_status(self):
        if self.solver is None or self.solver.status == 0:
            return OPTIMIZE_NOT_CALLED
        return {1: OPTIMAL, 2: INFEASIBLE, 3: INFEASIBLE_OR_UNBOUNDED, 4: ITERATION_LIMIT}[self.solver.status]

    def raw_status(self):
        return f"Terminated with status {self.solver.status}"

    def primal_status(self):
        t = self.termination_status()
        return {OPTIMIZE_NOT_CALLED: NO_SOLUTION, OPTIMAL: FEASIBLE_POINT, INFEASIBLE: INFEASIBLE_POINT}.get(
            t, UNKNOWN_RESULT_STATUS)

    def dual_status(self):
        t = self.termination_status()
        return {OPTIMIZE_NOT_CALLED: NO_SOLUTION, OPTIMAL: FEASIBLE_POINT}.get(t, UNKNOWN_RESULT_STATUS)

    def result_count(self):
        return 0 if self.termination_status() == OPTIMIZE_NOT_CALLED else 1

    def solve_time(self):
        return self.solver.tottime

    def objective_value(self):
        s = self.solver
        val = float(s.model.b @ s.y) - s.model.b_const
        return val if self.max_sense else -val

    def dual_objective_value(self):
        s = self.solver
        m = s.model
        val = sum(solvers._cdot(m.C[i], s.X[i]) for i in range(m.nlmi)) - m.b_const
        if m.nlin > 0:
            val += float(m.d_lin @ s.X_lin)
        return val if self.max_sense else -val

    def variable_primal(self):
        return self.solver.y.copy()

    def constraint_dual_psd(self, lmi):
        X = self.solver.X[lmi]
        n = X.shape[0]
        return np.array([X[i, j] for j in range(n) for i in range(j + 1)])

    def constraint_dual_lin(self):
        return self.solver.X_lin.copy()
