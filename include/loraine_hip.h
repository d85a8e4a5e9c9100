/*
 * loraine_hip.h -- C ABI of libloraine_hip.so, the MI355X (gfx950) implementation of the
 * per-IP-iteration linear-algebra hot path of Loraine.jl v0.2.5.
 *
 * The reference has no FFI layer: the boundary is the set of plain Julia calls made by
 * myIPstep / predictor / corrector (src/Solvers.jl:448-478, src/predictor_corrector.jl).
 * Each entry point below names the reference call it replaces (file:line relative to the
 * reference checkout).  INTEGRATION.md shows the Julia `ccall` glue that binds them.
 *
 * Conventions
 *   - return 0 = OK; negative = API / HIP error (text from lrn_last_error);
 *     numerical failure is reported LAPACK-style through `info` out-parameters so the host
 *     can replay the reference's regularisation loops (prepare_W.jl:12-24,
 *     predictor_corrector.jl:59-85).
 *   - FP64, column-major, sparse data in the reference's own format: SparseMatrixCSC
 *     (colptr, rowval, nzval), Int64, 1-based.
 *   - every data pointer may be HOST or DEVICE memory (detected per call); the caller owns
 *     it and it is only accessed during the call.  Device state is owned by the context.
 *   - one context per GPU / per process; calls are blocking and not re-entrant
 *     (the reference is single-threaded).
 */
#ifndef LORAINE_HIP_H
#define LORAINE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lrn_ctx lrn_ctx;

/* ---- lifetime ------------------------------------------------------------------------- */
int lrn_create(lrn_ctx** out, int device);
int lrn_destroy(lrn_ctx* ctx);
const char* lrn_last_error(lrn_ctx* ctx);
int lrn_version(void);
/* number of visible HIP devices (0 on a CPU-only host; never fails) */
int lrn_device_count(void);

/* ---- static model data: the outputs of _prepare_A (src/model.jl:120-150) -------------- */
/* AA[ilmi]: nvar x msz^2 CSC, row j = -vec(A_j) (model.jl:199-229).
 * B[ilmi] : nvar x msz CSC rank-one factors (model.jl:176-197) or NULL arrays.
 * sigmaA  : nvar x nlmi (col-major, 1-based), qA: 2 x nlmi (model.jl:153-174).
 * C_lin   : nvar x nlin CSC (MOI_wrapper.jl:145-149) or nlin = 0.                        */
int lrn_upload_model(lrn_ctx* ctx, int nlmi, int nvar, const int64_t* msizes,
                     const int64_t* const* AA_colptr, const int64_t* const* AA_rowval,
                     const double* const* AA_nzval,
                     const int64_t* const* B_colptr, const int64_t* const* B_rowval,
                     const double* const* B_nzval,
                     const int64_t* sigmaA, const int64_t* qA,
                     int nlin, const int64_t* Clin_colptr, const int64_t* Clin_rowval,
                     const double* Clin_nzval);
/* Rank-k constraint data of block ilmi (datarank >= 1; reference docs/src/low-rank_data.md): A_k = V_k diag(d_k) V_k'
 * with d in {+1, -1}, every constraint padded to khat columns (khat = 1, 2, 4, 8 or 16; padding columns empty, weight 0).
 * khat = 32 or 64 (a WIDE block, constraints of rank 17 .. 64) is accepted under lrn_set_option "lowrank_wide" = 1 and
 * refused with LRN_ERR_ARG otherwise, as any other value is: mode 1 assembles such a block by rank class whatever
 * "lowrank_ragged" says (one GPU: LRN_ERR_ARG from lrn_schur_assemble when world > 1; lrn_get_count "schur_wide"), and it
 * carries no diagonal parts (lrn_upload_diag on it, and this call with a wide khat on a block that holds them: LRN_ERR_ARG)
 * unless lrn_set_option "wide_diag" = 1 admits them.
 * V: (nvar * khat) x msz CSC, 1-based, row k * khat + p = column p of V_k (the orientation of B above); d: nvar * khat
 * weights in the same order.  Call after lrn_upload_model / lrn_synthetic_dense_model; lrn_schur_assemble(mode 1) uses
 * them.  AA stays what every other entry point reads (unless the block is declared factored, below).  If some constraint
 * with entries in AA has no factor column of non-zero weight, the factors do not cover the block: mode 1 then assembles a
 * block that is not declared factored from the entries of its AA (the general assembly; lrn_get_count "lowrank_from_entries"). */
int lrn_upload_lowrank(lrn_ctx* ctx, int ilmi, int khat, const int64_t* V_colptr, const int64_t* V_rowval,
                       const double* V_nzval, const double* d);
/* Factored block (after lrn_upload_model and lrn_upload_lowrank): on = 1 declares that the factors ARE the constraint data
 * of block ilmi -- its AA was uploaded without entries, no A_k exists as a matrix on host or device.  AA vec(.) and
 * mat(AA' .) of the resident path (lrn_ip_*) then run in factor form: Q = Z Vd by one FP64 MFMA product and a column dot
 * per constraint; M = -Vd diag(w o x) Vd' by one lower-triangle product, mirrored (exactly symmetric).  The Schur matrix
 * comes from lrn_schur_assemble(mode 1).
 * Hybrid block: the AA may hold the rows of a few STORED constraints (sparse or dense, -vec(A) as everywhere) provided the
 * factor columns of those constraints all have weight 0 -- every constraint is exactly one of the two.  The stored rows go
 * through the stored-entry kernels (sparse tier, dense slots) beside the factor form; mode 1 adds H_SS by the general
 * assembly over the stored rows and the cross terms H_sj = sum_p d_jp y_jp' A_s y_jp from Y = W Vd (one pass over Y, fixed
 * order, no atomics; option "fac_cross_lds").  One GPU only: mode 1 returns LRN_ERR_STATE for a hybrid block under world > 1.
 * LRN_ERR_STATE when no factors were uploaded or when a constraint of the block has both a stored row and a factor column
 * of non-zero weight ("has entries": no constraint may be counted twice; a fully materialised AA with factors is refused as
 * before).  On a factored block lrn_matvec / lrn_matvec_partial, lrn_prec_setup, lrn_pcg and modes 0 / -1 of
 * lrn_schur_assemble return LRN_ERR_STATE, and so does lrn_get_constraint for a factored constraint (a stored constraint of
 * a hybrid block is returned).  on = 0 takes the declaration back.
 * lrn_get_count: "op_factored" / "op_dense" / "op_sparse" count the operator calls by route, "op_dense_tri" /
 * "op_dense_stream" / "op_dense_scalar" the passes over dense constraint data by tier (column tails of symmetric data /
 * 16-byte loads over both triangles / one element per lane; the tier is decided when the model is uploaded);
 * "op_sparse_pattern" counts the blocks the CG operator took through the pattern-restricted route (once per block and call
 * of lrn_matvec / lrn_matvec_partial), "op_wmw_pattern" the right-hand sides AA vec(W M W) formed on the pattern; "device_bytes",
 * "device_bytes_peak" (device memory of this context now / at most) and "adense_bytes" (dense constraint slabs) are state. */
int lrn_set_factored(lrn_ctx* ctx, int ilmi, int on);
/* Diagonal parts of a factored block (after lrn_set_factored(ilmi, 1)): constraint rows[s] (0-based, as k of
 * lrn_get_constraint) of block ilmi is A = diag(a_s) + V D V' with a_s = column s of `a` (msz x nrows, column-major) and V, D
 * its factor columns (all of weight 0 for a purely diagonal constraint, e.g. a trace row: a_s = 1).  Host or device arrays.
 * nrows = 0 clears the diagonal parts; lrn_set_factored(ilmi, 0) and lrn_upload_model drop them, lrn_upload_lowrank keeps
 * them.  LRN_ERR_STATE when the block is not factored or when a row is a stored constraint of a hybrid block (it has entries:
 * put the diagonal into the stored matrix); LRN_ERR_ARG for a row out of range or listed twice.
 * The data operators subtract sum_i a_si Z_ii / add -sum_s x_s a_s to the diagonal of mat(AA' x) after the factor form; mode 1
 * of lrn_schur_assemble adds H_DD = Ad' (W o W) Ad, the cross terms Ad' (Y o Y) with Y = W Vd (weighted, summed over khat) and
 * a_k' diag(W A_s W) for the stored rows of a hybrid block -- dense products with one operand squared entrywise, no entry list
 * (option "diag_sq_mfma"), fixed order, no atomics.  With diagonal rows in any block lrn_matvec, lrn_matvec_partial,
 * lrn_prec_setup, lrn_prec_apply and lrn_pcg return LRN_ERR_STATE also under "cg_factored" = 1 (ts of H_alpha does not hold
 * the diagonal parts) -- unless option "cg_diag" = 1 is set beside it --, and mode 1 returns LRN_ERR_STATE under world > 1.
 * lrn_get_count: "diag_rows" (state: diagonal rows of all blocks), "op_diag" (operator calls that added a diagonal part),
 * "schur_diag" (assemblies of a block with diagonal rows), "diag_sq_rows" / "diag_sq_mfma" (squared-operand products by form),
 * "diag_stored_cross" (cross terms with stored rows); timing keys under "profile": "diag_dd", "diag_cross", "diag_stored". */
int lrn_upload_diag(lrn_ctx* ctx, int ilmi, int64_t nrows, const int64_t* rows, const double* a);
/* Low-rank detection: which of `cnt` dense symmetric m x m matrices (A: one after the other, column-major, host or device)
 * are V diag(d) V' with at most kmax (16 or 64) columns, and their factors -- what a caller that holds matrices needs to reach
 * lrn_upload_lowrank / lrn_set_factored.  Symmetric Nystrom identity with the caller's sketch matrix omega (m x l, l = kmax + 8,
 * column-major, e.g. standard normals): Y = A omega, C = omega' Y = U Lambda U' (batched two-sided Jacobi in LDS, one workgroup
 * per matrix), V = Y U_r |Lambda_r|^-1/2, d = sign Lambda_r over the r eigenvalues with |lambda| > rank_rtol max|lambda|.
 * Per matrix k: rank_out[k] = r >= 0, or -1 for "not of rank <= kmax within tol"; resid_out[k] = the computed
 * ||A_k - V_k D_k V_k'||_F (FP64 MFMA over 64 x 64 tiles, fixed summation order) -- of the factor returned, so ||A_k||_F for a
 * matrix rejected on its eigenvalue count, for which no factor is formed; V_out: cnt x (m x kmax, column-major), columns >= r
 * zero; d_out: cnt x kmax, +-1, zero in the padding.  The residual is the arbiter: rank_out[k] = r only if resid_out[k] <= tol
 * (absolute), -1 otherwise (V_out, d_out then hold the factor that missed).  m >= 1 (m < l is legal), 1 <= cnt <= 65535.
 * The result for a matrix depends on A_k and omega alone -- not on cnt, its place in the chunk or its neighbours -- and
 * repeated calls agree bit for bit (no atomics).  Stateless with respect to the model: needs the context only, may be called
 * before lrn_upload_model; the workspace (cnt m^2 + cnt m (kmax + l + 8) doubles and change, counted in "device_bytes") stays
 * with the context until lrn_set_option("detect_release", 1) (any non-zero value; 0 does nothing) or lrn_destroy -- the
 * caller chooses the chunk.  Symmetry of A is ASSUMED, not verified: the sketch reads all of A_k, the residual only its 64 x 64
 * tiles on and below the diagonal (and counts the off-diagonal ones twice), so for an unsymmetric A_k -- one triangle alone,
 * say -- resid_out is not ||A_k - V D V'||_F and the verdict is meaningless; the caller checks (the Python host does, in
 * detect.detect_factors).
 * lrn_get_count: "detect_calls", "detect_accepted", "detect_rejected" (matrices by verdict), "detect_sweeps_max" (most Jacobi
 * sweeps any matrix took); timing keys under "profile": "detect" and its steps "detect_upload", "detect_sketch",
 * "detect_core", "detect_eig", "detect_factor", "detect_resid". */
int lrn_lowrank_detect(lrn_ctx* ctx, int m, int cnt, const double* A, int kmax, double tol, double rank_rtol,
                       const double* omega, int32_t* rank_out, double* resid_out, double* V_out, double* d_out);
/* Builder-defined synthetic dense SDP data generated on the device:
 * A_k = (R_k + R_k')/2, R_k iid N(0,1) from a counter-based Philox stream; nlmi = 1. */
int lrn_synthetic_dense_model(lrn_ctx* ctx, int msz, int nvar, uint64_t seed);
/* Completes the synthetic data to a strictly feasible SDP: X0 = I + QQ'/msz,
 * b = AA vec(X0), y0 ~ N(0,1)/sqrt(nvar), S0 = I, C = S0 + mat(AA' y0).  C stays on the device
 * (resident path); b_out[nvar], y0_out[nvar] and ||C||_F are returned. */
int lrn_synthetic_dense_problem(lrn_ctx* ctx, uint64_t seed, double* b_out, double* y0_out, double* normC);
/* dense copy of constraint matrix A_k (0-based k) of block ilmi, msz x msz */
int lrn_get_constraint(lrn_ctx* ctx, int ilmi, int k, double* A_out);
/* tuning knobs (per context): "dense_threshold" (nnz above which a branch-1 constraint takes
 * the MFMA path), "profile" (0/1), "t_batch", "p_batch", "shard_bs" (0 = auto), "jacobi_warm" (0/1), "jacobi_block",
 * "jacobi_inner", "jacobi_wgs", "pivot_boost" (relative pivot level boosted in lrn_schur_factor, 0 = off),
 * "prec_eig" (0 auto / 1 full Jacobi eigendecomposition / 2 Lanczos extremes in lrn_prec_setup),
 * "matvec_sparse" (0 auto -- pattern-restricted mat-vec when every constraint is sparse and M = mat(AA'x) is sparse
 * enough: msz >= 1500, or msz in [256, 1500) with at most 1/12 of M stored -- / 1 dense GEMM mat-vec / 2 pattern-restricted
 * whenever every constraint is sparse),
 * "schur_chol" (dense Schur assembly through the Cholesky factor of W: -1 auto -- H_ij = <L'A_iL, L'A_jL> when
 * every constraint of the block is dense, T_k = L (L'A_kL) L' otherwise, both for msz >= 256 --,
 * 0 never (T_k = W A_k W), 1 as auto without the size threshold, 2 the T_k form only),
 * "schur_plan" (-1 decide locally / 0 / 1: the assembly path every rank of a sharded run agreed on, see lrn_schur_plan),
 * "gemm3_ksplit" (split-K factor of the inner-product GEMM, 0 = auto), "gemm3_sched" (1: regular and masked tiles of
 * GEMM3' in one launch, 0: two launches), "gemm3_tile" (0 auto / 128 / 160), "gemm3_strip" (1: nvar % 128 in (0, 32] -> the last
 * 128 + nvar % 128 rows of H as a launch of 128 x 160 tiles instead of a row of edge tiles), "gemm_no_skip" (1: no block masks
 * in the three GEMMs of the factor path -- A/B switch), "gemm_dyn_masks" (1: the masked K-steps of GEMM1'/2' branch per
 * block as in round 2 -- A/B switch), "gemm1_diag" (1, default: GEMM1' leaves out the blocks of its diagonal tiles that
 * GEMM2' never reads and stores zeros there; 0: computes them -- A/B switch, bit-identical), "gemm_lab" (measurement only:
 * GEMM1'/2' without epilogue / K loop / first load, one workgroup per CU, whole K range, one matrix for every batch
 * element -- tools/gemm12_overhead.py), "gemm3_stagger" (experiment: K-walk stagger of the workgroups of
 * GEMM3' in chunks of 16, 0 = off), "pair_lanes" (lanes per entry of the sparse pair kernel: 0 auto / 4 / 8 / 16 / 64),
 * "pair_local" (0, default / 1; anything else: LRN_ERR_ARG -- 1: the sparse owners of a block whose partners all have a support
 * of at most 32 rows and columns, and which have at least "pair_local_min" entries, are assembled from A[S, S] on their
 * supports, two small MFMA products per pair; one GPU -- an empty range or a sharded context counts "pair_local_skipped" and
 * takes the pair kernels, bit for bit; counts "pair_local_owners", "pair_local_pairs", timing "local"), "pair_local_min"
 * (>= 1, default 36 entries: read by the next lrn_upload_model),
 * "pair_long" (0, default / 1; anything else: LRN_ERR_ARG -- 1: the sparse owners of a block with at least "pair_long_min" entries
 * (>= 1: read by the next lrn_upload_model), a trace row or a band, are assembled from Z_i = (A_i W) on their rows, nnz_j |R_i|
 * products per pair cut into slices of "pair_long_split" products (>= 1) over workgroups; partners with a support of at most 32
 * through the FP64 MFMA unless "pair_long_mfma" is 0 (0 / 1); Z_i lives in a scratch of at most "pair_long_scratch_mb" MiB
 * (>= 0, default 1024).  One GPU -- an empty range, an owner that does not fit the scratch or a sharded context counts
 * "pair_long_skipped" and takes the pair kernels, bit for bit; counts "pair_long_owners", "pair_long_pairs",
 * "pair_long_mfma_pairs", "pair_long_slices", timing "long"),
 * "jacobi_cross" (1: cross-pair rotations only after round 0), "jacobi_early" (relative level below which a sweep's
 * rotations make it the last one; 0 = always run the confirming sweep), "eigmin_pair" (the two
 * smallest-eigenvalue searches of a step-length computation: 2, default = their Lanczos runs in lock-step, one launch per
 * pair of steps; 1 = as two launch chains on two streams; 0 = one after the other -- same results),
 * "lz_resident" (1, default: the Lanczos steps of these searches and of the H_alpha setup, matrix side <= 1024, as resident
 * launches of 16 / 24 steps -- the workgroup's columns of the matrix in registers, y and the partial dot products exchanged
 * through relaxed agent-scope atomics with no barrier (unwritten words hold a mark), every wait bounded by the wall clock; a launch that
 * gives up sends the context back to one launch per step; 0: one launch per step -- same results bit for bit),
 * "prepw_streams" (1: lrn_prepare_w runs the S side and the Gi solve on a second stream),
 * "nt_mode" (lrn_ip_prepare_w: 1 = NT scaling without singular vectors -- Newton-Schulz square roots of K = L_X'SL_X,
 * Lyapunov solve for the second-order term, SVD route as fallback --, 0 = the reference's SVD route always; lrn_prepare_w
 * with output pointers always takes the SVD route), "ns_l0" (assumed lower end of spec(K)/c of the Newton-Schulz schedule),
 * "ns_maxit", "ns_dual" (-1 auto / 1 / 0: transposed twins of the products from the GEMM epilogue or a transpose pass),
 * "lyap_tol", "lyap_maxit" (relative residual / step limit of the Lyapunov CG),
 * "prec_inv" (H_alpha: -1 auto / 1 / 0: SMW core through an explicit inverse + one refinement step, or two triangular solves),
 * "shard_passes" (multi-GPU, 1: the passes over dense constraint data in AA*vec(.) / mat(AA'x) split by rank),
 * "shard_products" / "shard_products_min" (multi-GPU, 1: the n^3 products of the resident path -- Newton-Schulz, Lyapunov CG,
 * step and right-hand sides -- as column blocks + all-gather from matrix side shard_products_min = 4096 on),
 * "matvec_h" (CG operator of lrn_pcg / lrn_matvec through the ASSEMBLED Schur matrix, one pass over its lower triangle per
 * application: 0 = a static cost model decides once per NT scaling from the CG iterations of the previous one, 1 = never,
 * 2 = always), "prec_dense" (H_alpha inside lrn_pcg as one dense symmetric matrix, nvar <= 8192: 0 cost model / 1 never /
 * 2 always, also in lrn_prec_apply), "pcg_lookahead" (iterations lrn_pcg queues beyond the convergence test it has read,
 * 0..8; the count and the result do not depend on it), "wmw_pattern_min" (right-hand sides AA vec(W M W) with all constraints
 * sparse: from this matrix side on through the pattern entries of W M W), "lyap_form" (second-order term of the corrector:
 * 1 = the better conditioned equivalent Lyapunov equation (Yh/s + s Zh) R + R (.) = C/s + s Zh C Zh, 0 = Yh R + R Yh = C),
 * "ns_lanczos" / "ns_lanczos_min" (1: scale and schedule of the Newton-Schulz iteration from a 24-step Lanczos run on K for
 * blocks of side >= ns_lanczos_min = 1500), "lowrank_form" (rank-k assembly, mode 1: U = G'V by a gather over the factor
 * entries (0), one dense MFMA product (1), or by the factors' density (-1, default)), "fac_cross_lds" (cross terms of a
 * hybrid factored block: each column of Y staged in LDS (1, columns of up to 64 KiB), gathered from global memory (0), or LDS
 * up to 32 KiB per column (-1, default); the same bits either way), "profile_ops" (measurement: every
 * AA vec(.) / mat(AA' .) timed by itself under "aa_times" / "aa_times2" / "aat_to_mat"; synchronises, not for solves), "comm_fail_ensure" (test hook: the next exchange of this rank fails its buffer
 * allocation), "lz_res_limit" (ticks of the 100 MHz wall clock a workgroup of a resident Lanczos launch waits for its peers
 * before the launch gives up; default 2 000 000 = 20 ms, clamped to [1000, 2 000 000]: the option shortens the wait, it
 * never lengthens it; lrn_get_count("lz_res_limit") returns the value in effect), "lz_test_withhold" (test hook, one shot:
 * value = k + 100000 (run + 2 (step + 3 wg)) arms the k-th resident Lanczos launch queued on this context from now on,
 * 1 <= k < 100000 -- in it ONE workgroup (wg 0: workgroup 0, which also writes for the host; 1: the last, ragged one) of ONE
 * run (run 0 / 1 of a pair in lock-step; a launch of a single run has run 0 only) keeps its publication of ONE step (step 0:
 * the first of the launch, 1: a middle one, 2: the last) to itself.  Its peers' wait runs into lz_res_limit, all workgroups
 * return normally, the host repeats the run with one launch per step; lrn_get_count("lz_test_withheld") goes up when the armed
 * launch is queued and, like "lz_no_persist", survives reset_timing; 0 disarms),
 * "cg_lowrank" (the CG path -- lrn_matvec, lrn_prec_setup, lrn_pcg -- from the rank-k factors of lrn_upload_lowrank: 0, default
 * = never, every route and every bit as without factors; 1 = always, for every COVERED block: one that is not declared
 * factored and whose factors reach every constraint that has entries; -1 = a static cost model decides per piece.  The
 * pieces: the assembled-matrix operator ("matvec_h") assembles H in mode 1 when every LMI block is covered; the matrix-free
 * operator takes mat(AA' x) and AA vec(W M W) of a covered block in the factor form of factored blocks; lrn_prec_setup forms
 * the block of ts = D^-1/2 AA (U (x) Z) of a covered block as P = L' Vd, T = Vd' Um and one weighted, transposing pass over P
 * instead of one pass over every A_k per eigenvector.  Everything else that reads AA -- lrn_make_rhs, lrn_ip_*, the general
 * assembly -- stays on the entries.  Factored and hybrid blocks keep refusing the CG entry points (see "cg_factored").  With world > 1
 * (lrn_set_shard, lrn_comm_init) the option is ignored and the entry routes run: the factor routes are not sharded and have
 * only been run on one GPU),
 * "cg_factored" (0, default: lrn_matvec, lrn_prec_setup and lrn_pcg return LRN_ERR_STATE for a factored block, as they always
 * have; 1: lrn_matvec, lrn_prec_setup, lrn_prec_apply and lrn_pcg accept pure and hybrid factored blocks and models that mix
 * them with stored-entry blocks -- the matrix-free operator runs in factor form, the assembled-matrix operator assembles H in
 * mode 1, ts of H_alpha comes from the factors (P = L' Vd, T = Vd' Um, one transposing pass) and, for the stored constraints
 * of a hybrid block, from their entries on a compact npos_nz x msz buffer.  lrn_matvec_partial and every call under world > 1
 * keep returning LRN_ERR_STATE for a factored block: the factor routes are not sharded and were run on one GPU only),
 * "cg_diag" (0, default: a factored block with diagonal parts, lrn_upload_diag, is refused by these entry points whatever
 * "cg_factored" says; 1, together with "cg_factored" = 1: accepted on one GPU -- the operators carry the diagonal parts as they
 * do for kit = 0, and lrn_prec_setup adds ts[nat(s), a msz + r] -= sum_i a_si Um[i, a] L[i, r] / sqrt(d) for every diagonal row s
 * to the factor part of ts, one FP64 MFMA tile product; lrn_matvec_partial and world > 1 stay refused; counter
 * "prec_ts_diag_rows": diagonal rows added in the LAST lrn_prec_setup),
 * "hop_max_mb" (budget of the assembled-matrix operator in MiB: when nvar^2 * 8 bytes exceed it H is not assembled, even under
 * "matvec_h" = 2, and the matrix-free operator runs; -1, default: no limit for a model without a factored block, and for one
 * with a factored block the free device memory minus the mode-1 workspace), "fac_op_scaled" (under "cg_factored", pure
 * factored blocks, matrix-free operator: 1 = Y = W Vd once per NT scaling and W mat(AA' x) W = -Y diag(w o x) Y' per
 * application, no W M W product; 0 = the composition mat(AA' x) -> W M W -> AA vec(.); -1, default = cost model, which is
 * "off" until the form has been measured faster), "fac_quadform" (under "cg_factored", pure and hybrid factored blocks, inside
 * the matrix-free operator only: 1 = AA vec(Z) of the factor part by the fused quadratic form of facops.hip, Q = Z Vd never
 * stored; 0 = Q and the column dots; -1, default = cost model, "off" likewise), "diag_sq_mfma" (squared-operand product of
 * the diagonal parts, lrn_upload_diag: 1 = the 64 x 64 FP64 MFMA tile form, 0 = the rows form, one wave per column group and
 * eight rows in registers, -1, default = by the number of diagonal rows),
 * "lowrank_ragged" (rank-k assembly, mode 1, of a block whose constraints have MIXED ranks: 0, default = every constraint on
 * khat columns, the padded route, every route, counter and bit as before; 1 = by rank class -- the constraints are grouped by
 * the power of two >= their rank (number of weighted factor columns; 1, 2, 4, 8, 16; rank 0: no group), the weighted columns
 * compacted class by class (16 first) into Vc, msz x Rc, and H_FF comes from U_c = G' Vc (W Vc) and one FP64 MFMA tile launch
 * over a host-built tile list (raggedops.hip), msz Rc^2 / 2 multiply-adds instead of msz (nvar khat)^2 / 2.  Taken per block
 * when world == 1 and 0 < Rc < nvar khat; a uniform block, an empty one and a sharded run keep the padded route and count
 * "ragged_fallback".  The data operators, the cross terms of a hybrid block and the terms of diagonal parts stay on the
 * padded layout (options "ragged_ops", "ragged_cross" below move them).  Counters: "schur_ragged" (blocks assembled by rank class), "ragged_fallback", and the STATE of the last
 * block assembled that way (survives reset_timing): "ragged_cols" (Rc), "ragged_classes" (classes present), "ragged_tiles";
 * timing key "ragged" (U_c and the tile launch, beside "lowrank_u"),
 * "lowrank_wide" (0, default = lrn_upload_lowrank takes khat up to 16; 1 = khat 32 and 64 as well.  A block uploaded so is
 * wide: the classes 64 and 32 lead the layout, mode 1 takes the rank-class route for it unconditionally, also when Rc = nvar
 * khat; "ragged_ops", "ragged_cross", "ragged_ts" keep their condition and move its other routes from the padded layout at
 * khat 32 / 64 to the compacted columns; counter "schur_wide" = assemblies of a wide block),
 * "wide_diag" (0, default = a wide block carries no diagonal parts: lrn_upload_diag on it, a wide lrn_upload_lowrank on a block
 * that holds diagonal rows, and the MFMA form of the squared-operand product at khat 32 / 64 return LRN_ERR_ARG, texts
 * unchanged; 1 = the three accept -- a factor-model constraint B S B' + diag(psi) with 17 .. 64 factors goes in as factors
 * and a diagonal row, the rows of a re-uploaded block stay as under a narrow re-upload, and C = Ad' (Y o Y) sums column groups
 * of 32 and 64 in a fixed order, no atomics (diagops.hip; per class under "ragged_cross").  The CG path takes such a block
 * where "cg_factored" and "cg_diag" take a narrow one.  One GPU, not through lrn_matvec_partial, stored constraints carry
 * their diagonal in their entries: those refusals stay.  Resets the operator choice, as "lowrank_wide" does),
 * "ragged_ops" (the factor form of AA vec(.) and mat(AA' .) of such a block: 0, default = on the nvar khat padded columns, every
 * route, counter, error text and bit as before; any other value = 1 = on the Rc compacted columns of "lowrank_ragged" -- Q = Z Vc
 * and sums by group, or the fused quadratic form on (Vc, Rc) under "fac_quadform"; mat(AA' x) = -sum_c s_c f_c f_c' by one FP64
 * MFMA launch over the lower 64 x 64 tiles and K-chunks with F = Vc, or Yc = W Vc under "fac_op_scaled" (raggedops.hip).
 * Independent of "lowrank_ragged", the same condition per block: world == 1 and 0 < Rc < nvar khat; otherwise the padded code
 * runs bit for bit and "ragged_ops_fallback" counts.  The first call by either route builds the plan and Vc.  Every caller of
 * the factor form gets it: the resident entry points, lrn_matvec / lrn_pcg under "cg_factored", the covered blocks of
 * "cg_lowrank"; lrn_matvec_partial and world > 1 stay as they are.  Counters: "op_ragged" (operator calls by this route;
 * "op_factored" counts as well), "ragged_ops_fallback", and the STATE "ragged_ops_chunks" (K-chunks of the last launch; survives
 * reset_timing); timing keys stay "aa_times" / "aat_to_mat"),
 * "ragged_ops_split" (K-chunks of that launch: 0, default = auto, 1 .. 16 forced, clamped to the K-steps ceil(Rc / 16) of the
 * block; chunk s covers the steps [s nsteps / ks, (s + 1) nsteps / ks) and the chunks are added in the order 0 .. ks - 1),
 * "ragged_cross" (Y = W V and its consumers in mode 1 of such a block, the cross terms of the stored constraints of a hybrid
 * block and of the diagonal parts: 0, default = on the nvar khat padded columns, every route, counter, error text and bit as
 * before; any other value = 1 = on the Rc compacted columns -- Yc = W Vc once per scaling, or the product the rank-class
 * assembly left when only W exists ("ragged_y_reused"), the cross terms summed by group, C = Ad' (Yc o Yc) class by class.
 * Independent of the options above, the same condition per block; otherwise the padded code runs bit for bit and
 * "ragged_cross_fallback" counts.  Counter "schur_cross_ragged", per block and assembly; timing keys stay "hybrid_y",
 * "hybrid_cross", "diag_cross"),
 * "ragged_ts" (ts of H_alpha, lrn_prec_setup(1, ..), of such a block on the factor route: 0, default = P = L' Vd and T = Vd' Um
 * on the padded columns; any other value = 1 = on the compacted ones, every element of the block's part of ts written once.
 * The same condition per block; otherwise the padded code bit for bit and "ragged_ts_fallback" counts.  Counter
 * "prec_ts_ragged", blocks of the last setup, "prec_ts_factored" counts them too; timing key "prec_ts_p" stays),
 * "reset_timing".
 * Counters of these options: "op_factored_scaled" (blocks per application through Y), "op_quadform_fused" (blocks per
 * application through the fused kernel), "fac_scaled_y" (products Y = W Vd), "hop_over_budget" (operator choices that found H
 * above the budget), "prec_ts_stored_rows" (rows of ts filled from stored entries in the LAST lrn_prec_setup).
 * Counters of this path (lrn_get_count): "lz_resident_launches" (resident launches queued), "lz_persist_abort" (those that
 * gave up), and the STATE "lz_no_persist" (0 / 1, survives reset_timing: a resident launch of this context has given up, all
 * Lanczos steps are launched one by one from then on). */
int lrn_set_option(lrn_ctx* ctx, const char* key, double value);
/* multi-GPU: this context assembles the Schur columns it owns (block-cyclic) */
int lrn_set_shard(lrn_ctx* ctx, int rank, int world);

/* ---- NT scaling: prepare_W (src/prepare_W.jl:28-94) ----------------------------------- */
/* X, S: msz x msz in; outputs may be NULL (kept on the device only).
 * info: 0 ok; 1 = X not PD, 2 = S not PD (host adds 1e-5*I and retries, :5-26). */
int lrn_prepare_w(lrn_ctx* ctx, int ilmi, const double* X, const double* S, double* D, double* G,
                  double* Gi, double* W, double* Si, double* DDsi, int* info);
/* directly set W (and optionally G) -- used when the scaling is produced elsewhere */
int lrn_set_scaling(lrn_ctx* ctx, int ilmi, const double* W, const double* G_or_null);
/* X_lin .* S_lin_inv for the C_lin terms (predictor_corrector.jl:37, Solvers.jl:609) */
int lrn_set_lin(lrn_ctx* ctx, const double* X_lin, const double* S_lin_inv);

/* ---- Schur complement: makeBBBBs / makeBBBB_rank1 (src/makeBBBB.jl:1-218) ------------- */
/* mode 0 = general (makeBBBBs), -1 = rank-one data (makeBBBB_rank1), 1 = rank-k factors of lrn_upload_lowrank
 * (H_ij = sum d_p d_q (u_p'u_q)^2 over the factor columns p of A_i, q of A_j, U = G'V; LRN_ERR_STATE without factors
 * or without G / W); adds the C_lin term (predictor_corrector.jl:36-38).  H_out (nvar x nvar) may be NULL; when given it receives
 * Matrix(Hermitian(BBBB, :L)) (predictor_corrector.jl:39). */
int lrn_schur_assemble(lrn_ctx* ctx, int mode, double* H_out);
int lrn_schur_get(lrn_ctx* ctx, double* H_out);
/* BBBB + eps*I (predictor_corrector.jl:74) */
int lrn_schur_add_diag(lrn_ctx* ctx, double eps);
/* cholesky(BBBB) (predictor_corrector.jl:57); info > 0: not PD at that column */
int lrn_schur_factor(lrn_ctx* ctx, int* info);
/* dely = L' \ (L \ h) (predictor_corrector.jl:90,199) */
int lrn_schur_solve(lrn_ctx* ctx, const double* h, double* dely);
/* multi-GPU exchange: pack the owned column blocks / unpack the all-gathered buffer */
int64_t lrn_schur_shard_doubles(lrn_ctx* ctx);
int lrn_schur_export_shard(lrn_ctx* ctx, double* buf);
int lrn_schur_import_all(lrn_ctx* ctx, const double* buf_all);
/* multi-GPU, dense data through the Cholesky factor of W: the ranks split the COLUMNS of the matrix variable, so
 * after lrn_schur_assemble every rank holds a partial SUM of the whole Schur matrix (lrn_schur_is_partial_sum = 1)
 * and the exchange is one all-reduce of nvar^2 doubles: export_full -> all-reduce(sum) -> import_full
 * (buffers host or device, position space, lower triangle authoritative).  When it returns 0 the owned column
 * blocks are exchanged with export_shard / all-gather / import_all as above. */
int lrn_schur_is_partial_sum(lrn_ctx* ctx);
/* multi-GPU: which of the two exchanges the next lrn_schur_assemble(mode) of THIS rank would need, from its own view
 * (options, data layout, world size, free device memory): *plan = 1 partial sums + all-reduce, 0 column blocks +
 * all-gather.  Free memory can differ between ranks, so the host all-reduces (MIN) the answers once after
 * lrn_set_shard and pins the result on every rank with lrn_set_option("schur_plan", 0 or 1); a pinned plan is not
 * re-decided by the assembly (a rank that then cannot allocate fails loudly instead of entering another
 * collective).  The reference has no counterpart (single process); this belongs to the sharded loop of
 * src/makeBBBB.jl:77-101. */
int lrn_schur_plan(lrn_ctx* ctx, int mode, int* plan);
int lrn_schur_export_full(lrn_ctx* ctx, double* buf);
int lrn_schur_import_full(lrn_ctx* ctx, const double* buf);

/* ---- right-hand sides: makeRHS (src/makeBBBB.jl:221-228), corrector :186 --------------- */
/* h = Rp + sum AA*vec(W (Rd+S) W) ; Rd_plus_S: msz x msz per block, concatenated */
int lrn_make_rhs(lrn_ctx* ctx, const double* Rp, const double* const* RdS, double* h);

/* ---- CG operator and preconditioners (src/Solvers.jl:572-904) ------------------------- */
/* Ax = sum AA vec(W mat(AA'x) W) + C_lin((X_lin.*S_lin_inv).*(C_lin'x))   (MyA, :582-614).
 * The same linear map is H x for the Schur matrix H of src/makeBBBB.jl:67-218: when lrn_pcg has chosen that form for the
 * current NT scaling (or option "matvec_h" = 2) the library assembles H once per scaling with the kernels of
 * lrn_schur_assemble and applies it as one bandwidth-bound pass over its lower triangle (csrc/hop.hip). */
int lrn_matvec(lrn_ctx* ctx, const double* x, double* Ax);
/* multi-GPU CG operator: this rank's share  AA[:, idx(R_g)] vec((W M W)[R_g,:])  of the mat-vec,
 * R_g = row block `rank` of `world` (lrn_set_shard); the caller all-reduces (sum) the nvar-vector. */
int lrn_matvec_partial(lrn_ctx* ctx, const double* x, double* Ax_partial);
/* prec: 0 none (MyM_no), 1 H_alpha (Prec_for_CG_tilS_prep :674-809), 2 H_beta
 * (Prec_for_CG_beta :624-663).  info > 0: a Cholesky inside the setup failed. */
int lrn_prec_setup(lrn_ctx* ctx, int prec, int erank, int aamat, int* info);
/* Mx = M^{-1} x (MyM :866-904, MyM_beta :670-672, MyM_no :620-622) */
int lrn_prec_apply(lrn_ctx* ctx, const double* x, double* Mx);
/* cg(A, h; tol, maxIter, precon) of ConjugateGradients.jl 0.1 (call sites
 * predictor_corrector.jl:134,235), device-resident: the recurrence is two multi-workgroup launches per iteration, the
 * relative-residual test runs on the device and the host reads it `pcg_lookahead` iterations behind the one it queues
 * (iterations queued beyond the last one leave x untouched: exit code, count and x are those of the loop that tests after
 * every step).  Operator: MyA matrix-free or through the assembled Schur matrix (see lrn_matvec). */
int lrn_pcg(lrn_ctx* ctx, const double* h, double tol, int maxit, double* x, int* exit_code,
            int* iters);

/* ---- device-resident iterate (find_step, check_convergence, RHS) ---
 * The matrix variables X, S, Rd, delX, delS, Xn, Sn, RNT live on the device; only nvar-/nlin-
 * vectors and scalars cross the boundary.  All functions act on every LMI block at once unless
 * they take `ilmi`. */
/* C[ilmi] = -A[ilmi,1] dense msz x msz (src/model.jl:133) */
int lrn_ip_set_c(lrn_ctx* ctx, int ilmi, const double* C);
/* initial point X = Eps*I, S = Eta*I (src/initial_point.jl:33,42) or any iterate */
int lrn_ip_set_iterate(lrn_ctx* ctx, int ilmi, const double* X, const double* S);
int lrn_ip_get_iterate(lrn_ctx* ctx, int ilmi, double* X, double* S);
/* X (which=1) or S (which=2) += eps*I : try_cholesky's regularisation (src/prepare_W.jl:14) */
int lrn_ip_add_diag(lrn_ctx* ctx, int ilmi, int which, double eps);
/* prepare_W on the resident X, S (src/prepare_W.jl:28-94); info as lrn_prepare_w */
int lrn_ip_prepare_w(lrn_ctx* ctx, int ilmi, int* info);
/* out = sum_i AA[i]*vec(X[i])   (src/predictor_corrector.jl:12) */
int lrn_ip_aa_x(lrn_ctx* ctx, double* out);
/* Rd[i] = C[i] - S[i] - mat(AA[i]'y)   (src/predictor_corrector.jl:13) */
int lrn_ip_residual_d(lrn_ctx* ctx, const double* y);
/* out = sum_i AA[i]*vec(W(Rd+S)W)   (makeRHS without Rp, src/makeBBBB.jl:221-228) */
int lrn_ip_rhs_pred(lrn_ctx* ctx, double* out);
/* lrn_ip_aa_x and lrn_ip_rhs_pred in one call: aax_out = sum_i AA[i]*vec(X[i]) (for Rp, src/predictor_corrector.jl:12) and
 * out as lrn_ip_rhs_pred (src/makeBBBB.jl:221-228), with dense constraint data read ONCE for both -- on the 128 GB
 * instance every pass over it costs 25 ms.  The residual Rp is not needed between :12 and :44. */
int lrn_ip_rhs_pred2(lrn_ctx* ctx, double* aax_out, double* out);
/* out = sum_i AA[i]*my_kron(G,G, G'RdG + D - sigma_mu./D - RNT)   (src/predictor_corrector.jl:186) */
int lrn_ip_rhs_corr(lrn_ctx* ctx, double sigma_mu, double* out);
/* delS, delX and the per-block step lengths alpha[nlmi], beta[nlmi]
 * (src/predictor_corrector.jl:248-291; eigmin: Lanczos Ritz value, Cholesky-certified, on the device) */
int lrn_ip_find_step(lrn_ctx* ctx, int predict, double sigma_mu, double tau, const double* dely,
                     double* alpha, double* beta);
/* predict=1: Xn, Sn, RNT with the per-block steps, trXnSn[nlmi] returned (:302-311);
 * predict=0: X, S updated and re-symmetrised with alpha[0], beta[0] (:313-322) */
int lrn_ip_update(lrn_ctx* ctx, int predict, const double* alpha, const double* beta, double* trXnSn);
/* per block 5 numbers: <X,S>, eigmin(X), eigmin(S), ||Rd||_F, <C,X>
 * (find_mu src/Solvers.jl:480-494, check_convergence :496-511) */
int lrn_ip_stats(lrn_ctx* ctx, double* out5);
/* smallest eigenvalue of a symmetric n x n matrix: steps != NULL -> the plain Lanczos Ritz value (unit
 * test of the kernel); steps == NULL -> the Cholesky-certified value lrn_ip_find_step / lrn_ip_stats use
 * (eigmin of src/predictor_corrector.jl:272,285 and src/Solvers.jl:503,505) */
int lrn_dbg_eigmin(lrn_ctx* ctx, int n, const double* M, double* lam, int* steps);
/* k largest eigenpairs (ascending; U_top n x k column-major, may be NULL), smallest eigenvalue and
 * trace of a symmetric matrix: what the preconditioner setup consumes of `eigen(W)`
 * (src/Solvers.jl:642-650,706-722); unit test of the Lanczos path (option "prec_eig") */
int lrn_dbg_lanczos(lrn_ctx* ctx, int n, int k, const double* M, double* lam_top, double* U_top,
                    double* lam_min, double* trace, int* steps);

/* copy one msz x msz (or msz) array of the resident state of block il to `out` (tests of the scaling):
 * name = "W", "Si", "G", "Gi", "D", "DDsi" (valid after the SVD route), "X", "S", "delX", "delS", "RNT",
 * and, after the eigen-free route (option "nt_mode" = 1, the default of lrn_ip_prepare_w; src/prepare_W.jl:28-94
 * without the singular vectors): "LX", "LXi", "LS", "LSi" (Cholesky factors and their inverses), "Yh", "Zh"
 * ((K/c)^1/2, (K/c)^-1/2 for K = L_X' S L_X), "Qm" (G RNT G' of the predictor).  *flag (may be NULL) receives 1 when the
 * current scaling of the block is the eigen-free one, and c = lrn_get_timing("ns_c") its scale. */
int lrn_dbg_get_block(lrn_ctx* ctx, int il, const char* name, double* out, int* flag);
/* Host only (no context, no GPU): k-th smallest eigenvalue (k = 0 .. m-1) of the symmetric tridiagonal matrix with diagonal
 * a[0..m) and off-diagonal b[0..m-1), as the Lanczos drivers of the step-length rule and of the H_alpha setup compute it after
 * every batch of steps (csrc/tridiag.h; reference: eigmin(XXX), src/predictor_corrector.jl:272,285, and eigen(W),
 * src/Solvers.jl:642,706).  upper (may be NULL): a value believed to be >= that eigenvalue (checked, never trusted);
 * width: how far it is expected to lie below (<= 0: unknown).  evals (may be NULL): Sturm counts evaluated. */
int lrn_dbg_tridiag_eig(int m, const double* a, const double* b, int k, const double* upper, double width, double* eig,
                        int64_t* evals);

/* ---- multi-GPU: one process per GPU, the exchange inside the library ---------------------------------------
 * The reference is one process (no MPI/NCCL); a sharded run keeps its predictor / corrector loop
 * (src/predictor_corrector.jl:24-40,119-139) unchanged and only creates a communicator:
 *   rank 0: lrn_comm_unique_id(id) -> the launcher distributes the 128 bytes -> every rank: lrn_comm_init(ctx, id, rank, world)
 * (ncclCommInitRank on the context's device; implies lrn_set_shard).  From then on
 *   lrn_schur_assemble  agrees on the assembly path with the other ranks (first call), assembles the rank's share, reduces
 *                       a status word that EVERY rank enters (a rank that failed makes all ranks return an error, nobody
 *                       is left waiting in a collective) and exchanges on the library's stream: one all-reduce of the
 *                       lower triangle, nvar (nvar + 1) / 2 doubles, on the Cholesky path of dense data; one all-gather
 *                       of the owned column blocks otherwise (makeBBBB.jl:24-36, then the replicated cholesky :57);
 *   lrn_pcg, lrn_matvec apply the operator as this rank's rows of W M W plus one all-reduce of the nvar-vector
 *                       (Solvers.jl:582-614) -- the CG recurrence stays on the device on every rank.
 * lrn_comm_init_host: the same entry points over callbacks that reduce / gather HOST buffers (ranks sharing one GPU,
 * launchers whose fabric is MPI or gloo on the CPU); op: 0 sum, 1 min, 2 max; callbacks return 0 on success.
 * lrn_comm_allreduce: in-place all-reduce of `count` doubles (host or device pointer) on the communicator, for the
 * host loop's own replicated scalars. */
typedef int (*lrn_host_allreduce_fn)(void* user, double* buf, int64_t count, int op);
typedef int (*lrn_host_allgather_fn)(void* user, const double* send, double* recv, int64_t count_per_rank);
int lrn_comm_unique_id(void* id128);
int lrn_comm_init(lrn_ctx* ctx, const void* id128, int rank, int world);
int lrn_comm_init_host(lrn_ctx* ctx, int rank, int world, lrn_host_allreduce_fn allreduce,
                       lrn_host_allgather_fn allgather, void* user);
int lrn_comm_destroy(lrn_ctx* ctx);
int lrn_comm_allreduce(lrn_ctx* ctx, double* buf, int64_t count, int op);

/* ---- measurement ----------------------------------------------------------------------- */
/* milliseconds of the named phase in the last call that ran it, measured with HIP events
 * on the context's stream ("gemm1","gemm2","gemm3","sparse","assemble","factor","solve",...);
 * returns LRN_ERR_ARG for an unknown key.  The reference's TimerOutputs section names are accepted as aliases:
 * "BBBBone1" (mul!(tmp1,W,A_i), src/makeBBBB.jl:87) = gemm1, "BBBBone2" (tmp1*W, :90) = gemm2, "BBBBone3"
 * (AA*vec(tmp), :94) = gemm3 + reduce3, "BBBBone4" (:98, the scatter into BBBB) = 0: it is the GEMM3 epilogue,
 * "BBBBone" (:86), "BBBBthree" (:140) = sparse, "BBBB_rank1" (:2) = rank1, "BBBBs" (:30) = assemble, "Ax"
 * (src/Solvers.jl:583) = matvec, "prec" (:676) = prec_setup, "prep W SVD" (src/prepare_W.jl:37) = prepw_svd,
 * "CG predictor" / "CG corrector" (src/predictor_corrector.jl:130,234) = pcg, "find step corrector" (:243). */
int lrn_get_timing(lrn_ctx* ctx, const char* key, double* ms);
/* launch / event counters of the same phases; "shard_bs" returns the column-block width of the Schur
 * sharding in effect (option "shard_bs": 0 = auto, two 128-aligned blocks per rank).  Option "cg_lowrank":
 * "hop_assemble_lowrank" (assemblies of the CG operator's H in mode 1; "hop_assemble" counts them too), "op_factored_cg"
 * (blocks the matrix-free CG operator took in factor form, per application), "prec_ts_factored" (STATE: the blocks whose
 * part of ts came from the factors in the last lrn_prec_setup) */
int64_t lrn_get_count(lrn_ctx* ctx, const char* key);
/* FP64 MFMA issue-rate probe (TFLOP/s of a register-only v_mfma_f64_16x16x4_f64 loop; an 8 ms warm-up launch and 43 ms
 * timed, so that the clock's ramp after an idle period is not what is measured: 77.3-77.8 on an MI355X) */
int lrn_mfma_f64_peak(lrn_ctx* ctx, double* tflops);
/* placement probe: launches a (nx, 1, nz) grid of 256-thread workgroups and writes, for workgroup
 * (x, z), the XCC (XCD) id the hardware ran it on (HW_REG_XCC_ID) to out[x + nx*z] (host or device int32);
 * with hold_us > 0 every workgroup spins that long so that a whole wave of workgroups is resident at once */
int lrn_xcc_probe(lrn_ctx* ctx, int nx, int nz, int hold_us, int32_t* out);
/* streaming-copy probe: achieved HBM GB/s of a 16 B/lane device copy of `bytes` */
int lrn_hbm_copy_peak(lrn_ctx* ctx, int64_t bytes, double* gbps);

/* ---- building blocks exposed for unit tests (tests/ only) ------------------------------ */
int lrn_dbg_gemm(lrn_ctx* ctx, int transA, int transB, int M, int N, int K, double alpha,
                 const double* A, int lda, const double* B, int ldb, double beta, double* C,
                 int ldc, int flags, int ksplit);
/* One function of csrc/products.hip (or symadd of matops.hip) on host operands, on the context's stream.
 * A, Bm: n x n column-major.  kind 0: pgemm_nt(A, Bm, out0, tri, alpha, Ct = out1 or NULL)
 *        1: pgemm_nt_sym(A, Bm, out0, alpha, tri)
 *        2: gemm_nt_sym_ns(A, Bm, scratch, a, T = out0, part) ; *scalar = part[0] + ... + part[npart-1], added on the host in index order
 *        3: gemm_nt_slabs(A, Bm, out0, alpha) + slabs_to_c_and_ct(out0, out1) ; *scalar = number of slabs the product came back in
 *        4: prod_slabs(A, Bm, work, alpha, tri) + symadd (scale = a, out = out0, dotp = A, grid = min(1024, tile pairs)) ;
 *           *scalar = sum of part[] in index order
 * tri: 0 or one of the four triangular-K flags (64, 128, 1024, 2048).  out0 (and out1 where given) are uploaded before the
 * call, so an element that no kernel writes comes back as the caller left it.  out1: required by kind 3; scalar: by 2, 3, 4. */
int lrn_dbg_product(lrn_ctx* ctx, int kind, int n, const double* A, const double* Bm, double alpha, double a, int tri,
                    double* out0, double* out1, double* scalar);
/* What lrn_dbg_gemm would launch for the same arguments, decided on the host alone (no context, no device): out6 =
 * { kernel, tile side, grid x, grid z, dynamic LDS bytes, split-K slabs }.  kernel: 0 nothing, 1 / 2 register-staged
 * 64 / 128 tile, 3 direct-to-LDS 128 tile, 4 64-tile DMA pipeline, 5 K-segment, 6 / 7 / 8 K-contiguous 128 / 160 / strip. */
int lrn_dbg_gemm_plan(int transA, int transB, int M, int N, int K, int lda, int ldb, double beta, int ldc, int flags,
                      int ksplit, int* out6);
/* What the Cholesky path of lrn_schur_assemble decides before its launches for a block of side msz with nd dense constraints on
 * rank `rank` of `world` (csrc/schur_plan.h), on the host alone (no context, no device).  pcap_hint: the GEMM1'/GEMM2' batch the
 * memory test found room for; opts6 = option values { p_batch, gemm3_tile, gemm3_ksplit, gemm3_sched, gemm3_strip, gemm_no_skip }.
 * out10 = { c0, c1 (this rank's columns of the matrix variable; -1, -1: an idle rank), doubles per P block, its leading
 * dimension, matrices per GEMM1'/GEMM2' launch, GEMM3' tile side, number of GEMM3' launches, tile class of the first, of the
 * second, split-K slabs }; kb, ke, weights (64 entries each): the K-chunk range [kb, ke) and the slab weight (1 / 2) of every
 * split; shares3 = this rank's share of the useful work of GEMM1', GEMM2', GEMM3'. */
int lrn_dbg_schur_chol_plan(int msz, int nd, int rank, int world, int64_t pcap_hint, const int* opts6, int64_t* out10, int* kb,
                            int* ke, int* weights, double* shares3);
/* What lrn_upload_model lays out for one LMI block, its rank-one factors and the linear part (csrc/model_layout.h), on the host
 * alone (no context, no device).  The arrays are the arguments of lrn_upload_model for one block: AA (nvar x msz^2 CSC, 1-based),
 * sigma = the block's column of sigmaA (1-based), qA = its first entry of qA; pos_space = 1 for a model of one block; B and
 * C_lin may be NULL (nlin = 0).  dense_threshold: the option of that name; free_bytes: what hipMemGetInfo would report.
 * name: "sigma" "ipos" "nnz" "qA" "npos_nz" "nd" "q_wave" "ent_ptr" "ent_r" "ent_c" "ent_v" "hidx" "cq_q" "cq_ptr" "cq_j" "cq_v"
 * "sp_ok" "pc_ptr" "pc_r" "pc_t" "ent_t" "sp_long_cols" | "b_ptr" "b_col" "b_val" | "cl_ptr" "cl_row" "cl_rown" "lp_r" "lp_c"
 * "lp_ptr" "lp_l" "lp_w" "cr_ptr" "cr_col" "cr_val" (ctx.h describes them).  *count = the length of that array; its elements go to
 * iout (integers, widened to int64) or dout (ent_v, cq_v, b_val, lp_w, cr_val) where the pointer is not NULL: call once with
 * both NULL for the length.  A failed check of the upload returns its code and writes its message to msg (msg_len bytes). */
int lrn_dbg_model_layout(const char* name, int msz, int nvar, const int64_t* AA_colptr, const int64_t* AA_rowval,
                         const double* AA_nzval, const int64_t* sigma, int64_t qA, int pos_space, double dense_threshold,
                         int64_t free_bytes, const int64_t* B_colptr, const int64_t* B_rowval, const double* B_nzval, int nlin,
                         const int64_t* Clin_colptr, const int64_t* Clin_rowval, const double* Clin_nzval, int64_t* count,
                         int64_t* iout, double* dout, char* msg, int msg_len);
/* The same for lrn_upload_lowrank (V, d, khat: its arguments; NULL / 0: none) and lrn_upload_diag (rows, nrows) on a block whose
 * constraint -> position map is ipos (0-based) and whose positions [0, npos_nz) are stored.  name: "v_ptr" "v_col" "v_val" "v_w"
 * (doubles: v_val, v_w), "v_partial", "stored_and_factored" (the first stored position with a weighted factor column, or -1) |
 * "dg_h" "dg_nat" "dg_of_pos".  Messages name block 0. */
int lrn_dbg_factor_layout(const char* name, int msz, int nvar, const int64_t* ipos, int npos_nz, int pos_space, int khat,
                          const int64_t* V_colptr, const int64_t* V_rowval, const double* V_nzval, const double* d, int64_t nrows,
                          const int64_t* rows, int64_t* count, int64_t* iout, double* dout, char* msg, int msg_len);
/* The keys of lrn_set_option (csrc/options.h), on the host alone.  lrn_dbg_option_name: the index-th key it accepts -- the value
 * options of the table, then the keys the context serves itself -- or NULL past the end. */
const char* lrn_dbg_option_name(int index);
/* lrn_set_option(key, value) on a context that exists on the host only (no stream, no device call, one block), started from
 * hop_version = 7, t_cap = 5 and p_cap = 6 of its block and one entry in the timing and the count map.  *rc = what
 * lrn_set_option returned, msg = the error text it left (msg_len bytes), opt_bytes = the first opt_cap bytes of the options
 * struct afterwards, *opt_size = its size, watched14 = { hop_version, profile, lz_res_limit, lz_wh_left, lz_wh_fired, lz_wh_run,
 * lz_wh_step, lz_wh_wg, shard_bs_opt, shard_bs, t_cap, p_cap, timing entries, count entries }.  key = NULL: nothing is set (the
 * defaults).  Returns LRN_ERR_ARG for the keys whose action needs a device or a communicator: "comm_fail_ensure",
 * "detect_release". */
int lrn_dbg_option_probe(const char* key, double value, int* rc, char* msg, int msg_len, unsigned char* opt_bytes, int opt_cap,
                         int* opt_size, int64_t* watched14);
int lrn_dbg_mfma_probe(lrn_ctx* ctx, const double* A16x4, const double* B4x16, double* D16x16);
int lrn_dbg_potrf(lrn_ctx* ctx, int n, double* A, int* info);
int lrn_dbg_potrs(lrn_ctx* ctx, int n, const double* A, const double* b, double* x, int* info);
int lrn_dbg_trsm(lrn_ctx* ctx, int n, int nrhs, int trans, const double* A, double* B, int* info);
/* One-sided Jacobi SVD of A (n x n, column-major): U_sigma = A V, sigma = its column norms (unsorted).  V may be NULL: the
 * rotations are then not accumulated, as in every call the solver itself makes; U_sigma, sigma and sweeps are the same. */
int lrn_dbg_svd_jacobi(lrn_ctx* ctx, int n, const double* A, double* U_sigma, double* V,
                       double* sigma, int* sweeps);

#ifdef __cplusplus
}
#endif
#endif /* LORAINE_HIP_H */
