// Library context: device-resident model data, NT scaling, Schur matrix, solver state.
#pragma once
#include <map>

#include "chol.h"
#include "lrn_common.h"

namespace lrn { struct Prec; struct Comm; }

struct LmiBlock {
  int msz = 0;
  long nent = 0;            // total stored entries (sparse lists)
  // --- constraint data in sigma-POSITION order (position p <-> constraint sigma[p])
  std::vector<int> sigma;   // position -> constraint (0-based)
  std::vector<int> ipos;    // constraint -> position
  std::vector<long> nnz;    // per position
  int qA = 0;               // reference dense/sparse split (positions < qA are "branch 1")
  int nd = 0;               // positions [0,nd): T_i = W A_i W by MFMA GEMM, A stored dense
  int q_wave = 0;           // positions [nd,q_wave): wave-per-pair kernel; [q_wave,n): thread-per-pair
  int npos_nz = 0;          // positions with nnz > 0 form the prefix [0,npos_nz)
  long p_cap = 0, t_cap = 0; // batch capacities (matrices) of the P / T workspaces for this block
  lrn::DBuf ent_ptr;        // int64 [nvar+1]
  lrn::DBuf ent_r, ent_c;   // int32 [nent]
  lrn::DBuf ent_v;          // double [nent]   value of A_j (= -AA)
  lrn::DBuf Adense;         // double [nd * msz^2], slot s = position s
  // route of the passes over Adense, set where Adense is filled (dataops.hip::dense_route_setup) and reset with it:
  // tri = column tails only (symmetric data), stream = 16-byte loads over both triangles, scalar = one element per lane
  enum DenseRoute { DENSE_SCALAR = 0, DENSE_STREAM, DENSE_TRI };
  DenseRoute dense_route = DENSE_SCALAR;
  lrn::DBuf tri_tab;        // DENSE_TRI: chunk table of the column tails (dataops.hip::TriChunk), tri_nch entries
  int tri_nch = 0;
  lrn::DBuf hidx;           // int32 [nvar] position -> row/col index of the Schur matrix
  lrn::DBuf sigma_d, ipos_d; // int32 [nvar] device copies of sigma / ipos
  // local route of the sparse owners (option "pair_local", localops.hip; the lists: model_layout.h::block_local): owners
  // [loc_lo, loc_hi).  The host lists wait here from the upload on; the first assembly by that route moves them to the device
  // (loc_ready) and empties them -- a model that never takes the route holds no device copy
  int loc_lo = 0, loc_hi = 0;
  bool loc_ready = false;
  std::vector<long> loc_sptr, loc_aptr;
  std::vector<int> loc_sup;
  std::vector<double> loc_a;
  lrn::DBuf loc_sptr_d, loc_aptr_d, loc_sup_d, loc_a_d;   // int64 [nvar+1], int64 [nvar+1], int32, double
  // long route of the sparse owners (option "pair_long", longops.hip; the lists: model_layout.h::block_long): eligible owners
  // [nd, lg_hi).  As above the host lists wait for the first assembly by that route (lg_ready) and are emptied then; lg_rho, the
  // number of distinct rows of every eligible owner, stays.  The launch plan (work items of the entry kernel, pairs of the reduce
  // and of the MFMA kernel, owner batches and offsets of Zc) is rebuilt when lg_plan_key -- the options and ranges it depends
  // on -- changes.  lg_z: Zc of one batch of owners, lg_part: one partial sum per work item
  int lg_hi = 0;
  bool lg_ready = false;
  std::vector<long> lg_rptr, lg_eptr;
  std::vector<int> lg_rows, lg_ec, lg_rho;
  std::vector<double> lg_ev;
  std::vector<long> lg_plan_key, lg_item_ptr, lg_pair_ptr, lg_mf_ptr;   // the three: [owners + 1] ranges of the tables by owner
  std::vector<int> lg_batch;                                             // owner index at which each batch of Zc starts, and the end
  lrn::DBuf lg_rptr_d, lg_rows_d, lg_eptr_d, lg_ec_d, lg_ev_d;          // int64, int32, int64, int32, double
  lrn::DBuf lg_items_d, lg_pairs_d, lg_mf_d, lg_zoff_d, lg_z, lg_part;  // int4, int4, int2, int64 [owners], double, double
  // stored columns of AA (sparse constraints only) for the deterministic AA'x gather
  long ncq = 0;
  lrn::DBuf cq_q, cq_ptr;   // int64 [ncq], [ncq+1]
  lrn::DBuf cq_j;           // int32 constraint (natural index)
  lrn::DBuf cq_v;           // double AA value
  // sparsity pattern of mat(AA'x) = the stored columns above, when no constraint is stored dense and
  // the pattern is symmetric: sparse-aware mat-vec (dataops.hip, Z = W M W only where AA needs it)
  bool sp_ok = false;
  std::vector<int> sp_long_cols;   // pattern columns with more than 64 stored entries (small-msz sparse mat-vec)
  lrn::DBuf pc_ptr;         // int64 [msz+1] pattern column -> range of stored columns
  lrn::DBuf pc_r;           // int32 [ncq] row of stored column t
  lrn::DBuf pc_t;           // int32 [ncq] stored column holding the transposed entry
  lrn::DBuf ent_t;          // int32 [nent] constraint entry -> stored column
  lrn::DBuf Mv, Zs;         // double [ncq] values of M and of Z on the pattern
  // rank-one factors (datarank = -1): CSR by constraint (natural order)
  bool has_B = false;
  long bnnz = 0;
  lrn::DBuf b_ptr, b_col, b_val;
  // rank-k factors (datarank >= 1, lrn_upload_lowrank): A_k = V_k diag(d_k) V_k', every constraint padded to lr_khat
  // columns; CSR by factor column h * lr_khat + p in H index order (h = position when nlmi == 1), weights in that order
  int lr_khat = 0;
  bool has_V = false;
  long vnnz = 0;
  lrn::DBuf v_ptr, v_col, v_val, v_w;
  bool v_partial = false;   // some constraint with stored entries has no weighted factor column: the factors are not the whole
                            // block.  Not factored: mode 1 assembles the block from its entries (AA is complete); factored: hybrid
  // --- NT scaling state (device, msz x msz col-major)
  lrn::DBuf X, S, W, G, Gi, Si, D, DDsi;
  lrn::DBuf Vprev;          // right singular vectors of the previous prepare_W (Jacobi warm start)
  // --- device-resident iterate (ipstep.hip; its Lyapunov solve: lyap.hip): C, residual, directions, predictor point
  lrn::DBuf Cd, Rd, delX, delS, Xn, Sn, RNT, t0, t1, t2;
  bool resident = false;
  bool have_Vprev = false;
  bool have_W = false, have_G = false;
  // --- eigen-free NT scaling (prepw.hip::prepare_w_ns, option nt_mode = 1): L_X and its transpose, Yh = (K/c)^1/2,
  // Zh = (K/c)^-1/2, Ki = (K/c)^-1 for K = L_X' S L_X; per direction Bs = L_X' dS L_X, TX = L_X^-1 dX L_X^-T;
  // Qm = G RNT G' of the predictor; Lyapunov-CG work; dense copy of the rank-one factors
  lrn::DBuf LXf, LXt, LSf, Yh, Zh, Ki, Bs, TX, Qm, lyap, Bd;
  double ns_c = 1.0;        // the scale c of K (host copy)
  bool nt_free = false;     // the current scaling came from prepare_w_ns: G, Gi, D, DDsi are NOT valid
  bool chol_valid = false;  // LXf, LSf hold the Cholesky factors of the CURRENT X, S (nt_factor; lrn_ip_stats computes them as its
                            // positive-definiteness certificate, the next prepare_w_ns re-uses them)
  bool have_Bd = false;     // dense copy of the rank-one factors (rank-one assembly from W)
  lrn::DBuf Vd;             // dense copy of the rank-k factors, msz x (nvar * lr_khat) (dense U product, assembly from W)
  bool have_Vd = false;
  // rank-class route of the rank-k assembly (option "lowrank_ragged", raggedops.hip, ragged_plan.h): rg_Rc = the compacted
  // column count, counted at lrn_upload_lowrank; the plan's device copies and the compacted dense factors Vc (msz x rg_Rc) are
  // built at the first assembly by that route (rg_ready) and dropped by a new upload
  long rg_Rc = 0, rg_ntiles = 0;
  int rg_ncls = 0;
  bool rg_ready = false;
  lrn::DBuf rg_src, rg_wc, rg_gh, rg_tiles, Vc;   // int64 [rg_Rc], double [rg_Rc], int32 [groups], RaggedTile [rg_ntiles]
  // option "ragged_ops" (the data operators on the compacted columns, fac_cols.h, raggedops.hip): column -> group, the segment starts and
  // first groups of the seven classes 64 .. 1 of ragged_plan.h (rg_grp0[7] = the number of groups), and Yc = W Vc (msz x rg_Rc)
  // of the scaling `Yc_version` for option "fac_op_scaled" -- all built with the plan, on the first call of either route
  lrn::DBuf rg_cg;                                // int32 [rg_Rc]
  long rg_seg0[7] = {};
  int rg_grp0[8] = {};
  lrn::DBuf Yc;
  long Yc_version = -1;
  // options "ragged_cross" / "ragged_ts" (cross terms of the assembly, ts of H_alpha on the compacted columns): H index -> group,
  // -1 for a constraint of rank 0 -- the inverse of rg_gh, built with the plan
  lrn::DBuf rg_hg;                                // int32 [nvar]
  // factored block (lrn_set_factored): the factors ARE the constraint data -- AA vec(.) and mat(AA' .) go through Vd
  // (dataops.hip, "factor form"), the Schur matrix through mode 1 only.  Pure: AA has no entry.  Hybrid: a few constraints
  // are stored instead (rows of AA, positions [0, npos_nz) as everywhere) and have weight-0 factor columns; every constraint
  // is exactly one of the two.  The stored-entry kernels serve the stored part, schur_factored.hip::assemble_cross the mixed terms
  bool factored = false;
  bool hybrid() const { return factored && npos_nz > 0; }
  // option "fac_op_scaled" (pure factored block): Y = W Vd (msz x nvar khat) of the scaling `Ys_version` (schur_factored.hip::fac_scaled_y)
  lrn::DBuf Ys;
  long Ys_version = -1;
  // diagonal parts (lrn_upload_diag, factored blocks only): constraint A_k = diag(a_k) + V_k D_k V_k' for the dg_n constraints
  // ("diagonal rows") listed there -- factored positions, never stored ones.  Row s: H index dg_h[s], natural constraint
  // number dg_nat[s], column s of dg_a (msz x dg_n, column-major, +a); dg_of_pos[p] = row of position p or -1 (diagops.hip)
  int dg_n = 0;
  lrn::DBuf dg_h, dg_nat, dg_of_pos;   // int32 [dg_n], [dg_n], [nvar]
  lrn::DBuf dg_a;                      // double [msz * dg_n]
  // --- every device buffer above, named once, in three lists: the rank-class plan (dropped with its scalars by
  // lrn::drop_rank_classes), the diagonal parts (lrn::drop_diag), and all the others.  A DBuf added to the block goes into one
  std::vector<lrn::DBuf*> rank_class_bufs() { return {&rg_src, &rg_wc, &rg_gh, &rg_hg, &rg_tiles, &rg_cg, &Vc, &Yc}; }
  std::vector<lrn::DBuf*> diag_bufs() { return {&dg_h, &dg_nat, &dg_of_pos, &dg_a}; }
  std::vector<lrn::DBuf*> other_bufs() {
    return {&ent_ptr, &ent_r, &ent_c, &ent_v, &Adense, &tri_tab, &hidx, &sigma_d, &ipos_d, &cq_q, &cq_ptr, &cq_j, &cq_v,
            &pc_ptr, &pc_r, &pc_t, &ent_t, &Mv, &Zs, &b_ptr, &b_col, &b_val, &v_ptr, &v_col, &v_val, &v_w,
            &X, &S, &W, &G, &Gi, &Si, &D, &DDsi, &Vprev, &Cd, &Rd, &delX, &delS, &Xn, &Sn, &RNT, &t0, &t1, &t2,
            &LXf, &LXt, &LSf, &Yh, &Zh, &Ki, &Bs, &TX, &Qm, &lyap, &Bd, &Vd, &Ys, &loc_sptr_d, &loc_aptr_d, &loc_sup_d, &loc_a_d,
            &lg_rptr_d, &lg_rows_d, &lg_eptr_d, &lg_ec_d, &lg_ev_d, &lg_items_d, &lg_pairs_d, &lg_mf_d, &lg_zoff_d, &lg_z, &lg_part};
  }
};

struct lrn_ctx;
namespace lrn { void update_shard_bs(lrn_ctx* c); }      // ctx.hip
void lrn_free_model(lrn_ctx* c);                         // model.hip

// lrn_set_option knobs: per context (two contexts of one process -- Julia threads, tests -- do not see each
// other's settings)
struct LrnOptions {
  double dense_threshold = -1.0;  // < 0: cost model decides which constraints are stored dense
  long t_batch = 0, p_batch = 0;  // matrices per T workspace / per GEMM1-2 launch (0 = auto)
  int prec_eig = 0;               // 0 auto (Lanczos for msz >= 256), 1 Jacobi eigendecomposition, 2 Lanczos
  double pivot_boost = 1e-12;     // lrn_schur_factor: pivots <= pivot_boost * diag (rounding noise of a matrix that is
                                  // PSD by construction) are boosted instead of failing, counted in "chol_boosted";
                                  // 0 = strict Cholesky, the literal LAPACK behaviour
  int schur_chol = -1;            // -1 auto, 0 never, 1 whenever the data allows it, 2 T-via-L only
  int schur_plan = -1;            // multi-GPU: the exchange all ranks agreed on (-1 undecided, 0 all-gather of
                                  // Schur column blocks, 1 all-reduce of partial sums); see lrn_schur_plan
  int gemm3_ksplit = 0;           // split-K factor of GEMM3 / GEMM3' (0 = auto)
  int gemm_dyn_masks = 0;         // measurement only: GEMM_DYN_MASKS on GEMM1'/2'
  int gemm_lab = 0;               // measurement only: GEMM_LAB_* bits (<< 20) on GEMM1'/2'; bit 4: every tile walks the whole K
                                  // range (tools/gemm12_overhead.py)
  int gemm1_diag = 1;             // GEMM1': diagonal tiles compute only the blocks GEMM2' reads (GEMM_DIAG_LOWER_Z); 0: all
  int gemm_no_skip = 0;           // measurement only: GEMM1'/2'/3' compute every 16x16 block (GEMM_NO_SKIP)
  int gemm3_sched = 1;            // 1: one launch, regular tiles of every split first, short tiles last; 0: two launches
  int gemm3_strip = 1;            // GEMM3': nd % 128 in (0, 32] -> last tile row of height 128 + nd % 128 (second launch)
  int gemm3_tile = 0;             // workgroup tile of GEMM3': 0 auto, 128, 160
  int gemm3_stagger = 0;          // K-walk stagger of GEMM3' in chunks of 16 (GemmDesc::kstagger)
  int jacobi_inner = 0;           // sweeps over the pair's Gram matrix per round (more did not cut the outer sweeps: 1)
  int jacobi_wgs = 0;             // workgroups per Gram / apply launch the row chunking aims for: 0 auto
  int jacobi_block = 0;           // column block width: 0 auto (32 for n >= 5000), 16, 32
  int jacobi_cross = 1;           // block Jacobi: cross-pair rotations only outside round 0 of a sweep
  int prepw_streams = 1;          // prepare_W: the S side and the Gi solve on a second stream beside cholesky(X) / the SVD / the GEMMs
  int lz_resident = 1;            // Lanczos steps of the eigmin searches (n <= 1024) as resident launches of 16 steps: M in registers, relaxed-atomic exchange
  int eigmin_pair = 2;            // the two eigmin calls of a step-length search: 2 = one launch per pair of Lanczos steps, 1 = two streams, 0 = one after the other
  double jacobi_early = 3e-8;     // a sweep whose rotated column pairs were all closer to orthogonal than this ends the SVD
  bool jacobi_warm = true;
  int shard_passes = 1;           // multi-GPU: split AA*vec(.) and mat(AA'x) over dense constraints by rank (+ one all-reduce)
  int prec_inv = -1;              // H_alpha: SMW core applied through an explicit inverse + one refinement step (1), the two
                                  // triangular solves (0), auto (-1: explicit from k msz = 256 on)
  int nt_mode = 1;                // lrn_ip_prepare_w: 1 = eigen-free NT scaling (Newton-Schulz square roots of K = L_X'SL_X, Lyapunov
                                  // solve for the second-order term; falls back to the SVD when it does not converge), 0 = SVD always
  double ns_l0 = 2e-3;            // Newton-Schulz schedule: assumed lower end of spec(K)/c (slower, never wrong, when cond(K) is larger)
  int ns_lanczos = 1;             // Newton-Schulz: scale c and schedule end l from a 24-step Lanczos run on K (blocks of side >= ns_lanczos_min)
  int ns_lanczos_min = 1500;
  int ns_dual = -1;               // Newton-Schulz: transposed twins from the GEMM epilogue (1), a transpose pass (0), auto (-1)
  int ns_maxit = 40;              // Newton-Schulz steps before the SVD fallback
  double lyap_tol = 1e-12;        // relative residual of the Lyapunov CG (second-order term of the corrector)
  int lyap_maxit = 300;
  int lyap_form = 1;              // 1: the better conditioned equivalent equation (Yh/s + s Zh) R + R (.) = C/s + s Zh C Zh, 0: Yh R + R Yh = C
  int pair_lanes = 0;             // pair_wave_kernel: lanes per Schur entry, 0 auto (16 for short products), 16, 64
  int pair_local = 0;             // sparse owners with a small support, [loc_lo, loc_hi) of a block, through the dense A[S, S] on the
                                  // MFMA (localops.hip): 1, the pair kernels as always: 0.  One GPU ("pair_local_skipped" otherwise)
  int pair_local_min = 36;        // read by lrn_upload_model: entries from which on a sparse owner may take that route (model_layout.h)
  int pair_long = 0;              // long sparse owners (a trace row, a band), [nd, lg_hi) of a block, from Z_i = (A_i W) on their rows
                                  // (longops.hip): 1, the pair kernels as always: 0.  One GPU ("pair_long_skipped" otherwise)
  int pair_long_min = 64;         // read by lrn_upload_model: entries from which on a sparse owner may take that route (measured:
                                  // model_layout.h, PAIR_LONG_MIN)
  long pair_long_split = 1L << 15; // products nnz_j rho_i of a pair per slice of the entry kernel (measured: PAIR_LONG_SPLIT)
  int pair_long_mfma = 1;         // partners with local lists (support <= 32) through the FP64 MFMA: 1, through the entry kernel: 0
  double pair_long_scratch_mb = 1024.0;   // cap of Zc, the scratch of that route; an owner that does not fit: the route is skipped
  int matvec_sparse = 0;          // 0 auto, 1 dense GEMM path, 2 sparse path whenever the pattern allows
  int shard_products = 1;         // multi-GPU: the n^3 products of the resident path (Newton-Schulz, Lyapunov CG, step) by
  int shard_products_min = 4096;  // column blocks + all-gather from this matrix side on (one product of 10^4: 31 ms; below, the
                                  // all-gather costs more than the product)
  int prec_dense = 0;             // H_alpha inside lrn_pcg as ONE dense symmetric matrix M^-1 (nvar <= 8192): 0 auto (cost model), 1 never, 2 always
                                  // (also in lrn_prec_apply)
  int wmw_pattern_min = 1500;     // right-hand sides AA vec(W M W) with all constraints sparse: from this side on through the
                                  // pattern entries of W M W (one n^3 product instead of two)
  int profile_ops = 0;            // measurement: time every AA vec(.) / mat(AA' .) by itself ("aa_times", "aa_times2", "aat_to_mat";
                                  // synchronises: not for solves; tools/factored_pass_times.py)
  int profile_symv = 0;           // measurement: time every application of H x by itself (synchronises: not for solves)
  int matvec_h = 0;               // CG operator through the assembled Schur matrix (hop.hip): 0 auto (cost model), 1 never
                                  // (the matrix-free MyA always), 2 always
  int pcg_lookahead = 2;          // lrn_pcg: iterations the host queues beyond the one whose convergence test it has read
  int fac_cross_lds = -1;         // cross terms of a hybrid factored block: the column of Y staged in LDS (1, where it fits), read from
                                  // global memory (0), by the column length (-1)
  int lowrank_form = -1;          // rank-k assembly: U = G' V (or W V) by a sparse gather (0), one dense MFMA product (1), by the
                                  // factors' density (-1)
  int cg_lowrank = 0;             // CG path (kit = 1) from the rank-k factors of a covered block (cg_lowrank_covered): 0 never (the
                                  // entry routes, bit for bit), 1 always, -1 the static cost model of hop.hip decides per piece --
                                  // the mode of the assembled-matrix operator, the form of the matrix-free operator, the route
                                  // of the H_alpha setup.  Ignored with world > 1
  int cg_factored = 0;            // CG path (lrn_matvec, lrn_prec_setup, lrn_prec_apply, lrn_pcg) on factored blocks: 0 refused (the
                                  // state error of cgops.hip::no_factored), 1 accepted on one GPU -- pure, hybrid and mixed models
  int cg_diag = 0;                // ... on factored blocks WITH diagonal parts (lrn_upload_diag): 0 refused whatever cg_factored says (the
                                  // state error of cgops.hip::no_diag), 1 accepted where cg_factored accepts the block -- ts of
                                  // H_alpha gets the diagonal-row term (diagops.hip::ts_diag); lrn_matvec_partial stays refused
  double hop_max_mb = -1.0;       // budget of the assembled-matrix operator in MiB: H (nvar^2 * 8 bytes) above it is not assembled
                                  // ("hop_over_budget").  -1: none for a model without a factored block; with one, the free device
                                  // memory minus the mode-1 workspace
  int fac_op_scaled = -1;         // matrix-free operator of a pure factored block through Y = W Vd (no W M W product): 1, the
                                  // composition mat(AA' x) -> W M W -> AA vec(.): 0, cost model (hop.hip::fac_op_scaled_on): -1
  int fac_quadform = -1;          // AA vec(Z) of a factored block inside the CG operator by the fused quadratic form of facops.hip
                                  // (Q = Z Vd never stored): 1, Q and fac_coldot_kernel: 0, cost model: -1
  int lowrank_ragged = 0;         // rank-k assembly of a block of mixed ranks by rank class (raggedops.hip): 1, the padded route: 0.  One
                                  // GPU, and only where the classes are not all khat -- the padded route otherwise ("ragged_fallback")
  int lowrank_wide = 0;           // lrn_upload_lowrank accepts khat 32 and 64 (factored constraints of rank 17 .. 64): 1, refuses them: 0.
                                  // A block uploaded so is assembled by rank class whatever lowrank_ragged says (raggedops.hip)
  int wide_diag = 0;              // diagonal parts on a wide block (khat 32 / 64): 1 = lrn_upload_diag accepts a wide block, a wide
                                  // lrn_upload_lowrank a block that holds diagonal rows, diag_sq groups of 32 and 64 in its MFMA form
                                  // (diagops.hip::diag_sq_wide_mfma_kernel); 0 = the three refuse, as before the option existed
  int ragged_ops = 0;             // AA vec(.) and mat(AA' .) of a block of mixed ranks in factor form on the compacted columns of the
                                  // rank classes (fac_cols.h, raggedops.hip): 1, on the padded layout: 0.  Independent of lowrank_ragged; the
                                  // same conditions, the padded code otherwise ("ragged_ops_fallback")
  int ragged_cross = 0;           // Y = W V and its consumers in the mode-1 assembly of a block of mixed ranks -- the cross terms of a hybrid
                                  // block and of the diagonal parts -- on the compacted columns (Yc = W Vc): 1, on the padded layout: 0.
                                  // Independent of the two above; the same conditions, the padded code otherwise ("ragged_cross_fallback")
  int ragged_ts = 0;              // ts of H_alpha of a block that takes the factor route, P = L' V and T = V' Um, on the compacted columns:
                                  // 1, on the padded layout: 0.  The same conditions, the padded code otherwise ("ragged_ts_fallback")
  int ragged_ops_split = 0;       // K-chunks of ragged_syrk_kernel: 0 auto, 1 .. 16 forced (clamped to the K-steps of the block)
  int diag_sq_mfma = -1;          // squared-operand product of the diagonal parts (diagops.hip::diag_sq): the MFMA tile form (1), the
                                  // rows form, one wave per column group (0), by the number of diagonal rows (-1)
};

struct lrn_ctx {
  int device = 0;
  LrnOptions opt;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;      // second Lanczos run of eigmin_certified_pair (created on first use)
  std::string err;
  int nlmi = 0, nvar = 0, nlin = 0;
  std::vector<LmiBlock> lmi;
  bool pos_space = false;       // Schur matrix kept in sigma-position space (nlmi == 1)
  // linear block C_lin (nvar x nlin) stored by linear constraint (CSC)
  lrn::DBuf cl_ptr, cl_row, cl_val;   // int64 [nlin+1], int32 (Schur-matrix index), double
  lrn::DBuf cl_rown;                  // int32 natural row index
  lrn::DBuf lin_xs;                   // X_lin .* S_lin_inv  [nlin]
  // deterministic gathers (no floating-point atomics): target entries of H with their contributions
  // (C_lin diag(xs) C_lin' term), and C_lin by rows (mat-vec / diagonal of the linear term)
  long lp_n = 0;                      // distinct lower-triangle targets
  lrn::DBuf lp_r, lp_c, lp_ptr, lp_l, lp_w;   // int32 row, col (Schur index); int64 ptr; int32 l; double C[i,l]*C[j,l]
  lrn::DBuf cr_ptr, cr_col, cr_val;   // CSR by natural row: int64 [nvar+1], int32 l, double
  // Schur complement
  lrn::DBuf H;          // assembled (lower triangle authoritative), nvar x nvar
  lrn::DBuf L;          // factor
  lrn::DBuf cholwork;   // workspace of the factorisation: chol_work_doubles(nvar)
  lrn::DBuf info_dev;   // int
  lrn::DBuf v0, v1, v2, v3;   // nvar-vectors (solve scratch)
  lrn::DBuf hdiag;            // diag(H) before the factorisation (pivot boosting)
  bool have_H = false, have_L = false;
  bool H_shifted = false;     // lrn_schur_add_diag since the last assembly: strict Cholesky only
  bool H_partial = false;     // world > 1, Cholesky path: H is this rank's partial SUM (exchange = all-reduce)
  bool H_owned_only = false;  // world > 1: H holds only the column blocks this rank assembled (CG operator, hop.hip)
  // which NT scaling (W of every block, X_lin ./ S_lin) the assembled H belongs to: scal_version counts the changes of the
  // scaling, H_version is its value at the last assembly, H_mode the mode of that assembly (0 general, -1 rank-one, 1 rank-k)
  long scal_version = 0, H_version = -1;
  int H_mode = 0;
  // CG operator through the assembled matrix (hop.hip): the decision taken for scaling `hop_version`, the operator
  // applications counted under the current and the previous scaling (input of the cost model)
  long hop_version = -1;
  bool hop_use = false;
  long cg_cur_iters = 0, cg_prev_iters = 0;
  lrn::DBuf hopbuf;           // partial sums of the triangular mat-vec
  bool lz_no_persist = false; // a resident Lanczos launch gave up waiting for its peers once (lz_record_give_up): launched steps from then on
  long long lz_res_limit = 2000000;   // option "lz_res_limit": ticks of the 100 MHz wall clock a resident workgroup waits for its peers (20 ms)
  // test hook "lz_test_withhold" (one shot): the lz_wh_left-th resident launch from now on has one workgroup of one run keep
  // one step's publication to itself (0: not armed); lz_wh_run 0/1, lz_wh_step 0/1/2 = first/middle/last step of the launch,
  // lz_wh_wg 0/1 = workgroup 0 / the last one
  long lz_wh_left = 0, lz_wh_fired = 0;      // fired: launches the hook has silenced (count "lz_test_withheld")
  int lz_wh_run = 0, lz_wh_step = 0, lz_wh_wg = 0;
  double* pin = nullptr;      // host-mapped words the CG kernels write their exit code to (lrn_pcg), and their device address
  double* pin_dev = nullptr;
  lrn::DBuf cgpart;           // partial sums of the CG recurrence kernels
  hipEvent_t pcg_ev[16] = {};
  // assembly workspaces
  lrn::DBuf P, P2, T, slabs, Hd, BG;
  lrn::DBuf m0, m1, m2, cgbuf;   // msz^2 work matrices (mat-vec / rhs), PCG vectors
  bool BG_ragged = false;        // the last assemble_lowrank left U_c of the rank-class route in BG (not Y = W Vd of the padded layout)
  long rg_last_cols = 0, rg_last_classes = 0, rg_last_tiles = 0;   // the last block assembled by rank class (lrn_get_count "ragged_*")
  long rg_last_chunks = 0;       // K-chunks of the last ragged_syrk_kernel launch (lrn_get_count "ragged_ops_chunks")
  lrn::DBuf facY, facM;          // hybrid factored block: Y = W Vd when U is G' Vd (msz x nvar khat); the stored part of mat(AA' x)
  lrn::DBuf dgP, dgC, dgH, dgT, dgTA;   // diagonal parts (diagops.hip): Ad' (W o W), Ad' (Y o Y) summed over khat, H_DD, T = rows diag(W A_s W), T' Ad
  int T_m = 0;                 // matrix side and block the T workspace was last laid out for
  const void* T_owner = nullptr;
  int T_layout = 0;            // 0: msz^2 per matrix, lower tiles (T_k = W A_k W); 1: packed lower tiles (L' A_k L)
  lrn::DBuf wchol;             // Cholesky path of the assembly: factor of W, its transpose, work
  // shard (multi-GPU): this rank assembles owner columns with (pos / shard_bs) % world == rank
  int rank = 0, world = 1, shard_bs = 128;
  int shard_bs_opt = 0;         // option "shard_bs": 0 = auto (see update_shard_bs)
  // timing of the last assembly / factor / solve (ms, HIP events on ctx stream)
  std::map<std::string, double> timing;
  std::map<std::string, long> counts;
  size_t dev_bytes = 0, dev_bytes_peak = 0;   // device memory held through lrn::ensure (lrn_get_count "device_bytes" / "device_bytes_peak")
  bool profile = true;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t evA = nullptr, evB = nullptr;      // stream <-> stream2 dependencies (prepare_w_block)
  hipStream_t stream3 = nullptr;                // Newton-Schulz: the T Z product beside Y T (prepare_w_ns)
  hipEvent_t evC = nullptr, evD = nullptr;
  // generic scratch
  lrn::DBuf scratch, jscratch, redbuf, redout, lzbuf, lzbuf2, lxbuf, ezbuf;
  lrn::DBuf triw;               // tri-weights of the matrices the dense passes multiply with (2 msz^2)
  lrn::DBuf commvec, commmat;   // multi-GPU: partial results of the sharded passes over dense constraint data
  // lrn_lowrank_detect (detect.hip): the chunk of matrices (host input only), Omega, Y = A Omega, the factors V, and
  // OmT | C | T | d | resid | tile sums | rank | sweeps in one buffer -- independent of the uploaded model
  lrn::DBuf det_A, det_Om, det_Y, det_V, det_small;
  // preconditioner / CG state
  lrn::Prec* prec = nullptr;
  // multi-GPU communicator (comm.hip; lrn_comm_init / lrn_comm_init_host)
  lrn::Comm* comm = nullptr;
  // the buffers that belong to the uploaded model, named once (lrn_free_model releases them with the blocks); every other
  // DBuf above lives as long as the context (lrn_destroy)
  std::vector<lrn::DBuf*> model_bufs() {
    return {&cl_ptr, &cl_row, &cl_val, &cl_rown, &lin_xs, &lp_r, &lp_c, &lp_ptr, &lp_l, &lp_w, &cr_ptr, &cr_col, &cr_val,
            &H, &L, &cholwork, &v0, &v1, &v2, &v3, &hdiag, &P, &P2, &T, &slabs, &Hd, &BG, &m0, &m1, &m2, &cgbuf,
            &facY, &facM, &dgP, &dgC, &dgH, &dgT, &dgTA, &wchol};
  }
};

namespace lrn {
int set_error(lrn_ctx* c, int code, const char* fmt, ...);
int ensure(lrn_ctx* c, DBuf& b, size_t bytes, bool zero = false);
void release(DBuf& b);
bool is_device_ptr(const void* p);
int copy_in(lrn_ctx* c, void* dst_dev, const void* src, size_t bytes);    // src host or device
int copy_out(lrn_ctx* c, void* dst, const void* src_dev, size_t bytes);   // dst host or device
void tic(lrn_ctx* c);
void toc(lrn_ctx* c, const char* key);
// ensure + copy_in: `bytes` from src (host or device) into b, allocated to at least alloc_bytes (>= bytes: some kernels read a
// few bytes past the last element)
int upload(lrn_ctx* c, DBuf& b, const void* src, size_t bytes, size_t alloc_bytes);
template <class T>
int upload(lrn_ctx* c, DBuf& b, const std::vector<T>& v, size_t pad_bytes = 0) {
  return upload(c, b, v.data(), v.size() * sizeof(T), v.size() * sizeof(T) + pad_bytes);
}
// the rank-class plan of a block and everything built with it; the diagonal parts of a block (buffers and scalars)
void drop_rank_classes(LmiBlock& b);
void drop_diag(LmiBlock& b);

// comm.hip
int comm_allreduce(lrn_ctx* c, double* buf_dev, long count, int op);     // in place on c->stream; op 0 sum, 1 min, 2 max
int comm_allgather(lrn_ctx* c, const double* send_dev, double* recv_dev, long count);
int comm_allgather_cols(lrn_ctx* c, double* C_dev, int n, int cb);   // column blocks of width cb of an n x n matrix, in place
int comm_schur_exchange(lrn_ctx* c, int rc_local, bool gather_blocks = true);
int comm_agree_plan(lrn_ctx* c, int mode);
int comm_status_max(lrn_ctx* c, double* words, int nw);
void comm_free(lrn_ctx* c);
void comm_inject_ensure_failure(lrn_ctx* c);
// schur.hip
int schur_assemble(lrn_ctx* c, int mode);
int schur_plan(lrn_ctx* c, int mode);
int schur_factor(lrn_ctx* c, int* info);
int schur_solve(lrn_ctx* c, const double* h, double* dely);
int schur_add_diag(lrn_ctx* c, double eps);
int schur_get(lrn_ctx* c, double* Hout);
// schur_factored.hip
int lowrank_dense_factors(lrn_ctx* c, LmiBlock& b);     // b.Vd from the uploaded rank-k factors (once per upload)
// a wide block: factors padded to 32 or 64 columns (lrn_upload_lowrank under option "lowrank_wide")
inline bool lowrank_wide(const LmiBlock& b) { return b.lr_khat > 16; }
// rank-class route of a block under option "lowrank_ragged": one GPU, some but not all columns survive the compaction.  A wide
// block takes it whatever the option says and also when every column survives (a uniform rank-32 block): the padded product
// sums blocks of at most 16 x 16 and must never see it
inline bool lowrank_ragged_on(const lrn_ctx* c, const LmiBlock& b) {
  if (c->world > 1 || b.rg_Rc <= 0) return false;
  return lowrank_wide(b) || (c->opt.lowrank_ragged != 0 && b.rg_Rc < (long)c->nvar * b.lr_khat);
}
// the compacted columns of a block can stand in for the padded ones: one GPU, some but not all columns survive the compaction
inline bool ragged_cols_usable(const lrn_ctx* c, const LmiBlock& b) {
  return c->world <= 1 && b.rg_Rc > 0 && b.rg_Rc < (long)c->nvar * b.lr_khat;
}
// ... for the data operators (option "ragged_ops"), Y and the cross terms of the mode-1 assembly (option "ragged_cross"), ts of
// H_alpha (option "ragged_ts").  Every path the last two serve refuses world > 1 before it gets here (hybrid blocks, diagonal
// parts, lrn_prec_setup on factored blocks)
inline bool ragged_ops_on(const lrn_ctx* c, const LmiBlock& b) { return c->opt.ragged_ops != 0 && ragged_cols_usable(c, b); }
inline bool ragged_cross_on(const lrn_ctx* c, const LmiBlock& b) { return c->opt.ragged_cross != 0 && ragged_cols_usable(c, b); }
inline bool ragged_ts_on(const lrn_ctx* c, const LmiBlock& b) { return c->opt.ragged_ts != 0 && ragged_cols_usable(c, b); }
// hop.hip: the CG operator through the assembled matrix
// y = H x; qpart (may be null): receives *nq partial sums of x'y (*nq = 0: not formed, e.g. sharded)
int hop_apply(lrn_ctx* c, const double* x_dev, double* y_dev, double* qpart = nullptr, int* nq = nullptr);
int symv_lower(lrn_ctx* c, const double* A_dev, int n, const int* idx, const double* x_dev, double* y_dev,
               double* qpart = nullptr, int* nq = nullptr, bool sharded = false);
bool hop_worthwhile(lrn_ctx* c, long expected_iters);
int hop_prepare(lrn_ctx* c);
// option "cg_lowrank" (hop.hip): the factors of a block are its whole constraint data and the block still has its entries
inline bool cg_lowrank_covered(const LmiBlock& b) { return !b.factored && b.has_V && !b.v_partial; }
bool cg_lowrank_operator(const lrn_ctx* c, const LmiBlock& b);   // matrix-free operator of this block in factor form?
bool cg_lowrank_ts(const lrn_ctx* c, const LmiBlock& b, int erank);   // ts of H_alpha for this block from the factors?
// option "cg_factored": the CG path accepts factored blocks (one GPU only)
inline bool cg_factored_on(const lrn_ctx* c) { return c->opt.cg_factored != 0 && c->world <= 1; }
// option "cg_diag": ... and factored blocks with diagonal parts among them
inline bool cg_diag_on(const lrn_ctx* c) { return c->opt.cg_diag != 0 && cg_factored_on(c); }
bool fac_op_scaled_on(const lrn_ctx* c, const LmiBlock& b);      // hop.hip: operator of this pure factored block through Y = W Vd?
bool fac_quadform_on(const lrn_ctx* c, const LmiBlock& b);       // hop.hip: AA vec(Z) of this factored block by the fused kernel?
// facops.hip: out[nat(h)] -= sum_c w_c v_c' Z v_c over the factor columns c of every constraint, on the columns of the view
// (fac_cols.h), Q = Z V never stored
struct FacCols;
int fac_quadform(lrn_ctx* c, const LmiBlock& b, const FacCols& v, const double* Z, const int* sigma, double* out);

// HIP-event timer of one phase on the context's stream (nothing unless enabled: c->profile for the outer phases, option
// "profile_ops" for a single data operator): elapsed_ms() is the time since the construction, stop() adds it to timing[key]
// and counts the phase; the events go with the scope, on an error return too
struct PhaseTimer {
  lrn_ctx* c;
  hipEvent_t a0 = nullptr, a1 = nullptr;
  PhaseTimer(lrn_ctx* ctx, bool enabled) : c(ctx) {
    if (!enabled) return;
    if (hipEventCreate(&a0) != hipSuccess) a0 = nullptr;
    if (hipEventCreate(&a1) != hipSuccess) a1 = nullptr;
    if (on()) (void)hipEventRecord(a0, c->stream);
  }
  PhaseTimer(const PhaseTimer&) = delete;
  bool on() const { return a0 && a1; }
  float elapsed_ms() {
    float ms = 0;
    if (!on()) return ms;
    (void)hipEventRecord(a1, c->stream);
    (void)hipEventSynchronize(a1);
    (void)hipEventElapsedTime(&ms, a0, a1);
    return ms;
  }
  void stop(const char* key) {
    if (!on()) return;
    c->timing[key] += elapsed_ms();
    c->counts[key] += 1;
  }
  ~PhaseTimer() {
    if (a0) (void)hipEventDestroy(a0);
    if (a1) (void)hipEventDestroy(a1);
  }
};
}  // namespace lrn

#define LRN_HIP(c, expr)                                                                   \
  do {                                                                                     \
    hipError_t e__ = (expr);                                                               \
    if (e__ != hipSuccess)                                                                 \
      return lrn::set_error((c), LRN_ERR_HIP, "%s failed: %s (%s:%d)", #expr,              \
                            hipGetErrorString(e__), __FILE__, __LINE__);                   \
  } while (0)
#define LRN_TRY(expr)             \
  do {                            \
    int rc__ = (expr);            \
    if (rc__ != LRN_OK) return rc__; \
  } while (0)
// a check of model_layout.h (LayoutError: code and message text) that failed becomes the context's error
#define LRN_LAYOUT(c, expr)                                                                 \
  do {                                                                                      \
    if (auto e__ = (expr)) return lrn::set_error((c), e__.code, "%s", e__.msg.c_str());     \
  } while (0)
