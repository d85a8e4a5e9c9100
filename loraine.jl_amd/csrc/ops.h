// Device-side operations shared between translation units: the data operators (dataops.hip), the NT scaling (prepw.hip),
// the n x n products (products.hip) and helpers (matops.hip), the Lyapunov solve (lyap.hip), the Lanczos searches (lz.hip)
// and the parts of the Schur assembly.
#pragma once
#include "ctx.h"
namespace lrn {
bool use_sparse_matvec(const lrn_ctx* c, const LmiBlock& b);                // the pattern-restricted form of MyA serves this block
int ensure_m(lrn_ctx* c, int m);                                            // c->m0..m2 >= msz^2
int wmw(lrn_ctx* c, LmiBlock& b, double* M, double* P, double* Z);          // Z = W M W (M symmetric)
int aa_times(lrn_ctx* c, LmiBlock& b, const double* Z, double* y, bool factor_form = false, bool fused = false);          // y += AA vec(Z)
// y += AA vec(W M W) through the entries of W M W the (all sparse) constraints read: N (work) = M W, then dots on the pattern
bool wmw_pattern_ok(const lrn_ctx* c, const LmiBlock& b);
int aa_times_wmw_pattern(lrn_ctx* c, LmiBlock& b, const double* M, double* N, double* y);
int aa_times2(lrn_ctx* c, LmiBlock& b, const double* Z1, double* y1, const double* Z2, double* y2);   // both, one pass over dense data
int aat_to_mat(lrn_ctx* c, LmiBlock& b, const double* x, double* M, bool factor_form = false);        // M = mat(AA' x)
// route of the passes over the dense constraint data of b, decided once b.Adense is filled (model.hip, synth.hip): the symmetry check
// on the device and the chunk table of the column tails; sym_known: the data are symmetric by construction, no check
int dense_route_setup(lrn_ctx* c, LmiBlock& b, bool sym_known);
int matvec_dev(lrn_ctx* c, const double* x, double* y);                     // y = AA vec(W mat(AA' x) W) (+ the C_lin term): MyA
int matvec_partial_dev(lrn_ctx* c, const double* x, double* y, int rank, int world);   // the rows of Z of one rank; the caller all-reduces
int lin_matvec(lrn_ctx* c, const double* x, double* y);                     // y += C_lin diag(xs) C_lin' x
void lin_diag(lrn_ctx* c, double* d);                                       // d_i += sum_l C_lin[i,l]^2 xs_l
// ---- prepw.hip
int prepare_w_block(lrn_ctx* c, LmiBlock& b, int* info);                    // NT scaling from b.X, b.S (SVD route)
// eigen-free NT scaling from b.X, b.S: W, Si, the Cholesky factors and K^(+-1/2); *converged = false: nothing usable, take
// the SVD route
int prepare_w_ns(lrn_ctx* c, LmiBlock& b, int* info, bool* converged);
// Cholesky factors of b.X, b.S into b.LXf, b.LSf (two streams); info = 0, 1 (X not PD), 2 (S not PD) as prepare_W.jl:33-34;
// minpiv[2] (may be null): smallest pivots L_ii^2 (upper bounds of the smallest eigenvalues).  Sets b.chol_valid.
int nt_factor(lrn_ctx* c, LmiBlock& b, int* info, double* minpiv);
// ---- products.hip: n x n products, column-major
// Border between the two routes of these products: from this side on the 128-tile direct-to-LDS kernel fills the chip (a
// symmetric product as lower tiles + mirror, triangular-K hints taken); below it the product runs on 64-tiles, split into
// slabs where that pays, and its consumers add the slabs while they read (at msz 800 the 28 lower tiles of 128 take 121 us,
// the full product on 64-tiles 35 us)
constexpr int BIG_TILE_MIN_N = 1500;
// C = op(A) op(B), op = transpose where tA / tB
int gemm_nn(hipStream_t st, int n, const double* A, bool tA, const double* B, bool tB, double* C, int flags = 0);
// C = alpha A Bm': the arrangement the direct-to-LDS GEMM kernel takes
int gemm_nt(hipStream_t st, int n, const double* A, const double* Bm, double* C, int flags = 0, double alpha = 1.0,
            double* Ct = nullptr);     // Ct: the transposed result as well
// the same, a mid-size product left as its split-K slabs for a consumer that adds them while it reads (lrn_common.h, SlabSrc;
// src->n == 1: the product is in C)
int gemm_nt_slabs(hipStream_t st, int n, const double* A, const double* Bm, double* C, double alpha, SlabSrc* src);
// C and its transposed twin Ct from one pass over the slabs of a product (or over C itself when the product was not split)
void slabs_to_c_and_ct(hipStream_t st, const SlabSrc& src, int n, double* C, double* Ct);
// P = A Bm' symmetrised (not stored) -> T = a (3 I - a^2 P) / 2, partial sums of ||I - P||_F^2 in part[0 .. *npart)
int gemm_nt_sym_ns(hipStream_t st, int n, const double* A, const double* Bm, double* scratchC, double a, double* T, double* part,
                   int* npart);
// the same for a product that is symmetric in exact arithmetic; C comes back exactly symmetric
int gemm_nt_sym(hipStream_t st, int n, const double* A, const double* Bm, double* C, double alpha = 1.0, int tri = 0);
// The same products for the resident path of a sharded run (one process per GPU): when the communicator has more than one
// rank, `st` is the context's stream and n >= option shard_products_min, this rank computes its block of columns and the
// blocks are all-gathered in place (csrc/comm.hip) -- every rank ends with the same bits; otherwise the plain product.
bool products_sharded(const lrn_ctx* c, hipStream_t st, int n);
// tri: GEMM_KFROM_M / GEMM_KFROM_N / GEMM_KTO_M / GEMM_KTO_N when op(A) / op(B) is triangular with stored zeros
int pgemm_nt(lrn_ctx* c, hipStream_t st, int n, const double* A, const double* Bm, double* C, int tri = 0,
             double alpha = 1.0, double* Ct = nullptr);
int pgemm_nt_sym(lrn_ctx* c, hipStream_t st, int n, const double* A, const double* Bm, double* C, double alpha = 1.0,
                 int tri = 0);
// pgemm_nt for a consumer that can add split-K slabs while it reads (src->n > 1: the product is in the slabs, C untouched)
int prod_slabs(lrn_ctx* c, hipStream_t st, int n, const double* A, const double* Bm, double* C, double alpha, int tri,
               SlabSrc* src);
// k largest eigenpairs (ascending), smallest eigenvalue and trace of a dense symmetric matrix
int lanczos_extremes(lrn_ctx* c, const double* M, int n, int k, double* lam_top, double* U_top, double* lam_min,
                     double* trace, int* steps_out);
// ---- lz.hip: the plain Lanczos recurrence
// both ends of the spectrum from nsteps plain Lanczos steps: lo >= lambda_min, an eigenvalue within res_hi of hi
int lanczos_ends(lrn_ctx* c, const double* M, int n, int nsteps, double* lo, double* hi, double* res_hi);
// smallest Ritz value (an UPPER bound of lambda_min) and the steps it took; scale: the norm estimate max |a_j| + |b_j|
int eigmin_dev(lrn_ctx* c, const double* M, int n, double* lam, int* steps_out, bool* converged = nullptr,
               double* scale_out = nullptr);
// lambda_min certified by Cholesky tests; _pair: of two matrices of the same size, their Lanczos runs side by side
int eigmin_certified(lrn_ctx* c, const double* M, int n, double* lam);
int eigmin_certified_pair(lrn_ctx* c, const double* M1, const double* M2, int n, double* lam1, double* lam2);
// ---- Schur assembly (schur.hip drives; its launch decisions: schur_plan.h)
// address of the entry (hi, hj) of H in its authoritative lower triangle, either order of the two indices
__device__ __forceinline__ long h_lower(int hi, int hj, int ldh) {
  int rr = hi > hj ? hi : hj, cc = hi > hj ? hj : hi;
  return (long)rr + (long)cc * ldh;
}
// schur_dense.hip: the dense owners of a block (positions < nd) -- Cholesky path, or W / via-L path with the gather against
// sparse partners; whether the next assembly of the block would take the Cholesky path, and its batch hint
int assemble_dense(lrn_ctx* c, LmiBlock& b);
bool chol_path_applicable(lrn_ctx* c, LmiBlock& b, long* pcap_out);
// localops.hip: the sparse owners [loc_lo, loc_hi) of a block against all their partners, from A[S, S] on the supports
// (option "pair_local"); the caller has checked that the range is not empty and that one GPU runs
int assemble_local(lrn_ctx* c, LmiBlock& b);
int local_upload(lrn_ctx* c, LmiBlock& b);      // the device copies of that route's lists, once per upload
// longops.hip: the long sparse owners [nd, lg_end) of a block against all their partners, from Z_i = (A_i W) on their rows
// (option "pair_long").  long_fits: the scratch cap admits every owner of the range one at a time; the caller has checked it,
// that the range is not empty and that one GPU runs
bool long_fits(const lrn_ctx* c, const LmiBlock& b, int lg_end);
int assemble_long(lrn_ctx* c, LmiBlock& b, int lg_end);
// schur_factored.hip: rank-one data (mode -1), rank-k data (mode 1), cross terms of a hybrid factored block
int assemble_rank1(lrn_ctx* c, LmiBlock& b);
int assemble_lowrank(lrn_ctx* c, LmiBlock& b);
// C = op(A) V into msz x R columns (op = transpose where transA): the product of every route that multiplies dense factor columns
int cols_product(lrn_ctx* c, const double* A, bool transA, const double* V, long R, int m, double* C);
// Y = W V of the current scaling, cached per scaling: Ys = W Vd (msz x nvar khat), or Yc = W Vc (msz x Rc) where compact
int fac_scaled_y(lrn_ctx* c, LmiBlock& b, bool compact);
int factored_y(lrn_ctx* c, LmiBlock& b, const double** Y);      // Y = W Vd (msz x nvar khat) after assemble_lowrank: its U, or one more product; Yc = W Vc (msz x Rc) under ragged_cross_on
int assemble_cross(lrn_ctx* c, LmiBlock& b, const double* Y);   // cross terms of a hybrid block from that Y, in its layout
// facops.hip: ts of H_alpha from P = L' V (msz x R) and T = V' Um (R x erank) on the columns of the view (fac_cols.h; prec.hip::prec_setup
// decides, option "ragged_ts"): every element of the block's nvar x erank msz part of ts written once
struct FacCols;
int fac_ts(lrn_ctx* c, const LmiBlock& b, const FacCols& v, const double* P, const double* T, const double* d, int erank,
           double* ts);
// raggedops.hip: H_FF of a block of mixed ranks by rank class (option "lowrank_ragged"; assemble_lowrank decides)
int assemble_ragged(lrn_ctx* c, LmiBlock& b);
// ... and mat(AA' x) in factor form on the same compacted columns (option "ragged_ops"; aat_to_mat_factored of dataops.hip
// decides).  ragged_setup: the plan of the block and Vc, once per upload, whichever route on the compacted columns comes first
int ragged_setup(lrn_ctx* c, LmiBlock& b);
// M = -F diag(wc o x) F', F = Vc (null) or Yc; *ks = 1: lower tiles only, the caller mirrors them
int aat_to_mat_ragged(lrn_ctx* c, LmiBlock& b, const double* x, double* M, const double* F, int* ks);
// diagops.hip: diagonal parts of a factored block (lrn_upload_diag), A_k = diag(a_k) + V_k D_k V_k'
int assemble_diag(lrn_ctx* c, LmiBlock& b, const double* Y);    // H_DD, the cross terms with the factors (Y) and with the stored rows
int aa_times_diag(lrn_ctx* c, LmiBlock& b, const double* Z, double* y);      // y[nat(s)] -= sum_i a_si Z_ii
int aat_to_mat_diag(lrn_ctx* c, LmiBlock& b, const double* x, double* M);    // M_ii -= sum_s x[nat(s)] a_si
// ts of H_alpha (option "cg_diag"): ts[nat(s), a m + r] -= sum_i a_si Um[i, a] L[i, r] / sqrt(d[nat(s)]), added to the factor part
int ts_diag(lrn_ctx* c, LmiBlock& b, const double* Lf, const double* Um, int erank, const double* d, double* ts);
// ---- matops.hip: passes over n x n matrices (column-major) on stream st, and the two-stage dot product
void tril(hipStream_t st, double* A, int n);                               // strict upper triangle <- 0
void eye_mat(hipStream_t st, double* V, int n);                            // V = I
void mirror_lower(hipStream_t st, double* A, int n);                       // upper triangle <- lower triangle, in place
void transpose_mat(hipStream_t st, const double* A, int n, double* B);     // B = A'
void scale_cols(hipStream_t st, const double* A, const double* d, int n, int mode, double* B);   // B[:,j] = A[:,j] d_j^p, p = -1/2, 1/2, -1 for mode 0, 1, 2
void coldot_rsqrt(hipStream_t st, const double* A, const double* B, int n, double* out);         // out_j = 1 / sqrt(A[:,j] . B[:,j])
void add_diag_mat(hipStream_t st, double* M, int n, double eps);           // M += eps I
// out = a A + b B + c C over n elements (null pointers skipped)
void lin3(hipStream_t st, double* out, long n, double a, const double* A, double b, const double* B, double c = 0.0,
          const double* C = nullptr);
void sym_half(hipStream_t st, const double* M, double* out, int n);        // out = (M + M') / 2, out != M
void scale_sym(hipStream_t st, const double* M, const double* dd, double* out, int n);           // out = sym(dd_i M_ij dd_j)
unsigned sym_grid(int n);                                                  // workgroups of a pass by 32 x 32 tile pairs (symadd)
// out = scale (T + T') from T or its slabs by `grid` workgroups; dotp: part[0 .. grid) = partial sums of <dotp, out>
void symadd(hipStream_t st, unsigned grid, const SlabSrc& T, int n, double scale, double* out, const double* dotp, double* part);
// out = alpha A Bm' for a product that is symmetric in exact arithmetic, exactly symmetric on either side of BIG_TILE_MIN_N:
// lower tiles + mirror from there on, below it the average of the two triangles of the full product (work: its slabs)
int sym_product(lrn_ctx* c, hipStream_t st, int n, const double* A, const double* Bm, double* work, double* out, double alpha,
                int tri);
// *out = sum A .* B (B null: A .* A) over n elements, in two launches through dot_parts_count(n) partial sums
int dot_parts_count(long n);
void dot_via(hipStream_t st, const double* A, const double* B, long n, double* part, double* out);
int dot_dev(lrn_ctx* c, const double* A, const double* B, long n, double* out_dev);      // ... on c->stream through c->redbuf
// ---- lyap.hip: R with Yh R + R Yh = Cm for the block's Yh (Zh beside it, option lyap_form) by CG; Cm is destroyed, work:
// msz^2 doubles; *ok = false: not converged within lyap_maxit steps
int lyap_solve(lrn_ctx* c, LmiBlock& b, double* Cm, double* R, double* work, bool* ok, int* steps);
// ---- model.hip: H, the solve vectors and the scaling matrices of every block, once the blocks are laid out
int alloc_common(lrn_ctx* c);
// ---- ipstep.hip
int ensure_resident(lrn_ctx* c, LmiBlock& b);                              // the arrays of the resident IP step of a block exist
}  // namespace lrn
