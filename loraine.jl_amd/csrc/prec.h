// prec.hip: the preconditioners of the CG path -- 0 none, 1 H_alpha (low rank, SMW apply), 2 H_beta (diagonal)
#pragma once
#include "ctx.h"
namespace lrn {
// info (may be null): non-zero when a factorisation of the setup failed (L_D, Z, S + I) -- LRN_OK all the same
int prec_setup(lrn_ctx* c, int kind, int erank, int aamat, int* info);
int prec_apply_dev(lrn_ctx* c, const double* x, double* Mx, double* tmpv);   // Mx = M^-1 x, device vectors; tmpv: nvar scratch
void prec_free(lrn_ctx* c);
int prec_kind(const lrn_ctx* c);                 // of the last setup, 0 without one
const double* prec_diag(const lrn_ctx* c);       // kind 2: the diagonal (device, nvar); null otherwise
// H_alpha as one dense matrix (option prec_dense), built now if it is not there and pays for `expected` applications
int prec_dense_if_worthwhile(lrn_ctx* c, long expected);
}  // namespace lrn
