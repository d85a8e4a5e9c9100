// The plain Lanczos recurrence (no re-orthogonalisation) as a step engine (lz.hip): one description of a run and one
// function that queues its steps, in whichever of the three forms.  The drivers on top of it -- eigmin_dev,
// eigmin_certified(_pair), lanczos_ends -- are declared in ops.h; lanczos.hip drives its own loop (H_alpha setup, k <= 1).
#pragma once
#include <vector>

#include "ctx.h"
namespace lrn {

enum LzForm {
  LZ_TWO_KERNEL,      // mat-vec in column chunks on all CUs + one single-workgroup kernel: two launches per step, any n
  LZ_FUSED,           // one launch per step (32 <= n <= 16384), and a finishing launch per call
  LZ_RESIDENT         // one launch per call: M in registers, relaxed-atomic exchange (n <= 1024); may give up, see lz_fetch
};

// One run: q_j lives in buffer j % qmod of Q (qmod = 3: a ring; larger: every q_j is kept), (alpha_j, beta_j) in ab[2 j ..].
struct LzWork {
  lrn_ctx* c = nullptr;           // resident launches: their wait limit, launch counter and test hook live on the context
  const double* M = nullptr;
  int n = 0, nwg = 0;             // nwg = ceil(n / 16)
  hipStream_t st = nullptr;
  LzForm form = LZ_TWO_KERNEL;
  double* Q = nullptr;
  int qmod = 3;
  double* Y = nullptr;            // fused: two n-vectors (y_j in buffer j & 1); resident: three (j % 3); two-kernel: w (n)
  double* PA = nullptr;           // fused / resident: as many nwg-vectors, the workgroups' shares of q_j . y_j; two-kernel:
                                  // the partial mat-vecs (n x number of chunks)
  double* ab = nullptr;
  unsigned* flag = nullptr;       // resident: two words, flag[1] = abort word
  std::vector<double> hab;        // host copy of ab (lz_fetch)
};

static constexpr int LZ_FUSED_LIMIT = 4096;      // lanczos.hip keeps every q_j: its bound for the plain recurrence
// the resident form serves this n on this context (option lz_resident; never again after a launch gave up)
bool lz_resident_ok(const lrn_ctx* c, int n);
// before the first step of a run (resident form: the exchange buffers hold the mark, the abort word is clear)
void lz_prepare(const LzWork& w);
// steps [j0, j1) of 1 or 2 runs (same n, qmod and form; two: never two-kernel) on w[0]->st: afterwards alpha_j, beta_j of
// all steps < j1 are in ab and q_{j1} in Q
int lz_queue_steps(const LzWork* const w[], int nruns, int j0, int j1);
// waits for w[0]->st and brings alpha, beta of the steps [0, m) of every run to its hab.  *gave_up: a resident launch ran
// out of time waiting for its peers (a shared or over-subscribed GPU) -- nothing of the runs is valid, the caller calls
// lz_record_give_up and repeats them in a launched form
int lz_fetch(lrn_ctx* c, LzWork* const w[], int nruns, int m, bool* gave_up);
void lz_record_give_up(lrn_ctx* c);      // launched steps on this context from now on; counter "lz_persist_abort"

}  // namespace lrn
