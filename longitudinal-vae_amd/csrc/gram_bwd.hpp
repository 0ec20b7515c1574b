// gram_bwd.hpp -- host descriptors of the batched Grams (gram.hip): up to 4 Grams in one forward launch
// (the inducing-point bounds' four: bound_grams_fwd, gp_bound.hip), and up to 4 Grams contracted against their G
// in two launches (used by lvae_gram_bwd_f64 and the bounds' bound_grams_bwd, which also sizes its partials with
// gram_bwd_part_bytes).
#pragma once
#include "common.hpp"

namespace lvae {

struct GramBwdJob {
  int spec;  // index into the specs[2] argument
  lvae_xview x1, x2;
  int nb, n1, n2, n_params;
  const double* params;
  const double* G;
  int64_t gsb, gsl, ldg;
  double* dparams;
  double* ddiag;
  int chunk0, nchunks;  // filled by gram_bwd_multi_f64
};

size_t gram_bwd_part_bytes(const GramBwdJob* jobs, int njobs, int L);

// forward: up to 4 fp64 Grams in one launch (gram_multi_f64; the bounds' four), each as
// lvae_gram_f64's arguments (gx, gy, blk0 filled by gram_multi_f64)
struct GramFwdJob {
  int spec, nb, n1, n2, gx, gy, blk0;
  lvae_xview x1, x2;
  const double* params;
  const double* diag;
  double* out;
  int64_t osb, osl, ldo;
};
int gram_multi_f64(const lvae_kernel_spec* const* specs, const GramFwdJob* jobs, int njobs, int L, hipStream_t st);
int gram_bwd_multi_f64(const lvae_kernel_spec* const* specs, const GramBwdJob* jobs, int njobs, int L, double* part,
                       hipStream_t st);

// input adjoint: up to 3 Grams of one spec with one x2 shape, d/dx2 of each against its G (element (b, l, i, j) at
// G[b gsb + l gsl + i gsi + j gsj]) summed into one dx2 [nb, L, n2, Q] in two launches (lvae_gram_bwd_x2_f64 and the
// bounds' bound_grams_bwd_z; nrc, nct, blk0, part0 filled by gram_bwd_x2_multi_f64)
struct GramX2Job {
  lvae_xview x1, x2;
  int nb, n1, n2;
  const double* G;
  int64_t gsb, gsl, gsi, gsj;
  int nrc, nct, blk0;
  int64_t part0;
};
size_t gram_bwd_x2_part_bytes(const GramX2Job* jobs, int njobs, int L, int Q);
// -1: spec null, outside every template bucket, or reading a column >= min(Q, 32); -4: a bad count or jobs whose
// nb / n2 differ; n2 == 0 writes nothing; a job with n1 == 0 adds nothing (dx2 is still overwritten)
int gram_bwd_x2_multi_f64(const lvae_kernel_spec* spec, const GramX2Job* jobs, int njobs, int L, int Q,
                          const double* params, double* dx2, double* part, hipStream_t st);

}  // namespace lvae
