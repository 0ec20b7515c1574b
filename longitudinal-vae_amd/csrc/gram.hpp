// gram.hpp -- the host functions the three Gram sources export to other sources.
//   gram.hip         the batched Grams: up to 4 Grams in one forward launch (the inducing-point bounds' four:
//                    bound_grams_fwd, gp_bound.hip), up to 4 Grams contracted against their G in two launches
//                    (lvae_gram_bwd_f64 and the bounds' bound_grams_bwd, which also sizes its partials with
//                    gram_bwd_part_bytes), and the input adjoint
//   kl_gram.hip      the exact KL's fp32 covariance fill and fused adjoint (kl_closed.hip)
//   gram_matvec.hip  the exact KL's fp64 residual (kl_closed.hip) and the fused fp64 Gram x vector products (the
//                    latent predictors, predict.hip; the conditioned KL, kl_cond.hip)
#pragma once
#include "common.hpp"

namespace lvae {

// ---- gram.hip ----
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

// ---- kl_gram.hip ----
// K_l = Gram_l(x, x) + noise_l I as fp32 lower 64-tiles of the padded [L, np, np] K (identity on the padding);
// *covflag (device) receives the covariates' class, which picks the table / fp32 / fp64 kernel among those
// launched here and in kl_gram_bwd.  -1: a spec outside every bucket, or reading a column >= min(16, ldx)
int kl_gram_fill(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int np_, int L,
                 const double* params, const double* noise, float* K, int* covflag, hipStream_t st);
size_t kl_gram_bwd_partials_bytes(int np_, int L);
// dparams, dnoise = gkl x the contraction of G = 1/2 (K^-1 - S - a a^T) with dK / dtheta; S in nsplit K-split
// partials (S, then Sx: syrk_x3_splits); part: kl_gram_bwd_partials_bytes.  hbws / hbon: the binned
// hyper-gradient's workspace and device flag (kl_hyper.hip; null: the tile kernels alone)
int kl_gram_bwd(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int np_, int L,
                const double* params, const float* Kinv, const float* S, const float* Sx, int nsplit,
                const double* alpha, const double* kdiag, const float* v, const double* gkl, double* part,
                double* dparams, double* dnoise, const int* covflag, void* hbws, const int* hbon, hipStream_t st);

// ---- gram_matvec.hip ----
size_t kl_resid_partials_bytes(int np_, int L);
// res = mu - K alpha0 in fp64, K never materialised; part: kl_resid_partials_bytes; rbws: the binned residual's
// planned workspace (kl_resid_bins.hip), or null for the tiled kernels alone
int kl_gram_resid(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int np_, int L,
                  const double* params, const double* noise, const double* alpha0, const double* muc, double* part,
                  double* res, void* rbws, hipStream_t st);
// 1 + the largest covariate column the fused product reads for this spec; 0: a spec it does not take
int gram_matvec_spec_ld(const lvae_kernel_spec* spec);
size_t gram_matvec_ws_bytes(int n1, int n2, int L);
// The fused product; v and out each in the public entry point's [n, ld] layout (v_t / o_t == 0: element (j, l) at
// [j ld + l]) or transposed, [L, ld] (element (j, l) at [l ld + j]: the exact predictor's work vectors).
// Argument codes are lvae_gram_matvec_f64's.
int gram_matvec_f64(const lvae_kernel_spec* spec, const double* x1, int64_t ld1, int n1, const double* x2, int64_t ld2,
                    int n2, int L, const double* params, const double* diag, const double* v, int64_t ld_v, int v_t,
                    double* out, int64_t ld_out, int o_t, void* workspace, hipStream_t st);
size_t gram_matvec_comp_ws_bytes(int n1, int n2, int L, int n_comp);
// The component-resolved fused product; v and out in gram_matvec_f64's two layouts, the R = spec->n_comp blocks of
// out ostride_r elements apart, x2 of latent dim l at x2 + l x2_stride_l.  The slabs are gram_matvec_f64's.
// Argument codes are lvae_gram_matvec_comp_f64's.
int gram_matvec_comp_f64(const lvae_kernel_spec* spec, const double* x1, int64_t ld1, int n1, const double* x2,
                         int64_t ld2, int64_t x2_stride_l, int n2, int L, const double* params, const double* v,
                         int64_t ld_v, int v_t, double* out, int64_t ld_out, int o_t, int64_t ostride_r,
                         void* workspace, hipStream_t st);

}  // namespace lvae
