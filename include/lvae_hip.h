/*
 * lvae_hip.h -- C ABI of the MI355X-native Longitudinal-VAE GP-prior ELBO hot path.
 *
 * Every entry point is a plain C function over caller-owned device pointers: no allocation of
 * device memory inside, all work enqueued asynchronously on the caller's hipStream_t (passed as
 * void*), safe to call from several host threads.  Process-wide state is limited to (1) the
 * opt-in phase timer (lvae_prof_*) and (2) the blocked inverses' side stream (lvae_spd_inv_chol_f32,
 * lvae_kl_closed_*): ONE high-priority stream + seven events (fork, prep, c, and
 * two pairs alternating by pass parity) per device, shared by every caller stream, created on first
 * use, kept for the process lifetime, and guarded by a mutex held for each call's whole enqueue
 * sequence (calls from different caller streams serialise on it).  The calls are graph-capturable (the side stream joins
 * the capture through the fork event and is joined back before the call returns).  Return value: 0 = ok, <0 = -(index of the bad argument),
 * LVAE_ERR_LAUNCH on a HIP launch error.  Numerical failure (a non-positive-definite pivot) is
 * NOT a return code (the call is asynchronous): it is written to the device `info` array,
 * LAPACK-style (first failing column + 1, 0 = ok), and the Python layer raises
 * torch.linalg.LinAlgError from it like torch.linalg.cholesky does.
 *
 * Reference interfaces replaced (SidRama/Longitudinal-VAE, /root/reference):
 *   covar_module(x1, x2).evaluate()       -> lvae_gram_*            (GP_model.py:31-144,
 *                                             kernel_gen.py:9-310, call sites elbo_functions.py:22,56,171-174)
 *   autograd of that Gram wrt (scale, lengthscale) -> lvae_gram_bwd_*
 *   autograd of that Gram wrt its second input (learnable inducing points, LVAE.py:204-208, 269;
 *                                             training.py:349) -> lvae_gram_bwd_x2_f64, lvae_*_bwd_z_f64
 *   torch.cholesky(K1) on N x N           -> lvae_potrf_f64 / _f32 (elbo_functions.py:26)
 *   torch.cholesky_solve(B, LK1)          -> lvae_potrs_f64 / _f32, lvae_trsm_* (elbo_functions.py:27-28)
 *   torch.cholesky / cholesky_solve(I) / log-det on N x N -> lvae_spd_inv_chol_f32
 *                                             (elbo_functions.py:26-29)
 *   KL_closed forward + autograd backward -> lvae_kl_closed_fwd_f32 / _bwd_f32 (elbo_functions.py:8-34)
 *   batched small fp64 factor + inverse   -> lvae_spd_inv_small_f64 (elbo_functions.py:176-186,
 *                                             training.py:130-134)
 *   minibatch_KLD_upper_bound + autograd  -> lvae_hensman_fwd_f64 / _bwd_f64 (elbo_functions.py:144-216)
 *   natural-gradient (m, H) update        -> lvae_natgrad_update_f64 (training.py:129-135)
 */
#ifndef LVAE_HIP_H
#define LVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LVAE_MAX_COMP 16   /* additive components per kernel                  */
#define LVAE_MAX_FAC 4     /* product factors per component                   */
#define LVAE_ERR_LAUNCH (-1000)

/* factor kinds (GP_model.py:31-85).  Periodic and linear are extensions: parity with the reference is undefined
 * (it has no such kernel); agreement with the fp64 oracle is pinned for every entry point that takes a spec. */
enum lvae_factor_kind {
  LVAE_CAT = 0,   /* 1[x1_d == x2_d]                                  GP_model.py:52-53 */
  LVAE_BIN = 1,   /* 1[x1_d + x2_d == 2]                              GP_model.py:40-41 */
  LVAE_RBF = 2,   /* exp(-(x1_d-x2_d)^2 / (2 l^2)), param l            GP_model.py:80-85 */
  LVAE_PER = 3,   /* exp(-2 sin^2(pi|x1_d-x2_d|/p) / l^2), params l, p  (extension)       */
  LVAE_LIN = 4    /* x1_d * x2_d                                      (extension)       */
};

/* An additive kernel: sum_r scale_r * prod_f factor_{r,f}.  Parameters are per latent dim
 * (row-major [L, n_params], constrained values); component r's scale is params[scale_idx[r]],
 * a factor's first parameter is params[param_idx[r][f]] (-1 when it has none). */
typedef struct lvae_kernel_spec {
  int32_t n_comp;
  int32_t n_params;
  int32_t n_fac[LVAE_MAX_COMP];
  int32_t scale_idx[LVAE_MAX_COMP];
  int32_t kind[LVAE_MAX_COMP][LVAE_MAX_FAC];
  int32_t dim[LVAE_MAX_COMP][LVAE_MAX_FAC];
  int32_t param_idx[LVAE_MAX_COMP][LVAE_MAX_FAC];
} lvae_kernel_spec;

/* Strided operand of a batched Gram: element (b, l, i, q) at
 *   ptr[b*stride_b + l*stride_l + i*ld + q]     (stride 0 = broadcast)                       */
typedef struct lvae_xview {
  const double* ptr;
  int64_t stride_b;
  int64_t stride_l;
  int64_t ld;
} lvae_xview;

/* ---------------------------------------------------------------------------------------- */
/* Gram                                                                                      */
/* ---------------------------------------------------------------------------------------- */

/* out[b, l, i, j] = sum_r s_r prod_f phi(x1[b,l,i], x2[b,l,j]) + (i == j ? diag[l] : 0)
 * for b < nb, l < L, i < n1, j < n2.  out element (b,l,i,j) at
 * out[b*ostride_b + l*ostride_l + i*ldo + j] (nothing else of out is written).  diag may be NULL
 * (it is added for i == j < min(n1, n2)).  params: [L, n_params] fp64.  -1: a spec outside
 * LVAE_MAX_COMP / LVAE_MAX_FAC / n_params <= 64, or a factor dim >= 32; -4: nb < 1, L < 1, n1 < 0 or
 * n2 < 0; n1 == 0 or n2 == 0: returns 0 and writes nothing.  The adjoint rejects the same.
 * Replaces covar_module(x1, x2).evaluate() (+ noise * I) in elbo_functions.py:22-23,171-174. */
int lvae_gram_f64(const lvae_kernel_spec* spec, lvae_xview x1, lvae_xview x2, int nb, int L, int n1,
                  int n2, const double* params, const double* diag, double* out, int64_t ostride_b,
                  int64_t ostride_l, int64_t ldo, void* stream);
int lvae_gram_f32(const lvae_kernel_spec* spec, lvae_xview x1, lvae_xview x2, int nb, int L, int n1,
                  int n2, const double* params, const double* diag, float* out, int64_t ostride_b,
                  int64_t ostride_l, int64_t ldo, void* stream);

/* Adjoint of lvae_gram_*: dparams[l, p] (+)= sum_{b,i,j} G[b,l,i,j] * d out[b,l,i,j] / d params[l,p]
 * (diag term excluded; d/d diag is returned separately in ddiag[l] = sum_{b,i} G[b,l,i,i] when
 * ddiag != NULL).  G strided like out.  Results are ADDED to dparams / ddiag (fp64), in a fixed
 * order (deterministic).  workspace: lvae_gram_bwd_workspace_size(nb, L, n1, n2) bytes.        */
size_t lvae_gram_bwd_workspace_size(int nb, int L, int n1, int n2);
int lvae_gram_bwd_f64(const lvae_kernel_spec* spec, lvae_xview x1, lvae_xview x2, int nb, int L, int n1,
                      int n2, const double* params, const double* G, int64_t gstride_b,
                      int64_t gstride_l, int64_t ldg, double* dparams, double* ddiag, void* workspace,
                      void* stream);

/* Input adjoint of lvae_gram_f64 with respect to its second operand (what autograd gives the reference for a
 * covar_module(x1, x2).evaluate() whose x2 requires grad: the inducing inputs, LVAE.py:204-208, 269 and
 * training.py:349, which the reference leaves commented out):
 *   dx2[b, l, j, q] = sum_{i < n1} G[b,l,i,j] * d k_l(x1[b,l,i], x2[b,l,j]) / d x2[b,l,j,q]    j < n2, q < Q
 * G element (b,l,i,j) at G[b*gstride_b + l*gstride_l + i*gstride_i + j*gstride_j]: a caller passes G transposed
 * through its strides, and gets the FIRST operand's adjoint by swapping x1 and x2 and passing G^T (every factor is
 * symmetric in its two arguments).  Per factor on column d, with a = x1[.., d], b = x2[.., d] and v the value of
 * the factor's component (scale and the other factors included): LVAE_CAT, LVAE_BIN: 0 (autograd through the
 * reference's == comparisons); LVAE_RBF: v (a - b) / l^2; LVAE_PER: v (2 pi / (p l^2)) sin(2 pi (a - b) / p) (0 at
 * a == b, as autograd through abs); LVAE_LIN: a times the component's other factors.  A column no differentiable
 * factor reads gets exact zeros.  An element with G == 0 is skipped, as in lvae_gram_bwd_f64: it adds nothing even
 * where the kernel value or its derivative is not finite (autograd would give 0 * inf = NaN there).
 * dx2 [nb, L, n2, Q] (contiguous, fp64) is OVERWRITTEN; x1 / x2 may broadcast
 * (stride 0).  fp64 throughout, both template buckets, factor dims below 32, arbitrary n1 / n2.  No atomics and a
 * fixed summation order (the same inputs give the same bits): each block of 64 rows of G writes its partial
 * [n2, min(Q, 32)] to the workspace, a second launch adds the blocks in row order.  workspace:
 * lvae_gram_bwd_x2_workspace_size(nb, L, n1, n2, Q) bytes (a multiple of 256; 0 for arguments the call rejects).
 * Returns 0, LVAE_ERR_LAUNCH, or before any launch, checked in this order, with lvae_gram_bwd_f64's codes for the
 * faults the two share: -1 (spec NULL, outside every template bucket, or a factor dim >= 32) -4 (nb < 1, L < 1,
 * n1 < 0, n2 < 0, or Q < 1 + the largest column the spec reads) -8 (params NULL) -9 (G NULL) -13 (dx2 NULL)
 * -15 (workspace NULL).  n1 == 0 writes zeros to dx2 and returns 0; n2 == 0 writes nothing and returns 0.     */
size_t lvae_gram_bwd_x2_workspace_size(int nb, int L, int n1, int n2, int Q);
int lvae_gram_bwd_x2_f64(const lvae_kernel_spec* spec, lvae_xview x1, lvae_xview x2, int nb, int L, int n1, int n2,
                         int Q, const double* params, const double* G, int64_t gstride_b, int64_t gstride_l,
                         int64_t gstride_i, int64_t gstride_j, double* dx2, void* workspace, void* stream);

/* Fused cross-Gram x vector in fp64, the [L, n1, n2] Gram never written:
 *   out[i, l] = sum_{j < n2} k_l(x1_i, x2_j) v[j, l] + (diag ? diag[l] v[i, l] : 0)      i < n1, l < L
 * x1 [n1, ld1] and x2 [n2, ld2] are the covariates of every latent dim; params [L, n_params]; v element (j, l)
 * at v[j*ld_v + l], out element (i, l) at out[i*ld_out + l] (nothing else of out is written).  diag [L] is
 * allowed only when n1 == n2.  The kernel family is lvae_gram_f64's: every factor kind, both template buckets,
 * factor dims below 32.  n1, n2 are arbitrary (edge tiles are masked).
 * One workgroup per 64 rows of x1 sweeps 64-column tiles of x2; when there are few row tiles the columns are cut
 * into S slabs (S a function of (n1, n2, L) alone), the partials [L, S, n1] go to the workspace and are summed in
 * slab order: no atomics, the same bits on every run.  workspace: lvae_gram_matvec_workspace_size(n1, n2, L)
 * bytes (0 when S == 1; then it may be NULL), 256-B aligned.
 * Returns 0, LVAE_ERR_LAUNCH, or before any launch, checked in this order:
 *   -1 (spec NULL, outside every template bucket, or a factor dim outside 0 .. 31)
 *   -4 (n1 < 0) -7 (n2 < 0) -8 (L < 1); then n1 == 0 returns 0 and writes nothing;
 *   -2 (x1 NULL) -3 (ld1 < 1 + the largest column the spec reads) -5 (x2 NULL) -6 (ld2, as ld1) -9 (params NULL)
 *   -10 (diag given and n1 != n2) -11 (v NULL) -12 (ld_v < L) -13 (out NULL) -14 (ld_out < L)
 *   -15 (workspace NULL or misaligned when S > 1).  x2, ld2, v and ld_v are not checked when n2 == 0: the call then
 *   writes zeros to out [n1, L] and returns 0.                                                           */
size_t lvae_gram_matvec_workspace_size(int n1, int n2, int L);
int lvae_gram_matvec_f64(const lvae_kernel_spec* spec, const double* x1, int64_t ld1, int n1, const double* x2,
                         int64_t ld2, int n2, int L, const double* params, const double* diag, const double* v,
                         int64_t ld_v, double* out, int64_t ld_out, void* workspace, void* stream);

/* The same product resolved by additive component of the spec (R = spec->n_comp), fp64, no Gram written:
 *   out[r, i, l] = sum_{j < n2} s_{l,r} prod_f phi_{r,f}(x1_i, x2_j) v[j, l]           r < R, i < n1, l < L
 * so that sum_r out[r] is lvae_gram_matvec_f64's out (diag = NULL) up to rounding.  Arguments as there, except:
 * x2 may differ per latent dim, element (l, j, q) at x2[l*x2_stride_l + j*ld2 + q] (x2_stride_l = 0: one x2 for
 * every dim; M*Q for inducing inputs [L, M, Q]); out element (r, i, l) at out[r*ostride_r + i*ld_out + l] (nothing
 * else of out is written); there is no diag.  Kernel family, limits, tiling and the slabs S are
 * lvae_gram_matvec_f64's; the per-(component, row) sums are kept in LDS, each with one owning lane, tiles added in
 * column order and slabs in slab order: no atomics, the same bits on every run.  A component whose cross-Gram is
 * zero everywhere (an id component between disjoint subject sets) gives exact zeros.  workspace:
 * lvae_gram_matvec_comp_workspace_size(n1, n2, L, R) bytes (partials [L, S, R, n1]; 0 when S == 1, then it may be
 * NULL), 256-B aligned.
 * Returns 0, LVAE_ERR_LAUNCH, or before any launch, checked in this order (lvae_gram_matvec_f64's codes where the
 * two share a fault):
 *   -1 (spec NULL, outside every template bucket, or a factor dim outside 0 .. 31)
 *   -4 (n1 < 0) -7 (n2 < 0) -8 (L < 1); then n1 == 0 returns 0 and writes nothing;
 *   -2 (x1 NULL) -3 (ld1 < 1 + the largest column the spec reads) -5 (x2 NULL) -6 (ld2, as ld1) -9 (params NULL)
 *   -11 (v NULL) -12 (ld_v < L) -13 (out NULL) -14 (ld_out < L) -16 (x2_stride_l < 0)
 *   -17 (R > 1 and ostride_r < n1*ld_out) -15 (workspace NULL or misaligned when S > 1).  x2, ld2, x2_stride_l, v
 *   and ld_v are not checked when n2 == 0: the call then writes zeros to all R blocks [n1, L] and returns 0.   */
size_t lvae_gram_matvec_comp_workspace_size(int n1, int n2, int L, int n_comp);
int lvae_gram_matvec_comp_f64(const lvae_kernel_spec* spec, const double* x1, int64_t ld1, int n1, const double* x2,
                              int64_t ld2, int64_t x2_stride_l, int n2, int L, const double* params, const double* v,
                              int64_t ld_v, double* out, int64_t ld_out, int64_t ostride_r, void* workspace,
                              void* stream);

/* ---------------------------------------------------------------------------------------- */
/* Regime B: exact KL over the full N x N covariance (elbo_functions.py:8-34), batched over L */
/* latent dims.  Arithmetic: fp32 storage; every GEMM on the f16 matrix cores with the       */
/* 3-product hi / lo split (fp32-equivalent, ~2^-22 of max|operand| per product; power-of-two */
/* split scales per 256 x 256 block from each block's exact max, so any K scale / noise level */
/* that fp32 itself can represent is safe); K^-1 mu refined once in fp64.  Covariance padded  */
/* to Np = lvae_kl_closed_padded_n(n) (identity on the padding).                              */
/* ---------------------------------------------------------------------------------------- */
int lvae_kl_closed_padded_n(int n);
/* bytes of device workspace the fwd+bwd pair needs (kept between the two calls); 0 for n <= 0, n > 16384
 * (the blocked inverse handles 64 blocks of 256) or L <= 0.
 * Env LVAE_KL_EARLY=1 (opt-in early reduce) adds that route's buffers.  The variable is read here and again by
 * the factor (lvae_kl_closed_factor_f32 / _fwd_f32) on that workspace: it must hold the same value at both calls.
 * The factor's decision is kept per workspace pointer for the reduce and the backward on it, so what any other
 * caller sizes or factors in between does not matter; a workspace no factor has run on takes the default route. */
size_t lvae_kl_closed_workspace_size(int n, int L);

/* Return codes of lvae_kl_closed_*: 0, LVAE_ERR_LAUNCH, or -(1-based index of the offending argument in the entry
 * point's own list), checked in that order before anything is launched or written:
 *   spec NULL or its n_comp / n_fac / dim out of range; x NULL; ldx < 1 + the largest covariate the spec reads; n <= 0 or n > 16384; L <= 0; params NULL;
 *   noise NULL; mu NULL; logv NULL; ld_mu < L; kl NULL; info NULL (info is required); gkl / dmu / dlogv / dparams /
 *   dnoise NULL; workspace NULL or not 256-B aligned.
 *   _factor_f32: -1 -2 -3 -4 -5 -6 -7 (noise) -8 (info) -9 (workspace)
 *   _reduce_f32: -1 .. -7, -8 (mu) -9 (logv) -10 (ld_mu) -11 (kl) -12 (workspace)
 *   _fwd_f32:    -1 .. -7, -8 (mu) -9 (logv) -10 (ld_mu) -11 (kl) -12 (info) -13 (workspace)
 *   _bwd_f32:    -1 .. -6, -8 (logv) -9 (ld_mu) -10 (gkl) -11 (dmu) -12 (dlogv) -13 (dparams) -14 (dnoise)
 *                -15 (workspace); mu is not read and may be NULL.  Both halves' arguments are checked before
 *                either half runs.
 *   _bwd_latent_f32 / _bwd_hyper_f32: the codes of the same arguments in _bwd_f32's list.
 *   _refine_state: -1 (n) -2 (L) -3 (workspace) -4 (est) -5 (flag);  _hyper_state: -1 -2 -3 (NULL) -4 (on);
 *   _resid_state: -1 (n) -2 (L) -3 (workspace) -4 (covflag) -5 (binned).
 * A spec outside the supported kernel family is rejected by the Gram fill (-1) before any other work.
 * A matrix that is not positive definite is not an error of the call: info[l] > 0 (first bad column + 1).     */

/* kl[l] = 1/2 (tr(K^-1 V) + mu^T K^-1 mu - n + log|K| - sum log v),  K = Gram_l(x, x) + noise_l I.
 * x: [n, ldx] fp64 covariates; mu, logv: element (i, l) at mu[i*ld_mu + l] (fp64);
 * params [L, n_params] fp64; noise [L] fp64; kl [L] fp64; info [L] int32.
 * workspace: lvae_kl_closed_workspace_size(n, L) bytes, 256-B aligned.
 * need_bwd != 0 also writes the backward's S-GEMM operand (fp16 planes of K^-1 diag(sqrt v),
 * one power-of-two scale per dim) into the workspace; the backward requires a need_bwd forward. */
int lvae_kl_closed_fwd_f32(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int L,
                           const double* params, const double* noise, const double* mu, const double* logv,
                           int ld_mu, double* kl, int32_t* info, void* workspace, int need_bwd,
                           void* stream);
/* The same forward in two calls, for callers that overlap the factorisation with the work that
 * produces (mu, logv) (the encoder): _factor_f32 needs only the covariates and hyperparameters
 * (Gram + the blocked Cholesky inverse: K^-1, log|K|, info into the workspace); _reduce_f32 then
 * takes mu / logv (alpha = K^-1 mu with one fp64 refinement step -- the residual mu - K alpha0 is
 * evaluated from the covariates in fp64, hence spec / x / params / noise again, the same as the
 * factor's -- the trace and quadratic terms, kl, and with need_bwd the S-GEMM operand).  factor then
 * reduce on one stream (or with the reduce stream waiting on the factor's) equals
 * lvae_kl_closed_fwd_f32.  One reduce per factor: the reduce (diag K^-1 refinement) and the backward
 * reuse the factor's triangular-inverse planes in the workspace.                                 */
int lvae_kl_closed_factor_f32(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int L,
                              const double* params, const double* noise, int32_t* info, void* workspace,
                              void* stream);
int lvae_kl_closed_reduce_f32(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int L,
                              const double* params, const double* noise, const double* mu, const double* logv,
                              int ld_mu, double* kl, void* workspace, int need_bwd, void* stream);

/* Backward of lvae_kl_closed_fwd_f32 given dL/dkl[l] = gkl[l]:
 *   dmu[i,l] = gkl_l (K^-1 mu)_i,  dlogv[i,l] = gkl_l/2 (v_i (K^-1)_ii - 1),
 *   dparams[l,:] = gkl_l sum_ij G_ij dK_ij/dparams,  dnoise[l] = gkl_l tr(G),
 *   G = 1/2 (K^-1 - K^-1 V K^-1 - K^-1 mu mu^T K^-1).
 * Outputs are OVERWRITTEN.  Workspace must be the one the forward filled.                   */
int lvae_kl_closed_bwd_f32(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int L,
                           const double* params, const double* mu, const double* logv, int ld_mu,
                           const double* gkl, double* dmu, double* dlogv, double* dparams, double* dnoise,
                           void* workspace, void* stream);
/* The same backward in its two independent halves (lvae_kl_closed_bwd_f32 = _latent then _hyper), for
 * callers that start the encoder's backward on d/d(mu, logv) while the hyper-parameter half (the
 * S = K^-1 V K^-1 GEMM and the Gram adjoint: ~all of the backward's time) still runs. Either order. */
int lvae_kl_closed_bwd_latent_f32(int n, int L, const double* logv, int ld_mu, const double* gkl, double* dmu,
                                  double* dlogv, void* workspace, void* stream);
int lvae_kl_closed_bwd_hyper_f32(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int L,
                                 const double* params, const double* gkl, double* dparams, double* dnoise,
                                 void* workspace, void* stream);

/* diag(K^-1) in fp64 for ill-conditioned dims (kl_refine.hip): the reduce estimates each dim's
 * diagonal error by est_l = (sum_r s_r + noise_l) max_i (K^-1)_ii (the first factor bounds max_i K_ii) and where est_l > tau (env LVAE_KL_REFINE_TAU,
 * default 16; LVAE_KL_REFINE=0 never, =1 always) replaces diag K^-1 by one fp64 Newton step,
 * 2 X_jj - (X K X)_jj (the trace term and dlogv; the reference's cholesky_solve(I) is fp64,
 * elbo_functions.py:27-31).  This copies the last reduce's est [L] (fp64) and flag [L] (int32, 1:
 * refined) to device buffers, on `stream`.  No reference counterpart (diagnostic).                  */
int lvae_kl_closed_refine_state(int n, int L, const void* workspace, double* est, int32_t* flag, void* stream);

/* The backward's hyper-parameter half takes one of two routes, decided on the device from the covariates by the
 * factor (kl_hyper.hip): the S = K^-1 V K^-1 GEMM + the Gram adjoint, or -- for the table family of kernels on
 * integer-coded covariates with the "big" (id) covariate in contiguous runs -- the binned route (bin sums of
 * K^-1 and the id runs' blocks, no S; env LVAE_KL_HYPER=0 forces the GEMM route).  This copies the last
 * factor's choice (int32: 1 = binned) to a device buffer, on `stream`.  No reference counterpart (diagnostic). */
int lvae_kl_closed_hyper_state(int n, int L, const void* workspace, int32_t* on, void* stream);

/* The fp64 residual mu - K alpha0 behind the K^-1 mu refinement likewise takes one of two routes: binned O(N W)
 * (kl_resid_bins.hip: integer-coded covariates, a time window of at most 64 values) or tiled O(N^2).  This copies,
 * on `stream`, the last factor's covariate flag (int32; 0: some covariate is not an integer below 2^22, the Gram
 * kernels read fp64 covariates; 1: integer-coded, fp32 covariates; 2: integer-coded and every distance covariate
 * spans fewer than 64 values, the table kernels) and whether the binned residual runs (int32, 1 = binned; 0 also
 * when the host's gate is off: env LVAE_RESID_BINS=0 or a kernel outside the binned family).  No reference
 * counterpart (diagnostic). */
int lvae_kl_closed_resid_state(int n, int L, const void* workspace, int32_t* covflag, int32_t* binned,
                               void* stream);

/* A^-1 and log|A| of L padded SPD matrices by a blocked Cholesky factorisation, triangular inverse
 * and product (LAPACK potrf + trtri + lauum, 256-wide blocks; the inverse lvae_kl_closed_* use):
 * potrf's pivot blocks factored and inverted in LDS (fp32 MFMA), its panel / rank-256 trailing
 * updates and trtri / lauum's whole-block GEMMs on the f16 cores with the 3-product split; the next
 * pivot runs on a side stream beside each trailing update.  np % 256 == 0, np <= 16384; A [L, np, np] (lower
 * 256-block tiles read, overwritten); Ainv [L, np, np] full symmetric out; logdet [L]; info [L]
 * LAPACK-style (first bad column + 1); scratch: lvae_spd_inv_chol_scratch_size(np, L) bytes, 256-B
 * aligned.  Backward-stable in the Cholesky sense: |I - A Ainv| ~ cond(A) 2^-24 (the rounds 1-2 block
 * Gauss-Jordan sweep, ~100x less accurate at cond 1e5, is gone: commit 97b7453 is the last that holds spd_sweep.hip).
 * Replaces torch.cholesky + cholesky_solve(I) + the log-det (elbo_functions.py:26-29).
 * Returns 0, LVAE_ERR_LAUNCH, or before any launch: -3 (A NULL) -4 (scratch NULL or misaligned) -5 (Ainv NULL)
 * -6 (logdet NULL) -7 (info NULL) -1 (np <= 0, np % 256 != 0 or np > 16384) -2 (L <= 0), checked in that order. */
size_t lvae_spd_inv_chol_scratch_size(int np_, int L);
int lvae_spd_inv_chol_f32(int np_, int L, float* A, void* scratch, float* Ainv, double* logdet, int32_t* info,
                          void* stream);

/* ---------------------------------------------------------------------------------------- */
/* N x N factor / solve (potrf.hip): the reference's own LAPACK calls on K1,                   */
/*   LK1 = torch.cholesky(K1);  torch.cholesky_solve(B, LK1);  logdet = 2 sum log diag(LK1)    */
/* (elbo_functions.py:26-29), batched over L matrices: element (l, i, j) of a matrix argument   */
/* at ptr[l*stride + i*ld + j].  Factors are lower triangular with a zero strict upper part    */
/* (torch.cholesky's output); only the lower triangle of A is read.  info[l] LAPACK-style.     */
/* ---------------------------------------------------------------------------------------- */
/* Lout <- chol(A) in fp64, log|A| into logdet[l]: 64-wide blocked right-looking potrf, the panel
 * by substitution (as LAPACK's trsm), the trailing update on the fp64 matrix cores.  Lout may be
 * A itself (in place; then ldo == lda and stride_o == stride_a).  No workspace.              */
int lvae_potrf_f64(int n, int L, const double* A, int64_t lda, int64_t stride_a, double* Lout, int64_t ldo,
                   int64_t stride_o, double* logdet, int32_t* info, void* stream);
/* The same in fp32 through the exact KL's own factorisation (chol_inv.hip: 256-wide blocks, the
 * pivot blocks on fp32 MFMA in LDS, panels and trailing updates on the f16 cores with the 3-product
 * split, ~2^-22 of each 256-block's max per product).  A is copied into the workspace (padded to a
 * multiple of 256 with the identity), so Lout may alias A.  workspace:
 * lvae_potrf_f32_workspace_size(n, L) bytes, 256-B aligned.  n <= 16384.                       */
size_t lvae_potrf_f32_workspace_size(int n, int L);
int lvae_potrf_f32(int n, int L, const float* A, int64_t lda, int64_t stride_a, float* Lout, int64_t ldo,
                   int64_t stride_o, double* logdet, int32_t* info, void* workspace, void* stream);
/* B [n, nrhs] <- op(Lf)^-1 B in place, op = Lf (trans = 0) or Lf^T (trans = 1), Lf lower
 * triangular (e.g. lvae_potrf_*'s output).  Blocked over 64 rows: the 64 x 64 diagonal blocks are
 * inverted first into the workspace (lvae_trsm_workspace_size(n, L) bytes, 256-B aligned), then one
 * workgroup per 64 columns of B sweeps the block rows in dependency order on the fp64 matrix cores.
 * The f32 variant reads / writes fp32 and computes in fp64.  The strict upper part of Lf is not
 * read (lvae_potrs_* too); of B only the [n, nrhs] extent is written; nrhs == 0 returns 0.       */
size_t lvae_trsm_workspace_size(int n, int L);
int lvae_trsm_f64(int trans, int n, int nrhs, int L, const double* Lf, int64_t ldl, int64_t stride_l, double* B,
                  int64_t ldb, int64_t stride_b, void* workspace, void* stream);
int lvae_trsm_f32(int trans, int n, int nrhs, int L, const float* Lf, int64_t ldl, int64_t stride_l, float* B,
                  int64_t ldb, int64_t stride_b, void* workspace, void* stream);
/* B <- A^-1 B given Lf = chol(A): torch.cholesky_solve(B, Lf) (elbo_functions.py:27-28; also
 * cholesky_solve(eye, LK1) = K1^-1).  Workspace as lvae_trsm_*.                                */
int lvae_potrs_f64(int n, int nrhs, int L, const double* Lf, int64_t ldl, int64_t stride_l, double* B, int64_t ldb,
                   int64_t stride_b, void* workspace, void* stream);
int lvae_potrs_f32(int n, int nrhs, int L, const float* Lf, int64_t ldl, int64_t stride_l, float* B, int64_t ldb,
                   int64_t stride_b, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------- */
/* Regime A: Hensman SVI, fp64 (elbo_functions.py:144-216; training.py:129-135)             */
/* ---------------------------------------------------------------------------------------- */

/* Batched SPD factor + inverse of small matrices (n <= 128), one workgroup per matrix:
 * Ainv[b] = A[b]^-1, logdet[b] = log|A[b]|, info[b].  A, Ainv element (b,i,j) at [b*stride + i*n + j].
 * Only the lower triangle of A (j <= i) is read; both triangles of Ainv are written, and Ainv is
 * exactly symmetric (Ainv[i][j] and Ainv[j][i] are the same bits).                              */
int lvae_spd_inv_small_f64(int n, int batch, const double* A, int64_t stride, double* Ainv,
                           int64_t stride_out, double* logdet, int32_t* info, void* stream);

/* Batched small fp64 GEMM: C[b] = alpha op(A[b]) op(B[b]) + beta C[b],
 * with b = (b1, b2), b1 < nb1, b2 < nb2, offsets b1*s?1 + b2*s?2.  op = transpose when t? != 0.
 * beta == 0 overwrites C (it is not read).  -3 / -4 / -5: m / n / k < 0; -20 / -21: nb1 / nb2 < 1. */
int lvae_gemm_small_f64(int ta, int tb, int m, int n, int k, double alpha, const double* A, int lda,
                        int64_t sa1, int64_t sa2, const double* B, int ldb, int64_t sb1, int64_t sb2,
                        double beta, double* C, int ldc, int64_t sc1, int64_t sc2, int nb1, int nb2,
                        void* stream);

/* Hensman bound sizes: L latent dims, M inducing points, P_b subjects x T time points, Q covariates */
typedef struct lvae_hensman_dims {
  int32_t L, M, P_b, T, Q;
  double P_tot;            /* subjects in the data set (scale P_tot / P_b)                     */
  double eps;              /* jitter on K0zz                                                   */
  int32_t natural_gradient;
  double ng_prior_share;   /* weight of the data-independent part (iK m, iK, iH) in grad_m /   */
                           /* grad_H: 1 for one process; 1/world under data parallelism, so a  */
                           /* SUM all-reduce of the per-rank directions equals the union batch */
  const int32_t* seg_len;  /* varying T (minibatch_KLD_upper_bound_iter, elbo_functions.py:219-307): */
                           /* device [P_b] valid rows per subject, rows T_p..T-1 of subject p are  */
                           /* padding (masked out of every term); NULL = all T rows valid.         */
                           /* Padding rows of x are any finite covariates; padding rows of mu /    */
                           /* logv are not read (they may hold anything, NaN included); padding    */
                           /* rows of dmu / dlogv are written as 0.  A subject with seg_len == 0   */
                           /* contributes nothing to any sum (it still counts in P_b: pass         */
                           /* P_tot = P P_b / (subjects with rows) for the scale P / P_in_batch)   */
  double n_total;          /* N of the constant -L N / 2; 0 -> P_tot * T                          */
} lvae_hensman_dims;

/* The two size functions read *d unchecked (d must not be NULL; sizes are only meaningful for dims that the
 * calls below accept). */
size_t lvae_hensman_workspace_size(const lvae_hensman_dims* d);
/* Byte offset inside the Hensman workspace of H^-1 [L, M, M] as left by lvae_hensman_fwd_f64
 * (valid until the workspace is reused; lets the natural-gradient update skip re-inverting H). */
size_t lvae_hensman_iH_offset(const lvae_hensman_dims* d);

/* Forward of minibatch_KLD_upper_bound: kld (scalar, sum over L), grad_m [L,M], grad_H [L,M,M]
 * (natural_gradient only; may be NULL otherwise).  x [P_b*T, Q], z [L, M, Q], m [L, M], H [L, M, M],
 * mu / logv [P_b*T, L] (fp64, row-major), params0 [L, P0], params1 [L, P1], noise [L].
 * info [L] (may be NULL): 0, or the first failed factorisation of dim l in the order K0zz (10000 + col),
 * B_p (20000 + col, the first such subject), H (30000 + col), col the 1-based failing column; kld and the
 * gradients of such a call mean nothing.
 * Return codes of the three Hensman calls (all checked before any launch, nothing is written): -1 / -2: spec0 /
 * spec1 NULL or outside every template bucket; -3: d NULL, L < 1, M or T outside 1..128, P_b < 1 or Q < 1; then,
 * forward: -18: part outside 0..2, -17: workspace NULL or not 256-byte aligned; backward: -21: workspace NULL
 * or not 256-byte aligned.  0 = ok.                                                             */
int lvae_hensman_fwd_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1,
                         const lvae_hensman_dims* d, const double* x, const double* z, const double* m,
                         const double* H, const double* mu, const double* logv, const double* params0,
                         const double* params1, const double* noise, double* kld, double* grad_m,
                         double* grad_H, int32_t* info, void* workspace, void* stream);
/* The same forward in two parts on one workspace (part 0: both): part 1 needs neither mu nor logv
 * (Grams, the K0zz / B_p / H inverses, iK m, K0xz iK m, Q = K0xz^T B^-1 K0xz, iK H iK and the
 * data-independent natural-gradient terms incl. grad_H) and can run beside the encoder; part 2 (the
 * residual, the sums -> kld, grad_m, info) then reads mu / logv.  Same results as the one call, bit for bit.
 * Part 1 may get NULL mu / logv (and kld / info, which part 2 writes).  Both parts must receive the same
 * grad_m / grad_H pointers (NULL in both, or the same buffers): part 1 writes grad_H and decides by them
 * whether to prepare the terms of grad_m, which part 2 writes.                                       */
int lvae_hensman_fwd_part_f64(int part, const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1,
                              const lvae_hensman_dims* d, const double* x, const double* z, const double* m,
                              const double* H, const double* mu, const double* logv, const double* params0,
                              const double* params1, const double* noise, double* kld, double* grad_m,
                              double* grad_H, int32_t* info, void* workspace, void* stream);

/* Backward given dL/dkld = *gkld (device scalar): dmu, dlogv [P_b*T, L]; dparams0 [L,P0],
 * dparams1 [L,P1], dnoise [L]; dm [L,M], dH [L,M,M] when !natural_gradient (else may be NULL).
 * Outputs are OVERWRITTEN (whatever they held); dnoise may be NULL; with natural_gradient dm / dH are not
 * touched, and without it the forward does not touch grad_m / grad_H.  Runs on the workspace the forward
 * left.                                                                                         */
int lvae_hensman_bwd_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1,
                         const lvae_hensman_dims* d, const double* x, const double* z, const double* m,
                         const double* H, const double* mu, const double* logv, const double* params0,
                         const double* params1, const double* noise, const double* gkld, double* dmu,
                         double* dlogv, double* dparams0, double* dparams1, double* dnoise, double* dm,
                         double* dH, void* workspace, void* stream);

/* Natural-gradient update of the inducing posterior (training.py:129-135), in place:
 *   iH' = H^-1 + lr (gH + gH^T);  H <- iH'^-1;  m <- H (H^-1 m - lr (gm - 2 gH m)).
 * iH: H^-1 if the caller already has it (e.g. workspace + lvae_hensman_iH_offset after the
 * forward on the same H), else NULL (H is inverted here, as training.py:130-131 does).
 * info[l] (may be NULL): the first failed factorisation of dim l (H's, then iH''s), LAPACK-style;
 * if any dim's factorisation fails, NO dim's (m, H) is changed (the reference's batched
 * torch.cholesky raises before assigning, training.py:130-134).
 * workspace: lvae_natgrad_workspace_size(L, M) bytes.                                        */
size_t lvae_natgrad_workspace_size(int L, int M);
int lvae_natgrad_update_f64(int L, int M, double* m, double* H, const double* grad_m,
                            const double* grad_H, double lr, const double* iH, int32_t* info,
                            void* workspace, void* stream);

/* Full-batch deviance upper bound (DUBO, elbo_functions.py:86-142) of all L latent dims, and its adjoint.
 * P subjects of T consecutive rows each (N = P T rows), M inducing points, Q covariates.  Subjects of varying
 * length: the lvae_*_seg_f64 calls further down.                                                          */
typedef struct lvae_dubo_dims {
  int32_t L, M, P, T, Q;
  double eps;              /* jitter on K0zz */
} lvae_dubo_dims;

/* Reads *d unchecked (d must not be NULL; the size is only meaningful for dims that the calls below accept). */
size_t lvae_dubo_workspace_size(const lvae_dubo_dims* d);

/* Forward: dubo [L], one value per latent dim.  x [P*T, Q], z [L, M, Q], mu / logv [P*T, L] (fp64, row-major),
 * params0 [L, P0], params1 [L, P1], noise [L].  info [L] (may be NULL): 0, or the first failed factorisation of
 * dim l in the order K0zz (10000 + col), B_p (20000 + col, the first such subject), W = K0zz + K0zx B^-1 K0xz
 * (30000 + col), col the 1-based failing column; dubo[l] and that dim's gradients then mean nothing, the other
 * dims are unaffected.  Kernel launches only, on the caller's stream; nothing is allocated; no atomics: the same
 * inputs give the same bits on every call and every device (the split of the subjects over workgroups depends
 * on P alone).  T <= 32 runs the fused subject pass, larger T batched small products.
 * Return codes of both calls, checked in this order before any launch (nothing is written): -1 / -2: spec0 /
 * spec1 NULL or outside every template bucket; -3: d NULL, L < 1, M or T outside 1..128, P < 1 or Q < 1;
 * -4: workspace NULL or not 256-byte aligned.  0 = ok.                                               */
int lvae_dubo_fwd_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const lvae_dubo_dims* d,
                      const double* x, const double* z, const double* mu, const double* logv,
                      const double* params0, const double* params1, const double* noise, double* dubo,
                      int32_t* info, void* workspace, void* stream);
/* Backward given the cotangents gdubo [L] (device): dmu, dlogv [P*T, L]; dparams0 [L, P0], dparams1 [L, P1],
 * dnoise [L] (may be NULL); each dim's gradients are scaled by its own gdubo[l].  Outputs are OVERWRITTEN
 * (whatever they held).  Runs on the workspace the forward left (it may be called again on it).  The gradient
 * with respect to z is a separate call, lvae_dubo_bwd_z_f64.                                           */
int lvae_dubo_bwd_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const lvae_dubo_dims* d,
                      const double* x, const double* z, const double* mu, const double* logv,
                      const double* params0, const double* params1, const double* noise, const double* gdubo,
                      double* dmu, double* dlogv, double* dparams0, double* dparams1, double* dnoise,
                      void* workspace, void* stream);

/* Full-batch sampled GP ELBO (type_KL 'GPapprox', elbo_functions.py:36-84) of all L latent dims and S samples of
 * the latent at once, and its adjoint.  P subjects of T consecutive rows each (N = P T rows), M inducing points,
 * Q covariates, S samples (1..16: the columns of one MFMA tile; a caller with more splits them over calls).
 * Everything but the right-hand sides is shared by a dim's samples: the four Grams, K0zz^-1, B_p^-1 and W^-1 are
 * formed once per dim.                                                                                   */
typedef struct lvae_gp_elbo_dims {
  int32_t L, M, P, T, Q, S;
  double eps;              /* jitter on K0zz */
} lvae_gp_elbo_dims;

/* Reads *d unchecked (d must not be NULL; the size is only meaningful for dims that the calls below accept).
 * Always a multiple of 256.                                                                             */
size_t lvae_gp_elbo_workspace_size(const lvae_gp_elbo_dims* d);

/* Forward: elbo [S, L], elbo[s][l] = the reference's elbo() of dim l on the sample y[s][:, l].  x [P*T, Q],
 * z [L, M, Q], y [S, P*T, L] (fp64, row-major), params0 [L, P0], params1 [L, P1], noise [L].  info [L] (may be
 * NULL): 0, or the first failed factorisation of dim l in the order K0zz (10000 + col), B_p (20000 + col, the
 * first such subject), W = K0zz + K0zx B^-1 K0xz (30000 + col), col the 1-based failing column; elbo[:, l] and
 * that dim's gradients then mean nothing, the other dims are unaffected.  Kernel launches only, on the caller's
 * stream; nothing is allocated; no atomics: the same inputs give the same bits on every call and every device
 * (the split of the subjects over workgroups depends on P alone).  T <= 32 runs the fused subject pass, larger
 * T batched small products.  Row s of a call with S samples agrees with the S = 1 call on that sample to
 * rounding, not bit for bit (the sample's MFMA column differs).
 * Return codes of both calls, checked in this order before any launch (nothing is written): -1 / -2: spec0 /
 * spec1 NULL or outside every template bucket; -3: d NULL, L < 1, M or T outside 1..128, P < 1, Q < 1 or S
 * outside 1..16; -4: workspace NULL or not 256-byte aligned.  0 = ok.                                    */
int lvae_gp_elbo_fwd_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const lvae_gp_elbo_dims* d,
                         const double* x, const double* z, const double* y, const double* params0,
                         const double* params1, const double* noise, double* elbo, int32_t* info,
                         void* workspace, void* stream);
/* Backward given the cotangents gelbo [S, L] (device): dy [S, P*T, L]; dparams0 [L, P0], dparams1 [L, P1],
 * dnoise [L] (may be NULL), summed over the dim's samples, each weighted by its own gelbo[s][l].  Outputs are
 * OVERWRITTEN (whatever they held).  Runs on the workspace the forward left (it may be called again on it, with
 * the same bits out).  The gradient with respect to z is a separate call, lvae_gp_elbo_bwd_z_f64.        */
int lvae_gp_elbo_bwd_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const lvae_gp_elbo_dims* d,
                         const double* x, const double* z, const double* y, const double* params0,
                         const double* params1, const double* noise, const double* gelbo, double* dy,
                         double* dparams0, double* dparams1, double* dnoise, void* workspace, void* stream);

/* Subjects of varying length for the DUBO and the sampled ELBO (an extension: the reference has neither; the
 * Hensman bound's recipe, lvae_hensman_dims.seg_len).  The batch is laid out as [P, T] with T = d->T the longest
 * subject: subject p has its seg_len[p] valid rows first, the rest of its T rows is padding.  x, mu, logv, y (and
 * dmu, dlogv, dy) keep the shapes of the calls above in this padded layout.
 *   seg_len: device int32 [P], or NULL = all T rows valid; NULL gives the bits of the calls above, which are
 *     these calls with seg_len == NULL.
 *   PRECONDITION: 1 <= seg_len[p] <= T for every p -- a full batch has no empty subject (the Hensman bound allows
 *     0, these calls do not: lvae_*_bwd_z_f64 reads its cotangent factor back from row 0 of subject 0).  The
 *     kernels clamp what they read to [0, T]: a bad array gives wrong numbers, never an out-of-range access.
 *   Padding rows of x may hold any finite covariates.  Padding rows of mu, logv and y are never read (they may
 *     hold anything, NaN included).  Padding rows of dmu, dlogv and dy are written as exact 0.
 *   N of the constants (-N of the DUBO, -N/2 log 2 pi of the ELBO) is sum_p seg_len[p], summed on the device: the
 *     host never reads seg_len.
 * Per dim the padding rows of k0(x, z) and the padding rows / columns of K0_p are zeroed and those of B_p set to
 * the identity, so B_p^-1 is the identity there and log|B_p| that of the valid block; a failing B_p still reports
 * 20000 + col, and col lies inside the valid block.  In the fused subject pass (T <= 32) a subject's matrix-core
 * trip counts follow seg_len[p], not T.  Everything else -- return codes and their order, info, the workspace
 * and its size (lvae_dubo_workspace_size / lvae_gp_elbo_workspace_size of the same d), no atomics and the same
 * bits on every call -- is as the calls above.  lvae_dubo_bwd_z_f64 / lvae_gp_elbo_bwd_z_f64 follow a *_bwd_seg
 * call unchanged: the padding rows of the cotangent of k0(x, z) are exact zeros.                            */
int lvae_dubo_fwd_seg_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const lvae_dubo_dims* d,
                          const int32_t* seg_len, const double* x, const double* z, const double* mu,
                          const double* logv, const double* params0, const double* params1, const double* noise,
                          double* dubo, int32_t* info, void* workspace, void* stream);
int lvae_dubo_bwd_seg_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const lvae_dubo_dims* d,
                          const int32_t* seg_len, const double* x, const double* z, const double* mu,
                          const double* logv, const double* params0, const double* params1, const double* noise,
                          const double* gdubo, double* dmu, double* dlogv, double* dparams0, double* dparams1,
                          double* dnoise, void* workspace, void* stream);
int lvae_gp_elbo_fwd_seg_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1,
                             const lvae_gp_elbo_dims* d, const int32_t* seg_len, const double* x, const double* z,
                             const double* y, const double* params0, const double* params1, const double* noise,
                             double* elbo, int32_t* info, void* workspace, void* stream);
int lvae_gp_elbo_bwd_seg_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1,
                             const lvae_gp_elbo_dims* d, const int32_t* seg_len, const double* x, const double* z,
                             const double* y, const double* params0, const double* params1, const double* noise,
                             const double* gelbo, double* dy, double* dparams0, double* dparams1, double* dnoise,
                             void* workspace, void* stream);

/* The DUBO conditioned on a frozen prior, for inferring the latents of new subjects (the second half of
 * variational_inference_optimization, training.py:688-749: kernels, noise, inducing points and the other subjects'
 * (mu, logv) are fixed; only Pn "free" subjects' latents move).  Per latent dim, with m, l the free rows' mean and
 * log-variance, Nn = Pn T rows ordered (free subject in free_idx order, t):
 *   dubo_l(m, l) = c + 1/2 (m^T A m - 2 r^T m + sum_i a_i e^{l_i} - sum_i l_i)
 *   A = blockdiag(B_p^-1 : p free) - G W^-1 G^T  (G: the free rows of B^-1 K0xz),  a = diag(A),
 *   r = G W^-1 sum_{p not free} (B_p^-1 K0xz,p)^T m_p,   c = dubo_l(joint batch, m_free = 0, l_free = 0) - 1/2 sum_i a_i
 * -- the joint lvae_dubo_fwd_seg_f64 value exactly, as a function of the free rows.
 *
 * lvae_dubo_cond_state_size: bytes of the state (c, r, a, A and a row-validity mask) for L dims and Pn free
 *   subjects of T rows; a multiple of 256; 0 if an argument is < 1.  Needs no device.
 *
 * lvae_dubo_cond_prepare_f64 READS d, seg_len, x, z, mu, logv, params0, params1, noise exactly as
 *   lvae_dubo_fwd_seg_f64 on the joint [P, T] batch does (free and fixed subjects in any order), except that the free
 *   subjects' rows of mu / logv are taken as 0: those rows are never read and may hold anything, NaN included.
 *   free_idx: device int32 [Pn], strictly increasing subject indices in [0, P).  The host reads neither free_idx nor
 *   seg_len; the kernels clamp what they read from them: a bad array gives wrong numbers, never an out-of-range
 *   access.  It WRITES the whole state (overwritten, whatever it held), info [L] (may be NULL; the forward's
 *   meaning: a dim with a non-zero word has a meaningless state, the other dims are unaffected) and the workspace
 *   (lvae_dubo_workspace_size(d) bytes: the forward runs in it, and the copies of mu / logv, G and G W^-1 take
 *   [L, N, M] buffers the forward leaves idle; the matrix products run on the fp64 matrix cores).  With seg_len the
 *   padding rows and columns of A and the padding entries of a and r are exact 0.
 *   Return codes, in this order, before any launch (nothing is written): -1 / -2 / -3: as lvae_dubo_fwd_f64, -3 also
 *   for Pn < 1 or Pn > P; -4: workspace NULL or not 256-byte aligned; -5: state NULL or not 256-byte aligned;
 *   -6: free_idx NULL.  0 = ok.
 *
 * lvae_dubo_cond_eval_f64 READS the state (never written: several evals may share it) and m, logv [Pn*T, L] fp64
 *   row-major in the state's row order, g [L] cotangents (device; NULL = ones).  Padding rows of m / logv are never
 *   read.  It WRITES (overwrites) dubo [L], the values; dm = g_l (A m - r) and dlogv = g_l / 2 (a e^l - 1)
 *   [Pn*T, L], exact 0 on the padding rows.  One launch for Nn <= 256; beyond that the rows split over workgroups of
 *   256 rows whose partial sums are added in a fixed order by a second launch (they pass through dlogv, which that
 *   launch then overwrites: dlogv must not alias an input).  L, Pn, T must be those of the state's prepare.
 *   Return codes, in this order, before any launch: -3: L, Pn or T < 1; -5: state NULL or not 256-byte aligned;
 *   -7: m, logv, dubo, dm or dlogv NULL.  0 = ok.
 * Both calls: kernel launches only, on the caller's stream; nothing is allocated; no atomics: the same inputs give
 * the same bits on every call.                                                                            */
size_t lvae_dubo_cond_state_size(int L, int Pn, int T);
int lvae_dubo_cond_prepare_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const lvae_dubo_dims* d,
                               const int32_t* seg_len, int Pn, const int32_t* free_idx, const double* x,
                               const double* z, const double* mu, const double* logv, const double* params0,
                               const double* params1, const double* noise, void* state, int32_t* info,
                               void* workspace, void* stream);
int lvae_dubo_cond_eval_f64(int L, int Pn, int T, const void* state, const double* m, const double* logv,
                            const double* g, double* dubo, double* dm, double* dlogv, void* stream);

/* The exact N x N prior KL (lvae_kl_closed_*, elbo_functions.py:8-34) conditioned on a frozen prior and frozen training
 * latents, for inferring the latents of new rows under the loss a KL_closed-trained model was trained with: the joint
 * KL of cat(new, train) as a function of the nn new rows' mean m and log-variance l alone.  Per latent dim, with t the
 * n training rows (mu_t, v_t = exp(logv_t)) and K = k(., .) + noise I on the joint rows (the new rows carry the noise):
 *   W = K_tt^-1 K_tn [n, nn],  S = K_nn - K_nt W,  A = S^-1,  a = diag(A),  abar = W^T mu_t,  r = A abar
 *   c = 1/2 (abar^T A abar - nn + log|S| + tr(A W^T diag(v_t) W))
 *   cond_l(m, l) = c + 1/2 (m^T A m - 2 r^T m + sum_i a_i e^{l_i} - sum_i l_i)
 *                = KL_closed(joint rows, new rows = (m, l)) - KL_closed(training rows alone)
 * -- values and gradients with respect to (m, l).  The state is lvae_dubo_cond_eval_f64's own, with Pn = nn, T = 1 and
 * the mask all ones: size it with lvae_dubo_cond_state_size(L_state, nn, 1) and evaluate it with
 * lvae_dubo_cond_eval_f64(L_state, nn, 1, ...).  All fp64, on lvae_predict_exact_f64's route (lvae_gram_f64,
 * lvae_potrf_f64, lvae_trsm_f64 / lvae_potrs_f64); S and W^T diag(v_t) W come from a weighted tall-skinny SYRK on the
 * fp64 matrix cores (kl_cond.hip: 64 x 64 output blocks, slabs of 512 panel rows staged through LDS, the slabs'
 * partials added in slab order).
 *
 * lvae_kl_cond_workspace_size: bytes of the workspace for n training rows, nn new rows and L dims a call (about
 *   8 L (n^2 + n nn + 2 nn^2) + the SYRK's partials); a multiple of 256; 0 for n < 0, nn < 1 or L < 1.  Needs no device.
 *
 * lvae_kl_cond_prepare_f64 READS x_train [n, ldx], x_new [nn, ldn], params [L, n_params], noise [L], and mu_train /
 *   logv_train element (i, l) at [i*ld_mu + l] / [i*ld_lv + l], l < L: the L dims of this call, which fill the dims
 *   l0 .. l0 + L - 1 of a state sized for L_state dims (a caller under a workspace cap processes the dims in groups,
 *   passing each group's params, noise, mu_train, logv_train and info at its first dim; the bits of a dim do not depend
 *   on its group).  n == 0 is legal (every row new: cond is the plain exact KL of the new rows); x_train, mu_train and
 *   logv_train are then never read and may be NULL.  It WRITES c, r, a and A of those dims (A symmetric bit for bit),
 *   the state's mask (all ones), info [L] and the workspace; no other dim of the state is touched.  info[l]: 0, or
 *   col (LAPACK-style, the first failing column + 1) when K_tt of dim l is not positive definite, or 20000 + col when
 *   S is not; such a dim's state is meaningless, the other dims are unaffected.
 *   Returns 0, LVAE_ERR_LAUNCH, or before any launch (nothing is written), checked in this order: -1 (spec NULL or
 *   outside the family of lvae_gram_matvec_f64); with n > 0: -2 (x_train NULL) -3 (ldx < 1 + the largest column the
 *   spec reads); -4 (n < 0) -5 (x_new NULL) -6 (ldn, as ldx) -7 (nn < 1) -8 (L < 1 or L > 65535) -9 (params NULL)
 *   -10 (noise NULL); with n > 0: -11 (mu_train NULL) -12 (ld_mu < L) -13 (logv_train NULL) -14 (ld_lv < L);
 *   -15 (state NULL or not 256-byte aligned) -16 (L_state < 1, l0 < 0 or l0 + L > L_state) -17 (info NULL)
 *   -18 (workspace NULL or not 256-byte aligned).
 * Kernel launches only, on the caller's stream; nothing is allocated; no atomics and every sum in a fixed order: the
 * same inputs give the same bits on every call.                                                            */
size_t lvae_kl_cond_workspace_size(int n, int nn, int L);
int lvae_kl_cond_prepare_f64(const lvae_kernel_spec* spec, const double* x_train, int64_t ldx, int n,
                             const double* x_new, int64_t ldn, int nn, int L, const double* params,
                             const double* noise, const double* mu_train, int64_t ld_mu, const double* logv_train,
                             int64_t ld_lv, void* state, int L_state, int l0, int32_t* info, void* workspace,
                             void* stream);

/* Learnable inducing points: the gradient of the three inducing-point bounds with respect to z [L, M, Q] (the
 * reference gets it from autograd once LVAE.py:204-208, 269 / training.py:349 are uncommented).  Each bound's
 * backward leaves the cotangents of X = k0(x, z) [L, N, M] and of Kz = k0(z, z) + eps I [L, M, M] in its
 * workspace; these calls contract them with the kernel's input derivative (lvae_gram_bwd_x2_f64's kernels, three
 * jobs in one partial launch and one sum launch):
 *   dz[l] = d/dx2 of k0(x, z) against dX[l] + d/dx2 of k0(z, z) against dKz[l] + d/dx1 of k0(z, z) against dKz[l]
 * (the last as d/dx2 against dKz[l]^T; the jitter does not depend on z).  dz [L, M, Q] is OVERWRITTEN; columns of
 * categorical / binary factors and unread columns get exact zeros.  No atomics: the same bits on every call.
 * The DUBO's and the ELBO's calls first re-form dKz in zworkspace with its terms iK Q iK and iW R iW built from
 * N x M factors ((X iK)^T (iBK iK), (iBK iW)^T B_p (F iW)): with inducing rows that coincide for k0, a product
 * like (iK Q) iK carries rounding times 1 / eps in directions the hyper-parameter adjoint is blind to and dz is not
 * (gp_bound.hpp; the backwards themselves form both terms from such factors too, for the period derivatives' sake,
 * so they are re-formed to the same values).  The Hensman call reads dK0zz as the backward left it, formed term by
 * term from B x M factors.  None of this writes the bound's own workspace: the backward may run again on it, and so
 * may these calls.
 * PRECONDITION: the matching lvae_*_bwd_f64 has run on `workspace` since the last forward on it; the cotangent
 * scaling (gdubo[l], gelbo[s][l], *gkld) is then already inside dX / dKz.  x, z, params0 and d as that call's.
 * zworkspace: lvae_bound_dz_workspace_size(L, M, N, Q) bytes, N = P T rows (a multiple of 256; 0 for L, M, N or
 * Q < 1), 256-byte aligned; it is separate so that the bounds' own workspace sizes stay what they were.
 * With seg_len (Hensman) the padding rows contribute nothing: their rows of dK0xz are exact zeros.  A dim whose
 * info[l] is non-zero has a meaningless dz[l], like its other gradients; the other dims are unaffected.
 * Return codes, checked in this order before any launch (nothing is written): -1: spec0 NULL or outside every
 * template bucket; -3: d NULL or the dims its bound rejects; -1: spec0 reads a column >= min(Q, 32); then
 * workspace / zworkspace NULL or not 256-byte aligned: -4 / -5 (DUBO, ELBO), -21 / -22 (Hensman).  0 = ok.   */
size_t lvae_bound_dz_workspace_size(int L, int M, int N, int Q);
int lvae_dubo_bwd_z_f64(const lvae_kernel_spec* spec0, const lvae_dubo_dims* d, const double* x, const double* z,
                        const double* params0, double* dz, void* workspace, void* zworkspace, void* stream);
int lvae_gp_elbo_bwd_z_f64(const lvae_kernel_spec* spec0, const lvae_gp_elbo_dims* d, const double* x,
                           const double* z, const double* params0, double* dz, void* workspace, void* zworkspace,
                           void* stream);
int lvae_hensman_bwd_z_f64(const lvae_kernel_spec* spec0, const lvae_hensman_dims* d, const double* x,
                           const double* z, const double* params0, double* dz, void* workspace, void* zworkspace,
                           void* stream);

/* ConvVAE encoder (VAE.py:44-50): y = max_pool2d(relu(x), 2, 2) over planes = N*C planes of H x W
 * (H, W even) fp32, idx = argmax byte (0..3, row-major in the window, first strict maximum);
 * backward gx = the pooled gradient routed to the argmax unless y <= 0, 0 elsewhere.
 * NaN is kept as torch keeps it, here and in every encoder entry point below: a window that holds
 * a NaN gives y = NaN with idx = its last NaN in scan order, and a NaN y passes its gradient.  */
int lvae_relu_maxpool2_fwd_f32(const float* x, int64_t planes, int H, int W, float* y, uint8_t* idx,
                               void* stream);
int lvae_relu_maxpool2_bwd_f32(const float* gy, const float* y, const uint8_t* idx, int64_t planes, int H,
                               int W, float* gx, void* stream);
/* The same with the conv's per-channel bias folded in (the conv then runs without one): x is the
 * bias-free conv output [N, C, H, W], y = max_pool2d(relu(x + bias)); the backward also writes
 * db [C] = the conv's bias gradient (deterministic; workspace: lvae_relu_maxpool2_bias_workspace_size
 * bytes).  Replaces nn.Conv2d's bias add and its bias-gradient sum (VAE.py:44-50).             */
size_t lvae_relu_maxpool2_bias_workspace_size(int N, int C);
int lvae_relu_maxpool2_bias_fwd_f32(const float* x, const float* bias, int N, int C, int H, int W, float* y,
                                    uint8_t* idx, void* stream);
int lvae_relu_maxpool2_bias_bwd_f32(const float* gy, const float* y, const uint8_t* idx, int N, int C, int H, int W,
                                    float* gx, float* db, void* workspace, void* stream);
/* The first encoder conv end to end (VAE.py:44-47): x [N, 1, H, W], w [C, 1, 3, 3], bias [C],
 * padding 1 -> y = max_pool2d(relu(conv(x) + bias), 2, 2), idx as above; the full-resolution conv
 * output is never written.                                                                      */
int lvae_conv1_relu_maxpool2_fwd_f32(const float* x, const float* w, const float* bias, int N, int C, int H, int W,
                                     float* y, uint8_t* idx, void* stream);
/* The second encoder conv end to end (VAE.py:48-50): x [N, Cin, H, W], w [C, Cin, 3, 3], bias [C], padding 1 ->
 * y = max_pool2d(relu(conv(x) + bias), 2, 2) and idx as above, in one pass (no full-resolution output, no
 * layout transposes).  Cin == 16, H == W == 18 (the 36 x 36 images after the first pool), C % 16 == 0; -3 for
 * other shapes (conv + lvae_relu_maxpool2_bias_fwd_f32 cover them).                             */
int lvae_conv3x3_relu_maxpool2_fwd_f32(const float* x, const float* w, const float* bias, int N, int Cin, int C, int H,
                                       int W, float* y, uint8_t* idx, void* stream);
/* Weight and bias gradients of a 3x3 / stride-1 / padding-1 conv followed by the fused relu + pool
 * (the encoder convs), from the pooled gradient: dw [C, Cin, 3, 3] and db [C] as sums over the
 * pooled outputs of g * (the 3x3 input patch at the window's argmax) -- the full-resolution
 * gradient is needed only for the input gradient (the first conv's input, the image, needs none).
 * x: the conv input [N, Cin, H, W]; y, idx: the layer's forward outputs.  C * Cin <= 1024 and
 * Cin (H+2)(W+2) + 2 C (H/2)(W/2) floats within 64 KB of LDS (-3 / -4 otherwise).  Deterministic
 * (workspace: lvae_conv3x3_pool_wgrad_workspace_size bytes).                                   */
size_t lvae_conv3x3_pool_wgrad_workspace_size(int N, int C, int Cin);
int lvae_conv3x3_pool_wgrad_f32(const float* gy, const float* y, const uint8_t* idx, const float* x, int N, int C,
                                int Cin, int H, int W, float* dw, float* db, void* workspace, void* stream);
/* The input gradient of the same layer (the second encoder conv, VAE.py:48-50; torch's conv2d backward-data
 * in the reference's autograd): gx [N, Cin, H, W] = the conv's backward-data of the routed gradient (gy at
 * each window's argmax unless y <= 0), formed per image in LDS, never in HBM.  w [C, Cin, 3, 3].  Cin == 16
 * (-3 otherwise), H W <= 1024 and lvae_conv3x3_pool_dgrad_lds(C, H, W) <= 64 KB (-4 otherwise).      */
size_t lvae_conv3x3_pool_dgrad_lds(int C, int H, int W);
int lvae_conv3x3_pool_dgrad_f32(const float* gy, const float* y, const uint8_t* idx, const float* w, int N, int C,
                                int Cin, int H, int W, float* gx, void* stream);
/* ConvVAE decoder output (VAE.py:75, 124): out = sigmoid(ConvTranspose2d(Cin, 1, 4, stride 2, padding 1)
 * (z) + bias), z [N, Cin, Hi, Wi] (Cin <= 16), w [Cin, 1, 4, 4], bias [1] -> out [N, 1, 2Hi, 2Wi].
 * Backward from g = dLoss/dout and the saved out: gz [N, Cin, Hi, Wi], dw [Cin, 1, 4, 4], db [1]
 * (deterministic; workspace: lvae_deconv2_sigmoid_workspace_size bytes).                        */
size_t lvae_deconv2_sigmoid_workspace_size(int N, int Cin, int Hi, int Wi);
int lvae_deconv2_sigmoid_fwd_f32(const float* z, const float* w, const float* bias, int N, int Cin, int Hi, int Wi,
                                 float* out, void* stream);
int lvae_deconv2_sigmoid_bwd_f32(const float* g, const float* out, const float* z, const float* w, int N, int Cin,
                                 int Hi, int Wi, float* gz, float* dw, float* db, void* workspace, void* stream);
/* ConvVAE decoder's first transposed conv (VAE.py:73, 122): y = relu(ConvTranspose2d(Cin, Cout, 4, stride 2,
 * padding 1)(x) + bias), x [N, Cin, Hi, Wi], w [Cin, Cout, 4, 4], bias [Cout] -> y [N, Cout, 2Hi, 2Wi] (relu:
 * v < 0 -> 0, NaN kept).  Backward from gy = dLoss/dy and the saved y (mask y > 0): dx [N, Cin, Hi, Wi],
 * dw [Cin, Cout, 4, 4], db [Cout] in one pass + a fixed-order partial sum (deterministic; workspace:
 * lvae_deconv4s2_relu_bwd_workspace_size bytes).  Cin == 32, Cout == 16, Hi == Wi == 9; -3 otherwise.       */
int lvae_deconv4s2_relu_fwd_f32(const float* x, const float* w, const float* bias, int N, int Cin, int Cout, int Hi,
                                int Wi, float* y, void* stream);
size_t lvae_deconv4s2_relu_bwd_workspace_size(int N, int Cin, int Cout);
int lvae_deconv4s2_relu_bwd_f32(const float* gy, const float* y, const float* x, const float* w, int N, int Cin,
                                int Cout, int Hi, int Wi, float* dx, float* dw, float* db, void* workspace,
                                void* stream);

/* The MLP encoder / decoder (SimpleVAE, VAE.py:165-253; selected by type_nnet='simple', LVAE.py:59-70, 141-143),
 * fp32, each half one launch forward with its weights resident in LDS and every activation kept on chip, products
 * on v_mfma_f32_32x32x2_f32 (exact f32).  Weights are nn.Linear's [out, in] row-major; H1 = 300 and H2 = 30 are
 * the reference's hidden widths.  Deterministic: fixed-order sums, no float atomics.  relu: v < 0 -> 0, NaN kept;
 * a NaN in a row of the input stays in that row.
 * Return codes of the four compute entries, checked in this order before any launch: -1 (a required pointer NULL)
 * -2 (B, D, H1, H2 or L < 1) -3 (H1 != 300, H2 != 30 or L > 32) -4 (D beyond the LDS bound) -5 (workspace not
 * 256-byte aligned); 0 = ok, LVAE_ERR_LAUNCH on a HIP error.
 * lvae_mlp_vae_lds_bytes: the largest dynamic LDS any of the kernels asks for, 0 for a shape -2 / -3 reject:
 *   4 max(332 (D|1) + 19984 + 64 L,  302 D + 62 (L|1) + 20254) bytes (encoder / decoder forward);
 * lvae_mlp_vae_fused_ok: 1 when that is within the 160 KiB of a CU, i.e. for L <= 32 exactly D <= 57 (and for
 * every 1 <= D <= 48, 1 <= L <= 32).  Host only, like the two workspace sizes and lvae_mlp_wgrad_splits.
 * More than 64 KB of dynamic LDS is asked for with hipFuncSetAttribute, per kernel and per device: each compute entry
 * remembers (one atomic bit per device id < 64) on which devices it has asked and asks again on a new one, so any
 * device of the process may be current; the first call per device should come before a stream capture.          */
int lvae_mlp_vae_fused_ok(int D, int H1, int H2, int L);
size_t lvae_mlp_vae_lds_bytes(int D, int H1, int H2, int L);
/* encode (VAE.py:215-224): x [B, D] -> h1 = relu(fc1 x) [B, 300], h2 = relu(fc21 h1) [B, 30], mu = fc211 h2,
 * log_var = fc221 h2 [B, L].  h1 / h2 are the backward's saved activations and may be NULL (no_grad).           */
int lvae_mlp_enc_fwd_f32(const float* x, const float* w1, const float* b1, const float* w21, const float* b21,
                         const float* w211, const float* b211, const float* w221, const float* b221, int B, int D,
                         int H1, int H2, int L, float* h1, float* h2, float* mu, float* log_var, void* stream);
/* decode (VAE.py:226-235): h3 = relu(fc3 z) [B, 30], h4 = relu(fc31 h3) [B, 300], recon = sigmoid(fc4 h4) [B, D].
 * Either z [B, L] is given, or z is NULL and (mu, log_var, eps) are: then z = mu + eps exp(log_var / 2)
 * (sample_latent, VAE.py:237-248) is formed in the same launch and written to z_out [B, L] (required then; not
 * touched when z is given).  h3 / h4 may be NULL (no_grad).                                                    */
int lvae_mlp_dec_fwd_f32(const float* z, const float* mu, const float* log_var, const float* eps, const float* w3,
                         const float* b3, const float* w31, const float* b31, const float* w4, const float* b4, int B,
                         int D, int H1, int H2, int L, float* z_out, float* h3, float* h4, float* recon,
                         void* stream);
/* The decoder's autograd backward (of VAE.py:226-248) from g_recon = dLoss/drecon and the saved recon, h4, h3, z:
 * all weight and bias gradients and g_z [B, L].  Sampled form (log_var and eps given, as saved by the forward's
 * sampled form): g_mu = g_z and g_log_var = g_z eps exp(log_var / 2) / 2 are written (both required; g_z may then
 * be NULL); otherwise log_var, eps, g_mu and g_log_var are all NULL and g_z is required.  Two launches: the
 * activation-gradient chain, then every dW = g^T h and db at once (dw3 .. db4 all NULL: a frozen decoder, the second
 * launch is skipped; some but not all NULL is -1); rows are summed in order, and for
 * lvae_mlp_wgrad_splits(B) >= 2 (B > 512) in that many chunks whose partial tiles are added in chunk order.
 * workspace: lvae_mlp_dec_bwd_workspace_size(B, D, L) bytes, 256-byte aligned.                                  */
size_t lvae_mlp_dec_bwd_workspace_size(int B, int D, int L);
int lvae_mlp_dec_bwd_f32(const float* g_recon, const float* recon, const float* h4, const float* h3, const float* z,
                         const float* log_var, const float* eps, const float* w3, const float* w31, const float* w4,
                         int B, int D, int H1, int H2, int L, float* dw3, float* db3, float* dw31, float* db31,
                         float* dw4, float* db4, float* g_z, float* g_mu, float* g_log_var, void* workspace,
                         void* stream);
/* The encoder's autograd backward (of VAE.py:215-224) from g_mu, g_log_var [B, L] (where the GP bound's gradient
 * arrives) and the saved x, h1, h2: all weight and bias gradients; the input gets none.  Two launches, as above.
 * workspace: lvae_mlp_enc_bwd_workspace_size(B, D, L) bytes, 256-byte aligned.                                  */
size_t lvae_mlp_enc_bwd_workspace_size(int B, int D, int L);
int lvae_mlp_enc_bwd_f32(const float* g_mu, const float* g_log_var, const float* x, const float* h1, const float* h2,
                         const float* w21, const float* w211, const float* w221, int B, int D, int H1, int H2, int L,
                         float* dw1, float* db1, float* dw21, float* db21, float* dw211, float* db211, float* dw221,
                         float* db221, void* workspace, void* stream);
/* The number of row chunks the two backward entries cut a batch of B rows into (1 up to 512 rows, then
 * min(64, ceil(B / 512))); 0 for B < 1.                                                                         */
int lvae_mlp_wgrad_splits(int B);

/* GP posterior mean of the latents at test covariates (utils.py:115-211 batch_predict_varying_T,
 * called by MSE_test_GPapprox, model_test.py:85-143).  Prediction set laid out [P, T] by subject
 * (seg_len [P] valid rows each; padding rows of x are any finite covariates, of mu must be 0),
 * x [P*T, Q], mu [P*T, L]; include [P] = 1 for subjects that also appear in test_x (the k1 term);
 * z [L, M, Q]; test_x [Nt, Q]; out [Nt, L].  info[l]: 10000/20000/30000 + col for a failed
 * K0zz / B_p / H factorisation, the first of them in that order (info may be NULL; it is written for
 * Nt == 0 too, out is not).  workspace: lvae_predict_workspace_size(L, M, P, T, Nt) bytes.
 * Return codes (all checked before any launch): -1: spec0 / spec1 NULL or outside every template bucket;
 * -3: L < 1 or M outside 1..128; -6: P < 1, T outside 1..128 or Q < 1; -8: seg_len or include NULL;
 * -13: Nt < 0; -20: workspace NULL or not 256-byte aligned.  0 = ok.                              */
size_t lvae_predict_workspace_size(int L, int M, int P, int T, int Nt);
int lvae_predict_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P,
                     int T, const int32_t* seg_len, const int32_t* include, const double* x,
                     const double* mu, const double* z, int Nt, const double* test_x,
                     const double* params0, const double* params1, const double* noise, double eps,
                     double* out, int32_t* info, void* workspace, void* stream);

/* Exact-GP posterior mean of the latents at test covariates (model_test.py:11-17 predict_gp as MSE_test calls it,
 * model_test.py:19-82), all in fp64:
 *   out[t, l] = k_l(tx_t, x) (k_l(x, x) + noise_l I)^-1 mu[:, l]         t < nt, l < L
 * x [n, ldx] the prediction set's covariates, mu element (i, l) at mu[i*ld_mu + l], tx [nt, ldt], out element
 * (t, l) at out[t*ld_out + l].  Kernel launches only, enqueued on the caller's stream, nothing allocated
 * (capture into a HIP graph is not covered by a test):
 * lvae_gram_f64 with diag = noise into the workspace, lvae_potrf_f64 in place (info[l] LAPACK-style: a dim that
 * is not positive definite leaves info[l] > 0, its outputs are then meaningless and every other dim's are
 * unaffected), lvae_potrs_f64 for a0 = K^-1 mu, one refinement step a = a0 + K^-1 (mu - K a0) with K a0 from
 * lvae_gram_matvec_f64's kernel (K is gone after the in-place factor), and that kernel again for k(tx, x) a.
 * The reference forms the explicit inverse instead (torch.cholesky_solve(eye, L)).  nt == 0: the factor runs
 * (info is written), out is untouched.  workspace: lvae_predict_exact_workspace_size(n, nt, L) bytes (about
 * 8 L n^2; 0 for n < 1, nt < 0 or L < 1), 256-B aligned.
 * Returns 0, LVAE_ERR_LAUNCH, or before any launch, checked in this order: -1 (spec NULL or outside the family of
 * lvae_gram_matvec_f64) -2 (x NULL) -3 (ldx < 1 + the largest column the spec reads) -4 (n < 1) -5 (L < 1)
 * -6 (params NULL) -7 (noise NULL) -8 (mu NULL) -9 (ld_mu < L) -12 (nt < 0); with nt > 0: -10 (tx NULL)
 * -11 (ldt, as ldx) -13 (out NULL) -14 (ld_out < L); -15 (info NULL) -16 (workspace NULL or misaligned).   */
size_t lvae_predict_exact_workspace_size(int n, int nt, int L);
int lvae_predict_exact_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                           const double* params, const double* noise, const double* mu, int64_t ld_mu,
                           const double* tx, int64_t ldt, int nt, double* out, int64_t ld_out, int32_t* info,
                           void* workspace, void* stream);

/* Both posterior means split by additive component of the kernel (each is linear in the kernel, so the split is
 * exact): what each covariate effect contributes to the predicted latents.
 *
 * lvae_predict_exact_comp_f64: lvae_predict_exact_f64's arguments and launches (out and info receive its bits), then
 *   out_comp[r, t, l] = k_{l,r}(tx_t, x) a_l,   a_l = (k_l(x, x) + noise_l I)^-1 mu[:, l] as refined there,
 * by lvae_gram_matvec_comp_f64's kernel, element (r, t, l) at out_comp[r*cstride_r + t*ld_comp + l], r < R =
 * spec->n_comp; sum_r out_comp[r] = out up to rounding.  nt == 0: the factor runs, out and out_comp are untouched.
 * workspace: lvae_predict_exact_comp_workspace_size(n, nt, L, R) bytes (lvae_predict_exact_f64's + the component
 * product's slab partials; 0 for n < 1, nt < 0, L < 1 or R < 1), 256-B aligned.
 * Returns 0, LVAE_ERR_LAUNCH, or before any launch, in this order: -1 .. -16 as lvae_predict_exact_f64; with nt > 0:
 * -17 (out_comp NULL) -18 (ld_comp < L) -19 (R > 1 and cstride_r < nt*ld_comp).
 *
 * lvae_predict_comp_f64: lvae_predict_f64's arguments and launches (out and info receive its bits; the dense
 * chunked k1 route of the summed mean included), then, with b_l = K0zz^-1 K0zx mu~_l and mu~m_l (mu~_l on the valid
 * rows of the subjects in the test set, 0 elsewhere) as they are left in the workspace,
 *   out_comp[r, i, l]      = k0_{l,r}(X*_i, z_l) b_l        r < R0 = spec0->n_comp
 *   out_comp[R0 + r, i, l] = k1_{l,r}(X*_i, x) mu~m_l       r < R1 = spec1->n_comp
 * two launches of lvae_gram_matvec_comp_f64's kernel (z per latent dim, x shared), element (r, i, l) at
 * out_comp[r*cstride_r + i*ld_comp + l]; sum_r out_comp[r] = out up to rounding.  Nt == 0: info is written, out and
 * out_comp are untouched.  workspace: lvae_predict_comp_workspace_size(L, M, P, T, Nt, R0, R1) bytes, 256-B aligned.
 * Return codes (before any launch): -1 -3 -6 -8 -13 -20 as lvae_predict_f64, and also -1: a factor dim of either
 * spec outside 0 .. 31; -6: Q < 1 + the largest column either spec reads; with Nt > 0: -21 (out_comp NULL)
 * -22 (ld_comp < L) -23 (R0 + R1 > 1 and cstride_r < Nt*ld_comp).  0 = ok.                                  */
size_t lvae_predict_exact_comp_workspace_size(int n, int nt, int L, int n_comp);
int lvae_predict_exact_comp_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                                const double* params, const double* noise, const double* mu, int64_t ld_mu,
                                const double* tx, int64_t ldt, int nt, double* out, int64_t ld_out, double* out_comp,
                                int64_t ld_comp, int64_t cstride_r, int32_t* info, void* workspace, void* stream);
size_t lvae_predict_comp_workspace_size(int L, int M, int P, int T, int Nt, int n_comp0, int n_comp1);
int lvae_predict_comp_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P,
                          int T, const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                          const double* z, int Nt, const double* test_x, const double* params0,
                          const double* params1, const double* noise, double eps, double* out, double* out_comp,
                          int64_t ld_comp, int64_t cstride_r, int32_t* info, void* workspace, void* stream);

/* Joint posterior covariance of the R additive component functions f_1(x*_t) .. f_R(x*_t) at each test row, under
 * both predictors, fp64: an R x R block per (latent dim, test row).  The component means stay those of the two
 * functions above; the observation noise belongs to no component and is never added.  Both return the raw
 * difference (not clamped), in blocks that are symmetric bit for bit ([r][s] and [s][r] are one computed value) and
 * laid out as the sibling covariances' [L, n_groups, n_max, n_max] with a group = one test row and n_max = R, without
 * padding.  Covariances between components at different test rows are not formed.
 *
 * lvae_predict_exact_comp_cov_f64: lvae_predict_exact_comp_f64's arguments plus chunk and out_ccov.  With
 * K_l = k_l(x, x) + noise_l I = L_l L_l^T and V_r = L_l^-1 k_{l,r}(x, tx_t),
 *   out_ccov[l, t, r, s] = (r == s) k_{l,r}(tx_t, tx_t) - V_r . V_s            r, s < R = spec->n_comp (1 .. 16)
 * block (l, t) at out_ccov[(l*nt + t)*R*R]; sum_{r,s} out_ccov[l, t] = lvae_predict_exact_var_f64's out_var[t, l]
 * (add_noise = 0) up to rounding.  out may be NULL (then mu may be too, as for lvae_predict_exact_var_f64) and
 * out_comp may be NULL; out_comp needs out.  When given, out, out_comp and info receive
 * lvae_predict_exact_comp_f64's bits (the same launches).  Route: the Gram, lvae_potrf_f64 and the means as there;
 * then per chunk of c = min(chunk, nt) test rows one kernel writes the component-resolved panel k_{l,r}(x, tx_chunk)
 * as [L, n, c R], column t R + r (row-major, component-minor; the spec is evaluated once per (i, t) pair and the R
 * component values scattered), lvae_trsm_f64 (trans = 0) runs in place on the c R columns, and an fp64 matrix-core
 * kernel (v_mfma_f64_16x16x4) forms each row's V^T V as one 16 x 16 tile (columns r >= R zero), the n prediction rows
 * cut into slabs of 512 whose partial tiles go to the workspace and are added in slab order under the prior
 * variances k_{l,r}(tx_t, tx_t) evaluated through the spec (lvae_predict_exact_cov_f64's V^T V step with a test
 * row's components in the role of a group's rows).  No atomics, every sum in a fixed order: the bits depend on
 * neither the grid nor the chunk.  A component whose cross-Gram vanishes everywhere (an id component for an unseen
 * subject) gives exact zeros off the diagonal and its exact prior on it.  n^2 R nt fp64 flops per dim in the
 * solves.  nt == 0: the factor runs (info is written), nothing else is touched.  workspace:
 * lvae_predict_exact_comp_cov_workspace_size(n, nt, L, R, chunk) bytes (lvae_predict_exact_comp_f64's + 8 L n c R
 * for the panel + 2048 L c ceil(n / 512) for the partial tiles; 0 for n < 1, nt < 0, L < 1, R outside 1 .. 16 or,
 * with nt > 0, chunk < 1), 256-B aligned.
 * Returns 0, LVAE_ERR_LAUNCH, or before any launch, in this order: -1 .. -7 as lvae_predict_exact_comp_f64 (-1 also
 * for a spec without components, -5 also for L > 65535); with out: -8 (mu NULL) -9 (ld_mu < L); -12 (nt < 0); with
 * nt > 0: -10 (tx NULL) -11 (ldt) -13 (out_comp given and out NULL); with out: -14 (ld_out < L); -15 (info NULL) -16
 * (workspace NULL or misaligned); with nt > 0 and out_comp: -18 (ld_comp < L) -19 (R > 1 and cstride_r < nt*ld_comp);
 * with nt > 0: -20 (chunk < 1) -21 (out_ccov NULL).
 *
 * lvae_predict_comp_cov_f64: lvae_predict_comp_f64's arguments plus the test-row groups of lvae_predict_var_f64
 * (n_groups, group_subject, group_start: test_x's rows grouped by subject) and out_ccov.  The model is
 * lvae_predict_var_f64's structured one, its algebra run with one column per (test row i, component r), column
 * i R + r, R = R0 + R1 <= 32, the components of spec0 first: a column r < R0 has K0zX* = k0_r(z, x*_i) and c = 0, a
 * column r >= R0 has K0zX* = 0 and c = k1_{r-R0}(x_s(i), x*_i) on the subject's valid rows (0 for an absent
 * subject); d, e, q, w, v follow from those columns by lvae_predict_var_f64's own kernels on the Nt R columns, and
 *   out_ccov[l, i, r, s] = K0zX*_(i,r) . q_(i,s) + [r = s >= R0] k1_{r-R0}(x*_i, x*_i)
 *                          - (q_(i,r) . w_(i,s) + e_(i,r) . q_(i,s) + c_(i,r) . d_(i,s)) + w_(i,r) . v_(i,s)
 * by lvae_predict_cov_f64's tile products with a test row as the group and its components as the group's rows (up
 * to 2 x 2 tiles of 16, on or below the diagonal and mirrored); block (l, i) at out_ccov[(l*Nt + i)*R*R];
 * sum_{r,s} out_ccov[l, i] = lvae_predict_var_f64's out_var[i, l] (add_noise = 0) up to rounding.  The prior of the
 * shared components is the Nystrom form k0_r(x*, z) K0zz^-1 k0_s(z, x*): in this model two different components of
 * spec0 are correlated a priori, and a shared component's prior variance is not k0_r(x*, x*).  Every reduction runs
 * over M or T in index order and a column's results do not depend on its neighbours, so a row's block does not
 * depend on which other rows are in the call.  A component whose column is zero (an id component for an absent
 * subject) gives exact zeros off the diagonal and its exact prior on it.  out (the mean) may be NULL (then mu may
 * be too) and out_comp may be NULL; out_comp needs out.  When given, out, out_comp and info receive
 * lvae_predict_comp_f64's bits (the same launches).  Nt == 0: info is written, nothing else is touched.
 * workspace: lvae_predict_comp_cov_workspace_size(L, M, P, T, Nt, R0, R1) bytes = lvae_predict_var_workspace_size(L,
 * M, P, T, Nt R) + the component products' slab partials (lvae_predict_comp_workspace_size -
 * lvae_predict_workspace_size at Nt rows); 0 for sizes the call rejects (L < 1, M or T outside 1 .. 128, P < 1, Nt < 0, R0 or R1 outside 1 .. 16,
 * Nt R > 2^31 - 1); 256-B aligned.
 * Return codes (before any launch), in this order: -1 (a spec NULL, outside every template bucket, without
 * components, or a factor dim outside 0 .. 31) -3 (L outside 1 .. 65535 or M outside 1 .. 128) -6 (P < 1, T outside
 * 1 .. 128, Q < 1 + the largest column either spec reads) -8 (seg_len or include NULL) -9 (out given and mu NULL)
 * -10 (x or z NULL) -11 (params0, params1 or noise NULL) -13 (Nt < 0 or Nt R > 2^31 - 1) -12 (Nt > 0 and test_x
 * NULL) -14 (n_groups < 0) -15 (n_groups > 0 and group_subject or group_start NULL) -20 (workspace NULL or
 * misaligned); with Nt > 0: -21 (out_comp given and out NULL) -22 (out_comp given and ld_comp < L) -23 (out_comp
 * given and cstride_r < Nt*ld_comp) -24 (out_ccov NULL).  0 = ok.                                            */
size_t lvae_predict_exact_comp_cov_workspace_size(int n, int nt, int L, int n_comp, int chunk);
int lvae_predict_exact_comp_cov_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                                    const double* params, const double* noise, const double* mu, int64_t ld_mu,
                                    const double* tx, int64_t ldt, int nt, double* out, int64_t ld_out,
                                    double* out_comp, int64_t ld_comp, int64_t cstride_r, int chunk, double* out_ccov,
                                    int32_t* info, void* workspace, void* stream);
size_t lvae_predict_comp_cov_workspace_size(int L, int M, int P, int T, int Nt, int n_comp0, int n_comp1);
int lvae_predict_comp_cov_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P,
                              int T, const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                              const double* z, int Nt, const double* test_x, int n_groups,
                              const int32_t* group_subject, const int32_t* group_start, const double* params0,
                              const double* params1, const double* noise, double eps, double* out, double* out_comp,
                              int64_t ld_comp, int64_t cstride_r, double* out_ccov, int32_t* info, void* workspace,
                              void* stream);

/* Exact-GP predictive variance (and, optionally, the mean) of the latent functions at test covariates, fp64.  With
 * K_l = k_l(x, x) + noise_l I = L_l L_l^T:
 *   out_var[t, l] = k_l(tx_t, tx_t) - |L_l^-1 k_l(x, tx_t)|^2  (+ noise_l when add_noise = 1)
 * the raw difference (not clamped), element (t, l) at out_var[t*ld_var + l].  Arguments as lvae_predict_exact_f64;
 * out_mean may be NULL (then mu may be too), and when given it receives lvae_predict_exact_f64's bits (the same
 * launches).  Route: the Gram and lvae_potrf_f64 as there; then per chunk of c = min(chunk, nt) test rows the
 * panel k(x, tx_chunk) [L, n, c] by lvae_gram_f64, lvae_trsm_f64 (trans = 0) in place, and one kernel that forms
 * k(tx, tx) through the spec and subtracts each column's sum of squares in a fixed order (no atomics): the bits
 * depend on neither the grid nor the chunk, and the [nt, n] cross-Gram is never whole in memory.  n^2 nt fp64 flops
 * per dim in the solves.  nt == 0: the factor runs (info is written), nothing else is touched.  workspace:
 * lvae_predict_exact_var_workspace_size(n, nt, L, chunk) bytes (lvae_predict_exact_f64's + 8 L n c; 0 for n < 1,
 * nt < 0, L < 1 or, with nt > 0, chunk < 1), 256-B aligned.
 * Returns 0, LVAE_ERR_LAUNCH, or before any launch, in this order: -1 .. -7 as lvae_predict_exact_f64; with
 * out_mean: -8 (mu NULL) -9 (ld_mu < L); -12 (nt < 0); with nt > 0: -10 (tx NULL) -11 (ldt); with out_mean: -14
 * (ld_out < L); -15 (info NULL) -16 (workspace NULL or misaligned); with nt > 0: -17 (out_var NULL) -18
 * (ld_var < L); -19 (add_noise not 0 / 1); with nt > 0: -20 (chunk < 1).                                  */
size_t lvae_predict_exact_var_workspace_size(int n, int nt, int L, int chunk);
int lvae_predict_exact_var_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                               const double* params, const double* noise, const double* mu, int64_t ld_mu,
                               const double* tx, int64_t ldt, int nt, double* out_mean, int64_t ld_out,
                               double* out_var, int64_t ld_var, int add_noise, int chunk, int32_t* info,
                               void* workspace, void* stream);

/* Predictive variance (and, optionally, the mean) of the inducing-point predictor, in the structured model
 * lvae_predict_f64's mean assumes: prior K~ = K0xz K0zz^-1 K0zx + blockdiag_p k1(x_p, x_p) (K0zz with eps I),
 * Sigma = K~ + noise I, Sigma^-1 = iB - iB K0xz H^-1 K0zx iB.  Per latent dim and test row i of subject s:
 *   q = K0zz^-1 K0zX*_i,  c = k1(x_s, x*_i) on subject s's valid rows (empty when s is not a prediction subject),
 *   d = iB_s c,  e = K0zx_s d,  G = H - K0zz = K0zx iB K0xz,  w = G q + e,
 *   out_var[i, l] = K0X*z_i . q + k1(x*_i, x*_i) - (q^T G q + 2 q^T e + c^T d) + w^T H^-1 w  (+ noise_l when add_noise = 1)
 * = k~** - k~*^T Sigma^-1 k~*, the raw difference (not clamped).  k1 is taken to vanish between subjects (every
 * component of spec1 carries the id covariate's cat factor).  Arguments as lvae_predict_f64, plus the test-row
 * layout: test_x's rows grouped by subject, group g = rows [group_start[g], group_start[g + 1]) (device arrays,
 * n_groups and n_groups + 1 entries) of prediction subject group_subject[g] (its index 0 .. P - 1 in the [P, T]
 * layout, or -1: absent); rows in no group count as absent.  out (the mean, [Nt, L]) may be NULL (then mu may be
 * too); when given it receives lvae_predict_f64's bits (the same launches).  out_var [Nt, L].  The per-row algebra
 * runs with the test rows as the columns of fp64 matrix-core tiles; q and H^-1 w take one residual refinement step
 * each; every reduction is in a fixed order.  O((M^2 + T^2 + M T) Nt) flops per dim.  info as lvae_predict_f64.
 * workspace: lvae_predict_var_workspace_size(L, M, P, T, Nt) bytes (lvae_predict_f64's + 8 L ((2 T + 6 M) Nt + M^2)).
 * Return codes (before any launch): -1 -3 -6 -8 -13 -20 as lvae_predict_f64; -9: out given and mu NULL; -10: x or
 * z NULL; -11: params0, params1 or noise NULL; -12: Nt > 0 and test_x NULL; -14: n_groups < 0; -15: n_groups > 0 and
 * group_subject or group_start NULL; -16: Nt > 0 and out_var NULL; -17: add_noise not 0 / 1.  0 = ok.   */
size_t lvae_predict_var_workspace_size(int L, int M, int P, int T, int Nt);
int lvae_predict_var_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P,
                         int T, const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                         const double* z, int Nt, const double* test_x, int n_groups, const int32_t* group_subject,
                         const int32_t* group_start, const double* params0, const double* params1,
                         const double* noise, double eps, double* out, double* out_var, int add_noise, int32_t* info,
                         void* workspace, void* stream);

/* Joint predictive covariance of each group of test rows under the inducing-point predictor (and, optionally, the
 * mean), fp64: per latent dim l and group g of n_g test rows, in lvae_predict_var_f64's model and notation (the
 * subscript g selects the group's columns of its [rows, Nt] matrices),
 *   Sigma_g = K0zX*_g^T Q_g + k1(x*_g, x*_g) - (Q_g^T W_g + E_g^T Q_g + C_g^T D_g) + W_g^T V_g      [n_g, n_g]
 * = k~**_g - k~*_g^T Sigma^-1 k~*_g, the raw difference; add_noise = 1 adds noise_l to its diagonal.  Its diagonal
 * is lvae_predict_var_f64's formula; for a group of an absent subject C, D and E are zero and the k1 term stays.
 * The covariance between rows of different groups is not zero (the shared components couple subjects) and is not
 * returned.  Arguments as lvae_predict_var_f64 with, in place of out_var: n_max, the rows of the largest group
 * (1 .. 128 when n_groups > 0), and out_cov [L, n_groups, n_max, n_max], block (l, g) at
 * out_cov[(l*n_groups + g)*n_max*n_max], row i of a block the group's i-th row (test_x's row group_start[g] + i);
 * rows of a group beyond n_max are left out.  Padding rows and columns (i or j >= n_g) carry the identity, and a
 * block is symmetric bit for bit ([i][j] and [j][i] are one computed value).  Route: lvae_predict_var_f64's
 * launches up to V (the same buffers, no second pass over the prediction set), one kernel that fills the blocks
 * with the identity, and one fp64 matrix-core kernel with a workgroup per (dim, group, 16 x 16 tile on or below the
 * diagonal) that accumulates the five products over M and T in index order and adds k1(x*_i, x*_j) through the
 * spec.  O((M + T) n_g^2) flops per dim and group on top of the variance's.  out, info, Nt == 0 as
 * lvae_predict_var_f64; with Nt == 0 or n_groups == 0 out_cov is untouched.  workspace:
 * lvae_predict_cov_workspace_size(L, M, P, T, Nt) bytes (= lvae_predict_var_workspace_size's).
 * Return codes (before any launch): -1 -6 -8 -9 -10 -11 -12 -13 -15 -17 -20 as lvae_predict_var_f64; -3: also
 * L > 65535; -14: n_groups outside 0 .. 65535; -16: n_groups > 0 and out_cov NULL; -18: n_groups > 0 and n_max
 * outside 1 .. 128 (a group above the cap).  0 = ok.                                                          */
size_t lvae_predict_cov_workspace_size(int L, int M, int P, int T, int Nt);
int lvae_predict_cov_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P,
                         int T, const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                         const double* z, int Nt, const double* test_x, int n_groups, const int32_t* group_subject,
                         const int32_t* group_start, int n_max, const double* params0, const double* params1,
                         const double* noise, double eps, double* out, double* out_cov, int add_noise, int32_t* info,
                         void* workspace, void* stream);

/* Joint predictive covariance of each group of test rows under the exact-GP predictor (and, optionally, the mean),
 * fp64.  With K_l = k_l(x, x) + noise_l I = L_l L_l^T and V = L_l^-1 k_l(x, tx_g):
 *   Sigma_g = k_l(tx_g, tx_g) - V^T V   (+ noise_l on the diagonal when add_noise = 1)              [n_g, n_g]
 * The covariance between rows of different groups is not returned.  Arguments as lvae_predict_exact_var_f64 with,
 * in place of out_var / ld_var: the groups, group g = the test rows [group_start[g], group_start[g + 1]) -- n_groups
 * + 1 entries in HOST memory (the chunks are cut at group boundaries on the host), group_start[0] = 0,
 * group_start[n_groups] = nt, every group of 1 .. n_max rows, n_max in 1 .. 128; and out_cov [L, n_groups, n_max,
 * n_max] laid out, padded and symmetric as lvae_predict_cov_f64's.  Route: the factor (and mean) as
 * lvae_predict_exact_f64; then per chunk of whole groups with at most c = min(chunk, nt) test rows the panel
 * k(x, tx_chunk) [L, n, c] and lvae_trsm_f64 in place as lvae_predict_exact_var_f64; V^T V on the fp64 matrix cores
 * with the n prediction rows cut into slabs of 512 whose partial 16 x 16 tiles go to the workspace and are added in
 * slab order (no atomics): the bits depend on neither the grid nor the chunk.  n^2 nt + n sum n_g^2 flops per dim.
 * nt == 0 (then n_groups == 0): the factor runs (info is written), nothing else is touched.  workspace:
 * lvae_predict_exact_cov_workspace_size(n, nt, L, chunk) bytes (lvae_predict_exact_var_f64's
 * + 2048 L c ceil(n / 512); 0 as there), 256-B aligned.
 * Returns 0, LVAE_ERR_LAUNCH, or before any launch, in this order: -1 .. -16 as lvae_predict_exact_var_f64 (-5 also
 * for L > 65535); -17 (n_groups outside 0 .. 65535, or n_groups == 0 with nt > 0 or the reverse); with nt > 0: -18
 * (n_max outside 1 .. 128: a group above the cap); -19 (add_noise not 0 / 1); with nt > 0: -20 (chunk < n_max) -21
 * (group_start NULL) -22 (group_start does not cut 0 .. nt into groups of 1 .. n_max rows) -23 (out_cov NULL). */
size_t lvae_predict_exact_cov_workspace_size(int n, int nt, int L, int chunk);
int lvae_predict_exact_cov_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                               const double* params, const double* noise, const double* mu, int64_t ld_mu,
                               const double* tx, int64_t ldt, int nt, int n_groups, const int32_t* group_start,
                               int n_max, double* out_mean, int64_t ld_out, double* out_cov, int add_noise, int chunk,
                               int32_t* info, void* workspace, void* stream);

/* S joint draws of every group's rows from N(mean, Sigma_g + jitter I), fp64, groups and latent dims drawn
 * independently of each other:
 *   out[s, r_i, l] = mean[r_i, l] + sum_{j <= i} Lc[l, g, i, j] eps[s, r_j, l],   Lc Lc^T = cov[l, g] + jitter I
 * cov [L, n_groups, n_max, n_max] as lvae_predict_cov_f64 / lvae_predict_exact_cov_f64 write it (the padding
 * identity keeps a padded block positive definite); index [n_groups, n_max] int32 (device): r_i = index[g, i], the
 * row of mean / eps / out that holds the group's i-th row, or -1 on padding (a group's rows first, then its
 * padding); mean [Nt, L], eps [S, Nt, L] standard normal draws, out [S, Nt, L].  Every row 0 .. Nt - 1 must appear
 * in exactly one group: rows in no group are not written, and of that only Nt > n_groups n_max can be seen here (-4)
 * -- the caller checks the rest (lvae_amd.sample_trajectories does, before the call).  Route: one kernel copies cov
 * with the jitter on the diagonals into the workspace, lvae_potrf_f64 factors the L n_groups blocks in place
 * (info[l*n_groups + g] LAPACK-style: > 0 for a block that is not positive definite, whose draws are then
 * meaningless; the others are unaffected), one kernel forms the draws, each sum in the order of j.  n_groups == 0
 * (then Nt == 0): returns 0, nothing is touched; S == 0 or Nt == 0: the factors run (info is written), out is
 * untouched.  workspace: lvae_predict_sample_workspace_size(L, n_groups, n_max) bytes (8 (L G n_max^2 + L G), each
 * array rounded up to 256 B, G = max(n_groups, 1); 0 for L < 1, n_groups < 0 or n_max < 1), 256-B aligned.
 * Returns 0, LVAE_ERR_LAUNCH, or before any launch, in this order: -1 (L < 1) -2 (n_groups < 0 or L n_groups >
 * 65535) -3 (n_max outside 1 .. 128) -4 (Nt < 0 or Nt > n_groups n_max) -5 (S < 0); with n_groups > 0: -6 (cov NULL)
 * -7 (index NULL); with Nt > 0 and S > 0: -8 (mean NULL) -9 (eps NULL); -10 (jitter negative or NaN); with Nt > 0
 * and S > 0: -11 (out NULL); with n_groups > 0: -12 (info NULL); -13 (workspace NULL or misaligned).        */
size_t lvae_predict_sample_workspace_size(int L, int n_groups, int n_max);
int lvae_predict_sample_f64(int L, int n_groups, int n_max, int Nt, int S, const double* cov, const int32_t* index,
                            const double* mean, const double* eps, double jitter, double* out, int32_t* info,
                            void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------- */
/* The early stream (per device; optional).  The blocked Cholesky inverse (lvae_spd_inv_chol_f32,   */
/* lvae_kl_closed_factor_f32) can start the part of its triangular inverse that needs only the      */
/* first block columns while the factorisation's last passes, bound by their chain of pivot blocks, */
/* leave the GPU nearly idle -- on a second stream, which the CALLER lends: a process may have as   */
/* few as 4 hardware queues, and a stream more than that serialises with another one, so the        */
/* library creates none of its own for this.  Lend a stream that is idle while the factor runs and   */
/* outlives every later call on the current device (its work is ordered by events: forked from the  */
/* call's stream and joined before the call returns; a call under stream capture does not use it);  */
/* NULL withdraws it.  Results are bitwise the same with and without.  0 or LVAE_ERR_LAUNCH.        */
/* ---------------------------------------------------------------------------------------- */
int lvae_set_early_stream(void* stream);

/* ---------------------------------------------------------------------------------------- */
/* Phase timing (profiling aid; with the early stream the only process-wide state of the library).  When enabled, */
/* the composite entry points bracket their phases with hipEvents on the caller's stream;  */
/* lvae_prof_collect synchronises on them, ADDS each phase's elapsed ms into ms[phase],    */
/* the number of bracketed intervals into count[phase], and forgets them.                  */
/* ---------------------------------------------------------------------------------------- */
enum lvae_phase {
  LVAE_PH_GRAM = 0, LVAE_PH_POTRF = 1 /* potrf (or the whole sweep) */, LVAE_PH_POTRI = 2 /* trtri + lauum */, LVAE_PH_KL_REDUCE = 3, LVAE_PH_SYRK = 4,
  LVAE_PH_GRAM_BWD = 5, LVAE_PH_BWD_ELEM = 6, LVAE_PH_HENSMAN_FWD = 7, LVAE_PH_HENSMAN_BWD = 8,
  LVAE_PH_NATGRAD = 9, LVAE_PH_SWEEP_UPD = 10 /* the trailing rank-256 update launches (U2), nested in POTRF */,
  LVAE_PH_HB_SLAB = 11 /* the binned hyper-gradient route's slab pass (kl_hyper.hip), nested in GRAM_BWD */, LVAE_N_PHASES = 12
};
int lvae_prof_enable(int on);
int lvae_prof_collect(double* ms, int32_t* count, int n_phases);

/* library identification: "lvae_hip <version> gfx950" */
const char* lvae_version(void);

/* ---------------------------------------------------------------------------------------- */
/* Glue (glue.hip): the elementwise pieces around the GP and ConvVAE kernels, one launch each    */
/* instead of a chain of framework ops (the steps are launch-paced at small shares).            */
/* ---------------------------------------------------------------------------------------- */
/* ConvVAE.loss_function (VAE.py:144-162) on [B, d] fp32 recon / x / mask, log_vy [d]:
 *   mse[i] = sum_j m (r - x)^2 / (sum_j m, or 1 where that is 0),
 *   nll[i] = sum_j (m (r - x)^2 / (2 exp(log_vy_j)) + (log 2 pi + log_vy_j) / 2);  msum[i] saved for the
 * backward.  The backward takes d mse / d nll (element i at g[i * stride]; stride 0 broadcasts) and writes
 * d recon [B, d] and per-pixel partials of d log_vy, dlv_part [lvae_vae_loss_bwd_partials(B), d] (their
 * column sums are d log_vy).                                                                     */
int lvae_vae_loss_fwd_f32(const float* recon, const float* x, const float* mask, const float* log_vy, int B, int d,
                          float* mse, float* nll, float* msum, void* stream);
size_t lvae_vae_loss_bwd_partials(int B);
int lvae_vae_loss_bwd_f32(const float* recon, const float* x, const float* mask, const float* log_vy, const float* msum,
                          const float* g_mse, int64_t g_mse_stride, const float* g_nll, int64_t g_nll_stride, int B,
                          int d, float* d_recon, float* dlv_part, void* stream);
/* ConvVAE.sample_latent (VAE.py:132-136): z = mu + eps exp(log_var / 2), n fp32 elements; backward
 * d log_var = d z eps exp(log_var / 2) / 2 (d mu = d z).                                         */
int lvae_reparam_fwd_f32(const float* mu, const float* log_var, const float* eps, int64_t n, float* z, void* stream);
int lvae_reparam_bwd_f32(const float* gz, const float* log_var, const float* eps, int64_t n, float* g_log_var,
                         void* stream);
/* The kernels' positivity transform exp(m + softplus(raw - m)) (GP_model.py:31-144) of n_raw [L] fp64
 * parameter tensors into column cols[k] of the [L, P] fp64 matrix out (other columns 1; raws[k], mlogs[k]:
 * host arrays of device pointers, mlogs[k] -> the [1] floor m).  Backward: grad [n_raw, L] =
 * g[l, cols[k]] exp(m + softplus(t)) sigmoid(t), t = raw - m (g element (l, p) at g[l s0 + p s1]).       */
int lvae_param_pack_fwd_f64(int n_raw, int L, int P, const int* cols, const double* const* raws,
                            const double* const* mlogs, double* out, void* stream);
/* The Hensman step's loss terms (training.py:100-120) from the per-image mse / nll [B] (fp32) and the KL
 * bound kld [1] (fp64): rec = c sum mse, nl = c sum nll (fp32), kd = ks kld, net = nl + kd (use_nll) or
 * rec + w kd (fp64).  Backward: d/d mse_i, d/d nll_i (the same for every image, fp32) and d/d kld from the
 * gradients of net / rec / nl / kd (nullptr: zero).                                                   */
/* The ConvVAE's bias + ReLU around its library GEMMs and transposed conv (VAE.py:44-75) on [N, C, HW] fp32
 * (HW = 1: a Linear's [B, F] rows).  Forward: y = relu(y + bias[c]) in place.  Backward: g = gy [y > 0]
 * (relu != 0; y the forward's output; with relu = 0 g is not written: g = gy) and db[c] = sum over n, hw
 * of g (per 64-image chunk partials in workspace [lvae_act_bwd_workspace_size(N, C) bytes], then the
 * chunks in order).  Replaces PyTorch's threshold_backward + the bias reduction of nn.Linear /
 * nn.ConvTranspose2d's backward (VAE.py:62-75).                                                     */
int lvae_bias_relu_fwd_f32(float* y, const float* bias, int N, int C, int HW, void* stream);
size_t lvae_act_bwd_workspace_size(int N, int C);
int lvae_act_bwd_f32(const float* gy, const float* y, int N, int C, int HW, int relu, float* g, float* db,
                     void* workspace, void* stream);
int lvae_step_terms_fwd(const float* mse, const float* nll, int B, const double* kld, float c, double ks, double w,
                        int use_nll, float* rec, float* nl, double* net, double* kd, void* stream);
int lvae_step_terms_bwd(const double* g_net, const float* g_rec, const float* g_nl, const double* g_kd, float c,
                        double ks, double w, int use_nll, float* g_mse, float* g_nll, double* g_kld, void* stream);
int lvae_param_pack_bwd_f64(int n_raw, int L, int P, const int* cols, const double* const* raws,
                            const double* const* mlogs, const double* g, int64_t g_stride0, int64_t g_stride1,
                            double* grad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LVAE_HIP_H */
