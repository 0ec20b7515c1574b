// predict.hip -- GP posterior mean of the latents at test covariates, for subjects of varying
// length: utils.batch_predict_varying_T (utils.py:115-211), as used by MSE_test_GPapprox
// (model_test.py:85-143).  fp64 (same M x M / T x T systems as the Hensman bound).
//
// Prediction set: P subjects laid out [P, T] (T = longest subject; seg_len[p] valid rows, the
// rest padding), encoder means mu [P*T, L].  Per latent dim:
//   B_p = k1(x_p, x_p) + noise I,  iB = B^-1 (block diagonal),  H = K0zz + K0xz^T iB K0xz
//   mu~ = iB mu - iB K0xz H^-1 K0xz^T iB mu
//   Z(X*) = K0X*z K0zz^-1 K0xz^T mu~ + k1(X*, x[test subjects]) mu~[test subjects]
// H^-1 and K0zz^-1 are applied as explicit inverses followed by one residual refinement step each (the reference
// solves; the bare product is cond(.) ulps worse than that).
// The reference's per-subject Python loops become one batched pass (padding rows of K0xz zeroed,
// padding blocks of B set to I, padding rows of mu zeroed by the caller).  The k1 term is the
// reference's dense product over all prediction rows of the test subjects (include[p] = 1),
// evaluated in chunks of test rows.
//
// Both predictors also give the predictive variance of the latent functions, which the reference does not:
// lvae_predict_exact_var_f64 and lvae_predict_var_f64 below, their kernels and formulas in predict_var.hpp.
// lvae_predict_cov_f64 and lvae_predict_exact_cov_f64 form the joint covariance of each group of test rows from the
// same buffers, and lvae_predict_sample_f64 draws whole trajectories from it (kernels in predict_cov.hpp).
// lvae_predict_exact_comp_f64 and lvae_predict_comp_f64 split the two means by additive component of the kernel
// (both are linear in it): the same launches, then gram.hip's component-resolved cross-Gram x vector.
// lvae_predict_exact_comp_cov_f64 and lvae_predict_comp_cov_f64 add the joint posterior covariance of the components
// at each test row (kernels in predict_ccov.hpp).
#include "small.hpp"
#include "prof.hpp"
#include "predict_var.hpp"
#include "predict_cov.hpp"
#include "predict_ccov.hpp"

namespace lvae {
namespace {

constexpr int64_t kPredChunkElems = 1 << 24;  // k1(X*, x) chunk: <= 128 MiB of fp64

struct PWs {
  double *K0xz, *iBK, *K0zz, *Hm, *iK, *iH, *Bst, *iB, *iBmu, *t, *muT, *muTm, *w, *v, *a, *b, *rr, *K0Xz, *out1, *K1;
  double *ldK, *ldH, *ldB;
  int32_t* info;
  int64_t chunk_rows;
  size_t bytes;
  PWs(char* base, int L, int M, int P, int T, int Nt) {
    WsCarve c(base);
    const size_t NP = (size_t)P * T, LMM = (size_t)L * M * M, LTT = (size_t)L * P * T * T;
    K0xz = c.take(L * NP * M);
    iBK = c.take(L * NP * M);
    K0zz = c.take(LMM);
    Hm = c.take(LMM);
    iK = c.take(LMM);
    iH = c.take(LMM);
    Bst = c.take(LTT);
    iB = c.take(LTT);
    iBmu = c.take(L * NP);
    t = c.take(L * NP);
    muT = c.take(L * NP);
    muTm = c.take(L * NP);
    w = c.take((size_t)L * M);
    v = c.take((size_t)L * M);
    a = c.take((size_t)L * M);
    b = c.take((size_t)L * M);
    rr = c.take((size_t)L * M);
    K0Xz = c.take((size_t)L * Nt * M);
    out1 = c.take((size_t)L * Nt);
    int64_t rows = kPredChunkElems / ((int64_t)L * (int64_t)NP);
    if (rows < 1) rows = 1;
    if (rows > Nt) rows = Nt;
    chunk_rows = rows;
    K1 = c.take((size_t)L * rows * NP);
    ldK = c.take(L);
    ldH = c.take(L);
    ldB = c.take((size_t)L * P);
    info = (int32_t*)c.take((size_t)2 * L + (size_t)L * P);
    bytes = c.off;
  }
};

__device__ inline bool pv(const int32_t* __restrict__ seg, int p, int q) { return q < seg[p]; }

// padding: K0xz rows -> 0, B_p rows/cols -> I
__global__ void pr_mask_kernel(int L, int P, int T, int M, const int32_t* __restrict__ seg, double* __restrict__ K0xz,
                               double* __restrict__ Bst) {
  const int64_t NP = (int64_t)P * T, nxz = (int64_t)L * NP * M, TT = (int64_t)T * T, nst = (int64_t)L * P * TT;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < nxz) {
    const int64_t row = (e / M) % NP;
    if (!pv(seg, (int)(row / T), (int)(row % T))) K0xz[e] = 0.0;
  } else if (e < nxz + nst) {
    const int64_t f = e - nxz;
    const int p = (int)((f / TT) % P), i = (int)((f % TT) / T), j = (int)(f % T);
    if (!pv(seg, p, i) || !pv(seg, p, j)) Bst[f] = (i == j) ? 1.0 : 0.0;
  }
}

// muT = iBmu - corr ; muTm = muT on the included subjects' valid rows, 0 elsewhere
__global__ void pr_mutilde_kernel(int L, int P, int T, const int32_t* __restrict__ seg,
                                  const int32_t* __restrict__ include, const double* __restrict__ iBmu,
                                  const double* __restrict__ corr, double* __restrict__ muT, double* __restrict__ muTm) {
  const int64_t NP = (int64_t)P * T;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L * NP) return;
  const int64_t row = e % NP;
  const int p = (int)(row / T), q = (int)(row % T);
  const bool ok = pv(seg, p, q);
  const double v = ok ? iBmu[e] - corr[e] : 0.0;
  muT[e] = v;
  muTm[e] = (ok && include[p]) ? v : 0.0;
}

// K0zz += eps I ; Hm += K0zz
__global__ void pr_eye_add_kernel(int L, int M, double eps, double* __restrict__ K0zz, double* __restrict__ Hm) {
  const int64_t MM = (int64_t)M * M;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L * MM) return;
  const int i = (int)((e % MM) / M), j = (int)(e % M);
  const double k = K0zz[e] + (i == j ? eps : 0.0);
  K0zz[e] = k;
  Hm[e] += k;
}

// info[l]: first failing factorisation in the order K0zz (10000 + col), B_p (20000 + col), H (30000 + col); w holds
// the raw codes as [K0zz: L][H: L][B_p: L*P]
__global__ void pr_info_kernel(int L, int P, const int32_t* __restrict__ w, int32_t* __restrict__ info) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  int v = 0;
  if (w[l]) v = 10000 + w[l];
  for (int p = 0; p < P && !v; ++p)
    if (w[2 * L + l * P + p]) v = 20000 + w[2 * L + l * P + p];
  if (!v && w[L + l]) v = 30000 + w[L + l];
  info[l] = v;
}

// out[i][l] = out1[l][i]
__global__ void pr_out_kernel(int L, int Nt, const double* __restrict__ out1, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)L * Nt) return;
  const int i = (int)(e / L), l = (int)(e % L);
  out[e] = out1[(int64_t)l * Nt + i];
}

inline int nblk(int64_t n) { return cdiv(n, 256); }

// ---- exact-GP predictor (model_test.py:11-17 predict_gp, as MSE_test calls it, model_test.py:19-82) ----
// workspace of lvae_predict_exact_f64: K [L, n, n] (factored in place), the work vectors a, r [L, n], the factor's
// log-determinants, the solves' inverted diagonal blocks and the fused products' slab partials
struct EWs {
  double *K, *a, *r, *logdet;
  char *trsm, *mv;
  size_t bytes;
  EWs(char* base, int n, int nt, int L) {
    size_t off = 0;
    auto take = [&](size_t b) {
      char* p = base ? base + off : nullptr;
      off += align256(b);
      return p;
    };
    K = (double*)take((size_t)L * n * n * sizeof(double));
    a = (double*)take((size_t)L * n * sizeof(double));
    r = (double*)take((size_t)L * n * sizeof(double));
    logdet = (double*)take((size_t)L * sizeof(double));
    trsm = take(lvae_trsm_workspace_size(n, L));
    const size_t m0 = lvae_gram_matvec_workspace_size(n, n, L), m1 = lvae_gram_matvec_workspace_size(nt, n, L);
    mv = take(m0 > m1 ? m0 : m1);
    bytes = off;
  }
};

// a[l][i] = mu[i][l]
__global__ void pe_gather_kernel(int L, int n, const double* __restrict__ mu, int64_t ld_mu, double* __restrict__ a) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)L * n) return;
  const int64_t l = e / n, i = e % n;
  a[e] = mu[i * ld_mu + l];
}
// r[l][i] = mu[i][l] - r[l][i]   (r holds K a0 on entry)
__global__ void pe_resid_kernel(int L, int n, const double* __restrict__ mu, int64_t ld_mu, double* __restrict__ r) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)L * n) return;
  const int64_t l = e / n, i = e % n;
  r[e] = mu[i * ld_mu + l] - r[e];
}
// a += r
__global__ void pe_add_kernel(int64_t m, double* __restrict__ a, const double* __restrict__ r) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < m) a[e] += r[e];
}

// workspace of lvae_predict_var_f64 behind lvae_predict_f64's own (PWs): G [L, M, M], the test rows' subjects, and
// per latent dim the [T, Nt] matrices C, D and the [M, Nt] matrices E, K0zX*, Q, W, V and the residual R
struct VWs {
  double *Gm, *C, *D, *E, *KzX, *Qm, *W, *V, *R;
  int32_t* rs;
  size_t bytes;
  VWs(char* base, size_t off0, int L, int M, int T, int Nt) {
    WsCarve c(base ? base + off0 : nullptr);
    const size_t tn = (size_t)L * T * Nt, mn = (size_t)L * M * Nt;
    Gm = c.take((size_t)L * M * M);
    rs = (int32_t*)c.take(((size_t)Nt + 1) / 2);
    C = c.take(tn);
    D = c.take(tn);
    E = c.take(mn);
    KzX = c.take(mn);
    Qm = c.take(mn);
    W = c.take(mn);
    V = c.take(mn);
    R = c.take(mn);
    bytes = off0 + c.off;
  }
};

// workspace of lvae_predict_exact_var_f64 behind lvae_predict_exact_f64's own (EWs): the panel k(X, X*_chunk)
// [L, n, c], solved in place
inline size_t exact_var_panel_bytes(int n, int nt, int L, int chunk) {
  const int c = chunk < nt ? chunk : nt;
  return align256((size_t)L * n * (c > 0 ? c : 0) * sizeof(double));
}

// workspace of lvae_predict_exact_cov_f64 behind EWs and the panel: the slabs' partial tiles [L, c, nslab, 16, 16]
// (a chunk of c columns in whole groups of <= 128 rows holds at most c tiles on and below the diagonals)
inline int exact_cov_slabs(int n) { return cdiv(n, kCovSlab); }
inline size_t exact_cov_part_bytes(int n, int nt, int L, int chunk) {
  const int c = chunk < nt ? chunk : nt;
  return align256((size_t)L * (c > 0 ? c : 0) * exact_cov_slabs(n) * 256 * sizeof(double));
}

// workspace of lvae_predict_exact_comp_cov_f64 behind lvae_predict_exact_comp_f64's own: the component-resolved panel
// k_r(X, X*_chunk) [L, n, c R], solved in place, and the slabs' partial tiles [L, c, nslab, 16, 16] (one tile a row)
inline size_t exact_ccov_panel_bytes(int n, int nt, int L, int R, int chunk) {
  const int c = chunk < nt ? chunk : nt;
  return align256((size_t)L * n * (c > 0 ? c : 0) * R * sizeof(double));
}

// workspace of lvae_predict_sample_f64: the factors Lc [L, G, n_max, n_max] and their log-determinants [L G]
struct SWs {
  double *Lc, *logdet;
  size_t bytes;
  SWs(char* base, int L, int G, int n_max) {
    WsCarve c(base);
    Lc = c.take((size_t)L * G * n_max * n_max);
    logdet = c.take((size_t)L * G);
    bytes = c.off;
  }
};

}  // namespace

int gram_matvec_f64(const lvae_kernel_spec* spec, const double* x1, int64_t ld1, int n1, const double* x2, int64_t ld2,
                    int n2, int L, const double* params, const double* diag, const double* v, int64_t ld_v, int v_t,
                    double* out, int64_t ld_out, int o_t, void* workspace, hipStream_t st);
int gram_matvec_spec_ld(const lvae_kernel_spec* spec);
int gram_matvec_comp_f64(const lvae_kernel_spec* spec, const double* x1, int64_t ld1, int n1, const double* x2,
                         int64_t ld2, int64_t x2_stride_l, int n2, int L, const double* params, const double* v,
                         int64_t ld_v, int v_t, double* out, int64_t ld_out, int o_t, int64_t ostride_r,
                         void* workspace, hipStream_t st);
}  // namespace lvae

using namespace lvae;

// The launches of lvae_predict_f64 on the carved workspace w (arguments checked by the caller).  mean = false
// stops after the factorisations (the variance alone needs no mu~); Gm, when given, receives
// G = K0zx iB K0xz [L, M, M] before K0zz is added to it (H - K0zz would lose G's low bits).
static int predict_core(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P, int T,
                        const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                        const double* z, int Nt, const double* test_x, const double* params0, const double* params1,
                        const double* noise, double eps, double* out, bool mean, double* Gm, int32_t* info, PWs& w,
                        void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int NP = P * T;
  const int64_t MM = (int64_t)M * M, TT = (int64_t)T * T, NPM = (int64_t)NP * M;
  // Grams (utils.py:139-160): K0xz [L,NP,M], K0zz + eps I, K0X*z [L,Nt,M], B_p = k1(x_p, x_p) + noise I
  const lvae_xview xv{x, 0, 0, Q}, zv{z, 0, (int64_t)M * Q, Q}, xs{x, (int64_t)T * Q, 0, Q}, tv{test_x, 0, 0, Q};
  LVAE_TRY(lvae_gram_f64(spec0, xv, zv, 1, L, NP, M, params0, nullptr, w.K0xz, 0, NPM, M, stream));
  LVAE_TRY(lvae_gram_f64(spec0, zv, zv, 1, L, M, M, params0, nullptr, w.K0zz, 0, MM, M, stream));
  LVAE_TRY(lvae_gram_f64(spec1, xs, xs, P, L, T, T, params1, noise, w.Bst, TT, (int64_t)P * TT, T, stream));
  if (Nt > 0) LVAE_TRY(lvae_gram_f64(spec0, tv, zv, 1, L, Nt, M, params0, nullptr, w.K0Xz, 0, (int64_t)Nt * M, M, stream));
  pr_mask_kernel<<<nblk((int64_t)L * NPM + (int64_t)L * P * TT), 256, 0, st>>>(L, P, T, M, seg_len, w.K0xz, w.Bst);
  // iB (per subject), iB mu, iB K0xz
  LVAE_TRY(spd_inv_small_f64(T, L * P, w.Bst, TT, w.iB, TT, w.ldB, w.info + 2 * L, st));
  if (mean)
    LVAE_TRY(gemm_small_f64(0, 0, T, 1, T, 1.0, w.iB, T, (int64_t)P * TT, TT, mu, L, 1, (int64_t)T * L, 0.0, w.iBmu,
                            1, NP, T, L, P, st));
  LVAE_TRY(gemm_small_f64(0, 0, T, M, T, 1.0, w.iB, T, (int64_t)P * TT, TT, w.K0xz, M, NPM, (int64_t)T * M, 0.0, w.iBK,
                          M, NPM, (int64_t)T * M, L, P, st));
  // H = K0zz + eps I + K0xz^T iB K0xz  (utils.py:147,171);  K0zz += eps I
  LVAE_TRY(gemm_small_f64(1, 0, M, M, NP, 1.0, w.K0xz, M, NPM, 0, w.iBK, M, NPM, 0, 0.0, w.Hm, M, MM, 0, L, 1, st));
  if (Gm) LVAE_TRY(copy_words_async(Gm, w.Hm, (size_t)L * MM * sizeof(double), st));
  pr_eye_add_kernel<<<nblk((int64_t)L * MM), 256, 0, st>>>(L, M, eps, w.K0zz, w.Hm);
  LVAE_TRY(spd_inv_small2_f64(M, L, w.K0zz, MM, w.iK, MM, w.ldK, w.info, L, w.Hm, MM, w.iH, MM, w.ldH, w.info + L, st));
  if (!mean) {
    if (info) pr_info_kernel<<<nblk(L), 256, 0, st>>>(L, P, w.info, info);
    LVAE_CHECK_LAUNCH();
    return 0;
  }
  // mu~ = iB mu - iB K0xz H^-1 K0xz^T iB mu
  LVAE_TRY(gemm_small_f64(1, 0, M, 1, NP, 1.0, w.K0xz, M, NPM, 0, w.iBmu, 1, NP, 0, 0.0, w.w, 1, M, 0, L, 1, st));
  LVAE_TRY(gemm_small_f64(0, 0, M, 1, M, 1.0, w.iH, M, MM, 0, w.w, 1, M, 0, 0.0, w.v, 1, M, 0, L, 1, st));
  // one refinement step, v += H^-1 (w - H v): the product with the explicit inverse alone loses cond(H) ulps where
  // the reference's solve (utils.py:183) does not; rr = w again (the same GEMM), then rr -= H v
  LVAE_TRY(gemm_small_f64(1, 0, M, 1, NP, 1.0, w.K0xz, M, NPM, 0, w.iBmu, 1, NP, 0, 0.0, w.rr, 1, M, 0, L, 1, st));
  LVAE_TRY(gemm_small_f64(0, 0, M, 1, M, -1.0, w.Hm, M, MM, 0, w.v, 1, M, 0, 1.0, w.rr, 1, M, 0, L, 1, st));
  LVAE_TRY(gemm_small_f64(0, 0, M, 1, M, 1.0, w.iH, M, MM, 0, w.rr, 1, M, 0, 1.0, w.v, 1, M, 0, L, 1, st));
  LVAE_TRY(gemm_small_f64(0, 0, NP, 1, M, 1.0, w.iBK, M, NPM, 0, w.v, 1, M, 0, 0.0, w.t, 1, NP, 0, L, 1, st));
  pr_mutilde_kernel<<<nblk((int64_t)L * NP), 256, 0, st>>>(L, P, T, seg_len, include, w.iBmu, w.t, w.muT, w.muTm);
  if (Nt > 0) {
    // K0X*z K0zz^-1 K0xz^T mu~
    LVAE_TRY(gemm_small_f64(1, 0, M, 1, NP, 1.0, w.K0xz, M, NPM, 0, w.muT, 1, NP, 0, 0.0, w.a, 1, M, 0, L, 1, st));
    LVAE_TRY(gemm_small_f64(0, 0, M, 1, M, 1.0, w.iK, M, MM, 0, w.a, 1, M, 0, 0.0, w.b, 1, M, 0, L, 1, st));
    // the same refinement step for b = K0zz^-1 a (utils.py:190 solves)
    LVAE_TRY(gemm_small_f64(1, 0, M, 1, NP, 1.0, w.K0xz, M, NPM, 0, w.muT, 1, NP, 0, 0.0, w.rr, 1, M, 0, L, 1, st));
    LVAE_TRY(gemm_small_f64(0, 0, M, 1, M, -1.0, w.K0zz, M, MM, 0, w.b, 1, M, 0, 1.0, w.rr, 1, M, 0, L, 1, st));
    LVAE_TRY(gemm_small_f64(0, 0, M, 1, M, 1.0, w.iK, M, MM, 0, w.rr, 1, M, 0, 1.0, w.b, 1, M, 0, L, 1, st));
    LVAE_TRY(gemm_small_f64(0, 0, Nt, 1, M, 1.0, w.K0Xz, M, (int64_t)Nt * M, 0, w.b, 1, M, 0, 0.0, w.out1, 1, Nt, 0, L,
                            1, st));
    // + k1(X*, x) mu~[test subjects], chunked over test rows (utils.py:191-209)
    for (int r0 = 0; r0 < Nt; r0 += (int)w.chunk_rows) {
      const int nr = (int)((Nt - r0) < w.chunk_rows ? (Nt - r0) : w.chunk_rows);
      const lvae_xview tc{test_x + (int64_t)r0 * Q, 0, 0, Q};
      LVAE_TRY(lvae_gram_f64(spec1, tc, xv, 1, L, nr, NP, params1, nullptr, w.K1, 0, (int64_t)nr * NP, NP, stream));
      LVAE_TRY(gemm_small_f64(0, 0, nr, 1, NP, 1.0, w.K1, NP, (int64_t)nr * NP, 0, w.muTm, 1, NP, 0, 1.0,
                              w.out1 + r0, 1, Nt, 0, L, 1, st));
    }
    pr_out_kernel<<<nblk((int64_t)L * Nt), 256, 0, st>>>(L, Nt, w.out1, out);
  }
  if (info) pr_info_kernel<<<nblk(L), 256, 0, st>>>(L, P, w.info, info);
  LVAE_CHECK_LAUNCH();
  return 0;
}

// The launches of lvae_predict_exact_f64 on the carved workspace w (arguments checked by the caller): the factor
// of K into w.K and, when out is given, the mean.
static int exact_core(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L, const double* params,
                      const double* noise, const double* mu, int64_t ld_mu, const double* tx, int64_t ldt, int nt,
                      double* out, int64_t ld_out, int32_t* info, EWs& w, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int64_t nn = (int64_t)n * n;
  // K = k(x, x) + noise I, factored in place (info[l] > 0: dim l is not positive definite; its outputs are
  // then meaningless, every other dim's are unaffected)
  const lvae_xview xv{x, 0, 0, ldx};
  LVAE_TRY(lvae_gram_f64(spec, xv, xv, 1, L, n, n, params, noise, w.K, 0, nn, n, stream));
  LVAE_TRY(lvae_potrf_f64(n, L, w.K, n, nn, w.K, n, nn, w.logdet, info, stream));
  if (nt == 0 || !out) {
    LVAE_CHECK_LAUNCH();
    return 0;
  }
  // a0 = K^-1 mu, then one refinement step a = a0 + K^-1 (mu - K a0) with K a0 from the covariates again (K itself
  // is overwritten by its factor): the solve alone is cond(K) ulps from the reference's explicit-inverse product
  pe_gather_kernel<<<nblk((int64_t)L * n), 256, 0, st>>>(L, n, mu, ld_mu, w.a);
  LVAE_TRY(lvae_potrs_f64(n, 1, L, w.K, n, nn, w.a, 1, n, w.trsm, stream));
  LVAE_TRY(gram_matvec_f64(spec, x, ldx, n, x, ldx, n, L, params, noise, w.a, n, 1, w.r, n, 1, w.mv, st));
  pe_resid_kernel<<<nblk((int64_t)L * n), 256, 0, st>>>(L, n, mu, ld_mu, w.r);
  LVAE_TRY(lvae_potrs_f64(n, 1, L, w.K, n, nn, w.r, 1, n, w.trsm, stream));
  pe_add_kernel<<<nblk((int64_t)L * n), 256, 0, st>>>((int64_t)L * n, w.a, w.r);
  // Zpred = k(X*, x) a
  LVAE_TRY(gram_matvec_f64(spec, tx, ldt, nt, x, ldx, n, L, params, nullptr, w.a, n, 1, out, ld_out, 0, w.mv, st));
  LVAE_CHECK_LAUNCH();
  return 0;
}

// Q, W and V of the variance routes from K0zX* (v.KzX) and E, each [L, M, N] with the N columns on the workspaces w
// and v (after predict_core's launches); a column's results do not depend on its neighbours.
static int var_solves(int L, int M, int N, PWs& w, VWs& v, hipStream_t st) {
  const int Nt = N;
  const int64_t MM = (int64_t)M * M, MN = (int64_t)M * Nt;
  const size_t mn_bytes = (size_t)L * MN * sizeof(double);
  // Q = K0zz^-1 K0zX* with one refinement step Q += K0zz^-1 (K0zX* - K0zz Q), as the mean refines its two products
  // with explicit inverses: the bare product is cond(K0zz) ulps off, and q enters the variance three times in
  // terms that cancel.  With this step and the one for V below, an fp64 emulation of the route against the dense
  // oracle gives 5e-15 of the largest prior variance at M = 128, eps = 1e-3 (cond K0zz 5e5) where the bare
  // products give 1.5e-10; the tests' bound is 2e-12.
  LVAE_TRY(gemm_small_f64(0, 0, M, Nt, M, 1.0, w.iK, M, MM, 0, v.KzX, Nt, MN, 0, 0.0, v.Qm, Nt, MN, 0, L, 1, st));
  LVAE_TRY(copy_words_async(v.R, v.KzX, mn_bytes, st));
  LVAE_TRY(gemm_small_f64(0, 0, M, Nt, M, -1.0, w.K0zz, M, MM, 0, v.Qm, Nt, MN, 0, 1.0, v.R, Nt, MN, 0, L, 1, st));
  LVAE_TRY(gemm_small_f64(0, 0, M, Nt, M, 1.0, w.iK, M, MM, 0, v.R, Nt, MN, 0, 1.0, v.Qm, Nt, MN, 0, L, 1, st));
  // W = G Q + E;  V = H^-1 W with the same refinement step, V += H^-1 (W - H V) (cond(H) ulps otherwise)
  LVAE_TRY(copy_words_async(v.W, v.E, mn_bytes, st));
  LVAE_TRY(gemm_small_f64(0, 0, M, Nt, M, 1.0, v.Gm, M, MM, 0, v.Qm, Nt, MN, 0, 1.0, v.W, Nt, MN, 0, L, 1, st));
  LVAE_TRY(gemm_small_f64(0, 0, M, Nt, M, 1.0, w.iH, M, MM, 0, v.W, Nt, MN, 0, 0.0, v.V, Nt, MN, 0, L, 1, st));
  LVAE_TRY(copy_words_async(v.R, v.W, mn_bytes, st));
  LVAE_TRY(gemm_small_f64(0, 0, M, Nt, M, -1.0, w.Hm, M, MM, 0, v.V, Nt, MN, 0, 1.0, v.R, Nt, MN, 0, L, 1, st));
  LVAE_TRY(gemm_small_f64(0, 0, M, Nt, M, 1.0, w.iH, M, MM, 0, v.R, Nt, MN, 0, 1.0, v.V, Nt, MN, 0, L, 1, st));
  LVAE_CHECK_LAUNCH();
  return 0;
}

// The launches of lvae_predict_var_f64 up to its last kernel, on the carved workspaces w and v (arguments checked by
// the caller): lvae_predict_f64's own (and the mean when out is given), then C, D, E, K0zX*, Q, W and V [rows, Nt].
static int var_pipeline(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P, int T,
                        const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                        const double* z, int Nt, const double* test_x, int n_groups, const int32_t* group_subject,
                        const int32_t* group_start, const double* params0, const double* params1,
                        const double* noise, double eps, double* out, int32_t* info, PWs& w, VWs& v, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // the Grams, iB, K0zz^-1, H^-1 (and the mean) by lvae_predict_f64's own launches; G kept aside
  LVAE_TRY(predict_core(spec0, spec1, L, M, Q, P, T, seg_len, include, x, mu, z, Nt, test_x, params0, params1, noise,
                        eps, out, out != nullptr, v.Gm, info, w, stream));
  if (Nt == 0) return 0;
  const size_t mn_bytes = (size_t)L * M * Nt * sizeof(double);
  const int b1 = spec_bucket(spec1);
  const DevSpec d1 = to_dev(spec1);
  // c_i, d_i = iB_s c_i, e_i = K0zx_s d_i per subject group (rows of no group, or of an absent subject: 0)
  pv_rowsubj_kernel<<<nblk(Nt), 256, 0, st>>>(Nt, P, n_groups, group_subject, group_start, v.rs);
  if (b1 == 1)
    pv_c_kernel<8, 2><<<nblk((int64_t)L * T * Nt), 256, 0, st>>>(d1, L, T, Nt, Q, seg_len, v.rs, x, test_x, params1, v.C);
  else
    pv_c_kernel<16, 4><<<nblk((int64_t)L * T * Nt), 256, 0, st>>>(d1, L, T, Nt, Q, seg_len, v.rs, x, test_x, params1, v.C);
  LVAE_TRY(zero_async(v.D, (size_t)L * T * Nt * sizeof(double), st));
  LVAE_TRY(zero_async(v.E, mn_bytes, st));
  if (n_groups > 0)
    pv_group_kernel<<<dim3(Nt / kPvC + n_groups, L), 256, 0, st>>>(M, P, T, Nt, n_groups, 1, group_subject,
                                                                  group_start, v.C, w.iB, w.K0xz, v.D, v.E);
  // K0zX* [L, M, Nt] is its own Gram (test rows as columns); then Q, W and V
  const lvae_xview zv{z, 0, (int64_t)M * Q, Q}, tv{test_x, 0, 0, Q};
  LVAE_TRY(lvae_gram_f64(spec0, zv, tv, 1, L, M, Nt, params0, nullptr, v.KzX, 0, (int64_t)M * Nt, Nt, stream));
  return var_solves(L, M, Nt, w, v, st);
}

extern "C" {

size_t lvae_predict_workspace_size(int L, int M, int P, int T, int Nt) {
  return PWs(nullptr, L, M, P, T, Nt > 0 ? Nt : 1).bytes;
}

int lvae_predict_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P, int T,
                     const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                     const double* z, int Nt, const double* test_x, const double* params0, const double* params1,
                     const double* noise, double eps, double* out, int32_t* info, void* workspace, void* stream) {
  if (!spec0 || !spec1 || !spec_bucket(spec0) || !spec_bucket(spec1)) return -1;  // (before any launch)
  if (L < 1 || M < 1 || M > 128) return -3;
  if (P < 1 || T < 1 || T > 128 || Q < 1) return -6;
  if (!seg_len || !include) return -8;
  if (Nt < 0) return -13;
  if (!workspace || ((uintptr_t)workspace & 255)) return -20;
  PWs w((char*)workspace, L, M, P, T, Nt > 0 ? Nt : 1);
  return predict_core(spec0, spec1, L, M, Q, P, T, seg_len, include, x, mu, z, Nt, test_x, params0, params1, noise,
                      eps, out, true, nullptr, info, w, stream);
}

static size_t predict_comp_mv_bytes(int L, int M, int P, int T, int Nt, int n_comp0, int n_comp1) {
  const size_t m0 = lvae_gram_matvec_comp_workspace_size(Nt, M, L, n_comp0);
  const size_t m1 = lvae_gram_matvec_comp_workspace_size(Nt, P * T, L, n_comp1);
  return align256(m0 > m1 ? m0 : m1);
}

size_t lvae_predict_comp_workspace_size(int L, int M, int P, int T, int Nt, int n_comp0, int n_comp1) {
  return lvae_predict_workspace_size(L, M, P, T, Nt) + predict_comp_mv_bytes(L, M, P, T, Nt, n_comp0, n_comp1);
}

int lvae_predict_comp_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P,
                          int T, const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                          const double* z, int Nt, const double* test_x, const double* params0, const double* params1,
                          const double* noise, double eps, double* out, double* out_comp, int64_t ld_comp,
                          int64_t cstride_r, int32_t* info, void* workspace, void* stream) {
  if (!spec0 || !spec1 || !spec_bucket(spec0) || !spec_bucket(spec1)) return -1;  // (before any launch)
  const int ld0 = gram_matvec_spec_ld(spec0), ld1 = gram_matvec_spec_ld(spec1);
  if (ld0 < 1 || ld1 < 1) return -1;  // (a factor dim outside 0 .. 31: the fused product does not take it)
  if (L < 1 || M < 1 || M > 128) return -3;
  if (P < 1 || T < 1 || T > 128 || Q < 1 || Q < ld0 || Q < ld1) return -6;
  if (!seg_len || !include) return -8;
  if (Nt < 0) return -13;
  if (!workspace || ((uintptr_t)workspace & 255)) return -20;
  if (Nt > 0 && !out_comp) return -21;
  if (Nt > 0 && ld_comp < L) return -22;
  if (Nt > 0 && spec0->n_comp + spec1->n_comp > 1 && cstride_r < (int64_t)Nt * ld_comp) return -23;
  PWs w((char*)workspace, L, M, P, T, Nt > 0 ? Nt : 1);
  // the mean by lvae_predict_f64's own launches (its dense chunked K1 route included), then per component
  // k0_r(X*, z_l) b_l (blocks 0 .. R0 - 1) and k1_r(X*, x) mu~m_l (blocks R0 .. R0 + R1 - 1) on the b and mu~m they
  // leave in the workspace; mu~m is 0 on padding rows and on subjects outside the test set
  LVAE_TRY(predict_core(spec0, spec1, L, M, Q, P, T, seg_len, include, x, mu, z, Nt, test_x, params0, params1, noise,
                        eps, out, true, nullptr, info, w, stream));
  if (Nt == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  void* mv = (char*)workspace + align256(w.bytes);
  LVAE_TRY(gram_matvec_comp_f64(spec0, test_x, Q, Nt, z, Q, (int64_t)M * Q, M, L, params0, w.b, M, 1, out_comp, ld_comp,
                                0, cstride_r, mv, st));
  return gram_matvec_comp_f64(spec1, test_x, Q, Nt, x, Q, 0, P * T, L, params1, w.muTm, (int64_t)P * T, 1,
                              out_comp + (int64_t)spec0->n_comp * cstride_r, ld_comp, 0, cstride_r, mv, st);
}

size_t lvae_predict_exact_workspace_size(int n, int nt, int L) {
  if (n < 1 || nt < 0 || L < 1) return 0;
  return EWs(nullptr, n, nt, L).bytes;
}

int lvae_predict_exact_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                           const double* params, const double* noise, const double* mu, int64_t ld_mu,
                           const double* tx, int64_t ldt, int nt, double* out, int64_t ld_out, int32_t* info,
                           void* workspace, void* stream) {
  const int ld_min = spec ? gram_matvec_spec_ld(spec) : 0;
  if (ld_min < 1 || ld_min > 32) return -1;  // (before any launch)
  if (!x) return -2;
  if (ldx < ld_min) return -3;
  if (n < 1) return -4;
  if (L < 1) return -5;
  if (!params) return -6;
  if (!noise) return -7;
  if (!mu) return -8;
  if (ld_mu < L) return -9;
  if (nt < 0) return -12;
  if (nt > 0 && !tx) return -10;
  if (nt > 0 && ldt < ld_min) return -11;
  if (nt > 0 && !out) return -13;
  if (nt > 0 && ld_out < L) return -14;
  if (!info) return -15;
  if (!workspace || ((uintptr_t)workspace & 255)) return -16;
  EWs w((char*)workspace, n, nt, L);
  return exact_core(spec, x, ldx, n, L, params, noise, mu, ld_mu, tx, ldt, nt, out, ld_out, info, w, stream);
}

size_t lvae_predict_exact_comp_workspace_size(int n, int nt, int L, int n_comp) {
  if (n < 1 || nt < 0 || L < 1 || n_comp < 1) return 0;
  return EWs(nullptr, n, nt, L).bytes + align256(lvae_gram_matvec_comp_workspace_size(nt, n, L, n_comp));
}

int lvae_predict_exact_comp_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                                const double* params, const double* noise, const double* mu, int64_t ld_mu,
                                const double* tx, int64_t ldt, int nt, double* out, int64_t ld_out, double* out_comp,
                                int64_t ld_comp, int64_t cstride_r, int32_t* info, void* workspace, void* stream) {
  const int ld_min = spec ? gram_matvec_spec_ld(spec) : 0;
  if (ld_min < 1 || ld_min > 32) return -1;  // (before any launch)
  if (!x) return -2;
  if (ldx < ld_min) return -3;
  if (n < 1) return -4;
  if (L < 1) return -5;
  if (!params) return -6;
  if (!noise) return -7;
  if (!mu) return -8;
  if (ld_mu < L) return -9;
  if (nt < 0) return -12;
  if (nt > 0 && !tx) return -10;
  if (nt > 0 && ldt < ld_min) return -11;
  if (nt > 0 && !out) return -13;
  if (nt > 0 && ld_out < L) return -14;
  if (!info) return -15;
  if (!workspace || ((uintptr_t)workspace & 255)) return -16;
  if (nt > 0 && !out_comp) return -17;
  if (nt > 0 && ld_comp < L) return -18;
  if (nt > 0 && spec->n_comp > 1 && cstride_r < (int64_t)nt * ld_comp) return -19;
  EWs w((char*)workspace, n, nt, L);
  // the factor and the mean by lvae_predict_exact_f64's own launches, then k_r(X*, x) a per component r on the
  // refined a they leave in the workspace
  LVAE_TRY(exact_core(spec, x, ldx, n, L, params, noise, mu, ld_mu, tx, ldt, nt, out, ld_out, info, w, stream));
  if (nt == 0) return 0;
  return gram_matvec_comp_f64(spec, tx, ldt, nt, x, ldx, 0, n, L, params, w.a, n, 1, out_comp, ld_comp, 0, cstride_r,
                              (char*)workspace + w.bytes, (hipStream_t)stream);
}

size_t lvae_predict_exact_comp_cov_workspace_size(int n, int nt, int L, int n_comp, int chunk) {
  if (n < 1 || nt < 0 || L < 1 || n_comp < 1 || n_comp > LVAE_MAX_COMP || (nt > 0 && chunk < 1)) return 0;
  return lvae_predict_exact_comp_workspace_size(n, nt, L, n_comp) + exact_ccov_panel_bytes(n, nt, L, n_comp, chunk) +
         exact_cov_part_bytes(n, nt, L, chunk);
}

int lvae_predict_exact_comp_cov_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                                    const double* params, const double* noise, const double* mu, int64_t ld_mu,
                                    const double* tx, int64_t ldt, int nt, double* out, int64_t ld_out,
                                    double* out_comp, int64_t ld_comp, int64_t cstride_r, int chunk, double* out_ccov,
                                    int32_t* info, void* workspace, void* stream) {
  const int ld_min = spec ? gram_matvec_spec_ld(spec) : 0;
  if (ld_min < 1 || ld_min > 32 || spec->n_comp < 1) return -1;  // (before any launch)
  if (!x) return -2;
  if (ldx < ld_min) return -3;
  if (n < 1) return -4;
  if (L < 1 || L > 65535) return -5;
  if (!params) return -6;
  if (!noise) return -7;
  if (out && !mu) return -8;
  if (out && ld_mu < L) return -9;
  if (nt < 0) return -12;
  if (nt > 0 && !tx) return -10;
  if (nt > 0 && ldt < ld_min) return -11;
  if (nt > 0 && out_comp && !out) return -13;
  if (out && ld_out < L) return -14;
  if (!info) return -15;
  if (!workspace || ((uintptr_t)workspace & 255)) return -16;
  if (nt > 0 && out_comp && ld_comp < L) return -18;
  if (nt > 0 && out_comp && spec->n_comp > 1 && cstride_r < (int64_t)nt * ld_comp) return -19;
  if (nt > 0 && chunk < 1) return -20;
  if (nt > 0 && !out_ccov) return -21;
  hipStream_t st = (hipStream_t)stream;
  const int R = spec->n_comp;
  EWs w((char*)workspace, n, nt, L);
  char* mv = (char*)workspace + w.bytes;
  double* panel = (double*)((char*)workspace + lvae_predict_exact_comp_workspace_size(n, nt, L, R));
  double* part = (double*)((char*)panel + exact_ccov_panel_bytes(n, nt, L, R, chunk));
  // the factor of K, and when wanted the mean and its split, by lvae_predict_exact_comp_f64's own launches
  LVAE_TRY(exact_core(spec, x, ldx, n, L, params, noise, mu, ld_mu, tx, ldt, nt, out, ld_out, info, w, stream));
  if (nt == 0) return 0;
  if (out && out_comp)
    LVAE_TRY(gram_matvec_comp_f64(spec, tx, ldt, nt, x, ldx, 0, n, L, params, w.a, n, 1, out_comp, ld_comp, 0,
                                  cstride_r, mv, st));
  // c test rows at a time: the component-resolved panel k_r(X, X*_chunk) [L, n, c R] (column t R + r), one
  // triangular solve in place on its c R columns, then per row the slabs' partial tiles of V^T V and their sum in
  // slab order under the components' prior variances.  A column's solve does not depend on its neighbours and a
  // tile's slabs depend on n alone, so the bits do not depend on the chunk.
  const int c = chunk < nt ? chunk : nt, nslab = exact_cov_slabs(n), bucket = spec_bucket(spec);
  const DevSpec ds = to_dev(spec);
  const int64_t ldp = (int64_t)c * R;
  for (int c0 = 0; c0 < nt; c0 += c) {
    const int nr = nt - c0 < c ? nt - c0 : c;
    const double* tc = tx + (int64_t)c0 * ldt;
    const int pb = nblk((int64_t)L * n * nr);
    if (bucket == 1)
      pcc_panel_kernel<2><<<pb, 256, 0, st>>>(ds, L, n, nr, x, ldx, tc, ldt, params, panel, ldp);
    else
      pcc_panel_kernel<4><<<pb, 256, 0, st>>>(ds, L, n, nr, x, ldx, tc, ldt, params, panel, ldp);
    LVAE_TRY(lvae_trsm_f64(0, n, nr * R, L, w.K, n, (int64_t)n * n, panel, ldp, (int64_t)n * ldp, w.trsm, stream));
    pcc_partial_kernel<<<dim3(nr, nslab, L), 64, 0, st>>>(n, R, panel, ldp, c, part);
    if (bucket == 1)
      pcc_reduce_kernel<2><<<dim3(nr, L), 256, 0, st>>>(ds, nslab, c, part, tc, ldt, params, c0, nt, out_ccov);
    else
      pcc_reduce_kernel<4><<<dim3(nr, L), 256, 0, st>>>(ds, nslab, c, part, tc, ldt, params, c0, nt, out_ccov);
  }
  LVAE_CHECK_LAUNCH();
  return 0;
}

size_t lvae_predict_exact_var_workspace_size(int n, int nt, int L, int chunk) {
  if (n < 1 || nt < 0 || L < 1 || (nt > 0 && chunk < 1)) return 0;
  return EWs(nullptr, n, nt, L).bytes + exact_var_panel_bytes(n, nt, L, chunk);
}

int lvae_predict_exact_var_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                               const double* params, const double* noise, const double* mu, int64_t ld_mu,
                               const double* tx, int64_t ldt, int nt, double* out_mean, int64_t ld_out,
                               double* out_var, int64_t ld_var, int add_noise, int chunk, int32_t* info,
                               void* workspace, void* stream) {
  const int ld_min = spec ? gram_matvec_spec_ld(spec) : 0;
  if (ld_min < 1 || ld_min > 32) return -1;  // (before any launch)
  if (!x) return -2;
  if (ldx < ld_min) return -3;
  if (n < 1) return -4;
  if (L < 1) return -5;
  if (!params) return -6;
  if (!noise) return -7;
  if (out_mean && !mu) return -8;
  if (out_mean && ld_mu < L) return -9;
  if (nt < 0) return -12;
  if (nt > 0 && !tx) return -10;
  if (nt > 0 && ldt < ld_min) return -11;
  if (out_mean && ld_out < L) return -14;
  if (!info) return -15;
  if (!workspace || ((uintptr_t)workspace & 255)) return -16;
  if (nt > 0 && !out_var) return -17;
  if (nt > 0 && ld_var < L) return -18;
  if (add_noise != 0 && add_noise != 1) return -19;
  if (nt > 0 && chunk < 1) return -20;
  hipStream_t st = (hipStream_t)stream;
  EWs w((char*)workspace, n, nt, L);
  double* panel = (double*)((char*)workspace + w.bytes);
  // the factor of K (and the mean, by lvae_predict_exact_f64's own launches)
  LVAE_TRY(exact_core(spec, x, ldx, n, L, params, noise, mu, ld_mu, tx, ldt, nt, out_mean, ld_out, info, w, stream));
  if (nt == 0) return 0;
  // var = k(x*, x*) - |L^-1 k(X, x*)|^2, c test rows at a time: the panel k(X, X*_chunk) [L, n, c], one
  // triangular solve in place, then the columns' sums of squares.  A column's solve and sum do not depend on its
  // neighbours, so the bits do not depend on the chunk.
  const int c = chunk < nt ? chunk : nt;
  const int bucket = spec_bucket(spec);
  const DevSpec ds = to_dev(spec);
  const lvae_xview xv{x, 0, 0, ldx};
  for (int c0 = 0; c0 < nt; c0 += c) {
    const int nr = nt - c0 < c ? nt - c0 : c;
    const double* tc = tx + (int64_t)c0 * ldt;
    const lvae_xview tv{tc, 0, 0, ldt};
    LVAE_TRY(lvae_gram_f64(spec, xv, tv, 1, L, n, nr, params, nullptr, panel, 0, (int64_t)n * c, c, stream));
    LVAE_TRY(lvae_trsm_f64(0, n, nr, L, w.K, n, (int64_t)n * n, panel, c, (int64_t)n * c, w.trsm, stream));
    const dim3 grid(cdiv(nr, 64), L);
    double* vo = out_var + (int64_t)c0 * ld_var;
    if (bucket == 1)
      pe_var_kernel<8, 2><<<grid, 256, 0, st>>>(ds, n, nr, panel, c, tc, ldt, params, noise, add_noise, vo, ld_var);
    else
      pe_var_kernel<16, 4><<<grid, 256, 0, st>>>(ds, n, nr, panel, c, tc, ldt, params, noise, add_noise, vo, ld_var);
  }
  LVAE_CHECK_LAUNCH();
  return 0;
}

size_t lvae_predict_var_workspace_size(int L, int M, int P, int T, int Nt) {
  const int nt1 = Nt > 0 ? Nt : 1;
  return VWs(nullptr, PWs(nullptr, L, M, P, T, nt1).bytes, L, M, T, nt1).bytes;
}

int lvae_predict_var_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P,
                         int T, const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                         const double* z, int Nt, const double* test_x, int n_groups, const int32_t* group_subject,
                         const int32_t* group_start, const double* params0, const double* params1,
                         const double* noise, double eps, double* out, double* out_var, int add_noise, int32_t* info,
                         void* workspace, void* stream) {
  if (!spec0 || !spec1 || !spec_bucket(spec0) || !spec_bucket(spec1)) return -1;  // (before any launch)
  if (L < 1 || M < 1 || M > 128) return -3;
  if (P < 1 || T < 1 || T > 128 || Q < 1) return -6;
  if (!seg_len || !include) return -8;
  if (out && !mu) return -9;
  if (!x || !z) return -10;
  if (!params0 || !params1 || !noise) return -11;
  if (Nt < 0) return -13;
  if (Nt > 0 && !test_x) return -12;
  if (n_groups < 0) return -14;
  if (n_groups > 0 && (!group_subject || !group_start)) return -15;
  if (Nt > 0 && !out_var) return -16;
  if (add_noise != 0 && add_noise != 1) return -17;
  if (!workspace || ((uintptr_t)workspace & 255)) return -20;
  hipStream_t st = (hipStream_t)stream;
  const int nt1 = Nt > 0 ? Nt : 1;
  PWs w((char*)workspace, L, M, P, T, nt1);
  VWs v((char*)workspace, w.bytes, L, M, T, nt1);
  LVAE_TRY(var_pipeline(spec0, spec1, L, M, Q, P, T, seg_len, include, x, mu, z, Nt, test_x, n_groups, group_subject,
                        group_start, params0, params1, noise, eps, out, info, w, v, stream));
  if (Nt == 0) return 0;
  const int b1 = spec_bucket(spec1);
  const DevSpec d1 = to_dev(spec1);
  if (b1 == 1)
    pv_var_kernel<8, 2><<<nblk((int64_t)L * Nt), 256, 0, st>>>(d1, L, M, T, Nt, Q, v.KzX, v.Qm, v.W, v.E, v.V, v.C, v.D,
                                                               test_x, params1, noise, add_noise, out_var);
  else
    pv_var_kernel<16, 4><<<nblk((int64_t)L * Nt), 256, 0, st>>>(d1, L, M, T, Nt, Q, v.KzX, v.Qm, v.W, v.E, v.V, v.C, v.D,
                                                                test_x, params1, noise, add_noise, out_var);
  LVAE_CHECK_LAUNCH();
  return 0;
}

size_t lvae_predict_comp_cov_workspace_size(int L, int M, int P, int T, int Nt, int n_comp0, int n_comp1) {
  const int64_t R = (int64_t)n_comp0 + n_comp1;
  if (L < 1 || M < 1 || M > 128 || P < 1 || T < 1 || T > 128 || Nt < 0 || n_comp0 < 1 || n_comp1 < 1 ||
      n_comp0 > LVAE_MAX_COMP || n_comp1 > LVAE_MAX_COMP || Nt * R > INT32_MAX)
    return 0;
  return lvae_predict_var_workspace_size(L, M, P, T, (int)(Nt * R)) +
         predict_comp_mv_bytes(L, M, P, T, Nt, n_comp0, n_comp1);
}

int lvae_predict_comp_cov_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P,
                              int T, const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                              const double* z, int Nt, const double* test_x, int n_groups,
                              const int32_t* group_subject, const int32_t* group_start, const double* params0,
                              const double* params1, const double* noise, double eps, double* out, double* out_comp,
                              int64_t ld_comp, int64_t cstride_r, double* out_ccov, int32_t* info, void* workspace,
                              void* stream) {
  if (!spec0 || !spec1 || !spec_bucket(spec0) || !spec_bucket(spec1)) return -1;  // (before any launch)
  const int ld0 = gram_matvec_spec_ld(spec0), ld1 = gram_matvec_spec_ld(spec1);
  if (ld0 < 1 || ld1 < 1 || spec0->n_comp < 1 || spec1->n_comp < 1) return -1;
  if (L < 1 || L > 65535 || M < 1 || M > 128) return -3;
  if (P < 1 || T < 1 || T > 128 || Q < 1 || Q < ld0 || Q < ld1) return -6;
  if (!seg_len || !include) return -8;
  if (out && !mu) return -9;
  if (!x || !z) return -10;
  if (!params0 || !params1 || !noise) return -11;
  const int R0 = spec0->n_comp, R1 = spec1->n_comp, R = R0 + R1;
  if (Nt < 0 || (int64_t)Nt * R > INT32_MAX) return -13;
  if (Nt > 0 && !test_x) return -12;
  if (n_groups < 0) return -14;
  if (n_groups > 0 && (!group_subject || !group_start)) return -15;
  if (!workspace || ((uintptr_t)workspace & 255)) return -20;
  if (Nt > 0 && out_comp && !out) return -21;
  if (Nt > 0 && out_comp && ld_comp < L) return -22;
  if (Nt > 0 && out_comp && cstride_r < (int64_t)Nt * ld_comp) return -23;
  if (Nt > 0 && !out_ccov) return -24;
  hipStream_t st = (hipStream_t)stream;
  const int Nc = Nt * R, nc1 = Nc > 0 ? Nc : 1;  // one column per (test row, component)
  PWs w((char*)workspace, L, M, P, T, nc1);
  VWs v((char*)workspace, w.bytes, L, M, T, nc1);
  void* mv = (char*)workspace + v.bytes;
  // the Grams, iB, K0zz^-1, H^-1 and, when wanted, the mean by lvae_predict_f64's own launches (a workspace carved
  // for Nt R rows leaves them as they are); G kept aside; then the mean's split as lvae_predict_comp_f64
  LVAE_TRY(predict_core(spec0, spec1, L, M, Q, P, T, seg_len, include, x, mu, z, Nt, test_x, params0, params1, noise,
                        eps, out, out != nullptr, v.Gm, info, w, stream));
  if (Nt == 0) return 0;
  if (out && out_comp) {
    LVAE_TRY(gram_matvec_comp_f64(spec0, test_x, Q, Nt, z, Q, (int64_t)M * Q, M, L, params0, w.b, M, 1, out_comp,
                                  ld_comp, 0, cstride_r, mv, st));
    LVAE_TRY(gram_matvec_comp_f64(spec1, test_x, Q, Nt, x, Q, 0, P * T, L, params1, w.muTm, (int64_t)P * T, 1,
                                  out_comp + (int64_t)R0 * cstride_r, ld_comp, 0, cstride_r, mv, st));
  }
  // the columns' K0zX* and C through the specs, D and E per subject group (group g: the columns
  // [R group_start[g], R group_start[g + 1])), Q, W and V by the variance route's own launches, then the blocks
  const DevSpec d0 = to_dev(spec0), d1 = to_dev(spec1);
  pv_rowsubj_kernel<<<nblk(Nt), 256, 0, st>>>(Nt, P, n_groups, group_subject, group_start, v.rs);
  if (spec_bucket(spec0) == 1)
    pcc_kzx_kernel<2><<<nblk((int64_t)L * M * Nt), 256, 0, st>>>(d0, L, M, Nt, Q, R, z, test_x, params0, v.KzX);
  else
    pcc_kzx_kernel<4><<<nblk((int64_t)L * M * Nt), 256, 0, st>>>(d0, L, M, Nt, Q, R, z, test_x, params0, v.KzX);
  if (spec_bucket(spec1) == 1)
    pcc_c_kernel<2><<<nblk((int64_t)L * T * Nt), 256, 0, st>>>(d1, L, T, Nt, Q, R0, seg_len, v.rs, x, test_x, params1,
                                                               v.C);
  else
    pcc_c_kernel<4><<<nblk((int64_t)L * T * Nt), 256, 0, st>>>(d1, L, T, Nt, Q, R0, seg_len, v.rs, x, test_x, params1,
                                                               v.C);
  LVAE_TRY(zero_async(v.D, (size_t)L * T * Nc * sizeof(double), st));
  LVAE_TRY(zero_async(v.E, (size_t)L * M * Nc * sizeof(double), st));
  if (n_groups > 0)
    pv_group_kernel<<<dim3(Nc / kPvC + n_groups, L), 256, 0, st>>>(M, P, T, Nc, n_groups, R, group_subject,
                                                                  group_start, v.C, w.iB, w.K0xz, v.D, v.E);
  LVAE_TRY(var_solves(L, M, Nc, w, v, st));
  const dim3 grid((unsigned)Nt * cov_tiles(R), L);
  if (spec_bucket(spec1) == 1)
    pcc_ind_kernel<2><<<grid, 64, 0, st>>>(d1, M, T, Nt, Q, R0, v.KzX, v.Qm, v.W, v.E, v.V, v.C, v.D, test_x, params1,
                                           out_ccov);
  else
    pcc_ind_kernel<4><<<grid, 64, 0, st>>>(d1, M, T, Nt, Q, R0, v.KzX, v.Qm, v.W, v.E, v.V, v.C, v.D, test_x, params1,
                                           out_ccov);
  LVAE_CHECK_LAUNCH();
  return 0;
}

size_t lvae_predict_cov_workspace_size(int L, int M, int P, int T, int Nt) {
  return lvae_predict_var_workspace_size(L, M, P, T, Nt);
}

int lvae_predict_cov_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P,
                         int T, const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                         const double* z, int Nt, const double* test_x, int n_groups, const int32_t* group_subject,
                         const int32_t* group_start, int n_max, const double* params0, const double* params1,
                         const double* noise, double eps, double* out, double* out_cov, int add_noise, int32_t* info,
                         void* workspace, void* stream) {
  if (!spec0 || !spec1 || !spec_bucket(spec0) || !spec_bucket(spec1)) return -1;  // (before any launch)
  if (L < 1 || L > 65535 || M < 1 || M > 128) return -3;
  if (P < 1 || T < 1 || T > 128 || Q < 1) return -6;
  if (!seg_len || !include) return -8;
  if (out && !mu) return -9;
  if (!x || !z) return -10;
  if (!params0 || !params1 || !noise) return -11;
  if (Nt < 0) return -13;
  if (Nt > 0 && !test_x) return -12;
  if (n_groups < 0 || n_groups > 65535) return -14;
  if (n_groups > 0 && (!group_subject || !group_start)) return -15;
  if (n_groups > 0 && !out_cov) return -16;
  if (add_noise != 0 && add_noise != 1) return -17;
  if (n_groups > 0 && (n_max < 1 || n_max > kPvT)) return -18;
  if (!workspace || ((uintptr_t)workspace & 255)) return -20;
  hipStream_t st = (hipStream_t)stream;
  const int nt1 = Nt > 0 ? Nt : 1;
  PWs w((char*)workspace, L, M, P, T, nt1);
  VWs v((char*)workspace, w.bytes, L, M, T, nt1);
  LVAE_TRY(var_pipeline(spec0, spec1, L, M, Q, P, T, seg_len, include, x, mu, z, Nt, test_x, n_groups, group_subject,
                        group_start, params0, params1, noise, eps, out, info, w, v, stream));
  if (Nt == 0 || n_groups == 0) return 0;
  const int64_t nb = (int64_t)L * n_groups;
  pc_eye_kernel<<<nblk(nb * n_max * n_max), 256, 0, st>>>(nb, n_max, out_cov);
  const DevSpec d1 = to_dev(spec1);
  const dim3 grid(cov_tiles(n_max), n_groups, L);
  if (spec_bucket(spec1) == 1)
    pc_cov_kernel<8, 2><<<grid, 64, 0, st>>>(d1, M, T, Nt, Q, n_max, group_start, v.KzX, v.Qm, v.W, v.E, v.V, v.C, v.D,
                                             test_x, params1, noise, add_noise, out_cov);
  else
    pc_cov_kernel<16, 4><<<grid, 64, 0, st>>>(d1, M, T, Nt, Q, n_max, group_start, v.KzX, v.Qm, v.W, v.E, v.V, v.C, v.D,
                                              test_x, params1, noise, add_noise, out_cov);
  LVAE_CHECK_LAUNCH();
  return 0;
}

size_t lvae_predict_exact_cov_workspace_size(int n, int nt, int L, int chunk) {
  if (n < 1 || nt < 0 || L < 1 || (nt > 0 && chunk < 1)) return 0;
  return EWs(nullptr, n, nt, L).bytes + exact_var_panel_bytes(n, nt, L, chunk) + exact_cov_part_bytes(n, nt, L, chunk);
}

int lvae_predict_exact_cov_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                               const double* params, const double* noise, const double* mu, int64_t ld_mu,
                               const double* tx, int64_t ldt, int nt, int n_groups, const int32_t* group_start,
                               int n_max, double* out_mean, int64_t ld_out, double* out_cov, int add_noise, int chunk,
                               int32_t* info, void* workspace, void* stream) {
  const int ld_min = spec ? gram_matvec_spec_ld(spec) : 0;
  if (ld_min < 1 || ld_min > 32) return -1;  // (before any launch)
  if (!x) return -2;
  if (ldx < ld_min) return -3;
  if (n < 1) return -4;
  if (L < 1 || L > 65535) return -5;
  if (!params) return -6;
  if (!noise) return -7;
  if (out_mean && !mu) return -8;
  if (out_mean && ld_mu < L) return -9;
  if (nt < 0) return -12;
  if (nt > 0 && !tx) return -10;
  if (nt > 0 && ldt < ld_min) return -11;
  if (out_mean && ld_out < L) return -14;
  if (!info) return -15;
  if (!workspace || ((uintptr_t)workspace & 255)) return -16;
  if (n_groups < 0 || n_groups > 65535 || (n_groups == 0) != (nt == 0)) return -17;
  if (nt > 0 && (n_max < 1 || n_max > kPvT)) return -18;
  if (add_noise != 0 && add_noise != 1) return -19;
  if (nt > 0 && chunk < n_max) return -20;
  if (nt > 0 && !group_start) return -21;
  if (nt > 0) {
    if (group_start[0] != 0 || group_start[n_groups] != nt) return -22;
    for (int g = 0; g < n_groups; ++g) {
      const int64_t len = (int64_t)group_start[g + 1] - group_start[g];
      if (len < 1 || len > n_max) return -22;
    }
  }
  if (nt > 0 && !out_cov) return -23;
  hipStream_t st = (hipStream_t)stream;
  EWs w((char*)workspace, n, nt, L);
  double* panel = (double*)((char*)workspace + w.bytes);
  double* part = (double*)((char*)panel + exact_var_panel_bytes(n, nt, L, chunk));
  // the factor of K (and the mean, by lvae_predict_exact_f64's own launches)
  LVAE_TRY(exact_core(spec, x, ldx, n, L, params, noise, mu, ld_mu, tx, ldt, nt, out_mean, ld_out, info, w, stream));
  if (nt == 0) return 0;
  const int64_t nb = (int64_t)L * n_groups;
  pc_eye_kernel<<<nblk(nb * n_max * n_max), 256, 0, st>>>(nb, n_max, out_cov);
  // whole groups at a time, as many as fit c panel columns: the panel k(X, X*_chunk) [L, n, c] and one triangular
  // solve in place as lvae_predict_exact_var_f64, then per launch of <= kCovBatch groups the slabs' partial tiles
  // and their sum in slab order.  A column's solve does not depend on its neighbours and a tile's slabs depend on n
  // alone, so the bits do not depend on the chunk.
  const int c = chunk < nt ? chunk : nt, nslab = exact_cov_slabs(n), bucket = spec_bucket(spec);
  const DevSpec ds = to_dev(spec);
  const lvae_xview xv{x, 0, 0, ldx};
  for (int g0 = 0; g0 < n_groups;) {
    int g1 = g0;
    while (g1 < n_groups && group_start[g1 + 1] - group_start[g0] <= c) ++g1;
    const int c0 = group_start[g0], nr = group_start[g1] - c0;
    const double* tc = tx + (int64_t)c0 * ldt;
    const lvae_xview tv{tc, 0, 0, ldt};
    LVAE_TRY(lvae_gram_f64(spec, xv, tv, 1, L, n, nr, params, nullptr, panel, 0, (int64_t)n * c, c, stream));
    LVAE_TRY(lvae_trsm_f64(0, n, nr, L, w.K, n, (int64_t)n * n, panel, c, (int64_t)n * c, w.trsm, stream));
    int tile0 = 0;
    for (int b0 = g0; b0 < g1; b0 += kCovBatch) {
      CovBatch cb;
      cb.n = g1 - b0 < kCovBatch ? g1 - b0 : kCovBatch;
      cb.tile[0] = 0;
      for (int b = 0; b <= cb.n; ++b) {
        cb.col[b] = group_start[b0 + b] - c0;
        if (b > 0) cb.tile[b] = cb.tile[b - 1] + cov_tiles(cb.col[b] - cb.col[b - 1]);
      }
      for (int b = cb.n + 1; b <= kCovBatch; ++b) cb.col[b] = cb.col[cb.n], cb.tile[b] = cb.tile[cb.n];
      const int nt_b = cb.tile[cb.n];
      pcx_partial_kernel<<<dim3(nt_b, nslab, L), 64, 0, st>>>(cb, n, panel, c, tile0, c, part);
      if (bucket == 1)
        pcx_reduce_kernel<8, 2><<<dim3(nt_b, L), 256, 0, st>>>(ds, cb, nslab, tile0, c, part, tc, ldt, params, noise,
                                                               add_noise, b0, n_groups, n_max, out_cov);
      else
        pcx_reduce_kernel<16, 4><<<dim3(nt_b, L), 256, 0, st>>>(ds, cb, nslab, tile0, c, part, tc, ldt, params, noise,
                                                                add_noise, b0, n_groups, n_max, out_cov);
      tile0 += nt_b;
    }
    g0 = g1;
  }
  LVAE_CHECK_LAUNCH();
  return 0;
}

size_t lvae_predict_sample_workspace_size(int L, int n_groups, int n_max) {
  if (L < 1 || n_groups < 0 || n_max < 1) return 0;
  return SWs(nullptr, L, n_groups > 0 ? n_groups : 1, n_max).bytes;
}

int lvae_predict_sample_f64(int L, int n_groups, int n_max, int Nt, int S, const double* cov, const int32_t* index,
                            const double* mean, const double* eps, double jitter, double* out, int32_t* info,
                            void* workspace, void* stream) {
  if (L < 1) return -1;  // (before any launch)
  if (n_groups < 0 || (int64_t)L * n_groups > 65535) return -2;
  if (n_max < 1 || n_max > kPvT) return -3;
  if (Nt < 0 || (int64_t)Nt > (int64_t)n_groups * n_max) return -4;  // (some row is in no group)
  if (S < 0) return -5;
  if (n_groups > 0 && !cov) return -6;
  if (n_groups > 0 && !index) return -7;
  if (Nt > 0 && S > 0 && !mean) return -8;
  if (Nt > 0 && S > 0 && !eps) return -9;
  if (!(jitter >= 0.0)) return -10;
  if (Nt > 0 && S > 0 && !out) return -11;
  if (n_groups > 0 && !info) return -12;
  if (!workspace || ((uintptr_t)workspace & 255)) return -13;
  if (n_groups == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  SWs w((char*)workspace, L, n_groups, n_max);
  const int64_t nb = (int64_t)L * n_groups, nn = (int64_t)n_max * n_max;
  pcs_jitter_kernel<<<nblk(nb * nn), 256, 0, st>>>(nb, n_max, jitter, cov, w.Lc);
  LVAE_TRY(lvae_potrf_f64(n_max, (int)nb, w.Lc, n_max, nn, w.Lc, n_max, nn, w.logdet, info, stream));
  if (Nt > 0 && S > 0)
    pcs_draw_kernel<<<nblk((int64_t)S * nb * n_max), 256, 0, st>>>(L, n_groups, n_max, Nt, S, w.Lc, index, mean, eps,
                                                                   out);
  LVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
