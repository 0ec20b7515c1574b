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
// Two routes, the inducing-point one above (lvae_predict_*_f64) and the exact-GP one (lvae_predict_exact_*_f64), each
// with a mean, its split by additive component of the kernel (_comp_: both means are linear in it), the components'
// joint covariance at each test row (_comp_cov_), the predictive variance (_var_) and the joint covariance of each
// group of test rows (_cov_); lvae_predict_sample_f64 draws whole trajectories from the latter.  The kernels and
// formulas are in predict_var.hpp, predict_cov.hpp and predict_ccov.hpp.  Per route this file holds, each once: the
// entries' arguments (InducingArgs / ExactArgs), the checks they share in their documented order (check), the
// workspace layout that the size query carves on a null base and the entry on the real one (InducingWs / ExactWs),
// the mean (core), its split by component (comp_split), the inducing route's C, D, E and Q, W, V (group_stage,
// var_solves, var_pipeline) and the exact route's pass over chunks of test rows (chunks).  An entry is then its own
// checks, its carve and the launches that are its alone.
#include <type_traits>

#include "gram.hpp"
#include "small.hpp"
#include "prof.hpp"
#include "predict_var.hpp"
#include "predict_cov.hpp"
#include "predict_ccov.hpp"

namespace lvae {

namespace {

constexpr int64_t kPredChunkElems = 1 << 24;  // k1(X*, x) chunk: <= 128 MiB of fp64

inline int nblk(int64_t n) { return cdiv(n, 256); }
inline bool ws_ok(const void* p) { return p && !((uintptr_t)p & 255); }
inline char* take_bytes(WsCarve& c, size_t b) { return (char*)c.take((b + 7) / 8); }  // (256-byte aligned too)

// f(BC, BF) with spec_bucket's template arguments as std::integral_constants: <8, 2> for bucket 1, else <16, 4>
template <class F>
inline void with_bucket(int bucket, F&& f) {
  if (bucket == 1)
    f(std::integral_constant<int, 8>{}, std::integral_constant<int, 2>{});
  else
    f(std::integral_constant<int, 16>{}, std::integral_constant<int, 4>{});
}

// What a route's shared argument check asks for beyond the part every entry has
enum : unsigned {
  kMeanRequired = 1,  // exact route: mu and out must be given (otherwise they are checked only when out is given)
  kPointers = 2,      // inducing route: mu (when out is given), x, z, params*, noise, test_x and the group arrays
  kGridL = 4,         // L <= 65535: L is a grid dimension
  kGridGroups = 8,    // n_groups <= 65535: the groups are a grid dimension
  kCompLd = 16,       // inducing route: the factor dims must suit the component product, and Q cover them
  kCompCount = 32,    // each spec has a component (inducing route: and Nt R fits an int)
};

// workspace of the mean (lvae_predict_f64)
struct PWs {
  double *K0xz, *iBK, *K0zz, *Hm, *iK, *iH, *Bst, *iB, *iBmu, *t, *muT, *muTm, *w, *v, *a, *b, *rr, *K0Xz, *out1, *K1;
  double *ldK, *ldH, *ldB;
  int32_t* info;
  int64_t chunk_rows;
  void carve(WsCarve& c, int L, int M, int P, int T, int Nt) {
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
  }
};

// workspace of the variance routes behind the mean's: G [L, M, M], the test rows' subjects, and per latent dim the
// [T, Nt] matrices C, D and the [M, Nt] matrices E, K0zX*, Q, W, V and the residual R
struct VWs {
  double *Gm, *C, *D, *E, *KzX, *Qm, *W, *V, *R;
  int32_t* rs;
  void carve(WsCarve& c, int L, int M, int T, int Nt) {
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
  }
};

// The inducing-point route's one workspace layout: the mean's part (w) for `cols` columns (at least 1), then, where
// asked for, the variance routes' (v) for the same columns and the component product's (cmv): comp_nt test rows
// against the M inducing points (R0 components) and against the P T prediction rows (R1)
struct InducingWs {
  PWs w;
  VWs v{};
  void* cmv = nullptr;
  size_t bytes;
  InducingWs(void* base, int L, int M, int P, int T, int cols, bool var, bool comp = false, int comp_nt = 0,
             int R0 = 0, int R1 = 0) {
    WsCarve c((char*)base);
    const int n1 = cols > 0 ? cols : 1;
    w.carve(c, L, M, P, T, n1);
    if (var) v.carve(c, L, M, T, n1);
    if (comp) {
      const size_t m0 = lvae_gram_matvec_comp_workspace_size(comp_nt, M, L, R0);
      const size_t m1 = lvae_gram_matvec_comp_workspace_size(comp_nt, P * T, L, R1);
      cmv = take_bytes(c, m0 > m1 ? m0 : m1);
    }
    bytes = c.off;
  }
};

// ---- inducing-point route: an entry's arguments, and as its members the stages the entries share ----
struct InducingArgs {
  const lvae_kernel_spec *spec0, *spec1;
  int L, M, Q, P, T;
  const int32_t *seg_len, *include;
  const double *x, *mu, *z;
  int Nt;
  const double* test_x;
  const double *params0, *params1, *noise;
  double eps;
  double* out;
  int32_t* info;
  void *workspace, *stream;
  int n_groups = 0;  // the test rows' subject groups (variance and covariance entries)
  const int32_t *group_subject = nullptr, *group_start = nullptr;
  double* out_comp = nullptr;  // the mean's split by component
  int64_t ld_comp = 0, cstride_r = 0;

  hipStream_t st() const { return (hipStream_t)stream; }
  int check(unsigned f) const;
  int core(bool mean, double* Gm, PWs& w) const;
  int comp_split(InducingWs& s) const;
  template <class LaunchC>
  int group_stage(InducingWs& s, int R, LaunchC launch_c) const;
  int var_pipeline(InducingWs& s) const;
};

// The checks the inducing-point entries share, codes -1 .. -15 in their documented order (-13 before -12); the
// workspace (-20) and an entry's own codes follow in the entry.
int InducingArgs::check(unsigned f) const {
  if (!spec0 || !spec1 || !spec_bucket(spec0) || !spec_bucket(spec1)) return -1;  // (before any launch)
  int ld0 = 1, ld1 = 1;
  if (f & kCompLd) {
    ld0 = gram_matvec_spec_ld(spec0), ld1 = gram_matvec_spec_ld(spec1);
    if (ld0 < 1 || ld1 < 1) return -1;  // (a factor dim outside 0 .. 31: the fused product does not take it)
  }
  if ((f & kCompCount) && (spec0->n_comp < 1 || spec1->n_comp < 1)) return -1;
  if (L < 1 || ((f & kGridL) && L > 65535) || M < 1 || M > 128) return -3;
  if (P < 1 || T < 1 || T > 128 || Q < 1 || Q < ld0 || Q < ld1) return -6;
  if (!seg_len || !include) return -8;
  const bool ptrs = (f & kPointers) != 0;
  if (ptrs && out && !mu) return -9;
  if (ptrs && (!x || !z)) return -10;
  if (ptrs && (!params0 || !params1 || !noise)) return -11;
  if (Nt < 0 || ((f & kCompCount) && (int64_t)Nt * (spec0->n_comp + spec1->n_comp) > INT32_MAX)) return -13;
  if (!ptrs) return 0;
  if (Nt > 0 && !test_x) return -12;
  if (n_groups < 0 || ((f & kGridGroups) && n_groups > 65535)) return -14;
  if (n_groups > 0 && (!group_subject || !group_start)) return -15;
  return 0;
}

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

// The launches of lvae_predict_f64 on the carved workspace w (arguments checked by the caller).  mean = false
// stops after the factorisations (the variance alone needs no mu~); Gm, when given, receives
// G = K0zx iB K0xz [L, M, M] before K0zz is added to it (H - K0zz would lose G's low bits).
int InducingArgs::core(bool mean, double* Gm, PWs& w) const {
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

// The mean's split by component on the b and mu~m that core leaves in the workspace: k0_r(X*, z_l) b_l
// (blocks 0 .. R0 - 1) and k1_r(X*, x) mu~m_l (blocks R0 .. R0 + R1 - 1); mu~m is 0 on padding rows and on subjects
// outside the test set
int InducingArgs::comp_split(InducingWs& s) const {
  LVAE_TRY(gram_matvec_comp_f64(spec0, test_x, Q, Nt, z, Q, (int64_t)M * Q, M, L, params0, s.w.b, M, 1, out_comp, ld_comp,
                                0, cstride_r, s.cmv, st()));
  return gram_matvec_comp_f64(spec1, test_x, Q, Nt, x, Q, 0, P * T, L, params1, s.w.muTm, (int64_t)P * T, 1,
                              out_comp + (int64_t)spec0->n_comp * cstride_r, ld_comp, 0, cstride_r, s.cmv, st());
}

// c_i, d_i = iB_s c_i, e_i = K0zx_s d_i per subject group, R columns a test row (group g: the columns
// [R group_start[g], R group_start[g + 1]); rows of no group, or of an absent subject: 0): the rows' subjects, the C
// kernel (launch_c), then D and E
template <class LaunchC>
int InducingArgs::group_stage(InducingWs& s, int R, LaunchC launch_c) const {
  const int Nc = Nt * R;
  pv_rowsubj_kernel<<<nblk(Nt), 256, 0, st()>>>(Nt, P, n_groups, group_subject, group_start, s.v.rs);
  launch_c();
  LVAE_TRY(zero_async(s.v.D, (size_t)L * T * Nc * sizeof(double), st()));
  LVAE_TRY(zero_async(s.v.E, (size_t)L * M * Nc * sizeof(double), st()));
  if (n_groups > 0)
    pv_group_kernel<<<dim3(Nc / kPvC + n_groups, L), 256, 0, st()>>>(M, P, T, Nc, n_groups, R, group_subject,
                                                                    group_start, s.v.C, s.w.iB, s.w.K0xz, s.v.D, s.v.E);
  return 0;
}

// Q, W and V of the variance routes from K0zX* (v.KzX) and E, each [L, M, N] with the N columns on the workspaces w
// and v (after core's launches); a column's results do not depend on its neighbours.
int var_solves(int L, int M, int N, PWs& w, VWs& v, hipStream_t st) {
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

// The launches of lvae_predict_var_f64 up to its last kernel, on the carved workspace s (arguments checked by the
// caller): lvae_predict_f64's own (and the mean when out is given), then C, D, E, K0zX*, Q, W and V [rows, Nt].
int InducingArgs::var_pipeline(InducingWs& s) const {
  // the Grams, iB, K0zz^-1, H^-1 (and the mean) by lvae_predict_f64's own launches; G kept aside
  LVAE_TRY(core(out != nullptr, s.v.Gm, s.w));
  if (Nt == 0) return 0;
  const DevSpec d1 = to_dev(spec1);
  LVAE_TRY(group_stage(s, 1, [&] {
    with_bucket(spec_bucket(spec1), [&](auto BC, auto BF) {
      pv_c_kernel<BC.value, BF.value><<<nblk((int64_t)L * T * Nt), 256, 0, st()>>>(d1, L, T, Nt, Q, seg_len, s.v.rs, x,
                                                                                  test_x, params1, s.v.C);
    });
  }));
  // K0zX* [L, M, Nt] is its own Gram (test rows as columns); then Q, W and V
  const lvae_xview zv{z, 0, (int64_t)M * Q, Q}, tv{test_x, 0, 0, Q};
  LVAE_TRY(lvae_gram_f64(spec0, zv, tv, 1, L, M, Nt, params0, nullptr, s.v.KzX, 0, (int64_t)M * Nt, Nt, stream));
  return var_solves(L, M, Nt, s.w, s.v, st());
}

inline int exact_cov_slabs(int n) { return cdiv(n, kCovSlab); }
// The exact route's one workspace layout: K [L, n, n] (factored in place), the work vectors a, r [L, n], the factor's
// log-determinants, the solves' inverted diagonal blocks and the fused products' slab partials; then, where asked
// for, the component product's workspace for n_comp components, the panel k(X, X*_chunk) [L, n, c panel_cols]
// (solved in place; c = chunk cut to nt) and the slabs' partial tiles [L, c, nslab, 16, 16] (a chunk of c columns in
// whole groups of <= 128 rows holds at most c tiles on and below the diagonals; one tile a row by component)
struct ExactWs {
  double *K, *a, *r, *logdet, *panel, *part;
  char *trsm, *mv, *cmv;
  size_t bytes;
  ExactWs(void* base, int n, int nt, int L, int n_comp = 0, int chunk = 0, int panel_cols = 0, bool parts = false) {
    WsCarve c((char*)base);
    K = c.take((size_t)L * n * n);
    a = c.take((size_t)L * n);
    r = c.take((size_t)L * n);
    logdet = c.take((size_t)L);
    trsm = take_bytes(c, lvae_trsm_workspace_size(n, L));
    const size_t m0 = lvae_gram_matvec_workspace_size(n, n, L), m1 = lvae_gram_matvec_workspace_size(nt, n, L);
    mv = take_bytes(c, m0 > m1 ? m0 : m1);
    cmv = take_bytes(c, n_comp > 0 ? lvae_gram_matvec_comp_workspace_size(nt, n, L, n_comp) : 0);
    const int cc = chunk < nt ? chunk : nt, c1 = cc > 0 ? cc : 0;
    panel = c.take((size_t)L * n * c1 * panel_cols);
    part = c.take(parts ? (size_t)L * c1 * exact_cov_slabs(n) * 256 : 0);
    bytes = c.off;
  }
};

// ---- exact-GP route (model_test.py:11-17 predict_gp, as MSE_test calls it, model_test.py:19-82) ----
struct ExactArgs {
  const lvae_kernel_spec* spec;
  const double* x;
  int64_t ldx;
  int n, L;
  const double *params, *noise, *mu;
  int64_t ld_mu;
  const double* tx;
  int64_t ldt;
  int nt;
  double* out;
  int64_t ld_out;
  int32_t* info;
  void *workspace, *stream;
  double* out_comp = nullptr;  // the mean's split by component
  int64_t ld_comp = 0, cstride_r = 0;

  int check(unsigned f) const;
  int core(ExactWs& w) const;
  int comp_split(ExactWs& w) const;
  template <class Rows, class Reduce>
  int chunks(ExactWs& w, int c, bool by_comp, Rows rows, Reduce reduce) const;
};

// The checks the exact-route entries share, codes -1 .. -16 in their documented order (-12 before -10); an entry's
// own codes follow in the entry.
int ExactArgs::check(unsigned f) const {
  const int ld_min = spec ? gram_matvec_spec_ld(spec) : 0;
  if (ld_min < 1 || ld_min > 32 || ((f & kCompCount) && spec->n_comp < 1)) return -1;  // (before any launch)
  if (!x) return -2;
  if (ldx < ld_min) return -3;
  if (n < 1) return -4;
  if (L < 1 || ((f & kGridL) && L > 65535)) return -5;
  if (!params) return -6;
  if (!noise) return -7;
  const bool required = (f & kMeanRequired) != 0, mean = required || out;
  if (mean && !mu) return -8;
  if (mean && ld_mu < L) return -9;
  if (nt < 0) return -12;
  if (nt > 0 && !tx) return -10;
  if (nt > 0 && ldt < ld_min) return -11;
  if (nt > 0 && (required || out_comp) && !out) return -13;
  if ((required ? nt > 0 : out != nullptr) && ld_out < L) return -14;
  if (!info) return -15;
  if (!ws_ok(workspace)) return -16;
  return 0;
}

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

// The launches of lvae_predict_exact_f64 on the carved workspace w (arguments checked by the caller): the factor
// of K into w.K and, when out is given, the mean.
int ExactArgs::core(ExactWs& w) const {
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

// The mean's split by component: k_r(X*, x) a per component r on the refined a that core leaves in the workspace
int ExactArgs::comp_split(ExactWs& w) const {
  return gram_matvec_comp_f64(spec, tx, ldt, nt, x, ldx, 0, n, L, params, w.a, n, 1, out_comp, ld_comp, 0, cstride_r,
                              w.cmv, (hipStream_t)stream);
}

// The exact route's pass over the test rows, rows(c0) of them at a time from row c0 on (at most c): the panel
// k(X, X*_chunk) [L, n, nr] with leading dimension c (by_comp: the component-resolved k_r(X, X*_chunk) [L, n, nr R],
// column t R + r, leading dimension c R), one triangular solve in place on its columns, then reduce(c0, nr, tc) with
// tc the chunk's test rows.  A column's solve does not depend on its neighbours, so the bits do not depend on c.
template <class Rows, class Reduce>
int ExactArgs::chunks(ExactWs& w, int c, bool by_comp, Rows rows, Reduce reduce) const {
  hipStream_t st = (hipStream_t)stream;
  const int R = by_comp ? spec->n_comp : 1;
  const int64_t ldp = (int64_t)c * R;
  const DevSpec ds = to_dev(spec);
  const lvae_xview xv{x, 0, 0, ldx};
  for (int c0 = 0; c0 < nt;) {
    const int nr = rows(c0);
    const double* tc = tx + (int64_t)c0 * ldt;
    if (by_comp) {
      with_bucket(spec_bucket(spec), [&](auto, auto BF) {
        pcc_panel_kernel<BF.value><<<nblk((int64_t)L * n * nr), 256, 0, st>>>(ds, L, n, nr, x, ldx, tc, ldt, params,
                                                                             w.panel, ldp);
      });
    } else {
      const lvae_xview tv{tc, 0, 0, ldt};
      LVAE_TRY(lvae_gram_f64(spec, xv, tv, 1, L, n, nr, params, nullptr, w.panel, 0, (int64_t)n * c, c, stream));
    }
    LVAE_TRY(lvae_trsm_f64(0, n, nr * R, L, w.K, n, (int64_t)n * n, w.panel, ldp, (int64_t)n * ldp, w.trsm, stream));
    LVAE_TRY(reduce(c0, nr, tc));
    c0 += nr;
  }
  return 0;
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
}  // namespace lvae

using namespace lvae;

extern "C" {

// ---- inducing-point route ----
size_t lvae_predict_workspace_size(int L, int M, int P, int T, int Nt) {
  return InducingWs(nullptr, L, M, P, T, Nt, false).bytes;
}

int lvae_predict_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P, int T,
                     const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                     const double* z, int Nt, const double* test_x, const double* params0, const double* params1,
                     const double* noise, double eps, double* out, int32_t* info, void* workspace, void* stream) {
  const InducingArgs a{spec0, spec1, L, M, Q, P, T, seg_len, include, x, mu, z, Nt, test_x, params0, params1, noise,
                       eps, out, info, workspace, stream};
  LVAE_TRY(a.check(0));
  if (!ws_ok(workspace)) return -20;
  InducingWs s(workspace, L, M, P, T, Nt, false);
  return a.core(true, nullptr, s.w);
}

size_t lvae_predict_comp_workspace_size(int L, int M, int P, int T, int Nt, int n_comp0, int n_comp1) {
  return InducingWs(nullptr, L, M, P, T, Nt, false, true, Nt, n_comp0, n_comp1).bytes;
}

int lvae_predict_comp_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P,
                          int T, const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                          const double* z, int Nt, const double* test_x, const double* params0, const double* params1,
                          const double* noise, double eps, double* out, double* out_comp, int64_t ld_comp,
                          int64_t cstride_r, int32_t* info, void* workspace, void* stream) {
  const InducingArgs a{spec0, spec1, L, M, Q, P, T, seg_len, include, x, mu, z, Nt, test_x, params0, params1, noise,
                       eps, out, info, workspace, stream, 0, nullptr, nullptr, out_comp, ld_comp, cstride_r};
  LVAE_TRY(a.check(kCompLd));
  if (!ws_ok(workspace)) return -20;
  if (Nt > 0 && !out_comp) return -21;
  if (Nt > 0 && ld_comp < L) return -22;
  if (Nt > 0 && spec0->n_comp + spec1->n_comp > 1 && cstride_r < (int64_t)Nt * ld_comp) return -23;
  InducingWs s(workspace, L, M, P, T, Nt, false, true, Nt, spec0->n_comp, spec1->n_comp);
  // the mean by lvae_predict_f64's own launches (its dense chunked K1 route included), then its split
  LVAE_TRY(a.core(true, nullptr, s.w));
  if (Nt == 0) return 0;
  return a.comp_split(s);
}

size_t lvae_predict_var_workspace_size(int L, int M, int P, int T, int Nt) {
  return InducingWs(nullptr, L, M, P, T, Nt, true).bytes;
}

int lvae_predict_var_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P,
                         int T, const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                         const double* z, int Nt, const double* test_x, int n_groups, const int32_t* group_subject,
                         const int32_t* group_start, const double* params0, const double* params1,
                         const double* noise, double eps, double* out, double* out_var, int add_noise, int32_t* info,
                         void* workspace, void* stream) {
  const InducingArgs a{spec0, spec1, L, M, Q, P, T, seg_len, include, x, mu, z, Nt, test_x, params0, params1, noise,
                       eps, out, info, workspace, stream, n_groups, group_subject, group_start};
  LVAE_TRY(a.check(kPointers));
  if (Nt > 0 && !out_var) return -16;
  if (add_noise != 0 && add_noise != 1) return -17;
  if (!ws_ok(workspace)) return -20;
  hipStream_t st = (hipStream_t)stream;
  InducingWs s(workspace, L, M, P, T, Nt, true);
  LVAE_TRY(a.var_pipeline(s));
  if (Nt == 0) return 0;
  const DevSpec d1 = to_dev(spec1);
  const VWs& v = s.v;
  with_bucket(spec_bucket(spec1), [&](auto BC, auto BF) {
    pv_var_kernel<BC.value, BF.value><<<nblk((int64_t)L * Nt), 256, 0, st>>>(
        d1, L, M, T, Nt, Q, v.KzX, v.Qm, v.W, v.E, v.V, v.C, v.D, test_x, params1, noise, add_noise, out_var);
  });
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
  const InducingArgs a{spec0, spec1, L, M, Q, P, T, seg_len, include, x, mu, z, Nt, test_x, params0, params1, noise,
                       eps, out, info, workspace, stream, n_groups, group_subject, group_start};
  LVAE_TRY(a.check(kPointers | kGridL | kGridGroups));
  if (n_groups > 0 && !out_cov) return -16;
  if (add_noise != 0 && add_noise != 1) return -17;
  if (n_groups > 0 && (n_max < 1 || n_max > kPvT)) return -18;
  if (!ws_ok(workspace)) return -20;
  hipStream_t st = (hipStream_t)stream;
  InducingWs s(workspace, L, M, P, T, Nt, true);
  LVAE_TRY(a.var_pipeline(s));
  if (Nt == 0 || n_groups == 0) return 0;
  const int64_t nb = (int64_t)L * n_groups;
  pc_eye_kernel<<<nblk(nb * n_max * n_max), 256, 0, st>>>(nb, n_max, out_cov);
  const DevSpec d1 = to_dev(spec1);
  const VWs& v = s.v;
  with_bucket(spec_bucket(spec1), [&](auto BC, auto BF) {
    pc_cov_kernel<BC.value, BF.value><<<dim3(cov_tiles(n_max), n_groups, L), 64, 0, st>>>(
        d1, M, T, Nt, Q, n_max, group_start, v.KzX, v.Qm, v.W, v.E, v.V, v.C, v.D, test_x, params1, noise, add_noise,
        out_cov);
  });
  LVAE_CHECK_LAUNCH();
  return 0;
}

size_t lvae_predict_comp_cov_workspace_size(int L, int M, int P, int T, int Nt, int n_comp0, int n_comp1) {
  const int64_t R = (int64_t)n_comp0 + n_comp1;
  if (L < 1 || M < 1 || M > 128 || P < 1 || T < 1 || T > 128 || Nt < 0 || n_comp0 < 1 || n_comp1 < 1 ||
      n_comp0 > LVAE_MAX_COMP || n_comp1 > LVAE_MAX_COMP || Nt * R > INT32_MAX)
    return 0;
  return InducingWs(nullptr, L, M, P, T, (int)(Nt * R), true, true, Nt, n_comp0, n_comp1).bytes;
}

int lvae_predict_comp_cov_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, int L, int M, int Q, int P,
                              int T, const int32_t* seg_len, const int32_t* include, const double* x, const double* mu,
                              const double* z, int Nt, const double* test_x, int n_groups,
                              const int32_t* group_subject, const int32_t* group_start, const double* params0,
                              const double* params1, const double* noise, double eps, double* out, double* out_comp,
                              int64_t ld_comp, int64_t cstride_r, double* out_ccov, int32_t* info, void* workspace,
                              void* stream) {
  const InducingArgs a{spec0, spec1, L, M, Q, P, T, seg_len, include, x, mu, z, Nt, test_x, params0, params1, noise,
                       eps, out, info, workspace, stream, n_groups, group_subject, group_start, out_comp, ld_comp,
                       cstride_r};
  LVAE_TRY(a.check(kPointers | kGridL | kCompLd | kCompCount));
  if (!ws_ok(workspace)) return -20;
  if (Nt > 0 && out_comp && !out) return -21;
  if (Nt > 0 && out_comp && ld_comp < L) return -22;
  if (Nt > 0 && out_comp && cstride_r < (int64_t)Nt * ld_comp) return -23;
  if (Nt > 0 && !out_ccov) return -24;
  hipStream_t st = (hipStream_t)stream;
  const int R0 = spec0->n_comp, R = R0 + spec1->n_comp;  // one column per (test row, component)
  InducingWs s(workspace, L, M, P, T, Nt * R, true, true, Nt, R0, R - R0);
  const VWs& v = s.v;
  // the Grams, iB, K0zz^-1, H^-1 and, when wanted, the mean by lvae_predict_f64's own launches (a workspace carved
  // for Nt R rows leaves them as they are); G kept aside; then the mean's split as lvae_predict_comp_f64
  LVAE_TRY(a.core(out != nullptr, s.v.Gm, s.w));
  if (Nt == 0) return 0;
  if (out && out_comp) LVAE_TRY(a.comp_split(s));
  // the columns' K0zX* and C through the specs, D and E per subject group, Q, W and V by the variance route's own
  // launches, then the blocks
  const DevSpec d0 = to_dev(spec0), d1 = to_dev(spec1);
  LVAE_TRY(a.group_stage(s, R, [&] {
    with_bucket(spec_bucket(spec0), [&](auto, auto BF) {
      pcc_kzx_kernel<BF.value><<<nblk((int64_t)L * M * Nt), 256, 0, st>>>(d0, L, M, Nt, Q, R, z, test_x, params0, v.KzX);
    });
    with_bucket(spec_bucket(spec1), [&](auto, auto BF) {
      pcc_c_kernel<BF.value><<<nblk((int64_t)L * T * Nt), 256, 0, st>>>(d1, L, T, Nt, Q, R0, seg_len, v.rs, x, test_x,
                                                                       params1, v.C);
    });
  }));
  LVAE_TRY(var_solves(L, M, Nt * R, s.w, s.v, st));
  with_bucket(spec_bucket(spec1), [&](auto, auto BF) {
    pcc_ind_kernel<BF.value><<<dim3((unsigned)Nt * cov_tiles(R), L), 64, 0, st>>>(
        d1, M, T, Nt, Q, R0, v.KzX, v.Qm, v.W, v.E, v.V, v.C, v.D, test_x, params1, out_ccov);
  });
  LVAE_CHECK_LAUNCH();
  return 0;
}

// ---- exact-GP route ----
size_t lvae_predict_exact_workspace_size(int n, int nt, int L) {
  if (n < 1 || nt < 0 || L < 1) return 0;
  return ExactWs(nullptr, n, nt, L).bytes;
}

int lvae_predict_exact_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                           const double* params, const double* noise, const double* mu, int64_t ld_mu,
                           const double* tx, int64_t ldt, int nt, double* out, int64_t ld_out, int32_t* info,
                           void* workspace, void* stream) {
  const ExactArgs a{spec, x, ldx, n, L, params, noise, mu, ld_mu, tx, ldt, nt, out, ld_out, info, workspace, stream};
  LVAE_TRY(a.check(kMeanRequired));
  ExactWs w(workspace, n, nt, L);
  return a.core(w);
}

size_t lvae_predict_exact_comp_workspace_size(int n, int nt, int L, int n_comp) {
  if (n < 1 || nt < 0 || L < 1 || n_comp < 1) return 0;
  return ExactWs(nullptr, n, nt, L, n_comp).bytes;
}

int lvae_predict_exact_comp_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                                const double* params, const double* noise, const double* mu, int64_t ld_mu,
                                const double* tx, int64_t ldt, int nt, double* out, int64_t ld_out, double* out_comp,
                                int64_t ld_comp, int64_t cstride_r, int32_t* info, void* workspace, void* stream) {
  const ExactArgs a{spec, x, ldx, n, L, params, noise, mu, ld_mu, tx, ldt, nt, out, ld_out, info, workspace, stream,
                    out_comp, ld_comp, cstride_r};
  LVAE_TRY(a.check(kMeanRequired));
  if (nt > 0 && !out_comp) return -17;
  if (nt > 0 && ld_comp < L) return -18;
  if (nt > 0 && spec->n_comp > 1 && cstride_r < (int64_t)nt * ld_comp) return -19;
  ExactWs w(workspace, n, nt, L, spec->n_comp);
  // the factor and the mean by lvae_predict_exact_f64's own launches, then the mean's split
  LVAE_TRY(a.core(w));
  if (nt == 0) return 0;
  return a.comp_split(w);
}

size_t lvae_predict_exact_comp_cov_workspace_size(int n, int nt, int L, int n_comp, int chunk) {
  if (n < 1 || nt < 0 || L < 1 || n_comp < 1 || n_comp > LVAE_MAX_COMP || (nt > 0 && chunk < 1)) return 0;
  return ExactWs(nullptr, n, nt, L, n_comp, chunk, n_comp, true).bytes;
}

int lvae_predict_exact_comp_cov_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                                    const double* params, const double* noise, const double* mu, int64_t ld_mu,
                                    const double* tx, int64_t ldt, int nt, double* out, int64_t ld_out,
                                    double* out_comp, int64_t ld_comp, int64_t cstride_r, int chunk, double* out_ccov,
                                    int32_t* info, void* workspace, void* stream) {
  const ExactArgs a{spec, x, ldx, n, L, params, noise, mu, ld_mu, tx, ldt, nt, out, ld_out, info, workspace, stream,
                    out_comp, ld_comp, cstride_r};
  LVAE_TRY(a.check(kGridL | kCompCount));
  if (nt > 0 && out_comp && ld_comp < L) return -18;
  if (nt > 0 && out_comp && spec->n_comp > 1 && cstride_r < (int64_t)nt * ld_comp) return -19;
  if (nt > 0 && chunk < 1) return -20;
  if (nt > 0 && !out_ccov) return -21;
  hipStream_t st = (hipStream_t)stream;
  const int R = spec->n_comp;
  ExactWs w(workspace, n, nt, L, R, chunk, R, true);
  // the factor of K, and when wanted the mean and its split, by lvae_predict_exact_comp_f64's own launches
  LVAE_TRY(a.core(w));
  if (nt == 0) return 0;
  if (out && out_comp) LVAE_TRY(a.comp_split(w));
  // c test rows at a time, the component-resolved panel solved in place; then per row the slabs' partial tiles of
  // V^T V and their sum in slab order under the components' prior variances.  A tile's slabs depend on n alone, so
  // the bits do not depend on the chunk.
  const int c = chunk < nt ? chunk : nt, nslab = exact_cov_slabs(n);
  const DevSpec ds = to_dev(spec);
  LVAE_TRY(a.chunks(
      w, c, true, [&](int c0) { return nt - c0 < c ? nt - c0 : c; },
      [&](int c0, int nr, const double* tc) {
        pcc_partial_kernel<<<dim3(nr, nslab, L), 64, 0, st>>>(n, R, w.panel, (int64_t)c * R, c, w.part);
        with_bucket(spec_bucket(spec), [&](auto, auto BF) {
          pcc_reduce_kernel<BF.value><<<dim3(nr, L), 256, 0, st>>>(ds, nslab, c, w.part, tc, ldt, params, c0, nt,
                                                                   out_ccov);
        });
        return 0;
      }));
  LVAE_CHECK_LAUNCH();
  return 0;
}

size_t lvae_predict_exact_var_workspace_size(int n, int nt, int L, int chunk) {
  if (n < 1 || nt < 0 || L < 1 || (nt > 0 && chunk < 1)) return 0;
  return ExactWs(nullptr, n, nt, L, 0, chunk, 1).bytes;
}

int lvae_predict_exact_var_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                               const double* params, const double* noise, const double* mu, int64_t ld_mu,
                               const double* tx, int64_t ldt, int nt, double* out_mean, int64_t ld_out,
                               double* out_var, int64_t ld_var, int add_noise, int chunk, int32_t* info,
                               void* workspace, void* stream) {
  const ExactArgs a{spec, x, ldx, n, L, params, noise, mu, ld_mu, tx, ldt, nt, out_mean, ld_out, info, workspace, stream};
  LVAE_TRY(a.check(0));
  if (nt > 0 && !out_var) return -17;
  if (nt > 0 && ld_var < L) return -18;
  if (add_noise != 0 && add_noise != 1) return -19;
  if (nt > 0 && chunk < 1) return -20;
  hipStream_t st = (hipStream_t)stream;
  ExactWs w(workspace, n, nt, L, 0, chunk, 1);
  // the factor of K (and the mean, by lvae_predict_exact_f64's own launches)
  LVAE_TRY(a.core(w));
  if (nt == 0) return 0;
  // var = k(x*, x*) - |L^-1 k(X, x*)|^2, c test rows at a time: the panel solved in place, then the columns' sums of
  // squares.  A column's sum does not depend on its neighbours, so the bits do not depend on the chunk.
  const int c = chunk < nt ? chunk : nt;
  const DevSpec ds = to_dev(spec);
  LVAE_TRY(a.chunks(
      w, c, false, [&](int c0) { return nt - c0 < c ? nt - c0 : c; },
      [&](int c0, int nr, const double* tc) {
        double* vo = out_var + (int64_t)c0 * ld_var;
        with_bucket(spec_bucket(spec), [&](auto BC, auto BF) {
          pe_var_kernel<BC.value, BF.value><<<dim3(cdiv(nr, 64), L), 256, 0, st>>>(ds, n, nr, w.panel, c, tc, ldt, params,
                                                                                  noise, add_noise, vo, ld_var);
        });
        return 0;
      }));
  LVAE_CHECK_LAUNCH();
  return 0;
}

size_t lvae_predict_exact_cov_workspace_size(int n, int nt, int L, int chunk) {
  if (n < 1 || nt < 0 || L < 1 || (nt > 0 && chunk < 1)) return 0;
  return ExactWs(nullptr, n, nt, L, 0, chunk, 1, true).bytes;
}

int lvae_predict_exact_cov_f64(const lvae_kernel_spec* spec, const double* x, int64_t ldx, int n, int L,
                               const double* params, const double* noise, const double* mu, int64_t ld_mu,
                               const double* tx, int64_t ldt, int nt, int n_groups, const int32_t* group_start,
                               int n_max, double* out_mean, int64_t ld_out, double* out_cov, int add_noise, int chunk,
                               int32_t* info, void* workspace, void* stream) {
  const ExactArgs a{spec, x, ldx, n, L, params, noise, mu, ld_mu, tx, ldt, nt, out_mean, ld_out, info, workspace, stream};
  LVAE_TRY(a.check(kGridL));
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
  ExactWs w(workspace, n, nt, L, 0, chunk, 1, true);
  // the factor of K (and the mean, by lvae_predict_exact_f64's own launches)
  LVAE_TRY(a.core(w));
  if (nt == 0) return 0;
  const int64_t nb = (int64_t)L * n_groups;
  pc_eye_kernel<<<nblk(nb * n_max * n_max), 256, 0, st>>>(nb, n_max, out_cov);
  // whole groups at a time, as many as fit c panel columns (the groups [g0, g1)): the panel solved in place as
  // lvae_predict_exact_var_f64's, then per launch of <= kCovBatch groups the slabs' partial tiles and their sum in
  // slab order.  A tile's slabs depend on n alone, so the bits do not depend on the chunk.
  const int c = chunk < nt ? chunk : nt, nslab = exact_cov_slabs(n);
  const DevSpec ds = to_dev(spec);
  int g0 = 0, g1 = 0;
  LVAE_TRY(a.chunks(
      w, c, false,
      [&](int c0) {
        for (g1 = g0; g1 < n_groups && group_start[g1 + 1] - group_start[g0] <= c;) ++g1;
        return group_start[g1] - c0;
      },
      [&](int c0, int, const double* tc) {
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
          pcx_partial_kernel<<<dim3(nt_b, nslab, L), 64, 0, st>>>(cb, n, w.panel, c, tile0, c, w.part);
          with_bucket(spec_bucket(spec), [&](auto BC, auto BF) {
            pcx_reduce_kernel<BC.value, BF.value><<<dim3(nt_b, L), 256, 0, st>>>(
                ds, cb, nslab, tile0, c, w.part, tc, ldt, params, noise, add_noise, b0, n_groups, n_max, out_cov);
          });
          tile0 += nt_b;
        }
        g0 = g1;
        return 0;
      }));
  LVAE_CHECK_LAUNCH();
  return 0;
}

// ---- trajectory draws ----
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
