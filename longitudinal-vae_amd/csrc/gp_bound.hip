// gp_bound.hip -- the host functions and kernels of gp_bound.hpp: what hensman.hip, dubo.hip and gp_elbo.hip share
// outside their own kernels.
#include "gp_bound.hpp"

namespace lvae {
namespace {

__global__ void bound_fill_kernel(double* p, int n, double v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// W = 1/2 ((Kz + Q) + (Kz + Q)^T)
__global__ void bound_w_kernel(int L, int M, const double* __restrict__ Kz, const double* __restrict__ Q,
                               double* __restrict__ W) {
  const int64_t MM = (int64_t)M * M;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L * MM) return;
  const int64_t b = (e / MM) * MM;
  const int i = (int)((e % MM) / M), j = (int)(e % M);
  const int64_t f = b + (int64_t)j * M + i;
  W[e] = 0.5 * ((Kz[e] + Q[e]) + (Kz[f] + Q[f]));
}

// E = I - W Y with every dot product accumulated in double-double (two-product by fma, two-sum), rounded to
// fp64 at the end, and Y1 = Y: the residual of the first inverse of W, for the one Newton step Y1 += Y E.
// W = K0zz + Q has cond ~1e8..1e9 (K0zz's jitter), so Y = spd_inv_small(W) carries a forward error of ~1e-9
// |Y|; the bound's W terms (sum iW.R, p.iW p) see it directly (2.3e-9 of the bound on the reference's golden
// vector, whose own bound is 1e-9), while a residual formed in plain fp64 is as inexact as Y itself.
__global__ void bound_resid_kernel(int L, int M, const double* __restrict__ W, const double* __restrict__ Y,
                                   double* __restrict__ E, double* __restrict__ Y1) {
#pragma clang fp contract(off)  // the error-free transforms below need every product and sum rounded on its own
  const int64_t MM = (int64_t)M * M;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L * MM) return;
  const int64_t b = (e / MM) * MM;
  const int i = (int)((e % MM) / M), j = (int)(e % M);
  const double* wr = W + b + (int64_t)i * M;
  const double* yc = Y + b + j;
  double hi = (i == j) ? 1.0 : 0.0, lo = 0.0;
  for (int k = 0; k < M; ++k) {
    const double a = -wr[k], y = yc[(int64_t)k * M];
    const double ph = a * y, pl = fma(a, y, -ph);  // a y = ph + pl exactly
    const double s = hi + ph, bb = s - hi;
    lo += ((hi - (s - bb)) + (ph - bb)) + pl;      // two-sum's error term + the product's
    hi = s;
  }
  E[e] = hi + lo;
  Y1[e] = Y[e];
}

__global__ void bound_info_kernel(int L, int P, const int32_t* __restrict__ w, int32_t* __restrict__ info) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  int v = 0;
  if (w[l]) v = 10000 + w[l];
  for (int p = 0; p < P && !v; ++p)
    if (w[L + (int64_t)l * P + p]) v = 20000 + w[L + (int64_t)l * P + p];
  if (!v && w[L + (int64_t)L * P + l]) v = 30000 + w[L + (int64_t)L * P + l];
  info[l] = v;
}

// varying T: padding rows of X -> 0, padding rows / columns of K0_p -> 0 and of B_p -> I
__global__ void bound_seg_mask_kernel(int L, int P, int T, int M, const int32_t* __restrict__ seg,
                                      double* __restrict__ X, double* __restrict__ K0st, double* __restrict__ Bst) {
  const int64_t N = (int64_t)P * T, nxz = (int64_t)L * N * M, TT = (int64_t)T * T, nst = (int64_t)L * P * TT;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < nxz) {
    const int64_t row = (e / M) % N;
    if (!bound_seg_valid(seg, (int)(row / T), (int)(row % T), T)) X[e] = 0.0;
  } else if (e < nxz + nst) {
    const int64_t f = e - nxz;
    const int p = (int)((f / TT) % P), i = (int)((f % TT) / T), j = (int)(f % T), n = bound_seg_n(seg, p, T);
    if (i >= n || j >= n) {
      K0st[f] = 0.0;
      Bst[f] = (i == j) ? 1.0 : 0.0;
    }
  }
}

__global__ void bound_seg_masked_rows_kernel(int64_t N, int L, int T, const int32_t* __restrict__ seg,
                                             const double* __restrict__ mu, double* __restrict__ mm) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N * L) return;
  const int64_t i = e / L;
  mm[e] = bound_seg_valid(seg, (int)(i / T), (int)(i % T), T) ? mu[e] : 0.0;
}

// The four Grams X [N,M], Kz [M,M], K0_p and B_p [P][T,T] as adjoint jobs.  bound_gram_part_doubles passes null
// pointers: gram_bwd_part_bytes reads the shapes alone.
void bound_bwd_jobs(const BoundDims& d, const double* x, const double* z, const double* params0,
                    const double* params1, const double* dX, const double* dKz, const double* dK0st,
                    const double* dBst, double* dparams0, double* dparams1, double* dnoise, GramBwdJob (&jobs)[4]) {
  const int M = d.M, P = d.P, T = d.T, Q = d.Q, N = P * T;
  const int64_t MM = (int64_t)M * M, TT = (int64_t)T * T, NM = (int64_t)N * M;
  const lvae_xview xv{x, 0, 0, Q}, zv{z, 0, (int64_t)M * Q, Q}, xs{x, (int64_t)T * Q, 0, Q};
  jobs[0] = {0, xv, zv, 1, N, M, 0, params0, dX, 0, NM, M, dparams0, nullptr, 0, 0};
  jobs[1] = {0, zv, zv, 1, M, M, 0, params0, dKz, 0, MM, M, dparams0, nullptr, 0, 0};
  jobs[2] = {0, xs, xs, P, T, T, 0, params0, dK0st, TT, P * TT, T, dparams0, nullptr, 0, 0};
  jobs[3] = {1, xs, xs, P, T, T, 0, params1, dBst, TT, P * TT, T, dparams1, dnoise, 0, 0};
}

}  // namespace

int bound_check(const lvae_kernel_spec* s0, const lvae_kernel_spec* s1, const BoundDims& d) {
  if (!s0 || !spec_bucket(s0)) return -1;
  if (!s1 || !spec_bucket(s1)) return -2;
  if (d.L < 1 || d.M < 1 || d.M > 128 || d.P < 1 || d.T < 1 || d.T > 128 || d.Q < 1) return -3;
  return 0;
}

size_t bound_gram_part_doubles(const BoundDims& d) {
  GramBwdJob jobs[4];
  bound_bwd_jobs(d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                 jobs);
  return gram_bwd_part_bytes(jobs, 4, d.L) / sizeof(double);
}

int bound_grams_fwd(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const BoundDims& d, const double* x,
                    const double* z, const double* params0, const double* params1, const double* noise, double eps,
                    double* epsv, double* X, double* Kz, double* K0st, double* Bst, hipStream_t st) {
  const int L = d.L, M = d.M, P = d.P, T = d.T, Q = d.Q, N = P * T;
  const int64_t MM = (int64_t)M * M, TT = (int64_t)T * T, NM = (int64_t)N * M;
  bound_fill_kernel<<<blocks(L), 256, 0, st>>>(epsv, L, eps);
  const lvae_xview xv{x, 0, 0, Q}, zv{z, 0, (int64_t)M * Q, Q}, xs{x, (int64_t)T * Q, 0, Q};
  const lvae_kernel_spec* specs[2] = {spec0, spec1};
  const GramFwdJob jobs[4] = {{0, 1, N, M, 0, 0, 0, xv, zv, params0, nullptr, X, 0, NM, M},
                              {0, 1, M, M, 0, 0, 0, zv, zv, params0, epsv, Kz, 0, MM, M},
                              {0, P, T, T, 0, 0, 0, xs, xs, params0, nullptr, K0st, TT, P * TT, T},
                              {1, P, T, T, 0, 0, 0, xs, xs, params1, noise, Bst, TT, P * TT, T}};
  return gram_multi_f64(specs, jobs, 4, L, st);
}

void bound_seg_mask(const BoundDims& d, const int32_t* seg, double* X, double* K0st, double* Bst, hipStream_t st) {
  const int64_t n = (int64_t)d.L * d.P * d.T * d.M + (int64_t)d.L * d.P * d.T * d.T;
  bound_seg_mask_kernel<<<blocks(n), 256, 0, st>>>(d.L, d.P, d.T, d.M, seg, X, K0st, Bst);
}

void bound_seg_masked_rows(const BoundDims& d, const int32_t* seg, const double* mu, double* mm, hipStream_t st) {
  const int64_t N = (int64_t)d.P * d.T;
  bound_seg_masked_rows_kernel<<<blocks(N * d.L), 256, 0, st>>>(N, d.L, d.T, seg, mu, mm);
}

int bound_grams_bwd(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const BoundDims& d, const double* x,
                    const double* z, const double* params0, const double* params1, const double* dX,
                    const double* dKz, const double* dK0st, const double* dBst, double* dparams0, double* dparams1,
                    double* dnoise, double* gpart, hipStream_t st) {
  (void)zero_async(dparams0, sizeof(double) * d.L * spec0->n_params, st);
  (void)zero_async(dparams1, sizeof(double) * d.L * spec1->n_params, st);
  if (dnoise) (void)zero_async(dnoise, sizeof(double) * d.L, st);
  GramBwdJob jobs[4];
  bound_bwd_jobs(d, x, z, params0, params1, dX, dKz, dK0st, dBst, dparams0, dparams1, dnoise, jobs);
  const lvae_kernel_spec* specs[2] = {spec0, spec1};
  return gram_bwd_multi_f64(specs, jobs, 4, d.L, gpart, st);
}

namespace {
// X [N,M] against dX, Kz [M,M] against dKz and against dKz^T as input-adjoint jobs (null pointers: the shapes alone)
void bound_z_jobs(int M, int N, int Q, const double* x, const double* z, const double* dX, const double* dKz,
                  GramX2Job (&jobs)[3]) {
  const int64_t MM = (int64_t)M * M, NM = (int64_t)N * M;
  const lvae_xview xv{x, 0, 0, Q}, zv{z, 0, (int64_t)M * Q, Q};
  jobs[0] = {xv, zv, 1, N, M, dX, 0, NM, M, 1, 0, 0, 0, 0};
  jobs[1] = {zv, zv, 1, M, M, dKz, 0, MM, M, 1, 0, 0, 0, 0};
  jobs[2] = {zv, zv, 1, M, M, dKz, 0, MM, 1, M, 0, 0, 0, 0};
}
}  // namespace

namespace {
// out = (first ? dKz : out) + h_l (S - T), h_l = GK0[l][0] / iB[l][0]: the factor the backward gave its iB term
// (g_l / 2 in the DUBO, -G_l / 2 in the ELBO), which is also the factor of T inside dKz.  Element [l][0] is row 0,
// column 0 of subject 0: with varying T (the *_seg_f64 calls) GK0 is zeroed on padding rows and columns, and this
// one is never padding because seg_len[0] >= 1 -- a mask or a reordering of the subjects must keep it so.
__global__ void bound_dkz_fix_kernel(int L, int64_t MM, int64_t PTT, int first, const double* __restrict__ dKz,
                                     const double* __restrict__ S, const double* __restrict__ T,
                                     const double* __restrict__ GK0, const double* __restrict__ iB,
                                     double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L * MM) return;
  const int64_t l = e / MM;
  const double h = GK0[l * PTT] / iB[l * PTT];
  out[e] = (first ? dKz[e] : out[e]) + h * (S[e] - T[e]);
}
}  // namespace

BoundZWs::BoundZWs(char* base, int L, int M, int N, int Q) {
  WsCarve c(base);
  part = c.take(bound_dz_part_bytes(L, M, N, Q) / sizeof(double));
  dKz = c.take((size_t)L * M * M);
  S = c.take((size_t)L * M * M);
  A = c.take((size_t)L * N * M);
  G = c.take((size_t)L * N * M);
  bytes = c.off;
}

int bound_dkz_stable(const BoundDims& d, const double* X, const double* iK, const double* iW, const double* U,
                     const double* UmZ, const double* F, const double* Bst, const double* iKQiK,
                     const double* iWRiW, const double* GK0, const double* iB, const double* dKz,
                     const BoundZWs& zw, hipStream_t st) {
  const int L = d.L, M = d.M, P = d.P, T = d.T, N = P * T;
  const int64_t MM = (int64_t)M * M, TT = (int64_t)T * T, NM = (int64_t)N * M, TM = (int64_t)T * M;
  // iK Q iK = (X iK)^T (iBK iK) = A^T (U - UmZ)
  LVAE_TRY(gemm_small_f64(0, 0, N, M, M, 1.0, X, M, NM, 0, iK, M, MM, 0, 0.0, zw.A, M, NM, 0, L, 1, st));
  LVAE_TRY(gemm_small_f64(1, 0, M, M, N, 1.0, zw.A, M, NM, 0, U, M, NM, 0, 0.0, zw.S, M, MM, 0, L, 1, st));
  LVAE_TRY(gemm_small_f64(1, 0, M, M, N, -1.0, zw.A, M, NM, 0, UmZ, M, NM, 0, 1.0, zw.S, M, MM, 0, L, 1, st));
  bound_dkz_fix_kernel<<<blocks(L * MM), 256, 0, st>>>(L, MM, P * TT, 1, dKz, zw.S, iKQiK, GK0, iB, zw.dKz);
  if (iWRiW) {
    // iW R iW = U^T D U = U^T B_p (F iW)   (F = iB D iBK)
    LVAE_TRY(gemm_small_f64(0, 0, N, M, M, 1.0, F, M, NM, 0, iW, M, MM, 0, 0.0, zw.A, M, NM, 0, L, 1, st));
    LVAE_TRY(gemm_small_f64(0, 0, T, M, T, 1.0, Bst, T, P * TT, TT, zw.A, M, NM, TM, 0.0, zw.G, M, NM, TM, L, P, st));
    LVAE_TRY(gemm_small_f64(1, 0, M, M, N, 1.0, U, M, NM, 0, zw.G, M, NM, 0, 0.0, zw.S, M, MM, 0, L, 1, st));
    bound_dkz_fix_kernel<<<blocks(L * MM), 256, 0, st>>>(L, MM, P * TT, 0, dKz, zw.S, iWRiW, GK0, iB, zw.dKz);
  }
  LVAE_CHECK_LAUNCH();
  return 0;
}

int bound_check_z(const lvae_kernel_spec* s0, const BoundDims& d) {
  LVAE_TRY(bound_check(s0, s0, d));
  for (int r = 0; r < s0->n_comp; ++r)
    for (int f = 0; f < s0->n_fac[r]; ++f)
      if (s0->dim[r][f] < 0 || s0->dim[r][f] >= (d.Q < 32 ? d.Q : 32)) return -1;  // (dz has Q columns, 32 staged)
  return 0;
}

size_t bound_dz_part_bytes(int L, int M, int N, int Q) {
  GramX2Job jobs[3];
  bound_z_jobs(M, N, Q, nullptr, nullptr, nullptr, nullptr, jobs);
  return gram_bwd_x2_part_bytes(jobs, 3, L, Q);
}

int bound_grams_bwd_z(const lvae_kernel_spec* spec0, const BoundDims& d, const double* x, const double* z,
                      const double* params0, const double* dX, const double* dKz, double* dz, double* part,
                      hipStream_t st) {
  GramX2Job jobs[3];
  bound_z_jobs(d.M, d.P * d.T, d.Q, x, z, dX, dKz, jobs);
  return gram_bwd_x2_multi_f64(spec0, jobs, 3, d.L, d.Q, params0, dz, part, st);
}

void bound_info(int L, int P, const int32_t* w, int32_t* info, hipStream_t st) {
  bound_info_kernel<<<blocks(L), 256, 0, st>>>(L, P, w, info);
}

int bound_w_inverse(int L, int M, const double* Kz, const double* Q, double* W, double* iW0, double* E, double* iW,
                    double* ldW, int32_t* info, hipStream_t st) {
  const int64_t MM = (int64_t)M * M;
  bound_w_kernel<<<blocks(L * MM), 256, 0, st>>>(L, M, Kz, Q, W);
  LVAE_TRY(spd_inv_small_f64(M, L, W, MM, iW0, MM, ldW, info, st));
  bound_resid_kernel<<<blocks(L * MM), 256, 0, st>>>(L, M, W, iW0, E, iW);
  return gemm_small_f64(0, 0, M, M, M, 1.0, iW0, M, MM, 0, E, M, MM, 0, 1.0, iW, M, MM, 0, L, 1, st);
}

}  // namespace lvae

extern "C" size_t lvae_bound_dz_workspace_size(int L, int M, int N, int Q) {
  if (L < 1 || M < 1 || N < 1 || Q < 1) return 0;
  return lvae::BoundZWs(nullptr, L, M, N, Q).bytes;
}
