// dubo.hip -- full-batch deviance upper bound (DUBO, elbo_functions.py:86-142) of all L latent dims and its
// analytic adjoint.  fp64 throughout; subjects are P blocks of T consecutive rows, N = P T.
//
// Per latent dim:
//   X = k0(x, z) [N,M]   Kz = k0(z, z) + eps I   K0_p = k0(x_p, x_p)   B_p = k1(x_p, x_p) + noise I
//   iK = Kz^-1, iB_p = B_p^-1 (+ log-dets)                                              spd_inv_small
//   iBK_p = iB_p X_p   Q = sum_p X_p^T iBK_p   R = sum_p iBK_p^T D_p iBK_p   p = sum_p iBK_p^T m_p   (D = diag e^logv)
//   W = sym(Kz + Q), iW = W^-1 (spd_inv_small + one Newton step on a double-double residual), w = iW p
//   dubo = 1/2 [ sum diag(iB) v - sum iW.R + sum_p m_p^T iB_p m_p - p.w - N - log|Kz| + sum log|B_p| + log|W|
//                - sum logv + sum iB.K0 - sum Q.iK ]
// The data-sized products (iBK, Q, R, p and the per-subject sums) are ONE pass over the subjects
// (dubo_subject_kernel): a workgroup walks kBoundS consecutive subjects with Q, R in MFMA accumulators and
// writes one partial; dubo_reduce_kernel adds the partials in group order (no atomics: bit-reproducible).
// T > 32 (X_p and iBK_p no longer fit the LDS tile) takes batched gemm_small launches instead.
//
// Adjoint (g = gdubo[l]; U = iBK iW, a = iB m - U p = Sigma^-1 m, F = iB D iBK, Z = iBK iK):
//   dmu = g a      dlogv = g/2 ((iB_ii - sum_j U_ij iBK_ij) v_i - 1)
//   dX  = g ((iBK + U R - F) iW - Z - a w^T)
//   dKz = g (-1/2 (iK - iW - iW R iW - w w^T) + 1/2 iK Q iK)      dK0_p = g/2 iB_p
//   dB_p = g/2 (iB - iB D iB - iB K0 iB - a a^T - (U - Z) iBK^T - (U R - 2 F) U^T)_p
// (dB_p is the adjoint of the dense form up to an antisymmetric part, which the symmetric Gram adjoint and the
// trace of dnoise do not see: F U^T + U F^T -> 2 F U^T.)
// (the Grams and their adjoints, the argument check, W's inverse, the info merge and the blocks of the subject walk
// that gp_elbo.hip's has too: gp_bound.hpp / gp_bound.hip; the workspace carving: common.hpp; the subject kernel
// itself: bound_subject.hpp; the workspace's layout, which dubo_cond.hip reads too: dubo_ws.hpp)
// Subjects of varying length (lvae_dubo_*_seg_f64, seg [P] valid rows of a [P, T] padded layout): the Grams are
// masked after bound_grams_fwd (padding rows of X and K0_p zero, B_p the identity there: gp_bound.hpp), every kernel
// that reads mu / logv skips the padding rows, N becomes sum_p seg[p], and the adjoint's outputs and the cotangents
// GB / GK0 are zero on the padding.  seg == NULL is the uniform call, launch for launch.
#include "bound_subject.hpp"
#include "dubo_ws.hpp"

namespace lvae {
namespace {

// The groups' partials in group order: grid (2 nt + 1, L), 256 threads.  Blocks [0, nt): a tile of Q, [nt, 2 nt):
// of R (mirrored into the upper triangle; a diagonal tile holds both of its halves itself), the last: p, scalars.
__global__ __launch_bounds__(256) void dubo_reduce_kernel(int M, int G, int nt, int64_t pstride,
                                                          const double* __restrict__ part, double* __restrict__ Q,
                                                          double* __restrict__ R, double* __restrict__ p,
                                                          double* __restrict__ scal) {
  const int b = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
  const double* pl = part + (int64_t)l * G * pstride;
  if (b < 2 * nt) {
    bound_reduce_tile(M, G, pstride, pl, b, b < nt ? b : b - nt, tid, (b < nt ? Q : R) + (int64_t)l * M * M);
  } else if (tid < 128 + 5) {
    double sum = 0.0;
    for (int g = 0; g < G; ++g) sum += pl[g * pstride + (int64_t)2 * nt * 256 + tid];
    if (tid < 128) {
      if (tid < M) p[(int64_t)l * M + tid] = sum;
    } else {
      scal[(int64_t)l * kDuboScal + tid - 128] = sum;
    }
  }
}

// the large-T route's scalar sums, one workgroup per dim: scal[l] = m.s, diag(iB).v, iB.K0, sum logv, sum log|B_p|
// (seg: the valid rows alone; mu / logv are not read on the padding)
__global__ __launch_bounds__(256) void dubo_scal_kernel(int P, int T, int L, const int32_t* __restrict__ seg,
                                                        const double* __restrict__ mu,
                                                        const double* __restrict__ logv,
                                                        const double* __restrict__ s, const double* __restrict__ iB,
                                                        const double* __restrict__ K0st,
                                                        const double* __restrict__ ldB, double* __restrict__ scal) {
  __shared__ double red[4];
  const int l = blockIdx.x, tid = threadIdx.x;
  const int64_t N = (int64_t)P * T, TT = (int64_t)P * T * T;
  double v0 = 0, v1 = 0, v2 = 0, v3 = 0, v4 = 0;
  for (int64_t i = tid; i < N; i += 256) {
    const int64_t p = i / T, q = i % T;
    if (!bound_seg_valid(seg, (int)p, (int)q, T)) continue;
    const double lv = logv[i * L + l];
    v0 += mu[i * L + l] * s[l * N + i];
    v1 += iB[l * TT + p * T * T + q * T + q] * exp(lv);
    v3 += lv;
  }
  for (int64_t e = tid; e < TT; e += 256) v2 += iB[l * TT + e] * K0st[l * TT + e];
  for (int p = tid; p < P; p += 256) v4 += ldB[(int64_t)l * P + p];
  const double vals[5] = {v0, v1, v2, v3, v4};
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const double v = block_sum<256>(vals[q], red);
    if (tid == 0) scal[(int64_t)l * kDuboScal + q] = v;
  }
}

// Y[l][i][:] = exp(logv[i][l]) X[l][i][:]   ([L,N,M]; seg: 0 on the padding rows, whose logv is not read)
__global__ void dubo_rowscale_nm_kernel(int64_t N, int M, int L, int T, const int32_t* __restrict__ seg,
                                        const double* __restrict__ logv,
                                        const double* __restrict__ X, double* __restrict__ Y) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)L * N * M) return;
  const int64_t l = e / (N * M), i = (e / M) % N;
  Y[e] = bound_seg_valid(seg, (int)(i / T), (int)(i % T), T) ? exp(logv[i * L + l]) * X[e] : 0.0;
}

// dubo[l] from the reduced sums, one workgroup per dim (seg: N = sum_p seg[p] of the P subjects, else n_rows)
__global__ __launch_bounds__(256) void dubo_final_kernel(int M, double n_rows, int P, int T,
                                                         const int32_t* __restrict__ seg,
                                                         const double* __restrict__ iW,
                                                         const double* __restrict__ R, const double* __restrict__ Q,
                                                         const double* __restrict__ iK, const double* __restrict__ p,
                                                         const double* __restrict__ w,
                                                         const double* __restrict__ scal,
                                                         const double* __restrict__ ldK,
                                                         const double* __restrict__ ldW, double* __restrict__ dubo) {
  __shared__ double red[4];
  const int l = blockIdx.x, tid = threadIdx.x;
  const int64_t MM = (int64_t)M * M;
  double a = 0, b = 0, c = 0;
  for (int64_t e = tid; e < MM; e += 256) {
    a += iW[l * MM + e] * R[l * MM + e];
    b += Q[l * MM + e] * iK[l * MM + e];
  }
  for (int i = tid; i < M; i += 256) c += p[(int64_t)l * M + i] * w[(int64_t)l * M + i];
  a = block_sum<256>(a, red);
  b = block_sum<256>(b, red);
  c = block_sum<256>(c, red);
  if (seg) n_rows = bound_seg_rows(seg, P, T, tid, red);
  if (tid == 0) {
    const double* sc = scal + (int64_t)l * kDuboScal;
    dubo[l] = 0.5 * ((sc[1] - a) + (sc[0] - c) - n_rows + (-ldK[l] + sc[4] + ldW[l]) - sc[3] + (sc[2] - b));
  }
}

// a = s - y;  dmu[i][l] = g_l a   (seg: both exact 0 on the padding rows)
__global__ void dubo_a_kernel(int64_t N, int L, int T, const int32_t* __restrict__ seg,
                              const double* __restrict__ g, const double* __restrict__ s,
                              const double* __restrict__ y, double* __restrict__ a, double* __restrict__ dmu) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N * L) return;
  const int64_t l = e / N, i = e % N;
  const bool ok = bound_seg_valid(seg, (int)(i / T), (int)(i % T), T);
  const double v = ok ? s[e] - y[e] : 0.0;
  a[e] = v;
  dmu[i * L + l] = ok ? g[l] * v : 0.0;
}

// dlogv[i][l] = g_l / 2 ((iB_ii - sum_j U_ij iBK_ij) v_i - 1): one wave per row (seg: 0 on the padding rows, whose
// logv is not read)
__global__ __launch_bounds__(256) void dubo_dlogv_kernel(int P, int T, int M, int L,
                                                         const int32_t* __restrict__ seg,
                                                         const double* __restrict__ g,
                                                         const double* __restrict__ U,
                                                         const double* __restrict__ iBK,
                                                         const double* __restrict__ iB,
                                                         const double* __restrict__ logv,
                                                         double* __restrict__ dlogv) {
  const int64_t N = (int64_t)P * T;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= N * L) return;
  const int64_t l = row / N, i = row % N, p = i / T, q = i % T;
  if (!bound_seg_valid(seg, (int)p, (int)q, T)) {  // (wave-uniform: a wave has one row)
    if (lane == 0) dlogv[i * L + l] = 0.0;
    return;
  }
  double sum = 0.0;
  for (int j = lane; j < M; j += 64) sum += U[row * M + j] * iBK[row * M + j];
  sum = wave_sum(sum);
  if (lane == 0) {
    const double d = iB[((l * P + p) * T + q) * T + q];
    dlogv[i * L + l] = 0.5 * g[l] * ((d - sum) * exp(logv[i * L + l]) - 1.0);
  }
}

// tNM = iBK + UR - F
__global__ void dubo_sum3_kernel(int64_t n, const double* __restrict__ iBK, const double* __restrict__ UR,
                                 const double* __restrict__ F, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) out[e] = iBK[e] + UR[e] - F[e];
}

// dX = g_l (dX - Z - a w^T);  Z <- U - Z;  UR <- UR - 2 F
__global__ void dubo_dx_kernel(int64_t N, int M, int L, const double* __restrict__ g, const double* __restrict__ a,
                               const double* __restrict__ w, const double* __restrict__ U,
                               const double* __restrict__ F, double* __restrict__ Z, double* __restrict__ UR,
                               double* __restrict__ dX) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)L * N * M) return;
  const int64_t l = e / (N * M), i = (e / M) % N, j = e % M;
  const double z = Z[e];
  dX[e] = g[l] * (dX[e] - z - a[l * N + i] * w[l * M + j]);
  Z[e] = U[e] - z;
  UR[e] = UR[e] - 2.0 * F[e];
}

// dKz = g_l (-1/2 (iK - iW - iW R iW - w w^T) + 1/2 iK Q iK)
__global__ void dubo_dkz_kernel(int L, int M, const double* __restrict__ g, const double* __restrict__ iK,
                                const double* __restrict__ iW, const double* __restrict__ iWRiW,
                                const double* __restrict__ w, const double* __restrict__ iKQiK,
                                double* __restrict__ dKz) {
  const int64_t MM = (int64_t)M * M;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L * MM) return;
  const int64_t l = e / MM;
  const int i = (int)((e % MM) / M), j = (int)(e % M);
  dKz[e] = 0.5 * g[l] * (iW[e] + iWRiW[e] + w[l * M + i] * w[l * M + j] - iK[e] + iKQiK[e]);
}

// VB[l,p][i][j] = v_{l,p,i} iB[l,p][i][j]   (seg: v = 0 on the padding rows, whose logv is not read)
__global__ void dubo_rowscale_tt_kernel(int P, int T, int L, const int32_t* __restrict__ seg,
                                        const double* __restrict__ logv,
                                        const double* __restrict__ iB, double* __restrict__ VB) {
  const int64_t TT = (int64_t)T * T;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)L * P * TT) return;
  const int64_t lp = e / TT, l = lp / P, p = lp % P;
  const int i = (int)((e % TT) / T);
  VB[e] = bound_seg_valid(seg, (int)p, i, T) ? exp(logv[(p * T + i) * L + l]) * iB[e] : 0.0;
}

// GB = g_l / 2 (iB - iBDiB - iBK0iB - a a^T - GB);  GK0 = g_l / 2 iB
// (lvae_dubo_bwd_z_f64 reads g_l / 2 back as GK0[l][0] / iB[l][0], bound_dkz_fix_kernel: keep GK0 = (g_l / 2) iB)
// seg: both are 0 on padding rows and columns -- iB's identity there must reach neither dnoise (through dB's trace)
// nor dparams0 (through K0's diagonal).  Element (0, 0) of subject 0 is valid (seg[0] >= 1), so the read-back holds.
__global__ void dubo_gb_kernel(int P, int T, int L, const int32_t* __restrict__ seg, const double* __restrict__ g,
                               const double* __restrict__ iB,
                               const double* __restrict__ a, const double* __restrict__ iBDiB,
                               const double* __restrict__ iBK0iB, double* __restrict__ GB,
                               double* __restrict__ GK0) {
  const int64_t TT = (int64_t)T * T, N = (int64_t)P * T;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)L * P * TT) return;
  const int64_t lp = e / TT, l = lp / P, p = lp % P;
  const int i = (int)((e % TT) / T), j = (int)(e % T);
  const int n = bound_seg_n(seg, (int)p, T);
  if (i >= n || j >= n) {
    GB[e] = 0.0;
    GK0[e] = 0.0;
    return;
  }
  const double h = 0.5 * g[l];
  const double ai = a[l * N + p * T + i], aj = a[l * N + p * T + j];
  GB[e] = h * (iB[e] - iBDiB[e] - iBK0iB[e] - ai * aj - GB[e]);
  GK0[e] = h * iB[e];
}

}  // namespace
}  // namespace lvae

using namespace lvae;

extern "C" {

size_t lvae_dubo_workspace_size(const lvae_dubo_dims* d) { return DWs(nullptr, *d).bytes; }

// (seg == NULL is the uniform call: the same launches with the same arguments as before there was a seg)
int lvae_dubo_fwd_seg_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const lvae_dubo_dims* dp,
                          const int32_t* seg, const double* x, const double* z, const double* mu, const double* logv,
                          const double* params0, const double* params1, const double* noise, double* dubo,
                          int32_t* info, void* workspace, void* stream) {
  const BoundDims bd = dubo_dims(dp);
  LVAE_TRY(bound_check(spec0, spec1, bd));
  if (!workspace || ((uintptr_t)workspace & 255)) return -4;
  hipStream_t st = (hipStream_t)stream;
  const lvae_dubo_dims& d = *dp;
  const int L = d.L, M = d.M, P = d.P, T = d.T, N = P * T;
  const int64_t MM = (int64_t)M * M, TT = (int64_t)T * T, NM = (int64_t)N * M;
  DWs w((char*)workspace, d);
  LVAE_TRY(bound_grams_fwd(spec0, spec1, bd, x, z, params0, params1, noise, d.eps, w.epsv, w.X, w.Kz, w.K0st, w.Bst,
                           st));
  if (seg) bound_seg_mask(bd, seg, w.X, w.K0st, w.Bst, st);
  LVAE_TRY(spd_inv_small_f64(M, L, w.Kz, MM, w.iK, MM, w.ldK, w.info, st));
  LVAE_TRY(spd_inv_small_f64(T, L * P, w.Bst, TT, w.iB, TT, w.ldB, w.info + L, st));
  if (T <= kBoundT) {
    const int G = bound_groups(P), nt = bound_tiles(M);
    const int64_t ps = dubo_part_stride(M);
    if (seg)
      dubo_subject_seg_launch(dim3(G, L), st, M, P, T, L, nt, ps, w.X, w.iB, w.K0st, w.ldB, mu, logv, w.iBK, w.part,
                              seg);
    else
      dubo_subject_kernel<><<<dim3(G, L), 512, 0, st>>>(M, P, T, L, nt, ps, w.X, w.iB, w.K0st, w.ldB, mu, logv, w.iBK,
                                                       w.part);
    dubo_reduce_kernel<<<dim3(2 * nt + 1, L), 256, 0, st>>>(M, G, nt, ps, w.part, w.Q, w.R, w.p, w.scal);
  } else {
    // large T: iBK, Q, R = iBK^T (D iBK), p = iBK^T m, s = iB m as batched products
    // (seg: m as a masked copy in UR, idle until the backward -- 0 * NaN from a padding row would be NaN)
    const double* mm = mu;
    if (seg) {
      bound_seg_masked_rows(bd, seg, mu, w.UR, st);
      mm = w.UR;
    }
    LVAE_TRY(gemm_small_f64(0, 0, T, M, T, 1.0, w.iB, T, P * TT, TT, w.X, M, NM, (int64_t)T * M, 0.0, w.iBK, M, NM,
                            (int64_t)T * M, L, P, st));
    LVAE_TRY(gemm_small_f64(1, 0, M, M, N, 1.0, w.X, M, NM, 0, w.iBK, M, NM, 0, 0.0, w.Q, M, MM, 0, L, 1, st));
    dubo_rowscale_nm_kernel<<<blocks((int64_t)L * NM), 256, 0, st>>>(N, M, L, T, seg, logv, w.iBK, w.tNM);
    LVAE_TRY(gemm_small_f64(1, 0, M, M, N, 1.0, w.iBK, M, NM, 0, w.tNM, M, NM, 0, 0.0, w.R, M, MM, 0, L, 1, st));
    LVAE_TRY(gemm_small_f64(1, 0, M, 1, N, 1.0, w.iBK, M, NM, 0, mm, L, 1, 0, 0.0, w.p, 1, M, 0, L, 1, st));
    LVAE_TRY(gemm_small_f64(0, 0, T, 1, T, 1.0, w.iB, T, P * TT, TT, mm, L, 1, (int64_t)T * L, 0.0, w.s, 1, N, T, L, P,
                            st));
    dubo_scal_kernel<<<L, 256, 0, st>>>(P, T, L, seg, mu, logv, w.s, w.iB, w.K0st, w.ldB, w.scal);
  }
  LVAE_TRY(bound_w_inverse(L, M, w.Kz, w.Q, w.W, w.iW0, w.E, w.iW, w.ldW, w.info + L + L * P, st));
  LVAE_TRY(gemm_small_f64(0, 0, M, 1, M, 1.0, w.iW, M, MM, 0, w.p, 1, M, 0, 0.0, w.w, 1, M, 0, L, 1, st));
  dubo_final_kernel<<<L, 256, 0, st>>>(M, (double)N, P, T, seg, w.iW, w.R, w.Q, w.iK, w.p, w.w, w.scal, w.ldK, w.ldW, dubo);
  if (info) bound_info(L, P, w.info, info, st);
  LVAE_CHECK_LAUNCH();
  return 0;
}

int lvae_dubo_fwd_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const lvae_dubo_dims* dp,
                      const double* x, const double* z, const double* mu, const double* logv, const double* params0,
                      const double* params1, const double* noise, double* dubo, int32_t* info, void* workspace,
                      void* stream) {
  return lvae_dubo_fwd_seg_f64(spec0, spec1, dp, nullptr, x, z, mu, logv, params0, params1, noise, dubo, info,
                               workspace, stream);
}

int lvae_dubo_bwd_seg_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const lvae_dubo_dims* dp,
                          const int32_t* seg, const double* x, const double* z, const double* mu, const double* logv,
                          const double* params0, const double* params1, const double* noise, const double* gdubo,
                          double* dmu, double* dlogv, double* dparams0, double* dparams1, double* dnoise,
                          void* workspace, void* stream) {
  (void)noise;
  const BoundDims bd = dubo_dims(dp);
  LVAE_TRY(bound_check(spec0, spec1, bd));
  if (!workspace || ((uintptr_t)workspace & 255)) return -4;
  hipStream_t st = (hipStream_t)stream;
  const lvae_dubo_dims& d = *dp;
  const int L = d.L, M = d.M, P = d.P, T = d.T, N = P * T;
  const int64_t MM = (int64_t)M * M, TT = (int64_t)T * T, NM = (int64_t)N * M, LTT = (int64_t)L * P * TT;
  const int64_t TM = (int64_t)T * M;
  DWs w((char*)workspace, d);
  // U = iBK iW ; s = iB m ; y = U p ; a = s - y -> dmu ; dlogv
  LVAE_TRY(gemm_small_f64(0, 0, N, M, M, 1.0, w.iBK, M, NM, 0, w.iW, M, MM, 0, 0.0, w.U, M, NM, 0, L, 1, st));
  // (seg: m as a masked copy in dX, which this call only forms further down)
  const double* mm = mu;
  if (seg) {
    bound_seg_masked_rows(bd, seg, mu, w.dX, st);
    mm = w.dX;
  }
  LVAE_TRY(gemm_small_f64(0, 0, T, 1, T, 1.0, w.iB, T, P * TT, TT, mm, L, 1, (int64_t)T * L, 0.0, w.s, 1, N, T, L, P,
                          st));
  LVAE_TRY(gemm_small_f64(0, 0, N, 1, M, 1.0, w.U, M, NM, 0, w.p, 1, M, 0, 0.0, w.y, 1, N, 0, L, 1, st));
  dubo_a_kernel<<<blocks((int64_t)N * L), 256, 0, st>>>(N, L, T, seg, gdubo, w.s, w.y, w.a, dmu);
  dubo_dlogv_kernel<<<cdiv((int64_t)N * L, 4), 256, 0, st>>>(P, T, M, L, seg, gdubo, w.U, w.iBK, w.iB, logv, dlogv);
  // UR = U R ; F = iB (D iBK) ; Z = iBK iK ; dX = (iBK + UR - F) iW, then g (dX - Z - a w^T)
  LVAE_TRY(gemm_small_f64(0, 0, N, M, M, 1.0, w.U, M, NM, 0, w.R, M, MM, 0, 0.0, w.UR, M, NM, 0, L, 1, st));
  dubo_rowscale_nm_kernel<<<blocks((int64_t)L * NM), 256, 0, st>>>(N, M, L, T, seg, logv, w.iBK, w.tNM);
  LVAE_TRY(gemm_small_f64(0, 0, T, M, T, 1.0, w.iB, T, P * TT, TT, w.tNM, M, NM, TM, 0.0, w.F, M, NM, TM, L, P, st));
  LVAE_TRY(gemm_small_f64(0, 0, N, M, M, 1.0, w.iBK, M, NM, 0, w.iK, M, MM, 0, 0.0, w.Z, M, NM, 0, L, 1, st));
  dubo_sum3_kernel<<<blocks((int64_t)L * NM), 256, 0, st>>>((int64_t)L * NM, w.iBK, w.UR, w.F, w.tNM);
  LVAE_TRY(gemm_small_f64(0, 0, N, M, M, 1.0, w.tNM, M, NM, 0, w.iW, M, MM, 0, 0.0, w.dX, M, NM, 0, L, 1, st));
  // dKz's two sandwiches from their N x M factors (tNM is free again, Z still iBK iK): iK Q iK = (X iK)^T Z and
  // iW R iW = U^T (D U).  As (iK Q) iK and (iW R) iW they carry the rounding of the inner product times |iK| ~ 1 / eps
  // (|iW| less so), which a derivative of Kz that oscillates over the inducing points (a period's) does not average
  // out -- ten times the oracle's own error in dparams0 at cond(Kz) ~ 5e4
  LVAE_TRY(gemm_small_f64(0, 0, N, M, M, 1.0, w.X, M, NM, 0, w.iK, M, MM, 0, 0.0, w.tNM, M, NM, 0, L, 1, st));
  LVAE_TRY(gemm_small_f64(1, 0, M, M, N, 1.0, w.tNM, M, NM, 0, w.Z, M, NM, 0, 0.0, w.iKQiK, M, MM, 0, L, 1, st));
  dubo_rowscale_nm_kernel<<<blocks((int64_t)L * NM), 256, 0, st>>>(N, M, L, T, seg, logv, w.U, w.tNM);
  LVAE_TRY(gemm_small_f64(1, 0, M, M, N, 1.0, w.U, M, NM, 0, w.tNM, M, NM, 0, 0.0, w.iWRiW, M, MM, 0, L, 1, st));
  dubo_dx_kernel<<<blocks((int64_t)L * NM), 256, 0, st>>>(N, M, L, gdubo, w.a, w.w, w.U, w.F, w.Z, w.UR, w.dX);
  // dKz
  dubo_dkz_kernel<<<blocks(L * MM), 256, 0, st>>>(L, M, gdubo, w.iK, w.iW, w.iWRiW, w.w, w.iKQiK, w.dKz);
  // dB_p, dK0_p (Z now holds U - Z, UR holds UR - 2 F)
  dubo_rowscale_tt_kernel<<<blocks(LTT), 256, 0, st>>>(P, T, L, seg, logv, w.iB, w.VB);
  LVAE_TRY(gemm_small_f64(0, 0, T, T, T, 1.0, w.iB, T, P * TT, TT, w.VB, T, P * TT, TT, 0.0, w.iBDiB, T, P * TT, TT,
                          L, P, st));
  LVAE_TRY(gemm_small_f64(0, 0, T, T, T, 1.0, w.K0st, T, P * TT, TT, w.iB, T, P * TT, TT, 0.0, w.K0iB, T, P * TT, TT,
                          L, P, st));
  LVAE_TRY(gemm_small_f64(0, 0, T, T, T, 1.0, w.iB, T, P * TT, TT, w.K0iB, T, P * TT, TT, 0.0, w.iBK0iB, T, P * TT,
                          TT, L, P, st));
  LVAE_TRY(gemm_small_f64(0, 1, T, T, M, 1.0, w.Z, M, NM, TM, w.iBK, M, NM, TM, 0.0, w.GB, T, P * TT, TT, L, P, st));
  LVAE_TRY(gemm_small_f64(0, 1, T, T, M, 1.0, w.UR, M, NM, TM, w.U, M, NM, TM, 1.0, w.GB, T, P * TT, TT, L, P, st));
  dubo_gb_kernel<<<blocks(LTT), 256, 0, st>>>(P, T, L, seg, gdubo, w.iB, w.a, w.iBDiB, w.iBK0iB, w.GB, w.GK0);
  // hyper-parameter gradients through the four Grams
  LVAE_TRY(bound_grams_bwd(spec0, spec1, bd, x, z, params0, params1, w.dX, w.dKz, w.GK0, w.GB, dparams0, dparams1,
                           dnoise, w.gpart, st));
  LVAE_CHECK_LAUNCH();
  return 0;
}

int lvae_dubo_bwd_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const lvae_dubo_dims* dp,
                      const double* x, const double* z, const double* mu, const double* logv, const double* params0,
                      const double* params1, const double* noise, const double* gdubo, double* dmu, double* dlogv,
                      double* dparams0, double* dparams1, double* dnoise, void* workspace, void* stream) {
  return lvae_dubo_bwd_seg_f64(spec0, spec1, dp, nullptr, x, z, mu, logv, params0, params1, noise, gdubo, dmu, dlogv,
                               dparams0, dparams1, dnoise, workspace, stream);
}

// dz from the dX / dKz lvae_dubo_bwd_f64 left in the workspace (gdubo[l] is already inside them).  After a
// lvae_dubo_bwd_seg_f64 nothing changes: the padding rows of dX are exact zeros.
int lvae_dubo_bwd_z_f64(const lvae_kernel_spec* spec0, const lvae_dubo_dims* dp, const double* x, const double* z,
                        const double* params0, double* dz, void* workspace, void* zworkspace, void* stream) {
  const BoundDims bd = dubo_dims(dp);
  LVAE_TRY(bound_check_z(spec0, bd));
  if (!workspace || ((uintptr_t)workspace & 255)) return -4;
  if (!zworkspace || ((uintptr_t)zworkspace & 255)) return -5;
  hipStream_t st = (hipStream_t)stream;
  DWs w((char*)workspace, *dp);
  BoundZWs zw((char*)zworkspace, bd.L, bd.M, bd.P * bd.T, bd.Q);
  // (w.Z holds U - iBK iK and w.F, w.iWRiW, w.iKQiK, w.GK0 what the backward left)
  LVAE_TRY(bound_dkz_stable(bd, w.X, w.iK, w.iW, w.U, w.Z, w.F, w.Bst, w.iKQiK, w.iWRiW, w.GK0, w.iB, w.dKz, zw, st));
  return bound_grams_bwd_z(spec0, bd, x, z, params0, w.dX, zw.dKz, dz, zw.part, st);
}

}  // extern "C"
