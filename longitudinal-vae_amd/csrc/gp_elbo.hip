// gp_elbo.hip -- full-batch sampled GP ELBO (type_KL 'GPapprox', elbo_functions.py:36-84) of all L latent dims and
// all S samples of the latent, and its analytic adjoint.  fp64 throughout; subjects are P blocks of T consecutive
// rows, N = P T.  The notation is dubo.hip's; what the two share (and share with hensman.hip) is gp_bound.hpp /
// gp_bound.hip; the subject kernel itself is in bound_subject.hpp.  Subjects of varying length
// (lvae_gp_elbo_*_seg_f64): as dubo.hip's -- masked Grams, y read on the valid rows only, N = sum_p seg[p], dy and
// the cotangents GB / GK0 zero on the padding; seg == NULL is the uniform call, launch for launch.
//
// Per latent dim (nothing here depends on the sample):
//   X = k0(x, z) [N,M]   Kz = k0(z, z) + eps I   K0_p = k0(x_p, x_p)   B_p = k1(x_p, x_p) + noise I
//   iK = Kz^-1, iB_p = B_p^-1 (+ log-dets)   iBK_p = iB_p X_p   Q = sum_p X_p^T iBK_p
//   W = sym(Kz + Q), iW = W^-1 (spd_inv_small + one Newton step on a double-double residual)
// Per sample s (right-hand sides only; the samples are the <= 16 columns of one MFMA tile):
//   p_s = sum_p iBK_p^T y_{p,s}   w_s = iW p_s   q_s = sum_p y_{p,s}^T iB_p y_{p,s} - p_s.w_s
//   elbo[s][l] = -N/2 log 2 pi - 1/2 (-log|Kz| + sum_p log|B_p| + log|W| + q_s) - 1/2 (sum iB.K0 - sum Q.iK)
// The data-sized products (iBK, Q, Pm = [p_s], s_p = iB_p Y_p, the sums) are ONE pass over the subjects
// (gp_elbo_subject_kernel): a workgroup walks kBoundS consecutive subjects with Q and Pm in MFMA accumulators and
// writes one partial; gp_elbo_reduce_kernel adds the partials in group order (no atomics: bit-reproducible).
// T > 32 takes batched gemm_small launches instead.
//
// Adjoint (g_s = gelbo[s][l], G = sum_s g_s; U = iBK iW, Z = iBK iK, a_s = iB y_s - U p_s, A = [a_s], Wm = [w_s],
// Gam = diag(g_s)): minus the DUBO's at R = F = 0, the sample terms as rank-S products
//   dy_s  = -g_s a_s
//   dX    = A Gam Wm^T - G (U - Z)
//   dKz   = -1/2 (G (iW - iK + iK Q iK) + Wm Gam Wm^T)      dK0_p = -G/2 iB_p
//   dB_p  = -1/2 (G (iB - iB K0 iB - (U - Z) iBK^T) - A Gam A^T)_p
#include "bound_subject.hpp"

namespace lvae {
namespace {

constexpr int kGeScal = 24;   // scalar slots per dim: 0 sum iB.K0, 1 sum log|B_p|, 8 + s: sum_p y_s^T iB_p y_s
constexpr double kHalfLog2Pi = 0.91893853320467274178;

// doubles of one (dim, group) partial: Q's lower tiles in accumulator order, Pm [128][16], the scalars
inline int64_t ge_part_stride(int M) { return (int64_t)bound_tiles(M) * 256 + 128 * kGeS + kGeScal; }

// (a null d: all zero, which bound_check answers with -3)
inline BoundDims ge_dims(const lvae_gp_elbo_dims* d) {
  return d ? BoundDims{d->L, d->M, d->P, d->T, d->Q} : BoundDims{};
}

// (iKQ: unused, as in dubo_ws.hpp's DWs; lvae_gp_elbo_workspace_size stays what it was)
struct GWs {
  double *X, *iBK, *U, *Z, *dX;                                   // [L,N,M]
  double *Kz, *iK, *Q, *W, *iW0, *E, *iW, *iKQ, *iKQiK, *dKz;     // [L,M,M]
  double *K0st, *Bst, *iB, *K0iB, *iBK0iB, *GB, *AAt, *GK0;       // [L,P,T,T]
  double *Pm, *Wm, *WG;                                           // [L,M,16]
  double *Yp, *s, *A, *AG;                                        // [L,N,16]
  double *ldK, *ldB, *ldW, *epsv, *scal, *Gs, *part, *gpart;
  int32_t* info;
  size_t bytes;
  GWs(char* base, const lvae_gp_elbo_dims& d) {
    WsCarve c(base);
    const size_t L = d.L, M = d.M, N = (size_t)d.P * d.T, TT = (size_t)d.P * d.T * d.T;
    double** nm[] = {&X, &iBK, &U, &Z, &dX};
    for (auto q : nm) *q = c.take(L * N * M);
    double** mm[] = {&Kz, &iK, &Q, &W, &iW0, &E, &iW, &iKQ, &iKQiK, &dKz};
    for (auto q : mm) *q = c.take(L * M * M);
    double** tt[] = {&K0st, &Bst, &iB, &K0iB, &iBK0iB, &GB, &AAt, &GK0};
    for (auto q : tt) *q = c.take(L * TT);
    double** ms[] = {&Pm, &Wm, &WG};
    for (auto q : ms) *q = c.take(L * M * kGeS);
    double** ns[] = {&Yp, &s, &A, &AG};
    for (auto q : ns) *q = c.take(L * N * kGeS);
    ldK = c.take(L);
    ldB = c.take(L * d.P);
    ldW = c.take(L);
    epsv = c.take(L);
    scal = c.take(L * kGeScal);
    Gs = c.take(L);
    part = c.take(L * (size_t)bound_groups(d.P) * (size_t)ge_part_stride(d.M));
    info = (int32_t*)c.take(L * (2 + (size_t)d.P));
    gpart = c.take(bound_gram_part_doubles(ge_dims(&d)));
    bytes = c.off;
  }
};

// The groups' partials in group order: grid (nt + 9, L), 256 threads.  Blocks [0, nt): a tile of Q (mirrored into
// the upper triangle; a diagonal tile holds both of its halves itself), the next 8: 16 rows of Pm [M][16] each
// (one element a thread), the last: the scalars.
__global__ __launch_bounds__(256) void gp_elbo_reduce_kernel(int M, int G, int nt, int64_t pstride,
                                                             const double* __restrict__ part,
                                                             double* __restrict__ Q, double* __restrict__ Pm,
                                                             double* __restrict__ scal) {
  const int b = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
  const double* pl = part + (int64_t)l * G * pstride;
  if (b < nt) {
    bound_reduce_tile(M, G, pstride, pl, b, b, tid, Q + (int64_t)l * M * M);
  } else if (b < nt + 8) {
    const int e = (b - nt) * 256 + tid;
    if (e < M * kGeS) {
      double sum = 0.0;
      for (int g = 0; g < G; ++g) sum += pl[g * pstride + (int64_t)nt * 256 + e];
      Pm[(int64_t)l * M * kGeS + e] = sum;
    }
  } else if (tid < 2 || (tid >= 8 && tid < kGeScal)) {
    double sum = 0.0;
    for (int g = 0; g < G; ++g) sum += pl[g * pstride + (int64_t)nt * 256 + 128 * kGeS + tid];
    scal[(int64_t)l * kGeScal + tid] = sum;
  }
}

// the large-T route: Yp[l][i][s] = y[s][i][l], columns S.. zero (seg: the padding rows too, whose y is not read)
__global__ void gp_elbo_pack_kernel(int64_t N, int L, int S, int T, const int32_t* __restrict__ seg,
                                    const double* __restrict__ y, double* __restrict__ Yp) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)L * N * kGeS) return;
  const int64_t l = e / (N * kGeS), i = (e / kGeS) % N;
  const int s = (int)(e % kGeS);
  Yp[e] = (s < S && bound_seg_valid(seg, (int)(i / T), (int)(i % T), T)) ? y[((int64_t)s * N + i) * L + l] : 0.0;
}

// the large-T route's scalar sums, one workgroup per dim (thread = (row phase, sample column))
__global__ __launch_bounds__(256) void gp_elbo_scal_kernel(int P, int T, const double* __restrict__ Yp,
                                                           const double* __restrict__ sbuf,
                                                           const double* __restrict__ iB,
                                                           const double* __restrict__ K0st,
                                                           const double* __restrict__ ldB,
                                                           double* __restrict__ scal) {
  __shared__ double red[4];
  __shared__ double sq[256];
  const int l = blockIdx.x, tid = threadIdx.x;
  const int64_t N = (int64_t)P * T, TT = (int64_t)P * T * T;
  double v = 0.0, v0 = 0.0, v1 = 0.0;
  for (int64_t e = tid; e < N * kGeS; e += 256) v += Yp[l * N * kGeS + e] * sbuf[l * N * kGeS + e];
  for (int64_t e = tid; e < TT; e += 256) v0 += iB[l * TT + e] * K0st[l * TT + e];
  for (int p = tid; p < P; p += 256) v1 += ldB[(int64_t)l * P + p];
  sq[tid] = v;
  v0 = block_sum<256>(v0, red);
  v1 = block_sum<256>(v1, red);
  if (tid == 0) {
    scal[(int64_t)l * kGeScal] = v0;
    scal[(int64_t)l * kGeScal + 1] = v1;
  }
  if (tid < kGeS) {
    double sum = 0.0;
    for (int r = 0; r < 16; ++r) sum += sq[r * 16 + tid];
    scal[(int64_t)l * kGeScal + 8 + tid] = sum;
  }
}

// elbo[s][l] from the reduced sums, one workgroup per dim (seg: N = sum_p seg[p] of the P subjects, else n_rows)
__global__ __launch_bounds__(256) void gp_elbo_final_kernel(int M, int L, int S, double n_rows, int P, int T,
                                                            const int32_t* __restrict__ seg,
                                                            const double* __restrict__ Q,
                                                            const double* __restrict__ iK,
                                                            const double* __restrict__ Pm,
                                                            const double* __restrict__ Wm,
                                                            const double* __restrict__ scal,
                                                            const double* __restrict__ ldK,
                                                            const double* __restrict__ ldW,
                                                            double* __restrict__ elbo) {
  __shared__ double red[4];
  __shared__ double sq[256];
  const int l = blockIdx.x, tid = threadIdx.x;
  const int64_t MM = (int64_t)M * M;
  double b = 0.0, c = 0.0;
  for (int64_t e = tid; e < MM; e += 256) b += Q[l * MM + e] * iK[l * MM + e];
  for (int e = tid; e < M * kGeS; e += 256) c += Pm[(int64_t)l * M * kGeS + e] * Wm[(int64_t)l * M * kGeS + e];
  sq[tid] = c;
  b = block_sum<256>(b, red);
  if (seg) n_rows = bound_seg_rows(seg, P, T, tid, red);
  if (tid < S) {
    double pw = 0.0;
    for (int r = 0; r < 16; ++r) pw += sq[r * 16 + tid];
    const double* sc = scal + (int64_t)l * kGeScal;
    const double logdet = -ldK[l] + sc[1] + ldW[l];
    elbo[(int64_t)tid * L + l] = -n_rows * kHalfLog2Pi - 0.5 * (logdet + (sc[8 + tid] - pw)) - 0.5 * (sc[0] - b);
  }
}

// Gs[l] = sum_s g[s][l];  WG[l][i][s] = g[s][l] Wm[l][i][s] (columns S.. zero)
__global__ void gp_elbo_g_kernel(int L, int M, int S, const double* __restrict__ g, const double* __restrict__ Wm,
                                 double* __restrict__ WG, double* __restrict__ Gs) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)L * M * kGeS) return;
  const int l = (int)(e / ((int64_t)M * kGeS)), s = (int)(e % kGeS);
  WG[e] = s < S ? g[(int64_t)s * L + l] * Wm[e] : 0.0;
  if (e % ((int64_t)M * kGeS) == 0) {
    double sum = 0.0;
    for (int q = 0; q < S; ++q) sum += g[(int64_t)q * L + l];
    Gs[l] = sum;
  }
}

// A = s - U Pm (A holds U Pm on entry);  AG = A Gam;  dy[s][i][l] = -g[s][l] A[l][i][s]
// (seg: A, AG and dy are exact 0 on the padding rows)
__global__ void gp_elbo_a_kernel(int64_t N, int L, int S, int T, const int32_t* __restrict__ seg,
                                 const double* __restrict__ g,
                                 const double* __restrict__ sbuf, double* __restrict__ A, double* __restrict__ AG,
                                 double* __restrict__ dy) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)L * N * kGeS) return;
  const int64_t l = e / (N * kGeS), i = (e / kGeS) % N;
  const int s = (int)(e % kGeS);
  if (!bound_seg_valid(seg, (int)(i / T), (int)(i % T), T)) {
    A[e] = 0.0;
    AG[e] = 0.0;
    if (s < S) dy[((int64_t)s * N + i) * L + l] = 0.0;
    return;
  }
  const double a = sbuf[e] - A[e];
  A[e] = a;
  if (s < S) {
    const double ga = g[(int64_t)s * L + l] * a;
    AG[e] = ga;
    dy[((int64_t)s * N + i) * L + l] = -ga;
  } else {
    AG[e] = 0.0;
  }
}

// Z <- U - Z;  dX = dX - G_l Z   (dX holds A Gam Wm^T on entry)
__global__ void gp_elbo_dx_kernel(int64_t NM, int L, const double* __restrict__ Gs, const double* __restrict__ U,
                                  double* __restrict__ Z, double* __restrict__ dX) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L * NM) return;
  const double z = U[e] - Z[e];
  Z[e] = z;
  dX[e] = dX[e] - Gs[e / NM] * z;
}

// dKz = -1/2 (G_l (iW - iK + iK Q iK) + dKz)   (dKz holds Wm Gam Wm^T on entry)
__global__ void gp_elbo_dkz_kernel(int L, int64_t MM, const double* __restrict__ Gs, const double* __restrict__ iK,
                                   const double* __restrict__ iW, const double* __restrict__ iKQiK,
                                   double* __restrict__ dKz) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L * MM) return;
  dKz[e] = -0.5 * (Gs[e / MM] * (iW[e] - iK[e] + iKQiK[e]) + dKz[e]);
}

// GB = -1/2 (G_l (iB - iBK0iB - GB) - AAt);  GK0 = -G_l / 2 iB   (GB holds (U - Z) iBK^T, AAt A Gam A^T on entry)
// (lvae_gp_elbo_bwd_z_f64 reads -G_l / 2 back as GK0[l][0] / iB[l][0], bound_dkz_fix_kernel: keep GK0 = (-G_l / 2) iB)
// seg: both are 0 on padding rows and columns -- iB's identity there must reach neither dnoise (through dB's trace)
// nor dparams0 (through K0's diagonal).  Element (0, 0) of subject 0 is valid (seg[0] >= 1), so the read-back holds.
__global__ void gp_elbo_gb_kernel(int64_t PTT, int L, int P, int T, const int32_t* __restrict__ seg,
                                  const double* __restrict__ Gs, const double* __restrict__ iB,
                                  const double* __restrict__ iBK0iB, const double* __restrict__ AAt,
                                  double* __restrict__ GB, double* __restrict__ GK0) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L * PTT) return;
  if (seg) {
    const int64_t TT = (int64_t)T * T;
    const int p = (int)((e / TT) % P), i = (int)((e % TT) / T), j = (int)(e % T), n = bound_seg_n(seg, p, T);
    if (i >= n || j >= n) {
      GB[e] = 0.0;
      GK0[e] = 0.0;
      return;
    }
  }
  const double G = Gs[e / PTT];
  GB[e] = -0.5 * (G * (iB[e] - iBK0iB[e] - GB[e]) - AAt[e]);
  GK0[e] = -0.5 * G * iB[e];
}

int ge_check(const lvae_kernel_spec* s0, const lvae_kernel_spec* s1, const lvae_gp_elbo_dims* d) {
  LVAE_TRY(bound_check(s0, s1, ge_dims(d)));
  return (d->S < 1 || d->S > kGeS) ? -3 : 0;
}

}  // namespace
}  // namespace lvae

using namespace lvae;

extern "C" {

size_t lvae_gp_elbo_workspace_size(const lvae_gp_elbo_dims* d) { return GWs(nullptr, *d).bytes; }

// (seg == NULL is the uniform call: the same launches with the same arguments as before there was a seg)
int lvae_gp_elbo_fwd_seg_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1,
                             const lvae_gp_elbo_dims* dp, const int32_t* seg, const double* x, const double* z,
                             const double* y, const double* params0, const double* params1, const double* noise,
                             double* elbo, int32_t* info, void* workspace, void* stream) {
  LVAE_TRY(ge_check(spec0, spec1, dp));
  if (!workspace || ((uintptr_t)workspace & 255)) return -4;
  hipStream_t st = (hipStream_t)stream;
  const lvae_gp_elbo_dims& d = *dp;
  const int L = d.L, M = d.M, P = d.P, T = d.T, S = d.S, N = P * T;
  const int64_t MM = (int64_t)M * M, TT = (int64_t)T * T, NM = (int64_t)N * M;
  const int64_t MS = (int64_t)M * kGeS, NS = (int64_t)N * kGeS;
  GWs w((char*)workspace, d);
  LVAE_TRY(bound_grams_fwd(spec0, spec1, ge_dims(dp), x, z, params0, params1, noise, d.eps, w.epsv, w.X, w.Kz,
                           w.K0st, w.Bst, st));
  if (seg) bound_seg_mask(ge_dims(dp), seg, w.X, w.K0st, w.Bst, st);
  LVAE_TRY(spd_inv_small_f64(M, L, w.Kz, MM, w.iK, MM, w.ldK, w.info, st));
  LVAE_TRY(spd_inv_small_f64(T, L * P, w.Bst, TT, w.iB, TT, w.ldB, w.info + L, st));
  if (T <= kBoundT) {
    const int G = bound_groups(P), nt = bound_tiles(M);
    const int64_t ps = ge_part_stride(M);
    if (seg)
      gp_elbo_subject_seg_launch(dim3(G, L), st, M, P, T, L, S, nt, ps, w.X, w.iB, w.K0st, w.ldB, y, w.iBK, w.s,
                                 w.part, seg);
    else
      gp_elbo_subject_kernel<><<<dim3(G, L), 512, 0, st>>>(M, P, T, L, S, nt, ps, w.X, w.iB, w.K0st, w.ldB, y, w.iBK,
                                                          w.s, w.part);
    gp_elbo_reduce_kernel<<<dim3(nt + 9, L), 256, 0, st>>>(M, G, nt, ps, w.part, w.Q, w.Pm, w.scal);
  } else {
    // large T: iBK, Q, Pm = iBK^T Y, s_p = iB_p Y_p as batched products
    gp_elbo_pack_kernel<<<blocks((int64_t)L * NS), 256, 0, st>>>(N, L, S, T, seg, y, w.Yp);
    LVAE_TRY(gemm_small_f64(0, 0, T, M, T, 1.0, w.iB, T, P * TT, TT, w.X, M, NM, (int64_t)T * M, 0.0, w.iBK, M, NM,
                            (int64_t)T * M, L, P, st));
    LVAE_TRY(gemm_small_f64(1, 0, M, M, N, 1.0, w.X, M, NM, 0, w.iBK, M, NM, 0, 0.0, w.Q, M, MM, 0, L, 1, st));
    LVAE_TRY(gemm_small_f64(1, 0, M, kGeS, N, 1.0, w.iBK, M, NM, 0, w.Yp, kGeS, NS, 0, 0.0, w.Pm, kGeS, MS, 0, L, 1,
                            st));
    LVAE_TRY(gemm_small_f64(0, 0, T, kGeS, T, 1.0, w.iB, T, P * TT, TT, w.Yp, kGeS, NS, (int64_t)T * kGeS, 0.0, w.s,
                            kGeS, NS, (int64_t)T * kGeS, L, P, st));
    gp_elbo_scal_kernel<<<L, 256, 0, st>>>(P, T, w.Yp, w.s, w.iB, w.K0st, w.ldB, w.scal);
  }
  // Wm = iW Pm
  LVAE_TRY(bound_w_inverse(L, M, w.Kz, w.Q, w.W, w.iW0, w.E, w.iW, w.ldW, w.info + L + L * P, st));
  LVAE_TRY(gemm_small_f64(0, 0, M, kGeS, M, 1.0, w.iW, M, MM, 0, w.Pm, kGeS, MS, 0, 0.0, w.Wm, kGeS, MS, 0, L, 1, st));
  gp_elbo_final_kernel<<<L, 256, 0, st>>>(M, L, S, (double)N, P, T, seg, w.Q, w.iK, w.Pm, w.Wm, w.scal, w.ldK, w.ldW, elbo);
  if (info) bound_info(L, P, w.info, info, st);
  LVAE_CHECK_LAUNCH();
  return 0;
}

int lvae_gp_elbo_fwd_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const lvae_gp_elbo_dims* dp,
                         const double* x, const double* z, const double* y, const double* params0,
                         const double* params1, const double* noise, double* elbo, int32_t* info, void* workspace,
                         void* stream) {
  return lvae_gp_elbo_fwd_seg_f64(spec0, spec1, dp, nullptr, x, z, y, params0, params1, noise, elbo, info, workspace,
                                  stream);
}

int lvae_gp_elbo_bwd_seg_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1,
                             const lvae_gp_elbo_dims* dp, const int32_t* seg, const double* x, const double* z,
                             const double* y, const double* params0, const double* params1, const double* noise,
                             const double* gelbo, double* dy, double* dparams0, double* dparams1, double* dnoise,
                             void* workspace, void* stream) {
  (void)y;
  (void)noise;
  LVAE_TRY(ge_check(spec0, spec1, dp));
  if (!workspace || ((uintptr_t)workspace & 255)) return -4;
  hipStream_t st = (hipStream_t)stream;
  const lvae_gp_elbo_dims& d = *dp;
  const int L = d.L, M = d.M, P = d.P, T = d.T, S = d.S, N = P * T;
  const int64_t MM = (int64_t)M * M, TT = (int64_t)T * T, NM = (int64_t)N * M, LTT = (int64_t)L * P * TT;
  const int64_t TM = (int64_t)T * M, MS = (int64_t)M * kGeS, NS = (int64_t)N * kGeS, TS = (int64_t)T * kGeS;
  GWs w((char*)workspace, d);
  // U = iBK iW ; Z = iBK iK ; A = s - U Pm -> dy ; the cotangent-scaled columns A Gam, Wm Gam and G = sum_s g_s
  LVAE_TRY(gemm_small_f64(0, 0, N, M, M, 1.0, w.iBK, M, NM, 0, w.iW, M, MM, 0, 0.0, w.U, M, NM, 0, L, 1, st));
  LVAE_TRY(gemm_small_f64(0, 0, N, M, M, 1.0, w.iBK, M, NM, 0, w.iK, M, MM, 0, 0.0, w.Z, M, NM, 0, L, 1, st));
  LVAE_TRY(gemm_small_f64(0, 0, N, kGeS, M, 1.0, w.U, M, NM, 0, w.Pm, kGeS, MS, 0, 0.0, w.A, kGeS, NS, 0, L, 1, st));
  gp_elbo_g_kernel<<<blocks((int64_t)L * MS), 256, 0, st>>>(L, M, S, gelbo, w.Wm, w.WG, w.Gs);
  gp_elbo_a_kernel<<<blocks((int64_t)L * NS), 256, 0, st>>>(N, L, S, T, seg, gelbo, w.s, w.A, w.AG, dy);
  // iK Q iK = (X iK)^T Z from the N x M factors, X iK in dX's place (why not (iK Q) iK: dubo.hip's backward)
  LVAE_TRY(gemm_small_f64(0, 0, N, M, M, 1.0, w.X, M, NM, 0, w.iK, M, MM, 0, 0.0, w.dX, M, NM, 0, L, 1, st));
  LVAE_TRY(gemm_small_f64(1, 0, M, M, N, 1.0, w.dX, M, NM, 0, w.Z, M, NM, 0, 0.0, w.iKQiK, M, MM, 0, L, 1, st));
  // dX = (A Gam) Wm^T - G (U - Z)   (one [N,16] x [16,M] product for all samples)
  LVAE_TRY(gemm_small_f64(0, 1, N, M, kGeS, 1.0, w.AG, kGeS, NS, 0, w.Wm, kGeS, MS, 0, 0.0, w.dX, M, NM, 0, L, 1, st));
  gp_elbo_dx_kernel<<<blocks((int64_t)L * NM), 256, 0, st>>>(NM, L, w.Gs, w.U, w.Z, w.dX);
  // dKz
  LVAE_TRY(gemm_small_f64(0, 1, M, M, kGeS, 1.0, w.WG, kGeS, MS, 0, w.Wm, kGeS, MS, 0, 0.0, w.dKz, M, MM, 0, L, 1, st));
  gp_elbo_dkz_kernel<<<blocks(L * MM), 256, 0, st>>>(L, MM, w.Gs, w.iK, w.iW, w.iKQiK, w.dKz);
  // dB_p, dK0_p (Z now holds U - Z)
  LVAE_TRY(gemm_small_f64(0, 0, T, T, T, 1.0, w.K0st, T, P * TT, TT, w.iB, T, P * TT, TT, 0.0, w.K0iB, T, P * TT, TT,
                          L, P, st));
  LVAE_TRY(gemm_small_f64(0, 0, T, T, T, 1.0, w.iB, T, P * TT, TT, w.K0iB, T, P * TT, TT, 0.0, w.iBK0iB, T, P * TT,
                          TT, L, P, st));
  LVAE_TRY(gemm_small_f64(0, 1, T, T, M, 1.0, w.Z, M, NM, TM, w.iBK, M, NM, TM, 0.0, w.GB, T, P * TT, TT, L, P, st));
  LVAE_TRY(gemm_small_f64(0, 1, T, T, kGeS, 1.0, w.AG, kGeS, NS, TS, w.A, kGeS, NS, TS, 0.0, w.AAt, T, P * TT, TT, L,
                          P, st));
  gp_elbo_gb_kernel<<<blocks(LTT), 256, 0, st>>>(P * TT, L, P, T, seg, w.Gs, w.iB, w.iBK0iB, w.AAt, w.GB, w.GK0);
  // hyper-parameter gradients through the four Grams
  LVAE_TRY(bound_grams_bwd(spec0, spec1, ge_dims(dp), x, z, params0, params1, w.dX, w.dKz, w.GK0, w.GB, dparams0,
                           dparams1, dnoise, w.gpart, st));
  LVAE_CHECK_LAUNCH();
  return 0;
}

int lvae_gp_elbo_bwd_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const lvae_gp_elbo_dims* dp,
                         const double* x, const double* z, const double* y, const double* params0,
                         const double* params1, const double* noise, const double* gelbo, double* dy,
                         double* dparams0, double* dparams1, double* dnoise, void* workspace, void* stream) {
  return lvae_gp_elbo_bwd_seg_f64(spec0, spec1, dp, nullptr, x, z, y, params0, params1, noise, gelbo, dy, dparams0,
                                  dparams1, dnoise, workspace, stream);
}

// dz from the dX / dKz lvae_gp_elbo_bwd_f64 left in the workspace (gelbo[s][l] is already inside them).  After a
// lvae_gp_elbo_bwd_seg_f64 nothing changes: the padding rows of dX are exact zeros.
int lvae_gp_elbo_bwd_z_f64(const lvae_kernel_spec* spec0, const lvae_gp_elbo_dims* dp, const double* x,
                           const double* z, const double* params0, double* dz, void* workspace, void* zworkspace,
                           void* stream) {
  LVAE_TRY(ge_check(spec0, spec0, dp));
  LVAE_TRY(bound_check_z(spec0, ge_dims(dp)));
  if (!workspace || ((uintptr_t)workspace & 255)) return -4;
  if (!zworkspace || ((uintptr_t)zworkspace & 255)) return -5;
  hipStream_t st = (hipStream_t)stream;
  const BoundDims bd = ge_dims(dp);
  GWs w((char*)workspace, *dp);
  BoundZWs zw((char*)zworkspace, bd.L, bd.M, bd.P * bd.T, bd.Q);
  // (w.Z holds U - iBK iK and w.iKQiK, w.GK0 what the backward left; the ELBO's dKz has no iW R iW term)
  LVAE_TRY(bound_dkz_stable(bd, w.X, w.iK, nullptr, w.U, w.Z, nullptr, nullptr, w.iKQiK, nullptr, w.GK0, w.iB, w.dKz,
                            zw, st));
  return bound_grams_bwd_z(spec0, bd, x, z, params0, w.dX, zw.dKz, dz, zw.part, st);
}

}  // extern "C"
