// dubo_cond.hip -- the DUBO conditioned on a frozen prior: the joint bound of dubo.hip as a closed form in the
// latents of Pn "free" subjects alone (the second half of variational_inference_optimization, training.py:688-749:
// decoder, kernels, noise, inducing points and the other subjects' (mu, log_var) are fixed, only the new subjects'
// are optimised).  Notation: the header of dubo.hip.
//
// Per latent dim, with m, l the free rows' mean and log-variance ([Nn], Nn = Pn T; rows ordered (free subject, t)):
//   dubo(m, l) = c + 1/2 ( m^T A m - 2 r^T m + sum_i a_i e^{l_i} - sum_i l_i )
//   G = the free subjects' rows of iBK [Nn, M]     U = G iW
//   A = blockdiag(iB_p : p free) - U G^T           (the free block of Sigma^-1)      a = diag(A)
//   r = U p_fixed,  p_fixed = sum_{p not free} iBK_p^T m_p
//   c = dubo(joint batch with m_free = 0, l_free = 0) - 1/2 sum_i a_i
// (Q, W, every log-det and the trace term do not depend on the latents; R enters linearly in v = e^l; p is affine in
// m.)  prepare runs the joint forward on a copy of mu / logv whose free rows are 0 -- so p = p_fixed and the value is
// the constant's first term -- and builds the state from what that forward leaves in its workspace; the copies, G
// and U live in the [L, N, M] buffers the forward leaves idle.  eval is one symmetric matvec per dim: y = A m gives
// both m^T y and the gradient, A is read once.
// Subjects of varying length: the padding rows of iBK are zero and iB is the identity there, so U G^T vanishes on
// the padding and the finish kernel zeroes iB's identity; eval skips the rows the state's mask marks as padding.
#include "cond_state.hpp"
#include "dubo_ws.hpp"

namespace lvae {
namespace {

constexpr int kCondRows = 256;     // rows of A per workgroup of the eval
constexpr int kCondChunk = 2048;   // columns of A whose m is staged in LDS at a time (16 KiB)

// subject of the k-th free slot, clamped to [0, P): a bad free_idx gives wrong numbers, never an out-of-range access
__device__ __forceinline__ int cond_subject(const int32_t* __restrict__ free_idx, int k, int P) {
  const int p = free_idx[k];
  return p < 0 ? 0 : (p >= P ? P - 1 : p);
}

// mu0 = mu, lv0 = logv ([N, L], n = N L doubles each)
__global__ void cond_copy_kernel(int64_t n, const double* __restrict__ mu, const double* __restrict__ logv,
                                 double* __restrict__ mu0, double* __restrict__ lv0) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  mu0[e] = mu[e];
  lv0[e] = logv[e];
}

// the free subjects' rows of mu0 / lv0 -> 0 (after cond_copy_kernel on the same stream: whatever mu / logv held there,
// NaN included, is gone)
__global__ void cond_zero_free_kernel(int Pn, int P, int64_t TL, const int32_t* __restrict__ free_idx,
                                      double* __restrict__ mu0, double* __restrict__ lv0) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= Pn * TL) return;
  const int64_t o = (int64_t)cond_subject(free_idx, (int)(e / TL), P) * TL + e % TL;
  mu0[o] = 0.0;
  lv0[o] = 0.0;
}

// G[l][k T + t][:] = iBK[l][free_idx[k] T + t][:]; mask[k T + t] = the row is inside its subject's seg
__global__ void cond_gather_kernel(int L, int M, int P, int T, int Pn, const int32_t* __restrict__ seg,
                                   const int32_t* __restrict__ free_idx, const double* __restrict__ iBK,
                                   double* __restrict__ G, int32_t* __restrict__ mask) {
  const int64_t Nn = (int64_t)Pn * T, N = (int64_t)P * T;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < Nn) {
    const int k = (int)(e / T);
    mask[e] = bound_seg_valid(seg, cond_subject(free_idx, k, P), (int)(e % T), T) ? 1 : 0;
  }
  if (e >= L * Nn * M) return;
  const int64_t l = e / (Nn * M), i = (e / M) % Nn, j = e % M;
  const int p = cond_subject(free_idx, (int)(i / T), P);
  G[e] = iBK[(l * N + (int64_t)p * T + i % T) * M + j];
}

// A <- blockdiag(iB_p : p free) - A (A holds U G^T), exact 0 on padding rows and columns; a = diag(A); r <- 0 on
// the padding rows
__global__ void cond_finish_kernel(int L, int P, int T, int Pn, const int32_t* __restrict__ free_idx,
                                   const int32_t* __restrict__ mask, const double* __restrict__ iB,
                                   double* __restrict__ A, double* __restrict__ a, double* __restrict__ r) {
  const int64_t Nn = (int64_t)Pn * T;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L * Nn * Nn) return;
  const int64_t l = e / (Nn * Nn), i = (e / Nn) % Nn, j = e % Nn;
  const int ki = (int)(i / T), kj = (int)(j / T);
  double v = 0.0;
  if (mask[i] && mask[j]) {
    const int p = cond_subject(free_idx, ki, P);
    const double b = ki == kj ? iB[(((int64_t)l * P + p) * T + i % T) * T + j % T] : 0.0;
    v = b - A[e];
  }
  A[e] = v;
  if (i == j) {
    a[l * Nn + i] = v;
    if (!mask[i]) r[l * Nn + i] = 0.0;
  }
}

// c[l] <- c[l] - 1/2 sum_i a[l][i] (c holds the joint bound at m_free = 0, l_free = 0): one workgroup per dim
__global__ __launch_bounds__(256) void cond_const_kernel(int64_t Nn, const double* __restrict__ a,
                                                         double* __restrict__ c) {
  __shared__ double red[4];
  const int l = blockIdx.x, tid = threadIdx.x;
  double s = 0.0;
  for (int64_t i = tid; i < Nn; i += 256) s += a[l * Nn + i];
  s = block_sum<256>(s, red);
  if (tid == 0) c[l] -= 0.5 * s;
}

__device__ __forceinline__ double cond_dlogv(double gl, double ai, double lv) { return 0.5 * gl * (ai * exp(lv) - 1.0); }

// The eval: grid (nb = ceil(Nn / 256), L), 1024 threads.  A workgroup owns 256 rows of A[l]; m[:, l] is staged in
// LDS a chunk of columns at a time (0 on the padding rows, whose m is not read), a wave walks its rows with
// coalesced row reads and a wave reduction, and y = A m stays in LDS.  Then a thread per row: dm = g (y - r) and
// the row's share q_i = m_i (y_i - 2 r_i) + a_i e^{l_i} - l_i of the value, summed over the workgroup in a fixed order.
// nb == 1: dubo and dlogv are written here.  nb > 1: the workgroup's partial goes to dlogv[b][l] (rows b < nb <= Nn
// of the output, which dubo_cond_sum_kernel reads before it writes dlogv itself) -- no scratch, no atomics.
__global__ __launch_bounds__(1024) void dubo_cond_eval_kernel(int64_t Nn, int L, int nb, const double* __restrict__ A,
                                                              const double* __restrict__ r,
                                                              const double* __restrict__ a,
                                                              const double* __restrict__ c,
                                                              const int32_t* __restrict__ mask,
                                                              const double* __restrict__ m,
                                                              const double* __restrict__ logv,
                                                              const double* __restrict__ g, double* __restrict__ dubo,
                                                              double* __restrict__ dm, double* __restrict__ dlogv) {
  __shared__ double sm[kCondChunk];
  __shared__ double sy[kCondRows];
  __shared__ double red[16];
  const int b = blockIdx.x, l = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t row0 = (int64_t)b * kCondRows;
  const int nr = Nn - row0 < kCondRows ? (int)(Nn - row0) : kCondRows;
  const double* Al = A + (int64_t)l * Nn * Nn;
  for (int64_t c0 = 0; c0 < Nn; c0 += kCondChunk) {
    const int cn = Nn - c0 < kCondChunk ? (int)(Nn - c0) : kCondChunk;
    __syncthreads();  // the previous chunk's readers are done
    for (int j = tid; j < cn; j += 1024) sm[j] = mask[c0 + j] ? m[(c0 + j) * L + l] : 0.0;
    __syncthreads();
    for (int rr = wave; rr < nr; rr += 16) {
      const double* Ar = Al + (row0 + rr) * Nn + c0;
      double s = 0.0;
      for (int j = lane; j < cn; j += 64) s += Ar[j] * sm[j];
      s = wave_sum(s);
      if (lane == 0) sy[rr] = (c0 ? sy[rr] : 0.0) + s;  // (a row keeps its wave: no barrier between the chunks)
    }
  }
  __syncthreads();
  double q = 0.0;
  if (tid < nr) {
    const int64_t i = row0 + tid, o = i * L + l;
    const double gl = g ? g[l] : 1.0;
    if (mask[i]) {
      const double mi = m[o], lv = logv[o], ai = a[l * Nn + i], ri = r[l * Nn + i], y = sy[tid];
      dm[o] = gl * (y - ri);
      if (nb == 1) dlogv[o] = cond_dlogv(gl, ai, lv);
      q = mi * (y - 2.0 * ri) + ai * exp(lv) - lv;
    } else {
      dm[o] = 0.0;
      if (nb == 1) dlogv[o] = 0.0;
    }
  }
  q = block_sum<1024>(q, red);
  if (tid == 0) {
    if (nb == 1)
      dubo[l] = c[l] + 0.5 * q;
    else
      dlogv[(int64_t)b * L + l] = q;
  }
}

// nb > 1: dubo[l] = c[l] + 1/2 sum_b partial[b][l], the groups added in group order (as dubo_reduce_kernel adds its
// groups), then dlogv[:, l], which held the partials.  One workgroup per dim: it reads and writes column l alone.
__global__ __launch_bounds__(256) void dubo_cond_sum_kernel(int64_t Nn, int L, int nb, const double* __restrict__ a,
                                                            const double* __restrict__ c,
                                                            const int32_t* __restrict__ mask,
                                                            const double* __restrict__ logv,
                                                            const double* __restrict__ g, double* __restrict__ dubo,
                                                            double* dlogv) {
  const int l = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += dlogv[(int64_t)b * L + l];
    dubo[l] = c[l] + 0.5 * s;
  }
  __syncthreads();  // every partial is read before any row of dlogv is written
  const double gl = g ? g[l] : 1.0;
  for (int64_t i = tid; i < Nn; i += 256)
    dlogv[i * L + l] = mask[i] ? cond_dlogv(gl, a[l * Nn + i], logv[i * L + l]) : 0.0;
}

}  // namespace
}  // namespace lvae

using namespace lvae;

extern "C" {

size_t lvae_dubo_cond_state_size(int L, int Pn, int T) {
  if (L < 1 || Pn < 1 || T < 1) return 0;
  return CondState(nullptr, L, Pn, T).bytes;
}

int lvae_dubo_cond_prepare_f64(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const lvae_dubo_dims* dp,
                               const int32_t* seg, int Pn, const int32_t* free_idx, const double* x, const double* z,
                               const double* mu, const double* logv, const double* params0, const double* params1,
                               const double* noise, void* state, int32_t* info, void* workspace, void* stream) {
  const BoundDims bd = dubo_dims(dp);
  LVAE_TRY(bound_check(spec0, spec1, bd));
  if (Pn < 1 || Pn > bd.P) return -3;
  if (!workspace || ((uintptr_t)workspace & 255)) return -4;
  if (!state || ((uintptr_t)state & 255)) return -5;
  if (!free_idx) return -6;
  hipStream_t st = (hipStream_t)stream;
  const lvae_dubo_dims& d = *dp;
  const int L = d.L, M = d.M, P = d.P, T = d.T;
  const int64_t N = (int64_t)P * T, Nn = (int64_t)Pn * T, MM = (int64_t)M * M, NnM = Nn * M;
  DWs w((char*)workspace, d);
  CondState s((char*)state, L, Pn, T);
  // the joint forward at m_free = 0, l_free = 0 (copies in U and F, which the forward leaves idle): its value -> c
  double *mu0 = w.U, *lv0 = w.F;
  cond_copy_kernel<<<blocks(N * L), 256, 0, st>>>(N * L, mu, logv, mu0, lv0);
  cond_zero_free_kernel<<<blocks(Nn * L), 256, 0, st>>>(Pn, P, (int64_t)T * L, free_idx, mu0, lv0);
  LVAE_CHECK_LAUNCH();
  LVAE_TRY(lvae_dubo_fwd_seg_f64(spec0, spec1, dp, seg, x, z, mu0, lv0, params0, params1, noise, s.c, info, workspace,
                                 stream));
  // G (in dX), U = G iW (in Z), U G^T -> A, r = U p
  double *G = w.dX, *Uc = w.Z;
  cond_gather_kernel<<<blocks(L * NnM), 256, 0, st>>>(L, M, P, T, Pn, seg, free_idx, w.iBK, G, s.mask);
  LVAE_TRY(gemm_small_f64(0, 0, (int)Nn, M, M, 1.0, G, M, NnM, 0, w.iW, M, MM, 0, 0.0, Uc, M, NnM, 0, L, 1, st));
  LVAE_TRY(gemm_small_f64(0, 1, (int)Nn, (int)Nn, M, 1.0, Uc, M, NnM, 0, G, M, NnM, 0, 0.0, s.A, (int)Nn, Nn * Nn, 0,
                          L, 1, st));
  LVAE_TRY(gemm_small_f64(0, 0, (int)Nn, 1, M, 1.0, Uc, M, NnM, 0, w.p, 1, M, 0, 0.0, s.r, 1, Nn, 0, L, 1, st));
  cond_finish_kernel<<<blocks(L * Nn * Nn), 256, 0, st>>>(L, P, T, Pn, free_idx, s.mask, w.iB, s.A, s.a, s.r);
  cond_const_kernel<<<L, 256, 0, st>>>(Nn, s.a, s.c);
  LVAE_CHECK_LAUNCH();
  return 0;
}

int lvae_dubo_cond_eval_f64(int L, int Pn, int T, const void* state, const double* m, const double* logv,
                            const double* g, double* dubo, double* dm, double* dlogv, void* stream) {
  if (L < 1 || Pn < 1 || T < 1) return -3;
  if (!state || ((uintptr_t)state & 255)) return -5;
  if (!m || !logv || !dubo || !dm || !dlogv) return -7;
  hipStream_t st = (hipStream_t)stream;
  const CondState s((char*)state, L, Pn, T);
  const int64_t Nn = (int64_t)Pn * T;
  const int nb = cdiv(Nn, kCondRows);
  dubo_cond_eval_kernel<<<dim3(nb, L), 1024, 0, st>>>(Nn, L, nb, s.A, s.r, s.a, s.c, s.mask, m, logv, g, dubo, dm,
                                                      dlogv);
  if (nb > 1) dubo_cond_sum_kernel<<<L, 256, 0, st>>>(Nn, L, nb, s.a, s.c, s.mask, logv, g, dubo, dlogv);
  LVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
