// kl_cond.hip -- the exact N x N prior KL (KL_closed, elbo_functions.py:8-34) conditioned on a frozen prior and
// frozen training latents: the joint KL of cat(new, train) as a closed form in the Nn new rows' (m, l) alone, in the
// state lvae_dubo_cond_eval_f64 evaluates (cond_state.hpp; Pn = nn, T = 1, mask all ones).  All fp64.
//
// Per latent dim, t the n training rows (mu_t, v_t = exp(logv_t)), K = k(.,.) + noise I on the joint rows:
//   W = K_tt^-1 K_tn [n, nn]     S = K_nn - K_nt W [nn, nn]     A = S^-1     a = diag(A)
//   abar = W^T mu_t              r = A abar
//   c = 1/2 ( abar^T A abar - nn + log|S| + tr(A W^T diag(v_t) W) )
//   cond(m, l) = c + 1/2 ( m^T A m - 2 r^T m + sum_i a_i e^{l_i} - sum_i l_i )
//              = KL_closed(joint rows; new rows = (m, l)) - KL_closed(training rows alone)
//
// Launches of lvae_kl_cond_prepare_f64, per group of dims:
//   1. lvae_gram_f64 (K_tt + noise I), lvae_potrf_f64 in place
//   2. lvae_gram_f64 (k(x_train, x_new) [L, n, nn]), lvae_trsm_f64(trans = 0): V = L^-1 K_tn
//   3. the weighted SYRK below with w = 1 and the prior epilogue: S = k(x_new, x_new) + noise I - V^T V
//   4. lvae_trsm_f64(trans = 1): W = L^-T V in place; the weighted SYRK with w = exp(logv_t): Tm = W^T diag(v_t) W;
//      kc_abar_kernel: abar = W^T mu_t
//   5. lvae_potrf_f64 on S in place; kc_eye_kernel + lvae_potrs_f64: A = S^-1; kc_mirror_kernel: the lower triangle
//      stored over the upper one, so A is symmetric bit for bit
//   6. kc_rows_kernel (a, r and each row's share of abar^T r + tr(A Tm)), kc_const_kernel (c, info, mask)
// n == 0: steps 1, 2 and 4 vanish, S = K_nn, abar = 0, Tm = 0.
//
// The weighted SYRK, C = D -/+ sum_r w_r P[r][i] P[r][j] over a tall panel P [n, nn], on v_mfma_f64_16x16x4:
//   block  64 x 64 outputs per workgroup of 4 waves (the lower blocks bj <= bi only); wave w owns the 16 rows
//          16 w .. 16 w + 15 of the block and its four 16 x 16 tiles (on a diagonal block only the tiles tj <= w)
//   slab   kSyrkSlab = 512 panel rows per workgroup and partial sum; the slab passes through LDS once per workgroup,
//          kSyrkStage = 32 rows at a time (the next stage's global loads are in flight while the current one feeds
//          the matrix cores), so a panel element is read from memory once per block column it belongs to instead of
//          once per 16 x 16 tile
//   LDS    rows of 64 doubles at a pitch of kSyrkPitch = 80 doubles: the 16 lanes of a k step read 128 contiguous
//          bytes, and the pitch puts consecutive k steps (lanes l and l + 16 of a ds_read_b64 group of 32) on
//          opposite halves of the 256-byte bank row: conflict-free.  2 x 20 KiB + the stage's weights per workgroup
//   sums   the slabs' 64 x 64 partials go to the workspace and kc_syrk_reduce_kernel adds them in slab order, then
//          applies D (the prior through kernel_eval, or nothing) and stores entry (i, j), i >= j, at both places
// No atomics; every sum runs in an order fixed by n and nn alone, so the same inputs give the same bits, whatever
// the group of dims a dim is processed in.
#include <type_traits>

#include "cond_state.hpp"
#include "gram.hpp"

namespace lvae {

namespace {

typedef double kc_f64x4 __attribute__((ext_vector_type(4)));

constexpr int kSyrkSlab = 512;   // panel rows per partial sum
constexpr int kSyrkBlk = 64;     // edge of a workgroup's output block
constexpr int kSyrkStage = 32;   // panel rows per LDS stage
constexpr int kSyrkPitch = 80;   // LDS row pitch in doubles

inline int syrk_slabs(int n) { return cdiv(n, kSyrkSlab); }
inline int64_t syrk_blocks(int nn) {
  const int64_t b = cdiv(nn, kSyrkBlk);
  return b * (b + 1) / 2;
}

// block x of the lower triangle, row by row: x = bi (bi + 1) / 2 + bj, bj <= bi
__device__ inline void kc_block(int x, int& bi, int& bj) {
  int r = (int)((sqrt(8.0 * (double)x + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= x) ++r;
  while (r * (r + 1) / 2 > x) --r;
  bi = r;
  bj = x - r * (r + 1) / 2;
}

// part[l][block][slab][64][64] = the slab's share of sum_r w_r P[l][r][i] P[l][r][j] on the block: grid
// (blocks, slabs, L), 256 threads.  w_r = exp(logv[r ld_lv + l]), or 1 when logv is NULL.  Rows past the slab's end
// and columns past nn enter as zeros.
__global__ __launch_bounds__(256) void kc_syrk_partial_kernel(int n, int nn, const double* __restrict__ P, int64_t ldp,
                                                              const double* __restrict__ logv, int64_t ld_lv,
                                                              double* __restrict__ part) {
  __shared__ double sI[kSyrkStage * kSyrkPitch];
  __shared__ double sJ[kSyrkStage * kSyrkPitch];
  __shared__ double sw[kSyrkStage];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int slab = blockIdx.y, nslab = gridDim.y, l = blockIdx.z;
  int bi, bj;
  kc_block(blockIdx.x, bi, bj);
  const bool diag = bi == bj;
  const int r_begin = slab * kSyrkSlab, r_end = r_begin + kSyrkSlab < n ? r_begin + kSyrkSlab : n;
  const double* Pl = P + (int64_t)l * n * ldp;
  // the loader: this thread's column of the stage and its rows lr + 4 q
  const int lc = tid & 63, lr = tid >> 6, ci = bi * kSyrkBlk + lc, cj = bj * kSyrkBlk + lc;
  const bool vi = ci < nn, vj = cj < nn && !diag;
  double ri[kSyrkStage / 4], rj[kSyrkStage / 4], rw = 0.0;
  auto fetch = [&](int rb) {
#pragma unroll
    for (int q = 0; q < kSyrkStage / 4; ++q) {
      const int row = rb + lr + 4 * q;
      const bool ok = row < r_end;
      ri[q] = (ok && vi) ? Pl[(int64_t)row * ldp + ci] : 0.0;
      rj[q] = (ok && vj) ? Pl[(int64_t)row * ldp + cj] : 0.0;
    }
    if (tid < kSyrkStage) {
      const int row = rb + tid;
      rw = row < r_end ? (logv ? exp(logv[(int64_t)row * ld_lv + l]) : 1.0) : 0.0;
    }
  };
  kc_f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = kc_f64x4{0.0, 0.0, 0.0, 0.0};
  const double* sB = diag ? sI : sJ;
  fetch(r_begin);
  for (int rb = r_begin; rb < r_end; rb += kSyrkStage) {
    __syncthreads();  // the previous stage's readers are done
#pragma unroll
    for (int q = 0; q < kSyrkStage / 4; ++q) {
      sI[(lr + 4 * q) * kSyrkPitch + lc] = ri[q];
      if (!diag) sJ[(lr + 4 * q) * kSyrkPitch + lc] = rj[q];
    }
    if (tid < kSyrkStage) sw[tid] = rw;
    __syncthreads();
    if (rb + kSyrkStage < r_end) fetch(rb + kSyrkStage);
#pragma unroll
    for (int kk = 0; kk < kSyrkStage; kk += 4) {
      const int k = kk + lk;
      const double a = sw[k] * sI[k * kSyrkPitch + wave * 16 + li];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (!diag || t <= wave)
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sB[k * kSyrkPitch + t * 16 + li], acc[t], 0, 0, 0);
    }
  }
  double* po = part + ((((int64_t)l * gridDim.x + blockIdx.x) * nslab + slab) << 12);
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (!diag || t <= wave) {
#pragma unroll
      for (int r = 0; r < 4; ++r) po[(wave * 16 + lk + 4 * r) * kSyrkBlk + t * 16 + li] = acc[t][r];
    }
}

// C[l][i][j] = C[l][j][i] = D - sum of the slabs' partials in slab order (prior != 0: D = k(xn_i, xn_j) +
// noise_l (i == j)), or + the sum with D = 0 (prior == 0), for the entries i >= j of a block: grid (blocks, L), 256
// threads, 16 entries each
template <int MC, int MF>
__global__ __launch_bounds__(256) void kc_syrk_reduce_kernel(DevSpec s, int nn, int nslab,
                                                             const double* __restrict__ part,
                                                             const double* __restrict__ xn, int64_t ldn,
                                                             const double* __restrict__ params,
                                                             const double* __restrict__ noise, int prior,
                                                             double* __restrict__ C) {
  const int l = blockIdx.y, tid = threadIdx.x;
  int bi, bj;
  kc_block(blockIdx.x, bi, bj);
  const double* pb = part + ((((int64_t)l * gridDim.x + blockIdx.x) * nslab) << 12);
  double* Cl = C + (int64_t)l * nn * nn;
  for (int e = tid; e < kSyrkBlk * kSyrkBlk; e += 256) {
    const int i = bi * kSyrkBlk + (e >> 6), j = bj * kSyrkBlk + (e & 63);
    if (i >= nn || j > i) continue;
    double ss = 0.0;
    for (int k = 0; k < nslab; ++k) ss += pb[((int64_t)k << 12) + e];
    double f = ss;
    if (prior) {
      double d = kernel_eval<MC, MF, double>(s, xn + (int64_t)i * ldn, xn + (int64_t)j * ldn,
                                             params + (int64_t)l * s.n_params);
      if (i == j) d += noise[l];
      f = d - ss;
    }
    Cl[(int64_t)i * nn + j] = f;
    Cl[(int64_t)j * nn + i] = f;
  }
}

// abar[l][j] = sum_r W[l][r][j] mu[r ld_mu + l]: 64 columns per workgroup; strand s = tid / 64 sums the rows
// s, s + 4, .. in order, then the four strands are added in order
__global__ __launch_bounds__(256) void kc_abar_kernel(int n, int nn, const double* __restrict__ W,
                                                      const double* __restrict__ mu, int64_t ld_mu,
                                                      double* __restrict__ abar) {
  __shared__ double red[4][64];
  const int l = blockIdx.y, jj = threadIdx.x & 63, st = threadIdx.x >> 6, j = blockIdx.x * 64 + jj;
  double acc = 0.0;
  if (j < nn) {
    const double* w = W + (int64_t)l * n * nn + j;
    for (int r = st; r < n; r += 4) acc = fma(w[(int64_t)r * nn], mu[(int64_t)r * ld_mu + l], acc);
  }
  red[st][jj] = acc;
  __syncthreads();
  if (st == 0 && j < nn) abar[(int64_t)l * nn + j] = ((red[0][jj] + red[1][jj]) + red[2][jj]) + red[3][jj];
}

// A[l] = the identity (the right-hand side of A = S^-1)
__global__ __launch_bounds__(256) void kc_eye_kernel(int64_t L, int nn, double* __restrict__ A) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, m = (int64_t)nn * nn;
  if (e >= L * m) return;
  const int64_t f = e % m;
  A[e] = (f / nn == f % nn) ? 1.0 : 0.0;
}

// A[l][j][i] = A[l][i][j] for i > j: a thread per entry of the strict lower triangle reads it and writes its mirror
__global__ __launch_bounds__(256) void kc_mirror_kernel(int64_t L, int nn, double* __restrict__ A) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, m = (int64_t)nn * nn;
  if (e >= L * m) return;
  const int64_t f = e % m, i = f / nn, j = f % nn;
  if (i > j) A[e - f + j * nn + i] = A[e];
}

// a wave per row i of A[l]: a[l][i] = A_ii, r[l][i] = sum_j A_ij abar_j, rowt[l][i] = abar_i r_i + sum_j A_ij Tm_ij
// (the row's share of abar^T A abar + tr(A Tm)); the lanes' sums over j = lane, lane + 64, .. meet in wave_sum's
// fixed order.  grid (ceil(nn / 4), L), 256 threads.  abar / Tm NULL (n == 0): taken as 0.
__global__ __launch_bounds__(256) void kc_rows_kernel(int nn, const double* __restrict__ A,
                                                      const double* __restrict__ abar, const double* __restrict__ Tm,
                                                      double* __restrict__ a, double* __restrict__ r,
                                                      double* __restrict__ rowt) {
  const int l = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= nn) return;
  const double* Ai = A + ((int64_t)l * nn + i) * nn;
  double sr = 0.0, st = 0.0;
  if (abar) {
    const double* ab = abar + (int64_t)l * nn;
    const double* Ti = Tm + ((int64_t)l * nn + i) * nn;
    for (int j = lane; j < nn; j += 64) {
      const double v = Ai[j];
      sr = fma(v, ab[j], sr);
      st = fma(v, Ti[j], st);
    }
    sr = wave_sum(sr);
    st = wave_sum(st);
  }
  if (lane == 0) {
    a[(int64_t)l * nn + i] = Ai[i];
    r[(int64_t)l * nn + i] = sr;
    rowt[(int64_t)l * nn + i] = (abar ? abar[(int64_t)l * nn + i] * sr : 0.0) + st;
  }
}

// c[l] = 1/2 (sum_i rowt[l][i] - nn + log|S_l|), info[l] = the training factor's word, else 20000 + S's, and (every
// workgroup, the same values) mask = 1: one workgroup per dim, thread t sums the rows t, t + 256, .. in order and
// block_sum adds the threads in its fixed order
__global__ __launch_bounds__(256) void kc_const_kernel(int nn, const double* __restrict__ rowt,
                                                       const double* __restrict__ logdet_s,
                                                       const int32_t* __restrict__ info_k,
                                                       const int32_t* __restrict__ info_s, double* __restrict__ c,
                                                       int32_t* __restrict__ info, int32_t* __restrict__ mask) {
  __shared__ double red[4];
  const int l = blockIdx.x, tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < nn; i += 256) {
    s += rowt[(int64_t)l * nn + i];
    mask[i] = 1;
  }
  s = block_sum<256>(s, red);
  if (tid == 0) {
    c[l] = 0.5 * ((s - (double)nn) + logdet_s[l]);
    const int32_t ik = info_k ? info_k[l] : 0, is = info_s[l];
    info[l] = ik ? ik : (is ? 20000 + is : 0);
  }
}

// The workspace: K [L, n, n] (the training factor), the panel [L, n, nn] (K_tn, V, then W), S and Tm [L, nn, nn],
// abar and rowt [L, nn], the two log-determinants and info words [L], the solves' inverted diagonal blocks and the
// SYRK's slab partials [L, blocks, slabs, 64, 64]
struct KcWs {
  double *K, *panel, *S, *Tm, *abar, *rowt, *logdet_k, *logdet_s, *part;
  int32_t *info_k, *info_s;
  char* trsm;
  size_t bytes;
  KcWs(char* base, int n, int nn, int L) {
    WsCarve c(base);
    const size_t l = (size_t)L, sq = (size_t)nn * nn;
    K = c.take(l * n * n);
    panel = c.take(l * n * nn);
    S = c.take(l * sq);
    Tm = c.take(n > 0 ? l * sq : 0);
    abar = c.take(l * nn);
    rowt = c.take(l * nn);
    logdet_k = c.take(l);
    logdet_s = c.take(l);
    info_k = (int32_t*)c.take((l + 1) / 2);
    info_s = (int32_t*)c.take((l + 1) / 2);
    const size_t t0 = n > 0 ? lvae_trsm_workspace_size(n, L) : 0, t1 = lvae_trsm_workspace_size(nn, L);
    trsm = (char*)c.take(((t0 > t1 ? t0 : t1) + 7) / 8);
    part = c.take(l * (size_t)syrk_blocks(nn) * syrk_slabs(n) * kSyrkBlk * kSyrkBlk);
    bytes = c.off;
  }
};

inline int nblk(int64_t n) { return cdiv(n, 256); }

// C [L, nn, nn] = D -/+ sum_r w_r P[r][i] P[r][j] (header): the partial launch over the slabs (none for n == 0),
// then the reduce launch
int weighted_syrk(const lvae_kernel_spec* spec, int n, int nn, int L, const double* P, const double* logv,
                  int64_t ld_lv, const double* xn, int64_t ldn, const double* params, const double* noise, int prior,
                  double* part, double* C, hipStream_t st) {
  const int nslab = syrk_slabs(n), nb = (int)syrk_blocks(nn);
  if (nslab > 0) kc_syrk_partial_kernel<<<dim3(nb, nslab, L), 256, 0, st>>>(n, nn, P, nn, logv, ld_lv, part);
  const DevSpec ds = to_dev(spec);
  if (spec_bucket(spec) == 1)
    kc_syrk_reduce_kernel<8, 2><<<dim3(nb, L), 256, 0, st>>>(ds, nn, nslab, part, xn, ldn, params, noise, prior, C);
  else
    kc_syrk_reduce_kernel<16, 4><<<dim3(nb, L), 256, 0, st>>>(ds, nn, nslab, part, xn, ldn, params, noise, prior, C);
  LVAE_CHECK_LAUNCH();
  return 0;
}

}  // namespace
}  // namespace lvae

using namespace lvae;

extern "C" {

size_t lvae_kl_cond_workspace_size(int n, int nn, int L) {
  if (n < 0 || nn < 1 || L < 1) return 0;
  return KcWs(nullptr, n, nn, L).bytes;
}

int lvae_kl_cond_prepare_f64(const lvae_kernel_spec* spec, const double* x_train, int64_t ldx, int n,
                             const double* x_new, int64_t ldn, int nn, int L, const double* params,
                             const double* noise, const double* mu_train, int64_t ld_mu, const double* logv_train,
                             int64_t ld_lv, void* state, int L_state, int l0, int32_t* info, void* workspace,
                             void* stream) {
  const int ld_min = spec ? gram_matvec_spec_ld(spec) : 0;
  if (ld_min < 1 || ld_min > 32) return -1;  // (before any launch)
  if (n > 0 && !x_train) return -2;
  if (n > 0 && ldx < ld_min) return -3;
  if (n < 0) return -4;
  if (!x_new) return -5;
  if (ldn < ld_min) return -6;
  if (nn < 1) return -7;
  if (L < 1 || L > 65535) return -8;
  if (!params) return -9;
  if (!noise) return -10;
  if (n > 0 && !mu_train) return -11;
  if (n > 0 && ld_mu < L) return -12;
  if (n > 0 && !logv_train) return -13;
  if (n > 0 && ld_lv < L) return -14;
  if (!state || ((uintptr_t)state & 255)) return -15;
  if (L_state < 1 || l0 < 0 || L > L_state - l0) return -16;
  if (!info) return -17;
  if (!workspace || ((uintptr_t)workspace & 255)) return -18;
  hipStream_t st = (hipStream_t)stream;
  KcWs w((char*)workspace, n, nn, L);
  const CondState s((char*)state, L_state, nn, 1);
  const int64_t n2 = (int64_t)n * n, q2 = (int64_t)nn * nn, np = (int64_t)n * nn;
  double *sc = s.c + l0, *sr = s.r + (int64_t)l0 * nn, *sa = s.a + (int64_t)l0 * nn, *sA = s.A + (int64_t)l0 * q2;
  const lvae_xview nv{x_new, 0, 0, ldn};
  if (n > 0) {
    // 1. the training factor; 2. V = L^-1 K_tn
    const lvae_xview xv{x_train, 0, 0, ldx};
    LVAE_TRY(lvae_gram_f64(spec, xv, xv, 1, L, n, n, params, noise, w.K, 0, n2, n, stream));
    LVAE_TRY(lvae_potrf_f64(n, L, w.K, n, n2, w.K, n, n2, w.logdet_k, w.info_k, stream));
    LVAE_TRY(lvae_gram_f64(spec, xv, nv, 1, L, n, nn, params, nullptr, w.panel, 0, np, nn, stream));
    LVAE_TRY(lvae_trsm_f64(0, n, nn, L, w.K, n, n2, w.panel, nn, np, w.trsm, stream));
  }
  // 3. S = k(x_new, x_new) + noise I - V^T V
  LVAE_TRY(weighted_syrk(spec, n, nn, L, w.panel, nullptr, 0, x_new, ldn, params, noise, 1, w.part, w.S, st));
  if (n > 0) {
    // 4. W = L^-T V, Tm = W^T diag(v_t) W, abar = W^T mu_t
    LVAE_TRY(lvae_trsm_f64(1, n, nn, L, w.K, n, n2, w.panel, nn, np, w.trsm, stream));
    LVAE_TRY(weighted_syrk(spec, n, nn, L, w.panel, logv_train, ld_lv, x_new, ldn, params, noise, 0, w.part, w.Tm, st));
    kc_abar_kernel<<<dim3(cdiv(nn, 64), L), 256, 0, st>>>(n, nn, w.panel, mu_train, ld_mu, w.abar);
  }
  // 5. A = S^-1 through the factor of S, symmetric bit for bit
  LVAE_TRY(lvae_potrf_f64(nn, L, w.S, nn, q2, w.S, nn, q2, w.logdet_s, w.info_s, stream));
  kc_eye_kernel<<<nblk(L * q2), 256, 0, st>>>(L, nn, sA);
  LVAE_TRY(lvae_potrs_f64(nn, nn, L, w.S, nn, q2, sA, nn, q2, w.trsm, stream));
  kc_mirror_kernel<<<nblk(L * q2), 256, 0, st>>>(L, nn, sA);
  // 6. a, r, c, info, mask
  kc_rows_kernel<<<dim3(cdiv(nn, 4), L), 256, 0, st>>>(nn, sA, n > 0 ? w.abar : nullptr, n > 0 ? w.Tm : nullptr, sa, sr,
                                                       w.rowt);
  kc_const_kernel<<<L, 256, 0, st>>>(nn, w.rowt, w.logdet_s, n > 0 ? w.info_k : nullptr, w.info_s, sc, info, s.mask);
  LVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
