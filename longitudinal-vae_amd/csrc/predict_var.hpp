// predict_var.hpp -- the kernels of the two predictive variances (predict.hip: lvae_predict_exact_var_f64,
// lvae_predict_var_f64).  All fp64; every reduction runs in a fixed order (no atomics), so the bits depend on
// neither the grid nor, for the exact route, the test-row chunk.
//
// Inducing-point route, per latent dim, test rows as the columns of every matrix ([rows, Nt], ld = Nt):
//   C [T, Nt]  c_i = k1(x_s(i), x*_i) on the valid rows of the row's subject (0 elsewhere / subject absent)
//   D [T, Nt]  d_i = iB_s(i) c_i          E [M, Nt]  e_i = K0zx_s(i) d_i       (pv_group_kernel, fp64 MFMA)
//   Q = K0zz^-1 K0zX*,  W = G Q + E,  V = H^-1 W                              (gemm_small_f64, fp64 MFMA)
//   var_i = K0zX*_i . q_i + k1(x*_i, x*_i) - (q_i . w_i + q_i . e_i + c_i . d_i) + w_i . v_i   (pv_var_kernel)
// (q . w + q . e = q^T G q + 2 q^T e).  k1 is taken to vanish between subjects (every component of the id
// kernel carries the id covariate's cat factor), as the mean's subject-blocked B already assumes.
#pragma once
#include "common.hpp"

namespace lvae {
namespace {

typedef double pv_f64x4 __attribute__((ext_vector_type(4)));

constexpr int kPvT = 128;  // T, M <= 128 (lvae_predict_f64's limits)
constexpr int kPvC = 16;   // test rows per MFMA column tile

// ---- exact route ----
// var[c0 + j][l] = k(x*_j, x*_j) (+ noise_l) - sum_i V[l][i][j]^2 over the solved panel V = L^-1 k(X, X*_chunk)
// [L, n, ldp].  64 columns per workgroup; strand s = tid / 64 sums rows s, s + 4, .. in order, then the four
// strands are added in order: the result depends on n alone.
template <int MC, int MF>
__global__ __launch_bounds__(256) void pe_var_kernel(DevSpec s, int n, int nr, const double* __restrict__ panel,
                                                     int64_t ldp, const double* __restrict__ tx, int64_t ldt,
                                                     const double* __restrict__ params,
                                                     const double* __restrict__ noise, int add_noise,
                                                     double* __restrict__ var, int64_t ld_var) {
  __shared__ double red[4][64];
  const int l = blockIdx.y, jj = threadIdx.x & 63, st = threadIdx.x >> 6, j = blockIdx.x * 64 + jj;
  double acc = 0.0;
  if (j < nr) {
    const double* v = panel + (int64_t)l * n * ldp + j;
    for (int i = st; i < n; i += 4) {
      const double a = v[(int64_t)i * ldp];
      acc = fma(a, a, acc);
    }
  }
  red[st][jj] = acc;
  __syncthreads();
  if (st == 0 && j < nr) {
    const double ss = ((red[0][jj] + red[1][jj]) + red[2][jj]) + red[3][jj];
    const double* xi = tx + (int64_t)j * ldt;
    const double prior = kernel_eval<MC, MF, double>(s, xi, xi, params + (int64_t)l * s.n_params);
    const double f = prior - ss;
    var[(int64_t)j * ld_var + l] = add_noise ? f + noise[l] : f;
  }
}

// ---- inducing-point route ----
// rs[i] = 1 + the prediction-set index of test row i's subject, 0 when no group holds the row or its subject is
// absent (group g: rows [start[g], start[g + 1]), subject gsub[g] or -1)
__global__ void pv_rowsubj_kernel(int Nt, int P, int G, const int32_t* __restrict__ gsub,
                                  const int32_t* __restrict__ gstart, int32_t* __restrict__ rs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Nt) return;
  int v = 0;
  for (int g = 0; g < G; ++g)
    if (i >= gstart[g] && i < gstart[g + 1]) {
      const int p = gsub[g];
      v = (p >= 0 && p < P) ? p + 1 : 0;
      break;
    }
  rs[i] = v;
}

// C[l][t][i] = k1(x[s(i)][t], x*_i) for t < seg_len[s(i)], 0 on padding rows and for absent subjects
template <int MC, int MF>
__global__ __launch_bounds__(256) void pv_c_kernel(DevSpec s, int L, int T, int Nt, int Q,
                                                   const int32_t* __restrict__ seg, const int32_t* __restrict__ rs,
                                                   const double* __restrict__ x, const double* __restrict__ tx,
                                                   const double* __restrict__ params, double* __restrict__ C) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)L * T * Nt) return;
  const int i = (int)(e % Nt), t = (int)((e / Nt) % T), l = (int)(e / ((int64_t)Nt * T));
  const int p = rs[i] - 1;
  double v = 0.0;
  if (p >= 0 && t < seg[p])
    v = kernel_eval<MC, MF, double>(s, x + ((int64_t)p * T + t) * Q, tx + (int64_t)i * Q,
                                    params + (int64_t)l * s.n_params);
  C[e] = v;
}

// D = iB_p C and E = K0zx_p D for one tile of <= 16 test rows of one subject group and one latent dim, on
// v_mfma_f64_16x16x4 (operand layout as gemm_small_kernel: A[row = lane & 15][k = lane >> 4],
// B[k = lane >> 4][col = lane & 15], acc[r] = C[(lane >> 4) + 4 r][lane & 15]).  Tile blockIdx.x is found by
// walking the groups (ceil(len / 16) tiles each); tiles past the last group and groups of absent subjects do
// nothing (D and E are zeroed beforehand).  iB is read through its symmetry, iB[k][row], so that the 16 lanes of
// a k read contiguous doubles; K0xz [NP, M] gives K0zx[m][t] the same way.  Padding rows (t >= seg_len) carry
// C = 0 and the identity in iB, and zero rows of K0xz: they add nothing to D or E.  cpr: columns per test row (1
// here; the component-resolved route of predict_ccov.hpp has n_comp columns a row, and Nt counts columns).
__global__ __launch_bounds__(256) void pv_group_kernel(int M, int P, int T, int Nt, int G, int cpr,
                                                       const int32_t* __restrict__ gsub,
                                                       const int32_t* __restrict__ gstart,
                                                       const double* __restrict__ C, const double* __restrict__ iB,
                                                       const double* __restrict__ K0xz, double* __restrict__ D,
                                                       double* __restrict__ E) {
  __shared__ double Cs[kPvT][kPvC + 1];
  __shared__ double Ds[kPvT][kPvC + 1];
  __shared__ int tile[3];  // subject, first row, rows
  const int l = blockIdx.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  if (tid == 0) {
    int left = blockIdx.x, p = -1, i0 = 0, nc = 0;
    for (int g = 0; g < G; ++g) {
      int64_t a = (int64_t)gstart[g] * cpr, b = (int64_t)gstart[g + 1] * cpr;
      a = a < 0 ? 0 : (a > Nt ? Nt : a);
      b = b < a ? a : (b > Nt ? Nt : b);
      const int ntile = (int)((b - a + kPvC - 1) / kPvC);
      if (left < ntile) {
        p = gsub[g];
        i0 = (int)a + kPvC * left;
        nc = (int)b - i0 < kPvC ? (int)b - i0 : kPvC;
        break;
      }
      left -= ntile;
    }
    tile[0] = (p >= 0 && p < P) ? p : -1;
    tile[1] = i0;
    tile[2] = nc;
  }
  __syncthreads();
  const int p = tile[0], i0 = tile[1], nc = tile[2];
  if (p < 0 || nc < 1) return;
  const int T4 = (T + 3) & ~3, Tt = (T + 15) >> 4, Mt = (M + 15) >> 4;
  const double* Cl = C + (int64_t)l * T * Nt;
  for (int e = tid; e < T4 * kPvC; e += 256) {
    const int t = e >> 4, j = e & 15;
    Cs[t][j] = (t < T && j < nc) ? Cl[(int64_t)t * Nt + i0 + j] : 0.0;
  }
  __syncthreads();
  const double* iBp = iB + ((int64_t)l * P + p) * T * T;
  double* Dl = D + (int64_t)l * T * Nt;
  for (int rt = w; rt < Tt; rt += 4) {
    pv_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    const int row = rt * 16 + li;
    for (int kk = 0; kk < T4; kk += 4) {
      const int k = kk + lk;
      const double a = (row < T && k < T) ? iBp[(int64_t)k * T + row] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Cs[k][li], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = rt * 16 + lk + 4 * r;  // (< 16 Tt <= 128)
      Ds[t][li] = acc[r];
      if (t < T && li < nc) Dl[(int64_t)t * Nt + i0 + li] = acc[r];
    }
  }
  __syncthreads();
  const double* Kp = K0xz + ((int64_t)l * P + p) * T * M;
  double* El = E + (int64_t)l * M * Nt;
  for (int rt = w; rt < Mt; rt += 4) {
    pv_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    const int m = rt * 16 + li;
    for (int kk = 0; kk < T4; kk += 4) {
      const int k = kk + lk;
      const double a = (m < M && k < T) ? Kp[(int64_t)k * M + m] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ds[k][li], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mo = rt * 16 + lk + 4 * r;
      if (mo < M && li < nc) El[(int64_t)mo * Nt + i0 + li] = acc[r];
    }
  }
}

// The five column-wise dot products and the variance, one thread per (l, test row), each sum in index order:
//   var[i][l] = KzX . Q + k1(x*_i, x*_i) (+ noise_l) - (Q . W + Q . E + C . D) + W . V
template <int MC, int MF>
__global__ __launch_bounds__(256) void pv_var_kernel(DevSpec s, int L, int M, int T, int Nt, int Q,
                                                     const double* __restrict__ KzX, const double* __restrict__ Qm,
                                                     const double* __restrict__ W, const double* __restrict__ E,
                                                     const double* __restrict__ V, const double* __restrict__ C,
                                                     const double* __restrict__ D, const double* __restrict__ tx,
                                                     const double* __restrict__ params,
                                                     const double* __restrict__ noise, int add_noise,
                                                     double* __restrict__ var) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)L * Nt) return;
  const int l = (int)(e / Nt), i = (int)(e % Nt);
  const int64_t om = (int64_t)l * M * Nt + i, ot = (int64_t)l * T * Nt + i;
  double kq = 0.0, qw = 0.0, qe = 0.0, cd = 0.0, wv = 0.0;
  for (int m = 0; m < M; ++m) {
    const int64_t o = om + (int64_t)m * Nt;
    const double q = Qm[o], ww = W[o];
    kq = fma(KzX[o], q, kq);
    qw = fma(q, ww, qw);
    qe = fma(q, E[o], qe);
    wv = fma(ww, V[o], wv);
  }
  for (int t = 0; t < T; ++t) {
    const int64_t o = ot + (int64_t)t * Nt;
    cd = fma(C[o], D[o], cd);
  }
  const double* xi = tx + (int64_t)i * Q;
  const double prior = kernel_eval<MC, MF, double>(s, xi, xi, params + (int64_t)l * s.n_params);
  const double f = (kq + prior) - ((qw + qe) + cd) + wv;
  var[(int64_t)i * L + l] = add_noise ? f + noise[l] : f;
}

}  // namespace
}  // namespace lvae
