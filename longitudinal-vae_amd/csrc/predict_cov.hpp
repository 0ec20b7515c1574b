// predict_cov.hpp -- the kernels of the joint predictive covariance of a group of test rows and of the trajectory
// draws from it (predict.hip: lvae_predict_cov_f64, lvae_predict_exact_cov_f64, lvae_predict_sample_f64).  All fp64;
// every reduction runs in a fixed order (no atomics), so the bits depend on neither the grid nor, for the exact
// route, the test-row chunk.
//
// Output: cov [L, G, n_max, n_max], block (l, g) the covariance of group g's rows in their order, the identity on
// its padding rows and columns (pc_eye_kernel fills every block first; the tile kernels write the real entries).
// Only the tiles on and below the diagonal are computed, and only their entries i >= j are used: each is stored at
// [i][j] and at [j][i], so a block is symmetric bit for bit.
//
// Inducing-point route, per latent dim, with the [rows, Nt] matrices of predict_var.hpp (g: the group's columns):
//   Sigma_g = KzX_g^T Q_g + k1(x*_g, x*_g) - (Q_g^T W_g + E_g^T Q_g + C_g^T D_g) + W_g^T V_g
// whose diagonal is pv_var_kernel's formula.  Exact route: Sigma_g = k(x*_g, x*_g) - V_g^T V_g over the solved panel
// V = L^-1 k(X, x*_g), the sum over the n prediction rows cut into slabs of kCovSlab rows whose partial tiles go to
// the workspace and are added in slab order.
#pragma once
#include "predict_var.hpp"

namespace lvae {
namespace {

constexpr int kCovBatch = 64;  // groups per launch of the exact route (their panel columns travel by value)
constexpr int kCovSlab = 512;  // prediction rows per partial sum of the exact route

// the groups of one launch of the exact route: group b holds the panel columns [col[b], col[b + 1]) of the chunk
// and the tiles [tile[b], tile[b + 1]) of the launch
struct CovBatch {
  int n;
  int col[kCovBatch + 1];
  int tile[kCovBatch + 1];
};

__host__ __device__ inline int cov_tiles(int rows) {  // 16 x 16 tiles on and below the diagonal
  const int t = (rows + kPvC - 1) / kPvC;
  return t * (t + 1) / 2;
}

// tile x of the lower triangle, row by row: x = ti (ti + 1) / 2 + tj, tj <= ti
__device__ inline void cov_tile(int x, int& ti, int& tj) {
  ti = 0;
  while (x > ti) {
    x -= ti + 1;
    ++ti;
  }
  tj = x;
}

// cov[b][i][j] = (i == j) for nb blocks of n_max x n_max
__global__ __launch_bounds__(256) void pc_eye_kernel(int64_t nb, int n_max, double* __restrict__ cov) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, nn = (int64_t)n_max * n_max;
  if (e >= nb * nn) return;
  const int64_t f = e % nn;
  cov[e] = (f / n_max == f % n_max) ? 1.0 : 0.0;
}

// ---- inducing-point route ----
// The five products of one 16 x 16 tile on v_mfma_f64_16x16x4 (operand layout as pv_group_kernel:
// A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15], acc[r] = C[(lane >> 4) + 4 r][lane & 15]).
// Every operand is a [rows, ld] matrix with the tile's rows and columns among its columns, so the 16 lanes of a k
// step read contiguous doubles straight from memory (each element is read once per workgroup: no LDS stage).  om /
// ot: the dim's [M, ld] / [T, ld] matrix at the group's first column; this lane holds column i of the A operands
// and column j of the B operands (vi / vj: inside the group).  The sums run over M and T in index order.  Shared
// with predict_ccov.hpp, where a test row's components take the role of a group's rows.
struct CovAcc {
  pv_f64x4 kq, qw, eq, cd, wv;
};
__device__ inline CovAcc cov_products(int M, int T, int64_t ld, int64_t om, int64_t ot, int i, int j, bool vi, bool vj,
                                      const double* __restrict__ KzX, const double* __restrict__ Qm,
                                      const double* __restrict__ W, const double* __restrict__ E,
                                      const double* __restrict__ V, const double* __restrict__ C,
                                      const double* __restrict__ D) {
  const int lk = threadIdx.x >> 4;
  pv_f64x4 kq = {0.0, 0.0, 0.0, 0.0}, qw = kq, eq = kq, cd = kq, wv = kq;
  for (int kk = 0; kk < M; kk += 4) {
    const int m = kk + lk;
    const bool ok = m < M;
    const int64_t oi = om + (int64_t)m * ld + i, oj = om + (int64_t)m * ld + j;
    const double k_i = (ok && vi) ? KzX[oi] : 0.0, q_i = (ok && vi) ? Qm[oi] : 0.0;
    const double e_i = (ok && vi) ? E[oi] : 0.0, w_i = (ok && vi) ? W[oi] : 0.0;
    const double q_j = (ok && vj) ? Qm[oj] : 0.0, w_j = (ok && vj) ? W[oj] : 0.0, v_j = (ok && vj) ? V[oj] : 0.0;
    kq = __builtin_amdgcn_mfma_f64_16x16x4f64(k_i, q_j, kq, 0, 0, 0);
    qw = __builtin_amdgcn_mfma_f64_16x16x4f64(q_i, w_j, qw, 0, 0, 0);
    eq = __builtin_amdgcn_mfma_f64_16x16x4f64(e_i, q_j, eq, 0, 0, 0);
    wv = __builtin_amdgcn_mfma_f64_16x16x4f64(w_i, v_j, wv, 0, 0, 0);
  }
  for (int kk = 0; kk < T; kk += 4) {
    const int t = kk + lk;
    const bool ok = t < T;
    const double c_i = (ok && vi) ? C[ot + (int64_t)t * ld + i] : 0.0;
    const double d_j = (ok && vj) ? D[ot + (int64_t)t * ld + j] : 0.0;
    cd = __builtin_amdgcn_mfma_f64_16x16x4f64(c_i, d_j, cd, 0, 0, 0);
  }
  return CovAcc{kq, qw, eq, cd, wv};
}

// One 64-lane workgroup per (tile, group, dim).  Group g: the columns [gstart[g], gstart[g + 1]) clamped to
// 0 .. Nt, of which the first n_max are used.  Tiles past the group's rows do nothing.  The five products
// (cov_products) keep an accumulator each and are combined as pv_var_kernel combines its sums.
template <int MC, int MF>
__global__ __launch_bounds__(64) void pc_cov_kernel(DevSpec s, int M, int T, int Nt, int Q, int n_max,
                                                    const int32_t* __restrict__ gstart,
                                                    const double* __restrict__ KzX, const double* __restrict__ Qm,
                                                    const double* __restrict__ W, const double* __restrict__ E,
                                                    const double* __restrict__ V, const double* __restrict__ C,
                                                    const double* __restrict__ D, const double* __restrict__ tx,
                                                    const double* __restrict__ params,
                                                    const double* __restrict__ noise, int add_noise,
                                                    double* __restrict__ cov) {
  const int g = blockIdx.y, l = blockIdx.z, G = gridDim.y, lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
  int a = gstart[g], b = gstart[g + 1];
  a = a < 0 ? 0 : (a > Nt ? Nt : a);
  b = b < a ? a : (b > Nt ? Nt : b);
  const int ng = b - a < n_max ? b - a : n_max;
  int ti, tj;
  cov_tile(blockIdx.x, ti, tj);
  if (ti * kPvC >= ng) return;
  const int i = ti * kPvC + li, j = tj * kPvC + li;  // this lane's row of the A operands, column of the B operands
  const bool vi = i < ng, vj = j < ng;
  const int64_t om = (int64_t)l * M * Nt + a, ot = (int64_t)l * T * Nt + a;
  const CovAcc p = cov_products(M, T, Nt, om, ot, i, j, vi, vj, KzX, Qm, W, E, V, C, D);
  const pv_f64x4 kq = p.kq, qw = p.qw, eq = p.eq, cd = p.cd, wv = p.wv;
  double* blk = cov + ((int64_t)l * G + g) * n_max * n_max;
  const double* pl = params + (int64_t)l * s.n_params;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int io = ti * kPvC + lk + 4 * r;  // (row of acc[r]; its column is j)
    if (io >= ng || j > io) continue;
    const double prior = kernel_eval<MC, MF, double>(s, tx + (int64_t)(a + io) * Q, tx + (int64_t)(a + j) * Q, pl);
    double f = (kq[r] + prior) - ((qw[r] + eq[r]) + cd[r]) + wv[r];
    if (add_noise && io == j) f += noise[l];
    blk[(int64_t)io * n_max + j] = f;
    blk[(int64_t)j * n_max + io] = f;
  }
}

// ---- exact route ----
// the group of tile x of a launch (tile[] ascending; x < tile[n])
__device__ inline int cov_batch_group(const CovBatch& cb, int x) {
  int b = 0;
  while (b + 1 < cb.n && x >= cb.tile[b + 1]) ++b;
  return b;
}

// One slab's share of a 16 x 16 tile of V^T V: sum over the rows r0 <= r < r1 of pl[r][i] pl[r][j], four rows a step
// in index order; this lane holds column i of the A operand and column j of the B operand (vi / vj: inside the
// group).  Shared with predict_ccov.hpp, where a test row's components take the role of a group's rows.
__device__ inline pv_f64x4 cov_slab_tile(const double* __restrict__ pl, int64_t ldp, int i, int j, bool vi, bool vj,
                                         int r0, int r1) {
  const int lk = threadIdx.x >> 4;
  pv_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int kk = r0; kk < r1; kk += 4) {
    const int r = kk + lk;
    const bool ok = r < r1;
    const double v_i = (ok && vi) ? pl[(int64_t)r * ldp + i] : 0.0;
    const double v_j = (ok && vj) ? pl[(int64_t)r * ldp + j] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v_i, v_j, acc, 0, 0, 0);
  }
  return acc;
}

// part[l][tile0 + x][slab][16][16] = the slab's share of V_g^T V_g on tile x: one 64-lane workgroup per
// (tile, slab, dim), panel [L, n, ldp] (this chunk's solved columns), tcap tiles per dim in part
__global__ __launch_bounds__(64) void pcx_partial_kernel(CovBatch cb, int n, const double* __restrict__ panel,
                                                         int64_t ldp, int tile0, int tcap,
                                                         double* __restrict__ part) {
  const int l = blockIdx.z, slab = blockIdx.y, nslab = gridDim.y, lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
  const int b = cov_batch_group(cb, blockIdx.x), c0 = cb.col[b], ng = cb.col[b + 1] - c0;
  int ti, tj;
  cov_tile(blockIdx.x - cb.tile[b], ti, tj);
  const int i = ti * kPvC + li, j = tj * kPvC + li;
  const bool vi = i < ng, vj = j < ng;
  const int r0 = slab * kCovSlab, r1 = r0 + kCovSlab < n ? r0 + kCovSlab : n;
  const double* pl = panel + (int64_t)l * n * ldp + c0;
  const pv_f64x4 acc = cov_slab_tile(pl, ldp, i, j, vi, vj, r0, r1);
  double* po = part + ((((int64_t)l * tcap + tile0 + blockIdx.x) * nslab + slab) << 8);
#pragma unroll
  for (int r = 0; r < 4; ++r) po[(lk + 4 * r) * kPvC + li] = acc[r];
}

// cov block entries of tile x: k(x*_i, x*_j) (+ noise_l on the diagonal) - the slabs' partials added in slab order.
// One 256-thread workgroup per (tile, dim), one thread per entry; tc the chunk's test rows, g0 the launch's first
// group, G the groups of the whole call.
template <int MC, int MF>
__global__ __launch_bounds__(256) void pcx_reduce_kernel(DevSpec s, CovBatch cb, int nslab, int tile0, int tcap,
                                                         const double* __restrict__ part,
                                                         const double* __restrict__ tc, int64_t ldt,
                                                         const double* __restrict__ params,
                                                         const double* __restrict__ noise, int add_noise, int g0,
                                                         int G, int n_max, double* __restrict__ cov) {
  const int l = blockIdx.y, ii = threadIdx.x >> 4, jj = threadIdx.x & 15;
  const int b = cov_batch_group(cb, blockIdx.x), c0 = cb.col[b], ng = cb.col[b + 1] - c0;
  int ti, tj;
  cov_tile(blockIdx.x - cb.tile[b], ti, tj);
  const int i = ti * kPvC + ii, j = tj * kPvC + jj;
  if (i >= ng || j > i) return;
  const double* pi = part + ((((int64_t)l * tcap + tile0 + blockIdx.x) * nslab) << 8) + ii * kPvC + jj;
  double ss = 0.0;
  for (int k = 0; k < nslab; ++k) ss += pi[(int64_t)k << 8];
  const double prior = kernel_eval<MC, MF, double>(s, tc + (int64_t)(c0 + i) * ldt, tc + (int64_t)(c0 + j) * ldt,
                                                   params + (int64_t)l * s.n_params);
  double f = prior - ss;
  if (add_noise && i == j) f += noise[l];
  double* blk = cov + ((int64_t)l * G + g0 + b) * n_max * n_max;
  blk[(int64_t)i * n_max + j] = f;
  blk[(int64_t)j * n_max + i] = f;
}

// ---- draws ----
// Lc[b][i][j] = cov[b][i][j] + jitter (i == j) for nb blocks (the copy lvae_potrf_f64 then factors in place)
__global__ __launch_bounds__(256) void pcs_jitter_kernel(int64_t nb, int n_max, double jitter,
                                                         const double* __restrict__ cov, double* __restrict__ Lc) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, nn = (int64_t)n_max * n_max;
  if (e >= nb * nn) return;
  const int64_t f = e % nn;
  Lc[e] = (f / n_max == f % n_max) ? cov[e] + jitter : cov[e];
}

// out[s][r_i][l] = mean[r_i][l] + sum_{j <= i} Lc[l][g][i][j] eps[s][r_j][l], r_i = index[g][i] (< 0: padding, and
// nothing is written), one thread per (s, g, i, l), the sum in the order of j
__global__ __launch_bounds__(256) void pcs_draw_kernel(int L, int G, int n_max, int Nt, int S,
                                                       const double* __restrict__ Lc,
                                                       const int32_t* __restrict__ index,
                                                       const double* __restrict__ mean,
                                                       const double* __restrict__ eps, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)S * G * n_max * L) return;
  const int l = (int)(e % L), i = (int)((e / L) % n_max), g = (int)((e / ((int64_t)L * n_max)) % G);
  const int64_t sm = e / ((int64_t)L * n_max * G);
  const int32_t* ix = index + (int64_t)g * n_max;
  const int ri = ix[i];
  if (ri < 0 || ri >= Nt) return;
  const double* row = Lc + (((int64_t)l * G + g) * n_max + i) * n_max;
  const double* es = eps + sm * Nt * L + l;
  double acc = 0.0;
  for (int j = 0; j <= i; ++j) {
    const int rj = ix[j];
    if (rj >= 0 && rj < Nt) acc = fma(row[j], es[(int64_t)rj * L], acc);
  }
  out[(sm * Nt + ri) * L + l] = mean[(int64_t)ri * L + l] + acc;
}

}  // namespace
}  // namespace lvae
