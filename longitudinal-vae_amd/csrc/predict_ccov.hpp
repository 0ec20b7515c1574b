// predict_ccov.hpp -- the kernels of the joint posterior covariance of the additive components at a test row under
// both predictors (predict.hip: lvae_predict_exact_comp_cov_f64, lvae_predict_comp_cov_f64).  All fp64; every
// reduction runs in a fixed order (no atomics), so the bits depend on neither the grid nor, for the exact route,
// the test-row chunk, nor, for the inducing-point route, on which other test rows are in the call.
//
// Exact route.
// Per latent dim l and test row t, with K_l = k_l(x, x) + noise_l I = L_l L_l^T and V_r = L_l^-1 k_{l,r}(x, tx_t):
//   ccov[l][t][r][s] = (r == s) k_{l,r}(tx_t, tx_t) - V_r . V_s                      r, s < R = spec.n_comp
// Output [L, nt, R, R] without padding; only the entries s <= r are computed, each stored at [r][s] and at [s][r],
// so a block is symmetric bit for bit.
//
// Panel: [L, n, c R] for a chunk of c test rows, column t R + r = component r at the chunk's t-th row (row-major,
// component-minor), written by pcc_panel_kernel, solved in place by lvae_trsm_f64.  A test row's R columns then
// take the role a group's rows have in predict_cov.hpp's exact route: one 16 x 16 tile per row (R <= 16, columns
// r >= R zero), the n prediction rows cut into the same slabs of kCovSlab rows (cov_slab_tile), the partial tiles
// in the workspace and added in slab order.
//
// Inducing-point route: predict_var.hpp's algebra with one column per (test row i, component r), column i R + r,
// R = R0 + R1, the components of spec0 first.  A column r < R0 carries KzX = k0_r(z, x*_i) and C = 0, a column
// r >= R0 carries KzX = 0 and C = k1_{r - R0}(x_s(i), x*_i) on the subject's valid rows (pcc_kzx_kernel,
// pcc_c_kernel); D, E, Q, W, V follow by the variance route's own kernels on the Nt R columns, and a test row's R
// columns take the role of a group in predict_cov.hpp's tile kernel (cov_products; up to 2 x 2 tiles):
//   ccov[l][i][r][s] = KzX_r . Q_s + (r == s >= R0) k1_{r - R0}(x*_i, x*_i)
//                      - (Q_r . W_s + E_r . Q_s + C_r . D_s) + W_r . V_s
#pragma once
#include "predict_cov.hpp"

namespace lvae {
namespace {

// component r of the spec alone, s_r prod_f phi_rf with kernel_eval's own expressions (r a runtime index: the spec
// is wave-uniform)
template <int MF>
__device__ inline double kernel_eval_comp(const DevSpec& s, int r, const double* __restrict__ xi,
                                          const double* __restrict__ xj, const double* __restrict__ p) {
  double prod = p[s.scale_idx[r]];
#pragma unroll
  for (int f = 0; f < MF; ++f) {
    if (f < s.n_fac[r]) {
      const int d = s.dim[r][f];
      const double a = xi[d], b = xj[d];
      switch (s.kind[r][f]) {
        case LVAE_CAT: prod = (a - b == 0.0) ? prod : 0.0; break;
        case LVAE_BIN: prod = (a + b == 2.0) ? prod : 0.0; break;
        case LVAE_RBF: {
          const double diff = a - b, ell = p[s.param_idx[r][f]];
          prod *= exp(-(diff * diff) / (2.0 * ell * ell));
          break;
        }
        case LVAE_PER: {
          const double ad = fabs(a - b), ell = p[s.param_idx[r][f]], per = p[s.param_idx[r][f] + 1];
          const double sn = sin(M_PI * ad / per);
          prod *= exp(-2.0 * sn * sn / (ell * ell));
          break;
        }
        default: prod *= a * b; break;  // LVAE_LIN
      }
    }
  }
  return prod;
}

// panel[l][i][t R + r] = k_{l,r}(x_i, tc_t) for i < n, t < nr: one thread per (l, i, t), the pair's covariates
// read once and the R component values scattered to the row's R columns (lvae_gram_matvec_comp_f64's evaluation
// without the vector).  A component whose gates fail writes an exact 0.
template <int MF>
__global__ __launch_bounds__(256) void pcc_panel_kernel(DevSpec s, int L, int n, int nr,
                                                        const double* __restrict__ x, int64_t ldx,
                                                        const double* __restrict__ tc, int64_t ldt,
                                                        const double* __restrict__ params,
                                                        double* __restrict__ panel, int64_t ldp) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)L * n * nr) return;
  const int t = (int)(e % nr), i = (int)((e / nr) % n), l = (int)(e / ((int64_t)nr * n));
  const double* xi = x + (int64_t)i * ldx;
  const double* xt = tc + (int64_t)t * ldt;
  const double* pl = params + (int64_t)l * s.n_params;
  const int R = s.n_comp;
  double* dst = panel + ((int64_t)l * n + i) * ldp + (int64_t)t * R;
  for (int r = 0; r < R; ++r) dst[r] = kernel_eval_comp<MF>(s, r, xi, xt, pl);
}

// part[l][t][slab][16][16] = the slab's share of V^T V over the R solved columns of the chunk's t-th test row: one
// 64-lane workgroup per (row, slab, dim), panel [L, n, ldp], tcap rows per dim in part
__global__ __launch_bounds__(64) void pcc_partial_kernel(int n, int R, const double* __restrict__ panel, int64_t ldp,
                                                         int tcap, double* __restrict__ part) {
  const int t = blockIdx.x, slab = blockIdx.y, nslab = gridDim.y, l = blockIdx.z;
  const int lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
  const bool v = li < R;
  const int r0 = slab * kCovSlab, r1 = r0 + kCovSlab < n ? r0 + kCovSlab : n;
  const double* pl = panel + (int64_t)l * n * ldp + (int64_t)t * R;
  const pv_f64x4 acc = cov_slab_tile(pl, ldp, li, li, v, v, r0, r1);
  double* po = part + ((((int64_t)l * tcap + t) * nslab + slab) << 8);
#pragma unroll
  for (int r = 0; r < 4; ++r) po[(lk + 4 * r) * kPvC + li] = acc[r];
}

// ccov[l][c0 + t][r][s] = (r == s) k_{l,r}(tc_t, tc_t) - the slabs' partials added in slab order, for s <= r < R,
// stored at [r][s] and [s][r].  One 256-thread workgroup per (row, dim), one thread per entry of the tile.
template <int MF>
__global__ __launch_bounds__(256) void pcc_reduce_kernel(DevSpec s, int nslab, int tcap,
                                                         const double* __restrict__ part,
                                                         const double* __restrict__ tc, int64_t ldt,
                                                         const double* __restrict__ params, int c0, int nt,
                                                         double* __restrict__ ccov) {
  const int t = blockIdx.x, l = blockIdx.y, ii = threadIdx.x >> 4, jj = threadIdx.x & 15, R = s.n_comp;
  if (ii >= R || jj > ii) return;
  const double* pi = part + ((((int64_t)l * tcap + t) * nslab) << 8) + ii * kPvC + jj;
  double ss = 0.0;
  for (int k = 0; k < nslab; ++k) ss += pi[(int64_t)k << 8];
  const double* xt = tc + (int64_t)t * ldt;
  const double prior = ii == jj ? kernel_eval_comp<MF>(s, ii, xt, xt, params + (int64_t)l * s.n_params) : 0.0;
  const double f = prior - ss;
  double* blk = ccov + ((int64_t)l * nt + c0 + t) * R * R;
  blk[ii * R + jj] = f;
  blk[jj * R + ii] = f;
}

// ---- inducing-point route ----
// KzX[l][m][i R + r] = k0_r(z_l[m], x*_i) for r < R0 = s.n_comp, 0 for R0 <= r < R: one thread per (l, m, i)
template <int MF>
__global__ __launch_bounds__(256) void pcc_kzx_kernel(DevSpec s, int L, int M, int Nt, int Q, int R,
                                                      const double* __restrict__ z, const double* __restrict__ tx,
                                                      const double* __restrict__ params, double* __restrict__ KzX) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)L * M * Nt) return;
  const int i = (int)(e % Nt), m = (int)((e / Nt) % M), l = (int)(e / ((int64_t)Nt * M));
  const double* zm = z + ((int64_t)l * M + m) * Q;
  const double* xt = tx + (int64_t)i * Q;
  const double* pl = params + (int64_t)l * s.n_params;
  double* dst = KzX + ((int64_t)l * M + m) * Nt * R + (int64_t)i * R;
  for (int r = 0; r < s.n_comp; ++r) dst[r] = kernel_eval_comp<MF>(s, r, zm, xt, pl);
  for (int r = s.n_comp; r < R; ++r) dst[r] = 0.0;
}

// C[l][t][i R + R0 + r] = k1_r(x[s(i)][t], x*_i) for r < R1 = s.n_comp and t < seg_len[s(i)], 0 on padding rows, for
// absent subjects (rs[i] = 0) and in the columns r < R0: one thread per (l, t, i)
template <int MF>
__global__ __launch_bounds__(256) void pcc_c_kernel(DevSpec s, int L, int T, int Nt, int Q, int R0,
                                                    const int32_t* __restrict__ seg, const int32_t* __restrict__ rs,
                                                    const double* __restrict__ x, const double* __restrict__ tx,
                                                    const double* __restrict__ params, double* __restrict__ C) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)L * T * Nt) return;
  const int i = (int)(e % Nt), t = (int)((e / Nt) % T), l = (int)(e / ((int64_t)Nt * T));
  const int R = R0 + s.n_comp, p = rs[i] - 1;
  const bool on = p >= 0 && t < seg[p];
  const double* xp = x + ((int64_t)(on ? p : 0) * T + t) * Q;
  const double* xt = tx + (int64_t)i * Q;
  const double* pl = params + (int64_t)l * s.n_params;
  double* dst = C + ((int64_t)l * T + t) * Nt * R + (int64_t)i * R;
  for (int r = 0; r < R0; ++r) dst[r] = 0.0;
  for (int r = 0; r < s.n_comp; ++r) dst[R0 + r] = on ? kernel_eval_comp<MF>(s, r, xp, xt, pl) : 0.0;
}

// The R x R block of test row i and dim l: one 64-lane workgroup per (row x tile on or below the diagonal, dim), the
// operands [rows, Nt R] with the row's columns at i R; entries s <= r only, stored at [r][s] and [s][r].  s1 is the
// id kernel's spec (its components are the block's rows R0 .. R - 1).
template <int MF>
__global__ __launch_bounds__(64) void pcc_ind_kernel(DevSpec s1, int M, int T, int Nt, int Q, int R0,
                                                     const double* __restrict__ KzX, const double* __restrict__ Qm,
                                                     const double* __restrict__ W, const double* __restrict__ E,
                                                     const double* __restrict__ V, const double* __restrict__ C,
                                                     const double* __restrict__ D, const double* __restrict__ tx,
                                                     const double* __restrict__ params1, double* __restrict__ ccov) {
  const int R = R0 + s1.n_comp, ntile = cov_tiles(R);
  const int row = blockIdx.x / ntile, l = blockIdx.y, lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
  int ti, tj;
  cov_tile(blockIdx.x % ntile, ti, tj);
  const int i = ti * kPvC + li, j = tj * kPvC + li;
  const bool vi = i < R, vj = j < R;
  const int64_t ld = (int64_t)Nt * R;
  const int64_t om = (int64_t)l * M * ld + (int64_t)row * R, ot = (int64_t)l * T * ld + (int64_t)row * R;
  const CovAcc p = cov_products(M, T, ld, om, ot, i, j, vi, vj, KzX, Qm, W, E, V, C, D);
  double* blk = ccov + ((int64_t)l * Nt + row) * R * R;
  const double* xt = tx + (int64_t)row * Q;
  const double* pl = params1 + (int64_t)l * s1.n_params;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int io = ti * kPvC + lk + 4 * r;  // (row of acc[r]; its column is j)
    if (io >= R || j > io) continue;
    const double prior = (io == j && io >= R0) ? kernel_eval_comp<MF>(s1, io - R0, xt, xt, pl) : 0.0;
    const double f = (p.kq[r] + prior) - ((p.qw[r] + p.eq[r]) + p.cd[r]) + p.wv[r];
    blk[io * R + j] = f;
    blk[j * R + io] = f;
  }
}

}  // namespace
}  // namespace lvae
