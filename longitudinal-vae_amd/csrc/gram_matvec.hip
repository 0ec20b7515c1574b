// gram_matvec.hip -- the fp64 fused tile kernels: the exact KL's residual r = mu - K alpha0 (kl_gram_resid) and the
// rectangular cross-Gram x vector products, whole and by additive component (gram_matvec_f64, gram_matvec_comp_f64:
// the latent predictors, predict.hip), none of which writes a Gram.  They share apply_factor64, exp_nonpos64 and
// the integer-distance tables.
#include "gram.hpp"
#include "gram_tile.hpp"
#include "kl_resid_bins.hpp"

namespace lvae {

// fp64 residual of the exact-KL solve, r = mu - K alpha0 (K = Gram + noise I, alpha0 = K^-1 mu from the
// fp32 inverse), the matrix never materialised: every lower 64-tile's kernel values are evaluated in
// fp64 (fp64 exp / sin, covariate tests and differences exact, as the reference's double arithmetic)
// and contracted with alpha0 on both sides -- the row sums K_IJ a_J of block I and, off the diagonal,
// the column sums K_IJ^T a_I of block J -- each written once to part[l][other block][row], summed in a
// fixed order by kl_resid_reduce (deterministic).  Grid (G, L) over the tiles t = g, g + G, ...;
// diagonal tiles are evaluated whole.  Components whose Cat / Bin gates are zero on a whole wave skip
// their exp / sin factors.  Refining alpha = alpha0 + K^-1 r (kl_alpha_sym_kernel) then makes K^-1 mu
// (and mu^T K^-1 mu) fp64-accurate up to cond(K)^2 x the inverse's error (elbo_functions.py:27-30).
// exp(x) for x <= 0 to ~1e-15 relative with a 64-entry table: 2^y = 2^m 2^(i/64) 2^f, y = x log2 e,
// f in [0, 1/64) by a degree-5 polynomial (truncation (f ln 2)^6 / 720 < 3e-15) -- about half the fp64
// instructions of the library exp.  tab[i] = 2^(i/64) in LDS.
__device__ inline double exp_nonpos64(double x, const double* __restrict__ tab) {
  constexpr double kLog2e = 1.4426950408889634074;
  constexpr double kLn2 = 0.69314718055994530942;
  const double y = fmax(x * kLog2e, -1100.0);
  const double k = floor(y * 64.0);
  const double f = (y - k * (1.0 / 64.0)) * kLn2;  // in [0, ln2 / 64)
  const int ki = (int)k;
  double p = 1.0 / 120.0;
  p = fma(p, f, 1.0 / 24.0);
  p = fma(p, f, 1.0 / 6.0);
  p = fma(p, f, 0.5);
  p = fma(p, f, 1.0);
  p = fma(p, f, 1.0);
  return ldexp(tab[ki & 63] * p, ki >> 6);
}

// Covariates are often integer-coded (time points, disease times): an RBF / periodic factor of an
// integer distance |d| < kIntTab is read from a per-(component, factor) table of its fp64 values (the
// same function of the same argument), and evaluated directly otherwise.
constexpr int kIntTab = 64;
__device__ inline double factor64_at(int kind, double ad, const double* __restrict__ pf,
                                     const double* __restrict__ tab) {
  if (kind == LVAE_RBF) return exp_nonpos64(-0.5 / (pf[0] * pf[0]) * ad * ad, tab);
  const double sn = sin(ad * (M_PI / pf[1]));
  return exp_nonpos64(-2.0 / (pf[0] * pf[0]) * sn * sn, tab);
}

template <int NTAB = kIntTab>
__device__ inline void apply_factor64(int kind, int d, const double* __restrict__ pf, const double* __restrict__ sx1,
                                      const double* __restrict__ sx2, int tr, int tc, int hf, double (&v)[2][4],
                                      const double* __restrict__ tab, const double* __restrict__ itab) {
  double xr[2], xc[4];
#pragma unroll
  for (int a = 0; a < 2; ++a) xr[a] = sx1[d * kGT + (2 * hf + a) * 16 + tr];
#pragma unroll
  for (int c = 0; c < 4; ++c) xc[c] = sx2[d * kGT + c * 16 + tc];
  if (kind == LVAE_CAT) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) v[a][c] = (xr[a] == xc[c]) ? v[a][c] : 0.0;
  } else if (kind == LVAE_BIN) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) v[a][c] = (xr[a] + xc[c] == 2.0) ? v[a][c] : 0.0;
  } else if (kind == LVAE_RBF || kind == LVAE_PER) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double ad = fabs(xr[a] - xc[c]);
        const bool hit = ad < (double)NTAB && ad == floor(ad);
        v[a][c] *= hit ? itab[hit ? (int)ad : 0] : factor64_at(kind, ad, pf, tab);
      }
  } else {  // LVAE_LIN
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) v[a][c] *= xr[a] * xc[c];
  }
}

// The two helpers below are the gram_matvec kernels' (further down).  kl_resid_tiles keeps its own text of the same
// two loops: calling either helper from it changed its register allocation (142 VGPRs and 48 B / lane of scratch
// against 150 and none), and it is on the training path.
// integer-distance tables of a workgroup: itab[(r MF + f) NTAB + m] = the RBF / periodic factor (r, f) at distance m
// (0 for the other kinds); sp = the dim's parameters in LDS.  The caller's next barrier publishes them.
template <int MC, int MF, int NTAB>
__device__ __attribute__((always_inline)) inline void build_itab64(const DevSpec& s, const double* __restrict__ sp,
                                                                   const double* __restrict__ tab,
                                                                   double* __restrict__ itab) {
  for (int e = threadIdx.x; e < MC * MF * NTAB; e += 256) {
    const int r = e / (MF * NTAB), f = (e / NTAB) % MF, m = e % NTAB;
    double val = 0.0;
    if (r < s.n_comp && f < s.n_fac[r] && (s.kind[r][f] == LVAE_RBF || s.kind[r][f] == LVAE_PER))
      val = factor64_at(s.kind[r][f], (double)m, sp + s.param_idx[r][f], tab);
    itab[e] = val;
  }
}

// k[a][c] += the additive kernel on half hf of the thread's 4 x 4 micro-tile (rows 4 tr + 2 hf + a, columns
// 4 tc + c of the staged tiles): per component the gates first (cheap, exact), then the transcendental factors
// unless the gates zeroed the whole wave
template <int MC, int MF, int NTAB>
__device__ __attribute__((always_inline)) inline void kernel_half64(const DevSpec& s, const double* __restrict__ sp,
                                                                    const double* __restrict__ sx1,
                                                                    const double* __restrict__ sx2, int tr, int tc,
                                                                    int hf, const double* __restrict__ tab,
                                                                    const double* __restrict__ itab,
                                                                    double (&k)[2][4]) {
#pragma unroll 1
  for (int r = 0; r < s.n_comp; ++r) {
    double v[2][4];
    const double sc = sp[s.scale_idx[r]];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) v[a][c] = sc;
#pragma unroll 1
    for (int f = 0; f < s.n_fac[r]; ++f) {
      const int kind = s.kind[r][f];
      if (kind != LVAE_CAT && kind != LVAE_BIN) continue;
      apply_factor64<NTAB>(kind, s.dim[r][f], sp, sx1, sx2, tr, tc, hf, v, tab, itab);
    }
    bool any = false;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) any |= v[a][c] != 0.0;
    if (!__any(any)) continue;
#pragma unroll 1
    for (int f = 0; f < s.n_fac[r]; ++f) {
      const int kind = s.kind[r][f];
      if (kind == LVAE_CAT || kind == LVAE_BIN) continue;
      const int pi = s.param_idx[r][f];
      apply_factor64<NTAB>(kind, s.dim[r][f], sp + (pi < 0 ? 0 : pi), sx1, sx2, tr, tc, hf, v, tab,
                           itab + (r * MF + f) * NTAB);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) k[a][c] += v[a][c];
  }
}

template <int MC, int MF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void kl_resid_tiles(DevSpec s, const double* __restrict__ x, int ldx, int n, int np_,
                                                      int qs, const double* __restrict__ params,
                                                      const double* __restrict__ noise,
                                                      const double* __restrict__ alpha, double* __restrict__ part,
                                                      int ntiles, const int* __restrict__ skip) {
  if (skip && *skip) return;  // the binned path (kl_resid_bins.hip) took this call
  __shared__ double sx1[kGT * kMaxQB];
  __shared__ double sx2[kGT * kMaxQB];
  __shared__ double sp[64];
  __shared__ double sa1[kGT], sa2[kGT];
  __shared__ double cred[4][kGT];
  __shared__ double tab[64];
  __shared__ double itab[MC * MF * kIntTab];  // integer-distance tables, slot r * MF + f
  const int G = gridDim.x, l = blockIdx.y, tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  if (tid < 64) tab[tid] = exp2((double)tid / 64.0);
  const int lane = tid & 63, wv = tid >> 6, nt = np_ / kGT;
  if (tid < s.n_params) sp[tid] = params[(int64_t)l * s.n_params + tid];
  __syncthreads();
  for (int e = tid; e < MC * MF * kIntTab; e += 256) {
    const int r = e / (MF * kIntTab), f = (e / kIntTab) % MF, m = e % kIntTab;
    double val = 0.0;
    if (r < s.n_comp && f < s.n_fac[r] && (s.kind[r][f] == LVAE_RBF || s.kind[r][f] == LVAE_PER))
      val = factor64_at(s.kind[r][f], (double)m, sp + s.param_idx[r][f], tab);
    itab[e] = val;
  }
  const double nz = noise[l];
  const double* al = alpha + (int64_t)l * np_;
  for (int t = blockIdx.x; t < ntiles; t += G) {
    int I, J;
    tri_index(t, I, J);
    const int i0 = I * kGT, j0 = J * kGT;
    __syncthreads();  // the previous tile's LDS readers are done
    stage_cov(x, ldx, n, qs, i0, j0, sx1, sx2);
    if (tid < kGT) sa1[tid] = al[i0 + tid];
    else if (tid < 2 * kGT) sa2[tid - kGT] = al[j0 + tid - kGT];
    __syncthreads();
    // the 4 x 4 micro-tile in two halves of 2 rows (fewer live fp64 registers): row sums of block I
    // (this tile's share, reduced over the 16 lanes tc of each row group) and the column sums of block
    // J accumulated over both halves
    double rs[4], cs[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int hf = 0; hf < 2; ++hf) {
      double k[2][4] = {};
#pragma unroll 1
      for (int r = 0; r < s.n_comp; ++r) {
        double v[2][4];
        const double sc = sp[s.scale_idx[r]];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) v[a][c] = sc;
        // gates first (cheap, exact), then the transcendental factors unless the gates zeroed the wave
#pragma unroll 1
        for (int f = 0; f < s.n_fac[r]; ++f) {
          const int kind = s.kind[r][f];
          if (kind != LVAE_CAT && kind != LVAE_BIN) continue;
          apply_factor64(kind, s.dim[r][f], sp, sx1, sx2, tr, tc, hf, v, tab, itab);
        }
        bool any = false;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) any |= v[a][c] != 0.0;
        if (!__any(any)) continue;
#pragma unroll 1
        for (int f = 0; f < s.n_fac[r]; ++f) {
          const int kind = s.kind[r][f];
          if (kind == LVAE_CAT || kind == LVAE_BIN) continue;
          const int pi = s.param_idx[r][f];
          apply_factor64(kind, s.dim[r][f], sp + (pi < 0 ? 0 : pi), sx1, sx2, tr, tc, hf, v, tab,
                         itab + (r * MF + f) * kIntTab);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) k[a][c] += v[a][c];
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int i = i0 + 4 * tr + 2 * hf + a, j = j0 + 4 * tc + c;
          if (i >= n || j >= n) k[a][c] = 0.0;
          else if (i == j) k[a][c] += nz;
        }
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        double v = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) v += k[a][c] * sa2[4 * tc + c];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
        rs[2 * hf + a] = v;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int a = 0; a < 2; ++a) cs[c] += k[a][c] * sa1[4 * tr + 2 * hf + a];
    }
    if (tc == 0) {
      double* pr = part + ((int64_t)l * nt + J) * np_ + i0 + 4 * tr;
#pragma unroll
      for (int a = 0; a < 4; ++a) pr[a] = rs[a];
    }
    if (I != J) {  // (uniform) column sums of block J: over tr (4 per wave, then the 4 waves)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        cs[c] += __shfl_xor(cs[c], 16, 64);
        cs[c] += __shfl_xor(cs[c], 32, 64);
      }
      if (lane < 16) {
#pragma unroll
        for (int c = 0; c < 4; ++c) cred[wv][4 * tc + c] = cs[c];
      }
      __syncthreads();
      if (tid < kGT) part[((int64_t)l * nt + I) * np_ + j0 + tid] = cred[0][tid] + cred[1][tid] + cred[2][tid] + cred[3][tid];
    }
  }
}

// r[l][i] = mu[l][i] - sum_s part[l][s][i] (fixed order), 0 on the padding.  Grid (np / 256, L).
__global__ __launch_bounds__(256) void kl_resid_reduce(const double* __restrict__ part, const double* __restrict__ muc,
                                                       int n, int np_, double* __restrict__ res,
                                                       const int* __restrict__ skip) {
  const int i = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y, nt = np_ / kGT;
  if (i >= np_ || (skip && *skip)) return;
  double acc = 0.0;
  for (int s = 0; s < nt; ++s) acc += part[((int64_t)l * nt + s) * np_ + i];
  res[(int64_t)l * np_ + i] = i < n ? muc[(int64_t)l * np_ + i] - acc : 0.0;
}

// Fused rectangular cross-Gram x vector in fp64 (the exact-GP predictor, predict.hip: k(X*, X) alpha and the
// refinement residual K alpha0): out[i][l] = sum_j k_l(x1_i, x2_j) v[j][l] (+ diag[l] v[i][l]), the [L, n1, n2]
// Gram never written.  kl_resid_tiles' arithmetic (kernel_half64: apply_factor64, exp_nonpos64, the integer-distance
// tables, the gates before the exp / sin factors) on its 4 x 4 micro-tile in two halves; one workgroup owns the 64-row tile I
// of x1 (staged once) and sweeps the 64-column tiles of its slab of x2, the row sums in registers, covariates and
// v staged in LDS per tile; each output is written once (no atomics: the same bits every run).  Grid
// (row tiles x S, L): slab sl covers column tiles [sl tps, (sl + 1) tps); S == 1 writes out, S > 1 writes
// part[l][sl][i], summed in slab order by gram_matvec_sum.  Rows >= n1 and columns >= n2 of the edge tiles are
// masked.  The spec's dims arrive remapped to the staged slots 0 .. qc.nq - 1 (source columns qc.col[]); QMAX slots
// fit in LDS, with integer-distance tables of NTAB entries (a distance beyond the table is evaluated directly: the
// same function of the same argument, so the table's length does not change a bit of the result).
struct MvCols {
  int32_t nq;
  int32_t col[kMaxQ];
};

// what gram_matvec_tiles and gram_matvec_comp_tiles do before their column tiles: the exp table, the dim's parameters,
// the integer-distance tables and the rows [i0, i0 + 64) of x1 (the first mv_stage_tile's barriers publish them)
template <int MC, int MF, int NTAB>
__device__ __attribute__((always_inline)) inline void mv_prologue(const DevSpec& s, const MvCols& qc,
                                                                  const double* __restrict__ params, int l,
                                                                  const double* __restrict__ x1, int64_t ld1, int n1,
                                                                  int i0, double* __restrict__ sp,
                                                                  double* __restrict__ tab, double* __restrict__ itab,
                                                                  double* __restrict__ sx1) {
  const int tid = threadIdx.x;
  if (tid < 64) tab[tid] = exp2((double)tid / 64.0);
  if (tid < s.n_params) sp[tid] = params[(int64_t)l * s.n_params + tid];
  __syncthreads();
  build_itab64<MC, MF, NTAB>(s, sp, tab, itab);
  for (int e = tid; e < kGT * qc.nq; e += 256) {
    const int r = e / qc.nq, q = e % qc.nq;
    sx1[q * kGT + cov_slot(r)] = (i0 + r < n1) ? x1[(int64_t)(i0 + r) * ld1 + qc.col[q]] : 0.0;
  }
}

// and per column tile: the rows [j0, j0 + 64) of x2 and of dim l's v (vl), between two barriers
__device__ __attribute__((always_inline)) inline void mv_stage_tile(const MvCols& qc, const double* __restrict__ x2,
                                                                    int64_t ld2, int n2, const double* __restrict__ vl,
                                                                    int64_t v_rs, int j0, double* __restrict__ sx2,
                                                                    double* __restrict__ sv) {
  const int tid = threadIdx.x;
  __syncthreads();  // the previous tile's LDS readers are done (first pass: sx1, sp, itab are written)
  for (int e = tid; e < kGT * qc.nq; e += 256) {
    const int r = e / qc.nq, q = e % qc.nq;
    sx2[q * kGT + cov_slot(r)] = (j0 + r < n2) ? x2[(int64_t)(j0 + r) * ld2 + qc.col[q]] : 0.0;
  }
  if (tid < kGT) sv[tid] = (j0 + tid < n2) ? vl[(int64_t)(j0 + tid) * v_rs] : 0.0;
  __syncthreads();
}

template <int MC, int MF, int QMAX, int NTAB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void gram_matvec_tiles(
    DevSpec s, MvCols qc, const double* __restrict__ x1, int64_t ld1, int n1, const double* __restrict__ x2,
    int64_t ld2, int n2, const double* __restrict__ params, const double* __restrict__ diag,
    const double* __restrict__ v, int64_t v_rs, int64_t v_ls, double* __restrict__ out, int64_t o_rs, int64_t o_ls,
    double* __restrict__ part, int S, int tps) {
  __shared__ double sx1[kGT * QMAX];
  __shared__ double sx2[kGT * QMAX];
  __shared__ double sp[64];
  __shared__ double sv[kGT];
  __shared__ double tab[64];
  __shared__ double itab[MC * MF * NTAB];  // integer-distance tables (distances < NTAB), slot r * MF + f
  const int l = blockIdx.y, I = blockIdx.x / S, sl = blockIdx.x % S, tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  const int i0 = I * kGT, ntc = (n2 + kGT - 1) / kGT;
  const int J0 = sl * tps, J1 = min(J0 + tps, ntc);
  mv_prologue<MC, MF, NTAB>(s, qc, params, l, x1, ld1, n1, i0, sp, tab, itab, sx1);
  const double dg = diag ? diag[l] : 0.0;
  const double* vl = v + (int64_t)l * v_ls;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};  // this thread's 4 columns' share of rows 4 tr + (0 .. 3)
  for (int J = J0; J < J1; ++J) {
    const int j0 = J * kGT;
    mv_stage_tile(qc, x2, ld2, n2, vl, v_rs, j0, sx2, sv);
#pragma unroll 1
    for (int hf = 0; hf < 2; ++hf) {
      double k[2][4] = {};
      kernel_half64<MC, MF, NTAB>(s, sp, sx1, sx2, tr, tc, hf, tab, itab, k);
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int i = i0 + 4 * tr + 2 * hf + a;
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int j = j0 + 4 * tc + c;
          double kv = k[a][c];
          if (i >= n1 || j >= n2) kv = 0.0;
          else if (i == j) kv += dg;
          t += kv * sv[4 * tc + c];
        }
        if (hf == 0) acc[a] += t;
        else acc[2 + a] += t;
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) acc[a] += __shfl_xor(acc[a], o, 64);
  if (tc == 0) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int i = i0 + 4 * tr + a;
      if (i >= n1) continue;
      if (S == 1) out[(int64_t)i * o_rs + (int64_t)l * o_ls] = acc[a];
      else part[((int64_t)l * S + sl) * n1 + i] = acc[a];
    }
  }
}

// out[i][l] = sum_s part[l][s][i] in slab order (S == 0: zeros, the product over no columns).  Grid (n1 / 256, L).
__global__ __launch_bounds__(256) void gram_matvec_sum(const double* __restrict__ part, int S, int n1,
                                                       double* __restrict__ out, int64_t o_rs, int64_t o_ls) {
  const int i = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
  if (i >= n1) return;
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc += part[((int64_t)l * S + s) * n1 + i];
  out[(int64_t)i * o_rs + (int64_t)l * o_ls] = acc;
}

// The same product resolved by additive component (the per-component view of the predictors' means, predict.hip):
//   out[r][i][l] = sum_j s_{l,r} prod_f phi_{r,f}(x1_i, x2_j) v[j][l],  sum_r out[r] = gram_matvec_tiles' out
// up to rounding.  gram_matvec_tiles' tiling, staging, tables, gates and masks (mv_prologue, mv_stage_tile); its
// own text of kernel_half64's component loop, because each component's micro-tile is contracted with the staged v at
// once and never summed into k.  The per-(component, row) sums live in LDS (racc: a register array indexed by the runtime component
// index would go to scratch): per tile half and component the row's 16 tc lanes reduce by shuffles and the lane
// tc == 0 adds into its own slot, so every slot has one owner, tiles are added in ascending J, and no barrier or
// atomic guards racc.  A component whose gates zero the whole wave adds nothing; one whose cross-Gram is zero
// everywhere leaves its 0.0.  x2 may differ per latent dim (x2_ls: elements between dims, 0: shared): the
// inducing inputs [L, M, Q].  S == 1 writes out element (r, i, l) at [r o_cs + i o_rs + l o_ls]; S > 1 writes
// part[l][sl][r][i], summed in slab order by gram_matvec_comp_sum.
template <int MC, int MF, int QMAX, int NTAB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void gram_matvec_comp_tiles(
    DevSpec s, MvCols qc, const double* __restrict__ x1, int64_t ld1, int n1, const double* __restrict__ x2,
    int64_t ld2, int64_t x2_ls, int n2, const double* __restrict__ params, const double* __restrict__ v, int64_t v_rs,
    int64_t v_ls, double* __restrict__ out, int64_t o_rs, int64_t o_ls, int64_t o_cs, double* __restrict__ part, int S,
    int tps) {
  __shared__ double sx1[kGT * QMAX];
  __shared__ double sx2[kGT * QMAX];
  __shared__ double sp[64];
  __shared__ double sv[kGT];
  __shared__ double tab[64];
  __shared__ double itab[MC * MF * NTAB];  // integer-distance tables (distances < NTAB), slot r * MF + f
  __shared__ double racc[MC][kGT];         // racc[r][row of the tile]: owned by the lane tc == 0 of the row's group
  const int l = blockIdx.y, I = blockIdx.x / S, sl = blockIdx.x % S, tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  const int i0 = I * kGT, ntc = (n2 + kGT - 1) / kGT;
  const int J0 = sl * tps, J1 = min(J0 + tps, ntc);
  mv_prologue<MC, MF, NTAB>(s, qc, params, l, x1, ld1, n1, i0, sp, tab, itab, sx1);
  if (tc == 0) {
    for (int r = 0; r < s.n_comp; ++r)
#pragma unroll
      for (int a = 0; a < 4; ++a) racc[r][4 * tr + a] = 0.0;
  }
  const double* x2l = x2 + (int64_t)l * x2_ls;
  const double* vl = v + (int64_t)l * v_ls;
  for (int J = J0; J < J1; ++J) {
    const int j0 = J * kGT;
    mv_stage_tile(qc, x2l, ld2, n2, vl, v_rs, j0, sx2, sv);
#pragma unroll 1
    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll 1
      for (int r = 0; r < s.n_comp; ++r) {
        double k[2][4];
        const double sc = sp[s.scale_idx[r]];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) k[a][c] = sc;
        // gates first (cheap, exact), then the transcendental factors unless the gates zeroed the wave
#pragma unroll 1
        for (int f = 0; f < s.n_fac[r]; ++f) {
          const int kind = s.kind[r][f];
          if (kind != LVAE_CAT && kind != LVAE_BIN) continue;
          apply_factor64<NTAB>(kind, s.dim[r][f], sp, sx1, sx2, tr, tc, hf, k, tab, itab);
        }
        bool any = false;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) any |= k[a][c] != 0.0;
        if (!__any(any)) continue;
#pragma unroll 1
        for (int f = 0; f < s.n_fac[r]; ++f) {
          const int kind = s.kind[r][f];
          if (kind == LVAE_CAT || kind == LVAE_BIN) continue;
          const int pi = s.param_idx[r][f];
          apply_factor64<NTAB>(kind, s.dim[r][f], sp + (pi < 0 ? 0 : pi), sx1, sx2, tr, tc, hf, k, tab,
                               itab + (r * MF + f) * NTAB);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const int i = i0 + 4 * tr + 2 * hf + a;
          double t = 0.0;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int j = j0 + 4 * tc + c;
            t += ((i >= n1 || j >= n2) ? 0.0 : k[a][c]) * sv[4 * tc + c];
          }
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) t += __shfl_xor(t, o, 64);
          if (tc == 0) racc[r][4 * tr + 2 * hf + a] += t;
        }
      }
    }
  }
  if (tc != 0) return;
  for (int r = 0; r < s.n_comp; ++r)
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int i = i0 + 4 * tr + a;
      if (i >= n1) continue;
      const double t = racc[r][4 * tr + a];
      if (S == 1) out[(int64_t)r * o_cs + (int64_t)i * o_rs + (int64_t)l * o_ls] = t;
      else part[(((int64_t)l * S + sl) * s.n_comp + r) * n1 + i] = t;
    }
}

// out[r][i][l] = sum_s part[l][s][r][i] in slab order (S == 0: zeros, the product over no columns).  Grid
// (n1 / 256, L, R).
__global__ __launch_bounds__(256) void gram_matvec_comp_sum(const double* __restrict__ part, int S, int R, int n1,
                                                            double* __restrict__ out, int64_t o_rs, int64_t o_ls,
                                                            int64_t o_cs) {
  const int i = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y, r = blockIdx.z;
  if (i >= n1) return;
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc += part[(((int64_t)l * S + s) * R + r) * n1 + i];
  out[(int64_t)r * o_cs + (int64_t)i * o_rs + (int64_t)l * o_ls] = acc;
}

// host launchers (their contracts: gram.hpp)
size_t kl_resid_partials_bytes(int np_, int L) { return (size_t)L * (np_ / kGT) * np_ * sizeof(double); }

int kl_gram_resid(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int np_, int L,
                  const double* params, const double* noise, const double* alpha0, const double* muc, double* part,
                  double* res, void* rbws, hipStream_t st) {
  const int bucket = spec_bucket(spec);
  const int qs = spec_qs(spec);
  if (!bucket || qs > kMaxQB || qs > ldx || spec->n_params > 64) return -1;
  const DevSpec ds = to_dev(spec);
  const int nt = np_ / kGT, ntiles = nt * (nt + 1) / 2;
  // ~8 resident workgroups per CU in 2 rounds; one round of 2 per CU behind the binned path (when it
  // runs, these launches only read the flag and exit: fewer of them)
  int G = ((rbws ? 512 : 2048) + L - 1) / L;
  G = G < ntiles ? G : ntiles;
  // rbws (the binned residual's planned workspace, kl_resid_bins_plan): integer-coded covariates take
  // the binned O(N W) residual and the tiled kernels below exit at once (checked on the device: *skip)
  int* skip = nullptr;
  if (rbws)
    LVAE_TRY(kl_resid_bins(spec, x, ldx, n, np_, L, params, noise, alpha0, muc, res, rbws, &skip, st));
  if (bucket == 1)
    kl_resid_tiles<8, 2><<<dim3(G, L), 256, 0, st>>>(ds, x, ldx, n, np_, qs, params, noise, alpha0, part, ntiles, skip);
  else
    kl_resid_tiles<16, 4><<<dim3(G, L), 256, 0, st>>>(ds, x, ldx, n, np_, qs, params, noise, alpha0, part, ntiles, skip);
  kl_resid_reduce<<<dim3(cdiv(np_, 256), L), 256, 0, st>>>(part, muc, n, np_, res, skip);
  LVAE_CHECK_LAUNCH();
  return 0;
}

// Column slabs of the fused Gram x vector, a function of (n1, n2, L) alone: about 512 workgroups in all (two per
// CU at gram_matvec_tiles' occupancy), a slab no shorter than 4 column tiles unless x2 has fewer (every workgroup
// builds its tables and stages its rows of x1 first), every slab non-empty.
static int matvec_slabs(int n1, int n2, int L, int* tps_out) {
  const int64_t rows = (int64_t)cdiv(n1, kGT) * L;
  const int ntc = cdiv(n2, kGT);
  int64_t S = rows > 0 ? 512 / rows : 1;
  const int cap = cdiv(ntc, 4);
  S = S > cap ? cap : S;
  S = S < 1 ? 1 : S;
  const int tps = ntc > 0 ? cdiv(ntc, S) : 1;
  if (tps_out) *tps_out = tps;
  return ntc > 0 ? cdiv(ntc, tps) : 1;
}

// the covariate columns the spec reads, compacted to staged slots (ds.dim rewritten to the slots); false when a
// factor's dim is outside 0 .. kMaxQ - 1 (lvae_gram_f64's limit, so at most kMaxQ distinct columns); *ld_min = 1 + the largest column
static bool matvec_cols(const lvae_kernel_spec* spec, DevSpec& ds, MvCols& qc, int* ld_min) {
  ds = to_dev(spec);
  qc.nq = 0;
  *ld_min = 1;
  for (int r = 0; r < spec->n_comp; ++r)
    for (int f = 0; f < spec->n_fac[r]; ++f) {
      const int d = spec->dim[r][f];
      if (d < 0 || d >= kMaxQ) return false;
      int q = 0;
      while (q < qc.nq && qc.col[q] != d) ++q;
      if (q == qc.nq) {
        if (qc.nq == kMaxQ) return false;
        qc.col[qc.nq++] = d;
      }
      ds.dim[r][f] = q;
      *ld_min = d + 1 > *ld_min ? d + 1 : *ld_min;
    }
  return true;
}

int gram_matvec_spec_ld(const lvae_kernel_spec* spec) {
  DevSpec ds;
  MvCols qc;
  int ld_min = 0;
  return spec && spec_bucket(spec) && matvec_cols(spec, ds, qc, &ld_min) ? ld_min : 0;
}

size_t gram_matvec_ws_bytes(int n1, int n2, int L) {
  if (n1 <= 0 || n2 <= 0 || L <= 0) return 0;
  const int S = matvec_slabs(n1, n2, L, nullptr);
  return S > 1 ? (size_t)L * S * n1 * sizeof(double) : 0;
}

// What the two fused-product hosts launch with: the spec remapped to its staged slots, the strides of v and out in
// either layout, the slabs.  Three helpers hold the checks the hosts share, in the public entries' order; a host's
// own checks (-10; -16 and -17) stand in the host, between them.
struct MvPlan {
  DevSpec ds;
  MvCols qc;
  int bucket, S, tps;
  int64_t v_rs, v_ls, o_rs, o_ls;
};

// codes -1 to -9: the spec, the sizes, the inputs.  n1 == 0 ends the checks with 0: the hosts return there.
static int matvec_check_in(const lvae_kernel_spec* spec, const double* x1, int64_t ld1, int n1, const double* x2,
                           int64_t ld2, int n2, int L, const double* params, MvPlan& p) {
  if (!spec) return -1;
  p.bucket = spec_bucket(spec);
  int ld_min = 1;
  if (!p.bucket || !matvec_cols(spec, p.ds, p.qc, &ld_min)) return -1;
  if (n1 < 0) return -4;
  if (n2 < 0) return -7;
  if (L < 1) return -8;
  if (n1 == 0) return 0;
  if (!x1) return -2;
  if (ld1 < ld_min) return -3;
  if (n2 > 0 && !x2) return -5;
  if (n2 > 0 && ld2 < ld_min) return -6;
  return params ? 0 : -9;
}

// codes -11 to -14: v and out, then their strides
static int matvec_check_out(int n1, int n2, int L, const double* v, int64_t ld_v, int v_t, const double* out,
                            int64_t ld_out, int o_t, MvPlan& p) {
  if (n2 > 0 && !v) return -11;
  if (n2 > 0 && ld_v < (v_t ? n2 : L)) return -12;
  if (!out) return -13;
  if (ld_out < (o_t ? n1 : L)) return -14;
  p.v_rs = v_t ? 1 : ld_v, p.v_ls = v_t ? ld_v : 1, p.o_rs = o_t ? 1 : ld_out, p.o_ls = o_t ? ld_out : 1;
  return 0;
}

// the slabs, and code -15: more than one slab needs the (256-byte aligned) workspace for the partials
static int matvec_check_ws(int n1, int n2, int L, const void* workspace, MvPlan& p) {
  p.tps = 1;
  p.S = n2 > 0 ? matvec_slabs(n1, n2, L, &p.tps) : 0;
  return p.S > 1 && (!workspace || ((uintptr_t)workspace & 255)) ? -15 : 0;
}

// KERNEL<MC, MF, QMAX, NTAB> on the plan's grid: (8, 2) reads at most 16 columns; (16, 4) beyond 16 takes the 32-slot
// image with 16-entry distance tables (2 x 16 KiB of covariates + 8 KiB of tables, where 64-entry tables alone take
// 32 KiB of the 64 KiB of LDS).  gram_matvec_comp_tiles has racc on top of each image (4 KiB for 8 components, 8 KiB
// for 16).
#define LVAE_MV_LAUNCH(KERNEL, ...)                                                                     \
  do {                                                                                                  \
    const dim3 grid(cdiv(n1, kGT) * p.S, L);                                                            \
    if (p.bucket == 1) KERNEL<8, 2, kMaxQB, kIntTab><<<grid, 256, 0, st>>>(__VA_ARGS__);                \
    else if (p.qc.nq <= kMaxQB) KERNEL<16, 4, kMaxQB, kIntTab><<<grid, 256, 0, st>>>(__VA_ARGS__);      \
    else KERNEL<16, 4, kMaxQ, 16><<<grid, 256, 0, st>>>(__VA_ARGS__);                                   \
  } while (0)

int gram_matvec_f64(const lvae_kernel_spec* spec, const double* x1, int64_t ld1, int n1, const double* x2, int64_t ld2,
                    int n2, int L, const double* params, const double* diag, const double* v, int64_t ld_v, int v_t,
                    double* out, int64_t ld_out, int o_t, void* workspace, hipStream_t st) {
  MvPlan p;
  LVAE_TRY(matvec_check_in(spec, x1, ld1, n1, x2, ld2, n2, L, params, p));
  if (n1 == 0) return 0;
  if (diag && n1 != n2) return -10;
  LVAE_TRY(matvec_check_out(n1, n2, L, v, ld_v, v_t, out, ld_out, o_t, p));
  LVAE_TRY(matvec_check_ws(n1, n2, L, workspace, p));
  double* part = (double*)workspace;
  if (p.S >= 1)
    LVAE_MV_LAUNCH(gram_matvec_tiles, p.ds, p.qc, x1, ld1, n1, x2, ld2, n2, params, diag, v, p.v_rs, p.v_ls, out,
                   p.o_rs, p.o_ls, part, p.S, p.tps);
  if (p.S != 1) gram_matvec_sum<<<dim3(cdiv(n1, 256), L), 256, 0, st>>>(part, p.S, n1, out, p.o_rs, p.o_ls);
  LVAE_CHECK_LAUNCH();
  return 0;
}

size_t gram_matvec_comp_ws_bytes(int n1, int n2, int L, int n_comp) {  // (a slab's partial per component)
  return n_comp > 0 ? n_comp * gram_matvec_ws_bytes(n1, n2, L) : 0;
}

int gram_matvec_comp_f64(const lvae_kernel_spec* spec, const double* x1, int64_t ld1, int n1, const double* x2,
                         int64_t ld2, int64_t x2_stride_l, int n2, int L, const double* params, const double* v,
                         int64_t ld_v, int v_t, double* out, int64_t ld_out, int o_t, int64_t ostride_r,
                         void* workspace, hipStream_t st) {
  MvPlan p;
  LVAE_TRY(matvec_check_in(spec, x1, ld1, n1, x2, ld2, n2, L, params, p));
  if (n1 == 0) return 0;
  LVAE_TRY(matvec_check_out(n1, n2, L, v, ld_v, v_t, out, ld_out, o_t, p));
  if (n2 > 0 && x2_stride_l < 0) return -16;
  const int R = spec->n_comp;
  if (R > 1 && ostride_r < (int64_t)(o_t ? L : n1) * ld_out) return -17;
  LVAE_TRY(matvec_check_ws(n1, n2, L, workspace, p));
  double* part = (double*)workspace;
  if (p.S >= 1)
    LVAE_MV_LAUNCH(gram_matvec_comp_tiles, p.ds, p.qc, x1, ld1, n1, x2, ld2, x2_stride_l, n2, params, v, p.v_rs,
                   p.v_ls, out, p.o_rs, p.o_ls, ostride_r, part, p.S, p.tps);
  if (p.S != 1)
    gram_matvec_comp_sum<<<dim3(cdiv(n1, 256), L, R), 256, 0, st>>>(part, p.S, R, n1, out, p.o_rs, p.o_ls, ostride_r);
  LVAE_CHECK_LAUNCH();
  return 0;
}
#undef LVAE_MV_LAUNCH

}  // namespace lvae

extern "C" {

size_t lvae_gram_matvec_workspace_size(int n1, int n2, int L) { return lvae::gram_matvec_ws_bytes(n1, n2, L); }

int lvae_gram_matvec_f64(const lvae_kernel_spec* spec, const double* x1, int64_t ld1, int n1, const double* x2,
                         int64_t ld2, int n2, int L, const double* params, const double* diag, const double* v,
                         int64_t ld_v, double* out, int64_t ld_out, void* workspace, void* stream) {
  return lvae::gram_matvec_f64(spec, x1, ld1, n1, x2, ld2, n2, L, params, diag, v, ld_v, 0, out, ld_out, 0, workspace,
                               (hipStream_t)stream);
}

size_t lvae_gram_matvec_comp_workspace_size(int n1, int n2, int L, int n_comp) {
  return lvae::gram_matvec_comp_ws_bytes(n1, n2, L, n_comp);
}

int lvae_gram_matvec_comp_f64(const lvae_kernel_spec* spec, const double* x1, int64_t ld1, int n1, const double* x2,
                              int64_t ld2, int64_t x2_stride_l, int n2, int L, const double* params, const double* v,
                              int64_t ld_v, double* out, int64_t ld_out, int64_t ostride_r, void* workspace,
                              void* stream) {
  return lvae::gram_matvec_comp_f64(spec, x1, ld1, n1, x2, ld2, x2_stride_l, n2, L, params, v, ld_v, 0, out, ld_out, 0,
                                    ostride_r, workspace, (hipStream_t)stream);
}

}  // extern "C"
