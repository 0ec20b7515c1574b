// kl_gram.hip -- the exact KL's fp32 covariance and its fused adjoint (kl_closed.hip): K = Gram + noise I as lower
// 64-tiles (kl_gram_fill) and the contraction of G = 1/2 (K^-1 - S - a a^T) with dK / dtheta (kl_gram_bwd), each
// with a direct path (fp64 or fp32 covariates) and a table path, chosen on the device by the covariates' class.
//
// 4 x 4 micro-tiles: a 256-thread workgroup owns a 64 x 64 tile; thread (tr, tc) = (tid >> 4, tid & 15) owns rows
// 4 tr + a and columns 4 tc + c (a, c < 4): per factor it reads 4 row and 4 column covariates (fp64, LDS) for 16
// elements and the tile rows go out / come in as float4 (16 B per lane, 256 contiguous bytes per row and 16 lanes).
// The (uniform) spec is walked once per 16 elements.  Category / binary tests and covariate differences stay in fp64
// (exact 0/1 and exact differences, as the reference's double arithmetic); factor values, products and sums are fp32
// (the covariance is fp32); RBF / periodic use the native exp2.
#include "gram.hpp"
#include "gram_tab.hpp"
#include "gram_tile.hpp"
#include "kl_hyper.hpp"

namespace lvae {

typedef float g_f32x4 __attribute__((ext_vector_type(4)));

// Integer-coded covariates (the common case: subject / time / class indices) take an fp32 path in the
// Regime B Gram kernels: covariates staged as fp32, category / binary tests and differences in fp32 --
// exact, and bitwise the same Gram, when every covariate is an integer of magnitude < 2^22 (the
// fp64 path rounds the exact fp64 difference to fp32 as well).  One workgroup, written by the factor for
// its kernels: flag 0 = not integer-coded (fp64 covariates), 1 = integer-coded, 2 = integer-coded and
// every dim of tabmask spans < kTabD values (the table path, gram_tab_*; tab_ok: the spec allows it).
__global__ __launch_bounds__(1024) void cov_int_check_kernel(const double* __restrict__ x, int ldx, int n, int qs,
                                                             int tab_ok, int tabmask, int* __restrict__ flag) {
  __shared__ int bad, wide;
  __shared__ int lo[kMaxQB], hi[kMaxQB];
  if (threadIdx.x == 0) bad = wide = 0;
  if (threadIdx.x < kMaxQB) {
    lo[threadIdx.x] = INT_MAX;
    hi[threadIdx.x] = INT_MIN;
  }
  __syncthreads();
  int b = 0;
  for (int q = 0; q < qs; ++q) {
    int mn = INT_MAX, mx = INT_MIN;
    for (int r = threadIdx.x; r < n; r += 1024) {
      const double v = x[(int64_t)r * ldx + q];
      const bool ok = v == rint(v) && fabs(v) < 4194304.0;
      b |= !ok;
      if (ok) {
        mn = min(mn, (int)v);
        mx = max(mx, (int)v);
      }
    }
    if ((tabmask >> q) & 1) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, __shfl_xor(mn, o, 64));
        mx = max(mx, __shfl_xor(mx, o, 64));
      }
      if ((threadIdx.x & 63) == 0) {
        atomicMin(&lo[q], mn);
        atomicMax(&hi[q], mx);
      }
    }
  }
  if (__any(b) && (threadIdx.x & 63) == 0) atomicOr(&bad, 1);
  __syncthreads();
  if (threadIdx.x < qs && ((tabmask >> threadIdx.x) & 1) && hi[threadIdx.x] - lo[threadIdx.x] >= kTabD)
    atomicOr(&wide, 1);
  __syncthreads();
  if (threadIdx.x == 0) *flag = bad ? 0 : (tab_ok && !wide ? 2 : 1);
}

// factor (kind, dim d, params pf) on the thread's 4 x 4 micro-tile: v[a][c] *= phi(x_i, x_j)
template <typename CT>
__device__ inline void apply_factor(int kind, int d, const float* __restrict__ pf, const CT* __restrict__ sx1,
                                    const CT* __restrict__ sx2, int tr, int tc, float (&v)[4][4]) {
  CT xr[4], xc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) xr[a] = sx1[d * kGT + a * 16 + tr];
#pragma unroll
  for (int c = 0; c < 4; ++c) xc[c] = sx2[d * kGT + c * 16 + tc];
  if (kind == LVAE_CAT) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) v[a][c] = (xr[a] == xc[c]) ? v[a][c] : 0.f;
  } else if (kind == LVAE_BIN) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) v[a][c] = (xr[a] + xc[c] == CT(2)) ? v[a][c] : 0.f;
  } else if (kind == LVAE_RBF) {
    const float ell = pf[0], cf = -0.5f * kLog2e / (ell * ell);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float df = float(xr[a] - xc[c]);
        v[a][c] *= __builtin_amdgcn_exp2f(cf * df * df);
      }
  } else if (kind == LVAE_PER) {
    const float ell = pf[0], cf = -2.f * kLog2e / (ell * ell);
    const double ip = 1.0 / (double)pf[1];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float sn = per_sin(fabs(double(xr[a]) - double(xc[c])) * ip);
        v[a][c] *= __builtin_amdgcn_exp2f(cf * sn * sn);
      }
  } else {  // LVAE_LIN
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) v[a][c] *= float(double(xr[a]) * double(xc[c]));
  }
}

// component r's factors on the micro-tile, Cat / Bin gates first: when they leave the whole WAVE at zero
// (e.g. Cat(subject) on a tile pair of different subjects) the parametrised factors (exp / sin) are
// skipped and false returned (v is then 0: the component adds nothing; wave-uniform, no divergence)
template <typename CT>
__device__ inline bool apply_factors_gated(const DevSpec& s, int r, const float* __restrict__ sp,
                                           const CT* __restrict__ sx1, const CT* __restrict__ sx2, int tr,
                                           int tc, float (&v)[4][4]) {
  bool gated = false;
#pragma unroll 1
  for (int f = 0; f < s.n_fac[r]; ++f) {
    const int kind = s.kind[r][f];
    if (kind != LVAE_CAT && kind != LVAE_BIN) continue;
    apply_factor(kind, s.dim[r][f], sp, sx1, sx2, tr, tc, v);
    gated = true;
  }
  if (gated) {
    bool any = false;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) any |= v[a][c] != 0.f;
    if (!__any(any)) return false;
  }
#pragma unroll 1
  for (int f = 0; f < s.n_fac[r]; ++f) {
    const int kind = s.kind[r][f];
    if (kind == LVAE_CAT || kind == LVAE_BIN) continue;
    const int pi = s.param_idx[r][f];
    apply_factor(kind, s.dim[r][f], sp + (pi < 0 ? 0 : pi), sx1, sx2, tr, tc, v);
  }
  return true;
}

// the adjoint's per-factor sums over the micro-tile: u0 = sum v d^2 (RBF) or sum v sin^2 u (PER),
// u1 = sum v |d| sin 2u (PER); the ingredients are recomputed so only v stays live
template <typename CT>
__device__ inline void factor_sums(int kind, int d, const float* __restrict__ pf, const CT* __restrict__ sx1,
                                   const CT* __restrict__ sx2, int tr, int tc, const float (&v)[4][4], float& u0,
                                   float& u1) {
  CT xr[4], xc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) xr[a] = sx1[d * kGT + a * 16 + tr];
#pragma unroll
  for (int c = 0; c < 4; ++c) xc[c] = sx2[d * kGT + c * 16 + tc];
  u0 = u1 = 0.f;
  if (kind == LVAE_RBF) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float df = float(xr[a] - xc[c]);
        u0 += v[a][c] * df * df;
      }
  } else {  // LVAE_PER
    const double ip = 1.0 / (double)pf[1];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double ad = fabs(double(xr[a]) - double(xc[c])), t = ad * ip;
        const float sn = per_sin(t);
        u0 += v[a][c] * sn * sn;
        u1 += v[a][c] * float(ad) * per_sin2(t);
      }
  }
}

// covariate prefetch: each thread carries up to kPre (row, dim) values of the next tile's two
// row blocks in registers while the current tile is evaluated
constexpr int kPre = (kGT * kMaxQB + 255) / 256;
template <typename T>
struct CovPrefetchT {
  T a[kPre], b[kPre];
  __device__ inline void load(const double* __restrict__ x, int ldx, int n, int qs, int i0, int j0) {
#pragma unroll
    for (int u = 0; u < kPre; ++u) {
      const int e = threadIdx.x + 256 * u, r = e / qs, q = e % qs;
      const bool ok = e < kGT * qs;
      a[u] = (ok && i0 + r < n) ? T(x[(int64_t)(i0 + r) * ldx + q]) : T(0);
      b[u] = (ok && j0 + r < n) ? T(x[(int64_t)(j0 + r) * ldx + q]) : T(0);
    }
  }
  template <typename CT>
  __device__ inline void store(int qs, CT* __restrict__ sx1, CT* __restrict__ sx2) const {
#pragma unroll
    for (int u = 0; u < kPre; ++u) {
      const int e = threadIdx.x + 256 * u, r = e / qs, q = e % qs;
      if (e < kGT * qs) {
        sx1[q * kGT + cov_slot(r)] = CT(a[u]);
        sx2[q * kGT + cov_slot(r)] = CT(b[u]);
      }
    }
  }
};
using CovPrefetch = CovPrefetchT<double>;
using CovPrefetchF = CovPrefetchT<float>;  // integer-coded covariates (flag >= 1: exact in fp32), half the registers

// the micro-tile of a tile that meets the diagonal or the padding, to K: + noise on the diagonal, identity on the padding
__device__ inline void fill_store_edge(const float (&out)[4][4], float nz, int n, int np_, int i0, int j0, int tr,
                                       int tc, float* __restrict__ o) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + 4 * tr + a;
    g_f32x4 w;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + 4 * tc + c;
      float e = out[a][c];
      if (i == j) e += nz;
      if (i >= n || j >= n) e = (i == j) ? 1.0f : 0.0f;
      w[c] = e;
    }
    *reinterpret_cast<g_f32x4*>(o + (int64_t)i * np_ + j0 + 4 * tc) = w;
  }
}

// Lower 64-tiles of the padded [np, np] covariance, f32 out, + noise on the diagonal, identity on
// the padding rows / cols (keeps log|K| and the leading block of K^-1).  Grid (G, L): workgroup g
// of dim l fills the tiles t = g, g + G, ... (t -> (I, J), I >= J), prefetching the next tile's
// covariates under the current tile's arithmetic.  HBM-write-bound: 4 B per element.
// CT: the covariates' type in LDS; both instantiations are launched and the one that does not match the
// factor's covariate flag (cov_int_check_kernel: float for integer covariates) exits at once.
template <int MC, int MF, typename CT>
__global__ __launch_bounds__(256) void gram_sq_fill_kernel(DevSpec s, const double* __restrict__ x, int ldx,
                                                           int n, int np_, int qs,
                                                           const double* __restrict__ params,
                                                           const double* __restrict__ noise,
                                                           float* __restrict__ K, int ntiles,
                                                           const int* __restrict__ covflag) {
  if (*covflag != (sizeof(CT) == 4 ? 1 : 0)) return;  // (uniform, before any barrier)
  __shared__ CT sx1[kGT * kMaxQB];
  __shared__ CT sx2[kGT * kMaxQB];
  __shared__ float sp[64];
  const int G = gridDim.x, l = blockIdx.y, tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  if (tid < s.n_params) sp[tid] = float(params[(int64_t)l * s.n_params + tid]);
  const float nz = float(noise[l]);
  float* o = K + (int64_t)l * np_ * np_;
  int t = blockIdx.x, I, J;
  if (t >= ntiles) return;
  tri_index(t, I, J);
  CovPrefetch pf;
  pf.load(x, ldx, n, qs, I * kGT, J * kGT);
  pf.store(qs, sx1, sx2);
  __syncthreads();
  for (; t < ntiles; t += G) {
    const int i0 = I * kGT, j0 = J * kGT;
    int In = 0, Jn = 0;
    const bool more = t + G < ntiles;
    if (more) {
      tri_index(t + G, In, Jn);
      pf.load(x, ldx, n, qs, In * kGT, Jn * kGT);
    }
    float out[4][4] = {};
#pragma unroll 1
    for (int r = 0; r < s.n_comp; ++r) {  // (rolled: the spec is uniform; keeps the live set small)
      float v[4][4];
      const float sc = sp[s.scale_idx[r]];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) v[a][c] = sc;
      if (!apply_factors_gated(s, r, sp, sx1, sx2, tr, tc, v)) continue;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) out[a][c] += v[a][c];
    }
    fill_store_edge(out, nz, n, np_, i0, j0, tr, tc, o);
    if (more) {
      __syncthreads();  // every reader of this tile's covariates is done
      pf.store(qs, sx1, sx2);
      __syncthreads();
      I = In, J = Jn;
    }
  }
}

// Fused adjoint for the exact KL: G = 1/2 (Kinv - S - a a^T) formed on the fly from the symmetric
// K^-1 (f32), S = K^-1 V K^-1 (f32, lower tiles) and a = K^-1 mu (f64), contracted with dK/dtheta.
// Grid (G, L): workgroup g of dim l loops over the lower 64-tiles t = g, g + G, ...; every thread
// keeps fp32 sums per PARAMETER (one slot per parameter -- each has exactly one -- plus the noise
// slot kNoiseSlot) in its private LDS column over 4 tiles (64 elements), then folds the wave sums
// into fp64 LDS accumulators; one partial per (dim, slot, workgroup) -> part[l][slot][g].  Raw sums
// (kl_gram_bwd_reduce applies the per-parameter constants):
//   scale s_r           sum w g prod_r                              (d k / d s_r = prod_r)
//   RBF lengthscale     sum w g k_r d^2                              x 1 / l^3
//   PER l / period      sum w g k_r sin^2 u,  sum w g k_r |d| sin 2u  x 4 / l^3,  2 pi / (l^2 p^2)
//   noise               sum_i G_ii
// with k_r = s_r prod_r and w = 2 strictly below the diagonal, 1 on it.
constexpr int kNoiseSlot = 64;
constexpr int kBwdSlots = 65;

// kl_gram_bwd_tiles and its table twin share this fold of the threads' fp32 sums (tacc(q): slot q's, by reference) and
// dd into the fp64 wave slots.  Each keeps its own text of the K^-1 / S row load and of forming g: either as a shared
// helper changed both kernels' registers (150 / 133 / 145 VGPRs against 159 / 141 / 147); they are on the training path.
template <typename TAcc>
__device__ __attribute__((always_inline)) inline void bwd_flush(TAcc& tacc, int np_s, float& dd,
                                                                double (&wred)[4][kBwdSlots]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  tacc(kNoiseSlot) += dd;
  dd = 0.f;
  for (int q = 0; q < kBwdSlots; ++q) {
    if (q >= np_s && q != kNoiseSlot) continue;  // (uniform)
    const float w = wave_sum(tacc(q));
    if (lane == 0) wred[wv][q] += (double)w;
    tacc(q) = 0.f;
  }
}

template <int MC, int MF, typename CT>
__global__ __launch_bounds__(256) void kl_gram_bwd_tiles(DevSpec s, const double* __restrict__ x, int ldx, int n,
                                                         int np_, int qs, const double* __restrict__ params,
                                                         const float* __restrict__ Kinv,
                                                         const float* __restrict__ S,
                                                         const float* __restrict__ Sx, int nsplit,
                                                         const double* __restrict__ alpha,
                                                         double* __restrict__ part, int ntiles,
                                                         const int* __restrict__ covflag) {
  if (*covflag != (sizeof(CT) == 4 ? 1 : 0)) return;  // (uniform, before any barrier)
  __shared__ CT sx1[kGT * kMaxQB];
  __shared__ CT sx2[kGT * kMaxQB];
  __shared__ float sp[64];
  __shared__ float sa1[kGT], sa2[kGT];
  __shared__ double wred[4][kBwdSlots];
  // per-thread fp32 sums (thread-private columns: no races): slots 0..n_params-1, then the noise
  // at row n_params (dynamic LDS: (n_params + 1) x 256 floats)
  extern __shared__ float tacc_dyn[];
  const int G = gridDim.x, g0 = blockIdx.x, l = blockIdx.y, tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  const int np_s = s.n_params;
  auto tacc = [&](int q) -> float& { return tacc_dyn[(q == kNoiseSlot ? np_s : q) * 256 + tid]; };
  if (tid < np_s) sp[tid] = float(params[(int64_t)l * np_s + tid]);
  for (int e = tid; e < 4 * kBwdSlots; e += 256) (&wred[0][0])[e] = 0.0;
  for (int q = 0; q < np_s; ++q) tacc(q) = 0.f;
  tacc(kNoiseSlot) = 0.f;
  const float* ki = Kinv + (int64_t)l * np_ * np_;
  const float* si = S + (int64_t)l * np_ * np_;
  float dd = 0.f;
  int since_flush = 0;
  for (int t = g0; t < ntiles; t += G) {
    int I, J;
    tri_index(t, I, J);
    const int i0 = I * kGT, j0 = J * kGT;
    // this tile's K^-1 / S rows first: their latency overlaps the covariate staging and barriers
    g_f32x4 kv4[4], sv4[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int64_t o = (int64_t)(i0 + 4 * tr + a) * np_ + j0 + 4 * tc;
      kv4[a] = __builtin_nontemporal_load(reinterpret_cast<const g_f32x4*>(ki + o));
      sv4[a] = __builtin_nontemporal_load(reinterpret_cast<const g_f32x4*>(si + o));
    }
    for (int q = 1; q < nsplit; ++q) {  // K-split partials of S (syrk_x3_splits)
      const float* sq = Sx + (int64_t)(q - 1) * gridDim.y * np_ * np_ + (int64_t)l * np_ * np_;
#pragma unroll
      for (int a = 0; a < 4; ++a)
        sv4[a] += __builtin_nontemporal_load(
            reinterpret_cast<const g_f32x4*>(sq + (int64_t)(i0 + 4 * tr + a) * np_ + j0 + 4 * tc));
    }
    __syncthreads();  // previous tile's LDS readers done
    stage_cov(x, ldx, n, qs, i0, j0, sx1, sx2);
    if (tid < kGT) sa1[tid] = float(alpha[(int64_t)l * np_ + i0 + tid]);
    else if (tid < 2 * kGT) sa2[tid - kGT] = float(alpha[(int64_t)l * np_ + j0 + tid - kGT]);
    __syncthreads();
    float g[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int i = i0 + 4 * tr + a;
      const g_f32x4 kv = kv4[a], sv = sv4[a];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + 4 * tc + c;
        const float gv = 0.5f * (kv[c] - sv[c] - sa1[4 * tr + a] * sa2[4 * tc + c]);
        const bool in = i < n && j < n && j <= i;
        if (in && i == j) dd += gv;
        g[a][c] = in ? ((i == j) ? gv : 2.f * gv) : 0.f;
      }
    }
#pragma unroll 1
    for (int r = 0; r < s.n_comp; ++r) {
      float v[4][4];
      const float sc = sp[s.scale_idx[r]];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) v[a][c] = g[a][c];
      if (!apply_factors_gated(s, r, sp, sx1, sx2, tr, tc, v)) continue;  // (every sum below is 0)
      // v = g prod_r: the scale's slot; g k_r = sc v for the parametrised factors
      float ssum = 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) ssum += v[a][c];
      tacc(s.scale_idx[r]) += ssum;
#pragma unroll 1
      for (int f = 0; f < s.n_fac[r]; ++f) {
        const int kind = s.kind[r][f];
        if (kind == LVAE_RBF || kind == LVAE_PER) {
          const int pi = s.param_idx[r][f];
          float u0, u1;
          factor_sums(kind, s.dim[r][f], sp + pi, sx1, sx2, tr, tc, v, u0, u1);
          tacc(pi) += sc * u0;
          if (kind == LVAE_PER) tacc(pi + 1) += sc * u1;
        }
      }
    }
    if (++since_flush == 4 || t + G >= ntiles) {  // fold the fp32 sums into the fp64 wave slots
      since_flush = 0;
      bwd_flush(tacc, np_s, dd, wred);
    }
  }
  __syncthreads();
  for (int sl = tid; sl < kBwdSlots; sl += 256)
    part[((int64_t)l * kBwdSlots + sl) * G + g0] = wred[0][sl] + wred[1][sl] + wred[2][sl] + wred[3][sl];
}

// ------------------------------------------------------------------------------------------
// Table path of the Regime B Gram fill and adjoint (covariate flag 2: integer-coded covariates whose
// continuous dims each span < kTabD values).  Every component is gates (Cat / Bin tests) times at most
// one RBF / periodic factor of |x_i[d] - x_j[d]|, so with B distinct gates and the components grouped by
// the dim of their continuous factor, an element of K is
//   K_ij = sum_g T_g[bits_ij][|x_i[d_g] - x_j[d_g]|],   T_g[b][m] = sum_{r in g, gates_r in b} s_r phi_r(m)
// (bits_ij: which of the B gates pass; components with no continuous factor join group 0 as
// d-independent terms), and each raw adjoint sum is  sum_ij w g_ij D_p[bits_ij][|d_ij|]  with D_p the
// same derivative factors as kl_gram_bwd_tiles'.  The tables (fp32, from the same fp32 formulas as the
// direct path) are built per workgroup into LDS; per element the work drops to the B gate tests, one
// difference + table read per group and, in the adjoint, one FMA per parameter.
// ------------------------------------------------------------------------------------------
#ifndef LVAE_TAB_WPE
#define LVAE_TAB_WPE 3  // the table adjoint's waves per SIMD (register cap)
#endif
// the micro-tile's gate bits as table row offsets: bits[a][c] = (sum_b pass_b << b) * kTabR
__device__ inline void tab_bits(const GramTab& t, const float* __restrict__ sx1, const float* __restrict__ sx2,
                                int tr, int tc, int (&bits)[4][4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) bits[a][c] = 0;
#pragma unroll 1
  for (int b = 0; b < t.nbits; ++b) {
    const int d = t.bdim[b], bit = kTabR << b;
    float xr[4], xc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) xr[a] = sx1[d * kGT + a * 16 + tr];
#pragma unroll
    for (int c = 0; c < 4; ++c) xc[c] = sx2[d * kGT + c * 16 + tc];
    if (t.bkind[b] == LVAE_CAT) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) bits[a][c] += (xr[a] == xc[c]) ? bit : 0;
    } else {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) bits[a][c] += (xr[a] + xc[c] == 2.f) ? bit : 0;
    }
  }
}

// group g's table index per element: bits + |x_i[d_g] - x_j[d_g]| (< kTabD by the covariate flag)
__device__ inline void tab_index(const GramTab& t, int g, const float* __restrict__ sx1,
                                 const float* __restrict__ sx2, int tr, int tc, const int (&bits)[4][4],
                                 int (&idx)[4][4]) {
  const int d = t.gdim[g];
  if (d < 0) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) idx[a][c] = bits[a][c];
    return;
  }
  float xr[4], xc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) xr[a] = sx1[d * kGT + a * 16 + tr];
#pragma unroll
  for (int c = 0; c < 4; ++c) xc[c] = sx2[d * kGT + c * 16 + tc];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) idx[a][c] = bits[a][c] + (int)fabsf(xr[a] - xc[c]);
}

// gram_sq_fill_kernel's table twin (flag 2)
__global__ __launch_bounds__(256) void gram_sq_fill_tab_kernel(GramTab tb, const double* __restrict__ x, int ldx,
                                                               int n, int np_, int qs,
                                                               const double* __restrict__ params,
                                                               const double* __restrict__ noise,
                                                               float* __restrict__ K, int ntiles,
                                                               const int* __restrict__ covflag) {
  if (*covflag != 2) return;  // (uniform, before any barrier)
  __shared__ float sx1[kGT * kMaxQB];
  __shared__ float sx2[kGT * kMaxQB];
  __shared__ float sp[64];
  extern __shared__ float tab[];  // ng 2^B kTabR floats
  const int G = gridDim.x, l = blockIdx.y, tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  if (tid < tb.n_params) sp[tid] = float(params[(int64_t)l * tb.n_params + tid]);
  const float nz = float(noise[l]);
  float* o = K + (int64_t)l * np_ * np_;
  int t = blockIdx.x, I, J;
  if (t >= ntiles) return;
  tri_index(t, I, J);
  CovPrefetchF pf;
  pf.load(x, ldx, n, qs, I * kGT, J * kGT);
  pf.store(qs, sx1, sx2);
  __syncthreads();
  tab_build_fill(tb, sp, tab);
  __syncthreads();
  const int tstride = (1 << tb.nbits) * kTabR;
  for (; t < ntiles; t += G) {
    const int i0 = I * kGT, j0 = J * kGT;
    int In = 0, Jn = 0;
    const bool more = t + G < ntiles;
    if (more) {
      tri_index(t + G, In, Jn);
      pf.load(x, ldx, n, qs, In * kGT, Jn * kGT);
    }
    int bits[4][4];
    tab_bits(tb, sx1, sx2, tr, tc, bits);
    float out[4][4] = {};
#pragma unroll 1
    for (int g = 0; g < tb.ng; ++g) {
      int idx[4][4];
      tab_index(tb, g, sx1, sx2, tr, tc, bits, idx);
      const float* tg = tab + g * tstride;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) out[a][c] += tg[idx[a][c]];
    }
    if (I != J && i0 + kGT <= n) {  // (uniform) an interior tile below the diagonal: no noise, no padding
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const g_f32x4 w = {out[a][0], out[a][1], out[a][2], out[a][3]};
        *reinterpret_cast<g_f32x4*>(o + (int64_t)(i0 + 4 * tr + a) * np_ + j0 + 4 * tc) = w;
      }
    } else {
      fill_store_edge(out, nz, n, np_, i0, j0, tr, tc, o);
    }
    if (more) {
      __syncthreads();  // every reader of this tile's covariates is done
      pf.store(qs, sx1, sx2);
      __syncthreads();
      I = In, J = Jn;
    }
  }
}

// kl_gram_bwd_tiles' table twin (flag 2): the same G, weights, slots and partials
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LVAE_TAB_WPE))) void kl_gram_bwd_tab_kernel(GramTab tb, const double* __restrict__ x, int ldx,
                                                              int n, int np_, int qs,
                                                              const double* __restrict__ params,
                                                              const float* __restrict__ Kinv,
                                                              const float* __restrict__ S,
                                                              const float* __restrict__ Sx, int nsplit,
                                                              const double* __restrict__ alpha,
                                                              double* __restrict__ part, int ntiles,
                                                              const int* __restrict__ covflag,
                                                              const int* __restrict__ hbon) {
  if (*covflag != 2 || (hbon && *hbon)) return;  // (uniform, before any barrier; hbon: kl_hyper.hip's path)
  __shared__ float sx1[2][kGT * kMaxQB];  // (two buffers: this tile's and the next one's)
  __shared__ float sx2[2][kGT * kMaxQB];
  __shared__ float sp[64];
  __shared__ float sa1[2][kGT], sa2[2][kGT];
  __shared__ double wred[4][kBwdSlots];
  extern __shared__ float tdyn[];  // [(n_params + 1) x 256] per-thread sums, then the tables
  const int G = gridDim.x, g0 = blockIdx.x, l = blockIdx.y, tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  const int np_s = tb.n_params;
  float* tab = tdyn + (np_s + 1) * 256;
  auto tacc = [&](int q) -> float& { return tdyn[(q == kNoiseSlot ? np_s : q) * 256 + tid]; };
  if (tid < np_s) sp[tid] = float(params[(int64_t)l * np_s + tid]);
  for (int e = tid; e < 4 * kBwdSlots; e += 256) (&wred[0][0])[e] = 0.0;
  for (int q = 0; q < np_s; ++q) tacc(q) = 0.f;
  tacc(kNoiseSlot) = 0.f;
  __syncthreads();
  tab_build_bwd(tb, sp, tab);
  const int tstride = (1 << tb.nbits) * kTabR;
  const float* ki = Kinv + (int64_t)l * np_ * np_;
  const float* si = S + (int64_t)l * np_ * np_;
  const double* al = alpha + (int64_t)l * np_;
  auto load_ks = [&](int i0, int j0, g_f32x4 (&kv4)[4], g_f32x4 (&sv4)[4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int64_t o = (int64_t)(i0 + 4 * tr + a) * np_ + j0 + 4 * tc;
      kv4[a] = __builtin_nontemporal_load(reinterpret_cast<const g_f32x4*>(ki + o));
      sv4[a] = __builtin_nontemporal_load(reinterpret_cast<const g_f32x4*>(si + o));
    }
    for (int q = 1; q < nsplit; ++q) {  // K-split partials of S (syrk_x3_splits)
      const float* sq = Sx + (int64_t)(q - 1) * gridDim.y * np_ * np_ + (int64_t)l * np_ * np_;
#pragma unroll
      for (int a = 0; a < 4; ++a)
        sv4[a] += __builtin_nontemporal_load(
            reinterpret_cast<const g_f32x4*>(sq + (int64_t)(i0 + 4 * tr + a) * np_ + j0 + 4 * tc));
    }
  };
  float dd = 0.f;
  int since_flush = 0;
  int t = g0, I = 0, J = 0, In = 0, Jn = 0;
  g_f32x4 kv4[4], sv4[4];
  CovPrefetchF pf;
  double an = 0.0;
  // software pipeline: tile t's K^-1 / S rows are loaded into registers during tile t - G and its
  // covariates / alpha entries during tile t - 2G (stored to the other LDS buffer at the end of tile
  // t - G), so that no tile waits for a global round trip and one barrier per tile suffices
  if (t < ntiles) {
    tri_index(t, I, J);
    load_ks(I * kGT, J * kGT, kv4, sv4);
    pf.load(x, ldx, n, qs, I * kGT, J * kGT);
    if (tid < 2 * kGT) an = al[(tid < kGT ? I : J) * kGT + (tid & (kGT - 1))];
    pf.store(qs, sx1[0], sx2[0]);
    if (tid < kGT) sa1[0][tid] = float(an);
    else if (tid < 2 * kGT) sa2[0][tid - kGT] = float(an);
    if (t + G < ntiles) {
      tri_index(t + G, In, Jn);
      pf.load(x, ldx, n, qs, In * kGT, Jn * kGT);
      if (tid < 2 * kGT) an = al[(tid < kGT ? In : Jn) * kGT + (tid & (kGT - 1))];
    }
  }
  __syncthreads();  // the tables and the first tile's LDS
  for (int b = 0; t < ntiles; t += G, b ^= 1) {
    const int i0 = I * kGT, j0 = J * kGT;
    const bool more = t + G < ntiles;
    const float* __restrict__ cx1 = sx1[b];
    const float* __restrict__ cx2 = sx2[b];
    float g[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int i = i0 + 4 * tr + a;
      const g_f32x4 kv = kv4[a], sv = sv4[a];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + 4 * tc + c;
        const float gv = 0.5f * (kv[c] - sv[c] - sa1[b][4 * tr + a] * sa2[b][4 * tc + c]);
        const bool in = i < n && j < n && j <= i;
        if (in && i == j) dd += gv;
        g[a][c] = in ? ((i == j) ? gv : 2.f * gv) : 0.f;
      }
    }
    if (more) load_ks(In * kGT, Jn * kGT, kv4, sv4);  // (in flight under this tile's tables)
#pragma unroll 1
    for (int gi = 0; gi < tb.ng; ++gi) {
      int idx[4][4];  // (the gate bits recomputed per group: fewer live registers)
      tab_bits(tb, cx1, cx2, tr, tc, idx);
      tab_index(tb, gi, cx1, cx2, tr, tc, idx, idx);
#pragma unroll 1
      for (int k = tb.pbeg[gi]; k < tb.pbeg[gi + 1]; ++k) {
        const float* tk = tab + k * tstride;
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc += g[a][c] * tk[idx[a][c]];
        tacc(tb.porder[k]) += acc;
      }
    }
    if (++since_flush == 4 || t + G >= ntiles) {  // fold the fp32 sums into the fp64 wave slots
      since_flush = 0;
      bwd_flush(tacc, np_s, dd, wred);
    }
    if (more) {
      // tile t + G's covariates (loaded during the previous tile) to the other buffer, whose last
      // readers finished before the previous barrier; then tile t + 2G's go in flight
      pf.store(qs, sx1[b ^ 1], sx2[b ^ 1]);
      if (tid < kGT) sa1[b ^ 1][tid] = float(an);
      else if (tid < 2 * kGT) sa2[b ^ 1][tid - kGT] = float(an);
      int I2 = 0, J2 = 0;
      if (t + 2 * G < ntiles) {
        tri_index(t + 2 * G, I2, J2);
        pf.load(x, ldx, n, qs, I2 * kGT, J2 * kGT);
        if (tid < 2 * kGT) an = al[(tid < kGT ? I2 : J2) * kGT + (tid & (kGT - 1))];
      }
      __syncthreads();  // buffer b ^ 1 written; every reader of buffer b done
      I = In, J = Jn, In = I2, Jn = J2;
    }
  }
  __syncthreads();
  for (int sl = tid; sl < kBwdSlots; sl += 256)
    part[((int64_t)l * kBwdSlots + sl) * G + g0] = wred[0][sl] + wred[1][sl] + wred[2][sl] + wred[3][sl];
}

// per-parameter derivative constants of kl_gram_bwd_tiles' raw sums (host-built from the spec):
// type 0 scale (1), 1 RBF lengthscale (1 / l^3), 2 PER lengthscale (4 / l^3), 3 PER period
// (2 pi / (l^2 p^2), l at index ell[p])
struct BwdParamInfo {
  int8_t type[64];
  int8_t ell[64];
};

// dparams[l, p] = gkl[l] c_p sum_g part[l][p][g]; dnoise[l] from kNoiseSlot.  Grid (n_params + 1, L).
__global__ __launch_bounds__(256) void kl_gram_bwd_reduce(BwdParamInfo pinfo, int n_params,
                                                          const double* __restrict__ part, int G,
                                                          const double* __restrict__ params,
                                                          const double* __restrict__ gkl,
                                                          double* __restrict__ dparams,
                                                          double* __restrict__ dnoise) {
  __shared__ double red[4];
  const int b = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
  const int slot = b == n_params ? kNoiseSlot : b;
  const double* p = part + ((int64_t)l * kBwdSlots + slot) * G;
  double v = 0.0;
  for (int t = tid; t < G; t += 256) v += p[t];
  v = block_sum<256>(v, red);
  if (tid != 0) return;
  if (slot == kNoiseSlot) {
    if (dnoise) dnoise[l] = gkl[l] * v;
    return;
  }
  const double* pl = params + (int64_t)l * n_params;
  double c = 1.0;
  const int ty = pinfo.type[b];
  if (ty == 1) c = 1.0 / (pl[b] * pl[b] * pl[b]);
  else if (ty == 2) c = 4.0 / (pl[b] * pl[b] * pl[b]);
  else if (ty == 3) {
    const double ell = pl[pinfo.ell[b]];
    c = 2.0 * M_PI / (ell * ell * pl[b] * pl[b]);
  }
  dparams[(int64_t)l * n_params + b] = gkl[l] * c * v;
}

// ------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------
// LVAE_<name>=0 in the environment switches a fast path off (A/B runs)
static bool getenv_off(const char* name) {
  const char* v = getenv(name);
  return v && atoi(v) == 0;
}

// the table kernels are launched iff the spec has a table form and LVAE_GRAM_TAB is not "0": kl_gram_fill and
// kl_gram_bwd must agree, since the covariate flag 2 that the one sets makes every other kernel of the other exit
static bool gram_tab_route(const lvae_kernel_spec* spec, GramTab& tb) {
  return gram_tab_build(spec, tb) && !getenv_off("LVAE_GRAM_TAB");
}

int kl_gram_fill(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int np_, int L,
                 const double* params, const double* noise, float* K, int* covflag, hipStream_t st) {
  const int bucket = spec_bucket(spec);
  const int qs = spec_qs(spec);
  if (!bucket || qs > kMaxQB || qs > ldx) return -1;
  const DevSpec ds = to_dev(spec);
  const int nt = np_ / kGT, ntiles = nt * (nt + 1) / 2;
  int G = (2048 + L - 1) / L;  // ~8 resident workgroups per CU, 2 rounds
  G = G < ntiles ? G : ntiles;
  dim3 grid(G, L);
  GramTab tb;
  const bool tab_ok = gram_tab_route(spec, tb);
  int tabmask = 0;
  for (int g = 0; g < tb.ng && tab_ok; ++g)
    if (tb.gdim[g] >= 0) tabmask |= 1 << tb.gdim[g];
  cov_int_check_kernel<<<1, 1024, 0, st>>>(x, ldx, n, qs, tab_ok, tabmask, covflag);
  if (tab_ok)
    gram_sq_fill_tab_kernel<<<grid, 256, (size_t)tb.ng * (1 << tb.nbits) * kTabR * sizeof(float), st>>>(
        tb, x, ldx, n, np_, qs, params, noise, K, ntiles, covflag);
  if (bucket == 1) {
    gram_sq_fill_kernel<8, 2, float><<<grid, 256, 0, st>>>(ds, x, ldx, n, np_, qs, params, noise, K, ntiles, covflag);
    gram_sq_fill_kernel<8, 2, double><<<grid, 256, 0, st>>>(ds, x, ldx, n, np_, qs, params, noise, K, ntiles, covflag);
  } else {
    gram_sq_fill_kernel<16, 4, float><<<grid, 256, 0, st>>>(ds, x, ldx, n, np_, qs, params, noise, K, ntiles, covflag);
    gram_sq_fill_kernel<16, 4, double><<<grid, 256, 0, st>>>(ds, x, ldx, n, np_, qs, params, noise, K, ntiles, covflag);
  }
  LVAE_CHECK_LAUNCH();
  return 0;
}

// workgroups per latent dim of the adjoint: ~1536 in all, each looping over ~ntiles / G tiles
static int kl_gram_bwd_groups(int np_, int L) {
  const int nt = np_ / kGT, ntiles = nt * (nt + 1) / 2;
  int G = (1536 + L - 1) / L;  // 2 full rounds of 256 CUs x 3 resident workgroups
  G = G < 8 ? 8 : G;
  return G < ntiles ? G : ntiles;
}

size_t kl_gram_bwd_partials_bytes(int np_, int L) {
  return (size_t)L * kl_gram_bwd_groups(np_, L) * kBwdSlots * sizeof(double);
}

int kl_gram_bwd(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int np_, int L,
                const double* params, const float* Kinv, const float* S, const float* Sx, int nsplit,
                const double* alpha, const double* kdiag, const float* v, const double* gkl, double* part,
                double* dparams, double* dnoise, const int* covflag, void* hbws, const int* hbon, hipStream_t st) {
  const int bucket = spec_bucket(spec);
  const int qs = spec_qs(spec);
  if (!bucket || qs > kMaxQB || spec->n_params > 64) return -1;
  const DevSpec ds = to_dev(spec);
  BwdParamInfo pinfo{};
  for (int r = 0; r < spec->n_comp; ++r)
    for (int f = 0; f < spec->n_fac[r]; ++f) {
      const int pi = spec->param_idx[r][f];
      if (spec->kind[r][f] == LVAE_RBF) pinfo.type[pi] = 1;
      if (spec->kind[r][f] == LVAE_PER) {
        pinfo.type[pi] = 2;
        pinfo.type[pi + 1] = 3;
        pinfo.ell[pi + 1] = (int8_t)pi;
      }
    }
  const int nt = np_ / kGT, ntiles = nt * (nt + 1) / 2, G = kl_gram_bwd_groups(np_, L);
  const size_t dyn = (size_t)(spec->n_params + 1) * 256 * sizeof(float);
  GramTab tb;
  if (gram_tab_route(spec, tb)) {
    const size_t tabb = (size_t)tb.pbeg[tb.ng] * (1 << tb.nbits) * kTabR * sizeof(float);
    kl_gram_bwd_tab_kernel<<<dim3(G, L), 256, dyn + tabb, st>>>(tb, x, ldx, n, np_, qs, params, Kinv, S, Sx, nsplit,
                                                                alpha, part, ntiles, covflag, hbon);
  }
  if (bucket == 1) {
    kl_gram_bwd_tiles<8, 2, float><<<dim3(G, L), 256, dyn, st>>>(ds, x, ldx, n, np_, qs, params, Kinv, S, Sx, nsplit,
                                                                  alpha, part, ntiles, covflag);
    kl_gram_bwd_tiles<8, 2, double><<<dim3(G, L), 256, dyn, st>>>(ds, x, ldx, n, np_, qs, params, Kinv, S, Sx, nsplit,
                                                                   alpha, part, ntiles, covflag);
  } else {
    kl_gram_bwd_tiles<16, 4, float><<<dim3(G, L), 256, dyn, st>>>(ds, x, ldx, n, np_, qs, params, Kinv, S, Sx,
                                                                   nsplit, alpha, part, ntiles, covflag);
    kl_gram_bwd_tiles<16, 4, double><<<dim3(G, L), 256, dyn, st>>>(ds, x, ldx, n, np_, qs, params, Kinv, S, Sx,
                                                                    nsplit, alpha, part, ntiles, covflag);
  }
  // the binned hyper-gradient (kl_hyper.hip; its kernels exit when the plan is off, the table kernel when it is on)
  if (hbws) LVAE_TRY(kl_hyper_bwd(spec, x, ldx, n, np_, L, params, Kinv, v, alpha, kdiag, hbws, part, G, st));
  kl_gram_bwd_reduce<<<dim3(spec->n_params + 1, L), 256, 0, st>>>(pinfo, spec->n_params, part, G, params, gkl,
                                                                  dparams, dnoise);
  LVAE_CHECK_LAUNCH();
  return 0;
}

}  // namespace lvae
