// bound_subject.hpp -- the fused subject pass of the DUBO (dubo.hip) and of the sampled ELBO (gp_elbo.hip): the two
// kernels that walk the subjects in groups of kBoundS with Q in MFMA accumulators (the blocks of the walk they share:
// gp_bound.hpp).  Each takes seg (subjects of varying length) as an optional trailing argument.  dubo.hip and
// gp_elbo.hip instantiate the uniform form alone; the seg form is instantiated in bound_seg.hip, behind the two
// launch functions below: with both forms in one translation unit the inliner's choices for the uniform kernel
// change, and that kernel is to stay the code it was before there was a seg form.
#pragma once
#include "gp_bound.hpp"

namespace lvae {

constexpr int kGeS = 16;      // sample columns of one call: one 16-wide MFMA column block (zero padded past S)

// the seg forms' launches (bound_seg.hip); arguments as the kernels', grid (groups, L)
void dubo_subject_seg_launch(dim3 grid, hipStream_t st, int M, int P, int T, int L, int nt, int64_t pstride,
                             const double* X, const double* iB, const double* K0st, const double* ldB,
                             const double* mu, const double* logv, double* iBK, double* part, const int32_t* seg);
void gp_elbo_subject_seg_launch(dim3 grid, hipStream_t st, int M, int P, int T, int L, int S, int nt, int64_t pstride,
                                const double* X, const double* iB, const double* K0st, const double* ldB,
                                const double* y, double* iBK, double* sbuf, double* part, const int32_t* seg);

namespace {

// The fused subject pass: grid (groups, L), 512 threads.  Group g walks subjects [g kBoundS, (g + 1) kBoundS).
// Per subject: iB_p [T,T], X_p [T,M], m_p, v_p into LDS (zero padded to whole MFMA steps); iBK_p = iB_p X_p on
// v_mfma_f64_16x16x4 (C[(lane >> 4) + 4 r][lane & 15]) -> LDS and HBM; then Q += X_p^T iBK_p and
// R += iBK_p^T D_p iBK_p on the lower 16 x 16 tiles, tile t = wave + 8 k in accumulators Qa[k] / Ra[k] for the
// whole walk, p and the five scalar sums in plain registers.  One partial per (dim, group).
// SEG (varying T, seg [P]): subject p has n = seg[p] valid rows; the Grams come masked (bound_seg_mask: zero rows of
// X_p, iB_p the identity on the padding), so the whole [T, .] blocks are still loaded -- no row of an earlier, longer
// subject survives in sB / sX -- but the MFMA trip counts follow n (wave-uniform): ceil(n / 16) row tiles of iBK_p
// and ceil(n / 4) steps of every product.  The rows of iBK_p those tiles skip are zero-filled in HBM (sY keeps an
// earlier subject's rows there; nothing reads them: every k loop ends at ceil4(n) <= 16 ceil(n / 16)).  mu / logv are
// read on the valid rows only.  Seg is either nothing or one const int32_t* (bound_seg_arg): without it this is the
// uniform pass as it was, argument list and code (n = T folds away).
template <class... Seg>
__global__ __launch_bounds__(512) void dubo_subject_kernel(int M, int P, int T, int L, int nt, int64_t pstride,
                                                           const double* __restrict__ X,
                                                           const double* __restrict__ iB,
                                                           const double* __restrict__ K0st,
                                                           const double* __restrict__ ldB,
                                                           const double* __restrict__ mu,
                                                           const double* __restrict__ logv,
                                                           double* __restrict__ iBK, double* __restrict__ part,
                                                           Seg... seg_arg) {
  constexpr bool SEG = sizeof...(Seg) > 0;
  const int32_t* seg = bound_seg_arg(seg_arg...);
  __shared__ double sB[kBoundT][kBoundT + 1];
  __shared__ double sX[kBoundT][kBoundLD];
  __shared__ double sY[kBoundT][kBoundLD];
  __shared__ double sm[kBoundT], sv[kBoundT];
  __shared__ double red[8];
  const int g = blockIdx.x, l = blockIdx.y, G = gridDim.x;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int tM = (M + 15) >> 4, tT = (T + 15) >> 4, T4 = (T + 3) & ~3;
  const int64_t N = (int64_t)P * T, TT = (int64_t)T * T;
  int ti[kBoundTPW], tj[kBoundTPW];
  bool on[kBoundTPW];
  bi_f64x4 Qa[kBoundTPW], Ra[kBoundTPW] = {};
  bound_walk_setup(wv, nt, ti, tj, on, Qa);
  double pj = 0.0, s_mbm = 0.0, s_dv = 0.0, s_bk0 = 0.0, s_lv = 0.0, s_ldb = 0.0;
  bound_lds_zero(tid, sB, sX, sY);
  if (tid < kBoundT) {
    sm[tid] = 0.0;
    sv[tid] = 0.0;
  }
  const int p0 = g * kBoundS, p1 = p0 + kBoundS < P ? p0 + kBoundS : P;
  for (int p = p0; p < p1; ++p) {
    __syncthreads();  // the previous subject's readers are done (and the zero fill is visible)
    bound_load_subject(tid, T, M, iB + ((int64_t)l * P + p) * TT, K0st + ((int64_t)l * P + p) * TT,
                       X + ((int64_t)l * N + (int64_t)p * T) * M, sB, sX, s_bk0);
    const int n = SEG ? bound_seg_n(seg, p, T) : T;
    const int n4 = SEG ? (n + 3) & ~3 : T4, tn = SEG ? (n + 15) >> 4 : tT;
    if (tid < n) {
      const int64_t q = ((int64_t)p * T + tid) * L + l;
      const double lv = logv[q];
      sm[tid] = mu[q];
      sv[tid] = exp(lv);
      s_lv += lv;
    } else if (SEG && tid < T) {
      sm[tid] = 0.0;
      sv[tid] = 0.0;
    }
    if (tid == 0) s_ldb += ldB[(int64_t)l * P + p];
    __syncthreads();
    for (int e = tid; e < T * T; e += 512) {
      const int i = e / T, j = e % T;
      const double b = sB[i][j];
      s_mbm += sm[i] * b * sm[j];
      if (i == j) s_dv += b * sv[i];
    }
    // iBK_p = iB_p X_p: tT x tM tiles over the 8 waves
    double* yp = iBK + ((int64_t)l * N + (int64_t)p * T) * M;
    for (int tt = wv; tt < tn * tM; tt += 8)
      bound_ibk_tile((tt / tM) << 4, (tt % tM) << 4, li, lk, T, M, n4, sB, sX, sY, yp);
    if (SEG)
      for (int e = (tn << 4) * M + tid; e < T * M; e += 512) yp[e] = 0.0;
    __syncthreads();
    if (tid < M) {
      double q = 0.0;
      for (int r = 0; r < n; ++r) q += sY[r][tid] * sm[r];
      pj += q;
    }
#pragma unroll
    for (int k = 0; k < kBoundTPW; ++k) {
      if (on[k]) {
        const int ci = (ti[k] << 4) + li, cj = (tj[k] << 4) + li;
        for (int kk = 0; kk < n4; kk += 4) {
          const double yb = sY[kk + lk][cj];
          Qa[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(sX[kk + lk][ci], yb, Qa[k], 0, 0, 0);
          Ra[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(sv[kk + lk] * sY[kk + lk][ci], yb, Ra[k], 0, 0, 0);
        }
      }
    }
  }
  double* pp = part + ((int64_t)l * G + g) * pstride;
  bound_store_tiles(pp, wv, lane, on, Qa);
  bound_store_tiles(pp + (int64_t)nt * 256, wv, lane, on, Ra);  // R's tiles follow Q's, in the same order
  double* pv = pp + (int64_t)2 * nt * 256;
  if (tid < 128) pv[tid] = pj;
  const double vals[5] = {s_mbm, s_dv, s_bk0, s_lv, s_ldb};
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const double v = block_sum<512>(vals[q], red);
    if (tid == 0) pv[128 + q] = v;
  }
}

// The fused subject pass: grid (groups, L), 512 threads.  Group g walks subjects [g kBoundS, (g + 1) kBoundS).
// Per subject: iB_p [T,T], X_p [T,M] and the samples Y_p [T,16] (columns S.. zero) into LDS, zero padded to whole
// MFMA steps; iBK_p = iB_p X_p and s_p = iB_p Y_p on v_mfma_f64_16x16x4 (C[(lane >> 4) + 4 r][lane & 15]), iBK_p
// -> LDS and HBM, s_p -> HBM with y.s summed per lane (a lane's column IS its sample); then Q += X_p^T iBK_p on
// the lower 16 x 16 tiles (tile t = wave + 8 k in Qa[k]) and Pm += iBK_p^T Y_p, row tile = wave, both in
// accumulators for the whole walk.  One partial per (dim, group).
// SEG (varying T, seg [P]): as dubo_subject_kernel's -- the masked [T, .] blocks are loaded whole, the samples on
// the n = seg[p] valid rows only (zeros below them), the MFMA trip counts follow n, and the rows of iBK_p and s_p
// that the skipped row tiles would have written are zero-filled in HBM.  Seg is either nothing or one const int32_t*
// (bound_seg_arg): without it this is the uniform pass as it was, argument list and code.
template <class... Seg>
__global__ __launch_bounds__(512) void gp_elbo_subject_kernel(int M, int P, int T, int L, int S, int nt,
                                                              int64_t pstride, const double* __restrict__ X,
                                                              const double* __restrict__ iB,
                                                              const double* __restrict__ K0st,
                                                              const double* __restrict__ ldB,
                                                              const double* __restrict__ y,
                                                              double* __restrict__ iBK, double* __restrict__ sbuf,
                                                              double* __restrict__ part, Seg... seg_arg) {
  constexpr bool SEG = sizeof...(Seg) > 0;
  const int32_t* seg = bound_seg_arg(seg_arg...);
  __shared__ double sB[kBoundT][kBoundT + 1];
  __shared__ double sX[kBoundT][kBoundLD];
  __shared__ double sY[kBoundT][kBoundLD];
  __shared__ double sS[kBoundT][kGeS + 1];
  __shared__ double sq[8][64];
  __shared__ double red[8];
  const int g = blockIdx.x, l = blockIdx.y, G = gridDim.x;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int tM = (M + 15) >> 4, tT = (T + 15) >> 4, T4 = (T + 3) & ~3;
  const int64_t N = (int64_t)P * T, TT = (int64_t)T * T;
  int ti[kBoundTPW], tj[kBoundTPW];
  bool on[kBoundTPW];
  bi_f64x4 Qa[kBoundTPW];
  bi_f64x4 Pa = {0.0, 0.0, 0.0, 0.0};
  bound_walk_setup(wv, nt, ti, tj, on, Qa);
  double s_ys = 0.0, s_bk0 = 0.0, s_ldb = 0.0;
  bound_lds_zero(tid, sB, sX, sY);
  // (sS likewise: rows T.., sample columns S..)
  for (int e = tid; e < kBoundT * (kGeS + 1); e += 512) (&sS[0][0])[e] = 0.0;
  const int p0 = g * kBoundS, p1 = p0 + kBoundS < P ? p0 + kBoundS : P;
  for (int p = p0; p < p1; ++p) {
    __syncthreads();  // the previous subject's readers are done (and the zero fill is visible)
    bound_load_subject(tid, T, M, iB + ((int64_t)l * P + p) * TT, K0st + ((int64_t)l * P + p) * TT,
                       X + ((int64_t)l * N + (int64_t)p * T) * M, sB, sX, s_bk0);
    const int n = SEG ? bound_seg_n(seg, p, T) : T;
    const int n4 = SEG ? (n + 3) & ~3 : T4, tn = SEG ? (n + 15) >> 4 : tT;
    for (int e = tid; e < T * kGeS; e += 512) {
      const int i = e >> 4, s = e & 15;
      if (s < S) sS[i][s] = (!SEG || i < n) ? y[((int64_t)s * N + (int64_t)p * T + i) * L + l] : 0.0;
    }
    if (tid == 0) s_ldb += ldB[(int64_t)l * P + p];
    __syncthreads();
    // iBK_p = iB_p X_p (tT x tM tiles) and s_p = iB_p Y_p (tT tiles) over the 8 waves
    double* yp = iBK + ((int64_t)l * N + (int64_t)p * T) * M;
    double* sp = sbuf + ((int64_t)l * N + (int64_t)p * T) * kGeS;
    for (int tt = wv; tt < tn * tM + tn; tt += 8) {
      if (tt < tn * tM) {
        bound_ibk_tile((tt / tM) << 4, (tt % tM) << 4, li, lk, T, M, n4, sB, sX, sY, yp);
      } else {
        const int r0 = (tt - tn * tM) << 4;
        bi_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int kk = 0; kk < n4; kk += 4)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sB[r0 + li][kk + lk], sS[kk + lk][li], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = r0 + lk + 4 * r;
          if (i < T) {
            sp[i * kGeS + li] = acc[r];
            s_ys += acc[r] * sS[i][li];
          }
        }
      }
    }
    if (SEG) {
      for (int e = (tn << 4) * M + tid; e < T * M; e += 512) yp[e] = 0.0;
      for (int e = (tn << 4) * kGeS + tid; e < T * kGeS; e += 512) sp[e] = 0.0;
    }
    __syncthreads();
    if (wv < tM) {
      const int ci = (wv << 4) + li;
      for (int kk = 0; kk < n4; kk += 4)
        Pa = __builtin_amdgcn_mfma_f64_16x16x4f64(sY[kk + lk][ci], sS[kk + lk][li], Pa, 0, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < kBoundTPW; ++k) {
      if (on[k]) {
        const int ci = (ti[k] << 4) + li, cj = (tj[k] << 4) + li;
        for (int kk = 0; kk < n4; kk += 4)
          Qa[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(sX[kk + lk][ci], sY[kk + lk][cj], Qa[k], 0, 0, 0);
      }
    }
  }
  double* pp = part + ((int64_t)l * G + g) * pstride;
  bound_store_tiles(pp, wv, lane, on, Qa);
  double* pm = pp + (int64_t)nt * 256;
  if (wv < tM) {
#pragma unroll
    for (int r = 0; r < 4; ++r) pm[((wv << 4) + lk + 4 * r) * kGeS + li] = Pa[r];
  }
  double* pv = pm + 128 * kGeS;
  sq[wv][lane] = s_ys;
  const double bk0 = block_sum<512>(s_bk0, red);  // (its barriers also publish sq)
  const double ldb = block_sum<512>(s_ldb, red);
  if (tid == 0) {
    pv[0] = bk0;
    pv[1] = ldb;
  }
  if (tid < kGeS) {
    double v = 0.0;
    for (int w = 0; w < 8; ++w)
      for (int q = 0; q < 4; ++q) v += sq[w][q * 16 + tid];
    pv[8 + tid] = v;
  }
}

}  // namespace
}  // namespace lvae
