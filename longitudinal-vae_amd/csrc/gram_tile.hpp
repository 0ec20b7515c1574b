// gram_tile.hpp -- what the Gram sources (gram.hip, kl_gram.hip, gram_matvec.hip) share: the tile edge, the staged
// covariate limits, the 64-tile covariate image of the micro-tile kernels and the host's column count of a spec.
#pragma once
#include "common.hpp"

namespace lvae {

constexpr int kGT = 64;     // Gram tile edge
constexpr int kMaxQ = 32;   // staged covariate columns

// lower 64-tile t -> (I, J), I >= J, row by row
__device__ inline void tri_index(int t, int& I, int& J) {
  int r = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  while (r * (r + 1) / 2 > t) --r;
  I = r;
  J = t - r * (r + 1) / 2;
}

// stage the covariates of rows [i0, i0 + 64) and [j0, j0 + 64) (zero beyond n) into LDS.  Layout
// [dim][slot]: row r of the tile sits at slot (r & 3) * 16 + (r >> 2), so the 16 lanes that read
// rows 4 tc + c (c fixed) touch 16 consecutive doubles -- conflict-free ds_read_b64 (a row-major
// [row][dim] image puts those 16 reads on one bank pair: 16-way conflicts).
constexpr int kMaxQB = 16;  // covariate columns the Regime B kernels stage (spec dims < 16)
__device__ inline int cov_slot(int r) { return (r & 3) * 16 + (r >> 2); }
template <typename CT>
__device__ inline void stage_cov(const double* __restrict__ x, int ldx, int n, int qs, int i0, int j0,
                                 CT* __restrict__ sx1, CT* __restrict__ sx2) {
  for (int e = threadIdx.x; e < kGT * qs; e += 256) {
    const int r = e / qs, q = e % qs;
    sx1[q * kGT + cov_slot(r)] = CT((i0 + r < n) ? x[(int64_t)(i0 + r) * ldx + q] : 0.0);
    sx2[q * kGT + cov_slot(r)] = CT((j0 + r < n) ? x[(int64_t)(j0 + r) * ldx + q] : 0.0);
  }
}

// 1 + the largest covariate column the spec reads
static inline int spec_qs(const lvae_kernel_spec* s) {
  int q = 0;
  for (int r = 0; r < s->n_comp; ++r)
    for (int f = 0; f < s->n_fac[r]; ++f) q = s->dim[r][f] + 1 > q ? s->dim[r][f] + 1 : q;
  return q;
}

}  // namespace lvae
