// bound_seg.hip -- the seg forms (subjects of varying length) of the two fused subject kernels of
// bound_subject.hpp, in a translation unit of their own (why: bound_subject.hpp).
#include "bound_subject.hpp"

namespace lvae {

void dubo_subject_seg_launch(dim3 grid, hipStream_t st, int M, int P, int T, int L, int nt, int64_t pstride,
                             const double* X, const double* iB, const double* K0st, const double* ldB,
                             const double* mu, const double* logv, double* iBK, double* part, const int32_t* seg) {
  dubo_subject_kernel<const int32_t*><<<grid, 512, 0, st>>>(M, P, T, L, nt, pstride, X, iB, K0st, ldB, mu, logv, iBK,
                                                           part, seg);
}

void gp_elbo_subject_seg_launch(dim3 grid, hipStream_t st, int M, int P, int T, int L, int S, int nt, int64_t pstride,
                                const double* X, const double* iB, const double* K0st, const double* ldB,
                                const double* y, double* iBK, double* sbuf, double* part, const int32_t* seg) {
  gp_elbo_subject_kernel<const int32_t*><<<grid, 512, 0, st>>>(M, P, T, L, S, nt, pstride, X, iB, K0st, ldB, y, iBK,
                                                              sbuf, part, seg);
}

}  // namespace lvae
