// kl_refine.hpp -- what kl_refine.hip exports to the exact KL's reduce (kl_closed.hip): the fp64 refinement of
// diag K^-1 for the latent dims whose conditioning asks for it.
#pragma once
#include "common.hpp"

namespace lvae {

// K64 holds ceil(L / 2) dims: the flagged dims go in (at most) two rounds through the caller's buffer
size_t kl_refine_bytes(int np_, int L);
size_t kl_refine_part_bytes(int np_, int L);
// the gate alone: est, flag from kdiag (mode 0: both zero)
int kl_refine_gate(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int np_, int L, const double* params,
                   const double* noise, const double* kdiag, double* est, int* flag, hipStream_t st);
// the refinement of the flagged dims' diag K^-1 (kdiag) from the fp32 K^-1 in Kinv (the gate ran before)
int kl_refine_apply(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int np_, int L, const double* params,
                    const double* noise, const float* Kinv, double* kdiag, double* K64, double* part, const int* flag,
                    hipStream_t st);
// the gate, then the refinement
int kl_refine_diag(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int np_, int L,
                   const double* params, const double* noise, const float* Kinv, double* kdiag, double* K64,
                   double* part, double* est, int* flag, hipStream_t st);

}  // namespace lvae
