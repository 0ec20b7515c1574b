// kl_hyper.hpp -- what kl_hyper.hip exports: the exact KL's binned hyper-gradient, planned by the factor
// (kl_closed.hip) and run inside kl_gram_bwd (kl_gram.hip) in the table adjoint's place.
#pragma once
#include "common.hpp"

namespace lvae {

struct HbDev;  // the plan's device state; `on` is its first int
size_t kl_hyper_bytes(int np_, int L);
HbDev* kl_hyper_dev(void* base, int np_, int L);
// the plan and the pair codes (after kl_gram_fill's covariate check, on the same stream)
int kl_hyper_plan(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int np_, int L, void* wsbase,
                  const int* covflag, hipStream_t st);
// the binned hyper-gradient (raw sums into part, the table adjoint's layout with G workgroup slots); its kernels
// exit at once when the plan is off
int kl_hyper_bwd(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int np_, int L, const double* params,
                 const float* Kinv, const float* v, const double* alpha, const double* kdiag, void* wsbase, double* part,
                 int G, hipStream_t st);

}  // namespace lvae
