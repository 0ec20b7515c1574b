// kl_resid_bins.hpp -- what kl_resid_bins.hip exports: the exact KL's fp64 residual in O(N W) for integer-coded
// covariates, planned by the factor (kl_closed.hip) and run inside kl_gram_resid (gram_matvec.hip).
#pragma once
#include "common.hpp"

namespace lvae {

size_t kl_resid_bins_bytes(int np_, int L, int ncomp);
// the plan's device flag (its place does not depend on the sizes); the factor zeroes it when the host gate is off
int* kl_resid_bins_okflag(void* wsbuf);
// the binned path runs iff the spec qualifies and LVAE_RESID_BINS is not "0"
bool kl_resid_bins_enabled(const lvae_kernel_spec* spec, int n);
// the plan (depends on x only; kl_closed.hip enqueues it on the side stream during the factorisation)
int kl_resid_bins_plan(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int np_, int L, void* wsbuf,
                       hipStream_t st);
// the bin sums and the residual, after the plan; *okflag = the plan's device flag (1: every component was binned --
// else these kernels exit at once and the caller's tiled kernels, given the flag, run)
int kl_resid_bins(const lvae_kernel_spec* spec, const double* x, int ldx, int n, int np_, int L,
                  const double* params, const double* noise, const double* alpha0, const double* muc, double* res,
                  void* wsbuf, int** okflag, hipStream_t st);

}  // namespace lvae
