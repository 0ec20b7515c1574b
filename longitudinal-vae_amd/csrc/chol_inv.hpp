// chol_inv.hpp -- what chol_inv.hip exports to the exact KL (kl_closed.hip) and to lvae_potrf_f32 (potrf.hip):
// the batched fp32 Cholesky factor, Y = L^-1 and K^-1 = Y^T Y of [L, np, np] matrices, np a multiple of 256.
#pragma once
#include "common.hpp"

namespace lvae {

// The ONE decision for the pipelined schedule: the scratch layout, the factor's schedule, the lauum's `pre` flag
// and the exact KL's early-reduce gate all ask here.
bool ci_pipe_mode(int np_, int L);
size_t ci_scratch_bytes(int np_, int L);
// potrf + trtri: Y = L^-1 as the Y^T planes YT (+ the per-tile scales in the scratch); A and Kinv are overwritten
// (Kinv holds the X^T planes).  lout: potrf only -- no trtri, no pipelined schedule -- with L written in fp32 into
// lout's lower tiles.
int ci_factor_f32(int np_, int L, float* A, void* scratch, _Float16* YT, float* Kinv, double* logdet,
                  int32_t* info, hipStream_t st, float* lout = nullptr);
// lauum, K^-1 = Y^T Y from ci_factor_f32's Y^T planes.  With mu (the exact KL's reduce): also the partials of
// K^-1 mu (apart) and, if Bh, the planes of B = K^-1 diag(sqrt v) with their scale bsc[L].
int ci_lauum_f32(int np_, int L, void* scratch, const _Float16* YT, float* Kinv, const double* mu, const float* sv,
                 float* apart, _Float16* Bh, float* bsc, hipStream_t st, const int* hbon);
// lauum for the dims with flag[l] != 0 only (device flags); K^-1 tiles + mirror into Kinv
int ci_lauum_flagged_f32(int np_, int L, void* scratch, const _Float16* YT, float* Kinv, const int* flag,
                         hipStream_t st);
// the per-tile split scales of Y (ysc(l, i, j), both plane orientations) in the factor's scratch
const float* ci_ysc_ptr(void* scratch, int np_, int L);
// potrf alone (lvae_potrf_f32): A [L, np, np] -> L in A's lower tiles (fp32; zero strict upper part of the diagonal
// tiles; the other upper tiles untouched), log|A|, info
int ci_potrf_f32(int np_, int L, float* A, void* scratch, double* logdet, int32_t* info, hipStream_t st);

}  // namespace lvae
