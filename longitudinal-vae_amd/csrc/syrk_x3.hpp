// syrk_x3.hpp -- what syrk_x3.hip exports to the exact KL's backward (kl_closed.hip): S = B B^T in fp32 from the
// fp16 hi / lo planes of B = K^-1 diag(sqrt v), lower tiles.
#pragma once
#include "common.hpp"

namespace lvae {

// K splits of the S GEMM (1, 2 or 4): the workspace holds splits - 1 further [L, np, np] partials (Sx), which
// kl_gram_bwd adds to S as it reads it
int syrk_x3_splits(int np_, int L);
// S (and the partials Sx) from the planes and their per-dim scale bsc[L]; *skip != 0 (device): the launch exits
int syrk_tiles_f32(int np_, int L, const float* bsc, const _Float16* planes, float* S, float* Sx, hipStream_t st,
                   const int* skip);

}  // namespace lvae
