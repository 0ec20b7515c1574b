// mfma_x3.hpp -- the fp32-accurate 3-product split on the f16 matrix cores: the error argument and the
// fragment types its users share (pv_lds.hpp, chol_inv.hip; x3_dma.hpp and x3_c16.hpp hold the GEMM cores).
//
// gfx950 has no xf32: fp32-input MFMA runs at 1/16 of the f16 rate (157 vs 2500 TFLOP/s dense).
// Each fp32 operand x is split once into x sc = hi + lo with hi, lo fp16 (sc a power of two from a bound on
// the operand's max |x|, x3_scale in common.hpp: the largest entries land in [2^13, 2^14), far from fp16
// overflow, and lo stays normal down to 2^-17 of them), and a product is
// hi_a hi_b + hi_a lo_b + lo_a hi_b: three v_mfma_f32_32x32x16_f16 with fp32 accumulation.  The
// dropped lo_a lo_b term and the split leave a relative error ~2^-22 per product -- between fp32
// (2^-24) and anything a 16-bit format gives -- at 3/16 of the fp32-MFMA cost.
//
// f16 operand maps (cdna_hip_programming.md §3): lane l holds A[row l&31][k = 8(l>>5) + j] and
// B[k = 8(l>>5) + j][col l&31], j = 0..7 -- both read as 8 contiguous halves of one LDS row [row][k].
//
// The generic 128 x 128 tile GEMMs that split their operands while staging them (tile_gemm on fp32 MFMA,
// tile_gemm_x3 on this split) had no caller left once every GEMM ran on the pre-split cores; commit 97b7453
// is the last that holds them (mfma_tile.hpp and this file).
#pragma once
#include "common.hpp"

namespace lvae {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 x3_half8 __attribute__((ext_vector_type(8)));
typedef _Float16 x3_half4 __attribute__((ext_vector_type(4)));

}  // namespace lvae
