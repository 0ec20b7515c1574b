// syrk_x3.hip -- S = K^-1 V K^-1 (lower tiles) for the exact-KL backward, the step's largest GEMM,
// on the f16 matrix cores with the fp32-accurate 3-product split (see mfma_x3.hpp for the error
// argument), specialised for throughput:
//
//   split : B = K^-1 diag(sqrt v) is split ONCE into fp16 hi / lo planes, with one power-of-two scale
//           per latent dim from a bound (ci_bscale_kernel), by the forward's lauum epilogue (which holds
//           the K^-1 tiles in registers anyway: chol_inv.hip, kCiLauumKL), into the chunk-major layout of
//           x3_c16.hpp; the epilogue here divides by the scale's square (the generic x3 tile GEMM would
//           re-split every operand chunk for every output tile);
//   syrk  : 256 x 256 output tiles, 512 threads = 8 waves, on the c16 core (x3_c16.hpp): a ring of
//           kC16NS 16-deep stages staged global -> LDS by DMA in whole 1 KB runs.
//
// Blocks are remapped so that each XCD (blockIdx % 8) works through a contiguous range of tiles
// of one latent dim, in the blocked order of sx_tri_blocked (row blocks of 4, inside a block by
// column): the 32 tiles an XCD runs at once form a 4 x 8 block sharing 4 A and 8 B panels in its L2
// (r3: 3.19 vs 3.46 ms at np = 4096, L = 16 against the row-major order; 51.1 vs 55.9 ms at
// np = 16384, L = 4).
//
// Earlier cores, measured against this one and removed (profiles/r3s_gemm_ab_c16.txt, DESIGN.md 4.1;
// commit 40b45d9 is the last that contains them and their dev entry point): row-major planes with one
// split scale per row on the 8-wave double-buffered core of x3_dma.hpp (r1-r2) and with one scale per dim
// (r3: 3.42 vs 2.85 ms here at np = 4096, L = 16; 51.6 vs 42.1 ms at np = 16384, L = 4, S bit-identical);
// per-tile scales with the accumulators rescaled at every K block (+10%); a 4-wave 4-stage core of
// 128 x 128 per wave; 256 x 128 half tiles with two workgroups per CU; the 8-wave core with 16-deep
// row-major chunks in a 4-stage ring (3.55 vs 3.18 ms at np = 4096, L = 16 and 87 vs 51 ms at np = 16384,
// L = 4: its 32-B row segments per chunk double the L2 traffic).
#include "syrk_x3.hpp"
#include "x3_c16.hpp"

#ifndef LVAE_SYRK_RESERVE
#define LVAE_SYRK_RESERVE 0
#endif

namespace lvae {

// K splits of the S GEMM: a 256-CU chip holds one 512-thread workgroup per CU (128 KB of LDS), so
// L * nt (nt + 1) / 2 tiles run in ceil(tiles / 256) rounds; with few latent dims per GPU (latent-dim
// sharding) the last round is mostly empty (L = 2: 272 tiles = 2 rounds for 1.06 rounds of work).
// Splitting K into s parts (partials summed by the Gram adjoint, which reads S anyway) runs
// ceil(s tiles / 256) rounds of 1/s the length, s in {2, 4}, taken only where the round count drops
// by more than 30%: a split pays its own prologue / epilogue and s-fold partial traffic (measured at
// np = 4096: L = 2 0.71 -> 0.60 ms with s = 4; L = 4 and L = 8 no gain or slower, L = 1 slower).
int syrk_x3_splits(int np_, int L) {
  const int nt = np_ / kSxT, tiles = L * nt * (nt + 1) / 2;
  auto cost = [&](int s) { return (double)((tiles * s + 255) / 256) / s; };
  int best = 1;
  for (int s : {2, 4})
    if (cost(s) < 0.7 * cost(best)) best = s;
  return best;
}

// The product S GEMM on the chunk-major planes (x3_c16.hpp): NS-stage ring of 16-deep chunks, fragments of
// the next chunk read under the current chunk's MFMAs.  B's planes carry ONE power-of-two scale per latent
// dim, bsc[l] (written by the exact KL's lauum epilogue, chol_inv.hip), so S = acc / bsc[l]^2; tiles in the
// blocked order above, K split by syrk_x3_splits.
template <int NS>
__global__ __launch_bounds__(512) void syrk_c16_kernel(const _Float16* __restrict__ Bh, const _Float16* __restrict__ Bl,
                                                       const float* __restrict__ bsc, float* __restrict__ S,
                                                       float* __restrict__ Sx, int np_, int ntl, int nwg, int L, int ns,
                                                       const int* __restrict__ skip) {
  __shared__ __attribute__((aligned(16))) _Float16 lds[NS * kC16Stage];
  if (skip && *skip) return;  // (uniform) the binned hyper-gradient needs no S (kl_hyper.hip)
  // tiles v = blockIdx.x, + gridDim.x, ...: one each with the full grid (nwg workgroups); a grid of fewer
  // (a multiple of 8: v keeps its blockIdx's XCD) leaves CUs to the ConvVAE stream (syrk_tiles_f32)
  for (int v = blockIdx.x; v < nwg; v += gridDim.x) {
    if (v != (int)blockIdx.x) __syncthreads();  // every wave's reads of the previous tile's stages are done
    const int orig = v, xcd = orig % 8, q8 = nwg / 8, r8 = nwg % 8;
    const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + orig / 8;
    const int sp = wgid / (ntl * L), l = (wgid / ntl) % L, nt = np_ / kSxT;
    int I, J;
    sx_tri_blocked(wgid % ntl, nt, I, J);
    const int kb0 = sp * nt / ns, kb1 = (sp + 1) * nt / ns;
    const int64_t ld = np_;
    const int64_t base = (int64_t)l * np_ * np_, c0 = (int64_t)kb0 * (kSxT / kC16BK) * kC16Part;
    sx_f32x16 acc[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = sx_f32x16{};
    if (kb1 > kb0) {
      const int64_t pa = c16_panel(l, np_, I) + c0, pb = c16_panel(l, np_, J) + c0;
      c16_gemm<NS>(C16Opnd{Bh + pa, Bl - Bh, 0}, C16Opnd{Bh + pb, Bl - Bh, 0}, (kb1 - kb0) * (kSxT / kC16BK), lds, acc);
    }
    const float sc = bsc[l], inv = 1.0f / (sc * sc);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float* C = (sp == 0 ? S : Sx + (int64_t)(sp - 1) * L * np_ * np_) + base + (int64_t)I * kSxT * ld + J * kSxT;
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(C, (short)0, 0x7fffffff, 0x00020000);
    const int vo = (((w >> 2) * 128 + 4 * (lane >> 5)) * np_ + (w & 3) * 64 + (lane & 31)) * 4;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int e = 0; e < 16; ++e)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[a][b][e] * inv), rc, vo,
                                                ((32 * a + (e & 3) + 8 * (e >> 2)) * np_ + 32 * b) * 4, 0);
  }
}

// CUs the S GEMM leaves free when its tiles outnumber the chip (LVAE_SYRK_RESERVE, compile-time, 0 = none): the
// exact KL's backward runs the S GEMM on the caller's stream while the encoder backward runs on the ConvVAE
// stream; with one 160 KB-LDS workgroup on every CU those small kernels wait for whole S-GEMM tiles
static int syrk_grid(int nwg) {
  static int cus = -1;
  if (cus < 0) {
    int dev = 0;
    hipDeviceProp_t pr;
    cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess) ? pr.multiProcessorCount
                                                                                                : 256;
  }
  constexpr int reserve = LVAE_SYRK_RESERVE;
  if (reserve <= 0 || nwg <= cus) return nwg;
  const int g = (cus - reserve) / 8 * 8;
  return g >= 8 ? g : nwg;
}

int syrk_tiles_f32(int np_, int L, const float* bsc, const _Float16* planes, float* S, float* Sx, hipStream_t st,
                   const int* skip) {
  if (np_ % kSxT) return -1;
  const int64_t per = (int64_t)np_ * np_;
  const int ns = syrk_x3_splits(np_, L);
  if (ns > 1 && !Sx) return -2;
  const int nt = np_ / kSxT, ntl = nt * (nt + 1) / 2, nwg = ntl * L * ns;
  syrk_c16_kernel<kC16NS><<<syrk_grid(nwg), 512, 0, st>>>(planes, planes + (int64_t)L * per, bsc, S, Sx, np_, ntl, nwg,
                                                          L, ns, skip);
  LVAE_CHECK_LAUNCH();
  return 0;
}

}  // namespace lvae
