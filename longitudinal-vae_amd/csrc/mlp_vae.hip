// mlp_vae.hip -- the MLP encoder / decoder (SimpleVAE, VAE.py:165-253) with each half's weights resident in LDS.
//
// Every product runs on v_mfma_f32_32x32x2_f32 (exact f32, a k-ordered fma chain).  A workgroup of 4 waves stages its
// half's weights once in their native [out][in] layout with an ODD row stride, then walks 32-row tiles of the batch:
//   forward   C [row][out] = sum_k act [row][k] W [out][k]   (B operand: lane = out, stride odd: conflict-free)
//   backward  C [row][in]  = sum_k g [row][k]   W [k][in]    (B operand: lane = in, consecutive: conflict-free)
// The activations of a tile live in LDS as [32][odd stride] (A operand: lane = row).  A layer whose output is at most
// 64 wide with K >= 128 (300 -> 30, 300 -> D) splits K over the waves and sums the partials in wave order.
// Weight gradients: one launch over every 32 x 32 output tile of the half's dW = g^T h, operands straight from global
// memory (lane = column: coalesced), K = the batch rows in order; above kSplitRows rows the batch is cut into chunks
// whose partial tiles go to the workspace, and the chunk that finishes last (an integer ticket per tile) adds them in
// chunk order -- the sum order is fixed, whichever chunk that is.
#include <atomic>

#include "common.hpp"

namespace {
using namespace lvae;

typedef float mv_f32x16 __attribute__((ext_vector_type(16)));
constexpr int kH1 = 300, kH2 = 30, kMaxL = 32;
constexpr int kS1 = 301, kS2 = 31;  // odd LDS row strides of the 300- and 30-wide rows
constexpr int kCUs = 256;
constexpr size_t kLdsMax = 160 * 1024;
constexpr int kSplitRows = 512, kMaxSplits = 64;
constexpr int kPartTile = 32 * 32 + 32;  // a partial tile and its bias-gradient slice

__host__ __device__ constexpr int odd(int k) { return k | 1; }
__device__ __forceinline__ int acc_row(int q, int hi) { return (q & 3) + 8 * (q >> 2) + 4 * hi; }

// dst [N][S] <- w [N][K] (row stride S >= K)
__device__ __forceinline__ void stage(const float* __restrict__ w, int N, int K, float* dst, int S) {
  for (int e = threadIdx.x; e < N * K; e += 256) {
    const int n = e / K;
    dst[n * S + (e - n * K)] = w[e];
  }
}

// epi(r, j, sum_k in [r][k] Wop [k][j]) for r < 32, j < N; Wop [k][j] = W [j WS + k] (TRANS = false) or W [k WS + j].
// With K >= 128 and N <= 64 the waves split K and `scratch` (4 x 32 x 33 floats; may alias `in`) holds their partials.
// The caller syncs before (operands staged) and after (epi's writes visible).
template <bool TRANS, class Epi>
__device__ __forceinline__ void layer(const float* in, int inS, int K, const float* W, int WS, int N, float* scratch,
                                      Epi epi) {
  const int t = threadIdx.x, lane = t & 63, l32 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nt = (N + 31) >> 5;
  const int ks = (K >= 128 && nt <= 2) ? 4 / nt : 1;
  const float* ar = in + l32 * inS;
  if (ks == 1) {
    for (int tile = wave; tile < nt; tile += 4) {
      const int j = tile * 32 + l32;
      const bool jv = j < N;
      const int jc = jv ? j : N - 1;
      mv_f32x16 acc;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll 4
      for (int k0 = 0; k0 < K; k0 += 2) {
        const int k = k0 + hi;
        const bool kv = k < K;
        const int kc = kv ? k : K - 1;
        const float a = ar[kc];
        const float b = TRANS ? W[kc * WS + jc] : W[jc * WS + kc];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kv ? a : 0.f, (kv && jv) ? b : 0.f, acc, 0, 0, 0);
      }
      if (jv) {
#pragma unroll
        for (int q = 0; q < 16; ++q) epi(acc_row(q, hi), j, acc[q]);
      }
    }
    return;
  }
  {  // nt ks == 4: wave -> (tile, K chunk)
    const int tile = wave / ks, chunk = wave - tile * ks;
    const int kch = (((K + ks - 1) / ks) + 1) & ~1;
    const int kb = chunk * kch, ke = min(K, kb + kch);
    const int j = tile * 32 + l32;
    const bool jv = j < N;
    const int jc = jv ? j : N - 1;
    mv_f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll 4
    for (int k0 = kb; k0 < ke; k0 += 2) {
      const int k = k0 + hi;
      const bool kv = k < ke;
      const int kc = kv ? k : ke - 1;
      const float a = ar[kc];
      const float b = TRANS ? W[kc * WS + jc] : W[jc * WS + kc];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kv ? a : 0.f, (kv && jv) ? b : 0.f, acc, 0, 0, 0);
    }
    __syncthreads();  // every wave is done reading `in`: scratch may overwrite it
#pragma unroll
    for (int q = 0; q < 16; ++q) scratch[(wave * 32 + acc_row(q, hi)) * 33 + l32] = acc[q];
    __syncthreads();
    for (int e = t; e < nt * 1024; e += 256) {
      const int tl = e >> 10, r = (e >> 5) & 31, c = e & 31, jj = tl * 32 + c;
      float s = scratch[((tl * ks) * 32 + r) * 33 + c];
      for (int ch = 1; ch < ks; ++ch) s += scratch[((tl * ks + ch) * 32 + r) * 33 + c];
      if (jj < N) epi(r, jj, s);
    }
  }
}

__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }

// ---------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------
__host__ __device__ constexpr size_t enc_fwd_floats(int D, int L) {
  return (size_t)kH1 * odd(D) + kH2 * kS1 + 2 * L * kS2 + kH1 + kH2 + 2 * L + 32 * odd(D) + 32 * kS1 + 32 * kS2;
}
__host__ __device__ constexpr size_t dec_fwd_floats(int D, int L) {
  return (size_t)kH2 * odd(L) + kH1 * kS2 + (size_t)D * kS1 + kH2 + kH1 + D + 32 * odd(L) + 32 * kS2 + 32 * kS1;
}
__host__ __device__ constexpr size_t dec_bwd_floats(int D, int L) {
  return (size_t)D * kS1 + kH1 * kS2 + kH2 * odd(L) + 32 * odd(D) + 32 * kS1 + 32 * kS2;
}
__host__ __device__ constexpr size_t enc_bwd_floats(int L) {
  return (size_t)2 * L * kS2 + kH2 * kS1 + 32 * odd(2 * L) + 32 * kS2;
}

__global__ __launch_bounds__(256) void mlp_enc_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w21, const float* __restrict__ b21, const float* __restrict__ w211,
    const float* __restrict__ b211, const float* __restrict__ w221, const float* __restrict__ b221, int B, int D, int L,
    float* __restrict__ h1, float* __restrict__ h2, float* __restrict__ mu, float* __restrict__ lv) {
  extern __shared__ float mlp_lds[];
  const int SD = odd(D), L2 = 2 * L, t = threadIdx.x;
  float* w1s = mlp_lds;             // [300][SD]
  float* w21s = w1s + kH1 * SD;     // [30][301]
  float* w2s = w21s + kH2 * kS1;    // [2L][31]: fc211 over fc221
  float* b1s = w2s + L2 * kS2;      // [300]
  float* b21s = b1s + kH1;          // [30]
  float* b2s = b21s + kH2;          // [2L]
  float* xs = b2s + L2;             // [32][SD]
  float* h1s = xs + 32 * SD;        // [32][301]
  float* h2s = h1s + 32 * kS1;      // [32][31]
  stage(w1, kH1, D, w1s, SD);
  stage(w21, kH2, kH1, w21s, kS1);
  stage(w211, L, kH2, w2s, kS2);
  stage(w221, L, kH2, w2s + L * kS2, kS2);
  for (int e = t; e < kH1; e += 256) b1s[e] = b1[e];
  if (t < kH2) b21s[t] = b21[t];
  if (t < L) {
    b2s[t] = b211[t];
    b2s[L + t] = b221[t];
  }
  const int ntile = (B + 31) >> 5;
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int r0 = tile * 32, nr = min(32, B - r0);
    for (int e = t; e < 32 * D; e += 256) {
      const int r = e / D, c = e - r * D;
      xs[r * SD + c] = r < nr ? x[(size_t)(r0 + r) * D + c] : 0.f;
    }
    __syncthreads();
    layer<false>(xs, SD, D, w1s, SD, kH1, nullptr, [&](int r, int j, float v) {
      v = relu_keep_nan(v + b1s[j]);
      h1s[r * kS1 + j] = v;
      if (h1 && r < nr) h1[(size_t)(r0 + r) * kH1 + j] = v;
    });
    __syncthreads();
    layer<false>(h1s, kS1, kH1, w21s, kS1, kH2, h1s, [&](int r, int j, float v) {
      v = relu_keep_nan(v + b21s[j]);
      h2s[r * kS2 + j] = v;
      if (h2 && r < nr) h2[(size_t)(r0 + r) * kH2 + j] = v;
    });
    __syncthreads();
    layer<false>(h2s, kS2, kH2, w2s, kS2, L2, nullptr, [&](int r, int j, float v) {
      v += b2s[j];
      if (r < nr) {
        if (j < L) mu[(size_t)(r0 + r) * L + j] = v;
        else lv[(size_t)(r0 + r) * L + (j - L)] = v;
      }
    });
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void mlp_dec_fwd_kernel(
    const float* __restrict__ z, const float* __restrict__ mu, const float* __restrict__ lv,
    const float* __restrict__ eps, const float* __restrict__ w3, const float* __restrict__ b3,
    const float* __restrict__ w31, const float* __restrict__ b31, const float* __restrict__ w4,
    const float* __restrict__ b4, int B, int D, int L, float* __restrict__ z_out, float* __restrict__ h3,
    float* __restrict__ h4, float* __restrict__ recon) {
  extern __shared__ float mlp_lds[];
  const int SL = odd(L), t = threadIdx.x;
  float* w3s = mlp_lds;             // [30][SL]
  float* w31s = w3s + kH2 * SL;     // [300][31]
  float* w4s = w31s + kH1 * kS2;    // [D][301]
  float* b3s = w4s + D * kS1;       // [30]
  float* b31s = b3s + kH2;          // [300]
  float* b4s = b31s + kH1;          // [D]
  float* zs = b4s + D;              // [32][SL]
  float* h3s = zs + 32 * SL;        // [32][31]
  float* h4s = h3s + 32 * kS2;      // [32][301]
  stage(w3, kH2, L, w3s, SL);
  stage(w31, kH1, kH2, w31s, kS2);
  stage(w4, D, kH1, w4s, kS1);
  if (t < kH2) b3s[t] = b3[t];
  for (int e = t; e < kH1; e += 256) b31s[e] = b31[e];
  for (int e = t; e < D; e += 256) b4s[e] = b4[e];
  const int ntile = (B + 31) >> 5;
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int r0 = tile * 32, nr = min(32, B - r0);
    for (int e = t; e < 32 * L; e += 256) {
      const int r = e / L, c = e - r * L;
      float v = 0.f;
      if (r < nr) {
        const size_t i = (size_t)(r0 + r) * L + c;
        if (z) {
          v = z[i];
        } else {  // the reparametrisation (VAE.py:246-248)
          v = mu[i] + eps[i] * expf(0.5f * lv[i]);
          z_out[i] = v;
        }
      }
      zs[r * SL + c] = v;
    }
    __syncthreads();
    layer<false>(zs, SL, L, w3s, SL, kH2, nullptr, [&](int r, int j, float v) {
      v = relu_keep_nan(v + b3s[j]);
      h3s[r * kS2 + j] = v;
      if (h3 && r < nr) h3[(size_t)(r0 + r) * kH2 + j] = v;
    });
    __syncthreads();
    layer<false>(h3s, kS2, kH2, w31s, kS2, kH1, nullptr, [&](int r, int j, float v) {
      v = relu_keep_nan(v + b31s[j]);
      h4s[r * kS1 + j] = v;
      if (h4 && r < nr) h4[(size_t)(r0 + r) * kH1 + j] = v;
    });
    __syncthreads();
    layer<false>(h4s, kS1, kH1, w4s, kS1, D, h4s, [&](int r, int j, float v) {
      if (r < nr) recon[(size_t)(r0 + r) * D + j] = 1.f / (1.f + expf(-(v + b4s[j])));
    });
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------
// backward: the chain of activation gradients (pre-activation gradients to the workspace for the weight gradients)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mlp_dec_bwd_chain_kernel(
    const float* __restrict__ g_recon, const float* __restrict__ recon, const float* __restrict__ h4,
    const float* __restrict__ h3, const float* __restrict__ lv, const float* __restrict__ eps,
    const float* __restrict__ w3, const float* __restrict__ w31, const float* __restrict__ w4, int B, int D, int L,
    float* __restrict__ gp4, float* __restrict__ gp31, float* __restrict__ gp3, float* __restrict__ g_z,
    float* __restrict__ g_mu, float* __restrict__ g_lv, unsigned* __restrict__ cnt, int ncnt) {
  extern __shared__ float mlp_lds[];
  const int SD = odd(D), SL = odd(L), t = threadIdx.x;
  float* w4s = mlp_lds;             // [D][301]
  float* w31s = w4s + D * kS1;      // [300][31]
  float* w3s = w31s + kH1 * kS2;    // [30][SL]
  float* g4s = w3s + kH2 * SL;      // [32][SD]
  float* gs = g4s + 32 * SD;        // [32][301]
  float* g3s = gs + 32 * kS1;       // [32][31]
  if (blockIdx.x == 0)
    for (int e = t; e < ncnt; e += 256) cnt[e] = 0u;  // the weight-gradient launch's tickets
  stage(w4, D, kH1, w4s, kS1);
  stage(w31, kH1, kH2, w31s, kS2);
  stage(w3, kH2, L, w3s, SL);
  const int ntile = (B + 31) >> 5;
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int r0 = tile * 32, nr = min(32, B - r0);
    for (int e = t; e < 32 * D; e += 256) {
      const int r = e / D, c = e - r * D;
      float v = 0.f;
      if (r < nr) {
        const size_t i = (size_t)(r0 + r) * D + c;
        const float y = recon[i];
        v = g_recon[i] * ((1.f - y) * y);
        gp4[i] = v;
      }
      g4s[r * SD + c] = v;
    }
    __syncthreads();
    layer<true>(g4s, SD, D, w4s, kS1, kH1, nullptr, [&](int r, int j, float v) {
      float o = 0.f;
      if (r < nr) {
        const size_t i = (size_t)(r0 + r) * kH1 + j;
        o = h4[i] <= 0.f ? 0.f : v;
        gp31[i] = o;
      }
      gs[r * kS1 + j] = o;
    });
    __syncthreads();
    layer<true>(gs, kS1, kH1, w31s, kS2, kH2, gs, [&](int r, int j, float v) {
      float o = 0.f;
      if (r < nr) {
        const size_t i = (size_t)(r0 + r) * kH2 + j;
        o = h3[i] <= 0.f ? 0.f : v;
        gp3[i] = o;
      }
      g3s[r * kS2 + j] = o;
    });
    __syncthreads();
    layer<true>(g3s, kS2, kH2, w3s, SL, L, nullptr, [&](int r, int j, float v) {
      if (r < nr) {
        const size_t i = (size_t)(r0 + r) * L + j;
        if (g_z) g_z[i] = v;
        if (g_mu) {  // the reparametrisation's adjoint
          g_mu[i] = v;
          g_lv[i] = v * eps[i] * (0.5f * expf(0.5f * lv[i]));
        }
      }
    });
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void mlp_enc_bwd_chain_kernel(
    const float* __restrict__ g_mu, const float* __restrict__ g_lv, const float* __restrict__ h1,
    const float* __restrict__ h2, const float* __restrict__ w21, const float* __restrict__ w211,
    const float* __restrict__ w221, int B, int L, float* __restrict__ gp1, float* __restrict__ gp21,
    unsigned* __restrict__ cnt, int ncnt) {
  extern __shared__ float mlp_lds[];
  const int L2 = 2 * L, S2L = odd(L2), t = threadIdx.x;
  float* w2s = mlp_lds;             // [2L][31]
  float* w21s = w2s + L2 * kS2;     // [30][301]
  float* g2s = w21s + kH2 * kS1;    // [32][S2L]
  float* g21s = g2s + 32 * S2L;     // [32][31]
  if (blockIdx.x == 0)
    for (int e = t; e < ncnt; e += 256) cnt[e] = 0u;
  stage(w211, L, kH2, w2s, kS2);
  stage(w221, L, kH2, w2s + L * kS2, kS2);
  stage(w21, kH2, kH1, w21s, kS1);
  const int ntile = (B + 31) >> 5;
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int r0 = tile * 32, nr = min(32, B - r0);
    for (int e = t; e < 32 * L2; e += 256) {
      const int r = e / L2, c = e - r * L2;
      float v = 0.f;
      if (r < nr) v = c < L ? g_mu[(size_t)(r0 + r) * L + c] : g_lv[(size_t)(r0 + r) * L + (c - L)];
      g2s[r * S2L + c] = v;
    }
    __syncthreads();
    layer<true>(g2s, S2L, L2, w2s, kS2, kH2, nullptr, [&](int r, int j, float v) {
      float o = 0.f;
      if (r < nr) {
        const size_t i = (size_t)(r0 + r) * kH2 + j;
        o = h2[i] <= 0.f ? 0.f : v;
        gp21[i] = o;
      }
      g21s[r * kS2 + j] = o;
    });
    __syncthreads();
    layer<true>(g21s, kS2, kH2, w21s, kS1, kH1, nullptr, [&](int r, int j, float v) {
      if (r < nr) {
        const size_t i = (size_t)(r0 + r) * kH1 + j;
        gp1[i] = h1[i] <= 0.f ? 0.f : v;
      }
    });
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------
// backward: every weight and bias gradient of a half in one launch
// ---------------------------------------------------------------------------------------------------
struct WgJob {  // dW [M][N] = g [B][M]^T h [B][N], db [M] = the column sums of g
  const float* g;
  const float* h;
  float* dW;
  float* db;
  int ldg, ldh, M, N, tile0, ntj;
};
struct WgArgs {
  WgJob job[4];
  int njobs, B, splits, rows;
  float* part;
  unsigned* cnt;
};

__global__ __launch_bounds__(64) void mlp_wgrad_kernel(WgArgs a) {
  const int lane = threadIdx.x, l32 = lane & 31, hi = lane >> 5;
  const int tile = blockIdx.x / a.splits, split = blockIdx.x - tile * a.splits;
  const float* g = a.job[0].g;
  const float* h = a.job[0].h;
  float* dW = a.job[0].dW;
  float* db = a.job[0].db;
  int ldg = a.job[0].ldg, ldh = a.job[0].ldh, M = a.job[0].M, N = a.job[0].N, tile0 = 0, ntj = a.job[0].ntj;
#pragma unroll
  for (int q = 1; q < 4; ++q) {
    if (q < a.njobs && tile >= a.job[q].tile0) {
      g = a.job[q].g, h = a.job[q].h, dW = a.job[q].dW, db = a.job[q].db;
      ldg = a.job[q].ldg, ldh = a.job[q].ldh, M = a.job[q].M, N = a.job[q].N;
      tile0 = a.job[q].tile0, ntj = a.job[q].ntj;
    }
  }
  const int lt = tile - tile0, ti = lt / ntj, tj = lt - ti * ntj;
  const int i = ti * 32 + l32, j = tj * 32 + l32;
  const bool iv = i < M, jv = j < N;
  const int ic = iv ? i : 0, jc = jv ? j : 0;
  const int b0 = split * a.rows, b1 = min(a.B, b0 + a.rows);
  mv_f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  float dbs = 0.f;
#pragma unroll 4
  for (int s = b0; s < b1; s += 2) {
    const int b = s + hi;
    const bool bv = b < b1;
    const size_t bc = (size_t)(bv ? b : b1 - 1);
    float av = g[bc * ldg + ic], hv = h[bc * ldh + jc];
    av = (bv && iv) ? av : 0.f;
    hv = (bv && jv) ? hv : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, hv, acc, 0, 0, 0);
    dbs += av;
  }
  dbs += __shfl_xor(dbs, 32);  // even rows + odd rows
  if (a.splits == 1) {
    if (jv) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int r = ti * 32 + acc_row(q, hi);
        if (r < M) dW[(size_t)r * N + j] = acc[q];
      }
    }
    if (tj == 0 && hi == 0 && iv) db[i] = dbs;
    return;
  }
  float* p = a.part + (size_t)(tile * a.splits + split) * kPartTile;
#pragma unroll
  for (int q = 0; q < 16; ++q) p[acc_row(q, hi) * 32 + l32] = acc[q];
  if (hi == 0) p[1024 + l32] = dbs;
  __threadfence();  // the partial is out before the ticket is taken
  unsigned old = 0u;
  if (lane == 0) old = atomicAdd(&a.cnt[tile], 1u);
  old = __shfl(old, 0);
  if (old != (unsigned)(a.splits - 1)) return;
  __threadfence();  // the last chunk of this tile: every chunk's partial is visible; add them in chunk order
  const float* p0 = a.part + (size_t)tile * a.splits * kPartTile;
  if (jv) {
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {
      const int rl = acc_row(q, hi), r = ti * 32 + rl;
      float s = 0.f;
      for (int sp = 0; sp < a.splits; ++sp) s += p0[(size_t)sp * kPartTile + rl * 32 + l32];
      if (r < M) dW[(size_t)r * N + j] = s;
    }
  }
  if (tj == 0 && hi == 0 && iv) {
    float s = 0.f;
    for (int sp = 0; sp < a.splits; ++sp) s += p0[(size_t)sp * kPartTile + 1024 + l32];
    db[i] = s;
  }
}

int splits_of(int B) { return B <= kSplitRows ? 1 : min(kMaxSplits, cdiv(B, kSplitRows)); }
int dec_tiles(int D, int L) { return cdiv(D, 32) * cdiv(kH1, 32) + cdiv(kH1, 32) + 1; }
int enc_tiles(int D, int L) { return cdiv(kH1, 32) * cdiv(D, 32) + cdiv(kH1, 32) + 2; }

bool shape_ok(int H1, int H2, int L) { return H1 == kH1 && H2 == kH2 && L <= kMaxL; }
size_t lds_bytes(int D, int L) {
  size_t f = enc_fwd_floats(D, L);
  f = f > dec_fwd_floats(D, L) ? f : dec_fwd_floats(D, L);
  f = f > dec_bwd_floats(D, L) ? f : dec_bwd_floats(D, L);
  f = f > enc_bwd_floats(L) ? f : enc_bwd_floats(L);
  return sizeof(float) * f;
}

// More than 64 KB of dynamic LDS has to be asked for, per kernel and per device.  `done` is the calling entry's bit
// mask of the devices (ids < 64; others ask every time) on which it has asked: the only state the library keeps here,
// and one that only saves repeating an idempotent call (and keeps it out of a stream capture after the warm-up).
template <class Kern>
int allow_lds(Kern k, std::atomic<uint64_t>& done) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return LVAE_ERR_LAUNCH;
  const uint64_t bit = dev >= 0 && dev < 64 ? uint64_t(1) << dev : 0;
  if (bit && (done.load(std::memory_order_acquire) & bit)) return 0;
  if (hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax) != hipSuccess)
    return LVAE_ERR_LAUNCH;
  done.fetch_or(bit, std::memory_order_release);
  return 0;
}

int launch_wgrad(WgArgs& a, int ntiles, int B, void* part, void* cnt, hipStream_t st) {
  a.B = B;
  a.splits = splits_of(B);
  a.rows = ((cdiv(B, a.splits) + 1) & ~1);
  a.part = (float*)part;
  a.cnt = (unsigned*)cnt;
  mlp_wgrad_kernel<<<ntiles * a.splits, 64, 0, st>>>(a);
  LVAE_CHECK_LAUNCH();
  return 0;
}

void add_job(WgArgs& a, int& tiles, const float* g, int ldg, const float* h, int ldh, int M, int N, float* dW,
             float* db) {
  WgJob& j = a.job[a.njobs++];
  j.g = g, j.h = h, j.dW = dW, j.db = db, j.ldg = ldg, j.ldh = ldh, j.M = M, j.N = N;
  j.tile0 = tiles, j.ntj = cdiv(N, 32);
  tiles += cdiv(M, 32) * j.ntj;
}

// workspace: the pre-activation gradients, the partial tiles (only with splits), the tickets
struct DecWs {
  float *gp4, *gp31, *gp3, *part;
  unsigned* cnt;
  size_t bytes;
  DecWs(char* base, int B, int D, int L) {
    size_t off = 0;
    auto take = [&](size_t n) {
      char* q = base ? base + off : nullptr;
      off += align256(n);
      return q;
    };
    gp4 = (float*)take(sizeof(float) * (size_t)B * D);
    gp31 = (float*)take(sizeof(float) * (size_t)B * kH1);
    gp3 = (float*)take(sizeof(float) * (size_t)B * kH2);
    const int s = splits_of(B);
    part = (float*)take(s > 1 ? sizeof(float) * (size_t)dec_tiles(D, L) * s * kPartTile : 0);
    cnt = (unsigned*)take(sizeof(unsigned) * dec_tiles(D, L));
    bytes = off;
  }
};
struct EncWs {
  float *gp1, *gp21, *part;
  unsigned* cnt;
  size_t bytes;
  EncWs(char* base, int B, int D, int L) {
    size_t off = 0;
    auto take = [&](size_t n) {
      char* q = base ? base + off : nullptr;
      off += align256(n);
      return q;
    };
    gp1 = (float*)take(sizeof(float) * (size_t)B * kH1);
    gp21 = (float*)take(sizeof(float) * (size_t)B * kH2);
    const int s = splits_of(B);
    part = (float*)take(s > 1 ? sizeof(float) * (size_t)enc_tiles(D, L) * s * kPartTile : 0);
    cnt = (unsigned*)take(sizeof(unsigned) * enc_tiles(D, L));
    bytes = off;
  }
};

}  // namespace

extern "C" {

size_t lvae_mlp_vae_lds_bytes(int D, int H1, int H2, int L) {
  if (D < 1 || L < 1 || !shape_ok(H1, H2, L)) return 0;
  return lds_bytes(D, L);
}

int lvae_mlp_vae_fused_ok(int D, int H1, int H2, int L) {
  const size_t b = lvae_mlp_vae_lds_bytes(D, H1, H2, L);
  return b > 0 && b <= kLdsMax ? 1 : 0;
}

int lvae_mlp_wgrad_splits(int B) { return B < 1 ? 0 : splits_of(B); }

size_t lvae_mlp_dec_bwd_workspace_size(int B, int D, int L) {
  return B < 1 || D < 1 || L < 1 ? 0 : DecWs(nullptr, B, D, L).bytes;
}
size_t lvae_mlp_enc_bwd_workspace_size(int B, int D, int L) {
  return B < 1 || D < 1 || L < 1 ? 0 : EncWs(nullptr, B, D, L).bytes;
}

#define MLP_CHECK_SHAPE()                                     \
  do {                                                        \
    if (B < 1 || D < 1 || H1 < 1 || H2 < 1 || L < 1) return -2; \
    if (!shape_ok(H1, H2, L)) return -3;                      \
    if (lds_bytes(D, L) > kLdsMax) return -4;                 \
  } while (0)

int lvae_mlp_enc_fwd_f32(const float* x, const float* w1, const float* b1, const float* w21, const float* b21,
                         const float* w211, const float* b211, const float* w221, const float* b221, int B, int D,
                         int H1, int H2, int L, float* h1, float* h2, float* mu, float* log_var, void* stream) {
  if (!x || !w1 || !b1 || !w21 || !b21 || !w211 || !b211 || !w221 || !b221 || !mu || !log_var) return -1;
  MLP_CHECK_SHAPE();
  static std::atomic<uint64_t> asked{0};
  LVAE_TRY(allow_lds(mlp_enc_fwd_kernel, asked));
  mlp_enc_fwd_kernel<<<min(cdiv(B, 32), kCUs), 256, sizeof(float) * enc_fwd_floats(D, L), (hipStream_t)stream>>>(
      x, w1, b1, w21, b21, w211, b211, w221, b221, B, D, L, h1, h2, mu, log_var);
  LVAE_CHECK_LAUNCH();
  return 0;
}

int lvae_mlp_dec_fwd_f32(const float* z, const float* mu, const float* log_var, const float* eps, const float* w3,
                         const float* b3, const float* w31, const float* b31, const float* w4, const float* b4, int B,
                         int D, int H1, int H2, int L, float* z_out, float* h3, float* h4, float* recon,
                         void* stream) {
  if (!w3 || !b3 || !w31 || !b31 || !w4 || !b4 || !recon) return -1;
  if (!z && (!mu || !log_var || !eps || !z_out)) return -1;
  MLP_CHECK_SHAPE();
  static std::atomic<uint64_t> asked{0};
  LVAE_TRY(allow_lds(mlp_dec_fwd_kernel, asked));
  mlp_dec_fwd_kernel<<<min(cdiv(B, 32), kCUs), 256, sizeof(float) * dec_fwd_floats(D, L), (hipStream_t)stream>>>(
      z, mu, log_var, eps, w3, b3, w31, b31, w4, b4, B, D, L, z_out, h3, h4, recon);
  LVAE_CHECK_LAUNCH();
  return 0;
}

int lvae_mlp_dec_bwd_f32(const float* g_recon, const float* recon, const float* h4, const float* h3, const float* z,
                         const float* log_var, const float* eps, const float* w3, const float* w31, const float* w4,
                         int B, int D, int H1, int H2, int L, float* dw3, float* db3, float* dw31, float* db31,
                         float* dw4, float* db4, float* g_z, float* g_mu, float* g_log_var, void* workspace,
                         void* stream) {
  if (!g_recon || !recon || !h4 || !h3 || !z || !w3 || !w31 || !w4 || !workspace) return -1;
  const bool wgrad = dw3 || db3 || dw31 || db31 || dw4 || db4;  // all six or none (a frozen decoder)
  if (wgrad && (!dw3 || !db3 || !dw31 || !db31 || !dw4 || !db4)) return -1;
  const bool sampled = log_var || eps || g_mu || g_log_var;
  if (sampled ? (!log_var || !eps || !g_mu || !g_log_var) : !g_z) return -1;
  MLP_CHECK_SHAPE();
  if ((uintptr_t)workspace & 255) return -5;
  static std::atomic<uint64_t> asked{0};
  LVAE_TRY(allow_lds(mlp_dec_bwd_chain_kernel, asked));
  hipStream_t st = (hipStream_t)stream;
  DecWs ws((char*)workspace, B, D, L);
  const int ntiles = dec_tiles(D, L);
  mlp_dec_bwd_chain_kernel<<<min(cdiv(B, 32), kCUs), 256, sizeof(float) * dec_bwd_floats(D, L), st>>>(
      g_recon, recon, h4, h3, log_var, eps, w3, w31, w4, B, D, L, ws.gp4, ws.gp31, ws.gp3, g_z,
      sampled ? g_mu : nullptr, g_log_var, ws.cnt, ntiles);
  LVAE_CHECK_LAUNCH();
  if (!wgrad) return 0;
  WgArgs a;
  a.njobs = 0;
  int tiles = 0;
  add_job(a, tiles, ws.gp4, D, h4, kH1, D, kH1, dw4, db4);
  add_job(a, tiles, ws.gp31, kH1, h3, kH2, kH1, kH2, dw31, db31);
  add_job(a, tiles, ws.gp3, kH2, z, L, kH2, L, dw3, db3);
  return launch_wgrad(a, tiles, B, ws.part, ws.cnt, st);
}

int lvae_mlp_enc_bwd_f32(const float* g_mu, const float* g_log_var, const float* x, const float* h1, const float* h2,
                         const float* w21, const float* w211, const float* w221, int B, int D, int H1, int H2, int L,
                         float* dw1, float* db1, float* dw21, float* db21, float* dw211, float* db211, float* dw221,
                         float* db221, void* workspace, void* stream) {
  if (!g_mu || !g_log_var || !x || !h1 || !h2 || !w21 || !w211 || !w221 || !dw1 || !db1 || !dw21 || !db21 ||
      !dw211 || !db211 || !dw221 || !db221 || !workspace)
    return -1;
  MLP_CHECK_SHAPE();
  if ((uintptr_t)workspace & 255) return -5;
  static std::atomic<uint64_t> asked{0};
  LVAE_TRY(allow_lds(mlp_enc_bwd_chain_kernel, asked));
  hipStream_t st = (hipStream_t)stream;
  EncWs ws((char*)workspace, B, D, L);
  const int ntiles = enc_tiles(D, L);
  mlp_enc_bwd_chain_kernel<<<min(cdiv(B, 32), kCUs), 256, sizeof(float) * enc_bwd_floats(L), st>>>(
      g_mu, g_log_var, h1, h2, w21, w211, w221, B, L, ws.gp1, ws.gp21, ws.cnt, ntiles);
  LVAE_CHECK_LAUNCH();
  WgArgs a;
  a.njobs = 0;
  int tiles = 0;
  add_job(a, tiles, ws.gp1, kH1, x, D, kH1, D, dw1, db1);
  add_job(a, tiles, ws.gp21, kH2, h1, kH1, kH2, kH1, dw21, db21);
  add_job(a, tiles, g_mu, L, h2, kH2, L, kH2, dw211, db211);
  add_job(a, tiles, g_log_var, L, h2, kH2, L, kH2, dw221, db221);
  return launch_wgrad(a, tiles, B, ws.part, ws.cnt, st);
}

}  // extern "C"
