// gp_bound.hpp -- what the full-batch GP-approximation bounds share: the DUBO (dubo.hip) and the sampled ELBO
// (gp_elbo.hip).  Both build X = k0(x, z), Kz, K0_p, B_p, walk the subjects in groups of kDuboS with Q in MFMA
// accumulators over the lower 16 x 16 tiles, form W = sym(Kz + Q) and invert it with one Newton step on a
// double-double residual; the tile maps, those two kernels, the info merge and the workspace carving are here.
#pragma once
#include "common.hpp"
#include "blkinv.hpp"
#include "gram_bwd.hpp"

namespace lvae {

int spd_inv_small_f64(int n, int batch, const double* A, int64_t stride, double* Ainv, int64_t stride_out,
                      double* logdet, int32_t* info, hipStream_t st);
int gemm_small_f64(int ta, int tb, int m, int n, int k, double alpha, const double* A, int lda, int64_t sa1,
                   int64_t sa2, const double* B, int ldb, int64_t sb1, int64_t sb2, double beta, double* C, int ldc,
                   int64_t sc1, int64_t sc2, int nb1, int nb2, hipStream_t st);

namespace {

constexpr int kDuboS = 16;     // subjects per workgroup of the fused pass (the group count is ceil(P / kDuboS))
constexpr int kDuboT = 32;     // largest T of the fused pass
constexpr int kDuboLD = 132;   // LDS row stride of the [T][M] tiles (128 + 4 doubles)
constexpr int kDuboTPW = 5;    // lower 16 x 16 tiles of Q (and of R) per wave: 36 tiles at M = 128 over 8 waves

inline int dubo_groups(int P) { return (P + kDuboS - 1) / kDuboS; }
inline int dubo_tiles(int M) {
  const int tm = (M + 15) / 16;
  return tm * (tm + 1) / 2;
}

inline int blocks(int64_t n) { return cdiv(n, 256); }

// Carves a workspace into 256-byte aligned arrays of doubles; a null base only measures (bytes = off at the end).
struct WsCarve {
  char* base;
  size_t off;
  explicit WsCarve(char* b) : base(b), off(0) {}
  double* take(size_t n) {
    double* q = base ? (double*)(base + off) : nullptr;
    off += align256(n * sizeof(double));
    return q;
  }
  // Gram-adjoint partials of the four Grams X, Kz, K0_p, B_p (gram.hip: 1024 elements per chunk, <= 145 slots)
  double* take_gram_part(size_t L, size_t N, size_t M, size_t TT) {
    const size_t chunks = (N * M + 1023) / 1024 + (M * M + 1023) / 1024 + 2 * ((TT + 1023) / 1024);
    return take(L * chunks * 145);
  }
};

__global__ void dubo_fill_kernel(double* p, int n, double v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// lower tile t -> (row tile, column tile), row-major over the lower triangle
__device__ inline void dubo_tile(int t, int& ti, int& tj) {
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  ti = i;
  tj = t - i * (i + 1) / 2;
}

// W = 1/2 ((Kz + Q) + (Kz + Q)^T)
__global__ void dubo_w_kernel(int L, int M, const double* __restrict__ Kz, const double* __restrict__ Q,
                              double* __restrict__ W) {
  const int64_t MM = (int64_t)M * M;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L * MM) return;
  const int64_t b = (e / MM) * MM;
  const int i = (int)((e % MM) / M), j = (int)(e % M);
  const int64_t f = b + (int64_t)j * M + i;
  W[e] = 0.5 * ((Kz[e] + Q[e]) + (Kz[f] + Q[f]));
}

// E = I - W Y with every dot product accumulated in double-double (two-product by fma, two-sum), rounded to
// fp64 at the end, and Y1 = Y: the residual of the first inverse of W, for the one Newton step Y1 += Y E.
// W = K0zz + Q has cond ~1e8..1e9 (K0zz's jitter), so Y = spd_inv_small(W) carries a forward error of ~1e-9
// |Y|; the bound's W terms (sum iW.R, p.iW p) see it directly (2.3e-9 of the bound on the reference's golden
// vector, whose own bound is 1e-9), while a residual formed in plain fp64 is as inexact as Y itself.
__global__ void dubo_resid_kernel(int L, int M, const double* __restrict__ W, const double* __restrict__ Y,
                                  double* __restrict__ E, double* __restrict__ Y1) {
#pragma clang fp contract(off)  // the error-free transforms below need every product and sum rounded on its own
  const int64_t MM = (int64_t)M * M;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L * MM) return;
  const int64_t b = (e / MM) * MM;
  const int i = (int)((e % MM) / M), j = (int)(e % M);
  const double* wr = W + b + (int64_t)i * M;
  const double* yc = Y + b + j;
  double hi = (i == j) ? 1.0 : 0.0, lo = 0.0;
  for (int k = 0; k < M; ++k) {
    const double a = -wr[k], y = yc[(int64_t)k * M];
    const double ph = a * y, pl = fma(a, y, -ph);  // a y = ph + pl exactly
    const double s = hi + ph, bb = s - hi;
    lo += ((hi - (s - bb)) + (ph - bb)) + pl;      // two-sum's error term + the product's
    hi = s;
  }
  E[e] = hi + lo;
  Y1[e] = Y[e];
}

// info[l]: first failure among Kz[l] (10000 + col), B_{l,p} (20000 + col), W[l] (30000 + col); w holds the
// factorisations' own info words as [L] (Kz), [L, P] (B_p), [L] (W)
__global__ void dubo_info_kernel(int L, int P, const int32_t* __restrict__ w, int32_t* __restrict__ info) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  int v = 0;
  if (w[l]) v = 10000 + w[l];
  for (int p = 0; p < P && !v; ++p)
    if (w[L + (int64_t)l * P + p]) v = 20000 + w[L + (int64_t)l * P + p];
  if (!v && w[L + (int64_t)L * P + l]) v = 30000 + w[L + (int64_t)L * P + l];
  info[l] = v;
}

}  // namespace
}  // namespace lvae
