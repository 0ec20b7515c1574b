// gp_bound.hpp -- what the inducing-point bounds share: the Hensman KL bound (hensman.hip), the DUBO (dubo.hip)
// and the sampled ELBO (gp_elbo.hip).  All three build X = k0(x, z), Kz, K0_p, B_p in one launch and contract the
// four adjoints in two; the host side of that, the argument check, the info merge and W's inverse (W = sym(Kz + Q),
// one Newton step on a double-double residual) are in gp_bound.hip.  The DUBO and the ELBO also walk the subjects
// in groups of kBoundS with Q in MFMA accumulators over the lower 16 x 16 tiles: the tile maps and the blocks of
// that walk the two subject kernels have in common are the device helpers below.
#pragma once
#include "common.hpp"
#include "blkinv.hpp"
#include "gram.hpp"
#include "small.hpp"

namespace lvae {

constexpr int kBoundS = 16;     // subjects per workgroup of the fused pass (the group count is ceil(P / kBoundS))
constexpr int kBoundT = 32;     // largest T of the fused pass
constexpr int kBoundLD = 132;   // LDS row stride of the [T][M] tiles (128 + 4 doubles)
constexpr int kBoundTPW = 5;    // lower 16 x 16 tiles of Q (and of R) per wave: 36 tiles at M = 128 over 8 waves

inline int bound_groups(int P) { return (P + kBoundS - 1) / kBoundS; }
inline int bound_tiles(int M) {
  const int tm = (M + 15) / 16;
  return tm * (tm + 1) / 2;
}

inline int blocks(int64_t n) { return cdiv(n, 256); }

// The sizes every bound's dims begin with: L latent dims, M inducing points, P subjects of T rows (the Hensman
// bound's P_b), Q covariates.  All zero stands for a null dims, which bound_check refuses like any L < 1.
struct BoundDims {
  int L, M, P, T, Q;
};

// -1 / -2: spec0 / spec1 null or outside every template bucket; -3: L < 1, M or T outside 1..128, P < 1 or Q < 1
int bound_check(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const BoundDims& d);

// doubles of the Gram adjoint's partials (gram_bwd_part_bytes of the four jobs of bound_grams_bwd)
size_t bound_gram_part_doubles(const BoundDims& d);

// epsv[l] = eps, then X = k0(x, z) [L,N,M], Kz = k0(z, z) + eps I [L,M,M], K0st = k0(x_p, x_p) and
// Bst = k1(x_p, x_p) + noise I [L,P,T,T] in one launch (gram_multi_f64)
int bound_grams_fwd(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const BoundDims& d, const double* x,
                    const double* z, const double* params0, const double* params1, const double* noise, double eps,
                    double* epsv, double* X, double* Kz, double* K0st, double* Bst, hipStream_t st);

// dparams0, dparams1, dnoise (may be null) = 0, then the four Grams' adjoints dX, dKz, dK0st, dBst contracted into
// them (gram_bwd_multi_f64 on gpart)
int bound_grams_bwd(const lvae_kernel_spec* spec0, const lvae_kernel_spec* spec1, const BoundDims& d, const double* x,
                    const double* z, const double* params0, const double* params1, const double* dX,
                    const double* dKz, const double* dK0st, const double* dBst, double* dparams0, double* dparams1,
                    double* dnoise, double* gpart, hipStream_t st);

// The z-adjoint the three bounds share.  bound_check_z: -1: spec0 null or outside every template bucket; -3: the
// dims, as bound_check.  bound_dz_part_bytes: bytes of the partials of bound_grams_bwd_z's three jobs.
int bound_check_z(const lvae_kernel_spec* spec0, const BoundDims& d);
size_t bound_dz_part_bytes(int L, int M, int N, int Q);
// dz[l] [M, Q] = d/dx2 of k0(x, z) against dX[l] + d/dx2 of k0(z, z) against dKz[l] + d/dx1 of k0(z, z) against
// dKz[l] (= d/dx2 against dKz[l]^T: the kernel is symmetric), as three jobs of gram_bwd_x2_multi_f64 on part; the
// eps I jitter does not depend on z.  dz is overwritten.
int bound_grams_bwd_z(const lvae_kernel_spec* spec0, const BoundDims& d, const double* x, const double* z,
                      const double* params0, const double* dX, const double* dKz, double* dz, double* part,
                      hipStream_t st);

// The z-adjoint's own workspace (lvae_bound_dz_workspace_size): the input adjoint's partials, and for the DUBO and
// the ELBO a re-formed dKz with its scratch (S [L,M,M]; A, G [L,N,M]).
struct BoundZWs {
  double *part, *dKz, *S, *A, *G;
  size_t bytes;
  BoundZWs(char* base, int L, int M, int N, int Q);
};
// dKz as the DUBO's / the ELBO's backward left it, with its two terms of the form iK Q iK and iW R iW (null: the
// ELBO has none) replaced by the same matrices formed from N x M factors, into zw.dKz:
//   iK Q iK = (X iK)^T (iBK iK),   iW R iW = (iBK iW)^T B_p (F iW)      (UmZ: the backward's Z = U - iBK iK)
// Inducing rows that coincide for k0 (rows of two subjects at one time point) leave Kz and W singular up to the
// jitter, iK and iW ~ 1 / eps on the pair's difference direction n; Q n = R n = 0 exactly, so the terms are
// moderate, but (iK Q) iK carries the rounding of iK Q times 1 / eps, as v n^T.  The hyper-parameter adjoint does
// not see that (dKz / dtheta has equal columns on the pair), the z-adjoint does (d k(z_i, z_a) / d z_a stands
// alone).  X iK and iBK iK lose nothing: the two columns of X are the same bits.  The replaced terms enter with
// the factor the backward used, read back as GK0[l][0] / iB[l][0].
int bound_dkz_stable(const BoundDims& d, const double* X, const double* iK, const double* iW, const double* U,
                     const double* UmZ, const double* F, const double* Bst, const double* iKQiK,
                     const double* iWRiW, const double* GK0, const double* iB, const double* dKz,
                     const BoundZWs& zw, hipStream_t st);

// info[l]: first failure among Kz[l] (10000 + col), B_{l,p} (20000 + col), W[l] or H[l] (30000 + col); w holds the
// factorisations' own info words as [L] (Kz), [L, P] (B_p), [L] (W / H)
void bound_info(int L, int P, const int32_t* w, int32_t* info, hipStream_t st);

// W = sym(Kz + Q); iW0 = spd_inv_small(W) (+ ldW, info); iW = iW0 + iW0 (I - W iW0), the residual E in double-double
int bound_w_inverse(int L, int M, const double* Kz, const double* Q, double* W, double* iW0, double* E, double* iW,
                    double* ldW, int32_t* info, hipStream_t st);

// ---- varying T (the DUBO's and the ELBO's *_seg_f64 calls): a [P, T] layout, subject p's seg[p] valid rows first ----

// valid rows of subject p, clamped to [0, T]: a bad seg gives wrong numbers, never an index out of range
// (seg == NULL: all T rows)
__device__ __forceinline__ int bound_seg_n(const int32_t* __restrict__ seg, int p, int T) {
  if (!seg) return T;
  const int n = seg[p];
  return n < 0 ? 0 : (n > T ? T : n);
}
__device__ __forceinline__ bool bound_seg_valid(const int32_t* __restrict__ seg, int p, int q, int T) {
  return q < bound_seg_n(seg, p, T);
}

// the subject kernels take seg as an optional trailing argument (a pack of none or one): the uniform instantiation
// then has the argument list it had before there was a seg
__device__ __forceinline__ const int32_t* bound_seg_arg() { return nullptr; }
__device__ __forceinline__ const int32_t* bound_seg_arg(const int32_t* seg) { return seg; }

// sum_p seg[p] as a double (integers: exact in any order), by all 256 threads of a workgroup
__device__ __forceinline__ double bound_seg_rows(const int32_t* __restrict__ seg, int P, int T, int tid,
                                                 double* red) {
  double n = 0.0;
  for (int p = tid; p < P; p += 256) n += (double)bound_seg_n(seg, p, T);
  return block_sum<256>(n, red);
}

// padding rows of X -> 0, padding rows / columns of K0_p -> 0 and of B_p -> I, in one launch (the Hensman bound's
// recipe, hn_seg_mask_kernel).  iB_p is then the identity on the padding, iBK_p has zero padding rows and log|B_p|
// is that of the valid block.
void bound_seg_mask(const BoundDims& d, const int32_t* seg, double* X, double* K0st, double* Bst, hipStream_t st);

// mm[i][l] = mu[i][l] on the valid rows, 0 on the padding rows whatever mu holds there ([N, L] like mu itself: the
// products that take mu as a GEMM operand must not read the padding, 0 * NaN is NaN)
void bound_seg_masked_rows(const BoundDims& d, const int32_t* seg, const double* mu, double* mm, hipStream_t st);

// ---- the fused subject walk (512 threads: 8 waves; lane = 16 lk + li) ----

// lower tile t -> (row tile, column tile), row-major over the lower triangle
__device__ inline void bound_tile(int t, int& ti, int& tj) {
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  ti = i;
  tj = t - i * (i + 1) / 2;
}

// wave wv owns the lower tiles t = wv + 8 k < nt of Q for the whole walk, in the accumulators Qa[k]
__device__ __forceinline__ void bound_walk_setup(int wv, int nt, int (&ti)[kBoundTPW], int (&tj)[kBoundTPW],
                                                 bool (&on)[kBoundTPW], bi_f64x4 (&Qa)[kBoundTPW]) {
#pragma unroll
  for (int k = 0; k < kBoundTPW; ++k) {
    const int t = wv + 8 * k;
    on[k] = t < nt;
    bound_tile(on[k] ? t : 0, ti[k], tj[k]);
    Qa[k] = bi_f64x4{0.0, 0.0, 0.0, 0.0};
  }
}

// the padding (rows T.., columns M..) is zeroed once; the walk only rewrites the valid parts
__device__ __forceinline__ void bound_lds_zero(int tid, double (&sB)[kBoundT][kBoundT + 1],
                                               double (&sX)[kBoundT][kBoundLD], double (&sY)[kBoundT][kBoundLD]) {
  for (int e = tid; e < kBoundT * (kBoundT + 1); e += 512) (&sB[0][0])[e] = 0.0;
  for (int e = tid; e < kBoundT * kBoundLD; e += 512) {
    (&sX[0][0])[e] = 0.0;
    (&sY[0][0])[e] = 0.0;
  }
}

// iB_p [T,T] -> sB with s_bk0 += sum iB_p . K0_p (this thread's elements), X_p [T,M] -> sX
__device__ __forceinline__ void bound_load_subject(int tid, int T, int M, const double* __restrict__ ib,
                                                   const double* __restrict__ k0, const double* __restrict__ xp,
                                                   double (&sB)[kBoundT][kBoundT + 1],
                                                   double (&sX)[kBoundT][kBoundLD], double& s_bk0) {
  for (int e = tid; e < T * T; e += 512) {
    const double b = ib[e];
    sB[e / T][e % T] = b;
    s_bk0 += b * k0[e];
  }
  for (int e = tid; e < T * M; e += 512) sX[e / M][e % M] = xp[e];
}

// one 16 x 16 tile at (r0, c0) of iBK_p = iB_p X_p on v_mfma_f64_16x16x4 (C[(lane >> 4) + 4 r][lane & 15]) -> sY
// and HBM (yp: iBK_p [T,M])
__device__ __forceinline__ void bound_ibk_tile(int r0, int c0, int li, int lk, int T, int M, int T4,
                                               const double (&sB)[kBoundT][kBoundT + 1],
                                               const double (&sX)[kBoundT][kBoundLD],
                                               double (&sY)[kBoundT][kBoundLD], double* __restrict__ yp) {
  bi_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int kk = 0; kk < T4; kk += 4)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sB[r0 + li][kk + lk], sX[kk + lk][c0 + li], acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = r0 + lk + 4 * r, j = c0 + li;
    sY[i][j] = acc[r];
    if (i < T && j < M) yp[(int64_t)i * M + j] = acc[r];
  }
}

// this wave's tiles of Q (or of R) into the group's partial, tile t at pp[256 t ..) in accumulator order
__device__ __forceinline__ void bound_store_tiles(double* __restrict__ pp, int wv, int lane,
                                                  const bool (&on)[kBoundTPW], const bi_f64x4 (&Qa)[kBoundTPW]) {
#pragma unroll
  for (int k = 0; k < kBoundTPW; ++k) {
    if (on[k]) {
      const int t = wv + 8 * k;
#pragma unroll
      for (int r = 0; r < 4; ++r) pp[((int64_t)t * 4 + r) * 64 + lane] = Qa[k][r];
    }
  }
}

// the reduce kernels' tile branch (256 threads): lower tile t of o [M,M] = the G groups' partials at pl[256 b ..),
// added in group order and mirrored into the upper triangle (a diagonal tile holds both of its halves itself)
__device__ __forceinline__ void bound_reduce_tile(int M, int G, int64_t pstride, const double* __restrict__ pl, int b,
                                                  int t, int tid, double* __restrict__ o) {
  double sum = 0.0;
  for (int g = 0; g < G; ++g) sum += pl[g * pstride + (int64_t)b * 256 + tid];
  const int r = tid >> 6, lane = tid & 63;
  int ti, tj;
  bound_tile(t, ti, tj);
  const int i = (ti << 4) + (lane >> 4) + 4 * r, j = (tj << 4) + (lane & 15);
  if (i < M && j < M) {
    o[(int64_t)i * M + j] = sum;
    if (ti != tj) o[(int64_t)j * M + i] = sum;
  }
}

}  // namespace lvae
