// gram.hip -- additive-kernel Gram assembly and its adjoint (GP_model.py:31-144; kernel_gen.py:9-310).
//
// Forward: one 256-thread workgroup per 64x64 output tile of one (batch, latent-dim) slice; the two
// covariate row blocks are staged in LDS (coalesced fp64 reads of the [n, Q] index arrays), each
// thread produces 16 elements of one column (consecutive lanes -> consecutive columns, so the
// stores are coalesced).  The Gram is HBM-write-bound: per element 4 B (f32) / 8 B (f64) out.
#include "gram.hpp"
#include "gram_tile.hpp"

namespace lvae {

// The RBF / periodic factor of an integer distance m < kGTab, evaluated once per workgroup into an LDS
// table with kernel_eval's own expression (so a table read equals the direct evaluation bit for bit): the
// covariates of the reference's data (time points, ages) are integer-coded, and the Hensman Grams are
// small tiles where the exp / sin per element and component dominated.
constexpr int kGTab = 64;
template <int MC, int MF, typename T>
__device__ inline T factor_at(const DevSpec& s, int r, int f, const T* __restrict__ p, T ad) {
  const T ell = p[s.param_idx[r][f]];
  if (s.kind[r][f] == LVAE_RBF) return exp(-(ad * ad) / (T(2) * ell * ell));
  const T per = p[s.param_idx[r][f] + 1];
  const T sn = sin(T(M_PI) * ad / per);
  return exp(T(-2) * sn * sn / (ell * ell));
}

template <int MC, int MF, typename T>
__device__ inline T kernel_eval_tab(const DevSpec& s, const double* __restrict__ xi, const double* __restrict__ xj,
                                    const T* __restrict__ p, const T* __restrict__ tab) {
  T sum = T(0);
#pragma unroll
  for (int r = 0; r < MC; ++r) {
    if (r < s.n_comp) {
      T prod = p[s.scale_idx[r]];
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        if (f < s.n_fac[r]) {
          const int d = s.dim[r][f];
          const double a = xi[d], b = xj[d];
          const int k = s.kind[r][f];
          if (k == LVAE_CAT) {
            prod = (a - b == 0.0) ? prod : T(0);
          } else if (k == LVAE_BIN) {
            prod = (a + b == 2.0) ? prod : T(0);
          } else if (k == LVAE_RBF || k == LVAE_PER) {
            const double ad = fabs(a - b);
            prod *= (ad < (double)kGTab && ad == floor(ad)) ? tab[(r * MF + f) * kGTab + (int)ad]
                                                            : factor_at<MC, MF, T>(s, r, f, p, T(ad));
          } else {
            prod *= T(a * b);  // LVAE_LIN
          }
        }
      }
      sum += prod;
    }
  }
  return sum;
}

// one 64 x 64 output block (bx, by) of Gram bz = b * L + l
template <int MC, int MF, typename T>
__device__ __attribute__((always_inline)) inline void gram_block(const DevSpec& s, const lvae_xview& x1,
                                                                 const lvae_xview& x2, int L, int n1, int n2, int qs,
                                                                 const double* __restrict__ params,
                                                                 const double* __restrict__ diag, T* __restrict__ out,
                                                                 int64_t osb, int64_t osl, int64_t ldo, int bx, int by,
                                                                 int bz) {
  __shared__ double sx1[kGT * kMaxQ];
  __shared__ double sx2[kGT * kMaxQ];
  __shared__ T sp[64];
  __shared__ T tab[MC * MF * kGTab];
  const int bl = bz, b = bl / L, l = bl % L;
  const int i0 = by * kGT, j0 = bx * kGT;
  const int tid = threadIdx.x;
  if (tid < s.n_params) sp[tid] = T(params[(int64_t)l * s.n_params + tid]);
  __syncthreads();
  for (int e = tid; e < MC * MF * kGTab; e += 256) {
    const int r = e / (MF * kGTab), f = (e / kGTab) % MF, m = e % kGTab;
    T v = T(0);
    if (r < s.n_comp && f < s.n_fac[r] && (s.kind[r][f] == LVAE_RBF || s.kind[r][f] == LVAE_PER))
      v = factor_at<MC, MF, T>(s, r, f, sp, T(m));
    tab[e] = v;
  }
  const double* p1 = x1.ptr + b * x1.stride_b + l * x1.stride_l;
  const double* p2 = x2.ptr + b * x2.stride_b + l * x2.stride_l;
  for (int e = tid; e < kGT * qs; e += 256) {
    const int r = e / qs, q = e % qs;
    sx1[r * kMaxQ + q] = (i0 + r < n1) ? p1[(int64_t)(i0 + r) * x1.ld + q] : 0.0;
    sx2[r * kMaxQ + q] = (j0 + r < n2) ? p2[(int64_t)(j0 + r) * x2.ld + q] : 0.0;
  }
  __syncthreads();
  const int jj = tid & 63, j = j0 + jj;
  if (j >= n2) return;
  const T dg = diag ? T(diag[l]) : T(0);
  T* o = out + b * osb + l * osl;
#pragma unroll 4
  for (int k = 0; k < kGT / 4; ++k) {
    const int ii = (tid >> 6) + 4 * k, i = i0 + ii;
    if (i >= n1) continue;
    T v = kernel_eval_tab<MC, MF, T>(s, &sx1[ii * kMaxQ], &sx2[jj * kMaxQ], sp, tab);
    if (i == j) v += dg;
    o[(int64_t)i * ldo + j] = v;
  }
}

template <int MC, int MF, typename T>
__global__ __launch_bounds__(256) void gram_kernel(DevSpec s, lvae_xview x1, lvae_xview x2, int L, int n1, int n2,
                                                   int qs, const double* __restrict__ params,
                                                   const double* __restrict__ diag, T* __restrict__ out,
                                                   int64_t osb, int64_t osl, int64_t ldo) {
  gram_block<MC, MF, T>(s, x1, x2, L, n1, n2, qs, params, diag, out, osb, osl, ldo, blockIdx.x, blockIdx.y,
                        blockIdx.z);
}

// several fp64 Grams in one launch (the Hensman forward's four: K0xz, K0zz, K0_p with spec0, B_p with
// spec1): a 1-D grid over every job's blocks, block r of job q at (r % gx, r / gx % gy, r / (gx gy))
constexpr int kGFMaxJobs = 4;
struct GramFwdJobs {
  DevSpec s[2];
  int qs[2];
  GramFwdJob j[kGFMaxJobs];
  int njobs;
};

template <int MC, int MF>
__global__ __launch_bounds__(256) void gram_multi_kernel(GramFwdJobs J, int L) {
  int q = 0;
  while (q + 1 < J.njobs && (int)blockIdx.x >= J.j[q + 1].blk0) ++q;  // (uniform)
  const GramFwdJob& jb = J.j[q];
  const int r = blockIdx.x - jb.blk0;
  gram_block<MC, MF, double>(J.s[jb.spec], jb.x1, jb.x2, L, jb.n1, jb.n2, J.qs[jb.spec], jb.params, jb.diag, jb.out,
                             jb.osb, jb.osl, jb.ldo, r % jb.gx, (r / jb.gx) % jb.gy, r / (jb.gx * jb.gy));
}

// Adjoint, generic strided G (fp64), several Grams in one launch (the Hensman backward contracts
// four: K0xz, K0zz, K0_p with spec0 and B_p with spec1).  Stage 1: grid (chunks over all jobs, L),
// each workgroup takes kGBChunk consecutive elements of one job's [nb, n1, n2] G, accumulates the
// per-slot sums of g dk/dparam in registers, reduces them over its waves, and writes one partial
// row part[l][chunk][slot] (slot NS-1: sum of the diagonal of G, the noise adjoint).  Stage 2: one
// workgroup per latent dim sums the chunks of every (job, slot) and adds them to the job's dparams /
// ddiag in a fixed order -- deterministic, and no single-workgroup loop over the whole Gram.
constexpr int kGBMaxJobs = 4;
constexpr int kGBChunk = 1024;  // elements per workgroup (4 per thread)

struct GramBwdJobs {
  DevSpec s[2];
  GramBwdJob j[kGBMaxJobs];
  int njobs, total_chunks;
};

// kernel_grad_acc with the factors of integer distances m < kGTab read from per-workgroup tables of phi(m),
// and for periodic factors sin(u) and sin(2u) (u = pi m / p), each with kernel_grad_acc's own expression:
// bit-identical to it, without the exp / sin per element and component
template <int MC, int MF>
__device__ inline void kernel_grad_acc_tab(const DevSpec& s, const double* __restrict__ xi,
                                           const double* __restrict__ xj, const double* __restrict__ p, double g,
                                           double (&acc_s)[MC], double (&acc_f)[MC][MF][2],
                                           const double* __restrict__ tphi, const double* __restrict__ tsn,
                                           const double* __restrict__ ts2) {
#pragma unroll
  for (int r = 0; r < MC; ++r) {
    if (r < s.n_comp) {
      double prod = 1.0;
      double dlog[MF][2];
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        dlog[f][0] = 0.0;
        dlog[f][1] = 0.0;
        if (f >= s.n_fac[r]) continue;
        const int d = s.dim[r][f];
        const double a = xi[d], b = xj[d];
        const int k = s.kind[r][f];
        if (k == LVAE_CAT) {
          prod = (a - b == 0.0) ? prod : 0.0;
        } else if (k == LVAE_BIN) {
          prod = (a + b == 2.0) ? prod : 0.0;
        } else if (k == LVAE_RBF || k == LVAE_PER) {
          const double ad = fabs(a - b);
          const bool hit = ad < (double)kGTab && ad == floor(ad);
          const int ti = (r * MF + f) * kGTab + (hit ? (int)ad : 0);
          const double ell = p[s.param_idx[r][f]];
          if (k == LVAE_RBF) {
            const double diff = a - b, d2 = diff * diff;
            prod *= hit ? tphi[ti] : exp(-d2 / (2.0 * ell * ell));
            dlog[f][0] = d2 / (ell * ell * ell);
          } else {
            const double per = p[s.param_idx[r][f] + 1];
            const double u = M_PI * ad / per;
            const double sn = hit ? tsn[ti] : sin(u);
            prod *= hit ? tphi[ti] : exp(-2.0 * sn * sn / (ell * ell));
            dlog[f][0] = 4.0 * sn * sn / (ell * ell * ell);
            dlog[f][1] = 2.0 * M_PI * ad * (hit ? ts2[ti] : sin(2.0 * u)) / (ell * ell * per * per);
          }
        } else {
          prod *= a * b;  // LVAE_LIN
        }
      }
      const double gp = g * prod;
      acc_s[r] += gp;
      const double gc = gp * p[s.scale_idx[r]];
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        acc_f[r][f][0] += gc * dlog[f][0];
        acc_f[r][f][1] += gc * dlog[f][1];
      }
    }
  }
}

template <int MC, int MF>
__global__ __launch_bounds__(256) void gram_bwd_part_kernel(GramBwdJobs J, int L, double* __restrict__ part) {
  constexpr int NS = MC + MC * MF * 2 + 1;
  constexpr bool kTab = MC * MF <= 16;  // (the tables: 3 x 8 KB at the small bucket)
  constexpr int NT = kTab ? MC * MF * kGTab : 1;
  __shared__ double sp[64];
  __shared__ double wred[4][NS];
  __shared__ double tphi[NT], tsn[NT], ts2[NT];
  const int c = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
  int jb = 0;
  while (jb + 1 < J.njobs && c >= J.j[jb + 1].chunk0) ++jb;
  const GramBwdJob& job = J.j[jb];
  const DevSpec& s = J.s[job.spec];
  if (tid < job.n_params) sp[tid] = job.params[(int64_t)l * job.n_params + tid];
  __syncthreads();
  if (kTab) {
    for (int e = tid; e < NT; e += 256) {
      const int r = e / (MF * kGTab), f = (e / kGTab) % MF, m = e % kGTab;
      double phi = 0.0, sn = 0.0, s2 = 0.0;
      if (r < s.n_comp && f < s.n_fac[r]) {
        const double ad = (double)m;   // (the parameters are read per kind: a gate or a linear factor has index -1)
        if (s.kind[r][f] == LVAE_RBF) {
          const double ell = sp[s.param_idx[r][f]];
          phi = exp(-(ad * ad) / (2.0 * ell * ell));
        } else if (s.kind[r][f] == LVAE_PER) {
          const double ell = sp[s.param_idx[r][f]];
          const double per = sp[s.param_idx[r][f] + 1], u = M_PI * ad / per;
          sn = sin(u);
          phi = exp(-2.0 * sn * sn / (ell * ell));
          s2 = sin(2.0 * u);
        }
      }
      tphi[e] = phi;
      tsn[e] = sn;
      ts2[e] = s2;
    }
    __syncthreads();
  }
  double acc_s[MC];
  double acc_f[MC][MF][2];
#pragma unroll
  for (int r = 0; r < MC; ++r) {
    acc_s[r] = 0.0;
#pragma unroll
    for (int f = 0; f < MF; ++f) acc_f[r][f][0] = acc_f[r][f][1] = 0.0;
  }
  double dd = 0.0;
  const int64_t per_b = (int64_t)job.n1 * job.n2, total = per_b * job.nb;
  const int64_t e0 = (int64_t)(c - job.chunk0) * kGBChunk;
  for (int64_t e = e0 + tid; e < e0 + kGBChunk && e < total; e += 256) {
    const int b = (int)(e / per_b);
    const int64_t rem = e - b * per_b;
    const int i = (int)(rem / job.n2), j = (int)(rem - (int64_t)i * job.n2);
    const double g = job.G[b * job.gsb + l * job.gsl + i * job.ldg + j];
    if (g == 0.0) continue;
    const double* xi = job.x1.ptr + b * job.x1.stride_b + l * job.x1.stride_l + i * job.x1.ld;
    const double* xj = job.x2.ptr + b * job.x2.stride_b + l * job.x2.stride_l + j * job.x2.ld;
    if (kTab)
      kernel_grad_acc_tab<MC, MF>(s, xi, xj, sp, g, acc_s, acc_f, tphi, tsn, ts2);
    else
      kernel_grad_acc<MC, MF, double, double>(s, xi, xj, sp, g, acc_s, acc_f);
    if (i == j) dd += g;
  }
  const int w = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int r = 0; r < MC; ++r) {
    const double v = wave_sum(acc_s[r]);
    if (lane == 0) wred[w][r] = v;
#pragma unroll
    for (int f = 0; f < MF; ++f)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const double u = wave_sum(acc_f[r][f][q]);
        if (lane == 0) wred[w][MC + (r * MF + f) * 2 + q] = u;
      }
  }
  {
    const double v = wave_sum(dd);
    if (lane == 0) wred[w][NS - 1] = v;
  }
  __syncthreads();
  double* out = part + ((int64_t)l * J.total_chunks + c) * NS;
  for (int sl = tid; sl < NS; sl += 256) out[sl] = wred[0][sl] + wred[1][sl] + wred[2][sl] + wred[3][sl];
}

template <int MC, int MF>
__global__ __launch_bounds__(256) void gram_bwd_sum_kernel(GramBwdJobs J, const double* __restrict__ part) {
  constexpr int NS = MC + MC * MF * 2 + 1;
  __shared__ double red[kGBMaxJobs][NS];
  const int l = blockIdx.x, tid = threadIdx.x;
  for (int t = tid; t < J.njobs * NS; t += 256) {
    const int jb = t / NS, sl = t % NS;
    const GramBwdJob& job = J.j[jb];
    double v = 0.0;
    for (int c = job.chunk0; c < job.chunk0 + job.nchunks; ++c) v += part[((int64_t)l * J.total_chunks + c) * NS + sl];
    red[jb][sl] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int jb = 0; jb < J.njobs; ++jb) {
    const GramBwdJob& job = J.j[jb];
    const DevSpec& s = J.s[job.spec];
    for (int sl = 0; sl < NS - 1; ++sl) {
      const int pi = slot_param<MC, MF>(s, sl);
      if (pi >= 0) job.dparams[(int64_t)l * job.n_params + pi] += red[jb][sl];
    }
    if (job.ddiag) job.ddiag[l] += red[jb][NS - 1];
  }
}

// Input adjoint: dx2[b,l,j,q] = sum_i G[b,l,i,j] d k_l(x1_i, x2_j) / d x2_{j,q}, up to kGXMaxJobs Grams that share
// one x2 shape summed into one dx2 (the bounds' z-adjoint: k0(x, z) against dX, k0(z, z) against dKz and dKz^T).
// Stage 1: one workgroup per (kGXRows rows, kGT columns) block of one (b, l) slice; lane = column, so G is read
// coalesced along j when gsj == 1, and the wave's row of x1 is an LDS broadcast.  Wave w takes rows w, w + 4, ..
// of the block; a thread keeps one accumulator per (component, factor) in registers (compile-time indexed), and
// the four waves then add theirs into the block's [column][covariate] LDS image one after the other, each thread
// in (component, factor) order on its own row: a fixed order, no atomics.  The image goes to
// part[job][b l][row chunk][j][q].  Stage 2: dx2[b,l,j,q] = the jobs' chunks added in (job, chunk) order; columns
// no differentiable factor reads (and columns q >= kMaxQ) get exact zeros.
constexpr int kGXMaxJobs = 3;
constexpr int kGXRows = 64;

struct GramX2Jobs {
  DevSpec s;
  GramX2Job j[kGXMaxJobs];
  int njobs, qs, qp;  // qs: columns staged (1 + the largest the spec reads); qp = min(Q, kMaxQ): partial row length
};

// acc[r][f] += g s_r (d phi_rf / d b) prod_{f' != f} phi_rf'  (b = xj[dim]: the second operand's column)
template <int MC, int MF>
__device__ __attribute__((always_inline)) inline void kernel_dx2_acc(const DevSpec& s, const double* __restrict__ xi,
                                                                     const double* __restrict__ xj,
                                                                     const double* __restrict__ p, double g,
                                                                     double (&acc)[MC][MF]) {
#pragma unroll
  for (int r = 0; r < MC; ++r) {
    if (r < s.n_comp) {
      double phi[MF], dphi[MF];
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        phi[f] = 1.0;
        dphi[f] = 0.0;
        if (f >= s.n_fac[r]) continue;
        const int d = s.dim[r][f];
        const double a = xi[d], b = xj[d];
        const int k = s.kind[r][f];
        if (k == LVAE_CAT) {
          phi[f] = (a - b == 0.0) ? 1.0 : 0.0;
        } else if (k == LVAE_BIN) {
          phi[f] = (a + b == 2.0) ? 1.0 : 0.0;
        } else if (k == LVAE_RBF) {
          const double diff = a - b, ell = p[s.param_idx[r][f]];
          phi[f] = exp(-(diff * diff) / (2.0 * ell * ell));
          dphi[f] = phi[f] * diff / (ell * ell);
        } else if (k == LVAE_PER) {
          const double diff = a - b, ell = p[s.param_idx[r][f]], per = p[s.param_idx[r][f] + 1];
          const double sn = sin(M_PI * fabs(diff) / per);
          phi[f] = exp(-2.0 * sn * sn / (ell * ell));
          dphi[f] = phi[f] * (2.0 * M_PI / (per * ell * ell)) * sin(2.0 * M_PI * diff / per);
        } else {  // LVAE_LIN
          phi[f] = a * b;
          dphi[f] = a;
        }
      }
      const double gs = g * p[s.scale_idx[r]];
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        double o = gs * dphi[f];
#pragma unroll
        for (int f2 = 0; f2 < MF; ++f2)
          if (f2 != f) o *= phi[f2];
        acc[r][f] += o;
      }
    }
  }
}

template <int MC, int MF>
__global__ __launch_bounds__(256) void gram_bwd_x2_part_kernel(GramX2Jobs J, int L, const double* __restrict__ params,
                                                               double* __restrict__ part) {
  constexpr int LD = kMaxQ + 1;  // (odd row stride: a wave's 64 rows fall on distinct banks)
  __shared__ double sx1[kGXRows * kMaxQ];
  __shared__ double sx2[kGT * LD];
  __shared__ double sdx[kGT * LD];
  __shared__ double sp[64];
  int q = 0;
  while (q + 1 < J.njobs && (int)blockIdx.x >= J.j[q + 1].blk0) ++q;  // (uniform)
  const GramX2Job& jb = J.j[q];
  const DevSpec& s = J.s;
  const int rb = blockIdx.x - jb.blk0;
  const int ct = rb % jb.nct, rc = (rb / jb.nct) % jb.nrc, bl = rb / (jb.nct * jb.nrc), b = bl / L, l = bl % L;
  const int i0 = rc * kGXRows, j0 = ct * kGT, tid = threadIdx.x, qs = J.qs, qp = J.qp;
  if (tid < s.n_params) sp[tid] = params[(int64_t)l * s.n_params + tid];
  const double* p1 = jb.x1.ptr + b * jb.x1.stride_b + l * jb.x1.stride_l;
  const double* p2 = jb.x2.ptr + b * jb.x2.stride_b + l * jb.x2.stride_l;
  for (int e = tid; e < kGT * qs; e += 256) {
    const int r = e / qs, c = e % qs;
    sx1[r * kMaxQ + c] = (i0 + r < jb.n1) ? p1[(int64_t)(i0 + r) * jb.x1.ld + c] : 0.0;
    sx2[r * LD + c] = (j0 + r < jb.n2) ? p2[(int64_t)(j0 + r) * jb.x2.ld + c] : 0.0;
  }
  for (int e = tid; e < kGT * LD; e += 256) sdx[e] = 0.0;
  __syncthreads();
  const int w = tid >> 6, jj = tid & 63, j = j0 + jj;
  double acc[MC][MF];
#pragma unroll
  for (int r = 0; r < MC; ++r)
#pragma unroll
    for (int f = 0; f < MF; ++f) acc[r][f] = 0.0;
  if (j < jb.n2) {
    const double* g = jb.G + b * jb.gsb + l * jb.gsl + (int64_t)j * jb.gsj;
    for (int ii = w; ii < kGXRows && i0 + ii < jb.n1; ii += 4) {
      const double gv = g[(int64_t)(i0 + ii) * jb.gsi];
      if (gv == 0.0) continue;  // (the Hensman bound's padding rows: dK0xz is exactly zero there)
      kernel_dx2_acc<MC, MF>(s, &sx1[ii * kMaxQ], &sx2[jj * LD], sp, gv, acc);
    }
  }
  for (int ww = 0; ww < 4; ++ww) {
    if (w == ww && j < jb.n2) {
#pragma unroll
      for (int r = 0; r < MC; ++r)
#pragma unroll
        for (int f = 0; f < MF; ++f)
          if (r < s.n_comp && f < s.n_fac[r] && s.kind[r][f] >= LVAE_RBF) sdx[jj * LD + s.dim[r][f]] += acc[r][f];
    }
    __syncthreads();
  }
  double* out = part + jb.part0 + ((int64_t)(bl * jb.nrc + rc) * jb.n2 + j0) * qp;
  for (int e = tid; e < kGT * qp; e += 256) {
    const int r = e / qp, c = e % qp;
    if (j0 + r < jb.n2) out[e] = sdx[r * LD + c];
  }
}

__global__ __launch_bounds__(256) void gram_bwd_x2_sum_kernel(GramX2Jobs J, int64_t total, int n2, int Q,
                                                              const double* __restrict__ part,
                                                              double* __restrict__ dx2) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int q = (int)(e % Q), j = (int)((e / Q) % n2);
  const int64_t bl = e / ((int64_t)Q * n2);
  double v = 0.0;
  if (q < J.qp) {
    for (int k = 0; k < J.njobs; ++k) {
      const GramX2Job& jb = J.j[k];
      for (int rc = 0; rc < jb.nrc; ++rc) v += part[jb.part0 + ((bl * jb.nrc + rc) * jb.n2 + j) * J.qp + q];
    }
  }
  dx2[e] = v;
}

// host launchers
template <typename T>
static int gram_launch(const lvae_kernel_spec* spec, lvae_xview x1, lvae_xview x2, int nb, int L, int n1, int n2,
                       const double* params, const double* diag, T* out, int64_t osb, int64_t osl, int64_t ldo,
                       void* stream) {
  const int bucket = spec_bucket(spec);
  if (!bucket) return -1;
  const int qs = spec_qs(spec);
  if (qs > kMaxQ) return -1;
  if (nb < 1 || L < 1 || n1 < 0 || n2 < 0) return -4;
  if (n1 == 0 || n2 == 0) return 0;
  const DevSpec ds = to_dev(spec);
  dim3 grid(cdiv(n2, kGT), cdiv(n1, kGT), nb * L), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (bucket == 1)
    gram_kernel<8, 2, T><<<grid, block, 0, st>>>(ds, x1, x2, L, n1, n2, qs, params, diag, out, osb, osl, ldo);
  else
    gram_kernel<16, 4, T><<<grid, block, 0, st>>>(ds, x1, x2, L, n1, n2, qs, params, diag, out, osb, osl, ldo);
  LVAE_CHECK_LAUNCH();
  return 0;
}

// host: up to kGFMaxJobs fp64 Grams (descriptors as lvae_gram_f64's arguments; spec index into specs[0..1])
int gram_multi_f64(const lvae_kernel_spec* const* specs, const GramFwdJob* jobs, int njobs, int L, hipStream_t st) {
  if (njobs < 1 || njobs > kGFMaxJobs || L < 1) return -4;
  GramFwdJobs J{};
  int bucket = 0, blocks = 0;
  for (int k = 0; k < 2; ++k) {
    if (!specs[k]) continue;
    const int bk = spec_bucket(specs[k]);
    if (!bk || spec_qs(specs[k]) > kMaxQ) return -1;
    bucket = bk > bucket ? bk : bucket;
    J.s[k] = to_dev(specs[k]);
    J.qs[k] = spec_qs(specs[k]);
  }
  J.njobs = 0;
  for (int q = 0; q < njobs; ++q) {
    GramFwdJob jb = jobs[q];
    if (jb.spec < 0 || jb.spec > 1 || !specs[jb.spec]) return -1;
    if (jb.nb < 1 || jb.n1 < 0 || jb.n2 < 0) return -4;
    if (jb.n1 == 0 || jb.n2 == 0) continue;
    jb.gx = cdiv(jb.n2, kGT), jb.gy = cdiv(jb.n1, kGT), jb.blk0 = blocks;
    blocks += jb.gx * jb.gy * jb.nb * L;
    J.j[J.njobs++] = jb;
  }
  if (J.njobs == 0) return 0;
  if (bucket == 1)
    gram_multi_kernel<8, 2><<<blocks, 256, 0, st>>>(J, L);
  else
    gram_multi_kernel<16, 4><<<blocks, 256, 0, st>>>(J, L);
  LVAE_CHECK_LAUNCH();
  return 0;
}

// Adjoints of up to kGBMaxJobs Grams in two launches (see gram_bwd_part_kernel); `jobs` hold
// host-side descriptors whose .spec indexes specs[0..1].  part: gram_bwd_part_bytes(...) bytes.
size_t gram_bwd_part_bytes(const GramBwdJob* jobs, int njobs, int L) {
  int64_t chunks = 0;
  for (int q = 0; q < njobs; ++q) chunks += cdiv((int64_t)jobs[q].nb * jobs[q].n1 * jobs[q].n2, kGBChunk);
  return (size_t)L * (size_t)(chunks > 0 ? chunks : 1) * (16 + 16 * 4 * 2 + 1) * sizeof(double);
}

int gram_bwd_multi_f64(const lvae_kernel_spec* const* specs, const GramBwdJob* jobs, int njobs, int L, double* part,
                       hipStream_t st) {
  if (njobs < 1 || njobs > kGBMaxJobs || L < 1) return -4;
  GramBwdJobs J;
  int bucket = 1;
  for (int q = 0; q < 2; ++q) {
    if (!specs[q]) {
      J.s[q] = J.s[0];
      continue;
    }
    const int bk = spec_bucket(specs[q]);
    if (!bk) return -1;
    bucket = bk > bucket ? bk : bucket;
    J.s[q] = to_dev(specs[q]);
  }
  int chunks = 0;
  for (int q = 0; q < njobs; ++q) {
    J.j[q] = jobs[q];
    J.j[q].n_params = specs[jobs[q].spec]->n_params;
    J.j[q].chunk0 = chunks;
    J.j[q].nchunks = cdiv((int64_t)jobs[q].nb * jobs[q].n1 * jobs[q].n2, kGBChunk);
    chunks += J.j[q].nchunks;
  }
  J.njobs = njobs;
  J.total_chunks = chunks;
  if (chunks == 0) return 0;
  if (bucket == 1) {
    gram_bwd_part_kernel<8, 2><<<dim3(chunks, L), 256, 0, st>>>(J, L, part);
    gram_bwd_sum_kernel<8, 2><<<L, 256, 0, st>>>(J, part);
  } else {
    gram_bwd_part_kernel<16, 4><<<dim3(chunks, L), 256, 0, st>>>(J, L, part);
    gram_bwd_sum_kernel<16, 4><<<L, 256, 0, st>>>(J, part);
  }
  LVAE_CHECK_LAUNCH();
  return 0;
}

// Input adjoints of up to kGXMaxJobs Grams with one x2 shape [nb, L, n2, Q], summed into dx2 in two launches (see
// gram_bwd_x2_part_kernel).  part: gram_bwd_x2_part_bytes(...) bytes.
static_assert(kGXRows == kGT, "gram_bwd_x2_part_kernel stages both row blocks in one loop");

size_t gram_bwd_x2_part_bytes(const GramX2Job* jobs, int njobs, int L, int Q) {
  const size_t qp = Q < kMaxQ ? Q : kMaxQ;
  size_t n = 0;
  for (int q = 0; q < njobs; ++q)
    n += (size_t)jobs[q].nb * L * cdiv(jobs[q].n1, kGXRows) * jobs[q].n2 * qp;
  return align256((n > 0 ? n : 1) * sizeof(double));
}

int gram_bwd_x2_multi_f64(const lvae_kernel_spec* spec, const GramX2Job* jobs, int njobs, int L, int Q,
                          const double* params, double* dx2, double* part, hipStream_t st) {
  if (njobs < 1 || njobs > kGXMaxJobs || L < 1 || Q < 1) return -4;
  const int bucket = spec ? spec_bucket(spec) : 0;
  if (!bucket || spec_qs(spec) > kMaxQ || spec_qs(spec) > Q) return -1;
  GramX2Jobs J;
  J.s = to_dev(spec);
  J.njobs = njobs;
  J.qs = spec_qs(spec);
  J.qp = Q < kMaxQ ? Q : kMaxQ;
  const int nb = jobs[0].nb, n2 = jobs[0].n2;
  int64_t blocks = 0, off = 0;
  for (int q = 0; q < njobs; ++q) {
    GramX2Job jb = jobs[q];
    if (jb.nb != nb || jb.n2 != n2 || jb.nb < 1 || jb.n1 < 0 || jb.n2 < 0) return -4;
    jb.nrc = cdiv(jb.n1, kGXRows), jb.nct = cdiv(jb.n2, kGT);
    jb.blk0 = (int)blocks, jb.part0 = off;
    blocks += (int64_t)jb.nrc * jb.nct * nb * L;
    off += (int64_t)nb * L * jb.nrc * n2 * J.qp;
    if (blocks > INT32_MAX) return -4;
    J.j[q] = jb;
  }
  if (n2 == 0) return 0;
  if (blocks > 0) {
    if (bucket == 1)
      gram_bwd_x2_part_kernel<8, 2><<<(unsigned)blocks, 256, 0, st>>>(J, L, params, part);
    else
      gram_bwd_x2_part_kernel<16, 4><<<(unsigned)blocks, 256, 0, st>>>(J, L, params, part);
  }
  const int64_t total = (int64_t)nb * L * n2 * Q;
  gram_bwd_x2_sum_kernel<<<cdiv(total, 256), 256, 0, st>>>(J, total, n2, Q, part, dx2);
  LVAE_CHECK_LAUNCH();
  return 0;
}

}  // namespace lvae

extern "C" {

int lvae_gram_f64(const lvae_kernel_spec* spec, lvae_xview x1, lvae_xview x2, int nb, int L, int n1, int n2,
                  const double* params, const double* diag, double* out, int64_t osb, int64_t osl, int64_t ldo,
                  void* stream) {
  return lvae::gram_launch<double>(spec, x1, x2, nb, L, n1, n2, params, diag, out, osb, osl, ldo, stream);
}

int lvae_gram_f32(const lvae_kernel_spec* spec, lvae_xview x1, lvae_xview x2, int nb, int L, int n1, int n2,
                  const double* params, const double* diag, float* out, int64_t osb, int64_t osl, int64_t ldo,
                  void* stream) {
  return lvae::gram_launch<float>(spec, x1, x2, nb, L, n1, n2, params, diag, out, osb, osl, ldo, stream);
}

size_t lvae_gram_bwd_workspace_size(int nb, int L, int n1, int n2) {
  lvae::GramBwdJob j{};
  j.nb = nb, j.n1 = n1, j.n2 = n2;
  return lvae::gram_bwd_part_bytes(&j, 1, L);
}

int lvae_gram_bwd_f64(const lvae_kernel_spec* spec, lvae_xview x1, lvae_xview x2, int nb, int L, int n1, int n2,
                      const double* params, const double* G, int64_t gsb, int64_t gsl, int64_t ldg, double* dparams,
                      double* ddiag, void* workspace, void* stream) {
  // (the forward's limits: a spec no template bucket holds, a factor on a covariate column >= kMaxQ)
  if (!spec || !lvae::spec_bucket(spec) || lvae::spec_qs(spec) > lvae::kMaxQ) return -1;
  if (nb < 1 || L < 1 || n1 < 0 || n2 < 0) return -4;
  if (!params) return -8;
  if (!G) return -9;
  if (!dparams) return -13;
  if (!workspace) return -15;
  lvae::GramBwdJob j{};
  j.spec = 0, j.x1 = x1, j.x2 = x2, j.nb = nb, j.n1 = n1, j.n2 = n2, j.params = params, j.G = G;
  j.gsb = gsb, j.gsl = gsl, j.ldg = ldg, j.dparams = dparams, j.ddiag = ddiag;
  const lvae_kernel_spec* specs[2] = {spec, nullptr};
  return lvae::gram_bwd_multi_f64(specs, &j, 1, L, (double*)workspace, (hipStream_t)stream);
}

size_t lvae_gram_bwd_x2_workspace_size(int nb, int L, int n1, int n2, int Q) {
  if (nb < 1 || L < 1 || n1 < 0 || n2 < 0 || Q < 1) return 0;
  lvae::GramX2Job j{};
  j.nb = nb, j.n1 = n1, j.n2 = n2;
  return lvae::gram_bwd_x2_part_bytes(&j, 1, L, Q);
}

int lvae_gram_bwd_x2_f64(const lvae_kernel_spec* spec, lvae_xview x1, lvae_xview x2, int nb, int L, int n1, int n2,
                         int Q, const double* params, const double* G, int64_t gsb, int64_t gsl, int64_t gsi,
                         int64_t gsj, double* dx2, void* workspace, void* stream) {
  if (!spec || !lvae::spec_bucket(spec) || lvae::spec_qs(spec) > lvae::kMaxQ) return -1;
  if (nb < 1 || L < 1 || n1 < 0 || n2 < 0 || Q < lvae::spec_qs(spec) || Q < 1) return -4;
  if (!params) return -8;
  if (!G) return -9;
  if (!dx2) return -13;
  if (!workspace) return -15;
  lvae::GramX2Job j{};
  j.x1 = x1, j.x2 = x2, j.nb = nb, j.n1 = n1, j.n2 = n2, j.G = G;
  j.gsb = gsb, j.gsl = gsl, j.gsi = gsi, j.gsj = gsj;
  return lvae::gram_bwd_x2_multi_f64(spec, &j, 1, L, Q, params, dx2, (double*)workspace, (hipStream_t)stream);
}

}  // extern "C"
