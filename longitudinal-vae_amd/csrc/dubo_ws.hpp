// dubo_ws.hpp -- the workspace of the all-dims DUBO (lvae_dubo_workspace_size), shared by dubo.hip and
// dubo_cond.hip, which reads what the forward leaves in it.
#pragma once
#include "gp_bound.hpp"

namespace lvae {

constexpr int kDuboScal = 8;   // scalar slots per dim: m.iB.m, diag(iB).v, iB.K0, sum logv, sum log|B_p|

// doubles of one (dim, group) partial: Q and R lower tiles in accumulator order, p [128], the scalars
inline int64_t dubo_part_stride(int M) { return (int64_t)2 * bound_tiles(M) * 256 + 128 + kDuboScal; }

// (a null d: all zero, which bound_check answers with -3)
inline BoundDims dubo_dims(const lvae_dubo_dims* d) {
  return d ? BoundDims{d->L, d->M, d->P, d->T, d->Q} : BoundDims{};
}

// (iWR and iKQ are unused since the backward forms iW R iW and iK Q iK from N x M factors; they keep their places
// so that lvae_dubo_workspace_size stays what it was)
struct DWs {
  double *X, *iBK, *U, *UR, *F, *Z, *tNM, *dX;                                    // [L,N,M]
  double *Kz, *iK, *Q, *R, *W, *iW0, *E, *iW, *iWR, *iWRiW, *iKQ, *iKQiK, *dKz;  // [L,M,M]
  double *K0st, *Bst, *iB, *VB, *iBDiB, *K0iB, *iBK0iB, *GB, *GK0;               // [L,P,T,T]
  double *p, *w;                                                                  // [L,M]
  double *s, *y, *a;                                                              // [L,N]
  double *ldK, *ldB, *ldW, *epsv, *scal, *part, *gpart;
  int32_t* info;
  size_t bytes;
  DWs(char* base, const lvae_dubo_dims& d) {
    WsCarve c(base);
    const size_t L = d.L, M = d.M, N = (size_t)d.P * d.T, TT = (size_t)d.P * d.T * d.T;
    double** nm[] = {&X, &iBK, &U, &UR, &F, &Z, &tNM, &dX};
    for (auto q : nm) *q = c.take(L * N * M);
    double** mm[] = {&Kz, &iK, &Q, &R, &W, &iW0, &E, &iW, &iWR, &iWRiW, &iKQ, &iKQiK, &dKz};
    for (auto q : mm) *q = c.take(L * M * M);
    double** tt[] = {&K0st, &Bst, &iB, &VB, &iBDiB, &K0iB, &iBK0iB, &GB, &GK0};
    for (auto q : tt) *q = c.take(L * TT);
    p = c.take(L * M);
    w = c.take(L * M);
    s = c.take(L * N);
    y = c.take(L * N);
    a = c.take(L * N);
    ldK = c.take(L);
    ldB = c.take(L * d.P);
    ldW = c.take(L);
    epsv = c.take(L);
    scal = c.take(L * kDuboScal);
    part = c.take(L * (size_t)bound_groups(d.P) * (size_t)dubo_part_stride(d.M));
    info = (int32_t*)c.take(L * (2 + (size_t)d.P));
    gpart = c.take(bound_gram_part_doubles(dubo_dims(&d)));
    bytes = c.off;
  }
};

}  // namespace lvae
