// cond_state.hpp -- the state of a conditioned prior term: the closed form
//   f(m, l) = c + 1/2 ( m^T A m - 2 r^T m + sum_i a_i e^{l_i} - sum_i l_i )
// per latent dim in the free rows' mean m and log-variance l.  lvae_dubo_cond_prepare_f64 (dubo_cond.hip) and
// lvae_kl_cond_prepare_f64 (kl_cond.hip) fill it, lvae_dubo_cond_eval_f64 evaluates it; lvae_dubo_cond_state_size
// is its size.  The layout depends on L and Nn = Pn T alone.
#pragma once
#include "common.hpp"

namespace lvae {

struct CondState {
  double *c, *r, *a, *A;   // [L], [L,Nn], [L,Nn], [L,Nn,Nn]
  int32_t* mask;           // [Nn]: 1 on the valid rows
  size_t bytes;
  CondState(char* base, int L, int Pn, int T) {
    WsCarve w(base);
    const size_t Nn = (size_t)Pn * T;
    c = w.take(L);
    r = w.take(L * Nn);
    a = w.take(L * Nn);
    A = w.take(L * Nn * Nn);
    mask = (int32_t*)w.take((Nn + 1) / 2);
    bytes = w.off;
  }
};

}  // namespace lvae
