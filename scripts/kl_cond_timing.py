"""Time the conditioned exact KL (condition_kl_closed) at N = 4096 training rows, L = 16 dims and Nn = 160 / 1024 new
rows (the kernel config and random hyper-parameters of scripts/dubo_cond_timing.py):
  prepare   one lvae_kl_cond_prepare_f64 on preallocated buffers, and its launch groups replayed through the public
            entries on the same shapes: (a) Gram + potrf of K_tt, (b) the cross Gram and the two triangular solves,
            (d) potrf of S and potrs on the identity; (c) the two weighted SYRKs, the product with mu_t and the
            finish are prepare - (a) - (b) - (d).  The SYRK kernel's own time comes from a
            rocprofv3 --kernel-trace --stats run of this script (kc_syrk_partial_kernel / kc_syrk_reduce_kernel).
  gemm      torch.matmul (rocBLAS dgemm, fp64) of the same [L, Nn, N] x [L, N, Nn] product, the yardstick of the SYRK
  eval      cond(m, l) forward + backward (lvae_dubo_cond_eval_f64), beside a condition_dubo state of the same Nn
            (Pn = Nn / 16 new subjects of T = 16 among 64 + Pn, M = 120)
Device events, 2 warm-up rounds, the median of 7 calls, one process.  DESIGN.md and profiles/kl_cond_timing.json hold
a run.

    python scripts/kl_cond_timing.py [out.json]
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "longitudinal-vae_amd")]
import lvae_amd as la  # noqa: E402
from lvae_amd import _lib  # noqa: E402
from lvae_amd.data import health_mnist_covariates  # noqa: E402
from lvae_amd.elbo import _stack_modules, check_pending  # noqa: E402

DEV = "cuda"
CFG = dict(cat_kernel=[2], bin_kernel=[], sqexp_kernel=[0],
           cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 2}, {'cont_covariate': 0, 'cat_covariate': 3},
                           {'cont_covariate': 1, 'cat_covariate': 4}],
           bin_int_kernel=[], covariate_missing_val=[])
N, L, T, M, EPS = 4096, 16, 16, 120, 1e-6
WARM, REPS = 2, 7


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def median_ms(routes):
    ms = {r: [] for r in routes}
    for rep in range(WARM + REPS):
        for r, fn in routes.items():
            t, _ = timed(fn)
            if rep >= WARM:
                ms[r].append(t)
    return {r: statistics.median(v) for r, v in ms.items()}


def set_raw(module, rng):
    with torch.no_grad():
        for _, p in module.named_parameters():
            p.copy_(torch.as_tensor(np.log(rng.uniform(0.5, 2.0, tuple(p.shape))), dtype=p.dtype))
            p.requires_grad_(False)


def measure(Nn, seed=43):
    lib = _lib.lib()
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    X = torch.tensor(health_mnist_covariates((N + Nn) // T, T, seed=seed)).to(DEV)   # cat(new, train)
    xn, xt = X[:Nn].contiguous(), X[Nn:].contiguous()
    mu = torch.randn(N, L, generator=gen, dtype=torch.float64).to(DEV)
    lv = (0.1 * torch.randn(N, L, generator=gen, dtype=torch.float64)).to(DEV)
    k = la.generate_kernel(**CFG, latent_dim=L).double()
    set_raw(k, rng)
    k = k.to(DEV)
    lik = la.GaussianLikelihood(L, noise=1.0).to(DEV)
    spec, params = _stack_modules(k)
    params, noise = params.detach().contiguous(), lik.noise.detach().contiguous()
    st = _lib.stream_ptr
    P = _lib.ptr
    Q = X.shape[1]
    state = torch.empty(int(lib.lvae_dubo_cond_state_size(L, Nn, 1)), dtype=torch.uint8, device=DEV)
    ws = torch.empty(int(lib.lvae_kl_cond_workspace_size(N, Nn, L)), dtype=torch.uint8, device=DEV)
    info = torch.empty(L, dtype=torch.int32, device=DEV)
    K = torch.empty(L, N, N, dtype=torch.float64, device=DEV)
    panel = torch.empty(L, N, Nn, dtype=torch.float64, device=DEV)
    S = torch.empty(L, Nn, Nn, dtype=torch.float64, device=DEV)
    eye = torch.empty(L, Nn, Nn, dtype=torch.float64, device=DEV)
    logdet = torch.empty(L, dtype=torch.float64, device=DEV)
    tws = torch.empty(int(lib.lvae_trsm_workspace_size(N, L)), dtype=torch.uint8, device=DEV)
    xv, nv = _lib.xview(xt, 0, 0), _lib.xview(xn, 0, 0)

    def ok(rc):
        assert rc == 0, rc

    def prepare():
        ok(lib.lvae_kl_cond_prepare_f64(spec, P(xt), Q, N, P(xn), Q, Nn, L, P(params), P(noise), P(mu), L, P(lv), L,
                                        P(state), L, 0, P(info), P(ws), st()))

    def gram_potrf():
        ok(lib.lvae_gram_f64(spec, xv, xv, 1, L, N, N, P(params), P(noise), P(K), 0, N * N, N, st()))
        ok(lib.lvae_potrf_f64(N, L, P(K), N, N * N, P(K), N, N * N, P(logdet), P(info), st()))

    def solves():
        ok(lib.lvae_gram_f64(spec, xv, nv, 1, L, N, Nn, P(params), None, P(panel), 0, N * Nn, Nn, st()))
        ok(lib.lvae_trsm_f64(0, N, Nn, L, P(K), N, N * N, P(panel), Nn, N * Nn, P(tws), st()))
        ok(lib.lvae_trsm_f64(1, N, Nn, L, P(K), N, N * N, P(panel), Nn, N * Nn, P(tws), st()))

    def s_inverse():
        S.copy_(S0)
        eye.copy_(I0)
        ok(lib.lvae_potrf_f64(Nn, L, P(S), Nn, Nn * Nn, P(S), Nn, Nn * Nn, P(logdet), P(info), st()))
        ok(lib.lvae_potrs_f64(Nn, Nn, L, P(S), Nn, Nn * Nn, P(eye), Nn, Nn * Nn, P(tws), st()))

    def s_copies():
        S.copy_(S0)
        eye.copy_(I0)

    prepare()
    torch.cuda.synchronize()
    assert not info.any()
    al = lambda n: (8 * n + 255) // 256 * 256                  # (cond_state.hpp: c, r, a, then A)
    off = al(L) + 2 * al(L * Nn)
    A = state[off:off + 8 * L * Nn * Nn].view(torch.float64).reshape(L, Nn, Nn)
    S0 = torch.linalg.inv(A)
    S0 = 0.5 * (S0 + S0.transpose(1, 2))
    I0 = torch.eye(Nn, dtype=torch.float64, device=DEV).expand(L, Nn, Nn).contiguous()
    gram_potrf()
    W = torch.randn(L, N, Nn, generator=gen, dtype=torch.float64).to(DEV)
    Wt = W.transpose(1, 2).contiguous()
    out = torch.empty(L, Nn, Nn, dtype=torch.float64, device=DEV)
    la.set_sync_checks(False)
    cond = la.condition_kl_closed(k, lik, xn, xt, mu, lv)
    m_new = torch.randn(Nn, L, generator=gen, dtype=torch.float64).to(DEV).requires_grad_()
    lv_new = (0.1 * torch.randn(Nn, L, generator=gen, dtype=torch.float64)).to(DEV).requires_grad_()
    # a conditioned-DUBO state of the same Nn: Pn = Nn / T new subjects among 64 + Pn
    Pn, Pj = Nn // T, 64 + Nn // T
    Xd = torch.tensor(health_mnist_covariates(Pj, T, seed=seed + 1)).to(DEV)
    k0, k1 = la.generate_kernel_batched(L, **CFG, id_covariate=2)
    set_raw(k0, rng)
    set_raw(k1, rng)
    k0, k1 = k0.to(DEV), k1.to(DEV)
    z = torch.stack([Xd[torch.linspace(0, Pj * T - 1, M).long()]] * L)
    mud = torch.randn(Pj * T, L, generator=gen, dtype=torch.float64).to(DEV)
    lvd = (0.1 * torch.randn(Pj * T, L, generator=gen, dtype=torch.float64)).to(DEV)
    dcond = la.condition_dubo(L, k0, k1, lik, Xd[:Nn], Xd[Nn:], mud[Nn:], lvd[Nn:], z, T, EPS)

    def ev(c):
        def run():
            m_new.grad, lv_new.grad = None, None
            c(m_new, lv_new).sum().backward()
        return run
    ms = median_ms({"prepare": prepare, "gram_potrf": gram_potrf, "solves": solves, "s_inverse": s_inverse,
                    "s_copies": s_copies, "gemm_rocblas": lambda: torch.matmul(Wt, W, out=out)})
    # (the two evals alternate in a loop of their own: each is a few launches, and its time follows what ran before)
    ms.update(median_ms({"eval_kl_cond": ev(cond), "eval_dubo_cond": ev(dcond), "eval_kl_cond_again": ev(cond)}))
    check_pending()
    ms["s_inverse"] -= ms.pop("s_copies")
    ms["syrks_abar_finish_by_difference"] = ms["prepare"] - ms["gram_potrf"] - ms["solves"] - ms["s_inverse"]
    return dict(N=N, Nn=Nn, L=L, **{f"{r}_ms": v for r, v in ms.items()})


if __name__ == "__main__":
    res = [measure(Nn) for Nn in (160, 1024)]
    line = json.dumps(res)
    print(line, flush=True)
    for a in sys.argv[1:]:
        if a.endswith(".json"):
            with open(a, "w") as f:
                f.write(line + "\n")
