"""Time the component-resolved cross-Gram x vector (lvae_gram_matvec_comp_f64) and the two predictors with and
without their per-component split.  Device events, 2 warm-up rounds, the median of 10 calls, the routes alternating
in one process.  Health-MNIST-shaped integer covariates, the sample config's kernel with random hyper-parameters.

  kernel     N = 4096 prediction rows, Nt = 1024 test rows, L = 16, the full kernel's R = 5 components:
             (a) lvae_gram_matvec_comp_f64 once;
             (b) what the library offered before it for the same numbers: R calls of lvae_gram_matvec_f64 with
                 one-component sub-specs (component r in slot 0, n_params and the parameter indices kept, so they
                 read the same parameter rows);
             (c) lvae_gram_matvec_f64 once: the sum alone.
             The largest difference of (a) from (b), and of sum_r (a) from (c), are reported too.
  exact      predict_exact against predict_exact_components at the same shape.
  inducing   batch_predict_varying_T against batch_predict_components at the Hensman shape of
             predict_var_timing.py (P = 256 x T = 16, M = 120, L = 16, Nt = 1024).

    python scripts/predict_components_timing.py [out.json]

DESIGN.md 4.3b-comp and profiles/predict_components_timing.json hold a run.
"""
import ctypes
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
from lvae_amd.elbo import check_pending  # noqa: E402

DEV = "cuda"
CFG = dict(cat_kernel=[2], bin_kernel=[], sqexp_kernel=[0],
           cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 2}, {'cont_covariate': 0, 'cat_covariate': 3},
                           {'cont_covariate': 1, 'cat_covariate': 4}],
           bin_int_kernel=[], covariate_missing_val=[])
N, NT, L, T = 4096, 1024, 16, 16
P, M, EPS = 256, 120, 1e-6


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def alternate(routes):
    ms, outs = {r: [] for r in routes}, {}
    for rep in range(12):
        for r, fn in routes.items():
            t, outs[r] = timed(fn)
            if rep >= 2:
                ms[r].append(t)
    check_pending()
    res = {f"{r}_ms_median": statistics.median(v) for r, v in ms.items()}
    res.update({f"{r}_ms_min": min(v) for r, v in ms.items()})
    return res, outs


def randomize(k, rng):
    with torch.no_grad():
        for name, p in k.named_parameters():
            lo, hi = (0.3, 1.5) if name.endswith("_log_scale") else (1.0, 4.0)
            p.copy_(torch.tensor(np.log(rng.uniform(lo, hi, p.shape[0])), dtype=p.dtype))


def sub_spec(spec, r):
    """Component r alone, in slot 0; n_params and the parameter indices kept"""
    s = _lib.KernelSpec.from_buffer_copy(spec)
    s.n_comp = 1
    s.n_fac[0], s.scale_idx[0] = spec.n_fac[r], spec.scale_idx[r]
    for f in range(_lib.MAX_FAC):
        s.kind[0][f], s.dim[0][f], s.param_idx[0][f] = spec.kind[r][f], spec.dim[r][f], spec.param_idx[r][f]
    return s


def measure_kernel(lib, k, X, Xt):
    spec, params = la.kernel_spec_and_params(k)
    params = params.detach().to(DEV, torch.float64).contiguous()
    R, Q = int(spec.n_comp), int(X.shape[1])
    v = torch.randn(N, L, generator=torch.Generator().manual_seed(5), dtype=torch.float64).to(DEV)
    subs = [sub_spec(spec, r) for r in range(R)]
    ws = torch.empty(max(int(lib.lvae_gram_matvec_comp_workspace_size(NT, N, L, R)),
                         int(lib.lvae_gram_matvec_workspace_size(NT, N, L)), 256), dtype=torch.uint8, device=DEV)
    p, st = _lib.ptr, _lib.stream_ptr

    def comp():
        out = torch.empty(R, NT, L, dtype=torch.float64, device=DEV)
        _lib.check(lib.lvae_gram_matvec_comp_f64(spec, p(Xt), Q, NT, p(X), Q, 0, N, L, p(params), p(v), L, p(out), L,
                                                 NT * L, p(ws), st()), "gram_matvec_comp")
        return out

    def per_component():
        out = torch.empty(R, NT, L, dtype=torch.float64, device=DEV)
        for r in range(R):
            _lib.check(lib.lvae_gram_matvec_f64(subs[r], p(Xt), Q, NT, p(X), Q, N, L, p(params), None, p(v), L,
                                                ctypes.c_void_p(out.data_ptr() + 8 * r * NT * L), L, p(ws), st()),
                       "gram_matvec")
        return out

    def summed():
        out = torch.empty(NT, L, dtype=torch.float64, device=DEV)
        _lib.check(lib.lvae_gram_matvec_f64(spec, p(Xt), Q, NT, p(X), Q, N, L, p(params), None, p(v), L, p(out), L,
                                            p(ws), st()), "gram_matvec")
        return out
    res, outs = alternate({"a_comp": comp, "b_per_component_calls": per_component, "c_sum_only": summed})
    scale = float(outs["c_sum_only"].abs().max())
    res["R"] = R
    res["a_vs_b_max_diff_rel"] = float((outs["a_comp"] - outs["b_per_component_calls"]).abs().max()) / scale
    res["sum_a_vs_c_max_diff_rel"] = float((outs["a_comp"].sum(0) - outs["c_sum_only"]).abs().max()) / scale
    res["a_over_c"] = res["a_comp_ms_median"] / res["c_sum_only_ms_median"]
    res["a_over_b"] = res["a_comp_ms_median"] / res["b_per_component_calls_ms_median"]
    return res


def measure():
    lib = _lib.lib()
    rng = np.random.default_rng(1)
    gen = torch.Generator().manual_seed(0)
    la.set_sync_checks(False)
    X = torch.tensor(health_mnist_covariates(N // T, T, seed=0), device=DEV)[:N]
    Xt = torch.tensor(health_mnist_covariates(NT // T, T, seed=1), device=DEV)[:NT]
    mu = torch.randn(N, L, generator=gen, dtype=torch.float64).to(DEV)
    k = la.generate_kernel(**CFG, latent_dim=L).to(DEV)
    randomize(k, rng)
    lik = la.GaussianLikelihood(L, noise=1.0).to(DEV)
    res = dict(N=N, Nt=NT, L=L, kernel=measure_kernel(lib, k, X, Xt))

    big = 64 << 30
    r, outs = alternate({"exact_mean": lambda: la.predict_exact(k, lik, X, Xt, mu, max_workspace_bytes=big),
                         "exact_components": lambda: la.predict_exact_components(k, lik, X, Xt, mu,
                                                                                 max_workspace_bytes=big)})
    r["mean_bit_equal"] = bool((outs["exact_mean"] == outs["exact_components"][0]).all())
    r["components_over_mean"] = r["exact_components_ms_median"] / r["exact_mean_ms_median"]
    res["exact"] = r

    # the Hensman-side shape of predict_var_timing.py: P x T prediction rows, 64 test subjects x 16 rows at half-step
    # times, every fourth of them outside the prediction set
    Xc = torch.tensor(health_mnist_covariates(P, T, seed=43))
    subj = rng.choice(P, NT // T, replace=False)
    tx = torch.cat([Xc[s * T:(s + 1) * T] for s in subj]).clone()
    tx[:, 0] += 0.5
    for j, s in enumerate(subj):
        if j % 4 == 3:
            tx[j * T:(j + 1) * T, 2] = float(P + j)
    tx = tx[torch.randperm(NT, generator=gen)].to(DEV)
    z = torch.stack([torch.cat([Xc[0:M // 2], Xc[P * T // 2:P * T // 2 + M // 2]])] * L).to(DEV)
    Xh = Xc.to(DEV)
    muh = torch.randn(P * T, L, generator=gen, dtype=torch.float64).to(DEV)
    k0, k1 = la.generate_kernel_batched(L, **CFG, id_covariate=2)
    randomize(k0, rng)
    randomize(k1, rng)
    k0, k1 = k0.to(DEV), k1.to(DEV)
    r, outs = alternate({
        "inducing_mean": lambda: la.batch_predict_varying_T(L, k0, k1, lik, Xh, tx, muh, z, 2, EPS),
        "inducing_components": lambda: la.batch_predict_components(L, k0, k1, lik, Xh, tx, muh, z, 2, EPS)})
    r["mean_bit_equal"] = bool((outs["inducing_mean"] == outs["inducing_components"][0]).all())
    r["components_over_mean"] = r["inducing_components_ms_median"] / r["inducing_mean_ms_median"]
    r.update(P=P, T=T, M=M)
    res["inducing"] = r
    return res


if __name__ == "__main__":
    line = json.dumps(measure())
    print(line, flush=True)
    for a in sys.argv[1:]:
        if a.endswith(".json"):
            with open(a, "w") as f:
                f.write(line + "\n")
