"""Time the components' posterior covariance against the predictive variance of the same predictor on the same inputs:

  exact     N = 2048 prediction rows (P = 128 subjects x T = 16), L = 16 dims, Nt = 512 test rows, the sample config's
            kernel (R = 5 components), one dim group and one test-row chunk:
            (a) lvae_predict_exact_var_f64 alone (no mean), (b) lvae_predict_exact_comp_cov_f64 alone (no means): the
            solves have R times the columns; and the Python calls predict_exact(return_var=True),
            predict_exact_components() and predict_exact_components(return_cov=True).
  inducing  the Hensman C4 shape of predict_var_timing.py (P = 256 x T = 16, M = 120, L = 16) with Nt = 1024 test rows
            of 64 subjects, every fourth absent: batch_predict_varying_T(return_var=True) against
            batch_predict_components() and batch_predict_components(return_cov=True) (R = 1 + 4 components).

Whole call between device events, 2 warm-up rounds, the median of 10 calls, the routes alternating in one process with
the pivot checks deferred.  DESIGN.md and profiles/predict_comp_cov_timing.json hold a run.

    python scripts/predict_comp_cov_timing.py [out.json]
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
from lvae_amd.elbo import check_pending  # noqa: E402

DEV = "cuda"
CFG = dict(cat_kernel=[2], bin_kernel=[], sqexp_kernel=[0],
           cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 2}, {'cont_covariate': 0, 'cat_covariate': 3},
                           {'cont_covariate': 1, 'cat_covariate': 4}],
           bin_int_kernel=[], covariate_missing_val=[])
N, NT, L, T = 2048, 512, 16, 16
P, M, NT_H, EPS = 256, 120, 1024, 1e-6


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


def measure_exact(lib, rng, gen):
    X = torch.tensor(health_mnist_covariates(N // T, T, seed=0), device=DEV)[:N]
    Xt = torch.tensor(health_mnist_covariates(NT // T, T, seed=1), device=DEV)[:NT]
    mu = torch.randn(N, L, generator=gen, dtype=torch.float64).to(DEV)
    k = la.generate_kernel(**CFG, latent_dim=L).to(DEV)
    randomize(k, rng)
    lik = la.GaussianLikelihood(L, noise=1.0).to(DEV)
    spec, params = la.kernel_spec_and_params(k)
    params = params.detach().to(DEV, torch.float64).contiguous()
    R, Q = int(spec.n_comp), int(X.shape[1])
    noise = torch.ones(L, dtype=torch.float64, device=DEV)
    info = torch.empty(L, dtype=torch.int32, device=DEV)
    var = torch.empty(NT, L, dtype=torch.float64, device=DEV)
    cov = torch.empty(L, NT, R, R, dtype=torch.float64, device=DEV)
    ws = torch.empty(int(lib.lvae_predict_exact_comp_cov_workspace_size(N, NT, L, R, NT)), dtype=torch.uint8,
                     device=DEV)
    assert int(lib.lvae_predict_exact_var_workspace_size(N, NT, L, NT)) <= ws.numel()
    p, st = _lib.ptr, _lib.stream_ptr

    def abi_var():
        _lib.check(lib.lvae_predict_exact_var_f64(spec, p(X), Q, N, L, p(params), p(noise), None, L, p(Xt), Q, NT, None,
                                                  L, p(var), L, 0, NT, p(info), p(ws), st()), "predict_exact_var")
        return var

    def abi_comp_cov():
        _lib.check(lib.lvae_predict_exact_comp_cov_f64(spec, p(X), Q, N, L, p(params), p(noise), None, L, p(Xt), Q, NT,
                                                       None, L, None, L, NT * L, NT, p(cov), p(info), p(ws), st()),
                   "predict_exact_comp_cov")
        return cov
    big = 64 << 30
    res, outs = alternate({
        "abi_var": abi_var, "abi_comp_cov": abi_comp_cov,
        "py_mean_var": lambda: la.predict_exact(k, lik, X, Xt, mu, max_workspace_bytes=big, return_var=True),
        "py_components": lambda: la.predict_exact_components(k, lik, X, Xt, mu, max_workspace_bytes=big),
        "py_components_cov": lambda: la.predict_exact_components(k, lik, X, Xt, mu, max_workspace_bytes=big,
                                                                 return_cov=True)})
    res.update(N=N, Nt=NT, L=L, R=R)
    res["abi_comp_cov_over_var"] = res["abi_comp_cov_ms_median"] / res["abi_var_ms_median"]
    res["py_components_cov_over_mean_var"] = res["py_components_cov_ms_median"] / res["py_mean_var_ms_median"]
    scale = float(outs["abi_var"].abs().max())
    diff = outs["abi_comp_cov"].sum((2, 3)).T - outs["abi_var"]
    res["sum_rs_vs_var_max_diff_rel"] = float(diff.abs().max()) / scale
    return res


def measure_inducing(rng, gen):
    Xc = torch.tensor(health_mnist_covariates(P, T, seed=43))
    subj = rng.choice(P, NT_H // T, replace=False)
    tx = torch.cat([Xc[s * T:(s + 1) * T] for s in subj]).clone()
    tx[:, 0] += 0.5
    for j, s in enumerate(subj):
        if j % 4 == 3:
            tx[j * T:(j + 1) * T, 2] = float(P + j)
    tx = tx[torch.randperm(NT_H, generator=gen)].to(DEV)
    z = torch.stack([torch.cat([Xc[0:M // 2], Xc[P * T // 2:P * T // 2 + M // 2]])] * L).to(DEV)
    Xh = Xc.to(DEV)
    muh = torch.randn(P * T, L, generator=gen, dtype=torch.float64).to(DEV)
    lik = la.GaussianLikelihood(L, noise=1.0).to(DEV)
    k0, k1 = la.generate_kernel_batched(L, **CFG, id_covariate=2)
    randomize(k0, rng)
    randomize(k1, rng)
    k0, k1 = k0.to(DEV), k1.to(DEV)
    args = (L, k0, k1, lik, Xh, tx, muh, z, 2, EPS)
    res, outs = alternate({
        "mean_var": lambda: la.batch_predict_varying_T(*args, return_var=True),
        "components": lambda: la.batch_predict_components(*args),
        "components_cov": lambda: la.batch_predict_components(*args, return_cov=True)})
    res.update(P=P, T=T, M=M, L=L, Nt=NT_H, R=int(outs["components"][1].values.shape[0]))
    res["components_cov_over_mean_var"] = res["components_cov_ms_median"] / res["mean_var_ms_median"]
    var, tv = outs["mean_var"][1], outs["components_cov"][1].total_variance()
    res["total_variance_vs_var_max_diff_rel"] = float((tv - var)[var > 0].abs().max()) / float(var.max())
    return res


def measure():
    lib = _lib.lib()
    rng = np.random.default_rng(1)
    gen = torch.Generator().manual_seed(0)
    la.set_sync_checks(False)
    return dict(exact=measure_exact(lib, rng, gen), inducing=measure_inducing(rng, gen))


if __name__ == "__main__":
    line = json.dumps(measure())
    print(line, flush=True)
    for a in sys.argv[1:]:
        if a.endswith(".json"):
            with open(a, "w") as f:
                f.write(line + "\n")
