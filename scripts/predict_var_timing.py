"""Time the two latent predictors with and without the predictive variance, mean-only against mean + variance on
the same inputs:

  exact     predict_exact at N = 4096 prediction rows (P = 256 subjects x T = 16), L = 16 dims, Nt = 1024 test rows
            (lvae_predict_exact_f64 against lvae_predict_exact_var_f64, one dim group, one test-row chunk);
  inducing  batch_predict_varying_T at the Hensman C4 shape (P = 256 x T = 16, M = 120 inducing points, L = 16;
            the kernel config and random hyper-parameters of scripts/dubo_timing.py) with Nt = 1024 test rows of 64
            subjects, every fourth of them absent from the prediction set (lvae_predict_f64 against
            lvae_predict_var_f64).

Wall time of the whole Python call between device events (the host-side layout, the copies and the workspace
allocation included: what a caller pays), 2 warm-up rounds, the median of 10 calls, the two routes alternating in one
process with the pivot checks deferred.  DESIGN.md and profiles/predict_var_timing.json hold a run.

    python scripts/predict_var_timing.py [out.json]
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
from lvae_amd.data import health_mnist_covariates  # noqa: E402
from lvae_amd.elbo import check_pending  # noqa: E402

DEV = "cuda"
CFG = dict(cat_kernel=[2], bin_kernel=[], sqexp_kernel=[0],
           cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 2}, {'cont_covariate': 0, 'cat_covariate': 3},
                           {'cont_covariate': 1, 'cat_covariate': 4}],
           bin_int_kernel=[], covariate_missing_val=[])
P, T, M, L, NT, EPS = 256, 16, 120, 16, 1024, 1e-6


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def set_raw(module, raw_rows):
    with torch.no_grad():
        for j, (_, p) in enumerate(module.named_parameters()):
            p.copy_(torch.as_tensor(raw_rows[:, j], dtype=p.dtype))


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


def measure(seed=43):
    N = P * T
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    Xc = torch.tensor(health_mnist_covariates(P, T, seed=seed))
    mu = torch.randn(N, L, generator=gen, dtype=torch.float64).to(DEV)
    # test rows: 64 subjects x 16 rows at half-step times; every fourth subject gets an id outside the prediction set
    subj = rng.choice(P, NT // T, replace=False)
    tx = torch.cat([Xc[s * T:(s + 1) * T] for s in subj]).clone()
    tx[:, 0] += 0.5
    for k, s in enumerate(subj):
        if k % 4 == 3:
            tx[k * T:(k + 1) * T, 2] = float(P + k)
    tx = tx[torch.randperm(NT, generator=gen)].to(DEV)
    z = torch.stack([torch.cat([Xc[0:M // 2], Xc[N // 2:N // 2 + M // 2]])] * L).to(DEV)
    X = Xc.to(DEV)
    la.set_sync_checks(False)
    res = dict(P=P, T=T, N=N, M=M, L=L, Nt=NT)

    # exact: the non-split kernel at its initial hyper-parameters
    k = la.generate_kernel(**CFG, latent_dim=L).to(DEV)
    lik = la.GaussianLikelihood(L, noise=1.0).to(DEV)
    r, outs = alternate({"exact_mean": lambda: la.predict_exact(k, lik, X, tx, mu),
                         "exact_mean_var": lambda: la.predict_exact(k, lik, X, tx, mu, return_var=True)})
    res.update(r)
    res["exact_var_over_mean"] = res["exact_mean_var_ms_median"] / res["exact_mean_ms_median"]
    res["exact_mean_bit_equal"] = bool((outs["exact_mean"] == outs["exact_mean_var"][0]).all())
    res["exact_var_min"], res["exact_var_max"] = (float(outs["exact_mean_var"][1].min()),
                                                  float(outs["exact_mean_var"][1].max()))

    # inducing points: the split kernels
    k0, k1 = la.generate_kernel_batched(L, **CFG, id_covariate=2)
    set_raw(k0, np.log(rng.uniform(0.5, 2.0, (L, len(list(k0.parameters()))))))
    set_raw(k1, np.log(rng.uniform(0.5, 2.0, (L, len(list(k1.parameters()))))))
    k0, k1 = k0.to(DEV), k1.to(DEV)
    call = lambda **kw: la.batch_predict_varying_T(L, k0, k1, lik, X, tx, mu, z, 2, EPS, **kw)
    r, outs = alternate({"inducing_mean": call, "inducing_mean_var": lambda: call(return_var=True)})
    res.update(r)
    res["inducing_var_over_mean"] = res["inducing_mean_var_ms_median"] / res["inducing_mean_ms_median"]
    res["inducing_mean_bit_equal"] = bool((outs["inducing_mean"] == outs["inducing_mean_var"][0]).all())
    res["inducing_var_min"], res["inducing_var_max"] = (float(outs["inducing_mean_var"][1].min()),
                                                        float(outs["inducing_mean_var"][1].max()))
    return res


if __name__ == "__main__":
    res = measure()
    line = json.dumps(res)
    print(line, flush=True)
    for a in sys.argv[1:]:
        if a.endswith(".json"):
            with open(a, "w") as f:
                f.write(line + "\n")
