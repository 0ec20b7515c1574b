"""Time the joint covariance of the two latent predictors beside their variance, on the inputs of
scripts/predict_var_timing.py (whose set-up this script imports):

  exact     predict_exact at N = 4096 prediction rows, L = 16 dims, Nt = 1024 test rows in 64 groups of 16 (the
            test subjects): return_var=True against return_cov=True, groups = the id covariate (one dim group, one
            test-row chunk);
  inducing  batch_predict_varying_T at the Hensman C4 shape (P = 256 x T = 16, M = 120, L = 16), the same 1024 test
            rows, 64 subjects of 16 rows, every fourth absent from the prediction set: return_var=True against
            return_cov=True;
  draws     sample_trajectories with S = 16 draws from the inducing-point route's covariance ([16, 64, 16, 16] blocks:
            the jitter copy, lvae_potrf_f64 over the 1024 blocks and the draw kernel).

Wall time of the whole Python call between device events (host-side grouping, copies and allocations included),
2 warm-up rounds, the median of 10 calls, the routes alternating in one process with the pivot checks deferred.
DESIGN.md and profiles/predict_cov_timing.json hold a run.

    python scripts/predict_cov_timing.py [out.json]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_var_timing as PV  # noqa: E402  (puts the package on the path)

import lvae_amd as la  # noqa: E402
from lvae_amd.data import health_mnist_covariates  # noqa: E402

DEV = PV.DEV
P, T, M, L, NT, EPS = PV.P, PV.T, PV.M, PV.L, PV.NT, PV.EPS


def measure(seed=43):
    N = P * T
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    Xc = torch.tensor(health_mnist_covariates(P, T, seed=seed))
    mu = torch.randn(N, L, generator=gen, dtype=torch.float64).to(DEV)
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
    res = dict(P=P, T=T, N=N, M=M, L=L, Nt=NT, groups=NT // T, group_rows=T)

    k = la.generate_kernel(**PV.CFG, latent_dim=L).to(DEV)
    lik = la.GaussianLikelihood(L, noise=1.0).to(DEV)
    r, outs = PV.alternate({"exact_mean_var": lambda: la.predict_exact(k, lik, X, tx, mu, return_var=True),
                            "exact_mean_cov": lambda: la.predict_exact(k, lik, X, tx, mu, return_cov=True,
                                                                       groups=tx[:, 2])})
    res.update(r)
    res["exact_cov_over_var"] = res["exact_mean_cov_ms_median"] / res["exact_mean_var_ms_median"]
    res["exact_mean_bit_equal"] = bool((outs["exact_mean_var"][0] == outs["exact_mean_cov"][0]).all())
    res["exact_diag_minus_var_max"] = float((outs["exact_mean_cov"][1].diagonal() - outs["exact_mean_var"][1]).abs().max())

    k0, k1 = la.generate_kernel_batched(L, **PV.CFG, id_covariate=2)
    PV.set_raw(k0, np.log(rng.uniform(0.5, 2.0, (L, len(list(k0.parameters()))))))
    PV.set_raw(k1, np.log(rng.uniform(0.5, 2.0, (L, len(list(k1.parameters()))))))
    k0, k1 = k0.to(DEV), k1.to(DEV)
    call = lambda **kw: la.batch_predict_varying_T(L, k0, k1, lik, X, tx, mu, z, 2, EPS, **kw)
    r, outs = PV.alternate({"inducing_mean_var": lambda: call(return_var=True),
                            "inducing_mean_cov": lambda: call(return_cov=True)})
    res.update(r)
    res["inducing_cov_over_var"] = res["inducing_mean_cov_ms_median"] / res["inducing_mean_var_ms_median"]
    res["inducing_mean_bit_equal"] = bool((outs["inducing_mean_var"][0] == outs["inducing_mean_cov"][0]).all())
    res["inducing_diag_minus_var_max"] = float((outs["inducing_mean_cov"][1].diagonal()
                                                - outs["inducing_mean_var"][1]).abs().max())

    mean, cov = outs["inducing_mean_cov"]
    eps = torch.randn(16, NT, L, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    r, outs = PV.alternate({"draws16": lambda: la.sample_trajectories(mean, cov, eps=eps)})
    res.update(r)
    res["draws_finite"] = bool(torch.isfinite(outs["draws16"]).all())
    return res


if __name__ == "__main__":
    res = measure()
    line = json.dumps(res)
    print(line, flush=True)
    for a in sys.argv[1:]:
        if a.endswith(".json"):
            with open(a, "w") as f:
                f.write(line + "\n")
