"""Time lvae_amd.predict_exact (lvae_predict_exact_f64) against what the library offered before it: Gram.evaluate()
for [L, N, N] and [L, Nt, N], then per latent dim torch.linalg.cholesky, cholesky_solve and matmul in fp64 on the
GPU.  Device events, 2 warm-up rounds, the median of 10 calls, the two routes alternating in one process; the
max-norm difference of the two Z_pred is reported too.  Health-MNIST-shaped integer covariates, the sample
config's kernel with random hyper-parameters.  DESIGN.md 4.3b and profiles/exact_predict_timing.json hold a run.

    python scripts/exact_predict_timing.py [fused] [shape index] > timing.jsonl

``fused`` times predict_exact alone (the run to put under ``rocprofv3 --kernel-trace --stats``:
profiles/exact_predict_kernel_stats.csv); shape index 0: N = 4096, Nt = 1024; 1: N = 6040, Nt = 4000 (L = 16).
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

DEV = "cuda"
CFG = dict(cat_kernel=[2], bin_kernel=[], sqexp_kernel=[0],
           cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 2}, {'cont_covariate': 0, 'cat_covariate': 3},
                           {'cont_covariate': 1, 'cat_covariate': 4}],
           bin_int_kernel=[], covariate_missing_val=[])
SHAPES = [(4096, 1024, 16, 16), (6040, 4000, 16, 20)]   # N, Nt, L, rows per subject


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def measure(N, Nt, L, T, only_fused):
    X = torch.tensor(health_mnist_covariates(N // T, T, seed=0), device=DEV)[:N]
    Xt = torch.tensor(health_mnist_covariates(Nt // T, T, seed=1), device=DEV)[:Nt]
    mu = torch.randn(N, L, generator=torch.Generator().manual_seed(0), dtype=torch.float64).to(DEV)
    k = la.generate_kernel(**CFG, latent_dim=L).to(DEV)
    rng = np.random.default_rng(1)
    with torch.no_grad():
        for name, p in k.named_parameters():
            lo, hi = (0.3, 1.5) if name.endswith("_log_scale") else (1.0, 4.0)
            p.copy_(torch.tensor(np.log(rng.uniform(lo, hi, L)), dtype=p.dtype))
    lik = la.GaussianLikelihood(L, noise=1.0).to(DEV)

    def fused():
        return la.predict_exact(k, lik, X, Xt, mu, max_workspace_bytes=64 << 30)

    def torch_route():
        with torch.no_grad():
            K = k(X, X).evaluate() + torch.eye(N, dtype=torch.float64, device=DEV)
            Ks = k(Xt, X).evaluate()
            cols = []
            for l in range(L):   # one dim at a time, as the reference loops
                cols.append(Ks[l] @ torch.cholesky_solve(mu[:, l:l + 1], torch.linalg.cholesky(K[l])))
            return torch.cat(cols, 1)
    routes = {"fused": fused} if only_fused else {"fused": fused, "torch": torch_route}
    ms, outs = {r: [] for r in routes}, {}
    for rep in range(12):
        for r, fn in routes.items():
            t, outs[r] = timed(fn)
            if rep >= 2:
                ms[r].append(t)
    res = dict(N=N, Nt=Nt, L=L, **{f"{r}_ms_median": statistics.median(v) for r, v in ms.items()},
               **{f"{r}_ms_min": min(v) for r, v in ms.items()})
    if not only_fused:
        res["rel_diff_fused_vs_torch"] = float((outs["fused"] - outs["torch"]).abs().max() / outs["torch"].abs().max())
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    only_fused = "fused" in args
    picks = [int(a) for a in args if a.isdigit()] or range(len(SHAPES))
    for i in picks:
        print(json.dumps(measure(*SHAPES[i], only_fused)), flush=True)
        torch.cuda.empty_cache()
