"""Time one forward + backward of the full-batch DUBO of all latent dims at the Regime A data shape (P = 256 subjects
x T = 16 rows, M = 120 inducing points, L = 16 dims; the kernel config and random hyper-parameters of
test_gpu_regime_a._c4_problem): (a) the per-dim route, sum_l lvae_amd.deviance_upper_bound (torch composition over
the HIP Grams and inverses, autograd backward), against (b) lvae_amd.deviance_upper_bound_batched (lvae_dubo_fwd_f64
/ lvae_dubo_bwd_f64).  Device events, 2 warm-up rounds, the median of 10 calls, the two routes alternating in one
process with the pivot checks deferred (set_sync_checks(False)); the relative difference of the two values is
reported too.  DESIGN.md and profiles/dubo_timing.json hold a run.

    python scripts/dubo_timing.py [batched] [zgrad] [out.json]

``batched`` times (b) alone (the run to put under ``rocprofv3 --kernel-trace --stats``:
profiles/dubo_kernel_stats.csv).  ``zgrad`` adds (c) = (b) with z.requires_grad (learnable inducing points: the
backward also runs lvae_dubo_bwd_z_f64), alternating with the others; ``batched zgrad`` under rocprofv3 gave
profiles/dubo_dz_kernel_stats.csv.
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
P, T, M, L, EPS = 256, 16, 120, 16, 1e-6


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


def measure(only_batched, zgrad=False, seed=41):
    N = P * T
    X = torch.tensor(health_mnist_covariates(P, T, seed=seed))
    gen = torch.Generator().manual_seed(seed)
    mu = torch.randn(N, L, generator=gen, dtype=torch.float64).to(DEV).requires_grad_()
    lv = (0.1 * torch.randn(N, L, generator=gen, dtype=torch.float64)).to(DEV).requires_grad_()
    z = torch.stack([torch.cat([X[0:M // 2], X[N // 2:N // 2 + M // 2]])] * L).to(DEV)
    X = X.to(DEV)
    k0, k1 = la.generate_kernel_batched(L, **CFG, id_covariate=2)
    rng = np.random.default_rng(seed)
    raw0 = np.log(rng.uniform(0.5, 2.0, (L, len(list(k0.parameters())))))
    raw1 = np.log(rng.uniform(0.5, 2.0, (L, len(list(k1.parameters())))))
    set_raw(k0, raw0)
    set_raw(k1, raw1)
    k0, k1 = k0.to(DEV), k1.to(DEV)
    lik = la.GaussianLikelihood(L, noise=1.0).to(DEV)
    k0s, k1s, liks = [], [], []
    for l in range(L):
        a, b = la.generate_kernel_approx(**CFG, id_covariate=2)
        set_raw(a, raw0[l:l + 1])
        set_raw(b, raw1[l:l + 1])
        k0s.append(a.to(DEV))
        k1s.append(b.to(DEV))
        liks.append(la.GaussianLikelihood(1, noise=1.0).to(DEV))
    params = [mu, lv] + [p for m in (k0, k1, lik, *k0s, *k1s, *liks) for p in m.parameters()]

    def zero():
        for p in params:
            p.grad = None

    z_dz = z.clone().requires_grad_()
    params.append(z_dz)

    def batched(zt=z):
        zero()
        d = la.deviance_upper_bound_batched(L, k0, k1, lik, X, mu, lv, zt, P, T, EPS)
        tot = d.sum()
        tot.backward()
        return tot.detach()

    def per_dim():
        zero()
        tot = 0.0
        for l in range(L):
            tot = tot + la.deviance_upper_bound(k0s[l], k1s[l], liks[l], X, mu[:, l], lv[:, l], z[l], P, T, EPS)
        tot.backward()
        return tot.detach()
    routes = {"batched": batched} if only_batched else {"per_dim": per_dim, "batched": batched}
    if zgrad:  # learnable inducing points: the same call with z.requires_grad (adds lvae_dubo_bwd_z_f64)
        routes["batched_dz"] = lambda: batched(z_dz)
    la.set_sync_checks(False)
    ms, outs = {r: [] for r in routes}, {}
    for rep in range(12):
        for r, fn in routes.items():
            t, outs[r] = timed(fn)
            if rep >= 2:
                ms[r].append(t)
    check_pending()
    res = dict(P=P, T=T, M=M, L=L, **{f"{r}_ms_median": statistics.median(v) for r, v in ms.items()},
               **{f"{r}_ms_min": min(v) for r, v in ms.items()})
    if not only_batched:
        res["speedup_median"] = res["per_dim_ms_median"] / res["batched_ms_median"]
        res["rel_diff_batched_vs_per_dim"] = float(abs(outs["batched"] - outs["per_dim"]) / abs(outs["per_dim"]))
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    res = measure("batched" in args, "zgrad" in args)
    line = json.dumps(res)
    print(line, flush=True)
    for a in args:
        if a.endswith(".json"):
            with open(a, "w") as f:
                f.write(line + "\n")
