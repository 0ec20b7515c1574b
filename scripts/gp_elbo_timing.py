"""Time one forward + backward of the full-batch sampled GP ELBO ('GPapprox') of all latent dims at the Regime A data
shape (P = 256 subjects x T = 16 rows, M = 120 inducing points, L = 16 dims; the kernel config and random
hyper-parameters of scripts/dubo_timing.py) with S = 1 and S = 4 samples of the latent: (a) the per-dim route,
-sum_{s,l} lvae_amd.elbo / S (torch composition over the HIP Grams and inverses, autograd backward: 16 S calls),
against (b) lvae_amd.elbo_batched (lvae_gp_elbo_fwd_f64 / lvae_gp_elbo_bwd_f64: one call each way).  Device
events, 2 warm-up rounds of every (route, S), the median of 10 calls, the two routes alternating in one process
with the pivot checks deferred (set_sync_checks(False)); the relative difference of the two values is reported
too.  DESIGN.md and profiles/gp_elbo_timing.json hold a run.

    python scripts/gp_elbo_timing.py [batched] [samples=4] [out.json]

``batched`` times (b) alone and ``samples=`` one sample count alone (the run to put under ``rocprofv3
--kernel-trace --stats``: profiles/gp_elbo_kernel_stats_S4.csv).
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
SAMPLES = (1, 4)


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


def fused_pass_work(S):
    """(bytes, f64 MFMA flops) the fused subject pass needs per call, from the shapes: it reads X [L, N, M], iB and
    K0 [L, P, T, T] and the samples [S, N, L], writes iBK [L, N, M], s [L, N, 16] and one partial per (dim, group);
    per subject and dim the MFMA products are iBK (T T Mp), Q on the lower tiles (T 256 per tile), Pm (T Mp 16)
    and s (T T 16), 2 flops a multiply-add, Mp = M rounded up to 16, T rounded up to 4 in the k loops."""
    N, G = P * T, (P + 15) // 16
    tm = (M + 15) // 16
    nt, Mp, T4, Tp = tm * (tm + 1) // 2, 16 * tm, (T + 3) // 4 * 4, (T + 15) // 16 * 16
    part = nt * 256 + 128 * 16 + 24
    byt = 8 * (2 * L * N * M + 2 * L * P * T * T + S * N * L + L * N * 16 + L * G * part)
    flops = 2 * L * P * (Tp * T4 * Mp + nt * 256 * T4 + Mp * 16 * T4 + Tp * T4 * 16)
    return byt, flops


def measure(only_batched, seed=41):
    N, Smax = P * T, max(SAMPLES)
    X = torch.tensor(health_mnist_covariates(P, T, seed=seed))
    gen = torch.Generator().manual_seed(seed)
    mu = torch.randn(N, L, generator=gen, dtype=torch.float64)
    y = (mu[None] + 0.3 * torch.randn(Smax, N, L, generator=gen, dtype=torch.float64)).to(DEV).requires_grad_()
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
    params = [y] + [p for m in (k0, k1, lik, *k0s, *k1s, *liks) for p in m.parameters()]

    def zero():
        for p in params:
            p.grad = None

    def batched(S):
        zero()
        tot = -la.elbo_batched(L, k0, k1, lik, X, y[:S], z, P, T, EPS).sum() / S
        tot.backward()
        return tot.detach()

    def per_dim(S):
        zero()
        tot = 0.0
        for s in range(S):
            for l in range(L):
                tot = tot - la.elbo(k0s[l], k1s[l], liks[l], X, y[s, :, l], z[l], P, T, EPS)
        tot = tot / S
        tot.backward()
        return tot.detach()
    routes = {"batched": batched} if only_batched else {"per_dim": per_dim, "batched": batched}
    la.set_sync_checks(False)
    ms, outs = {(r, S): [] for r in routes for S in SAMPLES}, {}
    for rep in range(12):
        for S in SAMPLES:
            for r, fn in routes.items():
                t, outs[r, S] = timed(lambda: fn(S))
                if rep >= 2:
                    ms[r, S].append(t)
    check_pending()
    res = dict(P=P, T=T, M=M, L=L)
    for S in SAMPLES:
        for r in routes:
            res[f"{r}_S{S}_ms_median"] = statistics.median(ms[r, S])
            res[f"{r}_S{S}_ms_min"] = min(ms[r, S])
        byt, flops = fused_pass_work(S)
        res[f"fused_pass_S{S}_bytes"], res[f"fused_pass_S{S}_mfma_flops"] = byt, flops
        if not only_batched:
            res[f"speedup_S{S}_median"] = res[f"per_dim_S{S}_ms_median"] / res[f"batched_S{S}_ms_median"]
            res[f"rel_diff_S{S}_batched_vs_per_dim"] = float(abs(outs["batched", S] - outs["per_dim", S]) /
                                                             abs(outs["per_dim", S]))
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    for a in args:
        if a.startswith("samples="):   # e.g. samples=4: that sample count alone (one profile per count)
            SAMPLES = tuple(int(v) for v in a[8:].split(","))
    res = measure("batched" in args)
    line = json.dumps(res)
    print(line, flush=True)
    for a in args:
        if a.endswith(".json"):
            with open(a, "w") as f:
                f.write(line + "\n")
