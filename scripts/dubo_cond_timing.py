"""Time the GP term of one iteration of new-subject latent inference (training.py:688-749) at P = 256 fixed + Pn = 8
new subjects x T = 16 rows, M = 120 inducing points, L = 16 dims (the kernel config and random hyper-parameters of
scripts/dubo_timing.py):
  (a) lvae_amd.deviance_upper_bound_batched on the joint batch, forward + backward, gradients on the new rows only
      (the kernels, the noise and the training latents do not require grad) -- the only route there was before
      condition_dubo;
  (b) cond(m_new, log_v_new) forward + backward (lvae_dubo_cond_eval_f64);
  (c) one lvae_amd.condition_dubo (lvae_dubo_cond_prepare_f64 and its allocations).
Device events, 2 warm-up rounds, the median of 10 calls, the routes alternating in one process with the pivot checks
deferred (set_sync_checks(False)); the relative difference of the values of (a) and (b), the ratio a / b and the
break-even iteration count c / (a - b) are reported too.  DESIGN.md and profiles/dubo_cond_timing.json hold a run.

    python scripts/dubo_cond_timing.py [out.json]
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
P, PN, T, M, L, EPS = 256, 8, 16, 120, 16, 1e-6


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
            p.requires_grad_(False)


def measure(seed=41):
    Pj = P + PN
    N, Nn = Pj * T, PN * T
    X = torch.tensor(health_mnist_covariates(Pj, T, seed=seed))       # cat(new, train): the first PN subjects are new
    gen = torch.Generator().manual_seed(seed)
    mu = torch.randn(N, L, generator=gen, dtype=torch.float64).to(DEV)
    lv = (0.1 * torch.randn(N, L, generator=gen, dtype=torch.float64)).to(DEV)
    z = torch.stack([torch.cat([X[0:M // 2], X[N // 2:N // 2 + M // 2]])] * L).to(DEV)
    X = X.to(DEV)
    k0, k1 = la.generate_kernel_batched(L, **CFG, id_covariate=2)
    rng = np.random.default_rng(seed)
    set_raw(k0, np.log(rng.uniform(0.5, 2.0, (L, len(list(k0.parameters()))))))
    set_raw(k1, np.log(rng.uniform(0.5, 2.0, (L, len(list(k1.parameters()))))))
    k0, k1 = k0.to(DEV), k1.to(DEV)
    lik = la.GaussianLikelihood(L, noise=1.0).to(DEV)
    for p in lik.parameters():
        p.requires_grad_(False)
    m_new, lv_new = mu[:Nn].clone().requires_grad_(), lv[:Nn].clone().requires_grad_()
    m_tr, lv_tr = mu[Nn:], lv[Nn:]

    def joint():
        m_new.grad, lv_new.grad = None, None
        d = la.deviance_upper_bound_batched(L, k0, k1, lik, X, torch.cat([m_new, m_tr]), torch.cat([lv_new, lv_tr]), z,
                                            Pj, T, EPS)
        tot = d.sum()
        tot.backward()
        return tot.detach()

    def prepare():
        return la.condition_dubo(L, k0, k1, lik, X[:Nn], X[Nn:], m_tr, lv_tr, z, T, EPS)

    cond = prepare()

    def conditioned():
        m_new.grad, lv_new.grad = None, None
        tot = cond(m_new, lv_new).sum()
        tot.backward()
        return tot.detach()
    routes = {"joint": joint, "cond": conditioned, "prepare": prepare}
    la.set_sync_checks(False)
    ms, outs = {r: [] for r in routes}, {}
    for rep in range(12):
        for r, fn in routes.items():
            t, outs[r] = timed(fn)
            if rep >= 2:
                ms[r].append(t)
    check_pending()
    res = dict(P=P, Pn=PN, T=T, M=M, L=L, **{f"{r}_ms_median": statistics.median(v) for r, v in ms.items()},
               **{f"{r}_ms_min": min(v) for r, v in ms.items()})
    a, b, c = (res[f"{r}_ms_median"] for r in ("joint", "cond", "prepare"))
    res["ratio_joint_over_cond"] = a / b
    res["break_even_iterations"] = c / (a - b)
    res["rel_diff_cond_vs_joint"] = float(abs(outs["cond"] - outs["joint"]) / abs(outs["joint"]))
    return res


if __name__ == "__main__":
    res = measure()
    line = json.dumps(res)
    print(line, flush=True)
    for a in sys.argv[1:]:
        if a.endswith(".json"):
            with open(a, "w") as f:
                f.write(line + "\n")
