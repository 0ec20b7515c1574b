"""Generate tests/golden/dubo_cond.npz: the loss the REFERENCE evaluates when it infers the latents of new
subjects (the second half of variational_inference_optimization, training.py:725-733): its own
elbo_functions.deviance_upper_bound on cat(pred, train) with P + Pn subjects, per latent dim, and the autograd
gradients with respect to the pred rows of (mu, log_var) alone -- the train rows, the kernels, the noise and the
inducing points are constants there.

Test infrastructure only, like gen_golden.py (whose shims and helpers it imports, and which it leaves as it is).
P = 5 train + Pn = 2 pred subjects of T = 4 rows, M = 8 inducing points per dim (rows of the batch with jittered
times), L = 2 dims with their own kernels and noise; two points: the drawn pred latents, and a far one (mu + 3,
log_var - 2).  The fixture holds inputs, raw hyper-parameters, noise and the results (data, not reference source).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_dubo_cond.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the reference shims, sets the default dtype to fp64)

import torch  # noqa: E402


def gen(seed=47, eps=1e-6):
    rng = np.random.default_rng(seed)
    P, Pn, T, M, L = 5, 2, 4, 8, 2
    Nn, N = Pn * T, (P + Pn) * T
    X = G.covariates(P + Pn, T, seed)            # cat(pred, train): subjects 0, 1 are the new ones
    Z = np.stack([X[np.sort(rng.choice(N, M, replace=False))] for _ in range(L)])
    Z[..., 0] += rng.uniform(-0.4, 0.4, (L, M))
    mu = rng.standard_normal((N, L))
    logv = 0.1 * rng.standard_normal((N, L))
    noise = rng.uniform(0.5, 1.5, L)
    points = [(mu[:Nn], logv[:Nn]), (mu[:Nn] + 3.0, logv[:Nn] - 2.0)]
    raw0, raw1 = [], []
    val, dmu, dlv = np.zeros((2, L)), np.zeros((2, Nn, L)), np.zeros((2, Nn, L))
    for l in range(L):
        k0, k1 = G.batched_kernels(1)
        G.randomise(k0, rng)
        G.randomise(k1, rng)
        raw0.append(np.concatenate(G.raw_params(k0)[1]))
        raw1.append(np.concatenate(G.raw_params(k1)[1]))
        lik = G.LikStub(torch.tensor([noise[l]]))
        for q, (mp, lp) in enumerate(points):
            m_pred = torch.tensor(mp[:, l], requires_grad=True)
            l_pred = torch.tensor(lp[:, l], requires_grad=True)
            m_all = torch.cat((m_pred, torch.tensor(mu[Nn:, l])), 0)
            l_all = torch.cat((l_pred, torch.tensor(logv[Nn:, l])), 0)
            du = EF_dubo(k0, k1, lik, X, m_all, l_all, Z[l], P + Pn, T, eps)
            gm, gl = torch.autograd.grad(du, (m_pred, l_pred))
            val[q, l], dmu[q, :, l], dlv[q, :, l] = du.item(), gm.numpy(), gl.numpy()
    return dict(X=X, Z=Z, mu=mu, logv=logv, noise=noise, raw0=np.stack(raw0), raw1=np.stack(raw1), P=P, Pn=Pn, T=T,
                M=M, L=L, eps=eps, id_covariate=2, m_pts=np.stack([p[0] for p in points]),
                lv_pts=np.stack([p[1] for p in points]), dubo=val, dubo_dm=dmu, dubo_dlogv=dlv)


def EF_dubo(k0, k1, lik, X, m, lv, Z, P, T, eps):
    du = G.EF.deviance_upper_bound(G.KernelAdapter(k0), G.KernelAdapter(k1), lik, torch.tensor(X), m, lv,
                                   torch.tensor(Z), P, T, eps)
    return du.reshape(-1)[0]


if __name__ == "__main__":
    G.save("dubo_cond.npz", **gen())
