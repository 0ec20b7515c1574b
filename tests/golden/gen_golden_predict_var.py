"""Generate tests/golden/predict_var.npz: the predictive variances (and means) of the exact and the
inducing-point latent predictors, formed densely in fp64 on the CPU from Grams of the REFERENCE's own kernel
modules (GP_model.generate_kernel_batched, ``.evaluate()``).

Test infrastructure only, like gen_golden.py (whose shims and helpers it imports, and which it leaves as it is).
The reference computes posterior means only (model_test.py:11-17, utils.py:115-211), so the variance's definition
is the project's ("Predictive variance"); what this script takes from the reference is the kernels.
Both variances are k** - k*^T Sigma^-1 k* with Sigma assembled whole and one torch.linalg.solve per test row.

* exact: exact_predict.npz's configuration (its 300 prediction rows, per-dim kernels, noise and encoder means;
  the 12 label rows of the hmnist_tiny trio as the test set), Sigma_l = k_l(X, X) + noise_l I.
* inducing: P = 7 prediction subjects of lengths 1..5 out of T = 5 time points, M = 20 inducing points with
  jittered times, L = 3, 15 test rows in unsorted subject order: two test subjects absent from the prediction
  set, subject 2 with test rows at times it was and was not observed at.  Prior
  K~ = K0xz K0zz^-1 K0zx + k1(x, x) (K0zz with eps I; k1 carries the subject id, so it is block diagonal),
  Sigma_l = K~_l + noise_l I, k~* = K0xz K0zz^-1 K0zX* + k1(x, X*), k~** likewise.

The fixture holds inputs, raw hyper-parameters, noise and the dense results (data, not reference source).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_predict_var.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the reference shims, sets the default dtype to fp64)
import gen_golden_exact_predict as GE  # noqa: E402

import torch  # noqa: E402


def dense_posterior(Sigma, kstar, kss, mu):
    """(mean [Nt], var [Nt]) of one latent dim from Sigma [n, n], k* [n, Nt], the prior diagonal kss [Nt] and the
    observations mu [n]: one solve per test row."""
    mean, var = [], []
    for i in range(kstar.shape[1]):
        a = torch.linalg.solve(Sigma, kstar[:, i])
        mean.append(a @ mu)
        var.append(kss[i] - kstar[:, i] @ a)
    return torch.stack(mean), torch.stack(var)


def gen_exact():
    g = np.load(os.path.join(G.OUT, "exact_predict.npz"))
    L = int(g["L"])
    X, mu = torch.tensor(g["X"]), torch.tensor(g["mu"])
    tx = torch.tensor(np.load(os.path.join(G.OUT, "hmnist_tiny.npz"))["label"].astype(np.float64))
    assert tx.shape == (12, X.shape[1])
    c = GE.CFG
    mean, var, prior = [], [], []
    for l in range(L):
        k0, k1 = G.R.generate_kernel_batched(1, c['cat_kernel'], c['bin_kernel'], c['sqexp_kernel'],
                                             c['cat_int_kernel'], c['bin_int_kernel'], c['covariate_missing_val'],
                                             c['id_covariate'])
        k = G.R.AdditiveKernel(list(k0.kernels) + list(k1.kernels))
        names = [n for n, _ in k.named_parameters()]
        assert names == [str(n) for n in g["param_names"]]
        with torch.no_grad():
            for j, (_, p) in enumerate(k.named_parameters()):
                p.copy_(torch.full_like(p, float(g["raw"][l, j])))
            ev = lambda a, b: G.KernelAdapter(k)(a, b).evaluate().reshape(a.shape[0], b.shape[0])
            Sigma = ev(X, X) + float(g["noise"][l]) * torch.eye(X.shape[0])
            kss = torch.diagonal(ev(tx, tx))
            m, v = dense_posterior(Sigma, ev(X, tx), kss, mu[:, l])
        mean.append(m)
        var.append(v)
        prior.append(kss)
    out = dict(exact_tx=tx.numpy(), exact_mean=torch.stack(mean, 1).numpy(), exact_var=torch.stack(var, 1).numpy(),
               exact_prior=torch.stack(prior, 1).numpy())
    # the dense mean is the reference predictor's (model_test.py:11-17 multiplies by the explicit inverse)
    assert np.abs(out["exact_mean"] - g["Z_pred"]).max() < 1e-10 * np.abs(g["Z_pred"]).max()
    return out


def gen_inducing(seed=31, eps=1e-3):
    rng = np.random.default_rng(seed)
    P_all, T, L, M = 9, 5, 3, 20
    X = G.covariates(P_all, T, seed)
    k0, k1 = G.batched_kernels(L)
    G.randomise(k0, rng)
    G.randomise(k1, rng)
    lengths = [3, 1, 3, 5, 2, 4, 5]                       # prediction subjects 0..6; 7 and 8 are test-only
    pidx = G.varying_batch(X, T, np.arange(7), lengths, rng)
    kept2 = sorted(int(r) - 2 * T for r in pidx if r // T == 2)
    missed2 = [t for t in range(T) if t not in kept2]
    trows = ([(5, 0), (5, 3)] + [(8, 1), (8, 4)] + [(2, kept2[0]), (2, missed2[0])] + [(0, 2)] + [(7, 0), (7, 2), (7, 3)]
             + [(2, kept2[-1]), (2, missed2[-1])] + [(3, 1), (1, 4), (6, 0)])
    tidx = np.array([T * s + t for s, t in trows])
    assert len(tidx) == 15 and len(pidx) == sum(lengths)
    zrows = np.concatenate([np.arange(0, M // 2), np.arange(P_all * T // 2, P_all * T // 2 + M // 2)])
    Z1 = X[zrows].copy()
    shift = rng.uniform(-0.4, 0.4, M)
    Z1[:, 0] += shift
    Z1[:, 1] += shift * (Z1[:, 4] == 1)                   # disease_time moves with time_age where sick
    Z = np.stack([Z1] * L)
    mu = rng.standard_normal((len(pidx), L))
    noise = rng.uniform(0.5, 1.5, L)
    # [L, n, Q] inputs: GP_model's batched kernels left-align their [L] parameters
    xp, xt, zt = (torch.tensor(a).unsqueeze(0).expand(L, *a.shape) for a in (X[pidx], X[tidx], Z1))
    with torch.no_grad():
        e0 = lambda a, b: G.KernelAdapter(k0)(a, b).evaluate()     # [L, n1, n2]
        e1 = lambda a, b: G.KernelAdapter(k1)(a, b).evaluate()
        K0zz = e0(zt, zt) + eps * torch.eye(M)
        K0xz, K0Xz = e0(xp, zt), e0(xt, zt)
        A = torch.linalg.solve(K0zz, K0xz.transpose(1, 2))          # K0zz^-1 K0zx [L, M, n]
        Q = torch.linalg.solve(K0zz, K0Xz.transpose(1, 2))          # K0zz^-1 K0zX* [L, M, Nt]
        Kt = K0xz @ A + e1(xp, xp)
        kstar = K0xz @ Q + e1(xp, xt)
        kss = torch.diagonal(K0Xz @ Q + e1(xt, xt), dim1=1, dim2=2)
        mean, var = [], []
        for l in range(L):
            m, v = dense_posterior(Kt[l] + noise[l] * torch.eye(len(pidx)), kstar[l], kss[l], torch.tensor(mu[:, l]))
            mean.append(m)
            var.append(v)
    n0, v0 = G.raw_params(k0)
    n1, v1 = G.raw_params(k1)
    return dict(ind_X_all=X, ind_pidx=pidx, ind_tidx=tidx, ind_Z=Z, ind_mu=mu, ind_noise=noise, ind_eps=eps,
                ind_raw0=np.stack(v0, 0), ind_raw1=np.stack(v1, 0), ind_id_covariate=2, ind_L=L, ind_M=M,
                ind_mean=torch.stack(mean, 1).numpy(), ind_var=torch.stack(var, 1).numpy(),
                ind_prior=kss.T.numpy().copy())


if __name__ == "__main__":
    G.save("predict_var.npz", **gen_exact(), **gen_inducing())
