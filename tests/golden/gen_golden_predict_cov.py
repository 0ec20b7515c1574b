"""Generate tests/golden/predict_cov.npz: the dense [Nt, Nt] joint predictive covariance per latent dim of the exact
and the inducing-point latent predictors, for exactly the inputs of predict_var.npz (which this script reads and
leaves as it is), formed in fp64 on the CPU from Grams of the REFERENCE's own kernel modules
(GP_model.generate_kernel_batched, ``.evaluate()``).

Test infrastructure only, like gen_golden_predict_var.py (whose definitions it follows; gen_golden's shims and
helpers are imported, not changed).  The reference computes posterior means only, so the covariance's definition is
the project's ("Joint covariance and trajectory draws"); what this script takes from the reference is
the kernels.  Both covariances are K** - K*^T Sigma^-1 K* with Sigma assembled whole and one torch.linalg.solve:

* exact: exact_predict.npz's 300 prediction rows, per-dim kernels and noise, predict_var.npz's 12 test rows,
  Sigma_l = k_l(X, X) + noise_l I  ->  exact_cov [L, 12, 12].
* inducing: predict_var.npz's P = 7 prediction subjects, M = 20 inducing points, L = 3, 15 test rows,
  prior K~ = K0xz K0zz^-1 K0zx + k1 (K0zz with eps I), Sigma_l = K~_l + noise_l I  ->  ind_cov [3, 15, 15].

The diagonals reproduce predict_var.npz's variances (asserted here at 1e-12 of the largest prior variance).  The
fixture holds the two arrays only (data, not reference source).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_predict_cov.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the reference shims, sets the default dtype to fp64)
import gen_golden_exact_predict as GE  # noqa: E402

import torch  # noqa: E402


def dense_cov(Sigma, kstar, kss):
    """K** - K*^T Sigma^-1 K* [Nt, Nt] of one latent dim, symmetrised (the two halves differ by rounding only)"""
    c = kss - kstar.T @ torch.linalg.solve(Sigma, kstar)
    return 0.5 * (c + c.T)


def gen_exact(gv):
    g = np.load(os.path.join(G.OUT, "exact_predict.npz"))
    X, tx = torch.tensor(g["X"]), torch.tensor(gv["exact_tx"])
    c = GE.CFG
    cov = []
    for l in range(int(g["L"])):
        k0, k1 = G.R.generate_kernel_batched(1, c['cat_kernel'], c['bin_kernel'], c['sqexp_kernel'],
                                             c['cat_int_kernel'], c['bin_int_kernel'], c['covariate_missing_val'],
                                             c['id_covariate'])
        k = G.R.AdditiveKernel(list(k0.kernels) + list(k1.kernels))
        assert [n for n, _ in k.named_parameters()] == [str(n) for n in g["param_names"]]
        with torch.no_grad():
            for j, (_, p) in enumerate(k.named_parameters()):
                p.copy_(torch.full_like(p, float(g["raw"][l, j])))
            ev = lambda a, b: G.KernelAdapter(k)(a, b).evaluate().reshape(a.shape[0], b.shape[0])
            Sigma = ev(X, X) + float(g["noise"][l]) * torch.eye(X.shape[0])
            cov.append(dense_cov(Sigma, ev(X, tx), ev(tx, tx)))
    return torch.stack(cov).numpy()


def gen_inducing(gv):
    L, M, eps = int(gv["ind_L"]), int(gv["ind_M"]), float(gv["ind_eps"])
    X, Z1 = gv["ind_X_all"], gv["ind_Z"][0]
    k0, k1 = G.batched_kernels(L)
    with torch.no_grad():
        for mod, raw in ((k0, gv["ind_raw0"]), (k1, gv["ind_raw1"])):   # raw [params, L] in named_parameters order
            for j, (_, p) in enumerate(mod.named_parameters()):
                p.copy_(torch.tensor(raw[j]).reshape(p.shape))
        xp, xt, zt = (torch.tensor(a).unsqueeze(0).expand(L, *a.shape)
                      for a in (X[gv["ind_pidx"]], X[gv["ind_tidx"]], Z1))
        e0 = lambda a, b: G.KernelAdapter(k0)(a, b).evaluate()     # [L, n1, n2]
        e1 = lambda a, b: G.KernelAdapter(k1)(a, b).evaluate()
        K0zz = e0(zt, zt) + eps * torch.eye(M)
        K0xz, K0Xz = e0(xp, zt), e0(xt, zt)
        A = torch.linalg.solve(K0zz, K0xz.transpose(1, 2))          # K0zz^-1 K0zx [L, M, n]
        Q = torch.linalg.solve(K0zz, K0Xz.transpose(1, 2))          # K0zz^-1 K0zX* [L, M, Nt]
        Kt = K0xz @ A + e1(xp, xp)
        kstar = K0xz @ Q + e1(xp, xt)
        kss = K0Xz @ Q + e1(xt, xt)
        n = xp.shape[1]
        cov = [dense_cov(Kt[l] + float(gv["ind_noise"][l]) * torch.eye(n), kstar[l], kss[l]) for l in range(L)]
    return torch.stack(cov).numpy()


if __name__ == "__main__":
    gv = np.load(os.path.join(G.OUT, "predict_var.npz"))
    out = dict(exact_cov=gen_exact(gv), ind_cov=gen_inducing(gv))
    for name in ("exact", "ind"):
        diag = np.diagonal(out[name + "_cov"], axis1=1, axis2=2).T          # [Nt, L]
        err = np.abs(diag - gv[name + "_var"]).max() / gv[name + "_prior"].max()
        print(f"{name}: diagonal against predict_var.npz {err:.2e}")
        assert err < 1e-12
    G.save("predict_cov.npz", **out)
