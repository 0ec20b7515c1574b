"""The driver over elbo_batched: one ElboStep (standard_training's 'GPapprox' branch) against the same step
assembled from the fp64 oracle, with fixed decoder and GP draws.

Bounds (test_dubo_step_vs_oracle's): the step's loss terms and raw kernel gradients 1e-4, network gradients 1e-3
(fp32 ConvVAE against the fp64 oracle)."""
import numpy as np
import pytest
import torch

import dubo_util as D
from oracle import lvae_oracle as O

pytestmark = pytest.mark.gpu
DEV = D.DEV


def test_elbo_step_vs_oracle(hip):
    """One ElboStep (P = 8, T = 8, L = 3, M = 12, S = 2, 'mse') against oracle.ConvVAE in fp64 with the same
    weights and oracle.gpapprox_elbo on Z_s = mu + eps_gp[s] exp(log_var / 2), assembled as training.py:499-575;
    then 'nll' for its loss terms."""
    import lvae_amd as la
    from lvae_amd.data import health_mnist_batch
    from lvae_amd.steps import ElboStep
    from lvae_amd.vae import ConvVAE
    L, P, T, M, S, weight = 3, 8, 8, 12, 2, 0.15
    img, mask, X = health_mnist_batch(P, T, seed=9, dtype=torch.float64)
    rng = np.random.default_rng(9)
    s0, s1 = O.spec_split(**D.CFG, id_covariate=2)
    raw0v = np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s0))))
    raw1v = np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s1))))
    Z = torch.stack([X[np.sort(np.random.default_rng(90 + l).choice(P * T, M, replace=False))] for l in range(L)])
    gen = torch.Generator().manual_seed(2)
    eps = torch.randn(P * T, L, generator=gen, dtype=torch.float64)
    eps_gp = torch.randn(S, P * T, L, generator=gen, dtype=torch.float64)

    def oracle_step(loss_function):
        ref = O.ConvVAE(L).double()
        ref.load_state_dict(O.vae_weights(ref, 23))
        raw0 = torch.tensor(raw0v, requires_grad=True)
        raw1 = torch.tensor(raw1v, requires_grad=True)
        mu, lv = ref.encode(img)
        recon = ref.decode(mu + eps * torch.exp(0.5 * lv))
        mse, nll = ref.loss_function(recon, img, mask)
        p0, p1 = O.constrain(raw0), O.constrain(raw1)
        gp = 0.0
        for s in range(S):
            Zs = mu + eps_gp[s] * torch.exp(0.5 * lv)
            for l in range(L):
                gp = gp - O.gpapprox_elbo(s0, p0[l], s1, p1[l], 1.0, X, Zs[:, l], Z[l], P, T, D.EPS)
        gp = gp / S
        if loss_function == "mse":
            gp = gp / L
            net = mse.sum() + weight * gp
        else:
            net = nll.sum() + gp
        net.backward()
        return ref, dict(net=net.detach(), recon=mse.sum().detach(), nll=nll.sum().detach(), gp=gp.detach(),
                         raw0=raw0.grad, raw1=raw1.grad)

    def hip_step(loss_function, ref):
        vae = ConvVAE(L, 1296, p_input=0.0, p=0.0).double()
        vae.load_state_dict(ref.state_dict())
        vae = vae.float().to(DEV)
        k0, k1 = la.generate_kernel_batched(L, **D.CFG, id_covariate=2)
        D.set_raw(k0, raw0v)
        D.set_raw(k1, raw1v)
        k0, k1 = k0.to(DEV), k1.to(DEV)
        lik = la.GaussianLikelihood(L, noise=1.0).to(DEV)
        opt = torch.optim.SGD(list(vae.parameters()) + list(k0.parameters()) + list(k1.parameters()), lr=0.0)
        step = ElboStep(vae, k0, k1, lik, opt, Z.to(DEV), T, weight=weight, loss_function=loss_function, eps=D.EPS,
                        num_samples=S)
        net, rl, nl, gp = step(img.float().to(DEV), mask.float().to(DEV), X.to(DEV), eps.float().to(DEV),
                               eps_gp.float().to(DEV))
        return vae, dict(net=net, recon=rl, nll=nl, gp=gp,
                         raw0=torch.stack([p.grad for _, p in k0.named_parameters()], 1),
                         raw1=torch.stack([p.grad for _, p in k1.named_parameters()], 1))
    for loss_function in ("mse", "nll"):
        ref, want = oracle_step(loss_function)
        vae, got = hip_step(loss_function, ref)
        errs = {k: D.rel(got[k], want[k]) for k in want}
        print(f"ElboStep {loss_function}:", {k: f"{e:.2e}" for k, e in errs.items()})
        for k, e in errs.items():
            assert e < 1e-4, (loss_function, k, e)
        if loss_function == "mse":
            for (name, p), (_, q) in zip(vae.named_parameters(), ref.named_parameters()):
                if q.grad is not None:   # (_log_vy has no gradient under loss='mse')
                    e = D.rel(p.grad, q.grad)
                    assert e < 1e-3, (name, e)
