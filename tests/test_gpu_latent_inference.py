"""LatentInferenceStep / infer_new_subjects (the second half of variational_inference_optimization,
training.py:688-749) against the same loop with the GP term taken from deviance_upper_bound_batched on the joint
batch -- the only route there was before condition_dubo."""
import numpy as np
import pytest
import torch

import abi_util as U
import dubo_cond_util as C
import dubo_util as D
from oracle import lvae_oracle as O

pytestmark = pytest.mark.gpu
DEV = C.DEV


class StubVAE(torch.nn.Module):
    """a deterministic fp64 model with the four methods the step uses: a linear encoder, a two-layer MLP decoder"""

    def __init__(self, L, D_img, H=16, seed=3):
        super().__init__()
        self.L = L
        self.enc = torch.nn.Linear(D_img, 2 * L)
        self.fc1, self.fc2 = torch.nn.Linear(L, H), torch.nn.Linear(H, D_img)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
        self.double()

    def encode(self, x):
        h = self.enc(x.reshape(x.shape[0], -1))
        return h[:, :self.L], 0.1 * h[:, self.L:]

    def sample_latent(self, mu, log_var, eps=None):
        eps = torch.randn_like(mu) if eps is None else eps
        return mu + eps * torch.exp(0.5 * log_var)

    def decode(self, z):
        return torch.sigmoid(self.fc2(torch.tanh(self.fc1(z))))

    def loss_function(self, recon, x, mask):
        se = (recon - x.reshape(recon.shape)) ** 2 * mask.reshape(recon.shape)
        return se.sum(1) / mask.reshape(recon.shape).sum(1), 0.5 * se.sum(1) + 0.1


def _joint_gp(c, k0, k1, lik, z, xn, xt, mt, lt):
    import lvae_amd as la
    x = torch.cat([xn, xt])
    return lambda mu, lv: la.deviance_upper_bound_batched(C.L, k0, k1, lik, x, torch.cat([mu, mt]),
                                                          torch.cat([lv, lt]), z, c["P"], c["T"], C.EPS)


def _setup(cid):
    c = C.problem(cid)
    k0, k1, lik = D.modules_batched(c)
    z = c["Z"].to(DEV)
    keep = torch.ones(c["N"], dtype=torch.bool)
    keep[c["rows"]] = False
    xn, xt, mt, lt = (t.to(DEV) for t in (c["X"][c["rows"]], c["X"][keep], c["mu"][keep], c["lv"][keep]))
    return c, k0, k1, lik, z, xn, xt, mt, lt


def test_infer_new_subjects_matches_the_joint_loop(hip):
    import lvae_amd as la
    from lvae_amd.steps import infer_new_subjects
    iters, weight, D_img = 5, 0.15, 20
    c, k0, k1, lik, z, xn, xt, mt, lt = _setup("6x7x33")
    Nn = c["Nn"]
    g = torch.Generator().manual_seed(11)
    img = torch.rand(Nn, D_img, generator=g, dtype=torch.float64).to(DEV)
    mask = (torch.rand(Nn, D_img, generator=g) < 0.8).double().to(DEV)
    mask[:, 0] = 1.0
    eps = torch.randn(iters, Nn, C.L, generator=g, dtype=torch.float64).to(DEV)
    vae = StubVAE(C.L, D_img).to(DEV)
    cond = la.condition_dubo(C.L, k0, k1, lik, xn, xt, mt, lt, z, c["T"], C.EPS)
    mu, lv, losses = infer_new_subjects(vae, cond, img, mask, iters=iters, weight=weight, eps=eps)
    assert isinstance(mu, torch.nn.Parameter) and mu.dtype == torch.float64 and tuple(losses.shape) == (iters, 4)
    # the same loop, the GP term from the joint batch
    gp_joint = _joint_gp(c, k0, k1, lik, z, xn, xt, mt, lt)
    with torch.no_grad():
        m0, l0 = vae.encode(img)
    mr, lr_ = torch.nn.Parameter(m0.clone()), torch.nn.Parameter(l0.clone())
    opt = torch.optim.Adam([{"params": mr}, {"params": lr_}], lr=1e-3)
    ref = []
    for it in range(iters):
        opt.zero_grad()
        mse, nll = vae.loss_function(vae.decode(vae.sample_latent(mr, lr_, eps[it])), img, mask)
        gp = gp_joint(mr, lr_).sum() / C.L
        net = mse.sum() + weight * gp
        mr.grad, lr_.grad = torch.autograd.grad(net, (mr, lr_))
        opt.step()
        ref.append(torch.stack([net, mse.sum(), nll.sum(), gp]).detach())
    ref = torch.stack(ref)
    errs = dict(mu=U.rel(mu, mr), log_var=U.rel(lv, lr_), **{f"loss{k}": U.rel(losses[:, k], ref[:, k]) for k in range(4)})
    print(errs, "moved:", U.rel(mu, m0))
    assert float((mu.detach() - m0).abs().max()) > 1e-3      # the loop did move the latents
    assert all(e <= 1e-7 for e in errs.values()), errs


def test_step_with_the_conv_vae(hip):
    """one forward_backward of each route on the fp32 ConvVAE with the same eps: mu.grad / log_var.grad to 2e-4 (the
    bound of the whole-step network gradients), the network untouched; 'nll' divides the GP term by L too"""
    import lvae_amd as la
    from lvae_amd.data import health_mnist_batch
    from lvae_amd.steps import LatentInferenceStep
    from lvae_amd.vae import ConvVAE
    L, P, T, Pn, M = C.L, 7, 4, 3, 10
    Nn, N = Pn * T, P * T
    img, mask, X = health_mnist_batch(P, T, seed=9, dtype=torch.float64)
    rng = np.random.default_rng(9)
    s0, s1 = O.spec_split(**D.CFG, id_covariate=2)
    k0, k1, lik = D.modules_batched(dict(raw0=np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s0)))),
                                         raw1=np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s1)))),
                                         noise=0.8 * np.array([1.0, 1.25, 1.5])))
    z = torch.stack([X[np.sort(np.random.default_rng(90 + l).choice(N, M, replace=False))] for l in range(L)]).to(DEV)
    gen = torch.Generator().manual_seed(9)
    mj = torch.randn(N, L, generator=gen, dtype=torch.float64).to(DEV)
    lj = (0.1 * torch.randn(N, L, generator=gen, dtype=torch.float64)).to(DEV)
    x = X.to(DEV)
    img, mask = img[:Nn].float().to(DEV), mask[:Nn].float().to(DEV)      # the images of the Pn new subjects
    xn, xt, mt, lt = x[:Nn], x[Nn:], mj[Nn:], lj[Nn:]
    ref = O.ConvVAE(L).double()
    ref.load_state_dict(O.vae_weights(ref, 23))
    vae = ConvVAE(L, 1296, p_input=0.0, p=0.0).double()
    vae.load_state_dict(ref.state_dict())
    vae = vae.float().to(DEV).eval()
    for p in vae.parameters():
        p.grad = torch.full_like(p, 0.5)
    before = [(p.detach().clone(), p.grad.clone()) for p in vae.parameters()]
    cond = la.condition_dubo(L, k0, k1, lik, xn, xt, mt, lt, z, T, C.EPS)
    eps = torch.randn(Nn, L, generator=torch.Generator().manual_seed(2)).to(DEV)
    mu0, lv0 = mj[:Nn].clone(), lj[:Nn].clone()
    out = {}
    for loss_function in ("mse", "nll"):
        mu, lv = torch.nn.Parameter(mu0.clone()), torch.nn.Parameter(lv0.clone())
        step = LatentInferenceStep(vae, cond, mu, lv, torch.optim.SGD([mu, lv], lr=0.0), weight=0.15,
                                   loss_function=loss_function)
        net, rl, nl, gp = step.forward_backward(img, mask, eps)
        mr, lr_ = mu0.clone().requires_grad_(), lv0.clone().requires_grad_()
        mse, nll = vae.loss_function(vae.decode(vae.sample_latent(mr.float(), lr_.float(), eps)), img, mask)
        gpr = la.deviance_upper_bound_batched(L, k0, k1, lik, x, torch.cat([mr, mt]), torch.cat([lr_, lt]), z, P, T,
                                              C.EPS).sum() / L
        netr = mse.sum() + 0.15 * gpr if loss_function == "mse" else nll.sum() + gpr
        gm, gl = torch.autograd.grad(netr, (mr, lr_))
        errs = dict(dmu=U.rel(mu.grad, gm), dlv=U.rel(lv.grad, gl), net=U.rel(net, netr), gp=U.rel(gp, gpr))
        print(loss_function, errs)
        assert mu.grad.dtype == torch.float64 and all(e <= 2e-4 for e in errs.values()), errs
        out[loss_function] = (net, nl, gp)
    net, nl, gp = out["nll"]
    full = la.deviance_upper_bound_batched(L, k0, k1, lik, x, mj, lj, z, P, T, C.EPS).sum()
    assert U.rel(gp, full / L) < 1e-7 and U.rel(net, nl.double() + full / L) < 2e-4
    for p, (w, g) in zip(vae.parameters(), before):
        assert U.bit_equal(p.detach(), w) and U.bit_equal(p.grad, g)
