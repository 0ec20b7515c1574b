"""The drivers over deviance_upper_bound_batched: validation_dubo with batched kernels, validate (lvae_amd.validation
and its drop-in module) on the tiny on-disk Health-MNIST set of tests/golden/hmnist_tiny (3 subjects x 4 rows), and
one DuboStep against the same step assembled from the fp64 oracle.

Bounds: DUBO values 1e-8 (test_gpu_dubo.py); validate's 'GPapprox' number is the same per-dim elbo calls on the same
seeded draw as the hand assembly, so 1e-12; the step's loss terms and raw kernel gradients 1e-4, network gradients
1e-3 (fp32 ConvVAE against the fp64 oracle, test_closed_step_vs_oracle's bounds)."""
import os
import sys

import numpy as np
import pytest
import torch

import abi_util as U
import dubo_util as D
from conftest import GOLDEN, PKG
from oracle import lvae_oracle as O

pytestmark = pytest.mark.gpu
DEV = D.DEV
DROPIN = os.path.join(PKG, "dropin")
TINY = os.path.join(GOLDEN, "hmnist_tiny")
FILES = ("tiny_data.csv", "tiny_labels.csv", "tiny_mask.csv")


def test_validation_dubo_batched_kernels(hip):
    """validation_dubo with L = 3 batched kernels == the sum of the per-dim composed values; [1] like the reference"""
    import lvae_amd as la
    cid = "6x7x33"
    c = D.problem(cid)
    k0, k1, lik = D.modules_batched(c)
    got = la.validation_dubo(D.L, k0, k1, lik, c["X"].to(DEV), c["mu"].to(DEV), c["lv"].to(DEV), c["Z"].to(DEV),
                             c["P"], c["T"], D.EPS)
    assert got.shape == (1,) and got.dtype == torch.float64
    want = D.composed(cid)["dubo"].sum()
    err = D.rel(got[0], want)
    print(f"validation_dubo: {float(got[0].detach()):.12e} composed sum {float(want):.12e} err {err:.2e}")
    assert err < 1e-8


def _tiny_setup(L=2, M=5, seed=3):
    import lvae_amd as la
    from lvae_amd.data import HealthMNISTDatasetConv
    from lvae_amd.vae import ConvVAE
    ref = O.ConvVAE(L).double()
    ref.load_state_dict(O.vae_weights(ref, seed))
    vae = ConvVAE(L, 1296, p_input=0.0, p=0.0).double()
    vae.load_state_dict(ref.state_dict())
    vae = vae.float().to(DEV).eval()
    ds = HealthMNISTDatasetConv(*FILES, TINY, device=DEV)
    rng = np.random.default_rng(seed)
    s0, s1 = O.spec_split(**D.CFG, id_covariate=2)
    raw0 = np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s0))))
    raw1 = np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s1))))
    noise = np.array([0.8, 1.1])[:L]
    kb0, kb1 = la.generate_kernel_batched(L, **D.CFG, id_covariate=2)
    D.set_raw(kb0, raw0)
    D.set_raw(kb1, raw1)
    likb = la.GaussianLikelihood(L, noise=1.0)
    likb.noise = torch.tensor(noise)
    k0s, k1s, liks = [], [], []
    for l in range(L):
        a, b = la.generate_kernel_approx(**D.CFG, id_covariate=2)
        D.set_raw(a, raw0[l:l + 1])
        D.set_raw(b, raw1[l:l + 1])
        k0s.append(a.to(DEV))
        k1s.append(b.to(DEV))
        liks.append(la.GaussianLikelihood(1, noise=float(noise[l])).to(DEV))
    labels = ds.batch(torch.arange(len(ds)))["label"].to(torch.float64)
    z = torch.stack([labels[np.sort(np.random.default_rng(seed + l).choice(len(ds), M, replace=False))]
                     for l in range(L)])
    return dict(L=L, vae=vae, ds=ds, batched=(kb0.to(DEV), kb1.to(DEV), likb.to(DEV)), lists=(k0s, k1s, liks), z=z,
                labels=labels, P=3, T=4)


def _by_hand(s, type_KL, num_samples, seed):
    """(recon sum, nll sum, GP loss summed over the dims) as validate forms them: VAEtest-style losses over the whole
    set as one batch and the per-dim deviance_upper_bound / elbo"""
    import lvae_amd as la
    from lvae_amd.evaluation import _whole_set
    k0s, k1s, liks = s["lists"]
    with torch.no_grad():
        torch.manual_seed(seed)
        images, mask, labels = _whole_set(s["ds"], s["vae"])
        recon, mu, lv = s["vae"](images)
        mse, nll = s["vae"].loss_function(recon, images, mask)
        mu, lv = mu.double(), lv.double()
        gp = 0.0
        if type_KL == "GPapprox_closed":
            for l in range(s["L"]):
                gp += float(la.deviance_upper_bound(k0s[l], k1s[l], liks[l], labels, mu[:, l], lv[:, l], s["z"][l],
                                                    s["P"], s["T"], D.EPS))
        else:
            for _ in range(num_samples):
                Z = s["vae"].sample_latent(mu, lv)
                for l in range(s["L"]):
                    gp -= float(la.elbo(k0s[l], k1s[l], liks[l], labels, Z[:, l], s["z"][l], s["P"], s["T"], D.EPS))
            gp /= num_samples
    return float(mse.sum()), float(nll.sum()), gp


def test_validate_tiny_dataset(hip):
    sys.path.insert(0, DROPIN)
    try:
        sys.modules.pop("validation", None)
        import validation as V
    finally:
        sys.path.remove(DROPIN)
    import lvae_amd as la
    from lvae_amd.validation import validate
    assert V.validate is validate and V.validation_dubo is la.validation_dubo
    s = _tiny_setup()
    L, T, weight, seed = s["L"], s["T"], 0.15, 11
    zl = [zi for zi in s["z"]]

    def run(mods, z, type_KL, loss, ns=1):
        torch.manual_seed(seed)
        out = V.validate(s["vae"], "conv", s["ds"], type_KL, ns, L, *mods, z, T, weight, None, None, 2, loss,
                         eps=D.EPS)
        assert isinstance(out, float)
        return out
    rec, nll, gp = _by_hand(s, "GPapprox_closed", 1, seed)
    want = dict(mse=weight * gp / L + rec, nll=gp + nll)
    for loss in ("mse", "nll"):
        for name, mods, z in (("lists", s["lists"], zl), ("batched", s["batched"], s["z"])):
            got = run(mods, z, "GPapprox_closed", loss)
            err = abs(got - want[loss]) / abs(want[loss])
            print(f"validate GPapprox_closed {loss} {name}: {got:.12e} by hand {want[loss]:.12e} err {err:.2e}")
            assert err < 1e-8
    rec, nll, gp = _by_hand(s, "GPapprox", 2, seed)
    want = dict(mse=weight * gp / L + rec, nll=gp + nll)
    for loss in ("mse", "nll"):
        got = run(s["lists"], zl, "GPapprox", loss, ns=2)
        err = abs(got - want[loss]) / abs(want[loss])
        print(f"validate GPapprox {loss}: {got:.12e} by hand {want[loss]:.12e} err {err:.2e}")
        assert err < 1e-12


def test_dubo_step_vs_oracle(hip):
    """One DuboStep (P = 8, T = 8, L = 3, M = 12, 'mse') against oracle.ConvVAE in fp64 with the same weights and
    oracle.deviance_upper_bound, assembled as training.py:499-575; then 'nll' for its loss terms."""
    import lvae_amd as la
    from lvae_amd.data import health_mnist_batch
    from lvae_amd.steps import DuboStep
    from lvae_amd.vae import ConvVAE
    L, P, T, M, weight = 3, 8, 8, 12, 0.15
    img, mask, X = health_mnist_batch(P, T, seed=9, dtype=torch.float64)
    rng = np.random.default_rng(9)
    s0, s1 = O.spec_split(**D.CFG, id_covariate=2)
    raw0v = np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s0))))
    raw1v = np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s1))))
    Z = torch.stack([X[np.sort(np.random.default_rng(90 + l).choice(P * T, M, replace=False))] for l in range(L)])
    eps = torch.randn(P * T, L, generator=torch.Generator().manual_seed(2), dtype=torch.float64)

    def oracle_step(loss_function):
        ref = O.ConvVAE(L).double()
        ref.load_state_dict(O.vae_weights(ref, 23))
        raw0 = torch.tensor(raw0v, requires_grad=True)
        raw1 = torch.tensor(raw1v, requires_grad=True)
        mu, lv = ref.encode(img)
        recon = ref.decode(mu + eps * torch.exp(0.5 * lv))
        mse, nll = ref.loss_function(recon, img, mask)
        p0, p1 = O.constrain(raw0), O.constrain(raw1)
        gp = sum(O.deviance_upper_bound(s0, p0[l], s1, p1[l], 1.0, X, mu[:, l], lv[:, l], Z[l], P, T, D.EPS)
                 for l in range(L))
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
        step = DuboStep(vae, k0, k1, lik, opt, Z.to(DEV), T, weight=weight, loss_function=loss_function, eps=D.EPS)
        net, rl, nl, gp = step(img.float().to(DEV), mask.float().to(DEV), X.to(DEV), eps.float().to(DEV))
        return vae, dict(net=net, recon=rl, nll=nl, gp=gp,
                         raw0=torch.stack([p.grad for _, p in k0.named_parameters()], 1),
                         raw1=torch.stack([p.grad for _, p in k1.named_parameters()], 1))
    for loss_function in ("mse", "nll"):
        ref, want = oracle_step(loss_function)
        vae, got = hip_step(loss_function, ref)
        errs = {k: D.rel(got[k], want[k]) for k in want}
        print(f"DuboStep {loss_function}:", {k: f"{e:.2e}" for k, e in errs.items()})
        for k, e in errs.items():
            assert e < 1e-4, (loss_function, k, e)
        if loss_function == "mse":
            for (name, p), (_, q) in zip(vae.named_parameters(), ref.named_parameters()):
                if q.grad is not None:   # (_log_vy has no gradient under loss='mse')
                    e = D.rel(p.grad, q.grad)
                    assert e < 1e-3, (name, e)
