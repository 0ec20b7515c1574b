"""predict_exact and the drop-in model_test module against tests/golden/exact_predict.npz, the reference's own
MSE_test (model_test.py:19-82) run on the CPU by tests/golden/gen_golden_exact_predict.py: the hmnist_tiny CSV trio
as the test set, a prediction set of 300 rows, L = 3 per-dim kernels of a config with a covariate_missing_val mask.

Z_pred: the project's tolerance rule, min(max(10 x yardstick, 2e-12), 1e-6), yardstick = the larger of the fp64
oracle's change under a relative 2^-50 perturbation of hyper-parameters, noise and mu and its CPU / device spread
(the oracle itself is pinned to the golden at 1e-12 on the CPU: the reference multiplies by the explicit inverse,
the oracle solves).
"""
import os
import sys

import numpy as np
import pytest
import torch

import abi_util as U
from conftest import GOLDEN, ROOT, golden
from oracle import lvae_oracle as O
from test_gpu_predict_exact_abi import solve_oracle

gpu = pytest.mark.gpu
DEV = "cuda"
DROPIN = os.path.join(ROOT, "longitudinal-vae_amd", "dropin")
CFG = dict(cat_kernel=[2, 3], bin_kernel=[5], sqexp_kernel=[0],
           cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 2}, {'cont_covariate': 1, 'cat_covariate': 4}],
           bin_int_kernel=[], covariate_missing_val=[{'covariate': 1, 'mask': 4}])


def spec():
    s0, s1 = O.spec_split(**CFG, id_covariate=2)
    return s0 + s1   # the fixture's per-dim kernel: non-id components, then id components


def tiny_batch():
    from lvae_amd.data import HealthMNISTDatasetConv
    g = golden("exact_predict.npz")
    fd, fl, fm = (str(f) for f in g["files"])
    ds = HealthMNISTDatasetConv(fd, fl, fm, os.path.join(GOLDEN, "hmnist_tiny"))
    return ds, ds.batch(torch.arange(len(ds)))


def oracle_zpred(g, dev="cpu", perturb=False):
    v = dict(params=O.constrain(torch.tensor(g["raw"])), noise=torch.tensor(g["noise"]), mu=torch.tensor(g["mu"]))
    if perturb:
        gen = torch.Generator().manual_seed(80)
        v = {k: U.perturbed(t, gen) for k, t in v.items()}
    tx = tiny_batch()[1]["label"].to(torch.float64)
    return solve_oracle(spec(), v["params"].to(dev), v["noise"].to(dev), torch.tensor(g["X"]).to(dev), tx.to(dev),
                        v["mu"].to(dev)).cpu()


def test_oracle_matches_reference_zpred():
    g = golden("exact_predict.npz")
    assert O.n_params(spec()) == g["raw"].shape[1] and g["Z_pred"].shape == (12, int(g["L"]))
    assert U.rel(oracle_zpred(g), torch.tensor(g["Z_pred"])) < 1e-12


def kernels(g, batched):
    """The fixture's kernels as the project's modules on the device: one batched module or a per-dim list"""
    import lvae_amd as la
    L = int(g["L"])

    def build(latent_dim, raw):
        k0, k1 = la.generate_kernel_batched(latent_dim, **CFG, id_covariate=2)
        k = (k0 + k1).double()
        assert [n.split(".")[-1] for n, _ in k.named_parameters()] == [str(n).split(".")[-1] for n in g["param_names"]]
        with torch.no_grad():   # raw [latent_dim, P] in named_parameters order
            for j, (_, p) in enumerate(k.named_parameters()):
                p.copy_(torch.as_tensor(raw[:, j], dtype=p.dtype))
        return k.to(DEV)
    if batched:
        return build(L, g["raw"]), L
    return [build(1, g["raw"][l:l + 1]) for l in range(L)], L


def likelihoods(g, batched):
    import lvae_amd as la
    L = int(g["L"])
    liks = [la.GaussianLikelihood(1, noise=float(g["noise"][l])).to(DEV) for l in range(L)]
    if not batched:
        return liks

    class Lik:   # a batched likelihood: .noise [L]
        noise = torch.tensor(g["noise"], device=DEV)

        def eval(self):
            return self
    return Lik()


@gpu
@pytest.mark.parametrize("batched", [False, True])
def test_predict_exact_matches_reference(hip, batched):
    import lvae_amd as la
    g = golden("exact_predict.npz")
    k, L = kernels(g, batched)
    tx = tiny_batch()[1]["label"].to(DEV, torch.float64)
    got = la.predict_exact(k, likelihoods(g, batched), torch.tensor(g["X"], device=DEV), tx,
                           torch.tensor(g["mu"], device=DEV))
    assert got.shape == (12, L) and got.dtype == torch.float64
    ref = oracle_zpred(g)
    yard = max(U.rel(oracle_zpred(g, perturb=True), ref), U.rel(oracle_zpred(g, DEV), ref))
    tol = min(max(10.0 * yard, 2e-12), 1e-6)
    err = U.rel(got, torch.tensor(g["Z_pred"]))
    print(f"predict_exact golden batched={batched}: err {err:.2e} yardstick {yard:.2e} bound {tol:.1e}")
    assert err <= tol


@gpu
def test_dim_groups_give_the_same_bits(hip):
    """A max_workspace_bytes that holds one dim's workspace but not two forces >= 2 groups at L = 3."""
    import lvae_amd as la
    g = golden("exact_predict.npz")
    k, L = kernels(g, True)
    lik = likelihoods(g, True)
    X, mu = torch.tensor(g["X"], device=DEV), torch.tensor(g["mu"], device=DEV)
    tx = tiny_batch()[1]["label"].to(DEV, torch.float64)
    one = la.predict_exact(k, lik, X, tx, mu)
    size = lambda n_dims: int(hip.lvae_predict_exact_workspace_size(X.shape[0], tx.shape[0], n_dims))
    assert size(1) < size(2) < size(3)
    for cap in (size(1), size(2)):
        assert U.bit_equal(la.predict_exact(k, lik, X, tx, mu, max_workspace_bytes=cap), one)


@gpu
def test_indefinite_dim_raises(hip):
    import lvae_amd as la
    g = golden("exact_predict.npz")
    k, L = kernels(g, True)
    X, mu = torch.tensor(g["X"], device=DEV), torch.tensor(g["mu"], device=DEV)
    tx = tiny_batch()[1]["label"].to(DEV, torch.float64)

    class Lik:
        noise = torch.tensor(g["noise"], device=DEV)
        noise[1] = -100.0   # below -(K's diagonal): dim 1 is indefinite

        def eval(self):
            return self
    with pytest.raises(torch.linalg.LinAlgError):
        la.predict_exact(k, Lik(), X, tx, mu)


def fixed_eps_vae(g, dtype, device):
    """The project's ConvVAE with the fixture's weights and its stored reparametrisation noise"""
    from lvae_amd.vae import ConvVAE

    class FixedEps(ConvVAE):
        decoded = ()   # every decode input, in call order

        def sample_latent(self, mu, log_var, eps=None):
            return super().sample_latent(mu, log_var, torch.tensor(g["eps"], dtype=mu.dtype, device=mu.device))

        def decode(self, z):
            self.decoded = (*self.decoded, z.detach().clone())
            return super().decode(z)
    L = int(g["L"])
    ref = O.ConvVAE(L).double()
    ref.load_state_dict(O.vae_weights(ref, int(g["seed"])))
    vae = FixedEps(L, p_input=0.0, p=0.0)
    vae.load_state_dict(ref.state_dict())
    return vae.to(device, dtype).eval()


def oracle_losses(g, dtype):
    """The two numbers of result_error.csv from the oracle ConvVAE in `dtype` on the CPU, given the golden Z_pred"""
    L = int(g["L"])
    vae = O.ConvVAE(L).double()
    vae.load_state_dict(O.vae_weights(vae, int(g["seed"])))
    vae = vae.to(dtype)
    b = tiny_batch()[1]
    data, mask = b["digit"].to(dtype), b["mask"].reshape(12, -1).to(dtype)
    with torch.no_grad():
        mu, lv = vae.encode(data)
        z = mu + torch.tensor(g["eps"], dtype=dtype) * torch.exp(0.5 * lv)
        a = vae.loss_function(vae.decode(z), data, mask)[0].mean()
        b_ = vae.loss_function(vae.decode(torch.tensor(g["Z_pred"], dtype=dtype)), data, mask)[0].mean()
    return np.array([float(a), float(b_)])


def test_oracle_vae_reproduces_reference_losses():
    g = golden("exact_predict.npz")
    assert np.abs(oracle_losses(g, torch.float64) - g["losses"]).max() < 1e-12


@gpu
def test_dropin_mse_test(hip, tmp_path):
    """Drop-in MSE_test on the tiny CSV trio writes result_error.csv with the golden's two numbers.  Bound: ten
    times the spread between the oracle ConvVAE in float32 and in float64 on the CPU on the same inputs (the
    project's network is fp32, the reference's fp64).  Measured spread on the CPU: 3.7e-09 (first number 3.7e-09,
    second 1.6e-09), so the bound is 3.7e-08 on numbers of 0.0933 and 0.0851."""
    sys.path.insert(0, DROPIN)
    try:
        sys.modules.pop("model_test", None)
        import model_test as MT
    finally:
        sys.path.remove(DROPIN)
    g = golden("exact_predict.npz")
    k, L = kernels(g, False)
    vae = fixed_eps_vae(g, torch.float32, DEV)
    fd, fl, fm = (str(f) for f in g["files"])
    MT.MSE_test(fd, fl, fm, os.path.join(GOLDEN, "hmnist_tiny"), 'conv', vae, k, likelihoods(g, False), str(tmp_path),
                L, torch.tensor(g["X"]), torch.tensor(g["mu"]))
    got = np.loadtxt(tmp_path / "result_error.csv")
    spread = float(np.abs(oracle_losses(g, torch.float32) - oracle_losses(g, torch.float64)).max())
    err = np.abs(got - g["losses"])
    print(f"MSE_test: got {got} golden {g['losses']} err {err} fp32/fp64 oracle spread {spread:.2e}")
    assert got.shape == (2,) and spread > 0
    assert float(err.max()) <= 10.0 * spread


@gpu
def test_dropin_mse_test_gpapprox(hip, tmp_path):
    """MSE_test_GPapprox runs on the same files and decodes batch_predict_varying_T's Z_pred."""
    import lvae_amd as la
    from lvae_amd.evaluation import MSE_test_GPapprox
    g = golden("exact_predict.npz")
    L = int(g["L"])
    cfg = dict(CFG, covariate_missing_val=[])
    k0, k1 = la.generate_kernel_batched(L, **cfg, id_covariate=2)
    k0, k1 = k0.double().to(DEV), k1.double().to(DEV)
    lik = la.GaussianLikelihood(L, noise=1.0).to(DEV)
    X, mu = torch.tensor(g["X"], device=DEV), torch.tensor(g["mu"], device=DEV)
    z = X[::30].clone().unsqueeze(0).expand(L, -1, -1).contiguous()
    vae = fixed_eps_vae(g, torch.float32, DEV)
    fd, fl, fm = (str(f) for f in g["files"])
    assert MSE_test_GPapprox(fd, fl, fm, os.path.join(GOLDEN, "hmnist_tiny"), 'conv', vae, k0, k1, lik,
                             str(tmp_path), L, X, mu, z, 20, 15, 2, varying_T=True, save_file='approx.csv') is None
    tx = tiny_batch()[1]["label"].to(DEV, torch.float64)
    want = la.batch_predict_varying_T(L, k0, k1, lik, X, tx, mu, z, 2, eps=1e-6)
    assert len(vae.decoded) == 2 and U.bit_equal(vae.decoded[1], want.to(torch.float32))   # decode(Z_pred)
    got = np.loadtxt(tmp_path / "approx.csv")
    assert got.shape == (2,) and bool(np.isfinite(got).all())
    from lvae_amd.data import HealthMNISTDatasetConv
    from lvae_amd.evaluation import VAEtest
    ds = HealthMNISTDatasetConv(fd, fl, fm, os.path.join(GOLDEN, "hmnist_tiny"), device=DEV)
    assert abs(VAEtest(ds, vae, 'conv', 2) - got[0]) <= 1e-7   # the autoencoder's own number, same noise
