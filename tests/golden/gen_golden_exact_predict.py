"""Generate tests/golden/exact_predict.npz by running the REFERENCE model_test.MSE_test (model_test.py:19-82) on
the CPU: the exact-GP test-set evaluation of a model trained with the exact KL.

Test infrastructure only, like gen_golden.py (whose shims and helpers it imports, and which it leaves as it is).
Further shims here: a ToTensor equivalent in the torchvision stub (MSE_test really transforms the images),
``torch.cholesky`` where torch no longer has it, and a ConvVAE subclass that draws the reparametrisation noise
from a stored array (MSE_test's first number goes through sample_latent) and records decode's input (Z_pred).

Inputs: the committed hmnist_tiny CSV trio as the test set; the reference ConvVAE (fp64, no dropout, eval) with
vae_weights(seed); per-dim GP_model kernels of a config with a covariate_missing_val mask (disease_time masked
by disease), hyper-parameters and noise randomised per dim; a prediction set of P x T = 20 x 15 rows.
The fixture holds inputs, raw hyper-parameters, noise, Z_pred and the two losses (data, not reference source).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_exact_predict.py
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the reference shims, sets the default dtype to fp64)

import torch  # noqa: E402

CFG = dict(cat_kernel=[2, 3], bin_kernel=[5], sqexp_kernel=[0],
           cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 2}, {'cont_covariate': 1, 'cat_covariate': 4}],
           bin_int_kernel=[], covariate_missing_val=[{'covariate': 1, 'mask': 4}], id_covariate=2)


def _to_tensor(pic):
    """torchvision.transforms.ToTensor on an [H, W, C] uint8 array: [C, H, W] fp32 in [0, 1]"""
    return torch.from_numpy(np.ascontiguousarray(pic.transpose(2, 0, 1))).to(torch.float32).div(255)


def gen_exact_predict(P, T, L, seed):
    sys.modules["torchvision"].transforms.ToTensor = lambda: _to_tensor
    if not hasattr(torch, "cholesky"):
        torch.cholesky = torch.linalg.cholesky
    import model_test as RM  # noqa: E402  (reference)
    rng = np.random.default_rng(seed)
    files = [str(f) for f in np.load(os.path.join(G.OUT, "hmnist_tiny.npz"))["files"]]
    root = os.path.join(G.OUT, "hmnist_tiny")

    class RecordingVAE(G.RV.ConvVAE):
        def sample_latent(self, mu, log_var):
            return mu + torch.tensor(self.eps) * torch.exp(0.5 * log_var)

        def decode(self, z):
            self.decoded.append(z.detach().numpy().copy())
            return super().decode(z)

    model = RecordingVAE(L, 1296, vy_init=1.0, p_input=0.0, p=0.0).double()
    model.load_state_dict(G.vae_weights(model, seed))
    model.eval()
    model.eps, model.decoded = rng.standard_normal((12, L)), []

    X = G.covariates(P, T, seed)
    mu = rng.standard_normal((P * T, L))
    noise = rng.uniform(0.5, 1.5, L)
    kernels, raws, names = [], [], None
    for _ in range(L):
        k0, k1 = G.R.generate_kernel_batched(1, CFG['cat_kernel'], CFG['bin_kernel'], CFG['sqexp_kernel'],
                                             CFG['cat_int_kernel'], CFG['bin_int_kernel'],
                                             CFG['covariate_missing_val'], CFG['id_covariate'])
        k = G.R.AdditiveKernel(list(k0.kernels) + list(k1.kernels))
        G.randomise(k, rng)
        names, vals = G.raw_params(k)
        raws.append(np.concatenate(vals))
        kernels.append(G.KernelAdapter(k))
    liks = [G.LikStub(torch.tensor([nz])) for nz in noise]
    with tempfile.TemporaryDirectory() as out:
        RM.MSE_test(files[0], files[1], files[2], root, 'conv', model, kernels, liks, out, L, torch.tensor(X),
                    torch.tensor(mu))
        losses = np.loadtxt(os.path.join(out, 'result_error.csv'))
    assert len(model.decoded) == 2   # forward's decode of the sampled latent, then decode(Z_pred)
    return dict(X=X, mu=mu, noise=noise, raw=np.stack(raws), param_names=np.array(names), eps=model.eps,
                Z_pred=model.decoded[1], losses=losses, L=L, seed=seed, files=np.array(files))


if __name__ == "__main__":
    G.save("exact_predict.npz", **gen_exact_predict(P=20, T=15, L=3, seed=23))
