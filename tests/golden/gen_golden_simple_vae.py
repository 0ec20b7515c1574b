"""Generate tests/golden/simple_vae.npz and tests/golden/physionet_tiny.npz by running the REFERENCE code:

  simple_vae.npz      VAE.SimpleVAE(L = 3, D = 11, 1.0, False) in fp64 (VAE.py:165-273) with the weights of
                      gen_golden.vae_weights (a numpy formula: regenerable from the seed), B = 35 rows, one of them
                      with an all-zero mask, a fixed eps;  loss = sum mse + 0.3 sum nll + 0.1 sum mu^2
                      + 0.05 sum log_var (the last two stand in for the GP bound's gradient on mu / log_var);
                      holds the inputs, the state_dict's key names, mu, log_var, recon, mse, nll, the loss and the
                      gradient of every parameter.
  physionet_tiny.npz  a Physionet-format file (data_readings, outcome_attrib, data_mask, outcome_mask;
                      P = 3 subjects x T = 4 rows, D = 5 readings, 10 outcome attributes) and, beside them, the
                      items dataset_def.PhysionetDataset (dataset_def.py:8-44) returns on its FIRST access of
                      each row (it subtracts 24 from its source again at every access).

Test infrastructure only, like gen_golden.py (whose shims and helpers it imports, and which it leaves as it is).
The fixtures hold data, not reference source.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_simple_vae.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the reference shims, sets the default dtype to fp64)

import torch  # noqa: E402

SEED, L, D, B, ZERO_ROW = 61, 3, 11, 35, 17


def gen_simple_vae():
    rng = np.random.default_rng(SEED)
    model = G.RV.SimpleVAE(L, D, 1.0, False).double()
    model.load_state_dict(G.vae_weights(model, SEED))
    x = rng.uniform(0, 1, (B, D))
    mask = rng.binomial(1, 0.75, (B, D)).astype(np.float64)
    mask[ZERO_ROW] = 0.0
    eps = rng.standard_normal((B, L))
    xt = torch.tensor(x)
    mu, logv = model.encode(xt)
    recon = model.decode(mu + torch.tensor(eps) * torch.exp(0.5 * logv))
    mse, nll = model.loss_function(recon, xt, torch.tensor(mask))
    loss = mse.sum() + 0.3 * nll.sum() + 0.1 * (mu ** 2).sum() + 0.05 * logv.sum()
    loss.backward()
    names = list(model.state_dict().keys())
    grads = {"g_" + n: p.grad.numpy().copy() for n, p in model.named_parameters()}
    return dict(x=x, mask=mask, eps=eps, L=L, D=D, seed=SEED, zero_row=ZERO_ROW, keys=np.array(names),
                mu=mu.detach().numpy(), logv=logv.detach().numpy(), recon=recon.detach().numpy(),
                mse=mse.detach().numpy(), nll=nll.detach().numpy(), loss=loss.item(), **grads)


def gen_physionet_tiny():
    import dataset_def as RD  # noqa: E402  (reference)
    rng = np.random.default_rng(SEED + 1)
    P, T, Dp, Qa = 3, 4, 5, 10
    src = dict(data_readings=rng.uniform(0, 1, (P, T, Dp)).astype(np.float32).astype(np.float64),
               outcome_attrib=np.round(rng.uniform(0, 60, (P, T, Qa))),
               data_mask=rng.binomial(1, 0.7, (P, T, Dp)).astype(np.float64),
               outcome_mask=rng.binomial(1, 0.8, (P, T, Qa)).astype(np.float64))
    G.save("physionet_tiny.npz", **src)
    ds = RD.PhysionetDataset("physionet_tiny.npz", G.OUT)
    items = [ds[i] for i in range(len(ds))]  # the first access of every row
    return dict(src, item_data=np.stack([it["data"].numpy() for it in items]),
                item_label=np.stack([it["label"].numpy() for it in items]),
                item_mask=np.stack([it["mask"] for it in items]), n=len(ds))


if __name__ == "__main__":
    G.save("simple_vae.npz", **gen_simple_vae())
    G.save("physionet_tiny.npz", **gen_physionet_tiny())
