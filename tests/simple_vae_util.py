"""Helpers of the SimpleVAE tests (test_simple_vae_cpu.py, test_gpu_simple_vae.py, test_gpu_mlp_vae_abi.py): the
weights' numpy formula (tests/golden/gen_golden.py:vae_weights), the loss the fixture differentiates, and the fp64 CPU
reference of a case, computed once per case and shared.

The reference is lvae_amd.SimpleVAE in fp64 on the CPU (its 'stock' route: plain torch ops), which
tests/golden/simple_vae.npz pins to the reference implementation at 1e-12.  Inputs and weights of the generated cases
are rounded to fp32 first, so the fp32 run starts from exactly the reference's numbers.
"""
import functools
import math

import numpy as np
import torch

DEV = "cuda"
TOL = 1e-4   # of each tensor's max-abs: the project's fp32 bar


def weights(model, seed, fp32_exact=False):
    """The state dict of gen_golden.vae_weights for ``model`` (fp64); fp32_exact: rounded to fp32 values"""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, p in model.state_dict().items():
        if name == "min_log_vy":
            sd[name] = p.clone()
            continue
        if name == "_log_vy":
            v = 0.1 * rng.standard_normal(tuple(p.shape))
        else:
            fan = p[0].numel() if p.dim() > 1 else p.numel()
            v = rng.standard_normal(tuple(p.shape)) / math.sqrt(max(fan, 1))
        sd[name] = torch.tensor(v.astype(np.float32).astype(np.float64) if fp32_exact else v)
    return sd


def loss_of(model, x, mask, eps):
    """(loss, outputs): sum mse + 0.3 sum nll + 0.1 sum mu^2 + 0.05 sum log_var -- the last two stand in for the GP
    bound's gradient on (mu, log_var)"""
    recon, mu, lv = model(x, eps)
    mse, nll = model.loss_function(recon, x, mask)
    loss = mse.sum() + 0.3 * nll.sum() + 0.1 * (mu ** 2).sum() + 0.05 * lv.sum()
    return loss, dict(mu=mu, logv=lv, recon=recon, mse=mse, nll=nll)


def inputs(B, D, L, seed):
    """(x, mask, eps) fp64 with fp32-exact values; row B // 2 has an all-zero mask (B > 1)"""
    rng = np.random.default_rng(seed)
    f = lambda a: torch.tensor(a.astype(np.float32).astype(np.float64))
    mask = rng.binomial(1, 0.75, (B, D)).astype(np.float64)
    if B > 1:
        mask[B // 2] = 0.0
    return f(rng.uniform(0, 1, (B, D))), torch.tensor(mask), f(rng.standard_normal((B, L)))


def build(L, D, hidden, seed):
    """lvae_amd.SimpleVAE in fp64 on the CPU with the formula's fp32-exact weights"""
    import lvae_amd as la
    model = la.SimpleVAE(L, D, hidden=hidden).double()
    model.load_state_dict(weights(model, seed, fp32_exact=True), strict=True)
    return model


def run(model, x, mask, eps):
    """{name: fp64 CPU tensor} of the outputs and 'g_<param>' gradients of loss_of"""
    for p in model.parameters():
        p.grad = None
    loss, out = loss_of(model, x, mask, eps)
    loss.backward()
    res = {k: v.detach().double().cpu() for k, v in out.items()}
    res.update({"g_" + n: p.grad.detach().double().cpu() for n, p in model.named_parameters()})
    return res


@functools.lru_cache(maxsize=None)
def reference(B, D, L, hidden=(300, 30), seed=5):
    """The case's inputs and its fp64 CPU results (computed once, shared, never modified)"""
    x, mask, eps = inputs(B, D, L, seed)
    return (x, mask, eps), run(build(L, D, hidden, seed), x, mask, eps)


def on_gpu(L, D, hidden, seed):
    return build(L, D, hidden, seed).float().to(DEV)


def rel(a, b):
    """max |a - b| / max |b| in fp64 on the CPU"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def worst(got, want):
    """(the largest rel over the reference's tensors, its name)"""
    errs = {k: rel(got[k], want[k]) for k in want}
    k = max(errs, key=errs.get)
    return errs[k], k
