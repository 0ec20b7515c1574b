"""Shared inputs and runners of the all-dims DUBO tests (test_gpu_dubo.py, test_gpu_dubo_abi.py,
test_gpu_dubo_drivers.py): one problem per (P, T, M) case with distinct per-dim raw parameters, noises and
inducing rows drawn from x, the fp64 oracle under CPU autograd (computed once per case), the batched HIP call
through Python, the per-dim composed route, and a raw C-ABI forward + backward on sentinel-filled outputs."""
import ctypes
import functools
import types

import numpy as np
import torch

import abi_util as U
from oracle import lvae_oracle as O

DEV = "cuda"
CFG = dict(cat_kernel=[2], bin_kernel=[], sqexp_kernel=[0],
           cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 2},
                           {'cont_covariate': 0, 'cat_covariate': 3},
                           {'cont_covariate': 1, 'cat_covariate': 4}],
           bin_int_kernel=[], covariate_missing_val=[])
EPS = 1e-6
SUBJECTS_PER_WORKGROUP = 16   # kBoundS of csrc/gp_bound.hpp: the fused pass runs ceil(P / 16) workgroups per dim
FAST_T = 32                   # kBoundT: larger T takes the batched-product route

# id: (P, T, M, noise of dim 0); every case has L = 3
CASES = {
    "6x7x33": (6, 7, 33, 0.8),        # odd sizes, M past two MFMA tiles
    "5x3x9": (5, 3, 9, 0.8),
    "1x4x3": (1, 4, 3, 0.8),          # one subject
    "3x1x1": (3, 1, 1, 0.8),          # T = M = 1
    "9x16x120": (9, 16, 120, 0.3),    # the workload's T and M: 8 column tiles, 36 lower tiles, 5 per wave
    "2x128x128": (2, 128, 128, 0.8),  # T > 32: the batched-product route, at both limits
    "4x32x17": (4, 32, 17, 0.8),      # the last T of the fused pass
    "3x33x17": (3, 33, 17, 0.8),      # the first T past it
    "15x3x9": (15, 3, 9, 0.8),        # one below a multiple of the subjects per workgroup
    "16x3x9": (16, 3, 9, 0.8),        # on it: one full group
    "17x3x9": (17, 3, 9, 0.8),        # one above: a second group of one subject
    "35x2x5": (35, 2, 5, 0.8),        # three groups, the last with three subjects
}
CASE_IDS = list(CASES)
L = 3
QUANT = ["dubo", "dmu", "dlogv", "draw0", "draw1", "dnoise"]
BOUND = dict(dubo=1e-8, dmu=1e-7, dlogv=1e-7, draw0=1e-6, draw1=1e-6, dnoise=1e-6)


def rel(a, b):
    return U.rel(torch.as_tensor(a), torch.as_tensor(b))


def set_raw(module, raw_rows):
    with torch.no_grad():
        for j, (_, p) in enumerate(module.named_parameters()):
            p.copy_(torch.as_tensor(raw_rows[:, j], dtype=p.dtype))


@functools.lru_cache(maxsize=None)
def problem(cid):
    from lvae_amd.data import health_mnist_covariates
    P, T, M, nz0 = CASES[cid]
    seed = 300 + CASE_IDS.index(cid)
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    N = P * T
    X = torch.tensor(health_mnist_covariates(P, T, seed=seed))
    s0, s1 = O.spec_split(**CFG, id_covariate=2)
    Z = torch.stack([X[np.sort(np.random.default_rng(seed + 17 * l).choice(N, M, replace=False))] for l in range(L)])
    return dict(cid=cid, P=P, T=T, M=M, N=N, X=X, Z=Z, s0=s0, s1=s1,
                raw0=np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s0)))),
                raw1=np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s1)))),
                noise=nz0 * np.array([1.0, 1.25, 1.5]),
                mu=torch.randn(N, L, generator=gen, dtype=torch.float64),
                lv=0.1 * torch.randn(N, L, generator=gen, dtype=torch.float64))


def modules_batched(c, dev=DEV):
    import lvae_amd as la
    k0, k1 = la.generate_kernel_batched(L, **CFG, id_covariate=2)
    set_raw(k0, c["raw0"])
    set_raw(k1, c["raw1"])
    lik = la.GaussianLikelihood(L, noise=1.0)
    lik.noise = torch.tensor(c["noise"])
    return k0.to(dev), k1.to(dev), lik.to(dev)


def modules_list(c, dev=DEV):
    import lvae_amd as la
    k0s, k1s, liks = [], [], []
    for l in range(L):
        k0, k1 = la.generate_kernel_approx(**CFG, id_covariate=2)
        set_raw(k0, c["raw0"][l:l + 1])
        set_raw(k1, c["raw1"][l:l + 1])
        k0s.append(k0.to(dev))
        k1s.append(k1.to(dev))
        liks.append(la.GaussianLikelihood(1, noise=float(c["noise"][l])).to(dev))
    return k0s, k1s, liks


def _raw_grads(k0, k1, lik):
    if isinstance(k0, list):
        return (torch.stack([torch.cat([p.grad for _, p in k.named_parameters()]) for k in k0]),
                torch.stack([torch.cat([p.grad for _, p in k.named_parameters()]) for k in k1]),
                torch.cat([lk._log_noise.grad for lk in lik]))
    return (torch.stack([p.grad for _, p in k0.named_parameters()], 1),
            torch.stack([p.grad for _, p in k1.named_parameters()], 1), lik._log_noise.grad)


def _collect(vals, mu, lv, k0, k1, lik):
    d0, d1, dn = _raw_grads(k0, k1, lik)
    out = dict(dubo=vals, dmu=mu.grad, dlogv=lv.grad, draw0=d0, draw1=d1, dnoise=dn)
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def run_batched(cid, form="batched", cot=None):
    """deviance_upper_bound_batched on the GPU with batched modules or per-dim lists; gradients of
    sum_l cot_l dubo_l (cot = None: ones)."""
    import lvae_amd as la
    c = problem(cid)
    k0, k1, lik = modules_batched(c) if form == "batched" else modules_list(c)
    mu, lv = c["mu"].to(DEV).requires_grad_(), c["lv"].to(DEV).requires_grad_()
    z = c["Z"].to(DEV) if form == "batched" else [zi.to(DEV) for zi in c["Z"]]
    vals = la.deviance_upper_bound_batched(L, k0, k1, lik, c["X"].to(DEV), mu, lv, z, c["P"], c["T"], EPS)
    assert vals.shape == (L,) and vals.dtype == torch.float64
    g = torch.ones(L, dtype=torch.float64) if cot is None else torch.as_tensor(cot, dtype=torch.float64)
    vals.backward(g.to(DEV))
    return _collect(vals, mu, lv, k0, k1, lik)


@functools.lru_cache(maxsize=None)
def batched(cid):
    return run_batched(cid)


@functools.lru_cache(maxsize=None)
def oracle(cid):
    """oracle.lvae_oracle.deviance_upper_bound per dim under CPU autograd (the raw -> positive transforms are the
    package's own CPU formulas)"""
    c = problem(cid)
    k0, k1, lik = modules_batched(c, "cpu")
    import lvae_amd as la
    _, p0 = la.kernel_spec_and_params(k0)
    _, p1 = la.kernel_spec_and_params(k1)
    nz = lik.noise
    mu, lv = c["mu"].clone().requires_grad_(), c["lv"].clone().requires_grad_()
    vals = torch.stack([O.deviance_upper_bound(c["s0"], p0[l], c["s1"], p1[l], nz[l], c["X"], mu[:, l], lv[:, l],
                                               c["Z"][l], c["P"], c["T"], EPS) for l in range(L)])
    vals.sum().backward()
    return _collect(vals, mu, lv, k0, k1, lik)


@functools.lru_cache(maxsize=None)
def composed(cid):
    """the per-dim lvae_amd.deviance_upper_bound (torch composition over the HIP Grams and inverses), dim by dim"""
    import lvae_amd as la
    c = problem(cid)
    k0, k1, lik = modules_list(c)
    mu, lv = c["mu"].to(DEV).requires_grad_(), c["lv"].to(DEV).requires_grad_()
    X = c["X"].to(DEV)
    vals = torch.stack([la.deviance_upper_bound(k0[l], k1[l], lik[l], X, mu[:, l], lv[:, l], c["Z"][l].to(DEV),
                                                c["P"], c["T"], EPS) for l in range(L)])
    vals.sum().backward()
    return _collect(vals, mu, lv, k0, k1, lik)


def noise_stub(values, dev=DEV):
    """a likelihood that only has noise_covar.noise [L, 1] (any sign: the positivity transform is bypassed)"""
    t = torch.as_tensor(values, dtype=torch.float64, device=dev).reshape(-1, 1)
    return types.SimpleNamespace(noise_covar=types.SimpleNamespace(noise=t))


# ------------------------------------------------------------------------------------------------------
# the C ABI directly
# ------------------------------------------------------------------------------------------------------
TAIL = 7


def as_problem(cid):
    """a case id of this module, or a problem given whole: problem()'s keys with any specs and covariates, the
    positive hyper-parameters as p0 / p1 [L, n] in place of raw0 / raw1, and its own jitter as eps (ext_util)"""
    return problem(cid) if isinstance(cid, str) else cid


def positive(c):
    """(p0, p1, noise) [L, .] fp64 of a problem, and its jitter"""
    if "p0" in c:
        p0, p1 = c["p0"], c["p1"]
    else:
        p0, p1 = O.constrain(torch.tensor(c["raw0"])), O.constrain(torch.tensor(c["raw1"]))
    return p0, p1, torch.as_tensor(c["noise"], dtype=torch.float64), c.get("eps", EPS)


def abi_inputs(cid, noise=None):
    from lvae_amd import _lib as P
    c = as_problem(cid)
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    p0, p1, nz, eps = positive(c)
    t = dict(x=c["X"], z=c["Z"], mu=c["mu"], lv=c["lv"], p0=p0, p1=p1,
             noise=nz if noise is None else torch.tensor(noise, dtype=torch.float64))
    d = {k: v.to(DEV).contiguous() for k, v in t.items()}
    dims = P.DuboDims(L, c["M"], c["P"], c["T"], c["X"].shape[1], eps)
    return c, s0, s1, dims, d


def abi_outputs(c, s0, s1):
    n = dict(dubo=L, dmu=c["N"] * L, dlogv=c["N"] * L, dp0=L * s0.n_params, dp1=L * s1.n_params, dnoise=L)
    return n, {k: U.sentinel(v + TAIL) for k, v in n.items()}


def abi_run(hip, cid, cot=None, noise=None, want_info=True, want_dnoise=True):
    """Forward then backward on a sentinel-tailed workspace with NaN-filled outputs (each with TAIL spare
    sentinels behind it).  Returns ({name: logical CPU tensor}, info or None, {name: whole buffer}, sizes)."""
    from lvae_amd import _lib as P
    c, s0, s1, dims, d = abi_inputs(cid, noise)
    n, o = abi_outputs(c, s0, s1)
    info = U.sentinel(L + TAIL, torch.int32)
    ws, tail = U.workspace(hip.lvae_dubo_workspace_size(ctypes.byref(dims)))
    g = torch.ones(L, dtype=torch.float64) if cot is None else torch.as_tensor(cot, dtype=torch.float64)
    g = g.to(DEV)
    st = P.stream_ptr()
    common = (ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), P.ptr(d["x"]), P.ptr(d["z"]), P.ptr(d["mu"]),
              P.ptr(d["lv"]), P.ptr(d["p0"]), P.ptr(d["p1"]), P.ptr(d["noise"]))
    rc = hip.lvae_dubo_fwd_f64(*common, P.ptr(o["dubo"]), P.ptr(info) if want_info else None, P.ptr(ws), st)
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)
    rc = hip.lvae_dubo_bwd_f64(*common, P.ptr(g), P.ptr(o["dmu"]), P.ptr(o["dlogv"]), P.ptr(o["dp0"]),
                               P.ptr(o["dp1"]), P.ptr(o["dnoise"]) if want_dnoise else None, P.ptr(ws), st)
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)
    shapes = dict(dubo=(L,), dmu=(c["N"], L), dlogv=(c["N"], L), dp0=(L, s0.n_params), dp1=(L, s1.n_params),
                  dnoise=(L,))
    out = {k: o[k][:n[k]].reshape(shapes[k]).cpu() for k in o}
    return out, (info.cpu() if want_info else None), o, n
