"""predict_exact(..., return_var=True), batch_predict_varying_T(..., return_var=True) and sample_predictions against
tests/golden/predict_var.npz (tests/golden/gen_golden_predict_var.py: both variances formed densely in fp64 from the
reference's own kernel modules), with batched modules and with per-dim lists.

Variance: the project's tolerance rule min(max(10 x yardstick, 2e-12), 1e-6) on max |got - ref| / max prior, the
yardstick being the larger of the dense oracle's change under a relative 2^-50 perturbation of hyper-parameters,
noise, mu and z and its CPU / device spread (test_predict_var_oracle.py pins the oracle to the golden at 1e-12).
Everything else is bit for bit: the mean beside the variance against the mean-only call, the default calls against
the C entry points they have always made, shuffled test rows, dim groups and test-row chunks under a workspace cap.
"""
import numpy as np
import pytest
import torch

import abi_util as U
import test_predict_var_oracle as V
from conftest import golden
from test_gpu_predict_exact import kernels as exact_kernels, likelihoods as exact_likelihoods

gpu = pytest.mark.gpu
DEV = "cuda"


def held_noise(lik, L):
    """[1, L] on the CPU: the noise the likelihood object(s) hold (a GaussianLikelihood stores its noise through a
    transform, a few ulps from the float it was built with)"""
    from lvae_amd.elbo import _noise_vector
    return _noise_vector(lik, L).detach().cpu().double().reshape(1, L)


def rule(kind, oracle_on_device):
    (_, var, prior), ya = V.cpu_ref(kind, None)
    yard = max(ya, V.var_err(oracle_on_device[1], var, prior))
    return min(max(10.0 * yard, 2e-12), 1e-6), yard


def exact_inputs():
    g, gv = golden("exact_predict.npz"), golden("predict_var.npz")
    return g, gv, (torch.tensor(g["X"], device=DEV), torch.tensor(gv["exact_tx"], device=DEV),
                   torch.tensor(g["mu"], device=DEV))


@gpu
@pytest.mark.parametrize("batched", [False, True])
def test_predict_exact_variance_matches_golden(hip, batched):
    import lvae_amd as la
    g, gv, (X, tx, mu) = exact_inputs()
    k, L = exact_kernels(g, batched)
    lik = exact_likelihoods(g, batched)
    mean, var = la.predict_exact(k, lik, X, tx, mu, return_var=True)
    assert var.shape == (12, L) and var.dtype == torch.float64 and mean.shape == (12, L)
    tol, yard = rule("golden-exact", V.golden_exact_oracle(DEV))
    prior = torch.tensor(gv["exact_prior"])
    err = V.var_err(var, torch.tensor(gv["exact_var"]), prior)
    print(f"predict_exact variance batched={batched}: err {err:.2e} yardstick {yard:.2e} bound {tol:.1e}")
    assert err <= tol
    assert bool((var >= 0).all())
    only = la.predict_exact(k, lik, X, tx, mu)
    assert U.bit_equal(mean, only)                                   # the mean beside the variance: the same bits
    _, vn = la.predict_exact(k, lik, X, tx, mu, return_var=True, add_noise=True)
    ulp = float(np.spacing(float(prior.max())))
    assert float((vn.cpu() - (var.cpu() + held_noise(lik, L))).abs().max()) <= ulp


@gpu
def test_predict_exact_default_is_todays_call(hip):
    """Without return_var the result is lvae_predict_exact_f64's, bit for bit."""
    import lvae_amd as la
    from lvae_amd import _lib as P
    g, gv, (X, tx, mu) = exact_inputs()
    k, L = exact_kernels(g, True)
    got = la.predict_exact(k, exact_likelihoods(g, True), X, tx, mu)
    spec, params = la.kernel_spec_and_params(k)
    params = params.detach().to(DEV, torch.float64).contiguous()
    noise = torch.tensor(g["noise"], device=DEV)
    n, nt = X.shape[0], tx.shape[0]
    out, info = torch.empty(nt, L, dtype=torch.float64, device=DEV), torch.empty(L, dtype=torch.int32, device=DEV)
    ws, _ = U.workspace(hip.lvae_predict_exact_workspace_size(n, nt, L))
    rc = hip.lvae_predict_exact_f64(spec, P.ptr(X), X.stride(0), n, L, P.ptr(params), P.ptr(noise), P.ptr(mu), L,
                                    P.ptr(tx), tx.stride(0), nt, P.ptr(out), L, P.ptr(info), P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and U.bit_equal(got, out)


@gpu
def test_predict_exact_shuffled_rows_and_workspace_cap(hip):
    """Shuffled test rows permute the output rows; a max_workspace_bytes that holds one dim with a few test rows
    forces >= 2 dim groups and >= 2 test-row chunks: the same bits."""
    import lvae_amd as la
    g, gv, (X, tx, mu) = exact_inputs()
    k, L = exact_kernels(g, True)
    lik = exact_likelihoods(g, True)
    mean, var = la.predict_exact(k, lik, X, tx, mu, return_var=True)
    perm = torch.randperm(tx.shape[0], generator=torch.Generator().manual_seed(3)).to(DEV)
    mp, vp = la.predict_exact(k, lik, X, tx[perm], mu, return_var=True)
    assert U.bit_equal(mp, mean[perm]) and U.bit_equal(vp, var[perm])
    n, nt = X.shape[0], tx.shape[0]
    size = lambda dims, chunk: int(hip.lvae_predict_exact_var_workspace_size(n, nt, dims, chunk))
    cap = size(1, 5)
    assert size(1, 1) < cap < size(2, 1) and cap < size(1, nt)      # one dim a group, fewer than nt rows a chunk
    mc, vc = la.predict_exact(k, lik, X, tx, mu, max_workspace_bytes=cap, return_var=True)
    assert U.bit_equal(mc, mean) and U.bit_equal(vc, var)


def inducing_modules(gv, batched):
    """The fixture's kernels, likelihood(s) and inducing points as the project's modules on the device"""
    import lvae_amd as la
    L = int(gv["ind_L"])

    def build(latent_dim, raw0, raw1):
        k0, k1 = la.generate_kernel_batched(latent_dim, **V.REF_CFG, id_covariate=2)
        with torch.no_grad():
            for mod, raw in ((k0, raw0), (k1, raw1)):   # raw [params, latent_dim] in named_parameters order
                for j, (_, p) in enumerate(mod.named_parameters()):
                    p.copy_(torch.as_tensor(raw[j], dtype=p.dtype))
        return k0.double().to(DEV), k1.double().to(DEV)
    Z = torch.tensor(gv["ind_Z"], device=DEV)
    if batched:
        k0, k1 = build(L, gv["ind_raw0"], gv["ind_raw1"])
        lik = la.GaussianLikelihood(L, noise=1.0).to(DEV)
        lik.noise = torch.tensor(gv["ind_noise"], device=DEV)
        return k0, k1, lik, Z
    pairs = [build(1, gv["ind_raw0"][:, l:l + 1], gv["ind_raw1"][:, l:l + 1]) for l in range(L)]
    liks = [la.GaussianLikelihood(1, noise=float(gv["ind_noise"][l])).to(DEV) for l in range(L)]
    return [p[0] for p in pairs], [p[1] for p in pairs], liks, [Z[l] for l in range(L)]


def inducing_call(gv, batched, tidx=None, **kw):
    import lvae_amd as la
    k0, k1, lik, Z = inducing_modules(gv, batched)
    X = gv["ind_X_all"]
    tidx = gv["ind_tidx"] if tidx is None else tidx
    return la.batch_predict_varying_T(int(gv["ind_L"]), k0, k1, lik, torch.tensor(X[gv["ind_pidx"]], device=DEV),
                                      torch.tensor(X[tidx], device=DEV), torch.tensor(gv["ind_mu"], device=DEV), Z,
                                      int(gv["ind_id_covariate"]), float(gv["ind_eps"]), **kw)


@gpu
@pytest.mark.parametrize("batched", [False, True])
def test_batch_predict_variance_matches_golden(hip, batched):
    gv = golden("predict_var.npz")
    mean, var = inducing_call(gv, batched, return_var=True)
    assert var.shape == (15, 3) and var.dtype == torch.float64 and mean.shape == (15, 3)
    lik = inducing_modules(gv, batched)[2]
    tol, yard = rule("golden-ind", V.inducing_oracle(V.golden_inducing_inputs(), DEV))
    prior = torch.tensor(gv["ind_prior"])
    err = V.var_err(var, torch.tensor(gv["ind_var"]), prior)
    merr = U.rel(mean, torch.tensor(gv["ind_mean"]))
    print(f"batch_predict variance batched={batched}: err {err:.2e} yardstick {yard:.2e} bound {tol:.1e} "
          f"(mean against the dense mean: {merr:.2e})")
    assert err <= tol
    assert bool((var >= 0).all())
    only = inducing_call(gv, batched)
    assert U.bit_equal(mean, only)                                   # the mean beside the variance: the same bits
    _, vn = inducing_call(gv, batched, return_var=True, add_noise=True)
    ulp = float(np.spacing(float(prior.max())))
    assert float((vn.cpu() - (var.cpu() + held_noise(lik, 3))).abs().max()) <= ulp


@gpu
def test_batch_predict_default_is_todays_call(hip):
    """Without return_var the result is lvae_predict_f64's on the caller's row order, bit for bit."""
    import lvae_amd as la
    from lvae_amd import _lib as P
    from lvae_amd.elbo import _subject_layout
    gv = golden("predict_var.npz")
    got = inducing_call(gv, True)
    k0, k1, lik, Z = inducing_modules(gv, True)
    (s0, p0), (s1, p1) = la.kernel_spec_and_params(k0), la.kernel_spec_and_params(k1)
    dv = lambda t: t.detach().to(DEV, torch.float64).contiguous()
    X = gv["ind_X_all"]
    xp, tx = torch.tensor(X[gv["ind_pidx"]]), dv(torch.tensor(X[gv["ind_tidx"]]))
    gather, valid, seg, T = _subject_layout(xp[:, 2])
    inc = torch.isin(torch.unique(xp[:, 2]), torch.unique(tx[:, 2].cpu())).to(torch.int32)
    x_pad = dv(xp[gather])
    mu_pad = dv(torch.tensor(gv["ind_mu"])[gather] * valid.to(torch.float64).unsqueeze(1))
    L, M, Pn, Nt = int(gv["ind_L"]), int(gv["ind_M"]), int(seg.numel()), int(tx.shape[0])
    out = torch.empty(Nt, L, dtype=torch.float64, device=DEV)
    ws, _ = U.workspace(hip.lvae_predict_workspace_size(L, M, Pn, T, Nt))
    seg_d, inc_d, p0, p1, nz = seg.to(DEV), inc.to(DEV), dv(p0), dv(p1), dv(lik.noise)
    rc = hip.lvae_predict_f64(s0, s1, L, M, X.shape[1], Pn, T, P.ptr(seg_d), P.ptr(inc_d), P.ptr(x_pad), P.ptr(mu_pad),
                              P.ptr(Z), Nt, P.ptr(tx), P.ptr(p0), P.ptr(p1), P.ptr(nz), float(gv["ind_eps"]), P.ptr(out),
                              None, P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and U.bit_equal(got, out)


@gpu
def test_batch_predict_shuffled_rows(hip):
    gv = golden("predict_var.npz")
    mean, var = inducing_call(gv, True, return_var=True)
    perm = torch.randperm(15, generator=torch.Generator().manual_seed(4))
    mp, vp = inducing_call(gv, True, tidx=gv["ind_tidx"][perm.numpy()], return_var=True)
    assert U.bit_equal(mp, mean[perm.to(DEV)]) and U.bit_equal(vp, var[perm.to(DEV)])


@gpu
def test_sample_predictions(hip):
    import lvae_amd as la
    gv = golden("predict_var.npz")
    mean, var = inducing_call(gv, True, return_var=True)
    assert U.bit_equal(la.sample_predictions(mean, var, eps=torch.zeros_like(mean)), mean)
    assert U.bit_equal(la.sample_predictions(mean, var, eps=torch.ones_like(mean)), mean + torch.sqrt(var))
    gen = lambda: torch.Generator(device=DEV).manual_seed(11)
    a, b = la.sample_predictions(mean, var, generator=gen()), la.sample_predictions(mean, var, generator=gen())
    assert a.shape == mean.shape and U.bit_equal(a, b) and not U.bit_equal(a, mean)


def test_sample_predictions_on_the_cpu():
    """sample_predictions is plain tensor arithmetic: no GPU, no library call."""
    from lvae_amd.predict import sample_predictions
    mean, var = torch.tensor([[1.0, -2.0]], dtype=torch.float64), torch.tensor([[4.0, 0.25]], dtype=torch.float64)
    assert sample_predictions(mean, var, eps=torch.zeros_like(mean)).tolist() == [[1.0, -2.0]]
    assert sample_predictions(mean, var, eps=torch.ones_like(mean)).tolist() == [[3.0, -1.5]]
    assert sample_predictions(mean, var, generator=torch.Generator().manual_seed(0)).shape == (1, 2)


def test_drop_in_utils_exports_sample_predictions():
    import os
    import sys
    from conftest import ROOT
    d = os.path.join(ROOT, "longitudinal-vae_amd", "dropin")
    sys.path.insert(0, d)
    try:
        sys.modules.pop("utils", None)
        import utils as DU
        import lvae_amd as la
        assert DU.sample_predictions is la.sample_predictions and "sample_predictions" in DU.__all__
    finally:
        sys.path.remove(d)
        sys.modules.pop("utils", None)
