"""GP posterior prediction of the latents (utils.py:115-211 batch_predict_varying_T), the step
MSE_test_GPapprox (model_test.py:85-143) runs after training.  Same signature and return value;
the computation is one batched HIP pass (lvae_predict_f64) instead of the reference's per-subject
Python loops and its removed ``torch.solve``.  ``predict_exact`` is the exact-GP predictor of MSE_test
(model_test.py:19-82) for models trained with the exact KL (lvae_predict_exact_f64).

Both predictors also return the predictive variance of the latent functions (``return_var=True``:
lvae_predict_var_f64, lvae_predict_exact_var_f64), which the reference does not compute; ``sample_predictions``
draws from the resulting marginals.
"""
import ctypes

import torch

from . import _lib
from .elbo import _check_info, _noise_vector, _stack_modules, _subject_layout


def batch_predict_varying_T(latent_dim, covar_module0, covar_module1, likelihoods, prediction_x, test_x, mu,
                            zt_list, id_covariate, eps, return_var=False, add_noise=False):
    """Z_pred [N_test, L]: posterior mean of the L latent GPs at ``test_x`` given the encoder means
    ``mu`` [N_pred, L] at ``prediction_x`` (subjects of any length).  ``covar_module0/1`` are
    batched modules or per-dim lists, ``zt_list`` the inducing points [L, M, Q] (or a per-dim
    list of [M, Q]).

    ``return_var=True`` returns ``(Z_pred, Z_var)``: Z_var [N_test, L] fp64 is the predictive variance of the
    latent functions in the same structured model (lvae_predict_var_f64; K0xz K0zz^-1 K0zx + blockdiag k1 as
    the prior), clamped at 0, in the caller's row order; ``add_noise=True`` adds the likelihood noise of each
    dim.  The id kernel ``covar_module1`` must vanish between subjects (generate_kernel_batched's does)."""
    lib = _lib.lib()
    L = int(latent_dim)
    spec0, params0 = _stack_modules(covar_module0)
    spec1, params1 = _stack_modules(covar_module1)
    if params0.shape[0] == 1 and L > 1:
        params0 = params0.expand(L, -1)
    if params1.shape[0] == 1 and L > 1:
        params1 = params1.expand(L, -1)
    for mod in (covar_module0, covar_module1, likelihoods):
        for m_ in (mod if isinstance(mod, (list, tuple, torch.nn.ModuleList)) else [mod]):
            if hasattr(m_, "eval"):
                m_.eval()
    dev = mu.device
    f64 = lambda t: t.detach().to(dev, torch.float64).contiguous()
    if isinstance(zt_list, (list, tuple)):
        z = torch.stack([f64(zi) for zi in zt_list])
    else:
        z = f64(zt_list)
        if z.dim() == 2:
            z = z.unsqueeze(0).expand(L, -1, -1).contiguous()
    M, Q = z.shape[1], z.shape[2]
    noise = f64(_noise_vector(likelihoods, L)).reshape(L)
    gather, valid, seg, T = _subject_layout(prediction_x[:, id_covariate])
    P = int(seg.numel())
    pred_ids = torch.unique(prediction_x[:, id_covariate].detach().to("cpu", torch.float64))
    test_ids = torch.unique(test_x[:, id_covariate].detach().to("cpu", torch.float64))
    include = torch.isin(pred_ids, test_ids).to(torch.int32)
    g = gather.to(dev)
    x_pad = f64(prediction_x)[g].contiguous()
    mu_pad = (f64(mu)[g] * valid.to(dev, torch.float64).unsqueeze(1)).contiguous()
    tx = f64(test_x)
    Nt = int(tx.shape[0])
    seg_d, inc_d = seg.to(dev), include.to(dev)
    p0, p1 = f64(params0), f64(params1)
    out = torch.empty(Nt, L, dtype=torch.float64, device=dev)
    info = torch.empty(L, dtype=torch.int32, device=dev)
    if return_var:
        # test rows grouped by subject (stable: a subject's rows keep their order), each group with its
        # subject's index in the prediction layout or -1; the grouping is undone on the way out
        tid = test_x[:, id_covariate].detach().to("cpu", torch.float64)
        order = torch.argsort(tid, stable=True)
        ids, counts = torch.unique_consecutive(tid[order], return_counts=True)
        where = torch.searchsorted(pred_ids, ids).clamp(max=P - 1)
        subj = torch.where(pred_ids[where] == ids, where, torch.full_like(where, -1)).to(torch.int32)
        start = torch.zeros(ids.numel() + 1, dtype=torch.int32)
        start[1:] = torch.cumsum(counts, 0)
        order_d = order.to(dev)
        txg = tx[order_d].contiguous()
        outg = torch.empty_like(out)
        var = torch.empty_like(out)
        subj_d, start_d = subj.to(dev), start.to(dev)
        ws = torch.empty(int(lib.lvae_predict_var_workspace_size(L, M, P, T, Nt)), dtype=torch.uint8, device=dev)
        rc = lib.lvae_predict_var_f64(spec0, spec1, L, M, Q, P, T, _lib.ptr(seg_d), _lib.ptr(inc_d), _lib.ptr(x_pad),
                                      _lib.ptr(mu_pad), _lib.ptr(z), Nt, _lib.ptr(txg), int(ids.numel()),
                                      _lib.ptr(subj_d), _lib.ptr(start_d), _lib.ptr(p0), _lib.ptr(p1),
                                      _lib.ptr(noise), float(eps), _lib.ptr(outg), _lib.ptr(var),
                                      1 if add_noise else 0, _lib.ptr(info), _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, "predict_var")
        _check_info(info, "batch_predict_varying_T cholesky (10000+col: K0zz, 20000+col: B_st, 30000+col: H)")
        out[order_d] = outg
        z_var = torch.empty_like(var)
        z_var[order_d] = var.clamp_(min=0.0)
        return out, z_var
    ws = torch.empty(int(lib.lvae_predict_workspace_size(L, M, P, T, Nt)), dtype=torch.uint8, device=dev)
    rc = lib.lvae_predict_f64(spec0, spec1, L, M, Q, P, T, _lib.ptr(seg_d), _lib.ptr(inc_d), _lib.ptr(x_pad),
                              _lib.ptr(mu_pad), _lib.ptr(z), Nt, _lib.ptr(tx), _lib.ptr(p0), _lib.ptr(p1),
                              _lib.ptr(noise), float(eps), _lib.ptr(out), _lib.ptr(info), _lib.ptr(ws),
                              _lib.stream_ptr())
    _lib.check(rc, "predict")
    _check_info(info, "batch_predict_varying_T cholesky (10000+col: K0zz, 20000+col: B_st, 30000+col: H)")
    return out


def predict_exact(covar_module, likelihoods, prediction_x, test_x, prediction_mu, max_workspace_bytes=4 << 30,
                  return_var=False, add_noise=False):
    """Z_pred [N_test, L] fp64: the exact-GP posterior mean k(X*, X) (k(X, X) + noise I)^-1 mu per latent dim
    (model_test.py:11-17 predict_gp as MSE_test calls it, model_test.py:65-76), one HIP pass per group of dims
    (lvae_predict_exact_f64) instead of the reference's per-dim explicit inverse and dense [N_test, N] Gram.

    ``covar_module`` is a batched module or a per-dim list (as MSE_test passes), ``prediction_mu`` [N, L] the
    encoder means at ``prediction_x`` [N, Q].  The dims are processed in groups whose workspace (about 8 N^2
    bytes a dim) stays under ``max_workspace_bytes``; a non-positive-definite K raises LinAlgError.

    ``return_var=True`` returns ``(Z_pred, Z_var)``: Z_var [N_test, L] fp64 is the latent functions' predictive
    variance k(x*, x*) - |L^-1 k(X, x*)|^2 (lvae_predict_exact_var_f64), clamped at 0; ``add_noise=True`` adds
    each dim's likelihood noise.  The test rows are then solved in chunks (8 N bytes a row and dim) sized, after
    the dim groups, to keep the workspace under ``max_workspace_bytes``; neither choice changes the bits."""
    lib = _lib.lib()
    spec, params = _stack_modules(covar_module)
    L = int(prediction_mu.shape[1])
    if params.shape[0] == 1 and L > 1:
        params = params.expand(L, -1)
    if params.shape[0] != L:
        raise ValueError(f"kernel batch {params.shape[0]} != latent dims {L}")
    for mod in (covar_module, likelihoods):
        for m_ in (mod if isinstance(mod, (list, tuple, torch.nn.ModuleList)) else [mod]):
            if hasattr(m_, "eval"):
                m_.eval()
    dev = prediction_mu.device
    f64 = lambda t: t.detach().to(dev, torch.float64).contiguous()
    x, tx, mu, p = f64(prediction_x), f64(test_x), f64(prediction_mu), f64(params)
    noise = f64(_noise_vector(likelihoods, L)).reshape(L)
    n, nt, n_params = int(x.shape[0]), int(tx.shape[0]), int(p.shape[1])
    if n < 1 or mu.shape[0] != n:
        raise ValueError(f"prediction_mu rows {mu.shape[0]} != prediction_x rows {n} (>= 1)")
    chunk = 1   # (the smallest panel decides the dim groups; the chunk then takes what is left)
    if return_var:
        size = lambda g: int(lib.lvae_predict_exact_var_workspace_size(n, nt, g, chunk))
    else:
        size = lambda g: int(lib.lvae_predict_exact_workspace_size(n, nt, g))
    group = L
    while group > 1 and size(group) > max_workspace_bytes:
        group -= 1
    if return_var and nt:
        chunk = nt
        while chunk > 1 and size(group) > max_workspace_bytes:
            chunk = (chunk + 1) // 2
    out = torch.empty(nt, L, dtype=torch.float64, device=dev)
    var = torch.empty(nt, L, dtype=torch.float64, device=dev) if return_var else None
    info = torch.empty(L, dtype=torch.int32, device=dev)
    ws = torch.empty(size(group), dtype=torch.uint8, device=dev)
    at = lambda t, off: ctypes.c_void_p(t.data_ptr() + 8 * off)
    for l0 in range(0, L, group):
        g = min(group, L - l0)
        if return_var:
            rc = lib.lvae_predict_exact_var_f64(spec, _lib.ptr(x), x.stride(0), n, g, at(p, l0 * n_params),
                                                at(noise, l0), at(mu, l0), L, _lib.ptr(tx) if nt else None,
                                                tx.stride(0), nt, at(out, l0) if nt else None, L,
                                                at(var, l0) if nt else None, L, 1 if add_noise else 0, chunk,
                                                ctypes.c_void_p(info.data_ptr() + 4 * l0), _lib.ptr(ws),
                                                _lib.stream_ptr())
            _lib.check(rc, "predict_exact_var")
            continue
        rc = lib.lvae_predict_exact_f64(spec, _lib.ptr(x), x.stride(0), n, g, at(p, l0 * n_params), at(noise, l0),
                                        at(mu, l0), L, _lib.ptr(tx) if nt else None, tx.stride(0), nt,
                                        at(out, l0) if nt else None, L,
                                        ctypes.c_void_p(info.data_ptr() + 4 * l0), _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, "predict_exact")
    _check_info(info, "predict_exact cholesky of k(X, X) + noise I")
    if return_var:
        return out, var.clamp_(min=0.0)
    return out


def sample_predictions(mean, var, eps=None, generator=None):
    """mean + sqrt(var) * eps, eps ~ N(0, 1) elementwise (drawn with ``generator`` unless given): independent draws
    from each test row's own marginal N(mean, var).  The rows are NOT drawn jointly: no covariance between test
    rows (or latent dims) is modelled, so a drawn trajectory is rougher than a joint posterior sample would be."""
    if eps is None:
        eps = torch.randn(mean.shape, dtype=mean.dtype, device=mean.device, generator=generator)
    return mean + torch.sqrt(var.clamp(min=0.0)) * eps
