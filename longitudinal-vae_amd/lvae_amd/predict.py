"""GP posterior prediction of the latents (utils.py:115-211 batch_predict_varying_T), the step
MSE_test_GPapprox (model_test.py:85-143) runs after training.  Same signature and return value;
the computation is one batched HIP pass (lvae_predict_f64) instead of the reference's per-subject
Python loops and its removed ``torch.solve``.  ``predict_exact`` is the exact-GP predictor of MSE_test
(model_test.py:19-82) for models trained with the exact KL (lvae_predict_exact_f64).

Both predictors also return the predictive variance of the latent functions (``return_var=True``:
lvae_predict_var_f64, lvae_predict_exact_var_f64), which the reference does not compute; ``sample_predictions``
draws from the resulting marginals.  ``return_cov=True`` returns the joint covariance of each group of test rows
(a subject's, for the inducing-point route) as a ``PredictiveCovariance`` (lvae_predict_cov_f64,
lvae_predict_exact_cov_f64), and ``sample_trajectories`` draws each group's rows jointly from it
(lvae_predict_sample_f64).  Groups are independent of each other: the covariance between rows of different groups
is not zero in the model, and is neither returned nor drawn from.

``predict_exact_components`` and ``batch_predict_components`` split the two means by additive component of the kernel
(a ``LatentComponents``); with ``return_cov=True`` they add the joint posterior covariance of the components at each
test row (lvae_predict_exact_comp_cov_f64, lvae_predict_comp_cov_f64): per-effect credible bands, and the
uncertainty of the reconstruction after the first k effects.
"""
import ctypes
from types import SimpleNamespace

import torch

from . import _lib
from .elbo import _check_info, _noise_vector, _stack_modules, _subject_layout

MAX_GROUP_ROWS = 128   # the largest group of test rows a joint covariance is formed for (kPvT)
# what _check_info names when a factorisation of a route fails
_INDUCING_INFO = "batch_predict_varying_T cholesky (10000+col: K0zz, 20000+col: B_st, 30000+col: H)"
_EXACT_INFO = "predict_exact cholesky of k(X, X) + noise I"


class PredictiveCovariance:
    """The joint predictive covariance of the latent functions at each group of test rows, per latent dim.

    ``blocks`` [L, G, n_max, n_max] fp64: block (l, g) is the covariance of group g's rows, row i of a block the
    group's i-th test row in order of appearance; padding rows and columns carry the identity and a block is
    symmetric bit for bit.  ``index`` [G, n_max] int32: the caller's row index of each block row, -1 on padding.
    ``counts`` [G] (CPU): the groups' rows.  Covariance between rows of different groups (or latent dims) is not
    held: groups are treated as independent of each other."""

    def __init__(self, blocks, index, counts):
        self.blocks, self.index, self.counts = blocks, index, counts

    @property
    def num_rows(self):
        return int(self.counts.sum())

    def diagonal(self):
        """[Nt, L]: the predictive variances in the caller's row order"""
        L, G, n_max = self.blocks.shape[:3]
        d = torch.diagonal(self.blocks, dim1=2, dim2=3).reshape(L, G * n_max)
        ix = self.index.reshape(-1).long()
        keep = ix >= 0
        out = torch.empty(self.num_rows, L, dtype=self.blocks.dtype, device=self.blocks.device)
        out[ix[keep]] = d[:, keep].T
        return out

    def block(self, g):
        """[L, n_g, n_g]: group g's covariance without padding"""
        n = int(self.counts[g])
        return self.blocks[:, g, :n, :n]


def _row_groups(labels, what, max_rows=MAX_GROUP_ROWS):
    """Test rows grouped by label, stable (a group's rows keep their order of appearance): (order [Nt], the
    groups' labels [G], counts [G], start [G + 1] int32, n_max), all on the CPU; a group above ``max_rows``
    (MAX_GROUP_ROWS where a joint covariance of the group is formed, None where none is) raises ValueError"""
    lab = labels.detach().to("cpu", torch.float64).reshape(-1)
    order = torch.argsort(lab, stable=True)
    ids, counts = torch.unique_consecutive(lab[order], return_counts=True)
    start = torch.zeros(ids.numel() + 1, dtype=torch.int32)
    start[1:] = torch.cumsum(counts, 0)
    n_max = int(counts.max()) if counts.numel() else 1
    if max_rows is not None and n_max > max_rows:
        g = int(counts.argmax())
        raise ValueError(f"{what}: group {g} (label {float(ids[g]):g}) has {n_max} test rows; a joint covariance "
                         f"is formed for groups of at most {max_rows}")
    return order, ids, counts, start, n_max


def _subject_groups(labels, pred_ids, what, max_rows):
    """_row_groups of the test rows' subject labels as a namespace (order, ids, counts, start, n_max, G) with
    ``subj`` [G] int32: each group's subject index in the sorted prediction-set ids ``pred_ids``, -1 where the
    subject is not in the prediction set.  The caller undoes the grouping on the way out."""
    order, ids, counts, start, n_max = _row_groups(labels, what, max_rows)
    where = torch.searchsorted(pred_ids, ids).clamp(max=pred_ids.numel() - 1)
    subj = torch.where(pred_ids[where] == ids, where, torch.full_like(where, -1)).to(torch.int32)
    return SimpleNamespace(order=order, ids=ids, counts=counts, start=start, n_max=n_max, G=int(ids.numel()), subj=subj)


def _group_index(order, counts, start, n_max, dev):
    """index [G, n_max] int32 on dev: the caller's row of each block row, -1 on padding"""
    G = int(counts.numel())
    index = torch.full((G, n_max), -1, dtype=torch.int32)
    if order.numel():
        g_of = torch.repeat_interleave(torch.arange(G), counts)
        index[g_of, torch.arange(order.numel()) - start[:-1].long()[g_of]] = order.to(torch.int32)
    return index.to(dev)


class _InducingInputs(SimpleNamespace):
    """_inducing_inputs' result; ``head`` and ``params`` are the argument runs every entry of the route shares"""

    def head(self, tx, nt, mean=True):
        """(spec0 .. test_x): the leading arguments for ``nt`` test rows at the pointer ``tx``"""
        return (self.spec0, self.spec1, self.L, self.M, self.Q, self.P, self.T, _lib.ptr(self.seg), _lib.ptr(self.inc),
                _lib.ptr(self.x_pad), _lib.ptr(self.mu_pad) if mean else None, _lib.ptr(self.z), nt, tx)

    def params(self):
        """(params0, params1, noise, eps)"""
        return _lib.ptr(self.p0), _lib.ptr(self.p1), _lib.ptr(self.noise), self.eps


def _inducing_inputs(latent_dim, covar_module0, covar_module1, likelihoods, prediction_x, test_x, mu, zt_list,
                     id_covariate, eps):
    """The arguments of batch_predict_varying_T as lvae_predict_f64 and its siblings take them: the modules in eval
    mode, everything fp64 on mu's device, the prediction set gathered into the padded [P, T] subject layout"""
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
    return _InducingInputs(L=L, spec0=spec0, spec1=spec1, p0=f64(params0), p1=f64(params1), dev=dev, z=z, M=M, Q=Q,
                           noise=noise, seg=seg.to(dev), inc=include.to(dev), T=T, P=P, pred_ids=pred_ids, x_pad=x_pad,
                           mu_pad=mu_pad, tx=tx, Nt=int(tx.shape[0]), eps=float(eps))


def batch_predict_varying_T(latent_dim, covar_module0, covar_module1, likelihoods, prediction_x, test_x, mu,
                            zt_list, id_covariate, eps, return_var=False, add_noise=False, return_cov=False):
    """Z_pred [N_test, L]: posterior mean of the L latent GPs at ``test_x`` given the encoder means
    ``mu`` [N_pred, L] at ``prediction_x`` (subjects of any length).  ``covar_module0/1`` are
    batched modules or per-dim lists, ``zt_list`` the inducing points [L, M, Q] (or a per-dim
    list of [M, Q]).

    ``return_var=True`` returns ``(Z_pred, Z_var)``: Z_var [N_test, L] fp64 is the predictive variance of the
    latent functions in the same structured model (lvae_predict_var_f64; K0xz K0zz^-1 K0zx + blockdiag k1 as
    the prior), clamped at 0, in the caller's row order; ``add_noise=True`` adds the likelihood noise of each
    dim.  The id kernel ``covar_module1`` must vanish between subjects (generate_kernel_batched's does).

    ``return_cov=True`` returns ``(Z_pred, cov)`` instead: ``cov`` is a PredictiveCovariance with one group per test
    subject (the rows sharing ``test_x[:, id_covariate]``), its blocks the joint covariance of the subject's rows
    in the same model (lvae_predict_cov_f64), not clamped; ``add_noise=True`` adds the noise to the diagonals.  A
    subject with more than 128 test rows raises ValueError.  The covariance between different subjects' rows is
    not zero (the shared components couple subjects) and is deliberately not returned: sample_trajectories draws
    the groups independently of each other."""
    if return_var and return_cov:
        raise ValueError("return_var and return_cov are exclusive: cov.diagonal() holds the variances")
    lib = _lib.lib()
    a = _inducing_inputs(latent_dim, covar_module0, covar_module1, likelihoods, prediction_x, test_x, mu, zt_list,
                         id_covariate, eps)
    L, M, P, T, Nt, dev = a.L, a.M, a.P, a.T, a.Nt, a.dev
    noisy = 1 if add_noise else 0
    out = torch.empty(Nt, L, dtype=torch.float64, device=dev)
    info = torch.empty(L, dtype=torch.int32, device=dev)
    if not (return_var or return_cov):
        ws = torch.empty(int(lib.lvae_predict_workspace_size(L, M, P, T, Nt)), dtype=torch.uint8, device=dev)
        rc = lib.lvae_predict_f64(*a.head(_lib.ptr(a.tx), Nt), *a.params(), _lib.ptr(out), _lib.ptr(info),
                                  _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, "predict")
        _check_info(info, _INDUCING_INFO)
        return out
    # test rows grouped by subject (stable: a subject's rows keep their order), each group with its subject's index
    # in the prediction layout or -1; the grouping is undone on the way out.  Only the joint covariance caps a group.
    g = _subject_groups(test_x[:, id_covariate], a.pred_ids, "batch_predict_varying_T",
                        MAX_GROUP_ROWS if return_cov else None)
    order_d = g.order.to(dev)
    txg = a.tx[order_d].contiguous()
    outg = torch.empty_like(out)
    subj_d, start_d = g.subj.to(dev), g.start.to(dev)
    groups = (g.G, _lib.ptr(subj_d), _lib.ptr(start_d))
    if return_cov:
        blocks = torch.empty(L, g.G, g.n_max, g.n_max, dtype=torch.float64, device=dev)
        ws = torch.empty(int(lib.lvae_predict_cov_workspace_size(L, M, P, T, Nt)), dtype=torch.uint8, device=dev)
        rc = lib.lvae_predict_cov_f64(*a.head(_lib.ptr(txg), Nt), *groups, g.n_max, *a.params(), _lib.ptr(outg),
                                      _lib.ptr(blocks), noisy, _lib.ptr(info), _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, "predict_cov")
        _check_info(info, _INDUCING_INFO)
        out[order_d] = outg
        return out, PredictiveCovariance(blocks, _group_index(g.order, g.counts, g.start, g.n_max, dev), g.counts)
    var = torch.empty_like(out)
    ws = torch.empty(int(lib.lvae_predict_var_workspace_size(L, M, P, T, Nt)), dtype=torch.uint8, device=dev)
    rc = lib.lvae_predict_var_f64(*a.head(_lib.ptr(txg), Nt), *groups, *a.params(), _lib.ptr(outg), _lib.ptr(var),
                                  noisy, _lib.ptr(info), _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "predict_var")
    _check_info(info, _INDUCING_INFO)
    out[order_d] = outg
    z_var = torch.empty_like(var)
    z_var[order_d] = var.clamp_(min=0.0)
    return out, z_var


def _exact_inputs(covar_module, likelihoods, prediction_x, test_x, prediction_mu):
    """The arguments of predict_exact as lvae_predict_exact_f64 and its siblings take them: the modules in eval
    mode, everything fp64 on prediction_mu's device"""
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
    return SimpleNamespace(spec=spec, L=L, dev=dev, x=x, tx=tx, mu=mu, p=p, noise=noise, n=n, nt=nt, n_params=n_params)


def _exact_run(lib, a, tx, max_workspace_bytes, size, entry, what, extra, floor=None):
    """The exact route's one driver: plan the dim groups and the test-row chunk under ``max_workspace_bytes``, then
    call ``entry`` once per group of dims.  ``size(dims, chunk)`` is the entry's workspace query.  The dim group is
    sized at the smallest chunk, ``floor`` rows (1 for the variance and the components' covariance, the largest
    group of test rows for the joint covariance); the chunk then starts at all test rows and is halved down to
    ``floor`` while the workspace is too large.  ``floor=None``: the entry takes no chunk.  ``extra(at, l0, chunk)``
    gives the entry's arguments between nt and info for the dims from l0 on, ``at(t, off)`` being the pointer
    ``off`` doubles into t (None without test rows); ``tx`` are the test rows in the order the entry takes them.
    Neither choice changes the bits."""
    L, nt = a.L, a.nt
    group = L
    while group > 1 and size(group, floor or 1) > max_workspace_bytes:
        group -= 1
    chunk = max(nt, 1) if floor else 1
    while floor and chunk > floor and size(group, chunk) > max_workspace_bytes:
        chunk = max((chunk + 1) // 2, floor)
    info = torch.empty(L, dtype=torch.int32, device=a.dev)
    ws = torch.empty(size(group, chunk), dtype=torch.uint8, device=a.dev)
    ptr = lambda t, off: ctypes.c_void_p(t.data_ptr() + 8 * off)
    at = lambda t, off: ptr(t, off) if nt else None
    for l0 in range(0, L, group):
        g = min(group, L - l0)
        rc = entry(a.spec, _lib.ptr(a.x), a.x.stride(0), a.n, g, ptr(a.p, l0 * a.n_params), ptr(a.noise, l0),
                   ptr(a.mu, l0), L, _lib.ptr(tx) if nt else None, tx.stride(0), nt, *extra(at, l0, chunk),
                   ctypes.c_void_p(info.data_ptr() + 4 * l0), _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, what)
    _check_info(info, _EXACT_INFO)


def predict_exact(covar_module, likelihoods, prediction_x, test_x, prediction_mu, max_workspace_bytes=4 << 30,
                  return_var=False, add_noise=False, return_cov=False, groups=None):
    """Z_pred [N_test, L] fp64: the exact-GP posterior mean k(X*, X) (k(X, X) + noise I)^-1 mu per latent dim
    (model_test.py:11-17 predict_gp as MSE_test calls it, model_test.py:65-76), one HIP pass per group of dims
    (lvae_predict_exact_f64) instead of the reference's per-dim explicit inverse and dense [N_test, N] Gram.

    ``covar_module`` is a batched module or a per-dim list (as MSE_test passes), ``prediction_mu`` [N, L] the
    encoder means at ``prediction_x`` [N, Q].  The dims are processed in groups whose workspace (about 8 N^2
    bytes a dim) stays under ``max_workspace_bytes``; a non-positive-definite K raises LinAlgError.

    ``return_var=True`` returns ``(Z_pred, Z_var)``: Z_var [N_test, L] fp64 is the latent functions' predictive
    variance k(x*, x*) - |L^-1 k(X, x*)|^2 (lvae_predict_exact_var_f64), clamped at 0; ``add_noise=True`` adds
    each dim's likelihood noise.  The test rows are then solved in chunks (8 N bytes a row and dim) sized, after
    the dim groups, to keep the workspace under ``max_workspace_bytes``; neither choice changes the bits.

    ``return_cov=True`` returns ``(Z_pred, cov)`` instead: ``cov`` is a PredictiveCovariance whose groups are the
    test rows sharing a label in ``groups`` [N_test] (for example ``test_x[:, id_covariate]``; None: all test rows
    form one group), its blocks k(x*_g, x*_g) - V^T V with V = L^-1 k(X, x*_g) (lvae_predict_exact_cov_f64), not
    clamped; ``add_noise=True`` adds the noise to the diagonals.  A group of more than 128 rows raises ValueError.
    The test rows are solved in chunks of whole groups under ``max_workspace_bytes`` as above (a chunk holds at
    least the largest group); the bits depend on neither the dim groups nor the chunks.  The covariance between
    rows of different groups is not zero and is deliberately not returned: sample_trajectories draws the groups
    independently of each other."""
    if return_var and return_cov:
        raise ValueError("return_var and return_cov are exclusive: cov.diagonal() holds the variances")
    lib = _lib.lib()
    a = _exact_inputs(covar_module, likelihoods, prediction_x, test_x, prediction_mu)
    L, dev, n, nt = a.L, a.dev, a.n, a.nt
    noisy = 1 if add_noise else 0
    if return_cov:
        labels = torch.zeros(nt) if groups is None else groups
        if labels.numel() != nt:
            raise ValueError(f"groups has {labels.numel()} labels for {nt} test rows")
        order, ids, counts, start, n_max = _row_groups(labels, "predict_exact")
        G = int(ids.numel())
        txg = a.tx[order.to(dev)].contiguous()
        outg = torch.empty(nt, L, dtype=torch.float64, device=dev)
        blocks = torch.empty(L, G, n_max, n_max, dtype=torch.float64, device=dev)
        start_h = (ctypes.c_int32 * (G + 1))(*start.tolist())   # host memory: the chunks are cut on the host
        _exact_run(lib, a, txg, max_workspace_bytes,
                   lambda g, c: int(lib.lvae_predict_exact_cov_workspace_size(n, nt, g, c)),
                   lib.lvae_predict_exact_cov_f64, "predict_exact_cov",
                   lambda at, l0, c: (G, ctypes.cast(start_h, ctypes.c_void_p), n_max, at(outg, l0), L,
                                      at(blocks, l0 * G * n_max * n_max), noisy, c), floor=n_max)
        out = torch.empty_like(outg)
        out[order.to(dev)] = outg
        return out, PredictiveCovariance(blocks, _group_index(order, counts, start, n_max, dev), counts)
    out = torch.empty(nt, L, dtype=torch.float64, device=dev)
    if return_var:
        var = torch.empty(nt, L, dtype=torch.float64, device=dev)
        _exact_run(lib, a, a.tx, max_workspace_bytes,
                   lambda g, c: int(lib.lvae_predict_exact_var_workspace_size(n, nt, g, c)),
                   lib.lvae_predict_exact_var_f64, "predict_exact_var",
                   lambda at, l0, c: (at(out, l0), L, at(var, l0), L, noisy, c), floor=1)
        return out, var.clamp_(min=0.0)
    _exact_run(lib, a, a.tx, max_workspace_bytes, lambda g, c: int(lib.lvae_predict_exact_workspace_size(n, nt, g)),
               lib.lvae_predict_exact_f64, "predict_exact", lambda at, l0, c: (at(out, l0), L))
    return out


class LatentComponents:
    """A posterior mean of the latents split by additive component of the kernel: what each covariate effect
    contributes (both predictors are linear in the kernel, so the split is exact).

    ``values`` [R, Nt, L] fp64: component r's share of Z_pred, in the caller's row order.  ``labels`` [R]: the
    component's factors, e.g. ``"rbf(0)"`` or ``"cat(3)*rbf(0)"`` (kind(covariate column); a masked factor carries
    its ``*bin(d)``).  ``module`` [R]: 0 for a component of ``covar_module0`` (or of the exact route's one kernel),
    1 for one of ``covar_module1``; the components of module 0 come first.

    ``cov`` [L, Nt, R, R] fp64 or None (``return_cov=True``): block (l, i) is the joint posterior covariance of the R
    component functions at test row i in latent dim l, the raw difference prior - explained (not clamped),
    symmetric bit for bit; the observation noise belongs to no component and is not in it.  Covariances between
    components at different test rows are not held.  ``variance``, ``total_variance``, ``partial_variance`` and
    ``credible_interval`` read it and raise ValueError without it."""

    def __init__(self, values, labels, module, cov=None):
        self.values, self.labels, self.module, self.cov = values, list(labels), list(module), cov

    def total(self):
        """[Nt, L]: the sum over components, Z_pred up to rounding"""
        return self.values.sum(0)

    def explained_variance(self):
        """[R, L]: the population variance over the test rows of each component, divided by the sum of those
        variances over the components (0 where that sum is 0: every component constant over the rows).  The
        covariances between components are ignored, so the shares describe the components one at a time and do
        not decompose the variance of ``total()``."""
        var = self.values.var(dim=1, unbiased=False) if self.values.shape[1] else self.values.new_zeros(
            self.values.shape[0], self.values.shape[2])
        den = var.sum(0, keepdim=True)
        return torch.where(den > 0, var / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(var))

    def _need_cov(self, what):
        if self.cov is None:
            raise ValueError(f"LatentComponents.{what}() needs the components' covariance: predict with "
                             "return_cov=True")
        return self.cov

    def variance(self):
        """[R, Nt, L]: each component's posterior variance at each test row (the blocks' diagonals), clamped at 0"""
        cov = self._need_cov("variance")
        return torch.diagonal(cov, dim1=2, dim2=3).permute(2, 1, 0).clamp(min=0.0)

    def total_variance(self):
        """[Nt, L]: the sum of a block over both component indices, the predictive variance of the latent function
        itself (``return_var=True`` without noise, up to rounding; not clamped)"""
        return self._need_cov("total_variance").sum(dim=(2, 3)).T

    def partial_variance(self, order=None):
        """[R', Nt, L]: entry k is the posterior variance of the sum of the first k + 1 components of ``order``
        (default: all R as stored, the order of ``generate_component_sequences``), the uncertainty of the
        reconstruction after those effects; with every component in ``order`` the last entry is
        ``total_variance()`` up to rounding.  Clamped at 0."""
        cov = self._need_cov("partial_variance")
        R = int(cov.shape[2])
        order = list(range(R)) if order is None else [int(r) for r in order]
        if not order or any(r < 0 or r >= R for r in order) or len(set(order)) != len(order):
            raise ValueError(f"order {order} must name at least one component, each in 0 .. {R - 1}, none twice")
        idx = torch.tensor(order, dtype=torch.long, device=cov.device)
        sub = cov.index_select(2, idx).index_select(3, idx)
        lead = torch.diagonal(sub.cumsum(2).cumsum(3), dim1=2, dim2=3)      # [L, Nt, R']: the leading blocks' sums
        return lead.permute(2, 1, 0).clamp(min=0.0)

    def credible_interval(self, level=0.95):
        """``(lo, hi)``, each [R, Nt, L]: ``values -+ z sqrt(variance())`` with z the standard normal quantile of
        (1 + level) / 2 (1.959964 at 0.95): each component's marginal credible band at each test row"""
        if not 0.0 < float(level) < 1.0:
            raise ValueError(f"level {level} must lie in (0, 1)")
        var = self.variance()
        z = torch.special.ndtri(torch.tensor(0.5 + 0.5 * float(level), dtype=torch.float64, device=var.device))
        half = z * torch.sqrt(var)
        return self.values - half, self.values + half


def component_labels(covar_module):
    """The labels of a kernel's additive components, from ``kernel.components()`` (a per-dim list: its first
    module's): the factors as kind(column) joined by ``*``."""
    mod = covar_module[0] if isinstance(covar_module, (list, tuple, torch.nn.ModuleList)) else covar_module
    names = {v: k for k, v in _lib.KIND_CODE.items()}
    return ["*".join(f"{names.get(k, k)}({int(d)})" for k, d in facs) for facs, _ in mod.components()]


def predict_exact_components(covar_module, likelihoods, prediction_x, test_x, prediction_mu,
                             max_workspace_bytes=4 << 30, return_cov=False):
    """``(Z_pred, comps)``: ``predict_exact``'s Z_pred [N_test, L] (the same launches, the same bits) and its split
    by additive component of ``covar_module`` as a LatentComponents, ``comps.values[r] = k_r(X*, X) alpha`` with
    alpha = (k(X, X) + noise I)^-1 mu as the mean uses it (lvae_predict_exact_comp_f64: one fused pass over the
    cross-Gram for all components, no [N_test, N] Gram formed).  Arguments, the dim groups under
    ``max_workspace_bytes`` and the errors are ``predict_exact``'s; the groups do not change the bits.

    ``return_cov=True`` also fills ``comps.cov`` [L, N_test, R, R]: per latent dim and test row the joint posterior
    covariance of the R component functions, ``delta_rs k_r(x*, x*) - V_r . V_s`` with V_r = L^-1 k_r(X, x*)
    (lvae_predict_exact_comp_cov_f64; N^2 R N_test flops a dim in the solves, R times the variance's).  The test
    rows are then solved in chunks (8 N R bytes a row and dim) sized, after the dim groups, to keep the workspace
    under ``max_workspace_bytes``; neither choice changes the bits.  With the default nothing new runs and the
    result is today's bit for bit, ``comps.cov`` None."""
    lib = _lib.lib()
    a = _exact_inputs(covar_module, likelihoods, prediction_x, test_x, prediction_mu)
    L, dev, n, nt, R = a.L, a.dev, a.n, a.nt, int(a.spec.n_comp)
    out = torch.empty(nt, L, dtype=torch.float64, device=dev)
    vals = torch.empty(R, nt, L, dtype=torch.float64, device=dev)
    cov = torch.empty(L, nt, R, R, dtype=torch.float64, device=dev) if return_cov else None
    split = lambda at, l0: (at(out, l0), L, at(vals, l0), L, nt * L)
    if return_cov:
        _exact_run(lib, a, a.tx, max_workspace_bytes,
                   lambda g, c: int(lib.lvae_predict_exact_comp_cov_workspace_size(n, nt, g, R, c)),
                   lib.lvae_predict_exact_comp_cov_f64, "predict_exact_comp_cov",
                   lambda at, l0, c: split(at, l0) + (c, at(cov, l0 * nt * R * R)), floor=1)
    else:
        _exact_run(lib, a, a.tx, max_workspace_bytes,
                   lambda g, c: int(lib.lvae_predict_exact_comp_workspace_size(n, nt, g, R)),
                   lib.lvae_predict_exact_comp_f64, "predict_exact_comp", lambda at, l0, c: split(at, l0))
    return out, LatentComponents(vals, component_labels(covar_module), [0] * R, cov)


def batch_predict_components(latent_dim, covar_module0, covar_module1, likelihoods, prediction_x, test_x, mu,
                             zt_list, id_covariate, eps, return_cov=False, max_workspace_bytes=4 << 30):
    """``(Z_pred, comps)``: ``batch_predict_varying_T``'s Z_pred [N_test, L] (the same launches, the same bits) and
    its split by additive component as a LatentComponents: the components of ``covar_module0`` first,
    ``k0_r(X*, z) K0zz^-1 K0zx mu~``, then those of ``covar_module1``, ``k1_r(X*, x) mu~`` over the prediction rows
    of the test subjects (lvae_predict_comp_f64).  Arguments and errors are ``batch_predict_varying_T``'s.

    ``return_cov=True`` also fills ``comps.cov`` [L, N_test, R, R], R = R0 + R1: per latent dim and test row the
    joint posterior covariance of the component functions in the structured model of ``return_var=True``
    (lvae_predict_comp_cov_f64: that route's algebra with one column per (test row, component)).  In that model
    the prior of the shared components is the Nystrom form ``k0_r(x*, z) K0zz^-1 k0_s(z, x*)``, so two different
    components of ``covar_module0`` are correlated already a priori and a shared component's prior variance is not
    ``k0_r(x*, x*)``; the components of ``covar_module1`` keep their own prior ``k1_r(x*, x*)``.  The test rows are
    cut into chunks of whole subjects whose workspace stays under ``max_workspace_bytes`` (a chunk holds at least
    one subject); each chunk repeats the pass over the prediction set, and the chunks do not change the bits.  With
    the default nothing new runs and the result is today's bit for bit, ``comps.cov`` None."""
    lib = _lib.lib()
    a = _inducing_inputs(latent_dim, covar_module0, covar_module1, likelihoods, prediction_x, test_x, mu, zt_list,
                         id_covariate, eps)
    L, M, Q, P, T, Nt, dev = a.L, a.M, a.Q, a.P, a.T, a.Nt, a.dev
    R0, R1 = int(a.spec0.n_comp), int(a.spec1.n_comp)
    R = R0 + R1
    labels = component_labels(covar_module0) + component_labels(covar_module1)
    out = torch.empty(Nt, L, dtype=torch.float64, device=dev)
    vals = torch.empty(R, Nt, L, dtype=torch.float64, device=dev)
    info = torch.empty(L, dtype=torch.int32, device=dev)

    def means(tx_, out_, vals_):
        """lvae_predict_comp_f64 over all test rows ``tx_``"""
        ws = torch.empty(int(lib.lvae_predict_comp_workspace_size(L, M, P, T, Nt, R0, R1)), dtype=torch.uint8,
                         device=dev)
        rc = lib.lvae_predict_comp_f64(*a.head(_lib.ptr(tx_), Nt), *a.params(), _lib.ptr(out_),
                                       _lib.ptr(vals_) if Nt else None, L, Nt * L, _lib.ptr(info), _lib.ptr(ws),
                                       _lib.stream_ptr())
        _lib.check(rc, "predict_comp")

    if not return_cov:
        means(a.tx, out, vals)
        _check_info(info, _INDUCING_INFO)
        return out, LatentComponents(vals, labels, [0] * R0 + [1] * R1)
    # test rows grouped by subject as batch_predict_varying_T(return_var=True) groups them (no cap on a group: no
    # joint covariance over a group's rows is formed)
    g = _subject_groups(test_x[:, id_covariate], a.pred_ids, "batch_predict_components", None)
    G, start = g.G, g.start
    order_d = g.order.to(dev)
    txg = a.tx[order_d].contiguous()
    outg, valsg = torch.empty_like(out), torch.empty_like(vals)
    covg = torch.empty(L, Nt, R, R, dtype=torch.float64, device=dev)
    size = lambda rows: int(lib.lvae_predict_comp_cov_workspace_size(L, M, P, T, rows, R0, R1))
    cuts = [0]   # chunks of whole subject groups: groups cuts[k] .. cuts[k + 1] - 1
    while cuts[-1] < G:
        g1 = cuts[-1] + 1
        while g1 < G and size(int(start[g1 + 1] - start[cuts[-1]])) <= max_workspace_bytes:
            g1 += 1
        cuts.append(g1)

    def call(g0, g1, mean):
        r0, r1 = int(start[g0]), int(start[g1])
        nr = r1 - r0
        gs = (start[g0:g1 + 1] - r0).to(dev)
        sb = g.subj[g0:g1].to(dev)
        cv = covg if nr == Nt else torch.empty(L, nr, R, R, dtype=torch.float64, device=dev)
        ws = torch.empty(size(nr), dtype=torch.uint8, device=dev)
        rc = lib.lvae_predict_comp_cov_f64(*a.head(ctypes.c_void_p(txg.data_ptr() + 8 * r0 * Q) if nr else None, nr,
                                                   mean), g1 - g0, _lib.ptr(sb), _lib.ptr(gs), *a.params(),
                                           _lib.ptr(outg) if mean else None,
                                           _lib.ptr(valsg) if mean and nr else None, L, nr * L,
                                           _lib.ptr(cv) if nr else None, _lib.ptr(info), _lib.ptr(ws),
                                           _lib.stream_ptr())
        _lib.check(rc, "predict_comp_cov")
        if nr != Nt:
            covg[:, r0:r1] = cv

    if len(cuts) <= 2:
        call(0, G, True)   # one chunk (or no test rows): the means and the covariance in one pass
    else:
        # the means by lvae_predict_comp_f64 over all rows (a chunk's own would be the same bits row by row only
        # where the component product cuts its columns the same way), then the chunks' covariances alone
        means(txg, outg, valsg)
        for g0, g1 in zip(cuts[:-1], cuts[1:]):
            call(g0, g1, False)
    _check_info(info, _INDUCING_INFO)
    out[order_d] = outg
    vals[:, order_d] = valsg
    cov = torch.empty_like(covg)
    cov[:, order_d] = covg
    return out, LatentComponents(vals, labels, [0] * R0 + [1] * R1, cov)


def sample_predictions(mean, var, eps=None, generator=None):
    """mean + sqrt(var) * eps, eps ~ N(0, 1) elementwise (drawn with ``generator`` unless given): independent draws
    from each test row's own marginal N(mean, var).  The rows are NOT drawn jointly, so a drawn trajectory is rougher
    than a joint posterior sample: for coherent trajectories take ``return_cov=True`` and ``sample_trajectories``,
    which draws each group's rows (a subject's) jointly from their covariance."""
    if eps is None:
        eps = torch.randn(mean.shape, dtype=mean.dtype, device=mean.device, generator=generator)
    return mean + torch.sqrt(var.clamp(min=0.0)) * eps


def sample_trajectories(mean, cov, num_samples=1, eps=None, generator=None, jitter=1e-8):
    """[S, Nt, L] fp64: S draws in which each group's rows are drawn jointly from N(mean_g, Sigma_g + jitter I),
    ``mean`` [Nt, L] and ``cov`` the PredictiveCovariance a ``return_cov=True`` call returned beside it
    (lvae_predict_sample_f64: the blocks are factored by lvae_potrf_f64, then out[s, r_i, l] = mean[r_i, l] +
    sum_{j <= i} Lc[l, g, i, j] eps[s, r_j, l]).  ``eps`` [S, Nt, L] in the caller's row order holds the standard
    normal draws (drawn with ``generator`` unless given; S is then ``num_samples``).  Groups, like latent dims, are
    drawn independently of each other: the covariance between different groups' rows is not modelled.  ``jitter``
    is added to the blocks' diagonals before the factorisation (rows observed without noise, or duplicated, make a
    block singular); a block that still fails raises torch.linalg.LinAlgError naming its dim and group.  Every test
    row must belong to exactly one group (ValueError otherwise).  With one-row groups and ``jitter=0`` this is
    ``sample_predictions`` to a few ulps."""
    lib = _lib.lib()
    dev = mean.device
    m = mean.detach().to(dev, torch.float64).contiguous()
    Nt, L = int(m.shape[0]), int(m.shape[1])
    blocks = cov.blocks.detach().to(dev, torch.float64).contiguous()
    index = cov.index.to(dev, torch.int32).contiguous()
    G, n_max = int(index.shape[0]), int(blocks.shape[2])
    if blocks.shape != (L, G, n_max, n_max) or index.shape != (G, n_max):
        raise ValueError(f"cov blocks {tuple(blocks.shape)} / index {tuple(index.shape)} do not fit L = {L}")
    rows = index[index >= 0].long()
    if rows.numel() != Nt or (Nt and (int(rows.max()) >= Nt or torch.unique(rows).numel() != Nt)):
        raise ValueError(f"sample_trajectories: cov's groups hold {rows.numel()} rows, not each of the {Nt} test "
                         "rows exactly once")
    if eps is None:
        eps = torch.randn(int(num_samples), Nt, L, dtype=torch.float64, device=dev, generator=generator)
    e = eps.detach().to(dev, torch.float64).contiguous()
    if e.dim() != 3 or e.shape[1:] != (Nt, L):
        raise ValueError(f"eps must be [S, {Nt}, {L}], got {tuple(e.shape)}")
    S = int(e.shape[0])
    out = torch.empty(S, Nt, L, dtype=torch.float64, device=dev)
    if G == 0:
        return out
    info = torch.empty(L * G, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.lvae_predict_sample_workspace_size(L, G, n_max)), dtype=torch.uint8, device=dev)
    rc = lib.lvae_predict_sample_f64(L, G, n_max, Nt, S, _lib.ptr(blocks), _lib.ptr(index), _lib.ptr(m), _lib.ptr(e),
                                     float(jitter), _lib.ptr(out), _lib.ptr(info), _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "predict_sample")
    bad = info.nonzero()
    if bad.numel():
        b = int(bad[0, 0])
        raise torch.linalg.LinAlgError(
            f"sample_trajectories: latent dim {b // G}, group {b % G}: the leading minor of order {int(info[b])} of "
            f"the covariance + {jitter:g} I is not positive-definite")
    return out
