"""Full-batch GP-approximation bounds of one latent dim: ``elbo`` (elbo_functions.py:36-84),
``deviance_upper_bound`` (DUBO, elbo_functions.py:86-142), and of all latent dims at once:
``deviance_upper_bound_batched`` and ``validation_dubo`` (validation.py:8-68).  Same signatures and values as
the reference.

The additive-kernel Grams and every SPD factorisation (K0zz, the per-subject B_p, the M x M
Woodbury matrix W) run in the HIP library: Grams through the differentiable ``covar_module(x1,
x2).evaluate()``, the factorisations through ``spd_inverse`` (lvae_spd_inv_small_f64, one
workgroup per matrix, returning A^-1 and log|A|).  The remaining M x M / T x M products are plain
library GEMMs (rocBLAS via torch.matmul); autograd composes the gradients (d A^-1 = -A^-1 dA A^-1,
d log|A| = tr(A^-1 dA)).  The all-dims DUBO is instead one batched HIP forward and one analytic HIP adjoint
(lvae_dubo_fwd_f64 / lvae_dubo_bwd_f64, csrc/dubo.hip: a fused pass over the subjects), and so is the all-dims,
all-samples ELBO ``elbo_batched`` (lvae_gp_elbo_fwd_f64 / lvae_gp_elbo_bwd_f64, csrc/gp_elbo.hip); the per-dim
functions stay as they are, as their baseline and comparison.

Subjects of varying length (an extension: the reference's two bounds reshape to [P, T]): ``subject_layout``,
``deviance_upper_bound_varying_T`` and ``elbo_varying_T`` lay the batch out as [P, T_max] and run the same two HIP
calls with the padding masked out (lvae_dubo_fwd_seg_f64 ... lvae_gp_elbo_bwd_seg_f64).

The latents of new subjects under a frozen prior (training.py:688-749): ``condition_dubo`` /
``condition_dubo_varying_T`` reduce the joint DUBO of cat(new, train) to a closed form in the new rows
(lvae_dubo_cond_prepare_f64, once) that ``cond(m_new, log_v_new)`` evaluates with one matvec per dim
(lvae_dubo_cond_eval_f64, csrc/dubo_cond.hip).
"""
import math

import torch

from . import _lib
from .elbo import _check_info


class _SpdInvFn(torch.autograd.Function):
    """(A^-1, log|A|) of a batch of SPD matrices [..., n, n], n <= 128 (HIP, fp64)."""

    @staticmethod
    def forward(ctx, A):
        lib = _lib.lib()
        n = A.shape[-1]
        lead = A.shape[:-2]
        Ab = A.detach().to(torch.float64).reshape(-1, n, n).contiguous()
        b = Ab.shape[0]
        Ai = torch.empty_like(Ab)
        ld = torch.empty(b, dtype=torch.float64, device=A.device)
        info = torch.empty(b, dtype=torch.int32, device=A.device)
        rc = lib.lvae_spd_inv_small_f64(n, b, _lib.ptr(Ab), n * n, _lib.ptr(Ai), n * n, _lib.ptr(ld), _lib.ptr(info),
                                        _lib.stream_ptr())
        _lib.check(rc, "spd_inv_small")
        _check_info(info, "cholesky")
        Ai = Ai.reshape(A.shape)
        ctx.save_for_backward(Ai)
        return Ai, ld.reshape(lead)

    @staticmethod
    def backward(ctx, g_inv, g_ld):
        (Ai,) = ctx.saved_tensors
        dA = torch.zeros_like(Ai)
        if g_inv is not None:
            dA = dA - Ai @ g_inv @ Ai
        if g_ld is not None:
            dA = dA + g_ld[..., None, None] * Ai
        return dA


def spd_inverse(A):
    """(A^-1, log|A|) for SPD A [..., n, n] (n <= 128), differentiable."""
    return _SpdInvFn.apply(A)


def _common(covar_module0, covar_module1, likelihood, train_xt, z, P, T, eps):
    dt = torch.float64
    M = z.shape[-2]
    x = train_xt.to(dt)
    x_st = x.reshape(P, T, x.shape[-1])
    K0xz = covar_module0(x, z).evaluate()
    K0zz = covar_module0(z, z).evaluate() + eps * torch.eye(M, dtype=dt, device=x.device)
    iK, ldK = spd_inverse(K0zz)
    K0_st = covar_module0(x_st, x_st).evaluate()
    B_st = covar_module1(x_st, x_st).evaluate() + torch.eye(T, dtype=dt, device=x.device) * \
        likelihood.noise_covar.noise.reshape(-1)[0]
    iB, ldB = spd_inverse(B_st)
    iBK = iB @ K0xz.reshape(P, T, M)
    Q = K0xz.transpose(-1, -2) @ iBK.reshape(P * T, M)
    W = K0zz + Q
    W = 0.5 * (W + W.transpose(-1, -2))
    iW, ldW = spd_inverse(W)
    logdet = -ldK + ldB.sum() + ldW
    tr = (iB * K0_st).sum() - (Q * iK).sum()
    return dict(K0xz=K0xz, iB=iB, iBK=iBK, iW=iW, logdet=logdet, tr=tr, M=M)


def _quad(c, y, P, T):
    y_st = y.reshape(P, T, 1)
    iBy = c["iB"] @ y_st
    q1 = (y_st * iBy).sum()
    p = c["K0xz"].transpose(-1, -2) @ iBy.reshape(P * T)
    return q1 - p @ (c["iW"] @ p)


def elbo(covar_module0, covar_module1, likelihood, train_xt, train_yt, z, P, T, eps):
    """log N(y | 0, K0xz K0zz^-1 K0zx + B) - 1/2 tr(...) of one latent dim (elbo_functions.py:36-84)."""
    c = _common(covar_module0, covar_module1, likelihood, train_xt, z, P, T, eps)
    y = train_yt.to(torch.float64)
    loglike = -0.5 * T * P * math.log(2 * math.pi) - 0.5 * (c["logdet"] + _quad(c, y, P, T))
    return loglike - 0.5 * c["tr"]


def deviance_upper_bound(covar_module0, covar_module1, likelihood, train_xt, m, log_v, z, P, T, eps):
    """DUBO of one latent dim from the variational mean / log-variance (elbo_functions.py:86-142)."""
    c = _common(covar_module0, covar_module1, likelihood, train_xt, z, P, T, eps)
    m = m.to(torch.float64)
    log_v = log_v.to(torch.float64)
    v = torch.exp(log_v)
    v_st = v.reshape(P, T)
    tr_iB_D = (torch.diagonal(c["iB"], dim1=-2, dim2=-1) * v_st).sum()
    Dh = (c["iBK"] * torch.sqrt(v_st)[:, :, None]).reshape(P * T, c["M"])
    tr2 = (c["iW"] * (Dh.transpose(0, 1) @ Dh)).sum()
    return 0.5 * ((tr_iB_D - tr2) + _quad(c, m, P, T) - P * T + c["logdet"] - log_v.sum() + c["tr"])


def _f64(t):
    return t.detach().to(torch.float64).contiguous()


def _bound_fwd(name, what, fwd, ws_bytes, out_shape, spec0, spec1, dims, params0, params1, noise, x, z, data):
    """One all-dims forward (lvae_dubo_fwd_f64 / lvae_gp_elbo_fwd_f64) on fp64 copies of the inputs: ``data`` are the
    call's own tensors between z and params0.  Returns (out, the tensors the backward needs: p0, p1, nz, x, z, *data,
    workspace)."""
    p0, p1, nz, x64, z64 = _f64(params0), _f64(params1), _f64(noise).reshape(-1), _f64(x), _f64(z)
    d64 = [_f64(t) for t in data]
    dev = d64[0].device
    ws = torch.empty(int(ws_bytes(dims)), dtype=torch.uint8, device=dev)
    out = torch.empty(out_shape, dtype=torch.float64, device=dev)
    info = torch.empty(dims.L, dtype=torch.int32, device=dev)
    rc = fwd(spec0, spec1, dims, _lib.ptr(x64), _lib.ptr(z64), *[_lib.ptr(t) for t in d64], _lib.ptr(p0),
             _lib.ptr(p1), _lib.ptr(nz), _lib.ptr(out), _lib.ptr(info), _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, name + "_fwd")
    _check_info(info, what + " cholesky (10000+col: K0zz, 20000+col: B_st, 30000+col: W)")
    return out, (p0, p1, nz, x64, z64, *d64, ws)


def _bound_dz(name, bwd_z, spec0, dims, x64, z64, p0, ws, N, z_dtype):
    """dz [L, M, Q] of one bound (lvae_dubo_bwd_z_f64 / lvae_gp_elbo_bwd_z_f64 / lvae_hensman_bwd_z_f64) from the
    cotangents its backward has just left in ``ws``, in z's dtype."""
    lib = _lib.lib()
    zws = torch.empty(int(lib.lvae_bound_dz_workspace_size(dims.L, dims.M, int(N), dims.Q)), dtype=torch.uint8,
                      device=z64.device)
    dz = torch.empty_like(z64)
    rc = bwd_z(spec0, dims, _lib.ptr(x64), _lib.ptr(z64), _lib.ptr(p0), _lib.ptr(dz), _lib.ptr(ws), _lib.ptr(zws),
               _lib.stream_ptr())
    _lib.check(rc, name + "_bwd_z")
    return dz.to(z_dtype)


def _with_seg(fn, seg):
    """A lvae_*_seg_f64 call with its seg_len argument (device int32 [P], after the dims) filled in: the argument
    list of the uniform call"""
    return lambda spec0, spec1, dims, *rest: fn(spec0, spec1, dims, _lib.ptr(seg), *rest)


def _cast_back(ctx, dp0, dp1, dnz):
    """(dparams0, dparams1, dnoise) in the dtypes (and the noise's shape) the forward was given"""
    t0, t1, tn, nshape = ctx.dtypes[:4]
    return dp0.to(t0), dp1.to(t1), dnz.to(tn).reshape(nshape)


class _DuboFn(torch.autograd.Function):
    """dubo [L] of all latent dims in one batched HIP pass (lvae_dubo_fwd_f64) with its analytic adjoint
    (lvae_dubo_bwd_f64); a z that requires grad adds lvae_dubo_bwd_z_f64 (nothing runs for one that does not)."""

    @staticmethod
    def forward(ctx, params0, params1, noise, mu, logv, x, z, spec0, spec1, dims, seg=None):
        lib = _lib.lib()
        fwd = lib.lvae_dubo_fwd_f64 if seg is None else _with_seg(lib.lvae_dubo_fwd_seg_f64, seg)
        dubo, saved = _bound_fwd("dubo", "deviance_upper_bound", fwd, lib.lvae_dubo_workspace_size,
                                 dims.L, spec0, spec1, dims, params0, params1, noise, x, z, (mu, logv))
        ctx.save_for_backward(*saved)
        ctx.seg = seg
        ctx.spec0, ctx.spec1, ctx.dims = spec0, spec1, dims
        ctx.dtypes = (params0.dtype, params1.dtype, noise.dtype, noise.shape, mu.dtype, logv.dtype)
        ctx.z_dtype = z.dtype
        return dubo

    @staticmethod
    def backward(ctx, gdubo):
        lib = _lib.lib()
        p0, p1, nz, x64, z64, mu64, lv64, ws = ctx.saved_tensors
        g = _f64(gdubo).reshape(-1)
        dmu, dlv = torch.empty_like(mu64), torch.empty_like(lv64)
        dp0, dp1, dnz = torch.empty_like(p0), torch.empty_like(p1), torch.empty_like(nz)
        bwd = lib.lvae_dubo_bwd_f64 if ctx.seg is None else _with_seg(lib.lvae_dubo_bwd_seg_f64, ctx.seg)
        rc = bwd(ctx.spec0, ctx.spec1, ctx.dims, _lib.ptr(x64), _lib.ptr(z64), _lib.ptr(mu64), _lib.ptr(lv64),
                 _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(nz), _lib.ptr(g), _lib.ptr(dmu), _lib.ptr(dlv), _lib.ptr(dp0),
                 _lib.ptr(dp1), _lib.ptr(dnz), _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, "dubo_bwd")
        tmu, tlv = ctx.dtypes[4:]
        dz = None
        if ctx.needs_input_grad[6]:
            dz = _bound_dz("dubo", lib.lvae_dubo_bwd_z_f64, ctx.spec0, ctx.dims, x64, z64, p0, ws,
                           ctx.dims.P * ctx.dims.T, ctx.z_dtype)
        return (*_cast_back(ctx, dp0, dp1, dnz), dmu.to(tmu), dlv.to(tlv), None, dz, None, None, None, None)


def _dubo_noise(likelihoods, L):
    """[L] noise of a batched likelihood (noise_covar.noise [L, 1] or [1]) or of a list of per-dim ones."""
    if isinstance(likelihoods, (list, tuple, torch.nn.ModuleList)):
        return torch.cat([lk.noise_covar.noise.reshape(-1)[:1] for lk in likelihoods]).reshape(L)
    nz = likelihoods.noise_covar.noise.reshape(-1)
    return nz.expand(L) if nz.numel() == 1 else nz.reshape(L)


def _batched_kernels(L, covar_module0, covar_module1, z, train_xt, P, T):
    """(spec0, params0 [L, P0], spec1, params1 [L, P1], z [L, M, Q]) of the all-dims calls from batched modules or
    per-dim lists and z as [L, M, Q], [M, Q] (shared) or a per-dim list; ValueError on mismatched shapes.  P None:
    subjects of varying length, the caller checks the rows against its layout."""
    from .elbo import _stack_modules
    spec0, params0 = _stack_modules(covar_module0)
    spec1, params1 = _stack_modules(covar_module1)
    if params0.shape[0] == 1 and L > 1:
        params0 = params0.expand(L, -1)
    if params1.shape[0] == 1 and L > 1:
        params1 = params1.expand(L, -1)
    if params0.shape[0] != L or params1.shape[0] != L:
        raise ValueError(f"kernel batches {params0.shape[0]}, {params1.shape[0]} != latent dims {L}")
    if isinstance(z, (list, tuple)):
        z = torch.stack([zi.reshape(zi.shape[-2], zi.shape[-1]) for zi in z], 0)
    if z.dim() not in (2, 3):
        raise ValueError(f"z must be [L, M, Q], [M, Q] or a per-dim list, got {tuple(z.shape)}")
    zz = z if z.dim() == 3 else z.unsqueeze(0).expand(L, -1, -1)
    if zz.shape[0] != L:
        raise ValueError(f"z has {zz.shape[0]} dims, expected {L}")
    if P is not None and train_xt.shape[0] != P * T:
        raise ValueError(f"train_xt has {train_xt.shape[0]} rows, expected P*T = {P * T}")
    return spec0, params0, spec1, params1, zz


def deviance_upper_bound_batched(latent_dim, covar_module0, covar_module1, likelihoods, train_xt, m, log_v, z, P, T,
                                 eps):
    """The DUBO of every latent dim, [L] fp64, from one batched HIP forward (and one batched adjoint):
    ``deviance_upper_bound`` for dim l on (m[:, l], log_v[:, l]).  covar_module0 / covar_module1: batched
    modules or per-dim lists; likelihoods: a batched likelihood or a per-dim list; z: [L, M, Q], [M, Q]
    (shared) or a per-dim list of [M, Q].  Gradients flow to m, log_v [N, L], the kernels' raw parameters,
    the noise, and to z in any of its forms when it requires grad (learnable inducing points; zero for the
    columns of categorical / binary factors, as the reference's autograd)."""
    L = int(latent_dim)
    spec0, params0, spec1, params1, zz = _batched_kernels(L, covar_module0, covar_module1, z, train_xt, P, T)
    if tuple(m.shape) != (P * T, L) or tuple(log_v.shape) != (P * T, L):
        raise ValueError(f"m / log_v must be [{P * T}, {L}]")
    noise = _dubo_noise(likelihoods, L).to(m.device)
    dims = _lib.DuboDims(L, int(zz.shape[-2]), int(P), int(T), int(train_xt.shape[-1]), float(eps))
    return _DuboFn.apply(params0, params1, noise, m, log_v, train_xt, zz, spec0, spec1, dims, None)


def validation_dubo(latent_dim, covar_module0, covar_module1, likelihood, train_xt, m, log_v, z, P, T, eps):
    """Sum over the latent dims of the DUBO with batched kernels (validation.py:8-68); m / log_v
    [N, L], z [L, M, Q].  Returns a [1] tensor like the reference.  One batched call
    (deviance_upper_bound_batched) for all dims."""
    L = int(latent_dim)
    return deviance_upper_bound_batched(L, covar_module0, covar_module1, likelihood, train_xt, m, log_v, z, P, T,
                                        eps).sum().reshape(1)



class _GpElboFn(torch.autograd.Function):
    """elbo [S, L] of all latent dims and S <= 16 samples in one batched HIP pass (lvae_gp_elbo_fwd_f64) with its
    analytic adjoint (lvae_gp_elbo_bwd_f64); a z that requires grad adds lvae_gp_elbo_bwd_z_f64 (nothing runs for
    one that does not)."""

    @staticmethod
    def forward(ctx, params0, params1, noise, y, x, z, spec0, spec1, dims, seg=None):
        lib = _lib.lib()
        fwd = lib.lvae_gp_elbo_fwd_f64 if seg is None else _with_seg(lib.lvae_gp_elbo_fwd_seg_f64, seg)
        out, saved = _bound_fwd("gp_elbo", "elbo_batched", fwd, lib.lvae_gp_elbo_workspace_size,
                                (dims.S, dims.L), spec0, spec1, dims, params0, params1, noise, x, z, (y,))
        ctx.save_for_backward(*saved)
        ctx.seg = seg
        ctx.spec0, ctx.spec1, ctx.dims = spec0, spec1, dims
        ctx.dtypes = (params0.dtype, params1.dtype, noise.dtype, noise.shape, y.dtype)
        ctx.z_dtype = z.dtype
        return out

    @staticmethod
    def backward(ctx, gelbo):
        lib = _lib.lib()
        p0, p1, nz, x64, z64, y64, ws = ctx.saved_tensors
        g = _f64(gelbo)
        dy = torch.empty_like(y64)
        dp0, dp1, dnz = torch.empty_like(p0), torch.empty_like(p1), torch.empty_like(nz)
        bwd = lib.lvae_gp_elbo_bwd_f64 if ctx.seg is None else _with_seg(lib.lvae_gp_elbo_bwd_seg_f64, ctx.seg)
        rc = bwd(ctx.spec0, ctx.spec1, ctx.dims, _lib.ptr(x64), _lib.ptr(z64), _lib.ptr(y64), _lib.ptr(p0),
                 _lib.ptr(p1), _lib.ptr(nz), _lib.ptr(g), _lib.ptr(dy), _lib.ptr(dp0), _lib.ptr(dp1), _lib.ptr(dnz),
                 _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, "gp_elbo_bwd")
        dz = None
        if ctx.needs_input_grad[5]:
            dz = _bound_dz("gp_elbo", lib.lvae_gp_elbo_bwd_z_f64, ctx.spec0, ctx.dims, x64, z64, p0, ws,
                           ctx.dims.P * ctx.dims.T, ctx.z_dtype)
        return (*_cast_back(ctx, dp0, dp1, dnz), dy.to(ctx.dtypes[4]), None, dz, None, None, None, None)


ELBO_MAX_SAMPLES = 16   # samples of one lvae_gp_elbo_* call (the columns of one MFMA tile)


def elbo_batched(latent_dim, covar_module0, covar_module1, likelihoods, train_xt, train_yt, z, P, T, eps):
    """``elbo`` of every latent dim and every sample at once, fp64: train_yt [N, L] -> [L], or [S, N, L] (S draws
    of the latent) -> [S, L], entry (s, l) = ``elbo`` for dim l on train_yt[s, :, l].  One batched HIP forward and
    one analytic adjoint per group of at most 16 samples (a dim's samples share its Grams and factorisations).
    covar_module0 / covar_module1: batched modules or per-dim lists; likelihoods: a batched likelihood or a
    per-dim list; z: [L, M, Q], [M, Q] (shared) or a per-dim list of [M, Q].  Gradients flow to train_yt, the
    kernels' raw parameters, the noise, and to z in any of its forms when it requires grad (each group of samples
    adds its own share; autograd sums them)."""
    L = int(latent_dim)
    spec0, params0, spec1, params1, zz = _batched_kernels(L, covar_module0, covar_module1, z, train_xt, P, T)
    single = train_yt.dim() == 2
    y = train_yt.unsqueeze(0) if single else train_yt
    if y.dim() != 3 or y.shape[0] < 1 or tuple(y.shape[1:]) != (P * T, L):
        raise ValueError(f"train_yt must be [{P * T}, {L}] or [S, {P * T}, {L}], got {tuple(train_yt.shape)}")
    noise = _dubo_noise(likelihoods, L).to(y.device)
    M, Q = int(zz.shape[-2]), int(train_xt.shape[-1])
    out = []
    for s0 in range(0, y.shape[0], ELBO_MAX_SAMPLES):
        ys = y[s0:s0 + ELBO_MAX_SAMPLES]
        dims = _lib.GpElboDims(L, M, int(P), int(T), Q, int(ys.shape[0]), float(eps))
        out.append(_GpElboFn.apply(params0, params1, noise, ys, train_xt, zz, spec0, spec1, dims, None))
    res = out[0] if len(out) == 1 else torch.cat(out, 0)
    return res[0] if single else res


class SubjectLayout:
    """The [P, T_max] layout of a batch whose subjects differ in length (``subject_layout``): subject p, in
    torch.unique order of the ids, has its ``seg_len[p]`` rows first, in the order they appear in the batch, and
    padding after them.  ``gather`` [P * T_max] int64: the batch row of every slot (a padding slot points at its
    subject's first row, so that padded covariates are real ones); ``valid`` [P * T_max] bool; ``seg_len`` [P]
    int32.  All three live on the device given; ``P``, ``T_max`` and ``N`` (the rows of the batch) are ints."""

    def __init__(self, gather, valid, seg_len, T_max, N):
        self.gather, self.valid, self.seg_len = gather, valid, seg_len
        self.P, self.T_max, self.N = int(seg_len.numel()), int(T_max), int(N)

    def to(self, device):
        return SubjectLayout(self.gather.to(device), self.valid.to(device), self.seg_len.to(device), self.T_max,
                             self.N)


def subject_layout(ids, device=None):
    """``SubjectLayout`` of a batch from its id column (one host round trip over ``ids``; rows of a subject may
    stand anywhere in the batch).  ``device``: where gather / valid / seg_len go (default: that of ``ids``)."""
    from .elbo import _subject_layout
    gather, valid, seg, T_max = _subject_layout(ids)
    dev = ids.device if device is None else device
    return SubjectLayout(gather.to(dev), valid.to(dev), seg.to(dev), T_max, ids.shape[0])


VARYING_T_MAX = 128   # longest subject of the varying-length calls (the T limit of lvae_dubo_dims / lvae_gp_elbo_dims)


def _varying_layout(train_xt, id_covariate, layout, n_rows, what):
    lay = subject_layout(train_xt[:, id_covariate]) if layout is None else layout
    if lay.N != train_xt.shape[0] or n_rows != lay.N:
        raise ValueError(f"{what}: the layout has {lay.N} rows, train_xt {train_xt.shape[0]}, the data {n_rows}")
    if lay.T_max > VARYING_T_MAX:
        raise ValueError(f"{what}: a subject has {lay.T_max} rows, at most {VARYING_T_MAX} are supported")
    if lay.gather.device != train_xt.device:
        lay = lay.to(train_xt.device)
    return lay


def deviance_upper_bound_varying_T(latent_dim, covar_module0, covar_module1, likelihoods, train_xt, m, log_v, z,
                                   id_covariate, eps, layout=None):
    """``deviance_upper_bound_batched`` for subjects of varying length (an extension: the reference's DUBO needs P
    subjects of T rows): [L] fp64.  The subjects are the distinct values of train_xt[:, id_covariate]; their rows
    may stand in any order.  The batch is laid out as [P, T_max] (``subject_layout``) and runs through the same HIP
    kernels with the padding masked out (lvae_dubo_fwd_seg_f64 / lvae_dubo_bwd_seg_f64); N of the bound is the
    number of rows.  Modules, likelihoods and z in every form ``deviance_upper_bound_batched`` takes; gradients
    flow to the caller's rows of m / log_v [N, L] where they stand, to the kernels, the noise and a z that requires
    grad.  ``layout``: a ``subject_layout`` of this batch's id column, to skip the host round trip over it.
    ValueError when a subject has more than 128 rows."""
    L = int(latent_dim)
    spec0, params0, spec1, params1, zz = _batched_kernels(L, covar_module0, covar_module1, z, train_xt, None, None)
    N = train_xt.shape[0]
    if tuple(m.shape) != (N, L) or tuple(log_v.shape) != (N, L):
        raise ValueError(f"m / log_v must be [{N}, {L}]")
    lay = _varying_layout(train_xt, id_covariate, layout, N, "deviance_upper_bound_varying_T")
    noise = _dubo_noise(likelihoods, L).to(m.device)
    dims = _lib.DuboDims(L, int(zz.shape[-2]), lay.P, lay.T_max, int(train_xt.shape[-1]), float(eps))
    # (the padding slots repeat a row of m / log_v that the kernels never read; their cotangent is an exact 0)
    return _DuboFn.apply(params0, params1, noise, m.index_select(0, lay.gather), log_v.index_select(0, lay.gather),
                         train_xt.detach().index_select(0, lay.gather), zz, spec0, spec1, dims, lay.seg_len)


def elbo_varying_T(latent_dim, covar_module0, covar_module1, likelihoods, train_xt, train_yt, z, id_covariate, eps,
                   layout=None):
    """``elbo_batched`` for subjects of varying length (an extension, as ``deviance_upper_bound_varying_T``):
    train_yt [N, L] -> [L], or [S, N, L] -> [S, L], one batched HIP forward and one adjoint per group of at most 16
    samples (lvae_gp_elbo_fwd_seg_f64 / lvae_gp_elbo_bwd_seg_f64).  Gradients flow to the caller's rows of train_yt
    where they stand, to the kernels, the noise and a z that requires grad."""
    L = int(latent_dim)
    spec0, params0, spec1, params1, zz = _batched_kernels(L, covar_module0, covar_module1, z, train_xt, None, None)
    N = train_xt.shape[0]
    single = train_yt.dim() == 2
    y = train_yt.unsqueeze(0) if single else train_yt
    if y.dim() != 3 or y.shape[0] < 1 or tuple(y.shape[1:]) != (N, L):
        raise ValueError(f"train_yt must be [{N}, {L}] or [S, {N}, {L}], got {tuple(train_yt.shape)}")
    lay = _varying_layout(train_xt, id_covariate, layout, N, "elbo_varying_T")
    noise = _dubo_noise(likelihoods, L).to(y.device)
    M, Q = int(zz.shape[-2]), int(train_xt.shape[-1])
    x_pad = train_xt.detach().index_select(0, lay.gather)
    y_pad = y.index_select(1, lay.gather)
    out = []
    for s0 in range(0, y.shape[0], ELBO_MAX_SAMPLES):
        ys = y_pad[s0:s0 + ELBO_MAX_SAMPLES]
        dims = _lib.GpElboDims(L, M, lay.P, lay.T_max, Q, int(ys.shape[0]), float(eps))
        out.append(_GpElboFn.apply(params0, params1, noise, ys, x_pad, zz, spec0, spec1, dims, lay.seg_len))
    res = out[0] if len(out) == 1 else torch.cat(out, 0)
    return res[0] if single else res


# ------------------------------------------------------------------------------------------------------
# the DUBO conditioned on a frozen prior: the latents of new subjects (training.py:688-749)
# ------------------------------------------------------------------------------------------------------
class _DuboCondFn(torch.autograd.Function):
    """dubo [L] of the conditioned bound (lvae_dubo_cond_eval_f64): the forward computes the values and the
    unit-cotangent gradients in one call, the backward scales them."""

    @staticmethod
    def forward(ctx, m, logv, cond):
        lib = _lib.lib()
        m64, lv64 = _f64(m), _f64(logv)
        dubo = torch.empty(cond.L, dtype=torch.float64, device=m64.device)
        dm, dlv = torch.empty_like(m64), torch.empty_like(lv64)
        rc = lib.lvae_dubo_cond_eval_f64(cond.L, cond.Pn, cond.T, _lib.ptr(cond.state), _lib.ptr(m64), _lib.ptr(lv64),
                                         None, _lib.ptr(dubo), _lib.ptr(dm), _lib.ptr(dlv), _lib.stream_ptr())
        _lib.check(rc, "dubo_cond_eval")
        ctx.save_for_backward(dm, dlv)
        ctx.dtypes = (m.dtype, logv.dtype)
        return dubo

    @staticmethod
    def backward(ctx, gdubo):
        dm, dlv = ctx.saved_tensors
        g = gdubo.detach().to(torch.float64).reshape(1, -1)
        return (dm * g).to(ctx.dtypes[0]), (dlv * g).to(ctx.dtypes[1]), None


class DuboCondition:
    """The joint DUBO as a function of the new subjects' latents alone (``condition_dubo``): ``cond(m_new,
    log_v_new)`` -> [L] fp64.  ``L``, ``Pn`` (new subjects), ``T`` (rows per subject of the state: T, or the longest
    subject) and ``Nn`` (the rows the caller passes) are ints; ``state`` is the device buffer
    lvae_dubo_cond_prepare_f64 filled, owned by this object; ``gather`` (varying length only): the caller's row of
    every state row."""

    def __init__(self, L, Pn, T, Nn, state, gather=None):
        self.L, self.Pn, self.T, self.Nn = int(L), int(Pn), int(T), int(Nn)
        self.state, self.gather = state, gather

    def __call__(self, m_new, log_v_new):
        if tuple(m_new.shape) != (self.Nn, self.L) or tuple(log_v_new.shape) != (self.Nn, self.L):
            raise ValueError(f"m_new / log_v_new must be [{self.Nn}, {self.L}]")
        if self.gather is not None:
            # (the padding slots repeat a row the kernel never reads; their cotangent is an exact 0)
            m_new, log_v_new = m_new.index_select(0, self.gather), log_v_new.index_select(0, self.gather)
        return _DuboCondFn.apply(m_new, log_v_new, self)


def _condition(L, spec0, params0, spec1, params1, zz, noise, x, mu, logv, P, T, seg, free_idx, eps):
    """lvae_dubo_cond_prepare_f64 on the joint [P, T] batch (everything detached); returns (state, Pn)"""
    lib = _lib.lib()
    p0, p1, nz, x64, z64, mu64, lv64 = (_f64(params0), _f64(params1), _f64(noise).reshape(-1), _f64(x), _f64(zz),
                                        _f64(mu), _f64(logv))
    dev = x64.device
    dims = _lib.DuboDims(L, int(zz.shape[-2]), int(P), int(T), int(x.shape[-1]), float(eps))
    Pn = int(free_idx.numel())
    free = free_idx.to(device=dev, dtype=torch.int32).contiguous()
    ws = torch.empty(int(lib.lvae_dubo_workspace_size(dims)), dtype=torch.uint8, device=dev)
    state = torch.empty(int(lib.lvae_dubo_cond_state_size(L, Pn, int(T))), dtype=torch.uint8, device=dev)
    info = torch.empty(L, dtype=torch.int32, device=dev)
    rc = lib.lvae_dubo_cond_prepare_f64(spec0, spec1, dims, _lib.ptr(seg), Pn, _lib.ptr(free), _lib.ptr(x64),
                                        _lib.ptr(z64), _lib.ptr(mu64), _lib.ptr(lv64), _lib.ptr(p0), _lib.ptr(p1),
                                        _lib.ptr(nz), _lib.ptr(state), _lib.ptr(info), _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "dubo_cond_prepare")
    _check_info(info, "condition_dubo cholesky (10000+col: K0zz, 20000+col: B_st, 30000+col: W)")
    return state, Pn


def _cond_joint(L, x_new, x_train, m_train, log_v_train):
    if x_new.shape[0] < 1:
        raise ValueError("x_new has no rows")
    Nt = x_train.shape[0]
    if tuple(m_train.shape) != (Nt, L) or tuple(log_v_train.shape) != (Nt, L):
        raise ValueError(f"m_train / log_v_train must be [{Nt}, {L}]")
    zeros = torch.zeros(x_new.shape[0], L, dtype=torch.float64, device=x_new.device)
    x = torch.cat([x_new.detach(), x_train.detach().to(x_new.dtype)], 0)
    return x, torch.cat([zeros, _f64(m_train)], 0), torch.cat([zeros, _f64(log_v_train)], 0)


def condition_dubo(latent_dim, covar_module0, covar_module1, likelihoods, x_new, x_train, m_train, log_v_train, z, T,
                   eps):
    """The DUBO of ``cat(new, train)`` with everything but the new subjects' latents frozen (the loss of the second
    half of variational_inference_optimization, training.py:688-749): returns ``cond`` (a ``DuboCondition``) with
    ``cond(m_new, log_v_new)`` [L] fp64 equal to ``deviance_upper_bound_batched`` on cat(x_new, x_train),
    cat(m_new, m_train), cat(log_v_new, log_v_train) with Pn + P subjects of T rows -- values and the gradients
    with respect to m_new / log_v_new [Pn * T, L], in the caller's dtype.

    THE PRIOR IS FROZEN: nothing flows to the kernels, the noise, z or the training latents, whatever requires
    grad; they are read once, here.  With them fixed the joint bound is an exact quadratic-plus-exponential form in
    the new rows (csrc/dubo_cond.hip): this call costs about one DUBO forward (lvae_dubo_cond_prepare_f64), every
    ``cond(...)`` after it is one symmetric [Pn T, Pn T] matvec per latent dim (lvae_dubo_cond_eval_f64) whose cost
    no longer depends on the training set or on M.  Modules, likelihoods and z in every form
    ``deviance_upper_bound_batched`` takes; x_train may have no rows (every subject new)."""
    L, T = int(latent_dim), int(T)
    if x_new.shape[0] % T or x_train.shape[0] % T:
        raise ValueError(f"x_new / x_train must hold whole subjects of T = {T} rows")
    x, mu, logv = _cond_joint(L, x_new, x_train, m_train, log_v_train)
    P, Pn = x.shape[0] // T, x_new.shape[0] // T
    spec0, params0, spec1, params1, zz = _batched_kernels(L, covar_module0, covar_module1, z, x, P, T)
    noise = _dubo_noise(likelihoods, L).to(x.device)
    state, _ = _condition(L, spec0, params0, spec1, params1, zz, noise, x, mu, logv, P, T, None,
                          torch.arange(Pn, dtype=torch.int32), eps)
    return DuboCondition(L, Pn, T, Pn * T, state)


def condition_dubo_varying_T(latent_dim, covar_module0, covar_module1, likelihoods, x_new, x_train, m_train,
                             log_v_train, z, id_covariate, eps):
    """``condition_dubo`` for subjects of varying length: ``cond(m_new, log_v_new)`` equals
    ``deviance_upper_bound_varying_T`` on the joint batch, values and gradients in the caller's row order.  The
    subjects are the distinct values of the id column; the joint ``subject_layout`` is built here.  The prior is
    frozen as in ``condition_dubo``.  ValueError when a new id also occurs in x_train, or a subject has more than 128
    rows."""
    L = int(latent_dim)
    x, mu, logv = _cond_joint(L, x_new, x_train, m_train, log_v_train)
    n_new = x_new.shape[0]
    ids_new = torch.unique(x_new[:, id_covariate].detach())
    if x_train.shape[0] and bool(torch.isin(ids_new, x_train[:, id_covariate].detach().to(ids_new.dtype)).any()):
        raise ValueError("condition_dubo_varying_T: a new subject's id also occurs in x_train")
    spec0, params0, spec1, params1, zz = _batched_kernels(L, covar_module0, covar_module1, z, x, None, None)
    lay = _varying_layout(x, id_covariate, None, x.shape[0], "condition_dubo_varying_T")
    # subjects stand in torch.unique order of the ids: the new ones keep that order among themselves
    ids_all = torch.unique(x[:, id_covariate])
    free_idx = torch.nonzero(torch.isin(ids_all, ids_new.to(ids_all.device))).reshape(-1)
    noise = _dubo_noise(likelihoods, L).to(x.device)
    state, Pn = _condition(L, spec0, params0, spec1, params1, zz, noise, x.index_select(0, lay.gather),
                           mu.index_select(0, lay.gather), logv.index_select(0, lay.gather), lay.P, lay.T_max,
                           lay.seg_len, free_idx, eps)
    gather = lay.gather.reshape(lay.P, lay.T_max).index_select(0, free_idx.to(lay.gather.device)).reshape(-1)
    return DuboCondition(L, Pn, lay.T_max, n_new, state, gather.contiguous())
