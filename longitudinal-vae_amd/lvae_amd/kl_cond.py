"""The latents of new rows under a model trained with the exact N x N prior KL (``KL_closed``): what
``condition_dubo`` is to a DUBO-trained model.  ``condition_kl_closed`` folds the trained prior and the training
latents into the closed form lvae_dubo_cond_eval_f64 evaluates (csrc/kl_cond.hip, lvae_kl_cond_prepare_f64), and
steps.LatentInferenceStep / steps.infer_new_subjects run the reference's Adam loop on it.
"""
import ctypes

import torch

from . import _lib
from .elbo import _check_info
from .gpapprox import DuboCondition
from .predict import _exact_inputs

_KL_COND_INFO = ("condition_kl_closed cholesky (col: k(x_train, x_train) + noise I, 20000+col: the new rows' Schur "
                 "complement S)")


def condition_kl_closed(covar_module, likelihoods, x_new, x_train, mu_train, log_var_train,
                        max_workspace_bytes=4 << 30):
    """The exact KL (``KL_closed_batched``) of ``cat(new, train)`` with everything but the new rows' latents frozen:
    returns ``cond`` (a ``DuboCondition`` with ``.L`` and ``.Nn``) such that ``cond(m_new, log_v_new)`` [L] fp64
    plus the exact KL of the training rows alone equals the exact KL of cat(x_new, x_train), cat(m_new, mu_train),
    cat(log_v_new, log_var_train) -- values and the gradients with respect to m_new / log_v_new [Nn, L], in the
    caller's dtype.  Subtracting the training rows' KL, which does not depend on the new rows, keeps the value a
    function of the conditioning alone: KL(q_new || the GP's posterior predictive at the new rows) plus the trace
    term that averaging the predictive mean over q_train leaves.

    THE PRIOR IS FROZEN: nothing flows to the kernels, the noise or the training latents, whatever requires grad;
    they are detached and read once, here.  With them fixed the joint KL is an exact quadratic-plus-exponential form
    in the new rows (csrc/kl_cond.hip): this call costs one factorisation of the training Gram and two solves
    against it (lvae_kl_cond_prepare_f64), every ``cond(...)`` after it is one symmetric [Nn, Nn] matvec per latent
    dim (lvae_dubo_cond_eval_f64) whose cost no longer depends on the training set.

    ``covar_module`` and ``likelihoods`` in every form ``predict_exact`` takes (a batched module or a per-dim
    list); ``mu_train`` / ``log_var_train`` [N, L] at ``x_train`` [N, Q].  x_train may have no rows (``cond`` is then
    the plain exact KL of the new rows).  The rows may come in any order and with any subject structure: the exact KL
    has none.  The dims are processed in groups whose workspace (about 8 (N^2 + N Nn + 2 Nn^2) bytes a dim) stays
    under ``max_workspace_bytes``; the state holds all L dims and its bits do not depend on the grouping.
    ValueError: an x_new without rows, mu_train / log_var_train not [N, L], a kernel batch that is neither 1 nor L;
    LinAlgError: a dim whose training Gram or Schur complement is not positive definite."""
    nn, n = int(x_new.shape[0]), int(x_train.shape[0])
    if nn < 1:
        raise ValueError("x_new has no rows")
    if mu_train.dim() != 2 or tuple(log_var_train.shape) != tuple(mu_train.shape) or mu_train.shape[0] != n:
        raise ValueError(f"mu_train / log_var_train must be [{n}, L], got {tuple(mu_train.shape)} and "
                         f"{tuple(log_var_train.shape)}")
    L = int(mu_train.shape[1])
    # predict_exact's stacking, with the new rows as its prediction set (their mean only carries L and the device)
    a = _exact_inputs(covar_module, likelihoods, x_new, x_train, mu_train.new_zeros((nn, L)))
    lib = _lib.lib()
    dev = a.dev
    mu = mu_train.detach().to(dev, torch.float64).contiguous()
    lv = log_var_train.detach().to(dev, torch.float64).contiguous()
    size = lambda g: int(lib.lvae_kl_cond_workspace_size(n, nn, g))
    group = L
    while group > 1 and size(group) > max_workspace_bytes:
        group -= 1
    state = torch.empty(int(lib.lvae_dubo_cond_state_size(L, nn, 1)), dtype=torch.uint8, device=dev)
    info = torch.empty(L, dtype=torch.int32, device=dev)
    ws = torch.empty(size(group), dtype=torch.uint8, device=dev)
    ptr = lambda t, off: ctypes.c_void_p(t.data_ptr() + 8 * off)
    for l0 in range(0, L, group):
        g = min(group, L - l0)
        rc = lib.lvae_kl_cond_prepare_f64(a.spec, _lib.ptr(a.tx) if n else None, a.tx.stride(0), n, _lib.ptr(a.x),
                                          a.x.stride(0), nn, g, ptr(a.p, l0 * a.n_params), ptr(a.noise, l0),
                                          ptr(mu, l0) if n else None, L, ptr(lv, l0) if n else None, L,
                                          _lib.ptr(state), L, l0, ctypes.c_void_p(info.data_ptr() + 4 * l0),
                                          _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, "kl_cond_prepare")
    _check_info(info, _KL_COND_INFO)
    return DuboCondition(L, nn, 1, nn, state)
