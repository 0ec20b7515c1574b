"""Validation-set loss of the GP-approximation regimes (validation.py:70-175): ``validate`` with the reference's
signature and return value (the net loss as a Python float), and ``validation_dubo`` (validation.py:8-68).

Differences from the reference, none of which changes a result it can produce:
  * the dataset is one of the project's device-resident datasets (lvae_amd.data: HealthMNISTDatasetConv for
    type_nnet='conv'; the flat HealthMNISTDataset or PhysionetDataset for 'simple'), evaluated as one device batch
    (no DataLoader workers) by the project's fp32 ConvVAE / SimpleVAE (the reference casts the data to fp64), as
    evaluation._evaluate does;
  * ``T`` is used as passed -- the reference overwrites it with 16 (validation.py:95);
  * 'GPapprox_closed' is ONE batched call for all latent dims (deviance_upper_bound_batched), for per-dim module
    lists (the reference's loop over deviance_upper_bound) and for batched modules (its validation_dubo branch);
  * ``varying_T=True`` (an extension: the reference's bounds need P subjects of T rows) takes the subjects from the
    labels' ``id_covariate`` column, of any lengths and in any row order, and ignores ``T``: the GP term comes from
    deviance_upper_bound_varying_T / elbo_varying_T, the sampled one as one batched call per draw;
  * nothing is printed.
As in the reference, 'GPapprox' (the sampled per-dim ``elbo``, ``num_samples`` draws) exists for per-dim module
lists only: with batched modules its GP term is 0 (validation.py:157-163 has no such branch).
"""
import torch

from .evaluation import _whole_set, check_type_nnet
from .gpapprox import (deviance_upper_bound_batched, deviance_upper_bound_varying_T, elbo, elbo_varying_T,  # noqa: F401
                       subject_layout, validation_dubo)


def validate(nnet_model, type_nnet, dataset, type_KL, num_samples, latent_dim, covar_module0, covar_module1,
             likelihoods, zt_list, T, weight, train_mu, train_x, id_covariate, loss_function, eps=1e-6,
             varying_T=False):
    """The validation set's net loss: recon + weight * GP / latent_dim ('mse') or nll + GP ('nll'), GP the DUBO
    ('GPapprox_closed') or minus the sampled ELBO ('GPapprox') summed over the latent dims.  ``train_mu``,
    ``train_x`` are accepted and not used, as in the reference, and so is ``id_covariate`` unless ``varying_T``:
    then the subjects are the distinct values of the labels' column ``id_covariate`` and ``T`` is ignored."""
    check_type_nnet(type_nnet, nnet_model)
    assert type_KL == 'GPapprox_closed' or type_KL == 'GPapprox'
    with torch.no_grad():
        images, mask, labels = _whole_set(dataset, nnet_model)
        P = None if varying_T else labels.shape[0] // T
        recon, mu, log_var = nnet_model(images)
        mse, nll = nnet_model.loss_function(recon, images, mask)
        recon_loss_sum, nll_loss_sum = float(mse.sum()), float(nll.sum())
        full_mu, full_log_var = mu.to(torch.float64), log_var.to(torch.float64)
        gp_loss_sum = 0.0
        per_dim = isinstance(covar_module0, (list, tuple, torch.nn.ModuleList))
        if varying_T:
            z = [zi.to(labels.device) for zi in zt_list] if isinstance(zt_list, (list, tuple)) else zt_list.to(
                labels.device)
            layout = subject_layout(labels[:, id_covariate])
            if type_KL == 'GPapprox_closed':
                gp_loss_sum = float(deviance_upper_bound_varying_T(latent_dim, covar_module0, covar_module1,
                                                                   likelihoods, labels, full_mu, full_log_var, z,
                                                                   id_covariate, eps, layout=layout).sum())
            elif per_dim:
                for _ in range(num_samples):
                    Z = nnet_model.sample_latent(full_mu, full_log_var)
                    gp_loss_sum -= float(elbo_varying_T(latent_dim, covar_module0, covar_module1, likelihoods, labels,
                                                        Z, z, id_covariate, eps, layout=layout).sum())
                gp_loss_sum /= num_samples
        elif type_KL == 'GPapprox_closed':
            z = [zi.to(labels.device) for zi in zt_list] if isinstance(zt_list, (list, tuple)) else zt_list.to(
                labels.device)
            gp_loss_sum = float(deviance_upper_bound_batched(latent_dim, covar_module0, covar_module1, likelihoods,
                                                             labels, full_mu, full_log_var, z, P, T, eps).sum())
        elif per_dim:
            for _ in range(num_samples):
                Z = nnet_model.sample_latent(full_mu, full_log_var)
                for i in range(latent_dim):
                    gp_loss_sum -= float(elbo(covar_module0[i], covar_module1[i], likelihoods[i], labels, Z[:, i],
                                              zt_list[i].to(labels.device), P, T, eps))
            gp_loss_sum /= num_samples
    if loss_function == 'mse':
        gp_loss_sum /= latent_dim
        return weight * gp_loss_sum + recon_loss_sum
    if loss_function == 'nll':
        return gp_loss_sum + nll_loss_sum
    raise ValueError(f"loss_function {loss_function!r}")
