"""Test-set evaluation after training (model_test.py:11-143): ``MSE_test`` for models trained with the exact KL
(the exact-GP predictor, lvae_predict_exact_f64) and ``MSE_test_GPapprox`` for the Hensman / GPapprox regimes
(batch_predict_varying_T, lvae_predict_f64).  Reference names and signatures; both write the two-number
``result_error.csv`` (mean masked MSE of the autoencoder's own reconstruction, and of the decoded GP prediction).

Differences from the reference, none of which changes a result it can produce:
  * the test set is read through the project's device-resident HealthMNISTDatasetConv (type_nnet='conv') or the
    flat HealthMNISTDataset ('simple', model_test.py:35-40) and evaluated as one device batch (no DataLoader
    workers), by the project's fp32 ConvVAE / SimpleVAE (the reference casts the images to fp64);
  * MSE_test solves with the Cholesky factor and one refinement step instead of forming K^-1;
  * the "more than 6040 prediction rows" rule draws its 6000 rows from 40..n-1 (model_test.py:60 draws from
    0..n-1 and then adds 40, which can index past the end); an ``rng`` keyword seeds the draw, the default is
    NumPy's global generator as in the reference;
  * nothing is printed: the numbers are in the file.
``VAEtest`` (model_test.py:145-167) is here because the reference's VAE.py imports it from this module; it
returns the autoencoder's mean masked MSE, which the reference only prints.
"""
import os

import numpy as np
import torch

from .data import HealthMNISTDataset, HealthMNISTDatasetConv
from .predict import batch_predict_varying_T, predict_exact

KEEP_ROWS, SAMPLE_ROWS = 40, 6000   # model_test.py:59-61


def predict_gp(kernel_component, full_kernel_inverse, z):
    """Predictive mean kernel_component @ full_kernel_inverse @ z (model_test.py:11-17).  With one additive
    component's cross-Gram as ``kernel_component`` this is that component's share of the predicted latents;
    predict_exact_components and batch_predict_components return all the shares at once without the dense Gram or
    the explicit inverse."""
    return torch.matmul(torch.matmul(kernel_component, full_kernel_inverse), z)


def select_prediction_rows(n, rng=None):
    """Row indices MSE_test keeps of an n-row prediction set: all of them up to 6040 rows (None), else rows
    0..39 and 6000 distinct rows drawn from 40..n-1 (model_test.py:59-63)."""
    if n <= KEEP_ROWS + SAMPLE_ROWS:
        return None
    r = (np.random if rng is None else rng).choice(n - KEEP_ROWS, SAMPLE_ROWS, replace=False) + KEEP_ROWS
    return np.concatenate((np.arange(KEEP_ROWS), r))


def check_type_nnet(type_nnet, model):
    """'conv' (any model, as before 'simple' existed) or 'simple' with a SimpleVAE (VAE.py:294-333); any other
    type_nnet raises NotImplementedError"""
    from .vae import SimpleVAE
    if type_nnet not in ("conv", "simple"):
        raise NotImplementedError(f"type_nnet must be 'conv' or 'simple', got {type_nnet!r}")
    if type_nnet == "simple" and not isinstance(model, SimpleVAE):
        raise TypeError(f"type_nnet='simple' needs a SimpleVAE, got {type(model).__name__}")


def _whole_set(dataset, model):
    """(images, mask [B, num_dim], labels [B, Q] fp64) of a device-resident dataset as one batch in the model's
    dtype; the images are the items' 'digit' or, for PhysionetDataset, 'data'"""
    dtype = next(model.parameters()).dtype
    everything = dataset.batch(torch.arange(len(dataset)))
    images = everything["digit" if "digit" in everything else "data"].to(dtype)
    return images, everything["mask"].reshape(images.shape[0], -1).to(dtype), everything["label"].to(torch.float64)


def _mean_mse(model, recon, images, mask):
    """The per-image masked MSE of the model's loss_function, averaged over the images"""
    return float(model.loss_function(recon, images, mask)[0].mean())


def _evaluate(files, root, type_nnet, model, out_file, predict):
    """The body the two tests share: the autoencoder's own mean masked MSE over the test set and that of the
    decoded latents ``predict(labels)``, written one per line to ``out_file``."""
    check_type_nnet(type_nnet, model)
    data_csv, label_csv, mask_csv = files
    dataset_cls = HealthMNISTDatasetConv if type_nnet == "conv" else HealthMNISTDataset
    dataset = dataset_cls(data_csv, label_csv, mask_csv, root, device=next(model.parameters()).device)
    with torch.no_grad():
        images, mask, labels = _whole_set(dataset, model)
        own = _mean_mse(model, model(images)[0], images, mask)
        latents = predict(labels).to(images.dtype)
        gp = _mean_mse(model, model.decode(latents), images, mask)
    np.savetxt(out_file, np.array([own, gp]))


def MSE_test(csv_file_test_data, csv_file_test_label, test_mask_file, data_source_path, type_nnet, nnet_model,
             covar_module, likelihoods, results_path, latent_dim, prediction_x, prediction_mu, rng=None):
    """Mean squared error of the test set under the exact-GP predictor (model_test.py:19-82); writes
    ``result_error.csv`` under ``results_path``."""
    ind = select_prediction_rows(prediction_x.shape[0], rng)
    if ind is not None:
        prediction_x, prediction_mu = prediction_x[ind], prediction_mu[ind]
    device = next(nnet_model.parameters()).device
    px, pm = prediction_x.to(device), prediction_mu[:, :latent_dim].to(device)
    if isinstance(covar_module, (list, tuple, torch.nn.ModuleList)):
        covar_module, likelihoods = list(covar_module)[:latent_dim], list(likelihoods)[:latent_dim]
    _evaluate((csv_file_test_data, csv_file_test_label, test_mask_file), data_source_path, type_nnet, nnet_model,
              os.path.join(results_path, "result_error.csv"),
              lambda labels: predict_exact(covar_module, likelihoods, px, labels, pm))


def MSE_test_GPapprox(csv_file_test_data, csv_file_test_label, test_mask_file, data_source_path, type_nnet,
                      nnet_model, covar_module0, covar_module1, likelihoods, results_path, latent_dim, prediction_x,
                      prediction_mu, zt_list, P, T, id_covariate, varying_T=False, save_file='result_error.csv'):
    """Mean squared error of the test set with the GP approximation (model_test.py:85-143); writes ``save_file``
    under ``results_path``.  ``P``, ``T`` and ``varying_T`` are accepted and not used, as in the reference (the
    predictor takes subjects of any length)."""
    device = next(nnet_model.parameters()).device
    px, pm = prediction_x.to(device), prediction_mu.to(device)
    _evaluate((csv_file_test_data, csv_file_test_label, test_mask_file), data_source_path, type_nnet, nnet_model,
              os.path.join(results_path, save_file),
              lambda labels: batch_predict_varying_T(latent_dim, covar_module0, covar_module1, likelihoods, px,
                                                     labels, pm, zt_list, id_covariate, eps=1e-6))


def generate_trajectories(nnet_model, mean, cov=None, num_samples=0, eps=None, generator=None, jitter=1e-8,
                          chunk_rows=4096):
    """Decoded image sequences at the predicted latents: ``(decode(mean), draws)``, the computational half of
    recon_complete_gen / variational_complete_gen (predict_HealthMNIST.py:131-138, 165-170; their plots are out of
    scope).  ``mean`` [Nt, L] is a predictor's Z_pred (batch_predict_varying_T or predict_exact at the generation
    set's labels).  With ``cov`` (the PredictiveCovariance of the same call with ``return_cov=True``) and
    ``num_samples`` > 0 or ``eps`` [S, Nt, L], ``draws`` [S, Nt, ...] holds the decoded trajectory draws of
    ``sample_trajectories(mean, cov, num_samples, eps, generator, jitter)``: each subject's frames are drawn
    jointly, so a drawn sequence is coherent over time, while different subjects are drawn independently of each
    other.  Otherwise ``draws`` is None.  Either model (ConvVAE, SimpleVAE), in the mode the caller left it in
    (``eval()`` for dropout-free images, as the reference's callers do); no gradients are recorded.  The decoder
    runs one draw at a time, over at most ``chunk_rows`` of its rows per call, exactly as it runs over ``mean``: the
    S * Nt images never need one set of activations, and a draw with ``eps = 0`` is ``decode(mean)`` bit for bit.
    A decoder call's bits do not depend on the other rows' values, so ``chunk_rows`` changes no bit as long as the
    decoder's GEMM library picks the same kernel for the shorter calls (the ConvVAE's fc layers run on hipBLASLt,
    which chooses by shape: 15 rows in calls of 4 gave the bits of one call on an MI355X, 30 rows did not)."""
    from .predict import sample_trajectories
    chunk_rows = max(int(chunk_rows), 1)
    dtype = next(nnet_model.parameters()).dtype

    def decode(z):
        parts = [nnet_model.decode(z[r0:r0 + chunk_rows].to(dtype)) for r0 in range(0, z.shape[0], chunk_rows)]
        return torch.cat(parts) if parts else nnet_model.decode(z.to(dtype))

    with torch.no_grad():
        images = decode(mean)
        if cov is None or (eps is None and int(num_samples) < 1):
            return images, None
        z = sample_trajectories(mean, cov, num_samples=num_samples, eps=eps, generator=generator, jitter=jitter)
        if z.shape[0] == 0:
            return images, images.new_empty((0,) + tuple(images.shape))
        return images, torch.stack([decode(zs) for zs in z])


def generate_component_sequences(nnet_model, comps, order=None):
    """Decoded images as the covariate effects are added one by one: ``[R', Nt, ...]``, entry r the decoder's output
    at the partial sum ``comps.values[order[:r + 1]].sum(0)`` of a LatentComponents (``predict_exact_components``,
    ``batch_predict_components``).  ``order`` lists the components to add, in that order (default: all R, as
    stored); with every component in it the last entry is ``decode(comps.total())``.  The split is additive in the
    latent space only: the decoder is not linear, so the images are NOT additive in image space, an entry is the
    reconstruction with the effects so far, and the difference of two entries is not "the image of" a component
    (it depends on the order).  Uses ``nnet_model.decode`` (ConvVAE or SimpleVAE, in the mode the caller left it
    in); no gradients are recorded."""
    R = int(comps.values.shape[0])
    order = list(range(R)) if order is None else [int(r) for r in order]
    if not order or any(r < 0 or r >= R for r in order):
        raise ValueError(f"order {order} must name at least one component, each in 0 .. {R - 1}")
    dtype = next(nnet_model.parameters()).dtype
    idx = torch.tensor(order, dtype=torch.long, device=comps.values.device)
    with torch.no_grad():
        return torch.stack([nnet_model.decode(comps.values[idx[:r + 1]].sum(0).to(dtype)) for r in range(len(order))])


def VAEtest(test_dataset, nnet_model, type_nnet, id_covariate):
    """Mean masked MSE of the autoencoder alone over a device-resident dataset (model_test.py:145-167); either
    model, ``type_nnet`` is not used."""
    with torch.no_grad():
        images, mask, _ = _whole_set(test_dataset, nnet_model)
        return _mean_mse(nnet_model, nnet_model(images)[0], images, mask)
