"""The drop-in model_test module (reference model_test.py:11-143) exposes the reference's names, backed by lvae_amd,
and MSE_test's "more than 6040 prediction rows" rule (model_test.py:59-63) keeps rows 0..39 and 6000 distinct rows
drawn from 40..n-1 (no compute here)."""
import importlib
import inspect
import os
import sys

import numpy as np

from conftest import ROOT

DROPIN = os.path.join(ROOT, "longitudinal-vae_amd", "dropin")


def _import(name):
    sys.path.insert(0, DROPIN)
    try:
        sys.modules.pop(name, None)
        return importlib.import_module(name)
    finally:
        sys.path.remove(DROPIN)


def test_surface_and_signatures():
    m = _import("model_test")
    assert m.__file__.startswith(DROPIN), m.__file__
    args = lambda f: list(inspect.signature(f).parameters)
    assert args(m.predict_gp) == ["kernel_component", "full_kernel_inverse", "z"]
    assert args(m.MSE_test) == ["csv_file_test_data", "csv_file_test_label", "test_mask_file", "data_source_path",
                                "type_nnet", "nnet_model", "covar_module", "likelihoods", "results_path", "latent_dim",
                                "prediction_x", "prediction_mu", "rng"]
    assert inspect.signature(m.MSE_test).parameters["rng"].default is None
    assert args(m.MSE_test_GPapprox) == ["csv_file_test_data", "csv_file_test_label", "test_mask_file",
                                         "data_source_path", "type_nnet", "nnet_model", "covar_module0",
                                         "covar_module1", "likelihoods", "results_path", "latent_dim", "prediction_x",
                                         "prediction_mu", "zt_list", "P", "T", "id_covariate", "varying_T", "save_file"]
    import lvae_amd as la
    assert m.MSE_test is la.MSE_test and m.MSE_test_GPapprox is la.MSE_test_GPapprox   # a re-export, one body
    assert callable(la.predict_exact)
    assert args(m.VAEtest) == ["test_dataset", "nnet_model", "type_nnet", "id_covariate"]   # VAE.py:14 imports it
    sys.modules.pop("model_test", None)


def test_predict_gp_is_the_reference_product():
    import torch
    m = _import("model_test")
    g = torch.Generator().manual_seed(0)
    kc, ik, z = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((5, 7), (7, 7), (7,)))
    assert torch.equal(m.predict_gp(kc, ik, z), torch.matmul(torch.matmul(kc, ik), z))
    sys.modules.pop("model_test", None)


def test_prediction_row_selection():
    from lvae_amd.evaluation import select_prediction_rows
    assert select_prediction_rows(1) is None and select_prediction_rows(6040) is None
    for n in (6041, 9000):
        ind = select_prediction_rows(n, np.random.default_rng(3))
        assert ind.shape == (6040,) and np.array_equal(ind[:40], np.arange(40))
        rest = ind[40:]
        assert len(set(rest.tolist())) == 6000 and rest.min() >= 40 and rest.max() <= n - 1
        assert np.array_equal(ind, select_prediction_rows(n, np.random.default_rng(3)))   # seeded: reproducible
    assert sorted(select_prediction_rows(6041, np.random.default_rng(1))[40:].tolist()) != list(range(40, 6040))
    np.random.seed(7)   # the default: NumPy's global generator, as the reference
    a = select_prediction_rows(7000)
    np.random.seed(7)
    assert np.array_equal(a, select_prediction_rows(7000))
