"""elbo_batched without a GPU: the drop-in elbo_functions exposes it, and wrong train_yt / z shapes raise
ValueError before the HIP library is touched (values: test_gpu_gp_elbo.py)."""
import ctypes
import importlib
import os
import sys

import pytest
import torch

from conftest import PKG

DROPIN = os.path.join(PKG, "dropin")
CFG = dict(cat_kernel=[2], bin_kernel=[], sqexp_kernel=[0],
           cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 2}, {'cont_covariate': 0, 'cat_covariate': 3},
                           {'cont_covariate': 1, 'cat_covariate': 4}],
           bin_int_kernel=[], covariate_missing_val=[])


def test_dropin_exposes_elbo_batched():
    import lvae_amd as la
    sys.path.insert(0, DROPIN)
    try:
        sys.modules.pop("elbo_functions", None)
        m = importlib.import_module("elbo_functions")
    finally:
        sys.path.remove(DROPIN)
        sys.modules.pop("elbo_functions", None)
    assert m.__file__.startswith(DROPIN)
    assert m.elbo_batched is la.elbo_batched and "elbo_batched" in m.__all__
    assert m.elbo is la.elbo


def test_elbo_batched_rejects_shapes_before_the_library(monkeypatch):
    import lvae_amd as la
    from lvae_amd import _lib

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    L, P, T, M, Q = 3, 4, 5, 6, 6
    k0, k1 = la.generate_kernel_batched(L, **CFG, id_covariate=2)
    lik = la.GaussianLikelihood(L, noise=1.0)
    g = torch.Generator().manual_seed(0)
    X = torch.randn(P * T, Q, generator=g, dtype=torch.float64)
    z = torch.randn(L, M, Q, generator=g, dtype=torch.float64)
    y = torch.randn(2, P * T, L, generator=g, dtype=torch.float64)

    def call(yy=y, zz=z, p=P):
        return la.elbo_batched(L, k0, k1, lik, X, yy, zz, p, T, 1e-6)
    bad_y = [y[:, :-1], y[:, :, :2], y[0, :-1], y[0, :, :2], y[None], y[:0], y[0, :, 0]]
    for yy in bad_y:
        with pytest.raises(ValueError):
            call(yy=yy)
    bad_z = [z[:2], z[None], [z[0], z[1]], z[0, 0]]
    for zz in bad_z:
        with pytest.raises(ValueError):
            call(zz=zz)
    with pytest.raises(ValueError):
        call(p=P + 1)
    # well-formed inputs get as far as the library
    for yy, zz in ((y, z), (y[0], z[0]), (y, [zi for zi in z])):
        with pytest.raises(AssertionError, match="the library was touched"):
            call(yy=yy, zz=zz)
    assert ctypes.sizeof(_lib.GpElboDims) == 32
