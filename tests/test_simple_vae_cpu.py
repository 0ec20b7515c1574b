"""SimpleVAE without a GPU: the fp64 CPU model against the reference's recorded outputs and gradients
(tests/golden/simple_vae.npz, written by tests/golden/gen_golden_simple_vae.py), its state-dict names, the vy setter,
the host queries of the fused kernels, and the flat Health-MNIST and Physionet datasets.

Bounds: 1e-12 of each tensor's max-abs (fp64 against fp64, the same operations in the same order up to the loss's
masked sums); dataset contents are exact."""
import os

import numpy as np
import pytest
import torch

import simple_vae_util as S
from conftest import GOLDEN, golden

TINY = os.path.join(GOLDEN, "hmnist_tiny")
FILES = ("tiny_data.csv", "tiny_labels.csv", "tiny_mask.csv")


def _fixture_model(g):
    import lvae_amd as la
    model = la.SimpleVAE(int(g["L"]), int(g["D"]), 1.0, False).double()
    model.load_state_dict(S.weights(model, int(g["seed"])), strict=True)
    return model


def test_fixture_outputs_and_gradients():
    g = golden("simple_vae.npz")
    model = _fixture_model(g)
    assert not g["mask"][int(g["zero_row"])].any()
    got = S.run(model, torch.tensor(g["x"]), torch.tensor(g["mask"]), torch.tensor(g["eps"]))
    names = ["mu", "logv", "recon", "mse", "nll"] + ["g_" + n for n, _ in model.named_parameters()]
    for k in names:
        err = S.rel(got[k], torch.tensor(g[k]))
        print(f"{k}: {err:.2e}")
        assert err < 1e-12, (k, err)


def test_state_dict_names_and_shapes():
    import lvae_amd as la
    g = golden("simple_vae.npz")
    model = la.SimpleVAE(int(g["L"]), int(g["D"]))
    assert list(model.state_dict().keys()) == [str(k) for k in g["keys"]]
    sd = {str(k): torch.zeros(tuple(g["g_" + str(k)].shape)) for k in g["keys"] if str(k) != "min_log_vy"}
    sd["min_log_vy"] = torch.full((1,), -8.0)
    model.load_state_dict(sd, strict=True)
    assert model.fc1.weight.shape == (300, 11) and model.fc4.weight.shape == (11, 300)


def test_vy_setter_round_trips():
    import lvae_amd as la
    model = la.SimpleVAE(2, 7, vy_init=1.0).double()
    assert S.rel(model.vy, torch.ones(7, dtype=torch.float64)) < 1e-6   # (the constructor's fp32 parameter)
    want = torch.linspace(0.01, 2.0, 7, dtype=torch.float64)
    model.vy = want
    assert S.rel(model.vy, want) < 1e-12
    with pytest.raises(AssertionError):
        model.vy = torch.full((7,), 1e-4, dtype=torch.float64)
    fixed = la.SimpleVAE(2, 7, vy_fixed=True)
    assert not fixed._log_vy.requires_grad


def test_forward_views_rows_and_draws_eps():
    import lvae_amd as la
    model = la.SimpleVAE(2, 6).double()
    x = torch.rand(4, 1, 1, 6, dtype=torch.float64)
    torch.manual_seed(0)
    recon, mu, lv = model(x)
    assert recon.shape == (4, 6) and mu.shape == lv.shape == (4, 2)
    assert model.last_route == {"encode": "stock", "decode": "stock"}
    torch.manual_seed(0)
    z = model.sample_latent(mu, lv)
    assert torch.equal(model.decode(z), recon)


def test_host_queries_need_no_gpu():
    from lvae_amd import _lib
    lib = _lib.load()
    for D in (1, 5, 37, 48):
        for L in (1, 16, 32):
            assert lib.lvae_mlp_vae_fused_ok(D, 300, 30, L) == 1, (D, L)
            assert 0 < lib.lvae_mlp_vae_lds_bytes(D, 300, 30, L) <= 160 * 1024
    assert lib.lvae_mlp_vae_fused_ok(57, 300, 30, 32) == 1 and lib.lvae_mlp_vae_fused_ok(58, 300, 30, 32) == 0
    assert lib.lvae_mlp_vae_fused_ok(1296, 300, 30, 16) == 0
    assert lib.lvae_mlp_vae_lds_bytes(1296, 300, 30, 16) > 160 * 1024
    for D, H1, H2, L in ((37, 64, 16, 4), (37, 300, 30, 33), (0, 300, 30, 4), (37, 300, 30, 0)):
        assert lib.lvae_mlp_vae_fused_ok(D, H1, H2, L) == 0 and lib.lvae_mlp_vae_lds_bytes(D, H1, H2, L) == 0
    assert [lib.lvae_mlp_wgrad_splits(B) for B in (0, 1, 80, 512)] == [0, 1, 1, 1]
    B2 = next(B for B in range(1, 5000) if lib.lvae_mlp_wgrad_splits(B) >= 2)
    assert B2 == 513 and lib.lvae_mlp_wgrad_splits(40960) == 64
    for size in (lib.lvae_mlp_enc_bwd_workspace_size, lib.lvae_mlp_dec_bwd_workspace_size):
        assert size(0, 37, 16) == 0 and size(80, 37, 16) >= 4 * 80 * 330
        assert size(513, 37, 16) > size(512, 37, 16) + 2 * 1024 * 4


def test_flat_health_mnist_dataset():
    from lvae_amd.data import HealthMNISTDataset, HealthMNISTDatasetConv
    import dropin.dataset_def as DD
    assert DD.HealthMNISTDataset is HealthMNISTDataset
    flat, conv = HealthMNISTDataset(*FILES, TINY), HealthMNISTDatasetConv(*FILES, TINY)
    idx = torch.tensor([3, 0, 11, 5])
    a, b = flat.batch(idx), conv.batch(idx)
    assert a["digit"].shape == (4, 1, 1, 1296) and a["digit"].dtype == torch.float32
    assert torch.equal(a["digit"].reshape(4, 1296), b["digit"].reshape(4, 1296))
    assert torch.equal(a["label"], b["label"]) and torch.equal(a["mask"], b["mask"]) and a["mask"].shape == (4, 1, 1296)
    g = golden("hmnist_tiny.npz")
    item = flat[7]
    assert item["digit"].shape == (1, 1296) and item["digit"].dtype == np.uint8
    assert np.array_equal(item["digit"].reshape(-1), g["digit"][7].reshape(-1))
    assert item["idx"] == 7 and np.array_equal(item["mask"].numpy(), g["mask"][7])
    assert len(flat) == int(g["n"]) and len(flat[2:5]) == 3


def test_physionet_dataset_matches_recorded_items():
    import lvae_amd as la
    import dropin.dataset_def as DD
    assert DD.PhysionetDataset is la.PhysionetDataset
    g = golden("physionet_tiny.npz")
    ds = la.PhysionetDataset("physionet_tiny.npz", GOLDEN)
    assert len(ds) == int(g["n"]) == 12
    for _ in range(2):   # a second access returns the same item (the 24 is subtracted once)
        for i in range(len(ds)):
            it = ds[i]
            assert set(it) == {"data", "label", "idx", "mask"} and it["idx"] == i
            assert np.array_equal(it["data"].numpy(), g["item_data"][i].astype(np.float32))
            assert np.array_equal(it["label"].numpy(), g["item_label"][i].astype(np.float32))
            assert it["mask"].dtype == torch.uint8 and np.array_equal(it["mask"].numpy(), g["item_mask"][i])
    assert np.array_equal(g["item_label"][:, 8], g["outcome_attrib"].reshape(12, -1)[:, 8] - 24)
    b = ds.batch([4, 1])
    assert b["data"].shape == (2, 5) and b["label"].shape == (2, 20) and b["mask"].shape == (2, 5)
    assert torch.equal(b["data"][0], ds[4]["data"]) and torch.equal(b["label"][1], ds[1]["label"])


def test_type_nnet_is_checked_against_the_model():
    import lvae_amd as la
    from lvae_amd.evaluation import VAEtest, check_type_nnet
    from lvae_amd.validation import validate
    simple, conv = la.SimpleVAE(2, 1296), la.ConvVAE(2)
    check_type_nnet("simple", simple)
    check_type_nnet("conv", conv)
    with pytest.raises(TypeError):
        check_type_nnet("simple", conv)
    with pytest.raises(NotImplementedError):
        check_type_nnet("mlp", simple)
    with pytest.raises(TypeError):     # (raised before anything touches a GPU)
        validate(conv, "simple", None, "GPapprox_closed", 1, 2, None, None, None, None, 4, 0.15, None, None, 2, "mse")
    from lvae_amd.data import HealthMNISTDataset
    ds = HealthMNISTDataset(*FILES, TINY)
    torch.manual_seed(1)
    got = VAEtest(ds, simple, "simple", 2)
    with torch.no_grad():
        b = ds.batch(torch.arange(len(ds)))
        x, m = b["digit"].reshape(-1, 1296), b["mask"].reshape(-1, 1296).float()
        torch.manual_seed(1)
        want = float((((simple(b["digit"])[0] - x) ** 2 * m).sum(1) / m.sum(1)).mean())
    assert abs(got - want) <= 1e-6 * abs(want)
