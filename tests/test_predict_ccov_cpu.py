"""The oracles of the components' posterior covariance (predict_ccov_util.py) checked against the variance oracles of
test_predict_var_oracle.py, and the LatentComponents methods that read a covariance, on a hand-built one.  No GPU.

Every case of the GPU tests: the oracle's sum over both component indices is the dense predictive variance
(V.dense_exact / V.dense_inducing) to 1e-10 of the largest prior variance, and every block's smallest eigenvalue is
>= -1e-10 of the largest prior component variance (a posterior covariance is positive semi-definite).
"""
import math

import pytest
import torch

import predict_ccov_util as CC
import test_predict_var_oracle as V


@pytest.mark.parametrize("cid", CC.EXACT_IDS)
def test_exact_oracle_sums_to_the_variance(cid):
    c = CC.exact_problem(cid)
    ref, ya = CC.exact_ref(cid)
    if ref is None:
        assert c["Nt"] == 0
        return
    cov, prior = ref
    _, var, kss = V.dense_exact(c["spec"], c["params"], c["noise"], c["x"], c["tx"], c["mu"])   # [Nt, L]
    assert cov.shape == (c["L"], c["Nt"], len(c["spec"]), len(c["spec"])) and ya <= 1e-7
    assert float((prior.sum(2).T - kss).abs().max()) <= 1e-10 * float(kss.max())
    assert float((cov.sum((2, 3)).T - var).abs().max()) <= 1e-10 * float(kss.max())
    assert float(torch.linalg.eigvalsh(cov).min()) >= -1e-10 * float(prior.max())
    assert bool((cov == cov.transpose(2, 3)).all())


@pytest.mark.parametrize("cid", CC.IND_IDS)
def test_inducing_oracle_sums_to_the_variance(cid):
    c = CC.ind_problem(cid)
    ref, ya = CC.ind_ref(cid)
    if ref is None:
        assert c["Nt"] == 0
        return
    cov, prior = ref
    ok = c["valid"]
    _, var, kss = V.dense_inducing(c["s0"], c["p0"], c["s1"], c["p1"], c["noise"], c["x"][ok], c["tx"], c["mu"][ok],
                                   c["z"], CC.EPS)
    R = len(c["s0"]) + len(c["s1"])
    assert cov.shape == (c["L"], c["Nt"], R, R) and ya <= 1e-7
    assert float((cov.sum((2, 3)).T - var).abs().max()) <= 1e-10 * float(kss.max())
    assert float(torch.linalg.eigvalsh(0.5 * (cov + cov.transpose(2, 3))).min()) >= -1e-10 * float(prior.max())
    assert float((cov - cov.transpose(2, 3)).abs().max()) <= 1e-12 * float(prior.max())
    if cid == "two-tiles":
        assert R > 16


def hand_built():
    from lvae_amd.predict import LatentComponents
    gen = torch.Generator().manual_seed(5)
    L, Nt, R = 2, 3, 4
    A = torch.randn(L, Nt, R, R, generator=gen, dtype=torch.float64)
    cov = A @ A.transpose(2, 3)
    vals = torch.randn(R, Nt, L, generator=gen, dtype=torch.float64)
    return LatentComponents(vals, list("abcd"), [0, 0, 1, 1], cov=cov), cov, vals


def test_latent_components_variances():
    comps, cov, vals = hand_built()
    R, Nt, L = vals.shape
    var = comps.variance()
    assert var.shape == (R, Nt, L)
    for r in range(R):
        assert torch.equal(var[r], cov[:, :, r, r].T)
    tot = comps.total_variance()
    assert tot.shape == (Nt, L) and torch.allclose(tot, cov.sum((2, 3)).T, rtol=1e-14, atol=0)
    pv = comps.partial_variance()
    assert pv.shape == (R, Nt, L)
    for k in range(R):
        assert torch.allclose(pv[k], cov[:, :, :k + 1, :k + 1].sum((2, 3)).T, rtol=1e-13, atol=0)
    assert torch.allclose(pv[-1], tot, rtol=1e-13, atol=0)          # the last entry is the total variance
    order = [2, 0, 3, 1]
    po = comps.partial_variance(order)
    for k in range(R):
        ix = torch.tensor(order[:k + 1])
        assert torch.allclose(po[k], cov[:, :, ix][:, :, :, ix].sum((2, 3)).T, rtol=1e-13, atol=0)
    assert torch.equal(po[0], var[2]) and torch.allclose(po[-1], tot, rtol=1e-13, atol=0)
    assert comps.partial_variance([3, 1]).shape == (2, Nt, L)
    for bad in ([], [4], [-1], [1, 1]):
        with pytest.raises(ValueError):
            comps.partial_variance(bad)


def test_latent_components_clamp_at_zero():
    from lvae_amd.predict import LatentComponents
    cov = torch.tensor([[[[-1e-17, 0.0], [0.0, 2.0]]]], dtype=torch.float64)        # L = Nt = 1, R = 2
    comps = LatentComponents(torch.zeros(2, 1, 1, dtype=torch.float64), ["a", "b"], [0, 0], cov=cov)
    assert comps.variance()[:, 0, 0].tolist() == [0.0, 2.0]
    assert comps.partial_variance()[:, 0, 0].tolist() == [0.0, 2.0 - 1e-17]
    assert float(comps.total_variance()) == 2.0 - 1e-17


def test_latent_components_credible_interval():
    comps, cov, vals = hand_built()
    lo, hi = comps.credible_interval(0.95)
    sd = torch.sqrt(comps.variance())
    z = (hi - lo) / (2.0 * sd)
    assert lo.shape == hi.shape == vals.shape
    assert float((z - 1.959963984540054).abs().max()) < 1e-12
    assert torch.allclose(0.5 * (lo + hi), vals, rtol=1e-13, atol=1e-13)
    lo5, hi5 = comps.credible_interval(0.5)
    assert float(((hi5 - lo5) / (2.0 * sd) - 0.6744897501960817).abs().max()) < 1e-12
    for bad in (0.0, 1.0, 1.5):
        with pytest.raises(ValueError):
            comps.credible_interval(bad)
    assert math.isclose(float(torch.special.ndtri(torch.tensor(0.975, dtype=torch.float64))), 1.959963984540054,
                        rel_tol=1e-12)


def test_latent_components_without_cov():
    from lvae_amd.predict import LatentComponents
    comps = LatentComponents(torch.zeros(2, 3, 1, dtype=torch.float64), ["a", "b"], [0, 1])
    assert comps.cov is None
    for fn in (comps.variance, comps.total_variance, comps.partial_variance, comps.credible_interval):
        with pytest.raises(ValueError):
            fn()
