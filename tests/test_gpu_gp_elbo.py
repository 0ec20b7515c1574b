"""elbo_batched (lvae_gp_elbo_fwd_f64 / lvae_gp_elbo_bwd_f64: the fused subject pass over all samples, the partial
reduction, the composed M x M / per-subject algebra with the rank-S sample terms and the Gram adjoint) against the
reference's golden vector, the fp64 oracle under CPU autograd, and the per-dim composed lvae_amd.elbo.

Bounds (relative to each quantity's max-norm, dubo_util.BOUND): value 1e-8; dy 1e-7; raw gradients (kernels and
noise) 1e-6.  The golden case keeps test_gpapprox_elbo_and_dubo_golden's own bounds (1e-9 / 1e-7 / 1e-6).

Shapes (L = 3 each, S = 3 samples with random cotangents [S, L]): one subject, T = M = 1, odd sizes, the workload's
(T, M) = (16, 120), both sides of the fused pass's T <= 32 limit and T = M = 128 on the batched-product route, P one
below / on / one above a multiple of the 16 subjects a workgroup walks, three groups; 6x7x33 also at S = 1 (and as
[N, L]), S = 16 (a full MFMA column block) and S = 17 (two calls through Python).
"""
import pytest
import torch

import abi_util as U
import dubo_util as D
import gp_elbo_util as G
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = G.DEV


def test_gp_elbo_batched_reference_golden(hip):
    """The reference's own elbo (gpapprox.npz: P = T = 16, M = 40, one dim), L = 1, S = 1: value and gradients"""
    import lvae_amd as la
    g = golden("gpapprox.npz")
    P, T = int(g["P"]), int(g["T"])
    X, Z = torch.tensor(g["X"], device=DEV), torch.tensor(g["Z"], device=DEV)
    k0, k1 = la.generate_kernel_batched(1, **D.CFG, id_covariate=2)
    D.set_raw(k0, g["raw0"].T)
    D.set_raw(k1, g["raw1"].T)
    k0, k1 = k0.to(DEV), k1.to(DEV)
    lik = la.GaussianLikelihood(1, noise=float(g["noise"])).to(DEV)
    y = torch.tensor(g["y"], device=DEV)[None, :, None].requires_grad_()
    el = la.elbo_batched(1, k0, k1, lik, X, y, Z[None], P, T, float(g["eps"]))
    assert el.shape == (1, 1) and el.dtype == torch.float64
    el.sum().backward()
    errs = dict(elbo=G.rel(el[0, 0], g["elbo"]), dy=G.rel(y.grad[0, :, 0], g["elbo_dy"]),
                draw0=G.rel(torch.cat([p.grad for _, p in k0.named_parameters()]), g["elbo_draw0"][:, 0]),
                draw1=G.rel(torch.cat([p.grad for _, p in k1.named_parameters()]), g["elbo_draw1"][:, 0]))
    print("golden", errs)
    assert errs["elbo"] < 1e-9
    assert errs["dy"] < 1e-7
    assert errs["draw0"] < 1e-6
    assert errs["draw1"] < 1e-6


@pytest.mark.parametrize("cid", G.CASE_IDS)
def test_gp_elbo_batched_vs_oracle(hip, cid):
    G.check(G.batched(cid, 3), G.oracle(cid, 3), G.BOUND, f"{cid} S=3 vs oracle:")


@pytest.mark.parametrize("S", [1, 16, 17])
def test_gp_elbo_sample_counts_vs_oracle(hip, S):
    """6x7x33 with one sample, a full column block and one sample past it (elbo_batched's split into two calls)"""
    G.check(G.batched("6x7x33", S), G.oracle("6x7x33", S), G.BOUND, f"6x7x33 S={S} vs oracle:")


def test_gp_elbo_matrix_input_returns_a_vector(hip):
    """train_yt [N, L] -> [L]: the S = 1 call without its sample axis, bit for bit"""
    cid = "6x7x33"
    y, g = G.samples(cid, 1)
    flat = G.run_batched(cid, 1, y=y[0])
    assert flat["elbo"].shape == (G.L,) and flat["dy"].shape == y[0].shape
    ref = G.batched(cid, 1)
    assert U.bit_equal(flat["elbo"], ref["elbo"][0]) and U.bit_equal(flat["dy"], ref["dy"][0])
    for k in ("draw0", "draw1", "dnoise"):
        assert U.bit_equal(flat[k], ref[k]), k


def test_gp_elbo_module_lists(hip):
    """per-dim module / likelihood / z lists == batched modules, bitwise"""
    got, lst = G.batched("6x7x33", 3), G.run_batched("6x7x33", 3, "list")
    for k in G.QUANT:
        assert U.bit_equal(lst[k], got[k]), k


@pytest.mark.parametrize("cid", ["6x7x33", "9x16x120"])
def test_gp_elbo_batched_vs_composed(hip, cid):
    """each elbo[s][l] and every gradient against the per-dim lvae_amd.elbo loop on the GPU"""
    G.check(G.batched(cid, 3), G.composed(cid, 3), G.BOUND, f"{cid} S=3 vs composed:")


@pytest.mark.parametrize("cid", ["6x7x33", "3x33x17"])
def test_gp_elbo_samples_are_independent(hip, cid):
    """row s of the S = 3 call == the S = 1 call on sample s (1e-12: the sample's MFMA column differs); a cotangent
    with one non-zero entry (s0, l0) gives dy zero in every other sample and dim, and no parameter gradient in
    the other dims"""
    c = D.problem(cid)
    y, _ = G.samples(cid, 3)
    all3 = G.batched(cid, 3)
    for s in range(3):
        one = G.run_batched(cid, 1, y=y[s:s + 1], cot=torch.ones(1, G.L))
        assert G.rel(all3["elbo"][s], one["elbo"][0]) < 1e-12, s
    s0, l0 = 1, 2
    cot = torch.zeros(3, G.L, dtype=torch.float64)
    cot[s0, l0] = -1.7
    got = G.run_batched(cid, 3, cot=cot)
    dy = got["dy"].clone()
    assert float(dy[s0, :, l0].abs().max()) > 0.0
    dy[s0, :, l0] = 0.0
    assert float(dy.abs().max()) == 0.0
    others = [l for l in range(G.L) if l != l0]
    for k in ("draw0", "draw1", "dnoise"):
        assert float(got[k][l0].abs().max()) > 0.0, k
        assert float(got[k][others].abs().max()) == 0.0, k
    # and that entry's gradients are the single-sample call's, scaled
    one = G.run_batched(cid, 1, y=y[s0:s0 + 1], cot=cot[s0:s0 + 1])
    assert G.rel(got["dy"][s0], one["dy"][0]) < 1e-12
    for k in ("draw0", "draw1", "dnoise"):
        assert G.rel(got[k], one[k]) < 1e-10, k
    assert c["N"] == got["dy"].shape[1]


@pytest.mark.parametrize("cid", ["35x2x5", "9x16x120"])
def test_gp_elbo_reproducible(hip, cid):
    a, b = G.run_batched(cid, 3), G.run_batched(cid, 3)
    for k in G.QUANT:
        assert U.bit_equal(a[k], b[k]), k
    x, _, _, _ = G.abi_run(hip, cid, 3)
    y, _, _, _ = G.abi_run(hip, cid, 3)
    for k in x:
        assert U.bit_equal(x[k], y[k]), k


def test_gp_elbo_failure_reporting(hip):
    """a noise that makes B_p indefinite in dim 1: LinAlgError through Python; info = 20000 + col for that dim, 0
    for the others, whose values are unaffected"""
    import lvae_amd as la
    cid, S = "6x7x33", 3
    c = D.problem(cid)
    bad = [float(c["noise"][0]), -50.0, float(c["noise"][2])]
    k0, k1, _ = D.modules_batched(c)
    with pytest.raises(torch.linalg.LinAlgError):
        la.elbo_batched(G.L, k0, k1, D.noise_stub(bad), c["X"].to(DEV), G.samples(cid, S)[0].to(DEV),
                        c["Z"].to(DEV), c["P"], c["T"], G.EPS)
    got, info, _, _ = G.abi_run(hip, cid, S, noise=bad)
    info = info[:G.L].tolist()
    assert info[0] == 0 and info[2] == 0
    assert 20001 <= info[1] <= 20000 + c["T"]
    good, _, _, _ = G.abi_run(hip, cid, S)
    for l in (0, 2):
        assert U.bit_equal(got["elbo"][:, l].contiguous(), good["elbo"][:, l].contiguous())
        assert U.bit_equal(got["dy"][:, :, l].contiguous(), good["dy"][:, :, l].contiguous())


def test_gp_elbo_inputs_are_checked(hip):
    import lvae_amd as la
    cid = "6x7x33"
    c = D.problem(cid)
    k0, k1, lik = D.modules_batched(c)
    X, Z = c["X"].to(DEV), c["Z"].to(DEV)
    y = G.samples(cid, 3)[0].to(DEV)
    with pytest.raises(ValueError):
        la.elbo_batched(G.L, k0, k1, lik, X, y, Z, c["P"] + 1, c["T"], G.EPS)
    with pytest.raises(ValueError):
        la.elbo_batched(G.L, k0, k1, lik, X, y[:, :, :2], Z, c["P"], c["T"], G.EPS)
    with pytest.raises(ValueError):
        la.elbo_batched(G.L, k0, k1, lik, X, y, Z[:2], c["P"], c["T"], G.EPS)
    # a shared [M, Q] z is every dim's z
    a = la.elbo_batched(G.L, k0, k1, lik, X, y, Z[0], c["P"], c["T"], G.EPS)
    b = la.elbo_batched(G.L, k0, k1, lik, X, y, Z[0][None].expand(G.L, -1, -1), c["P"], c["T"], G.EPS)
    assert U.bit_equal(a.detach().cpu(), b.detach().cpu())
    assert bool(torch.isfinite(a).all())
