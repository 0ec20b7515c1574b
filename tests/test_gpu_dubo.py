"""deviance_upper_bound_batched (lvae_dubo_fwd_f64 / lvae_dubo_bwd_f64: the fused subject pass, the partial
reduction, the composed M x M / per-subject algebra and the Gram adjoint) against the reference's golden vector,
the fp64 oracle under CPU autograd, and the per-dim composed lvae_amd.deviance_upper_bound.

Bounds (relative to each quantity's max-norm): value 1e-8; dmu / dlogv 1e-7; raw gradients (kernels and noise)
1e-6 -- about 10 x what two fp64 evaluations of the same bound (explicit inverses, as spd_inv_small implies, vs
the oracle's Cholesky solves) differ by on the CPU at these shapes (1.1e-9, 4.6e-9, 1.2e-8: K0zz's 1e-6 jitter,
cond 1e7..1e8), or the project's existing bound where that is looser.  The golden case keeps
test_gpapprox_elbo_and_dubo_golden's own bounds.

Shapes (dubo_util.CASES, L = 3 each): odd sizes, one subject, T = M = 1, the workload's (T, M) = (16, 120), both
sides of the fused pass's T <= 32 limit and T = M = 128 on the batched-product route, and P one below / on / one
above a multiple of the 16 subjects a workgroup walks, plus three groups.  The group count is ceil(P / 16), so
it never exceeds P: "fewer subjects than groups" cannot occur, the P < 16 cases run one partly filled group.
"""
import numpy as np
import pytest
import torch

import abi_util as U
import dubo_util as D
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = D.DEV


def check(got, ref, bounds, what):
    errs = {k: D.rel(got[k], ref[k]) for k in D.QUANT}
    print(what, " ".join(f"{k} {errs[k]:.2e}" for k in D.QUANT))
    for k in D.QUANT:
        assert errs[k] < bounds[k], (what, k, errs[k])


def test_dubo_batched_reference_golden(hip):
    """The reference's own deviance_upper_bound (gpapprox.npz: P = T = 16, M = 40, one dim): value and gradients"""
    import lvae_amd as la
    g = golden("gpapprox.npz")
    P, T = int(g["P"]), int(g["T"])
    X, Z = torch.tensor(g["X"], device=DEV), torch.tensor(g["Z"], device=DEV)
    k0, k1 = la.generate_kernel_batched(1, **D.CFG, id_covariate=2)
    D.set_raw(k0, g["raw0"].T)
    D.set_raw(k1, g["raw1"].T)
    k0, k1 = k0.to(DEV), k1.to(DEV)
    lik = la.GaussianLikelihood(1, noise=float(g["noise"])).to(DEV)
    mu = torch.tensor(g["mu"], device=DEV)[:, None].requires_grad_()
    lv = torch.tensor(g["logv"], device=DEV)[:, None].requires_grad_()
    du = la.deviance_upper_bound_batched(1, k0, k1, lik, X, mu, lv, Z[None], P, T, float(g["eps"]))
    assert du.shape == (1,)
    du.sum().backward()
    errs = dict(dubo=D.rel(du[0], g["dubo"]), dmu=D.rel(mu.grad[:, 0], g["dubo_dmu"]),
                dlogv=D.rel(lv.grad[:, 0], g["dubo_dlogv"]),
                draw0=D.rel(torch.cat([p.grad for _, p in k0.named_parameters()]), g["dubo_draw0"][:, 0]),
                draw1=D.rel(torch.cat([p.grad for _, p in k1.named_parameters()]), g["dubo_draw1"][:, 0]))
    print("golden", errs)
    assert errs["dubo"] < 1e-9
    assert errs["dmu"] < 1e-7
    assert errs["dlogv"] < 1e-7
    assert errs["draw0"] < 1e-6
    assert errs["draw1"] < 1e-6


@pytest.mark.parametrize("cid", D.CASE_IDS)
def test_dubo_batched_vs_oracle(hip, cid):
    check(D.batched(cid), D.oracle(cid), D.BOUND, f"{cid} vs oracle:")


@pytest.mark.parametrize("cid", D.CASE_IDS)
def test_dubo_batched_vs_composed(hip, cid):
    """each dubo_l and every gradient against the per-dim composed route; module lists == batched modules, bitwise"""
    got = D.batched(cid)
    check(got, D.composed(cid), D.BOUND, f"{cid} vs composed:")
    lst = D.run_batched(cid, "list")
    for k in D.QUANT:
        assert U.bit_equal(lst[k], got[k]), k


@pytest.mark.parametrize("cid", ["9x16x120", "17x3x9", "2x128x128"])
def test_dubo_reproducible(hip, cid):
    a, b = D.run_batched(cid), D.run_batched(cid)
    for k in D.QUANT:
        assert U.bit_equal(a[k], b[k]), k
    x, _, _, _ = D.abi_run(hip, cid)
    y, _, _, _ = D.abi_run(hip, cid)
    for k in x:
        assert U.bit_equal(x[k], y[k]), k


@pytest.mark.parametrize("cid", ["6x7x33", "3x33x17"])
def test_dubo_cotangent_scales_each_dim(hip, cid):
    """gdubo [L] non-uniform: dim l's gradients are gdubo[l] x those of a unit cotangent; every output, pre-filled
    with NaN, is overwritten (and nothing behind it is)"""
    cot = [0.5, -2.0, 3.0]
    one, _, _, _ = D.abi_run(hip, cid)
    got, info, bufs, n = D.abi_run(hip, cid, cot=cot)
    assert info[:D.L].tolist() == [0] * D.L
    g = torch.tensor(cot, dtype=torch.float64)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
        assert U.all_sentinel(bufs[k][n[k]:]), k
    assert U.bit_equal(got["dubo"], one["dubo"])
    for k in ("dmu", "dlogv"):
        assert D.rel(got[k], one[k] * g[None, :]) < 1e-12, k
    for k in ("dp0", "dp1"):
        assert D.rel(got[k], one[k] * g[:, None]) < 1e-12, k
    assert D.rel(got["dnoise"], one["dnoise"] * g) < 1e-12
    # through Python
    py = D.run_batched(cid, cot=cot)
    ref = D.batched(cid)
    assert D.rel(py["dmu"], ref["dmu"] * g[None, :]) < 1e-12
    assert D.rel(py["draw1"], ref["draw1"] * g[:, None]) < 1e-12


def test_dubo_failure_reporting(hip):
    """a noise that makes B_p indefinite in dim 1: LinAlgError through Python; info = 20000 + col for that dim, 0
    for the others, whose values are unaffected"""
    import lvae_amd as la
    cid = "6x7x33"
    c = D.problem(cid)
    bad = [float(c["noise"][0]), -50.0, float(c["noise"][2])]
    k0, k1, _ = D.modules_batched(c)
    with pytest.raises(torch.linalg.LinAlgError):
        la.deviance_upper_bound_batched(D.L, k0, k1, D.noise_stub(bad), c["X"].to(DEV), c["mu"].to(DEV),
                                        c["lv"].to(DEV), c["Z"].to(DEV), c["P"], c["T"], D.EPS)
    got, info, _, _ = D.abi_run(hip, cid, noise=bad)
    info = info[:D.L].tolist()
    assert info[0] == 0 and info[2] == 0
    assert 20001 <= info[1] <= 20000 + c["T"]
    good, _, _, _ = D.abi_run(hip, cid)
    for l in (0, 2):
        assert U.bit_equal(got["dubo"][l], good["dubo"][l])
        assert U.bit_equal(got["dmu"][:, l].contiguous(), good["dmu"][:, l].contiguous())


def test_dubo_inputs_are_checked(hip):
    import lvae_amd as la
    c = D.problem("5x3x9")
    k0, k1, lik = D.modules_batched(c)
    X, mu, lv, Z = c["X"].to(DEV), c["mu"].to(DEV), c["lv"].to(DEV), c["Z"].to(DEV)
    with pytest.raises(ValueError):
        la.deviance_upper_bound_batched(D.L, k0, k1, lik, X, mu, lv, Z, c["P"] + 1, c["T"], D.EPS)
    with pytest.raises(ValueError):
        la.deviance_upper_bound_batched(D.L, k0, k1, lik, X, mu[:, :2], lv[:, :2], Z, c["P"], c["T"], D.EPS)
    # a shared [M, Q] z is every dim's z
    a = la.deviance_upper_bound_batched(D.L, k0, k1, lik, X, mu, lv, Z[0], c["P"], c["T"], D.EPS)
    b = la.deviance_upper_bound_batched(D.L, k0, k1, lik, X, mu, lv, Z[0][None].expand(D.L, -1, -1), c["P"], c["T"],
                                        D.EPS)
    assert U.bit_equal(a.detach().cpu(), b.detach().cpu())
    assert np.isfinite(a.detach().cpu().numpy()).all()
