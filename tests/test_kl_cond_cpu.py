"""The conditioned exact KL without a GPU: the closed form the kernels implement against the oracle's joint
kl_closed, the Python surface's rejections, the host side of the C ABI, and LatentInferenceStep's gp_divisor."""
import os
import re

import pytest
import torch

import abi_util as U
import kl_cond_util as C
import simple_vae_util as S
from conftest import ROOT
from oracle import lvae_oracle as O

SYMBOLS = ("lvae_kl_cond_workspace_size", "lvae_kl_cond_prepare_f64")
TOL = 1e-10   # fp64 against fp64 at these condition numbers (noise >= 0.8): relative, on values and gradients


@pytest.mark.parametrize("name", C.POINTS)
@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_closed_form_is_the_joint_kl(cid, name):
    m, lv, cot = C.point(cid, name)
    got, ref = C.closed_eval(C.closed_form(cid), m, lv, cot), C.oracle(cid, name)
    errs = {q: U.rel(got[q], ref[q]) for q in C.QUANT}
    print(cid, name, {q: f"{e:.2e}" for q, e in errs.items()})
    for q, e in errs.items():
        assert e <= TOL, (q, e)
    A = C.closed_form(cid)[3]
    assert float(torch.linalg.eigvalsh(A).min()) > 0.0


def test_no_training_rows_is_the_plain_kl():
    c = C.problem("0+5")
    p, nz = C.hypers(c)
    m, lv, cot = C.point("0+5", "own")
    got = C.closed_eval(C.closed_form("0+5"), m, lv, cot)["val"]
    ref = torch.stack([O.kl_closed(c["spec"], p[l], c["xn"], nz[l], m[:, l], lv[:, l]) for l in range(C.L)])
    assert U.rel(got, ref) <= TOL


@pytest.mark.parametrize("form", ["batched", "list"])
def test_modules_carry_the_oracles_parameters(form):
    """the modules the GPU tests pass hold the oracle's constrained parameters, in its order"""
    from lvae_amd.elbo import _stack_modules
    c = C.problem("5+17")
    k, _ = C.modules(c, form, "cpu")
    _, params = _stack_modules(k)
    assert U.rel(params, C.hypers(c)[0]) < 1e-14


def test_rejections_raise_before_the_library_is_touched(monkeypatch):
    import lvae_amd as la
    from lvae_amd import _lib

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    c = C.problem("5+17")
    k, lik = C.modules(c, "batched", "cpu")
    xn, xt, mu, lv = c["xn"], c["xt"], c["mu_t"], c["lv_t"]
    with pytest.raises(ValueError, match="x_new has no rows"):
        la.condition_kl_closed(k, lik, xn[:0], xt, mu, lv)
    for bad_mu, bad_lv in [(mu[:-1], lv[:-1]), (mu, lv[:, :2]), (mu[:, 0], lv[:, 0]), (mu, lv[:-1])]:
        with pytest.raises(ValueError, match="mu_train / log_var_train"):
            la.condition_kl_closed(k, lik, xn, xt, bad_mu, bad_lv)
    with pytest.raises(ValueError, match="kernel batch"):       # a batch of 3 kernels against L = 2
        la.condition_kl_closed(k, lik, xn, xt, mu[:, :2], lv[:, :2])
    ks, liks = C.modules(c, "list", "cpu")
    with pytest.raises(ValueError, match="kernel batch"):       # a list of 2 kernels against L = 3
        la.condition_kl_closed(ks[:2], liks[:2], xn, xt, mu, lv)
    with pytest.raises(AssertionError, match="touched"):         # valid arguments do reach the library
        la.condition_kl_closed(k, lik, xn, xt, mu, lv)


def test_symbols_declared_exported_and_bound():
    import lvae_amd as la
    from lvae_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lvae_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", src), s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert callable(la.condition_kl_closed)


def test_workspace_size_needs_no_gpu():
    from lvae_amd import _lib
    lib = _lib.load()
    for n, nn, Lh in [(0, 1, 1), (0, 5, 3), (1, 1, 1), (37, 1, 3), (C.SLAB + 3, 40, 3), (130, 257, 2), (4096, 160, 16)]:
        b = lib.lvae_kl_cond_workspace_size(n, nn, Lh)
        assert b > 0 and b % 256 == 0
        assert b >= 8 * Lh * (n * n + n * nn + (2 if n else 1) * nn * nn)
    for bad in [(-1, 5, 3), (4, 0, 3), (4, -2, 3), (4, 5, 0), (4, 5, -1)]:
        assert lib.lvae_kl_cond_workspace_size(*bad) == 0
    sizes = [lib.lvae_kl_cond_workspace_size(70, 33, g) for g in (1, 2, 3)]
    assert sizes[0] < sizes[1] < sizes[2]


class StubCond:
    """a conditioned term in plain torch: a closed form with A = 2 I, r = 0.5, a = 1.5 per dim"""

    def __init__(self, L):
        self.L = L

    def __call__(self, m, lv):
        return (m * m - m + 0.5 * (1.5 * torch.exp(lv) - lv)).sum(0)


@pytest.mark.parametrize("loss_function", ["mse", "nll"])
def test_gp_divisor_none_is_the_step_as_it_was(loss_function):
    """gp_divisor=None: bit for bit the step built without the keyword; a number divides by it instead of by L"""
    from lvae_amd.steps import LatentInferenceStep, infer_new_subjects
    L, D, B = 3, 11, 6
    x, mask, eps = S.inputs(B, D, L, 4)
    vae = S.build(L, D, (300, 30), 21)
    g = torch.Generator().manual_seed(1)
    mu0, lv0 = torch.randn(B, L, generator=g, dtype=torch.float64), 0.1 * torch.randn(B, L, generator=g, dtype=torch.float64)
    outs = {}
    for key, kw in (("plain", {}), ("none", dict(gp_divisor=None)), ("one", dict(gp_divisor=1)), ("L", dict(gp_divisor=L))):
        mu, lv = torch.nn.Parameter(mu0.clone()), torch.nn.Parameter(lv0.clone())
        step = LatentInferenceStep(vae, StubCond(L), mu, lv, torch.optim.Adam([mu, lv], lr=1e-2), weight=0.15,
                                   loss_function=loss_function, **kw)
        out = step(x, mask, eps)
        outs[key] = [o.clone() for o in out] + [mu.detach().clone(), lv.detach().clone()]
    for key in ("none", "L"):
        assert all(torch.equal(a, b) for a, b in zip(outs["plain"], outs[key])), key
    net, _, _, gp = outs["plain"][:4]
    net1, rl1, nl1, gp1 = outs["one"][:4]
    assert U.rel(gp1, L * gp) < 1e-15
    assert U.rel(net1, rl1 + 0.15 * gp1 if loss_function == "mse" else nl1 + gp1) < 1e-15
    # infer_new_subjects hands the keyword on
    res = {}
    for key, kw in (("plain", {}), ("none", dict(gp_divisor=None)), ("one", dict(gp_divisor=1))):
        res[key] = infer_new_subjects(vae, StubCond(L), x, mask, iters=2, loss_function=loss_function,
                                      eps=torch.stack([eps, -eps]), **kw)
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(res["plain"], res["none"]))
    assert U.rel(res["one"][2][:, 3], L * res["plain"][2][:, 3]) < 1e-3 and not torch.equal(res["one"][0], res["plain"][0])
