"""The conditioned DUBO on the GPU (lvae_dubo_cond_prepare_f64 / lvae_dubo_cond_eval_f64, condition_dubo,
condition_dubo_varying_T) against the oracle's joint DUBO: value, dm and dlogv at m = 0 / l = 0, at the problem's own
latents and at a far point with non-unit cotangents.  Cases, free sets, bounds: dubo_cond_util."""
import functools
import os

import numpy as np
import pytest
import torch

import dubo_cond_util as C
import dubo_util as D
import varying_util as V
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = C.DEV
L = C.L


@functools.lru_cache(maxsize=None)
def _prepared(cid):
    from lvae_amd import _lib
    return C.prepare(_lib.lib(), cid)


@pytest.mark.parametrize("name", C.POINTS)
@pytest.mark.parametrize("cid", C.GPU_CASES)
def test_abi_matches_joint_oracle(hip, cid, name):
    prep = _prepared(cid)
    assert not prep["info"].any()
    m, lv, cot = C.point(cid, name)
    got = C.evaluate(hip, prep, m, lv, cot)
    C.check(got, C.oracle(cid, name), f"{cid} {name}", C.bound_for(cid, name))


def _split(c):
    """(x_new, x_train, m_train, lv_train) of a problem: the free subjects' rows first, as condition_dubo takes them"""
    keep = torch.ones(c["N"], dtype=torch.bool)
    keep[c["rows"]] = False
    return c["X"][c["rows"]], c["X"][keep], c["mu"][keep], c["lv"][keep]


def _run_python(cond, m, lv, cot, dtype=torch.float64):
    md, ld = m.to(DEV, dtype).requires_grad_(), lv.to(DEV, dtype).requires_grad_()
    vals = cond(md, ld)
    assert vals.shape == (L,) and vals.dtype == torch.float64
    vals.backward(cot.to(DEV))
    assert md.grad.dtype == dtype and ld.grad.dtype == dtype
    return dict(dubo=vals.detach().cpu(), dm=md.grad.cpu(), dlogv=ld.grad.cpu())


@pytest.mark.parametrize("form", ["batched", "list"])
@pytest.mark.parametrize("cid", ["6x7x33", "3x33x17", "1x4x3"])
def test_condition_dubo_forms(cid, form):
    """(the joint bound does not depend on the order of the subjects: the oracle's joint batch serves as it stands)"""
    import lvae_amd as la
    c = C.problem(cid)
    k0, k1, lik = D.modules_batched(c) if form == "batched" else D.modules_list(c)
    z = c["Z"].to(DEV) if form == "batched" else [zi.to(DEV) for zi in c["Z"]]
    xn, xt, mt, lt = (t.to(DEV) for t in _split(c))
    cond = la.condition_dubo(L, k0, k1, lik, xn, xt, mt, lt, z, c["T"], C.EPS)
    assert (cond.L, cond.Pn, cond.Nn) == (L, c["Pn"], c["Nn"])
    for name in ("own", "far"):
        got = _run_python(cond, *C.point(cid, name))
        C.check(got, C.oracle(cid, name), f"{cid} {form} {name}", C.bound_for(cid, name))


def test_condition_dubo_agrees_with_the_batched_dubo_and_freezes_the_prior():
    """HIP against HIP on the joint batch, and: nothing reaches the kernels, the noise, z or the training latents"""
    import lvae_amd as la
    cid = "9x16x120"
    c = C.problem(cid)
    k0, k1, lik = D.modules_batched(c)
    z = c["Z"].to(DEV).requires_grad_()
    xn, xt, mt, lt = (t.to(DEV) for t in _split(c))
    mt.requires_grad_()
    lt.requires_grad_()
    cond = la.condition_dubo(L, k0, k1, lik, xn, xt, mt, lt, z, c["T"], C.EPS)
    m, lv, cot = C.point(cid, "far")
    got = _run_python(cond, m, lv, cot)
    params = list(k0.parameters()) + list(k1.parameters()) + list(lik.parameters())
    assert params and all(p.requires_grad for p in params)
    assert all(p.grad is None for p in params + [z, mt, lt])
    mj, lj = m.to(DEV).requires_grad_(), lv.to(DEV).requires_grad_()
    vals = la.deviance_upper_bound_batched(L, k0, k1, lik, torch.cat([xn, xt]), torch.cat([mj, mt.detach()]),
                                           torch.cat([lj, lt.detach()]), z.detach(), c["P"], c["T"], C.EPS)
    vals.backward(cot.to(DEV))
    C.check(got, dict(dubo=vals.detach(), dm=mj.grad, dlogv=lj.grad), f"{cid} hip-vs-hip")


VARYING = {"7x9": (1, 3), "3x33": (1,)}    # the free subjects' ids; subject 1 has one row in both cases


@pytest.mark.parametrize("form", ["batched", "list"])
@pytest.mark.parametrize("cid", list(VARYING))
def test_condition_dubo_varying_T(cid, form):
    import lvae_amd as la
    c = V.problem(cid)
    new = torch.isin(c["X"][:, V.ID_COL], torch.tensor(VARYING[cid], dtype=torch.float64))
    order = torch.randperm(int(new.sum()), generator=torch.Generator().manual_seed(5))   # the caller's own row order
    xn, mn, ln = c["X"][new][order], c["mu"][new][order], c["lv"][new][order]
    xt, mt, lt = c["X"][~new], c["mu"][~new], c["lv"][~new]
    n_new = xn.shape[0]
    dubo = lambda p0, p1, nz, x, mj, lj, l: V.loop_dubo(c["s0"], p0[l], c["s1"], p1[l], nz[l], x, mj[:, l], lj[:, l],
                                                        c["Z"][l], V.ID_COL, V.EPS)
    k0, k1, lik = D.modules_batched(c) if form == "batched" else D.modules_list(c)
    z = c["Z"].to(DEV) if form == "batched" else [zi.to(DEV) for zi in c["Z"]]
    cond = la.condition_dubo_varying_T(L, k0, k1, lik, xn.to(DEV), xt.to(DEV), mt.to(DEV), lt.to(DEV), z, V.ID_COL,
                                       V.EPS)
    assert (cond.L, cond.Pn, cond.Nn) == (L, len(VARYING[cid]), n_new)
    cot = torch.tensor(C.COT, dtype=torch.float64)
    for name, (m, lv, g) in dict(own=(mn, ln, torch.ones(L, dtype=torch.float64)), far=(mn + 3.0, ln - 3.0, cot)).items():
        ref = C.oracle_at(c, m, lv, g, x=torch.cat([xn, xt]), mu=torch.cat([mn, mt]), logv=torch.cat([ln, lt]),
                          rows=torch.arange(n_new), dubo_fn=dubo)
        C.check(_run_python(cond, m, lv, g), ref, f"varying {cid} {form} {name}")
    with pytest.raises(ValueError):
        la.condition_dubo_varying_T(L, k0, k1, lik, xn.to(DEV), c["X"].to(DEV), c["mu"].to(DEV), c["lv"].to(DEV), z,
                                    V.ID_COL, V.EPS)


def test_golden_of_the_reference_loss():
    """the reference's deviance_upper_bound on cat(pred, train) and its autograd gradients wrt the pred latents"""
    import lvae_amd as la
    g = np.load(os.path.join(ROOT, "tests", "golden", "dubo_cond.npz"))
    Lg, Pn, T = int(g["L"]), int(g["Pn"]), int(g["T"])
    k0, k1 = la.generate_kernel_batched(Lg, **D.CFG, id_covariate=int(g["id_covariate"]))
    D.set_raw(k0, g["raw0"])
    D.set_raw(k1, g["raw1"])
    lik = la.GaussianLikelihood(Lg, noise=1.0)
    lik.noise = torch.tensor(g["noise"])
    X, mu, lv = (torch.tensor(g[k]).to(DEV) for k in ("X", "mu", "logv"))
    n = Pn * T
    cond = la.condition_dubo(Lg, k0.to(DEV), k1.to(DEV), lik.to(DEV), X[:n], X[n:], mu[n:], lv[n:],
                             torch.tensor(g["Z"]).to(DEV), T, float(g["eps"]))
    for q in range(2):
        m, l = torch.tensor(g["m_pts"][q]).to(DEV).requires_grad_(), torch.tensor(g["lv_pts"][q]).to(DEV).requires_grad_()
        vals = cond(m, l)
        vals.sum().backward()
        C.check(dict(dubo=vals.detach(), dm=m.grad, dlogv=l.grad),
                dict(dubo=torch.tensor(g["dubo"][q]), dm=torch.tensor(g["dubo_dm"][q]),
                     dlogv=torch.tensor(g["dubo_dlogv"][q])), f"golden point {q}")
