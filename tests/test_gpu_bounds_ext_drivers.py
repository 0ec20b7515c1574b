"""The module route to the three bounds with periodic and linear factors: kernels built from the package's own
modules (AdditiveKernel of ScaleKernel(PeriodicKernel | LinearKernel | ProductKernel(..))), batched over L = 3 and as
per-dim lists, with distinct raw parameters per dim, through deviance_upper_bound_batched, elbo_batched and
minibatch_KLD_upper_bound, against the fp64 oracle under CPU autograd through O.constrain: the values and the RAW
parameter gradients (every named_parameters() entry: scale, lengthscale, period; a LinearKernel has none), so that
PeriodicKernel.factor_params' order and the two-parameter / no-parameter columns of _ParamPackFn and
lvae_param_pack_bwd_f64 are pinned beyond the exact KL.

Problems: ext_util's ext-a (both kernels in bucket (8, 2)) and ext-c (a (16, 4) spec0) on 6x7x33 / int and
3x33x17 / real (ext_util.DRIVER_KEYS; test_bounds_ext_cpu.py holds their conditions).  Tolerances: the rule of
test_gpu_bounds_ext_abi.py (max(10 x yardstick, 2e-12) under the caps, single slots at the caps), the yardstick taken
on the raw gradients.  The batched and the per-dim-list forms must agree with each other within the same bound (the
Hensman driver takes batched modules only).

Measured on the MI355X (the quantity closest to its bound per driver):
    driver                    case                 quantity   err        yardstick   bound     err / bound
    dubo, batched and list    6x7x33 ext-a int     draw1      1.48e-12   4.09e-13    4.1e-12   0.36
    elbo, batched and list    3x33x17 ext-a real   draw0      2.77e-13   1.71e-13    2.0e-12   0.14
    hensman, ng 1 and 0       3x33x17 ext-a real   draw0      6.19e-13   3.37e-13    3.4e-12   0.18
The list form gives the batched form's bits in every quantity.  kernel_spec_and_params returns the parameters within
2.5e-15 of the values set.  The module's 18 tests take about 4 s together (the first 1.7 s).
"""
import functools

import pytest
import torch

import abi_util as U
import dubo_util as D
import ext_util as E
import gp_elbo_util as G
from oracle import lvae_oracle as O

pytestmark = pytest.mark.gpu
DEV = U.DEV
L = E.L


def build_kernel(spec, latent_dim):
    """the spec as the package's modules: one ScaleKernel per component over the product of its factors"""
    import lvae_amd as la
    make = dict(cat=lambda d: la.CatKernel(d), bin=lambda d: la.BinKernel(d), lin=lambda d: la.LinearKernel(d),
                rbf=lambda d: la.RbfKernel(d, latent_dim), per=lambda d: la.PeriodicKernel(d, latent_dim))
    comps = []
    for comp in spec:
        k = make[comp[0][0]](comp[0][1])
        for kind, d in comp[1:]:
            k = la.ProductKernel(k, make[kind](d))
        comps.append(la.ScaleKernel(k, latent_dim))
    return la.AdditiveKernel(comps)


def modules(c, form, dev=DEV):
    """(k0, k1, likelihood): batched modules, or per-dim lists of one-dim modules, with the problem's parameters"""
    import lvae_amd as la
    raw0, raw1 = O.unconstrain(c["p0"]), O.unconstrain(c["p1"])
    if form == "batched":
        k0, k1 = build_kernel(c["s0"], L), build_kernel(c["s1"], L)
        D.set_raw(k0, raw0)
        D.set_raw(k1, raw1)
        lik = la.GaussianLikelihood(L, noise=1.0)
        lik.noise = c["noise"]
        return k0.to(dev), k1.to(dev), lik.to(dev)
    k0s, k1s, liks = [], [], []
    for l in range(L):
        k0, k1 = build_kernel(c["s0"], 1), build_kernel(c["s1"], 1)
        D.set_raw(k0, raw0[l:l + 1])
        D.set_raw(k1, raw1[l:l + 1])
        k0s.append(k0.to(dev))
        k1s.append(k1.to(dev))
        liks.append(la.GaussianLikelihood(1, noise=float(c["noise"][l])).to(dev))
    return k0s, k1s, liks


@pytest.mark.parametrize("pair", ["ext-a", "ext-c"])
def test_modules_reproduce_the_specs(hip, pair):
    """kernel_spec_and_params of the built modules: the hand-written spec, bit for bit, and the parameter matrix in
    the oracle's column order (scale, then per factor lengthscale, then period), batched and per dim"""
    import lvae_amd as la
    from lvae_amd import _lib as P
    c = E.problem("6x7x33", pair, "int")
    for which, spec, want in ((0, c["s0"], c["p0"]), (1, c["s1"], c["p1"])):
        kb = modules(c, "batched")[which]
        got_spec, params = la.kernel_spec_and_params(kb)
        assert bytes(got_spec) == bytes(P.make_spec(spec)), (pair, which)
        # unconstrain then constrain: log / exp around |m| = 16, a rounding of 16 x 2^-52 on the logarithm each way
        assert params.shape == want.shape and U.rel(params, want) <= 1e-14
        names = [n.rsplit(".", 1)[1] for n, _ in kb.named_parameters()]
        order = []
        for comp in spec:
            order.append("_log_scale")
            for kind, _ in comp:
                order += dict(rbf=["_log_lengthscale"], per=["_log_lengthscale", "_log_period"]).get(kind, [])
        assert names == order and len(order) == O.n_params(spec)
        kl = modules(c, "list")[which]
        rows = torch.cat([la.kernel_spec_and_params(k)[1] for k in kl], 0)
        assert torch.equal(rows, params)
        assert bytes(la.kernel_spec_and_params(kl[0])[0]) == bytes(got_spec)
    assert torch.unique(c["p0"]).numel() == c["p0"].numel()   # (distinct values: a swapped column cannot match)


# ------------------------------------------------------------------------------------------------------
# the oracle in raw parameters
# ------------------------------------------------------------------------------------------------------
def _jac(p):
    """d constrain(raw) / d raw at raw = unconstrain(p), by autograd through O.constrain (elementwise)"""
    raw = O.unconstrain(p).detach().requires_grad_()
    return torch.autograd.grad(O.constrain(raw).sum(), raw)[0]


def raw_oracle(kind, c, perturb=False, dev="cpu"):
    """ext_util's oracle with the hyper-parameter and noise gradients taken to the raw parameters"""
    out = dict(E.ORACLES[kind](c, perturb=perturb, dev=dev))
    v = E.float_inputs(c, perturb)
    out["dp0"], out["dp1"] = out["dp0"] * _jac(v["p0"]), out["dp1"] * _jac(v["p1"])
    out["dnoise"] = out["dnoise"] * _jac(v["noise"])
    return E.slots(out)


@functools.lru_cache(maxsize=None)
def raw_ref(kind, key):
    c = E.problem(*key)
    ref, per, dev = raw_oracle(kind, c), raw_oracle(kind, c, perturb=True), raw_oracle(kind, c, dev=DEV)
    return ref, {k: max(U.rel(per[k], ref[k]), U.rel(dev[k], ref[k])) for k in ref}


# ------------------------------------------------------------------------------------------------------
# the drivers
# ------------------------------------------------------------------------------------------------------
def _named(out):
    out = dict(out)
    out["dp0"], out["dp1"] = out.pop("draw0"), out.pop("draw1")
    return out


def run_dubo(c, form):
    import lvae_amd as la
    k0, k1, lik = modules(c, form)
    mu, lv = c["mu"].to(DEV).requires_grad_(), c["lv"].to(DEV).requires_grad_()
    z = c["Z"].to(DEV) if form == "batched" else [zi.to(DEV) for zi in c["Z"]]
    vals = la.deviance_upper_bound_batched(L, k0, k1, lik, c["X"].to(DEV), mu, lv, z, c["P"], c["T"], c["eps"])
    vals.backward(torch.tensor(E.COT, dtype=torch.float64, device=DEV))
    return _named(D._collect(vals, mu, lv, k0, k1, lik))


def run_elbo(c, form):
    import lvae_amd as la
    k0, k1, lik = modules(c, form)
    y = c["ys"].to(DEV).requires_grad_()
    z = c["Z"].to(DEV) if form == "batched" else [zi.to(DEV) for zi in c["Z"]]
    vals = la.elbo_batched(L, k0, k1, lik, c["X"].to(DEV), y, z, c["P"], c["T"], c["eps"])
    assert vals.shape == (E.S, L)
    vals.backward(c["g"].to(DEV))
    return _named(G._collect(vals, y, k0, k1, lik))


def run_hensman(c, ng):
    import lvae_amd as la
    k0, k1, lik = modules(c, "batched")
    h = E.hensman_problem(c)
    mu, lv = c["mu"].to(DEV).requires_grad_(), c["lv"].to(DEV).requires_grad_()
    m, H = c["m"].to(DEV).requires_grad_(not ng), c["H"].to(DEV).requires_grad_(not ng)
    kld, gm, gH = la.minibatch_KLD_upper_bound(k0, k1, lik, L, m, H, c["X"].to(DEV), mu, lv, c["Z"].to(DEV),
                                               h["P_tot"], c["P"], c["T"], bool(ng), c["eps"])
    kld.backward()
    d0, d1, dn = D._raw_grads(k0, k1, lik)
    out = dict(kld=kld.reshape(1), dmu=mu.grad, dlogv=lv.grad, dp0=d0, dp1=d1, dnoise=dn)
    out.update(dict(gm=gm, gH=gH) if ng else dict(dm=m.grad, dH=H.grad))
    return {k: v.detach().cpu().clone() for k, v in out.items()}


@pytest.mark.parametrize("key", E.DRIVER_KEYS, ids=["-".join(k) for k in E.DRIVER_KEYS])
def test_dubo_driver(hip, key):
    c = E.problem(*key)
    ref, yard = raw_ref("dubo", key)
    b, lst = run_dubo(c, "batched"), run_dubo(c, "list")
    E.check("dubo driver batched " + "-".join(key), b, ref, yard, E.DUBO_QUANT)
    E.check("dubo driver list " + "-".join(key), lst, ref, yard, E.DUBO_QUANT)
    E.check("dubo driver list / batched " + "-".join(key), lst, b, yard, E.DUBO_QUANT)


@pytest.mark.parametrize("key", E.DRIVER_KEYS, ids=["-".join(k) for k in E.DRIVER_KEYS])
def test_elbo_driver(hip, key):
    c = E.problem(*key)
    ref, yard = raw_ref("elbo", key)
    b, lst = run_elbo(c, "batched"), run_elbo(c, "list")
    E.check("elbo driver batched " + "-".join(key), b, ref, yard, E.ELBO_QUANT)
    E.check("elbo driver list " + "-".join(key), lst, ref, yard, E.ELBO_QUANT)
    E.check("elbo driver list / batched " + "-".join(key), lst, b, yard, E.ELBO_QUANT)


@pytest.mark.parametrize("ng", [1, 0])
@pytest.mark.parametrize("key", E.DRIVER_KEYS, ids=["-".join(k) for k in E.DRIVER_KEYS])
def test_hensman_driver(hip, key, ng):
    import test_gpu_hensman_abi as TH
    ref, yard = raw_ref("hensman", key)
    E.check(f"hensman driver ng={ng} " + "-".join(key), run_hensman(E.problem(*key), ng), ref, yard, TH.active(ng))
