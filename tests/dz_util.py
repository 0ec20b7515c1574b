"""Shared inputs and runners of the learnable-inducing-point tests (test_dz_cpu.py, test_gpu_dz.py): the gradient of
the three inducing-point bounds with respect to z, and the Gram input adjoint under it.

The yardstick is CPU autograd through oracle/lvae_oracle.py with z.requires_grad_(): O.gram is plain differentiable
torch, so O.deviance_upper_bound, O.gpapprox_elbo, O.hensman_kld and O.hensman_kld_iter give dz as they stand.  The
DUBO and ELBO problems are dubo_util's / gp_elbo_util's (inducing rows drawn from x: a == b hits in every Gram); the
Hensman problems are built from abi_util's covariates and inducing points.

Bound: dz is a contraction of the same dX, dKz that give the raw kernel gradients, so it is held to their bound on
these cases, dubo_util.BOUND["draw0"] = 1e-6 with abi_util.rel (max |a - b| / max |b|)."""
import ctypes
import functools
import zlib

import numpy as np
import torch

import abi_util as U
import dubo_util as D
import gp_elbo_util as G
from oracle import lvae_oracle as O

DEV = D.DEV
L = D.L
BOUND = D.BOUND["draw0"]
assert G.BOUND["draw0"] == BOUND
COT = (1.0, -0.5, 2.0)     # a non-uniform gdubo
# The one named case that misses 1e-6 on the MI355X, 6x7x33: 33 of its 42 rows are inducing rows and many coincide
# for k0 (rows of two subjects at one time point), cond(Kz) = 4.6e7, 3.5e7, 4.7e7 per dim from the oracle.  dX and
# dKz carry the ~1e-9 relative error the raw kernel gradients show there (draw0: 6.6e-9 .. 9.4e-9), and this case's
# dz amplifies it ~1e3-fold (CPU experiment: 1e-9 of max |dKz| as noise moves dim 0's dz by 1e-5); the oracle's own
# dz moves by 2.5e-7 under a 2^-50 perturbation of its inputs.  As the issue prescribes for such a case, its bound
# is 4x the measured error: {(bound, case, samples): 4 x measured}; DESIGN.md 4.3e has both numbers.
CASE_BOUND = {("dubo", "6x7x33", 0): 4 * 1.04e-6,
              ("elbo", "6x7x33", 1): 4 * 1.61e-6, ("elbo", "6x7x33", 3): 4 * 2.54e-6,
              ("elbo", "6x7x33", 16): 4 * 4.54e-6, ("elbo", "6x7x33", 17): 4 * 9.62e-6}
TAIL = 7


def bound_for(kind, cid, S=0, form="batched"):
    """(the shared-z form of 6x7x33 meets 1e-6, 4.89e-7 and 8.72e-7 measured, and is held to it; the list form is the
    batched form's computation)"""
    return BOUND if form == "shared" else CASE_BOUND.get((kind, cid, S), BOUND)


# ------------------------------------------------------------------------------------------------------
# the Gram input adjoint
# ------------------------------------------------------------------------------------------------------
QX = U.QC
# every factor kind, an rbf x cat product and an rbf x rbf product on two columns; template bucket (8, 2)
SPEC_SMALL = [[("rbf", 0)], [("per", 1)], [("lin", 6)], [("cat", 3)], [("bin", 5)], [("rbf", 0), ("cat", 4)],
              [("rbf", 1), ("rbf", 6)]]
# + three-factor components: bucket (16, 4)
SPEC_BIG = SPEC_SMALL + [[("cat", 3), ("rbf", 0), ("bin", 7)], [("per", 6), ("lin", 1), ("rbf", 0)]]
SPECS = {"8x2": SPEC_SMALL, "16x4": SPEC_BIG}
assert U.bucket(SPEC_SMALL) == (8, 2) and U.bucket(SPEC_BIG) == (16, 4)
# 1e-11 of max |dx2|: a term G_ij dk/dx2 carries a few ulp from exp / sin and the rounding of the periodic
# argument 2 pi (a - b) / p, amplified by its size (|a - b| <= 4, p >= 0.5: <= 51 rad, 51 x 2^-53 = 6e-15); with the
# scale, the other factors and G, <= 2e-14 of the term.  A sum of n1 <= 257 such terms in any order adds
# 257 x 2^-53 = 3e-14 of sum |term|, and sum |term| <= 257 max |term|: 1.3e-11 max |term| at the very worst, an
# order less for terms of random sign, so 1e-11 of the largest entry (lvae_gram_bwd_f64's own test holds 1e-12).
GRAM_BOUND = 1e-11


def covariates(rng, shape):
    """[*shape, QX] fp64: columns 0, 1, 6 reals (0 in [0, 4), 1 and 6 in [-2, 2)), 2 an id, 3 and 4 categories,
    5 and 7 0/1 flags (the columns abi_util.subject_covariates gives these roles)"""
    X = np.empty(tuple(shape) + (QX,))
    X[..., 0] = rng.uniform(0.0, 4.0, shape)
    X[..., 1] = rng.uniform(-2.0, 2.0, shape)
    X[..., 2] = rng.integers(0, 5, shape)
    X[..., 3] = rng.integers(0, 3, shape)
    X[..., 4] = rng.integers(0, 4, shape)
    X[..., 5] = rng.integers(0, 2, shape)
    X[..., 6] = rng.uniform(-2.0, 2.0, shape)
    X[..., 7] = rng.integers(0, 2, shape)
    return torch.tensor(X)


@functools.lru_cache(maxsize=None)
def gram_case(bucket, n1, n2, nb=1, Lg=2, mode="plain"):
    """Inputs of one lvae_gram_bwd_x2_f64 case and the oracle's dx2 (autograd of sum G . O.gram wrt x2).  mode:
    'plain'; 'bcast' (one x2 [n2, Q] for every (b, l), stride 0); 'copy' (x2 rows copied from x1: a == b hits);
    'gt' (G handed over transposed, through its strides)."""
    spec = SPECS[bucket]
    rng = np.random.default_rng(zlib.crc32(repr((bucket, n1, n2, nb, Lg, mode)).encode()))
    x1 = covariates(rng, (nb, Lg, n1))
    if mode == "bcast":
        x2s = covariates(rng, (n2,))
        x2 = x2s.expand(nb, Lg, n2, QX).clone()
    elif mode == "copy":
        x2 = x1[:, :, rng.integers(0, n1, n2)].clone()
        x2s = x2
    else:
        x2 = covariates(rng, (nb, Lg, n2))
        x2s = x2
    params = U.draw_hypers(rng, Lg, O.n_params(spec))
    Gm = torch.tensor(rng.standard_normal((nb, Lg, n1, n2)))
    leaf = x2.clone().requires_grad_()
    (O.gram(spec, params, x1, leaf) * Gm).sum().backward()
    return dict(spec=spec, x1=x1, x2=x2s, params=params, G=Gm, ref=leaf.grad, nb=nb, L=Lg, n1=n1, n2=n2, mode=mode)


def gram_x2_call(hip, c, calls=1, Q=QX):
    """lvae_gram_bwd_x2_f64 on sentinel-tailed dx2 and workspace; returns the logical dx2 (CPU) of each call"""
    from lvae_amd import _lib as P
    spec = P.make_spec(c["spec"])
    nb, Lg, n1, n2 = c["nb"], c["L"], c["n1"], c["n2"]
    x1, x2, params = c["x1"].to(DEV).contiguous(), c["x2"].to(DEV).contiguous(), c["params"].to(DEV).contiguous()
    v1 = P.xview(x1, Lg * n1 * QX, n1 * QX)
    v2 = P.xview(x2, 0, 0) if c["mode"] == "bcast" else P.xview(x2, Lg * n2 * QX, n2 * QX)
    if c["mode"] == "gt":
        Gd = c["G"].transpose(-1, -2).contiguous().to(DEV)
        gs = (Lg * n1 * n2, n1 * n2, 1, n1)
    else:
        Gd = c["G"].to(DEV).contiguous()
        gs = (Lg * n1 * n2, n1 * n2, n2, 1)
    nbytes = hip.lvae_gram_bwd_x2_workspace_size(nb, Lg, n1, n2, Q)
    assert nbytes > 0 and nbytes % 256 == 0
    outs = []
    for _ in range(calls):
        n = nb * Lg * n2 * Q
        out = U.sentinel(n + TAIL)
        ws, tail = U.workspace(nbytes)
        rc = hip.lvae_gram_bwd_x2_f64(ctypes.byref(spec), v1, v2, nb, Lg, n1, n2, Q, P.ptr(params), P.ptr(Gd), *gs,
                                      P.ptr(out), P.ptr(ws), P.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        assert U.tail_untouched(tail) and U.all_sentinel(out[n:])
        outs.append(out[:n].reshape(nb, Lg, n2, Q).cpu())
    return outs


# ------------------------------------------------------------------------------------------------------
# DUBO and ELBO through Python, z requiring grad
# ------------------------------------------------------------------------------------------------------
def z_forms(c, form, dev):
    """(what the call gets as z, the leaf tensors whose .grad is dz) for z as [L, M, Q] ('batched'), a per-dim list
    ('list') or one shared [M, Q] ('shared': dim 0's rows for every dim)"""
    if form == "list":
        zs = [zi.clone().to(dev).requires_grad_() for zi in c["Z"]]
        return zs, zs
    z = (c["Z"][0] if form == "shared" else c["Z"]).clone().to(dev).requires_grad_()
    return z, [z]


def z_grad(leaves, form):
    g = torch.stack([t.grad for t in leaves]) if form == "list" else leaves[0].grad
    return g.detach().cpu().clone()


def dubo_gpu(cid, form="batched", cot=COT):
    """deviance_upper_bound_batched with z requiring grad; every quantity of dubo_util plus dz"""
    import lvae_amd as la
    c = D.problem(cid)
    k0, k1, lik = D.modules_list(c) if form == "list" else D.modules_batched(c)
    mu, lv = c["mu"].to(DEV).requires_grad_(), c["lv"].to(DEV).requires_grad_()
    z, leaves = z_forms(c, form, DEV)
    vals = la.deviance_upper_bound_batched(L, k0, k1, lik, c["X"].to(DEV), mu, lv, z, c["P"], c["T"], D.EPS)
    vals.backward(torch.as_tensor(cot, dtype=torch.float64).to(DEV))
    out = D._collect(vals, mu, lv, k0, k1, lik)
    out["dz"] = z_grad(leaves, form)
    return out


@functools.lru_cache(maxsize=None)
def dubo_oracle(cid, form="batched", cot=COT):
    c = D.problem(cid)
    import lvae_amd as la
    k0, k1, lik = D.modules_batched(c, "cpu")
    _, p0 = la.kernel_spec_and_params(k0)
    _, p1 = la.kernel_spec_and_params(k1)
    nz = lik.noise
    mu, lv = c["mu"].clone().requires_grad_(), c["lv"].clone().requires_grad_()
    z, leaves = z_forms(c, form, "cpu")
    zl = (lambda l: z) if form == "shared" else (lambda l: z[l])
    vals = torch.stack([O.deviance_upper_bound(c["s0"], p0[l], c["s1"], p1[l], nz[l], c["X"], mu[:, l], lv[:, l],
                                               zl(l), c["P"], c["T"], D.EPS) for l in range(L)])
    vals.backward(torch.as_tensor(cot, dtype=torch.float64))
    out = D._collect(vals, mu, lv, k0, k1, lik)
    out["dz"] = z_grad(leaves, form)
    return out


def cond_kz(cid):
    """cond(Kz) per dim from the oracle's Gram (for the report a missed bound asks for)"""
    c = D.problem(cid)
    p0 = O.constrain(torch.tensor(c["raw0"]))
    return [float(torch.linalg.cond(O.gram(c["s0"], p0[l], c["Z"][l], c["Z"][l])
                                    + D.EPS * torch.eye(c["M"], dtype=torch.float64))) for l in range(L)]


def elbo_gpu(cid, S, form="batched"):
    """elbo_batched with z requiring grad on gp_elbo_util's samples and seeded (non-uniform) cotangents"""
    import lvae_amd as la
    c = D.problem(cid)
    ys, g = G.samples(cid, S)
    y = ys.to(DEV).requires_grad_()
    k0, k1, lik = D.modules_list(c) if form == "list" else D.modules_batched(c)
    z, leaves = z_forms(c, form, DEV)
    vals = la.elbo_batched(L, k0, k1, lik, c["X"].to(DEV), y, z, c["P"], c["T"], D.EPS)
    vals.backward(g.to(DEV))
    out = G._collect(vals, y, k0, k1, lik)
    out["dz"] = z_grad(leaves, form)
    return out


@functools.lru_cache(maxsize=None)
def elbo_oracle(cid, S, form="batched"):
    import lvae_amd as la
    c = D.problem(cid)
    ys, g = G.samples(cid, S)
    k0, k1, lik = D.modules_batched(c, "cpu")
    _, p0 = la.kernel_spec_and_params(k0)
    _, p1 = la.kernel_spec_and_params(k1)
    nz = lik.noise
    y = ys.clone().requires_grad_()
    z, leaves = z_forms(c, form, "cpu")
    zl = (lambda l: z) if form == "shared" else (lambda l: z[l])
    vals = torch.stack([torch.stack([O.gpapprox_elbo(c["s0"], p0[l], c["s1"], p1[l], nz[l], c["X"], y[s, :, l],
                                                     zl(l), c["P"], c["T"], D.EPS) for l in range(L)])
                        for s in range(S)])
    vals.backward(g)
    out = G._collect(vals, y, k0, k1, lik)
    out["dz"] = z_grad(leaves, form)
    return out


# ------------------------------------------------------------------------------------------------------
# the Hensman bound
# ------------------------------------------------------------------------------------------------------
# id: (L, M, T, P_b, seg_len or None); eps = 1e-3 as test_gpu_hensman_abi.py's cases on these covariates
HN_EPS = 1e-3
HN_CASES = {
    "1x1x1": (1, 1, 1, 1, None),                    # the smallest of everything
    "3x3x2": (3, 3, 3, 2, None),                    # abi_util.info_problem's sizes
    "120x16": (2, 120, 16, 3, None),                # the workload's M and T
    "var-3x3x2": (3, 3, 3, 2, (3, 1)),              # unequal subjects
    "var-17x5x4": (2, 17, 5, 4, (5, 1, 3, 4)),
}


@functools.lru_cache(maxsize=None)
def hn_problem(cid):
    Lh, M, T, P_b, seg = HN_CASES[cid]
    s0, s1 = U.spec_pairs()["ref"]
    seed = 4000 + list(HN_CASES).index(cid)
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    B = P_b * T
    Xh = torch.randn(Lh, M, M, generator=gen, dtype=torch.float64)
    valid = torch.ones(P_b, T, dtype=torch.bool)
    if seg is not None:
        valid = torch.arange(T)[None, :] < torch.tensor(seg)[:, None]
    return dict(cid=cid, s0=s0, s1=s1, L=Lh, M=M, T=T, P_b=P_b, seg=seg, B=B, P_tot=float(4 * P_b + 3),
                x=U.subject_covariates(rng, P_b, T).reshape(B, U.QC), z=U.inducing_points(rng, Lh, M, T),
                raw0=np.log(rng.uniform(0.5, 2.0, (Lh, O.n_params(s0)))),
                raw1=np.log(rng.uniform(0.5, 2.0, (Lh, O.n_params(s1)))),
                noise=rng.uniform(0.5, 2.0, Lh), m=torch.randn(Lh, M, 1, generator=gen, dtype=torch.float64),
                H=Xh @ Xh.transpose(1, 2) / 100.0 + 0.1 * torch.eye(M, dtype=torch.float64),
                mu=torch.randn(B, Lh, generator=gen, dtype=torch.float64),
                logv=0.1 * torch.randn(B, Lh, generator=gen, dtype=torch.float64), valid=valid.reshape(B),
                n_total=float(7 * int(valid.sum()) + 5))


def hn_modules(c, dev=DEV):
    import lvae_amd as la
    k0, k1 = la.generate_kernel_batched(c["L"], **U._REF_CFG, id_covariate=U.ID_COL)
    D.set_raw(k0, c["raw0"])
    D.set_raw(k1, c["raw1"])
    lik = la.GaussianLikelihood(c["L"], noise=1.0)
    lik.noise = torch.tensor(c["noise"])
    return k0.to(dev), k1.to(dev), lik.to(dev)


def hn_gpu(cid, natural_gradient, shared=False):
    """minibatch_KLD_upper_bound (or _iter for the varying cases, on the valid rows alone) with z requiring grad;
    returns (kld, dz, dp0 raw)"""
    from lvae_amd.elbo import minibatch_KLD_upper_bound, minibatch_KLD_upper_bound_iter
    c = hn_problem(cid)
    k0, k1, lik = hn_modules(c)
    ok = c["valid"]
    x, mu, lv = c["x"][ok].to(DEV), c["mu"][ok].to(DEV).requires_grad_(), c["logv"][ok].to(DEV).requires_grad_()
    m, H = c["m"].to(DEV), c["H"].to(DEV)
    if not natural_gradient:
        m, H = m.requires_grad_(), H.requires_grad_()
    z = (c["z"][0] if shared else c["z"]).clone().to(DEV).requires_grad_()
    if c["seg"] is None:
        kld, _, _ = minibatch_KLD_upper_bound(k0, k1, lik, c["L"], m, H, x, mu, lv, z, c["P_tot"], c["P_b"], c["T"],
                                              natural_gradient, HN_EPS)
    else:
        P_in = sum(1 for s in c["seg"] if s > 0)
        kld, _, _ = minibatch_KLD_upper_bound_iter(k0, k1, lik, c["L"], m, H, x, mu, lv, z, c["P_tot"], P_in,
                                                   c["n_total"], natural_gradient, U.ID_COL, HN_EPS)
    (-2.5 * kld).backward()
    dp0 = torch.stack([p.grad for _, p in k0.named_parameters()], 1)
    return kld.detach().cpu(), z.grad.detach().cpu(), dp0.detach().cpu()


@functools.lru_cache(maxsize=None)
def hn_oracle(cid, shared=False):
    c = hn_problem(cid)
    k0, k1, lik = hn_modules(c, "cpu")
    import lvae_amd as la
    _, p0 = la.kernel_spec_and_params(k0)
    _, p1 = la.kernel_spec_and_params(k1)
    ok = c["valid"]
    x, mu, lv = c["x"][ok], c["mu"][ok], c["logv"][ok]
    z = (c["z"][0] if shared else c["z"]).clone().requires_grad_()
    zz = z.unsqueeze(0).expand(c["L"], -1, -1) if shared else z
    if c["seg"] is None:
        kld, _, _ = O.hensman_kld(c["s0"], p0, c["s1"], p1, lik.noise.reshape(-1), c["m"], c["H"], x, mu, lv, zz,
                                  c["P_tot"], c["P_b"], c["T"], False, HN_EPS)
    else:
        P_in = sum(1 for s in c["seg"] if s > 0)
        kld, _, _ = O.hensman_kld_iter(c["s0"], p0, c["s1"], p1, lik.noise.reshape(-1), c["m"], c["H"], x, mu, lv, zz,
                                       c["P_tot"], P_in, c["n_total"], False, U.ID_COL, HN_EPS)
    (-2.5 * kld).backward()
    dp0 = torch.stack([p.grad for _, p in k0.named_parameters()], 1)
    return kld.detach(), z.grad.detach().clone(), dp0.detach().clone()


# ------------------------------------------------------------------------------------------------------
# the raw C ABI of the three _bwd_z calls
# ------------------------------------------------------------------------------------------------------
def dz_buffers(hip, Lh, M, N, Q):
    """(dz with a sentinel tail, its logical length, zworkspace, its tail)"""
    nbytes = hip.lvae_bound_dz_workspace_size(Lh, M, N, Q)
    assert nbytes > 0 and nbytes % 256 == 0
    zws, ztail = U.workspace(nbytes)
    n = Lh * M * Q
    return U.sentinel(n + TAIL), n, zws, ztail
