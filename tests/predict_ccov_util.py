"""Oracles and cases of the components' posterior covariance (test_predict_ccov_cpu.py, test_gpu_predict_ccov.py):
per latent dim and test row the joint covariance of the R additive component functions, [L, Nt, R, R], all fp64 from
O.gram + torch.linalg with per-component Grams via predict_comp_util.comp_gram.

Exact route, per dim: Lc = chol(K + noise I), V_r = solve_triangular(Lc, k_r(x, tx)), block = prior diag - V^T V with
prior diag_r = k_r(tx_t, tx_t).

Inducing-point route, per dim, DENSE (independent of the Woodbury route the library takes): over the valid prediction
rows Sigma = K0xz K0zz^-1 K0zx + k1(x, x) + noise I (K0zz with eps I; k1 vanishes between subjects through its cat
factor on the id column, so k1(x, x) is the block diagonal); cross-covariances kc_r = k0_r(x*, z) K0zz^-1 K0zx for a
component of spec0 and kc_r = k1_r(x*, x) for one of spec1; prior[r, s] = k0_r(x*, z) K0zz^-1 k0_s(z, x*) for two
components of spec0 (the Nystrom form: correlated a priori), k1_r(x*, x*) on the diagonal for one of spec1, 0
elsewhere; block = prior - kc_r Sigma^-1 kc_s^T by torch.linalg.solve.

Errors are measured against the largest prior component variance, max |got - ref| / max prior diag.  The yardstick of
the project's tolerance rule is the oracle's change under a relative 2^-50 perturbation (abi_util.perturbed) of
hyper-parameters, noise and, on the inducing route, the continuous columns of z, and on the GPU its CPU / device
spread.

Exact cases: predict_comp_util.EXACT_IDS and three more: r16, a 16-component spec of bucket (16, 4) concatenated
from ext_util's lists (_C0 + _A1 + _B1[1:]; ext_util holds no single spec of 16 components); r1, one component
(predict_comp_util.R1_SPEC); n513, 513 prediction rows: one row past a 512-row slab.  Inducing cases:
predict_comp_util.IND_CASES and two-tiles, ext_util's _C0 (9 components) against an id kernel of 8: R = 17, so a
block spans two tiles of 16.
"""
import functools

import numpy as np
import torch

import abi_util as U
import ext_util
import predict_comp_util as C
import test_predict_var_oracle as V
from oracle import lvae_oracle as O

EPS = C.EPS
R16_SPEC = ext_util._C0 + ext_util._A1 + ext_util._B1[1:]
ID8_SPEC = ext_util._A1 + ext_util._B1[1:] + [[("cat", 2), ("rbf", 1)]]
# id: (spec, L, P, T, prediction rows kept, Nt), as test_gpu_predict_exact_abi.CASES
NEW_EXACT = {
    "r16": (R16_SPEC, 2, 6, 9, None, 21),
    "r1": (C.R1_SPEC, 2, 5, 9, None, 9),
    "n513": (None, 2, 20, 27, 513, 5),      # (None: the reference split as one kernel)
}
EXACT_IDS = C.EXACT_IDS + list(NEW_EXACT)
# id: (spec0, spec1, L, M, P, T, Nt, seg_len, subject ids of the test rows (cycled)), as predict_comp_util.IND_CASES
NEW_IND = {"two-tiles": (ext_util._C0, ID8_SPEC, 2, 5, 3, 6, 11, (6, 1, 4), (1, 0, 5))}
IND_IDS = C.IND_IDS + list(NEW_IND)


# ---- oracles (device-agnostic) ----
def exact_ccov(spec, params, noise, x, tx):
    """(cov [L, Nt, R, R], prior [L, Nt, R]) of the exact route"""
    R = len(spec)
    eye = torch.eye(x.shape[0], dtype=x.dtype, device=x.device)
    covs, priors = [], []
    for l in range(params.shape[0]):
        Lc = torch.linalg.cholesky(O.gram(spec, params[l], x, x) + noise[l] * eye)
        Vs = torch.stack([torch.linalg.solve_triangular(Lc, C.comp_gram(spec, params[l], r, x, tx), upper=False)
                          for r in range(R)])                                          # [R, n, Nt]
        prior = torch.stack([torch.diagonal(C.comp_gram(spec, params[l], r, tx, tx)) for r in range(R)], 1)
        covs.append(torch.diag_embed(prior) - torch.einsum("rit,sit->trs", Vs, Vs))
        priors.append(prior)
    return torch.stack(covs), torch.stack(priors)


def inducing_ccov(s0, p0, s1, p1, noise, xp, xt, z, eps):
    """(cov [L, Nt, R, R], prior [L, Nt, R]) of the inducing-point route; xp the valid prediction rows, z [L, M, Q]"""
    n, M, Nt, R0, R1 = xp.shape[0], z.shape[1], xt.shape[0], len(s0), len(s1)
    dt, dev = xp.dtype, xp.device
    covs, priors = [], []
    for l in range(p0.shape[0]):
        K0zz = O.gram(s0, p0[l], z[l], z[l]) + eps * torch.eye(M, dtype=dt, device=dev)
        K0xz = O.gram(s0, p0[l], xp, z[l])
        A = torch.linalg.solve(K0zz, K0xz.T)                                           # [M, n]
        Sigma = K0xz @ A + O.gram(s1, p1[l], xp, xp) + noise[l] * torch.eye(n, dtype=dt, device=dev)
        k0 = torch.stack([C.comp_gram(s0, p0[l], r, xt, z[l]) for r in range(R0)])    # [R0, Nt, M]
        kc = torch.cat([k0 @ A, torch.stack([C.comp_gram(s1, p1[l], r, xt, xp) for r in range(R1)])])   # [R, Nt, n]
        prior = torch.zeros(Nt, R0 + R1, R0 + R1, dtype=dt, device=dev)
        q0 = torch.linalg.solve(K0zz, k0.transpose(1, 2)).transpose(1, 2)              # [R0, Nt, M]: K0zz^-1 k0_s(z, x*)
        prior[:, :R0, :R0] = torch.einsum("rim,sim->irs", k0, q0)
        for r in range(R1):
            prior[:, R0 + r, R0 + r] = torch.diagonal(C.comp_gram(s1, p1[l], r, xt, xt))
        S = torch.linalg.solve(Sigma, kc.reshape(-1, n).T).T.reshape(kc.shape)        # [R, Nt, n]: Sigma^-1 kc_s
        covs.append(prior - torch.einsum("rin,sin->irs", kc, S))
        priors.append(torch.diagonal(prior, dim1=1, dim2=2))
    return torch.stack(covs), torch.stack(priors)


def ccov_err(got, ref, prior):
    """max |got - ref| / max prior component variance, in fp64 on the CPU"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / float(prior.max()))


def bound(yard):
    """The project's rule: min(max(10 x yardstick, 2e-12), 1e-6)"""
    return min(max(10.0 * yard, 2e-12), 1e-6)


# ---- exact-route problems ----
@functools.lru_cache(maxsize=None)
def exact_problem(cid):
    """test_gpu_predict_exact_abi.problem()'s dict (spec, L, n, Nt, x, tx, mu, params, noise)"""
    import test_gpu_predict_exact_abi as E
    if cid in C.EXACT_IDS:
        return E.problem(cid)
    spec, L, Pn, T, keep, Nt = NEW_EXACT[cid]
    spec = E.SPECS["ref"] if spec is None else spec
    k = list(NEW_EXACT).index(cid)
    rng = np.random.default_rng(11000 + k)
    gen = torch.Generator().manual_seed(11100 + k)
    xa = U.subject_covariates(rng, Pn, T).reshape(Pn * T, U.QC)
    if keep is None:
        rows = np.nonzero(rng.random(Pn * T) >= 0.1)[0]
    else:
        rows = np.sort(rng.choice(Pn * T, keep, replace=False))
    x = xa[torch.tensor(rows)].contiguous()
    n = x.shape[0]
    tx = U.subject_covariates(rng, Nt, 1).reshape(Nt, U.QC)
    tx[:, 0] = torch.tensor(rng.uniform(0.0, 0.5 * T, Nt))
    tids = [0, Pn + 2, Pn - 1, Pn + 5]               # subjects inside and outside the prediction set
    tx[:, U.ID_COL] = torch.tensor([float(tids[i % len(tids)]) for i in range(Nt)])
    return dict(spec=spec, L=L, n=n, Nt=Nt, x=x, tx=tx, mu=torch.randn(n, L, generator=gen, dtype=torch.float64),
                params=U.draw_hypers(rng, L, O.n_params(spec)), noise=U.draw_hypers(rng, L, None))


def exact_oracle(cid, dev="cpu", perturb=False):
    """(cov, prior) on the CPU, computed on dev; None without test rows"""
    c = exact_problem(cid)
    if c["Nt"] == 0:
        return None
    v = {k: c[k] for k in ("params", "noise")}
    if perturb:
        gen = torch.Generator().manual_seed(91)
        v = {k: U.perturbed(t, gen) for k, t in v.items()}
    return tuple(t.cpu() for t in exact_ccov(c["spec"], v["params"].to(dev), v["noise"].to(dev), c["x"].to(dev),
                                             c["tx"].to(dev)))


@functools.lru_cache(maxsize=None)
def exact_ref(cid):
    """((cov, prior), perturbation yardstick) on the CPU; (None, 0) without test rows"""
    ref = exact_oracle(cid)
    if ref is None:
        return None, 0.0
    return ref, ccov_err(exact_oracle(cid, perturb=True)[0], ref[0], ref[1])


# ---- inducing-route problems, in the layout lvae_predict_comp_cov_f64 takes ----
@functools.lru_cache(maxsize=None)
def ind_problem(cid):
    """predict_comp_util.ind_problem()'s dict plus the test rows grouped by subject (stable): order [Nt] (grouped
    row k is the caller's row order[k]), group_subject / group_start (the subject's index in the [P, T] layout, -1
    when it is absent from the prediction set)"""
    if cid in C.IND_CASES:
        c = dict(C.ind_problem(cid))
    else:
        s0, s1, L, M, Pn, T, Nt, seg, tids = NEW_IND[cid]
        k = list(NEW_IND).index(cid)
        rng = np.random.default_rng(12000 + k)
        gen = torch.Generator().manual_seed(12100 + k)
        NP = Pn * T
        valid = (torch.arange(T)[None, :] < torch.tensor(seg)[:, None]).reshape(NP)
        tx = U.subject_covariates(rng, Nt, 1).reshape(Nt, U.QC)
        tx[:, 0] = torch.tensor(rng.uniform(0.0, 0.5 * T, Nt))
        tx[:, U.ID_COL] = torch.tensor([float(tids[i % len(tids)]) for i in range(Nt)])
        c = dict(s0=s0, s1=s1, L=L, M=M, P=Pn, T=T, Nt=Nt, NP=NP, seg=seg, valid=valid, tx=tx,
                 include=torch.tensor([int(p in tids) for p in range(Pn)], dtype=torch.int32),
                 mu=torch.randn(NP, L, generator=gen, dtype=torch.float64) * valid[:, None],
                 x=U.subject_covariates(rng, Pn, T).reshape(NP, U.QC), z=U.inducing_points(rng, L, M, T),
                 p0=U.draw_hypers(rng, L, O.n_params(s0)), p1=U.draw_hypers(rng, L, O.n_params(s1)),
                 noise=U.draw_hypers(rng, L, None))
    tid = c["tx"][:, U.ID_COL]
    order = torch.argsort(tid, stable=True)
    ids, counts = torch.unique_consecutive(tid[order], return_counts=True)
    c["order"] = order
    c["group_subject"] = [int(i) if 0 <= i < c["P"] else -1 for i in ids.tolist()]
    c["group_start"] = [0] + torch.cumsum(counts, 0).tolist()
    return c


def ind_oracle(cid, dev="cpu", perturb=False):
    """(cov, prior) in the caller's row order on the CPU, computed on dev; None without test rows"""
    c = ind_problem(cid)
    if c["Nt"] == 0:
        return None
    v = {k: c[k] for k in ("p0", "p1", "noise", "z")}
    if perturb:
        gen = torch.Generator().manual_seed(92)
        v.update({k: U.perturbed(v[k], gen) for k in ("p0", "p1", "noise")})
        v["z"] = V.perturbed_z(v["z"], c["s0"], gen)
    v = {k: t.to(dev) for k, t in v.items()}
    return tuple(t.cpu() for t in inducing_ccov(c["s0"], v["p0"], c["s1"], v["p1"], v["noise"],
                                                c["x"][c["valid"]].to(dev), c["tx"].to(dev), v["z"], EPS))


@functools.lru_cache(maxsize=None)
def ind_ref(cid):
    ref = ind_oracle(cid)
    if ref is None:
        return None, 0.0
    return ref, ccov_err(ind_oracle(cid, perturb=True)[0], ref[0], ref[1])
