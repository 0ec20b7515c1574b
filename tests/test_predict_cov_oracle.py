"""The dense fp64 oracle of the joint predictive covariance ("Joint covariance and trajectory draws") on
top of test_predict_var_oracle's definitions, and the cases the GPU tests of the covariance run
(test_gpu_predict_cov.py, test_gpu_predict_cov_abi.py).  No GPU here.

Per latent dim the oracle forms the whole [Nt, Nt] matrix K** - K*^T Sigma^-1 K* with Sigma, K* and K** exactly as
test_predict_var_oracle assembles them (one torch.linalg.solve), symmetrised; a group's block is its rows and
columns in the group's order of appearance.  tests/golden/predict_cov.npz (the same algebra on the reference's own
kernel modules, tests/golden/gen_golden_predict_cov.py) pins it at 1e-12, and its diagonal is predict_var.npz's.

Errors are measured as for the variance, max |got - ref| / max prior variance, over whole blocks.  The yardstick of
the rule min(max(10 x yardstick, 2e-12), 1e-6) is the change of the oracle's blocks under the relative 2^-50
perturbation of hyper-parameters, noise, mu and z that test_predict_var_oracle applies (same helpers, same seeds);
the GPU tests add the oracle's CPU / device spread.

Two inducing-point cases beyond V.IND_CASES: "group-128" (a group of exactly 128 rows, the cap: eight column
tiles) and "tiles-15-16-17" (groups of 15, 16 and 17 rows, one short of, at and one past a tile, with M = 17, T = 5
and ragged seg_len, test rows not grouped by subject).
"""
import functools

import numpy as np
import torch

import abi_util as U
import test_predict_var_oracle as V
from conftest import golden
from oracle import lvae_oracle as O


# ------------------------------------------------------------------------------------------------------
# the dense oracle (device-agnostic): (cov [L, Nt, Nt], prior [Nt, L])
# ------------------------------------------------------------------------------------------------------
def _joint(Sigma, kstar, kss):
    c = kss - kstar.T @ torch.linalg.solve(Sigma, kstar)
    return 0.5 * (c + c.T)


def dense_exact_cov(spec, params, noise, x, tx):
    eye = torch.eye(x.shape[0], dtype=x.dtype, device=x.device)
    cov, prior = [], []
    for l in range(params.shape[0]):
        kss = O.gram(spec, params[l], tx, tx)
        cov.append(_joint(O.gram(spec, params[l], x, x) + noise[l] * eye, O.gram(spec, params[l], x, tx), kss))
        prior.append(torch.diagonal(kss))
    return torch.stack(cov), torch.stack(prior, 1)


def dense_inducing_cov(s0, p0, s1, p1, noise, xp, xt, z, eps):
    n, M = xp.shape[0], z.shape[1]
    eye_n = torch.eye(n, dtype=xp.dtype, device=xp.device)
    cov, prior = [], []
    for l in range(p0.shape[0]):
        K0zz = O.gram(s0, p0[l], z[l], z[l]) + eps * torch.eye(M, dtype=xp.dtype, device=xp.device)
        K0xz, K0Xz = O.gram(s0, p0[l], xp, z[l]), O.gram(s0, p0[l], xt, z[l])
        A, Q = torch.linalg.solve(K0zz, K0xz.T), torch.linalg.solve(K0zz, K0Xz.T)
        Sigma = K0xz @ A + O.gram(s1, p1[l], xp, xp) + noise[l] * eye_n
        kstar = K0xz @ Q + O.gram(s1, p1[l], xp, xt)
        kss = K0Xz @ Q + O.gram(s1, p1[l], xt, xt)
        cov.append(_joint(Sigma, kstar, kss))
        prior.append(torch.diagonal(kss))
    return torch.stack(cov), torch.stack(prior, 1)


def groups_of(labels):
    """The groups of an [Nt] label vector in ascending label order, each the caller's row indices in order of
    appearance: what PredictiveCovariance.index holds"""
    lab = torch.as_tensor(labels, dtype=torch.float64).reshape(-1)
    order = torch.argsort(lab, stable=True)
    _, counts = torch.unique_consecutive(lab[order], return_counts=True)
    return list(torch.split(order, counts.tolist()))


def ref_blocks(cov, groups):
    """[L, G, n_max, n_max]: the groups' blocks of a dense cov [L, Nt, Nt], the identity on padding"""
    L, n_max = cov.shape[0], max([len(g) for g in groups] + [1])
    out = torch.eye(n_max, dtype=cov.dtype).repeat(L, len(groups), 1, 1)
    for k, g in enumerate(groups):
        out[:, k, :len(g), :len(g)] = cov[:, g][:, :, g]
    return out


def block_err(got, ref, prior):
    """max |got - ref| / max prior over whole blocks, in fp64 on the CPU"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / float(prior.max())) if ref.numel() else 0.0


# ------------------------------------------------------------------------------------------------------
# oracle runs of the cases, plain or perturbed (V's perturbations and seeds)
# ------------------------------------------------------------------------------------------------------
def golden_exact_cov(dev="cpu", perturb=False):
    c = V.golden_exact_inputs()
    if perturb:
        gen = torch.Generator().manual_seed(81)
        c.update({k: U.perturbed(c[k], gen) for k in ("params", "noise", "mu")})
    c = {k: t.to(dev) for k, t in c.items()}
    return tuple(t.cpu() for t in dense_exact_cov(V.exact_spec(), c["params"], c["noise"], c["x"], c["tx"]))


def inducing_cov(c, dev="cpu", perturb=False, seed=82):
    s0, s1 = O.spec_split(**V.REF_CFG, id_covariate=2) if "s0" not in c else (c["s0"], c["s1"])
    v = {k: c[k] for k in ("p0", "p1", "noise", "mu", "z", "xp", "xt")}
    if perturb:
        gen = torch.Generator().manual_seed(seed)
        v.update({k: U.perturbed(v[k], gen) for k in ("p0", "p1", "noise", "mu")})
        v["z"] = V.perturbed_z(v["z"], s0, gen)
    v = {k: t.to(dev) for k, t in v.items()}
    return tuple(t.cpu() for t in dense_inducing_cov(s0, v["p0"], s1, v["p1"], v["noise"], v["xp"], v["xt"], v["z"],
                                                     c["eps"]))


def exact_cov(cid, dev="cpu", perturb=False):
    c = V.exact_problem(cid)
    v = {k: c[k] for k in ("params", "noise", "mu")}
    if perturb:
        gen = torch.Generator().manual_seed(83)
        v = {k: U.perturbed(t, gen) for k, t in v.items()}
    v = {k: t.to(dev) for k, t in v.items()}
    return tuple(t.cpu() for t in dense_exact_cov(c["spec"], v["params"], v["noise"], c["x"].to(dev), c["tx"].to(dev)))


# inducing cases beyond V.IND_CASES, in its format: (pair, L, M, P, T, seg_len, subject ids of the test rows in caller
# order); ids >= P are absent from the prediction set
def _interleaved(counts):
    """subject ids with the given {id: count}, dealt round robin so that no subject's rows are contiguous"""
    left, out = dict(counts), []
    while any(left.values()):
        for s in left:
            if left[s]:
                out.append(s)
                left[s] -= 1
    return tuple(out)


NEW_IND_CASES = {
    "group-128": ("ref", 2, 20, 3, 5, (5, 2, 4), tuple([1] * 128 + [0, 4, 0])),                           # Nt = 131
    "tiles-15-16-17": ("mix1", 3, 17, 4, 5, (5, 1, 3, 4), _interleaved({0: 15, 2: 16, 3: 17, 9: 2})),     # Nt = 50
}
OVER_CAP = ("ref", 1, 20, 3, 5, (5, 2, 4), tuple([1] * 129))    # a group of 129 rows: refused
IND_CASES = {**V.IND_CASES, **NEW_IND_CASES}


@functools.lru_cache(maxsize=None)
def ind_problem(cid):
    """V.ind_problem for V's cases; the same construction for the cases added here"""
    if cid in V.IND_CASES:
        return V.ind_problem(cid)
    pair, L, M, Pn, T, seg, tids = OVER_CAP if cid == "over-cap" else NEW_IND_CASES[cid]
    s0, s1 = U.spec_pairs()[pair]
    k = 50 + sorted(list(NEW_IND_CASES) + ["over-cap"]).index(cid)
    rng = np.random.default_rng(8000 + k)
    gen = torch.Generator().manual_seed(8100 + k)
    NP, Nt = Pn * T, len(tids)
    valid = (torch.arange(T)[None, :] < torch.tensor(seg)[:, None]).reshape(NP)
    tx = U.subject_covariates(rng, Nt, 1).reshape(Nt, U.QC)
    order = np.argsort(np.asarray(tids, dtype=np.int64), kind="stable")
    tx[:, 0] = torch.tensor(rng.uniform(0.0, 0.5 * T, Nt))
    tx[:, U.ID_COL] = torch.tensor([float(t) for t in tids])
    ids = sorted(set(tids))
    counts = [tids.count(s) for s in ids]
    include = torch.tensor([int(p in tids) for p in range(Pn)], dtype=torch.int32)
    mu = torch.randn(NP, L, generator=gen, dtype=torch.float64) * valid[:, None]
    x = U.subject_covariates(rng, Pn, T).reshape(NP, U.QC)
    return dict(s0=s0, s1=s1, L=L, M=M, P=Pn, T=T, Nt=Nt, NP=NP, seg=seg, valid=valid, include=include,
                tx=tx, order=torch.tensor(order), group_subject=[s if s < Pn else -1 for s in ids],
                group_start=[0] + list(np.cumsum(counts)), x=x, z=U.inducing_points(rng, L, M, T), mu_pad=mu,
                p0=U.draw_hypers(rng, L, O.n_params(s0)), p1=U.draw_hypers(rng, L, O.n_params(s1)),
                noise=U.draw_hypers(rng, L, None), eps=V.EPS, xp=x[valid], mu=mu[valid], xt=tx)


def ind_cov(cid, dev="cpu", perturb=False):
    return inducing_cov(ind_problem(cid), dev, perturb, seed=84)


def case_groups(kind, cid):
    """The groups of a case: test subjects (the id covariate) for the inducing-point route, and for the exact
    route, where the caller names them, the same labels"""
    if kind == "golden-exact":
        return groups_of(golden("predict_var.npz")["exact_tx"][:, 2])
    if kind == "golden-ind":
        gv = golden("predict_var.npz")
        return groups_of(gv["ind_X_all"][gv["ind_tidx"], 2])
    c = V.exact_problem(cid) if kind == "exact" else ind_problem(cid)
    return groups_of(c["tx"][:, U.ID_COL])


ORACLES = {"exact": exact_cov, "ind": ind_cov, "golden-exact": lambda _c, **kw: golden_exact_cov(**kw),
           "golden-ind": lambda _c, **kw: inducing_cov(V.golden_inducing_inputs(), **kw)}


@functools.lru_cache(maxsize=None)
def cpu_ref(kind, cid):
    """(cov [L, Nt, Nt], prior [Nt, L], groups, blocks [L, G, n_max, n_max], perturbation yardstick of the blocks),
    on the CPU"""
    cov, prior = ORACLES[kind](cid)
    groups = case_groups(kind, cid)
    blocks = ref_blocks(cov, groups)
    if cov.shape[1] == 0:
        return cov, prior, groups, blocks, 0.0
    pert = ref_blocks(ORACLES[kind](cid, perturb=True)[0], groups)
    return cov, prior, groups, blocks, block_err(pert, blocks, prior)


ALL_CASES = ([("golden-exact", None), ("golden-ind", None)] + [("exact", c) for c in V.EXACT_CASES]
             + [("ind", c) for c in IND_CASES])


# ------------------------------------------------------------------------------------------------------
# CPU tests
# ------------------------------------------------------------------------------------------------------
def test_oracle_reproduces_golden_covariance():
    gc, gv = golden("predict_cov.npz"), golden("predict_var.npz")
    assert set(gc.files) == {"exact_cov", "ind_cov"}                     # data only, two arrays
    for kind, name, nt in (("golden-exact", "exact", 12), ("golden-ind", "ind", 15)):
        cov, prior = ORACLES[kind](None)
        assert cov.shape == (3, nt, nt) and gc[name + "_cov"].shape == (3, nt, nt)
        err = block_err(cov, torch.tensor(gc[name + "_cov"]), prior)
        diag = V.var_err(torch.diagonal(cov, dim1=1, dim2=2).T, torch.tensor(gv[name + "_var"]), prior)
        gdiag = V.var_err(torch.tensor(np.diagonal(gc[name + "_cov"], axis1=1, axis2=2).T.copy()),
                          torch.tensor(gv[name + "_var"]), prior)
        print(f"{name}: oracle against predict_cov.npz {err:.2e}, diagonals against predict_var.npz {diag:.2e} "
              f"{gdiag:.2e}")
        assert err < 1e-12 and diag < 1e-12 and gdiag < 1e-12
        assert U.rel(prior, torch.tensor(gv[name + "_prior"])) < 1e-12


def test_oracle_diagonal_is_the_variance_oracle():
    """On every case the dense covariance's diagonal is test_predict_var_oracle's variance (1e-12 of the prior)."""
    for kind, cid in ALL_CASES:
        if kind == "ind" and cid not in V.IND_CASES:
            continue
        cov, prior = cpu_ref(kind, cid)[:2]
        (_, var, vprior), _ = V.cpu_ref(kind, cid)
        if var.numel():
            assert V.var_err(torch.diagonal(cov, dim1=1, dim2=2).T, var, vprior) < 1e-12, (kind, cid)
            assert U.rel(prior, vprior) < 1e-12, (kind, cid)


def test_cases_are_well_posed():
    """For every GPU case: ten times the blocks' perturbation yardstick stays under the 1e-6 cap; every block is
    symmetric and positive semi-definite up to that yardstick (smallest eigenvalue over the largest prior variance
    >= -yardstick; the oracle symmetrises, so symmetry is exact); and the cases hold the shapes they are named for."""
    for kind, cid in ALL_CASES:
        cov, prior, groups, blocks, ya = cpu_ref(kind, cid)
        assert 10.0 * ya <= 1e-6, (kind, cid, ya)
        if not groups:
            continue
        assert bool((blocks == blocks.transpose(2, 3)).all()), (kind, cid)
        low = float(torch.linalg.eigvalsh(blocks).min()) / float(prior.max())
        print(f"{kind} {cid}: yardstick {ya:.2e}, smallest eigenvalue / max prior {low:.2e}, "
              f"groups {[len(g) for g in groups]}")
        assert low >= -ya, (kind, cid, low, ya)
        assert sorted(int(i) for g in groups for i in g) == list(range(cov.shape[1]))
    sizes = lambda cid: sorted(len(g) for g in case_groups("ind", cid))
    assert max(sizes("tile-cross")) == 70 and max(sizes("group-128")) == 128
    assert sizes("tiles-15-16-17") == [2, 15, 16, 17]
    c = ind_problem("tiles-15-16-17")
    assert (c["M"], c["T"], c["seg"]) == (17, 5, (5, 1, 3, 4)) and -1 in c["group_subject"]
    assert list(c["tx"][:, U.ID_COL]) != sorted(c["tx"][:, U.ID_COL])          # test rows not grouped by subject
    assert max(len(g) for g in groups_of(ind_problem("over-cap")["tx"][:, U.ID_COL])) == 129
    assert max(len(g) for g in case_groups("exact", "n130")) >= 17              # exact groups across a tile


def test_groups_and_blocks_helpers():
    g = groups_of([2.0, 0.0, 2.0, 1.0, 0.0, 2.0])
    assert [t.tolist() for t in g] == [[1, 4], [3], [0, 2, 5]]
    cov = torch.arange(36, dtype=torch.float64).reshape(1, 6, 6)
    b = ref_blocks(cov, g)
    assert b.shape == (1, 3, 3, 3) and b[0, 0, :2, :2].tolist() == [[7.0, 10.0], [25.0, 28.0]]
    assert b[0, 1].tolist() == [[21.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def test_predictive_covariance_object_on_the_cpu():
    """PredictiveCovariance is plain tensor bookkeeping: diagonal() in the caller's row order, block(g) unpadded."""
    from lvae_amd.predict import PredictiveCovariance, _group_index, _row_groups
    order, ids, counts, start, n_max = _row_groups(torch.tensor([2.0, 0.0, 2.0, 1.0, 0.0, 2.0]), "test")
    index = _group_index(order, counts, start, n_max, "cpu")
    assert index.tolist() == [[1, 4, -1], [3, -1, -1], [0, 2, 5]] and counts.tolist() == [2, 1, 3] and n_max == 3
    cov = torch.arange(72, dtype=torch.float64).reshape(2, 6, 6)
    pc = PredictiveCovariance(ref_blocks(cov, groups_of([2.0, 0.0, 2.0, 1.0, 0.0, 2.0])), index, counts)
    assert bool((pc.diagonal() == torch.diagonal(cov, dim1=1, dim2=2).T).all())
    assert pc.block(2).shape == (2, 3, 3) and bool((pc.block(0) == cov[:, [1, 4]][:, :, [1, 4]]).all())
    try:
        _row_groups(torch.zeros(129), "test")
    except ValueError as e:
        assert "group 0" in str(e) and "129" in str(e)
    else:
        raise AssertionError("a group of 129 rows must be refused")


def test_drop_in_utils_exports_sample_trajectories():
    import os
    import sys
    from conftest import ROOT
    d = os.path.join(ROOT, "longitudinal-vae_amd", "dropin")
    sys.path.insert(0, d)
    try:
        sys.modules.pop("utils", None)
        import utils as DU
        import lvae_amd as la
        assert DU.sample_trajectories is la.sample_trajectories and "sample_trajectories" in DU.__all__
    finally:
        sys.path.remove(d)
        sys.modules.pop("utils", None)
