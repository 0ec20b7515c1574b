"""The dense fp64 oracle of the two predictive variances ("Predictive variance"), on top of
oracle.lvae_oracle's Grams, and the cases the GPU tests of the variance run (test_gpu_predict_var.py,
test_gpu_predict_var_abi.py).  No GPU here.

Per latent dim the oracle assembles Sigma whole and solves against it:
    exact:     Sigma = k(X, X) + noise I,                  k* = k(X, X*),                      k** = k(x*, x*)
    inducing:  Sigma = K0xz K0zz^-1 K0zx + k1(X, X) + noise I,  k* = K0xz K0zz^-1 K0zX* + k1(X, X*),
               k** = K0X*z K0zz^-1 K0zX* + k1(x*, x*)                    (K0zz with eps I)
    mean = k*^T Sigma^-1 mu,   var = k** - k*^T Sigma^-1 k*
It reproduces tests/golden/predict_var.npz (the same algebra on the reference's own kernel modules) to 1e-12, and
its mean reproduces the golden Z_pred of the two mean predictors (exact_predict.npz, predict_varying.npz), which
ties the variance's model to the reference's predictors.

Errors of a variance are measured against the largest prior variance, max |got - ref| / max k**: the variance
itself cancels to near zero at observed points.  The yardstick of the project's tolerance rule
min(max(10 x yardstick, 2e-12), 1e-6) is the oracle's change under a relative 2^-50 perturbation of
hyper-parameters, noise, mu and z (and, on the GPU tests, its CPU / device spread).  Of z only the columns a
continuous factor (rbf, per, lin) reads are perturbed: a cat or bin factor compares its column for equality, so
a perturbed category is another category, not a rounding error.
"""
import functools

import numpy as np
import torch

import abi_util as U
from conftest import golden
from oracle import lvae_oracle as O

EPS = 1e-3   # the jitter of the inducing-point ABI cases (as test_gpu_predict_abi.py)
REF_CFG = dict(cat_kernel=[2], bin_kernel=[], sqexp_kernel=[0],
               cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 2}, {'cont_covariate': 0, 'cat_covariate': 3},
                               {'cont_covariate': 1, 'cat_covariate': 4}],
               bin_int_kernel=[], covariate_missing_val=[])   # the golden inducing-point fixtures' config
EXACT_CFG = dict(cat_kernel=[2, 3], bin_kernel=[5], sqexp_kernel=[0],
                 cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 2}, {'cont_covariate': 1, 'cat_covariate': 4}],
                 bin_int_kernel=[], covariate_missing_val=[{'covariate': 1, 'mask': 4}])   # exact_predict.npz's


# ------------------------------------------------------------------------------------------------------
# the dense oracle (device-agnostic); every result [Nt, L]
# ------------------------------------------------------------------------------------------------------
def _posterior(Sigma, kstar, kss, mu):
    a = torch.linalg.solve(Sigma, kstar)                       # [n, Nt]: one solve per test row
    return a.T @ mu, kss - (kstar * a).sum(0)


def dense_exact(spec, params, noise, x, tx, mu):
    """(mean, var, prior) of the exact predictor"""
    eye = torch.eye(x.shape[0], dtype=x.dtype, device=x.device)
    cols = []
    for l in range(params.shape[0]):
        kss = torch.diagonal(O.gram(spec, params[l], tx, tx))
        m, v = _posterior(O.gram(spec, params[l], x, x) + noise[l] * eye, O.gram(spec, params[l], x, tx), kss, mu[:, l])
        cols.append((m, v, kss))
    return tuple(torch.stack(c, 1) for c in zip(*cols))


def dense_inducing(s0, p0, s1, p1, noise, xp, xt, mu, z, eps):
    """(mean, var, prior) of the inducing-point predictor; xp the prediction rows (no padding), z [L, M, Q]"""
    n, M = xp.shape[0], z.shape[1]
    eye_n = torch.eye(n, dtype=xp.dtype, device=xp.device)
    cols = []
    for l in range(p0.shape[0]):
        K0zz = O.gram(s0, p0[l], z[l], z[l]) + eps * torch.eye(M, dtype=xp.dtype, device=xp.device)
        K0xz, K0Xz = O.gram(s0, p0[l], xp, z[l]), O.gram(s0, p0[l], xt, z[l])
        A, Q = torch.linalg.solve(K0zz, K0xz.T), torch.linalg.solve(K0zz, K0Xz.T)
        Sigma = K0xz @ A + O.gram(s1, p1[l], xp, xp) + noise[l] * eye_n
        kstar = K0xz @ Q + O.gram(s1, p1[l], xp, xt)
        kss = (K0Xz * Q.T).sum(1) + torch.diagonal(O.gram(s1, p1[l], xt, xt))
        m, v = _posterior(Sigma, kstar, kss, mu[:, l])
        cols.append((m, v, kss))
    return tuple(torch.stack(c, 1) for c in zip(*cols))


def var_err(got, ref, prior):
    """max |got - ref| / max prior, in fp64 on the CPU"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / float(prior.max()))


# ------------------------------------------------------------------------------------------------------
# the golden fixture's two cases as oracle inputs
# ------------------------------------------------------------------------------------------------------
def exact_spec():
    s0, s1 = O.spec_split(**EXACT_CFG, id_covariate=2)
    return s0 + s1


def golden_exact_inputs():
    g, gv = golden("exact_predict.npz"), golden("predict_var.npz")
    return dict(params=O.constrain(torch.tensor(g["raw"])), noise=torch.tensor(g["noise"]), mu=torch.tensor(g["mu"]),
                x=torch.tensor(g["X"]), tx=torch.tensor(gv["exact_tx"]))


def golden_exact_oracle(dev="cpu", perturb=False):
    c = golden_exact_inputs()
    if perturb:
        gen = torch.Generator().manual_seed(81)
        c.update({k: U.perturbed(c[k], gen) for k in ("params", "noise", "mu")})
    c = {k: t.to(dev) for k, t in c.items()}
    return tuple(t.cpu() for t in dense_exact(exact_spec(), c["params"], c["noise"], c["x"], c["tx"], c["mu"]))


def golden_inducing_inputs(name="predict_var.npz", prefix="ind_"):
    g = golden(name)
    f = lambda k: g[prefix + k]
    X = f("X_all")
    return dict(p0=O.constrain(torch.tensor(f("raw0").T.copy())), p1=O.constrain(torch.tensor(f("raw1").T.copy())),
                noise=torch.tensor(f("noise")).reshape(-1), mu=torch.tensor(f("mu")), z=torch.tensor(f("Z")),
                xp=torch.tensor(X[f("pidx")]), xt=torch.tensor(X[f("tidx")]), eps=float(f("eps")))


def perturbed_z(z, s0, gen):
    """z with the columns that s0's continuous factors read perturbed by a relative 2^-50"""
    cols = sorted({d for comp in s0 for kind, d in comp if kind in ("rbf", "per", "lin")})
    out = z.clone()
    out[..., cols] = U.perturbed(z[..., cols], gen)
    return out


def inducing_oracle(c, dev="cpu", perturb=False, seed=82):
    s0, s1 = O.spec_split(**REF_CFG, id_covariate=2) if "s0" not in c else (c["s0"], c["s1"])
    v = {k: c[k] for k in ("p0", "p1", "noise", "mu", "z", "xp", "xt")}
    if perturb:
        gen = torch.Generator().manual_seed(seed)
        v.update({k: U.perturbed(v[k], gen) for k in ("p0", "p1", "noise", "mu")})
        v["z"] = perturbed_z(v["z"], s0, gen)
    v = {k: t.to(dev) for k, t in v.items()}
    return tuple(t.cpu() for t in dense_inducing(s0, v["p0"], s1, v["p1"], v["noise"], v["xp"], v["xt"], v["mu"],
                                                 v["z"], c["eps"]))


# ------------------------------------------------------------------------------------------------------
# the ABI edge cases (test_gpu_predict_var_abi.py runs them on the GPU)
# ------------------------------------------------------------------------------------------------------
SPECS = {k: s0 + s1 for k, (s0, s1) in U.spec_pairs().items()}
# exact: id: (spec, L, n, nt, chunks): n across the 64-row blocks of potrf / trsm, nt across the 64-column blocks
# of the solve and the variance kernel, both template buckets ("mix2": (16, 4))
EXACT_CASES = {
    "n1": ("ref", 1, 1, 1, (1,)),
    "n63": ("ref", 3, 63, 17, (1, 16, 17)),
    "n65": ("mix2", 1, 65, 70, (1, 16, 70)),
    "n130": ("ref", 3, 130, 70, (1, 16, 70)),
    "nt0": ("ref", 3, 65, 0, (1,)),
}
# inducing: id: (pair, L, M, P, T, seg_len, subject ids of the test rows in caller order).  Ids >= P are absent
# from the prediction set.  "tile-cross": subject 1 has 70 test rows (5 column tiles of 16, the last partial).
IND_CASES = {
    "smallest": ("ref", 1, 1, 1, 1, (1,), (0,)),
    "ragged": ("mix1", 3, 20, 4, 5, (5, 1, 3, 4), tuple([2, 0, 7, 3, 1, 9] * 6 + [2])),          # Nt = 37
    "limits": ("mix2", 1, 128, 3, 20, (20, 1, 13), tuple([1, 0, 2, 5] * 9 + [0])),               # Nt = 37
    "tile-cross": ("ref", 3, 20, 3, 5, (5, 2, 4), tuple([1] * 70 + [0, 2, 4, 0, 2])),            # Nt = 75
    "all-absent": ("ref", 3, 20, 3, 5, (5, 2, 4), tuple([9, 11] * 18 + [9])),                    # Nt = 37
    "one-row": ("mix1", 1, 20, 2, 20, (20, 7), (1,)),                                            # Nt = 1
    "no-test-rows": ("ref", 3, 20, 3, 5, (5, 2, 4), ()),
    # ext_util's ext-b: periodic and linear factors in both kernels, a (16, 4) id kernel
    "ext-b": ("ext-b", 3, 20, 4, 5, (5, 1, 3, 4), tuple([2, 0, 7, 3, 1, 9] * 6 + [2])),          # Nt = 37
}


@functools.lru_cache(maxsize=None)
def exact_problem(cid):
    name, L, n, nt, chunks = EXACT_CASES[cid]
    spec = SPECS[name]
    k = list(EXACT_CASES).index(cid)
    rng = np.random.default_rng(7000 + k)
    gen = torch.Generator().manual_seed(7100 + k)
    Pn, T = max(2, (n + 9) // 10 + 1), 10
    xa = U.subject_covariates(rng, Pn, T).reshape(Pn * T, U.QC)
    x = xa[torch.tensor(np.sort(rng.choice(Pn * T, n, replace=False)))].contiguous()
    tx = U.subject_covariates(rng, max(nt, 1), 1).reshape(max(nt, 1), U.QC)[:nt]
    if nt:
        tx[:, 0] = torch.tensor(rng.uniform(0.0, 0.5 * T, nt))
        tids = [0, Pn + 2, Pn - 1, Pn + 5]
        tx[:, U.ID_COL] = torch.tensor([float(tids[i % len(tids)]) for i in range(nt)])
    return dict(spec=spec, L=L, n=n, nt=nt, chunks=chunks, x=x, tx=tx,
                mu=torch.randn(n, L, generator=gen, dtype=torch.float64),
                params=U.draw_hypers(rng, L, O.n_params(spec)), noise=U.draw_hypers(rng, L, None))


def exact_oracle(cid, dev="cpu", perturb=False):
    c = exact_problem(cid)
    v = {k: c[k] for k in ("params", "noise", "mu")}
    if perturb:
        gen = torch.Generator().manual_seed(83)
        v = {k: U.perturbed(t, gen) for k, t in v.items()}
    v = {k: t.to(dev) for k, t in v.items()}
    return tuple(t.cpu() for t in dense_exact(c["spec"], v["params"], v["noise"], c["x"].to(dev), c["tx"].to(dev),
                                              v["mu"]))


@functools.lru_cache(maxsize=None)
def ind_problem(cid):
    """The [P, T] subject layout with ragged seg_len (padding rows of mu zero) and the test rows grouped by
    subject (stable), with the layout arrays lvae_predict_var_f64 takes."""
    import ext_util
    pair, L, M, Pn, T, seg, tids = IND_CASES[cid]
    s0, s1 = ext_util.all_spec_pairs()[pair]
    k = list(IND_CASES).index(cid)
    rng = np.random.default_rng(8000 + k)
    gen = torch.Generator().manual_seed(8100 + k)
    NP, Nt = Pn * T, len(tids)
    valid = (torch.arange(T)[None, :] < torch.tensor(seg)[:, None]).reshape(NP)
    tx = U.subject_covariates(rng, max(Nt, 1), 1).reshape(max(Nt, 1), U.QC)[:Nt]
    order = np.argsort(np.asarray(tids, dtype=np.int64), kind="stable") if Nt else np.zeros(0, dtype=np.int64)
    if Nt:
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
                noise=U.draw_hypers(rng, L, None), eps=EPS,
                # the oracle's view: valid rows only, test rows in caller order
                xp=x[valid], mu=mu[valid], xt=tx)


def ind_oracle(cid, dev="cpu", perturb=False):
    return inducing_oracle(ind_problem(cid), dev, perturb, seed=84)


@functools.lru_cache(maxsize=None)
def cpu_ref(kind, cid):
    """((mean, var, prior), perturbation yardstick of the variance) on the CPU"""
    fn = {"exact": exact_oracle, "ind": ind_oracle, "golden-exact": lambda _c, **kw: golden_exact_oracle(**kw),
          "golden-ind": lambda _c, **kw: inducing_oracle(golden_inducing_inputs(), **kw)}[kind]
    ref = fn(cid)
    if ref[1].numel() == 0:
        return ref, 0.0
    return ref, var_err(fn(cid, perturb=True)[1], ref[1], ref[2])


ALL_CASES = ([("golden-exact", None), ("golden-ind", None)] + [("exact", c) for c in EXACT_CASES]
             + [("ind", c) for c in IND_CASES])


# ------------------------------------------------------------------------------------------------------
# CPU tests
# ------------------------------------------------------------------------------------------------------
def test_oracle_reproduces_golden_variance():
    gv = golden("predict_var.npz")
    mean, var, prior = golden_exact_oracle()
    assert var.shape == (12, 3)
    assert var_err(var, torch.tensor(gv["exact_var"]), prior) < 1e-12
    assert U.rel(prior, torch.tensor(gv["exact_prior"])) < 1e-12 and U.rel(mean, torch.tensor(gv["exact_mean"])) < 1e-12
    mean, var, prior = inducing_oracle(golden_inducing_inputs())
    assert var.shape == (15, 3)
    assert var_err(var, torch.tensor(gv["ind_var"]), prior) < 1e-12
    assert U.rel(prior, torch.tensor(gv["ind_prior"])) < 1e-12 and U.rel(mean, torch.tensor(gv["ind_mean"])) < 1e-12


def test_golden_inducing_case_is_the_one_described():
    """7 prediction subjects of lengths 1..5, two test subjects absent from them, one subject with test rows at
    observed and at unobserved times, test rows not grouped by subject."""
    gv = golden("predict_var.npz")
    X = gv["ind_X_all"]
    ps, ts = X[gv["ind_pidx"], 2], X[gv["ind_tidx"], 2]
    lengths = sorted(int((ps == s).sum()) for s in np.unique(ps))
    assert len(lengths) == 7 and lengths[0] == 1 and lengths[-1] == 5 and len(ts) == 15
    assert len(set(ts) - set(ps)) == 2
    seen = set(X[gv["ind_pidx"]][ps == 2.0, 0])
    at = [t in seen for t in X[gv["ind_tidx"]][ts == 2.0, 0]]
    assert any(at) and not all(at)
    assert list(ts) != sorted(ts)


def test_dense_mean_is_the_reference_predictors():
    """The model whose variance is defined here has the reference's posterior means: the golden Z_pred of
    model_test.predict_gp (explicit inverse) and of utils.batch_predict_varying_T (eps = 1e-6, cond(K0zz) ~1e8:
    1e-9, the bound test_oracle_golden.py holds the oracle's own Woodbury route to on this fixture)."""
    g = golden("exact_predict.npz")
    from test_gpu_predict_exact import tiny_batch
    assert bool((golden_exact_inputs()["tx"] == tiny_batch()[1]["label"].to(torch.float64)).all())
    assert U.rel(golden_exact_oracle()[0], torch.tensor(g["Z_pred"])) < 1e-10
    gp = golden("predict_varying.npz")
    mean = inducing_oracle(golden_inducing_inputs("predict_varying.npz", ""))[0]
    err = U.rel(mean, torch.tensor(gp["Z_pred"]))
    print(f"dense inducing mean against predict_varying.npz: {err:.2e}")
    assert err < 1e-9


def test_cases_are_well_posed():
    """For every case: ten times the oracle's own yardstick stays under the 1e-6 cap, every oracle variance lies
    in [0, prior], and the cases hold the shapes they are named for."""
    for kind, cid in ALL_CASES:
        (mean, var, prior), ya = cpu_ref(kind, cid)
        assert 10.0 * ya <= 1e-6, (kind, cid, ya)
        if var.numel():
            assert bool((var >= 0).all()) and bool((var <= prior).all()), (kind, cid)
            assert bool(torch.isfinite(mean).all()) and float(prior.min()) > 0
    assert sorted(c[2] for c in EXACT_CASES.values()) == [1, 63, 65, 65, 130]
    assert {c[3] for c in EXACT_CASES.values()} == {0, 1, 17, 70}
    assert {c[2] for c in IND_CASES.values()} == {1, 20, 128} and {c[4] for c in IND_CASES.values()} == {1, 5, 20}
    assert {len(c[6]) for c in IND_CASES.values()} == {0, 1, 37, 75}
    c = ind_problem("tile-cross")
    assert max(b - a for a, b in zip(c["group_start"], c["group_start"][1:])) == 70
    assert set(ind_problem("all-absent")["group_subject"]) == {-1} and not bool(ind_problem("all-absent")["include"].any())
    assert -1 in ind_problem("ragged")["group_subject"] and 0 in ind_problem("ragged")["group_subject"]
