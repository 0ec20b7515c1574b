"""Oracles and cases of the per-component predictions (test_predict_comp_cpu.py, test_gpu_gram_matvec_comp_abi.py,
test_gpu_predict_comp.py), all from O.gram + torch.linalg in fp64.

Component r of a spec alone is the one-component spec [spec[r]] with the parameter columns o_r .. o_{r+1} - 1, o the
running sum of 1 + N_PARAMS per factor (the scale first, as O.gram reads them).

Exact route (test_gpu_predict_exact_abi.solve_oracle with alpha kept):  F[r] = k_r(X*, X) alpha.
Inducing route (utils.py:152-209 as O.batch_predict_varying_T restates it, with b = K0zz^-1 K0zx mu~ and mu~[mask]
kept): the components of spec0 first, k0_r(X*, z) b, then those of spec1, k1_r(X*, x[mask]) mu~[mask], mask = the
prediction rows of subjects that are in the test set.
"""
import functools

import numpy as np
import torch

import abi_util as U
import ext_util
from oracle import lvae_oracle as O

EPS = 1e-3
PAIRS = ext_util.all_spec_pairs()


def offsets(spec):
    """[R + 1]: component r's parameters are columns o[r] .. o[r + 1] - 1"""
    o = [0]
    for comp in spec:
        o.append(o[-1] + 1 + sum(O.N_PARAMS[k] for k, _ in comp))
    return o


def comp_gram(spec, params, r, x1, x2):
    """Component r's Gram: O.gram of the one-component spec on its own parameter columns"""
    o = offsets(spec)
    return O.gram([spec[r]], params[..., o[r]:o[r + 1]], x1, x2)


def labels(spec):
    return ["*".join(f"{k}({d})" for k, d in comp) for comp in spec]


def exact_components(spec, params, noise, x, tx, mu):
    """[R, Nt, L]: k_r(X*, X) (k(X, X) + noise I)^-1 mu per component, one latent dim at a time as solve_oracle"""
    eye = torch.eye(x.shape[0], dtype=x.dtype, device=x.device)
    cols = []
    for l in range(params.shape[0]):
        Lc, _ = O.potrf(O.gram(spec, params[l], x, x) + noise[l] * eye)
        alpha = O.potrs(mu[:, l:l + 1], Lc)
        cols.append(torch.stack([comp_gram(spec, params[l], r, tx, x) @ alpha for r in range(len(spec))]))
    return torch.cat(cols, 2)


def inducing_components(spec0, params0, spec1, params1, noise, pred_x, test_x, mu, z, id_col, eps):
    """[R0 + R1, Nt, L]: O.batch_predict_varying_T's two products split by component"""
    Lh, M = z.shape[0], z.shape[1]
    dt, dev = pred_x.dtype, pred_x.device
    K0xz = O.gram(spec0, params0, pred_x, z)
    K0zz = O.gram(spec0, params0, z, z) + eps * torch.eye(M, dtype=dt, device=dev)
    K0zx = K0xz.transpose(-1, -2)
    H = K0zz
    iB_mu = torch.zeros(Lh, pred_x.shape[0], 1, dtype=dt, device=dev)
    iBs = []
    subjects = torch.unique(pred_x[:, id_col]).tolist()
    for s in subjects:
        sel = pred_x[:, id_col] == s
        xs = pred_x[sel]
        T = xs.shape[0]
        st = xs.unsqueeze(0).expand(Lh, T, xs.shape[-1])
        Bm = O.gram(spec1, params1, st, st) + torch.eye(T, dtype=dt, device=dev) * noise.reshape(Lh, 1, 1)
        iB = torch.cholesky_solve(torch.eye(T, dtype=dt, device=dev), torch.linalg.cholesky(Bm))
        Ks = K0xz[:, sel]
        H = H + Ks.transpose(-1, -2) @ iB @ Ks
        iB_mu[:, sel] = iB @ mu[sel].T.unsqueeze(2)
        iBs.append(iB)
    t = K0xz @ torch.linalg.solve(H, K0zx @ iB_mu)
    corr = torch.zeros_like(iB_mu)
    for i, s in enumerate(subjects):
        sel = pred_x[:, id_col] == s
        corr[:, sel] = iBs[i] @ t[:, sel]
    mu_tilde = iB_mu - corr
    b = torch.linalg.solve(K0zz, K0zx @ mu_tilde)                                   # [L, M, 1]
    test_subjects = torch.unique(test_x[:, id_col]).tolist()
    mask = torch.isin(pred_x[:, id_col], torch.tensor(test_subjects, dtype=dt, device=dev))
    pm, mt = pred_x[mask], mu_tilde[:, mask]
    tl = test_x.unsqueeze(0).expand(Lh, test_x.shape[0], test_x.shape[-1])
    pl = pm.unsqueeze(0).expand(Lh, pm.shape[0], pm.shape[-1])
    out = [comp_gram(spec0, params0, r, tl, z) @ b for r in range(len(spec0))]
    out += [comp_gram(spec1, params1, r, tl, pl) @ mt for r in range(len(spec1))]
    return torch.stack(out).squeeze(3).transpose(1, 2).contiguous()                  # [R, Nt, L]


# ---- inducing-route problems of test_gpu_predict_abi.py's kind ----
# id: (pair, L, M, P, T, Nt, seg_len, subject ids of the test rows (cycled over the rows))
IND_CASES = {
    "smallest": ("ref", 2, 1, 1, 1, 1, (1,), (0,)),
    "m3-mixed": ("mix1", 3, 3, 4, 17, 70, (17, 1, 9, 16), (2, 0, 7)),             # 7: not a prediction subject
    "m128-ragged": ("mix2", 2, 128, 3, 64, 9, (64, 1, 40), (1, 0, 5)),
    "no-test-rows": ("ref", 2, 3, 5, 16, 0, (16, 1, 7, 12, 16), ()),
    "none-included": ("mix1", 2, 3, 5, 16, 7, (16, 1, 7, 12, 16), (9, 11)),        # the k1 components vanish
    "ref-ragged": ("ref", 3, 17, 4, 17, 30, (17, 1, 9, 16), (2, 0, 7)),            # (the Python tests' problem)
    # periodic and linear factors (ext_util): both buckets for spec0; Nt not a multiple of 64, subject 7 / 5 absent
    "ext-a": ("ext-a", 3, 9, 4, 7, 70, (7, 1, 4, 6), (2, 0, 7)),
    "ext-c": ("ext-c", 2, 17, 3, 9, 67, (9, 1, 5), (1, 0, 5)),
}
IND_IDS = list(IND_CASES)


@functools.lru_cache(maxsize=None)
def ind_problem(cid):
    pair, L, M, Pn, T, Nt, seg, tids = IND_CASES[cid]
    s0, s1 = PAIRS[pair]
    rng = np.random.default_rng(7000 + IND_IDS.index(cid))
    gen = torch.Generator().manual_seed(8000 + IND_IDS.index(cid))
    NP = Pn * T
    valid = (torch.arange(T)[None, :] < torch.tensor(seg)[:, None]).reshape(NP)
    tx = U.subject_covariates(rng, max(Nt, 1), 1).reshape(max(Nt, 1), U.QC)[:Nt]
    if Nt:
        tx[:, 0] = torch.tensor(rng.uniform(0.0, 0.5 * T, Nt))
        tx[:, U.ID_COL] = torch.tensor([float(tids[i % len(tids)]) for i in range(Nt)])
    include = torch.tensor([int(p in tids) for p in range(Pn)], dtype=torch.int32)
    mu = torch.randn(NP, L, generator=gen, dtype=torch.float64) * valid[:, None]   # (padding rows of mu: 0)
    return dict(s0=s0, s1=s1, L=L, M=M, P=Pn, T=T, Nt=Nt, NP=NP, seg=seg, valid=valid, include=include, tx=tx,
                x=U.subject_covariates(rng, Pn, T).reshape(NP, U.QC), z=U.inducing_points(rng, L, M, T), mu=mu,
                p0=U.draw_hypers(rng, L, O.n_params(s0)), p1=U.draw_hypers(rng, L, O.n_params(s1)),
                noise=U.draw_hypers(rng, L, None))


def ind_oracle(cid, dev="cpu", perturb=False, total=False):
    """The component oracle [R0 + R1, Nt, L] (total: O.batch_predict_varying_T [Nt, L]); None without test rows"""
    c = ind_problem(cid)
    if c["Nt"] == 0:
        return None
    v = {k: c[k] for k in ("p0", "p1", "noise", "mu")}
    if perturb:
        gen = torch.Generator().manual_seed(78)
        v = {k: U.perturbed(t, gen) for k, t in v.items()}
    ok = c["valid"]
    v = {k: t.to(dev) for k, t in v.items()}
    fn = O.batch_predict_varying_T if total else inducing_components
    return fn(c["s0"], v["p0"], c["s1"], v["p1"], v["noise"], c["x"][ok].to(dev), c["tx"].to(dev),
              v["mu"][ok.to(dev)], c["z"].to(dev), U.ID_COL, EPS).cpu()


@functools.lru_cache(maxsize=None)
def ind_ref(cid):
    """(component oracle, its perturbation yardstick) on the CPU; (None, 0) without test rows"""
    ref = ind_oracle(cid)
    return (None, 0.0) if ref is None else (ref, U.rel(ind_oracle(cid, perturb=True), ref))


# ---- exact-route problems: test_gpu_predict_exact_abi.problem()'s ----
EXACT_IDS = ["smallest", "tile-edge", "mix1", "ext", "few-rows", "no-test-rows", "ext-a"]


def exact_oracle(cid, dev="cpu", perturb=False):
    import test_gpu_predict_exact_abi as E
    c = E.problem(cid)
    if c["Nt"] == 0:
        return None
    v = {k: c[k] for k in ("params", "noise", "mu")}
    if perturb:
        gen = torch.Generator().manual_seed(79)
        v = {k: U.perturbed(t, gen) for k, t in v.items()}
    v = {k: t.to(dev) for k, t in v.items()}
    return exact_components(c["spec"], v["params"], v["noise"], c["x"].to(dev), c["tx"].to(dev), v["mu"]).cpu()


@functools.lru_cache(maxsize=None)
def exact_ref(cid):
    ref = exact_oracle(cid)
    return (None, 0.0) if ref is None else (ref, U.rel(exact_oracle(cid, perturb=True), ref))


def bound(yard):
    """The project's rule: min(max(10 x yardstick, 2e-12), 1e-6)"""
    return min(max(10.0 * yard, 2e-12), 1e-6)


# ---- the fused component product alone (test_gpu_gram_matvec_comp_abi.py) ----
R1_SPEC = [[("cat", 3), ("rbf", 0)]]
# a bare lin on a signed real column, cat x lin, bin x lin, per, per x rbf and the reference kinds; bucket (8, 2)
XLIN = [[("lin", 1)], [("cat", 3), ("lin", 6)], [("bin", 5), ("lin", 6)], [("per", 0)], [("per", 0), ("rbf", 1)],
        [("cat", 2)], [("cat", 2), ("rbf", 0)], [("rbf", 0)]]
MIX1_0 = PAIRS["mix1"][0]


def mv_specs():
    import test_gpu_predict_exact_abi as E
    return {**E.SPECS, "r1": R1_SPEC, "mix1-0": MIX1_0, "xlin": XLIN}


def slabs(n1, n2, L, R):
    """Column slabs S of the component product, read off its workspace size (L S R n1 doubles for S > 1)"""
    from lvae_amd import _lib
    return max(1, int(_lib.load().lvae_gram_matvec_comp_workspace_size(n1, n2, L, R)) // (8 * L * R * n1))


@functools.lru_cache(maxsize=None)
def slab_cols(n1, L, R, limit=4096):
    """The fewest columns (one more than a multiple of 64) at which n1 rows take S >= 2 slabs"""
    for n2 in range(65, limit + 1, 64):
        if slabs(n1, n2, L, R) >= 2:
            return n2
    raise AssertionError(f"no slab path up to {limit} columns")


# id: (spec, L, n1, n2 ("slab" / "slab-64": see slab_cols), per-dim x2, test subjects all absent from x2)
MV_CASES = {
    **{f"e{n1}x{n2}": ("ref", 2, n1, n2, False, False) for n1 in (63, 64, 65) for n2 in (59, 64, 65)},
    "mix1": ("mix1", 3, 130, 243, False, False),
    "mix2": ("mix2", 2, 70, 200, False, False),
    "ext": ("ext", 2, 70, 115, False, False),
    "wide-cols": ("wide-cols", 2, 70, 86, False, False),
    "L1": ("ref", 1, 40, 30, False, False),
    "L16": ("ref", 16, 40, 30, False, False),
    "slab": ("ref", 2, 3, "slab", False, False),
    "slab-64": ("ref", 2, 3, "slab-64", False, False),
    "z1": ("mix1-0", 3, 70, 1, True, False),
    "z17": ("mix1-0", 3, 70, 17, True, False),
    "z128": ("mix1-0", 3, 70, 128, True, False),
    "r1": ("r1", 2, 70, 67, False, False),
    "zero-id": ("ref", 2, 70, 130, False, True),
    # XLIN (linear factors bare and gated, periodic ones): shared and per-dim x2, real and integer-coded times ("-int")
    "xl-1x1": ("xlin", 2, 1, 1, False, False),
    "xl-65x130": ("xlin", 3, 65, 130, False, False),
    "xl-65x130-int": ("xlin", 3, 65, 130, False, False),
    "xl-z65x130": ("xlin", 3, 65, 130, True, False),
    "xl-z65x130-int": ("xlin", 3, 65, 130, True, False),
    "xl-slab": ("xlin", 2, 3, "slab", False, False),
    "xl-zslab-int": ("xlin", 2, 3, "slab", True, False),
    # (the rest of the cross of the three shapes with both x2 forms and both time variants; appended: the ids above
    # keep their seeds)
    "xl-1x1-int": ("xlin", 2, 1, 1, False, False),
    "xl-z1x1": ("xlin", 2, 1, 1, True, False),
    "xl-z1x1-int": ("xlin", 2, 1, 1, True, False),
    "xl-slab-int": ("xlin", 2, 3, "slab", False, False),
    "xl-zslab": ("xlin", 2, 3, "slab", True, False),
}
XL_ZERO_COMP = 2     # XLIN's bin(5) x lin(6): column 6 of x1 is 0 on its first 64-row tile, the gate is on in places
MV_IDS = list(MV_CASES)


@functools.lru_cache(maxsize=None)
def mv_problem(cid):
    name, L, n1, n2, per_dim, absent = MV_CASES[cid]
    spec = mv_specs()[name]
    R = len(spec)
    if n2 == "slab":
        n2 = slab_cols(n1, L, R)
    elif n2 == "slab-64":
        n2 = slab_cols(n1, L, R) - 64
    k = MV_IDS.index(cid)
    rng = np.random.default_rng(9000 + k)
    gen = torch.Generator().manual_seed(9500 + k)
    reps = 3 if name == "wide-cols" else 1
    Pn = max(2, (n2 + 9) // 10)
    if per_dim:
        x2 = U.inducing_points(rng, L, n2, 10)                                      # [L, M, Q]
    else:
        xa = torch.cat([U.subject_covariates(rng, Pn, 11).reshape(Pn * 11, U.QC) for _ in range(reps)], 1)
        x2 = xa[torch.tensor(np.sort(rng.choice(Pn * 11, n2, replace=False)))].contiguous()
    x1 = torch.cat([U.subject_covariates(rng, n1, 1).reshape(n1, U.QC) for _ in range(reps)], 1)
    x1[:, 0] = torch.tensor(rng.uniform(0.0, 5.5, n1))
    tids = [Pn + 1, Pn + 4] if absent else [0, Pn + 2, Pn - 1, Pn + 5]
    x1[:, U.ID_COL] = torch.tensor([float(tids[i % len(tids)]) for i in range(n1)])
    if name == "xlin":
        if n1 > 64:   # the linear factor of column 6 vanishes on the whole first 64-row tile, under bin gates that
            x1[:64, 6] = 0.0       # are on for pairs of that tile and of the rows after it
            x1[::2, 5], x2[..., ::2, 5] = 1.0, 1.0
        if per_dim:                # (inducing rows carry an id no subject has: give some the test rows' id 0)
            x2[..., ::3, U.ID_COL] = 0.0
        if n1 == 1 and n2 == 1:    # the single pair passes every gate
            x1[0, 5], x2[..., 0, 5] = 1.0, 1.0
            if per_dim:
                x2[..., 0, 2], x2[..., 0, 3] = x1[0, 2], x1[0, 3]
            else:
                x1[0, 2], x1[0, 3] = x2[0, 2], x2[0, 3]
        if cid.endswith("-int"):   # integer-coded times: ext_util's walk for x1, distinct integers for x2
            x1[:, 0] = torch.tensor(ext_util.T0[np.arange(n1) % 7])
            tz = np.stack([rng.choice(max(201, 2 * n2), n2, replace=False) for _ in range(L if per_dim else 1)])
            if n2 == 1:
                # one pair has one distance: 2, so that sin's argument pi d / p stays O(1).  At a drawn d ~ 100 the
                # argument ~ 300 carries its own rounding 300-fold into the kernel value on both sides, which the
                # bound's n2 + 16 ulps absorb at n2 = 130 but not at n2 = 1 (measured there: 6.0e-15 against 4.3e-16)
                tz[:] = 2.0
            x2[..., 0] = torch.tensor(tz.astype(np.float64)).reshape(x2.shape[:-1])
    return dict(spec=spec, R=R, L=L, n1=n1, n2=n2, per_dim=per_dim, absent=absent, x1=x1, x2=x2,
                v=torch.randn(n2, L, generator=gen, dtype=torch.float64),
                params=U.draw_hypers(rng, L, O.n_params(spec)))


@functools.lru_cache(maxsize=None)
def mv_ref(cid):
    """(ref [R, n1, L], mag [R, L] = max_i sum_j |K_r,ij v_j|, full-kernel mag [L]) on the CPU"""
    c = mv_problem(cid)
    vt = c["v"].T.unsqueeze(-1)                                                      # [L, n2, 1]
    x1 = c["x1"].unsqueeze(0).expand(c["L"], -1, -1)
    x2 = c["x2"] if c["per_dim"] else c["x2"].unsqueeze(0).expand(c["L"], -1, -1)
    Ks = [comp_gram(c["spec"], c["params"], r, x1, x2) for r in range(c["R"])]      # each [L, n1, n2]
    ref = torch.stack([(K @ vt).squeeze(-1).T for K in Ks])
    mag = torch.stack([(K.abs() @ vt.abs()).squeeze(-1).max(1).values for K in Ks])
    full = (sum(Ks).abs() @ vt.abs()).squeeze(-1).max(1).values
    return ref, mag, full
