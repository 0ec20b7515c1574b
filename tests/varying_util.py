"""Shared inputs, oracle and runners of the varying-length DUBO / ELBO tests (test_varying_cpu.py,
test_gpu_varying.py): deviance_upper_bound_varying_T, elbo_varying_T and the four lvae_*_seg_f64 calls under them.

The reference has no varying-length DUBO or ELBO, so the yardstick is a loop-form fp64 oracle on the CPU: it
restates oracle.lvae_oracle._gpapprox_common with a list of per-subject blocks of differing size (Cholesky
throughout, O.gram for every Gram), takes its subjects from torch.unique of the id column and accepts the rows in
any order.  At uniform T it is the same mathematics as O.deviance_upper_bound / O.gpapprox_elbo (test_varying_cpu.py
holds the two together at 1e-8; 1.8e-10 / 5.7e-11 measured, the jitter's conditioning).

Problems: dubo_util's recipe (L = 3, dubo_util.CFG, health_mnist_covariates, distinct per-dim raw parameters and
noises), made ragged by keeping the first seg[p] rows of each subject of a uniform [P, T_max] set; inducing rows are
drawn from the rows kept, without replacement wherever the case keeps at least M rows.  9x16 keeps 86 rows, fewer
than its M = 120 (which the 36 lower tiles need): its 120 inducing rows are drawn from the 86 with replacement.
Repeated inducing rows are the regime dz_util describes (rows that coincide for k0; the uniform 9x16x120 has them
too, k0 does not read the id); on the CPU the oracle's own dz of this case moves by 2.1e-7 of its largest entry
under a 2^-50 perturbation of the inputs.  (Taking all 86 kept rows instead leaves a dz of 3e-6 at most, which
the same perturbation moves by 9e-2 of itself: nothing to compare against.)

Bounds are the project's: dubo_util.BOUND / gp_elbo_util.BOUND (value 1e-8, data gradients 1e-7, raw kernel and
noise gradients 1e-6) and dz_util.BOUND (1e-6), all with abi_util.rel."""
import ctypes
import functools

import numpy as np
import torch

import abi_util as U
import dubo_util as D
import dz_util as Z
import gp_elbo_util as G
from oracle import lvae_oracle as O

DEV = D.DEV
L = D.L
EPS = D.EPS
ID_COL = 2
# id: (P, T_max, seg, M)
CASES = {
    "7x9": (7, 9, (9, 1, 4, 7, 2, 9, 5), 20),        # a full subject, then a one-row subject, in one group
    "17x3": (17, 3, tuple(1 + p % 3 for p in range(16)) + (1,), 9),   # a second group of one short subject
    "4x32": (4, 32, (32, 5, 31, 1), 17),             # the last T of the fused pass
    "3x33": (3, 33, (33, 1, 17), 17),                # the first T of the batched-product route
    "9x16": (9, 16, (16, 3, 16, 9, 1, 12, 16, 5, 8), 120),   # the workload's T and M, 36 lower tiles
    "abi2x8": (2, 8, (3, 5), 5),                     # no subject reaches T (C ABI only)
}
PY_CASES = ["7x9", "17x3", "4x32", "3x33", "9x16"]   # every case that goes through the Python calls
DUBO_QUANT = D.QUANT + ["dz"]
ELBO_QUANT = G.QUANT + ["dz"]
DUBO_BOUND = dict(D.BOUND, dz=Z.BOUND)
ELBO_BOUND = dict(G.BOUND, dz=Z.BOUND)
COT = Z.COT
# dz cases that miss dz_util.BOUND for the reason dz_util.CASE_BOUND documents (inducing rows that coincide for k0),
# held to 4 x the measured error: {(bound, case, samples): 4 x measured}.  None was needed.
DZ_CASE_BOUND = {}


def dz_bound(kind, cid, S=0):
    return DZ_CASE_BOUND.get((kind, cid, S), Z.BOUND)


@functools.lru_cache(maxsize=None)
def problem(cid):
    from lvae_amd.data import health_mnist_covariates
    P, T, seg, M = CASES[cid]
    assert len(seg) == P and max(seg) <= T and min(seg) >= 1
    seed = 900 + list(CASES).index(cid)
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    Xfull = torch.tensor(health_mnist_covariates(P, T, seed=seed))          # [P*T, Q], subject-major
    valid = (torch.arange(T)[None, :] < torch.tensor(seg)[:, None]).reshape(-1)
    X = Xfull[valid]
    N = X.shape[0]
    s0, s1 = O.spec_split(**D.CFG, id_covariate=ID_COL)
    Zs = []
    for l in range(L):
        r = np.random.default_rng(seed + 17 * l)
        Zs.append(X[np.sort(r.choice(N, M, replace=M > N))])
    return dict(cid=cid, P=P, T=T, seg=seg, M=M, N=N, X=X, Xfull=Xfull, valid=valid, Z=torch.stack(Zs), s0=s0, s1=s1,
                raw0=np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s0)))),
                raw1=np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s1)))),
                noise=0.8 * np.array([1.0, 1.25, 1.5]),
                mu=torch.randn(N, L, generator=gen, dtype=torch.float64),
                lv=0.1 * torch.randn(N, L, generator=gen, dtype=torch.float64))


@functools.lru_cache(maxsize=None)
def samples(cid, S):
    """y [S, N, L] = mu + 0.3 randn and the cotangents g [S, L], both seeded by (case, S)"""
    c = problem(cid)
    gen = torch.Generator().manual_seed(9000 + 100 * list(CASES).index(cid) + S)
    y = c["mu"][None] + 0.3 * torch.randn(S, c["N"], L, generator=gen, dtype=torch.float64)
    return y, torch.randn(S, L, generator=gen, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def permutation(cid):
    c = problem(cid)
    return torch.randperm(c["N"], generator=torch.Generator().manual_seed(77 + list(CASES).index(cid)))


# ------------------------------------------------------------------------------------------------------
# the loop-form oracle
# ------------------------------------------------------------------------------------------------------
def subject_rows(x, id_col=ID_COL):
    ids = x[:, id_col]
    return [torch.nonzero(ids == s, as_tuple=False).reshape(-1) for s in torch.unique(ids)]


def loop_common(spec0, params0, spec1, params1, noise, x, z, id_col, eps):
    dt = x.dtype
    M = z.shape[0]
    K0xz = O.gram(spec0, params0, x, z)
    K0zz = O.gram(spec0, params0, z, z) + eps * torch.eye(M, dtype=dt)
    LK = torch.linalg.cholesky(K0zz)
    iK = torch.cholesky_solve(torch.eye(M, dtype=dt), LK)
    Q = torch.zeros(M, M, dtype=dt)
    ldB, tr, blocks = 0.0, 0.0, []
    for r in subject_rows(x, id_col):
        xs, n = x[r], int(r.numel())
        K0 = O.gram(spec0, params0, xs, xs)
        LB = torch.linalg.cholesky(O.gram(spec1, params1, xs, xs) + torch.eye(n, dtype=dt) * noise)
        iB = torch.cholesky_solve(torch.eye(n, dtype=dt), LB)
        iBK = iB @ K0xz[r]
        Q = Q + K0xz[r].T @ iBK
        ldB = ldB + 2 * torch.log(torch.diagonal(LB)).sum()
        tr = tr + (iB * K0).sum()
        blocks.append(dict(r=r, LB=LB, iB=iB, iBK=iBK))
    W = K0zz + Q
    LW = torch.linalg.cholesky(0.5 * (W + W.T))
    logdet = -2 * torch.log(torch.diagonal(LK)).sum() + ldB + 2 * torch.log(torch.diagonal(LW)).sum()
    return dict(K0xz=K0xz, blocks=blocks, LW=LW, logdet=logdet, tr=tr - (Q * iK).sum(), M=M)


def loop_quad(c, y):
    q1, p = 0.0, torch.zeros(c["M"], dtype=y.dtype)
    for b in c["blocks"]:
        yr = y[b["r"]]
        iBy = torch.cholesky_solve(yr[:, None], b["LB"])[:, 0]
        q1 = q1 + (yr * iBy).sum()
        p = p + c["K0xz"][b["r"]].T @ iBy
    return q1 - (torch.linalg.solve_triangular(c["LW"], p[:, None], upper=False) ** 2).sum()


def loop_elbo(spec0, params0, spec1, params1, noise, x, y, z, id_col, eps):
    c = loop_common(spec0, params0, spec1, params1, noise, x, z, id_col, eps)
    return -0.5 * x.shape[0] * np.log(2 * np.pi) - 0.5 * (c["logdet"] + loop_quad(c, y)) - 0.5 * c["tr"]


def loop_dubo(spec0, params0, spec1, params1, noise, x, mu, logv, z, id_col, eps):
    c = loop_common(spec0, params0, spec1, params1, noise, x, z, id_col, eps)
    v = torch.exp(logv)
    tr_iB_D, S = 0.0, torch.zeros(c["M"], c["M"], dtype=x.dtype)
    for b in c["blocks"]:
        vr = v[b["r"]]
        tr_iB_D = tr_iB_D + (torch.diagonal(b["iB"]) * vr).sum()
        S = S + (b["iBK"] * vr[:, None]).T @ b["iBK"]
    tr2 = torch.diagonal(torch.cholesky_solve(S, c["LW"])).sum()
    return 0.5 * ((tr_iB_D - tr2) + loop_quad(c, mu) - x.shape[0] + c["logdet"] - logv.sum() + c["tr"])


def _oracle_setup(c):
    import lvae_amd as la
    k0, k1, lik = D.modules_batched(c, "cpu")
    _, p0 = la.kernel_spec_and_params(k0)
    _, p1 = la.kernel_spec_and_params(k1)
    return k0, k1, lik, p0, p1, lik.noise, c["Z"].clone().requires_grad_()


def _rows(c, shuffled):
    return permutation(c["cid"]) if shuffled else torch.arange(c["N"])


@functools.lru_cache(maxsize=None)
def oracle_dubo(cid, shuffled=False):
    """loop_dubo per dim under CPU autograd with the cotangents COT, on the sorted or the shuffled rows; the data
    gradients are those of the rows as given"""
    c = problem(cid)
    k0, k1, lik, p0, p1, nz, z = _oracle_setup(c)
    r = _rows(c, shuffled)
    x = c["X"][r]
    mu, lv = c["mu"][r].clone().requires_grad_(), c["lv"][r].clone().requires_grad_()
    vals = torch.stack([loop_dubo(c["s0"], p0[l], c["s1"], p1[l], nz[l], x, mu[:, l], lv[:, l], z[l], ID_COL, EPS)
                        for l in range(L)])
    vals.backward(torch.as_tensor(COT, dtype=torch.float64))
    out = D._collect(vals, mu, lv, k0, k1, lik)
    out["dz"] = z.grad.detach().clone()
    return out


@functools.lru_cache(maxsize=None)
def oracle_elbo(cid, S, shuffled=False):
    c = problem(cid)
    ys, g = samples(cid, S)
    k0, k1, lik, p0, p1, nz, z = _oracle_setup(c)
    r = _rows(c, shuffled)
    x = c["X"][r]
    y = ys[:, r].clone().requires_grad_()
    vals = torch.stack([torch.stack([loop_elbo(c["s0"], p0[l], c["s1"], p1[l], nz[l], x, y[s, :, l], z[l], ID_COL,
                                               EPS) for l in range(L)]) for s in range(S)])
    vals.backward(g)
    out = G._collect(vals, y, k0, k1, lik)
    out["dz"] = z.grad.detach().clone()
    return out


# ------------------------------------------------------------------------------------------------------
# the Python calls on the GPU
# ------------------------------------------------------------------------------------------------------
def _gpu_setup(c, form):
    k0, k1, lik = D.modules_list(c) if form == "list" else D.modules_batched(c)
    z, leaves = Z.z_forms(c, form, DEV)
    return k0, k1, lik, z, leaves


def gpu_dubo(cid, form="batched", shuffled=False, layout=None):
    import lvae_amd as la
    c = problem(cid)
    k0, k1, lik, z, leaves = _gpu_setup(c, form)
    r = _rows(c, shuffled)
    mu, lv = c["mu"][r].to(DEV).requires_grad_(), c["lv"][r].to(DEV).requires_grad_()
    vals = la.deviance_upper_bound_varying_T(L, k0, k1, lik, c["X"][r].to(DEV), mu, lv, z, ID_COL, EPS, layout=layout)
    assert vals.shape == (L,) and vals.dtype == torch.float64
    vals.backward(torch.as_tensor(COT, dtype=torch.float64).to(DEV))
    out = D._collect(vals, mu, lv, k0, k1, lik)
    out["dz"] = Z.z_grad(leaves, form)
    return out


def gpu_elbo(cid, S, form="batched", shuffled=False):
    import lvae_amd as la
    c = problem(cid)
    ys, g = samples(cid, S)
    k0, k1, lik, z, leaves = _gpu_setup(c, form)
    r = _rows(c, shuffled)
    y = ys[:, r].to(DEV).requires_grad_()
    vals = la.elbo_varying_T(L, k0, k1, lik, c["X"][r].to(DEV), y, z, ID_COL, EPS)
    assert vals.shape == (S, L) and vals.dtype == torch.float64
    vals.backward(g.to(DEV))
    out = G._collect(vals, y, k0, k1, lik)
    out["dz"] = Z.z_grad(leaves, form)
    return out


def check(got, ref, quant, bounds, what):
    errs = {k: D.rel(got[k], ref[k]) for k in quant}
    print(what, " ".join(f"{k} {errs[k]:.2e}" for k in quant))
    for k in quant:
        assert errs[k] < bounds[k], (what, k, errs[k])


# ------------------------------------------------------------------------------------------------------
# the C ABI directly, in the padded layout
# ------------------------------------------------------------------------------------------------------
TAIL = 7
S_ABI = 3


def padded_inputs(cid, dirty):
    """The [P * T, .] padded layout of a case.  dirty = False: padding rows of mu / logv / y are 0 and those of x
    repeat the subject's first row; True: they are NaN, and x's padding rows hold the NEXT subject's covariates.
    cid: a case id, or a ragged problem given whole (ext_util.problem: this module's keys, p0 / p1, ys / g, eps)."""
    c = as_problem(cid)
    P, T, valid = c["P"], c["T"], c["valid"]
    Q = c["X"].shape[1]
    xf = c["Xfull"].reshape(P, T, Q)
    x = (torch.roll(xf, -1, 0) if dirty else xf[:, :1].expand(P, T, Q)).reshape(P * T, Q).clone()
    x[valid] = c["X"]
    fill = float("nan") if dirty else 0.0

    def pad(t):   # [..., N, L] -> [..., P * T, L]
        out = torch.full(t.shape[:-2] + (P * T, L), fill, dtype=torch.float64)
        out[..., valid, :] = t
        return out
    return dict(x=x, mu=pad(c["mu"]), lv=pad(c["lv"]), y=pad(abi_samples(cid)[0]))


def as_problem(cid):
    return problem(cid) if isinstance(cid, str) else cid


def abi_samples(cid):
    """(y, g) of the C-ABI runs: S_ABI seeded samples of a case, a given problem's own"""
    return samples(cid, S_ABI) if isinstance(cid, str) else (cid["ys"], cid["g"])


def _abi_common(cid, dirty):
    from lvae_amd import _lib as P
    c = as_problem(cid)
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    p0, p1, nz, _ = D.positive(c)
    t = dict(padded_inputs(cid, dirty), z=c["Z"], p0=p0, p1=p1, noise=nz)
    d = {k: v.to(DEV).contiguous() for k, v in t.items()}
    d["seg"] = torch.tensor(c["seg"], dtype=torch.int32, device=DEV)
    return c, s0, s1, d


def _finish(o, n, shapes):
    for k in o:
        assert U.all_sentinel(o[k][n[k]:]), k
    return {k: o[k][:n[k]].reshape(shapes[k]).cpu() for k in o}


def abi_dubo(hip, cid, dirty, seg=True):
    """lvae_dubo_fwd_seg_f64, lvae_dubo_bwd_seg_f64 and lvae_dubo_bwd_z_f64 on sentinel-tailed buffers; the logical
    outputs (CPU), info included"""
    from lvae_amd import _lib as P
    c, s0, s1, d = _abi_common(cid, dirty)
    NP, Q = c["P"] * c["T"], c["X"].shape[1]
    dims = P.DuboDims(L, c["M"], c["P"], c["T"], Q, c.get("eps", EPS))
    n = dict(dubo=L, dmu=NP * L, dlogv=NP * L, dp0=L * s0.n_params, dp1=L * s1.n_params, dnoise=L)
    o = {k: U.sentinel(v + TAIL) for k, v in n.items()}
    info = U.sentinel(L + TAIL, torch.int32)
    ws, tail = U.workspace(hip.lvae_dubo_workspace_size(ctypes.byref(dims)))
    g = torch.as_tensor(COT, dtype=torch.float64).to(DEV)
    st = P.stream_ptr()
    common = (ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), P.ptr(d["seg"]) if seg else None, P.ptr(d["x"]),
              P.ptr(d["z"]), P.ptr(d["mu"]), P.ptr(d["lv"]), P.ptr(d["p0"]), P.ptr(d["p1"]), P.ptr(d["noise"]))
    rc = hip.lvae_dubo_fwd_seg_f64(*common, P.ptr(o["dubo"]), P.ptr(info), P.ptr(ws), st)
    torch.cuda.synchronize()
    assert rc == 0 and U.tail_untouched(tail)
    rc = hip.lvae_dubo_bwd_seg_f64(*common, P.ptr(g), P.ptr(o["dmu"]), P.ptr(o["dlogv"]), P.ptr(o["dp0"]),
                                   P.ptr(o["dp1"]), P.ptr(o["dnoise"]), P.ptr(ws), st)
    torch.cuda.synchronize()
    assert rc == 0 and U.tail_untouched(tail)
    dz, nz, zws, ztail = Z.dz_buffers(hip, L, c["M"], NP, Q)
    rc = hip.lvae_dubo_bwd_z_f64(ctypes.byref(s0), ctypes.byref(dims), P.ptr(d["x"]), P.ptr(d["z"]), P.ptr(d["p0"]),
                                 P.ptr(dz), P.ptr(ws), P.ptr(zws), st)
    torch.cuda.synchronize()
    assert rc == 0 and U.tail_untouched(tail) and U.tail_untouched(ztail)
    o["dz"], n["dz"] = dz, nz
    shapes = dict(dubo=(L,), dmu=(NP, L), dlogv=(NP, L), dp0=(L, s0.n_params), dp1=(L, s1.n_params), dnoise=(L,),
                  dz=(L, c["M"], Q))
    out = _finish(o, n, shapes)
    assert U.all_sentinel(info[L:])
    out["info"] = info[:L].cpu()
    return out


def abi_elbo(hip, cid, dirty, seg=True):
    """the same for lvae_gp_elbo_fwd_seg_f64, lvae_gp_elbo_bwd_seg_f64 and lvae_gp_elbo_bwd_z_f64 (S_ABI samples)"""
    from lvae_amd import _lib as P
    c, s0, s1, d = _abi_common(cid, dirty)
    ys, gs = abi_samples(cid)
    S, NP, Q = ys.shape[0], c["P"] * c["T"], c["X"].shape[1]
    dims = P.GpElboDims(L, c["M"], c["P"], c["T"], Q, S, c.get("eps", EPS))
    n = dict(elbo=S * L, dy=S * NP * L, dp0=L * s0.n_params, dp1=L * s1.n_params, dnoise=L)
    o = {k: U.sentinel(v + TAIL) for k, v in n.items()}
    info = U.sentinel(L + TAIL, torch.int32)
    ws, tail = U.workspace(hip.lvae_gp_elbo_workspace_size(ctypes.byref(dims)))
    g = gs.contiguous().to(DEV)
    st = P.stream_ptr()
    common = (ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), P.ptr(d["seg"]) if seg else None, P.ptr(d["x"]),
              P.ptr(d["z"]), P.ptr(d["y"]), P.ptr(d["p0"]), P.ptr(d["p1"]), P.ptr(d["noise"]))
    rc = hip.lvae_gp_elbo_fwd_seg_f64(*common, P.ptr(o["elbo"]), P.ptr(info), P.ptr(ws), st)
    torch.cuda.synchronize()
    assert rc == 0 and U.tail_untouched(tail)
    rc = hip.lvae_gp_elbo_bwd_seg_f64(*common, P.ptr(g), P.ptr(o["dy"]), P.ptr(o["dp0"]), P.ptr(o["dp1"]),
                                      P.ptr(o["dnoise"]), P.ptr(ws), st)
    torch.cuda.synchronize()
    assert rc == 0 and U.tail_untouched(tail)
    dz, nz, zws, ztail = Z.dz_buffers(hip, L, c["M"], NP, Q)
    rc = hip.lvae_gp_elbo_bwd_z_f64(ctypes.byref(s0), ctypes.byref(dims), P.ptr(d["x"]), P.ptr(d["z"]),
                                    P.ptr(d["p0"]), P.ptr(dz), P.ptr(ws), P.ptr(zws), st)
    torch.cuda.synchronize()
    assert rc == 0 and U.tail_untouched(tail) and U.tail_untouched(ztail)
    o["dz"], n["dz"] = dz, nz
    shapes = dict(elbo=(S, L), dy=(S, NP, L), dp0=(L, s0.n_params), dp1=(L, s1.n_params), dnoise=(L,),
                  dz=(L, c["M"], Q))
    out = _finish(o, n, shapes)
    assert U.all_sentinel(info[L:])
    out["info"] = info[:L].cpu()
    return out
