"""Shared inputs, yardsticks and runners of the conditioned-DUBO tests (test_dubo_cond_cpu.py, test_gpu_dubo_cond.py,
test_gpu_dubo_cond_abi.py): lvae_dubo_cond_prepare_f64 / lvae_dubo_cond_eval_f64 and condition_dubo over them.

Problems are dubo_util's recipe and cases (plus 12x32x17, whose 9 free subjects give Nn = 288 rows: past one
256-row workgroup of the eval), each with a set of free subjects.  The yardstick is oracle.lvae_oracle's joint
deviance_upper_bound per dim under CPU autograd, the free rows of (mu, logv) replaced by the point and
differentiated alone.  ``closed_form`` restates the identity the kernels implement from O._gpapprox_common's pieces:

    dubo(m, l) = c + 1/2 (m^T A m - 2 r^T m + sum_i a_i e^{l_i} - sum_i l_i)
    G = iBK[free rows]   U = G iW   A = blockdiag(iB_p : p free) - U G^T   a = diag(A)
    r = U sum_{p fixed} iBK_p^T m_p          c = dubo(joint, m_free = 0, l_free = 0) - 1/2 sum_i a_i

Bounds: dubo_util.BOUND with abi_util.rel (value 1e-8, dm / dlogv 1e-7), the project's own for the DUBO."""
import ctypes
import functools

import numpy as np
import torch

import abi_util as U
import dubo_util as D
from oracle import lvae_oracle as O

DEV = D.DEV
L = D.L
EPS = D.EPS
BOUND = dict(dubo=D.BOUND["dubo"], dm=D.BOUND["dmu"], dlogv=D.BOUND["dlogv"])
# GPU cases that miss BOUND for the coinciding-inducing-rows reason dz_util documents would be held to 4 x their
# measured error here: {(case, point, quantity): 4 x measured}.  None was needed.
CASE_BOUND = {}
COT = (1.0, -0.5, 2.0)
NEW_CASES = {"12x32x17": (12, 32, 17, 0.8)}     # the last T of the fused pass, 9 free subjects: Nn = 288
# id: the free subjects
FREE = {
    "3x1x1": (0,),                     # Nn = 1
    "1x4x3": (0,),                     # every subject free: p_fixed = 0
    "5x3x9": (0, 1, 2, 3, 4),          # the same with several subjects
    "6x7x33": (1, 4),                  # scattered free subjects, odd sizes
    "9x16x120": (0, 1, 2),             # the workload's T and M, leading free subjects as in the reference
    "17x3x9": (16,),                   # the lone subject of the second group
    "35x2x5": tuple(range(17)),        # free subjects straddle a group boundary
    "3x33x17": (2,),                   # the batched-product route
    "2x128x128": (0, 1),               # Nn = 256 exactly: the largest single-workgroup eval
    "12x32x17": (0, 2, 3, 4, 6, 7, 8, 10, 11),   # Nn = 288: two workgroups and the sum launch
}
CPU_CASES = ["6x7x33", "9x16x120", "17x3x9", "3x33x17", "35x2x5", "5x3x9", "1x4x3"]
GPU_CASES = ["3x1x1", "1x4x3", "6x7x33", "9x16x120", "17x3x9", "35x2x5", "3x33x17", "2x128x128", "12x32x17"]
POINTS = ["zero", "own", "far"]
TAIL = D.TAIL


def case_dims(cid):
    return D.CASES[cid] if cid in D.CASES else NEW_CASES[cid]


@functools.lru_cache(maxsize=None)
def problem(cid):
    """dubo_util.problem, extended by the cases of NEW_CASES (the same recipe), with free = FREE[cid]"""
    if cid in D.CASES:
        c = dict(D.problem(cid))
    else:
        from lvae_amd.data import health_mnist_covariates
        P, T, M, nz0 = NEW_CASES[cid]
        seed = 400 + list(NEW_CASES).index(cid)
        rng = np.random.default_rng(seed)
        gen = torch.Generator().manual_seed(seed)
        N = P * T
        X = torch.tensor(health_mnist_covariates(P, T, seed=seed))
        s0, s1 = O.spec_split(**D.CFG, id_covariate=2)
        Z = torch.stack([X[np.sort(np.random.default_rng(seed + 17 * l).choice(N, M, replace=False))]
                         for l in range(L)])
        c = dict(cid=cid, P=P, T=T, M=M, N=N, X=X, Z=Z, s0=s0, s1=s1,
                 raw0=np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s0)))),
                 raw1=np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s1)))),
                 noise=nz0 * np.array([1.0, 1.25, 1.5]),
                 mu=torch.randn(N, L, generator=gen, dtype=torch.float64),
                 lv=0.1 * torch.randn(N, L, generator=gen, dtype=torch.float64))
    c["free"] = FREE[cid]
    c["rows"] = free_rows(c["free"], c["T"])
    c["Pn"], c["Nn"] = len(c["free"]), len(c["free"]) * c["T"]
    return c


def free_rows(free, T):
    return torch.cat([torch.arange(p * T, (p + 1) * T) for p in free])


def point(cid, name):
    """(m [Nn, L], logv [Nn, L], cotangents [L]) of a named point"""
    c = problem(cid)
    m, lv = c["mu"][c["rows"]], c["lv"][c["rows"]]
    ones = torch.ones(L, dtype=torch.float64)
    if name == "zero":
        return torch.zeros_like(m), torch.zeros_like(lv), ones
    if name == "own":
        return m.clone(), lv.clone(), ones
    return m + 3.0, lv - 3.0, torch.tensor(COT, dtype=torch.float64)


def hypers(c):
    return D.positive(c)[:3]


def oracle_at(c, m, lv, cot, x=None, mu=None, logv=None, rows=None, dubo_fn=None):
    """the joint DUBO per dim with the rows ``rows`` of (mu, logv) replaced by (m, lv): values [L] and the gradients
    of sum_l cot_l dubo_l with respect to (m, lv)"""
    p0, p1, nz = hypers(c)
    x = c["X"] if x is None else x
    mu = c["mu"] if mu is None else mu
    logv = c["lv"] if logv is None else logv
    rows = c["rows"] if rows is None else rows
    m, lv = m.clone().requires_grad_(), lv.clone().requires_grad_()
    mj, lj = mu.index_copy(0, rows, m), logv.index_copy(0, rows, lv)
    if dubo_fn is None:
        dubo_fn = lambda l: O.deviance_upper_bound(c["s0"], p0[l], c["s1"], p1[l], nz[l], x, mj[:, l], lj[:, l],
                                                   c["Z"][l], x.shape[0] // c["T"], c["T"], EPS)
    else:
        dubo_fn = functools.partial(dubo_fn, p0, p1, nz, x, mj, lj)
    vals = torch.stack([dubo_fn(l) for l in range(L)])
    gm, gl = torch.autograd.grad(vals, (m, lv), cot)
    return dict(dubo=vals.detach(), dm=gm, dlogv=gl)


@functools.lru_cache(maxsize=None)
def oracle(cid, name):
    return oracle_at(problem(cid), *point(cid, name))


@functools.lru_cache(maxsize=None)
def closed_form(cid):
    """(c [L], r [L, Nn], a [L, Nn], A [L, Nn, Nn]) on the CPU from O._gpapprox_common's pieces"""
    c = problem(cid)
    p0, p1, nz = hypers(c)
    P, T, M, free = c["P"], c["T"], c["M"], list(c["free"])
    fixed = [p for p in range(P) if p not in free]
    mu0, lv0 = c["mu"].clone(), c["lv"].clone()
    mu0[c["rows"]] = 0.0
    lv0[c["rows"]] = 0.0
    out = []
    for l in range(L):
        k = O._gpapprox_common(c["s0"], p0[l], c["s1"], p1[l], nz[l], c["X"], c["Z"][l], P, T, EPS)
        iW = torch.cholesky_solve(torch.eye(M, dtype=torch.float64), k["LW"])
        G = k["iBK"][free].reshape(-1, M)
        Um = G @ iW
        A = torch.block_diag(*k["iB"][free]) - Um @ G.T
        pf = sum((k["iBK"][p].T @ c["mu"][p * T:(p + 1) * T, l] for p in fixed), torch.zeros(M, dtype=torch.float64))
        a = torch.diagonal(A).clone()
        d0 = O.deviance_upper_bound(c["s0"], p0[l], c["s1"], p1[l], nz[l], c["X"], mu0[:, l], lv0[:, l], c["Z"][l], P,
                                    T, EPS)
        out.append((d0 - 0.5 * a.sum(), Um @ pf, a, A))
    return tuple(torch.stack([o[q] for o in out]) for q in range(4))


def closed_eval(cf, m, lv, cot):
    """value, dm, dlogv of the closed form at (m, lv) [Nn, L] with cotangents cot [L]"""
    c0, r, a, A = cf
    mt, lt = m.T, lv.T                                         # [L, Nn]
    y = torch.einsum("lij,lj->li", A, mt)
    val = c0 + 0.5 * ((mt * y).sum(1) - 2 * (r * mt).sum(1) + (a * torch.exp(lt)).sum(1) - lt.sum(1))
    return dict(dubo=val, dm=(cot[:, None] * (y - r)).T, dlogv=(0.5 * cot[:, None] * (a * torch.exp(lt) - 1.0)).T)


def check(got, ref, what, bound=None):
    """every quantity of ``got`` within its bound of ``ref`` (abi_util.rel); prints each figure before it asserts"""
    errs = {q: U.rel(torch.as_tensor(got[q]), ref[q]) for q in ("dubo", "dm", "dlogv")}
    print(what, {q: f"{e:.2e}" for q, e in errs.items()})
    for q, e in errs.items():
        b = (bound or {}).get(q, BOUND[q])
        assert e <= b, (what, q, e, b)


def bound_for(cid, name):
    return {q: CASE_BOUND.get((cid, name, q), BOUND[q]) for q in BOUND}


# ------------------------------------------------------------------------------------------------------
# the C ABI directly
# ------------------------------------------------------------------------------------------------------
def abi_inputs(cid, noise=None):
    """dubo_util.abi_inputs for every case of this module + the free set as a device int32 array"""
    from lvae_amd import _lib as P
    c = problem(cid) if isinstance(cid, str) else cid   # (or a problem given whole, with free / rows / Pn / Nn)
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    p0, p1, nz = hypers(c)
    t = dict(x=c["X"], z=c["Z"], mu=c["mu"], lv=c["lv"], p0=p0, p1=p1,
             noise=nz if noise is None else torch.tensor(noise, dtype=torch.float64))
    d = {k: v.to(DEV).contiguous() for k, v in t.items()}
    d["free"] = torch.tensor(c["free"], dtype=torch.int32, device=DEV)
    dims = P.DuboDims(L, c["M"], c["P"], c["T"], c["X"].shape[1], c.get("eps", EPS))
    return c, s0, s1, dims, d


def prepare(hip, cid, noise=None, seg=None, mu=None, lv=None, want_info=True):
    """lvae_dubo_cond_prepare_f64 on sentinel-tailed state and workspace; returns a dict with the state, the tails,
    info (or None) and the call's dims"""
    from lvae_amd import _lib as P
    c, s0, s1, dims, d = abi_inputs(cid, noise)
    if mu is not None:
        d["mu"], d["lv"] = mu.to(DEV).contiguous(), lv.to(DEV).contiguous()
    Pn, T = c["Pn"], c["T"]
    state, stail = U.workspace(hip.lvae_dubo_cond_state_size(L, Pn, T))
    ws, wtail = U.workspace(hip.lvae_dubo_workspace_size(ctypes.byref(dims)))
    info = U.sentinel(L + TAIL, torch.int32)
    segd = None if seg is None else torch.as_tensor(seg, dtype=torch.int32).to(DEV)
    rc = hip.lvae_dubo_cond_prepare_f64(ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), P.ptr(segd), Pn,
                                        P.ptr(d["free"]), P.ptr(d["x"]), P.ptr(d["z"]), P.ptr(d["mu"]), P.ptr(d["lv"]),
                                        P.ptr(d["p0"]), P.ptr(d["p1"]), P.ptr(d["noise"]), P.ptr(state),
                                        P.ptr(info) if want_info else None, P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(stail) and U.tail_untouched(wtail)
    assert U.all_sentinel(info[L:])
    return dict(c=c, state=state, ws=ws, info=info[:L].cpu() if want_info else None, Pn=Pn, T=T, Nn=c["Nn"],
                state_tail=stail, seg=segd)


def evaluate(hip, prep, m, lv, cot=None):
    """lvae_dubo_cond_eval_f64 on NaN-filled outputs, each with TAIL spare sentinels behind it (cot None: g = NULL);
    returns the logical CPU tensors"""
    from lvae_amd import _lib as P
    Nn = prep["Nn"]
    md, ld = m.to(DEV).contiguous(), lv.to(DEV).contiguous()
    g = None if cot is None else torch.as_tensor(cot, dtype=torch.float64).to(DEV)
    n = dict(dubo=L, dm=Nn * L, dlogv=Nn * L)
    o = {k: U.sentinel(v + TAIL) for k, v in n.items()}
    rc = hip.lvae_dubo_cond_eval_f64(L, prep["Pn"], prep["T"], P.ptr(prep["state"]), P.ptr(md), P.ptr(ld), P.ptr(g),
                                     P.ptr(o["dubo"]), P.ptr(o["dm"]), P.ptr(o["dlogv"]), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(prep["state_tail"])
    for k in o:
        assert U.all_sentinel(o[k][n[k]:]), k
    return dict(dubo=o["dubo"][:L].cpu(), dm=o["dm"][:Nn * L].reshape(Nn, L).cpu(),
                dlogv=o["dlogv"][:Nn * L].reshape(Nn, L).cpu())
