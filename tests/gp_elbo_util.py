"""Shared inputs and runners of the all-dims sampled GP ELBO tests (test_gpu_gp_elbo.py, test_gpu_gp_elbo_abi.py,
test_gpu_gp_elbo_drivers.py): dubo_util's problem per (P, T, M) case (L = 3, distinct per-dim raw parameters,
noises and inducing rows), S seeded samples y = mu + 0.3 randn [S, N, L] and seeded random cotangents [S, L]; the
fp64 oracle under CPU autograd (oracle.gpapprox_elbo per (s, l), computed once per (case, S)), lvae_amd.elbo_batched
through Python, the per-dim lvae_amd.elbo loop, and a raw C-ABI forward + backward on sentinel-filled outputs."""
import ctypes
import functools

import torch

import abi_util as U
import dubo_util as D
from oracle import lvae_oracle as O

DEV = D.DEV
L = D.L
EPS = D.EPS
# the issue's cases (dubo_util.CASES without its ABI-only 5x3x9)
CASE_IDS = ["1x4x3", "3x1x1", "6x7x33", "9x16x120", "4x32x17", "3x33x17", "2x128x128", "15x3x9", "16x3x9", "17x3x9",
            "35x2x5"]
QUANT = ["elbo", "dy", "draw0", "draw1", "dnoise"]
# dubo_util.BOUND: value 1e-8, the data gradient 1e-7, raw kernel and noise gradients 1e-6
BOUND = dict(elbo=D.BOUND["dubo"], dy=D.BOUND["dmu"], draw0=D.BOUND["draw0"], draw1=D.BOUND["draw1"],
             dnoise=D.BOUND["dnoise"])
rel = D.rel


def samples(cid, S):
    """y [S, N, L] = mu + 0.3 randn and the cotangents g [S, L], both seeded by (case, S); a problem given whole
    (dubo_util.as_problem) brings its own as ys / g"""
    if not isinstance(cid, str):
        assert cid["ys"].shape[0] == S
        return cid["ys"], cid["g"]
    return _samples(cid, S)


@functools.lru_cache(maxsize=None)
def _samples(cid, S):
    c = D.problem(cid)
    gen = torch.Generator().manual_seed(7000 + 100 * D.CASE_IDS.index(cid) + S)
    y = c["mu"][None] + 0.3 * torch.randn(S, c["N"], L, generator=gen, dtype=torch.float64)
    g = torch.randn(S, L, generator=gen, dtype=torch.float64)
    return y, g


def _collect(vals, y, k0, k1, lik):
    d0, d1, dn = D._raw_grads(k0, k1, lik)
    out = dict(elbo=vals, dy=y.grad, draw0=d0, draw1=d1, dnoise=dn)
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def run_batched(cid, S, form="batched", cot=None, y=None):
    """elbo_batched on the GPU with batched modules or per-dim lists on y [S, N, L] (default: samples(cid, S));
    gradients of sum_{s,l} cot[s][l] elbo[s][l] (default: the seeded cotangents)"""
    import lvae_amd as la
    c = D.problem(cid)
    ys, g = samples(cid, S)
    y = (ys if y is None else y).to(DEV).requires_grad_()
    g = g if cot is None else torch.as_tensor(cot, dtype=torch.float64)
    k0, k1, lik = D.modules_batched(c) if form == "batched" else D.modules_list(c)
    z = c["Z"].to(DEV) if form == "batched" else [zi.to(DEV) for zi in c["Z"]]
    vals = la.elbo_batched(L, k0, k1, lik, c["X"].to(DEV), y, z, c["P"], c["T"], EPS)
    assert vals.shape == tuple(y.shape[:-2]) + (L,) and vals.dtype == torch.float64
    vals.backward(g.reshape(vals.shape).to(DEV))
    return _collect(vals, y, k0, k1, lik)


@functools.lru_cache(maxsize=None)
def batched(cid, S):
    return run_batched(cid, S)


@functools.lru_cache(maxsize=None)
def oracle(cid, S):
    """oracle.lvae_oracle.gpapprox_elbo per (s, l) under CPU autograd with the seeded cotangents (the raw ->
    positive transforms are the package's own CPU formulas)"""
    import lvae_amd as la
    c = D.problem(cid)
    ys, g = samples(cid, S)
    k0, k1, lik = D.modules_batched(c, "cpu")
    _, p0 = la.kernel_spec_and_params(k0)
    _, p1 = la.kernel_spec_and_params(k1)
    nz = lik.noise
    y = ys.clone().requires_grad_()
    vals = torch.stack([torch.stack([O.gpapprox_elbo(c["s0"], p0[l], c["s1"], p1[l], nz[l], c["X"], y[s, :, l],
                                                     c["Z"][l], c["P"], c["T"], EPS) for l in range(L)])
                        for s in range(S)])
    vals.backward(g)
    return _collect(vals, y, k0, k1, lik)


@functools.lru_cache(maxsize=None)
def composed(cid, S):
    """the per-dim lvae_amd.elbo (torch composition over the HIP Grams and inverses), sample by sample, dim by dim"""
    import lvae_amd as la
    c = D.problem(cid)
    ys, g = samples(cid, S)
    k0, k1, lik = D.modules_list(c)
    y = ys.to(DEV).requires_grad_()
    X = c["X"].to(DEV)
    vals = torch.stack([torch.stack([la.elbo(k0[l], k1[l], lik[l], X, y[s, :, l], c["Z"][l].to(DEV), c["P"], c["T"],
                                             EPS) for l in range(L)]) for s in range(S)])
    vals.backward(g.to(DEV))
    return _collect(vals, y, k0, k1, lik)


def check(got, ref, bounds, what):
    errs = {k: rel(got[k], ref[k]) for k in QUANT}
    print(what, " ".join(f"{k} {errs[k]:.2e}" for k in QUANT))
    for k in QUANT:
        assert errs[k] < bounds[k], (what, k, errs[k])


# ------------------------------------------------------------------------------------------------------
# the C ABI directly
# ------------------------------------------------------------------------------------------------------
TAIL = 7


def make_dims(c, S, **kw):
    from lvae_amd import _lib as P
    f = dict(L=L, M=c["M"], P=c["P"], T=c["T"], Q=c["X"].shape[1], S=S)
    f.update(kw)
    return P.GpElboDims(f["L"], f["M"], f["P"], f["T"], f["Q"], f["S"], c.get("eps", EPS))


def abi_inputs(cid, S, noise=None):
    from lvae_amd import _lib as P
    c = D.as_problem(cid)
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    p0, p1, nz, _ = D.positive(c)
    t = dict(x=c["X"], z=c["Z"], y=samples(cid, S)[0], p0=p0, p1=p1,
             noise=nz if noise is None else torch.tensor(noise, dtype=torch.float64))
    d = {k: v.to(DEV).contiguous() for k, v in t.items()}
    return c, s0, s1, make_dims(c, S), d


def abi_sizes(c, s0, s1, S):
    return dict(elbo=S * L, dy=S * c["N"] * L, dp0=L * s0.n_params, dp1=L * s1.n_params, dnoise=L)


def abi_outputs(c, s0, s1, S):
    n = abi_sizes(c, s0, s1, S)
    return n, {k: U.sentinel(v + TAIL) for k, v in n.items()}


def abi_run(hip, cid, S, cot=None, noise=None, want_info=True, want_dnoise=True, bwd_calls=1):
    """Forward then backward (bwd_calls times, each on fresh NaN-filled outputs) on a sentinel-tailed workspace.
    Returns ([{name: logical CPU tensor}] per backward call, or the one dict for bwd_calls = 1; info or None;
    {name: whole buffer} of the last call; sizes)."""
    from lvae_amd import _lib as P
    c, s0, s1, dims, d = abi_inputs(cid, S, noise)
    n, o = abi_outputs(c, s0, s1, S)
    info = U.sentinel(L + TAIL, torch.int32)
    ws, tail = U.workspace(hip.lvae_gp_elbo_workspace_size(ctypes.byref(dims)))
    g = (samples(cid, S)[1] if cot is None else torch.as_tensor(cot, dtype=torch.float64)).reshape(S, L)
    g = g.contiguous().to(DEV)
    st = P.stream_ptr()
    common = (ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), P.ptr(d["x"]), P.ptr(d["z"]), P.ptr(d["y"]),
              P.ptr(d["p0"]), P.ptr(d["p1"]), P.ptr(d["noise"]))
    rc = hip.lvae_gp_elbo_fwd_f64(*common, P.ptr(o["elbo"]), P.ptr(info) if want_info else None, P.ptr(ws), st)
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)
    shapes = dict(elbo=(S, L), dy=(S, c["N"], L), dp0=(L, s0.n_params), dp1=(L, s1.n_params), dnoise=(L,))
    outs = []
    for call in range(bwd_calls):
        if call:
            for k in ("dy", "dp0", "dp1", "dnoise"):
                o[k] = U.sentinel(n[k] + TAIL)
        rc = hip.lvae_gp_elbo_bwd_f64(*common, P.ptr(g), P.ptr(o["dy"]), P.ptr(o["dp0"]), P.ptr(o["dp1"]),
                                      P.ptr(o["dnoise"]) if want_dnoise else None, P.ptr(ws), st)
        torch.cuda.synchronize()
        assert rc == 0
        assert U.tail_untouched(tail)
        outs.append({k: o[k][:n[k]].reshape(shapes[k]).cpu() for k in o})
    return (outs[0] if bwd_calls == 1 else outs), (info.cpu() if want_info else None), o, n
