"""lvae_predict_exact_var_f64 and lvae_predict_var_f64 through the C ABI, at the smallest shapes where their kernels
can go wrong, against the dense fp64 oracle and the cases of test_predict_var_oracle.py.

Exact: n in {1, 63, 65, 130} (across the 64-row blocks of potrf / trsm), nt in {0, 1, 17, 70} (across the 64-column
blocks of the solve and of the variance kernel), chunks in {1, 16, nt}, L in {1, 3}, both template buckets;
non-unit ldx / ldt / ld_mu / ld_out / ld_var on sentinel buffers.  Inducing-point: M in {1, 20, 128}, T in
{1, 5, 20} with ragged seg_len, Nt in {1, 37}, a subject with 70 test rows (five 16-column tiles, the last partial),
test subjects absent from the prediction set (some, and all), L in {1, 3}; ext_util's ext-b pair (periodic and
linear factors in both kernels, a (16, 4) id kernel) on the ragged layout: err 3.98e-15 against a yardstick of 2.40e-15.

Tolerance: the project's rule min(max(10 x yardstick, 2e-12), 1e-6) on max |got - ref| / max prior, the yardstick
being the larger of the oracle's change under a relative 2^-50 perturbation of its inputs and its CPU / device
spread.  The oracle's yardsticks are 1e-16 .. 4e-15 on the CPU (test_cases_are_well_posed), so the 2e-12 floor sets
the bound unless the device spread is larger.  The means returned alongside are compared bit for bit with
lvae_predict_exact_f64 / lvae_predict_f64.
"""
import ctypes

import numpy as np
import pytest
import torch

import abi_util as U
import test_predict_var_oracle as V
from oracle import lvae_oracle as O

gpu = pytest.mark.gpu
DEV = U.DEV


def bound(kind, cid, ref):
    """(tolerance, yardstick) of the rule for a case, given its CPU reference"""
    (_, var, prior), ya = V.cpu_ref(kind, cid)
    fn = V.exact_oracle if kind == "exact" else V.ind_oracle
    yard = max(ya, V.var_err(fn(cid, DEV)[1], var, prior))
    return min(max(10.0 * yard, 2e-12), 1e-6), yard


# ------------------------------------------------------------------------------------------------------
# exact
# ------------------------------------------------------------------------------------------------------
def run_exact(hip, cid, chunk, pad=3, noise=None, add_noise=0, want_mean=True):
    """One lvae_predict_exact_var_f64 call on sentinel-filled buffers, every leading dimension padded by `pad`;
    returns (mean [nt, L] or None, var [nt, L], info list)"""
    from lvae_amd import _lib as P
    c = V.exact_problem(cid)
    L, n, nt = c["L"], c["n"], c["nt"]
    spec = P.make_spec(c["spec"])
    dv = lambda t: t.to(DEV).contiguous()
    ldx = U.QC + pad
    xb, _ = U.padded(c["x"], (ldx, 1))
    tb, _ = U.padded(c["tx"], (ldx, 1)) if nt else (None, None)
    mb, _ = U.padded(c["mu"], (L + pad, 1))
    params, nz = dv(c["params"]), dv(c["noise"] if noise is None else noise)
    ld_out, ld_var = L + pad, L + pad + 1
    out, var = U.sentinel(max(nt, 1) * ld_out + 7), U.sentinel(max(nt, 1) * ld_var + 7)
    info = U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_exact_var_workspace_size(n, nt, L, chunk))
    rc = hip.lvae_predict_exact_var_f64(ctypes.byref(spec), P.ptr(xb), ldx, n, L, P.ptr(params), P.ptr(nz),
                                        P.ptr(mb) if want_mean else None, L + pad, P.ptr(tb) if nt else None, ldx, nt,
                                        P.ptr(out) if want_mean else None, ld_out, P.ptr(var), ld_var, add_noise,
                                        chunk, P.ptr(info), P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)                                     # the workspace size is enough
    assert U.untouched_outside(var, (nt, L), (ld_var, 1))
    assert U.untouched_outside(out, (nt, L), (ld_out, 1)) if want_mean else U.all_sentinel(out)
    mean = U.view(out, (nt, L), (ld_out, 1)).cpu() if want_mean else None
    return mean, U.view(var, (nt, L), (ld_var, 1)).cpu(), info.cpu().tolist()


def exact_mean_only(hip, cid):
    """lvae_predict_exact_f64 on the same inputs: [nt, L]"""
    from lvae_amd import _lib as P
    c = V.exact_problem(cid)
    L, n, nt = c["L"], c["n"], c["nt"]
    spec = P.make_spec(c["spec"])
    dv = lambda t: t.to(DEV).contiguous()
    x, tx, mu, params, nz = dv(c["x"]), dv(c["tx"]), dv(c["mu"]), dv(c["params"]), dv(c["noise"])
    out, info = torch.empty(nt, L, dtype=torch.float64, device=DEV), torch.empty(L, dtype=torch.int32, device=DEV)
    ws, _ = U.workspace(hip.lvae_predict_exact_workspace_size(n, nt, L))
    rc = hip.lvae_predict_exact_f64(ctypes.byref(spec), P.ptr(x), U.QC, n, L, P.ptr(params), P.ptr(nz), P.ptr(mu), L,
                                    P.ptr(tx), U.QC, nt, P.ptr(out), L, P.ptr(info), P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return out.cpu()


@gpu
@pytest.mark.parametrize("cid", list(V.EXACT_CASES))
def test_exact_var_values(hip, cid):
    c = V.exact_problem(cid)
    runs = [run_exact(hip, cid, ch) for ch in c["chunks"]]
    mean, var, info = runs[0]
    assert info == [0] * c["L"]
    for m2, v2, i2 in runs[1:]:
        assert U.bit_equal(v2, var) and U.bit_equal(m2, mean) and i2 == info   # the chunk changes no bit
    m3, v3, _ = run_exact(hip, cid, c["chunks"][-1], pad=0)
    assert U.bit_equal(v3, var) and U.bit_equal(m3, mean)            # a second run, other strides: the same bits
    none, v4, _ = run_exact(hip, cid, c["chunks"][-1], want_mean=False)
    assert none is None and U.bit_equal(v4, var)                     # without the mean (mu NULL too)
    if c["nt"] == 0:
        assert var.numel() == 0                                      # rc 0, info written, nothing else touched
        return
    assert U.bit_equal(mean, exact_mean_only(hip, cid))              # the mean is lvae_predict_exact_f64's
    (_, ref, prior), _ = V.cpu_ref("exact", cid)
    tol, yard = bound("exact", cid, ref)
    err = V.var_err(var, ref, prior)
    print(f"exact var {cid}: err {err:.2e} yardstick {yard:.2e} bound {tol:.1e} min var {float(var.min()):.3e}")
    assert bool(torch.isfinite(var).all()) and err <= tol
    _, vn, _ = run_exact(hip, cid, c["chunks"][-1], add_noise=1)
    ulp = float(np.spacing(float(prior.max())))
    assert float((vn - (var + c["noise"][None, :])).abs().max()) <= ulp   # + noise_l, to 1 ulp of the prior


@gpu
def test_exact_var_info_codes(hip):
    """A dim whose noise is below -(K's diagonal) is indefinite: info[l] = 1 for that dim only, and the other dims'
    variances and means keep their bits."""
    c = V.exact_problem("n130")
    mean, var, info = run_exact(hip, "n130", 16)
    assert info == [0, 0, 0]
    diag_max = float(O.gram(c["spec"], c["params"], c["x"], c["x"]).diagonal(dim1=-2, dim2=-1).max())
    bad = c["noise"].clone()
    bad[1] = -(diag_max + 1.0)
    m2, v2, info = run_exact(hip, "n130", 16, noise=bad)
    assert info[0] == 0 and info[2] == 0 and info[1] == 1
    assert U.bit_equal(v2[:, [0, 2]], var[:, [0, 2]]) and U.bit_equal(m2[:, [0, 2]], mean[:, [0, 2]])


@gpu
def test_exact_var_return_codes(hip):
    """Every documented bad-argument code, each rejected before any launch: nothing is written."""
    from lvae_amd import _lib as P
    c = V.exact_problem("n63")
    L, n, nt = c["L"], c["n"], c["nt"]
    good = P.make_spec(c["spec"])
    bad = P.KernelSpec.from_buffer_copy(good)
    bad.n_comp = 17
    dv = lambda t: t.to(DEV).contiguous()
    x, tx, mu, params, nz = dv(c["x"]), dv(c["tx"]), dv(c["mu"]), dv(c["params"]), dv(c["noise"])
    out, var, info = U.sentinel(nt * L), U.sentinel(nt * L), U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_exact_var_workspace_size(n, nt, L, 16))
    r = ctypes.byref

    def call(**kw):
        a = dict(spec=r(good), x=P.ptr(x), ldx=U.QC, n=n, L=L, params=P.ptr(params), noise=P.ptr(nz), mu=P.ptr(mu),
                 ld_mu=L, tx=P.ptr(tx), ldt=U.QC, nt=nt, out=P.ptr(out), ld_out=L, var=P.ptr(var), ld_var=L,
                 add_noise=0, chunk=16, info=P.ptr(info), ws=ws.data_ptr())
        a.update(kw)
        rc = hip.lvae_predict_exact_var_f64(a["spec"], a["x"], a["ldx"], a["n"], a["L"], a["params"], a["noise"],
                                            a["mu"], a["ld_mu"], a["tx"], a["ldt"], a["nt"], a["out"], a["ld_out"],
                                            a["var"], a["ld_var"], a["add_noise"], a["chunk"], a["info"], a["ws"],
                                            P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    ld_need = 1 + max(d for comp in c["spec"] for _, d in comp)
    codes = [(dict(spec=None), -1), (dict(spec=r(bad)), -1), (dict(x=None), -2), (dict(ldx=ld_need - 1), -3),
             (dict(n=0), -4), (dict(L=0), -5), (dict(params=None), -6), (dict(noise=None), -7), (dict(mu=None), -8),
             (dict(ld_mu=L - 1), -9), (dict(tx=None), -10), (dict(ldt=ld_need - 1), -11), (dict(nt=-1), -12),
             (dict(ld_out=L - 1), -14), (dict(info=None), -15), (dict(ws=None), -16),
             (dict(ws=ws.data_ptr() + 8), -16), (dict(var=None), -17), (dict(ld_var=L - 1), -18),
             (dict(add_noise=2), -19), (dict(add_noise=-1), -19), (dict(chunk=0), -20)]
    for kw, want in codes:
        assert call(**kw) == want, kw
    assert U.all_sentinel(out) and U.all_sentinel(var) and U.all_sentinel(info) and bool((ws == 0x7F).all())
    size = hip.lvae_predict_exact_var_workspace_size
    assert size(0, nt, L, 16) == 0 and size(n, -1, L, 16) == 0 and size(n, nt, 0, 16) == 0 and size(n, nt, L, 0) == 0
    base = hip.lvae_predict_exact_workspace_size(n, nt, L)
    assert size(n, nt, L, 1) - base >= 8 * L * n and size(n, nt, L, 16) - base >= 8 * L * n * 16
    assert size(n, nt, L, nt) == size(n, nt, L, nt + 100)            # a chunk beyond nt is nt
    assert call() == 0 and not U.all_sentinel(var) and U.tail_untouched(tail)   # (nothing wrong: it runs)


# ------------------------------------------------------------------------------------------------------
# inducing-point
# ------------------------------------------------------------------------------------------------------
def ind_args(cid, fill_seed=1):
    """Device tensors of a case in the ABI's layout: padded x, test rows grouped by subject"""
    c = V.ind_problem(cid)
    other = U.subject_covariates(np.random.default_rng(fill_seed), c["P"], c["T"]).reshape(c["NP"], U.QC)
    x = torch.where(c["valid"][:, None], c["x"], other)   # padding rows of x: any finite covariates
    dv = lambda t: t.to(DEV).contiguous()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    return dict(x=dv(x), z=dv(c["z"]), mu=dv(c["mu_pad"]), tx=dv(c["tx"][c["order"]]), p0=dv(c["p0"]), p1=dv(c["p1"]),
                noise=dv(c["noise"]), seg=i32(c["seg"]), inc=dv(c["include"]), gsub=i32(c["group_subject"]),
                gstart=i32(c["group_start"]))


def run_ind(hip, cid, fill_seed=1, add_noise=0, want_mean=True):
    """One lvae_predict_var_f64 call; returns (mean or None, var) [Nt, L] in the caller's row order, on the CPU"""
    from lvae_amd import _lib as P
    c = V.ind_problem(cid)
    L, M, Pn, T, Nt = c["L"], c["M"], c["P"], c["T"], c["Nt"]
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    a = ind_args(cid, fill_seed)
    out, var = U.sentinel(max(Nt, 1) * L + 7), U.sentinel(max(Nt, 1) * L + 7)
    info = U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_var_workspace_size(L, M, Pn, T, Nt))
    rc = hip.lvae_predict_var_f64(ctypes.byref(s0), ctypes.byref(s1), L, M, U.QC, Pn, T, P.ptr(a["seg"]), P.ptr(a["inc"]),
                                  P.ptr(a["x"]), P.ptr(a["mu"]) if want_mean else None, P.ptr(a["z"]), Nt,
                                  P.ptr(a["tx"]) if Nt else None, len(c["group_subject"]), P.ptr(a["gsub"]),
                                  P.ptr(a["gstart"]), P.ptr(a["p0"]), P.ptr(a["p1"]), P.ptr(a["noise"]), V.EPS,
                                  P.ptr(out) if want_mean else None, P.ptr(var), add_noise, P.ptr(info), P.ptr(ws),
                                  P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)
    assert U.all_sentinel(var[Nt * L:]) and U.all_sentinel(out[Nt * L:] if want_mean else out)
    assert info.cpu().tolist() == [0] * L
    back = torch.empty(Nt, dtype=torch.int64)
    back[c["order"]] = torch.arange(Nt)                             # caller row i sits at grouped row back[i]
    mean = out[:Nt * L].reshape(Nt, L).cpu()[back] if want_mean else None
    return mean, var[:Nt * L].reshape(Nt, L).cpu()[back]


def ind_mean_only(hip, cid):
    """lvae_predict_f64 on the same inputs (test rows in the caller's order): [Nt, L]"""
    from lvae_amd import _lib as P
    c = V.ind_problem(cid)
    L, M, Pn, T, Nt = c["L"], c["M"], c["P"], c["T"], c["Nt"]
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    a = ind_args(cid)
    tx = c["tx"].to(DEV).contiguous()
    out = torch.empty(Nt, L, dtype=torch.float64, device=DEV)
    ws, _ = U.workspace(hip.lvae_predict_workspace_size(L, M, Pn, T, Nt))
    rc = hip.lvae_predict_f64(ctypes.byref(s0), ctypes.byref(s1), L, M, U.QC, Pn, T, P.ptr(a["seg"]), P.ptr(a["inc"]),
                              P.ptr(a["x"]), P.ptr(a["mu"]), P.ptr(a["z"]), Nt, P.ptr(tx), P.ptr(a["p0"]), P.ptr(a["p1"]),
                              P.ptr(a["noise"]), V.EPS, P.ptr(out), None, P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return out.cpu()


@gpu
@pytest.mark.parametrize("cid", list(V.IND_CASES))
def test_inducing_var_values(hip, cid):
    c = V.ind_problem(cid)
    mean, var = run_ind(hip, cid)
    m2, v2 = run_ind(hip, cid, fill_seed=2)
    assert U.bit_equal(v2, var) and U.bit_equal(m2, mean)            # another fill of x's padding rows: the same bits
    none, v3 = run_ind(hip, cid, want_mean=False)
    assert none is None and U.bit_equal(v3, var)                     # without the mean (mu NULL too)
    if c["Nt"] == 0:
        assert var.numel() == 0                                      # rc 0, info written, outputs untouched
        return
    assert U.bit_equal(mean, ind_mean_only(hip, cid))                # the mean is lvae_predict_f64's
    (_, ref, prior), _ = V.cpu_ref("ind", cid)
    tol, yard = bound("ind", cid, ref)
    err = V.var_err(var, ref, prior)
    print(f"inducing var {cid}: err {err:.2e} yardstick {yard:.2e} bound {tol:.1e} min var {float(var.min()):.3e}")
    assert bool(torch.isfinite(var).all()) and err <= tol
    _, vn = run_ind(hip, cid, add_noise=1)
    ulp = float(np.spacing(float(prior.max())))
    assert float((vn - (var + c["noise"][None, :])).abs().max()) <= ulp   # + noise_l, to 1 ulp of the prior


def info_call(hip, eps, noise, Nt=4):
    """lvae_predict_var_f64 on abi_util.info_problem; returns (info list, var [Nt, L])"""
    from lvae_amd import _lib as P
    c = U.info_problem()
    L, M, T, Pn = c["L"], c["M"], c["T"], c["P_b"]
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    dv = lambda t: t.to(DEV).contiguous()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    x, z, p0, p1, nz = dv(c["x"]), dv(c["z"]), dv(c["p0"]), dv(c["p1"]), dv(noise)
    tx = dv(c["x"][:Nt])                                             # rows of subject 0, then of subject 1
    gsub, gstart = i32([0, 1]), i32([0, min(T, Nt), Nt])
    mu = torch.ones(Pn * T, L, dtype=torch.float64, device=DEV)
    seg, inc = i32([T, T]), i32([1, 1])
    out, var, info = U.sentinel(Nt * L), U.sentinel(Nt * L), U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_var_workspace_size(L, M, Pn, T, Nt))
    rc = hip.lvae_predict_var_f64(ctypes.byref(s0), ctypes.byref(s1), L, M, U.QC, Pn, T, P.ptr(seg), P.ptr(inc), P.ptr(x),
                                  P.ptr(mu), P.ptr(z), Nt, P.ptr(tx), 2, P.ptr(gsub), P.ptr(gstart), P.ptr(p0), P.ptr(p1),
                                  P.ptr(nz), eps, P.ptr(out), P.ptr(var), 0, P.ptr(info), P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and U.tail_untouched(tail)
    return info.cpu().tolist(), var.reshape(Nt, L).cpu()


@gpu
def test_inducing_var_info_codes(hip):
    """info as lvae_predict_f64's (10000 / 20000 + the failing column of K0zz / B_p); dim 1 only is indefinite by
    construction, and the other dims' variances keep their bits."""
    good = torch.ones(3, dtype=torch.float64)
    bad = good.clone()
    bad[1] = -(2 * 0.5 + 1.0)   # B_p[1] has the diagonal 1 - 2
    info, var = info_call(hip, V.EPS, good)
    assert info == [0, 0, 0] and bool(torch.isfinite(var).all())
    info, v2 = info_call(hip, V.EPS, bad)
    assert info == [0, 20001, 0] and U.bit_equal(v2[:, [0, 2]], var[:, [0, 2]])
    info, v3 = info_call(hip, -3.0, good)                            # K0zz[1] = 1.5 I - 3 I (dims 0, 2: 6 I - 3 I)
    assert info == [0, 10001, 0] and bool(torch.isfinite(v3[:, [0, 2]]).all())


@gpu
def test_inducing_var_return_codes(hip):
    """Every code lvae_predict_var_f64 returns for a bad argument, each rejected before any launch."""
    from lvae_amd import _lib as P
    cid = "ragged"
    c = V.ind_problem(cid)
    L, M, Pn, T, Nt = c["L"], c["M"], c["P"], c["T"], c["Nt"]
    good0, good1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    bad = P.KernelSpec.from_buffer_copy(good0)
    bad.n_comp = 17
    t = ind_args(cid)
    out, var, info = U.sentinel(Nt * L), U.sentinel(Nt * L), U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_var_workspace_size(L, M, Pn, T, Nt))
    r = ctypes.byref

    def call(**kw):
        a = dict(s0=r(good0), s1=r(good1), L=L, M=M, Q=U.QC, P=Pn, T=T, seg=P.ptr(t["seg"]), inc=P.ptr(t["inc"]),
                 x=P.ptr(t["x"]), mu=P.ptr(t["mu"]), z=P.ptr(t["z"]), Nt=Nt, tx=P.ptr(t["tx"]),
                 G=len(c["group_subject"]), gsub=P.ptr(t["gsub"]), gstart=P.ptr(t["gstart"]), p0=P.ptr(t["p0"]),
                 p1=P.ptr(t["p1"]), noise=P.ptr(t["noise"]), out=P.ptr(out), var=P.ptr(var), add_noise=0,
                 ws=ws.data_ptr())
        a.update(kw)
        rc = hip.lvae_predict_var_f64(a["s0"], a["s1"], a["L"], a["M"], a["Q"], a["P"], a["T"], a["seg"], a["inc"],
                                      a["x"], a["mu"], a["z"], a["Nt"], a["tx"], a["G"], a["gsub"], a["gstart"],
                                      a["p0"], a["p1"], a["noise"], V.EPS, a["out"], a["var"], a["add_noise"],
                                      P.ptr(info), a["ws"], P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    codes = [(dict(s0=None), -1), (dict(s1=None), -1), (dict(s0=r(bad)), -1), (dict(s1=r(bad)), -1),
             (dict(L=0), -3), (dict(M=0), -3), (dict(M=129), -3),
             (dict(P=0), -6), (dict(T=0), -6), (dict(T=129), -6), (dict(Q=0), -6),
             (dict(seg=None), -8), (dict(inc=None), -8), (dict(mu=None), -9), (dict(x=None), -10), (dict(z=None), -10),
             (dict(p0=None), -11), (dict(p1=None), -11), (dict(noise=None), -11), (dict(tx=None), -12),
             (dict(Nt=-1), -13), (dict(G=-1), -14), (dict(gsub=None), -15), (dict(gstart=None), -15),
             (dict(var=None), -16), (dict(add_noise=2), -17), (dict(ws=None), -20), (dict(ws=ws.data_ptr() + 8), -20),
             (dict(ws=ws.data_ptr() + 128), -20)]
    for kw, want in codes:
        assert call(**kw) == want, kw
    assert U.all_sentinel(out) and U.all_sentinel(var) and U.all_sentinel(info) and bool((ws == 0x7F).all())
    extra = hip.lvae_predict_var_workspace_size(L, M, Pn, T, Nt) - hip.lvae_predict_workspace_size(L, M, Pn, T, Nt)
    assert extra >= 8 * L * ((2 * T + 6 * M) * Nt + M * M)
    assert call() == 0 and not U.all_sentinel(var) and U.tail_untouched(tail)   # (nothing wrong: it runs)
