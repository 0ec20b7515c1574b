"""The posterior covariance of the additive components end to end: lvae_predict_exact_comp_cov_f64 and
lvae_predict_comp_cov_f64 through the C ABI, and predict_exact_components / batch_predict_components with
return_cov=True, against the oracles of predict_ccov_util.py (the exact one from the Cholesky factor, the inducing
one dense: Sigma assembled whole over the prediction rows).

Per case: the blocks [L, Nt, R, R] against the oracle and their sums over (r, s) against the device's own
lvae_predict_exact_var_f64 / lvae_predict_var_f64, both by the project's rule min(max(10 x yardstick, 2e-12), 1e-6)
on max |got - ref| / max prior component variance, the yardstick being the larger of the oracle's change under a
relative 2^-50 perturbation of its inputs on the CPU and its CPU / device spread; blocks symmetric bit for bit; out,
out_comp and info the bits of lvae_predict_exact_comp_f64 / lvae_predict_comp_f64; sentinels after out_ccov and after
the workspace intact; Nt = 0 writes info only.  Exact route: the same bits for chunk in {1, 3, nt, nt + 5}.  Inducing
route: a row's block has the same bits when the call holds only that row's subject group.  A component whose
cross-covariance with the data vanishes (an id component at a subject outside the prediction set; every id component
in none-included) has exact zeros off the diagonal and its exact prior on it.

Exact cases: predict_comp_util.EXACT_IDS, r16 (16 components, bucket (16, 4)), r1 (one component), n513 (one row past a
512-row slab).  Inducing cases: predict_comp_util.IND_CASES and two-tiles (R = 17: a block spans two tiles).

Measured on the MI355X (err and yardstick relative to the largest prior component variance; |sum - var| is the
blocks' sum over (r, s) against the device's own variance call; every bound is the 2e-12 floor):
    case                    R    err        yardstick   |sum - var|
    exact smallest          5    3.26e-17   9.12e-16    2.61e-16
    exact tile-edge         5    5.13e-16   9.12e-16    1.60e-15
    exact mix1              9    7.98e-16   1.14e-15    3.65e-15
    exact ext               5    8.95e-16   8.95e-16    1.45e-15
    exact few-rows          5    3.37e-16   6.74e-16    1.69e-15
    exact ext-a             9    5.60e-16   1.23e-15    8.97e-16
    exact r16               16   2.30e-16   1.26e-15    1.15e-15
    exact r1                1    3.75e-16   8.74e-16    4.99e-16
    exact n513              5    9.55e-16   1.09e-15    1.50e-15
    inducing smallest       5    5.94e-17   5.35e-16    7.13e-16
    inducing m3-mixed       9    8.07e-16   2.62e-15    2.53e-15
    inducing m128-ragged    12   1.06e-13   1.68e-14    2.22e-13
    inducing none-included  9    2.31e-16   9.26e-16    9.26e-16
    inducing ref-ragged     5    7.23e-16   2.28e-15    1.78e-15
    inducing ext-a          9    2.56e-15   2.19e-15    8.81e-15
    inducing ext-c          13   6.77e-16   2.30e-15    3.64e-15
    inducing two-tiles      17   1.95e-16   9.09e-16    9.09e-16
    predict_exact_components (both forms)      5.88e-16   7.35e-16    8.83e-16
    batch_predict_components batched / list    6.07e-15 / 3.80e-15   1.71e-15   8.10e-15 / 5.19e-15
The module's 27 tests take about 5 s.
"""
import ctypes

import numpy as np
import pytest
import torch

import abi_util as U
import predict_ccov_util as CC
import predict_comp_util as C
import test_gpu_predict_comp as TC
from oracle import lvae_oracle as O

gpu = pytest.mark.gpu
DEV = U.DEV
TAIL = 37   # sentinels after out_ccov


# ------------------------------------------------------------------------------------------------------
# exact route
# ------------------------------------------------------------------------------------------------------
def run_exact(hip, cid, chunk, pad=3, noise=None, mean=True, comp=True):
    """One lvae_predict_exact_comp_cov_f64 call on sentinel buffers; (out [Nt, L] or None, out_comp [R, Nt, L] or
    None, ccov [L, Nt, R, R], info)"""
    from lvae_amd import _lib as P
    c = CC.exact_problem(cid)
    L, n, Nt, R = c["L"], c["n"], c["Nt"], len(c["spec"])
    spec = P.make_spec(c["spec"])
    dv = lambda t: t.to(DEV).contiguous()
    ldx = c["x"].shape[1] + pad
    xb, _ = U.padded(c["x"], (ldx, 1))
    tb, _ = U.padded(c["tx"], (ldx, 1)) if Nt else (None, None)
    mb, _ = U.padded(c["mu"], (L + pad, 1))
    params, nz = dv(c["params"]), dv(c["noise"] if noise is None else noise)
    ld_out, ld_comp = L + pad, L + pad + (1 if pad else 0)
    cs = max(Nt, 1) * ld_comp + 2 * pad
    out, cbuf = U.sentinel(max(Nt, 1) * ld_out + 7), U.sentinel(R * cs + 7)
    ccov = U.sentinel(L * Nt * R * R + TAIL)
    info = U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_exact_comp_cov_workspace_size(n, Nt, L, R, chunk))
    rc = hip.lvae_predict_exact_comp_cov_f64(ctypes.byref(spec), P.ptr(xb), ldx, n, L, P.ptr(params), P.ptr(nz),
                                             P.ptr(mb) if mean else None, L + pad, P.ptr(tb) if Nt else None, ldx, Nt,
                                             P.ptr(out) if mean else None, ld_out, P.ptr(cbuf) if comp else None,
                                             ld_comp, cs, chunk, P.ptr(ccov), P.ptr(info), P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)                                              # the workspace size is enough
    assert U.all_sentinel(ccov[L * Nt * R * R:])                               # nothing beyond L nt R R
    assert U.untouched_outside(out, (Nt, L), (ld_out, 1)) if mean else U.all_sentinel(out)
    assert U.untouched_outside(cbuf, (R, Nt, L), (cs, ld_comp, 1)) if mean and comp else U.all_sentinel(cbuf)
    o = U.view(out, (Nt, L), (ld_out, 1)).cpu() if mean and Nt else None
    k = U.view(cbuf, (R, Nt, L), (cs, ld_comp, 1)).cpu() if mean and comp and Nt else None
    return o, k, ccov[:L * Nt * R * R].reshape(L, Nt, R, R).cpu(), info.cpu().tolist()


def run_exact_comp(hip, cid, pad=3):
    """lvae_predict_exact_comp_f64 on the same buffers' layout: (out, out_comp, info)"""
    from lvae_amd import _lib as P
    c = CC.exact_problem(cid)
    L, n, Nt, R = c["L"], c["n"], c["Nt"], len(c["spec"])
    spec = P.make_spec(c["spec"])
    dv = lambda t: t.to(DEV).contiguous()
    x, tx, mu, params, nz = dv(c["x"]), dv(c["tx"]), dv(c["mu"]), dv(c["params"]), dv(c["noise"])
    out = torch.empty(Nt, L, dtype=torch.float64, device=DEV)
    comp = torch.empty(R, Nt, L, dtype=torch.float64, device=DEV)
    info = U.sentinel(L, torch.int32)
    ws, _ = U.workspace(hip.lvae_predict_exact_comp_workspace_size(n, Nt, L, R))
    rc = hip.lvae_predict_exact_comp_f64(ctypes.byref(spec), P.ptr(x), x.shape[1], n, L, P.ptr(params), P.ptr(nz),
                                         P.ptr(mu), L, P.ptr(tx) if Nt else None, x.shape[1], Nt,
                                         P.ptr(out) if Nt else None, L, P.ptr(comp) if Nt else None, L, Nt * L,
                                         P.ptr(info), P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return out.cpu(), comp.cpu(), info.cpu().tolist()


def exact_var(hip, cid):
    """lvae_predict_exact_var_f64 (add_noise = 0, no mean) on the same inputs: [Nt, L]"""
    from lvae_amd import _lib as P
    c = CC.exact_problem(cid)
    L, n, Nt = c["L"], c["n"], c["Nt"]
    spec = P.make_spec(c["spec"])
    dv = lambda t: t.to(DEV).contiguous()
    x, tx, params, nz = dv(c["x"]), dv(c["tx"]), dv(c["params"]), dv(c["noise"])
    var, info = torch.empty(Nt, L, dtype=torch.float64, device=DEV), torch.empty(L, dtype=torch.int32, device=DEV)
    ws, _ = U.workspace(hip.lvae_predict_exact_var_workspace_size(n, Nt, L, Nt))
    rc = hip.lvae_predict_exact_var_f64(ctypes.byref(spec), P.ptr(x), x.shape[1], n, L, P.ptr(params), P.ptr(nz), None,
                                        L, P.ptr(tx), x.shape[1], Nt, None, L, P.ptr(var), L, 0, Nt, P.ptr(info),
                                        P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return var.cpu()


def zero_rows_exact(c):
    """test rows of subjects outside the prediction set"""
    return ~torch.isin(c["tx"][:, U.ID_COL], torch.unique(c["x"][:, U.ID_COL]))


def id_comps(spec):
    return [r for r, comp in enumerate(spec) if ("cat", U.ID_COL) in comp]


def check_zero_components(cov, prior, rows, comps):
    """exact zeros off the diagonal and the exact prior on it, for the given test rows x components"""
    R = cov.shape[2]
    for r in comps:
        blk = cov[:, rows]                                                     # [L, rows, R, R]
        off = [s for s in range(R) if s != r]
        assert bool((blk[:, :, r, off] == 0.0).all()) and bool((blk[:, :, off, r] == 0.0).all())
        assert bool((blk[:, :, r, r] == prior[:, rows, r]).all())


@gpu
@pytest.mark.parametrize("cid", CC.EXACT_IDS)
def test_exact_comp_cov_abi(hip, cid):
    c = CC.exact_problem(cid)
    L, Nt, R = c["L"], c["Nt"], len(c["spec"])
    chunks = sorted({1, 3, max(Nt, 1), Nt + 5})
    runs = [run_exact(hip, cid, ch) for ch in chunks]
    out, comp, cov, info = runs[0]
    assert info == [0] * L
    for o2, k2, c2, i2 in runs[1:]:                                            # the chunk changes no bit
        assert U.bit_equal(c2, cov) and i2 == info
        assert (o2 is None and k2 is None) if Nt == 0 else (U.bit_equal(o2, out) and U.bit_equal(k2, comp))
    pout, pcomp, pinfo = run_exact_comp(hip, cid)
    assert pinfo == info
    if Nt == 0:
        assert cov.numel() == 0                                                # rc 0, info written, nothing else
        return
    assert U.bit_equal(out, pout) and U.bit_equal(comp, pcomp)                 # lvae_predict_exact_comp_f64's bits
    _, _, c3, _ = run_exact(hip, cid, chunks[-1], pad=0, mean=False, comp=False)
    assert U.bit_equal(c3, cov)                                                # without the means, other strides
    o4, k4, c4, _ = run_exact(hip, cid, 3, comp=False)
    assert U.bit_equal(c4, cov) and U.bit_equal(o4, out) and k4 is None
    assert U.bit_equal(cov, cov.transpose(2, 3))                               # symmetric bit for bit
    (ref, prior), ya = CC.exact_ref(cid)
    yard = max(ya, CC.ccov_err(CC.exact_oracle(cid, DEV)[0], ref, prior))
    err, tol = CC.ccov_err(cov, ref, prior), CC.bound(yard)
    var = exact_var(hip, cid)
    serr = float((cov.sum((2, 3)).T - var).abs().max() / float(prior.max()))
    print(f"exact comp cov {cid}: n {c['n']} nt {Nt} R {R} err {err:.2e} yardstick {yard:.2e} bound {tol:.1e}; "
          f"|sum_rs - var| {serr:.2e}")
    assert bool(torch.isfinite(cov).all())
    assert err <= tol
    assert serr <= tol
    absent = zero_rows_exact(c)
    if bool(absent.any()) and id_comps(c["spec"]):
        check_zero_components(cov, prior, absent, id_comps(c["spec"]))


@gpu
def test_exact_comp_cov_info(hip):
    """A dim whose noise makes K indefinite: info[l] > 0 for that dim only, the other dims' blocks keep their bits."""
    c = CC.exact_problem("mix1")
    _, _, good, info = run_exact(hip, "mix1", 16)
    assert info == [0, 0, 0]
    diag_max = float(O.gram(c["spec"], c["params"], c["x"], c["x"]).diagonal(dim1=-2, dim2=-1).max())
    bad = c["noise"].clone()
    bad[1] = -(diag_max + 1.0)
    _, _, got, info = run_exact(hip, "mix1", 16, noise=bad)
    assert info[0] == 0 and info[2] == 0 and info[1] == 1
    assert U.bit_equal(got[[0, 2]], good[[0, 2]])


@gpu
def test_exact_comp_cov_return_codes(hip):
    """Every documented bad-argument code in its documented order, each with only that argument bad and each
    rejected before any launch: nothing is written.  The size function gives 0 for rejected sizes."""
    from lvae_amd import _lib as P
    r = ctypes.byref
    dv = lambda t: t.to(DEV).contiguous()
    c = CC.exact_problem("tile-edge")
    L, n, Nt, R = c["L"], c["n"], c["Nt"], len(c["spec"])
    good = P.make_spec(c["spec"])
    far = P.KernelSpec.from_buffer_copy(good)
    far.dim[0][0] = 32
    none = P.KernelSpec.from_buffer_copy(good)
    none.n_comp = 0
    x, tx, mu, params, nz = dv(c["x"]), dv(c["tx"]), dv(c["mu"]), dv(c["params"]), dv(c["noise"])
    out, comp, info = U.sentinel(Nt * L), U.sentinel(R * Nt * L), U.sentinel(L, torch.int32)
    ccov = U.sentinel(L * Nt * R * R)
    ws, tail = U.workspace(hip.lvae_predict_exact_comp_cov_workspace_size(n, Nt, L, R, 16))

    def call(**kw):
        a = dict(spec=r(good), x=P.ptr(x), ldx=U.QC, n=n, L=L, params=P.ptr(params), noise=P.ptr(nz), mu=P.ptr(mu),
                 ld_mu=L, tx=P.ptr(tx), ldt=U.QC, nt=Nt, out=P.ptr(out), ld_out=L, comp=P.ptr(comp), ld_comp=L,
                 cs=Nt * L, chunk=16, ccov=P.ptr(ccov), info=P.ptr(info), ws=ws.data_ptr())
        a.update(kw)
        rc = hip.lvae_predict_exact_comp_cov_f64(a["spec"], a["x"], a["ldx"], a["n"], a["L"], a["params"], a["noise"],
                                                 a["mu"], a["ld_mu"], a["tx"], a["ldt"], a["nt"], a["out"],
                                                 a["ld_out"], a["comp"], a["ld_comp"], a["cs"], a["chunk"], a["ccov"],
                                                 a["info"], a["ws"], P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    ld_need = 1 + max(d for cp in c["spec"] for _, d in cp)
    codes = [(dict(spec=None), -1), (dict(spec=r(far)), -1), (dict(spec=r(none)), -1), (dict(x=None), -2),
             (dict(ldx=ld_need - 1), -3), (dict(n=0), -4), (dict(L=0), -5), (dict(L=65536), -5),
             (dict(params=None), -6), (dict(noise=None), -7), (dict(mu=None), -8), (dict(ld_mu=L - 1), -9),
             (dict(nt=-1), -12), (dict(tx=None), -10), (dict(ldt=ld_need - 1), -11), (dict(out=None), -13),
             (dict(ld_out=L - 1), -14), (dict(info=None), -15), (dict(ws=None), -16),
             (dict(ws=ws.data_ptr() + 8), -16), (dict(ld_comp=L - 1), -18), (dict(cs=Nt * L - 1), -19),
             (dict(chunk=0), -20), (dict(chunk=-3), -20), (dict(ccov=None), -21),
             # the documented order where two arguments are bad
             (dict(ccov=None, chunk=0), -20), (dict(chunk=0, cs=0), -19), (dict(cs=0, ld_comp=0), -18),
             (dict(ld_comp=0, ws=None), -16), (dict(out=None, tx=None), -10), (dict(nt=-1, mu=None), -8)]
    for kw, want in codes:
        assert call(**kw) == want, kw
    assert all(U.all_sentinel(t) for t in (out, comp, ccov, info)) and bool((ws == 0x7F).all())
    size = hip.lvae_predict_exact_comp_cov_workspace_size
    for bad in ((0, Nt, L, R, 16), (n, -1, L, R, 16), (n, Nt, 0, R, 16), (n, Nt, L, 0, 16), (n, Nt, L, 17, 16),
                (n, Nt, L, R, 0)):
        assert size(*bad) == 0, bad
    base = hip.lvae_predict_exact_comp_workspace_size(n, Nt, L, R)
    assert size(n, Nt, L, R, 1) - base >= 8 * L * n * R + 2048 * L
    assert size(n, Nt, L, R, 16) - base >= 8 * L * n * 16 * R + 2048 * L * 16
    assert size(n, Nt, L, R, Nt) == size(n, Nt, L, R, Nt + 100)             # a chunk beyond nt is nt
    assert size(n, 0, L, R, 0) == hip.lvae_predict_exact_comp_workspace_size(n, 0, L, R)
    # out and out_comp may be NULL (then mu may be too); no test rows: none of the row arguments is looked at
    assert call(out=None, comp=None, mu=None) == 0 and U.all_sentinel(out) and U.all_sentinel(comp)
    assert not U.all_sentinel(ccov) and U.tail_untouched(tail)
    ccov.fill_(float("nan"))
    assert call(nt=0, tx=None, out=None, comp=None, ccov=None, chunk=0) == 0 and U.all_sentinel(ccov)
    assert call() == 0 and not U.all_sentinel(comp) and U.tail_untouched(tail)


# ------------------------------------------------------------------------------------------------------
# inducing-point route
# ------------------------------------------------------------------------------------------------------
def ind_args(cid, groups=None, fill_seed=1, noise=None):
    """Device tensors of a case in the ABI's layout (test rows grouped by subject); groups: the subject groups to
    keep (default all).  Returns (args, rows): rows the kept grouped rows' indices among all grouped rows."""
    c = CC.ind_problem(cid)
    other = U.subject_covariates(np.random.default_rng(fill_seed), c["P"], c["T"]).reshape(c["NP"], U.QC)
    x = torch.where(c["valid"][:, None], c["x"], other)    # padding rows of x: any finite covariates
    dv = lambda t: t.to(DEV).contiguous()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    gs, gsub = c["group_start"], c["group_subject"]
    groups = list(range(len(gsub))) if groups is None else groups
    rows = [k for g in groups for k in range(gs[g], gs[g + 1])]
    start = [0]
    for g in groups:
        start.append(start[-1] + gs[g + 1] - gs[g])
    txg = c["tx"][c["order"]][rows] if rows else c["tx"][:0]
    a = dict(x=dv(x), z=dv(c["z"]), mu=dv(c["mu"]), tx=dv(txg), p0=dv(c["p0"]), p1=dv(c["p1"]),
             noise=dv(c["noise"] if noise is None else noise), seg=i32(c["seg"]), inc=dv(c["include"]),
             gsub=i32([gsub[g] for g in groups] + [0]), gstart=i32(start), G=len(groups), Nt=len(rows))
    return a, rows


def run_ind(hip, cid, groups=None, fill_seed=1, noise=None, mean=True, comp=True, pad=2):
    """One lvae_predict_comp_cov_f64 call; (out, out_comp, ccov [L, Nt', R, R], info) in the grouped row order"""
    from lvae_amd import _lib as P
    c = CC.ind_problem(cid)
    L, M, Pn, T = c["L"], c["M"], c["P"], c["T"]
    R0, R1 = len(c["s0"]), len(c["s1"])
    R = R0 + R1
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    a, _ = ind_args(cid, groups, fill_seed, noise)
    Nt = a["Nt"]
    ld_comp = L + pad
    cs = max(Nt, 1) * ld_comp + 3 * pad
    out, cbuf = U.sentinel(max(Nt, 1) * L + 7), U.sentinel(R * cs + 7)
    ccov = U.sentinel(L * Nt * R * R + TAIL)
    info = U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_comp_cov_workspace_size(L, M, Pn, T, Nt, R0, R1))
    r = ctypes.byref
    rc = hip.lvae_predict_comp_cov_f64(r(s0), r(s1), L, M, U.QC, Pn, T, P.ptr(a["seg"]), P.ptr(a["inc"]), P.ptr(a["x"]),
                                       P.ptr(a["mu"]) if mean else None, P.ptr(a["z"]), Nt,
                                       P.ptr(a["tx"]) if Nt else None, a["G"], P.ptr(a["gsub"]), P.ptr(a["gstart"]),
                                       P.ptr(a["p0"]), P.ptr(a["p1"]), P.ptr(a["noise"]), C.EPS,
                                       P.ptr(out) if mean else None, P.ptr(cbuf) if comp else None, ld_comp, cs,
                                       P.ptr(ccov), P.ptr(info), P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)
    assert U.all_sentinel(ccov[L * Nt * R * R:])
    assert U.all_sentinel(out[Nt * L:]) if mean else U.all_sentinel(out)
    assert U.untouched_outside(cbuf, (R, Nt, L), (cs, ld_comp, 1)) if mean and comp else U.all_sentinel(cbuf)
    o = out[:Nt * L].reshape(Nt, L).cpu() if mean and Nt else None
    k = U.view(cbuf, (R, Nt, L), (cs, ld_comp, 1)).cpu() if mean and comp and Nt else None
    return o, k, ccov[:L * Nt * R * R].reshape(L, Nt, R, R).cpu(), info.cpu().tolist()


def ind_siblings(hip, cid):
    """lvae_predict_comp_f64 (out, out_comp) and lvae_predict_var_f64 (var, add_noise = 0) on the grouped rows"""
    from lvae_amd import _lib as P
    c = CC.ind_problem(cid)
    L, M, Pn, T = c["L"], c["M"], c["P"], c["T"]
    R0, R1 = len(c["s0"]), len(c["s1"])
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    a, _ = ind_args(cid)
    Nt = a["Nt"]
    r = ctypes.byref
    out = torch.empty(Nt, L, dtype=torch.float64, device=DEV)
    comp = torch.empty(R0 + R1, Nt, L, dtype=torch.float64, device=DEV)
    var = torch.empty(Nt, L, dtype=torch.float64, device=DEV)
    info = U.sentinel(L, torch.int32)
    ws, _ = U.workspace(hip.lvae_predict_comp_workspace_size(L, M, Pn, T, Nt, R0, R1))
    rc = hip.lvae_predict_comp_f64(r(s0), r(s1), L, M, U.QC, Pn, T, P.ptr(a["seg"]), P.ptr(a["inc"]), P.ptr(a["x"]),
                                   P.ptr(a["mu"]), P.ptr(a["z"]), Nt, P.ptr(a["tx"]), P.ptr(a["p0"]), P.ptr(a["p1"]),
                                   P.ptr(a["noise"]), C.EPS, P.ptr(out), P.ptr(comp), L, Nt * L, P.ptr(info),
                                   P.ptr(ws), P.stream_ptr())
    assert rc == 0
    ws, _ = U.workspace(hip.lvae_predict_var_workspace_size(L, M, Pn, T, Nt))
    rc = hip.lvae_predict_var_f64(r(s0), r(s1), L, M, U.QC, Pn, T, P.ptr(a["seg"]), P.ptr(a["inc"]), P.ptr(a["x"]),
                                  None, P.ptr(a["z"]), Nt, P.ptr(a["tx"]), a["G"], P.ptr(a["gsub"]), P.ptr(a["gstart"]),
                                  P.ptr(a["p0"]), P.ptr(a["p1"]), P.ptr(a["noise"]), C.EPS, None, P.ptr(var), 0, None,
                                  P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return out.cpu(), comp.cpu(), var.cpu(), info.cpu().tolist()


@gpu
@pytest.mark.parametrize("cid", CC.IND_IDS)
def test_comp_cov_abi(hip, cid):
    c = CC.ind_problem(cid)
    L, Nt, R0, R1 = c["L"], c["Nt"], len(c["s0"]), len(c["s1"])
    out, comp, cov, info = run_ind(hip, cid)
    assert info == [0] * L
    o2, k2, c2, _ = run_ind(hip, cid, fill_seed=2, pad=0)
    assert U.bit_equal(c2, cov)                                                # other padding rows and strides
    if Nt == 0:
        assert cov.numel() == 0 and out is None                                # rc 0, info written, nothing else
        return
    assert U.bit_equal(o2, out) and U.bit_equal(k2, comp)
    pout, pcomp, var, pinfo = ind_siblings(hip, cid)
    assert pinfo == info and U.bit_equal(out, pout) and U.bit_equal(comp, pcomp)   # lvae_predict_comp_f64's bits
    _, _, c3, _ = run_ind(hip, cid, mean=False, comp=False)
    assert U.bit_equal(c3, cov)                                                # without the means (mu NULL too)
    assert U.bit_equal(cov, cov.transpose(2, 3))                               # symmetric bit for bit
    # a row's block does not depend on the other rows of the call: each subject group alone
    gs = c["group_start"]
    for g in range(len(c["group_subject"])):
        _, _, cg, _ = run_ind(hip, cid, groups=[g], mean=False, comp=False)
        assert U.bit_equal(cg, cov[:, gs[g]:gs[g + 1]]), g
    (ref, prior), ya = CC.ind_ref(cid)
    order = c["order"]
    ref, prior = ref[:, order], prior[:, order]                                # the grouped row order
    yard = max(ya, CC.ccov_err(CC.ind_oracle(cid, DEV)[0][:, order], ref, prior))
    err, tol = CC.ccov_err(cov, ref, prior), CC.bound(yard)
    serr = float((cov.sum((2, 3)).T - var).abs().max() / float(prior.max()))
    print(f"inducing comp cov {cid}: M {c['M']} Nt {Nt} R {R0 + R1} err {err:.2e} yardstick {yard:.2e} "
          f"bound {tol:.1e}; |sum_rs - var| {serr:.2e}")
    assert bool(torch.isfinite(cov).all())
    assert err <= tol
    assert serr <= tol
    # an id component at a subject outside the prediction set (every test row of none-included): its column is zero
    absent = torch.tensor([c["group_subject"][g] < 0 for g in range(len(gs) - 1) for _ in range(gs[g], gs[g + 1])])
    if cid == "none-included":
        assert bool(absent.all())
    if bool(absent.any()):
        check_zero_components(cov, prior, absent, list(range(R0, R0 + R1)))


@gpu
def test_comp_cov_info(hip):
    """A dim whose noise makes every B_p indefinite: info[l] = 20001 for that dim only, the other dims' blocks keep
    their bits."""
    c = CC.ind_problem("m3-mixed")
    _, _, good, info = run_ind(hip, "m3-mixed")
    assert info == [0, 0, 0]
    bad = c["noise"].clone()
    bad[1] = -100.0
    _, _, got, info = run_ind(hip, "m3-mixed", noise=bad)
    assert info == [0, 20001, 0]
    assert U.bit_equal(got[[0, 2]], good[[0, 2]])


@gpu
def test_comp_cov_return_codes(hip):
    """Every documented bad-argument code in its documented order, each with only that argument bad and each
    rejected before any launch: nothing is written.  The size function gives 0 for rejected sizes."""
    from lvae_amd import _lib as P
    r = ctypes.byref
    cid = "m3-mixed"
    c = CC.ind_problem(cid)
    L, M, Pn, T = c["L"], c["M"], c["P"], c["T"]
    R0, R1 = len(c["s0"]), len(c["s1"])
    R = R0 + R1
    g0, g1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    bad = P.KernelSpec.from_buffer_copy(g0)
    bad.n_comp = 17
    far = P.KernelSpec.from_buffer_copy(g1)
    far.dim[0][0] = 32
    none = P.KernelSpec.from_buffer_copy(g1)
    none.n_comp = 0
    t, _ = ind_args(cid)
    Nt = t["Nt"]
    out, comp, info = U.sentinel(Nt * L), U.sentinel(R * Nt * L), U.sentinel(L, torch.int32)
    ccov = U.sentinel(L * Nt * R * R)
    ws, tail = U.workspace(hip.lvae_predict_comp_cov_workspace_size(L, M, Pn, T, Nt, R0, R1))

    def call(**kw):
        a = dict(s0=r(g0), s1=r(g1), L=L, M=M, Q=U.QC, P=Pn, T=T, seg=P.ptr(t["seg"]), inc=P.ptr(t["inc"]),
                 x=P.ptr(t["x"]), mu=P.ptr(t["mu"]), z=P.ptr(t["z"]), Nt=Nt, tx=P.ptr(t["tx"]), G=t["G"],
                 gsub=P.ptr(t["gsub"]), gstart=P.ptr(t["gstart"]), p0=P.ptr(t["p0"]), p1=P.ptr(t["p1"]),
                 noise=P.ptr(t["noise"]), out=P.ptr(out), comp=P.ptr(comp), ld_comp=L, cs=Nt * L, ccov=P.ptr(ccov),
                 info=P.ptr(info), ws=ws.data_ptr())
        a.update(kw)
        rc = hip.lvae_predict_comp_cov_f64(a["s0"], a["s1"], a["L"], a["M"], a["Q"], a["P"], a["T"], a["seg"], a["inc"],
                                           a["x"], a["mu"], a["z"], a["Nt"], a["tx"], a["G"], a["gsub"], a["gstart"],
                                           a["p0"], a["p1"], a["noise"], C.EPS, a["out"], a["comp"], a["ld_comp"],
                                           a["cs"], a["ccov"], a["info"], a["ws"], P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    q_need = 1 + max(d for cp in c["s0"] + c["s1"] for _, d in cp)
    codes = [(dict(s0=None), -1), (dict(s1=None), -1), (dict(s0=r(bad)), -1), (dict(s1=r(far)), -1),
             (dict(s1=r(none)), -1), (dict(L=0), -3), (dict(L=65536), -3), (dict(M=0), -3), (dict(M=129), -3),
             (dict(P=0), -6), (dict(T=0), -6), (dict(T=129), -6), (dict(Q=0), -6), (dict(Q=q_need - 1), -6),
             (dict(seg=None), -8), (dict(inc=None), -8), (dict(mu=None), -9), (dict(x=None), -10), (dict(z=None), -10),
             (dict(p0=None), -11), (dict(p1=None), -11), (dict(noise=None), -11), (dict(Nt=-1), -13),
             (dict(Nt=2 ** 31 // R + 1), -13), (dict(tx=None), -12), (dict(G=-1), -14), (dict(gsub=None), -15),
             (dict(gstart=None), -15), (dict(ws=None), -20), (dict(ws=ws.data_ptr() + 8), -20),
             (dict(ws=ws.data_ptr() + 128), -20), (dict(out=None), -21), (dict(ld_comp=L - 1), -22),
             (dict(cs=Nt * L - 1), -23), (dict(cs=0), -23), (dict(ccov=None), -24),
             # the documented order where two arguments are bad
             (dict(ccov=None, cs=0), -23), (dict(cs=0, ld_comp=0), -22), (dict(ld_comp=0, out=None), -21),
             (dict(out=None, ws=None), -20), (dict(ws=None, gsub=None), -15), (dict(G=-1, tx=None), -12),
             (dict(tx=None, Nt=-1), -13), (dict(Nt=-1, noise=None), -11), (dict(p0=None, z=None), -10)]
    for kw, want in codes:
        assert call(**kw) == want, kw
    assert all(U.all_sentinel(v) for v in (out, comp, ccov, info)) and bool((ws == 0x7F).all())
    size = hip.lvae_predict_comp_cov_workspace_size
    for badsz in ((0, M, Pn, T, Nt, R0, R1), (L, 0, Pn, T, Nt, R0, R1), (L, 129, Pn, T, Nt, R0, R1),
                  (L, M, 0, T, Nt, R0, R1), (L, M, Pn, 0, Nt, R0, R1), (L, M, Pn, 129, Nt, R0, R1),
                  (L, M, Pn, T, -1, R0, R1), (L, M, Pn, T, Nt, 0, R1), (L, M, Pn, T, Nt, R0, 17),
                  (L, M, Pn, T, 2 ** 31 // R + 1, R0, R1)):
        assert size(*badsz) == 0, badsz
    extra = (hip.lvae_predict_comp_workspace_size(L, M, Pn, T, Nt, R0, R1)
             - hip.lvae_predict_workspace_size(L, M, Pn, T, Nt))
    assert size(L, M, Pn, T, Nt, R0, R1) == hip.lvae_predict_var_workspace_size(L, M, Pn, T, Nt * R) + extra
    assert call(out=None, comp=None, mu=None) == 0 and U.all_sentinel(out) and U.all_sentinel(comp)
    assert not U.all_sentinel(ccov) and U.tail_untouched(tail)
    assert call() == 0 and not U.all_sentinel(comp) and U.tail_untouched(tail)


# ------------------------------------------------------------------------------------------------------
# the Python functions
# ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("batched", [True, False])
def test_predict_exact_components_cov(hip, batched):
    import lvae_amd as la
    import test_gpu_predict_exact_abi as E
    c = E.problem("tile-edge")
    L, Nt = c["L"], c["Nt"]
    k0, k1, p0, p1 = TC.ref_kernels(L, 11)
    w0, w1 = U.spec_pairs()["ref"]
    spec, params = w0 + w1, torch.cat([p0, p1], 1)
    R = len(spec)
    k = k0 + k1
    if not batched:
        def one():
            a, b = la.generate_kernel_batched(1, **U._REF_CFG, id_covariate=U.ID_COL)
            return a + b
        k = TC.per_dim(k, L, one)
    lik = TC.liks(c["noise"], batched)
    X, tx, mu = c["x"].to(DEV), c["tx"].to(DEV), c["mu"].to(DEV)
    z0, plain = la.predict_exact_components(k, lik, X, tx, mu)
    assert plain.cov is None                                                   # the default: nothing new
    z_pred, comps = la.predict_exact_components(k, lik, X, tx, mu, return_cov=True)
    assert U.bit_equal(z_pred, z0) and U.bit_equal(comps.values, plain.values)
    assert comps.cov.shape == (L, Nt, R, R) and comps.cov.dtype == torch.float64

    def oracle(dev, pert=False):
        v = [params, c["noise"]]
        if pert:
            v = [U.perturbed(t, torch.Generator().manual_seed(93 + i)) for i, t in enumerate(v)]
        return tuple(t.cpu() for t in CC.exact_ccov(spec, v[0].to(dev), v[1].to(dev), c["x"].to(dev), c["tx"].to(dev)))
    ref, prior = oracle("cpu")
    yard = max(CC.ccov_err(oracle("cpu", True)[0], ref, prior), CC.ccov_err(oracle(DEV)[0], ref, prior))
    err, tol = CC.ccov_err(comps.cov, ref, prior), CC.bound(yard)
    _, var = la.predict_exact(k, lik, X, tx, mu, return_var=True)
    tv = comps.total_variance()
    up = var > 0                                                               # above predict_exact's clamp
    verr = float((tv - var)[up].abs().max() / float(prior.max()))
    print(f"predict_exact_components cov batched={batched}: err {err:.2e} yardstick {yard:.2e} bound {tol:.1e}; "
          f"|total_variance - var| {verr:.2e}")
    assert err <= tol and verr <= tol and bool(up.any())
    assert comps.variance().shape == (R, Nt, L) and bool((comps.partial_variance()[-1] - tv.clamp(min=0)).abs().max()
                                                        <= 1e-12 * float(prior.max()))
    lo, hi = comps.credible_interval()
    assert bool((lo <= comps.values).all()) and bool((comps.values <= hi).all())
    # a cap that forces several dim groups and, after them, several test-row chunks: the same bits
    size = lambda g, ch: int(hip.lvae_predict_exact_comp_cov_workspace_size(c["n"], Nt, g, R, ch))
    cap = size(1, 5)
    assert cap < size(2, 1) and cap < size(1, Nt)
    z2, c2 = la.predict_exact_components(k, lik, X, tx, mu, max_workspace_bytes=cap, return_cov=True)
    assert U.bit_equal(z2, z_pred) and U.bit_equal(c2.values, comps.values) and U.bit_equal(c2.cov, comps.cov)


@gpu
@pytest.mark.parametrize("batched", [True, False])
def test_batch_predict_components_cov(hip, batched):
    import lvae_amd as la
    c = C.ind_problem("ref-ragged")
    L, ok, Nt = c["L"], c["valid"], c["Nt"]
    k0, k1, p0, p1 = TC.ref_kernels(L, 12)
    if not batched:
        k0 = TC.per_dim(k0, L, lambda: la.generate_kernel_batched(1, **U._REF_CFG, id_covariate=U.ID_COL)[0])
        k1 = TC.per_dim(k1, L, lambda: la.generate_kernel_batched(1, **U._REF_CFG, id_covariate=U.ID_COL)[1])
    lik = TC.liks(c["noise"], batched)
    X, tx, mu = c["x"][ok].to(DEV), c["tx"].to(DEV), c["mu"][ok].to(DEV)
    z = c["z"].to(DEV) if batched else [zl.to(DEV) for zl in c["z"]]
    args = (L, k0, k1, lik, X, tx, mu, z, U.ID_COL, C.EPS)
    R0, R1 = len(c["s0"]), len(c["s1"])
    R = R0 + R1
    z0, plain = la.batch_predict_components(*args)
    assert plain.cov is None
    z_pred, comps = la.batch_predict_components(*args, return_cov=True)
    assert U.bit_equal(z_pred, z0) and U.bit_equal(comps.values, plain.values)
    assert comps.cov.shape == (L, Nt, R, R) and comps.module == [0] * R0 + [1] * R1

    def oracle(dev, pert=False):
        v = [p0, p1, c["noise"], c["z"]]
        if pert:
            gen = torch.Generator().manual_seed(94)
            v = [U.perturbed(t, gen) for t in v[:3]] + [CC.V.perturbed_z(v[3], c["s0"], gen)]
        v = [t.to(dev) for t in v]
        return tuple(t.cpu() for t in CC.inducing_ccov(c["s0"], v[0], c["s1"], v[1], v[2], c["x"][ok].to(dev),
                                                       c["tx"].to(dev), v[3], C.EPS))
    ref, prior = oracle("cpu")
    yard = max(CC.ccov_err(oracle("cpu", True)[0], ref, prior), CC.ccov_err(oracle(DEV)[0], ref, prior))
    err, tol = CC.ccov_err(comps.cov, ref, prior), CC.bound(yard)
    _, var = la.batch_predict_varying_T(*args, return_var=True)
    tv = comps.total_variance()
    up = var > 0
    verr = float((tv - var)[up].abs().max() / float(prior.max()))
    print(f"batch_predict_components cov batched={batched}: err {err:.2e} yardstick {yard:.2e} bound {tol:.1e}; "
          f"|total_variance - var| {verr:.2e}")
    assert err <= tol and verr <= tol and bool(up.any())
    # a cap below two subjects' workspace: one chunk a subject, the same bits
    counts = torch.unique(c["tx"][:, U.ID_COL], return_counts=True)[1]
    two = int(counts.sort().values[:2].sum())
    cap = int(hip.lvae_predict_comp_cov_workspace_size(L, c["M"], c["P"], c["T"], two, R0, R1)) - 1
    z2, c2 = la.batch_predict_components(*args, return_cov=True, max_workspace_bytes=cap)
    assert U.bit_equal(z2, z_pred) and U.bit_equal(c2.values, comps.values) and U.bit_equal(c2.cov, comps.cov)
