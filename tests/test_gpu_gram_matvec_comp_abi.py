"""lvae_gram_matvec_comp_f64 alone through the C ABI, on sentinel buffers with ld_v > L, ld_out > L and
ostride_r > n1 ld_out, against per-component references on the CPU: component r's Gram is O.gram of the
one-component spec on its own parameter columns (predict_comp_util.comp_gram), ref[r] = K_r v.

Shapes (predict_comp_util.MV_CASES): 63 / 64 / 65 rows against 59 / 64 / 65 columns, both template buckets (ref;
mix1 / mix2), per / lin factors (ext), 18 covariate columns (wide-cols: the 32-slot LDS image), L = 1 and L = 16, the
slab path (3 rows against the fewest columns at which the size query reports S >= 2, and one tile fewer: S = 1),
per-dim x2 [L, M, Q] with M = 1 / 17 / 128, one component (R = 1), and test subjects all absent from x2 (the id
components are then exactly zero).
The xl-* cases run predict_comp_util.XLIN (a bare lin on a signed real column, cat x lin, bin x lin, per, per x rbf
and the reference kinds) at 1 x 1, 65 x 130 and the slab path, with a shared and a per-dim x2 and with real and
integer-coded times, all twelve combinations (a single pair has one distance: 2 in its integer cases,
predict_comp_util.mv_problem says why); at 65 x 130 the column of the gated lin factors is zero on the whole first
64-row tile of x1 while bin gates of that tile are on: the component is zero there with no gate saying so (the wave
skip of an all-zero component), exact zeros are asserted, and the rows after the tile are not zero.

Bound per component and latent dim: max_i |got - ref| <= 2^-52 (n2 + 16) max_i sum_j |K_r,ij v_j|, the a-priori
forward error of an n2-term fp64 dot product in any order (16: the few ulps of each kernel value's exp / sin on
either side), as test_gpu_predict_exact_abi.test_gram_matvec_values bounds the summed product.

Measured on the MI355X: the worst err / bound over components and dims is 0.57 at z1 (one column: the bound is 17
ulps of the single product), 0.27 at z17, 0.11 at L16 and at most 0.06 elsewhere; sum_r differs from
lvae_gram_matvec_f64's result by at most 1.4e-14 absolute against bounds of 5e-13 .. 2.5e-11.  The xl-* cases: worst
err / bound 0.68 (xl-1x1-int), 0.65 (xl-z65x130-int), 0.47 (xl-z1x1), 0.28 (xl-65x130-int), 0.22 (xl-1x1), 0.19
(xl-z1x1-int), 0.17 (xl-slab-int), at most 0.11 elsewhere; sum_r within 2.9e-14 of lvae_gram_matvec_f64 against
bounds of 1.7e-11 and more (within 1.8e-15 on the single products of the 1 x 1 cases).  The module's 36 tests take
under 3 s.
"""
import ctypes

import pytest
import torch

import abi_util as U
import predict_comp_util as C

gpu = pytest.mark.gpu
DEV = U.DEV
EPS52 = 2.0 ** -52


def call_comp(hip, cid, pad):
    """One call on sentinel buffers (pad > 0: ld_v = L + 2, ld_out = L + 3, ostride_r = n1 ld_out + 5 and padded
    covariates; pad = 0: everything dense); returns out [R, n1, L] on the CPU"""
    from lvae_amd import _lib as P
    c = C.mv_problem(cid)
    L, R, n1, n2 = c["L"], c["R"], c["n1"], c["n2"]
    spec = P.make_spec(c["spec"])
    Q = c["x1"].shape[1]
    ldx = Q + pad
    x1b, _ = U.padded(c["x1"], (ldx, 1))
    if c["per_dim"]:
        x2_ls = n2 * ldx + 2 * pad
        x2b, _ = U.padded(c["x2"], (x2_ls, ldx, 1))
    else:
        x2_ls = 0
        x2b, _ = U.padded(c["x2"], (ldx, 1))
    ld_v = L + (2 if pad else 0)
    vb, _ = U.padded(c["v"], (ld_v, 1))
    ld_out = L + (3 if pad else 0)
    os_r = n1 * ld_out + (5 if pad else 0)
    out = U.sentinel(U.extent((R, n1, L), (os_r, ld_out, 1)) + 7)
    params = c["params"].to(DEV).contiguous()
    ws, tail = U.workspace(hip.lvae_gram_matvec_comp_workspace_size(n1, n2, L, R))
    rc = hip.lvae_gram_matvec_comp_f64(ctypes.byref(spec), P.ptr(x1b), ldx, n1, P.ptr(x2b), ldx, x2_ls, n2, L,
                                       P.ptr(params), P.ptr(vb), ld_v, P.ptr(out), ld_out, os_r, P.ptr(ws),
                                       P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)                                          # the workspace size is enough
    assert U.untouched_outside(out, (R, n1, L), (os_r, ld_out, 1))         # nothing outside the logical extent
    return U.view(out, (R, n1, L), (os_r, ld_out, 1)).cpu()


def call_sum(hip, cid):
    """lvae_gram_matvec_f64 at the same inputs (per-dim x2: one call per latent dim); out [n1, L] on the CPU"""
    from lvae_amd import _lib as P
    c = C.mv_problem(cid)
    L, n1, n2 = c["L"], c["n1"], c["n2"]
    spec = P.make_spec(c["spec"])
    dv = lambda t: t.to(DEV).contiguous()
    x1, x2, v, params = dv(c["x1"]), dv(c["x2"]), dv(c["v"]), dv(c["params"])
    Q = x1.shape[1]
    out = torch.empty(n1, L, dtype=torch.float64, device=DEV)
    groups = [(l, 1, x2[l]) for l in range(L)] if c["per_dim"] else [(0, L, x2)]
    for l0, g, xx in groups:
        ws, _ = U.workspace(hip.lvae_gram_matvec_workspace_size(n1, n2, g))
        at = lambda t, off: ctypes.c_void_p(t.data_ptr() + 8 * off)
        rc = hip.lvae_gram_matvec_f64(ctypes.byref(spec), P.ptr(x1), Q, n1, P.ptr(xx), Q, n2, g,
                                      at(params, l0 * params.shape[1]), None, at(v, l0), L, at(out, l0), L,
                                      P.ptr(ws), P.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
    return out.cpu()


@gpu
@pytest.mark.parametrize("cid", C.MV_IDS)
def test_gram_matvec_comp_values(hip, cid):
    c = C.mv_problem(cid)
    L, R, n1, n2 = c["L"], c["R"], c["n1"], c["n2"]
    got = call_comp(hip, cid, pad=3)
    assert U.bit_equal(got, call_comp(hip, cid, pad=0))                    # other strides: the same bits
    ref, mag, full = C.mv_ref(cid)
    assert bool(torch.isfinite(got).all())
    ids = [r for r, comp in enumerate(c["spec"]) if ("cat", U.ID_COL) in comp]
    worst = 0.0
    for r in range(R):
        if c["absent"] and r in ids:
            assert bool((got[r] == 0.0).all()), (cid, r)                   # a zero cross-Gram: exact zeros
            continue
        err = (got[r] - ref[r]).abs().max(0).values                        # [L]: max over the rows
        tol = EPS52 * (n2 + 16) * mag[r]
        worst = max(worst, float((err / tol.clamp(min=1e-300)).max()))   # (tol = 0: a dim the gates zero, err = 0)
        print(f"gram_matvec_comp {cid} r={r}: err {float(err.max()):.2e} bound {float(tol.min()):.1e}")
        assert bool((err <= tol).all()), (cid, r, err.tolist(), tol.tolist())
    # against the existing kernel at the same inputs: twice the bound of the full kernel
    tot = call_sum(hip, cid)
    derr = (got.sum(0) - tot).abs().max(0).values
    dtol = 2.0 * EPS52 * (n2 + 16) * full
    print(f"gram_matvec_comp {cid}: [{n1} x {n2}] L {L} R {R} S {C.slabs(n1, n2, L, R)} worst err / bound "
          f"{worst:.2g}; |sum_r - matvec| {float(derr.max()):.2e} bound {float(dtol.min()):.1e}")
    assert bool((derr <= dtol).all())
    if c["spec"] is C.XLIN and n1 > 64:   # a component that is zero on a whole tile with no gate saying so
        z = C.XL_ZERO_COMP
        assert bool((ref[z][:64] == 0).all()) and bool((got[z][:64] == 0).all()) and bool((got[z][64:] != 0).any())
        assert bool((c["x1"][:64, 5] == 1).any()) and bool((ref[1][:64] == 0).all()) and bool((ref[0] != 0).all())
    if cid in ("slab", "xl-slab", "xl-zslab-int", "xl-slab-int", "xl-zslab"):
        assert C.slabs(n1, n2, L, R) >= 2
    if cid == "slab-64":
        assert C.slabs(n1, n2, L, R) == 1
    if c["absent"]:
        assert len(ids) == 2


@gpu
def test_gram_matvec_comp_empty_sides(hip):
    """n2 == 0 writes zeros to all R blocks [n1, L] and returns 0; n1 == 0 returns 0 and writes nothing."""
    from lvae_amd import _lib as P
    c = C.mv_problem("e63x59")
    L, R, n = c["L"], c["R"], c["n1"]
    spec = P.make_spec(c["spec"])
    x, params = c["x1"].to(DEV).contiguous(), c["params"].to(DEV).contiguous()
    ld_out, os_r = L + 1, n * (L + 1) + 3
    out = U.sentinel(U.extent((R, n, L), (os_r, ld_out, 1)) + 3)
    rc = hip.lvae_gram_matvec_comp_f64(ctypes.byref(spec), P.ptr(x), U.QC, n, None, 0, 0, 0, L, P.ptr(params), None, 0,
                                       P.ptr(out), ld_out, os_r, None, P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and U.untouched_outside(out, (R, n, L), (os_r, ld_out, 1))
    assert bool((U.view(out, (R, n, L), (os_r, ld_out, 1)) == 0).all())
    out = U.sentinel(8)
    rc = hip.lvae_gram_matvec_comp_f64(ctypes.byref(spec), None, 0, 0, P.ptr(x), U.QC, 0, n, L, P.ptr(params), None, 0,
                                       P.ptr(out), L, 0, None, P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and U.all_sentinel(out)


@gpu
def test_gram_matvec_comp_return_codes(hip):
    """Every documented bad-argument code, each rejected before any launch: nothing is written.  On the slab shape
    (its workspace is needed there)."""
    from lvae_amd import _lib as P
    c = C.mv_problem("slab")
    L, R, n1, n2 = c["L"], c["R"], c["n1"], c["n2"]
    good = P.make_spec(c["spec"])
    bad = P.KernelSpec.from_buffer_copy(good)
    bad.n_comp = 17                                  # no bucket holds it
    far = P.KernelSpec.from_buffer_copy(good)
    far.dim[0][0] = 32                               # factor dims below 32
    neg = P.KernelSpec.from_buffer_copy(good)
    neg.dim[0][0] = -1
    one = P.make_spec(C.R1_SPEC)                     # R = 1: ostride_r is not looked at
    dv = lambda t: t.to(DEV).contiguous()
    x1, x2, v, params = dv(c["x1"]), dv(c["x2"]), dv(c["v"]), dv(c["params"])
    out = U.sentinel(R * n1 * L)
    nbytes = hip.lvae_gram_matvec_comp_workspace_size(n1, n2, L, R)
    assert nbytes > 0
    ws, tail = U.workspace(nbytes)
    r = ctypes.byref

    def mvc(**kw):
        a = dict(spec=r(good), x1=P.ptr(x1), ld1=U.QC, n1=n1, x2=P.ptr(x2), ld2=U.QC, x2s=0, n2=n2, L=L,
                 params=P.ptr(params), v=P.ptr(v), ld_v=L, out=P.ptr(out), ld_out=L, os_r=n1 * L, ws=ws.data_ptr())
        a.update(kw)
        rc = hip.lvae_gram_matvec_comp_f64(a["spec"], a["x1"], a["ld1"], a["n1"], a["x2"], a["ld2"], a["x2s"], a["n2"],
                                           a["L"], a["params"], a["v"], a["ld_v"], a["out"], a["ld_out"], a["os_r"],
                                           a["ws"], P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    ld_need = 1 + max(d for comp in c["spec"] for _, d in comp)
    for kw in (dict(spec=None), dict(spec=r(bad)), dict(spec=r(far)), dict(spec=r(neg))):
        assert mvc(**kw) == -1, kw
    codes = [(dict(n1=-1), -4), (dict(n2=-1), -7), (dict(L=0), -8), (dict(x1=None), -2), (dict(ld1=ld_need - 1), -3),
             (dict(x2=None), -5), (dict(ld2=ld_need - 1), -6), (dict(params=None), -9), (dict(v=None), -11),
             (dict(ld_v=L - 1), -12), (dict(out=None), -13), (dict(ld_out=L - 1), -14), (dict(x2s=-1), -16),
             (dict(os_r=n1 * L - 1), -17), (dict(os_r=0), -17), (dict(os_r=-5), -17),
             (dict(ws=None), -15), (dict(ws=ws.data_ptr() + 8), -15), (dict(ws=ws.data_ptr() + 128), -15)]
    for kw, want in codes:
        assert mvc(**kw) == want, kw
    # the order of the checks: the earlier fault wins
    assert mvc(ld_out=L - 1, x2s=-1, os_r=0, ws=None) == -14 and mvc(x2s=-1, os_r=0, ws=None) == -16
    assert mvc(os_r=0, ws=None) == -17 and mvc(n1=-1, x1=None) == -4 and mvc(n1=0, x1=None, out=None) == 0
    assert U.all_sentinel(out) and bool((ws == 0x7F).all())
    assert mvc(spec=r(one), os_r=0) == 0             # R = 1: any ostride_r
    assert U.all_sentinel(out[n1 * L:]) and not U.all_sentinel(out[:n1 * L])
    assert mvc() == 0 and not U.all_sentinel(out) and U.tail_untouched(tail)   # (nothing wrong: it runs)
