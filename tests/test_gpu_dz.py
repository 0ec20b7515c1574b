"""Learnable inducing points on the GPU: lvae_gram_bwd_x2_f64 against autograd of O.gram, and the gradient with
respect to z of the DUBO, the sampled ELBO and the Hensman bound (through Python with z.requires_grad_(), through
the raw C ABI of the three _bwd_z calls, and through DuboStep / ElboStep with z a parameter) against CPU autograd
through the oracle.  Inputs, runners and the bounds' reasoning: dz_util.py.

Bounds: the Gram input adjoint 1e-11 of max |dx2| (dz_util.GRAM_BOUND); dz of the three bounds 1e-6 with
abi_util.rel, the bound the raw kernel gradients of the same cases are held to (they contract the same dX, dKz),
but for the one named case that misses it on the MI355X, 6x7x33 (cond(Kz) 4.6e7: coinciding inducing rows), which
is held to 4x its measured error (dz_util.CASE_BOUND has the figures and the reason);
the steps' z.grad 1e-4 (an fp32 ConvVAE against the fp64 oracle: test_dubo_step_vs_oracle's bound for the raw kernel
gradients)."""
import ctypes

import numpy as np
import pytest
import torch

import abi_util as U
import dubo_util as D
import dz_util as Z
import gp_elbo_util as G
from oracle import lvae_oracle as O

pytestmark = pytest.mark.gpu
DEV = Z.DEV
L = Z.L


# ------------------------------------------------------------------------------------------------------
# 1. lvae_gram_bwd_x2_f64
# ------------------------------------------------------------------------------------------------------
def _gram_check(hip, c, what):
    (got,) = Z.gram_x2_call(hip, c)
    ref = c["ref"]
    err = U.rel(got, ref)
    print(f"gram_bwd_x2 {what}: max |dx2| {float(ref.abs().max()):.3e} err {err:.2e}")
    assert err < Z.GRAM_BOUND, (what, err)
    dead = [q for q in range(Z.QX) if not any(k in ("rbf", "per", "lin") and d == q for comp in c["spec"]
                                               for k, d in comp)]
    assert dead and bool((got[..., dead] == 0).all()) and bool((ref[..., dead] == 0).all())


@pytest.mark.parametrize("bucket", list(Z.SPECS))
@pytest.mark.parametrize("n2", [1, 33, 128])
@pytest.mark.parametrize("n1", [1, 63, 64, 65, 257])
def test_gram_bwd_x2_vs_autograd(hip, n1, n2, bucket):
    _gram_check(hip, Z.gram_case(bucket, n1, n2), f"{bucket} {n1}x{n2}")


@pytest.mark.parametrize("bucket", list(Z.SPECS))
@pytest.mark.parametrize("nb,mode", [(2, "plain"), (2, "bcast"), (1, "copy"), (1, "gt")])
def test_gram_bwd_x2_layouts(hip, nb, mode, bucket):
    """nb = 2; a stride-0 x2 (every (b, l) slice still gets its own dx2); x2 rows copied from x1 (a == b hits: the
    periodic factor's derivative is 0 there, as autograd through abs); G through its transposed strides"""
    c = Z.gram_case(bucket, 65, 33, nb=nb, mode=mode)
    if mode == "copy":
        assert bool((c["x1"][..., None, :, 1] == c["x2"][..., :, None, 1]).any())
    _gram_check(hip, c, f"{bucket} nb={nb} {mode}")


def test_gram_bwd_x2_same_bits_twice(hip):
    a, b = Z.gram_x2_call(hip, Z.gram_case("16x4", 257, 128), calls=2)
    assert U.bit_equal(a, b)


def test_gram_bwd_x2_wide_q_and_swapped_operands(hip):
    """Q past the spec's columns: the extra columns are exact zeros; and the first operand's adjoint as the header
    says: x1 and x2 swapped, G transposed."""
    from lvae_amd import _lib as P
    c = Z.gram_case("8x2", 65, 33)
    spec = P.make_spec(c["spec"])
    Lg, n1, n2, Qw = c["L"], c["n1"], c["n2"], 11
    x1 = torch.zeros(1, Lg, n1, Qw, dtype=torch.float64)
    x2 = torch.zeros(1, Lg, n2, Qw, dtype=torch.float64)
    x1[..., :Z.QX], x2[..., :Z.QX] = c["x1"], c["x2"]
    x1, x2 = x1.to(DEV), x2.to(DEV)
    params, Gd = c["params"].to(DEV), c["G"].to(DEV).contiguous()
    out = U.sentinel(Lg * n2 * Qw + Z.TAIL)
    ws, tail = U.workspace(hip.lvae_gram_bwd_x2_workspace_size(1, Lg, n1, n2, Qw))
    rc = hip.lvae_gram_bwd_x2_f64(ctypes.byref(spec), P.xview(x1, 0, n1 * Qw), P.xview(x2, 0, n2 * Qw), 1, Lg, n1, n2,
                                  Qw, P.ptr(params), P.ptr(Gd), 0, n1 * n2, n2, 1, P.ptr(out), P.ptr(ws),
                                  P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and U.tail_untouched(tail) and U.all_sentinel(out[Lg * n2 * Qw:])
    got = out[:Lg * n2 * Qw].reshape(1, Lg, n2, Qw).cpu()
    assert U.rel(got[..., :Z.QX], c["ref"]) < Z.GRAM_BOUND and bool((got[..., Z.QX:] == 0).all())
    # d/dx1: swap the operands, hand G over transposed
    leaf = c["x1"].clone().requires_grad_()
    (O.gram(c["spec"], c["params"], leaf, c["x2"]) * c["G"]).sum().backward()
    out = U.sentinel(Lg * n1 * Qw + Z.TAIL)
    ws, tail = U.workspace(hip.lvae_gram_bwd_x2_workspace_size(1, Lg, n2, n1, Qw))
    rc = hip.lvae_gram_bwd_x2_f64(ctypes.byref(spec), P.xview(x2, 0, n2 * Qw), P.xview(x1, 0, n1 * Qw), 1, Lg, n2, n1,
                                  Qw, P.ptr(params), P.ptr(Gd), 0, n1 * n2, 1, n2, P.ptr(out), P.ptr(ws),
                                  P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and U.tail_untouched(tail) and U.all_sentinel(out[Lg * n1 * Qw:])
    got = out[:Lg * n1 * Qw].reshape(1, Lg, n1, Qw).cpu()
    err = U.rel(got[..., :Z.QX], leaf.grad)
    print(f"gram_bwd_x2 swapped operands: err {err:.2e}")
    assert err < Z.GRAM_BOUND


def test_gram_bwd_x2_return_codes(hip):
    """The header's order: -1 (spec) -4 (counts, Q) -8 (params) -9 (G) -13 (dx2) -15 (workspace), nothing written
    before any of them; n1 == 0 writes zeros, n2 == 0 writes nothing."""
    from lvae_amd import _lib as P
    c = Z.gram_case("8x2", 63, 33)
    spec = P.make_spec(c["spec"])
    Lg, n1, n2, Q = c["L"], c["n1"], c["n2"], Z.QX
    x1, x2 = c["x1"].to(DEV), c["x2"].to(DEV)
    params, Gd = c["params"].to(DEV), c["G"].to(DEV).contiguous()
    n = Lg * n2 * Q
    out = U.sentinel(n + Z.TAIL)
    ws, tail = U.workspace(hip.lvae_gram_bwd_x2_workspace_size(1, Lg, n1, n2, Q))
    v1, v2 = P.xview(x1, 0, n1 * Q), P.xview(x2, 0, n2 * Q)

    def call(spec_=spec, nb=1, Lc=Lg, a=n1, b=n2, q=Q, p=params, g=Gd, o=out, w=ws):
        rc = hip.lvae_gram_bwd_x2_f64(None if spec_ is None else ctypes.byref(spec_), v1, v2, nb, Lc, a, b, q,
                                      P.ptr(p), P.ptr(g), 0, n1 * n2, n2, 1, P.ptr(o), P.ptr(w), P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    wide = P.make_spec([[("rbf", 32)]])           # a factor dim >= 32
    many = P.make_spec(c["spec"])
    many.n_comp = 17                              # outside every template bucket
    assert call(spec_=None, nb=0, p=None) == -1 and call(spec_=wide, q=40) == -1 and call(spec_=many) == -1
    assert call(nb=0, p=None) == -4 and call(Lc=0) == -4 and call(a=-1) == -4 and call(b=-1, g=None) == -4
    assert call(q=0) == -4 and call(q=6) == -4    # the spec reads column 6: Q >= 7
    assert call(p=None, g=None) == -8
    assert call(g=None, o=None) == -9
    assert call(o=None, w=None) == -13
    assert call(w=None) == -15
    assert U.all_sentinel(out) and U.tail_untouched(tail)
    assert call(b=0) == 0 and U.all_sentinel(out)
    assert call(a=0) == 0
    assert bool((out[:n] == 0).all()) and U.all_sentinel(out[n:]) and U.tail_untouched(tail)
    fresh = U.sentinel(n + Z.TAIL)                # Q = 7: a shorter dx2 row, the rest of the buffer untouched
    assert call(q=7, o=fresh) == 0 and U.all_sentinel(fresh[Lg * n2 * 7:])
    assert not bool(torch.isnan(fresh[:Lg * n2 * 7]).any())


# ------------------------------------------------------------------------------------------------------
# 2. DUBO dz
# ------------------------------------------------------------------------------------------------------
DUBO_CASES = ["1x4x3", "3x1x1", "6x7x33", "17x3x9", "4x32x17", "3x33x17", "9x16x120", "2x128x128"]


def _dz_check(got, ref, what, cid, bound=Z.BOUND):
    err = U.rel(got["dz"], ref["dz"])
    others = {k: U.rel(got[k], ref[k]) for k in got if k != "dz"}
    print(f"{what}: max |dz| {float(ref['dz'].abs().max()):.3e} dz err {err:.2e} cond(Kz) "
          + " ".join(f"{v:.1e}" for v in Z.cond_kz(cid)) + " | " + " ".join(f"{k} {v:.1e}" for k, v in others.items()))
    assert err < bound, (what, err, bound)


@pytest.mark.parametrize("cid", DUBO_CASES)
def test_dubo_dz_vs_oracle(hip, cid):
    """deviance_upper_bound_batched with z.requires_grad_() and a non-uniform cotangent against the oracle's dz;
    the columns of categorical factors and unread columns are exact zeros"""
    got, ref = Z.dubo_gpu(cid), Z.dubo_oracle(cid)
    assert got["dz"].shape == ref["dz"].shape == (L, D.CASES[cid][2], D.problem(cid)["X"].shape[1])
    _dz_check(got, ref, f"dubo dz {cid}", cid, Z.bound_for("dubo", cid))
    assert bool((got["dz"][..., 2:] == 0).all()) and bool((ref["dz"][..., 2:] == 0).all())


@pytest.mark.parametrize("form", ["shared", "list"])
def test_dubo_dz_z_forms(hip, form):
    """a shared [M, Q] z (autograd sums the dims' dz through the expand) and a per-dim list (through the stack)"""
    cid = "6x7x33"
    _dz_check(Z.dubo_gpu(cid, form), Z.dubo_oracle(cid, form), f"dubo dz {cid} {form}", cid,
              Z.bound_for("dubo", cid, form=form))


@pytest.mark.parametrize("cid", ["6x7x33", "3x33x17"])
def test_dubo_other_quantities_same_bits_with_and_without_dz(hip, cid):
    ones = (1.0, 1.0, 1.0)
    with_z, without = Z.dubo_gpu(cid, cot=ones), D.batched(cid)
    for k in D.QUANT:
        assert U.bit_equal(with_z[k], without[k]), k


# ------------------------------------------------------------------------------------------------------
# 3. ELBO dz
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,S", [("6x7x33", 1), ("6x7x33", 3), ("6x7x33", 16), ("6x7x33", 17), ("3x33x17", 3),
                                   ("9x16x120", 3), ("1x4x3", 16), ("17x3x9", 1)])
def test_elbo_dz_vs_oracle(hip, cid, S):
    """elbo_batched with z.requires_grad_() and gp_elbo_util's seeded non-uniform cotangents; S = 17 splits into two
    calls whose dz autograd adds"""
    got, ref = Z.elbo_gpu(cid, S), Z.elbo_oracle(cid, S)
    _dz_check(got, ref, f"elbo dz {cid} S={S}", cid, Z.bound_for("elbo", cid, S))
    assert bool((got["dz"][..., 2:] == 0).all())


@pytest.mark.parametrize("form", ["shared", "list"])
def test_elbo_dz_z_forms(hip, form):
    cid, S = "6x7x33", 3
    _dz_check(Z.elbo_gpu(cid, S, form), Z.elbo_oracle(cid, S, form), f"elbo dz {cid} S={S} {form}", cid,
              Z.bound_for("elbo", cid, S, form))


def test_elbo_other_quantities_same_bits_with_and_without_dz(hip):
    cid, S = "6x7x33", 3
    with_z, without = Z.elbo_gpu(cid, S), G.batched(cid, S)
    for k in G.QUANT:
        assert U.bit_equal(with_z[k], without[k]), k


# ------------------------------------------------------------------------------------------------------
# 4. Hensman dz
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ng", [True, False])
@pytest.mark.parametrize("cid", list(Z.HN_CASES))
def test_hensman_dz_vs_oracle(hip, cid, ng):
    """minibatch_KLD_upper_bound / _iter (the var- cases: unequal subject lengths, seg_len inside) with
    z.requires_grad_() and gkld = -2.5, both natural_gradient settings"""
    kld, dz, dp0 = Z.hn_gpu(cid, ng)
    kld_r, dz_r, dp0_r = Z.hn_oracle(cid)
    errs = (U.rel(kld, kld_r), U.rel(dz, dz_r), U.rel(dp0, dp0_r))
    print(f"hensman dz {cid} ng={ng}: max |dz| {float(dz_r.abs().max()):.3e} kld {errs[0]:.1e} dz {errs[1]:.2e} "
          f"draw0 {errs[2]:.1e}")
    assert errs[0] < 1e-8 and errs[1] < Z.BOUND
    assert bool((dz[..., 2:] == 0).all())   # (the reference split differentiates columns 0 and 1 alone)


def test_hensman_dz_shared_z(hip):
    kld, dz, _ = Z.hn_gpu("3x3x2", True, shared=True)
    _, dz_r, _ = Z.hn_oracle("3x3x2", shared=True)
    assert dz.shape == dz_r.shape == (3, U.QC) and U.rel(dz, dz_r) < Z.BOUND


# ------------------------------------------------------------------------------------------------------
# 5. the raw C ABI of the three _bwd_z calls
# ------------------------------------------------------------------------------------------------------
def _bwd_z_abi(hip, fn, spec0, dims, d, ws, wtail, Lh, M, N, Q, want, codes, rebuild, bound=Z.BOUND):
    """sentinels behind dz and both workspaces, the return codes in the header's order, equal bits from a second
    call on the same workspaces; `rebuild(**fields)` gives dims with fields replaced"""
    from lvae_amd import _lib as P
    st = P.stream_ptr()
    dz, n, zws, ztail = Z.dz_buffers(hip, Lh, M, N, Q)
    args = (P.ptr(d["x"]), P.ptr(d["z"]), P.ptr(d["p0"]))

    def call(s=spec0, dm=dims, o=dz, w=ws, zw=zws):
        rc = fn(None if s is None else ctypes.byref(s), None if dm is None else ctypes.byref(dm), *args, P.ptr(o),
                P.ptr(w), P.ptr(zw), st)
        torch.cuda.synchronize()
        return rc
    bad = P.make_spec([[("rbf", 0)]])
    bad.n_comp = 17
    wide = P.make_spec([[("rbf", Q)]])            # reads a column dz does not have
    assert call(s=None, dm=None) == -1 and call(s=bad, w=None) == -1
    assert call(dm=None, w=None) == -3 and call(dm=rebuild(M=129), zw=None) == -3 and call(dm=rebuild(L=0)) == -3
    assert call(s=wide, w=None) == -1
    assert call(w=None, zw=None) == codes[0] and call(w=ws[8:], zw=None) == codes[0]
    assert call(zw=None) == codes[1] and call(zw=zws[8:]) == codes[1]
    assert U.all_sentinel(dz) and U.tail_untouched(ztail) and U.tail_untouched(wtail)
    assert call() == 0
    assert U.all_sentinel(dz[n:]) and U.tail_untouched(ztail) and U.tail_untouched(wtail)
    first = dz[:n].reshape(Lh, M, Q).cpu()
    dz2 = U.sentinel(n + Z.TAIL)
    assert call(o=dz2) == 0 and U.bit_equal(dz2[:n].reshape(Lh, M, Q).cpu(), first)
    err = U.rel(first, want)
    print(f"{fn.__name__}: dz err {err:.2e}")
    assert bool(torch.isfinite(first).all()) and err < bound
    return first


def test_dubo_bwd_z_abi(hip):
    from lvae_amd import _lib as P
    cid = "6x7x33"
    c, s0, s1, dims, d = D.abi_inputs(cid)
    n, o = D.abi_outputs(c, s0, s1)
    ws, tail = U.workspace(hip.lvae_dubo_workspace_size(ctypes.byref(dims)))
    g = torch.tensor(Z.COT, dtype=torch.float64, device=DEV)
    common = (ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), P.ptr(d["x"]), P.ptr(d["z"]), P.ptr(d["mu"]),
              P.ptr(d["lv"]), P.ptr(d["p0"]), P.ptr(d["p1"]), P.ptr(d["noise"]))
    assert hip.lvae_dubo_fwd_f64(*common, P.ptr(o["dubo"]), None, P.ptr(ws), P.stream_ptr()) == 0
    assert hip.lvae_dubo_bwd_f64(*common, P.ptr(g), P.ptr(o["dmu"]), P.ptr(o["dlogv"]), P.ptr(o["dp0"]),
                                 P.ptr(o["dp1"]), P.ptr(o["dnoise"]), P.ptr(ws), P.stream_ptr()) == 0
    Q = c["X"].shape[1]

    def rebuild(**kw):
        f = dict(L=L, M=c["M"], P=c["P"], T=c["T"], Q=Q)
        f.update(kw)
        return P.DuboDims(f["L"], f["M"], f["P"], f["T"], f["Q"], D.EPS)
    _bwd_z_abi(hip, hip.lvae_dubo_bwd_z_f64, s0, dims, d, ws, tail, L, c["M"], c["N"], Q, Z.dubo_oracle(cid)["dz"],
               (-4, -5), rebuild, Z.bound_for("dubo", cid))


def test_gp_elbo_bwd_z_abi(hip):
    from lvae_amd import _lib as P
    cid, S = "6x7x33", 3
    c, s0, s1, dims, d = G.abi_inputs(cid, S)
    n, o = G.abi_outputs(c, s0, s1, S)
    ws, tail = U.workspace(hip.lvae_gp_elbo_workspace_size(ctypes.byref(dims)))
    g = G.samples(cid, S)[1].contiguous().to(DEV)
    common = (ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), P.ptr(d["x"]), P.ptr(d["z"]), P.ptr(d["y"]),
              P.ptr(d["p0"]), P.ptr(d["p1"]), P.ptr(d["noise"]))
    assert hip.lvae_gp_elbo_fwd_f64(*common, P.ptr(o["elbo"]), None, P.ptr(ws), P.stream_ptr()) == 0
    assert hip.lvae_gp_elbo_bwd_f64(*common, P.ptr(g), P.ptr(o["dy"]), P.ptr(o["dp0"]), P.ptr(o["dp1"]),
                                    P.ptr(o["dnoise"]), P.ptr(ws), P.stream_ptr()) == 0
    Q = c["X"].shape[1]
    assert hip.lvae_gp_elbo_bwd_z_f64(ctypes.byref(s0), ctypes.byref(G.make_dims(c, 17)), P.ptr(d["x"]),
                                      P.ptr(d["z"]), P.ptr(d["p0"]), None, None, None, P.stream_ptr()) == -3
    _bwd_z_abi(hip, hip.lvae_gp_elbo_bwd_z_f64, s0, dims, d, ws, tail, L, c["M"], c["N"], Q,
               Z.elbo_oracle(cid, S)["dz"], (-4, -5), lambda **kw: G.make_dims(c, S, **kw),
               Z.bound_for("elbo", cid, S))


@pytest.mark.parametrize("cid", ["var-17x5x4", "120x16"])
def test_hensman_bwd_z_abi(hip, cid):
    """the Hensman z-adjoint on the workspace of a forward + backward pair; with seg_len the padding rows of mu and
    logv hold NaN (the header allows anything there) and their covariates are another subject's: dz stays finite
    and equals the oracle's on the valid rows alone"""
    from lvae_amd import _lib as P
    c = Z.hn_problem(cid)
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    mu, lv = c["mu"].clone(), c["logv"].clone()
    seg_d = None
    if c["seg"] is not None:
        mu[~c["valid"]] = float("nan")
        lv[~c["valid"]] = float("nan")
        seg_d = torch.tensor(c["seg"], dtype=torch.int32, device=DEV)
    t = dict(x=c["x"], z=c["z"], m=c["m"], H=c["H"], mu=mu, lv=lv, p0=O.constrain(torch.tensor(c["raw0"])),
             p1=O.constrain(torch.tensor(c["raw1"])), noise=torch.tensor(c["noise"]))
    d = {k: v.to(DEV).contiguous() for k, v in t.items()}
    Lh, M, T, P_b, B = c["L"], c["M"], c["T"], c["P_b"], c["B"]
    P_in = P_b if c["seg"] is None else sum(1 for s in c["seg"] if s > 0)

    def rebuild(**kw):
        f = dict(L=Lh, M=M, P_b=P_b, T=T, Q=U.QC)
        f.update(kw)
        return P.HensmanDims(f["L"], f["M"], f["P_b"], f["T"], f["Q"], c["P_tot"] * P_b / P_in, Z.HN_EPS, 0, 1.0,
                             None if seg_d is None else seg_d.data_ptr(), 0.0 if seg_d is None else c["n_total"])
    dims = rebuild()
    ws, tail = U.workspace(hip.lvae_hensman_workspace_size(ctypes.byref(dims)))
    kld = U.sentinel(1)
    g = torch.tensor([-2.5], dtype=torch.float64, device=DEV)
    outs = {k: U.sentinel(v) for k, v in dict(dmu=B * Lh, dlv=B * Lh, dp0=Lh * s0.n_params, dp1=Lh * s1.n_params,
                                              dnz=Lh, dm=Lh * M, dH=Lh * M * M).items()}
    common = (ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), P.ptr(d["x"]), P.ptr(d["z"]), P.ptr(d["m"]),
              P.ptr(d["H"]), P.ptr(d["mu"]), P.ptr(d["lv"]), P.ptr(d["p0"]), P.ptr(d["p1"]), P.ptr(d["noise"]))
    assert hip.lvae_hensman_fwd_f64(*common, P.ptr(kld), None, None, None, P.ptr(ws), P.stream_ptr()) == 0
    assert hip.lvae_hensman_bwd_f64(*common, P.ptr(g), P.ptr(outs["dmu"]), P.ptr(outs["dlv"]), P.ptr(outs["dp0"]),
                                    P.ptr(outs["dp1"]), P.ptr(outs["dnz"]), P.ptr(outs["dm"]), P.ptr(outs["dH"]),
                                    P.ptr(ws), P.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert U.rel(kld.cpu(), Z.hn_oracle(cid)[0].reshape(1)) < 1e-8
    _bwd_z_abi(hip, hip.lvae_hensman_bwd_z_f64, s0, dims, d, ws, tail, Lh, M, B, U.QC, Z.hn_oracle(cid)[1],
               (-21, -22), rebuild)


# ------------------------------------------------------------------------------------------------------
# 6. DuboStep and ElboStep with z a parameter
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dubo", "elbo"])
def test_steps_train_z(hip, kind):
    """One step (P = 8, T = 8, L = 3, M = 12, 'mse') with z an nn.Parameter in the optimiser: after
    forward_backward z.grad matches the oracle's composition of the same step (test_dubo_step_vs_oracle's and
    test_elbo_step_vs_oracle's assembly, Z requiring grad), after apply z has moved by -lr z.grad."""
    import lvae_amd as la
    from lvae_amd.data import health_mnist_batch
    from lvae_amd.steps import DuboStep, ElboStep
    from lvae_amd.vae import ConvVAE
    Ls, P_, T, M, S, weight, lr = 3, 8, 8, 12, 2, 0.15, 0.05
    img, mask, X = health_mnist_batch(P_, T, seed=9, dtype=torch.float64)
    rng = np.random.default_rng(9)
    s0, s1 = O.spec_split(**D.CFG, id_covariate=2)
    raw0v = np.log(rng.uniform(0.5, 2.0, (Ls, O.n_params(s0))))
    raw1v = np.log(rng.uniform(0.5, 2.0, (Ls, O.n_params(s1))))
    Z0 = torch.stack([X[np.sort(np.random.default_rng(90 + l).choice(P_ * T, M, replace=False))] for l in range(Ls)])
    gen = torch.Generator().manual_seed(2)
    eps = torch.randn(P_ * T, Ls, generator=gen, dtype=torch.float64)
    eps_gp = torch.randn(S, P_ * T, Ls, generator=gen, dtype=torch.float64)
    # the oracle's step
    ref = O.ConvVAE(Ls).double()
    ref.load_state_dict(O.vae_weights(ref, 23))
    zr = Z0.clone().requires_grad_()
    mu, lv = ref.encode(img)
    recon = ref.decode(mu + eps * torch.exp(0.5 * lv))
    mse, _ = ref.loss_function(recon, img, mask)
    p0, p1 = O.constrain(torch.tensor(raw0v)), O.constrain(torch.tensor(raw1v))
    if kind == "dubo":
        gp = sum(O.deviance_upper_bound(s0, p0[l], s1, p1[l], 1.0, X, mu[:, l], lv[:, l], zr[l], P_, T, D.EPS)
                 for l in range(Ls))
    else:
        gp = 0.0
        for s in range(S):
            Zs = mu + eps_gp[s] * torch.exp(0.5 * lv)
            for l in range(Ls):
                gp = gp - O.gpapprox_elbo(s0, p0[l], s1, p1[l], 1.0, X, Zs[:, l], zr[l], P_, T, D.EPS)
        gp = gp / S
    (mse.sum() + weight * gp / Ls).backward()
    # the package's step
    vae = ConvVAE(Ls, 1296, p_input=0.0, p=0.0).double()
    vae.load_state_dict(ref.state_dict())
    vae = vae.float().to(DEV)
    k0, k1 = la.generate_kernel_batched(Ls, **D.CFG, id_covariate=2)
    D.set_raw(k0, raw0v)
    D.set_raw(k1, raw1v)
    k0, k1 = k0.to(DEV), k1.to(DEV)
    lik = la.GaussianLikelihood(Ls, noise=1.0).to(DEV)
    z = torch.nn.Parameter(Z0.clone().to(DEV))
    opt = torch.optim.SGD([dict(params=list(vae.parameters()) + list(k0.parameters()) + list(k1.parameters()),
                                lr=0.0), dict(params=[z], lr=lr)])
    inputs = [img.float().to(DEV), mask.float().to(DEV), X.to(DEV), eps.float().to(DEV)]
    if kind == "dubo":
        step = DuboStep(vae, k0, k1, lik, opt, z, T, weight=weight, loss_function="mse", eps=D.EPS)
    else:
        step = ElboStep(vae, k0, k1, lik, opt, z, T, weight=weight, loss_function="mse", eps=D.EPS, num_samples=S)
        inputs.append(eps_gp.float().to(DEV))
    step.forward_backward(*inputs)
    assert z.grad is not None and z.grad.shape == z.shape and z.grad.dtype == z.dtype
    grad = z.grad.detach().cpu().clone()
    err = U.rel(grad, zr.grad)
    print(f"{kind} step: max |z.grad| {float(zr.grad.abs().max()):.3e} err {err:.2e}")
    assert err < 1e-4
    step.communicate()
    step.apply()
    moved = z.detach().cpu()
    assert not torch.equal(moved, Z0)
    # (z <- z - lr z.grad in fp64: within 2 ulp of the largest |z| < 16)
    assert float((moved - (Z0 - lr * grad)).abs().max()) <= 2 * 2.0 ** -49
