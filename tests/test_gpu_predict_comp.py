"""The per-component predictions end to end: lvae_predict_exact_comp_f64 and lvae_predict_comp_f64 through the C ABI,
and predict_exact_components / batch_predict_components / generate_component_sequences, against the component
oracles of predict_comp_util.py (O.gram of each one-component spec times the oracle's own alpha, b and mu~).

out and info must be the bits of lvae_predict_exact_f64 / lvae_predict_f64 (the same launches); out_comp is compared
over the whole [R, Nt, L] array by the project's rule, min(max(10 x yardstick, 2e-12), 1e-6), the yardstick being the
larger of the component oracle's change under a relative 2^-50 perturbation of hyper-parameters, noise and mu and
its CPU / device spread.

Exact-route cases: test_gpu_predict_exact_abi.problem()'s smallest, tile-edge, mix1, ext, few-rows (the slab path)
and no-test-rows.  Inducing-route cases (predict_comp_util.IND_CASES): M = 1, 3, 17 and 128, ragged subjects up to
64 rows with a one-row subject among them, test subjects inside and outside the prediction set, none inside (the k1
components are exact zeros) and no test rows.  Periodic and linear factors: the exact route on ext_util's ext-a as one
kernel (spec0 + spec1, 9 components: bucket (16, 4)), the inducing route on ext-a and ext-c (13 components), each
with 70 / 67 test rows (no multiple of 64) and a test subject outside the prediction set.

Measured on the MI355X (err and yardstick relative to max |oracle|; every bound is the 2e-12 floor but one):
    case                  err        yardstick   err / yardstick   bound
    exact smallest        6.45e-16   6.45e-16    1                 2.0e-12
    exact tile-edge       1.87e-14   5.81e-15    3.2               2.0e-12
    exact mix1            1.91e-14   1.09e-14    1.7               2.0e-12
    exact ext             1.75e-14   1.95e-14    0.9               2.0e-12
    exact few-rows        9.08e-15   4.41e-15    2.1               2.0e-12
    inducing smallest     8.67e-16   1.73e-15    0.5               2.0e-12
    inducing m3-mixed     7.02e-15   3.56e-15    2                 2.0e-12
    inducing m128-ragged  2.52e-13   2.34e-13    1.1               2.3e-12
    inducing none-incl.   5.78e-15   5.03e-15    1.1               2.0e-12
    inducing ref-ragged   3.36e-15   2.59e-15    1.3               2.0e-12
    exact ext-a           8.39e-15   1.31e-14    0.64              2.0e-12
    inducing ext-a        3.27e-15   2.54e-14    0.13              2.0e-12
    inducing ext-c        3.37e-15   7.23e-15    0.47              2.0e-12
The module's 24 tests take under 4 s.
"""
import ctypes

import numpy as np
import pytest
import torch

import abi_util as U
import predict_comp_util as C
import test_gpu_predict_exact_abi as E
from oracle import lvae_oracle as O

gpu = pytest.mark.gpu
DEV = U.DEV


def run_exact_comp(hip, cid, pad=3, noise=None):
    """One lvae_predict_exact_comp_f64 call on sentinel buffers, strides as E.run's plus ld_comp = L + pad + 1 and
    cstride_r = Nt ld_comp + 2 pad; returns (out [Nt, L], out_comp [R, Nt, L], info)"""
    from lvae_amd import _lib as P
    c = E.problem(cid)
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
    out = U.sentinel(max(Nt, 1) * ld_out + 7)
    comp = U.sentinel(R * cs + 7)
    info = U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_exact_comp_workspace_size(n, Nt, L, R))
    rc = hip.lvae_predict_exact_comp_f64(ctypes.byref(spec), P.ptr(xb), ldx, n, L, P.ptr(params), P.ptr(nz),
                                         P.ptr(mb), L + pad, P.ptr(tb) if Nt else None, ldx, Nt, P.ptr(out), ld_out,
                                         P.ptr(comp), ld_comp, cs, P.ptr(info), P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)
    assert U.untouched_outside(out, (Nt, L), (ld_out, 1))
    assert U.untouched_outside(comp, (R, Nt, L), (cs, ld_comp, 1))
    if not Nt:
        return torch.empty(0, L, dtype=torch.float64), torch.empty(R, 0, L, dtype=torch.float64), info.cpu().tolist()
    return (U.view(out, (Nt, L), (ld_out, 1)).cpu(), U.view(comp, (R, Nt, L), (cs, ld_comp, 1)).cpu(),
            info.cpu().tolist())


@gpu
@pytest.mark.parametrize("cid", C.EXACT_IDS)
def test_predict_exact_comp_abi(hip, cid):
    c = E.problem(cid)
    out, comp, info = run_exact_comp(hip, cid)
    plain, pinfo = E.run(hip, cid)
    assert info == pinfo == [0] * c["L"] and U.bit_equal(out, plain)       # lvae_predict_exact_f64's bits
    out0, comp0, _ = run_exact_comp(hip, cid, pad=0)
    assert U.bit_equal(out0, out) and U.bit_equal(comp0, comp)             # other strides: the same bits
    ref, ya = C.exact_ref(cid)
    if ref is None:
        assert comp.numel() == 0                                           # Nt = 0: nothing but info is written
        return
    yard = max(ya, U.rel(C.exact_oracle(cid, DEV), ref))
    err, tol = U.rel(comp, ref), C.bound(yard)
    print(f"predict_exact_comp {cid}: n {c['n']} R {len(c['spec'])} err {err:.2e} yardstick {yard:.2e} "
          f"ratio {err / max(yard, 1e-300):.2g} bound {tol:.1e}; |sum_r - out| {U.rel(comp.sum(0), out):.2e}")
    assert bool(torch.isfinite(comp).all())
    assert err <= tol
    assert U.rel(comp.sum(0), out) <= tol


@gpu
def test_predict_exact_comp_info(hip):
    """A dim whose noise makes K indefinite: info[l] > 0 for that dim only, the other dims' components keep their
    bits."""
    c = E.problem("mix1")
    _, good, info = run_exact_comp(hip, "mix1")
    assert info == [0, 0, 0]
    diag_max = float(O.gram(c["spec"], c["params"], c["x"], c["x"]).diagonal(dim1=-2, dim2=-1).max())
    bad = c["noise"].clone()
    bad[1] = -(diag_max + 1.0)
    _, got, info = run_exact_comp(hip, "mix1", noise=bad)
    assert info[0] == 0 and info[2] == 0 and info[1] == 1
    assert U.bit_equal(got[:, :, [0, 2]], good[:, :, [0, 2]])


def run_ind(hip, cid, comp=True, fill_seed=1, noise=None, pad=2):
    """lvae_predict_comp_f64 (comp) or lvae_predict_f64 on the problem; (out [Nt, L], out_comp [R, Nt, L] or None,
    info)"""
    from lvae_amd import _lib as P
    c = C.ind_problem(cid)
    L, M, Pn, T, Nt = c["L"], c["M"], c["P"], c["T"], c["Nt"]
    R0, R1 = len(c["s0"]), len(c["s1"])
    R = R0 + R1
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    other = U.subject_covariates(np.random.default_rng(fill_seed), Pn, T).reshape(c["NP"], U.QC)
    x = torch.where(c["valid"][:, None], c["x"], other)   # padding rows of x: any finite covariates
    dv = lambda t: t.to(DEV).contiguous()
    xd, z, mu, tx, p0, p1 = dv(x), dv(c["z"]), dv(c["mu"]), dv(c["tx"]), dv(c["p0"]), dv(c["p1"])
    nz = dv(c["noise"] if noise is None else noise)
    seg, inc = torch.tensor(c["seg"], dtype=torch.int32, device=DEV), dv(c["include"])
    out = U.sentinel(max(Nt, 1) * L + 7)
    info = U.sentinel(L, torch.int32)
    r = ctypes.byref
    if not comp:
        ws, tail = U.workspace(hip.lvae_predict_workspace_size(L, M, Pn, T, Nt))
        rc = hip.lvae_predict_f64(r(s0), r(s1), L, M, U.QC, Pn, T, P.ptr(seg), P.ptr(inc), P.ptr(xd), P.ptr(mu),
                                  P.ptr(z), Nt, P.ptr(tx) if Nt else None, P.ptr(p0), P.ptr(p1), P.ptr(nz), C.EPS,
                                  P.ptr(out), P.ptr(info), P.ptr(ws), P.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and U.tail_untouched(tail)
        return out[:Nt * L].reshape(Nt, L).cpu(), None, info.cpu().tolist()
    ld_comp = L + pad
    cs = max(Nt, 1) * ld_comp + 3 * pad
    cbuf = U.sentinel(R * cs + 7)
    ws, tail = U.workspace(hip.lvae_predict_comp_workspace_size(L, M, Pn, T, Nt, R0, R1))
    rc = hip.lvae_predict_comp_f64(r(s0), r(s1), L, M, U.QC, Pn, T, P.ptr(seg), P.ptr(inc), P.ptr(xd), P.ptr(mu),
                                   P.ptr(z), Nt, P.ptr(tx) if Nt else None, P.ptr(p0), P.ptr(p1), P.ptr(nz), C.EPS,
                                   P.ptr(out), P.ptr(cbuf), ld_comp, cs, P.ptr(info), P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)
    assert U.all_sentinel(out[Nt * L:])
    assert U.untouched_outside(cbuf, (R, Nt, L), (cs, ld_comp, 1))
    got = U.view(cbuf, (R, Nt, L), (cs, ld_comp, 1)).cpu() if Nt else torch.empty(R, 0, L, dtype=torch.float64)
    return out[:Nt * L].reshape(Nt, L).cpu(), got, info.cpu().tolist()


@gpu
@pytest.mark.parametrize("cid", C.IND_IDS)
def test_predict_comp_abi(hip, cid):
    c = C.ind_problem(cid)
    out, comp, info = run_ind(hip, cid)
    plain, _, pinfo = run_ind(hip, cid, comp=False)
    assert info == pinfo == [0] * c["L"] and U.bit_equal(out, plain)       # lvae_predict_f64's bits
    out2, comp2, _ = run_ind(hip, cid, fill_seed=2, pad=0)
    assert U.bit_equal(out2, out) and U.bit_equal(comp2, comp)             # other padding rows and strides
    ref, ya = C.ind_ref(cid)
    if ref is None:
        assert comp.numel() == 0
        return
    yard = max(ya, U.rel(C.ind_oracle(cid, DEV), ref))
    err, tol = U.rel(comp, ref), C.bound(yard)
    print(f"predict_comp {cid}: M {c['M']} R {ref.shape[0]} err {err:.2e} yardstick {yard:.2e} "
          f"ratio {err / max(yard, 1e-300):.2g} bound {tol:.1e}; |sum_r - out| {U.rel(comp.sum(0), out):.2e}")
    assert bool(torch.isfinite(comp).all())
    assert err <= tol
    assert U.rel(comp.sum(0), out) <= tol
    if cid == "none-included":
        assert bool((comp[len(c["s0"]):] == 0.0).all())                   # no included subject: exact zeros


@gpu
def test_predict_comp_info(hip):
    """A dim whose noise makes every B_p indefinite: info[l] = 20001 for that dim only, the other dims' components
    keep their bits."""
    c = C.ind_problem("m3-mixed")
    _, good, info = run_ind(hip, "m3-mixed")
    assert info == [0, 0, 0]
    bad = c["noise"].clone()
    bad[1] = -100.0
    _, got, info = run_ind(hip, "m3-mixed", noise=bad)
    assert info == [0, 20001, 0]
    assert U.bit_equal(got[:, :, [0, 2]], good[:, :, [0, 2]])


@gpu
def test_predict_comp_return_codes(hip):
    """The codes the two predictor entry points add to those of the functions they mirror (pinned in
    test_gpu_predict_exact_abi.py and test_gpu_predict_abi.py), the shared ones in the same place, each rejected
    before any launch: nothing is written."""
    from lvae_amd import _lib as P
    r = ctypes.byref
    dv = lambda t: t.to(DEV).contiguous()
    # exact route
    c = E.problem("tile-edge")
    L, n, Nt, R = c["L"], c["n"], c["Nt"], len(c["spec"])
    good = P.make_spec(c["spec"])
    far = P.KernelSpec.from_buffer_copy(good)
    far.dim[0][0] = 32
    x, tx, mu, params, nz = dv(c["x"]), dv(c["tx"]), dv(c["mu"]), dv(c["params"]), dv(c["noise"])
    out, comp, info = U.sentinel(Nt * L), U.sentinel(R * Nt * L), U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_exact_comp_workspace_size(n, Nt, L, R))

    def pe(**kw):
        a = dict(spec=r(good), x=P.ptr(x), ldx=U.QC, n=n, L=L, params=P.ptr(params), noise=P.ptr(nz), mu=P.ptr(mu),
                 ld_mu=L, tx=P.ptr(tx), ldt=U.QC, nt=Nt, out=P.ptr(out), ld_out=L, comp=P.ptr(comp), ld_comp=L,
                 cs=Nt * L, info=P.ptr(info), ws=ws.data_ptr())
        a.update(kw)
        rc = hip.lvae_predict_exact_comp_f64(a["spec"], a["x"], a["ldx"], a["n"], a["L"], a["params"], a["noise"],
                                             a["mu"], a["ld_mu"], a["tx"], a["ldt"], a["nt"], a["out"], a["ld_out"],
                                             a["comp"], a["ld_comp"], a["cs"], a["info"], a["ws"], P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    ld_need = 1 + max(d for cp in c["spec"] for _, d in cp)
    codes = [(dict(spec=None), -1), (dict(spec=r(far)), -1), (dict(x=None), -2), (dict(ldx=ld_need - 1), -3),
             (dict(n=0), -4), (dict(L=0), -5), (dict(params=None), -6), (dict(noise=None), -7), (dict(mu=None), -8),
             (dict(ld_mu=L - 1), -9), (dict(tx=None), -10), (dict(ldt=ld_need - 1), -11), (dict(nt=-1), -12),
             (dict(out=None), -13), (dict(ld_out=L - 1), -14), (dict(info=None), -15), (dict(ws=None), -16),
             (dict(ws=ws.data_ptr() + 8), -16), (dict(comp=None), -17), (dict(ld_comp=L - 1), -18),
             (dict(cs=Nt * L - 1), -19), (dict(cs=-1), -19), (dict(comp=None, ws=None), -16),
             (dict(comp=None, ld_comp=0, cs=0), -17), (dict(ld_comp=0, cs=0), -18)]
    for kw, want in codes:
        assert pe(**kw) == want, kw
    assert U.all_sentinel(out) and U.all_sentinel(comp) and U.all_sentinel(info) and bool((ws == 0x7F).all())
    assert pe(nt=0, tx=None, out=None, comp=None, ld_comp=0, cs=0) == 0    # no test rows: none of them is looked at
    assert U.all_sentinel(out) and U.all_sentinel(comp) and not U.all_sentinel(info)
    assert pe() == 0 and not U.all_sentinel(comp) and U.tail_untouched(tail)
    # inducing route
    c = C.ind_problem("m3-mixed")
    L, M, Pn, T, Nt = c["L"], c["M"], c["P"], c["T"], c["Nt"]
    R0, R1 = len(c["s0"]), len(c["s1"])
    g0, g1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    bad = P.KernelSpec.from_buffer_copy(g0)
    bad.n_comp = 17
    far = P.KernelSpec.from_buffer_copy(g1)
    far.dim[0][0] = 32
    x, z, mu, tx, p0, p1, nz = (dv(c[k]) for k in ("x", "z", "mu", "tx", "p0", "p1", "noise"))
    seg, inc = torch.tensor(c["seg"], dtype=torch.int32, device=DEV), dv(c["include"])
    out, comp, info = U.sentinel(Nt * L), U.sentinel((R0 + R1) * Nt * L), U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_comp_workspace_size(L, M, Pn, T, Nt, R0, R1))

    def call(**kw):
        a = dict(s0=r(g0), s1=r(g1), L=L, M=M, Q=U.QC, P=Pn, T=T, seg=P.ptr(seg), inc=P.ptr(inc), Nt=Nt,
                 comp=P.ptr(comp), ld_comp=L, cs=Nt * L, ws=ws.data_ptr())
        a.update(kw)
        rc = hip.lvae_predict_comp_f64(a["s0"], a["s1"], a["L"], a["M"], a["Q"], a["P"], a["T"], a["seg"], a["inc"],
                                       P.ptr(x), P.ptr(mu), P.ptr(z), a["Nt"], P.ptr(tx), P.ptr(p0), P.ptr(p1),
                                       P.ptr(nz), C.EPS, P.ptr(out), a["comp"], a["ld_comp"], a["cs"], P.ptr(info),
                                       a["ws"], P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    q_need = 1 + max(d for cp in c["s0"] + c["s1"] for _, d in cp)
    codes = [(dict(s0=None), -1), (dict(s1=None), -1), (dict(s0=r(bad)), -1), (dict(s1=r(far)), -1), (dict(L=0), -3),
             (dict(M=0), -3), (dict(M=129), -3), (dict(P=0), -6), (dict(T=0), -6), (dict(T=129), -6), (dict(Q=0), -6),
             (dict(Q=q_need - 1), -6), (dict(seg=None), -8), (dict(inc=None), -8), (dict(Nt=-1), -13),
             (dict(ws=None), -20), (dict(ws=ws.data_ptr() + 8), -20), (dict(ws=ws.data_ptr() + 128), -20),
             (dict(comp=None), -21), (dict(ld_comp=L - 1), -22), (dict(cs=Nt * L - 1), -23), (dict(cs=0), -23),
             (dict(comp=None, ws=None), -20), (dict(comp=None, ld_comp=0, cs=0), -21), (dict(ld_comp=0, cs=0), -22)]
    for kw, want in codes:
        assert call(**kw) == want, kw
    assert U.all_sentinel(out) and U.all_sentinel(comp) and U.all_sentinel(info) and bool((ws == 0x7F).all())
    assert call() == 0 and not U.all_sentinel(comp) and U.tail_untouched(tail)


# ---- the Python functions ----
def ref_kernels(L, seed):
    """The reference split's two kernels (abi_util._REF_CFG) as the project's batched modules on the device, raw
    parameters drawn at random; returns (k0, k1, params0 [L, P0], params1 [L, P1]) with the constrained parameters
    in spec order on the CPU"""
    import lvae_amd as la
    k0, k1 = la.generate_kernel_batched(L, **U._REF_CFG, id_covariate=U.ID_COL)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k in (k0, k1):
            for p in k.parameters():
                p.add_(0.4 * torch.randn(p.shape, generator=gen, dtype=torch.float64).to(p.dtype))
    k0, k1 = k0.double().to(DEV), k1.double().to(DEV)
    (s0, p0), (s1, p1) = la.kernel_spec_and_params(k0), la.kernel_spec_and_params(k1)
    from lvae_amd import _lib as P
    w0, w1 = U.spec_pairs()["ref"]
    assert bytes(s0) == bytes(P.make_spec(w0)) and bytes(s1) == bytes(P.make_spec(w1))
    return k0, k1, p0.detach().cpu(), p1.detach().cpu()


def per_dim(k, L, build):
    """The batched module k as a list of L one-dim modules with the same parameters"""
    out = []
    for l in range(L):
        m = build().double().to(DEV)
        with torch.no_grad():
            for (_, pb), (_, p1) in zip(k.named_parameters(), m.named_parameters()):
                p1.copy_(pb[l:l + 1])
        out.append(m)
    return out


def liks(noise, batched):
    import lvae_amd as la
    if not batched:
        return [la.GaussianLikelihood(1, noise=float(v)).to(DEV) for v in noise]

    class Lik:   # a batched likelihood: .noise [L]
        def eval(self):
            return self
    Lik.noise = noise.to(DEV)
    return Lik()


@gpu
@pytest.mark.parametrize("batched", [True, False])
def test_predict_exact_components(hip, batched):
    import lvae_amd as la
    c = E.problem("tile-edge")
    L = c["L"]
    k0, k1, p0, p1 = ref_kernels(L, 11)
    w0, w1 = U.spec_pairs()["ref"]
    spec, params = w0 + w1, torch.cat([p0, p1], 1)
    k = k0 + k1
    if not batched:
        def one():
            a, b = la.generate_kernel_batched(1, **U._REF_CFG, id_covariate=U.ID_COL)
            return a + b
        k = per_dim(k, L, one)
    lik = liks(c["noise"], batched)
    X, tx, mu = c["x"].to(DEV), c["tx"].to(DEV), c["mu"].to(DEV)
    z_pred, comps = la.predict_exact_components(k, lik, X, tx, mu)
    assert U.bit_equal(z_pred, la.predict_exact(k, lik, X, tx, mu))
    assert comps.values.shape == (len(spec), c["Nt"], L) and comps.values.dtype == torch.float64
    assert comps.labels == C.labels(spec) and comps.module == [0] * len(spec)
    oracle = lambda dev, pert=False: C.exact_components(
        spec, *[(U.perturbed(t, torch.Generator().manual_seed(81 + i)) if pert else t).to(dev)
                for i, t in enumerate((params, c["noise"]))], c["x"].to(dev), c["tx"].to(dev),
        (U.perturbed(c["mu"], torch.Generator().manual_seed(83)) if pert else c["mu"]).to(dev)).cpu()
    ref = oracle("cpu")
    yard = max(U.rel(oracle("cpu", True), ref), U.rel(oracle(DEV), ref))
    err, tol = U.rel(comps.values, ref), C.bound(yard)
    print(f"predict_exact_components batched={batched}: err {err:.2e} yardstick {yard:.2e} bound {tol:.1e}")
    assert err <= tol and U.rel(comps.total(), z_pred) <= tol
    ev = comps.explained_variance()
    assert ev.shape == (len(spec), L) and bool(((ev.sum(0) - 1.0).abs() < 1e-12).all())
    if batched:   # two dim groups under a cap that holds one dim's workspace but not two: the same bits
        size = lambda g: int(hip.lvae_predict_exact_comp_workspace_size(c["n"], c["Nt"], g, len(spec)))
        assert size(1) < size(2)
        z2, c2 = la.predict_exact_components(k, lik, X, tx, mu, max_workspace_bytes=size(1))
        assert U.bit_equal(z2, z_pred) and U.bit_equal(c2.values, comps.values)


@gpu
@pytest.mark.parametrize("batched", [True, False])
def test_batch_predict_components(hip, batched):
    import lvae_amd as la
    c = C.ind_problem("ref-ragged")
    L, ok = c["L"], c["valid"]
    k0, k1, p0, p1 = ref_kernels(L, 12)
    if not batched:
        k0 = per_dim(k0, L, lambda: la.generate_kernel_batched(1, **U._REF_CFG, id_covariate=U.ID_COL)[0])
        k1 = per_dim(k1, L, lambda: la.generate_kernel_batched(1, **U._REF_CFG, id_covariate=U.ID_COL)[1])
    lik = liks(c["noise"], batched)
    X, tx, mu = c["x"][ok].to(DEV), c["tx"].to(DEV), c["mu"][ok].to(DEV)
    z = c["z"].to(DEV) if batched else [zl.to(DEV) for zl in c["z"]]
    z_pred, comps = la.batch_predict_components(L, k0, k1, lik, X, tx, mu, z, U.ID_COL, C.EPS)
    assert U.bit_equal(z_pred, la.batch_predict_varying_T(L, k0, k1, lik, X, tx, mu, z, U.ID_COL, C.EPS))
    R0, R1 = len(c["s0"]), len(c["s1"])
    assert comps.values.shape == (R0 + R1, c["Nt"], L)
    assert comps.labels == C.labels(c["s0"]) + C.labels(c["s1"]) and comps.module == [0] * R0 + [1] * R1

    def oracle(dev, pert=False):
        v = [p0, p1, c["noise"], c["mu"]]
        if pert:
            v = [U.perturbed(t, torch.Generator().manual_seed(84 + i)) for i, t in enumerate(v)]
        v = [t.to(dev) for t in v]
        return C.inducing_components(c["s0"], v[0], c["s1"], v[1], v[2], c["x"][ok].to(dev), c["tx"].to(dev),
                                     v[3][ok.to(dev)], c["z"].to(dev), U.ID_COL, C.EPS).cpu()
    ref = oracle("cpu")
    yard = max(U.rel(oracle("cpu", True), ref), U.rel(oracle(DEV), ref))
    err, tol = U.rel(comps.values, ref), C.bound(yard)
    print(f"batch_predict_components batched={batched}: err {err:.2e} yardstick {yard:.2e} bound {tol:.1e}")
    assert err <= tol and U.rel(comps.total(), z_pred) <= tol


@gpu
@pytest.mark.parametrize("model", ["simple", "conv"])
def test_generate_component_sequences(hip, model):
    """Entry r decodes the first r + 1 components' sum; the last entry of the full order is decode(total()), bit
    for bit, for both VAEs"""
    import lvae_amd as la
    from lvae_amd.predict import LatentComponents
    torch.manual_seed(3)
    L, Nt = 4, 6
    vae = (la.SimpleVAE(L, 36) if model == "simple" else la.ConvVAE(L)).to(DEV).eval()
    vals = torch.randn(3, Nt, L, dtype=torch.float64, device=DEV)
    comps = LatentComponents(vals, ["a", "b", "c"], [0, 0, 1])
    seq = la.generate_component_sequences(vae, comps)
    with torch.no_grad():
        assert seq.shape[:2] == (3, Nt) and not seq.requires_grad
        assert U.bit_equal(seq[-1], vae.decode(comps.total().to(torch.float32)))
        assert U.bit_equal(seq[0], vae.decode(vals[0].to(torch.float32)))
        rev = la.generate_component_sequences(vae, comps, order=[2, 1, 0])
        assert U.bit_equal(rev[0], vae.decode(vals[2].to(torch.float32))) and rev.shape == seq.shape
