"""lvae_predict_cov_f64, lvae_predict_exact_cov_f64 and lvae_predict_sample_f64 at the edges of their C ABI (their
values: test_gpu_predict_cov.py): every documented return code with all other arguments valid and nothing written,
the workspace-size queries against their documented formulas, and Nt = 0 / n_groups = 0 (info is written, the
outputs are untouched).  Follows test_gpu_predict_var_abi.py.
"""
import ctypes

import pytest
import torch

import abi_util as U
import test_predict_cov_oracle as C
import test_predict_var_oracle as V
from test_gpu_predict_cov import ind_args

gpu = pytest.mark.gpu
DEV = U.DEV
a256 = lambda b: (int(b) + 255) & ~255


@gpu
def test_inducing_cov_return_codes(hip):
    from lvae_amd import _lib as P
    cid = "ragged"
    c = C.ind_problem(cid)
    L, M, Pn, T, Nt, G = c["L"], c["M"], c["P"], c["T"], c["Nt"], len(c["group_subject"])
    good0, good1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    bad = P.KernelSpec.from_buffer_copy(good0)
    bad.n_comp = 17
    t = ind_args(cid)
    n_max = t["n_max"]
    out, cov, info = U.sentinel(Nt * L), U.sentinel(L * G * n_max * n_max), U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_cov_workspace_size(L, M, Pn, T, Nt))
    r = ctypes.byref

    def call(**kw):
        a = dict(s0=r(good0), s1=r(good1), L=L, M=M, Q=U.QC, P=Pn, T=T, seg=P.ptr(t["seg"]), inc=P.ptr(t["inc"]),
                 x=P.ptr(t["x"]), mu=P.ptr(t["mu"]), z=P.ptr(t["z"]), Nt=Nt, tx=P.ptr(t["tx"]), G=G,
                 gsub=P.ptr(t["gsub"]), gstart=P.ptr(t["gstart"]), n_max=n_max, p0=P.ptr(t["p0"]), p1=P.ptr(t["p1"]),
                 noise=P.ptr(t["noise"]), out=P.ptr(out), cov=P.ptr(cov), add_noise=0, ws=ws.data_ptr())
        a.update(kw)
        rc = hip.lvae_predict_cov_f64(a["s0"], a["s1"], a["L"], a["M"], a["Q"], a["P"], a["T"], a["seg"], a["inc"],
                                      a["x"], a["mu"], a["z"], a["Nt"], a["tx"], a["G"], a["gsub"], a["gstart"],
                                      a["n_max"], a["p0"], a["p1"], a["noise"], V.EPS, a["out"], a["cov"],
                                      a["add_noise"], P.ptr(info), a["ws"], P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    codes = [(dict(s0=None), -1), (dict(s1=None), -1), (dict(s0=r(bad)), -1), (dict(s1=r(bad)), -1),
             (dict(L=0), -3), (dict(L=65536), -3), (dict(M=0), -3), (dict(M=129), -3),
             (dict(P=0), -6), (dict(T=0), -6), (dict(T=129), -6), (dict(Q=0), -6),
             (dict(seg=None), -8), (dict(inc=None), -8), (dict(mu=None), -9), (dict(x=None), -10), (dict(z=None), -10),
             (dict(p0=None), -11), (dict(p1=None), -11), (dict(noise=None), -11), (dict(tx=None), -12),
             (dict(Nt=-1), -13), (dict(G=-1), -14), (dict(G=65536), -14), (dict(gsub=None), -15),
             (dict(gstart=None), -15), (dict(cov=None), -16), (dict(add_noise=2), -17), (dict(add_noise=-1), -17),
             (dict(n_max=0), -18), (dict(n_max=129), -18), (dict(ws=None), -20), (dict(ws=ws.data_ptr() + 8), -20),
             (dict(ws=ws.data_ptr() + 128), -20)]
    for kw, want in codes:
        assert call(**kw) == want, kw
    assert U.all_sentinel(out) and U.all_sentinel(cov) and U.all_sentinel(info) and bool((ws == 0x7F).all())
    assert hip.lvae_predict_cov_workspace_size(L, M, Pn, T, Nt) == hip.lvae_predict_var_workspace_size(L, M, Pn, T, Nt)
    assert call() == 0 and not U.all_sentinel(cov) and U.tail_untouched(tail)   # (nothing wrong: it runs)
    # n_groups = 0 with test rows: info and the mean are written, out_cov is untouched (n_max is then not read)
    cov.fill_(float("nan"))
    info.view(torch.uint8).fill_(0x7F)
    assert call(G=0, n_max=0, gsub=None, gstart=None, cov=None) == 0
    assert call(G=0, n_max=0) == 0 and U.all_sentinel(cov) and info.cpu().tolist() == [0] * L
    # Nt = 0: info is written, both outputs untouched
    out.fill_(float("nan"))
    info.view(torch.uint8).fill_(0x7F)
    assert call(Nt=0, tx=None, G=0) == 0 and U.all_sentinel(out) and U.all_sentinel(cov)
    assert info.cpu().tolist() == [0] * L


@gpu
def test_exact_cov_return_codes(hip):
    from lvae_amd import _lib as P
    c = V.exact_problem("n63")
    L, n, nt = c["L"], c["n"], c["nt"]
    groups = C.case_groups("exact", "n63")
    G, n_max = len(groups), max(len(g) for g in groups)
    order = torch.cat(groups)
    mk = lambda v: (ctypes.c_int32 * len(v))(*v)
    sizes = [len(g) for g in groups]
    start = mk([0] + [sum(sizes[:k + 1]) for k in range(G)])
    good = P.make_spec(c["spec"])
    bad = P.KernelSpec.from_buffer_copy(good)
    bad.n_comp = 17
    dv = lambda t: t.to(DEV).contiguous()
    x, tx, mu, params, nz = dv(c["x"]), dv(c["tx"][order]), dv(c["mu"]), dv(c["params"]), dv(c["noise"])
    out, cov, info = U.sentinel(nt * L), U.sentinel(L * G * n_max * n_max), U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_exact_cov_workspace_size(n, nt, L, 9))
    r = ctypes.byref
    vp = lambda arr: ctypes.cast(arr, ctypes.c_void_p)

    def call(**kw):
        a = dict(spec=r(good), x=P.ptr(x), ldx=U.QC, n=n, L=L, params=P.ptr(params), noise=P.ptr(nz), mu=P.ptr(mu),
                 ld_mu=L, tx=P.ptr(tx), ldt=U.QC, nt=nt, G=G, start=vp(start), n_max=n_max, out=P.ptr(out), ld_out=L,
                 cov=P.ptr(cov), add_noise=0, chunk=9, info=P.ptr(info), ws=ws.data_ptr())
        a.update(kw)
        rc = hip.lvae_predict_exact_cov_f64(a["spec"], a["x"], a["ldx"], a["n"], a["L"], a["params"], a["noise"],
                                            a["mu"], a["ld_mu"], a["tx"], a["ldt"], a["nt"], a["G"], a["start"],
                                            a["n_max"], a["out"], a["ld_out"], a["cov"], a["add_noise"], a["chunk"],
                                            a["info"], a["ws"], P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    ld_need = 1 + max(d for comp in c["spec"] for _, d in comp)
    shifted, long_, empty = list(start), list(start), list(start)
    shifted[0] = 1                       # does not begin at 0
    long_[1] = n_max + 1                 # a first group above n_max
    empty[2] = empty[1]                  # an empty group
    codes = [(dict(spec=None), -1), (dict(spec=r(bad)), -1), (dict(x=None), -2), (dict(ldx=ld_need - 1), -3),
             (dict(n=0), -4), (dict(L=0), -5), (dict(L=65536), -5), (dict(params=None), -6), (dict(noise=None), -7),
             (dict(mu=None), -8), (dict(ld_mu=L - 1), -9), (dict(tx=None), -10), (dict(ldt=ld_need - 1), -11),
             (dict(nt=-1), -12), (dict(ld_out=L - 1), -14), (dict(info=None), -15), (dict(ws=None), -16),
             (dict(ws=ws.data_ptr() + 8), -16), (dict(G=-1), -17), (dict(G=0), -17), (dict(G=65536), -17),
             (dict(nt=0, tx=None), -17), (dict(n_max=0), -18), (dict(n_max=129), -18), (dict(add_noise=2), -19),
             (dict(add_noise=-1), -19), (dict(chunk=n_max - 1), -20), (dict(chunk=0), -20), (dict(start=None), -21),
             (dict(start=vp(mk(shifted))), -22), (dict(start=vp(mk(long_))), -22), (dict(start=vp(mk(empty))), -22),
             (dict(G=G - 1), -22), (dict(cov=None), -23)]
    for kw, want in codes:
        assert call(**kw) == want, kw
    assert U.all_sentinel(out) and U.all_sentinel(cov) and U.all_sentinel(info) and bool((ws == 0x7F).all())
    size, base = hip.lvae_predict_exact_cov_workspace_size, hip.lvae_predict_exact_var_workspace_size
    assert size(0, nt, L, 9) == 0 and size(n, -1, L, 9) == 0 and size(n, nt, 0, 9) == 0 and size(n, nt, L, 0) == 0
    for nn, ch in ((n, 9), (n, nt), (n, nt + 100), (513, 5), (1200, 1)):
        cc, slabs = min(ch, nt), (nn + 511) // 512
        assert size(nn, nt, L, ch) == base(nn, nt, L, ch) + a256(2048 * L * cc * slabs), (nn, ch)
    assert call() == 0 and not U.all_sentinel(cov) and U.tail_untouched(tail)   # (nothing wrong: it runs)
    # nt = 0 (then n_groups = 0): the factor runs and info is written, nothing else is touched
    out.fill_(float("nan"))
    cov.fill_(float("nan"))
    info.view(torch.uint8).fill_(0x7F)
    assert call(nt=0, G=0, tx=None, start=None, cov=None, n_max=0, chunk=0) == 0
    assert U.all_sentinel(out) and U.all_sentinel(cov) and info.cpu().tolist() == [0] * L


@gpu
def test_sample_return_codes(hip):
    from lvae_amd import _lib as P
    L, G, n_max, Nt, S = 2, 3, 4, 7, 5
    gen = torch.Generator().manual_seed(9)
    A = torch.randn(L, G, n_max, n_max, generator=gen, dtype=torch.float64)
    blocks = (A @ A.transpose(2, 3) + torch.eye(n_max, dtype=torch.float64)).to(DEV).contiguous()
    index = torch.tensor([[5, 0, 3, -1], [1, -1, -1, -1], [2, 6, 4, -1]], dtype=torch.int32, device=DEV)
    mean = torch.randn(Nt, L, generator=gen, dtype=torch.float64).to(DEV)
    eps = torch.randn(S, Nt, L, generator=gen, dtype=torch.float64).to(DEV)
    out, info = U.sentinel(S * Nt * L + 7), U.sentinel(L * G, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_sample_workspace_size(L, G, n_max))

    def call(**kw):
        a = dict(L=L, G=G, n_max=n_max, Nt=Nt, S=S, cov=P.ptr(blocks), index=P.ptr(index), mean=P.ptr(mean),
                 eps=P.ptr(eps), jitter=0.0, out=P.ptr(out), info=P.ptr(info), ws=ws.data_ptr())
        a.update(kw)
        rc = hip.lvae_predict_sample_f64(a["L"], a["G"], a["n_max"], a["Nt"], a["S"], a["cov"], a["index"], a["mean"],
                                         a["eps"], a["jitter"], a["out"], a["info"], a["ws"], P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    codes = [(dict(L=0), -1), (dict(G=-1), -2), (dict(L=256, G=256), -2), (dict(n_max=0), -3), (dict(n_max=129), -3),
             (dict(Nt=-1), -4), (dict(Nt=G * n_max + 1), -4), (dict(G=0), -4), (dict(S=-1), -5), (dict(cov=None), -6),
             (dict(index=None), -7), (dict(mean=None), -8), (dict(eps=None), -9), (dict(jitter=-1e-9), -10),
             (dict(jitter=float("nan")), -10), (dict(out=None), -11), (dict(info=None), -12), (dict(ws=None), -13),
             (dict(ws=ws.data_ptr() + 8), -13)]
    for kw, want in codes:
        assert call(**kw) == want, kw
    assert U.all_sentinel(out) and U.all_sentinel(info) and bool((ws == 0x7F).all())
    size = hip.lvae_predict_sample_workspace_size
    assert size(0, G, n_max) == 0 and size(L, -1, n_max) == 0 and size(L, G, 0) == 0
    assert size(L, G, n_max) == a256(8 * L * G * n_max * n_max) + a256(8 * L * G)
    assert size(L, 0, n_max) == size(L, 1, n_max)
    # it runs: the draws are mean + chol(block) eps in the groups' row order, rows written exactly once
    assert call() == 0 and U.tail_untouched(tail) and info.cpu().tolist() == [0] * (L * G)
    assert U.all_sentinel(out[S * Nt * L:])
    got = out[:S * Nt * L].reshape(S, Nt, L).cpu()
    want = torch.empty(S, Nt, L, dtype=torch.float64)
    Lc = torch.linalg.cholesky(blocks.cpu())
    for g in range(G):
        rows = [int(i) for i in index[g].tolist() if i >= 0]
        for l in range(L):
            F = Lc[l, g, :len(rows), :len(rows)]
            want[:, rows, l] = mean.cpu()[rows, l] + eps.cpu()[:, rows, l] @ F.T
    assert U.rel(got, want) < 1e-13
    # S = 0 and Nt = 0: the factors run (info is written), out is untouched; n_groups = 0: nothing is touched
    out.fill_(float("nan"))
    info.view(torch.uint8).fill_(0x7F)
    assert call(S=0, mean=None, eps=None, out=None) == 0 and U.all_sentinel(out) and info.cpu().tolist() == [0] * (L * G)
    info.view(torch.uint8).fill_(0x7F)
    assert call(Nt=0, mean=None, eps=None, out=None) == 0 and U.all_sentinel(out) and info.cpu().tolist() == [0] * (L * G)
    info.view(torch.uint8).fill_(0x7F)
    assert call(G=0, Nt=0, cov=None, index=None, info=None) == 0 and U.all_sentinel(out) and U.all_sentinel(info)
    # a block that is not positive definite: info of that block alone, the other groups' draws keep their bits
    worse = blocks.clone()
    worse[1, 1, 0, 0] = -2.0
    assert call(cov=P.ptr(worse)) == 0
    assert info.cpu().tolist() == [0, 0, 0, 0, 1, 0]
    again = out[:S * Nt * L].reshape(S, Nt, L).cpu()
    keep = [0, 2, 3, 4, 5, 6]                                            # every row but group 1's row 1
    assert U.bit_equal(again[:, keep], got[:, keep]) and U.bit_equal(again[:, :, 0], got[:, :, 0])
