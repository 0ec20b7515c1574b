"""lvae_predict_f64 through the C ABI against the fp64 oracle on the CPU (O.batch_predict_varying_T), with the spec
pairs, hyper-parameters and jitter (eps = 1e-3) of test_gpu_hensman_abi.py: prediction subjects of ragged length
(a one-row subject among them), test rows of subjects inside and outside the prediction set, no test rows at all,
no included subject at all, and the one shape at which the chunk loop over the test rows runs twice
(L P T Nt > 2^24, the second chunk shorter: its results land at out1 + r0).

Tolerance: as in test_gpu_hensman_abi.py, max(10 x yardstick, 2e-12) capped at 1e-6, the yardstick being the larger
of the oracle's change under a relative 2^-50 perturbation of hyper-parameters, noise and mu and the CPU / device
spread of the oracle.

Measured on the MI355X (yardstick = max of the two figures above, bound = max(10 x yardstick, 2e-12)):
    case            kernel err   yardstick   err / yardstick   bound
    smallest        0            9.89e-16    0                 2.0e-12
    mixed-include   2.50e-15     3.17e-15    0.79              2.0e-12
    limits          8.73e-14     5.55e-14    1.6               2.0e-12
    none-included   4.54e-14     2.79e-14    1.6               2.0e-12
    chunked         2.61e-13     9.29e-14    2.8               2.0e-12
    ext-b           9.63e-15     2.22e-14    0.43              2.0e-12   (ext_util's ext-b: per / lin in both kernels)
Before lvae_predict_f64 refined its two products with explicit inverses (H^-1 w, K0zz^-1 a; cond ~1e5 at
eps = 1e-3) by one residual step, "limits" measured 4.59e-12 (83 x its yardstick) and "none-included" 4.33e-12
(160 x): beyond the bound, where the oracle's solves are not.  The chunked case (workspace ~130 MiB, 7711 test rows
against 2176 prediction rows) takes about 0.3 s as a test (its first lvae_predict_f64 call with the copies in and out: 8.8 ms); the module's
8 tests take under 1 s, the two modules about 5 s together.
"""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

import abi_util as U
import ext_util
from oracle import lvae_oracle as O

gpu = pytest.mark.gpu
DEV = U.DEV
PAIRS = ext_util.all_spec_pairs()
EPS = 1e-3

# id: (pair, L, M, P, T, Nt, seg_len, subject ids of the test rows (cycled over the rows))
CASES = {
    "smallest": ("ref", 2, 1, 1, 1, 1, (1,), (0,)),
    "mixed-include": ("mix1", 3, 17, 4, 17, 9, (17, 1, 9, 16), (2, 0, 7)),      # 7: not a prediction subject
    "limits": ("mix2", 2, 128, 2, 128, 5, (128, 1), (1, 0)),
    "no-test-rows": ("ref", 2, 33, 5, 16, 0, (16, 1, 7, 12, 16), ()),
    "none-included": ("mix1", 2, 33, 5, 16, 7, (16, 1, 7, 12, 16), (9, 11)),    # the k1 term vanishes
    "chunked": ("mix2", 1, 16, 17, 128, 7711, tuple([128, 1, 77] + [128 - 7 * p for p in range(14)]),
                tuple(range(0, 20, 2))),
    # periodic and linear factors in both kernels, a (16, 4) id kernel, Nt not a multiple of 64
    "ext-b": ("ext-b", 3, 17, 4, 17, 70, (17, 1, 9, 16), (2, 0, 7)),
}
CASE_IDS = list(CASES)


@functools.lru_cache(maxsize=None)
def problem(cid):
    pair, L, M, Pn, T, Nt, seg, tids = CASES[cid]
    s0, s1 = PAIRS[pair]
    rng = np.random.default_rng(3000 + CASE_IDS.index(cid))
    gen = torch.Generator().manual_seed(4000 + CASE_IDS.index(cid))
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


def oracle(cid, dev="cpu", perturb=False):
    c = problem(cid)
    if c["Nt"] == 0:
        return None
    v = {k: c[k] for k in ("p0", "p1", "noise", "mu")}
    if perturb:
        gen = torch.Generator().manual_seed(78)
        v = {k: U.perturbed(t, gen) for k, t in v.items()}
    ok = c["valid"]
    v = {k: t.to(dev) for k, t in v.items()}
    return O.batch_predict_varying_T(c["s0"], v["p0"], c["s1"], v["p1"], v["noise"], c["x"][ok].to(dev),
                                     c["tx"].to(dev), v["mu"][ok.to(dev)], c["z"].to(dev), U.ID_COL, EPS).cpu()


@functools.lru_cache(maxsize=None)
def cpu_ref(cid):
    """(oracle, yardstick (a)) on the CPU; (None, 0) without test rows"""
    ref = oracle(cid)
    return (None, 0.0) if ref is None else (ref, U.rel(oracle(cid, perturb=True), ref))


def chunk_rows(lib, L, M, Pn, T):
    """Test rows per k1(X*, x) chunk, read off the library's own workspace sizes: the K1 block grows by
    L P T doubles per test row up to that many rows, and not at all beyond."""
    size = lambda nt: int(lib.lvae_predict_workspace_size(L, M, Pn, T, nt))
    step = 8 * L * Pn * T
    lo, hi = 1, 1 << 26   # size(n + 1) - size(n) >= step iff n < rows
    assert size(lo + 1) - size(lo) >= step > size(hi + 1) - size(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if size(mid + 1) - size(mid) >= step:
            lo = mid
        else:
            hi = mid
    return hi


def run(hip, cid, fill_seed=1, want_info=True):
    from lvae_amd import _lib as P
    c = problem(cid)
    L, M, Pn, T, Nt = c["L"], c["M"], c["P"], c["T"], c["Nt"]
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    other = U.subject_covariates(np.random.default_rng(fill_seed), Pn, T).reshape(c["NP"], U.QC)
    x = torch.where(c["valid"][:, None], c["x"], other)   # padding rows of x: any finite covariates
    dv = lambda t: t.to(DEV).contiguous()
    xd, z, mu, tx, p0, p1, nz = dv(x), dv(c["z"]), dv(c["mu"]), dv(c["tx"]), dv(c["p0"]), dv(c["p1"]), dv(c["noise"])
    seg, inc = torch.tensor(c["seg"], dtype=torch.int32, device=DEV), dv(c["include"])
    out = U.sentinel(max(Nt, 1) * L + 7)
    info = U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_workspace_size(L, M, Pn, T, Nt))
    rc = hip.lvae_predict_f64(ctypes.byref(s0), ctypes.byref(s1), L, M, U.QC, Pn, T, P.ptr(seg), P.ptr(inc), P.ptr(xd),
                              P.ptr(mu), P.ptr(z), Nt, P.ptr(tx) if Nt else None, P.ptr(p0), P.ptr(p1), P.ptr(nz), EPS,
                              P.ptr(out), P.ptr(info) if want_info else None, P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)               # lvae_predict_workspace_size bytes are enough
    assert U.all_sentinel(out[Nt * L:])         # out [Nt, L] and nothing after it
    assert info.cpu().tolist() == [0] * L if want_info else U.all_sentinel(info)
    return out[:Nt * L].reshape(Nt, L).cpu()


@gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_predict_values(hip, cid):
    c = problem(cid)
    t0 = time.perf_counter()
    got = run(hip, cid)
    t_kernel = time.perf_counter() - t0
    again = run(hip, cid, fill_seed=2)
    assert U.bit_equal(got, again)               # another fill of x's padding rows: the same bits
    assert U.bit_equal(got, run(hip, cid, want_info=False))
    ref, ya = cpu_ref(cid)
    if ref is None:
        assert got.numel() == 0                  # Nt = 0: rc 0, info written, out untouched (checked in run)
        return
    yard = max(ya, U.rel(oracle(cid, DEV), ref))
    err, tol = U.rel(got, ref), min(max(10.0 * yard, 2e-12), 1e-6)
    print(f"predict {cid}: err {err:.2e} yardstick {yard:.2e} ratio {err / max(yard, 1e-300):.2g} bound {tol:.1e} "
          f"(call + copies {1e3 * t_kernel:.1f} ms)")
    assert bool(torch.isfinite(got).all())
    assert err <= tol
    assert bool(c["include"].any()) == (cid != "none-included") and float(ref.abs().max()) > 0


@gpu
def test_predict_info_codes(hip):
    """info[l] = 10000 / 20000 + the failing column of K0zz / B_p (which H = K0zz + K0xz^T B^-1 K0xz then follows:
    the first failure in the order K0zz, B_p, H is the one reported); dim 1 only is indefinite by construction."""
    from lvae_amd import _lib as P
    c = U.info_problem()
    L, M, T, Pn, Nt = c["L"], c["M"], c["T"], c["P_b"], 4
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    dv = lambda t: t.to(DEV).contiguous()
    x, z, p0, p1 = dv(c["x"]), dv(c["z"]), dv(c["p0"]), dv(c["p1"])
    tx = dv(c["x"][:Nt])
    mu = torch.ones(Pn * T, L, dtype=torch.float64, device=DEV)
    seg = torch.tensor([T, T], dtype=torch.int32, device=DEV)
    inc = torch.ones(Pn, dtype=torch.int32, device=DEV)
    ws, tail = U.workspace(hip.lvae_predict_workspace_size(L, M, Pn, T, Nt))

    def info_of(eps, noise):
        out, info = U.sentinel(Nt * L), U.sentinel(L, torch.int32)
        nz = dv(noise)
        rc = hip.lvae_predict_f64(ctypes.byref(s0), ctypes.byref(s1), L, M, U.QC, Pn, T, P.ptr(seg), P.ptr(inc), P.ptr(x),
                                  P.ptr(mu), P.ptr(z), Nt, P.ptr(tx), P.ptr(p0), P.ptr(p1), P.ptr(nz), eps, P.ptr(out),
                                  P.ptr(info), P.ptr(ws), P.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and U.tail_untouched(tail)
        return info.cpu().tolist()
    good = torch.ones(L, dtype=torch.float64)
    bad = good.clone()
    bad[1] = -(2 * 0.5 + 1.0)   # B_p[1] has the diagonal 1 - 2
    assert info_of(EPS, good) == [0, 0, 0]
    assert info_of(-3.0, good) == [0, 10001, 0]   # K0zz[1] = 1.5 I - 3 I (dims 0, 2: 6 I - 3 I)
    assert info_of(EPS, bad) == [0, 20001, 0]
    assert info_of(-3.0, bad) == [0, 10001, 0]


@gpu
def test_predict_return_codes(hip):
    """Every code predict.hip returns for a bad argument, each rejected before any launch: nothing is written."""
    from lvae_amd import _lib as P
    c = problem("mixed-include")
    L, M, Pn, T, Nt = c["L"], c["M"], c["P"], c["T"], c["Nt"]
    good0, good1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    bad = P.KernelSpec.from_buffer_copy(good0)
    bad.n_comp = 17   # no bucket holds it
    dv = lambda t: t.to(DEV).contiguous()
    x, z, mu, tx, p0, p1, nz = dv(c["x"]), dv(c["z"]), dv(c["mu"]), dv(c["tx"]), dv(c["p0"]), dv(c["p1"]), dv(c["noise"])
    seg, inc = torch.tensor(c["seg"], dtype=torch.int32, device=DEV), dv(c["include"])
    out, info = U.sentinel(Nt * L), U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_workspace_size(L, M, Pn, T, Nt))
    r = ctypes.byref

    def call(**kw):
        a = dict(s0=r(good0), s1=r(good1), L=L, M=M, Q=U.QC, P=Pn, T=T, seg=P.ptr(seg), inc=P.ptr(inc), Nt=Nt,
                 ws=ws.data_ptr())
        a.update(kw)
        rc = hip.lvae_predict_f64(a["s0"], a["s1"], a["L"], a["M"], a["Q"], a["P"], a["T"], a["seg"], a["inc"], P.ptr(x),
                                  P.ptr(mu), P.ptr(z), a["Nt"], P.ptr(tx), P.ptr(p0), P.ptr(p1), P.ptr(nz), EPS,
                                  P.ptr(out), P.ptr(info), a["ws"], P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    for kw in (dict(s0=None), dict(s1=None), dict(s0=r(bad)), dict(s1=r(bad))):
        assert call(**kw) == -1, kw
    for kw in (dict(L=0), dict(M=0), dict(M=129)):
        assert call(**kw) == -3, kw
    for kw in (dict(P=0), dict(T=0), dict(T=129), dict(Q=0)):
        assert call(**kw) == -6, kw
    assert call(seg=None) == -8 and call(inc=None) == -8
    assert call(Nt=-1) == -13
    for w in (None, ws.data_ptr() + 8, ws.data_ptr() + 128):
        assert call(ws=w) == -20
    assert U.all_sentinel(out) and U.all_sentinel(info) and bool((ws == 0x7F).all())
    assert call() == 0 and not U.all_sentinel(out) and U.tail_untouched(tail)   # (nothing wrong: it runs)
