"""lvae_predict_exact_f64 and lvae_gram_matvec_f64 through the C ABI against an fp64 oracle on the CPU built here
from O.gram + torch.linalg.cholesky / cholesky_solve:
    Zpred[t, l] = k_l(X*_t, X) (k_l(X, X) + noise_l I)^-1 mu[:, l].
Full kernels are spec0 + spec1 of abi_util.spec_pairs() plus an extension spec with per and lin factors.  The
prediction covariates are abi_util.subject_covariates with about 10 % of the rows dropped (ragged subjects), or an
exact number of rows kept where the case is about a tile edge; the test rows have real-valued times and subject ids
inside and outside the prediction set.  Hyper-parameters and noise from abi_util.draw_hypers.

Shapes: the 64-wide tiles' edges (63 / 64 / 65 rows on either side), more than one row and column tile, both
template buckets, L = 1 and L = 16, the slab path (few test rows against a prediction set long enough for the host
to cut the columns into S >= 2 slabs; S is read off lvae_gram_matvec_workspace_size), no test rows at all, and a
spec that reads 18 covariate columns (more than the 16 the fused kernel's narrow LDS image stages).

Tolerance: the project's rule, min(max(10 x yardstick, 2e-12), 1e-6), the yardstick being the larger of the
oracle's change under a relative 2^-50 perturbation of hyper-parameters, noise and mu and the CPU / device spread
of the oracle.  On the CPU every oracle factorisation of these draws succeeds and the perturbation yardsticks are
1e-15 .. 5e-14 (test_cases_are_well_posed), so the 2e-12 floor sets the bound.

The case ext-a is ext_util's pair ext-a as one kernel, spec0 + spec1 (9 components, bucket (16, 4): bare, gated and
id-gated periodic and linear factors).  Measured on the MI355X: 48 prediction rows, err 6.61e-15 against a yardstick
of 1.23e-14 and the bound 2.0e-12.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import abi_util as U
import ext_util
from oracle import lvae_oracle as O

gpu = pytest.mark.gpu
DEV = U.DEV
EXT = [[("per", 0)], [("lin", 1)], [("cat", 3), ("per", 0)], [("lin", 6), ("cat", 4)], [("rbf", 0)]]
# 18 distinct covariate columns of a 3 x QC-column matrix (column c + 8 m is column c of an independent draw m):
# beyond the 16 the narrow LDS image of the fused kernel stages, in the (16, 4) bucket
WIDE = [[("rbf", 0), ("rbf", 8)], [("rbf", 1), ("rbf", 17)], [("cat", 3), ("rbf", 16)],
        [("rbf", 6), ("rbf", 14), ("rbf", 22)], [("lin", 9)], [("cat", 4), ("cat", 12), ("cat", 20)],
        [("bin", 5), ("rbf", 13)], [("bin", 7), ("bin", 15), ("rbf", 21)]]
SPECS = {**{k: s0 + s1 for k, (s0, s1) in U.spec_pairs().items()}, "ext": EXT, "wide-cols": WIDE,
         "ext-a": sum(ext_util.ext_pairs()["ext-a"], [])}   # 9 components: bucket (16, 4)

# id: (spec, L, P, T, prediction rows kept (None: about 90 % at random; "slab": see slab_rows), Nt)
CASES = {
    "smallest": ("ref", 1, 1, 1, 1, 1),
    "tile-edge": ("ref", 2, 5, 13, None, 63),
    "tile-edge-64": ("ref", 2, 5, 13, 64, 64),
    "tile-edge-65": ("ref", 2, 5, 13, 65, 65),
    "mix1": ("mix1", 3, 18, 15, None, 130),
    "mix2-big": ("mix2", 2, 17, 64, None, 257),
    "ext": ("ext", 2, 8, 16, None, 70),
    "wide": ("ref", 16, 3, 11, None, 40),
    "few-rows": ("ref", 2, 20, 26, "slab", 3),
    "no-test-rows": ("ref", 2, 4, 10, 40, 0),
    "wide-cols": ("wide-cols", 2, 6, 16, None, 70),
    "ext-a": ("ext-a", 3, 6, 9, None, 70),
}
CASE_IDS = list(CASES)


def slabs(n1, n2, L):
    """Column slabs S the host picks for the fused product, read off its workspace size (L S n1 doubles for
    S > 1, nothing for S = 1)"""
    from lvae_amd import _lib
    return max(1, int(_lib.load().lvae_gram_matvec_workspace_size(n1, n2, L)) // (8 * L * n1))


@functools.lru_cache(maxsize=None)
def slab_rows(nt, L, limit):
    """The fewest prediction rows (one more than a multiple of 64) at which nt test rows take S >= 2 slabs"""
    for n in range(65, limit + 1, 64):
        if slabs(nt, n, L) >= 2:
            return n
    raise AssertionError(f"no slab path up to {limit} prediction rows")


@functools.lru_cache(maxsize=None)
def problem(cid):
    name, L, Pn, T, keep, Nt = CASES[cid]
    spec = SPECS[name]
    rng = np.random.default_rng(5000 + CASE_IDS.index(cid))
    gen = torch.Generator().manual_seed(6000 + CASE_IDS.index(cid))
    reps = 3 if name == "wide-cols" else 1
    xa = torch.cat([U.subject_covariates(rng, Pn, T).reshape(Pn * T, U.QC) for _ in range(reps)], 1)
    if keep == "slab":
        keep = slab_rows(Nt, L, Pn * T)
    if keep is None:
        rows = np.nonzero(rng.random(Pn * T) >= 0.1)[0]
    else:
        rows = np.sort(rng.choice(Pn * T, keep, replace=False))
    x = xa[torch.tensor(rows)].contiguous()
    n = x.shape[0]
    tx = torch.cat([U.subject_covariates(rng, max(Nt, 1), 1).reshape(max(Nt, 1), U.QC) for _ in range(reps)], 1)[:Nt]
    if Nt:
        tx[:, 0] = torch.tensor(rng.uniform(0.0, 0.5 * T, Nt))
        tids = [0, Pn + 2, Pn - 1, Pn + 5]           # subjects inside and outside the prediction set
        tx[:, U.ID_COL] = torch.tensor([float(tids[i % len(tids)]) for i in range(Nt)])
    return dict(spec=spec, L=L, n=n, Nt=Nt, x=x, tx=tx, mu=torch.randn(n, L, generator=gen, dtype=torch.float64),
                params=U.draw_hypers(rng, L, O.n_params(spec)), noise=U.draw_hypers(rng, L, None))


def solve_oracle(spec, params, noise, x, tx, mu):
    """[Nt, L]: k(X*, X) K^-1 mu from the Cholesky factor (raises where K is not positive definite), one latent dim
    at a time through the oracle's own unbatched O.potrf / O.potrs, as O.kl_closed factors and solves (on the
    device too: the [N, N] calls test_gpu_regime_b.py makes there at N = 4096)"""
    eye = torch.eye(x.shape[0], dtype=x.dtype, device=x.device)
    cols = []
    for l in range(params.shape[0]):
        Lc, _ = O.potrf(O.gram(spec, params[l], x, x) + noise[l] * eye)
        cols.append(O.gram(spec, params[l], tx, x) @ O.potrs(mu[:, l:l + 1], Lc))
    return torch.cat(cols, 1)


def oracle(cid, dev="cpu", perturb=False):
    c = problem(cid)
    if c["Nt"] == 0:
        return None
    v = {k: c[k] for k in ("params", "noise", "mu")}
    if perturb:
        gen = torch.Generator().manual_seed(79)
        v = {k: U.perturbed(t, gen) for k, t in v.items()}
    v = {k: t.to(dev) for k, t in v.items()}
    return solve_oracle(c["spec"], v["params"], v["noise"], c["x"].to(dev), c["tx"].to(dev), v["mu"]).cpu()


@functools.lru_cache(maxsize=None)
def cpu_ref(cid):
    """(oracle, perturbation yardstick) on the CPU; (None, 0) without test rows"""
    ref = oracle(cid)
    return (None, 0.0) if ref is None else (ref, U.rel(oracle(cid, perturb=True), ref))


def test_cases_are_well_posed():
    """Every oracle factorisation succeeds, every perturbation yardstick is <= 1e-7 (10 x it stays under the 1e-6
    cap), the references are not zero, and the few-rows case really takes the slab path."""
    for cid in CASE_IDS:
        c = problem(cid)
        K = O.gram(c["spec"], c["params"], c["x"], c["x"]) + c["noise"][:, None, None] * torch.eye(c["n"], dtype=torch.float64)
        _, info = torch.linalg.cholesky_ex(K)
        assert info.tolist() == [0] * c["L"], cid
        ref, ya = cpu_ref(cid)
        if ref is not None:
            assert ya <= 1e-7 and float(ref.abs().max()) > 0, (cid, ya)
    c = problem("few-rows")
    assert slabs(c["Nt"], c["n"], c["L"]) >= 2 and slabs(c["Nt"], c["n"] - 64, c["L"]) == 1
    sizes = {cid: problem(cid)["n"] for cid in CASE_IDS}
    assert sizes["tile-edge-64"] == 64 and sizes["tile-edge-65"] == 65 and 50 <= sizes["tile-edge"] < 64
    assert sizes["mix2-big"] > 900 and sizes["smallest"] == 1 and sizes["no-test-rows"] == 40


def run(hip, cid, pad=3, noise=None):
    """One lvae_predict_exact_f64 call on sentinel-filled buffers with ld_mu = L + pad, ld_out = L + pad and the
    covariates at ld = columns + pad; returns (out [Nt, L] on the CPU, info list)"""
    from lvae_amd import _lib as P
    c = problem(cid)
    L, n, Nt = c["L"], c["n"], c["Nt"]
    spec = P.make_spec(c["spec"])
    dv = lambda t: t.to(DEV).contiguous()
    ldx = c["x"].shape[1] + pad
    xb, xv = U.padded(c["x"], (ldx, 1))
    tb, tv = U.padded(c["tx"], (ldx, 1)) if Nt else (None, None)
    mb, mv = U.padded(c["mu"], (L + pad, 1))
    params, nz = dv(c["params"]), dv(c["noise"] if noise is None else noise)
    ld_out = L + pad
    out = U.sentinel(max(Nt, 1) * ld_out + 7)
    info = U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_exact_workspace_size(n, Nt, L))
    rc = hip.lvae_predict_exact_f64(ctypes.byref(spec), P.ptr(xb), ldx, n, L, P.ptr(params), P.ptr(nz),
                                    P.ptr(mb), L + pad, P.ptr(tb) if Nt else None, ldx, Nt, P.ptr(out), ld_out,
                                    P.ptr(info), P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)                                     # the workspace size is enough
    assert U.untouched_outside(out, (Nt, L), (ld_out, 1))             # out [Nt, L] at ld_out and nothing else
    got = U.view(out, (Nt, L), (ld_out, 1)).cpu() if Nt else torch.empty(0, L, dtype=torch.float64)
    return got, info.cpu().tolist()


@gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_predict_exact_values(hip, cid):
    c = problem(cid)
    got, info = run(hip, cid)
    assert info == [0] * c["L"]
    again, _ = run(hip, cid, pad=0)
    assert U.bit_equal(got, again)                                    # a second run, other strides: the same bits
    ref, ya = cpu_ref(cid)
    if ref is None:
        assert got.numel() == 0                                       # Nt = 0: rc 0, info written, out untouched
        return
    yard = max(ya, U.rel(oracle(cid, DEV), ref))
    err, tol = U.rel(got, ref), min(max(10.0 * yard, 2e-12), 1e-6)
    print(f"predict_exact {cid}: n {c['n']} err {err:.2e} yardstick {yard:.2e} ratio {err / max(yard, 1e-300):.2g} "
          f"bound {tol:.1e}")
    assert bool(torch.isfinite(got).all())
    assert err <= tol


@gpu
@pytest.mark.parametrize("cid", ["tile-edge", "tile-edge-64", "tile-edge-65", "ext", "few-rows", "wide-cols"])
@pytest.mark.parametrize("diag", [False, True])
def test_gram_matvec_values(hip, cid, diag):
    """lvae_gram_matvec_f64 alone against O.gram(...) @ v, with ld_v > L and ld_out > L: the rectangular product
    k(X*, X) v, and with diag the square one (k(X, X) + diag I) v (diag needs n1 == n2).  Bound: the a-priori
    forward error of an n2-term fp64 dot product in any summation order, (n2 + 16) 2^-52 max_i sum_j |K_ij v_j|
    (16: the few ulps of each kernel value's exp / sin on either side), relative to max|ref|."""
    from lvae_amd import _lib as P
    c = problem(cid)
    L, n2 = c["L"], c["n"]
    x1 = c["x"] if diag else c["tx"]
    n1 = x1.shape[0]
    spec = P.make_spec(c["spec"])
    gen = torch.Generator().manual_seed(91)
    v = torch.randn(n2, L, generator=gen, dtype=torch.float64)
    dg = U.draw_hypers(np.random.default_rng(92), L, None)
    K = O.gram(c["spec"], c["params"], x1, c["x"])
    if diag:
        K = K + dg[:, None, None] * torch.eye(n2, dtype=torch.float64)
    ref = (K @ v.T.unsqueeze(-1)).squeeze(-1).T
    mag = float((K.abs() @ v.T.abs().unsqueeze(-1)).max())
    dv = lambda t: t.to(DEV).contiguous()
    x1d, x2d, params, dgd = dv(x1), dv(c["x"]), dv(c["params"]), dv(dg)
    vb, _ = U.padded(v, (L + 2, 1))
    ld_out = L + 3

    def call():
        out = U.sentinel(n1 * ld_out + 5)
        ws, tail = U.workspace(hip.lvae_gram_matvec_workspace_size(n1, n2, L))
        rc = hip.lvae_gram_matvec_f64(ctypes.byref(spec), P.ptr(x1d), x1d.shape[1], n1, P.ptr(x2d), x2d.shape[1], n2, L, P.ptr(params),
                                      P.ptr(dgd) if diag else None, P.ptr(vb), L + 2, P.ptr(out), ld_out, P.ptr(ws),
                                      P.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and U.tail_untouched(tail)
        assert U.untouched_outside(out, (n1, L), (ld_out, 1))
        return U.view(out, (n1, L), (ld_out, 1)).cpu()
    got = call()
    assert U.bit_equal(got, call())
    err, tol = U.rel(got, ref), 2.0 ** -52 * (n2 + 16) * mag / float(ref.abs().max())
    print(f"gram_matvec {cid} diag={diag}: [{n1} x {n2}] S {slabs(n1, n2, L)} err {err:.2e} bound {tol:.1e}")
    assert err <= tol
    if cid == "few-rows" and not diag:
        assert slabs(n1, n2, L) >= 2


@gpu
def test_gram_matvec_empty_sides(hip):
    """n2 == 0 writes zeros to out [n1, L] and returns 0; n1 == 0 returns 0 and writes nothing."""
    from lvae_amd import _lib as P
    c = problem("tile-edge")
    L, n = c["L"], c["n"]
    spec = P.make_spec(c["spec"])
    x, params = c["x"].to(DEV), c["params"].to(DEV)
    out = U.sentinel(n * (L + 1) + 3)
    rc = hip.lvae_gram_matvec_f64(ctypes.byref(spec), P.ptr(x), U.QC, n, None, 0, 0, L, P.ptr(params), None, None, 0,
                                  P.ptr(out), L + 1, None, P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and U.untouched_outside(out, (n, L), (L + 1, 1))
    assert bool((U.view(out, (n, L), (L + 1, 1)) == 0).all())
    out = U.sentinel(8)
    rc = hip.lvae_gram_matvec_f64(ctypes.byref(spec), None, 0, 0, P.ptr(x), U.QC, n, L, P.ptr(params), None, None, 0,
                                  P.ptr(out), L, None, P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and U.all_sentinel(out)
    assert hip.lvae_gram_matvec_workspace_size(0, n, L) == 0 and hip.lvae_gram_matvec_workspace_size(n, 0, L) == 0


@gpu
def test_predict_exact_info_codes(hip):
    """A dim whose noise is negative and larger than K's diagonal is indefinite by construction: info[l] > 0 for
    that dim only (LAPACK-style: the first failing column + 1 = 1), and the other dims' outputs keep their bits."""
    c = problem("mix1")
    good, info = run(hip, "mix1")
    assert info == [0, 0, 0]
    diag_max = float(O.gram(c["spec"], c["params"], c["x"], c["x"]).diagonal(dim1=-2, dim2=-1).max())
    bad = c["noise"].clone()
    bad[1] = -(diag_max + 1.0)
    got, info = run(hip, "mix1", noise=bad)
    assert info[0] == 0 and info[2] == 0 and info[1] == 1
    assert U.bit_equal(got[:, [0, 2]], good[:, [0, 2]])


@gpu
def test_return_codes(hip):
    """Every documented bad-argument code of the two entry points, each rejected before any launch: nothing is
    written."""
    from lvae_amd import _lib as P
    c = problem("tile-edge")
    L, n, Nt = c["L"], c["n"], c["Nt"]
    good = P.make_spec(c["spec"])
    bad = P.KernelSpec.from_buffer_copy(good)
    bad.n_comp = 17                                  # no bucket holds it
    far = P.KernelSpec.from_buffer_copy(good)
    far.dim[0][0] = 32                               # lvae_gram_f64's limit: factor dims below 32
    neg = P.KernelSpec.from_buffer_copy(good)
    neg.dim[0][0] = -1
    dv = lambda t: t.to(DEV).contiguous()
    x, tx, mu, params, nz = dv(c["x"]), dv(c["tx"]), dv(c["mu"]), dv(c["params"]), dv(c["noise"])
    out, info = U.sentinel(Nt * L), U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_exact_workspace_size(n, Nt, L))
    r = ctypes.byref

    def pe(**kw):
        a = dict(spec=r(good), x=P.ptr(x), ldx=U.QC, n=n, L=L, params=P.ptr(params), noise=P.ptr(nz), mu=P.ptr(mu),
                 ld_mu=L, tx=P.ptr(tx), ldt=U.QC, nt=Nt, out=P.ptr(out), ld_out=L, info=P.ptr(info), ws=ws.data_ptr())
        a.update(kw)
        rc = hip.lvae_predict_exact_f64(a["spec"], a["x"], a["ldx"], a["n"], a["L"], a["params"], a["noise"], a["mu"],
                                        a["ld_mu"], a["tx"], a["ldt"], a["nt"], a["out"], a["ld_out"], a["info"],
                                        a["ws"], P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    ld_need = 1 + max(d for comp in c["spec"] for _, d in comp)
    for kw in (dict(spec=None), dict(spec=r(bad)), dict(spec=r(far)), dict(spec=r(neg))):
        assert pe(**kw) == -1, kw
    codes = [(dict(x=None), -2), (dict(ldx=ld_need - 1), -3), (dict(n=0), -4), (dict(n=-1), -4), (dict(L=0), -5),
             (dict(params=None), -6), (dict(noise=None), -7), (dict(mu=None), -8), (dict(ld_mu=L - 1), -9),
             (dict(tx=None), -10), (dict(ldt=ld_need - 1), -11), (dict(nt=-1), -12), (dict(out=None), -13),
             (dict(ld_out=L - 1), -14), (dict(info=None), -15), (dict(ws=None), -16),
             (dict(ws=ws.data_ptr() + 8), -16), (dict(ws=ws.data_ptr() + 128), -16)]
    for kw, want in codes:
        assert pe(**kw) == want, kw
    assert U.all_sentinel(out) and U.all_sentinel(info) and bool((ws == 0x7F).all())
    assert hip.lvae_predict_exact_workspace_size(0, Nt, L) == 0
    assert hip.lvae_predict_exact_workspace_size(n, -1, L) == 0 and hip.lvae_predict_exact_workspace_size(n, Nt, 0) == 0

    # lvae_gram_matvec_f64, on the slab shape (its workspace is needed there)
    s = problem("few-rows")
    n1, n2, Ls = s["Nt"], s["n"], s["L"]
    x1, x2, ps = dv(s["tx"]), dv(s["x"]), dv(s["params"])
    v, dg = dv(s["mu"]), dv(s["noise"])
    mo = U.sentinel(n1 * Ls)
    mws, _ = U.workspace(hip.lvae_gram_matvec_workspace_size(n1, n2, Ls))
    assert hip.lvae_gram_matvec_workspace_size(n1, n2, Ls) > 0

    def mvc(**kw):
        a = dict(spec=r(good), x1=P.ptr(x1), ld1=U.QC, n1=n1, x2=P.ptr(x2), ld2=U.QC, n2=n2, L=Ls, params=P.ptr(ps),
                 diag=None, v=P.ptr(v), ld_v=Ls, out=P.ptr(mo), ld_out=Ls, ws=mws.data_ptr())
        a.update(kw)
        rc = hip.lvae_gram_matvec_f64(a["spec"], a["x1"], a["ld1"], a["n1"], a["x2"], a["ld2"], a["n2"], a["L"],
                                      a["params"], a["diag"], a["v"], a["ld_v"], a["out"], a["ld_out"], a["ws"],
                                      P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    for kw in (dict(spec=None), dict(spec=r(bad)), dict(spec=r(far)), dict(spec=r(neg))):
        assert mvc(**kw) == -1, kw
    codes = [(dict(n1=-1), -4), (dict(n2=-1), -7), (dict(L=0), -8), (dict(x1=None), -2), (dict(ld1=ld_need - 1), -3),
             (dict(x2=None), -5), (dict(ld2=ld_need - 1), -6), (dict(params=None), -9), (dict(diag=P.ptr(dg)), -10),
             (dict(v=None), -11), (dict(ld_v=Ls - 1), -12), (dict(out=None), -13), (dict(ld_out=Ls - 1), -14),
             (dict(ws=None), -15), (dict(ws=mws.data_ptr() + 8), -15)]
    for kw, want in codes:
        assert mvc(**kw) == want, kw
    assert U.all_sentinel(mo) and bool((mws == 0x7F).all())
    assert mvc() == 0 and not U.all_sentinel(mo)     # (nothing wrong: it runs)
    assert pe() == 0 and not U.all_sentinel(out) and U.tail_untouched(tail)
