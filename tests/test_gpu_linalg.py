"""The N x N factor / solve entry points (potrf.hip: lvae_potrf_*, lvae_trsm_*, lvae_potrs_*) against the
oracle's LAPACK restatement of the reference's calls (elbo_functions.py:26-29: torch.cholesky,
torch.cholesky_solve, 2 sum log diag L), through lvae_amd.linalg.

Tolerances: fp64 paths 1e-11 relative to the result's max (LAPACK-grade backward error at cond <= 1e4);
the fp32 potrf is the exact KL's f16 3-product-split factorisation, ~2^-22 of each 256-block's max per
product: 2e-5 of max |L|; fp32 solves compute in fp64 from fp32 operands: 1e-5 of the result's max.
"""
import numpy as np
import pytest
import torch

from oracle import lvae_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(cat_kernel=[2], bin_kernel=[], sqexp_kernel=[0],
           cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 2},
                           {'cont_covariate': 0, 'cat_covariate': 3},
                           {'cont_covariate': 1, 'cat_covariate': 4}],
           bin_int_kernel=[], covariate_missing_val=[])


def rel(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / max(b.abs().max(), 1e-300))


def spd(L, n, seed, cond=1e3):
    g = torch.Generator().manual_seed(seed)
    Q, _ = torch.linalg.qr(torch.randn(L, n, n, generator=g, dtype=torch.float64))
    ev = torch.logspace(0, np.log10(cond), n, dtype=torch.float64)
    return (Q * ev) @ Q.transpose(-1, -2)


def health_mnist_K(P, L, seed):
    """the exact KL's K = Gram + noise I on Health-MNIST covariates (the C2 shape at P = 64, L = 8)"""
    from lvae_amd.data import health_mnist_covariates
    X = torch.tensor(health_mnist_covariates(P, 16, seed=seed))
    spec = O.spec_full(**CFG)
    rng = np.random.default_rng(seed)
    Ks = []
    for _ in range(L):
        params = torch.tensor(rng.uniform(0.5, 3.0, O.n_params(spec)))
        Ks.append(O.gram(spec, params, X, X) + torch.eye(X.shape[0], dtype=torch.float64))
    return torch.stack(Ks)


@pytest.mark.parametrize("n,L", [(1, 2), (63, 3), (64, 1), (65, 2), (200, 3), (1024, 2)])
def test_potrf_f64_vs_oracle(hip, n, L):
    import lvae_amd.linalg as LA
    A = spd(L, n, seed=n)
    Lr, ldr = O.potrf(A)
    Lg, ldg, info = LA.cholesky_ex(A.to(DEV))
    assert int(info.abs().sum()) == 0
    assert rel(Lg, Lr) < 1e-11
    assert rel(ldg, ldr) < 1e-12
    assert torch.equal(torch.triu(Lg.cpu(), 1), torch.zeros_like(Lr))  # torch.cholesky's zero upper part


def test_potrf_f64_many_workgroups(hip):
    """n = 2048, L = 16: the first pass launches 31 x 16 panel workgroups, more than are resident at once
    (the former fused diagonal + panel launch raced on A_kk exactly when its workgroups did not all
    start together; the tests above all fit in one wave of workgroups)."""
    import lvae_amd.linalg as LA
    n, L = 2048, 16
    g = torch.Generator().manual_seed(5)
    B = torch.randn(L, n, n, generator=g, dtype=torch.float64)
    A = B @ B.transpose(-1, -2) / n + torch.eye(n, dtype=torch.float64)
    Lr, ldr = O.potrf(A)
    Lg, ldg, info = LA.cholesky_ex(A.to(DEV))
    assert int(info.abs().sum()) == 0
    assert rel(Lg, Lr) < 1e-11
    assert rel(ldg, ldr) < 1e-12


def test_potrf_f64_in_place(hip):
    """Lout == A: the factor overwrites A's lower triangle (upper zeroed)."""
    n, L = 300, 2
    A = spd(L, n, seed=3)
    Ad = A.to(DEV).contiguous()
    ld = torch.empty(L, dtype=torch.float64, device=DEV)
    info = torch.empty(L, dtype=torch.int32, device=DEV)
    from lvae_amd import _lib
    rc = hip.lvae_potrf_f64(n, L, _lib.ptr(Ad), n, n * n, _lib.ptr(Ad), n, n * n, _lib.ptr(ld), _lib.ptr(info),
                            _lib.stream_ptr())
    assert rc == 0
    assert rel(Ad, O.potrf(A)[0]) < 1e-11


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_potrf_not_pd_raises(hip, dtype):
    """info = the first non-positive leading minor (LAPACK / torch.cholesky's error), per batch element."""
    import lvae_amd.linalg as LA
    n = 600
    A = spd(2, n, seed=7)
    A[1, 437, 437] = -5.0  # leading minor 438 fails (the earlier ones are untouched)
    _, _, info = LA.cholesky_ex(A.to(DEV, dtype))
    info = info.cpu()
    assert int(info[0]) == 0 and int(info[1]) == 438
    with pytest.raises(torch.linalg.LinAlgError):
        LA.cholesky(A.to(DEV, dtype))


@pytest.mark.parametrize("n,L", [(100, 2), (256, 1), (1000, 2), (1024, 3)])
def test_potrf_f32_vs_oracle(hip, n, L):
    """fp32 through the exact KL's own blocked factorisation (chol_inv.hip, f16 x3 split)."""
    import lvae_amd.linalg as LA
    A = spd(L, n, seed=n + 1, cond=1e2)
    Lr, ldr = O.potrf(A)
    Lg, ldg, info = LA.cholesky_ex(A.to(DEV, torch.float32))
    assert int(info.abs().sum()) == 0
    assert Lg.dtype == torch.float32
    assert rel(Lg, Lr) < 2e-5
    assert rel(ldg, ldr) < 1e-5
    assert torch.equal(torch.triu(Lg.cpu(), 1), torch.zeros(L, n, n, dtype=torch.float32))


def test_potrf_f32_c2_shape(hip):
    """C2 (N = 1024, L = 8): the HIP factor of the exact KL's own K against LAPACK fp64 (BASELINE configs[1])."""
    import lvae_amd.linalg as LA
    K = health_mnist_K(64, 8, seed=2)
    Lr, ldr = O.potrf(K)
    Lg, ldg, info = LA.cholesky_ex(K.to(DEV, torch.float32))
    assert int(info.abs().sum()) == 0
    assert rel(Lg, Lr) < 2e-5
    assert rel(ldg, ldr) < 1e-5
    Lg64, ldg64, info = LA.cholesky_ex(K.to(DEV))
    assert rel(Lg64, Lr) < 1e-11 and rel(ldg64, ldr) < 1e-12


@pytest.mark.parametrize("n,nrhs", [(64, 1), (65, 5), (300, 64), (1024, 100)])
def test_potrs_f64_vs_oracle(hip, n, nrhs):
    import lvae_amd.linalg as LA
    L = 2
    A = spd(L, n, seed=nrhs)
    g = torch.Generator().manual_seed(nrhs)
    B = torch.randn(L, n, nrhs, generator=g, dtype=torch.float64)
    Lr, _ = O.potrf(A)
    Xr = O.potrs(B, Lr)
    Xg = LA.cholesky_solve(B.to(DEV), Lr.to(DEV))
    assert rel(Xg, Xr) < 1e-11
    # triangular solves, both orientations
    Yr = torch.linalg.solve_triangular(Lr, B, upper=False)
    assert rel(LA.solve_triangular(Lr.to(DEV), B.to(DEV)), Yr) < 1e-11
    Zr = torch.linalg.solve_triangular(Lr.transpose(-1, -2), B, upper=True)
    assert rel(LA.solve_triangular(Lr.to(DEV), B.to(DEV), transpose=True), Zr) < 1e-11


def test_potrs_f32_vs_oracle(hip):
    import lvae_amd.linalg as LA
    n, nrhs, L = 500, 7, 2
    A = spd(L, n, seed=11, cond=1e2)
    Lr, _ = O.potrf(A)
    B = torch.randn(L, n, nrhs, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    Xr = O.potrs(B.float().double(), Lr.float().double())
    Xg = LA.cholesky_solve(B.to(DEV, torch.float32), Lr.to(DEV, torch.float32))
    assert Xg.dtype == torch.float32
    assert rel(Xg, Xr) < 1e-5


def test_kl_closed_through_linalg_matches_oracle(hip):
    """The reference's KL_closed (elbo_functions.py:21-33) written with lvae_amd.linalg in place of
    torch.cholesky / cholesky_solve, in fp64, against the oracle's KL at 1e-11."""
    import lvae_amd.linalg as LA
    P, L = 16, 3
    K = health_mnist_K(P, L, seed=4)
    n = K.shape[-1]
    g = torch.Generator().manual_seed(4)
    mu = torch.randn(L, n, generator=g, dtype=torch.float64)
    lv = 0.1 * torch.randn(L, n, generator=g, dtype=torch.float64)
    Kd = K.to(DEV)
    LK1, logdet11 = LA.cholesky_logdet(Kd)
    iK1 = LA.cholesky_solve(torch.eye(n, dtype=torch.float64, device=DEV).expand(L, n, n), LK1)
    mud, v1 = mu.to(DEV), torch.exp(lv).to(DEV)
    qf1 = (mud * (iK1 @ mud.unsqueeze(-1)).squeeze(-1)).sum(-1)
    tr1 = (v1 * torch.diagonal(iK1, dim1=-2, dim2=-1)).sum(-1)
    kld = 0.5 * (tr1 + qf1 - n + logdet11 - lv.to(DEV).sum(-1))
    Lr, ldr = O.potrf(K)
    iKr = O.potrs(torch.eye(n, dtype=torch.float64).expand(L, n, n), Lr)
    ref = 0.5 * ((torch.exp(lv) * torch.diagonal(iKr, dim1=-2, dim2=-1)).sum(-1)
                 + (mu * (iKr @ mu.unsqueeze(-1)).squeeze(-1)).sum(-1) - n + ldr - lv.sum(-1))
    assert rel(kld, ref) < 1e-11


# ------------------------------------------------------------------------------------------------------------------
# The solves and factors called directly through the C ABI at their edges: n below / at / above one 64-block,
# ld > the row length and padded batch strides in NaN-filled buffers (the padding must come back untouched), the
# strict upper triangle of every triangular or symmetric input NaN (the header: it is not read), and the 1-based
# argument-index return codes.  Tolerances: this file's own (above).
# ------------------------------------------------------------------------------------------------------------------
import ctypes  # noqa: E402

import abi_util as U  # noqa: E402


def _solve_operands(n, nrhs, L, dtype):
    """fp64 CPU (Lf, B) already rounded to dtype, and their padded device buffers (Lf's strict upper part NaN)"""
    A = U.spd(L, n, seed=100 * n + nrhs, cond=1e3 if dtype == torch.float64 else 1e2)
    Lf = O.potrf(A)[0].to(dtype)
    B = torch.randn(L, n, max(nrhs, 1), generator=torch.Generator().manual_seed(n + nrhs), dtype=torch.float64)
    B = B[:, :, :nrhs].to(dtype)
    ldl, ldb = n + 3, nrhs + 3
    ls, bs = (n * ldl + 5, ldl, 1), (n * ldb + 7, ldb, 1)
    Lbuf, _ = U.padded(U.nan_upper(Lf), ls)
    return Lf.double(), B.double(), Lbuf, ls, bs


def _solve(fn, lead, n, nrhs, L, Lbuf, ls, B, bs, dtype, hip):
    """one lvae_trsm_* (lead = (trans,)) or lvae_potrs_* (lead = ()) call on a fresh padded copy of B"""
    from lvae_amd import _lib as P
    if nrhs:
        Bbuf, _ = U.padded(B.to(dtype), bs)
    else:
        Bbuf = U.sentinel(L * bs[0] + 5, dtype)
    ws, tail = U.workspace(hip.lvae_trsm_workspace_size(n, L))
    rc = fn(*lead, n, nrhs, L, P.ptr(Lbuf), ls[1], ls[0], P.ptr(Bbuf), bs[1], bs[0], P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)
    if not nrhs:
        assert U.all_sentinel(Bbuf)   # nrhs = 0: ok, nothing written
        return None
    assert U.untouched_outside(Bbuf, B.shape, bs)
    return U.view(Bbuf, B.shape, bs).cpu().double()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("nrhs", [0, 1, 63, 64, 65])
@pytest.mark.parametrize("n", [1, 17, 63, 64, 65, 130])
def test_trsm_potrs_abi_edges(hip, n, nrhs, dtype):
    L = 2
    f64 = dtype == torch.float64
    tol = 1e-11 if f64 else 1e-5
    trsm = hip.lvae_trsm_f64 if f64 else hip.lvae_trsm_f32
    potrs = hip.lvae_potrs_f64 if f64 else hip.lvae_potrs_f32
    Lf, B, Lbuf, ls, bs = _solve_operands(n, nrhs, L, dtype)
    refs = [((0,), trsm, lambda: torch.linalg.solve_triangular(Lf, B, upper=False)),
            ((1,), trsm, lambda: torch.linalg.solve_triangular(Lf.transpose(-1, -2), B, upper=True)),
            ((), potrs, lambda: O.potrs(B, Lf))]
    for lead, fn, ref in refs:
        got = _solve(fn, lead, n, nrhs, L, Lbuf, ls, B, bs, dtype, hip)
        if nrhs:
            assert rel(got, ref()) < tol, (lead, rel(got, ref()))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", [1, 65, 300])
def test_potrf_abi_edges(hip, n, dtype):
    """lda > n, ldo > n, padded batch strides, A's strict upper triangle NaN: only the lower triangle is read, the
    factor's strict upper part is zero, nothing outside the [n, n] extents is written"""
    from lvae_amd import _lib as P
    L = 2
    f64 = dtype == torch.float64
    A = U.spd(L, n, seed=n + 2, cond=1e3 if f64 else 1e2)
    Lr, ldr = O.potrf(A)
    lda, ldo = n + 3, n + 5
    sa, so = (n * lda + 5, lda, 1), (n * ldo + 7, ldo, 1)
    Abuf, _ = U.padded(U.nan_upper(A).to(dtype), sa)
    Obuf = U.sentinel(U.extent((L, n, n), so) + 5, dtype)
    ld = U.sentinel(L + 2)
    info = U.sentinel(L + 2, torch.int32)
    if f64:
        rc = hip.lvae_potrf_f64(n, L, P.ptr(Abuf), lda, sa[0], P.ptr(Obuf), ldo, so[0], P.ptr(ld), P.ptr(info),
                                P.stream_ptr())
    else:
        ws, tail = U.workspace(hip.lvae_potrf_f32_workspace_size(n, L))
        rc = hip.lvae_potrf_f32(n, L, P.ptr(Abuf), lda, sa[0], P.ptr(Obuf), ldo, so[0], P.ptr(ld), P.ptr(info),
                                P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert f64 or U.tail_untouched(tail)
    assert U.untouched_outside(Obuf, (L, n, n), so) and U.all_sentinel(ld[L:]) and U.all_sentinel(info[L:])
    assert info[:L].tolist() == [0] * L
    Lg = U.view(Obuf, (L, n, n), so).cpu()
    assert torch.equal(torch.triu(Lg, 1), torch.zeros(L, n, n, dtype=dtype))
    assert rel(Lg, Lr) < (1e-11 if f64 else 2e-5)
    assert rel(ld[:L], ldr) < (1e-12 if f64 else 1e-5) or (n == 1 and float((ld[:L].cpu() - ldr).abs().max()) < 1e-12)


def _rc_fixture(dtype):
    n, nrhs, L = 8, 4, 1
    A = U.spd(L, n, seed=1, cond=10.0)
    Ad = A.to(DEV, dtype).contiguous()
    Lf = O.potrf(A)[0].to(DEV, dtype).contiguous()
    B = torch.arange(n * nrhs, dtype=dtype, device=DEV).reshape(L, n, nrhs) + 1
    return n, nrhs, L, Ad, Lf, B


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_potrf_return_codes(hip, dtype):
    """-(1-based index of the offending argument); nothing is written"""
    from lvae_amd import _lib as P
    f64 = dtype == torch.float64
    n, _, L, Ad, _, _ = _rc_fixture(dtype)
    A0 = Ad.clone()
    out = U.sentinel(L * n * n, dtype)
    ld, info = U.sentinel(L), U.sentinel(L, torch.int32)
    ws, _ = U.workspace(hip.lvae_potrf_f32_workspace_size(n, L))
    good = dict(n=n, L=L, A=P.ptr(Ad), lda=n, sa=n * n, Lo=P.ptr(out), ldo=n, so=n * n, ld=P.ptr(ld), info=P.ptr(info),
                ws=P.ptr(ws))

    def call(**kw):
        a = dict(good, **kw)
        lead = (a["n"], a["L"], a["A"], a["lda"], a["sa"], a["Lo"], a["ldo"], a["so"], a["ld"], a["info"])
        rc = (hip.lvae_potrf_f64(*lead, P.stream_ptr()) if f64 else hip.lvae_potrf_f32(*lead, a["ws"], P.stream_ptr()))
        torch.cuda.synchronize()
        return rc
    cases = [(dict(n=0), -1), (dict(L=0), -2), (dict(A=None), -3), (dict(lda=n - 1), -4), (dict(Lo=None), -6),
             (dict(ldo=n - 1), -7), (dict(ld=None), -9), (dict(info=None), -10)]
    if f64:
        cases.append((dict(Lo=P.ptr(Ad), ldo=n + 1), -7))   # in place needs ldo == lda
    else:
        cases += [(dict(ws=None), -11), (dict(ws=ctypes.c_void_p(ws.data_ptr() + 8)), -11),
                  (dict(n=16385, lda=16385, ldo=16385), -1)]   # n <= 16384
    for kw, want in cases:
        assert call(**kw) == want, (kw, want)
        assert U.all_sentinel(out) and U.all_sentinel(ld) and U.all_sentinel(info) and torch.equal(Ad, A0), kw
    assert call() == 0 and not U.all_sentinel(out)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_trsm_potrs_return_codes(hip, dtype):
    """lvae_trsm_*: trans is argument 1, so n .. workspace are 2 .. 11; lvae_potrs_* has no trans: the same checks
    report one less.  B is unchanged after a rejected call."""
    from lvae_amd import _lib as P
    f64 = dtype == torch.float64
    n, nrhs, L, _, Lf, B = _rc_fixture(dtype)
    B0 = B.clone()
    ws, _ = U.workspace(hip.lvae_trsm_workspace_size(n, L))
    good = dict(trans=0, n=n, nrhs=nrhs, L=L, Lf=P.ptr(Lf), ldl=n, sl=n * n, B=P.ptr(B), ldb=nrhs, sb=n * nrhs,
                ws=P.ptr(ws))
    trsm = hip.lvae_trsm_f64 if f64 else hip.lvae_trsm_f32
    potrs = hip.lvae_potrs_f64 if f64 else hip.lvae_potrs_f32

    def call(fn, **kw):
        a = dict(good, **kw)
        rest = (a["n"], a["nrhs"], a["L"], a["Lf"], a["ldl"], a["sl"], a["B"], a["ldb"], a["sb"], a["ws"])
        rc = fn(a["trans"], *rest, P.stream_ptr()) if fn is trsm else fn(*rest, P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    assert call(trsm, trans=2) == -1 and torch.equal(B, B0)
    assert call(trsm, trans=-1) == -1 and torch.equal(B, B0)
    cases = [(dict(n=0), -2), (dict(nrhs=-1), -3), (dict(L=0), -4), (dict(Lf=None), -5), (dict(ldl=n - 1), -6),
             (dict(B=None), -8), (dict(ldb=nrhs - 1), -9), (dict(ws=None), -11),
             (dict(ws=ctypes.c_void_p(ws.data_ptr() + 8)), -11)]
    for kw, want in cases:
        assert call(trsm, **kw) == want, (kw, want)
        assert call(potrs, **kw) == want + 1, (kw, want + 1)
        assert torch.equal(B, B0), kw
    assert call(trsm) == 0 and not torch.equal(B, B0)
    assert call(potrs) == 0
