"""lvae_gemm_small_f64, lvae_spd_inv_small_f64 and lvae_natgrad_update_f64 through the C ABI against torch
fp64 on the CPU / the oracle, at the sizes where small.hip, blkinv.hpp and the natural-gradient update take
another path: the gemm's K passes (k <= 128 one pass, k > 128 several; k not a multiple of the MFMA's 4), its
32-tiles, all four transpose combinations, the beta == 0 overwrite; the inverse's four template buckets
(n <= 16, 32, 64, 128), the identity padding (n not a multiple of 16), info in every 16-block; the update's
all-or-nothing commit.

Tolerances.  gemm: componentwise |C - C_ref|_ij <= 2 (k + 2) 2^-53 (|alpha| (|op A| |op B|)_ij + |beta| |C0|_ij)
(the standard inner-product bound for either summation order, doubled for the reference's own error).  Inverse,
cond 1e3: 1e-12 of max|A^-1| and 1e-12 on log|A| (test_spd_inv_small_and_gemm's bounds).  Inverse, cond 1e8 (the
K0zz regime): the yardstick is LAPACK's fp64 inverse on the CPU; max|I - A Ainv| must stay within
max(8 x LAPACK's own residual, n 2^-52 cond) (two backward-stable factorisations with different blocking and
summation order differ by a modest constant; the floor is the rounding of forming the residual itself).
Natural-gradient update: 1e-7 of the result's max against O.natural_gradient_update (test_natural_gradient's
bound).

Measured on the MI355X at cond 1e8, max|I - A Ainv| (batch 1 / batch 5; bound: 8 x LAPACK, floor n 2^-52 cond):
    n      LAPACK               kernel               kernel / LAPACK
    2      3.7e-09 / 3.7e-09    3.7e-09 / 7.5e-09    1.00 / 2.00
    15     1.2e-09 / 4.2e-09    1.7e-09 / 3.8e-09    1.41 / 0.91
    16     1.9e-09 / 1.4e-09    1.2e-09 / 8.1e-09    0.67 / 5.77
    17     1.4e-09 / 1.2e-09    4.2e-09 / 7.0e-09    3.01 / 5.85
    31     7.0e-10 / 1.5e-09    1.4e-09 / 2.1e-09    1.96 / 1.41
    32     6.1e-10 / 1.0e-09    7.9e-10 / 2.5e-09    1.30 / 2.40
    33     7.2e-10 / 1.8e-09    2.1e-09 / 7.5e-09    2.93 / 4.25
    48     8.2e-10 / 1.3e-09    2.1e-09 / 2.5e-09    2.54 / 1.87
    63     5.6e-10 / 1.2e-09    1.6e-09 / 2.2e-09    2.79 / 1.91
    64     8.4e-10 / 1.0e-09    3.0e-09 / 2.3e-09    3.56 / 2.26
    65     6.6e-10 / 1.2e-09    1.9e-09 / 2.2e-09    2.90 / 1.87
    100    9.1e-10 / 1.2e-09    2.5e-09 / 2.2e-09    2.77 / 1.90
    127    9.6e-10 / 6.6e-10    1.9e-09 / 2.6e-09    1.95 / 4.01
    128    5.8e-10 / 9.0e-10    1.3e-09 / 1.9e-09    2.20 / 2.13
(n = 1: both residuals 0.)  Every ratio is below the 8x margin, and every kernel residual below the floor
(4.4e-08 at n = 2 up to 2.8e-06 at n = 128).
"""
import numpy as np
import pytest
import torch

import abi_util as U
from oracle import lvae_oracle as O

pytestmark = pytest.mark.gpu
DEV = U.DEV
F64 = torch.float64
EPS = 2.0 ** -53


# ------------------------------------------------------------------------------------------------------
# gemm
# ------------------------------------------------------------------------------------------------------
def _operand(mat, pad=3):
    """(buffer, ld) of a [r, c] matrix with ld = c + pad in a NaN buffer (an empty matrix: a dummy buffer)"""
    ld = mat.shape[1] + pad
    if mat.numel() == 0:
        return U.sentinel(8), ld
    buf, _ = U.padded(mat, (ld, 1))
    return buf, ld


def _gemm_bound(k, alpha, opA, opB, beta, C0):
    b = abs(alpha) * (opA.abs() @ opB.abs())
    if beta != 0.0:
        b = b + abs(beta) * C0.abs()
    return 2.0 * (k + 2) * EPS * b


def gemm_once(hip, gen, ta, tb, m, n, k, alpha, beta):
    from lvae_amd import _lib as P
    opA = torch.randn(m, k, generator=gen, dtype=F64)
    opB = torch.randn(k, n, generator=gen, dtype=F64)
    C0 = torch.randn(m, n, generator=gen, dtype=F64)
    ref = alpha * (opA @ opB) + (beta * C0 if beta != 0.0 else 0.0)
    Ab, lda = _operand(opA.T.contiguous() if ta else opA)
    Bb, ldb = _operand(opB.T.contiguous() if tb else opB)
    ldc = n + 3
    Cb = U.sentinel(U.extent((m, n), (ldc, 1)) + 5)
    if beta != 0.0:   # (beta == 0: C stays NaN and must be overwritten, not propagated)
        U.view(Cb, (m, n), (ldc, 1)).copy_(C0)
    rc = hip.lvae_gemm_small_f64(ta, tb, m, n, k, alpha, P.ptr(Ab), lda, 0, 0, P.ptr(Bb), ldb, 0, 0, beta, P.ptr(Cb),
                                 ldc, 0, 0, 1, 1, P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.untouched_outside(Cb, (m, n), (ldc, 1))
    got = U.view(Cb, (m, n), (ldc, 1)).cpu()
    excess = (got - ref).abs() - _gemm_bound(k, alpha, opA, opB, beta, C0)
    assert not torch.isnan(got).any() and float(excess.max()) <= 0.0, (ta, tb, m, n, k, alpha, beta, float(excess.max()))


GEMM_MN = [(1, 1), (31, 33), (32, 32), (33, 65), (65, 31), (1, 65), (65, 1)]
GEMM_AB = [(1.0, 0.0), (0.5, 2.0), (-1.0, 1.0), (0.0, 1.0)]


@pytest.mark.parametrize("k", [0, 1, 3, 4, 5, 127, 128, 129, 260])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_small(hip, ta, tb, k):
    gen = torch.Generator().manual_seed(1000 * k + 2 * ta + tb)
    for (m, n) in GEMM_MN:
        for (alpha, beta) in GEMM_AB:
            gemm_once(hip, gen, ta, tb, m, n, k, alpha, beta)


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("bcast", ["A", "B"])
def test_gemm_small_batched(hip, ta, tb, bcast):
    """(nb1, nb2) = (2, 3): one operand broadcast (both strides 0), the other and C with padded batch strides"""
    from lvae_amd import _lib as P
    nb1, nb2, m, n, k, alpha, beta = 2, 3, 33, 31, 129, 0.5, 2.0
    gen = torch.Generator().manual_seed(17 + 2 * ta + tb)
    opA = torch.randn(*((1, 1) if bcast == "A" else (nb1, nb2)), m, k, generator=gen, dtype=F64)
    opB = torch.randn(*((1, 1) if bcast == "B" else (nb1, nb2)), k, n, generator=gen, dtype=F64)
    C0 = torch.randn(nb1, nb2, m, n, generator=gen, dtype=F64)
    ref = alpha * (opA @ opB) + beta * C0

    def batched(op, t, is_bcast):
        st = op.transpose(-1, -2).contiguous() if t else op
        r, c = st.shape[-2:]
        ld = c + 3
        if is_bcast:
            buf, _ = U.padded(st[0, 0], (ld, 1))
            return buf, ld, 0, 0
        s2 = r * ld + 5
        s1 = nb2 * s2 + 7
        buf, _ = U.padded(st, (s1, s2, ld, 1))
        return buf, ld, s1, s2
    Ab, lda, sa1, sa2 = batched(opA, ta, bcast == "A")
    Bb, ldb, sb1, sb2 = batched(opB, tb, bcast == "B")
    ldc = n + 3
    sc2 = m * ldc + 5
    sc1 = nb2 * sc2 + 7
    cs = (sc1, sc2, ldc, 1)
    Cb, _ = U.padded(C0, cs)
    rc = hip.lvae_gemm_small_f64(ta, tb, m, n, k, alpha, P.ptr(Ab), lda, sa1, sa2, P.ptr(Bb), ldb, sb1, sb2, beta,
                                 P.ptr(Cb), ldc, sc1, sc2, nb1, nb2, P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.untouched_outside(Cb, C0.shape, cs)
    got = U.view(Cb, C0.shape, cs).cpu()
    bound = 2.0 * (k + 2) * EPS * (abs(alpha) * (opA.abs() @ opB.abs()) + abs(beta) * C0.abs())
    assert float(((got - ref).abs() - bound).max()) <= 0.0


def test_gemm_small_rejections(hip):
    from lvae_amd import _lib as P
    A = torch.ones(64, dtype=F64, device=DEV)
    C = U.sentinel(64)

    def call(m, n, k, nb1=1, nb2=1):
        rc = hip.lvae_gemm_small_f64(0, 0, m, n, k, 1.0, P.ptr(A), 8, 0, 0, P.ptr(A), 8, 0, 0, 0.0, P.ptr(C), 8, 0, 0,
                                     nb1, nb2, P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    # -(1-based index of the bad argument): ta, tb, m, n, k are arguments 1..5, nb1 / nb2 20 / 21
    assert call(-1, 4, 4) == -3 and U.all_sentinel(C)
    assert call(4, -1, 4) == -4 and U.all_sentinel(C)
    assert call(4, 4, -1) == -5 and U.all_sentinel(C)
    assert call(4, 4, 4, nb1=0) == -20 and U.all_sentinel(C)
    assert call(4, 4, 4, nb2=0) == -21 and U.all_sentinel(C)
    assert call(0, 4, 4) == 0 and U.all_sentinel(C)   # m = 0: ok, nothing written
    assert call(4, 0, 4) == 0 and U.all_sentinel(C)
    assert call(4, 4, 4) == 0 and not U.all_sentinel(C)


# ------------------------------------------------------------------------------------------------------
# spd_inv_small
# ------------------------------------------------------------------------------------------------------
def spd_inv(hip, A):
    """The kernel's (Ainv, logdet, info) of the [b, n, n] CPU matrices A (strict upper part replaced by NaN: only
    the lower triangle may be read), with stride, stride_out > n^2 in sentinel buffers."""
    from lvae_amd import _lib as P
    b, n, _ = A.shape
    sa, so = n * n + 7, n * n + 5
    Ab, _ = U.padded(U.nan_upper(A), (sa, n, 1))
    Ob = U.sentinel(U.extent((b, n, n), (so, n, 1)) + 5)
    ld = U.sentinel(b + 3)
    info = U.sentinel(b + 3, torch.int32)
    rc = hip.lvae_spd_inv_small_f64(n, b, P.ptr(Ab), sa, P.ptr(Ob), so, P.ptr(ld), P.ptr(info), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.untouched_outside(Ob, (b, n, n), (so, n, 1))
    assert U.all_sentinel(ld[b:]) and U.all_sentinel(info[b:])
    return U.view(Ob, (b, n, n), (so, n, 1)).cpu(), ld[:b].cpu(), info[:b].cpu()


INV_N = [1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 100, 127, 128]


@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n", INV_N)
def test_spd_inv_small_well_conditioned(hip, n, batch):
    A = U.spd(batch, n, seed=10 * n + batch, cond=1e3)
    Ai, ld, info = spd_inv(hip, A)
    assert int(info.abs().sum()) == 0
    assert torch.equal(Ai, Ai.mT)   # exactly symmetric
    assert U.rel(Ai, torch.linalg.inv(A)) < 1e-12
    assert float((ld - torch.logdet(A)).abs().max()) < 1e-12 * max(1.0, float(torch.logdet(A).abs().max()))


@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n", INV_N)
def test_spd_inv_small_ill_conditioned(hip, n, batch):
    cond = 1e8
    A = U.spd(batch, n, seed=20 * n + batch, cond=cond)
    Ai, ld, info = spd_inv(hip, A)
    assert int(info.abs().sum()) == 0
    assert torch.equal(Ai, Ai.mT)
    eye = torch.eye(n, dtype=F64)
    r_kernel = float((eye - A @ Ai).abs().max())
    r_lapack = float((eye - A @ torch.linalg.inv(A)).abs().max())
    floor = n * 2.0 ** -52 * (cond if n > 1 else 1.0)
    print(f"spd_inv cond 1e8 n={n} batch={batch}: LAPACK {r_lapack:.3e} kernel {r_kernel:.3e} "
          f"ratio {r_kernel / max(r_lapack, 1e-300):.2f} floor {floor:.3e}")
    assert r_kernel <= max(8.0 * r_lapack, floor)


@pytest.mark.parametrize("n", [16, 17, 40, 64, 100, 128])
def test_spd_inv_small_info(hip, n):
    """info = the first non-positive pivot's column + 1, in whichever 16-block it lies; the other batch entries
    are unaffected"""
    for c in sorted({1, 16, 17, n}):
        if c > n:
            continue
        A = U.spd(3, n, seed=30 * n + c, cond=1e3)
        good = A.clone()
        A[1, c - 1, c - 1] = -5.0   # leading minor c fails, the earlier ones are untouched
        Ai, ld, info = spd_inv(hip, A)
        assert info.tolist() == [0, c, 0], (n, c, info.tolist())
        for b in (0, 2):
            assert U.rel(Ai[b], torch.linalg.inv(good[b])) < 1e-12
            assert abs(float(ld[b] - torch.logdet(good[b]))) < 1e-12 * max(1.0, abs(float(torch.logdet(good[b]))))


def test_spd_inv_small_rejections(hip):
    from lvae_amd import _lib as P
    A = torch.eye(4, dtype=F64, device=DEV).reshape(-1)
    Ai, ld, info = U.sentinel(16), U.sentinel(1), U.sentinel(1, torch.int32)

    def call(n, batch):
        rc = hip.lvae_spd_inv_small_f64(n, batch, P.ptr(A), 16, P.ptr(Ai), 16, P.ptr(ld), P.ptr(info), P.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def untouched():
        return U.all_sentinel(Ai) and U.all_sentinel(ld) and U.all_sentinel(info)
    assert call(0, 1) == -1 and untouched()
    assert call(129, 1) == -1 and untouched()
    assert call(4, 0) == 0 and untouched()
    assert call(4, 1) == 0 and not untouched()


# ------------------------------------------------------------------------------------------------------
# natural-gradient update
# ------------------------------------------------------------------------------------------------------
def natgrad(hip, m, H, gm, gH, lr, iH=None):
    """lvae_natgrad_update_f64 on copies of the CPU tensors m [L, M, 1], H [L, M, M]; the workspace is exactly
    lvae_natgrad_workspace_size bytes + a sentinel tail.  Returns (rc, m', H', info)."""
    from lvae_amd import _lib as P
    L, M = H.shape[0], H.shape[-1]
    md, Hd = m.to(DEV).contiguous(), H.to(DEV).contiguous()
    gmd, gHd = gm.to(DEV).contiguous(), gH.to(DEV).contiguous()
    iHd = iH.to(DEV).contiguous() if iH is not None else None
    ws, tail = U.workspace(hip.lvae_natgrad_workspace_size(L, M))
    info = U.sentinel(L + 2, torch.int32)
    rc = hip.lvae_natgrad_update_f64(L, M, P.ptr(md), P.ptr(Hd), P.ptr(gmd), P.ptr(gHd), lr, P.ptr(iHd), P.ptr(info),
                                     P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert U.tail_untouched(tail) and U.all_sentinel(info[L:])
    return rc, md.cpu(), Hd.cpu(), info[:L].cpu()


def natgrad_inputs(L, M, seed):
    g = torch.Generator().manual_seed(seed)
    H = U.spd(L, M, seed, cond=1e2)
    m = torch.randn(L, M, 1, generator=g, dtype=F64)
    gm = torch.randn(L, M, 1, generator=g, dtype=F64)
    X = torch.randn(L, M, M, generator=g, dtype=F64)
    S = torch.randn(L, M, M, generator=g, dtype=F64)
    gH = X @ X.mT / M + 0.05 * (S - S.mT)   # (its symmetric part is positive semi-definite: iH' stays SPD)
    return m, H, gm, gH


@pytest.mark.parametrize("given_iH", [False, True])
@pytest.mark.parametrize("M", [1, 17, 60, 128])
def test_natgrad_update_vs_oracle(hip, M, given_iH):
    L, lr = 3, 0.05
    m, H, gm, gH = natgrad_inputs(L, M, seed=M)
    m_ref, H_ref = O.natural_gradient_update(m, H, gm, gH, lr)
    rc, m2, H2, info = natgrad(hip, m, H, gm, gH, lr, torch.linalg.inv(H) if given_iH else None)
    assert rc == 0 and info.tolist() == [0] * L
    assert U.rel(H2, H_ref) < 1e-7 and U.rel(m2, m_ref) < 1e-7


def failing_grad_H(H, gH, lr, dim=1):
    """gH with gH[dim] = -c I, 2 lr c > lambda_max(H[dim]^-1): iH' = H^-1 + lr (gH + gH^T) is negative definite"""
    M = H.shape[-1]
    iH = torch.linalg.inv(H[dim])
    c = 1.5 * float(torch.linalg.eigvalsh(iH).max()) / (2.0 * lr)
    gH = gH.clone()
    gH[dim] = -c * torch.eye(M, dtype=F64)
    assert float(torch.linalg.eigvalsh(iH + lr * (gH[dim] + gH[dim].T)).max()) < 0.0
    return gH


@pytest.mark.parametrize("given_iH", [False, True])
@pytest.mark.parametrize("M", [20, 60])
def test_natgrad_all_or_nothing(hip, M, given_iH):
    """one dim's iH' not positive definite: NO dim's (m, H) changes (the header's contract)"""
    L, lr = 3, 0.05
    m, H, gm, gH = natgrad_inputs(L, M, seed=100 + M)
    gH = failing_grad_H(H, gH, lr)
    rc, m2, H2, info = natgrad(hip, m, H, gm, gH, lr, torch.linalg.inv(H) if given_iH else None)
    assert rc == 0
    assert int(info[0]) == 0 and int(info[2]) == 0 and int(info[1]) >= 1
    assert torch.equal(m2, m) and torch.equal(H2, H)


@pytest.mark.parametrize("M", [20, 60])
def test_natgrad_H_not_pd_changes_nothing(hip, M):
    """H itself not positive definite in dim 2 (iH = NULL: H is factored here): info[2] is H's own failing column,
    not the first column of the NaN iH' that follows from it, and nothing changes"""
    L, lr = 3, 0.05
    m, H, gm, gH = natgrad_inputs(L, M, seed=200 + M)
    H[2, 3, 3] = -5.0
    rc, m2, H2, info = natgrad(hip, m, H, gm, gH, lr, None)
    assert rc == 0 and info.tolist() == [0, 0, 4]
    assert torch.equal(m2, m) and torch.equal(H2, H)


def test_natgrad_failure_through_python(hip):
    from lvae_amd.elbo import natural_gradient_update, natural_gradient_update_
    L, M, lr = 3, 20, 0.05
    m, H, gm, gH = natgrad_inputs(L, M, seed=300)
    gH = failing_grad_H(H, gH, lr)
    md, Hd, gmd, gHd = m.to(DEV), H.to(DEV), gm.to(DEV), gH.to(DEV)
    with pytest.raises(torch.linalg.LinAlgError):
        natural_gradient_update(md, Hd, gmd, gHd, lr)
    with pytest.raises(torch.linalg.LinAlgError):
        natural_gradient_update_(md, Hd, gmd, gHd, lr)
    assert torch.equal(md.cpu(), m) and torch.equal(Hd.cpu(), H)


def test_natgrad_rejections(hip):
    from lvae_amd import _lib as P
    ws, _ = U.workspace(hip.lvae_natgrad_workspace_size(1, 128))
    buf = U.sentinel(130 * 130)
    info = U.sentinel(1, torch.int32)
    for M in (0, 129):
        rc = hip.lvae_natgrad_update_f64(1, M, P.ptr(buf), P.ptr(buf), P.ptr(buf), P.ptr(buf), 0.1, None, P.ptr(info),
                                         P.ptr(ws), P.stream_ptr())
        torch.cuda.synchronize()
        assert rc == -2 and U.all_sentinel(buf) and U.all_sentinel(info)
