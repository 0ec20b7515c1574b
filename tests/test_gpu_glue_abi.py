"""The glue launches of glue.hip through the C ABI, called directly (lvae_amd._lib): return codes of every entry
point, the loss at d and B around its 256-thread / 64-image tiles with strided output gradients, reparam around
one block, the Hensman step's loss terms with each optional gradient absent, act_bwd on both of its kernels
around their 64-row / 64-column / 256-pixel tiles, bias_relu_fwd, and param_pack's refusals.

Every output is a sentinel buffer whose tail must survive the call; act_bwd's workspace has exactly the queried
size.  References are fp64 torch on the CPU.  Tolerances: the loss 2e-5 and reparam 1e-6 (test_gpu_glue.py's);
an fp32 sum of n terms x_i is allowed n 2^-24 sum |x_i| (the standard bound of recursive summation, which covers
any order; a factor applied to the sum scales the bound and its one rounding is inside it for n >= 1); fp64 outputs
formed by at most three operations are allowed 4 * 2^-53 relative.  act_bwd's g and bias_relu_fwd's y are bit-equal
to torch (threshold_backward / relu), a NaN included.
"""
import ctypes

import pytest
import torch

import abi_util as U
from lvae_amd import _lib as P
from test_gpu_glue import _loss_ref
from test_gpu_vae_ops_abi import Out, call, gen, nan_equal, relerr

pytestmark = pytest.mark.gpu
DEV = U.DEV
F32, F64 = torch.float32, torch.float64
U32, U64 = 2.0 ** -24, 2.0 ** -53
NAN = float("nan")


def dev(*ts):
    return [t.to(DEV) for t in ts]


def dev1(*ts):
    """Flat device copies with at least one element each (an empty input still has a non-null pointer)"""
    out = []
    for t in ts:
        buf = torch.zeros(max(t.numel(), 1), dtype=t.dtype, device=DEV)
        buf[:t.numel()] = t.reshape(-1).to(DEV)
        out.append(buf)
    return out


# ------------------------------------------------------------------------------------------------------
# return codes
# ------------------------------------------------------------------------------------------------------
def _t(n=64, dtype=F32):
    return torch.zeros(n, dtype=dtype, device=DEV)


def _sweep(fn, args, pointers, bad):
    """args: the valid argument list (tensors / Out / numbers); pointers: indices that must return -1 when null;
    bad: (index, value) pairs that must return -2.  Outputs stay all-sentinel throughout."""
    outs = [a for a in args if isinstance(a, Out)]
    for i in pointers:
        assert call(fn, *[None if j == i else a for j, a in enumerate(args)]) == -1, i
    for i, v in bad:
        assert call(fn, *[v if j == i else a for j, a in enumerate(args)]) == -2, (i, v)
    assert all(o.untouched() for o in outs)


def test_return_codes(hip):
    _sweep(hip.lvae_vae_loss_fwd_f32, [_t(), _t(), _t(), _t(), 2, 5, Out((2,)), Out((2,)), Out((2,))],
           [0, 1, 2, 3, 6, 7, 8], [(4, -1), (5, 0), (5, -3)])
    _sweep(hip.lvae_vae_loss_bwd_f32, [_t(), _t(), _t(), _t(), _t(), _t(), 1, _t(), 1, 2, 5, Out((10,)), Out((5,))],
           [0, 1, 2, 3, 4, 5, 7, 11, 12], [(9, -1), (10, 0)])
    _sweep(hip.lvae_reparam_fwd_f32, [_t(), _t(), _t(), 7, Out((7,))], [0, 1, 2, 4], [(3, -1)])
    _sweep(hip.lvae_reparam_bwd_f32, [_t(), _t(), _t(), 7, Out((7,))], [0, 1, 2, 4], [(3, -1)])
    _sweep(hip.lvae_step_terms_fwd, [_t(), _t(), 3, _t(1, F64), 1.0, 1.0, 1.0, 0, Out((1,)), Out((1,)), Out((1,), F64),
                                    Out((1,), F64)], [0, 1, 3, 8, 9, 10, 11], [(2, -1)])
    _sweep(hip.lvae_step_terms_bwd, [_t(1, F64), _t(1), _t(1), _t(1, F64), 1.0, 1.0, 1.0, 0, Out((1,)), Out((1,)),
                                    Out((1,), F64)], [8, 9, 10], [])
    y = Out((12,))
    _sweep(hip.lvae_bias_relu_fwd_f32, [y, _t(), 2, 3, 2], [0, 1], [(2, -1), (3, 0), (4, 0)])
    ws = U.workspace(hip.lvae_act_bwd_workspace_size(2, 3))[0]
    _sweep(hip.lvae_act_bwd_f32, [_t(), _t(), 2, 3, 2, 1, Out((12,)), Out((3,)), ws], [0, 1, 6, 7, 8],
           [(2, -1), (3, 0), (4, 0)])
    # without the relu, y and g may be absent; gy, db and the workspace may not
    _sweep(hip.lvae_act_bwd_f32, [_t(), None, 2, 3, 2, 0, None, Out((3,)), ws], [0, 7, 8], [(2, -1)])


def test_zero_sizes(hip):
    """B = 0 / n = 0 / N = 0: rc 0 and nothing written (act_bwd writes db as zeros, step_terms its zero sums)"""
    o = [Out((4,)) for _ in range(3)]
    assert call(hip.lvae_vae_loss_fwd_f32, _t(), _t(), _t(), _t(), 0, 5, *o) == 0
    o += [Out((4,)), Out((4,))]
    assert call(hip.lvae_vae_loss_bwd_f32, _t(), _t(), _t(), _t(), _t(), _t(), 1, _t(), 1, 0, 5, o[3], o[4]) == 0
    assert hip.lvae_vae_loss_bwd_partials(0) == 0
    o += [Out((4,)), Out((4,)), Out((4,))]
    assert call(hip.lvae_reparam_fwd_f32, _t(), _t(), _t(), 0, o[5]) == 0
    assert call(hip.lvae_reparam_bwd_f32, _t(), _t(), _t(), 0, o[6]) == 0
    assert call(hip.lvae_bias_relu_fwd_f32, o[7], _t(), 0, 3, 2) == 0
    assert all(x.untouched() for x in o)
    db, g = Out((3,)), Out((4,))
    assert hip.lvae_act_bwd_workspace_size(0, 3) == 0
    assert call(hip.lvae_act_bwd_f32, _t(), _t(), 0, 3, 2, 1, g, db, U.workspace(0)[0]) == 0
    assert float(db.v.abs().max()) == 0.0 and db.tail_ok() and g.untouched()


def _pack_args(cols, raws, mlogs):
    n = len(cols)
    ca = (ctypes.c_int32 * max(n, 1))(*cols)
    ra = (ctypes.c_void_p * max(n, 1))(*[None if r is None else r.data_ptr() for r in raws])
    ma = (ctypes.c_void_p * max(n, 1))(*[None if m is None else m.data_ptr() for m in mlogs])
    return ca, ra, ma


def _pack_fwd(hip, n, L, Pn, ca, ra, ma, out):
    rc = hip.lvae_param_pack_fwd_f64(n, L, Pn, ca, ra, ma, None if out is None else P.ptr(out.buf), P.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _pack_bwd(hip, n, L, Pn, ca, ra, ma, g, gs0, gs1, grad):
    rc = hip.lvae_param_pack_bwd_f64(n, L, Pn, ca, ra, ma, None if g is None else P.ptr(g), gs0, gs1,
                                     None if grad is None else P.ptr(grad.buf), P.stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_param_pack_abi(hip):
    L, Pn = 3, 4
    g0 = gen(0)
    raws = dev(torch.randn(L, generator=g0, dtype=F64), torch.tensor([30.0, -2.0, 0.5], dtype=F64))
    mlogs = dev(torch.tensor([-3.0], dtype=F64), torch.tensor([0.25], dtype=F64))
    cols = [2, 0]
    ca, ra, ma = _pack_args(cols, raws, mlogs)
    out, grad = Out((L, Pn), F64), Out((2, L), F64)
    gbuf, g = U.padded(torch.randn(L, Pn, generator=g0, dtype=F64), (11, 2))  # (both gradient strides in use)
    # refusals: nothing written
    assert _pack_fwd(hip, 2, L, Pn, ca, ra, ma, None) == -1
    assert _pack_fwd(hip, 2, L, Pn, None, ra, ma, out) == -1
    assert _pack_fwd(hip, 2, L, Pn, ca, None, ma, out) == -1
    assert _pack_fwd(hip, 2, L, Pn, ca, ra, None, out) == -1
    assert _pack_bwd(hip, 2, L, Pn, ca, ra, ma, None, 11, 2, grad) == -1
    assert _pack_bwd(hip, 2, L, Pn, ca, ra, ma, gbuf, 11, 2, None) == -1
    for n, l, p in ((65, L, Pn), (2, L, 65), (-1, L, Pn), (2, 0, Pn), (2, L, 0)):
        assert _pack_fwd(hip, n, l, p, ca, ra, ma, out) == -2, (n, l, p)
        assert _pack_bwd(hip, n, l, p, ca, ra, ma, gbuf, 11, 2, grad) == -2, (n, l, p)
    bad_col = _pack_args([2, Pn], raws, mlogs)
    null_raw = _pack_args(cols, [raws[0], None], mlogs)
    null_mlog = _pack_args(cols, raws, [None, mlogs[1]])
    for bad in (bad_col, null_raw, null_mlog, _pack_args([-1, 0], raws, mlogs)):
        assert _pack_fwd(hip, 2, L, Pn, *bad, out) == -3
        assert _pack_bwd(hip, 2, L, Pn, *bad, gbuf, 11, 2, grad) == -3
    assert out.untouched() and grad.untouched()
    # no raw parameter: all ones forward (the arrays may be absent), a no-op backward
    assert _pack_fwd(hip, 0, L, Pn, None, None, None, out) == 0
    assert torch.equal(out.v.cpu(), torch.ones(L, Pn, dtype=F64)) and out.tail_ok()
    assert _pack_bwd(hip, 0, L, Pn, None, None, None, gbuf, 11, 2, grad) == 0 and grad.untouched()
    # values, with a strided g
    out = Out((L, Pn), F64)
    assert _pack_fwd(hip, 2, L, Pn, ca, ra, ma, out) == 0 and out.tail_ok()
    assert _pack_bwd(hip, 2, L, Pn, ca, ra, ma, gbuf, 11, 2, grad) == 0 and grad.tail_ok()
    r64 = [r.cpu().requires_grad_() for r in raws]
    cols_ref = {c: torch.exp(m.cpu() + torch.nn.functional.softplus(r - m.cpu())) for c, r, m in zip(cols, r64, mlogs)}
    ref = torch.stack([cols_ref.get(c, torch.ones(L, dtype=F64)) for c in range(Pn)], 1)
    (ref * g.cpu()).sum().backward()
    assert relerr(out.v, ref) < 1e-15
    assert relerr(grad.v, torch.stack([r.grad for r in r64])) < 1e-13


# ------------------------------------------------------------------------------------------------------
# vae_loss, reparam
# ------------------------------------------------------------------------------------------------------
def _strided_grad(values, stride):
    """(device buffer, fp64 values the kernel sees) of a [B] output gradient passed with `stride`"""
    if stride == 0:
        return U.padded(values[:1], (1,))[0], values[:1].double().expand(values.shape[0])
    return U.padded(values, (stride,))[0], values.double()


@pytest.mark.parametrize("d", [1, 5, 255, 256, 257])
@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_vae_loss_direct(hip, B, d):
    g0 = gen(B * 1000 + d)
    r, x = torch.rand(B, d, generator=g0), torch.rand(B, d, generator=g0)
    m = (torch.rand(B, d, generator=g0) > 0.2).float()
    m[0] = 0.0  # an all-zero mask: msum -> 1
    lv = 0.3 * torch.randn(d, generator=g0)
    rd, xd, md, lvd = dev(r, x, m, lv)
    mse, nll, msum = Out((B,)), Out((B,)), Out((B,))
    assert call(hip.lvae_vae_loss_fwd_f32, rd, xd, md, lvd, B, d, mse, nll, msum) == 0
    assert mse.tail_ok() and nll.tail_ok() and msum.tail_ok()
    r64, lv64 = r.double().requires_grad_(), lv.double().requires_grad_()
    mse_r, nll_r = _loss_ref(r64, x.double(), m.double(), lv64)
    assert relerr(mse.v, mse_r) < 2e-5 and relerr(nll.v, nll_r) < 2e-5
    assert torch.equal(msum.v.cpu(), m.sum(1).clamp_min(1.0))
    rows = int(hip.lvae_vae_loss_bwd_partials(B))
    assert rows == (B + 63) // 64
    gm, gn = torch.rand(B, generator=g0) + 0.1, torch.rand(B, generator=g0) + 0.1
    for sm, sn in ((1, 1), (0, 3), (3, 0), (0, 0)):
        gmb, gm64 = _strided_grad(gm, sm)
        gnb, gn64 = _strided_grad(gn, sn)
        dr, part = Out((B, d)), Out((rows, d))
        assert call(hip.lvae_vae_loss_bwd_f32, rd, xd, md, lvd, msum.v, gmb, sm, gnb, sn, B, d, dr, part) == 0
        assert dr.tail_ok() and part.tail_ok()
        r64.grad = lv64.grad = None
        mse_r, nll_r = _loss_ref(r64, x.double(), m.double(), lv64)
        ((mse_r * gm64).sum() + (nll_r * gn64).sum()).backward()
        errs = (relerr(dr.v, r64.grad), relerr(part.v.sum(0), lv64.grad))
        assert errs[0] < 2e-5 and errs[1] < 2e-5, (B, d, sm, sn, errs)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_reparam_direct(hip, n):
    g0 = gen(n)
    mu, lv, eps, gz = (torch.randn(n, generator=g0) for _ in range(4))
    z, glv = Out((n,)), Out((n,))
    assert call(hip.lvae_reparam_fwd_f32, *dev1(mu, lv, eps), n, z) == 0
    assert call(hip.lvae_reparam_bwd_f32, *dev1(gz, lv, eps), n, glv) == 0
    assert z.tail_ok() and glv.tail_ok()
    if n == 0:
        assert z.untouched() and glv.untouched()
        return
    s = torch.exp(0.5 * lv.double())
    assert relerr(z.v, mu.double() + eps.double() * s) < 1e-6
    assert relerr(glv.v, 0.5 * gz.double() * eps.double() * s) < 1e-6


# ------------------------------------------------------------------------------------------------------
# step_terms (training.py:100-120): rec = c sum mse, nl = c sum nll (fp32), kd = ks kld (fp64),
# net = use_nll ? nl + kd : rec + w kd
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [0, 1, 255, 256, 257, 1000])
@pytest.mark.parametrize("use_nll", [0, 1])
def test_step_terms_fwd(hip, B, use_nll):
    g0 = gen(B)
    mse, nll = torch.rand(B, generator=g0), torch.randn(B, generator=g0) * 50.0
    kld = torch.tensor([37.25], dtype=F64)
    c = float(torch.tensor(0.37, dtype=F32))  # (passed as a C float: a value fp32 holds exactly)
    ks, w = 1.0 / 3.0, 0.7
    rec, nl, net, kd = Out((1,)), Out((1,)), Out((1,), F64), Out((1,), F64)
    assert call(hip.lvae_step_terms_fwd, *dev1(mse, nll), B, kld.to(DEV), c, ks, w, use_nll, rec, nl, net, kd) == 0
    assert rec.tail_ok() and nl.tail_ok() and net.tail_ok() and kd.tail_ok()
    rec_r, nl_r = c * float(mse.double().sum()), c * float(nll.double().sum())
    kd_r = ks * float(kld)
    b_rec = B * U32 * abs(c) * float(mse.double().abs().sum())
    b_nl = B * U32 * abs(c) * float(nll.double().abs().sum())
    assert abs(float(rec.v) - rec_r) <= b_rec and abs(float(nl.v) - nl_r) <= b_nl
    assert abs(float(kd.v) - kd_r) <= 4 * U64 * abs(kd_r)
    net_r = nl_r + kd_r if use_nll else rec_r + w * kd_r
    b_net = (b_nl if use_nll else b_rec) + 4 * U64 * (abs(nl_r if use_nll else rec_r) + abs(kd_r))
    assert abs(float(net.v) - net_r) <= b_net


@pytest.mark.parametrize("use_nll", [0, 1])
def test_step_terms_bwd(hip, use_nll):
    """Each optional output gradient absent in turn, and all of them: an absent one counts as zero"""
    c = float(torch.tensor(0.37, dtype=F32))
    ks, w = 1.0 / 3.0, 0.7
    vals = dict(g_net=1.75, g_rec=0.6, g_nl=0.3, g_kd=2.5)  # (all positive: no cancellation in the sums)
    tens = dict(g_net=torch.tensor([vals["g_net"]], dtype=F64), g_rec=torch.tensor([vals["g_rec"]]),
                g_nl=torch.tensor([vals["g_nl"]]), g_kd=torch.tensor([vals["g_kd"]], dtype=F64))
    tens = {k: v.to(DEV) for k, v in tens.items()}
    for absent in [(), ("g_net",), ("g_rec",), ("g_nl",), ("g_kd",), tuple(vals)]:
        a = {k: (None if k in absent else tens[k]) for k in tens}
        v = {k: (0.0 if k in absent else float(tens[k])) for k in tens}
        g_mse, g_nll, g_kld = Out((1,)), Out((1,)), Out((1,), F64)
        assert call(hip.lvae_step_terms_bwd, a["g_net"], a["g_rec"], a["g_nl"], a["g_kd"], c, ks, w, use_nll, g_mse,
                    g_nll, g_kld) == 0
        assert g_mse.tail_ok() and g_nll.tail_ok() and g_kld.tail_ok()
        r_mse = c * ((0.0 if use_nll else v["g_net"]) + v["g_rec"])
        r_nll = c * ((v["g_net"] if use_nll else 0.0) + v["g_nl"])
        r_kld = ks * ((v["g_net"] if use_nll else w * v["g_net"]) + v["g_kd"])
        # fp32: the fp64 gradient rounded, the fp32 input's own rounding, one add, one multiply
        assert abs(float(g_mse.v) - r_mse) <= 4 * U32 * abs(r_mse), absent
        assert abs(float(g_nll.v) - r_nll) <= 4 * U32 * abs(r_nll), absent
        assert abs(float(g_kld.v) - r_kld) <= 4 * U64 * abs(r_kld), absent


# ------------------------------------------------------------------------------------------------------
# act_bwd, bias_relu_fwd
# ------------------------------------------------------------------------------------------------------
def check_act_bwd(hip, N, C, HW, relu):
    g0 = gen(N * 1000 + C + HW)
    gy = torch.randn(N, C, HW, generator=g0)
    y = torch.randn(N, C, HW, generator=g0).clamp_min(0.0)
    y[0, 0, 0] = NAN           # passes its gradient
    y[N - 1, C - 1, HW - 1] = -1.0
    g, db = Out((N, C, HW)), Out((C,))
    ws, tail = U.workspace(hip.lvae_act_bwd_workspace_size(N, C))
    assert hip.lvae_act_bwd_workspace_size(N, C) == 4 * C * ((N + 63) // 64)
    if relu:
        rc = call(hip.lvae_act_bwd_f32, gy.to(DEV), y.to(DEV), N, C, HW, 1, g, db, ws)
        ref = torch.ops.aten.threshold_backward(gy, y, 0.0)
        assert g.tail_ok() and U.bit_equal(g.v.cpu(), ref)
    else:
        rc = call(hip.lvae_act_bwd_f32, gy.to(DEV), None, N, C, HW, 0, None, db, ws)
        ref = gy
    assert rc == 0 and db.tail_ok() and U.tail_untouched(tail)
    r64 = ref.double()
    excess = (db.v.cpu().double() - r64.sum((0, 2))).abs() - N * HW * U32 * r64.abs().sum((0, 2))
    assert not bool(torch.isnan(db.v).any()) and float(excess.max()) <= 0.0, (N, C, HW, relu, float(excess.max()))


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
def test_act_bwd_rows(hip, N, relu):
    for C in (1, 63, 64, 65, 300):
        check_act_bwd(hip, N, C, 1, relu)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("HW", [2, 81, 255, 256, 257])
def test_act_bwd_channels(hip, HW, relu):
    for N in (1, 65):
        for C in (1, 3, 16):
            check_act_bwd(hip, N, C, HW, relu)


@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("HW", [1, 7])
def test_bias_relu_fwd(hip, C, HW):
    g0 = gen(C + HW)
    N = 3
    y0 = torch.randn(N, C, HW, generator=g0)
    y0[1, C - 1, HW - 1] = NAN
    b = torch.randn(C, generator=g0)
    y = Out((N, C, HW))
    y.v.copy_(y0)
    assert call(hip.lvae_bias_relu_fwd_f32, y, b.to(DEV), N, C, HW) == 0
    assert y.tail_ok()
    ref = torch.relu(y0 + b.view(1, C, 1))
    assert bool(torch.isnan(ref[1, C - 1, HW - 1])) and nan_equal(y.v, ref)
