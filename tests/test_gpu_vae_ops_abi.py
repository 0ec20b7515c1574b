"""The ConvVAE kernels of vae_ops.hip through the C ABI, called directly (lvae_amd._lib), at the edges the
module tests of test_gpu_regime_b.py / test_gpu_glue.py do not reach: return codes of every entry point,
H != W and minimal shapes, every form of the pooled weight gradient (conv3x3_pool_wgrad_kernel<1..4>, its
position split with idle threads, the MFMA form and the VALU form inside an MFMA-sized workspace), the grid
thresholds of the MFMA input gradient and of deconv4s2, the retained A/B variants (each set in a fresh child
process: the variables are read once), and NaN through the encoder's fused relu + pool kernels.

Rules of every case: each output is a sentinel buffer (NaN floats, 0x7f bytes) with a tail that must still hold
the sentinel after the call; each workspace has exactly the size its *_workspace_size query returns, 0x7f-filled
(an unwritten partial read back is ~3.4e38 and breaks the value check) with an untouched tail.  References are
fp64 torch on the same inputs (CPU; on the GPU for N in the thousands).  The routed gradient of a pooled layer is
built as test_conv3x3_pool_dgrad_vs_fp64 does: random idx in 0..3, y = randn.clamp_min(0), scattered in fp64 with
the mask ~(y <= 0) (= y > 0 for finite y; a NaN y passes its gradient, torch's threshold_backward).

Tolerances (of the existing tests of the same kernels): pooled values, indices and routed gradients bit-equal to
torch; conv / deconv values and input gradients 1e-5 of the reference's max; deconv2's dw, db 1e-4; the pooled
weight / bias gradients 5e-5; pool-bias db 1e-5.

The argmax byte.  The kernels take the first strict maximum of the window *before* the relu (relu and max
commute), so idx is compared with the indices of max_pool2d(x + b) everywhere, and with those of
max_pool2d(relu(x + b)) -- the element torch routes the gradient to -- wherever y is not 0 (in a window the relu
switches off torch's index is 0, the kernels' the largest negative: no gradient flows there either way).
"""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import abi_util as U
from lvae_amd import _lib as P

pytestmark = pytest.mark.gpu
DEV = U.DEV
F32, U8 = torch.float32, torch.uint8
TAIL = 67
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------
# buffers and calls
# ------------------------------------------------------------------------------------------------------
class Out:
    """A sentinel output buffer: `v` the logical [shape] view, TAIL sentinels behind it."""

    def __init__(self, shape, dtype=F32):
        self.n = int(math.prod(shape))
        self.buf = U.sentinel(self.n + TAIL, dtype)
        self.v = self.buf[:self.n].view(tuple(shape))

    def tail_ok(self):
        return U.all_sentinel(self.buf[self.n:])

    def untouched(self):
        return U.all_sentinel(self.buf)


def call(fn, *args):
    """fn(args..., stream) with tensors / Out buffers passed as device pointers; synchronised."""
    conv = [P.ptr(a.buf) if isinstance(a, Out) else P.ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    rc = fn(*conv, P.stream_ptr())
    torch.cuda.synchronize()
    return rc


def relerr(a, b):
    """max |a - b| / max |b| in fp64 on b's device (NaN when a holds one)"""
    b = b.detach().double()
    a = a.detach().to(b.device).double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def nan_equal(a, b):
    """NaN at the same places, every other element bit-equal"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    return U.bit_equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def window_pos(ind, W):
    """torch's max_pool2d index (flat in the H x W plane) -> the window position 2 dy + dx"""
    return (2 * ((ind // W) % 2) + (ind % W) % 2).to(U8)


def windows(z):
    """[n, c, H, W] -> [n, c, H/2, W/2, 4], last axis in scan order"""
    n, c, H, W = z.shape
    return z.view(n, c, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, H // 2, W // 2, 4)


def routed(gy, y, idx):
    """The full-resolution fp64 gradient of a pooled layer: gy at each window's idx where not y <= 0, else 0"""
    n, c, ho, wo = gy.shape
    g = torch.where(y <= 0, torch.zeros_like(gy), gy).double()
    g0 = torch.zeros(n, c, ho, wo, 4, dtype=torch.float64, device=gy.device)
    g0.scatter_(-1, idx.long().unsqueeze(-1), g.unsqueeze(-1))
    return g0.view(n, c, ho, wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, 2 * ho, 2 * wo)


def pooled_inputs(g, n, c, ho, wo):
    """(gy, y, idx) of a pooled layer: ~half the windows relu'd off, random argmax positions"""
    gy = torch.randn(n, c, ho, wo, generator=g)
    y = torch.randn(n, c, ho, wo, generator=g).clamp_min(0.0)
    idx = torch.randint(0, 4, (n, c, ho, wo), generator=g).to(U8)
    return gy, y, idx


# ------------------------------------------------------------------------------------------------------
# the checks (shared by the tests and by the child processes of the A/B variants)
# ------------------------------------------------------------------------------------------------------
def check_pool(hip, x, b, gy):
    """relu_maxpool2 (b None) / relu_maxpool2_bias fwd + bwd on the CPU tensors x [N, C, H, W], b [C], gy against
    torch's max_pool2d(relu(x + b)) on the CPU: values, indices and the routed gradient bit-equal (NaN-aware),
    db within 1e-5 of its max of the fp64 sum."""
    N, C, H, W = x.shape
    ho, wo = H // 2, W // 2
    pre = (x if b is None else x + b.view(1, -1, 1, 1)).requires_grad_()
    yr, ind = F.max_pool2d(F.relu(pre), 2, 2, return_indices=True)
    _, ind_pre = F.max_pool2d(pre.detach(), 2, 2, return_indices=True)
    yr.backward(gy)
    y, idx, gx = Out((N, C, ho, wo)), Out((N, C, ho, wo), U8), Out((N, C, H, W))
    xd, gyd = x.to(DEV), gy.to(DEV)
    if b is None:
        assert call(hip.lvae_relu_maxpool2_fwd_f32, xd, N * C, H, W, y, idx) == 0
    else:
        bd = b.to(DEV)
        assert call(hip.lvae_relu_maxpool2_bias_fwd_f32, xd, bd, N, C, H, W, y, idx) == 0
    assert y.tail_ok() and idx.tail_ok()
    assert nan_equal(y.v, yr)
    got_idx = idx.v.cpu()
    assert torch.equal(got_idx, window_pos(ind_pre, W))
    live = ~(yr.detach() == 0)
    assert torch.equal(got_idx[live], window_pos(ind, W)[live])
    if b is None:
        assert call(hip.lvae_relu_maxpool2_bwd_f32, gyd, y.v, idx.v, N * C, H, W, gx) == 0
    else:
        db = Out((C,))
        ws, tail = U.workspace(hip.lvae_relu_maxpool2_bias_workspace_size(N, C))
        assert call(hip.lvae_relu_maxpool2_bias_bwd_f32, gyd, y.v, idx.v, N, C, H, W, gx, db, ws) == 0
        assert db.tail_ok() and U.tail_untouched(tail)
        assert relerr(db.v, pre.grad.double().sum((0, 2, 3))) < 1e-5
    assert gx.tail_ok()
    assert nan_equal(gx.v, pre.grad)
    return y.v, idx.v, gx.v


def pool_case(seed, N, C, H, W):
    g = gen(seed)
    x = torch.randn(N, C, H, W, generator=g)
    x[0, 0, :2, :2] = -1.0                 # an all-negative window (and a tie)
    x[N - 1, C - 1, H - 2:, W - 2:] = 0.5  # a positive tie in the last window: the first maximum takes the gradient
    return x, torch.randn(C, generator=g), torch.randn(N, C, H // 2, W // 2, generator=g)


def check_conv_fwd(y, idx, z64):
    """A fused conv + relu + pool forward (y, idx on the GPU) against the fp64 conv output z64: y within 1e-5 of the
    max of max_pool2d(relu(z64)); idx the fp64 argmax wherever the window's top two values are apart by more than
    fp32 rounding (the rule of test_conv3x3_relu_maxpool2_fused_vs_fp64)."""
    ref = F.max_pool2d(F.relu(z64), 2, 2)
    assert relerr(y, ref) < 1e-5
    win = windows(z64)
    top2 = win.topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > 1e-5 * float(z64.abs().max())
    got = idx.to(z64.device).long()
    assert int(got.max()) <= 3
    assert torch.equal(got[clear], win.argmax(-1)[clear])


def check_conv1(hip, seed, N, C, H, W):
    g = gen(seed)
    x = torch.randn(N, 1, H, W, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.5
    b = torch.randn(C, generator=g) * 0.1
    y, idx = Out((N, C, H // 2, W // 2)), Out((N, C, H // 2, W // 2), U8)
    assert call(hip.lvae_conv1_relu_maxpool2_fwd_f32, x.to(DEV), w.to(DEV), b.to(DEV), N, C, H, W, y, idx) == 0
    assert y.tail_ok() and idx.tail_ok()
    check_conv_fwd(y.v, idx.v, F.conv2d(x.double(), w.double(), b.double(), padding=1))


def check_conv2_fwd(hip, seed, N, C, dev="cpu"):
    g = gen(seed)
    x = torch.randn(N, 16, 18, 18, generator=g).clamp_min(0.0)
    w = torch.randn(C, 16, 3, 3, generator=g) * 0.1
    b = torch.randn(C, generator=g) * 0.1
    y, idx = Out((N, C, 9, 9)), Out((N, C, 9, 9), U8)
    assert call(hip.lvae_conv3x3_relu_maxpool2_fwd_f32, x.to(DEV), w.to(DEV), b.to(DEV), N, 16, C, 18, 18, y,
                idx) == 0
    assert y.tail_ok() and idx.tail_ok()
    check_conv_fwd(y.v, idx.v, F.conv2d(x.to(dev).double(), w.to(dev).double(), b.to(dev).double(), padding=1))


def run_dgrad(hip, gy, y, idx, w, H, W):
    N, C = gy.shape[:2]
    gx = Out((N, 16, H, W))
    rc = call(hip.lvae_conv3x3_pool_dgrad_f32, gy.to(DEV), y.to(DEV), idx.to(DEV), w.to(DEV), N, C, 16, H, W, gx)
    assert rc == 0 and gx.tail_ok()
    return gx.v


def check_dgrad(hip, seed, N, C, H, W, dev="cpu"):
    g = gen(seed)
    gy, y, idx = pooled_inputs(g, N, C, H // 2, W // 2)
    w = torch.randn(C, 16, 3, 3, generator=g)
    gx = run_dgrad(hip, gy, y, idx, w, H, W)
    g0 = routed(gy.to(dev), y.to(dev), idx.to(dev))
    ref = torch.nn.grad.conv2d_input((N, 16, H, W), w.to(dev).double(), g0, padding=1)
    assert relerr(gx, ref) < 1e-5, (N, C, H, W)


def run_wgrad(hip, gy, y, idx, x):
    """(dw, db) through a workspace of exactly the queried size; tails checked"""
    N, C, ho, wo = gy.shape
    Cin = x.shape[1]
    dw, db = Out((C, Cin, 3, 3)), Out((C,))
    ws, tail = U.workspace(hip.lvae_conv3x3_pool_wgrad_workspace_size(N, C, Cin))
    rc = call(hip.lvae_conv3x3_pool_wgrad_f32, gy.to(DEV), y.to(DEV), idx.to(DEV), x.to(DEV), N, C, Cin, 2 * ho,
              2 * wo, dw, db, ws)
    assert rc == 0 and dw.tail_ok() and db.tail_ok() and U.tail_untouched(tail), (N, C, Cin, ho, wo)
    return dw.v, db.v


def wgrad_ref(gy, y, idx, x):
    g0 = routed(gy, y, idx)
    C, Cin = gy.shape[1], x.shape[1]
    return torch.nn.grad.conv2d_weight(x.double(), (C, Cin, 3, 3), g0, padding=1), g0.sum((0, 2, 3))


def check_wgrad(hip, seed, N, C, Cin, H, W, dev="cpu"):
    g = gen(seed)
    gy, y, idx = pooled_inputs(g, N, C, H // 2, W // 2)
    x = torch.randn(N, Cin, H, W, generator=g)
    dw, db = run_wgrad(hip, gy, y, idx, x)
    rw, rb = wgrad_ref(gy.to(dev), y.to(dev), idx.to(dev), x.to(dev))
    errs = (relerr(dw, rw), relerr(db, rb))
    assert errs[0] < 5e-5 and errs[1] < 5e-5, (N, C, Cin, H, W, errs)


def check_deconv4s2(hip, seed, N, dev="cpu"):
    """lvae_deconv4s2_relu_fwd / _bwd_f32 against fp64 conv_transpose2d, the gradients through the GPU forward's
    y > 0 mask (test_deconv_relu_fused); every figure within 1e-5."""
    g = gen(seed)
    x = torch.randn(N, 32, 9, 9, generator=g)
    w = torch.randn(32, 16, 4, 4, generator=g) * 0.1
    b = torch.randn(16, generator=g) * 0.1
    gy = torch.randn(N, 16, 18, 18, generator=g)
    xd, wd, bd, gyd = (t.to(DEV) for t in (x, w, b, gy))
    y = Out((N, 16, 18, 18))
    assert call(hip.lvae_deconv4s2_relu_fwd_f32, xd, wd, bd, N, 32, 16, 9, 9, y) == 0
    assert y.tail_ok()
    x64, w64, b64 = (t.to(dev).double().requires_grad_() for t in (x, w, b))
    pre = F.conv_transpose2d(x64, w64, b64, stride=2, padding=1)
    errs = dict(y=relerr(y.v, torch.relu(pre)))
    dx, dw, db = Out((N, 32, 9, 9)), Out((32, 16, 4, 4)), Out((16,))
    ws, tail = U.workspace(hip.lvae_deconv4s2_relu_bwd_workspace_size(N, 32, 16))
    assert call(hip.lvae_deconv4s2_relu_bwd_f32, gyd, y.v, xd, wd, N, 32, 16, 9, 9, dx, dw, db, ws) == 0
    assert dx.tail_ok() and dw.tail_ok() and db.tail_ok() and U.tail_untouched(tail)
    (pre * (y.v.to(dev) > 0).double() * gy.to(dev).double()).sum().backward()
    errs.update(dx=relerr(dx.v, x64.grad), dw=relerr(dw.v, w64.grad), db=relerr(db.v, b64.grad))
    assert all(e < 1e-5 for e in errs.values()), (N, errs)


def check_deconv2(hip, seed, N, Cin, Hi, Wi):
    """lvae_deconv2_sigmoid_fwd / _bwd_f32 against fp64 conv_transpose2d + sigmoid autograd"""
    g = gen(seed)
    z = torch.randn(N, Cin, Hi, Wi, generator=g)
    w = torch.randn(Cin, 1, 4, 4, generator=g) * 0.3
    b = torch.randn(1, generator=g) * 0.3
    gr = torch.randn(N, 1, 2 * Hi, 2 * Wi, generator=g)
    zd, wd, bd, gd = (t.to(DEV) for t in (z, w, b, gr))
    out = Out((N, 1, 2 * Hi, 2 * Wi))
    assert call(hip.lvae_deconv2_sigmoid_fwd_f32, zd, wd, bd, N, Cin, Hi, Wi, out) == 0
    assert out.tail_ok()
    z64, w64, b64 = (t.double().requires_grad_() for t in (z, w, b))
    ref = torch.sigmoid(F.conv_transpose2d(z64, w64, b64, stride=2, padding=1))
    ref.backward(gr.double())
    gz, dw, db = Out((N, Cin, Hi, Wi)), Out((Cin, 1, 4, 4)), Out((1,))
    ws, tail = U.workspace(hip.lvae_deconv2_sigmoid_workspace_size(N, Cin, Hi, Wi))
    assert call(hip.lvae_deconv2_sigmoid_bwd_f32, gd, out.v, zd, wd, N, Cin, Hi, Wi, gz, dw, db, ws) == 0
    assert gz.tail_ok() and dw.tail_ok() and db.tail_ok() and U.tail_untouched(tail)
    errs = dict(out=relerr(out.v, ref), gz=relerr(gz.v, z64.grad), dw=relerr(dw.v, w64.grad),
                db=relerr(db.v, b64.grad))
    tol = dict(out=1e-5, gz=1e-5, dw=1e-4, db=1e-4)
    assert all(errs[k] < tol[k] for k in errs), (N, Cin, Hi, Wi, errs)


# ------------------------------------------------------------------------------------------------------
# return codes
# ------------------------------------------------------------------------------------------------------
# Every launching entry point of vae_ops.hip: the parameters in order, ("name", "in" | "out" | "grad" | "ws", dtype,
# elements) for pointers ("grad": a dw / db the zero-image call writes as zeros over exactly `elements`) and
# ("name", value) for integers, at small valid sizes.  The sweep's calls are all refused or image-free, so no kernel
# reads these buffers.
def _p(name, kind, n=64, dtype=F32):
    return (name, kind, dtype, n)


ENTRIES = {
    "lvae_relu_maxpool2_fwd_f32": [_p("x", "in"), ("planes", 3), ("H", 4), ("W", 6), _p("y", "out"),
                                   _p("idx", "out", 64, U8)],
    "lvae_relu_maxpool2_bwd_f32": [_p("gy", "in"), _p("y", "in"), _p("idx", "in", 64, U8), ("planes", 3), ("H", 4),
                                   ("W", 6), _p("gx", "out", 128)],
    "lvae_conv1_relu_maxpool2_fwd_f32": [_p("x", "in"), _p("w", "in"), _p("bias", "in"), ("N", 2), ("C", 3), ("H", 4),
                                         ("W", 6), _p("y", "out"), _p("idx", "out", 64, U8)],
    "lvae_deconv2_sigmoid_fwd_f32": [_p("z", "in"), _p("w", "in"), _p("bias", "in"), ("N", 2), ("Cin", 3), ("Hi", 2),
                                     ("Wi", 3), _p("out", "out")],
    "lvae_deconv2_sigmoid_bwd_f32": [_p("g", "in"), _p("out", "in"), _p("z", "in"), _p("w", "in"), ("N", 2), ("Cin", 3),
                                     ("Hi", 2), ("Wi", 3), _p("gz", "out"), _p("dw", "grad", 48), _p("db", "grad", 1),
                                     _p("workspace", "ws")],
    "lvae_relu_maxpool2_bias_fwd_f32": [_p("x", "in", 256), _p("bias", "in"), ("N", 2), ("C", 3), ("H", 4), ("W", 6),
                                        _p("y", "out"), _p("idx", "out", 64, U8)],
    "lvae_relu_maxpool2_bias_bwd_f32": [_p("gy", "in"), _p("y", "in"), _p("idx", "in", 64, U8), ("N", 2), ("C", 3),
                                        ("H", 4), ("W", 6), _p("gx", "out", 256), _p("db", "grad", 3),
                                        _p("workspace", "ws")],
    "lvae_conv3x3_pool_wgrad_f32": [_p("gy", "in"), _p("y", "in"), _p("idx", "in", 64, U8), _p("x", "in", 128), ("N", 2),
                                    ("C", 3), ("Cin", 2), ("H", 4), ("W", 6), _p("dw", "grad", 54), _p("db", "grad", 3),
                                    _p("workspace", "ws")],
    "lvae_conv3x3_pool_dgrad_f32": [_p("gy", "in"), _p("y", "in"), _p("idx", "in", 64, U8), _p("w", "in", 512), ("N", 2),
                                    ("C", 3), ("Cin", 16), ("H", 4), ("W", 6), _p("gx", "out", 1024)],
    "lvae_conv3x3_relu_maxpool2_fwd_f32": [_p("x", "in"), _p("w", "in"), _p("bias", "in"), ("N", 2), ("Cin", 16),
                                           ("C", 16), ("H", 18), ("W", 18), _p("y", "out"), _p("idx", "out", 64, U8)],
    "lvae_deconv4s2_relu_fwd_f32": [_p("x", "in"), _p("w", "in"), _p("bias", "in"), ("N", 2), ("Cin", 32), ("Cout", 16),
                                    ("Hi", 9), ("Wi", 9), _p("y", "out")],
    "lvae_deconv4s2_relu_bwd_f32": [_p("gy", "in"), _p("y", "in"), _p("x", "in"), _p("w", "in"), ("N", 2), ("Cin", 32),
                                    ("Cout", 16), ("Hi", 9), ("Wi", 9), _p("dx", "out"), _p("dw", "grad", 8192),
                                    _p("db", "grad", 16), _p("workspace", "ws")],
}
COUNT = ("N", "planes")


def sweep_call(hip, name, over=None, null=None):
    """Call entry `name` at its table sizes with the integer overrides `over` and the pointer `null` passed as a null;
    returns (rc, {pointer name: (kind, buffer, elements)}) of the outputs."""
    over = over or {}
    args, outs = [], {}
    for p in ENTRIES[name]:
        if len(p) == 2:
            args.append(over.get(p[0], p[1]))
            continue
        pname, kind, dtype, n = p
        if kind == "in":
            t = torch.zeros(n, dtype=dtype, device=DEV)
        elif kind == "ws":
            t = U.workspace(4 * n)[0]
        else:
            t = U.sentinel(n + TAIL, dtype)
            outs[pname] = (kind, t, n)
        args.append(None if pname == null else t)
    return call(getattr(hip, name), *args), outs


def outputs_untouched(outs):
    return all(U.all_sentinel(t) for _, t, _ in outs.values())


def _ints(name):
    return [p[0] for p in ENTRIES[name] if len(p) == 2]


NULL_CASES = [(n, p[0]) for n, ps in ENTRIES.items() for p in ps if len(p) == 4]


def test_entry_table_covers_vae_ops():
    """The table names every launching entry point the binding declares for vae_ops.hip"""
    mine = {n for n in P.SIGNATURES if any(k in n for k in ("maxpool2", "deconv", "conv3x3", "conv1_"))
            and not n.endswith(("_workspace_size", "_lds"))}
    assert mine == set(ENTRIES)


@pytest.mark.parametrize("name,pointer", NULL_CASES)
def test_null_pointer_returns_m1(hip, name, pointer):
    rc, outs = sweep_call(hip, name, null=pointer)
    assert rc == -1 and outputs_untouched(outs)


def _bad_values(name):
    """(parameter, value) pairs that must return -2"""
    cases = []
    for q in _ints(name):
        if q in COUNT:
            cases.append((q, -1))
        elif q in ("C", "Cin", "Cout"):
            cases.append((q, 0))
        elif q in ("H", "W"):
            cases += [(q, 5), (q, 1), (q, 0)]
        elif q in ("Hi", "Wi"):
            cases.append((q, 0))
    if "deconv2_sigmoid" in name:
        cases.append(("Cin", 17))
    return cases


BAD_CASES = [(n, q, v) for n in ENTRIES for q, v in _bad_values(n)]


@pytest.mark.parametrize("name,param,value", BAD_CASES)
def test_bad_size_returns_m2(hip, name, param, value):
    rc, outs = sweep_call(hip, name, over={param: value})
    assert rc == -2 and outputs_untouched(outs)


GATES = [
    ("lvae_conv3x3_relu_maxpool2_fwd_f32", dict(Cin=8), -3),
    ("lvae_conv3x3_relu_maxpool2_fwd_f32", dict(H=20, W=20), -3),
    ("lvae_conv3x3_relu_maxpool2_fwd_f32", dict(H=20), -3),
    ("lvae_conv3x3_relu_maxpool2_fwd_f32", dict(C=24), -3),
    ("lvae_deconv4s2_relu_fwd_f32", dict(Cin=16), -3),
    ("lvae_deconv4s2_relu_fwd_f32", dict(Hi=8, Wi=8), -3),
    ("lvae_deconv4s2_relu_fwd_f32", dict(Cout=32), -3),
    ("lvae_deconv4s2_relu_bwd_f32", dict(Cin=16), -3),
    ("lvae_deconv4s2_relu_bwd_f32", dict(Wi=8), -3),
    ("lvae_deconv4s2_relu_bwd_f32", dict(Cout=8), -3),
    ("lvae_conv3x3_pool_dgrad_f32", dict(Cin=5), -3),
    ("lvae_conv3x3_pool_dgrad_f32", dict(C=4, H=34, W=32), -4),     # H W > 1024 (LDS 19.6 KB)
    ("lvae_conv3x3_pool_dgrad_f32", dict(C=15, H=32, W=32), -4),    # 15 * 34 * 34 * 4 B = 69360 B > 64 KB
    ("lvae_conv3x3_pool_wgrad_f32", dict(C=41, Cin=25), -3),        # Q = 1025 pairs: a fifth pass
    ("lvae_conv3x3_pool_wgrad_f32", dict(C=32, Cin=16, H=36, W=36), -4),
    ("lvae_deconv2_sigmoid_fwd_f32", dict(Cin=16, Hi=31, Wi=31), -3),
    ("lvae_deconv2_sigmoid_fwd_f32", dict(Cin=16, Hi=30, Wi=30), -3),  # 16 * 1025 * 4 B = 65600 B
    ("lvae_deconv2_sigmoid_bwd_f32", dict(Cin=1, Hi=57, Wi=57), -3),   # (116^2 + 57^2) * 4 B = 66820 B
    ("lvae_deconv2_sigmoid_bwd_f32", dict(Cin=16, Hi=29, Wi=29), -3),  # (60^2 + 16 * 29^2) * 4 B = 68224 B
]


@pytest.mark.parametrize("name,over,want", GATES)
def test_shape_gates(hip, name, over, want):
    rc, outs = sweep_call(hip, name, over=over)
    assert rc == want and outputs_untouched(outs)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_zero_images(hip, name):
    """N = 0 (planes = 0): rc 0, outputs untouched, the dw / db a backward owns written as zeros"""
    count = [q for q in _ints(name) if q in COUNT][0]
    rc, outs = sweep_call(hip, name, over={count: 0})
    assert rc == 0
    for pname, (kind, t, n) in outs.items():
        if kind == "grad":
            assert float(t[:n].abs().max()) == 0.0 and U.all_sentinel(t[n:]), pname
        else:
            assert U.all_sentinel(t), pname


def test_zero_images_own_their_gradients():
    owners = sorted(n for n, ps in ENTRIES.items() if any(len(p) == 4 and p[1] == "grad" for p in ps))
    assert owners == ["lvae_conv3x3_pool_wgrad_f32", "lvae_deconv2_sigmoid_bwd_f32", "lvae_deconv4s2_relu_bwd_f32",
                      "lvae_relu_maxpool2_bias_bwd_f32"]


def test_workspace_sizes_of_zero_images(hip):
    assert hip.lvae_relu_maxpool2_bias_workspace_size(0, 5) == 0
    assert hip.lvae_conv3x3_pool_wgrad_workspace_size(0, 32, 16) == 0
    assert hip.lvae_deconv2_sigmoid_workspace_size(0, 16, 18, 18) == 0
    assert hip.lvae_deconv4s2_relu_bwd_workspace_size(0, 32, 16) == 0


def test_dgrad_largest_accepted(hip):
    """C = 14 at 32 x 32 (14 * 34 * 34 * 4 B = 64736 B of LDS, 1024 pixels): the last shape the gates accept"""
    check_dgrad(hip, 14, 3, 14, 32, 32)


DECONV2_GRID = [(16, 28, 28), (16, 28, 29), (16, 29, 29), (16, 29, 30), (16, 30, 30), (16, 31, 31), (5, 42, 42),
                (5, 42, 43), (5, 43, 43), (1, 56, 56), (1, 56, 57), (1, 57, 56), (1, 57, 57)]


@pytest.mark.parametrize("cin,hi,wi", DECONV2_GRID)
def test_deconv2_lds_gates_agree(hip, cin, hi, wi):
    """lvae_amd.vae._deconv2_lds_ok (the module's choice of the fused path) against the two gates in C, on shapes
    either side of the forward's bound (Cin = 16: 29 x 30 | 30 x 30) and of the backward's (Cin = 16: 28 x 29 |
    29 x 29; Cin = 5: 42 x 42 | 42 x 43; Cin = 1: 56 x 56 | 56 x 57); one image each"""
    from lvae_amd.vae import _deconv2_lds_ok
    g = gen(cin + hi + wi)
    z = torch.randn(1, cin, hi, wi, generator=g).to(DEV)
    w = (torch.randn(cin, 1, 4, 4, generator=g) * 0.1).to(DEV)
    b = torch.zeros(1, device=DEV)
    s = torch.rand(1, 1, 2 * hi, 2 * wi, generator=g).to(DEV)
    out, gz, dw, db = Out((1, 1, 2 * hi, 2 * wi)), Out((1, cin, hi, wi)), Out((cin, 1, 4, 4)), Out((1,))
    ws, tail = U.workspace(hip.lvae_deconv2_sigmoid_workspace_size(1, cin, hi, wi))
    rf = call(hip.lvae_deconv2_sigmoid_fwd_f32, z, w, b, 1, cin, hi, wi, out)
    rb = call(hip.lvae_deconv2_sigmoid_bwd_f32, s, s, z, w, 1, cin, hi, wi, gz, dw, db, ws)
    assert rf in (0, -3) and rb in (0, -3)
    assert rf == (0 if 4 * cin * (((hi + 2) * (wi + 2)) | 1) <= 65536 else -3)
    assert rb == (0 if 4 * ((2 * hi + 2) * (2 * wi + 2) + cin * hi * wi) <= 65536 else -3)
    assert _deconv2_lds_ok(cin, hi, wi) == (rf == 0 and rb == 0)
    assert out.tail_ok() and gz.tail_ok() and dw.tail_ok() and db.tail_ok() and U.tail_untouched(tail)
    assert out.untouched() == (rf != 0) and gz.untouched() == (rb != 0)
    if rf == 0:
        assert bool(torch.isfinite(out.v).all())
    if rb == 0:
        assert bool(torch.isfinite(gz.v).all() and torch.isfinite(dw.v).all() and torch.isfinite(db.v).all())


# ------------------------------------------------------------------------------------------------------
# non-square and minimal shapes
# ------------------------------------------------------------------------------------------------------
SHAPES = [(2, 2), (2, 6), (6, 2), (6, 10), (10, 6)]


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("N", [3, 37])  # x 7 channels: 21 and 259 planes (an uneven second 256-thread block)
@pytest.mark.parametrize("bias", [False, True])
def test_pool_nonsquare(hip, H, W, N, bias):
    x, b, gy = pool_case(H * 100 + W + N, N, 7, H, W)
    check_pool(hip, x, b if bias else None, gy)


@pytest.mark.parametrize("N", [1, 15, 16, 17, 33])  # around kPoolBiasPer = 16 images per backward block
@pytest.mark.parametrize("C", [1, 5])
def test_pool_bias_bwd_image_chunks(hip, N, C):
    x, b, gy = pool_case(N + C, N, C, 4, 6)
    check_pool(hip, x, b, gy)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("C", [1, 4, 16])
def test_conv1_nonsquare(hip, H, W, C):
    for N in (3, 300):  # (300 images: more than one 256-thread block at every shape)
        check_conv1(hip, H * 100 + W + C, N, C, H, W)


@pytest.mark.parametrize("H,W", [(6, 10), (10, 6)])
@pytest.mark.parametrize("C", [4, 20])
def test_dgrad_valu_nonsquare(hip, H, W, C):
    check_dgrad(hip, H + C, 3, C, H, W)


@pytest.mark.parametrize("Hi,Wi", [(1, 1), (1, 5), (5, 1), (3, 7), (7, 3), (17, 16)])  # 17 x 16: the q += 256 loop
@pytest.mark.parametrize("Cin", [1, 5, 16])
def test_deconv2_nonsquare(hip, Hi, Wi, Cin):
    for N in (1, 3):
        check_deconv2(hip, Hi * 100 + Wi + Cin, N, Cin, Hi, Wi)


# ------------------------------------------------------------------------------------------------------
# the pooled weight gradient, direct
# ------------------------------------------------------------------------------------------------------
# (C, Cin): Q = C Cin pairs -> S = 256 / Q position splits (Q < 256) or NP = ceil(Q / 256) passes
WGRAD_PAIRS = [(4, 16), (6, 8), (2, 3), (16, 16), (20, 15), (24, 24), (32, 32)]


@pytest.mark.parametrize("C,Cin", WGRAD_PAIRS)
def test_wgrad_direct(hip, C, Cin):
    """conv3x3_pool_wgrad_kernel<1..4>: S = 4; S = 5 with 16 idle threads; S = 42 (the 2560-float LDS floor of the
    split reduction: the stage itself is 171 floats at 4 x 6); S = 1; two ragged, three and four passes (Q = 1024, the
    last accepted)"""
    for N in (1, 3, 5):
        for H, W in ((6, 10), (10, 6), (4, 6)):
            check_wgrad(hip, N + H, N, C, Cin, H, W)


@pytest.mark.parametrize("N", [1, 2, 3, 5])
def test_wgrad_mfma_ragged(hip, N):
    """The MFMA form's shape: two images a block (ragged at odd N), four partial rows per block"""
    check_wgrad(hip, N, N, 32, 16, 18, 18)


def test_wgrad_valu_in_mfma_sized_workspace(hip):
    """(C, Cin) = (32, 16) at 6 x 10: lvae_conv3x3_pool_wgrad_workspace_size cannot see H and W and sizes for the MFMA
    form; the launch takes the VALU form and stays inside"""
    for N in (1, 3, 5):
        check_wgrad(hip, N, N, 32, 16, 6, 10)


def test_wgrad_four_images_per_block(hip):
    """N = 2050: four images per block, a ragged last block, two passes; reference on the GPU"""
    check_wgrad(hip, 2050, 2050, 20, 15, 4, 6, dev=DEV)


# ------------------------------------------------------------------------------------------------------
# grid thresholds (the smallest N of each form + a ragged last block); references on the GPU
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1025, 4099])  # 2 and 8 images per block
def test_dgrad_mfma_thresholds(hip, N):
    check_dgrad(hip, N, N, 32, 18, 18, dev=DEV)


@pytest.mark.parametrize("N", [2, 3, 4099])  # a full and a ragged 2-image block; 8 images per block, 3 in the last
def test_deconv4s2_thresholds(hip, N):
    check_deconv4s2(hip, N, N, dev=DEV if N > 100 else "cpu")


# ------------------------------------------------------------------------------------------------------
# the retained A/B variants: read once per process, so each set runs in a fresh child
# ------------------------------------------------------------------------------------------------------
VARIANTS = [
    dict(LVAE_DGRAD_MFMA="0", LVAE_WGRAD_MFMA="0", LVAE_DECONV_MFMA="0", LVAE_CONV2_IPB="2", LVAE_DECONV_IPB="2"),
    dict(LVAE_DGRAD_PAIR="0"),
]


def run_variant_checks():
    """What a child runs: the four layers at N = 5 against the same fp64 references (dgrad at the second conv's shape
    and at one the MFMA form does not take, so that LVAE_DGRAD_PAIR=0 selects a kernel whatever LVAE_DGRAD_MFMA is)"""
    hip = P.lib()
    check_dgrad(hip, 5, 5, 32, 18, 18)
    check_dgrad(hip, 6, 5, 20, 6, 10)
    check_wgrad(hip, 5, 5, 32, 16, 18, 18)
    check_conv2_fwd(hip, 5, 5, 32)
    check_deconv4s2(hip, 5, 5)
    print("variant checks passed")


def test_retained_variants(hip):
    """Two children, one after the other, each with its own timeout and a disjoint set of the variables.  A child
    that fails, ends on a signal or runs out of time fails the test at once: the next one is not started."""
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here] + [p for p in sys.path if p]
    for env_set in VARIANTS:
        env = dict(os.environ, PYTHONPATH=os.pathsep.join(paths), **env_set)
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
            "-c", "import test_gpu_vae_ops_abi as T; T.run_variant_checks()"]
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=180)
        except subprocess.TimeoutExpired:
            pytest.fail(f"variant child {env_set} hit its timeout")
        assert r.returncode >= 0, f"variant child {env_set} ended on signal {-r.returncode}\n{r.stderr[-2000:]}"
        assert r.returncode == 0 and "variant checks passed" in r.stdout, f"{env_set}\n{r.stdout}\n{r.stderr[-4000:]}"


# ------------------------------------------------------------------------------------------------------
# NaN: the encoder's fused kernels keep it, as torch's max_pool2d(relu(.)) and threshold_backward do
# ------------------------------------------------------------------------------------------------------
NAN_SPOTS = [(0,), (1,), (2,), (3,), (1, 3), (0, 2)]  # window positions (scan order) that hold a NaN


def nan_pool_case(spots):
    """x [2, 3, 4, 6] finite and moderate, with NaN at `spots` of window (1, 1) of plane (1, 2)"""
    x, b, gy = pool_case(sum(spots) + 10 * len(spots), 2, 3, 4, 6)
    for k in spots:
        x[1, 2, 2 + k // 2, 2 + k % 2] = NAN
    return x, b, gy


@pytest.mark.parametrize("spots", NAN_SPOTS)
@pytest.mark.parametrize("bias", [False, True])
def test_pool_nan(hip, spots, bias):
    """lvae_relu_maxpool2_bias_fwd / _bwd_f32 and, without a bias, lvae_relu_maxpool2_fwd / _bwd_f32: y is NaN exactly
    where torch's is, idx is torch's (the last NaN of the window), the gradient passes at that element"""
    x, b, gy = nan_pool_case(spots)
    y, idx, gx = check_pool(hip, x, b if bias else None, gy)
    assert bool(torch.isnan(y[1, 2, 1, 1])) and int(torch.isnan(y).sum()) == 1
    assert int(idx[1, 2, 1, 1]) == spots[-1]
    win = gx[1, 2, 2:4, 2:4].reshape(4).cpu()
    want = torch.zeros(4)
    want[spots[-1]] = gy[1, 2, 1, 1]
    assert torch.equal(win, want)


@pytest.mark.parametrize("spots", NAN_SPOTS)
def test_relu_maxpool2_module_nan(hip, spots):
    """lvae_amd.vae.relu_maxpool2 (the autograd function) on a NaN input against torch on the GPU"""
    from lvae_amd.vae import relu_maxpool2
    x, _, gy = nan_pool_case(spots)
    xa, xb = x.to(DEV).requires_grad_(), x.to(DEV).requires_grad_()
    ya, yb = relu_maxpool2(xa), F.max_pool2d(F.relu(xb), 2, 2)
    assert nan_equal(ya, yb) and bool(torch.isnan(ya[1, 2, 1, 1]))
    ya.backward(gy.to(DEV))
    yb.backward(gy.to(DEV))
    assert nan_equal(xa.grad, xb.grad)
    assert float(xa.grad[1, 2, 2 + spots[-1] // 2, 2 + spots[-1] % 2]) == float(gy[1, 2, 1, 1])


def check_conv_nan(y, idx, z64):
    """NaN mask of y = that of fp64 max_pool2d(relu(conv)); idx at a NaN window = its last NaN conv output; the
    other windows within 1e-5 of the finite maximum"""
    ref = F.max_pool2d(F.relu(z64), 2, 2)
    nan_ref = torch.isnan(ref)
    assert bool(nan_ref.any()) and not bool(nan_ref.all())
    yc = y.cpu()
    assert torch.equal(torch.isnan(yc), nan_ref)
    nan_win = torch.isnan(windows(z64))
    assert torch.equal(nan_win.any(-1), nan_ref)
    last = 3 - nan_win.flip(-1).int().argmax(-1)
    assert torch.equal(idx.cpu().long()[nan_ref], last[nan_ref])
    fin = ~nan_ref
    assert float((yc.double()[fin] - ref[fin]).abs().max()) < 1e-5 * float(ref[fin].abs().max())


@pytest.mark.parametrize("what", ["pixel", "weight"])
@pytest.mark.parametrize("H,W", [(6, 10), (10, 6)])
def test_conv1_nan(hip, what, H, W):
    g = gen(H)
    N, C = 3, 4
    x = torch.randn(N, 1, H, W, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.5
    b = torch.randn(C, generator=g) * 0.1
    if what == "pixel":
        x[1, 0, 3, 2] = NAN   # conv outputs of rows 2..4, columns 1..3 of image 1, every channel
    else:
        w[2, 0, 1, 1] = NAN   # the centre tap: every output of channel 2
    y, idx = Out((N, C, H // 2, W // 2)), Out((N, C, H // 2, W // 2), U8)
    assert call(hip.lvae_conv1_relu_maxpool2_fwd_f32, x.to(DEV), w.to(DEV), b.to(DEV), N, C, H, W, y, idx) == 0
    check_conv_nan(y.v, idx.v, F.conv2d(x.double(), w.double(), b.double(), padding=1))


@pytest.mark.parametrize("what", ["pixel", "weight"])
def test_conv3x3_fused_nan(hip, what):
    g = gen(7)
    N, C = 3, 32
    x = torch.randn(N, 16, 18, 18, generator=g).clamp_min(0.0)
    w = torch.randn(C, 16, 3, 3, generator=g) * 0.1
    b = torch.randn(C, generator=g) * 0.1
    if what == "pixel":
        x[2, 5, 7, 10] = NAN
    else:
        w[17, 3, 1, 1] = NAN
    y, idx = Out((N, C, 9, 9)), Out((N, C, 9, 9), U8)
    assert call(hip.lvae_conv3x3_relu_maxpool2_fwd_f32, x.to(DEV), w.to(DEV), b.to(DEV), N, 16, C, 18, 18, y,
                idx) == 0
    check_conv_nan(y.v, idx.v, F.conv2d(x.double(), w.double(), b.double(), padding=1))


# wgrad / dgrad forms: (C, Cin, H, W) -> the VALU kernels and the MFMA ones
@pytest.mark.parametrize("C,Cin,H,W", [(6, 8, 6, 10), (20, 15, 4, 6), (32, 16, 18, 18)])
def test_wgrad_nan_y_routes(hip, C, Cin, H, W):
    """A NaN y passes its window's gradient into dw and db (the mask ~(y <= 0))"""
    g = gen(C)
    N = 3
    gy, y, idx = pooled_inputs(g, N, C, H // 2, W // 2)
    x = torch.randn(N, Cin, H, W, generator=g)
    y[1, C - 1, 1, 2] = NAN
    gy[1, C - 1, 1, 2] = 3.0
    dw, db = run_wgrad(hip, gy, y, idx, x)
    rw, rb = wgrad_ref(gy, y, idx, x)
    dropped = wgrad_ref(gy, torch.nan_to_num(y, nan=0.0), idx, x)
    assert abs(float(rb[C - 1] - dropped[1][C - 1]) - 3.0) < 1e-12  # (the reference itself routes it)
    assert relerr(dw, rw) < 5e-5 and relerr(db, rb) < 5e-5


@pytest.mark.parametrize("C,H,W", [(20, 6, 10), (32, 18, 18)])
def test_dgrad_nan_y_routes(hip, C, H, W):
    g = gen(C)
    N = 3
    gy, y, idx = pooled_inputs(g, N, C, H // 2, W // 2)
    w = torch.randn(C, 16, 3, 3, generator=g)
    y[2, 1, 2, 1] = NAN
    gy[2, 1, 2, 1] = 3.0
    gx = run_dgrad(hip, gy, y, idx, w, H, W)
    ref = torch.nn.grad.conv2d_input((N, 16, H, W), w.double(), routed(gy, y, idx), padding=1)
    drop = torch.nn.grad.conv2d_input((N, 16, H, W), w.double(), routed(gy, torch.nan_to_num(y, nan=0.0), idx),
                                      padding=1)
    assert float((ref - drop).abs().max()) > 1e-2 * float(ref.abs().max())
    assert relerr(gx, ref) < 1e-5


def test_convvae_nan_pixel_reaches_the_loss(hip):
    """One NaN input pixel: the image's mse is NaN (a diverged encoder must not yield a finite loss); the other
    image's stays finite"""
    from lvae_amd.vae import ConvVAE
    torch.manual_seed(0)
    vae = ConvVAE(4, 1296).to(DEV).eval()
    clean = torch.rand(2, 1, 36, 36, device=DEV)
    x = clean.clone()
    x[0, 0, 17, 20] = NAN
    with torch.no_grad():
        recon, mu, _ = vae(x, eps=torch.zeros(2, 4, device=DEV))
        mse, _ = vae.loss_function(recon, clean, torch.ones_like(clean))
    assert bool(torch.isnan(mu[0]).all()) and bool(torch.isfinite(mu[1]).all())
    assert bool(torch.isnan(mse[0])) and bool(torch.isfinite(mse[1]))
