"""Conv encoder / decoder of the L-VAE (VAE.py:16-162), on PyTorch-ROCm (MIOpen / hipBLASLt).

Same layer names and shapes as the reference's ConvVAE so its state dicts load unchanged.  The
reference runs it in fp64 (LVAE.py:139-140, 152); here it runs in the dtype of its parameters
(fp32 by default: mu / logvar drift ~1e-7 relative vs fp64).
"""
import math
import os

import torch
import torch.nn.functional as F
from torch import nn


# LVAE_CONV_DGRAD=0: the second encoder conv's input gradient on MIOpen (routed gradient + backward-data conv)
# instead of lvae_conv3x3_pool_dgrad_f32 (A/B runs)
_CONV_DGRAD = os.environ.get("LVAE_CONV_DGRAD", "1") != "0"
# LVAE_CONV_BWD_FORK=0: that layer's weight-gradient and input-gradient kernels one after the other on the
# backward's stream instead of side by side (the weight gradient on a side stream, joined before returning)
_CONV_BWD_FORK = os.environ.get("LVAE_CONV_BWD_FORK", "1") != "0"
# LVAE_CONV_FUSED=0: the second encoder conv's forward and the first decoder transposed conv (forward and backward)
# on MIOpen (+ the fused bias / relu / pool passes) instead of the direct HIP kernels (vae_ops.hip)
_CONV2_FUSED = os.environ.get("LVAE_CONV_FUSED", "1") != "0"
_SIDE_STREAMS = {}


def _side_stream(dev):
    s = _SIDE_STREAMS.get(dev)
    if s is None:
        s = _SIDE_STREAMS[dev] = torch.cuda.Stream(device=dev)
    return s


def lend_early_stream(dev):
    """Lend the weight gradient's side stream -- idle while the exact KL's factor runs, and kept for the process
    lifetime -- to the HIP library as its early stream (lvae_set_early_stream: the blocked inverse starts part of its
    triangular inverse there beside the factorisation's pivot-bound last passes).  No new stream: a step already uses
    the 4 hardware queues a process has here."""
    import ctypes

    from . import _lib
    dev = torch.device(dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().lvae_set_early_stream(ctypes.c_void_p(_side_stream(dev).cuda_stream)), "set_early_stream")


class _ReluMaxPool2(torch.autograd.Function):
    """max_pool2d(relu(x), 2, 2) in one HIP pass (lvae_relu_maxpool2_fwd/bwd_f32, vae_ops.hip):
    one byte of argmax per output instead of torch's int64 indices, one write per input in the
    backward.  Same values and gradient routing as relu + max_pool2d (first strict maximum; a NaN
    in the window is kept and takes the gradient, as in torch)."""

    @staticmethod
    def forward(ctx, x):
        from . import _lib
        lib = _lib.lib()
        x = x.contiguous()
        N, C, H, W = x.shape
        y = torch.empty(N, C, H // 2, W // 2, dtype=x.dtype, device=x.device)
        idx = torch.empty(N, C, H // 2, W // 2, dtype=torch.uint8, device=x.device)
        _lib.check(lib.lvae_relu_maxpool2_fwd_f32(_lib.ptr(x), N * C, H, W, _lib.ptr(y), _lib.ptr(idx),
                                                   _lib.stream_ptr()), "relu_maxpool2_fwd")
        ctx.save_for_backward(y, idx)
        ctx.shape = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        from . import _lib
        lib = _lib.lib()
        y, idx = ctx.saved_tensors
        N, C, H, W = ctx.shape
        gy = gy.contiguous()
        gx = torch.empty(N, C, H, W, dtype=gy.dtype, device=gy.device)
        _lib.check(lib.lvae_relu_maxpool2_bwd_f32(_lib.ptr(gy), _lib.ptr(y), _lib.ptr(idx), N * C, H, W, _lib.ptr(gx),
                                                   _lib.stream_ptr()), "relu_maxpool2_bwd")
        return gx


class _ConvReluMaxPool2(torch.autograd.Function):
    """max_pool2d(relu(conv2d(x, w, b, padding=1)), 2, 2) (VAE.py:44-50).
    Forward: a 1-channel input (the first conv) is one direct HIP pass (lvae_conv1_relu_maxpool2_fwd_f32);
    otherwise the conv runs without its bias on MIOpen and bias add, relu and pool are one HIP pass
    (lvae_relu_maxpool2_bias_fwd_f32).  Backward: weight and bias gradients straight from the pooled
    gradient (lvae_conv3x3_pool_wgrad_f32), and for 16 input channels the input gradient too
    (lvae_conv3x3_pool_dgrad_f32; the first conv needs none); otherwise the routed full-resolution
    gradient is formed for MIOpen's backward-data conv."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        from . import _lib
        lib = _lib.lib()
        b = bias.contiguous()
        if x.shape[1] == 1:  # first conv: one direct HIP pass, no full-resolution output
            xc, wc = x.contiguous(), weight.contiguous()
            N, C, H, W = x.shape[0], weight.shape[0], x.shape[2], x.shape[3]
            y = torch.empty(N, C, H // 2, W // 2, dtype=x.dtype, device=x.device)
            idx = torch.empty(N, C, H // 2, W // 2, dtype=torch.uint8, device=x.device)
            _lib.check(lib.lvae_conv1_relu_maxpool2_fwd_f32(_lib.ptr(xc), _lib.ptr(wc), _lib.ptr(b), N, C, H, W,
                                                             _lib.ptr(y), _lib.ptr(idx), _lib.stream_ptr()),
                       "conv1_relu_maxpool2_fwd")
        elif _CONV2_FUSED and x.shape[1] == 16 and x.shape[2] == x.shape[3] == 18 and weight.shape[0] % 16 == 0:
            # the second conv end to end: one direct HIP pass (no MIOpen conv, no layout transposes, no
            # full-resolution output)
            xc, wc = x.contiguous(), weight.contiguous()
            N, C, H, W = x.shape[0], weight.shape[0], x.shape[2], x.shape[3]
            y = torch.empty(N, C, H // 2, W // 2, dtype=x.dtype, device=x.device)
            idx = torch.empty(N, C, H // 2, W // 2, dtype=torch.uint8, device=x.device)
            _lib.check(lib.lvae_conv3x3_relu_maxpool2_fwd_f32(_lib.ptr(xc), _lib.ptr(wc), _lib.ptr(b), N, x.shape[1], C,
                                                               H, W, _lib.ptr(y), _lib.ptr(idx), _lib.stream_ptr()),
                       "conv3x3_relu_maxpool2_fwd")
        else:
            y0 = F.conv2d(x, weight, None, 1, 1).contiguous()
            N, C, H, W = y0.shape
            y = torch.empty(N, C, H // 2, W // 2, dtype=y0.dtype, device=y0.device)
            idx = torch.empty(N, C, H // 2, W // 2, dtype=torch.uint8, device=y0.device)
            _lib.check(lib.lvae_relu_maxpool2_bias_fwd_f32(_lib.ptr(y0), _lib.ptr(b), N, C, H, W, _lib.ptr(y),
                                                            _lib.ptr(idx), _lib.stream_ptr()), "relu_maxpool2_bias_fwd")
        ctx.save_for_backward(x, weight, y, idx)
        ctx.shape = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        from . import _lib
        lib = _lib.lib()
        x, weight, y, idx = ctx.saved_tensors
        N, C, H, W = ctx.shape
        gy = gy.contiguous()
        Cin = x.shape[1]
        if N >= 512 and C * Cin <= 1024 and 4 * (Cin * (((H + 2) * (W + 2)) | 1) + 2 * C * (H // 2) * (W // 2)) <= 65536:
            # (below a few hundred images the per-image kernel cannot fill the GPU: MIOpen path)
            # weight and bias gradients from the pooled gradient (lvae_conv3x3_pool_wgrad_f32); the first
            # conv (image input) needs no input gradient
            xc = x.contiguous()
            dgrad = (ctx.needs_input_grad[0] and _CONV_DGRAD and Cin == 16 and H * W <= 1024
                     and lib.lvae_conv3x3_pool_dgrad_lds(C, H, W) <= 65536)
            cur = torch.cuda.current_stream(gy.device)
            # (eager only: with this fork inside a HIP graph capture the process segfaults in torch.cuda.graph's
            # capture_end, i.e. in the runtime's hipStreamEndCapture / graph instantiation -- still after r6's
            # memset fix, so not the memset nodes (profiles/r6_fork_under_capture_segv.log); captured steps keep
            # the one-stream order)
            side = (_side_stream(gy.device)
                    if dgrad and _CONV_BWD_FORK and not torch.cuda.is_current_stream_capturing() else None)
            if side is not None:  # (the weight gradient beside the input gradient; joined below)
                side.wait_stream(cur)
            with torch.cuda.stream(side if side is not None else cur):
                dw = torch.empty_like(weight)
                db = torch.empty(C, dtype=gy.dtype, device=gy.device)
                ws = torch.empty(lib.lvae_conv3x3_pool_wgrad_workspace_size(N, C, Cin) // 4 + 1, dtype=torch.float32,
                                 device=gy.device)
                _lib.check(lib.lvae_conv3x3_pool_wgrad_f32(_lib.ptr(gy), _lib.ptr(y), _lib.ptr(idx), _lib.ptr(xc), N, C,
                                                            Cin, H, W, _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws),
                                                            _lib.stream_ptr()), "conv3x3_pool_wgrad")
            gx = None
            if dgrad:
                # the input gradient straight from the pooled gradient too (lvae_conv3x3_pool_dgrad_f32: the
                # routed gradient formed per image in LDS; no MIOpen backward-data conv, no transposes)
                gx = torch.empty(N, Cin, H, W, dtype=gy.dtype, device=gy.device)
                _lib.check(lib.lvae_conv3x3_pool_dgrad_f32(_lib.ptr(gy), _lib.ptr(y), _lib.ptr(idx),
                                                            _lib.ptr(weight.contiguous()), N, C, Cin, H, W,
                                                            _lib.ptr(gx), _lib.stream_ptr()), "conv3x3_pool_dgrad")
                if side is not None:
                    cur.wait_stream(side)
                    dw.record_stream(cur)
                    db.record_stream(cur)
            elif ctx.needs_input_grad[0]:
                g0 = torch.empty(N, C, H, W, dtype=gy.dtype, device=gy.device)
                _lib.check(lib.lvae_relu_maxpool2_bwd_f32(_lib.ptr(gy), _lib.ptr(y), _lib.ptr(idx), N * C, H, W,
                                                           _lib.ptr(g0), _lib.stream_ptr()), "relu_maxpool2_bwd")
                gx = torch.ops.aten.convolution_backward(g0, x, weight, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                         [True, False, False])[0]
            return gx, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None
        g0 = torch.empty(N, C, H, W, dtype=gy.dtype, device=gy.device)
        db = torch.empty(C, dtype=gy.dtype, device=gy.device)
        ws = torch.empty(lib.lvae_relu_maxpool2_bias_workspace_size(N, C) // 4 + 1, dtype=torch.float32,
                         device=gy.device)
        _lib.check(lib.lvae_relu_maxpool2_bias_bwd_f32(_lib.ptr(gy), _lib.ptr(y), _lib.ptr(idx), N, C, H, W,
                                                        _lib.ptr(g0), _lib.ptr(db), _lib.ptr(ws), _lib.stream_ptr()),
                   "relu_maxpool2_bias_bwd")
        gx = gw = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gx, gw, _ = torch.ops.aten.convolution_backward(
                g0, x, weight, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                [ctx.needs_input_grad[0], ctx.needs_input_grad[1], False])
        return gx, gw, db if ctx.needs_input_grad[2] else None


def conv_relu_maxpool2(conv, x):
    """pool(relu(conv(x))) for the encoder's 3x3 / padding-1 convs: fused bias path for CUDA fp32."""
    if (x.is_cuda and x.dtype == torch.float32 and conv.bias is not None and conv.weight.dtype == torch.float32
            and tuple(conv.kernel_size) == (3, 3) and tuple(conv.padding) == (1, 1) and tuple(conv.stride) == (1, 1)
            and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and x.shape[-1] % 2 == 0 and x.shape[-2] % 2 == 0):
        return _ConvReluMaxPool2.apply(x, conv.weight, conv.bias)
    return relu_maxpool2(conv(x))


class _Deconv2Sigmoid(torch.autograd.Function):
    """sigmoid(ConvTranspose2d(Cin, 1, 4, stride 2, padding 1)(z)) (VAE.py:75, 124) as one direct HIP pass
    each way (lvae_deconv2_sigmoid_fwd/bwd_f32): the backward forms the pre-sigmoid gradient on the fly
    and returns the input, weight and bias gradients together (no MIOpen transposed conv, no
    sigmoid / bias-sum kernels)."""

    @staticmethod
    def forward(ctx, z, weight, bias):
        from . import _lib
        lib = _lib.lib()
        zc, wc, bc = z.contiguous(), weight.contiguous(), bias.contiguous()
        N, Cin, Hi, Wi = zc.shape
        out = torch.empty(N, 1, 2 * Hi, 2 * Wi, dtype=z.dtype, device=z.device)
        _lib.check(lib.lvae_deconv2_sigmoid_fwd_f32(_lib.ptr(zc), _lib.ptr(wc), _lib.ptr(bc), N, Cin, Hi, Wi,
                                                     _lib.ptr(out), _lib.stream_ptr()), "deconv2_sigmoid_fwd")
        ctx.save_for_backward(zc, wc, out)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import _lib
        lib = _lib.lib()
        z, w, out = ctx.saved_tensors
        N, Cin, Hi, Wi = z.shape
        g = g.contiguous()
        gz = torch.empty_like(z)
        dw = torch.empty_like(w)
        db = torch.empty(1, dtype=z.dtype, device=z.device)
        ws = torch.empty(lib.lvae_deconv2_sigmoid_workspace_size(N, Cin, Hi, Wi) // 4 + 1, dtype=torch.float32,
                         device=z.device)
        _lib.check(lib.lvae_deconv2_sigmoid_bwd_f32(_lib.ptr(g), _lib.ptr(out), _lib.ptr(z), _lib.ptr(w), N, Cin, Hi,
                                                     Wi, _lib.ptr(gz), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws),
                                                     _lib.stream_ptr()), "deconv2_sigmoid_bwd")
        return gz, dw, db


def _deconv2_lds_ok(cin, hi, wi):
    """The LDS bounds lvae_deconv2_sigmoid_fwd / _bwd_f32 enforce (64 KB each; rc -3 beyond):
    forward Cin ((Hi+2)(Wi+2) | 1) floats, backward (2Hi+2)(2Wi+2) + Cin Hi Wi floats."""
    return (4 * cin * (((hi + 2) * (wi + 2)) | 1) <= 65536
            and 4 * ((2 * hi + 2) * (2 * wi + 2) + cin * hi * wi) <= 65536)


def deconv_sigmoid(deconv, z):
    """sigmoid(deconv(z)) for the decoder's last layer: fused HIP path for CUDA fp32 (torch's
    transposed conv + sigmoid when the geometry or the kernel's LDS bound rules it out)."""
    if (z.is_cuda and z.dtype == torch.float32 and deconv.weight.dtype == torch.float32 and deconv.bias is not None
            and z.dim() == 4 and _deconv2_lds_ok(z.shape[1], z.shape[2], z.shape[3])
            and deconv.out_channels == 1 and deconv.in_channels <= 16 and tuple(deconv.kernel_size) == (4, 4)
            and tuple(deconv.stride) == (2, 2) and tuple(deconv.padding) == (1, 1)
            and tuple(deconv.output_padding) == (0, 0) and tuple(deconv.dilation) == (1, 1) and deconv.groups == 1):
        return _Deconv2Sigmoid.apply(z, deconv.weight, deconv.bias)
    return torch.sigmoid(deconv(z))


def _act_bwd(gy, y, relu, N, C, HW):
    """(g, db): g = gy [y > 0] (gy itself without relu) and the bias gradient, one HIP pass
    (lvae_act_bwd_f32, glue.hip)."""
    from . import _lib
    lib = _lib.lib()
    g = torch.empty_like(gy) if relu else gy
    db = torch.empty(C, dtype=gy.dtype, device=gy.device)
    ws = torch.empty(lib.lvae_act_bwd_workspace_size(N, C) // 4 + 1, dtype=torch.float32, device=gy.device)
    _lib.check(lib.lvae_act_bwd_f32(_lib.ptr(gy), _lib.ptr(y) if relu else None, N, C, HW, 1 if relu else 0,
                                    _lib.ptr(g) if relu else None, _lib.ptr(db), _lib.ptr(ws), _lib.stream_ptr()),
               "act_bwd")
    return g, db


class _LinearAct(torch.autograd.Function):
    """relu(x W^T + b) or x W^T + b: the ConvVAE's fc layers (VAE.py:44-75).  The GEMMs stay on hipBLASLt
    (torch.mm / addmm); bias + ReLU is one HIP pass forward (lvae_bias_relu_fwd_f32) and the backward's
    pre-activation gradient and bias gradient one more (lvae_act_bwd_f32), in place of PyTorch's relu,
    threshold_backward and the strided bias reduction."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        from . import _lib
        x2 = x.contiguous()
        B, F_ = x2.shape[0], weight.shape[0]
        if relu:
            y = torch.mm(x2, weight.t())
            _lib.check(_lib.lib().lvae_bias_relu_fwd_f32(_lib.ptr(y), _lib.ptr(bias.contiguous()), B, F_, 1,
                                                          _lib.stream_ptr()), "bias_relu_fwd")
        else:
            y = torch.addmm(bias, x2, weight.t())
        ctx.relu = relu
        ctx.save_for_backward(x2, weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        gy = gy.contiguous()
        g, db = _act_bwd(gy, y, ctx.relu, gy.shape[0], gy.shape[1], 1)
        dx = torch.mm(g, w) if ctx.needs_input_grad[0] else None
        dw = torch.mm(g.t(), x)
        return dx, dw, db, None


def _deconv4s2_fused(x, weight, stride, padding, output_padding, dilation, groups):
    """The shapes lvae_deconv4s2_relu_fwd / _bwd_f32 take: the ConvVAE's deconv1 (32 -> 16, 4 x 4, stride 2,
    padding 1) on 9 x 9 inputs."""
    return (_CONV2_FUSED and x.dim() == 4 and tuple(x.shape[1:]) == (32, 9, 9) and tuple(weight.shape) == (32, 16, 4, 4)
            and tuple(stride) == (2, 2) and tuple(padding) == (1, 1) and tuple(output_padding) == (0, 0)
            and tuple(dilation) == (1, 1) and groups == 1)


class _DeconvRelu(torch.autograd.Function):
    """relu(ConvTranspose2d(x)) (VAE.py:73, 122).  The ConvVAE's shape (32 -> 16, 4 x 4, stride 2, padding 1, 9 x 9
    inputs): one direct HIP pass each way (lvae_deconv4s2_relu_fwd / _bwd_f32: the backward returns the input,
    weight and bias gradients together from the masked output gradient).  Other shapes: the transposed conv
    without its bias on MIOpen, then bias + ReLU in place as one HIP pass; backward: the pre-activation and bias
    gradients in one HIP pass, the input / weight gradients from MIOpen's convolution backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, output_padding, dilation, groups):
        from . import _lib
        ctx.fused = _deconv4s2_fused(x, weight, stride, padding, output_padding, dilation, groups)
        if ctx.fused:
            xc, wc = x.contiguous(), weight.contiguous()
            N = x.shape[0]
            y = torch.empty(N, 16, 18, 18, dtype=x.dtype, device=x.device)
            _lib.check(_lib.lib().lvae_deconv4s2_relu_fwd_f32(_lib.ptr(xc), _lib.ptr(wc), _lib.ptr(bias.contiguous()), N,
                                                               32, 16, 9, 9, _lib.ptr(y), _lib.stream_ptr()),
                       "deconv4s2_relu_fwd")
            ctx.save_for_backward(xc, wc, y)
            return y
        y = F.conv_transpose2d(x, weight, None, stride, padding, output_padding, groups, dilation).contiguous()
        N, C = y.shape[0], y.shape[1]
        _lib.check(_lib.lib().lvae_bias_relu_fwd_f32(_lib.ptr(y), _lib.ptr(bias.contiguous()), N, C,
                                                      y.shape[2] * y.shape[3], _lib.stream_ptr()), "bias_relu_fwd")
        ctx.conf = (stride, padding, output_padding, dilation, groups)
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        gy = gy.contiguous()
        if ctx.fused:
            from . import _lib
            lib = _lib.lib()
            N = x.shape[0]
            dx = torch.empty_like(x)
            dw = torch.empty_like(w)
            db = torch.empty(16, dtype=x.dtype, device=x.device)
            ws = torch.empty(lib.lvae_deconv4s2_relu_bwd_workspace_size(N, 32, 16) // 4 + 1, dtype=torch.float32,
                             device=x.device)
            _lib.check(lib.lvae_deconv4s2_relu_bwd_f32(_lib.ptr(gy), _lib.ptr(y), _lib.ptr(x), _lib.ptr(w), N, 32, 16,
                                                        9, 9, _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws),
                                                        _lib.stream_ptr()), "deconv4s2_relu_bwd")
            return dx if ctx.needs_input_grad[0] else None, dw, db, None, None, None, None, None
        stride, padding, output_padding, dilation, groups = ctx.conf
        g, db = _act_bwd(gy, y, True, y.shape[0], y.shape[1], y.shape[2] * y.shape[3])
        dx, dw, _ = torch.ops.aten.convolution_backward(g, x, w, None, list(stride), list(padding), list(dilation),
                                                        True, list(output_padding), groups,
                                                        [ctx.needs_input_grad[0], True, False])
        return dx, dw, db, None, None, None, None, None


def _f32_cuda(*ts):
    return all(t.is_cuda and t.dtype == torch.float32 for t in ts)


def linear_act(fc, x, relu):
    """relu(fc(x)) / fc(x) for the fc layers: the fused bias / ReLU HIP passes for CUDA fp32 2-D inputs."""
    if fc.bias is not None and x.dim() == 2 and _f32_cuda(x, fc.weight, fc.bias):
        return _LinearAct.apply(x, fc.weight, fc.bias, relu)
    y = fc(x)
    return F.relu(y) if relu else y


def deconv_relu(deconv, x):
    """relu(deconv(x)) for the decoder's first transposed conv: bias + ReLU fused for CUDA fp32."""
    if deconv.bias is not None and x.dim() == 4 and _f32_cuda(x, deconv.weight, deconv.bias):
        return _DeconvRelu.apply(x, deconv.weight, deconv.bias, tuple(deconv.stride), tuple(deconv.padding),
                                 tuple(deconv.output_padding), tuple(deconv.dilation), deconv.groups)
    return F.relu(deconv(x))


def relu_maxpool2(x):
    """pool(relu(x)) of the encoder (VAE.py:44-50): fused HIP kernel for CUDA fp32 activations."""
    if x.is_cuda and x.dtype == torch.float32 and x.shape[-1] % 2 == 0 and x.shape[-2] % 2 == 0:
        return _ReluMaxPool2.apply(x)
    return F.max_pool2d(F.relu(x), kernel_size=2, stride=2)


class ConvVAE(nn.Module):
    def __init__(self, latent_dim, num_dim=1296, vy_init=1.0, vy_fixed=False, p_input=0.2, p=0.5):
        super().__init__()
        self.latent_dim = latent_dim
        self.num_dim = num_dim
        self.p_input = p_input
        self.p = p
        log_vy_init = math.log(vy_init - math.exp(-8.0))
        self._log_vy = nn.Parameter(torch.full((num_dim,), log_vy_init))
        if vy_fixed:
            self._log_vy.requires_grad_(False)
        # encoder (VAE.py:44-60)
        self.conv1 = nn.Conv2d(1, 16, kernel_size=3, stride=1, padding=1)
        self.pool1 = nn.MaxPool2d(kernel_size=2, stride=2, padding=0)
        self.dropout2d_1 = nn.Dropout2d(p=p)
        self.conv2 = nn.Conv2d(16, 32, kernel_size=3, stride=1, padding=1)
        self.pool2 = nn.MaxPool2d(kernel_size=2, stride=2, padding=0)
        self.dropout2d_2 = nn.Dropout2d(p=p)
        self.fc1 = nn.Linear(32 * 9 * 9, 300)
        self.dropout1 = nn.Dropout(p=p)
        self.fc21 = nn.Linear(300, 30)
        self.dropout2 = nn.Dropout(p=p)
        self.fc211 = nn.Linear(30, latent_dim)
        self.fc221 = nn.Linear(30, latent_dim)
        # decoder (VAE.py:62-75)
        self.fc3 = nn.Linear(latent_dim, 30)
        self.dropout3 = nn.Dropout(p=p)
        self.fc31 = nn.Linear(30, 300)
        self.dropout4 = nn.Dropout(p=p)
        self.fc4 = nn.Linear(300, 32 * 9 * 9)
        self.dropout2d_3 = nn.Dropout2d(p=p)
        self.deconv1 = nn.ConvTranspose2d(32, 16, kernel_size=4, stride=2, padding=1)
        self.dropout2d_4 = nn.Dropout2d(p=p)
        self.deconv2 = nn.ConvTranspose2d(16, 1, kernel_size=4, stride=2, padding=1)
        self.register_buffer("min_log_vy", torch.full((1,), -8.0))

    @property
    def vy(self):
        return torch.exp(self.min_log_vy + F.softplus(self._log_vy - self.min_log_vy))

    def encode(self, x):
        z = self.dropout2d_1(conv_relu_maxpool2(self.conv1, x))   # pool1(relu(conv1))
        z = self.dropout2d_2(conv_relu_maxpool2(self.conv2, z))   # pool2(relu(conv2))
        h1 = self.dropout1(linear_act(self.fc1, z.reshape(-1, 32 * 9 * 9), True))
        h2 = self.dropout2(linear_act(self.fc21, h1, True))
        return linear_act(self.fc211, h2, False), linear_act(self.fc221, h2, False)

    def decode(self, z):
        x = self.dropout3(linear_act(self.fc3, z, True))
        x = self.dropout4(linear_act(self.fc31, x, True))
        x = linear_act(self.fc4, x, True)
        x = self.dropout2d_3(x.reshape(-1, 32, 9, 9))
        x = self.dropout2d_4(deconv_relu(self.deconv1, x))
        return deconv_sigmoid(self.deconv2, x)

    def sample_latent(self, mu, log_var, eps=None):
        if eps is None:
            eps = torch.randn_like(log_var)
        if _glue_ok(mu, log_var, eps) and mu.shape == log_var.shape == eps.shape:
            return _ReparamFn.apply(mu, log_var, eps)  # (glue.hip: one launch each way)
        return mu + eps * torch.exp(0.5 * log_var)

    def forward(self, x, eps=None):
        mu, log_var = self.encode(x)
        return self.decode(self.sample_latent(mu, log_var, eps)), mu, log_var

    def loss_function(self, recon_x, x, mask):
        """(per-image masked MSE, per-image NLL) -- VAE.py:144-162."""
        d = self.num_dim
        if _glue_ok(recon_x, x, mask, self._log_vy) and self._log_vy.numel() == d:
            return _VaeLossFn.apply(recon_x, x, mask, self._log_vy)  # (glue.hip: one launch each way)
        se = (recon_x.reshape(-1, d) - x.reshape(-1, d)) ** 2 * mask.reshape(-1, d)
        msum = mask.reshape(-1, d).sum(1)
        msum = torch.where(msum == 0, torch.ones_like(msum), msum)
        mse = se.sum(1) / msum
        nll = se / (2 * torch.exp(self._log_vy)) + 0.5 * (math.log(2 * math.pi) + self._log_vy)
        return mse, nll.sum(1)


# Rows above which SimpleVAE takes the layered route although the fused kernels fit (None: no gate; the timings of
# scripts/simple_vae_timing.py, DESIGN.md "MLP VAE"): the default of a model's ``fused_max_rows``
_MLP_FUSED_MAX_ROWS = None


def _mlp_dims(x, w1, w21, w211):
    return x.shape[0], w1.shape[1], w1.shape[0], w21.shape[0], w211.shape[0]


class _MlpEncodeFn(torch.autograd.Function):
    """(mu, log_var) of SimpleVAE.encode (VAE.py:215-224) in one HIP launch (lvae_mlp_enc_fwd_f32, mlp_vae.hip): the
    four layers with their weights in LDS; backward: every weight and bias gradient in two launches
    (lvae_mlp_enc_bwd_f32).  x gets no gradient.  grad_on: torch.is_grad_enabled() at the call (a Function's forward
    cannot see it, and ctx.needs_input_grad does not: a Parameter needs grad under no_grad too); without it the
    activations are neither written (NULL h1 / h2) nor saved."""

    @staticmethod
    def forward(ctx, grad_on, x, w1, b1, w21, b21, w211, b211, w221, b221):
        from . import _lib
        lib = _lib.lib()
        ts = [t.contiguous() for t in (x, w1, b1, w21, b21, w211, b211, w221, b221)]
        x, w1, w21, w211, w221 = ts[0], ts[1], ts[3], ts[5], ts[7]
        B, D, H1, H2, L = _mlp_dims(x, w1, w21, w211)
        train = grad_on and any(ctx.needs_input_grad)
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=x.device)
        h1, h2 = (new(B, H1), new(B, H2)) if train else (None, None)
        mu, log_var = new(B, L), new(B, L)
        _lib.check(lib.lvae_mlp_enc_fwd_f32(*(_lib.ptr(t) for t in ts), B, D, H1, H2, L, _lib.ptr(h1), _lib.ptr(h2),
                                            _lib.ptr(mu), _lib.ptr(log_var), _lib.stream_ptr()), "mlp_enc_fwd")
        if train:
            ctx.save_for_backward(x, h1, h2, w1, w21, w211, w221)
        return mu, log_var

    @staticmethod
    def backward(ctx, g_mu, g_lv):
        from . import _lib
        lib = _lib.lib()
        x, h1, h2, w1, w21, w211, w221 = ctx.saved_tensors
        B, D, H1, H2, L = _mlp_dims(x, w1, w21, w211)
        g_mu, g_lv = g_mu.contiguous(), g_lv.contiguous()
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=x.device)
        dw1, db1, dw21, db21 = new(H1, D), new(H1), new(H2, H1), new(H2)
        dw211, db211, dw221, db221 = new(L, H2), new(L), new(L, H2), new(L)
        ws = torch.empty(lib.lvae_mlp_enc_bwd_workspace_size(B, D, L), dtype=torch.uint8, device=x.device)
        _lib.check(lib.lvae_mlp_enc_bwd_f32(*(_lib.ptr(t) for t in (g_mu, g_lv, x, h1, h2, w21, w211, w221)), B, D, H1,
                                            H2, L, *(_lib.ptr(t) for t in (dw1, db1, dw21, db21, dw211, db211, dw221,
                                                                           db221, ws)), _lib.stream_ptr()),
                   "mlp_enc_bwd")
        return None, None, dw1, db1, dw21, db21, dw211, db211, dw221, db221


def _mlp_dec_fwd(ctx, grad_on, z, mu, log_var, eps, params):
    """recon of SimpleVAE.decode from z, or from (mu, log_var, eps) with the reparametrisation inside the launch;
    grad_on as in _MlpEncodeFn (NULL h3 / h4 and nothing saved without it)"""
    from . import _lib
    lib = _lib.lib()
    w3, b3, w31, b31, w4, b4 = (t.contiguous() for t in params)
    sampled = z is None
    lat = [t.contiguous() for t in ((mu, log_var, eps) if sampled else (z,))]
    B, L, H2, H1, D = lat[0].shape[0], w3.shape[1], w3.shape[0], w31.shape[0], w4.shape[0]
    train = grad_on and any(ctx.needs_input_grad)
    ctx.wgrad = any(ctx.needs_input_grad[-6:])   # (a frozen decoder: the backward skips the weight-gradient launch)
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=w3.device)
    h3, h4 = (new(B, H2), new(B, H1)) if train else (None, None)
    z_out = new(B, L) if sampled else None
    recon = new(B, D)
    args = [None] + lat if sampled else lat + [None, None, None]
    _lib.check(lib.lvae_mlp_dec_fwd_f32(*(_lib.ptr(t) for t in args), *(_lib.ptr(t) for t in (w3, b3, w31, b31, w4, b4)),
                                        B, D, H1, H2, L, _lib.ptr(z_out), _lib.ptr(h3), _lib.ptr(h4), _lib.ptr(recon),
                                        _lib.stream_ptr()), "mlp_dec_fwd")
    if train:
        ctx.save_for_backward(recon, h4, h3, z_out if sampled else lat[0], lat[1] if sampled else None,
                              lat[2] if sampled else None, w3, w31, w4)
    return recon


def _mlp_dec_bwd(ctx, g_recon):
    """(g_z or (g_mu, g_log_var), the six weight and bias gradients) in two launches (lvae_mlp_dec_bwd_f32); one, and
    no weight gradients, when no decoder parameter needs one (LatentInferenceStep on a frozen model)"""
    from . import _lib
    lib = _lib.lib()
    recon, h4, h3, z, log_var, eps, w3, w31, w4 = ctx.saved_tensors
    sampled = eps is not None
    B, L, H2, H1, D = z.shape[0], w3.shape[1], w3.shape[0], w31.shape[0], w4.shape[0]
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=z.device)
    dws = (new(H2, L), new(H2), new(H1, H2), new(H1), new(D, H1), new(D)) if ctx.wgrad else (None,) * 6
    g_z = None if sampled else new(B, L)
    g_mu, g_lv = (new(B, L), new(B, L)) if sampled else (None, None)
    ws = torch.empty(lib.lvae_mlp_dec_bwd_workspace_size(B, D, L), dtype=torch.uint8, device=z.device)
    ins = (g_recon.contiguous(), recon, h4, h3, z, log_var, eps, w3, w31, w4)
    outs = dws + (g_z, g_mu, g_lv, ws)
    _lib.check(lib.lvae_mlp_dec_bwd_f32(*(_lib.ptr(t) for t in ins), B, D, H1, H2, L, *(_lib.ptr(t) for t in outs),
                                        _lib.stream_ptr()), "mlp_dec_bwd")
    return (None,) + ((g_mu, g_lv, None) if sampled else (g_z,)) + dws


class _MlpDecodeFn(torch.autograd.Function):
    """SimpleVAE.decode (VAE.py:226-235) in one HIP launch (lvae_mlp_dec_fwd_f32); backward: g_z and the weight and
    bias gradients in two (lvae_mlp_dec_bwd_f32)."""

    @staticmethod
    def forward(ctx, grad_on, z, w3, b3, w31, b31, w4, b4):
        return _mlp_dec_fwd(ctx, grad_on, z, None, None, None, (w3, b3, w31, b31, w4, b4))

    @staticmethod
    def backward(ctx, g_recon):
        return _mlp_dec_bwd(ctx, g_recon)


class _MlpSampleDecodeFn(torch.autograd.Function):
    """decode(mu + eps exp(log_var / 2)) (VAE.py:246-253) in one HIP launch: the reparametrisation inside the
    decoder's launch, and its adjoint inside the backward's."""

    @staticmethod
    def forward(ctx, grad_on, mu, log_var, eps, w3, b3, w31, b31, w4, b4):
        return _mlp_dec_fwd(ctx, grad_on, None, mu, log_var, eps, (w3, b3, w31, b31, w4, b4))

    @staticmethod
    def backward(ctx, g_recon):
        return _mlp_dec_bwd(ctx, g_recon)


class SimpleVAE(nn.Module):
    """The MLP encoder / decoder (VAE.py:165-273, the reference's type_nnet='simple'): the reference's parameter
    names and shapes, so its state dicts load with strict=True, and ConvVAE's method signatures here, so every step
    and driver takes either model.  ``x`` is [.., num_dim] (forward views it as (-1, num_dim)).

    Three routes, recorded in ``last_route`` ({'encode': .., 'decode': ..}):
      'fused'    CUDA fp32 with hidden == (300, 30), a shape lvae_mlp_vae_fused_ok accepts (num_dim <= 57) and, for
                 the encoder, an input that needs no gradient: each half is one HIP launch with its weights in LDS
                 (mlp_vae.hip), the backward two per half; in forward() the reparametrisation rides in the decoder's;
                 under torch.no_grad() the activations the backward would need are not written at all;
                 ``fused_max_rows`` (None: no gate) sends batches of more rows to the layered route;
      'layered'  CUDA fp32 otherwise (flat Health-MNIST's 1296 inputs, other hidden widths): linear_act per layer
                 (hipBLASLt GEMMs + the fused bias / ReLU passes) and torch.sigmoid;
      'stock'    CPU or fp64: plain torch ops (in fp64 on the CPU, the restatement the GPU tests compare against).
    All launches go to the caller's stream."""

    def __init__(self, latent_dim, num_dim, vy_init=1.0, vy_fixed=False, hidden=(300, 30)):
        super().__init__()
        self.latent_dim = latent_dim
        self.num_dim = num_dim
        self.hidden = (int(hidden[0]), int(hidden[1]))
        if isinstance(vy_init, (int, float)):
            self._log_vy = nn.Parameter(torch.full((num_dim,), math.log(vy_init - math.exp(-8.0))))
        else:
            self._log_vy = nn.Parameter(torch.log(torch.as_tensor(vy_init, dtype=torch.float32) - math.exp(-8.0)))
        if vy_fixed:
            self._log_vy.requires_grad_(False)
        h1, h2 = self.hidden
        # encoder (VAE.py:192-195)
        self.fc1 = nn.Linear(num_dim, h1)
        self.fc21 = nn.Linear(h1, h2)
        self.fc211 = nn.Linear(h2, latent_dim)
        self.fc221 = nn.Linear(h2, latent_dim)
        # decoder (VAE.py:198-200)
        self.fc3 = nn.Linear(latent_dim, h2)
        self.fc31 = nn.Linear(h2, h1)
        self.fc4 = nn.Linear(h1, num_dim)
        self.register_buffer("min_log_vy", torch.full((1,), -8.0))
        self.last_route = {}
        self.fused_max_rows = _MLP_FUSED_MAX_ROWS
        self._fused_shape = None

    @property
    def vy(self):
        return torch.exp(self.min_log_vy + F.softplus(self._log_vy - self.min_log_vy))

    @vy.setter
    def vy(self, vy):
        vy = torch.as_tensor(vy, dtype=self._log_vy.dtype, device=self._log_vy.device)
        assert torch.min(vy) >= 0.0005, "Smallest allowed value for vy is 0.0005"
        with torch.no_grad():
            self._log_vy.copy_(torch.log(vy - torch.exp(self.min_log_vy)))

    def _route(self, half, t, layers):
        route = "stock"
        if _f32_cuda(t, *(p for fc in layers for p in (fc.weight, fc.bias))) and t.dim() == 2:
            if self._fused_shape is None:
                from . import _lib
                self._fused_shape = bool(_lib.load().lvae_mlp_vae_fused_ok(self.num_dim, *self.hidden,
                                                                           self.latent_dim))
            gated = self.fused_max_rows is not None and t.shape[0] > self.fused_max_rows
            fused = self._fused_shape and not gated and t.shape[0] > 0 and not (half == "encode" and t.requires_grad)
            route = "fused" if fused else "layered"
        self.last_route[half] = route
        return route

    @staticmethod
    def _wb(layers):
        return [p for fc in layers for p in (fc.weight, fc.bias)]

    def encode(self, x):
        layers = (self.fc1, self.fc21, self.fc211, self.fc221)
        if x.dim() != 2:  # (a collated flat image [B, 1, 1, num_dim]: the rows, as forward() views them)
            x = x.reshape(-1, self.num_dim)
        route = self._route("encode", x, layers)
        if route == "fused":
            return _MlpEncodeFn.apply(torch.is_grad_enabled(), x, *self._wb(layers))
        if route == "layered":
            h2 = linear_act(self.fc21, linear_act(self.fc1, x, True), True)
            return linear_act(self.fc211, h2, False), linear_act(self.fc221, h2, False)
        h2 = F.relu(self.fc21(F.relu(self.fc1(x))))
        return self.fc211(h2), self.fc221(h2)

    def decode(self, z):
        layers = (self.fc3, self.fc31, self.fc4)
        route = self._route("decode", z, layers)
        if route == "fused":
            return _MlpDecodeFn.apply(torch.is_grad_enabled(), z, *self._wb(layers))
        if route == "layered":
            return torch.sigmoid(linear_act(self.fc4, linear_act(self.fc31, linear_act(self.fc3, z, True), True), False))
        return torch.sigmoid(self.fc4(F.relu(self.fc31(F.relu(self.fc3(z))))))

    def sample_latent(self, mu, log_var, eps=None):
        if eps is None:
            eps = torch.randn_like(log_var)
        if _glue_ok(mu, log_var, eps) and mu.shape == log_var.shape == eps.shape:
            return _ReparamFn.apply(mu, log_var, eps)  # (glue.hip: one launch each way)
        return mu + eps * torch.exp(0.5 * log_var)

    def forward(self, x, eps=None):
        mu, log_var = self.encode(x.reshape(-1, self.num_dim))
        layers = (self.fc3, self.fc31, self.fc4)
        if self._route("decode", mu, layers) == "fused":
            if eps is None:
                eps = torch.randn_like(log_var)
            if _glue_ok(eps) and eps.shape == mu.shape:
                recon = _MlpSampleDecodeFn.apply(torch.is_grad_enabled(), mu, log_var, eps, *self._wb(layers))
                return recon, mu, log_var
        return self.decode(self.sample_latent(mu, log_var, eps)), mu, log_var

    # (per-row masked MSE, per-row NLL) -- VAE.py:255-273, the formula of ConvVAE's (lvae_vae_loss_*, glue.hip)
    loss_function = ConvVAE.loss_function


class _VaeLossFn(torch.autograd.Function):
    """(mse [B], nll [B]) of ConvVAE.loss_function in one HIP launch (glue.hip); backward: d recon and
    d log_vy in one launch + the column sum of the d log_vy partials."""

    @staticmethod
    def forward(ctx, recon, x, mask, log_vy):
        from . import _lib
        lib = _lib.lib()
        d = log_vy.numel()
        r, xx, mm = (t.reshape(-1, d).contiguous() for t in (recon, x, mask))
        lv = log_vy.contiguous()
        B = r.shape[0]
        mse, nll, msum = (torch.empty(B, dtype=torch.float32, device=r.device) for _ in range(3))
        _lib.check(lib.lvae_vae_loss_fwd_f32(_lib.ptr(r), _lib.ptr(xx), _lib.ptr(mm), _lib.ptr(lv), B, d, _lib.ptr(mse),
                                             _lib.ptr(nll), _lib.ptr(msum), _lib.stream_ptr()), "vae_loss_fwd")
        ctx.save_for_backward(r, xx, mm, lv, msum)
        ctx.rshape = recon.shape
        ctx.need_lv = log_vy.requires_grad
        return mse, nll

    @staticmethod
    def backward(ctx, g_mse, g_nll):
        from . import _lib
        lib = _lib.lib()
        r, xx, mm, lv, msum = ctx.saved_tensors
        B, d = r.shape
        g_mse, g_nll = (g.to(torch.float32).reshape(B) for g in (g_mse, g_nll))  # (stride 0 kept: broadcasts)
        dr = torch.empty_like(r)
        part = torch.empty(int(lib.lvae_vae_loss_bwd_partials(B)), d, dtype=torch.float32, device=r.device)
        _lib.check(lib.lvae_vae_loss_bwd_f32(_lib.ptr(r), _lib.ptr(xx), _lib.ptr(mm), _lib.ptr(lv), _lib.ptr(msum),
                                             _lib.ptr(g_mse), g_mse.stride(0), _lib.ptr(g_nll), g_nll.stride(0), B, d,
                                             _lib.ptr(dr), _lib.ptr(part), _lib.stream_ptr()), "vae_loss_bwd")
        dlv = part.sum(0) if ctx.need_lv else None
        return dr.reshape(ctx.rshape), None, None, dlv


class _ReparamFn(torch.autograd.Function):
    """z = mu + eps exp(log_var / 2) in one HIP launch (glue.hip); backward: d log_var in one launch."""

    @staticmethod
    def forward(ctx, mu, log_var, eps):
        from . import _lib
        lib = _lib.lib()
        mu_, lv_, e_ = (t.contiguous() for t in (mu, log_var, eps))
        z = torch.empty_like(mu_)
        _lib.check(lib.lvae_reparam_fwd_f32(_lib.ptr(mu_), _lib.ptr(lv_), _lib.ptr(e_), mu_.numel(), _lib.ptr(z),
                                            _lib.stream_ptr()), "reparam_fwd")
        ctx.save_for_backward(lv_, e_)
        return z

    @staticmethod
    def backward(ctx, gz):
        from . import _lib
        lib = _lib.lib()
        lv_, e_ = ctx.saved_tensors
        gz = gz.contiguous()
        glv = torch.empty_like(lv_)
        _lib.check(lib.lvae_reparam_bwd_f32(_lib.ptr(gz), _lib.ptr(lv_), _lib.ptr(e_), lv_.numel(), _lib.ptr(glv),
                                            _lib.stream_ptr()), "reparam_bwd")
        return gz, glv, None


def _glue_ok(*ts):
    return all(t.is_cuda and t.dtype == torch.float32 for t in ts)
