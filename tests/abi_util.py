"""Helpers of the C-ABI edge tests (test_gpu_gram_abi.py, test_gpu_small_abi.py, the solve / factor
edge tests of test_gpu_linalg.py): sentinel-filled device buffers with strided logical views, and the
checks that a call wrote its logical extent only.

Sentinel rule: a buffer passed with padding (ld > columns, padded batch strides) is allocated whole,
filled with NaN (floats) or 0x7f bytes (integers); after the call every element outside the logical
extent must still hold that bit pattern.
"""
import numpy as np
import torch

DEV = "cuda"
_BITS = {8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}


def sentinel(numel, dtype=torch.float64, device=DEV):
    """A flat buffer of `numel` sentinels: NaN for floating dtypes, 0x7f bytes for integer ones."""
    if dtype.is_floating_point:
        return torch.full((int(numel),), float("nan"), dtype=dtype, device=device)
    t = torch.empty(int(numel), dtype=dtype, device=device)
    t.view(torch.uint8).fill_(0x7F)
    return t


def bits(t):
    return t.view(_BITS[t.element_size()])


def extent(shape, strides, offset=0):
    """Elements a buffer needs to hold the strided view."""
    return offset + sum((int(s) - 1) * int(st) for s, st in zip(shape, strides)) + 1


def view(buf, shape, strides, offset=0):
    return torch.as_strided(buf, tuple(shape), tuple(strides), offset)


def padded(values, strides, offset=0, tail=5):
    """A sentinel buffer holding `values` (a CPU or device tensor) at the given strides; returns
    (buffer, logical view).  `tail` extra sentinels follow the last logical element."""
    buf = sentinel(extent(values.shape, strides, offset) + tail, values.dtype)
    v = view(buf, values.shape, strides, offset)
    v.copy_(values.to(buf.device))
    return buf, v


def untouched_outside(buf, shape, strides, offset=0):
    """True when every element of buf outside the strided logical extent is still the sentinel, bit for bit."""
    mask = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    view(mask, shape, strides, offset).fill_(True)
    want = bits(sentinel(1, buf.dtype, buf.device))
    return bool((bits(buf)[~mask] == want).all())


def all_sentinel(buf):
    return bool((bits(buf) == bits(sentinel(1, buf.dtype, buf.device))).all())


def rel(a, b):
    """max |a - b| / max |b| in fp64 on the CPU"""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def spd(L, n, seed, cond=1e3):
    """[L, n, n] SPD fp64 with eigenvalues logspace(1, cond) in a random orthogonal basis (test_gpu_linalg.spd)"""
    g = torch.Generator().manual_seed(seed)
    Q, _ = torch.linalg.qr(torch.randn(L, n, n, generator=g, dtype=torch.float64))
    ev = torch.logspace(0, np.log10(cond), n, dtype=torch.float64)
    A = (Q * ev) @ Q.transpose(-1, -2)
    return 0.5 * (A + A.transpose(-1, -2))


def nan_upper(A):
    """A copy of the [.., n, n] matrices with the strict upper triangle NaN (never read by the kernels)"""
    n = A.shape[-1]
    up = torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
    return torch.where(up, torch.full_like(A, float("nan")), A)


def workspace(nbytes, tail=256):
    """A 256-B aligned uint8 device buffer of exactly nbytes + a sentinel tail; returns (buffer, tail view)."""
    buf = torch.empty(int(nbytes) + tail, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    buf.fill_(0x7F)
    return buf, buf[int(nbytes):]


def tail_untouched(tail):
    return bool((tail == 0x7F).all())
