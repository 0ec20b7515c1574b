"""trtri's early part beside potrf's pivot-bound tail (chol_inv.hip, schedule (a), recursive doubling): the split
launch order against fp64 torch, bitwise against the unsplit order (LVAE_CI_TRTRI_EARLY=0, read once per process: a
fresh child each), with two calls in flight on the shared early stream, and under a graph capture.

The early stream is one the caller lends (lvae_set_early_stream; the library creates none: a fifth stream in a step
that already uses the process's 4 hardware queues serialises it).  Every process here lends one before its first call.

All shapes have L >= 3 latent dims per call: off the pipelined schedule (kCiPipeMaxL = 2), which has no
recursive doubling to split.  s = the largest power of two below nt = n / 256 is the split point."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_regime_b import _spd_inverse, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (n, L): nt = 2 (s = 1: the early part is one diagonal copy and one X tile), 3 (s = 2, a ragged C group), 4,
# 5 (s = 4, a one-block C group), 8, and the fuse bound L = 16
SHAPES = [(512, 3), (768, 3), (1024, 3), (1280, 5), (2048, 3), (1024, 16)]
BITWISE = [(1280, 5), (2048, 3)]


@functools.lru_cache(maxsize=None)
def spd_case(n, L, seed=None):
    """test_spd_inverse's construction: A [L, n, n] fp64 SPD with an uneven diagonal scale (0.5 .. 50), and its fp32
    lower triangle under a garbage upper triangle (never read) on the host.  Shared, left unchanged."""
    gen = torch.Generator().manual_seed(n + L if seed is None else seed)
    Xm = torch.randn(L, n, n, generator=gen, dtype=torch.float64) / n ** 0.5
    A = Xm @ Xm.transpose(1, 2) + torch.eye(n, dtype=torch.float64)
    s = torch.exp(torch.rand(L, n, 1, generator=gen, dtype=torch.float64) * 4.6 - 0.7) ** 0.5
    A = s * A * s.transpose(1, 2)
    Ad = (torch.tril(A) + 7.0 * torch.triu(torch.ones(n, n, dtype=torch.float64), 1)).float().contiguous()
    return A, Ad


_LENT = []


def lend():
    """Lend the library one stream of this process (kept for its lifetime) as the early stream, once."""
    from lvae_amd import _lib
    if not _LENT:
        _LENT.append(torch.cuda.Stream())
        _lib.check(_lib.lib().lvae_set_early_stream(ctypes.c_void_p(_LENT[0].cuda_stream)), "set_early_stream")
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def alone(n, L, seed=None):
    """The stand-alone result of a case (its own call, synchronised): Ainv, logdet, info on the device."""
    return _spd_inverse(lend(), "chol", n, L, spd_case(n, L, seed)[1].to(DEV))


@pytest.mark.parametrize("n,L", SHAPES)
def test_split_trtri_vs_fp64(hip, n, L):
    """The bounds of test_spd_inverse: inverse rel < 1e-4, log-det < 1e-6, info == 0."""
    A = spd_case(n, L)[0]
    Ai, logdet, info = alone(n, L)
    assert int(info.abs().sum()) == 0
    got = Ai.cpu().double()
    assert torch.isfinite(got).all()
    err = rel(got, torch.linalg.inv(A))
    lerr = rel(logdet.cpu(), torch.logdet(A))
    print(f"n={n} L={L}: inverse rel err {err:.3e}, log-det rel err {lerr:.3e}")
    assert err < 1e-4
    assert lerr < 1e-6


def run_child(out):
    """What a child runs: the BITWISE cases' outputs as .npy files under `out`."""
    for n, L in BITWISE:
        Ai, logdet, info = alone(n, L)
        np.save(os.path.join(out, f"ainv_{n}_{L}.npy"), Ai.cpu().numpy())
        np.save(os.path.join(out, f"logdet_{n}_{L}.npy"), logdet.cpu().numpy())
        np.save(os.path.join(out, f"info_{n}_{L}.npy"), info.cpu().numpy())
    print("child outputs written")


def test_launch_orders_bitwise_equal(hip, tmp_path):
    """Every output tile comes from one workgroup, the same operands and the same K order in both launch orders:
    Ainv, logdet and info are bitwise equal with LVAE_CI_TRTRI_EARLY=0 and with it unset.  Two children, one after the
    other, each with its own timeout; a child that fails, ends on a signal or runs out of time fails the test at
    once: the next one is not started."""
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here] + [p for p in sys.path if p]
    outs = {}
    for name, env_set in (("unsplit", {"LVAE_CI_TRTRI_EARLY": "0"}), ("split", {})):
        env = dict(os.environ, PYTHONPATH=os.pathsep.join(paths))
        env.pop("LVAE_CI_TRTRI_EARLY", None)
        env.update(env_set)
        outs[name] = tmp_path / name
        outs[name].mkdir()
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
            "-c", f"import test_gpu_trtri_early as T; T.run_child({str(outs[name])!r})"]
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=180)
        except subprocess.TimeoutExpired:
            pytest.fail(f"child {name} hit its timeout")
        assert r.returncode >= 0, f"child {name} ended on signal {-r.returncode}\n{r.stderr[-2000:]}"
        assert r.returncode == 0 and "child outputs written" in r.stdout, f"{name}\n{r.stdout}\n{r.stderr[-4000:]}"
    for n, L in BITWISE:
        for what in ("ainv", "logdet", "info"):
            a = np.load(outs["unsplit"] / f"{what}_{n}_{L}.npy")
            b = np.load(outs["split"] / f"{what}_{n}_{L}.npy")
            assert np.isfinite(a).all(), (what, n, L)
            assert np.array_equal(a, b), (what, n, L)
        # (and this process, which runs the default order, agrees with both)
        assert np.array_equal(alone(n, L)[0].cpu().numpy(), np.load(outs["split"] / f"ainv_{n}_{L}.npy"))


class Call:
    """The buffers of one lvae_spd_inv_chol_f32 call, allocated up front; enqueue() launches it on the current stream
    and does not synchronise."""

    def __init__(self, hip, n, L):
        self.hip, self.n, self.L = hip, n, L
        self.A = torch.empty(L, n, n, device=DEV)
        self.scr = torch.full((hip.lvae_spd_inv_chol_scratch_size(n, L) // 4,), float("nan"), device=DEV)
        self.Ai = torch.full((L, n, n), float("nan"), device=DEV)
        self.logdet = torch.zeros(L, dtype=torch.float64, device=DEV)
        self.info = torch.zeros(L, dtype=torch.int32, device=DEV)

    def enqueue(self):
        import lvae_amd as la
        P = la._lib
        P.check(self.hip.lvae_spd_inv_chol_f32(self.n, self.L, P.ptr(self.A), P.ptr(self.scr), P.ptr(self.Ai),
                                               P.ptr(self.logdet), P.ptr(self.info), P.stream_ptr()), "chol")

    def equals(self, ref):
        return (torch.equal(self.Ai, ref[0]) and torch.equal(self.logdet, ref[1]) and torch.equal(self.info, ref[2])
                and bool(torch.isfinite(self.Ai).all()))


@pytest.mark.parametrize("streams", [1, 2])
def test_two_calls_in_flight(hip, streams):
    """Two inverses enqueued back to back with no synchronisation between them, different inputs, scratch and outputs,
    on one caller stream and on two: the shared early stream and its reused events keep each equal, bitwise, to its
    stand-alone result."""
    lend()
    cases = [(1280, 5, None), (1024, 3, 77)]
    refs = [alone(*c) for c in cases]
    calls = [Call(hip, n, L) for n, L, _ in cases]
    for c, case in zip(calls, cases):
        c.A.copy_(spd_case(*case)[1])
    torch.cuda.synchronize()
    qs = [torch.cuda.Stream() for _ in range(streams)]
    for k, c in enumerate(calls):
        with torch.cuda.stream(qs[k % streams]):
            c.enqueue()
    torch.cuda.synchronize()
    for c, ref, case in zip(calls, refs, cases):
        assert c.equals(ref), case


def test_split_trtri_under_capture(hip):
    """One call at (1024, 3) captured with torch.cuda.graph after an eager warm-up call (the side stream and its
    events exist by then), replayed twice on fresh inputs copied into the static buffers: each replay equals the eager
    result (the split order) bitwise.  The captured call leaves the lent stream alone -- it is the caller's, and is not
    pulled into the caller's capture -- and keeps the unsplit order."""
    n, L = 1024, 3
    seeds = [None, 91]
    refs = [alone(n, L, s) for s in seeds]  # (eager calls: the warm-up too)
    c = Call(hip, n, L)
    c.A.copy_(spd_case(n, L, 5)[1])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.enqueue()
    for s, ref in zip(seeds, refs):
        c.A.copy_(spd_case(n, L, s)[1])
        c.Ai.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert c.equals(ref), s
