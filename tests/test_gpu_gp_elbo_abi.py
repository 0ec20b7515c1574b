"""lvae_gp_elbo_workspace_size / lvae_gp_elbo_fwd_f64 / lvae_gp_elbo_bwd_f64 at their edges, in the manner of
test_gpu_dubo_abi.py: every return code in the documented order with nothing written, the logical extents of the
outputs, and the workspace rules (values against the oracle: test_gpu_gp_elbo.py)."""
import ctypes

import pytest
import torch

import abi_util as U
import dubo_util as D
import gp_elbo_util as G

pytestmark = pytest.mark.gpu
DEV = G.DEV


def test_gp_elbo_return_codes(hip):
    """-1 / -2 (specs), -3 (dims, S = 0 and S = 17 among them), -4 (workspace), in that order, each before any
    launch: nothing is written"""
    from lvae_amd import _lib as P
    S = 3
    c, good0, good1, ok, d = G.abi_inputs("5x3x9", S)
    bad = P.KernelSpec.from_buffer_copy(good0)
    bad.n_comp = 17   # no bucket holds it
    n, o = G.abi_outputs(c, good0, good1, S)
    info = U.sentinel(G.L, torch.int32)
    g = torch.ones(S, G.L, dtype=torch.float64, device=DEV)
    ws, tail = U.workspace(hip.lvae_gp_elbo_workspace_size(ctypes.byref(ok)))
    wsp = ws.data_ptr()
    ins = (P.ptr(d["x"]), P.ptr(d["z"]), P.ptr(d["y"]), P.ptr(d["p0"]), P.ptr(d["p1"]), P.ptr(d["noise"]))

    def fwd(s0, s1, dd, w):
        return hip.lvae_gp_elbo_fwd_f64(s0, s1, dd, *ins, P.ptr(o["elbo"]), P.ptr(info), w, P.stream_ptr())

    def bwd(s0, s1, dd, w):
        return hip.lvae_gp_elbo_bwd_f64(s0, s1, dd, *ins, P.ptr(g), P.ptr(o["dy"]), P.ptr(o["dp0"]), P.ptr(o["dp1"]),
                                        P.ptr(o["dnoise"]), w, P.stream_ptr())

    def dims(**kw):
        return G.make_dims(c, kw.pop("S", S), **kw)
    r = ctypes.byref
    rejected = [(-1, (None, r(good1), r(ok), wsp)), (-1, (r(bad), r(good1), r(ok), wsp)),
                (-2, (r(good0), None, r(ok), wsp)), (-2, (r(good0), r(bad), r(ok), wsp)),
                (-3, (r(good0), r(good1), None, wsp))]
    for kw in (dict(L=0), dict(M=0), dict(M=129), dict(P=0), dict(T=0), dict(T=129), dict(Q=0), dict(S=0),
               dict(S=17), dict(S=-1)):
        rejected.append((-3, (r(good0), r(good1), r(dims(**kw)), wsp)))
    for w in (None, wsp + 8, wsp + 128):   # NULL or not 256-B aligned
        rejected.append((-4, (r(good0), r(good1), r(ok), w)))
    # the order: spec0, then spec1, then the dims, then the workspace
    rejected += [(-1, (r(bad), r(bad), r(dims(S=17)), None)), (-2, (r(good0), r(bad), r(dims(S=0)), None)),
                 (-3, (r(good0), r(good1), r(dims(S=17)), None))]
    for want, a in rejected:
        assert fwd(*a) == want and bwd(*a) == want, (want, a)
    torch.cuda.synchronize()
    assert all(U.all_sentinel(t) for t in o.values()) and U.all_sentinel(info)
    assert bool((ws == 0x7F).all())
    assert fwd(r(good0), r(good1), r(ok), wsp) == 0 and bwd(r(good0), r(good1), r(ok), wsp) == 0
    torch.cuda.synchronize()
    assert U.tail_untouched(tail)
    assert not any(U.all_sentinel(t[:n[k]]) for k, t in o.items())


@pytest.mark.parametrize("cid,S", [("6x7x33", 3), ("17x3x9", 1), ("3x33x17", 16), ("4x32x17", 16)])
def test_gp_elbo_writes_its_logical_extents_only(hip, cid, S):
    """elbo, dy, dparams0 / 1, dnoise and info: every logical element overwritten, the sentinels behind each
    buffer and behind the workspace untouched"""
    out, info, bufs, n = G.abi_run(hip, cid, S)
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), k
        assert U.all_sentinel(bufs[k][n[k]:]), k
    assert info[:G.L].tolist() == [0] * G.L
    assert U.all_sentinel(info[G.L:].to(DEV))
    ref = G.oracle(cid, S)   # (hyper-parameters from the CPU transform here: the bounds of test_gpu_gp_elbo.py apply)
    assert G.rel(out["elbo"], ref["elbo"]) < G.BOUND["elbo"]
    assert G.rel(out["dy"], ref["dy"]) < G.BOUND["dy"]


def test_gp_elbo_workspace_and_optional_outputs(hip):
    from lvae_amd import _lib as P
    for cid in ("3x1x1", "9x16x120", "2x128x128"):
        for S in (1, 16):
            c, _, _, dims, _ = G.abi_inputs(cid, S)
            size = int(hip.lvae_gp_elbo_workspace_size(ctypes.byref(dims)))
            assert size > 0 and size % 256 == 0
            assert size >= 8 * G.L * c["N"] * c["M"] * 2   # at least K0xz and iBK
    full, _, _, _ = G.abi_run(hip, "6x7x33", 3)
    part, info, bufs, n = G.abi_run(hip, "6x7x33", 3, want_info=False, want_dnoise=False)
    assert info is None and U.all_sentinel(bufs["dnoise"])
    for k in ("elbo", "dy", "dp0", "dp1"):
        assert U.bit_equal(part[k], full[k]), k
    assert ctypes.sizeof(P.GpElboDims) == 32   # 6 int32, double
    d = P.GpElboDims(16, 120, 256, 16, 6, 4, 1e-6)   # the size query needs no GPU state: the workload's shape
    assert int(P.load().lvae_gp_elbo_workspace_size(ctypes.byref(d))) > 8 * 16 * 4096 * 120 * 2


@pytest.mark.parametrize("cid", ["6x7x33", "3x33x17"])
def test_gp_elbo_backward_twice_on_one_workspace(hip, cid):
    """the backward leaves the forward's workspace usable: a second call gives the same bits"""
    (a, b), _, _, _ = G.abi_run(hip, cid, 3, bwd_calls=2)
    for k in ("dy", "dp0", "dp1", "dnoise"):
        assert bool(torch.isfinite(a[k]).all()), k
        assert U.bit_equal(a[k], b[k]), k
    assert D.problem(cid)["N"] == a["dy"].shape[1]
