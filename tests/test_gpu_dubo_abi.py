"""lvae_dubo_workspace_size / lvae_dubo_fwd_f64 / lvae_dubo_bwd_f64 at their edges, in the manner of
test_gpu_hensman_abi.py: every return code in the documented order with nothing written, the logical extents of
the outputs, and the workspace rules (values against the oracle: test_gpu_dubo.py)."""
import ctypes

import pytest
import torch

import abi_util as U
import dubo_util as D

pytestmark = pytest.mark.gpu
DEV = D.DEV


def test_dubo_return_codes(hip):
    """-1 / -2 (specs), -3 (dims), -4 (workspace), in that order, each before any launch: nothing is written"""
    from lvae_amd import _lib as P
    c, good0, good1, ok, d = D.abi_inputs("5x3x9")
    bad = P.KernelSpec.from_buffer_copy(good0)
    bad.n_comp = 17   # no bucket holds it
    n, o = D.abi_outputs(c, good0, good1)
    info = U.sentinel(D.L, torch.int32)
    g = torch.ones(D.L, dtype=torch.float64, device=DEV)
    ws, tail = U.workspace(hip.lvae_dubo_workspace_size(ctypes.byref(ok)))
    wsp = ws.data_ptr()
    ins = (P.ptr(d["x"]), P.ptr(d["z"]), P.ptr(d["mu"]), P.ptr(d["lv"]), P.ptr(d["p0"]), P.ptr(d["p1"]),
           P.ptr(d["noise"]))

    def fwd(s0, s1, dd, w):
        return hip.lvae_dubo_fwd_f64(s0, s1, dd, *ins, P.ptr(o["dubo"]), P.ptr(info), w, P.stream_ptr())

    def bwd(s0, s1, dd, w):
        return hip.lvae_dubo_bwd_f64(s0, s1, dd, *ins, P.ptr(g), P.ptr(o["dmu"]), P.ptr(o["dlogv"]), P.ptr(o["dp0"]),
                                     P.ptr(o["dp1"]), P.ptr(o["dnoise"]), w, P.stream_ptr())

    def dims(**kw):
        f = dict(L=D.L, M=c["M"], P=c["P"], T=c["T"], Q=c["X"].shape[1])
        f.update(kw)
        return P.DuboDims(f["L"], f["M"], f["P"], f["T"], f["Q"], D.EPS)
    r = ctypes.byref
    rejected = [(-1, (None, r(good1), r(ok), wsp)), (-1, (r(bad), r(good1), r(ok), wsp)),
                (-2, (r(good0), None, r(ok), wsp)), (-2, (r(good0), r(bad), r(ok), wsp)),
                (-3, (r(good0), r(good1), None, wsp))]
    for kw in (dict(L=0), dict(M=0), dict(M=129), dict(P=0), dict(T=0), dict(T=129), dict(Q=0)):
        rejected.append((-3, (r(good0), r(good1), r(dims(**kw)), wsp)))
    for w in (None, wsp + 8, wsp + 128):   # NULL or not 256-B aligned
        rejected.append((-4, (r(good0), r(good1), r(ok), w)))
    # the order: spec0, then spec1, then the dims, then the workspace
    rejected += [(-1, (r(bad), r(bad), r(dims(M=0)), None)), (-2, (r(good0), r(bad), r(dims(M=0)), None)),
                 (-3, (r(good0), r(good1), r(dims(T=129)), None))]
    for want, a in rejected:
        assert fwd(*a) == want and bwd(*a) == want, (want, a)
    torch.cuda.synchronize()
    assert all(U.all_sentinel(t) for t in o.values()) and U.all_sentinel(info)
    assert bool((ws == 0x7F).all())
    assert fwd(r(good0), r(good1), r(ok), wsp) == 0 and bwd(r(good0), r(good1), r(ok), wsp) == 0
    torch.cuda.synchronize()
    assert U.tail_untouched(tail)
    assert not any(U.all_sentinel(t[:n[k]]) for k, t in o.items())


@pytest.mark.parametrize("cid", ["6x7x33", "17x3x9", "3x33x17"])
def test_dubo_writes_its_logical_extents_only(hip, cid):
    """dubo, dmu, dlogv, dparams0 / 1, dnoise and info: every logical element overwritten, the sentinels behind
    each buffer and behind the workspace untouched"""
    out, info, bufs, n = D.abi_run(hip, cid)
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), k
        assert U.all_sentinel(bufs[k][n[k]:]), k
    assert info[:D.L].tolist() == [0] * D.L
    assert U.all_sentinel(info[D.L:].to(DEV))
    ref = D.oracle(cid)   # (hyper-parameters from the CPU transform here: the bounds of test_gpu_dubo.py apply)
    assert D.rel(out["dubo"], ref["dubo"]) < D.BOUND["dubo"] and D.rel(out["dmu"], ref["dmu"]) < D.BOUND["dmu"]
    assert D.rel(out["dlogv"], ref["dlogv"]) < D.BOUND["dlogv"]


def test_dubo_workspace_and_optional_outputs(hip):
    from lvae_amd import _lib as P
    for cid in ("3x1x1", "9x16x120", "2x128x128"):
        c, _, _, dims, _ = D.abi_inputs(cid)
        size = int(hip.lvae_dubo_workspace_size(ctypes.byref(dims)))
        assert size > 0 and size % 256 == 0
        assert size >= 8 * D.L * c["N"] * c["M"] * 2   # at least K0xz and iBK
    full, _, _, _ = D.abi_run(hip, "6x7x33")
    part, info, bufs, n = D.abi_run(hip, "6x7x33", want_info=False, want_dnoise=False)
    assert info is None and U.all_sentinel(bufs["dnoise"])
    for k in ("dubo", "dmu", "dlogv", "dp0", "dp1"):
        assert U.bit_equal(part[k], full[k]), k
    assert ctypes.sizeof(P.DuboDims) == 32   # 5 int32 + pad, double
    d = P.DuboDims(16, 120, 256, 16, 6, 1e-6)   # the size query needs no GPU state: the workload's shape
    assert int(P.load().lvae_dubo_workspace_size(ctypes.byref(d))) > 8 * 16 * 4096 * 120 * 2
