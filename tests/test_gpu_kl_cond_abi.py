"""lvae_kl_cond_workspace_size / lvae_kl_cond_prepare_f64 at their edges, in the manner of
test_gpu_dubo_cond_abi.py: every return code in the documented order with nothing written, the extents of state,
workspace and info, l0 / L_state, what n == 0 never reads, and the info words (values against the oracle:
test_gpu_kl_cond.py)."""
import ctypes

import pytest
import torch

import abi_util as U
import kl_cond_util as C

pytestmark = pytest.mark.gpu
DEV = C.DEV
L = C.L


def test_return_codes_in_order_with_nothing_written(hip):
    from lvae_amd import _lib as P
    cid = "5+17"
    c, good, d = C.abi_inputs(cid)
    bad = P.KernelSpec.from_buffer_copy(good)
    bad.n_comp = 17   # no bucket holds it
    N, Nn, Q = c["N"], c["Nn"], d["xn"].shape[1]
    state, _ = U.workspace(hip.lvae_dubo_cond_state_size(L, Nn, 1))
    ws, _ = U.workspace(hip.lvae_kl_cond_workspace_size(N, Nn, L))
    info = U.sentinel(L, torch.int32)
    r = ctypes.byref
    ok = dict(spec=r(good), xt=d["xt"].data_ptr(), ldx=Q, n=N, xn=d["xn"].data_ptr(), ldn=Q, nn=Nn, L=L,
              p=d["p"].data_ptr(), noise=d["noise"].data_ptr(), mu=d["mu"].data_ptr(), ld_mu=L, lv=d["lv"].data_ptr(),
              ld_lv=L, state=state.data_ptr(), L_state=L, l0=0, info=info.data_ptr(), ws=ws.data_ptr())

    def prep(**kw):
        a = dict(ok)
        a.update(kw)
        return hip.lvae_kl_cond_prepare_f64(*a.values(), P.stream_ptr())
    sp, wp = ok["state"], ok["ws"]
    rejected = [(-1, dict(spec=None)), (-1, dict(spec=r(bad))), (-2, dict(xt=None)), (-3, dict(ldx=1)),
                (-3, dict(ldx=4)), (-4, dict(n=-1)), (-5, dict(xn=None)), (-6, dict(ldn=4)), (-7, dict(nn=0)),
                (-7, dict(nn=-3)), (-8, dict(L=0)), (-8, dict(L=65536, L_state=65536)), (-9, dict(p=None)),
                (-10, dict(noise=None)), (-11, dict(mu=None)), (-12, dict(ld_mu=L - 1)), (-13, dict(lv=None)),
                (-14, dict(ld_lv=L - 1)), (-15, dict(state=None)), (-15, dict(state=sp + 8)), (-15, dict(state=sp + 128)),
                (-16, dict(L_state=0)), (-16, dict(l0=-1)), (-16, dict(l0=1)), (-16, dict(L=2, L_state=3, l0=2)),
                (-17, dict(info=None)), (-18, dict(ws=None)), (-18, dict(ws=wp + 8)), (-18, dict(ws=wp + 128))]
    # the order: each code with everything after it bad too
    order = ["spec", "xt", "ldx", "n", "xn", "ldn", "nn", "L", "p", "noise", "mu", "ld_mu", "lv", "ld_lv", "state",
             "L_state", "info", "ws"]
    wrong = dict(spec=None, xt=None, ldx=0, xn=None, ldn=0, nn=0, L=0, p=None, noise=None, mu=None, ld_mu=0, lv=None,
                 ld_lv=0, state=None, L_state=0, info=None, ws=None)
    for k, name in enumerate(order):
        if name == "n":
            continue   # (n < 0 turns the training arguments' checks off: its own entry above)
        rejected.append((-(k + 1), {q: wrong[q] for q in order[k:] if q != "n"}))
    for want, kw in rejected:
        assert prep(**kw) == want, (want, kw)
    torch.cuda.synchronize()
    assert U.all_sentinel(info) and bool((ws == 0x7F).all()) and bool((state == 0x7F).all())
    # and the accepted call writes
    assert prep() == 0
    torch.cuda.synchronize()
    assert info.tolist() == [0] * L
    assert all(bool(torch.isfinite(t).all()) for t in C.read_state(state, Nn)[:4])


@pytest.mark.parametrize("cid", ["70+33", "37+1", f"{C.SLAB + 3}+40"])
def test_extents_and_reproducibility(hip, cid):
    """tails of state, workspace and info untouched after real calls (kl_cond_util.prepare asserts them); two runs
    give the same state; the eval on it writes its logical extents alone and leaves the state as it was"""
    a, b = C.prepare(hip, cid), C.prepare(hip, cid)
    assert a["info"].tolist() == [0] * L
    n = a["state_bytes"]
    assert n == a["state"].numel() - 256
    sa, sb = C.read_state(a["state"], a["Nn"]), C.read_state(b["state"], b["Nn"])
    assert all(U.bit_equal(x, y) for x, y in zip(sa, sb))
    m, lv, _ = C.point(cid, "far")
    ra, rb = C.evaluate(hip, a, m, lv, C.COT), C.evaluate(hip, b, m, lv, C.COT)
    for k in ra:
        assert bool(torch.isfinite(ra[k]).all()) and U.bit_equal(ra[k], rb[k]), k
    assert all(U.bit_equal(x, y) for x, y in zip(sa, C.read_state(a["state"], a["Nn"])))
    assert U.tail_untouched(a["state_tail"])


@pytest.mark.parametrize("cid", ["70+33", "0+5"])
def test_l0_and_L_state_write_only_their_dims(hip, cid):
    """one dim at a time into a sentinel-filled state: after the call for dim l the later dims' c, r, a and A are still
    sentinels, and the finished state is the all-at-once call's"""
    from lvae_amd import _lib as P
    c, s, d = C.abi_inputs(cid)
    N, Nn, Q, n_par = c["N"], c["Nn"], d["xn"].shape[1], d["p"].shape[1]
    whole = C.read_state(C.prepare(hip, cid)["state"], Nn)
    st, stail = U.workspace(hip.lvae_dubo_cond_state_size(L, Nn, 1))
    ws, wtail = U.workspace(hip.lvae_kl_cond_workspace_size(N, Nn, 1))
    info = U.sentinel(L, torch.int32)
    at = lambda t, off: ctypes.c_void_p(t.data_ptr() + off * t.element_size())
    sent = 0x7F7F7F7F7F7F7F7F
    for l0 in (1, 0, 2):   # (in any order)
        rc = hip.lvae_kl_cond_prepare_f64(ctypes.byref(s), P.ptr(d["xt"]) if N else None, Q, N, P.ptr(d["xn"]), Q, Nn, 1,
                                          at(d["p"], l0 * n_par), at(d["noise"], l0), at(d["mu"], l0) if N else None, L,
                                          at(d["lv"], l0) if N else None, L, P.ptr(st), L, l0, at(info, l0), P.ptr(ws),
                                          P.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        done = {1: (1,), 0: (0, 1), 2: (0, 1, 2)}[l0]
        got = C.read_state(st, Nn)
        for l in range(L):
            for q, g, w in zip(C.STATE, got, whole):
                if l in done:
                    assert U.bit_equal(g[l:l + 1], w[l:l + 1]), (l0, l, q)
                else:
                    assert bool((U.bits(g[l:l + 1].contiguous()) == sent).all()), (l0, l, q)
            assert (int(U.bits(info)[l]) == 0) == (l in done)
    assert U.tail_untouched(stail) and U.tail_untouched(wtail) and info.tolist() == [0] * L


def test_no_training_rows_never_reads_the_training_arguments(hip):
    """n == 0: NULL x_train / mu_train / logv_train are accepted (kl_cond_util.prepare passes NULL), and pointers to
    NaN give the same state"""
    from lvae_amd import _lib as P
    cid = "0+5"
    a = C.prepare(hip, cid)
    c, s, d = C.abi_inputs(cid)
    Nn, Q = c["Nn"], d["xn"].shape[1]
    nan = U.sentinel(64)
    st, _ = U.workspace(hip.lvae_dubo_cond_state_size(L, Nn, 1))
    ws, _ = U.workspace(hip.lvae_kl_cond_workspace_size(0, Nn, L))
    info = U.sentinel(L, torch.int32)
    rc = hip.lvae_kl_cond_prepare_f64(ctypes.byref(s), P.ptr(nan), Q, 0, P.ptr(d["xn"]), Q, Nn, L, P.ptr(d["p"]),
                                      P.ptr(d["noise"]), P.ptr(nan), L, P.ptr(nan), L, P.ptr(st), L, 0, P.ptr(info),
                                      P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and info.tolist() == [0] * L and U.all_sentinel(nan)
    assert all(U.bit_equal(x, y) for x, y in zip(C.read_state(a["state"], Nn), C.read_state(st, Nn)))


@pytest.mark.parametrize("cid", ["70+33", "0+5"])
def test_a_failing_dim_is_reported_and_leaves_the_others(hip, cid):
    """a negative noise for dim 1: with training rows K_tt of that dim fails (info = its column, below 20000), without
    them S fails at its first column (info = 20001); dims 0 and 2 are the clean run's bits"""
    c = C.problem(cid)
    noise = c["noise"].copy()
    noise[1] = -50.0
    clean, bad = C.prepare(hip, cid), C.prepare(hip, cid, noise=noise)
    print(cid, "info", bad["info"].tolist())
    assert clean["info"].tolist() == [0, 0, 0] and bad["info"][0] == 0 and bad["info"][2] == 0
    if c["N"]:
        assert 1 <= int(bad["info"][1]) <= c["N"]
    else:
        assert int(bad["info"][1]) == 20001
    sc, sb = C.read_state(clean["state"], c["Nn"]), C.read_state(bad["state"], c["Nn"])
    for l in (0, 2):
        assert all(U.bit_equal(x[l:l + 1], y[l:l + 1]) for x, y in zip(sc[:4], sb[:4])), l


def test_workspace_size(hip):
    for n, nn, Lh in [(0, 1, 1), (1, 1, 1), (70, 33, 3), (C.SLAB + 3, 40, 2)]:
        b = hip.lvae_kl_cond_workspace_size(n, nn, Lh)
        assert b > 0 and b % 256 == 0
    for bad in [(-1, 5, 3), (4, 0, 3), (4, 5, 0)]:
        assert hip.lvae_kl_cond_workspace_size(*bad) == 0
