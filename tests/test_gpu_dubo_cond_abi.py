"""lvae_dubo_cond_state_size / lvae_dubo_cond_prepare_f64 / lvae_dubo_cond_eval_f64 at their edges, in the manner of
test_gpu_dubo_abi.py: every return code in the documented order with nothing written, the extents of state,
workspace and outputs, what is never read, reproducibility, and the optional arguments (values against the oracle:
test_gpu_dubo_cond.py)."""
import ctypes

import pytest
import torch

import abi_util as U
import dubo_cond_util as C

pytestmark = pytest.mark.gpu
DEV = C.DEV
L = C.L
NAN = float("nan")


def test_return_codes_in_order_with_nothing_written(hip):
    from lvae_amd import _lib as P
    cid = "5x3x9"
    c, good0, good1, ok, d = C.abi_inputs(cid)
    bad = P.KernelSpec.from_buffer_copy(good0)
    bad.n_comp = 17   # no bucket holds it
    Pn, T, Nn = c["Pn"], c["T"], c["Nn"]
    state, _ = U.workspace(hip.lvae_dubo_cond_state_size(L, Pn, T))
    ws, _ = U.workspace(hip.lvae_dubo_workspace_size(ctypes.byref(ok)))
    info = U.sentinel(L, torch.int32)
    sp, wp, fp = state.data_ptr(), ws.data_ptr(), d["free"].data_ptr()
    ins = (P.ptr(d["x"]), P.ptr(d["z"]), P.ptr(d["mu"]), P.ptr(d["lv"]), P.ptr(d["p0"]), P.ptr(d["p1"]),
           P.ptr(d["noise"]))

    def prep(s0, s1, dd, pn, free, st, w):
        return hip.lvae_dubo_cond_prepare_f64(s0, s1, dd, None, pn, free, *ins, st, P.ptr(info), w, P.stream_ptr())

    def dims(**kw):
        f = dict(L=L, M=c["M"], P=c["P"], T=c["T"], Q=c["X"].shape[1])
        f.update(kw)
        return P.DuboDims(f["L"], f["M"], f["P"], f["T"], f["Q"], C.EPS)
    r = ctypes.byref
    rejected = [(-1, (None, r(good1), r(ok), Pn, fp, sp, wp)), (-1, (r(bad), r(good1), r(ok), Pn, fp, sp, wp)),
                (-2, (r(good0), None, r(ok), Pn, fp, sp, wp)), (-2, (r(good0), r(bad), r(ok), Pn, fp, sp, wp)),
                (-3, (r(good0), r(good1), None, Pn, fp, sp, wp))]
    for kw in (dict(L=0), dict(M=0), dict(M=129), dict(P=0), dict(T=0), dict(T=129), dict(Q=0)):
        rejected.append((-3, (r(good0), r(good1), r(dims(**kw)), Pn, fp, sp, wp)))
    for pn in (0, -1, c["P"] + 1):
        rejected.append((-3, (r(good0), r(good1), r(ok), pn, fp, sp, wp)))
    for w in (None, wp + 8, wp + 128):
        rejected.append((-4, (r(good0), r(good1), r(ok), Pn, fp, sp, w)))
    for s in (None, sp + 8, sp + 128):
        rejected.append((-5, (r(good0), r(good1), r(ok), Pn, fp, s, wp)))
    rejected.append((-6, (r(good0), r(good1), r(ok), Pn, None, sp, wp)))
    # the order: spec0, spec1, the dims and Pn, the workspace, the state, free_idx
    rejected += [(-1, (r(bad), r(bad), r(dims(M=0)), 0, None, None, None)),
                 (-2, (r(good0), r(bad), r(dims(M=0)), 0, None, None, None)),
                 (-3, (r(good0), r(good1), r(ok), 0, None, None, None)),
                 (-4, (r(good0), r(good1), r(ok), Pn, None, None, None)),
                 (-5, (r(good0), r(good1), r(ok), Pn, None, None, wp))]
    for want, a in rejected:
        assert prep(*a) == want, (want, a)
    torch.cuda.synchronize()
    assert U.all_sentinel(info) and bool((ws == 0x7F).all()) and bool((state == 0x7F).all())

    m, lv, _ = C.point(cid, "own")
    md, ld = m.to(DEV), lv.to(DEV)
    o = dict(dubo=U.sentinel(L), dm=U.sentinel(Nn * L), dlogv=U.sentinel(Nn * L))

    def ev(l_, pn, t, st, m_, lv_, du, dm, dl):
        return hip.lvae_dubo_cond_eval_f64(l_, pn, t, st, m_, lv_, None, du, dm, dl, P.stream_ptr())
    outs = (o["dubo"].data_ptr(), o["dm"].data_ptr(), o["dlogv"].data_ptr())
    mp, lp = md.data_ptr(), ld.data_ptr()
    rejected = [(-3, (0, Pn, T, sp, mp, lp, *outs)), (-3, (L, 0, T, sp, mp, lp, *outs)),
                (-3, (L, Pn, 0, sp, mp, lp, *outs)), (-5, (L, Pn, T, None, mp, lp, *outs)),
                (-5, (L, Pn, T, sp + 8, mp, lp, *outs)), (-7, (L, Pn, T, sp, None, lp, *outs)),
                (-7, (L, Pn, T, sp, mp, None, *outs))]
    for k in range(3):
        a = list(outs)
        a[k] = None
        rejected.append((-7, (L, Pn, T, sp, mp, lp, *a)))
    rejected += [(-3, (0, Pn, T, None, None, None, None, None, None)), (-5, (L, Pn, T, None, None, None, None, None, None))]
    for want, a in rejected:
        assert ev(*a) == want, (want, a)
    torch.cuda.synchronize()
    assert all(U.all_sentinel(t) for t in o.values()) and bool((state == 0x7F).all())
    # and the accepted calls write
    assert prep(r(good0), r(good1), r(ok), Pn, fp, sp, wp) == 0
    assert ev(L, Pn, T, sp, mp, lp, *outs) == 0
    torch.cuda.synchronize()
    assert info.tolist() == [0] * L
    assert all(bool(torch.isfinite(t).all()) for t in o.values())


@pytest.mark.parametrize("cid", ["6x7x33", "3x33x17", "12x32x17"])
def test_extents_reproducibility_and_optional_arguments(hip, cid):
    """tails of state, workspace and outputs untouched after real calls and NaN-filled outputs overwritten
    (dubo_cond_util's runners assert both); two prepare + eval runs give the same bits; g = NULL is g = ones;
    info = NULL changes nothing"""
    m, lv, _ = C.point(cid, "far")
    a = C.prepare(hip, cid)
    b = C.prepare(hip, cid, want_info=False)
    assert a["info"].tolist() == [0] * L and b["info"] is None
    n = int(hip.lvae_dubo_cond_state_size(L, a["Pn"], a["T"]))
    assert n == a["state"].numel() - 256 and U.bit_equal(a["state"][:n], b["state"][:n])
    ra, rb = C.evaluate(hip, a, m, lv, C.COT), C.evaluate(hip, b, m, lv, C.COT)
    none, ones = C.evaluate(hip, a, m, lv, None), C.evaluate(hip, a, m, lv, (1.0, 1.0, 1.0))
    for k in ra:
        assert bool(torch.isfinite(ra[k]).all()), k
        assert U.bit_equal(ra[k], rb[k]) and U.bit_equal(none[k], ones[k]), k
    assert U.bit_equal(a["state"][:n], b["state"][:n])   # the evals left the state as it was


@pytest.mark.parametrize("cid", ["6x7x33", "3x33x17"])
def test_free_rows_are_not_read_at_prepare(hip, cid):
    c = C.problem(cid)
    mu, lv = c["mu"].clone(), c["lv"].clone()
    mu[c["rows"]] = NAN
    lv[c["rows"]] = NAN
    a, b = C.prepare(hip, cid), C.prepare(hip, cid, mu=mu, lv=lv)
    n = int(hip.lvae_dubo_cond_state_size(L, a["Pn"], a["T"]))
    assert U.bit_equal(a["state"][:n], b["state"][:n])
    assert b["info"].tolist() == [0] * L


# free subjects and seg_len per case: padding in free and fixed subjects, a one-row free subject
SEG = {"6x7x33": (7, 3, 7, 5, 1, 6), "3x33x17": (33, 20, 9), "12x32x17": (32, 5, 31, 1, 32, 7, 20, 32, 2, 9, 32, 17)}


def _seg_problem(cid):
    """the case made ragged: (seg, valid rows [N] bool, valid free rows [Nn] bool)"""
    c = C.problem(cid)
    seg = torch.tensor(SEG[cid])
    valid = (torch.arange(c["T"])[None, :] < seg[:, None]).reshape(-1)
    return c, seg, valid, valid[c["rows"]]


@pytest.mark.parametrize("cid", list(SEG))
def test_padding_rows(hip, cid):
    """with seg_len: the padding of A, a and r is exact 0; NaN in padding rows at prepare and at eval changes nothing;
    padding gradients are exact 0; the values are the oracle's on the valid rows"""
    import varying_util as V
    c, seg, valid, vfree = _seg_problem(cid)
    mu, lv = c["mu"].clone(), c["lv"].clone()
    mu[~valid] = NAN
    lv[~valid] = NAN
    a, b = C.prepare(hip, cid, seg=seg), C.prepare(hip, cid, seg=seg, mu=mu, lv=lv)
    n = int(hip.lvae_dubo_cond_state_size(L, a["Pn"], a["T"]))
    assert U.bit_equal(a["state"][:n], b["state"][:n])
    Nn = a["Nn"]
    al = lambda k: (8 * k + 255) // 256 * 256
    st = a["state"]
    off = al(L)
    r = st[off:off + 8 * L * Nn].view(torch.float64).reshape(L, Nn).cpu()
    off += al(L * Nn)
    av = st[off:off + 8 * L * Nn].view(torch.float64).reshape(L, Nn).cpu()
    off += al(L * Nn)
    A = st[off:off + 8 * L * Nn * Nn].view(torch.float64).reshape(L, Nn, Nn).cpu()
    off += al(L * Nn * Nn)
    mask = st[off:off + 4 * Nn].view(torch.int32).cpu()
    assert mask.tolist() == vfree.int().tolist()
    assert bool((r[:, ~vfree] == 0).all()) and bool((av[:, ~vfree] == 0).all())
    assert bool((A[:, ~vfree, :] == 0).all()) and bool((A[:, :, ~vfree] == 0).all())
    assert bool((av[:, vfree] > 0).all())
    m, l, cot = C.point(cid, "far")
    mn, ln = m.clone(), l.clone()
    mn[~vfree] = NAN
    ln[~vfree] = NAN
    clean, dirty = C.evaluate(hip, a, m, l, cot), C.evaluate(hip, b, mn, ln, cot)
    for k in clean:
        assert U.bit_equal(clean[k], dirty[k]), k
    assert bool((clean["dm"][~vfree] == 0).all()) and bool((clean["dlogv"][~vfree] == 0).all())
    # the oracle on the valid rows alone (varying_util's loop form: subjects from the id column)
    keep = torch.nonzero(valid).reshape(-1)
    pos = torch.full((c["N"],), -1, dtype=torch.long)
    pos[keep] = torch.arange(keep.numel())
    rows = pos[c["rows"]][vfree]
    dubo = lambda p0, p1, nz, x, mj, lj, d: V.loop_dubo(c["s0"], p0[d], c["s1"], p1[d], nz[d], x, mj[:, d], lj[:, d],
                                                        c["Z"][d], 2, C.EPS)
    ref = C.oracle_at(c, m[vfree], l[vfree], cot, x=c["X"][keep], mu=c["mu"][keep], logv=c["lv"][keep], rows=rows,
                      dubo_fn=dubo)
    got = dict(dubo=clean["dubo"], dm=clean["dm"][vfree], dlogv=clean["dlogv"][vfree])
    C.check(got, ref, f"seg {cid}")


@pytest.mark.parametrize("cid", ["6x7x33", "3x33x17"])
def test_seg_null_is_seg_all_T(hip, cid):
    c = C.problem(cid)
    a, b = C.prepare(hip, cid), C.prepare(hip, cid, seg=[c["T"]] * c["P"])
    m, lv, cot = C.point(cid, "far")
    C.check(C.evaluate(hip, b, m, lv, cot), C.evaluate(hip, a, m, lv, cot), f"seg all-T {cid}")


def test_a_failing_dim_is_reported_and_leaves_the_others(hip):
    """a negative noise for dim 1 (past the positivity transform, as dubo_util.noise_stub hands it over): B_p of that
    dim fails at its first column, info = 20001; dims 0 and 2 are the clean run's bits"""
    cid = "5x3x9"
    c = C.problem(cid)
    noise = c["noise"].copy()
    noise[1] = -50.0
    clean, bad = C.prepare(hip, cid), C.prepare(hip, cid, noise=noise)
    assert clean["info"].tolist() == [0, 0, 0]
    assert bad["info"][0] == 0 and bad["info"][2] == 0 and 20001 <= int(bad["info"][1]) <= 20000 + c["T"]
    m, lv, cot = C.point(cid, "far")
    x, y = C.evaluate(hip, clean, m, lv, cot), C.evaluate(hip, bad, m, lv, cot)
    for d in (0, 2):
        assert U.bit_equal(x["dubo"][d], y["dubo"][d])
        assert U.bit_equal(x["dm"][:, d].contiguous(), y["dm"][:, d].contiguous())
        assert U.bit_equal(x["dlogv"][:, d].contiguous(), y["dlogv"][:, d].contiguous())
        C.check({k: (v[d:d + 1] if k == "dubo" else v[:, d]) for k, v in y.items()},
                {k: (v[d:d + 1] if k == "dubo" else v[:, d]) for k, v in C.oracle(cid, "far").items()},
                f"failing dim, dim {d}")
