"""lvae_hensman_fwd_f64 / lvae_hensman_fwd_part_f64 / lvae_hensman_bwd_f64 through the C ABI, against the fp64
oracle on the CPU (O.hensman_kld, O.hensman_kld_iter and autograd through them), at the (M, T, P_b) where the
composites or the primitives under them take another path, with hand-written kernel specs (abi_util.spec_pairs:
the reference split and two mixed-bucket pairs), hyper-parameters and noise uniform in [0.5, 2] per latent dim,
m random, H = X X^T / 100 + 0.1 I and the jitter eps = 1e-3 (one case at the reference's 1e-6).

Tolerances.  Nothing is fixed in advance: per case and quantity the yardstick is the larger of (a) the change of
the oracle's own output when every floating-point input (hyper-parameters, noise, m, H re-symmetrised, mu, logv)
is perturbed by a relative 2^-50 of random sign (fixed seed) and (b) the spread between the oracle on the CPU
(LAPACK) and the same formula in torch fp64 on the device.  The kernel must be within max(10 x yardstick, 2e-12)
(2e-12 = 2^-53 x the longest sum, ~2^14 terms), and never looser than the project's caps: 1e-8 (bound), 1e-6
(gradients), 1e-4 (gradients through B_p: dparams1, dnoise).  Entries that the oracle gives as exact zeros, with
and without the perturbation, are compared exactly.

Measured on the MI355X (per case the quantity closest to its bound over both natural_gradient settings and the
values / gkld / n_total / share runs; the yardstick is max((a), (b)), bound = max(10 x yardstick, 2e-12)):
    case          quantity                  kernel err   yardstick   err / yardstick   bound     err / bound
    1x1x1         dparams1                  9.54e-15     1.96e-14    0.49              2.0e-12   0.005
    16-ref        dH                        2.95e-14     2.51e-14    1.2               2.0e-12   0.015
    16-mix1       dH (gkld = -2.5)          1.53e-14     1.39e-14    1.1               2.0e-12   0.008
    17-ref        grad_H (share = 0.25)     7.69e-13     4.93e-13    1.6               4.9e-12   0.157
    17-mix1       dH                        1.97e-13     1.71e-13    1.2               2.0e-12   0.099
    17-mix2       dH                        1.11e-14     1.68e-14    0.66              2.0e-12   0.006
    33x32         dH                        1.17e-14     2.15e-14    0.54              2.0e-12   0.006
    65x64         dH                        1.25e-12     2.61e-13    4.8               2.6e-12   0.481
    128x128       kld                       1.14e-12     3.21e-13    3.6               3.2e-12   0.356
    rows-wrap     dH                        1.70e-14     1.49e-14    1.1               2.0e-12   0.009
    var-40x16     dparams1 (gkld = -2.5)    1.46e-11     5.60e-12    2.6               5.6e-11   0.261
    var-17-mix1   grad_H (share = 0.25)     1.89e-13     1.62e-13    1.2               2.0e-12   0.095
    var-17-mix2   dH                        3.27e-15     4.11e-15    0.8               2.0e-12   0.002
    eps1e-6       dm                        1.80e-11     1.53e-11    1.2               1.5e-10   0.120
The bound itself (kld): err <= 3.2e-12 at eps = 1e-3 (var-40x16: 3.14e-12 against a yardstick of 1.52e-12), 3.13e-11
at eps = 1e-6 (yardstick 7.94e-11).  The caps never decided.  The module's 64 GPU tests take about 4 s together.

Found by these tests: with seg_len set and natural_gradient, grad_m was NaN when the padding rows of mu held NaN
(u = iB mu read them: 0 x NaN through iB's identity padding).  The varying-T path now forms u from a masked copy
of mu; the fixed-T path is unchanged.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import abi_util as U
from oracle import lvae_oracle as O

gpu = pytest.mark.gpu
DEV = U.DEV
PAIRS = U.spec_pairs()

# id: (pair, L, M, T, P_b, seg_len, eps)
CASES = {
    "1x1x1": ("ref", 1, 1, 1, 1, None, 1e-3),                      # the smallest of everything
    "16-ref": ("ref", 2, 16, 16, 2, None, 1e-3),                   # spd_inv_small's n <= 16 template, M and T
    "16-mix1": ("mix1", 2, 16, 16, 2, None, 1e-3),
    "17-ref": ("ref", 3, 17, 17, 3, None, 1e-3),                   # the first switch, past it
    "17-mix1": ("mix1", 3, 17, 17, 3, None, 1e-3),
    "17-mix2": ("mix2", 3, 17, 17, 3, None, 1e-3),
    "33x32": ("mix2", 2, 33, 32, 2, None, 1e-3),                   # second switch: T on it, M past it
    "65x64": ("ref", 2, 65, 64, 2, None, 1e-3),                    # third switch
    "128x128": ("mix1", 2, 128, 128, 2, None, 1e-3),               # both limits; M M and P_b T T wrap the 2048 stride
    "rows-wrap": ("mix2", 1, 16, 128, 17, None, 1e-3),             # B = 2176 > 2048; nb2 = 17 in the batched GEMMs
    "var-40x16": ("ref", 3, 40, 16, 5, (16, 1, 7, 0, 16), 1e-3),   # full, one-row, ragged and empty subjects
    "var-17-mix1": ("mix1", 3, 17, 17, 3, (17, 16, 1), 1e-3),
    "var-17-mix2": ("mix2", 2, 17, 17, 3, (17, 16, 1), 1e-3),
    "eps1e-6": ("ref", 3, 40, 16, 5, None, 1e-6),                  # the production jitter
}
CASE_IDS = list(CASES)
CAPS = dict(kld=1e-8, dp1=1e-4, dnoise=1e-4)   # (every other quantity: 1e-6)
QUANT = ["kld", "gm", "gH", "dm", "dH", "dmu", "dlogv", "dp0", "dp1", "dnoise", "iH", "gm_q", "gH_q"]
SHARE = 0.25


@functools.lru_cache(maxsize=None)
def problem(cid):
    pair, L, M, T, P_b, seg, eps = CASES[cid]
    s0, s1 = PAIRS[pair]
    rng = np.random.default_rng(1000 + CASE_IDS.index(cid))
    gen = torch.Generator().manual_seed(2000 + CASE_IDS.index(cid))
    B = P_b * T
    Xh = torch.randn(L, M, M, generator=gen, dtype=torch.float64)
    valid = torch.ones(P_b, T, dtype=torch.bool)
    if seg is not None:
        valid = torch.arange(T)[None, :] < torch.tensor(seg)[:, None]
    P_tot = float(4 * P_b + 3)
    c = dict(cid=cid, s0=s0, s1=s1, L=L, M=M, T=T, P_b=P_b, seg=seg, eps=eps, B=B, P_tot=P_tot,
             x=U.subject_covariates(rng, P_b, T).reshape(B, U.QC), z=U.inducing_points(rng, L, M, T),
             p0=U.draw_hypers(rng, L, O.n_params(s0)), p1=U.draw_hypers(rng, L, O.n_params(s1)),
             noise=U.draw_hypers(rng, L, None), m=torch.randn(L, M, 1, generator=gen, dtype=torch.float64),
             H=Xh @ Xh.transpose(1, 2) / 100.0 + 0.1 * torch.eye(M, dtype=torch.float64),
             mu=torch.randn(B, L, generator=gen, dtype=torch.float64),
             logv=0.1 * torch.randn(B, L, generator=gen, dtype=torch.float64), valid=valid.reshape(B))
    if seg is not None:   # elbo.py's P_tot' = P P_b / P_in (P_b counts the empty subject), N = n_total
        c["P_in"] = sum(1 for s in seg if s > 0)
        c["n_total"] = float(7 * sum(seg) + 5)
        c["P_call"] = P_tot * P_b / c["P_in"]
    else:
        c["n_total"], c["P_call"] = 0.0, P_tot
    return c


FLOAT_INPUTS = ["p0", "p1", "noise", "m", "H", "mu", "logv"]


def oracle(cid, dev="cpu", perturb=False):
    """Every compared quantity from the oracle (one evaluation, autograd for the gradients); perturb: the
    floating-point inputs times 1 + 2^-50 s.  Gradients of padding rows are zeros.  cid: a case id, or a problem
    in problem()'s keys (ext_util.hensman_problem; its perturb_cols names covariate columns perturbed as well)."""
    c = problem(cid) if isinstance(cid, str) else cid
    v = {k: c[k] for k in FLOAT_INPUTS}
    x, z = c["x"], c["z"]
    if perturb:
        gen = torch.Generator().manual_seed(77)
        v = {k: U.perturbed(t, gen) for k, t in v.items()}
        v["H"] = 0.5 * (v["H"] + v["H"].transpose(1, 2))
        x, z = x.clone(), z.clone()
        for q in c.get("perturb_cols", []):
            x[..., q] = U.perturbed(x[..., q], gen)
            z[..., q] = U.perturbed(z[..., q], gen)
    ok = c["valid"]
    v["mu"], v["logv"] = v["mu"][ok], v["logv"][ok]
    v = {k: t.detach().clone().to(dev).requires_grad_() for k, t in v.items()}
    x, z = x[ok].to(dev), z.to(dev)
    if c["seg"] is None:
        kld, gm, gH = O.hensman_kld(c["s0"], v["p0"], c["s1"], v["p1"], v["noise"], v["m"], v["H"], x, v["mu"],
                                    v["logv"], z, c["P_tot"], c["P_b"], c["T"], True, c["eps"])
    else:
        kld, gm, gH = O.hensman_kld_iter(c["s0"], v["p0"], c["s1"], v["p1"], v["noise"], v["m"], v["H"], x, v["mu"],
                                         v["logv"], z, c["P_tot"], c["P_in"], c["n_total"], True, U.ID_COL, c["eps"])
    kld.backward()
    with torch.no_grad():
        eye = torch.eye(c["M"], dtype=torch.float64, device=dev)
        K0zz = O.gram(c["s0"], v["p0"], z, z) + c["eps"] * eye
        iK = torch.cholesky_solve(eye, torch.linalg.cholesky(K0zz))
        iH = torch.cholesky_solve(eye, torch.linalg.cholesky(v["H"]))
        out = dict(kld=kld.reshape(1), gm=gm, gH=gH, dm=v["m"].grad, dH=v["H"].grad, dp0=v["p0"].grad,
                   dp1=v["p1"].grad, dnoise=v["noise"].grad, iH=iH,
                   gm_q=gm - (1.0 - SHARE) * (iK @ v["m"]), gH_q=gH - 0.5 * (1.0 - SHARE) * (iK - iH))
        for k, g in (("dmu", v["mu"].grad), ("dlogv", v["logv"].grad)):
            full = torch.zeros(c["B"], c["L"], dtype=torch.float64, device=dev)
            full[ok.to(dev)] = g
            out[k] = full
    return {k: t.detach().cpu() for k, t in out.items()}


@functools.lru_cache(maxsize=None)
def cpu_ref(cid):
    """(oracle, perturbed oracle, yardstick (a) per quantity) on the CPU"""
    ref, per = oracle(cid), oracle(cid, perturb=True)
    return ref, per, {k: U.rel(per[k], ref[k]) for k in QUANT}


@functools.lru_cache(maxsize=None)
def yardstick(cid):
    """max((a) perturbation, (b) CPU / device oracle spread) per quantity"""
    ref, _, ya = cpu_ref(cid)
    dev = oracle(cid, DEV)
    return {k: max(ya[k], U.rel(dev[k], ref[k])) for k in QUANT}


def bound(key, yard):
    return min(max(10.0 * yard, 2e-12), CAPS.get(key, 1e-6))


def test_cases_reach_the_paths_and_are_well_conditioned():
    """The case lists of this module and of test_gpu_predict_abi.py, on the CPU: every oracle Cholesky succeeds
    (the oracle raises otherwise), the perturbation yardsticks at eps = 1e-3 are below 1e-9 (the caps never
    decide), the shapes reach each spd_inv_small template, the 2048-row wrap, and the second predict chunk."""
    import test_gpu_predict_abi as TP
    from lvae_amd import _lib as P
    for name, (s0, s1) in PAIRS.items():
        for s in (s0, s1):
            assert P.make_spec(s).n_params == O.n_params(s)
            assert all(d in (5, 7) for comp in s for k, d in comp if k == "bin")
    assert [U.bucket(s) for s in PAIRS["ref"]] == [(8, 2), (8, 2)]
    assert [U.bucket(s) for s in PAIRS["mix1"]] == [(8, 2), (16, 4)] and max(len(c) for c in PAIRS["mix1"][1]) >= 3
    assert [U.bucket(s) for s in PAIRS["mix2"]] == [(16, 4), (8, 2)] and len(PAIRS["mix2"][0]) >= 9
    worst = 0.0
    for cid, (pair, L, M, T, P_b, seg, eps) in CASES.items():
        assert 1 <= L <= 3
        ref, _, ya = cpu_ref(cid)
        assert all(bool(torch.isfinite(t).all()) for t in ref.values()), cid
        print(f"{cid}: yardstick (a) " + " ".join(f"{k} {ya[k]:.1e}" for k in QUANT))
        if eps == 1e-3:
            worst = max(worst, max(ya.values()))
    assert worst < 1e-9
    for n in ("M", "T"):
        sizes = [c[2] if n == "M" else c[3] for c in CASES.values()]
        assert any(s <= 16 for s in sizes) and any(17 <= s <= 32 for s in sizes)
        assert any(33 <= s <= 64 for s in sizes) and any(s > 64 for s in sizes)
    assert any(c[4] * c[3] > 2048 for c in CASES.values())
    assert any(c[5] is not None and 0 in c[5] and 1 in c[5] for c in CASES.values())
    assert {c[0] for c in CASES.values() if c[5] is not None} >= {"ref", "mix1", "mix2"}
    assert {CASES[k][2] for k in CASES} >= {1, 17, 128}   # lvae_hensman_iH_offset at these M
    # predict
    for cid in TP.CASES:
        ref, ya = TP.cpu_ref(cid)
        if ref is not None:
            assert bool(torch.isfinite(ref).all()) and ya < 1e-9, cid
            print(f"predict {cid}: yardstick (a) {ya:.1e}")
    L, M, Pn, T, Nt = TP.CASES["chunked"][1:6]
    rows = TP.chunk_rows(P.load(), L, M, Pn, T)
    assert rows < Nt == rows + 1 and -(-Nt // rows) >= 2


# ------------------------------------------------------------------------------------------------------
# one forward + backward through the C ABI
# ------------------------------------------------------------------------------------------------------
OUT_NAMES = ["kld", "gm", "gH", "dm", "dH", "dmu", "dlogv", "dp0", "dp1", "dnoise"]


def x_filled(c, fill_seed):
    """x with the padding rows replaced by other finite covariates (another draw per fill_seed)"""
    if c["seg"] is None:
        return c["x"]
    other = U.subject_covariates(np.random.default_rng(fill_seed), c["P_b"], c["T"]).reshape(c["B"], U.QC)
    return torch.where(c["valid"][:, None], c["x"], other)


def run(hip, cid, ng, pad=float("nan"), fill_seed=1, gk=1.0, n_total=None, share=1.0, want_info=True,
        want_dnoise=True, split=False, overrides=None):
    """Forward then backward on one sentinel-tailed workspace, every output pre-filled with sentinels.  Returns
    ({name: CPU tensor}, info, H^-1 as left in the workspace)."""
    from lvae_amd import _lib as P
    c = problem(cid) if isinstance(cid, str) else cid
    L, M, T, P_b, B = c["L"], c["M"], c["T"], c["P_b"], c["B"]
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    t = {k: c[k].clone() for k in FLOAT_INPUTS}
    t.update(overrides or {})
    t["mu"][~c["valid"]] = pad
    t["logv"][~c["valid"]] = pad
    d = {k: v.to(DEV).contiguous() for k, v in t.items()}
    x, z = x_filled(c, fill_seed).to(DEV).contiguous(), c["z"].to(DEV).contiguous()
    seg = torch.tensor(c["seg"], dtype=torch.int32, device=DEV) if c["seg"] is not None else None
    dims = P.HensmanDims(L, M, P_b, T, U.QC, c["P_call"], c["eps"], int(ng), share,
                         seg.data_ptr() if seg is not None else None, c["n_total"] if n_total is None else n_total)
    o = dict(kld=U.sentinel(1), gm=U.sentinel(L * M), gH=U.sentinel(L * M * M), dm=U.sentinel(L * M),
             dH=U.sentinel(L * M * M), dmu=U.sentinel(B * L), dlogv=U.sentinel(B * L),
             dp0=U.sentinel(L * s0.n_params), dp1=U.sentinel(L * s1.n_params), dnoise=U.sentinel(L))
    info = U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_hensman_workspace_size(ctypes.byref(dims)))
    g = torch.tensor([gk], dtype=torch.float64, device=DEV)
    st = P.stream_ptr()
    common = (P.ptr(x), P.ptr(z), P.ptr(d["m"]), P.ptr(d["H"]))
    hyp = (P.ptr(d["p0"]), P.ptr(d["p1"]), P.ptr(d["noise"]))
    fout = (P.ptr(o["kld"]), P.ptr(o["gm"]), P.ptr(o["gH"]), P.ptr(info) if want_info else None, P.ptr(ws), st)
    if split:   # part 1 sees neither mu nor logv, nor kld and info (part 2 writes them)
        rc = hip.lvae_hensman_fwd_part_f64(1, ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), *common, None,
                                           None, *hyp, None, P.ptr(o["gm"]), P.ptr(o["gH"]), None, P.ptr(ws), st)
        assert rc == 0
        rc = hip.lvae_hensman_fwd_part_f64(2, ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), *common,
                                           P.ptr(d["mu"]), P.ptr(d["logv"]), *hyp, *fout)
    else:
        rc = hip.lvae_hensman_fwd_f64(ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), *common, P.ptr(d["mu"]),
                                      P.ptr(d["logv"]), *hyp, *fout)
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)
    off = int(hip.lvae_hensman_iH_offset(ctypes.byref(dims)))
    iH = ws[off:off + L * M * M * 8].view(torch.float64).view(L, M, M).cpu()
    rc = hip.lvae_hensman_bwd_f64(ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), *common, P.ptr(d["mu"]),
                                  P.ptr(d["logv"]), *hyp, P.ptr(g), P.ptr(o["dmu"]), P.ptr(o["dlogv"]), P.ptr(o["dp0"]),
                                  P.ptr(o["dp1"]), P.ptr(o["dnoise"]) if want_dnoise else None, P.ptr(o["dm"]),
                                  P.ptr(o["dH"]), P.ptr(ws), st)
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)   # lvae_hensman_workspace_size bytes are enough, forward and backward
    # outputs of the other path stay sentinel; everything else is overwritten with finite values
    idle = ("dm", "dH") if ng else ("gm", "gH")
    for k in OUT_NAMES:
        if k in idle or (k == "dnoise" and not want_dnoise):
            assert U.all_sentinel(o[k]), k
        else:
            assert bool(torch.isfinite(o[k]).all()), k
    if not want_info:
        assert U.all_sentinel(info)
    shapes = dict(kld=(1,), gm=(L, M, 1), gH=(L, M, M), dm=(L, M, 1), dH=(L, M, M), dmu=(B, L), dlogv=(B, L),
                  dp0=(L, -1), dp1=(L, -1), dnoise=(L,))
    return {k: o[k].cpu().reshape(shapes[k]) for k in OUT_NAMES}, info.cpu(), iH


def active(ng, want_dnoise=True):
    ks = ["kld", "dmu", "dlogv", "dp0", "dp1"] + (["gm", "gH"] if ng else ["dm", "dH"])
    return ks + (["dnoise"] if want_dnoise else [])


def same_bits(a, b, keys):
    return all(U.bit_equal(a[k], b[k]) for k in keys)


def check(cid, ng, got, want, yard, tag, rename=None):
    """got[k] within the bound of want[k] for every active quantity; exact where the oracle is an exact zero"""
    ref, per, _ = cpu_ref(cid)
    for k in active(ng) + (["iH"] if "iH" in got else []):
        rk = (rename or {}).get(k, k)
        err, tol = U.rel(got[k], want[rk]), bound(rk, yard[rk])
        print(f"hensman {cid} ng={ng} {tag} {rk}: err {err:.2e} yardstick {yard[rk]:.2e} "
              f"ratio {err / max(yard[rk], 1e-300):.2g} bound {tol:.1e}")
        assert err <= tol, (k, err, tol)
        zero = (ref[rk] == 0) & (per[rk] == 0)
        assert bool((got[k][zero] == 0).all()), k


@gpu
@pytest.mark.parametrize("ng", [1, 0])
@pytest.mark.parametrize("cid", CASE_IDS)
def test_hensman_values(hip, cid, ng):
    """The bound, every gradient and the H^-1 left at lvae_hensman_iH_offset against the oracle (padding rows of
    mu / logv hold NaN), the padding rows of dmu / dlogv exactly zero, info all zero, and the run repeated:
    bit-identical."""
    c = problem(cid)
    ref, yard = cpu_ref(cid)[0], yardstick(cid)
    got, info, iH = run(hip, cid, ng)
    assert info.tolist() == [0] * c["L"]
    check(cid, ng, dict(got, iH=iH), ref, yard, "values")
    assert bool((got["dmu"][~c["valid"]] == 0).all()) and bool((got["dlogv"][~c["valid"]] == 0).all())
    again, info2, iH2 = run(hip, cid, ng)
    assert same_bits(got, again, active(ng)) and U.bit_equal(iH, iH2) and torch.equal(info, info2)


@gpu
@pytest.mark.parametrize("ng", [1, 0])
@pytest.mark.parametrize("cid", [k for k in CASE_IDS if CASES[k][5] is not None])
def test_hensman_padding_is_masked(hip, cid, ng):
    """Padding rows: mu / logv are not read (NaN there or 0: the same bits out), x may hold any finite
    covariates (two fills: the same bits out)."""
    nan_pad, _, _ = run(hip, cid, ng)
    zero_pad, _, _ = run(hip, cid, ng, pad=0.0)
    for k in active(ng):
        assert U.bit_equal(nan_pad[k], zero_pad[k]), k
    other_x, _, _ = run(hip, cid, ng, fill_seed=2)
    assert not torch.equal(x_filled(problem(cid), 1), x_filled(problem(cid), 2))
    for k in active(ng):
        assert U.bit_equal(nan_pad[k], other_x[k]), k


@gpu
@pytest.mark.parametrize("ng", [1, 0])
@pytest.mark.parametrize("cid", CASE_IDS)
def test_hensman_scalings_nulls_and_split(hip, cid, ng):
    """gkld = -2.5 scales every gradient, n_total shifts the bound, ng_prior_share = 0.25 weighs the
    data-independent directions; NULL info / dnoise change nothing else; part 1 (no mu / logv) + part 2 = part 0."""
    c = problem(cid)
    ref, yard = cpu_ref(cid)[0], yardstick(cid)
    base, info, _ = run(hip, cid, ng)
    # gkld
    got, _, _ = run(hip, cid, ng, gk=-2.5)
    want = {k: (v if k in ("kld", "gm", "gH") else -2.5 * v) for k, v in ref.items()}
    check(cid, ng, got, want, yard, "gkld=-2.5")
    # n_total = X: kld shifts by -L (X - N0) / 2, N0 the case's own N
    n0 = c["n_total"] if c["seg"] is not None else c["P_tot"] * c["T"]
    X = n0 + 37.0
    got, _, _ = run(hip, cid, ng, n_total=X)
    want = dict(ref, kld=ref["kld"] - c["L"] * (X - n0) / 2.0)
    check(cid, ng, got, want, yard, "n_total")
    assert same_bits(got, base, [k for k in active(ng) if k != "kld"])
    # ng_prior_share
    got, _, _ = run(hip, cid, ng, share=SHARE)
    check(cid, ng, got, ref, yard, "share=0.25", rename=dict(gm="gm_q", gH="gH_q"))
    assert same_bits(got, base, [k for k in active(ng) if k not in ("gm", "gH")])
    # NULL info, NULL dnoise
    got, _, _ = run(hip, cid, ng, want_info=False, want_dnoise=False)
    assert same_bits(got, base, active(ng, want_dnoise=False))
    # split forward
    got, info2, _ = run(hip, cid, ng, split=True)
    assert same_bits(got, base, active(ng)) and torch.equal(info, info2)


# ------------------------------------------------------------------------------------------------------
# info and return codes
# ------------------------------------------------------------------------------------------------------
def _info_run(hip, eps, noise, H):
    from lvae_amd import _lib as P
    c = U.info_problem()
    L, M, T, P_b = c["L"], c["M"], c["T"], c["P_b"]
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    dims = P.HensmanDims(L, M, P_b, T, U.QC, 11.0, eps, 1, 1.0, None, 0.0)
    dv = lambda t: t.to(DEV).contiguous()
    x, z, p0, p1, nz, Hd = dv(c["x"]), dv(c["z"]), dv(c["p0"]), dv(c["p1"]), dv(noise), dv(H)
    m, mu, lv = (torch.zeros(n, dtype=torch.float64, device=DEV) for n in (L * M, P_b * T * L, P_b * T * L))
    kld, gm, gH = U.sentinel(1), U.sentinel(L * M), U.sentinel(L * M * M)
    info = U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_hensman_workspace_size(ctypes.byref(dims)))
    rc = hip.lvae_hensman_fwd_f64(ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), P.ptr(x), P.ptr(z), P.ptr(m),
                                  P.ptr(Hd), P.ptr(mu), P.ptr(lv), P.ptr(p0), P.ptr(p1), P.ptr(nz), P.ptr(kld),
                                  P.ptr(gm), P.ptr(gH), P.ptr(info), P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and U.tail_untouched(tail)
    return info.cpu().tolist()


@gpu
def test_hensman_info_codes_and_precedence(hip):
    """info[l] = 10000 / 20000 / 30000 + the failing column of K0zz / B_p / H, the first of them in that order;
    matrices indefinite by construction in dim 1 only (nothing is asserted about kld)."""
    L, M = 3, 3
    good_noise = torch.ones(L, dtype=torch.float64)
    eye = torch.eye(M, dtype=torch.float64).expand(L, M, M).contiguous()
    assert _info_run(hip, 1e-3, good_noise, eye) == [0, 0, 0]
    # K0zz[1] = 1.5 I - 3 I (dims 0, 2: 6 I - 3 I); B_p[1] has the diagonal 1 - 2; H[1] = diag(1, -1, 1)
    bad_eps = -3.0
    bad_noise = good_noise.clone()
    bad_noise[1] = -(2 * 0.5 + 1.0)
    for j in range(M):
        bad_H = eye.clone()
        bad_H[1, j, j] = -1.0
        assert _info_run(hip, 1e-3, good_noise, bad_H) == [0, 30000 + j + 1, 0]
    bad_H = eye.clone()
    bad_H[1, 1, 1] = -1.0
    assert _info_run(hip, bad_eps, good_noise, eye) == [0, 10001, 0]
    assert _info_run(hip, 1e-3, bad_noise, eye) == [0, 20001, 0]
    assert _info_run(hip, bad_eps, bad_noise, eye) == [0, 10001, 0]
    assert _info_run(hip, bad_eps, good_noise, bad_H) == [0, 10001, 0]
    assert _info_run(hip, 1e-3, bad_noise, bad_H) == [0, 20001, 0]
    assert _info_run(hip, bad_eps, bad_noise, bad_H) == [0, 10001, 0]


@gpu
def test_hensman_return_codes(hip):
    """Every code hensman.hip returns for a bad argument, each rejected before any launch: nothing is written."""
    from lvae_amd import _lib as P
    c = problem("16-ref")
    L, M, T, P_b, B = c["L"], c["M"], c["T"], c["P_b"], c["B"]
    good0, good1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    bad = P.KernelSpec.from_buffer_copy(good0)
    bad.n_comp = 17   # no bucket holds it
    dv = lambda t: t.to(DEV).contiguous()
    x, z, m, H, mu, lv, p0, p1, nz = (dv(c[k]) for k in ("x", "z", "m", "H", "mu", "logv", "p0", "p1", "noise"))
    g = torch.ones(1, dtype=torch.float64, device=DEV)
    outs = [U.sentinel(n) for n in (1, L * M, L * M * M, B * L, B * L, L * good0.n_params, L * good1.n_params, L,
                                    L * M, L * M * M)]
    kld, gm, gH, dmu, dlv, dp0, dp1, dnz, dm, dH = outs
    info = U.sentinel(L, torch.int32)

    def dims(**kw):
        f = dict(L=L, M=M, P_b=P_b, T=T, Q=U.QC)
        f.update(kw)
        return P.HensmanDims(f["L"], f["M"], f["P_b"], f["T"], f["Q"], c["P_tot"], c["eps"], 1, 1.0, None, 0.0)
    ws, tail = U.workspace(hip.lvae_hensman_workspace_size(ctypes.byref(dims())))
    wsp = ws.data_ptr()

    def fwd(part, s0, s1, d, w):
        rc = hip.lvae_hensman_fwd_part_f64(part, s0, s1, d, P.ptr(x), P.ptr(z), P.ptr(m), P.ptr(H), P.ptr(mu),
                                           P.ptr(lv), P.ptr(p0), P.ptr(p1), P.ptr(nz), P.ptr(kld), P.ptr(gm),
                                           P.ptr(gH), P.ptr(info), w, P.stream_ptr())
        rc1 = rc if part else hip.lvae_hensman_fwd_f64(s0, s1, d, P.ptr(x), P.ptr(z), P.ptr(m), P.ptr(H), P.ptr(mu),
                                                       P.ptr(lv), P.ptr(p0), P.ptr(p1), P.ptr(nz), P.ptr(kld),
                                                       P.ptr(gm), P.ptr(gH), P.ptr(info), w, P.stream_ptr())
        assert rc1 == rc   # (part 0 and the one-call entry point agree)
        return rc

    def bwd(s0, s1, d, w):
        return hip.lvae_hensman_bwd_f64(s0, s1, d, P.ptr(x), P.ptr(z), P.ptr(m), P.ptr(H), P.ptr(mu), P.ptr(lv),
                                        P.ptr(p0), P.ptr(p1), P.ptr(nz), P.ptr(g), P.ptr(dmu), P.ptr(dlv), P.ptr(dp0),
                                        P.ptr(dp1), P.ptr(dnz), P.ptr(dm), P.ptr(dH), w, P.stream_ptr())
    r = ctypes.byref
    ok = dims()
    rejected = [(-1, (None, r(good1), r(ok), wsp)), (-1, (r(bad), r(good1), r(ok), wsp)),
                (-2, (r(good0), None, r(ok), wsp)), (-2, (r(good0), r(bad), r(ok), wsp)),
                (-3, (r(good0), r(good1), None, wsp))]
    for kw in (dict(L=0), dict(M=0), dict(M=129), dict(P_b=0), dict(T=0), dict(T=129), dict(Q=0)):
        rejected.append((-3, (r(good0), r(good1), r(dims(**kw)), wsp)))
    for want, (s0, s1, d, w) in rejected:
        assert fwd(0, s0, s1, d, w) == want and fwd(1, s0, s1, d, w) == want and fwd(2, s0, s1, d, w) == want
        assert bwd(s0, s1, d, w) == want
    for w in (None, wsp + 8, wsp + 128):   # NULL or not 256-B aligned
        assert fwd(0, r(good0), r(good1), r(ok), w) == -17 and bwd(r(good0), r(good1), r(ok), w) == -21
    assert fwd(3, r(good0), r(good1), r(ok), wsp) == -18 and fwd(-1, r(good0), r(good1), r(ok), wsp) == -18
    assert fwd(3, r(good0), r(good1), r(dims(M=0)), None) == -3   # the dims are checked first, then part, then ws
    assert fwd(3, r(good0), r(good1), r(ok), None) == -18
    torch.cuda.synchronize()
    assert all(U.all_sentinel(t) for t in outs) and U.all_sentinel(info)
    assert bool((ws == 0x7F).all())
    assert fwd(0, r(good0), r(good1), r(ok), wsp) == 0 and bwd(r(good0), r(good1), r(ok), wsp) == 0
    torch.cuda.synchronize()
    assert not U.all_sentinel(kld) and U.tail_untouched(tail)   # (the same calls with nothing wrong run)
