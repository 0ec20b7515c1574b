"""lvae_kl_closed_* and lvae_spd_inv_chol_f32 through the C ABI against the fp64 oracle on the CPU (O.kl_closed per
latent dim, autograd for dmu, dlogv, dparams, dnoise), at the shapes where the exact-KL path takes another host
schedule or route, with strided operands (ld_mu = L + 3, ldx = Q + 2), NaN in every input's padding, sentinels in
every output and behind the workspace, and the route gates (kl_hyper.hip, kl_resid_bins.hip) at their thresholds.

Inputs: health_mnist_covariates rows cut to n (or hand-built integer covariates for the gate cases), the reference
kernel set, hyper-parameters uniform in [0.5, 2] (abi_util.draw_hypers), noise in [0.5, 1] unless the case says
otherwise, mu ~ N(0, 1), logv ~ 0.1 N(0, 1), gkl distinct per dim and of alternating sign.

Bounds.  Nothing is fixed in advance.  Per case and quantity the yardstick is the worst error, against the fp64
oracle, of the same oracle evaluated in fp32 on the CPU, over the case's inputs and three copies with params, mu and
logv perturbed by one fp32 ulp (a single fp32 sample can land by luck far below its typical error).  The kernel must
be within max(8 x yardstick, FLOOR), FLOOR = 2^-23 (fp32 epsilon): 8 = 4 (the header's ~2^-22 per product against
fp32's 2^-24) x 2 (the yardstick's own sample noise).  Errors are relative max-norm errors per latent dim (dmu,
dlogv: the dim's column; dparams: its row), the worst dim counting; kl and dnoise, one number per dim, in the
max-norm over the dims.  dmu = gkl K^-1 mu is refined once in fp64 and sits far below that bound (the ratio is printed), so
it has a second, tighter one: after one refinement step with an fp64 residual the error of K^-1 mu is the product of
the inverse's relative error and the first solve's, each at most 8 x yardstick, hence (8 x yardstick)^2, floored at
DMU_FLOOR = 2^-53 x 1024 (fp64 sums of fewer than 1024 terms).  Without the refinement dmu errs by ~1e-6.

Measured on the MI355X (per case the quantity closest to its bound, and dmu for the value cases; the yardstick is
the one computed on that machine's CPU, bound = max(8 x yardstick, 2^-23)):
    case            quantity  yardstick  kernel err  err/yardstick  bound     err/bound
    1x1             dparams   9.67e-08   3.67e-07    3.8            7.7e-07   0.47
    1x1             dmu       1.11e-07   6.53e-14    5.9e-07        8.9e-07   7.4e-08
    2x3             dlogv     2.49e-07   2.75e-07    1.1            2.0e-06   0.14
    2x3             dmu       3.55e-07   3.55e-13    1e-06          2.8e-06   1.3e-07
    255x2           dlogv     2.50e-06   1.87e-06    0.75           2.0e-05   0.094
    255x2           dmu       1.21e-06   3.35e-12    2.8e-06        9.6e-06   3.5e-07
    256x3           dlogv     3.21e-06   3.18e-06    0.99           2.6e-05   0.12
    256x3           dmu       2.74e-06   1.03e-11    3.8e-06        2.2e-05   4.7e-07
    257x1           dlogv     1.51e-06   1.53e-06    1              1.2e-05   0.13
    257x1           dmu       2.25e-06   4.71e-12    2.1e-06        1.8e-05   2.6e-07
    300x3           dlogv     5.35e-06   4.00e-06    0.75           4.3e-05   0.093
    300x3           dmu       2.53e-06   7.07e-12    2.8e-06        2.0e-05   3.5e-07
    511x2           dlogv     3.58e-06   3.67e-06    1              2.9e-05   0.13
    511x2           dmu       2.64e-06   1.60e-11    6.1e-06        2.1e-05   7.6e-07
    512x17          dlogv     8.57e-06   1.15e-05    1.3            6.9e-05   0.17
    512x17          dmu       3.89e-06   3.73e-11    9.6e-06        3.1e-05   1.2e-06
    513x2           dlogv     5.45e-06   3.69e-06    0.68           4.4e-05   0.084
    513x2           dmu       2.72e-06   3.13e-11    1.2e-05        2.2e-05   1.4e-06
    513x3           dlogv     4.20e-06   3.37e-06    0.8            3.4e-05   0.1
    513x3           dmu       2.49e-06   1.19e-11    4.8e-06        2.0e-05   6e-07
    700x17          dlogv     7.75e-06   1.41e-05    1.8            6.2e-05   0.23
    700x17          dmu       4.03e-06   1.07e-10    2.7e-05        3.2e-05   3.3e-06
    700x17-binned   dlogv     6.74e-06   1.17e-05    1.7            5.4e-05   0.22
    700x17-binned   dmu       3.89e-06   1.04e-10    2.7e-05        3.1e-05   3.3e-06
    700x22          dlogv     1.01e-05   1.42e-05    1.4            8.1e-05   0.18
    700x22          dmu       4.40e-06   6.86e-11    1.6e-05        3.5e-05   1.9e-06
    noise1e-2       dparams   4.47e-05   2.74e-05    0.61           3.6e-04   0.077
    noise1e-2       dmu       3.77e-05   2.84e-09    7.5e-05        3.0e-04   9.4e-06
    run-64          dlogv     5.60e-06   3.74e-06    0.67           4.5e-05   0.084
    run-65          dparams   1.23e-05   8.67e-06    0.71           9.8e-05   0.088
    ids-5           dlogv     5.81e-07   5.95e-07    1              4.6e-06   0.13
    ids-4           dlogv     1.84e-06   9.33e-07    0.51           1.5e-05   0.063
    cat-16          dlogv     5.10e-06   3.12e-06    0.61           4.1e-05   0.076
    cat-17          dlogv     4.18e-06   1.80e-06    0.43           3.3e-05   0.054
    bins-128        dlogv     9.24e-06   6.32e-06    0.68           7.4e-05   0.085
    bins-129        dlogv     7.25e-06   1.77e-05    2.4            5.8e-05   0.3
    window-64       dlogv     1.63e-06   1.48e-06    0.91           1.3e-05   0.11
    window-65       dlogv     1.11e-06   1.33e-06    1.2            8.9e-06   0.15
    integer         dlogv     1.80e-06   1.54e-06    0.85           1.4e-05   0.11
    half-time       dlogv     2.33e-06   2.87e-06    1.2            1.9e-05   0.15
    300x3 late (A)  dlogv     5.35e-06   4.00e-06    0.75           4.3e-05   0.093
    300x3 early (B) dlogv     5.35e-06   4.08e-06    0.76           4.3e-05   0.095
dmu (K^-1 mu, refined once in fp64) stays 5 to 7 orders below its yardstick; every other quantity sits at 0.4 to 4
times the fp32 oracle's own error.  The floor never decided.

The module's GPU tests take about 12 s together (the CPU references included).

What the tests rest on in the library: the early-reduce decision travels with the workspace (it was a
process-global that a later size query could flip: test_kl_closed_early_route_travels_with_the_workspace), every
argument is validated before any launch, and lvae_kl_closed_resid_state reports the residual's route.  No kernel
was found wrong.  Scratch mutants of the kernels, each against the whole suite: kl_prep_kernel reading mu with L
for ld (every strided test here red, no older test); alpha left at its first solve (every value and gate test here
red through dmu's second bound, and the older test_kl_closed_resid_paths and test_kl_closed_small_noise[0.001]);
the run-length gate's > as >= (the run-64 gate test alone); one hi x lo product dropped in schedule (b)'s rank-256
updates (the four L >= 17 value cases alone).
"""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import abi_util as U
from oracle import lvae_oracle as O

gpu = pytest.mark.gpu
DEV = U.DEV
FLOOR = 2.0 ** -23
FACTOR = 8.0
DMU_FLOOR = 2.0 ** -53 * 1024
QC = 6                       # columns of health_mnist_covariates
SPEC = O.spec_full(**U._REF_CFG)
# four far binnings (the far-bin limit of the binned hyper route needs 4 x 32 bins: three binnings of 128 bins in
# all have sum nbins^2 >= 5462 > 4096, so the 128-bin limit can only decide with four)
SPEC4 = O.spec_full(cat_kernel=[2], bin_kernel=[], sqexp_kernel=[0, 1],
                    cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 3}, {'cont_covariate': 1, 'cat_covariate': 4}],
                    bin_int_kernel=[], covariate_missing_val=[])
QUANT = ["kl", "dmu", "dlogv", "dparams", "dnoise"]


def padded_n(n):
    return (n + 255) // 256 * 256


def pipe_mode(n, L):
    """chol_inv.hip ci_pipe_mode (defaults): the pipelined trtri + lauum for L <= 2 and Np >= 512"""
    return 2 if L <= 2 and padded_n(n) >= 512 else 0


def fused(L):
    """chol_inv.hip kCiFuseMaxL: schedule (a) up to 16 dims per call, (b) above"""
    return L <= 16


def syrk_splits(n, L):
    """syrk_x3.hip syrk_x3_splits: the K splits of the S GEMM (256 x 256 tiles, 256 workgroups a round)"""
    nt = padded_n(n) // 256
    tiles = L * nt * (nt + 1) // 2
    cost = lambda s: ((tiles * s + 255) // 256) / s
    best = 1
    for s in (2, 4):
        if cost(s) < 0.7 * cost(best):
            best = s
    return best


# ------------------------------------------------------------------------------------------------------
# covariates
# ------------------------------------------------------------------------------------------------------
def x_std(n):
    from lvae_amd.data import health_mnist_covariates
    return torch.tensor(health_mnist_covariates(-(-n // 16), 16, seed=3)[:n])


def x_runs(runs, period=16, ncat3=2):
    """Integer covariates with id runs of the given lengths: time = row-in-run mod period, the disease time of
    every second subject, cat 3 = subject mod ncat3, cat 4 = sick"""
    rows = []
    for p, r in enumerate(runs):
        t = np.arange(r) % period
        sick = p % 2
        rows.append(np.stack([t, np.where(sick, t - period // 2, 0), np.full(r, p), np.full(r, p % ncat3),
                              np.full(r, sick), np.zeros(r)], 1))
    return torch.tensor(np.concatenate(rows).astype(np.float64))


def x_bins(w0, w1, r4):
    """SPEC4 covariates with far binnings of w0, w1, w0 and r4 w1 bins: time 0..w0-1, covariate 1 in 0..w1-1, one
    value of cat 3, r4 values of cat 4; 40 ids in runs of 8"""
    i = np.arange(320)
    return torch.tensor(np.stack([i % w0, (5 * i) % w1, i // 8, np.zeros(320), (i // 8) % r4, np.zeros(320)],
                                 1).astype(np.float64))


def x_window(w):
    """the standard layout with the time covariate running over w integer values (5 ids in runs of 52)"""
    i = np.arange(260)
    sick = (i // 52) % 2
    return torch.tensor(np.stack([i % w, np.where(sick, i % 16 - 9, 0), i // 52, (i // 52) % 2, sick,
                                  np.zeros(260)], 1).astype(np.float64))


def x_half(n):
    x = x_std(n)
    x[:, 0] += 0.5
    return x


# id: n, L, then options: x (covariates), spec, hyper ("0": LVAE_KL_HYPER=0, the S-GEMM route), noise, and what the
# state queries must report: on (binned hyper route), binned (binned residual), covflag
def case(n, L, x=None, spec=SPEC, hyper=None, noise=None, on=1, binned=1, covflag=2):
    return dict(n=n, L=L, x=x, spec=spec, hyper=hyper, noise=noise, on=on, binned=binned, covflag=covflag)


VALUE_CASES = {
    "1x1": case(1, 1, on=0),              # one point, one dim (<= 4 ids: the S-GEMM route, 4 splits)
    "2x3": case(2, 3, on=0),
    "255x2": case(255, 2),                # Np = 256: one block; binned hyper route
    "256x3": case(256, 3, hyper="0", on=0),   # S-GEMM route, 4 splits
    "257x1": case(257, 1),                # Np = 512, pipe mode 2
    "300x3": case(300, 3),                # mode 0 at Np = 512 (the early-route test's shape)
    "511x2": case(511, 2, hyper="0", on=0),   # mode 2, S-GEMM route, 4 splits
    "512x17": case(512, 17, hyper="0", on=0),  # schedule (b), 51 tiles: 4 splits
    "513x2": case(513, 2),                # Np = 768, mode 2
    "513x3": case(513, 3),                # Np = 768, mode 0
    "700x17": case(700, 17, hyper="0", on=0),  # schedule (b) at Np = 768, 102 tiles: 2 splits
    "700x17-binned": case(700, 17),       # schedule (b) with the binned hyper route
    "700x22": case(700, 22, hyper="0", on=0),  # 132 tiles: the smallest count (at Np <= 768) with 1 split
    "noise1e-2": case(513, 2, noise=[1.0, 1e-2]),   # the refinement gate flags dim 1 alone
}
GATE_CASES = {
    "run-64": case(320, 2, x=lambda: x_runs([64] * 5)),
    "run-65": case(321, 2, x=lambda: x_runs([64] * 4 + [65]), on=0),
    "ids-5": case(80, 2, x=lambda: x_runs([16] * 5)),
    "ids-4": case(64, 2, x=lambda: x_runs([16] * 4), on=0),
    "cat-16": case(80, 2, x=lambda: x_runs([4] * 20, period=2, ncat3=16)),
    "cat-17": case(80, 2, x=lambda: x_runs([4] * 20, period=2, ncat3=17), on=0),
    "bins-128": case(320, 2, x=lambda: x_bins(32, 32, 1), spec=SPEC4),
    "bins-129": case(320, 2, x=lambda: x_bins(33, 21, 2), spec=SPEC4, on=0),   # 33 + 21 + 33 + 42
    "window-64": case(260, 2, x=lambda: x_window(64), on=0),   # (64 + 128 far bins: the binned hyper route is off)
    "window-65": case(260, 2, x=lambda: x_window(65), on=0, binned=0, covflag=1),   # (also past the tables' range)
    "integer": case(256, 2),
    "half-time": case(256, 2, x=lambda: x_half(256), on=0, binned=0, covflag=0),
}
CASES = dict(VALUE_CASES, **GATE_CASES)
CASE_IDS = list(CASES)
TAU = 16.0   # kl_refine.hip: the gate's default threshold on est_l


@functools.lru_cache(maxsize=None)
def problem(cid):
    c = CASES[cid]
    n, L, spec = c["n"], c["L"], c["spec"]
    k = CASE_IDS.index(cid)
    rng = np.random.default_rng(4000 + k)
    gen = torch.Generator().manual_seed(5000 + k)
    x = x_std(n) if c["x"] is None else c["x"]()
    assert tuple(x.shape) == (n, QC)
    noise = torch.tensor(rng.uniform(0.5, 1.0, L)) if c["noise"] is None else torch.tensor(c["noise"],
                                                                                          dtype=torch.float64)
    gkl = torch.tensor([(-1.0) ** l * (0.5 + (l + 1.0) / (L + 1.0)) for l in range(L)], dtype=torch.float64)
    return dict(c, cid=cid, x=x, params=U.draw_hypers(rng, L, O.n_params(spec)), noise=noise, gkl=gkl,
                mu=torch.randn(n, L, generator=gen, dtype=torch.float64),
                logv=0.1 * torch.randn(n, L, generator=gen, dtype=torch.float64))


def oracle(c, params, mu, logv, dtype):
    """O.kl_closed per latent dim in `dtype` with autograd; {quantity: fp64 CPU tensor}"""
    L, x = c["L"], c["x"].to(dtype)
    out = dict(kl=[], dmu=[], dlogv=[], dparams=[], dnoise=[])
    for l in range(L):
        p = params[l].to(dtype).requires_grad_()
        nz = c["noise"][l].to(dtype).requires_grad_()
        m, v = mu[:, l].to(dtype).requires_grad_(), logv[:, l].to(dtype).requires_grad_()
        kl = O.kl_closed(c["spec"], p, x, nz, m, v)
        (c["gkl"][l].to(dtype) * kl).backward()
        for key, t in (("kl", kl.detach()), ("dmu", m.grad), ("dlogv", v.grad), ("dparams", p.grad),
                       ("dnoise", nz.grad)):
            out[key].append(t.double())
    return dict(kl=torch.stack(out["kl"]), dmu=torch.stack(out["dmu"], 1), dlogv=torch.stack(out["dlogv"], 1),
                dparams=torch.stack(out["dparams"]), dnoise=torch.stack(out["dnoise"]))


def err(key, got, ref):
    """the relative max-norm error of a quantity (module docstring): per dim for dmu / dlogv (columns) and dparams
    (rows), over the dims for kl and dnoise"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if key in ("kl", "dnoise"):
        return U.rel(got, ref)
    if key == "dparams":
        got, ref = got.t(), ref.t()
    return max(U.rel(got[:, l], ref[:, l]) for l in range(ref.shape[1]))


def ulp_perturbed(t, gen):
    """t (1 + 2^-23 s), s = +-1 at random: one fp32 ulp"""
    s = torch.randint(0, 2, t.shape, generator=gen, dtype=torch.int64).to(t.dtype) * 2.0 - 1.0
    return t * (1.0 + 2.0 ** -23 * s)


@functools.lru_cache(maxsize=None)
def cpu_ref(cid):
    """(fp64 oracle, {quantity: yardstick}, the gate's fp64 estimate est [L]) of a case"""
    c = problem(cid)
    ref = oracle(c, c["params"], c["mu"], c["logv"], torch.float64)
    yard = {k: 0.0 for k in QUANT}
    gen = torch.Generator().manual_seed(91)
    for copy in range(4):
        p, m, v = c["params"], c["mu"], c["logv"]
        if copy:
            p, m, v = ulp_perturbed(p, gen), ulp_perturbed(m, gen), ulp_perturbed(v, gen)
        r64 = ref if not copy else oracle(c, p, m, v, torch.float64)
        r32 = oracle(c, p, m, v, torch.float32)
        for k in QUANT:
            yard[k] = max(yard[k], err(k, r32[k], r64[k]))
    # est_l = (sum_r scale_r + noise_l) max_i (K_l^-1)_ii, kl_refine.hip's proxy of the diagonal's error
    from lvae_amd import _lib as P
    s = P.make_spec(c["spec"])
    est = []
    for l in range(c["L"]):
        K = O.gram(c["spec"], c["params"][l], c["x"], c["x"]) + c["noise"][l] * torch.eye(c["n"], dtype=torch.float64)
        ks = float(c["noise"][l]) + sum(float(c["params"][l, s.scale_idx[r]]) for r in range(s.n_comp))
        est.append(ks * float(torch.linalg.inv(K).diagonal().max()))
    return ref, yard, torch.tensor(est, dtype=torch.float64)


def bound(yard):
    return max(FACTOR * yard, FLOOR)


def test_case_lists_reach_the_paths():
    """The case lists on the CPU: every pipe mode, both host schedules at Np = 512 and 768, every split count of
    the S GEMM among the cases that run it, n one below / at / above each block edge; the oracle is finite, no
    case sits within 0.1 % of the refinement gate's threshold, the small-noise case flags exactly dim 1, and the
    gate cases sit exactly at and one past each limit of kl_hyper.hip / kl_resid_bins.hip."""
    V = VALUE_CASES
    assert {c["n"] for c in V.values()} >= {1, 2, 255, 256, 257, 511, 512, 513, 700}
    assert {c["L"] for c in V.values()} >= {1, 2, 3, 17}
    assert max(padded_n(c["n"]) for c in CASES.values()) == 768
    assert {pipe_mode(c["n"], c["L"]) for c in V.values()} == {0, 2}
    for np_ in (512, 768):
        assert any(not fused(c["L"]) and padded_n(c["n"]) == np_ for c in V.values())
        assert any(fused(c["L"]) and padded_n(c["n"]) == np_ for c in V.values())
    gemm = [c for c in V.values() if not c["on"]]   # (the binned hyper route skips the S GEMM)
    assert {syrk_splits(c["n"], c["L"]) for c in gemm} == {1, 2, 4}
    assert all(syrk_splits(n, L) != 1 for n in (256, 512, 768) for L in range(1, 22))   # hence the L = 22 case
    for cid in CASE_IDS:
        c = problem(cid)
        ref, yard, est = cpu_ref(cid)
        assert all(bool(torch.isfinite(t).all()) for t in ref.values()), cid
        assert bool(((est / TAU - 1.0).abs() > 1e-3).all()), (cid, est)
        print(f"{cid}: est max {float(est.max()):.3g}; yardstick " + " ".join(f"{k} {yard[k]:.1e}" for k in QUANT))
        ids = c["x"][:, 2]
        if c["on"] == 1:   # what the device gate needs (kl_hyper.hip hb_plan_kernel)
            assert len(ids.unique()) > 4 and int(ids.unique(return_counts=True)[1].max()) <= 64
    assert (cpu_ref("noise1e-2")[2] > TAU).tolist() == [False, True]
    G = {k: problem(k)["x"] for k in GATE_CASES}
    runs = lambda x: x[:, 2].unique(return_counts=True)[1]
    assert runs(G["run-64"]).tolist() == [64] * 5 and runs(G["run-65"]).tolist() == [64] * 4 + [65]
    assert len(runs(G["ids-5"])) == 5 and len(runs(G["ids-4"])) == 4
    assert len(G["cat-16"][:, 3].unique()) == 16 and len(G["cat-17"][:, 3].unique()) == 17
    assert len(runs(G["cat-16"])) > 17   # (the id stays the widest Cat gate)

    def far_bins(x):   # SPEC4's four far binnings: rbf(0), rbf(1), cat(3) x rbf(0), cat(4) x rbf(1)
        w = lambda d: int(x[:, d].max() - x[:, d].min()) + 1
        return [w(0), w(1), w(3) * w(0), w(4) * w(1)]
    assert far_bins(G["bins-128"]) == [32] * 4 and far_bins(G["bins-129"]) == [33, 21, 33, 42]   # 129
    assert sum(b * b for b in far_bins(G["bins-128"])) == 4096   # (the other limits hold at 128 as well)
    assert len(G["window-64"][:, 0].unique()) == 64 and len(G["window-65"][:, 0].unique()) == 65
    assert bool((G["integer"] == G["integer"].round()).all()) and bool((G["half-time"][:, 0] % 1.0 == 0.5).all())


# ------------------------------------------------------------------------------------------------------
# one problem on the device: strided, NaN-padded inputs, sentinel outputs, an exact workspace
# ------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Session:
    def __init__(self, hip, cid, early=None, ws_tail=256, noise=None):
        from lvae_amd import _lib as P
        self.P, self.hip, self.c = P, hip, problem(cid)
        c = self.c
        n, L = c["n"], c["L"]
        self.n, self.L, self.ld, self.ldx = n, L, L + 3, QC + 2
        self.env = dict(LVAE_KL_HYPER=c["hyper"], LVAE_KL_EARLY=early, LVAE_KL_REFINE=None, LVAE_KL_REFINE_TAU=None,
                        LVAE_RESID_BINS=None)
        self.spec = P.make_spec(c["spec"])
        self.npar = self.spec.n_params
        self.xb, self.x = U.padded(c["x"], (self.ldx, 1))
        self.mub, self.mu = U.padded(c["mu"], (self.ld, 1))
        self.lvb, self.lv = U.padded(c["logv"], (self.ld, 1))
        self.inputs0 = [t.clone() for t in (self.xb, self.mub, self.lvb)]
        self.params = c["params"].to(DEV).contiguous()
        self.noise = (c["noise"] if noise is None else noise).to(DEV).contiguous()
        self.gkl = c["gkl"].to(DEV).contiguous()
        with env(**self.env):
            self.nbytes = int(hip.lvae_kl_closed_workspace_size(n, L))
        self.ws, self.tail = U.workspace(self.nbytes, ws_tail)
        self.reset_outputs()

    def reset_outputs(self):
        n, L = self.n, self.L
        ext = U.extent((n, L), (self.ld, 1)) + 5
        self.kl, self.info = U.sentinel(L), U.sentinel(L, torch.int32)
        self.dmub, self.dlvb = U.sentinel(ext), U.sentinel(ext)
        self.dparams, self.dnoise = U.sentinel(L * self.npar), U.sentinel(L)

    def outputs(self):
        return [self.kl, self.info, self.dmub, self.dlvb, self.dparams, self.dnoise]

    # argument lists (tests of the return codes replace entries)
    def a_problem(self):
        p = self.P.ptr
        return [ctypes.byref(self.spec), p(self.x), self.ldx, self.n, self.L, p(self.params)]

    def a_factor(self):
        p = self.P.ptr
        return self.a_problem() + [p(self.noise), p(self.info), p(self.ws), self.P.stream_ptr()]

    def a_reduce(self, need_bwd=1):
        p = self.P.ptr
        return self.a_problem() + [p(self.noise), p(self.mu), p(self.lv), self.ld, p(self.kl), p(self.ws), need_bwd,
                                   self.P.stream_ptr()]

    def a_fwd(self, need_bwd=1):
        p = self.P.ptr
        return self.a_problem() + [p(self.noise), p(self.mu), p(self.lv), self.ld, p(self.kl), p(self.info),
                                   p(self.ws), need_bwd, self.P.stream_ptr()]

    def a_bwd(self):
        p = self.P.ptr
        return self.a_problem() + [p(self.mu), p(self.lv), self.ld, p(self.gkl), p(self.dmub), p(self.dlvb),
                                   p(self.dparams), p(self.dnoise), p(self.ws), self.P.stream_ptr()]

    def a_latent(self):
        p = self.P.ptr
        return [self.n, self.L, p(self.lv), self.ld, p(self.gkl), p(self.dmub), p(self.dlvb), p(self.ws),
                self.P.stream_ptr()]

    def a_hyper(self):
        p = self.P.ptr
        return self.a_problem() + [p(self.gkl), p(self.dparams), p(self.dnoise), p(self.ws), self.P.stream_ptr()]

    def call(self, name, args):
        with env(**self.env):
            rc = getattr(self.hip, name)(*args)
        torch.cuda.synchronize()
        return rc

    def forward(self, split=False, need_bwd=1):
        if split:
            assert self.call("lvae_kl_closed_factor_f32", self.a_factor()) == 0
            assert self.call("lvae_kl_closed_reduce_f32", self.a_reduce(need_bwd)) == 0
        else:
            assert self.call("lvae_kl_closed_fwd_f32", self.a_fwd(need_bwd)) == 0
        assert U.tail_untouched(self.tail), "the forward wrote past lvae_kl_closed_workspace_size bytes"

    def backward(self, order="whole"):
        if order == "whole":
            assert self.call("lvae_kl_closed_bwd_f32", self.a_bwd()) == 0
        else:
            halves = [("lvae_kl_closed_bwd_latent_f32", self.a_latent()), ("lvae_kl_closed_bwd_hyper_f32", self.a_hyper())]
            for name, args in (halves if order == "latent-first" else halves[::-1]):
                assert self.call(name, args) == 0
        assert U.tail_untouched(self.tail), "the backward wrote past lvae_kl_closed_workspace_size bytes"

    def states(self):
        p, hip, n, L = self.P.ptr, self.hip, self.n, self.L
        est, flag = U.sentinel(L), U.sentinel(L, torch.int32)
        one = [U.sentinel(1, torch.int32) for _ in range(3)]
        st = self.P.stream_ptr()
        assert hip.lvae_kl_closed_refine_state(n, L, p(self.ws), p(est), p(flag), st) == 0
        assert hip.lvae_kl_closed_hyper_state(n, L, p(self.ws), p(one[0]), st) == 0
        assert hip.lvae_kl_closed_resid_state(n, L, p(self.ws), p(one[1]), p(one[2]), st) == 0
        torch.cuda.synchronize()
        return dict(est=est.cpu(), flag=flag.cpu().tolist(), on=int(one[0]), covflag=int(one[1]), binned=int(one[2]))

    def results(self, backward=True):
        """every output on the CPU, after the checks that hold for every run: info zero, the padding of the
        outputs and the inputs untouched, the outputs finite"""
        n, L = self.n, self.L
        assert self.info.cpu().tolist() == [0] * L
        for now, before in zip((self.xb, self.mub, self.lvb), self.inputs0):
            assert U.bit_equal(now, before), "an input was written"
        out = dict(kl=self.kl.cpu())
        if backward:
            for b in (self.dmub, self.dlvb):
                assert U.untouched_outside(b, (n, L), (self.ld, 1)), "dmu / dlogv: padding written"
            out.update(dmu=U.view(self.dmub, (n, L), (self.ld, 1)).cpu(), dlogv=U.view(self.dlvb, (n, L), (self.ld, 1)).cpu(),
                       dparams=self.dparams.cpu().reshape(L, self.npar), dnoise=self.dnoise.cpu())
        else:
            assert all(U.all_sentinel(t) for t in (self.dmub, self.dlvb, self.dparams, self.dnoise))
        assert all(bool(torch.isfinite(t).all()) for t in out.values()), "an output kept its NaN pre-fill"
        return out


def run(hip, cid, split=False, order="whole", need_bwd=1, early=None):
    s = Session(hip, cid, early=early)
    s.forward(split, need_bwd)
    st = s.states()
    if need_bwd:
        s.backward(order)
    return s.results(backward=bool(need_bwd)), st


def check_values(cid, got, tag="", keys=QUANT):
    ref, yard, _ = cpu_ref(cid)
    bad = []
    for k in keys:
        e, tol = err(k, got[k], ref[k]), bound(yard[k])
        print(f"kl_closed {cid} {tag} {k}: yardstick {yard[k]:.2e} kernel err {e:.2e} ratio {e / yard[k]:.2g} "
              f"bound {tol:.1e} err/bound {e / tol:.2g}")
        if k == "dmu":   # the refined solve (module docstring)
            tol = max((FACTOR * yard[k]) ** 2, DMU_FLOOR)
            print(f"kl_closed {cid} {tag} dmu, refined: bound {tol:.1e} err/bound {e / tol:.2g}")
        if not e <= tol:
            bad.append((k, e, tol))
    assert not bad, (cid, tag, bad)


def check_states(cid, st):
    c = problem(cid)
    _, _, est = cpu_ref(cid)
    assert st["flag"] == [int(e > TAU) for e in est.tolist()], (st["flag"], est)
    assert U.rel(st["est"], est) < 1e-3   # (est: a product of fp32-accurate diag K^-1; the gate's margin above)
    for k in ("on", "binned", "covflag"):
        if c[k] is not None:
            assert st[k] == c[k], (cid, k, st)


@gpu
@pytest.mark.parametrize("cid", list(VALUE_CASES))
def test_kl_closed_values(hip, cid):
    """Every output against the oracle within the yardstick bound, strided and NaN-padded, on a workspace of
    exactly lvae_kl_closed_workspace_size bytes; the state queries report the expected routes and gate; fwd =
    factor + reduce and bwd = latent + hyper in either order, bit for bit; a repeated run and a need_bwd = 0
    forward give the same bits."""
    got, st = run(hip, cid)
    check_values(cid, got)
    check_states(cid, st)
    for kw in (dict(split=True, order="latent-first"), dict(order="hyper-first"), dict()):
        again, st2 = run(hip, cid, **kw)
        assert all(U.bit_equal(got[k], again[k]) for k in QUANT), kw
        assert st2["flag"] == st["flag"] and U.bit_equal(st2["est"], st["est"]) and st2["on"] == st["on"]
    fwd_only, _ = run(hip, cid, need_bwd=0)
    assert U.bit_equal(fwd_only["kl"], got["kl"])


@gpu
def test_kl_closed_small_noise_gate(hip):
    """noise 1e-2 in dim 1 of two at n = 513: the gate (LVAE_KL_REFINE unset) flags exactly that dim, and dlogv
    (the refined diagonal) meets the yardstick bound like every other quantity."""
    got, st = run(hip, "noise1e-2")
    assert st["flag"] == [0, 1]
    check_values("noise1e-2", got, keys=["dlogv", "kl"])


@gpu
@pytest.mark.parametrize("pair", [("run-64", "run-65"), ("ids-5", "ids-4"), ("cat-16", "cat-17"),
                                  ("bins-128", "bins-129"), ("window-64", "window-65"), ("integer", "half-time")],
                         ids=lambda p: p[0])
def test_kl_closed_route_gates_at_their_limits(hip, pair):
    """Covariates exactly at a limit of a device-side route gate and one past it: the route the state queries
    report, and every value against the oracle on both sides (dmu within 1e-8 on both sides of the covariate
    coding, as test_kl_closed_resid_paths holds)."""
    seen = []
    for cid in pair:
        got, st = run(hip, cid)
        print(f"{cid}: {st}")
        check_states(cid, st)
        check_values(cid, got)
        seen.append(st)
    if pair[0] == "integer":
        assert (seen[0]["covflag"], seen[1]["covflag"]) == (2, 0)
        for cid in pair:
            got, _ = run(hip, cid)
            assert err("dmu", got["dmu"], cpu_ref(cid)[0]["dmu"]) < 1e-8


@gpu
def test_kl_closed_early_route_travels_with_the_workspace(hip):
    """n = 300, L = 3 (pipe mode 0: the early reduce is live).  Workspace A is sized and factored with
    LVAE_KL_EARLY unset, B with it on; size queries with the other setting come between the forwards and the
    backwards.  A carries a sentinel tail as long as the early route's extra buffers, so a reduce or backward that
    took the early route on A would show as a damaged tail (and as values off their bounds)."""
    cid = "300x3"
    c = problem(cid)
    with env(LVAE_KL_EARLY=None):
        size_off = int(hip.lvae_kl_closed_workspace_size(c["n"], c["L"]))
    with env(LVAE_KL_EARLY="1"):
        size_on = int(hip.lvae_kl_closed_workspace_size(c["n"], c["L"]))
    assert size_on > size_off
    A = Session(hip, cid, early=None, ws_tail=size_on - size_off + 256)
    B = Session(hip, cid, early="1")
    assert (A.nbytes, B.nbytes) == (size_off, size_on)
    A.forward(split=True)
    B.forward(split=True)
    with env(LVAE_KL_EARLY="1"):
        assert int(hip.lvae_kl_closed_workspace_size(c["n"], c["L"])) == size_on
    A.backward()
    with env(LVAE_KL_EARLY=None):
        assert int(hip.lvae_kl_closed_workspace_size(c["n"], c["L"])) == size_off
    B.backward()
    assert U.tail_untouched(A.tail) and U.tail_untouched(B.tail)
    a, b = A.results(), B.results()
    check_values(cid, a, "late (A)")
    check_values(cid, b, "early (B)")
    late, _ = run(hip, cid)
    assert all(U.bit_equal(a[k], late[k]) for k in QUANT)          # A took the default route throughout
    assert not all(U.bit_equal(a[k], b[k]) for k in ("kl", "dmu"))  # and B the other one


# ------------------------------------------------------------------------------------------------------
# return codes: every rejection before any launch, nothing written
# ------------------------------------------------------------------------------------------------------
def _swap(args, i, v):
    a = list(args)
    a[i] = v
    return a


@gpu
def test_kl_closed_return_codes(hip):
    """Every code include/lvae_hip.h documents for the lvae_kl_closed_* family, each call made on sentinel outputs
    and a sentinel workspace that must be untouched afterwards; then the same calls with nothing wrong run."""
    from lvae_amd import _lib as P
    s = Session(hip, "255x2")
    n, L = s.n, s.L
    bad_spec = P.KernelSpec.from_buffer_copy(s.spec)
    bad_spec.n_comp = 17
    wsp = s.ws.data_ptr()
    # (index of the argument in the call's list, replacement) -> the documented code
    problem_rej = [(0, None, -1), (0, ctypes.byref(bad_spec), -1), (1, None, -2), (2, 4, -3), (2, 0, -3), (3, 0, -4),
                   (3, -5, -4), (3, 16385, -4), (3, 16640, -4), (4, 0, -5), (5, None, -6)]
    ws_rej = lambda i, code: [(i, None, code), (i, wsp + 8, code), (i, wsp + 128, code)]
    table = {
        "lvae_kl_closed_factor_f32": (s.a_factor, problem_rej + [(6, None, -7), (7, None, -8)] + ws_rej(8, -9)),
        "lvae_kl_closed_reduce_f32": (s.a_reduce, problem_rej + [(6, None, -7), (7, None, -8), (8, None, -9),
                                                                 (9, L - 1, -10), (10, None, -11)] + ws_rej(11, -12)),
        "lvae_kl_closed_fwd_f32": (s.a_fwd, problem_rej + [(6, None, -7), (7, None, -8), (8, None, -9), (9, L - 1, -10),
                                                           (10, None, -11), (11, None, -12)] + ws_rej(12, -13)),
        "lvae_kl_closed_bwd_f32": (s.a_bwd, problem_rej + [(7, None, -8), (8, L - 1, -9), (9, None, -10),
                                                           (10, None, -11), (11, None, -12), (12, None, -13),
                                                           (13, None, -14)] + ws_rej(14, -15)),
        "lvae_kl_closed_bwd_latent_f32": (s.a_latent, [(0, 0, -4), (0, 16640, -4), (1, 0, -5), (2, None, -8),
                                                       (3, L - 1, -9), (4, None, -10), (5, None, -11), (6, None, -12)]
                                          + ws_rej(7, -15)),
        "lvae_kl_closed_bwd_hyper_f32": (s.a_hyper, problem_rej + [(6, None, -10), (7, None, -13), (8, None, -14)]
                                         + ws_rej(9, -15)),
    }
    for name, (args, rej) in table.items():
        for i, v, code in rej:
            assert s.call(name, _swap(args(), i, v)) == code, (name, i, v, code)
    # the first bad argument in the list decides; bwd rejects a bad hyper-half argument before its latent half runs
    assert s.call("lvae_kl_closed_fwd_f32", _swap(_swap(s.a_fwd(), 12, None), 3, 0)) == -4
    assert s.call("lvae_kl_closed_bwd_f32", _swap(s.a_bwd(), 13, None)) == -14
    # the state queries
    p = P.ptr
    est, flag, one, two = U.sentinel(L), U.sentinel(L, torch.int32), U.sentinel(1, torch.int32), U.sentinel(1, torch.int32)
    st = P.stream_ptr()
    q = [("lvae_kl_closed_refine_state", [n, L, wsp, p(est), p(flag), st],
          [(0, 0, -1), (0, 16640, -1), (1, 0, -2), (2, None, -3), (2, wsp + 8, -3), (3, None, -4), (4, None, -5)]),
         ("lvae_kl_closed_hyper_state", [n, L, wsp, p(one), st], [(0, 0, -1), (1, 0, -2), (2, None, -3), (3, None, -4)]),
         ("lvae_kl_closed_resid_state", [n, L, wsp, p(one), p(two), st],
          [(0, 0, -1), (0, 16640, -1), (1, 0, -2), (2, None, -3), (2, wsp + 8, -3), (3, None, -4), (4, None, -5)])]
    for name, args, rej in q:
        for i, v, code in rej:
            assert getattr(hip, name)(*_swap(args, i, v)) == code, (name, i, v, code)
    # the host queries
    assert [hip.lvae_kl_closed_padded_n(k) for k in (1, 255, 256, 257, 16640)] == [256, 256, 256, 512, 16640]
    assert [int(hip.lvae_kl_closed_workspace_size(*a)) for a in ((0, 2), (-1, 2), (16385, 2), (16640, 2), (256, 0))] == [0] * 5
    assert int(hip.lvae_kl_closed_workspace_size(16384, 1)) > 3 * 16384 * 16384 * 4   # (64 blocks: the largest accepted)
    torch.cuda.synchronize()
    assert all(U.all_sentinel(t) for t in s.outputs() + [est, flag, one, two]), "a rejected call wrote an output"
    assert bool((s.ws == 0x7F).all()), "a rejected call wrote the workspace"
    s.forward()
    s.backward()
    check_values("255x2", s.results())


@gpu
def test_spd_inv_chol_return_codes(hip):
    """lvae_spd_inv_chol_f32's documented codes, np = 16640 (65 blocks) among them, on sentinel buffers nothing
    may touch (no large allocation: every rejection comes before any launch); then a 256 x 256 identity runs."""
    from lvae_amd import _lib as P
    p = P.ptr
    np_, L = 256, 1
    A, Ai = U.sentinel(np_ * np_, torch.float32), U.sentinel(np_ * np_, torch.float32)
    logdet, info = U.sentinel(L), U.sentinel(L, torch.int32)
    scr, tail = U.workspace(hip.lvae_spd_inv_chol_scratch_size(np_, L))
    sp = scr.data_ptr()
    args = [np_, L, p(A), sp, p(Ai), p(logdet), p(info), P.stream_ptr()]
    rej = [(2, None, -3), (3, None, -4), (3, sp + 8, -4), (3, sp + 128, -4), (4, None, -5), (5, None, -6),
           (6, None, -7), (0, 0, -1), (0, -256, -1), (0, 300, -1), (0, 16640, -1), (1, 0, -2), (1, -1, -2)]
    for i, v, code in rej:
        assert hip.lvae_spd_inv_chol_f32(*_swap(args, i, v)) == code, (i, v, code)
    assert hip.lvae_spd_inv_chol_f32(*_swap(_swap(args, 0, 16640), 2, None)) == -3   # (the pointers come first)
    torch.cuda.synchronize()
    assert all(U.all_sentinel(t) for t in (A, Ai, logdet, info)) and bool((scr == 0x7F).all())
    A.view(np_, np_).copy_(2.0 * torch.eye(np_, device=DEV))
    assert hip.lvae_spd_inv_chol_f32(*args) == 0
    torch.cuda.synchronize()
    assert U.tail_untouched(tail) and info.tolist() == [0]
    assert U.rel(Ai.view(np_, np_), 0.5 * torch.eye(np_)) < 8 * FLOOR
    assert abs(float(logdet[0]) - np_ * np.log(2.0)) < 1e-9
