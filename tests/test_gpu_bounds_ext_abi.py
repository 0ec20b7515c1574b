"""The three inducing-point bounds through the C ABI on kernel specs with periodic and linear factors, against the
fp64 oracle on the CPU: lvae_dubo_fwd/bwd_f64, lvae_gp_elbo_fwd/bwd_f64, lvae_hensman_fwd/bwd_f64 on ext_util's
selected (case, pair, time variant) problems, the two _seg_ pairs and lvae_dubo_cond_prepare_f64 + _eval_f64 on its
ragged ones.  The calls are the shared runners' (dubo_util.abi_run, gp_elbo_util.abi_run, varying_util.abi_dubo /
abi_elbo, dubo_cond_util.prepare / evaluate, test_gpu_hensman_abi.run), given ext_util's problems whole: NaN-filled
outputs with spare sentinels behind them, sentinel-tailed workspaces.

Under every call sit gram_multi_f64 / gram_bwd_multi_f64 with two DevSpecs in the larger bucket of the pair: ext-a
runs the (8, 2) build (kernel_grad_acc_tab: the `int` variant hits and misses its tables, `real` misses them all),
ext-b, ext-c and ext-a-pad the (16, 4) build (kernel_grad_acc), with 2-parameter periodic and 0-parameter linear
factors in both specs.

Tolerances: the project's rule, per case and quantity max(10 x yardstick, 2e-12), never looser than the caps of
test_gpu_hensman_abi (1e-8 values, 1e-4 dparams1 / dnoise, 1e-6 the rest); the yardstick is the larger of (a) the
change of the oracle under a 2^-50 perturbation of every continuous input and (b) the spread between the oracle on
the CPU and the same formula in torch fp64 on the device.  dparams0 / dparams1 are held to it as whole matrices and
slot by slot, each slot by the same rule on its own yardstick and relative to its own largest entry (ext_util.slots;
test_bounds_ext_cpu.py holds every slot's largest entry to 1e-5 of its matrix's).  ext-a-pad (a zero-scale component
that moves spec1 to bucket (16, 4)) must agree with ext-a within the same bound in everything they share: the tabled
and the direct adjoint on identical data.

Measured on the MI355X (per group of tests the quantity, then the single slot, closest to its bound; yardstick =
max((a), (b))):
    calls                 case                    quantity   kernel err   yardstick   bound     err / bound
    dubo                  9x16x40 ext-a real      dmu        1.01e-12     1.40e-13    2.0e-12   0.51
    dubo                  9x16x40 ext-b real      dparams0:4 1.84e-11     4.06e-12    4.1e-11   0.45
    gp_elbo               6x7x33 ext-a real       dy         1.38e-12     2.24e-13    2.2e-12   0.62
    gp_elbo               9x16x40 ext-a real      dparams1:3 3.54e-12     6.86e-13    6.9e-12   0.52
    hensman (ng 1 and 0)  6x7x33 ext-a real       kld        5.43e-13     7.49e-14    2.0e-12   0.27
    hensman (ng 1 and 0)  9x16x40 ext-b real      dparams1:0 1.37e-12     1.26e-13    2.0e-12   0.68
    dubo_seg              3x33r ext-a int         dparams0:8 3.21e-13     8.51e-13    8.5e-12   0.04
    gp_elbo_seg           3x33r ext-c real        dparams1:0 1.09e-13     5.69e-14    2.0e-12   0.05
    dubo_cond             5x7r ext-a int          dm         4.79e-15     9.52e-14    2.0e-12   0.002
    ext-a-pad, own oracle 9x16x40 real            dmu        1.01e-12     1.92e-13    2.0e-12   0.51   (dubo)
    ext-a-pad / ext-a     both cases              all        0            -           2.0e-12   0      (the same bits)
The caps never decided.  This module and test_gpu_bounds_ext_drivers.py take about 11 s together (117 tests; the
first call 2 s, every other under 0.6 s).

What these tests found, all of it where cond(Kz) is ~5e4 (ext-a's spec0 on real times) and all of it fixed in the
kernels' host code.  A 60-digit evaluation of the DUBO (central differences in the period) put the oracle within
1.4e-11 of the truth; the backwards' formulas replayed in fp64 on the CPU, with every inverse refined to its last
bit, showed the kernels' errors, and taking one product at a time in extended precision named the product.
  * DUBO and ELBO, dparams0's period slots 13 to 19 times the whole-matrix yardstick off (2.87e-10, 3.61e-10,
    7.11e-11): dKz's term iK Q iK formed as (iK Q) iK.  Its rounding is that of iK Q times |iK| ~ 1 / eps, and
    d Kz / d period, which oscillates over the inducing times, does not average it out as the smoother derivatives
    do.  Now (X iK)^T (iBK iK), as the z-adjoint already formed it: 3.22e-11, 5.52e-11, 6.01e-12.
  * DUBO, the period slot alone 17 times its own yardstick off (1.9e-9 at 9x16x40 ext-a real): (iW R) iW, the same
    shape.  Now U^T (D U), U = iBK iW: 1.84e-11 at the worst slot.
  * Hensman, dparams0 at 0.94 of its bound (2.27e-10 at 6x7x33 ext-a real) and its period slot 2.2 times over
    (1.43e-10): (iK G_iK) iK.  Now term by term from B x M factors (hensman.hip): 8.50e-12 and 2.08e-11.
  * Hensman, the id kernel's scale (dparams1:0) 5.59e-12 against a yardstick of 1.26e-13 (bound 2.0e-12): t = iK m
    carried iK's forward error into the residual.  Now one refinement step with a double-double residual: 1.37e-12.
"""
import functools

import pytest
import torch

import abi_util as U
import dubo_cond_util as C
import dubo_util as D
import ext_util as E
import gp_elbo_util as G
import test_gpu_hensman_abi as TH
import varying_util as V

pytestmark = pytest.mark.gpu
L = E.L
ids = lambda keys: ["-".join(k) for k in keys]
PAD_KEYS = [("6x7x33", "ext-a", "int"), ("9x16x40", "ext-a", "real")]


def _tails_clean(o, n):
    return all(U.all_sentinel(o[k][n[k]:]) for k in o)


def run_dubo(hip, key):
    out, info, o, n = D.abi_run(hip, E.problem(*key), cot=E.COT)
    assert info[:L].tolist() == [0] * L and U.all_sentinel(info[L:].to(U.DEV)) and _tails_clean(o, n)
    return out


def run_elbo(hip, key):
    out, info, o, n = G.abi_run(hip, E.problem(*key), E.S)
    assert info[:L].tolist() == [0] * L and U.all_sentinel(info[L:].to(U.DEV)) and _tails_clean(o, n)
    return out


def run_hensman(hip, key, ng):
    got, info, iH = TH.run(hip, E.hensman_problem(E.problem(*key)), ng)
    assert info.tolist() == [0] * L
    return dict(got, iH=iH)


@pytest.mark.parametrize("key", E.SELECTED, ids=E.SELECTED_IDS)
def test_dubo(hip, key):
    """lvae_dubo_fwd_f64 + lvae_dubo_bwd_f64 (cotangents 1, -0.5, 2): values and every gradient against the oracle"""
    E.check("dubo " + "-".join(key), run_dubo(hip, key), E.cpu_ref("dubo", *key)[0], E.yardstick("dubo", *key),
            E.DUBO_QUANT)


@pytest.mark.parametrize("key", E.SELECTED, ids=E.SELECTED_IDS)
def test_gp_elbo(hip, key):
    """lvae_gp_elbo_fwd_f64 + lvae_gp_elbo_bwd_f64 on 2 samples with random cotangents"""
    E.check("elbo " + "-".join(key), run_elbo(hip, key), E.cpu_ref("elbo", *key)[0], E.yardstick("elbo", *key),
            E.ELBO_QUANT)


@pytest.mark.parametrize("ng", [1, 0])
@pytest.mark.parametrize("key", E.SELECTED, ids=E.SELECTED_IDS)
def test_hensman(hip, key, ng):
    """lvae_hensman_fwd_f64 + lvae_hensman_bwd_f64: kld, the natural-gradient directions or dm / dH, the data and
    hyper-parameter gradients and the H^-1 left in the workspace"""
    E.check(f"hensman ng={ng} " + "-".join(key), run_hensman(hip, key, ng), E.cpu_ref("hensman", *key)[0],
            E.yardstick("hensman", *key), TH.active(ng) + ["iH"])


# ------------------------------------------------------------------------------------------------------
# the ragged inputs: the _seg_ calls and the conditioned DUBO
# ------------------------------------------------------------------------------------------------------
def _valid_rows(c, got, names):
    """the logical rows of the padded outputs; their padding rows must be exact zeros"""
    out = dict(got)
    for k in names:
        rows = got[k][..., c["valid"], :]
        assert bool((got[k][..., ~c["valid"], :] == 0).all()), k
        out[k] = rows
    return out


@pytest.mark.parametrize("key", E.SEG_SELECTED, ids=E.SEG_IDS)
def test_dubo_seg(hip, key):
    """lvae_dubo_fwd_seg_f64 + lvae_dubo_bwd_seg_f64 (NaN in the padding rows, another subject's covariates in x's)
    against varying_util.loop_dubo on the valid rows"""
    c = E.problem(*key)
    got = V.abi_dubo(hip, c, dirty=True)
    assert got["info"].tolist() == [0] * L
    E.check("dubo_seg " + "-".join(key), _valid_rows(c, got, ["dmu", "dlogv"]), E.cpu_ref("dubo", *key)[0],
            E.yardstick("dubo", *key), E.DUBO_QUANT)


@pytest.mark.parametrize("key", E.SEG_SELECTED, ids=E.SEG_IDS)
def test_gp_elbo_seg(hip, key):
    c = E.problem(*key)
    got = V.abi_elbo(hip, c, dirty=True)
    assert got["info"].tolist() == [0] * L
    E.check("elbo_seg " + "-".join(key), _valid_rows(c, got, ["dy"]), E.cpu_ref("elbo", *key)[0],
            E.yardstick("elbo", *key), E.ELBO_QUANT)


def cond_problem(c):
    """the ragged problem in the conditioned DUBO's padded layout: x, mu, logv [P T, .] (zeros in the padding)"""
    p = V.padded_inputs(c, dirty=False)
    return dict(c, X=p["x"], mu=p["mu"], lv=p["lv"], N=c["P"] * c["T"])


def cond_oracle(c, perturb=False, dev="cpu"):
    """the joint loop-form DUBO on the valid rows with the free subjects' rows replaced by the point
    (m, logv) = (mu + 3, logv - 3) there, differentiated with respect to the point alone (cotangents ext_util.COT)"""
    v = {k: t.to(dev) for k, t in E.float_inputs(c, perturb).items()}
    pos = torch.full((c["P"] * c["T"],), -1, dtype=torch.long)
    pos[c["valid"]] = torch.arange(c["N"])
    rows = pos[c["rows"]]
    rows = rows[rows >= 0].to(dev)
    m, lv = (v["mu"][rows] + 3.0).requires_grad_(), (v["lv"][rows] - 3.0).requires_grad_()
    mj, lj = v["mu"].index_copy(0, rows, m), v["lv"].index_copy(0, rows, lv)
    with E._on(dev):
        vals = torch.stack([V.loop_dubo(c["s0"], v["p0"][l], c["s1"], v["p1"][l], v["noise"][l], v["x"], mj[:, l],
                                        lj[:, l], v["z"][l], U.ID_COL, c["eps"]) for l in range(L)])
        gm, gl = torch.autograd.grad(vals, (m, lv), torch.tensor(E.COT, dtype=torch.float64, device=dev))
    return {k: t.detach().cpu() for k, t in dict(dubo=vals, dm=gm, dlogv=gl).items()}


@functools.lru_cache(maxsize=None)
def cond_ref(key):
    c = E.problem(*key)
    ref, per, dev = cond_oracle(c), cond_oracle(c, perturb=True), cond_oracle(c, dev=U.DEV)
    return ref, {k: max(U.rel(per[k], ref[k]), U.rel(dev[k], ref[k])) for k in ref}


def run_cond(hip, key):
    c = E.problem(*key)
    prep = C.prepare(hip, cond_problem(c), seg=c["seg"])
    assert prep["info"].tolist() == [0] * L
    vfree = c["valid"][c["rows"]]
    m = torch.zeros(c["Nn"], L, dtype=torch.float64)
    lv = torch.zeros(c["Nn"], L, dtype=torch.float64)
    pos = torch.cumsum(c["valid"].long(), 0) - 1
    m[vfree] = c["mu"][pos[c["rows"]][vfree]] + 3.0
    lv[vfree] = c["lv"][pos[c["rows"]][vfree]] - 3.0
    got = C.evaluate(hip, prep, m, lv, E.COT)
    for k in ("dm", "dlogv"):
        assert bool((got[k][~vfree] == 0).all()), k
    return dict(dubo=got["dubo"], dm=got["dm"][vfree], dlogv=got["dlogv"][vfree]), prep


@pytest.mark.parametrize("key", E.SEG_SELECTED, ids=E.SEG_IDS)
def test_dubo_cond(hip, key):
    """lvae_dubo_cond_prepare_f64 (with seg_len) + lvae_dubo_cond_eval_f64 at a point away from the encoder's"""
    got, _ = run_cond(hip, key)
    ref, yard = cond_ref(key)
    E.check("dubo_cond " + "-".join(key), got, ref, yard, ["dubo", "dm", "dlogv"])


# ------------------------------------------------------------------------------------------------------
# a fixed summation order; the tabled and the direct adjoint on the same data
# ------------------------------------------------------------------------------------------------------
def test_bit_reproducible(hip):
    """every bound called twice on one problem: the same bits (the header's fixed summation order)"""
    key, seg_key = ("6x7x33", "ext-b", "int"), ("5x7r", "ext-a", "int")
    for run, keys in ((run_dubo, E.DUBO_QUANT), (run_elbo, E.ELBO_QUANT)):
        a, b = run(hip, key), run(hip, key)
        assert all(U.bit_equal(a[k], b[k]) for k in keys), run.__name__
    for ng in (1, 0):
        a, b = run_hensman(hip, key, ng), run_hensman(hip, key, ng)
        assert all(U.bit_equal(a[k], b[k]) for k in TH.active(ng) + ["iH"]), ng
    c = E.problem(*seg_key)
    for run, keys in ((V.abi_dubo, E.DUBO_QUANT), (V.abi_elbo, E.ELBO_QUANT)):
        a, b = run(hip, c, dirty=True), run(hip, c, dirty=True)
        assert all(U.bit_equal(a[k], b[k]) for k in keys), run.__name__
    (a, pa), (b, pb) = run_cond(hip, seg_key), run_cond(hip, seg_key)
    n = int(hip.lvae_dubo_cond_state_size(L, pa["Pn"], pa["T"]))
    assert U.bit_equal(pa["state"][:n], pb["state"][:n]) and all(U.bit_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("key", PAD_KEYS, ids=ids(PAD_KEYS))
def test_zero_scale_padding_to_the_large_bucket(hip, key):
    """ext-a-pad = ext-a + one zero-scale three-factor component in spec1: the pair runs in bucket (16, 4) (the direct
    adjoint) instead of (8, 2) (the tabled one).  Each agrees with its own oracle, the padded scale's gradient
    included, and they agree with each other in every value and shared gradient within ext-a's bound."""
    pad = (key[0], "ext-a-pad", key[2])
    n1 = E.problem(*key)["p1"].shape[1]
    runs = [("dubo", run_dubo, E.DUBO_QUANT), ("elbo", run_elbo, E.ELBO_QUANT),
            ("hensman", lambda h, k: run_hensman(h, k, 1), TH.active(1)),
            ("hensman", lambda h, k: run_hensman(h, k, 0), TH.active(0))]
    for kind, run, keys in runs:
        plain, padded = run(hip, key), run(hip, pad)
        ref_pad, yard = E.cpu_ref(kind, *pad)[0], E.yardstick(kind, *key)
        E.check(f"pad {kind} own oracle " + "-".join(pad), padded, ref_pad, E.yardstick(kind, *pad), keys)
        assert bool((ref_pad["dp1"][:, n1] != 0).all())
        shared = dict(padded, dp1=padded["dp1"][:, :n1])
        E.check(f"pad {kind} against ext-a " + "-".join(key), shared, plain, yard, keys)
