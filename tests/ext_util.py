"""Shared inputs, oracles and yardsticks of the tests that take the periodic and linear factors (LVAE_PER, LVAE_LIN)
through every bound and predictor that reads a kernel spec (test_bounds_ext_cpu.py, test_gpu_bounds_ext_abi.py,
test_gpu_bounds_ext_drivers.py and the ext cases of the component and predict modules).

Spec pairs (ext_pairs): three (spec0, spec1) over abi_util.subject_covariates' columns, each spec with a bare per, a
bare lin, cat x per and a gate x lin; ext-a in bucket (8, 2) twice (the tabled adjoint), ext-b with a (16, 4) id
kernel, ext-c with a (16, 4) spec0 of nine components; the (16, 4) specs carry a three-factor product of per with
rbf or lin.  ext-a-pad is ext-a with spec1 padded to (16, 4) by one three-factor component whose scale is exactly 0.

Inputs per (case P x T x M, pair, time variant): L = 3, covariates abi_util.subject_covariates, inducing rows
abi_util.inducing_points, hyper-parameters and noise abi_util.draw_hypers (uniform in [0.5, 2], distinct per latent
dim), eps = 1e-3.  Variant `real` keeps column 0 as abi_util makes it (half-integer steps plus an offset below the
step) but draws the offset per row, not per subject: with one offset per subject the distances inside a subject are
the exact integers 1, 2, .., table hits, and `real` is the variant in which every off-diagonal distance misses the
tables.  `int` codes column 0 in integers: rows walk
T0 = [0, 1, 2, 64, 65, 66, 200] from a per-subject offset and the inducing times are distinct integers of 0..200, so
that the adjoint's integer tables (64 entries) are hit, hit at their last entry and missed.

Yardstick (a): the relative change of each oracle quantity when every continuous input (hyper-parameters, noise, mu,
logv / y, m, H and, in the `real` variant, covariate columns 0, 1 and 6 of x and z) is perturbed by a relative 2^-50
of random sign, fixed seed.  Id, category and flag columns are never perturbed (that flips a gate)."""
import contextlib
import functools

import numpy as np
import torch

import abi_util as U
from oracle import lvae_oracle as O

L = 3
EPS = 1e-3
S = 2                                    # samples of the sampled ELBO
T0 = np.array([0.0, 1.0, 2.0, 64.0, 65.0, 66.0, 200.0])
TAB = 64                                 # kGTab of csrc/gram.hip (the generic Grams): integer distances below are hits
CONT_COLS = [0, 1, 6]
COT = (1.0, -0.5, 2.0)

_A0 = [[("rbf", 0)], [("per", 0)], [("lin", 1)], [("cat", 3), ("per", 0)], [("bin", 5), ("lin", 6)]]
_A1 = [[("cat", 2)], [("cat", 2), ("per", 0)], [("cat", 2), ("lin", 6)], [("cat", 2), ("rbf", 0)]]
_B1 = [[("cat", 2)], [("cat", 2), ("per", 0), ("bin", 7)], [("cat", 2), ("lin", 1), ("rbf", 0)],
       [("cat", 2), ("rbf", 6), ("per", 0)]]
_C0 = [[("rbf", 0)], [("rbf", 1)], [("per", 0)], [("lin", 6)], [("cat", 3)], [("cat", 3), ("per", 0), ("rbf", 1)],
       [("bin", 5), ("lin", 1), ("per", 0)], [("cat", 4), ("rbf", 0)], [("per", 6), ("bin", 7)]]
PAD = [("cat", 2), ("rbf", 0), ("bin", 7)]   # the zero-scale component of ext-a-pad


def ext_pairs():
    """{name: (spec0, spec1)}; every component of spec1 carries ("cat", 2), bin sits on columns 5 and 7 only"""
    return {"ext-a": (_A0, _A1), "ext-b": (_A0, _B1), "ext-c": (_C0, _A1)}


PAIRS = ext_pairs()


def all_spec_pairs():
    """abi_util.spec_pairs() and the three extension pairs under one lookup (the predictors' case tables)"""
    return {**U.spec_pairs(), **ext_pairs()}


ALL_PAIRS = dict(PAIRS, **{"ext-a-pad": (_A0, _A1 + [PAD])})

# id: (P, T, M)
CASES = {
    "3x1x1": (3, 1, 1),
    "6x7x33": (6, 7, 33),       # odd sizes, the x-z Gram past one 1024-element adjoint chunk
    "17x3x9": (17, 3, 9),       # a second workgroup of one subject
    "3x33x17": (3, 33, 17),     # T > 32: the batched-product route
    "9x16x40": (9, 16, 40),
}
FULL_CROSS = ["6x7x33", "9x16x40"]
DIAGONAL = [("ext-a", "int"), ("ext-b", "real"), ("ext-c", "int")]
SELECTED = [(cid, pair, var) for cid in CASES
            for pair, var in ([(p, v) for p in PAIRS for v in ("real", "int")] if cid in FULL_CROSS else DIAGONAL)]
SELECTED_IDS = ["-".join(k) for k in SELECTED]
# the module route (test_gpu_bounds_ext_drivers.py): both buckets of spec0, both time variants, both T routes
DRIVER_KEYS = [(cid, pair, var) for pair in ("ext-a", "ext-c") for cid, var in (("6x7x33", "int"), ("3x33x17", "real"))]
# the ragged inputs of the _seg_ and conditioned calls: id: (P, T_max, seg, M, free subjects)
SEG_CASES = {
    "5x7r": (5, 7, (7, 1, 4, 7, 2), 9, (1, 3)),      # a one-row subject (free), full and short ones
    "3x33r": (3, 33, (33, 1, 17), 17, (2,)),         # a segment longer than 32
}
SEG_SELECTED = [(cid, pair, var) for cid in SEG_CASES for pair, var in (("ext-a", "int"), ("ext-c", "real"))]
SEG_IDS = ["-".join(k) for k in SEG_SELECTED]


def _sym(A):
    return 0.5 * (A + A.transpose(-1, -2))


def _seed(*key):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate("/".join(str(k) for k in key))) % 100003


@functools.lru_cache(maxsize=None)
def problem(cid, pair, var):
    """One problem: a uniform case of CASES or a ragged one of SEG_CASES (then X, mu, lv, ys hold the valid rows
    only, varying_util's convention, and Xfull / valid / seg / free describe the padded layout)."""
    if cid in CASES:
        (P, T, M), seg, free = CASES[cid], None, None
    else:
        P, T, seg, M, free = SEG_CASES[cid]
    s0, s1 = ALL_PAIRS[pair]
    seed = _seed(cid, pair.replace("-pad", ""), var)
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    xs = U.subject_covariates(rng, P, T)
    z = U.inducing_points(rng, L, M, T)
    if var == "real":   # (one offset per subject leaves in-subject distances 1, 2, ..: exact integers, table hits)
        xs[..., 0] = torch.tensor(0.5 * np.arange(T)[None, :] + rng.uniform(0.0, 0.5, (P, T)))
    else:
        xs[..., 0] = torch.tensor(T0[(np.arange(T)[None, :] + np.arange(P)[:, None]) % 7])
        z[..., 0] = torch.tensor(np.stack([rng.choice(201, M, replace=False) for _ in range(L)]).astype(np.float64))
    Xfull = xs.reshape(P * T, U.QC)
    valid = torch.ones(P * T, dtype=torch.bool)
    if seg is not None:
        valid = (torch.arange(T)[None, :] < torch.tensor(seg)[:, None]).reshape(-1)
    N = int(valid.sum())
    base0, base1 = PAIRS[pair.replace("-pad", "")]
    p0 = U.draw_hypers(rng, L, O.n_params(base0))
    p1 = U.draw_hypers(rng, L, O.n_params(base1))
    if pair.endswith("-pad"):   # scale exactly 0, a lengthscale of its own
        p1 = torch.cat([p1, torch.zeros(L, 1, dtype=torch.float64), torch.tensor([[1.25], [0.75], [1.5]])], 1)
    noise = U.draw_hypers(rng, L, None)
    # m and H in the range of K0zz (m = K w, H = K / 2 + K A A^T K / (100 M)): a random m has m^T K^-1 m ~ M / eps,
    # which the rbf and periodic parameters move 10^5 times more than a linear component's scale
    Kz = O.gram(s0, p0, z, z) + EPS * torch.eye(M, dtype=torch.float64)
    Xh = torch.randn(L, M, M, generator=gen, dtype=torch.float64)
    mu = torch.randn(N, L, generator=gen, dtype=torch.float64)
    c = dict(cid=cid, pair=pair, var=var, P=P, T=T, M=M, N=N, L=L, eps=EPS, s0=s0, s1=s1, X=Xfull[valid], Xfull=Xfull,
             valid=valid, seg=seg, Z=z, p0=p0, p1=p1, noise=noise, mu=mu,
             lv=0.1 * torch.randn(N, L, generator=gen, dtype=torch.float64),
             m=Kz @ (0.3 * torch.randn(L, M, 1, generator=gen, dtype=torch.float64)),
             H=_sym(0.5 * Kz + Kz @ Xh @ Xh.transpose(1, 2) @ Kz / (100.0 * M)),
             ys=mu[None] + 0.3 * torch.randn(S, N, L, generator=gen, dtype=torch.float64),
             g=torch.randn(S, L, generator=gen, dtype=torch.float64),
             perturb_cols=CONT_COLS if var == "real" else [])
    if free is not None:
        c["free"] = free
        c["rows"] = torch.cat([torch.arange(p * T, (p + 1) * T) for p in free])
        c["Pn"], c["Nn"] = len(free), len(free) * T
    return c


def hits_and_misses(c):
    """(table hits, misses) among the column-0 distances the bounds' Grams evaluate off their diagonals: rows of one
    subject against each other, rows against the inducing rows, inducing rows against each other (per latent dim).
    A hit is an integer distance below TAB, as kernel_grad_acc_tab decides it."""
    t = c["X"][:, 0]
    sid = c["X"][:, U.ID_COL]
    d = []
    same = (sid[:, None] == sid[None, :]) & ~torch.eye(c["N"], dtype=torch.bool)
    d.append((t[:, None] - t[None, :]).abs()[same])
    for l in range(L):
        tz = c["Z"][l, :, 0]
        d.append((t[:, None] - tz[None, :]).abs().reshape(-1))
        d.append((tz[:, None] - tz[None, :]).abs()[~torch.eye(c["M"], dtype=torch.bool)])
    d = torch.cat(d)
    hit = (d < TAB) & (d == torch.floor(d))
    return d[hit], d[~hit]


# ------------------------------------------------------------------------------------------------------
# the oracles (CPU autograd, or the same formulas in torch fp64 on a device) and the yardsticks
# ------------------------------------------------------------------------------------------------------
FLOAT_INPUTS = ["p0", "p1", "noise", "mu", "lv", "ys", "m", "H"]


def float_inputs(c, perturb):
    """{name: tensor} of every continuous input, x and z included; perturb: times 1 + 2^-50 s, seed 77"""
    v = {k: c[k] for k in FLOAT_INPUTS}
    v["x"], v["z"] = c["X"], c["Z"]
    if perturb:
        gen = torch.Generator().manual_seed(77)
        v = {k: (U.perturbed(t, gen) if k not in ("x", "z") else t) for k, t in v.items()}
        v["H"] = 0.5 * (v["H"] + v["H"].transpose(1, 2))
        for k in ("x", "z"):
            t = v[k].clone()
            for q in c["perturb_cols"]:
                t[..., q] = U.perturbed(t[..., q], gen)
            v[k] = t
    return v


@contextlib.contextmanager
def _on(dev):
    """the oracle's own torch.eye / torch.zeros calls follow the default device"""
    if dev == "cpu":
        yield
    else:
        with torch.device(dev):
            yield


DUBO_QUANT = ["dubo", "dmu", "dlogv", "dp0", "dp1", "dnoise"]
ELBO_QUANT = ["elbo", "dy", "dp0", "dp1", "dnoise"]


def _leaves(v, dev, names):
    out = {k: t.detach().clone().to(dev) for k, t in v.items()}
    for k in names:
        out[k].requires_grad_()
    return out


def oracle_dubo(c, perturb=False, dev="cpu", cot=None):
    """O.deviance_upper_bound per dim (uniform problems) or varying_util.loop_dubo (ragged ones), gradients of
    sum_l cot_l dubo_l with respect to the positive hyper-parameters, the noise, mu and logv"""
    import varying_util as V
    v = _leaves(float_inputs(c, perturb), dev, ["p0", "p1", "noise", "mu", "lv"])
    with _on(dev):
        if c["seg"] is None:
            f = lambda l: O.deviance_upper_bound(c["s0"], v["p0"][l], c["s1"], v["p1"][l], v["noise"][l], v["x"],
                                                 v["mu"][:, l], v["lv"][:, l], v["z"][l], c["P"], c["T"], c["eps"])
        else:
            f = lambda l: V.loop_dubo(c["s0"], v["p0"][l], c["s1"], v["p1"][l], v["noise"][l], v["x"], v["mu"][:, l],
                                      v["lv"][:, l], v["z"][l], U.ID_COL, c["eps"])
        vals = torch.stack([f(l) for l in range(L)])
        vals.backward(torch.as_tensor(COT if cot is None else cot, dtype=torch.float64, device=dev))
    out = dict(dubo=vals, dmu=v["mu"].grad, dlogv=v["lv"].grad, dp0=v["p0"].grad, dp1=v["p1"].grad,
               dnoise=v["noise"].grad)
    return {k: t.detach().cpu() for k, t in out.items()}


def oracle_elbo(c, perturb=False, dev="cpu"):
    """O.gpapprox_elbo per (sample, dim) (or varying_util.loop_elbo), gradients of sum g[s][l] elbo[s][l]"""
    import varying_util as V
    v = _leaves(float_inputs(c, perturb), dev, ["p0", "p1", "noise", "ys"])
    with _on(dev):
        if c["seg"] is None:
            f = lambda s, l: O.gpapprox_elbo(c["s0"], v["p0"][l], c["s1"], v["p1"][l], v["noise"][l], v["x"],
                                             v["ys"][s, :, l], v["z"][l], c["P"], c["T"], c["eps"])
        else:
            f = lambda s, l: V.loop_elbo(c["s0"], v["p0"][l], c["s1"], v["p1"][l], v["noise"][l], v["x"],
                                         v["ys"][s, :, l], v["z"][l], U.ID_COL, c["eps"])
        vals = torch.stack([torch.stack([f(s, l) for l in range(L)]) for s in range(S)])
        vals.backward(c["g"].to(dev))
    out = dict(elbo=vals, dy=v["ys"].grad, dp0=v["p0"].grad, dp1=v["p1"].grad, dnoise=v["noise"].grad)
    return {k: t.detach().cpu() for k, t in out.items()}


def hensman_problem(c):
    """the problem in test_gpu_hensman_abi's keys (a uniform case: P_b = P subjects, P_tot = 4 P + 3)"""
    assert c["seg"] is None
    return dict(cid="-".join((c["cid"], c["pair"], c["var"])), s0=c["s0"], s1=c["s1"], L=L, M=c["M"], T=c["T"],
                P_b=c["P"], seg=None, eps=c["eps"], B=c["N"], P_tot=float(4 * c["P"] + 3), x=c["X"], z=c["Z"],
                p0=c["p0"], p1=c["p1"], noise=c["noise"], m=c["m"], H=c["H"], mu=c["mu"], logv=c["lv"],
                valid=c["valid"], n_total=0.0, P_call=float(4 * c["P"] + 3), perturb_cols=c["perturb_cols"])


def oracle_hensman(c, perturb=False, dev="cpu"):
    import test_gpu_hensman_abi as TH
    return TH.oracle(hensman_problem(c), dev, perturb)


ORACLES = dict(dubo=oracle_dubo, elbo=oracle_elbo, hensman=oracle_hensman)


def slots(q):
    """the quantities + one entry "dp0:j" / "dp1:j" per parameter slot (the column [L] of that slot over the latent
    dims).  The gradients of one kernel spread over up to seven decades (a period's derivative grows with the
    distances, up to 200 in the `int` variant; a linear component's scale sits far below it), so a slot that is wrong
    by its whole size can hide under abi_util.rel of the whole matrix.  Each slot is therefore also compared on its
    own, relative to the slot's own largest entry, by the same rule on the slot's own yardstick (bound).  The CPU
    module holds every slot's largest entry to SLOT_FLOOR of its matrix's."""
    out = dict(q)
    for k in ("dp0", "dp1"):
        if k in q:
            out.update({f"{k}:{j}": q[k][:, j] for j in range(q[k].shape[1])})
    return out


@functools.lru_cache(maxsize=None)
def cpu_ref(kind, cid, pair, var):
    """(oracle, yardstick (a) per quantity and parameter slot) of one bound on the CPU, computed once"""
    c = problem(cid, pair, var)
    ref, per = slots(ORACLES[kind](c)), slots(ORACLES[kind](c, perturb=True))
    return ref, {k: U.rel(per[k], ref[k]) for k in ref}


@functools.lru_cache(maxsize=None)
def yardstick(kind, cid, pair, var):
    """max((a) perturbation, (b) the spread between the CPU oracle and the same formula in torch fp64 on the GPU)"""
    ref, ya = cpu_ref(kind, cid, pair, var)
    dev = slots(ORACLES[kind](problem(cid, pair, var), dev=U.DEV))
    return {k: max(ya[k], U.rel(dev[k], ref[k])) for k in ref}


# The smallest a parameter slot's largest entry may be, relative to its matrix's largest entry (asserted on the CPU).
# Rounding that a slot shares with the large slots of its matrix is at most the whole matrix's yardstick, held below
# 1e-9 on the CPU, times matrix / slot: with this floor at most 1e-4 of the slot, the looser of the project's caps,
# so a slot that is swapped, dropped, misindexed or off by a thousandth of itself stands out of it.
SLOT_FLOOR = 1e-5


def caps():
    """test_gpu_hensman_abi.CAPS with the two values of the other bounds; every other quantity: 1e-6"""
    import test_gpu_hensman_abi as TH
    return dict(TH.CAPS, dubo=1e-8, elbo=1e-8)


def bound(key, yard):
    """the project's rule, for a quantity and for a single parameter slot alike (yard: its own yardstick):
    max(10 x yardstick, 2e-12), never looser than the caps"""
    return min(max(10.0 * yard, 2e-12), caps().get(key.split(":")[0], 1e-6))


def check(what, got, want, yard, keys):
    """got[k] within bound(k) of want[k] (abi_util.rel) for every quantity of keys and every parameter slot of
    dp0 / dp1 among them; prints error, yardstick and bound before it asserts"""
    got, want = slots({k: got[k] for k in keys}), slots({k: want[k] for k in keys})
    missed = []
    for k in got:
        err, tol = U.rel(got[k].reshape(want[k].shape), want[k]), bound(k, yard[k])
        print(f"{what} {k}: err {err:.2e} yardstick {yard[k]:.2e} ratio {err / max(yard[k], 1e-300):.2g} "
              f"bound {tol:.1e} err/bound {err / tol:.3f}")
        if not err <= tol:
            missed.append((what, k, err, tol))
    assert not missed, missed
