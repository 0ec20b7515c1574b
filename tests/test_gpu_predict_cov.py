"""The joint predictive covariance of both latent predictors (return_cov=True; lvae_predict_cov_f64,
lvae_predict_exact_cov_f64), the trajectory draws (sample_trajectories; lvae_predict_sample_f64) and
generate_trajectories, against the dense fp64 oracle of test_predict_cov_oracle.py and tests/golden/predict_cov.npz.

Tolerance: the project's rule min(max(10 x yardstick, 2e-12), 1e-6) on max |got - ref| / max prior variance, applied
to whole blocks; the yardstick is the larger of the oracle's change under the relative 2^-50 perturbation of its
inputs and its CPU / device spread.  Every test prints error, yardstick and bound.  Everything else is bit for bit:
the mean beside the covariance, a repeated call, dim groups and test-row chunks under a workspace cap, the symmetry of
a block, its padding identity, the decoded images of generate_trajectories.

The golden fixture runs through the Python predictors (batched modules and per-dim lists); every case of
test_predict_cov_oracle.py (V.EXACT_CASES, V.IND_CASES, "group-128", "tiles-15-16-17") runs through the C ABI on
sentinel-filled buffers, as the variance's cases do in test_gpu_predict_var_abi.py.

V.IND_CASES holds the case ext-b (ext_util's pair ext-b: periodic and linear factors in both kernels, a (16, 4) id
kernel, ragged subjects, 37 test rows), so it runs here through lvae_predict_cov_f64 as it does through the variance
in test_gpu_predict_var_abi.py; test_gpu_predict_cov_abi.py takes its inducing-point inputs from this module
(ind_args) and holds the ABI's edges, not further values.  Measured on the MI355X: ext-b err 3.88e-15 against a
yardstick of 2.38e-15 and the bound 2.0e-12, in dim groups of 6, 6, 7, 6, 6, 6 blocks.
"""
import ctypes

import numpy as np
import pytest
import torch

import abi_util as U
import test_predict_cov_oracle as C
import test_predict_var_oracle as V
from conftest import golden
from test_gpu_predict_exact import kernels as exact_kernels, likelihoods as exact_likelihoods
from test_gpu_predict_var import exact_inputs, inducing_call, inducing_modules

gpu = pytest.mark.gpu
DEV = U.DEV


def rule(kind, cid):
    """(tolerance, yardstick, reference blocks, prior, groups) of a case"""
    _, prior, groups, blocks, ya = C.cpu_ref(kind, cid)
    if not groups:
        return 2e-12, ya, blocks, prior, groups
    on_device = C.ref_blocks(C.ORACLES[kind](cid, dev=DEV)[0], groups)
    yard = max(ya, C.block_err(on_device, blocks, prior))
    return min(max(10.0 * yard, 2e-12), 1e-6), yard, blocks, prior, groups


def check_blocks(what, blocks, kind, cid):
    """blocks [L, G, n_max, n_max] against the oracle under the rule; symmetric bit for bit, the identity on padding"""
    tol, yard, ref, prior, groups = rule(kind, cid)
    blocks = blocks.detach().cpu()
    assert blocks.shape == ref.shape and blocks.dtype == torch.float64
    err = C.block_err(blocks, ref, prior)
    print(f"{what}: err {err:.2e} yardstick {yard:.2e} bound {tol:.1e} groups {[len(g) for g in groups]}")
    assert bool(torch.isfinite(blocks).all()) and err <= tol
    assert U.bit_equal(blocks, blocks.transpose(2, 3).contiguous())
    pad = torch.ones(ref.shape[1:], dtype=torch.bool)
    for k, g in enumerate(groups):
        pad[k, :len(g), :len(g)] = False
    eye = torch.eye(ref.shape[2], dtype=torch.float64).expand(ref.shape)
    assert U.bit_equal(blocks[:, pad], eye[:, pad])
    return tol, yard


def check_index(cov, groups):
    assert cov.counts.tolist() == [len(g) for g in groups]
    for k, g in enumerate(groups):
        assert cov.index[k, :len(g)].cpu().tolist() == g.tolist() and bool((cov.index[k, len(g):] == -1).all())
    assert cov.index.dtype == torch.int32 and all(cov.block(k).shape[1:] == (len(g), len(g)) for k, g in enumerate(groups))


# ------------------------------------------------------------------------------------------------------
# the golden fixture through the Python predictors
# ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("batched", [False, True])
def test_predict_exact_covariance_matches_golden(hip, batched):
    import lvae_amd as la
    g, gv, (X, tx, mu) = exact_inputs()
    gc = golden("predict_cov.npz")
    k, L = exact_kernels(g, batched)
    lik = exact_likelihoods(g, batched)
    mean, cov = la.predict_exact(k, lik, X, tx, mu, return_cov=True, groups=tx[:, 2])
    _, prior, groups, ref, _ = C.cpu_ref("golden-exact", None)
    assert C.block_err(ref, C.ref_blocks(torch.tensor(gc["exact_cov"]), groups), prior) < 1e-12   # the fixture's blocks
    tol, _ = check_blocks(f"predict_exact cov batched={batched}", cov.blocks, "golden-exact", None)
    check_index(cov, groups)
    assert U.bit_equal(mean, la.predict_exact(k, lik, X, tx, mu))            # the mean beside it: the same bits
    m2, c2 = la.predict_exact(k, lik, X, tx, mu, return_cov=True, groups=tx[:, 2])
    assert U.bit_equal(m2, mean) and U.bit_equal(c2.blocks, cov.blocks)     # a repeated call: the same bits
    _, var = la.predict_exact(k, lik, X, tx, mu, return_var=True)
    derr = V.var_err(cov.diagonal(), var, prior)
    print(f"  diagonal against return_var: {derr:.2e}")
    assert derr <= tol and cov.diagonal().shape == (12, L)
    # groups=None: all 12 test rows form one group, the whole dense matrix
    m1, one = la.predict_exact(k, lik, X, tx, mu, return_cov=True)
    assert one.blocks.shape == (L, 1, 12, 12) and one.index.tolist() == [list(range(12))] and U.bit_equal(m1, mean)
    err = C.block_err(one.blocks[:, 0], torch.tensor(gc["exact_cov"]), prior)
    print(f"  one group of 12: err {err:.2e} bound {tol:.1e}")
    assert err <= tol
    _, cn = la.predict_exact(k, lik, X, tx, mu, return_cov=True, groups=tx[:, 2], add_noise=True)
    from test_gpu_predict_var import held_noise
    noisy = cov.blocks.cpu() + held_noise(lik, L).reshape(L, 1, 1, 1) * (C.ref_blocks(torch.zeros(L, 12, 12), groups) == 0) \
        * torch.eye(cov.blocks.shape[2], dtype=torch.float64)
    assert float((cn.blocks.cpu() - noisy).abs().max()) <= float(np.spacing(float(prior.max())))
    with pytest.raises(ValueError):
        la.predict_exact(k, lik, X, tx, mu, return_cov=True, return_var=True)


@gpu
def test_predict_exact_covariance_shuffled_rows_and_workspace_cap(hip):
    """Shuffled test rows permute index and blocks consistently (under the rule: exact symmetry stores one of the two
    products of a pair, so bit equality under permutation is too strong); a max_workspace_bytes that holds one dim
    and one group's chunk forces >= 2 dim groups and >= 2 test-row chunks: the same bits."""
    import lvae_amd as la
    g, gv, (X, tx, mu) = exact_inputs()
    k, L = exact_kernels(g, True)
    lik = exact_likelihoods(g, True)
    mean, cov = la.predict_exact(k, lik, X, tx, mu, return_cov=True, groups=tx[:, 2])
    tol, yard, ref, prior, groups = rule("golden-exact", None)
    perm = torch.randperm(12, generator=torch.Generator().manual_seed(3))
    mp, cp = la.predict_exact(k, lik, X, tx[perm.to(DEV)], mu, return_cov=True, groups=tx[perm.to(DEV), 2])
    assert U.bit_equal(mp, mean[perm.to(DEV)]) and cp.counts.tolist() == cov.counts.tolist()
    dense = torch.tensor(golden("predict_cov.npz")["exact_cov"])
    worst = 0.0
    for kk in range(len(groups)):
        rows = perm[cp.index[kk, :int(cp.counts[kk])].cpu().long()]       # the original rows of the permuted group
        assert sorted(rows.tolist()) == groups[kk].tolist()
        worst = max(worst, C.block_err(cp.block(kk), dense[:, rows][:, :, rows], prior))
    print(f"shuffled rows: err {worst:.2e} yardstick {yard:.2e} bound {tol:.1e}")
    assert worst <= tol
    n, nt, n_max = X.shape[0], 12, int(cov.counts.max())
    size = lambda dims, chunk: int(hip.lvae_predict_exact_cov_workspace_size(n, nt, dims, chunk))
    cap = size(1, 5)
    assert n_max == 4 and size(1, n_max) < cap < size(2, n_max) and cap < size(1, 6)   # one dim, one group a chunk
    mc, cc = la.predict_exact(k, lik, X, tx, mu, max_workspace_bytes=cap, return_cov=True, groups=tx[:, 2])
    assert U.bit_equal(mc, mean) and U.bit_equal(cc.blocks, cov.blocks)


@gpu
@pytest.mark.parametrize("batched", [False, True])
def test_batch_predict_covariance_matches_golden(hip, batched):
    gv, gc = golden("predict_var.npz"), golden("predict_cov.npz")
    mean, cov = inducing_call(gv, batched, return_cov=True)
    _, prior, groups, ref, _ = C.cpu_ref("golden-ind", None)
    assert C.block_err(ref, C.ref_blocks(torch.tensor(gc["ind_cov"]), groups), prior) < 1e-12
    tol, _ = check_blocks(f"batch_predict cov batched={batched}", cov.blocks, "golden-ind", None)
    check_index(cov, groups)
    assert U.bit_equal(mean, inducing_call(gv, batched))                    # the mean beside it: the same bits
    m2, c2 = inducing_call(gv, batched, return_cov=True)
    assert U.bit_equal(m2, mean) and U.bit_equal(c2.blocks, cov.blocks)     # a repeated call: the same bits
    _, var = inducing_call(gv, batched, return_var=True)
    derr = V.var_err(cov.diagonal(), var, prior)
    print(f"  diagonal against return_var: {derr:.2e}")
    assert derr <= tol and cov.diagonal().shape == (15, 3)
    with pytest.raises(ValueError):
        inducing_call(gv, batched, return_cov=True, return_var=True)


@gpu
def test_batch_predict_covariance_shuffled_rows(hip):
    gv = golden("predict_var.npz")
    mean, cov = inducing_call(gv, True, return_cov=True)
    tol, yard, ref, prior, groups = rule("golden-ind", None)
    perm = torch.randperm(15, generator=torch.Generator().manual_seed(4))
    mp, cp = inducing_call(gv, True, tidx=gv["ind_tidx"][perm.numpy()], return_cov=True)
    assert U.bit_equal(mp, mean[perm.to(DEV)]) and cp.counts.tolist() == cov.counts.tolist()
    dense = torch.tensor(golden("predict_cov.npz")["ind_cov"])
    worst = 0.0
    for kk in range(len(groups)):
        rows = perm[cp.index[kk, :int(cp.counts[kk])].cpu().long()]
        assert sorted(rows.tolist()) == groups[kk].tolist()
        worst = max(worst, C.block_err(cp.block(kk), dense[:, rows][:, :, rows], prior))
    print(f"shuffled rows: err {worst:.2e} yardstick {yard:.2e} bound {tol:.1e}")
    assert worst <= tol


# ------------------------------------------------------------------------------------------------------
# every case through the C ABI
# ------------------------------------------------------------------------------------------------------
def ind_args(cid, fill_seed=1):
    """Device tensors of an inducing-point case in the ABI's layout: padded x, test rows grouped by subject"""
    c = C.ind_problem(cid)
    other = U.subject_covariates(np.random.default_rng(fill_seed), c["P"], c["T"]).reshape(c["NP"], U.QC)
    x = torch.where(c["valid"][:, None], c["x"], other)   # padding rows of x: any finite covariates
    dv = lambda t: t.to(DEV).contiguous()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    starts = c["group_start"]
    return dict(x=dv(x), z=dv(c["z"]), mu=dv(c["mu_pad"]), tx=dv(c["tx"][c["order"]]), p0=dv(c["p0"]), p1=dv(c["p1"]),
                noise=dv(c["noise"]), seg=i32(c["seg"]), inc=dv(c["include"]), gsub=i32(c["group_subject"]),
                gstart=i32(starts), n_max=max([b - a for a, b in zip(starts, starts[1:])] + [1]))


def run_ind_cov(hip, cid, fill_seed=1, add_noise=0, want_mean=True):
    """One lvae_predict_cov_f64 call on sentinel buffers; (mean [Nt, L] in the caller's order or None, blocks) on
    the CPU"""
    from lvae_amd import _lib as P
    c = C.ind_problem(cid)
    L, M, Pn, T, Nt, G = c["L"], c["M"], c["P"], c["T"], c["Nt"], len(c["group_subject"])
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    a = ind_args(cid, fill_seed)
    n_max = a["n_max"]
    out, cov = U.sentinel(max(Nt, 1) * L + 7), U.sentinel(L * G * n_max * n_max + 7)
    info = U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_cov_workspace_size(L, M, Pn, T, Nt))
    rc = hip.lvae_predict_cov_f64(ctypes.byref(s0), ctypes.byref(s1), L, M, U.QC, Pn, T, P.ptr(a["seg"]), P.ptr(a["inc"]),
                                  P.ptr(a["x"]), P.ptr(a["mu"]) if want_mean else None, P.ptr(a["z"]), Nt,
                                  P.ptr(a["tx"]) if Nt else None, G, P.ptr(a["gsub"]), P.ptr(a["gstart"]), n_max,
                                  P.ptr(a["p0"]), P.ptr(a["p1"]), P.ptr(a["noise"]), V.EPS,
                                  P.ptr(out) if want_mean else None, P.ptr(cov), add_noise, P.ptr(info), P.ptr(ws),
                                  P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and U.tail_untouched(tail)
    nb = L * G * n_max * n_max if Nt else 0
    assert U.all_sentinel(cov[nb:]) and U.all_sentinel(out[Nt * L:] if want_mean else out)
    assert info.cpu().tolist() == [0] * L
    back = torch.empty(Nt, dtype=torch.int64)
    back[c["order"]] = torch.arange(Nt)
    mean = out[:Nt * L].reshape(Nt, L).cpu()[back] if want_mean else None
    return mean, cov[:nb].reshape(L, G, n_max, n_max).cpu() if Nt else torch.empty(L, 0, 1, 1, dtype=torch.float64)


@gpu
@pytest.mark.parametrize("cid", list(C.IND_CASES))
def test_inducing_cov_values(hip, cid):
    from test_gpu_predict_var_abi import ind_mean_only, run_ind
    c = C.ind_problem(cid)
    mean, blocks = run_ind_cov(hip, cid)
    m2, b2 = run_ind_cov(hip, cid, fill_seed=2)
    assert U.bit_equal(b2, blocks) and U.bit_equal(m2, mean)        # a repeated call, another padding fill: same bits
    none, b3 = run_ind_cov(hip, cid, want_mean=False)
    assert none is None and U.bit_equal(b3, blocks)                  # without the mean (mu NULL too)
    if c["Nt"] == 0:
        assert blocks.numel() == 0                                   # rc 0, info written, outputs untouched
        return
    tol, _ = check_blocks(f"inducing cov {cid}", blocks, "ind", cid)
    _, prior, groups, ref, _ = C.cpu_ref("ind", cid)
    if cid in V.IND_CASES:
        assert U.bit_equal(mean, ind_mean_only(hip, cid))            # the mean is lvae_predict_f64's
        _, var = run_ind(hip, cid)                                   # the existing variance
        diag = torch.empty_like(var)
        for k, g in enumerate(groups):
            diag[g] = torch.diagonal(blocks[:, k, :len(g), :len(g)], dim1=1, dim2=2).T
        derr = V.var_err(diag, var, prior)
        print(f"  diagonal against lvae_predict_var_f64: {derr:.2e}")
        assert derr <= tol
    _, bn = run_ind_cov(hip, cid, add_noise=1)
    real = C.ref_blocks(torch.zeros_like(C.cpu_ref("ind", cid)[0]), groups) == 0
    want = blocks + c["noise"].reshape(-1, 1, 1, 1) * real * torch.eye(blocks.shape[2], dtype=torch.float64)
    assert float((bn - want).abs().max()) <= float(np.spacing(float(prior.max())))   # + noise_l on the real diagonal


def run_exact_cov(hip, cid, chunk, pad=3, add_noise=0, want_mean=True):
    """One lvae_predict_exact_cov_f64 call on sentinel buffers, the test rows grouped by their id covariate;
    (mean [nt, L] in the caller's order or None, blocks, info list)"""
    from lvae_amd import _lib as P
    c = V.exact_problem(cid)
    L, n, nt = c["L"], c["n"], c["nt"]
    groups = C.case_groups("exact", cid)
    G, n_max = len(groups), max([len(g) for g in groups] + [1])
    order = torch.cat(groups) if groups else torch.zeros(0, dtype=torch.int64)
    start = (ctypes.c_int32 * (G + 1))(*np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(int).tolist())
    spec = P.make_spec(c["spec"])
    dv = lambda t: t.to(DEV).contiguous()
    ldx = U.QC + pad
    xb, _ = U.padded(c["x"], (ldx, 1))
    tb, _ = U.padded(c["tx"][order], (ldx, 1)) if nt else (None, None)
    mb, _ = U.padded(c["mu"], (L + pad, 1))
    params, nz = dv(c["params"]), dv(c["noise"])
    ld_out = L + pad
    out, cov = U.sentinel(max(nt, 1) * ld_out + 7), U.sentinel(L * G * n_max * n_max + 7)
    info = U.sentinel(L, torch.int32)
    ws, tail = U.workspace(hip.lvae_predict_exact_cov_workspace_size(n, nt, L, chunk))
    rc = hip.lvae_predict_exact_cov_f64(ctypes.byref(spec), P.ptr(xb), ldx, n, L, P.ptr(params), P.ptr(nz),
                                        P.ptr(mb) if want_mean else None, L + pad, P.ptr(tb) if nt else None, ldx, nt,
                                        G, ctypes.cast(start, ctypes.c_void_p), n_max,
                                        P.ptr(out) if want_mean else None, ld_out, P.ptr(cov), add_noise, chunk,
                                        P.ptr(info), P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and U.tail_untouched(tail)
    nb = L * G * n_max * n_max
    assert U.all_sentinel(cov[nb:])
    assert U.untouched_outside(out, (nt, L), (ld_out, 1)) if want_mean else U.all_sentinel(out)
    back = torch.empty(nt, dtype=torch.int64)
    back[order] = torch.arange(nt)
    mean = U.view(out, (nt, L), (ld_out, 1)).cpu()[back] if want_mean else None
    return mean, cov[:nb].reshape(L, G, n_max, n_max).cpu(), info.cpu().tolist()


@gpu
@pytest.mark.parametrize("cid", list(V.EXACT_CASES))
def test_exact_cov_values(hip, cid):
    from test_gpu_predict_var_abi import exact_mean_only, run_exact
    c = V.exact_problem(cid)
    groups = C.case_groups("exact", cid)
    n_max = max([len(g) for g in groups] + [1])
    chunks = sorted({n_max, min(2 * n_max + 1, max(c["nt"], 1)), max(c["nt"], 1)})   # one group, two, all
    runs = [run_exact_cov(hip, cid, ch) for ch in chunks]
    mean, blocks, info = runs[0]
    assert info == [0] * c["L"]
    for m2, b2, i2 in runs[1:]:
        assert U.bit_equal(b2, blocks) and U.bit_equal(m2, mean) and i2 == info    # the chunk changes no bit
    m3, b3, _ = run_exact_cov(hip, cid, chunks[-1], pad=0)
    assert U.bit_equal(b3, blocks) and U.bit_equal(m3, mean)        # a repeated call, other strides: the same bits
    none, b4, _ = run_exact_cov(hip, cid, chunks[-1], want_mean=False)
    assert none is None and U.bit_equal(b4, blocks)                  # without the mean (mu NULL too)
    if c["nt"] == 0:
        assert blocks.numel() == 0                                   # rc 0, info written, nothing else touched
        return
    assert U.bit_equal(mean, exact_mean_only(hip, cid))              # the mean is lvae_predict_exact_f64's
    tol, _ = check_blocks(f"exact cov {cid} chunks {chunks}", blocks, "exact", cid)
    _, prior = C.cpu_ref("exact", cid)[:2]
    _, var, _ = run_exact(hip, cid, c["chunks"][-1])                 # the existing variance
    diag = torch.empty_like(var)
    for k, g in enumerate(groups):
        diag[g] = torch.diagonal(blocks[:, k, :len(g), :len(g)], dim1=1, dim2=2).T
    derr = V.var_err(diag, var, prior)
    print(f"  diagonal against lvae_predict_exact_var_f64: {derr:.2e}")
    assert derr <= tol
    _, bn, _ = run_exact_cov(hip, cid, chunks[-1], add_noise=1)
    real = C.ref_blocks(torch.zeros_like(C.cpu_ref("exact", cid)[0]), groups) == 0
    want = blocks + c["noise"].reshape(-1, 1, 1, 1) * real * torch.eye(blocks.shape[2], dtype=torch.float64)
    assert float((bn - want).abs().max()) <= float(np.spacing(float(prior.max())))


@gpu
def test_group_above_the_cap_is_refused(hip):
    """A group of 129 rows: lvae_predict_cov_f64 and lvae_predict_exact_cov_f64 return -18 before any launch, the
    Python predictors raise ValueError naming the group."""
    import lvae_amd as la
    from lvae_amd import _lib as P
    c = C.ind_problem("over-cap")
    a = ind_args("over-cap")
    assert a["n_max"] == 129
    L, M, Pn, T, Nt = c["L"], c["M"], c["P"], c["T"], c["Nt"]
    s0, s1 = P.make_spec(c["s0"]), P.make_spec(c["s1"])
    out, cov, info = U.sentinel(Nt * L), U.sentinel(L * 129 * 129), U.sentinel(L, torch.int32)
    ws, _ = U.workspace(hip.lvae_predict_cov_workspace_size(L, M, Pn, T, Nt))
    rc = hip.lvae_predict_cov_f64(ctypes.byref(s0), ctypes.byref(s1), L, M, U.QC, Pn, T, P.ptr(a["seg"]), P.ptr(a["inc"]),
                                  P.ptr(a["x"]), P.ptr(a["mu"]), P.ptr(a["z"]), Nt, P.ptr(a["tx"]), 1, P.ptr(a["gsub"]),
                                  P.ptr(a["gstart"]), 129, P.ptr(a["p0"]), P.ptr(a["p1"]), P.ptr(a["noise"]), V.EPS,
                                  P.ptr(out), P.ptr(cov), 0, P.ptr(info), P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -18 and U.all_sentinel(out) and U.all_sentinel(cov) and U.all_sentinel(info) and bool((ws == 0x7F).all())
    g, gv, (X, tx, mu) = exact_inputs()
    k, _ = exact_kernels(g, True)
    big = tx[torch.arange(129, device=DEV) % 12]
    with pytest.raises(ValueError, match="group 0.*129"):
        la.predict_exact(k, exact_likelihoods(g, True), X, big, mu, return_cov=True)
    gvv = golden("predict_var.npz")
    sub2 = [int(i) for i in gvv["ind_tidx"] if gvv["ind_X_all"][i, 2] == 2.0]
    with pytest.raises(ValueError, match="label 2.*129"):
        inducing_call(gvv, True, tidx=np.array((sub2 * 33)[:129]), return_cov=True)


# ------------------------------------------------------------------------------------------------------
# draws
# ------------------------------------------------------------------------------------------------------
def abi_cov(hip, cid):
    """The PredictiveCovariance of an inducing-point case (blocks from the C ABI, index as the predictors build it)
    and a mean [Nt, L], on the device"""
    from lvae_amd.predict import PredictiveCovariance, _group_index, _row_groups
    c = C.ind_problem(cid)
    mean, blocks = run_ind_cov(hip, cid)
    order, _, counts, start, n_max = _row_groups(c["tx"][:, U.ID_COL], cid)
    return mean.to(DEV), PredictiveCovariance(blocks.to(DEV), _group_index(order, counts, start, n_max, DEV), counts)


def read_factor(cov, jitter):
    """Lc [L, G, n_max, n_max] read out of sample_trajectories with a zero mean and unit-vector eps: draw s holds, for
    every group, column s of its factor"""
    import lvae_amd as la
    L, G, n_max = cov.blocks.shape[:3]
    Nt = cov.num_rows
    eps = torch.zeros(n_max, Nt, L, dtype=torch.float64, device=DEV)
    for g in range(G):
        for s in range(int(cov.counts[g])):
            eps[s, int(cov.index[g, s]), :] = 1.0
    out = la.sample_trajectories(torch.zeros(Nt, L, dtype=torch.float64, device=DEV), cov, eps=eps, jitter=jitter)
    assert out.shape == (n_max, Nt, L) and out.dtype == torch.float64
    Lc = torch.zeros(L, G, n_max, n_max, dtype=torch.float64)
    for g in range(G):
        n = int(cov.counts[g])
        rows = cov.index[g, :n].long()
        Lc[:, g, :n, :n] = out[:n][:, rows].permute(2, 1, 0).cpu()      # [s, i, l] -> [l, i, s]
    return Lc


@gpu
@pytest.mark.parametrize("cid", ["tile-cross", "tiles-15-16-17"])
def test_draws_read_out_the_factor(hip, cid):
    """Lc is lower triangular with a positive diagonal and Lc Lc^T = Sigma_ref + jitter I under the rule (jitter 1e-6
    passed explicitly): the factor and the draw kernel without the conditioning of a Cholesky comparison."""
    jitter = 1e-6
    mean, cov = abi_cov(hip, cid)
    Lc = read_factor(cov, jitter)
    tol, yard, ref, prior, groups = rule("ind", cid)
    assert bool((torch.triu(Lc, 1) == 0).all())
    worst = 0.0
    for g, rows in enumerate(groups):
        n = len(rows)
        F = Lc[:, g, :n, :n]
        assert bool((torch.diagonal(F, dim1=1, dim2=2) > 0).all())
        want = ref[:, g, :n, :n] + jitter * torch.eye(n, dtype=torch.float64)
        worst = max(worst, C.block_err(F @ F.transpose(1, 2), want, prior))
    print(f"draws {cid}: Lc Lc^T err {worst:.2e} yardstick {yard:.2e} bound {tol:.1e}")
    assert worst <= tol


@gpu
def test_draws_generator_duplicates_and_errors(hip):
    import lvae_amd as la
    gv = golden("predict_var.npz")
    mean, cov = inducing_call(gv, True, return_cov=True)
    gen = lambda: torch.Generator(device=DEV).manual_seed(11)
    a = la.sample_trajectories(mean, cov, num_samples=3, generator=gen())
    b = la.sample_trajectories(mean, cov, num_samples=3, generator=gen())
    assert a.shape == (3, 15, 3) and U.bit_equal(a, b) and not U.bit_equal(a[0], a[1])   # a seeded generator reproduces
    assert U.bit_equal(la.sample_trajectories(mean, cov, eps=torch.zeros(2, 15, 3, dtype=torch.float64, device=DEV)),
                       mean.expand(2, 15, 3).contiguous())
    # one test row twice: its group is singular, and factors with the default jitter
    tidx = np.concatenate([gv["ind_tidx"], gv["ind_tidx"][4:5]])
    md, cd = inducing_call(gv, True, tidx=tidx, return_cov=True)
    k = int((cd.index == 15).nonzero()[0, 0])
    blk = cd.block(k).cpu()
    i, j = cd.index[k].tolist().index(4), cd.index[k].tolist().index(15)
    assert float((blk[:, i, i] - blk[:, i, j]).abs().max()) <= 1e-12 * float(blk.abs().max())   # (a duplicated row)
    d = la.sample_trajectories(md, cd, num_samples=4, generator=gen())
    assert d.shape == (4, 16, 3) and bool(torch.isfinite(d).all())
    assert float((d[:, 4] - d[:, 15]).abs().max()) < 1e-2            # the two copies move together (jitter 1e-8)
    # a block that is not positive definite raises, naming dim and group
    bad = la.PredictiveCovariance(cov.blocks.clone(), cov.index, cov.counts)
    bad.blocks[1, 2, 0, 0] = -1.0
    with pytest.raises(torch.linalg.LinAlgError, match="latent dim 1, group 2"):
        la.sample_trajectories(mean, bad)
    # rows in no group are an error before any launch
    part = la.PredictiveCovariance(cov.blocks[:, 1:].contiguous(), cov.index[1:].contiguous(), cov.counts[1:])
    with pytest.raises(ValueError):
        la.sample_trajectories(mean, part)


@gpu
def test_one_row_groups_agree_with_sample_predictions(hip):
    """With one-row groups and jitter = 0 a trajectory draw is a marginal draw: mean + sqrt(var) eps to a few ulps."""
    import lvae_amd as la
    gv = golden("predict_var.npz")
    tidx = gv["ind_tidx"][[0, 2, 4, 6, 7, 12, 13, 14]]                 # one row each of subjects 5 8 2 0 7 3 1 6
    mean, cov = inducing_call(gv, True, tidx=tidx, return_cov=True)
    assert cov.blocks.shape == (3, 8, 1, 1) and cov.counts.tolist() == [1] * 8
    eps = torch.randn(5, 8, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).to(DEV)
    got = la.sample_trajectories(mean, cov, eps=eps, jitter=0.0)
    want = torch.stack([la.sample_predictions(mean, cov.diagonal(), eps=e) for e in eps])
    ulp = float(np.spacing(float(want.abs().max())))
    err = float((got - want).abs().max())
    print(f"one-row groups against sample_predictions: {err / ulp:.1f} ulp of the largest draw")
    assert err <= 4 * ulp


# ------------------------------------------------------------------------------------------------------
# generate_trajectories
# ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("net", ["conv", "simple"])
def test_generate_trajectories(hip, net):
    import lvae_amd as la
    gv = golden("predict_var.npz")
    mean, cov = inducing_call(gv, True, return_cov=True)
    torch.manual_seed(0)
    model = (la.ConvVAE(3) if net == "conv" else la.SimpleVAE(3, 36)).to(DEV).eval()
    eps = torch.randn(2, 15, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(6)).to(DEV)
    images, draws = la.generate_trajectories(model, mean, cov, eps=eps)
    with torch.no_grad():
        want = model.decode(mean.float())
        z = la.sample_trajectories(mean, cov, eps=eps)
        want_draws = torch.stack([model.decode(zs.float()) for zs in z])     # one draw at a time, as the mean
    assert images.shape[0] == 15 and draws.shape[:2] == (2, 15) and draws.shape[2:] == images.shape[1:]
    assert U.bit_equal(images, want) and U.bit_equal(draws, want_draws)
    assert not images.requires_grad and bool(torch.isfinite(draws).all()) and not U.bit_equal(draws[0], draws[1])
    _, still = la.generate_trajectories(model, mean, cov, eps=torch.zeros_like(eps[:1]))
    assert U.bit_equal(still[0], images)                                     # eps = 0: the mean images
    i4, d4 = la.generate_trajectories(model, mean, cov, eps=eps, chunk_rows=4)   # 15 rows = 4 + 4 + 4 + 3
    assert U.bit_equal(i4, images) and U.bit_equal(d4, draws)
    only, none = la.generate_trajectories(model, mean)
    assert none is None and U.bit_equal(only, images)
    _, seeded = la.generate_trajectories(model, mean, cov, num_samples=2, generator=torch.Generator(device=DEV).manual_seed(1))
    _, again = la.generate_trajectories(model, mean, cov, num_samples=2, generator=torch.Generator(device=DEV).manual_seed(1))
    assert seeded.shape == draws.shape and U.bit_equal(seeded, again)
