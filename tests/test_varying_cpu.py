"""The varying-length DUBO / ELBO without a GPU: the loop-form oracle of varying_util.py against the pinned
oracle where both apply (uniform T) and against itself on shuffled rows, subject_layout, and the four
lvae_*_seg_f64 symbols in the header, the library and lvae_amd._lib.SIGNATURES, with unchanged workspace sizes.

Bounds: 1e-8 (dubo_util.BOUND's value bound) between two fp64 forms of one bound, the project's gradient bounds
(1e-7 data, 1e-6 dz) between their gradients; measured: 1.8e-10 / 5.7e-11 (uniform T, loop vs pinned, DUBO / ELBO)
and 1.7e-10 / 6.7e-11 (sorted vs shuffled rows)."""
import ctypes
import os
import re

import numpy as np
import torch

import dubo_util as D
import varying_util as V
from conftest import PKG, ROOT
from oracle import lvae_oracle as O

SYMBOLS = ["lvae_dubo_fwd_seg_f64", "lvae_dubo_bwd_seg_f64", "lvae_gp_elbo_fwd_seg_f64", "lvae_gp_elbo_bwd_seg_f64"]


def _uniform(P=7, T=9, M=20, seed=5):
    from lvae_amd.data import health_mnist_covariates
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    X = torch.tensor(health_mnist_covariates(P, T, seed=seed))
    s0, s1 = O.spec_split(**D.CFG, id_covariate=2)
    p0 = torch.tensor(rng.uniform(0.5, 2.0, O.n_params(s0)))
    p1 = torch.tensor(rng.uniform(0.5, 2.0, O.n_params(s1)))
    Z = X[np.sort(rng.choice(P * T, M, replace=False))]
    mu = torch.randn(P * T, generator=gen, dtype=torch.float64)
    lv = 0.1 * torch.randn(P * T, generator=gen, dtype=torch.float64)
    return s0, p0, s1, p1, 0.8, X, mu, lv, Z, P, T


def test_loop_oracle_equals_pinned_oracle_at_uniform_T():
    s0, p0, s1, p1, nz, X, mu, lv, Z, P, T = _uniform()
    want = O.deviance_upper_bound(s0, p0, s1, p1, nz, X, mu, lv, Z, P, T, D.EPS)
    got = V.loop_dubo(s0, p0, s1, p1, nz, X, mu, lv, Z, 2, D.EPS)
    e_d = D.rel(got, want)
    want = O.gpapprox_elbo(s0, p0, s1, p1, nz, X, mu, Z, P, T, D.EPS)
    got = V.loop_elbo(s0, p0, s1, p1, nz, X, mu, Z, 2, D.EPS)
    e_e = D.rel(got, want)
    print(f"loop vs pinned oracle, uniform T: dubo {e_d:.2e} elbo {e_e:.2e}")
    assert e_d < 1e-8 and e_e < 1e-8


def test_loop_oracle_shuffled_rows():
    cid = "7x9"
    perm = V.permutation(cid)
    a, b = V.oracle_dubo(cid), V.oracle_dubo(cid, shuffled=True)
    errs = dict(dubo=D.rel(b["dubo"], a["dubo"]), dmu=D.rel(b["dmu"], a["dmu"][perm]),
                dlogv=D.rel(b["dlogv"], a["dlogv"][perm]), dz=D.rel(b["dz"], a["dz"]))
    a, b = V.oracle_elbo(cid, 1), V.oracle_elbo(cid, 1, shuffled=True)
    errs.update(elbo=D.rel(b["elbo"], a["elbo"]), dy=D.rel(b["dy"], a["dy"][:, perm]))
    print("loop oracle, shuffled vs sorted rows:", {k: f"{e:.2e}" for k, e in errs.items()})
    assert errs["dubo"] < 1e-8 and errs["elbo"] < 1e-8
    assert errs["dmu"] < 1e-7 and errs["dlogv"] < 1e-7 and errs["dy"] < 1e-7
    assert errs["dz"] < 1e-6


def test_ragged_problem_is_ragged():
    for cid, (P, T, seg, M) in V.CASES.items():
        c = V.problem(cid)
        assert c["N"] == sum(seg) and c["Z"].shape == (V.L, M, c["X"].shape[1])
        assert [int(r.numel()) for r in V.subject_rows(c["X"])] == list(seg)
        for l in range(V.L):   # inducing rows are rows kept, distinct ones where enough are kept
            assert all(bool((c["X"] == zr).all(1).any()) for zr in c["Z"][l])
            assert torch.unique(c["Z"][l], dim=0).shape[0] == M or M > c["N"]


def test_subject_layout_shuffled_ids():
    import lvae_amd as la
    ids = torch.tensor([3.0, 1.0, 3.0, 2.0, 1.0, 3.0, 7.0])
    lay = la.subject_layout(ids)
    assert (lay.P, lay.T_max, lay.N) == (4, 3, 7)
    assert lay.seg_len.dtype == torch.int32 and lay.seg_len.tolist() == [2, 1, 3, 1]
    assert lay.gather.dtype == torch.int64
    assert lay.gather.reshape(4, 3).tolist() == [[1, 4, 1], [3, 3, 3], [0, 2, 5], [6, 6, 6]]
    assert lay.valid.reshape(4, 3).tolist() == [[True, True, False], [True, False, False], [True, True, True],
                                                [True, False, False]]
    # every row of the batch sits in exactly one valid slot
    assert sorted(lay.gather[lay.valid].tolist()) == list(range(7))
    c = V.problem("7x9")
    perm = V.permutation("7x9")
    lay = la.subject_layout(c["X"][perm][:, V.ID_COL])
    assert lay.seg_len.tolist() == list(c["seg"]) and lay.T_max == c["T"] and lay.P == c["P"]
    assert torch.equal(c["X"][perm][lay.gather][lay.valid][:, V.ID_COL],
                       torch.repeat_interleave(torch.arange(7.0, dtype=torch.float64), torch.tensor(c["seg"])))


def test_varying_T_argument_checks():
    import lvae_amd as la
    c = V.problem("abi2x8")
    k0, k1, lik = D.modules_batched(c, "cpu")
    long_ids = torch.zeros(129, c["X"].shape[1], dtype=torch.float64)
    try:
        la.deviance_upper_bound_varying_T(V.L, k0, k1, lik, long_ids, torch.zeros(129, V.L, dtype=torch.float64),
                                          torch.zeros(129, V.L, dtype=torch.float64), c["Z"], V.ID_COL, V.EPS)
    except ValueError as e:
        assert "128" in str(e)
    else:
        raise AssertionError("T_max = 129 was accepted")
    try:
        la.elbo_varying_T(V.L, k0, k1, lik, c["X"], c["mu"][:-1], c["Z"], V.ID_COL, V.EPS)
    except ValueError as e:
        assert "train_yt" in str(e)
    else:
        raise AssertionError("a short train_yt was accepted")
    from lvae_amd.steps import DuboStep, ElboStep
    for cls in (DuboStep, ElboStep):
        try:
            cls(None, k0, k1, lik, None, c["Z"], None)
        except ValueError as e:
            assert "id_covariate" in str(e)
        else:
            raise AssertionError("T=None without id_covariate was accepted")


def test_seg_symbols_in_header_library_and_signatures():
    from lvae_amd import _lib
    with open(os.path.join(ROOT, "include", "lvae_hip.h")) as f:
        header = f.read()
    assert "no varying T" not in header
    so = os.path.join(PKG, "lvae_amd", "liblvae_hip.so")
    lib = ctypes.CDLL(so) if os.path.exists(so) else None
    for name in SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
        base = name.replace("_seg", "")
        # seg_len is one pointer more than the uniform call takes, right after the dims
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[base][1]) + 1
        assert _lib.SIGNATURES[name][1][:3] == _lib.SIGNATURES[base][1][:3]
        if lib is not None:
            assert hasattr(lib, name), name
    # (the library itself is there whenever build() has run; a GPU is not needed to load it)
    assert lib is not None, "liblvae_hip.so is not built"


def test_workspace_sizes_unchanged_for_the_workload():
    """lvae_dubo_workspace_size / lvae_gp_elbo_workspace_size at the workload's dims (L = 3, M = 120, P = 64, T = 16,
    Q = 6) are the bytes they were before the seg calls, which run on these same sizes; the arrays the two files
    carve add up to them (each rounded up to 256 bytes, the Gram adjoint's partials being the rest)."""
    from lvae_amd import _lib
    lib = _lib.load()

    def a(n):
        return (8 * n + 255) // 256 * 256
    Lw, M, P, T, Q = 3, 120, 64, 16, 6
    N, nt, G = P * T, 36, 4
    dub = (8 * a(Lw * N * M) + 13 * a(Lw * M * M) + 9 * a(Lw * P * T * T) + 2 * a(Lw * M) + 3 * a(Lw * N)
           + 3 * a(Lw) + a(Lw * P) + a(Lw * 8) + a(Lw * G * (2 * nt * 256 + 128 + 8)) + a(Lw * (2 + P)))
    ge = (5 * a(Lw * N * M) + 10 * a(Lw * M * M) + 8 * a(Lw * P * T * T) + 3 * a(Lw * M * 16) + 4 * a(Lw * N * 16)
          + 4 * a(Lw) + a(Lw * P) + a(Lw * 24) + a(Lw * G * (nt * 256 + 128 * 16 + 24)) + a(Lw * (2 + P)))
    for S in (1, 16):
        dd = _lib.DuboDims(Lw, M, P, T, Q, 1e-6)
        gd = _lib.GpElboDims(Lw, M, P, T, Q, S, 1e-6)
        got_d = int(lib.lvae_dubo_workspace_size(ctypes.byref(dd)))
        got_g = int(lib.lvae_gp_elbo_workspace_size(ctypes.byref(gd)))
        assert (got_d, got_g) == (34072832, 24728576)
        assert got_d - dub == got_g - ge and got_d - dub > 0
