"""Helpers of the C-ABI edge tests (test_gpu_gram_abi.py, test_gpu_small_abi.py, the solve / factor
edge tests of test_gpu_linalg.py, test_gpu_hensman_abi.py, test_gpu_predict_abi.py, test_gpu_kl_closed_abi.py): sentinel-filled device
buffers with strided logical views, the checks that a call wrote its logical extent only, and the inputs the
two composite modules share (spec pairs, subject-layout covariates, hyper-parameter draws, the perturbation of
their tolerance yardstick).

Sentinel rule: a buffer passed with padding (ld > columns, padded batch strides) is allocated whole,
filled with NaN (floats) or 0x7f bytes (integers); after the call every element outside the logical
extent must still hold that bit pattern.
"""
import numpy as np
import torch

DEV = "cuda"
_BITS = {8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}


def sentinel(numel, dtype=torch.float64, device=DEV):
    """A flat buffer of `numel` sentinels: NaN for floating dtypes, 0x7f bytes for integer ones."""
    if dtype.is_floating_point:
        return torch.full((int(numel),), float("nan"), dtype=dtype, device=device)
    t = torch.empty(int(numel), dtype=dtype, device=device)
    t.view(torch.uint8).fill_(0x7F)
    return t


def bits(t):
    return t.view(_BITS[t.element_size()])


def extent(shape, strides, offset=0):
    """Elements a buffer needs to hold the strided view."""
    return offset + sum((int(s) - 1) * int(st) for s, st in zip(shape, strides)) + 1


def view(buf, shape, strides, offset=0):
    return torch.as_strided(buf, tuple(shape), tuple(strides), offset)


def padded(values, strides, offset=0, tail=5):
    """A sentinel buffer holding `values` (a CPU or device tensor) at the given strides; returns
    (buffer, logical view).  `tail` extra sentinels follow the last logical element."""
    buf = sentinel(extent(values.shape, strides, offset) + tail, values.dtype)
    v = view(buf, values.shape, strides, offset)
    v.copy_(values.to(buf.device))
    return buf, v


def untouched_outside(buf, shape, strides, offset=0):
    """True when every element of buf outside the strided logical extent is still the sentinel, bit for bit."""
    mask = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    view(mask, shape, strides, offset).fill_(True)
    want = bits(sentinel(1, buf.dtype, buf.device))
    return bool((bits(buf)[~mask] == want).all())


def all_sentinel(buf):
    return bool((bits(buf) == bits(sentinel(1, buf.dtype, buf.device))).all())


def rel(a, b):
    """max |a - b| / max |b| in fp64 on the CPU"""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def spd(L, n, seed, cond=1e3):
    """[L, n, n] SPD fp64 with eigenvalues logspace(1, cond) in a random orthogonal basis (test_gpu_linalg.spd)"""
    g = torch.Generator().manual_seed(seed)
    Q, _ = torch.linalg.qr(torch.randn(L, n, n, generator=g, dtype=torch.float64))
    ev = torch.logspace(0, np.log10(cond), n, dtype=torch.float64)
    A = (Q * ev) @ Q.transpose(-1, -2)
    return 0.5 * (A + A.transpose(-1, -2))


def nan_upper(A):
    """A copy of the [.., n, n] matrices with the strict upper triangle NaN (never read by the kernels)"""
    n = A.shape[-1]
    up = torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
    return torch.where(up, torch.full_like(A, float("nan")), A)


def workspace(nbytes, tail=256):
    """A 256-B aligned uint8 device buffer of exactly nbytes + a sentinel tail; returns (buffer, tail view)."""
    buf = torch.empty(int(nbytes) + tail, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    buf.fill_(0x7F)
    return buf, buf[int(nbytes):]


def tail_untouched(tail):
    return bool((tail == 0x7F).all())


# ------------------------------------------------------------------------------------------------------
# shared inputs of the composite edge tests (test_gpu_hensman_abi.py, test_gpu_predict_abi.py)
# ------------------------------------------------------------------------------------------------------
# Covariates (Q = 8) in the subject layout [P, T, Q]: column 0 time (half-integer steps + a sub-step offset per
# subject), 1 and 6 reals in [-2, 2], 2 the subject id (0..P-1, the id covariate), 3 a category in 0..2 and 4 a
# category in 0..3 (both per subject), 5 a 0/1 flag per subject, 7 a 0/1 flag per row.  `bin` factors sit on
# columns 5 and 7 only (0/1-valued: 1[a + b == 2] = a b there, positive semi-definite).
QC = 8
ID_COL = 2
_REF_CFG = dict(cat_kernel=[2], bin_kernel=[], sqexp_kernel=[0],
                cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 2}, {'cont_covariate': 0, 'cat_covariate': 3},
                                {'cont_covariate': 1, 'cat_covariate': 4}],
                bin_int_kernel=[], covariate_missing_val=[])   # CFG of test_gpu_regime_a.py


def spec_pairs():
    """{name: (spec0, spec1)}: the reference split (both in template bucket (8, 2)); mix1 = bucket (8, 2) with a
    (16, 4) id kernel (3 factors in a component); mix2 = a (16, 4) kernel (9 components) with a (8, 2) id kernel.
    gram_multi_f64 / gram_bwd_multi_f64 run both specs of a pair in the larger bucket."""
    from oracle import lvae_oracle as O
    ref = O.spec_split(**_REF_CFG, id_covariate=ID_COL)
    mix1 = ([[("rbf", 0)], [("rbf", 6)], [("cat", 3), ("rbf", 0)], [("bin", 5), ("rbf", 1)], [("cat", 4)]],
            [[("cat", 2)], [("cat", 2), ("rbf", 0)], [("cat", 2), ("rbf", 0), ("bin", 7)], [("cat", 2), ("rbf", 6)]])
    mix2 = ([[("rbf", 0)], [("rbf", 1)], [("rbf", 6)], [("cat", 3)], [("cat", 4)], [("cat", 3), ("rbf", 0)],
             [("cat", 4), ("rbf", 1)], [("bin", 5), ("rbf", 0)], [("bin", 7), ("rbf", 6)]],
            [[("cat", 2)], [("cat", 2), ("rbf", 0)], [("cat", 2), ("rbf", 1)]])
    return {"ref": ref, "mix1": mix1, "mix2": mix2}


def bucket(spec):
    """(components, most factors in a component) -> the template bucket the library picks: (8, 2) or (16, 4)"""
    return (8, 2) if len(spec) <= 8 and max(len(c) for c in spec) <= 2 else (16, 4)


def subject_covariates(rng, P, T, ids=None):
    """[P, T, QC] fp64 covariates of P subjects x T rows (ids: the subject ids, default 0..P-1)"""
    X = np.empty((P, T, QC))
    X[..., 0] = 0.5 * np.arange(T)[None, :] + rng.uniform(0.0, 0.5, (P, 1))
    X[..., 1] = rng.uniform(-2.0, 2.0, (P, T))
    X[..., 2] = (np.arange(P) if ids is None else np.asarray(ids))[:, None]
    X[..., 3] = rng.integers(0, 3, (P, 1))
    X[..., 4] = rng.integers(0, 4, (P, 1))
    X[..., 5] = rng.integers(0, 2, (P, 1))
    X[..., 6] = rng.uniform(-2.0, 2.0, (P, T))
    X[..., 7] = rng.integers(0, 2, (P, T))
    return torch.tensor(X)


def inducing_points(rng, L, M, T):
    """[L, M, QC]: M distinct points per latent dim over the covariates' range (an id no subject has)"""
    Z = subject_covariates(rng, L * M, 1, ids=np.full(L * M, -1.0)).reshape(L, M, QC)
    Z[..., 0] = torch.tensor(rng.uniform(0.0, 0.5 * T, (L, M)))
    return Z


def draw_hypers(rng, L, n):
    """[L, n] hyper-parameters (or noise with n = None -> [L]) per latent dim, uniform in [0.5, 2]"""
    return torch.tensor(rng.uniform(0.5, 2.0, (L,) if n is None else (L, n)))


def perturbed(t, gen):
    """t (1 + 2^-50 s), s = +-1 at random: the input perturbation of the tolerance yardstick"""
    s = torch.randint(0, 2, t.shape, generator=gen, dtype=torch.int64).to(t.dtype) * 2.0 - 1.0
    return t * (1.0 + 2.0 ** -50 * s)


def bit_equal(a, b):
    return a.shape == b.shape and bool((bits(a.contiguous()) == bits(b.contiguous())).all())


def info_problem():
    """L = 3, M = T = 3, P_b = 2, the reference split; covariates 10 apart in columns 0 and 1 (the Grams are
    diagonally dominant); every hyper-parameter 2 in dims 0 and 2, 0.5 in dim 1: K0zz[l] ~ 6 I, 1.5 I, 6 I and
    k1(x_p, x_p) has the diagonal 4, 1, 4."""
    from oracle import lvae_oracle as O
    s0, s1 = spec_pairs()["ref"]
    L, M, T, P_b = 3, 3, 3, 2
    rng = np.random.default_rng(5)
    x = subject_covariates(rng, P_b, T)
    x[..., 0] = 10.0 * torch.arange(T)[None, :]
    x[..., 1] = 10.0 * torch.arange(T)[None, :]
    z = inducing_points(rng, L, M, T)
    z[..., 0] = 10.0 * torch.arange(M)[None, :] + 5.0
    z[..., 1] = 10.0 * torch.arange(M)[None, :] + 5.0
    scale = torch.tensor([2.0, 0.5, 2.0], dtype=torch.float64)
    return dict(s0=s0, s1=s1, L=L, M=M, T=T, P_b=P_b, x=x.reshape(P_b * T, QC), z=z,
                p0=scale[:, None].expand(L, O.n_params(s0)).contiguous(),
                p1=scale[:, None].expand(L, O.n_params(s1)).contiguous())
