"""lvae_gram_f64, lvae_gram_f32 and lvae_gram_bwd_f64 through the C ABI, against the fp64 oracle (O.gram and
autograd through it), at the shapes, layouts and spec sizes where the kernels take another path.

Spec families: (a) the reference family (template bucket (8, 2)); (b) bucket (16, 4) by factor count (the
covariate_missing_val masks: cat x bin x rbf x bin); (c9, c16) bucket (16, 4) by component count; (d) the
extensions (per, lin, per x rbf, lin x cat; bucket (8, 2): the adjoint's table path with sin tables); (e) a
spec at the limits: 16 components, 4 factors in some, n_params = 64 (per, rbf, lin, cat, bin mixed: the
(16, 4) adjoint's direct kernel_grad_acc path with periodic and linear factors).

Covariates (Q = 8, every value exact in fp32): column 0 integer-coded with pairwise distances 0, 1, 62, 63, 64,
65, 200 (a table hit, the last table entry, the first misses); 1 small signed integers; 2, 3 categories; 4, 7
0/1/2-valued (bin: 1 + 1 and 0 + 2 both equal 2); 5 half-integers; 6 reals rounded to multiples of 2^-10.
Hyper-parameters uniform in [0.3, 4] per latent dim, rounded to fp32 (so that the fp32 yardstick and the fp32
kernel see the very same values).

Tolerances.  f64 forward: 1e-13 of max|K| (test_gram_batched_semantics' bound).  Adjoint: 1e-12 of the max
gradient entry (the same test's bound).  f32 forward: the yardstick is the oracle itself evaluated in torch
float32 on the CPU; its max-abs error against the fp64 oracle relative to max|K| is taken over every forward
case of the family (one figure per family: a single (1, 1) case can round to an exact result and says nothing
about the format), and each case's kernel error must stay within 4x that (device vs host expf / sinf ulp
differences, another summation order over <= 16 components).

Measured on the MI355X (max over the family's 40 forward calls, relative to max|K|; bound = 4 x yardstick):
    family   oracle in fp32 (yardstick)   lvae_gram_f32   kernel / yardstick
    a        1.05e-07                     1.33e-07        1.26
    b        1.52e-07                     1.95e-07        1.28
    c9       1.40e-07                     1.40e-07        1.00
    c16      1.61e-07                     1.61e-07        1.00
    d        1.14e-06                     1.14e-06        1.00
    e        4.49e-06                     4.49e-06        1.00
(d, e: the periodic factor's argument pi |dx| / p at |dx| = 200 rounds to ~1e-4 in fp32, for the oracle and the
kernel alike.)  f64 forward: <= 2.7e-16 of max|K| in every family; adjoint: dparams <= 1.7e-15 of the max
gradient entry, ddiag <= 1.2e-16 of sum |G_ii|.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import abi_util as U
from oracle import lvae_oracle as O

pytestmark = pytest.mark.gpu
DEV = U.DEV
Q = 8
T0 = np.array([0.0, 1.0, 2.0, 64.0, 65.0, 66.0, 200.0])

_MISS = [{"covariate": 0, "mask": 4}, {"covariate": 3, "mask": 7}]
FAMILIES = {
    "a": O.spec_full(cat_kernel=[2], bin_kernel=[], sqexp_kernel=[0],
                     cat_int_kernel=[{"cont_covariate": 0, "cat_covariate": 2},
                                     {"cont_covariate": 0, "cat_covariate": 3},
                                     {"cont_covariate": 1, "cat_covariate": 3}],
                     bin_int_kernel=[], covariate_missing_val=[]),
    "b": O.spec_full(cat_kernel=[2], bin_kernel=[4], sqexp_kernel=[0, 6],
                     cat_int_kernel=[{"cont_covariate": 0, "cat_covariate": 3},
                                     {"cont_covariate": 6, "cat_covariate": 2}],
                     bin_int_kernel=[{"cont_covariate": 5, "bin_covariate": 4}], covariate_missing_val=_MISS),
    "c9": [[("rbf", 0)], [("rbf", 5)], [("rbf", 6)], [("cat", 2)], [("cat", 3)], [("cat", 2), ("rbf", 0)],
           [("cat", 3), ("rbf", 1)], [("bin", 4), ("rbf", 5)], [("cat", 2), ("rbf", 6)]],
    "d": [[("per", 0)], [("lin", 6)], [("per", 5), ("rbf", 0)], [("lin", 1), ("cat", 2)]],
}
FAMILIES["c16"] = FAMILIES["c9"] + [[("bin", 4)], [("rbf", 1)], [("cat", 3), ("rbf", 6)], [("bin", 7), ("rbf", 0)],
                                    [("cat", 2), ("cat", 3)], [("rbf", 0), ("rbf", 1)], [("bin", 4), ("cat", 2)]]
_CONT = [0, 1, 5, 6]
FAMILIES["e"] = [[("per", _CONT[r % 4]), ("rbf", _CONT[(r + 1 + r // 4) % 4])]
                 + ([("cat", 2), ("bin", 4)] if r % 5 == 0 else [("lin", 6)] if r % 5 == 2 else
                    [("cat", 3)] if r % 5 == 3 else [])
                 for r in range(16)]
FAM_IDS = list(FAMILIES)

FWD_SHAPES = [(1, 1), (64, 64), (63, 65), (65, 1), (130, 70)]
FWD_BATCH = [(1, 1), (3, 3)]
LAYOUTS = ["bcast", "distinct"]


def test_families_reach_the_buckets_and_limits():
    from lvae_amd import _lib as P
    mf = {k: max(len(c) for c in v) for k, v in FAMILIES.items()}
    nc = {k: len(v) for k, v in FAMILIES.items()}
    assert nc["a"] == 5 and mf["a"] == 2 and nc["d"] == 4 and mf["d"] == 2   # bucket (8, 2)
    assert nc["b"] <= 8 and mf["b"] == 4                                     # (16, 4) by factor count
    assert any([k for k, _ in c] == ["cat", "bin", "rbf", "bin"] for c in FAMILIES["b"])
    assert (nc["c9"], nc["c16"]) == (9, 16) and mf["c9"] == mf["c16"] == 2   # (16, 4) by component count
    assert nc["e"] == 16 and mf["e"] == 4 and O.n_params(FAMILIES["e"]) == 64
    for k, v in FAMILIES.items():
        assert P.make_spec(v).n_params == O.n_params(v)
    d = np.abs(T0[:, None] - T0[None, :])
    assert {0, 1, 62, 63, 64, 65, 200} <= set(d.ravel().tolist())


def covariates(prefix, n, seed, phase, off_seed):
    """[*prefix, n, Q] fp64; column 0 walks T0 with step `phase` (1 for x1, 3 for x2: every pair of T0 values
    meets once n1, n2 >= 7) from an offset x1 and x2 share (off_seed), so that x1[0] and x2[0] are at distance 0
    there and even a 1 x 1 Gram is O(1), not an underflowed RBF tail"""
    rng = np.random.default_rng(seed)
    sh = tuple(prefix) + (n,)
    X = np.empty(sh + (Q,))
    off = np.random.default_rng(off_seed).integers(0, 7, size=tuple(prefix) + (1,))
    X[..., 0] = T0[(phase * np.arange(n) + off) % 7]
    X[..., 1] = rng.integers(-3, 4, size=sh)
    X[..., 2] = rng.integers(0, 4, size=sh)
    X[..., 3] = rng.integers(0, 3, size=sh)
    X[..., 4] = rng.integers(0, 3, size=sh)
    X[..., 5] = rng.integers(-8, 9, size=sh) / 2.0
    X[..., 6] = np.round(rng.uniform(-3.0, 3.0, size=sh) * 1024.0) / 1024.0
    X[..., 7] = rng.integers(0, 3, size=sh)
    assert np.array_equal(X.astype(np.float32).astype(np.float64), X)
    return torch.tensor(X)


def draw_params(rng, L, P):
    return torch.tensor(rng.uniform(0.3, 4.0, (L, P)).astype(np.float32).astype(np.float64))


@functools.lru_cache(maxsize=None)
def fwd_case(fam, n1, n2, nb, L, layout):
    """Inputs and the fp64 / fp32 oracle Grams of one forward case, computed once and shared."""
    spec = FAMILIES[fam]
    seed = 100000 * FAM_IDS.index(fam) + 1000 * n1 + 10 * n2 + nb + (5 if layout == "bcast" else 0)
    rng = np.random.default_rng(seed)
    params = draw_params(rng, L, O.n_params(spec))
    prefix = () if layout == "bcast" else (nb, L)
    x1, x2 = covariates(prefix, n1, seed + 1, 1, seed), covariates(prefix, n2, seed + 2, 3, seed)
    K = O.gram(spec, params, x1, x2).expand(nb, L, n1, n2).contiguous()
    K32 = O.gram(spec, params.float(), x1.float(), x2.float()).expand(nb, L, n1, n2)
    assert K32.dtype == torch.float32
    diag = torch.tensor(rng.uniform(0.3, 4.0, L).astype(np.float32).astype(np.float64))
    kmax = float(K.abs().max()) or 1.0   # (an all-zero Gram: absolute error then)
    return dict(params=params, x1=x1, x2=x2, K=K, diag=diag, kmax=kmax,
                yard=float((K32.double() - K).abs().max()) / kmax)


@functools.lru_cache(maxsize=None)
def f32_yardstick(fam):
    """oracle-in-fp32 error against the fp64 oracle, relative to max|K|: the max over the family's forward cases"""
    return max(fwd_case(fam, n1, n2, nb, L, lay)["yard"]
               for (n1, n2) in FWD_SHAPES for (nb, L) in FWD_BATCH for lay in LAYOUTS)


def xview(x, nb, L, layout):
    """(device buffer, XView) of covariates x: broadcast [n, Q] with both strides 0, or a distinct x per (b, l)
    with ld > Q and padded batch strides in a NaN-filled buffer"""
    from lvae_amd import _lib as P
    if layout == "bcast":
        xd = x.to(DEV).contiguous()
        return xd, P.XView(ctypes.c_void_p(xd.data_ptr()), 0, 0, Q)
    n = x.shape[-2]
    ld = Q + 3
    sl = n * ld + 5
    sb = L * sl + 7
    buf, _ = U.padded(x, (sb, sl, ld, 1))
    return buf, P.XView(ctypes.c_void_p(buf.data_ptr()), sb, sl, ld)


def out_layout(nb, L, n1, n2):
    ldo = n2 + 3
    osl = n1 * ldo + 5
    osb = L * osl + 7
    return (nb, L, n1, n2), (osb, osl, ldo, 1)


def run_fwd(hip, fam, c, nb, L, n1, n2, layout, dtype, with_diag):
    """One forward call into a sentinel buffer with ldo > n2 and padded batch strides; returns the logical view
    (asserts the padding is untouched)."""
    from lvae_amd import _lib as P
    fn = hip.lvae_gram_f64 if dtype == torch.float64 else hip.lvae_gram_f32
    spec = P.make_spec(FAMILIES[fam])
    b1, v1 = xview(c["x1"], nb, L, layout)
    b2, v2 = xview(c["x2"], nb, L, layout)
    shape, strides = out_layout(nb, L, n1, n2)
    out = U.sentinel(U.extent(shape, strides) + 9, dtype)
    pd = c["params"].to(DEV)
    dg = c["diag"].to(DEV) if with_diag else None
    rc = fn(ctypes.byref(spec), v1, v2, nb, L, n1, n2, P.ptr(pd), P.ptr(dg), P.ptr(out), strides[0], strides[1],
            strides[2], P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.untouched_outside(out, shape, strides)
    return U.view(out, shape, strides).cpu()


def with_diag(K, diag):
    """K + diag[l] on i == j < min(n1, n2)"""
    nb, L, n1, n2 = K.shape
    eye = torch.zeros(n1, n2, dtype=K.dtype)
    k = min(n1, n2)
    eye[:k, :k] = torch.eye(k, dtype=K.dtype)
    return K + diag.reshape(1, L, 1, 1) * eye


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("nb,L", FWD_BATCH)
@pytest.mark.parametrize("n1,n2", FWD_SHAPES)
@pytest.mark.parametrize("fam", FAM_IDS)
def test_gram_f64(hip, fam, n1, n2, nb, L, layout):
    c = fwd_case(fam, n1, n2, nb, L, layout)
    for wd in (False, True):
        ref = with_diag(c["K"], c["diag"]) if wd else c["K"]
        got = run_fwd(hip, fam, c, nb, L, n1, n2, layout, torch.float64, wd)
        err = float((got - ref).abs().max()) / (float(ref.abs().max()) or 1.0)
        print(f"gram_f64 {fam} {n1}x{n2} nb={nb} L={L} {layout} diag={wd}: err {err:.3e}")
        assert err <= 1e-13


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("nb,L", FWD_BATCH)
@pytest.mark.parametrize("n1,n2", FWD_SHAPES)
@pytest.mark.parametrize("fam", FAM_IDS)
def test_gram_f32(hip, fam, n1, n2, nb, L, layout):
    c = fwd_case(fam, n1, n2, nb, L, layout)
    yard = f32_yardstick(fam)
    assert 2.0 ** -26 < yard < 1e-2  # (an fp32 figure: a few ulp up to the periodic factor's argument rounding)
    for wd in (False, True):
        ref = with_diag(c["K"], c["diag"]) if wd else c["K"]
        got = run_fwd(hip, fam, c, nb, L, n1, n2, layout, torch.float32, wd)
        err = float((got.double() - ref).abs().max()) / c["kmax"]
        print(f"gram_f32 {fam} {n1}x{n2} nb={nb} L={L} {layout} diag={wd}: kernel {err:.3e} "
              f"oracle-in-fp32 case {c['yard']:.3e} family {yard:.3e}")
        assert err <= 4.0 * yard


# ------------------------------------------------------------------------------------------------------
# adjoint
# ------------------------------------------------------------------------------------------------------
# (nb, L, n1, n2, G, x layout): 1023 / 1024 / 1025 elements around one 1024-element chunk; 3 x 20 x 20: the
# second chunk starts inside batch 2; 2 x 50 x 50: 5 chunks.  "half": about half of G exactly zero (the skip
# branch); "padded": ldg > n2 and padded gstride_l / gstride_b.
BWD_CASES = [(1, 3, 31, 33, "dense", "bcast"), (1, 3, 32, 32, "half", "distinct"), (1, 3, 41, 25, "padded", "bcast"),
             (3, 3, 20, 20, "dense", "distinct"), (2, 2, 50, 50, "half+padded", "distinct")]


@functools.lru_cache(maxsize=None)
def bwd_case(fam, nb, L, n1, n2, gmode, layout):
    spec = FAMILIES[fam]
    seed = 7000000 + 100000 * FAM_IDS.index(fam) + 1000 * n1 + 10 * n2 + nb
    rng = np.random.default_rng(seed)
    params = draw_params(rng, L, O.n_params(spec)).requires_grad_()
    prefix = () if layout == "bcast" else (nb, L)
    x1, x2 = covariates(prefix, n1, seed + 1, 1, seed), covariates(prefix, n2, seed + 2, 3, seed)
    G = torch.tensor(rng.standard_normal((nb, L, n1, n2)))
    if "half" in gmode:
        G = G * torch.tensor(rng.random((nb, L, n1, n2)) < 0.5)
        assert 0.3 < float((G == 0).double().mean()) < 0.7
    (O.gram(spec, params, x1, x2).expand(nb, L, n1, n2) * G).sum().backward()
    k = min(n1, n2)
    gd = torch.diagonal(G[:, :, :k, :k], dim1=-2, dim2=-1)   # [nb, L, k]
    return dict(params=params.detach(), x1=x1, x2=x2, G=G, grad=params.grad.clone(), ddiag=gd.sum((0, 2)),
                dscale=float(gd.abs().sum((0, 2)).max()),
                pre_p=torch.tensor(rng.standard_normal((L, O.n_params(spec)))),
                pre_d=torch.tensor(rng.standard_normal(L)))


def run_bwd(hip, fam, c, nb, L, n1, n2, gmode, layout, want_ddiag=True):
    from lvae_amd import _lib as P
    spec = P.make_spec(FAMILIES[fam])
    b1, v1 = xview(c["x1"], nb, L, layout)
    b2, v2 = xview(c["x2"], nb, L, layout)
    if "padded" in gmode:
        shape, gs = out_layout(nb, L, n1, n2)
        Gbuf, _ = U.padded(c["G"], gs)   # (NaN around the logical extent: reading it would poison the sums)
    else:
        Gbuf, gs = c["G"].to(DEV).contiguous(), (L * n1 * n2, n1 * n2, n2, 1)
    pd = c["params"].to(DEV)
    dp, dd = c["pre_p"].to(DEV), c["pre_d"].to(DEV)
    nbytes = hip.lvae_gram_bwd_workspace_size(nb, L, n1, n2)
    ws, tail = U.workspace(nbytes)
    rc = hip.lvae_gram_bwd_f64(ctypes.byref(spec), v1, v2, nb, L, n1, n2, P.ptr(pd), P.ptr(Gbuf), gs[0], gs[1], gs[2],
                               P.ptr(dp), P.ptr(dd) if want_ddiag else None, P.ptr(ws), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert U.tail_untouched(tail)   # lvae_gram_bwd_workspace_size bytes are enough
    return dp.cpu(), dd.cpu()


@pytest.mark.parametrize("nb,L,n1,n2,gmode,layout", BWD_CASES)
@pytest.mark.parametrize("fam", FAM_IDS)
def test_gram_bwd(hip, fam, nb, L, n1, n2, gmode, layout):
    c = bwd_case(fam, nb, L, n1, n2, gmode, layout)
    dp, dd = run_bwd(hip, fam, c, nb, L, n1, n2, gmode, layout)
    gmax = float(c["grad"].abs().max())
    err = float((dp - (c["pre_p"] + c["grad"])).abs().max()) / gmax
    derr = float((dd - (c["pre_d"] + c["ddiag"])).abs().max()) / c["dscale"]
    print(f"gram_bwd {fam} {nb}x{n1}x{n2} L={L} {gmode} {layout}: dparams {err:.3e} ddiag {derr:.3e}")
    assert gmax > 1e-2
    assert err <= 1e-12      # results are ADDED to the pre-filled dparams
    assert derr <= 1e-12     # ddiag[l] += sum_b sum_{i < min(n1, n2)} G[b, l, i, i]
    dp2, dd2 = run_bwd(hip, fam, c, nb, L, n1, n2, gmode, layout)
    assert torch.equal(dp, dp2) and torch.equal(dd, dd2)   # fixed summation order: bit-equal
    dp3, dd3 = run_bwd(hip, fam, c, nb, L, n1, n2, gmode, layout, want_ddiag=False)
    assert torch.equal(dp, dp3) and torch.equal(dd3, c["pre_d"])   # ddiag = NULL: dparams the same


# ------------------------------------------------------------------------------------------------------
# rejections
# ------------------------------------------------------------------------------------------------------
def _bad_specs():
    from lvae_amd import _lib as P
    good = P.make_spec(FAMILIES["a"])

    def mutated(f):
        s = P.KernelSpec.from_buffer_copy(good)
        f(s)
        return s
    def n_comp(s): s.n_comp = 17
    def n_fac(s): s.n_fac[0] = 5
    def n_params(s): s.n_params = 65
    def dim(s): s.dim[1][0] = 32
    return good, {"n_comp=17": mutated(n_comp), "n_fac=5": mutated(n_fac), "n_params=65": mutated(n_params),
                  "dim=32": mutated(dim)}


def _reject_operands(n1, n2):
    """covariates with 40 columns (a factor dim of 32 stays inside the rows whatever a launcher does with it)"""
    from lvae_amd import _lib as P
    x1 = torch.zeros(max(n1, 1), 40, dtype=torch.float64, device=DEV)
    x2 = torch.ones(max(n2, 1), 40, dtype=torch.float64, device=DEV)
    v = [P.XView(ctypes.c_void_p(x.data_ptr()), 0, 0, 40) for x in (x1, x2)]
    return (x1, x2), v


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gram_fwd_rejections(hip, dtype):
    from lvae_amd import _lib as P
    fn = hip.lvae_gram_f64 if dtype == torch.float64 else hip.lvae_gram_f32
    good, bad = _bad_specs()
    n1, n2, L = 5, 6, 2
    keep, v = _reject_operands(n1, n2)
    pd = torch.ones(L, 65, dtype=torch.float64, device=DEV)
    out = U.sentinel(2 * L * n1 * n2, dtype)

    def call(spec, nb, a, b):
        rc = fn(ctypes.byref(spec), v[0], v[1], nb, L, a, b, P.ptr(pd), None, P.ptr(out), L * a * b, a * b, b,
                P.stream_ptr())
        torch.cuda.synchronize()
        return rc
    for name, s in bad.items():
        assert call(s, 1, n1, n2) < 0, name
        assert U.all_sentinel(out), name
    assert call(good, 0, n1, n2) == -4 and U.all_sentinel(out)   # nb = 0 (argument 4)
    assert call(good, 1, 0, n2) == 0 and U.all_sentinel(out)     # empty: ok, nothing written
    assert call(good, 1, n1, 0) == 0 and U.all_sentinel(out)
    assert call(good, 1, n1, n2) == 0 and not U.all_sentinel(out)   # (the same call with nothing wrong runs)


def test_gram_bwd_rejections(hip):
    from lvae_amd import _lib as P
    good, bad = _bad_specs()
    n1, n2, L = 5, 6, 2
    keep, v = _reject_operands(n1, n2)
    pd = torch.ones(L, 65, dtype=torch.float64, device=DEV)
    G = torch.ones(L * n1 * n2, dtype=torch.float64, device=DEV)
    pre_p = torch.arange(L * 65, dtype=torch.float64).reshape(L, 65)
    pre_d = torch.tensor([3.0, -7.0], dtype=torch.float64)
    dp, dd = pre_p.to(DEV), pre_d.to(DEV)
    ws, tail = U.workspace(hip.lvae_gram_bwd_workspace_size(1, L, n1, n2))

    def call(spec, nb, a, b):
        rc = hip.lvae_gram_bwd_f64(ctypes.byref(spec), v[0], v[1], nb, L, a, b, P.ptr(pd), P.ptr(G), L * a * b, a * b,
                                   b, P.ptr(dp), P.ptr(dd), P.ptr(ws), P.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def unchanged():
        return torch.equal(dp.cpu(), pre_p) and torch.equal(dd.cpu(), pre_d)
    for name, s in bad.items():
        assert call(s, 1, n1, n2) < 0, name
        assert unchanged(), name
    assert call(good, 0, n1, n2) == -4 and unchanged()
    assert call(good, 1, 0, n2) == 0 and unchanged()
    assert call(good, 1, n1, 0) == 0 and unchanged()
    assert call(good, 1, n1, n2) == 0 and not unchanged()
