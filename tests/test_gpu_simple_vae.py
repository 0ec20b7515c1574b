"""SimpleVAE on the GPU: the fused HIP route (mlp_vae.hip), the layered route and the drivers that take the model.

Reference: lvae_amd.SimpleVAE in fp64 on the CPU with the same weights (simple_vae_util.reference; pinned to the
reference implementation by tests/golden/simple_vae.npz at 1e-12 in test_simple_vae_cpu.py).
Bound: 1e-4 of each tensor's max-abs, the project's fp32 bar.  It lies far above the error of correct fp32 code (stock
fp32 torch on a CPU sits at <= 3.4e-7 on every output and gradient of these shapes) and far below the error any
indexing mistake makes (of the order of the tensor itself).
Shapes: the smallest at which the kernels take another path -- B = 1 (a lone row), 33 (a one-row tail tile), 80 (three
tiles), 513 (the first B with two weight-gradient chunks); D = 5 (K no multiple of 2 or 4), 37 (Physionet's width, two
column tiles), 48; L = 1, 4, 16; and D = 57 with L = 32, the largest shape the fused route takes (163 824 of the CU's
163 840 bytes of LDS).  The steps that have no CPU oracle with this model (ElboStep, LatentInferenceStep)
are compared with the same step on the model's fp64 twin on the GPU (its 'stock' route), to the same bound."""
import os
import sys

import numpy as np
import pytest
import torch

import simple_vae_util as S
from conftest import GOLDEN, PKG, golden

pytestmark = pytest.mark.gpu
DEV = S.DEV
FUSED = {"encode": "fused", "decode": "fused"}
LAYERED = {"encode": "layered", "decode": "layered"}


def _check(model, case, route, tol=S.TOL):
    (x, mask, eps), want = case
    got = S.run(model, x.float().to(DEV), mask.float().to(DEV), eps.float().to(DEV))
    assert model.last_route == route, model.last_route
    err, name = S.worst(got, want)
    print(f"worst {err:.2e} ({name})")
    for k in want:
        e = S.rel(got[k], want[k])
        assert e < tol, (k, e)
    return err


def test_fixture_on_the_fused_route(hip):
    import lvae_amd as la
    g = golden("simple_vae.npz")
    model = la.SimpleVAE(int(g["L"]), int(g["D"])).double()
    model.load_state_dict(S.weights(model, int(g["seed"])), strict=True)
    model = model.float().to(DEV)
    names = ["mu", "logv", "recon", "mse", "nll"] + ["g_" + n for n, _ in model.named_parameters()]
    want = {k: torch.tensor(g[k]) for k in names}
    _check(model, ((torch.tensor(g["x"]), torch.tensor(g["mask"]), torch.tensor(g["eps"])), want), FUSED)


def _split_rows():
    from lvae_amd import _lib
    lib = _lib.load()
    return next(B for B in range(1, 1 << 16) if lib.lvae_mlp_wgrad_splits(B) >= 2)


@pytest.mark.parametrize("L", [1, 4, 16])
@pytest.mark.parametrize("D", [5, 37])
@pytest.mark.parametrize("B", [1, 33, 80])
def test_fused_forward_backward(hip, B, D, L):
    _check(S.on_gpu(L, D, (300, 30), 5), S.reference(B, D, L), FUSED)


def test_fused_forward_backward_split_rows(hip):
    B = _split_rows()
    assert hip.lvae_mlp_wgrad_splits(B) == 2 and hip.lvae_mlp_wgrad_splits(B - 1) == 1
    _check(S.on_gpu(16, 37, (300, 30), 5), S.reference(B, 37, 16), FUSED)


@pytest.mark.parametrize("D,hidden,route", [(48, (300, 30), FUSED), (1296, (300, 30), LAYERED),
                                            (37, (64, 16), LAYERED)])
def test_routes_agree_with_fp64(hip, D, hidden, route):
    _check(S.on_gpu(4, D, hidden, 5), S.reference(33, D, 4, hidden), route)


def test_fused_at_the_lds_bound(hip):
    """D = 57, L = 32: the encoder forward asks for 163 824 B of dynamic LDS, 16 B under a CU's 160 KiB"""
    assert hip.lvae_mlp_vae_lds_bytes(57, 300, 30, 32) == 163824 and hip.lvae_mlp_vae_fused_ok(58, 300, 30, 32) == 0
    _check(S.on_gpu(32, 57, (300, 30), 5), S.reference(33, 57, 32), FUSED)


class _Spy:
    """The HIP library with every lvae_mlp_* call's arguments recorded: {name: [args, ...]}"""

    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("lvae_mlp_"):
            return fn

        def call(*args):
            self.calls.setdefault(name, []).append(args)
            return fn(*args)
        return call


@pytest.fixture
def spy(hip, monkeypatch):
    from lvae_amd import _lib
    s = _Spy(hip)
    monkeypatch.setattr(_lib, "lib", lambda: s)
    return s


def _null(a):
    return a is None or a.value is None


def test_input_that_needs_grad_takes_the_layered_encoder(hip):
    model = S.on_gpu(4, 37, (300, 30), 5)
    x = torch.rand(8, 37, device=DEV, requires_grad=True)
    mu, _ = model.encode(x)
    assert model.last_route["encode"] == "layered"
    mu.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()


def test_decode_and_no_grad_are_bitwise_the_training_outputs(spy):
    """forward() in training mode writes the saved activations; under no_grad -- with parameters that still require
    grad -- NULL goes down for h1 .. h4 and nothing is saved; outputs bit for bit the same.  Positions: enc_fwd's
    (h1, h2) are arguments 14, 15, dec_fwd's (z_out, h3, h4) 15, 16, 17."""
    (x, mask, eps), _ = S.reference(80, 37, 16)
    x, eps = x.float().to(DEV), eps.float().to(DEV)
    model = S.on_gpu(16, 37, (300, 30), 5)
    assert all(p.requires_grad for p in model.parameters())
    recon, mu, lv = model(x, eps)                      # training mode: the activations are written
    assert model.last_route == FUSED and recon.requires_grad and mu.requires_grad
    enc, dec = spy.calls["lvae_mlp_enc_fwd_f32"], spy.calls["lvae_mlp_dec_fwd_f32"]
    assert len(enc) == len(dec) == 1
    assert not any(_null(a) for a in enc[0][14:16]) and not any(_null(a) for a in dec[0][15:18])
    assert len(recon.grad_fn.saved_tensors) == 9 and len(mu.grad_fn.saved_tensors) == 7
    with torch.no_grad():
        recon0, mu0, lv0 = model(x, eps)               # no_grad: NULL activation outputs
    assert model.last_route == FUSED and not recon0.requires_grad and recon0.grad_fn is None
    assert len(enc) == len(dec) == 2
    assert all(_null(a) for a in enc[1][14:16]) and all(_null(a) for a in dec[1][16:18]) and not _null(dec[1][15])
    assert torch.equal(recon0, recon) and torch.equal(mu0, mu) and torch.equal(lv0, lv)
    z = model.sample_latent(mu.detach(), lv.detach(), eps)
    for zz in (z, z.clone().requires_grad_()):
        assert torch.equal(model.decode(zz), recon) and model.last_route["decode"] == "fused"
    with torch.no_grad():
        assert torch.equal(model.decode(z), recon) and torch.equal(model.encode(x)[0], mu)
    assert all(_null(a) for a in dec[-1][15:18]) and all(_null(a) for a in enc[-1][14:16])
    assert torch.equal(model.encode(x)[0], mu)
    # frozen parameters and an input that needs no grad: nothing to save either, with grad mode on
    for p in model.parameters():
        p.requires_grad_(False)
    assert torch.equal(model(x, eps)[0], recon)
    assert all(_null(a) for a in enc[-1][14:16]) and all(_null(a) for a in dec[-1][16:18])


@pytest.mark.parametrize("B", [80, 0])
def test_backward_is_deterministic(hip, B):
    B = B or _split_rows()
    (x, mask, eps), _ = S.reference(B, 37, 16)
    args = (x.float().to(DEV), mask.float().to(DEV), eps.float().to(DEV))
    model = S.on_gpu(16, 37, (300, 30), 5)
    a, b = S.run(model, *args), S.run(model, *args)
    assert model.last_route == FUSED
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_nan_stays_in_its_row(hip):
    (x, _, eps), _ = S.reference(80, 37, 16)
    x, eps = x.float().to(DEV), eps.float().to(DEV)
    model = S.on_gpu(16, 37, (300, 30), 5)
    with torch.no_grad():
        recon, mu, lv = model(x, eps)
        bad = x.clone()
        bad[41, 3] = float("nan")
        recon_b, mu_b, lv_b = model(bad, eps)
    assert model.last_route == FUSED
    assert torch.isnan(mu_b[41]).all() and torch.isnan(lv_b[41]).all() and torch.isnan(recon_b[41]).all()
    keep = torch.arange(80, device=DEV) != 41
    for got, want in ((mu_b, mu), (lv_b, lv), (recon_b, recon)):
        assert torch.isfinite(got[keep]).all() and torch.equal(got[keep], want[keep])


# ------------------------------------------------------------------------------------------------------
# drivers: P = 6 subjects x T = 4 rows, D = 11, L = 3, M = 8
# ------------------------------------------------------------------------------------------------------
P, T, D, L, M, WEIGHT, EPS = 6, 4, 11, 3, 8, 0.15, 1e-6


def _driver_problem():
    import dubo_util as DU
    from lvae_amd.data import health_mnist_covariates
    from oracle import lvae_oracle as O
    x, mask, eps = S.inputs(P * T, D, L, 21)
    X = torch.tensor(health_mnist_covariates(P, T, seed=21))
    rng = np.random.default_rng(21)
    s0, s1 = O.spec_split(**DU.CFG, id_covariate=2)
    raw0 = np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s0))))
    raw1 = np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s1))))
    Z = torch.stack([X[np.sort(np.random.default_rng(210 + l).choice(P * T, M, replace=False))] for l in range(L)])
    return dict(x=x, mask=mask, eps=eps, X=X, s0=s0, s1=s1, raw0=raw0, raw1=raw1, Z=Z, cfg=DU.CFG)


def _kernels(c):
    import dubo_util as DU
    import lvae_amd as la
    k0, k1 = la.generate_kernel_batched(L, **c["cfg"], id_covariate=2)
    DU.set_raw(k0, c["raw0"])
    DU.set_raw(k1, c["raw1"])
    return k0.to(DEV), k1.to(DEV), la.GaussianLikelihood(L, noise=1.0, constrain=False).to(DEV)


def _watch_latents(model):
    """model.encode keeps its (mu, log_var) and their gradients"""
    kept, inner = {}, model.encode

    def encode(x):
        mu, lv = inner(x)
        mu.retain_grad()
        lv.retain_grad()
        kept["mu"], kept["lv"] = mu, lv
        return mu, lv
    model.encode = encode
    return kept


def _hensman_state(c):
    from oracle import lvae_oracle as O
    with torch.no_grad():
        H = O.gram(c["s0"], O.constrain(torch.tensor(c["raw0"])), c["Z"], c["Z"]) + 1e-6 * torch.eye(
            M, dtype=torch.float64)
    return torch.zeros(L, M, 1, dtype=torch.float64), H


def _hensman_cpu(c):
    """the oracle's Hensman step with the fp64 stock SimpleVAE on the CPU"""
    from oracle import lvae_oracle as O
    vae = S.build(L, D, (300, 30), 21)
    kept = _watch_latents(vae)
    m, H = _hensman_state(c)
    raw0, raw1 = torch.tensor(c["raw0"], requires_grad=True), torch.tensor(c["raw1"], requires_grad=True)
    loss, recon, kld, m2, H2 = O.hensman_step(vae, c["s0"], raw0, c["s1"], raw1, torch.ones(L), m, H, c["x"], c["mask"],
                                              c["X"], c["Z"], c["eps"], P, T, WEIGHT, 0.01, eps=EPS)
    assert vae.last_route == {"encode": "stock", "decode": "stock"}
    return dict(net=loss, recon=recon, gp=kld, dmu=kept["mu"].grad, dlv=kept["lv"].grad)


def _hensman_gpu(c, capturable=False):
    from lvae_amd.steps import HensmanStep
    vae = S.on_gpu(L, D, (300, 30), 21)
    kept = _watch_latents(vae)
    k0, k1, lik = _kernels(c)
    m, H = _hensman_state(c)
    params = list(vae.parameters()) + list(k0.parameters()) + list(k1.parameters())
    opt = torch.optim.Adam(params, lr=1e-3, capturable=True) if capturable else torch.optim.SGD(params, lr=0.0)
    step = HensmanStep(vae, k0, k1, lik, opt, m.to(DEV), H.to(DEV), c["Z"].to(DEV), P, T, weight=WEIGHT, eps=EPS)
    args = (c["x"].float().to(DEV), c["mask"].float().to(DEV), c["X"].to(DEV), c["eps"].float().to(DEV))
    return step, vae, kept, args


def test_hensman_step_with_simple_vae(hip):
    c = _driver_problem()
    want = _hensman_cpu(c)
    step, vae, kept, args = _hensman_gpu(c)
    net, rl, _, kl = step(*args)
    assert vae.last_route == FUSED
    got = dict(net=net, recon=rl, gp=kl, dmu=kept["mu"].grad, dlv=kept["lv"].grad)
    errs = {k: S.rel(got[k], want[k]) for k in want}
    print("HensmanStep:", {k: f"{e:.2e}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e < S.TOL, (k, e)


def test_dubo_step_with_simple_vae(hip):
    from lvae_amd.steps import DuboStep
    from oracle import lvae_oracle as O
    c = _driver_problem()
    ref = S.build(L, D, (300, 30), 21)
    recon, mu, lv = ref(c["x"], c["eps"])
    mu.retain_grad()
    lv.retain_grad()
    mse, _ = ref.loss_function(recon, c["x"], c["mask"])
    p0, p1 = O.constrain(torch.tensor(c["raw0"])), O.constrain(torch.tensor(c["raw1"]))
    gp = sum(O.deviance_upper_bound(c["s0"], p0[l], c["s1"], p1[l], 1.0, c["X"], mu[:, l], lv[:, l], c["Z"][l], P, T,
                                    EPS) for l in range(L)) / L
    net = mse.sum() + WEIGHT * gp
    net.backward()
    want = dict(net=net.detach(), recon=mse.sum().detach(), gp=gp.detach(), dmu=mu.grad, dlv=lv.grad)
    vae = S.on_gpu(L, D, (300, 30), 21)
    kept = _watch_latents(vae)
    k0, k1, lik = _kernels(c)
    opt = torch.optim.SGD(list(vae.parameters()) + list(k0.parameters()) + list(k1.parameters()), lr=0.0)
    step = DuboStep(vae, k0, k1, lik, opt, c["Z"].to(DEV), T, weight=WEIGHT, eps=EPS)
    out = step(c["x"].float().to(DEV), c["mask"].float().to(DEV), c["X"].to(DEV), c["eps"].float().to(DEV))
    assert vae.last_route == FUSED
    got = dict(net=out[0], recon=out[1], gp=out[3], dmu=kept["mu"].grad, dlv=kept["lv"].grad)
    errs = {k: S.rel(got[k], want[k]) for k in want}
    print("DuboStep:", {k: f"{e:.2e}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e < S.TOL, (k, e)
    for (name, p), (_, q) in zip(vae.named_parameters(), ref.named_parameters()):
        if q.grad is not None:
            assert S.rel(p.grad, q.grad) < S.TOL, name


def test_graphed_hensman_step_with_simple_vae(hip):
    """GraphedStep over the HensmanStep: three replays match three eager steps (Adam + the natural-gradient update
    move the state between them)"""
    import lvae_amd as la
    from lvae_amd.steps import GraphedStep
    c = _driver_problem()
    la.set_sync_checks(False)
    try:
        eager, vae_e, _, args = _hensman_gpu(c, capturable=True)
        eager(*args)                                             # = the graph's warm-up step
        outs_e = [[float(v) for v in eager(*args)] for _ in range(3)]
        graphed, vae_g, _, args_g = _hensman_gpu(c, capturable=True)
        g = GraphedStep(graphed, args_g, warmup=1)
        outs_g = [[float(v) for v in g()] for _ in range(3)]
        g.check()
    finally:
        la.set_sync_checks(True)
    assert vae_g.last_route == FUSED
    print("eager", outs_e, "graphed", outs_g)
    for a, b in zip(outs_e, outs_g):
        for va, vb in zip(a, b):
            assert abs(va - vb) <= S.TOL * abs(va), (a, b)
    assert S.rel(graphed.m, eager.m) < S.TOL and S.rel(graphed.H, eager.H) < S.TOL
    for (n, p), (_, q) in zip(vae_g.named_parameters(), vae_e.named_parameters()):
        assert S.rel(p, q) < S.TOL, n


def test_validate_simple_on_the_flat_tiny_dataset(hip):
    """validate(type_nnet='simple') == the value assembled by hand from its parts (test_gpu_dubo_drivers.py's check
    for 'conv'), with lvae_amd.validation and its drop-in module; an unknown type_nnet is refused"""
    import dubo_util as DU
    import lvae_amd as la
    from lvae_amd.data import HealthMNISTDataset
    from lvae_amd.evaluation import _whole_set
    from oracle import lvae_oracle as O
    dropin = os.path.join(PKG, "dropin")
    sys.path.insert(0, dropin)
    try:
        sys.modules.pop("validation", None)
        import validation as V
    finally:
        sys.path.remove(dropin)
    from lvae_amd.validation import validate
    assert V.validate is validate
    Lv, Mv, Tv, Pv, weight = 2, 5, 4, 3, 0.15
    ds = HealthMNISTDataset("tiny_data.csv", "tiny_labels.csv", "tiny_mask.csv", os.path.join(GOLDEN, "hmnist_tiny"),
                            device=DEV)
    vae = S.on_gpu(Lv, 1296, (300, 30), 3).eval()
    rng = np.random.default_rng(3)
    s0, s1 = O.spec_split(**DU.CFG, id_covariate=2)
    k0, k1 = la.generate_kernel_batched(Lv, **DU.CFG, id_covariate=2)
    DU.set_raw(k0, np.log(rng.uniform(0.5, 2.0, (Lv, O.n_params(s0)))))
    DU.set_raw(k1, np.log(rng.uniform(0.5, 2.0, (Lv, O.n_params(s1)))))
    k0, k1, lik = k0.to(DEV), k1.to(DEV), la.GaussianLikelihood(Lv, noise=1.0).to(DEV)
    labels = ds.batch(torch.arange(len(ds)))["label"].to(torch.float64)
    z = torch.stack([labels[np.sort(np.random.default_rng(3 + l).choice(len(ds), Mv, replace=False))]
                     for l in range(Lv)])
    seed = 11
    with torch.no_grad():
        torch.manual_seed(seed)
        images, mask, lab = _whole_set(ds, vae)
        assert images.shape == (12, 1, 1, 1296)
        recon, mu, lv = vae(images)
        assert vae.last_route == LAYERED
        mse, nll = vae.loss_function(recon, images, mask)
        gp = float(la.deviance_upper_bound_batched(Lv, k0, k1, lik, lab, mu.double(), lv.double(), z, Pv, Tv,
                                                   DU.EPS).sum())
    want = dict(mse=weight * gp / Lv + float(mse.sum()), nll=gp + float(nll.sum()))
    for loss in ("mse", "nll"):
        torch.manual_seed(seed)
        got = V.validate(vae, "simple", ds, "GPapprox_closed", 1, Lv, k0, k1, lik, z, Tv, weight, None, None, 2, loss,
                         eps=DU.EPS)
        err = abs(got - want[loss]) / abs(want[loss])
        print(f"validate simple {loss}: {got:.12e} by hand {want[loss]:.12e} err {err:.2e}")
        assert isinstance(got, float) and err < 1e-8
    with pytest.raises(NotImplementedError):
        V.validate(vae, "mlp", ds, "GPapprox_closed", 1, Lv, k0, k1, lik, z, Tv, weight, None, None, 2, "mse")


def _fp64_twin(vae):
    """the same model in fp64 on the GPU: its 'stock' route (plain torch ops) under the same HIP GP bound"""
    twin = S.build(L, D, (300, 30), 21).to(DEV)
    assert all(torch.equal(p.float(), q) for p, q in zip(twin.parameters(), vae.parameters()))
    return twin


def test_elbo_step_with_simple_vae(hip):
    """ElboStep (2 draws) on the fused fp32 model against the same step on its fp64 twin: loss terms and every
    network gradient"""
    from lvae_amd.steps import ElboStep
    c = _driver_problem()
    eps_gp = torch.randn(2, P * T, L, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    res = {}
    for name, dtype in (("fused", torch.float32), ("stock", torch.float64)):
        vae = S.on_gpu(L, D, (300, 30), 21)
        vae = vae if name == "fused" else _fp64_twin(vae)
        k0, k1, lik = _kernels(c)
        opt = torch.optim.SGD(list(vae.parameters()) + list(k0.parameters()) + list(k1.parameters()), lr=0.0)
        step = ElboStep(vae, k0, k1, lik, opt, c["Z"].to(DEV), T, weight=WEIGHT, eps=EPS, num_samples=2)
        out = step.forward_backward(c["x"].to(dtype).to(DEV), c["mask"].to(dtype).to(DEV), c["X"].to(DEV),
                                    c["eps"].to(dtype).to(DEV), eps_gp.to(dtype).to(DEV))
        assert vae.last_route == {"encode": name, "decode": name}
        res[name] = dict(net=out[0], recon=out[1], gp=out[3],
                         **{"g_" + n: p.grad for n, p in vae.named_parameters() if p.grad is not None})
    errs = {k: S.rel(res["fused"][k], res["stock"][k]) for k in res["stock"]}
    print("ElboStep:", {k: f"{e:.2e}" for k, e in errs.items()})
    # ('mse' leaves _log_vy out of the loss: autograd gives the fp64 twin no gradient there, the loss kernel zeros)
    extra = set(res["fused"]) - set(res["stock"])
    assert extra <= {"g__log_vy"} and all(not res["fused"][k].any() for k in extra) and len(errs) == 3 + 14
    for k, e in errs.items():
        assert e < S.TOL, (k, e)


def test_latent_inference_with_simple_vae(spy):
    """LatentInferenceStep / infer_new_subjects with the fused decoder (2 new subjects of 6): mu.grad / log_var.grad
    and the loss terms against the fp64 twin; the frozen network and its .grad stay bit for bit as they were.  With
    parameters that require grad the backward forms the weight gradients (autograd.grad drops them); with
    requires_grad off it passes NULL for all six (arguments 15 .. 20 of dec_bwd) and skips that launch: same
    mu.grad / log_var.grad bit for bit."""
    import lvae_amd as la
    from lvae_amd.steps import LatentInferenceStep, infer_new_subjects
    c = _driver_problem()
    Nn = 2 * T
    gen = torch.Generator().manual_seed(9)
    mj = torch.randn(P * T, L, generator=gen, dtype=torch.float64).to(DEV)
    lj = (0.1 * torch.randn(P * T, L, generator=gen, dtype=torch.float64)).to(DEV)
    X, z = c["X"].to(DEV), c["Z"].to(DEV)
    k0, k1, lik = _kernels(c)
    cond = la.condition_dubo(L, k0, k1, lik, X[:Nn], X[Nn:], mj[Nn:], lj[Nn:], z, T, EPS)
    res = {}
    for name, dtype in (("fused", torch.float32), ("stock", torch.float64)):
        vae = S.on_gpu(L, D, (300, 30), 21)
        vae = vae if name == "fused" else _fp64_twin(vae)
        for p in vae.parameters():
            p.grad = torch.full_like(p, 0.5)
        before = [(p.detach().clone(), p.grad.clone()) for p in vae.parameters()]
        mu, lv = torch.nn.Parameter(mj[:Nn].clone()), torch.nn.Parameter(lj[:Nn].clone())
        step = LatentInferenceStep(vae, cond, mu, lv, torch.optim.SGD([mu, lv], lr=0.0), weight=WEIGHT)
        net, rl, _, gp = step.forward_backward(c["x"][:Nn].to(dtype).to(DEV), c["mask"][:Nn].to(dtype).to(DEV),
                                               c["eps"][:Nn].to(dtype).to(DEV))
        assert vae.last_route["decode"] == name and mu.grad.dtype == torch.float64
        for p, (w, g) in zip(vae.parameters(), before):
            assert torch.equal(p.detach(), w) and torch.equal(p.grad, g)
        res[name] = dict(net=net, recon=rl, gp=gp, dmu=mu.grad, dlv=lv.grad)
    errs = {k: S.rel(res["fused"][k], res["stock"][k]) for k in res["stock"]}
    print("LatentInferenceStep:", {k: f"{e:.2e}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e < S.TOL, (k, e)
    bwd = spy.calls["lvae_mlp_dec_bwd_f32"]
    assert len(bwd) == 1 and not any(_null(a) for a in bwd[0][15:21])
    vae = S.on_gpu(L, D, (300, 30), 21).requires_grad_(False)
    mu, lv = torch.nn.Parameter(mj[:Nn].clone()), torch.nn.Parameter(lj[:Nn].clone())
    step = LatentInferenceStep(vae, cond, mu, lv, torch.optim.SGD([mu, lv], lr=0.0), weight=WEIGHT)
    step.forward_backward(c["x"][:Nn].float().to(DEV), c["mask"][:Nn].float().to(DEV), c["eps"][:Nn].float().to(DEV))
    assert len(bwd) == 2 and all(_null(a) for a in bwd[1][15:21]) and not _null(bwd[1][21])
    assert torch.equal(mu.grad, res["fused"]["dmu"]) and torch.equal(lv.grad, res["fused"]["dlv"])
    vae = S.on_gpu(L, D, (300, 30), 21)
    mu, lv, losses = infer_new_subjects(vae, cond, c["x"][:Nn].float().to(DEV), c["mask"][:Nn].float().to(DEV), iters=3)
    assert vae.last_route == FUSED and tuple(losses.shape) == (3, 4) and torch.isfinite(losses).all()
    assert mu.shape == (Nn, L) and mu.dtype == torch.float64 and torch.isfinite(mu).all() and torch.isfinite(lv).all()
