"""condition_kl_closed on the GPU (lvae_kl_cond_prepare_f64 + lvae_dubo_cond_eval_f64) against the fp64 CPU oracle:
kl_closed on the joint rows minus kl_closed on the training rows (kl_cond_util).  Bounds: the project's rule
min(max(10 x yardstick, 2e-12), 1e-6), the yardstick the change of the closed form under a relative 2^-50
perturbation of its inputs; every measured error is printed before it is asserted."""
import functools
import math
from fractions import Fraction

import pytest
import torch

import abi_util as U
import kl_cond_util as C
import simple_vae_util as S
from oracle import lvae_oracle as O

pytestmark = pytest.mark.gpu
DEV = C.DEV


@functools.lru_cache(maxsize=None)
def cond_of(cid):
    return C.condition(cid)


@pytest.mark.parametrize("name", C.POINTS)
@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_condition_matches_the_joint_kl(hip, cid, name):
    cond = cond_of(cid)
    c = C.problem(cid)
    assert (cond.L, cond.Nn) == (C.L, c["Nn"])
    m, lv, cot = C.point(cid, name)
    got, ref, bounds = C.run_cond(cond, m, lv, cot), C.oracle(cid, name), C.point_bounds(cid, name)
    errs = {q: U.rel(got[q], ref[q]) for q in C.QUANT}
    print(cid, name, {q: f"err {errs[q]:.2e} yardstick {bounds[q][1]:.2e} bound {bounds[q][0]:.1e}" for q in C.QUANT})
    for q in C.QUANT:
        assert got[q].dtype == torch.float64 and errs[q] <= bounds[q][0], (q, errs[q], bounds[q])


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_state_matches_the_closed_form(hip, cid):
    cond = cond_of(cid)
    Nn = C.problem(cid)["Nn"]
    *got, mask = C.read_state(cond.state, Nn)
    ref, bounds = C.closed_form(cid), C.state_bounds(cid)
    errs = {q: U.rel(g, r) for q, g, r in zip(C.STATE, got, ref)}
    print(cid, {q: f"err {errs[q]:.2e} yardstick {bounds[q][1]:.2e} bound {bounds[q][0]:.1e}" for q in C.STATE})
    for q in C.STATE:
        assert errs[q] <= bounds[q][0], (q, errs[q], bounds[q])
    A = got[3]
    assert U.bit_equal(A, A.transpose(1, 2)) and U.bit_equal(got[2], torch.diagonal(A, dim1=1, dim2=2))
    assert bool((mask == 1).all())


@pytest.mark.parametrize("cid", ["70+33", f"{C.SLAB + 3}+40", "0+5"])
def test_same_bits_on_every_call_and_for_every_grouping(hip, cid):
    """two calls give the same state; a max_workspace_bytes that holds one dim's workspace but not two forces one
    dim per group and gives it too"""
    c = C.problem(cid)
    one = C.read_state(cond_of(cid).state, c["Nn"])
    size = lambda g: int(hip.lvae_kl_cond_workspace_size(c["N"], c["Nn"], g))
    assert size(1) < size(2) < size(3)
    for kw in ({}, dict(max_workspace_bytes=size(1)), dict(max_workspace_bytes=size(2))):
        again = C.read_state(C.condition(cid, **kw).state, c["Nn"])
        assert all(U.bit_equal(a, b) for a, b in zip(one, again)), kw


def test_per_dim_lists_and_the_callers_dtype(hip):
    """modules and likelihoods as per-dim lists; fp32 latents get fp32 gradients of the same fp64 evaluation"""
    cid = "5+17"
    cond = C.condition(cid, "list")
    m, lv, cot = C.point(cid, "far")
    got, ref, bounds = C.run_cond(cond, m, lv, cot), C.oracle(cid, "far"), C.point_bounds(cid, "far")
    for q in C.QUANT:
        e = U.rel(got[q], ref[q])
        print("list", q, f"{e:.2e}", bounds[q])
        assert e <= bounds[q][0], (q, e, bounds[q])
    m32, lv32 = m.float().to(DEV).requires_grad_(), lv.float().to(DEV).requires_grad_()
    vals = cond(m32, lv32)
    gm, gl = torch.autograd.grad(vals, (m32, lv32), cot.to(DEV))
    want = C.run_cond(cond, m32.detach().double(), lv32.detach().double(), cot)
    assert vals.dtype == torch.float64 and gm.dtype == torch.float32 and gl.dtype == torch.float32
    assert U.bit_equal(vals.detach().cpu(), want["val"])
    assert U.bit_equal(gm.cpu(), want["dm"].float()) and U.bit_equal(gl.cpu(), want["dlogv"].float())


def _singular_problem():
    """0+5 with new row 1 a copy of new row 0 and dim 1's noise 0: S of dim 1 is exactly singular.  The second pivot
    of its factor is d - c^2 with d = k(x_0, x_0) = the sum of the scales and c = d (1 / sqrt(d)) as rounded: dim 1's
    first scale is moved until c^2 > d exactly, so that the pivot is negative (or rounds to 0) instead of resting on
    the sign of a rounding error.  Returns (problem, constrained params as the device holds them)."""
    from lvae_amd.elbo import _stack_modules
    c = dict(C.problem("0+5"))
    c["xn"] = c["xn"].clone()
    c["xn"][1] = c["xn"][0]
    c["raw"] = c["raw"].copy()
    c["noise"] = c["noise"].copy()
    c["noise"][1] = 0.0
    scale_idx, j = [], 0
    for comp in c["spec"]:
        scale_idx.append(j)
        j += 1 + sum(O.N_PARAMS[f[0]] for f in comp)
    for trial in range(400):
        c["raw"][1, 0] = math.log(0.5 + 0.003 * trial)
        params = _stack_modules(C.modules(c)[0])[1].detach().cpu()
        d = 0.0
        for i in scale_idx:
            d += float(params[1, i])
        cc = d * (1.0 / math.sqrt(d))
        if Fraction(cc) ** 2 > Fraction(d):
            return c, params
    raise AssertionError("no singular problem found")


def test_a_singular_dim_is_reported_and_stays_alone(hip):
    import lvae_amd as la
    c, params = _singular_problem()
    k, lik = C.modules(c)
    with pytest.raises(torch.linalg.LinAlgError, match="Schur"):
        la.condition_kl_closed(k, lik, c["xn"].to(DEV), c["xt"].to(DEV), c["mu_t"].to(DEV), c["lv_t"].to(DEV))
    bad = C.prepare(hip, c, noise=c["noise"], params=params)
    clean = C.prepare(hip, c, noise=C.NOISE, params=params)
    print("info", bad["info"].tolist(), clean["info"].tolist())
    assert bad["info"].tolist() == [0, 20002, 0] and clean["info"].tolist() == [0, 0, 0]
    sb, sc = C.read_state(bad["state"], c["Nn"]), C.read_state(clean["state"], c["Nn"])
    for l in (0, 2):
        assert all(U.bit_equal(a[l:l + 1], b[l:l + 1]) for a, b in zip(sb[:4], sc[:4])), l
    assert torch.isfinite(torch.stack([sc[3][l] for l in range(C.L)])).all()


@pytest.mark.parametrize("gp_divisor", [None, 1])
@pytest.mark.parametrize("loss_function", ["mse", "nll"])
def test_infer_new_subjects_matches_the_cpu_loop(hip, loss_function, gp_divisor):
    """infer_new_subjects with the fused fp32 SimpleVAE on 70+33's new rows against the same Adam loop in fp64 on the
    CPU, the GP term from closed_eval: to simple_vae_util.TOL, the bar test_gpu_simple_vae.py holds the DUBO route to"""
    from lvae_amd.steps import infer_new_subjects
    cid, iters, weight, D_img, L = "70+33", 5, 0.15, 37, C.L
    Nn = C.problem(cid)["Nn"]
    g = torch.Generator().manual_seed(12)
    img = torch.rand(Nn, D_img, generator=g).double()                     # fp32-exact values
    mask = (torch.rand(Nn, D_img, generator=g) < 0.75).double()
    mask[:, 0] = 1.0
    eps = torch.randn(iters, Nn, L, generator=g).double()
    vae = S.on_gpu(L, D_img, (300, 30), 21)
    for p in vae.parameters():
        p.grad = torch.full_like(p, 0.5)
    before = [(p.detach().clone(), p.grad.clone()) for p in vae.parameters()]
    mu, lv, losses = infer_new_subjects(vae, cond_of(cid), img.float().to(DEV), mask.float().to(DEV), iters=iters,
                                        weight=weight, loss_function=loss_function, eps=eps.float().to(DEV),
                                        gp_divisor=gp_divisor)
    assert isinstance(mu, torch.nn.Parameter) and mu.dtype == torch.float64 and tuple(losses.shape) == (iters, 4)
    for p, (w, gr) in zip(vae.parameters(), before):
        assert U.bit_equal(p.detach(), w) and U.bit_equal(p.grad, gr)
    ref_vae, cf, ones = S.build(L, D_img, (300, 30), 21), C.closed_form(cid), torch.ones(L, dtype=torch.float64)
    with torch.no_grad():
        m0, l0 = ref_vae.encode(img)
    mr, lr_ = torch.nn.Parameter(m0.clone()), torch.nn.Parameter(l0.clone())
    opt = torch.optim.Adam([{"params": mr}, {"params": lr_}], lr=1e-3)
    ref = []
    for it in range(iters):
        opt.zero_grad()
        mse, nll = ref_vae.loss_function(ref_vae.decode(ref_vae.sample_latent(mr, lr_, eps[it])), img, mask)
        gp = C.closed_eval(cf, mr, lr_, ones)["val"].sum() / (L if gp_divisor is None else gp_divisor)
        net = mse.sum() + weight * gp if loss_function == "mse" else nll.sum() + gp
        mr.grad, lr_.grad = torch.autograd.grad(net, (mr, lr_))
        opt.step()
        ref.append(torch.stack([net, mse.sum(), nll.sum(), gp]).detach())
    ref = torch.stack(ref)
    errs = dict(mu=S.rel(mu, mr), log_var=S.rel(lv, lr_), **{f"loss{k}": S.rel(losses[:, k], ref[:, k]) for k in range(4)})
    print(loss_function, gp_divisor, {k: f"{e:.2e}" for k, e in errs.items()}, "moved:", S.rel(mu, m0))
    assert float((mu.detach().cpu() - m0).abs().max()) > 1e-3      # the loop did move the latents
    assert all(e < S.TOL for e in errs.values()), errs
