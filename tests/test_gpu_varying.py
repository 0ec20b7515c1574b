"""deviance_upper_bound_varying_T / elbo_varying_T and the four lvae_*_seg_f64 calls under them (the masked Grams,
the fused subject pass whose MFMA trip counts follow seg_len, the masked large-T route and adjoint kernels) against
the loop-form fp64 oracle of varying_util.py, on the padded C ABI itself, and through DuboStep / ElboStep (T=None)
and validate(varying_T=True).

Bounds (varying_util): value 1e-8, data gradients 1e-7, raw kernel and noise gradients 1e-6, dz 1e-6 -- the
project's dubo_util.BOUND / gp_elbo_util.BOUND / dz_util.BOUND, abi_util.rel; the golden case keeps
test_dubo_batched_reference_golden's bounds, the steps test_dubo_step_vs_oracle's.

Shapes (varying_util.CASES, L = 3): a full subject followed by a one-row subject in one workgroup's group of 16
(rows of the long one must not survive in LDS), a second group of one short subject, both sides of the fused
pass's T <= 32 limit, the workload's T = 16 / M = 120, and a batch in which no subject reaches T."""
import ctypes

import pytest
import torch

import abi_util as U
import dubo_util as D
import gp_elbo_util as G
import varying_util as V
from conftest import golden
from oracle import lvae_oracle as O

pytestmark = pytest.mark.gpu
DEV = D.DEV
L = V.L


# ---- 1. value and gradients against the oracle ----
@pytest.mark.parametrize("cid", V.PY_CASES)
def test_dubo_varying_vs_oracle(hip, cid):
    got = V.gpu_dubo(cid)
    V.check(got, V.oracle_dubo(cid), V.DUBO_QUANT, dict(V.DUBO_BOUND, dz=V.dz_bound("dubo", cid)),
            f"dubo {cid} vs loop oracle:")
    if cid == "7x9":   # per-dim module lists and a per-dim list of z are the batched computation
        lst = V.gpu_dubo(cid, "list")
        for k in V.DUBO_QUANT:
            assert U.bit_equal(lst[k], got[k]), k


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("cid", V.PY_CASES)
def test_elbo_varying_vs_oracle(hip, cid, S):
    got = V.gpu_elbo(cid, S)
    V.check(got, V.oracle_elbo(cid, S), V.ELBO_QUANT, dict(V.ELBO_BOUND, dz=V.dz_bound("elbo", cid, S)),
            f"elbo {cid} S = {S} vs loop oracle:")
    if cid == "7x9" and S == 4:
        lst = V.gpu_elbo(cid, S, "list")
        for k in V.ELBO_QUANT:
            assert U.bit_equal(lst[k], got[k]), k


def test_elbo_varying_sample_groups_and_single(hip):
    """17 samples = a group of 16 and a group of 1; train_yt [N, L] gives [L]"""
    import lvae_amd as la
    cid = "17x3"
    got = V.gpu_elbo(cid, 17)
    V.check(got, V.oracle_elbo(cid, 17), V.ELBO_QUANT, dict(V.ELBO_BOUND, dz=V.dz_bound("elbo", cid, 17)),
            f"elbo {cid} S = 17 vs loop oracle:")
    c = V.problem(cid)
    k0, k1, lik = D.modules_batched(c)
    y = V.samples(cid, 17)[0][0].to(DEV)
    one = la.elbo_varying_T(L, k0, k1, lik, c["X"].to(DEV), y, c["Z"].to(DEV), V.ID_COL, V.EPS)
    assert one.shape == (L,)
    assert D.rel(one, got["elbo"][0]) < 1e-12   # (its sample sits in another MFMA column: rounding, not bits)


# ---- 2. shuffled rows ----
@pytest.mark.parametrize("cid", ["7x9", "3x33"])
def test_varying_shuffled_rows(hip, cid):
    """rows in a random order: the same bound as the oracle on that order, gradients on the rows as given"""
    got = V.gpu_dubo(cid, shuffled=True)
    ref = V.oracle_dubo(cid, shuffled=True)
    V.check(got, ref, V.DUBO_QUANT, dict(V.DUBO_BOUND, dz=V.dz_bound("dubo", cid)), f"dubo {cid} shuffled:")
    perm = V.permutation(cid)
    srt = V.gpu_dubo(cid)
    assert D.rel(got["dmu"], srt["dmu"][perm]) < V.DUBO_BOUND["dmu"]
    assert D.rel(got["dlogv"], srt["dlogv"][perm]) < V.DUBO_BOUND["dlogv"]
    got = V.gpu_elbo(cid, 4, shuffled=True)
    V.check(got, V.oracle_elbo(cid, 4, shuffled=True), V.ELBO_QUANT, dict(V.ELBO_BOUND, dz=V.dz_bound("elbo", cid, 4)),
            f"elbo {cid} S = 4 shuffled:")
    assert D.rel(got["dy"], V.gpu_elbo(cid, 4)["dy"][:, perm]) < V.ELBO_BOUND["dy"]


def test_varying_layout_argument(hip):
    """a layout handed in gives the bits of the call that builds it"""
    import lvae_amd as la
    cid = "7x9"
    c = V.problem(cid)
    perm = V.permutation(cid)
    lay = la.subject_layout(c["X"][perm][:, V.ID_COL].to(DEV))
    assert lay.seg_len.is_cuda and lay.gather.is_cuda and lay.valid.is_cuda
    a, b = V.gpu_dubo(cid, shuffled=True), V.gpu_dubo(cid, shuffled=True, layout=lay)
    for k in V.DUBO_QUANT:
        assert U.bit_equal(a[k], b[k]), k


# ---- 3. seg_len == NULL is the uniform call, bit for bit ----
def _uniform_seg_null(hip, cid):
    """(existing entry points, *_seg entry points with seg_len == NULL) on one dubo_util case"""
    from lvae_amd import _lib as P
    old, _, _, _ = D.abi_run(hip, cid, cot=V.COT)
    c, s0, s1, dims, d = D.abi_inputs(cid)
    n, o = D.abi_outputs(c, s0, s1)
    ws, tail = U.workspace(hip.lvae_dubo_workspace_size(ctypes.byref(dims)))
    g = torch.as_tensor(V.COT, dtype=torch.float64).to(DEV)
    st = P.stream_ptr()
    common = (ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), None, P.ptr(d["x"]), P.ptr(d["z"]),
              P.ptr(d["mu"]), P.ptr(d["lv"]), P.ptr(d["p0"]), P.ptr(d["p1"]), P.ptr(d["noise"]))
    assert hip.lvae_dubo_fwd_seg_f64(*common, P.ptr(o["dubo"]), None, P.ptr(ws), st) == 0
    assert hip.lvae_dubo_bwd_seg_f64(*common, P.ptr(g), P.ptr(o["dmu"]), P.ptr(o["dlogv"]), P.ptr(o["dp0"]),
                                     P.ptr(o["dp1"]), P.ptr(o["dnoise"]), P.ptr(ws), st) == 0
    torch.cuda.synchronize()
    assert U.tail_untouched(tail)
    return old, {k: o[k][:n[k]].cpu() for k in o}


def _uniform_seg_null_elbo(hip, cid, S=3):
    from lvae_amd import _lib as P
    old, _, _, _ = G.abi_run(hip, cid, S)
    c, s0, s1, dims, d = G.abi_inputs(cid, S)
    n, o = G.abi_outputs(c, s0, s1, S)
    ws, tail = U.workspace(hip.lvae_gp_elbo_workspace_size(ctypes.byref(dims)))
    g = G.samples(cid, S)[1].contiguous().to(DEV)
    st = P.stream_ptr()
    common = (ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), None, P.ptr(d["x"]), P.ptr(d["z"]),
              P.ptr(d["y"]), P.ptr(d["p0"]), P.ptr(d["p1"]), P.ptr(d["noise"]))
    assert hip.lvae_gp_elbo_fwd_seg_f64(*common, P.ptr(o["elbo"]), None, P.ptr(ws), st) == 0
    assert hip.lvae_gp_elbo_bwd_seg_f64(*common, P.ptr(g), P.ptr(o["dy"]), P.ptr(o["dp0"]), P.ptr(o["dp1"]),
                                        P.ptr(o["dnoise"]), P.ptr(ws), st) == 0
    torch.cuda.synchronize()
    assert U.tail_untouched(tail)
    return old, {k: o[k][:n[k]].cpu() for k in o}


@pytest.mark.parametrize("cid", ["6x7x33", "3x33x17"])
def test_seg_null_is_the_uniform_call(hip, cid):
    for old, new in (_uniform_seg_null(hip, cid), _uniform_seg_null_elbo(hip, cid)):
        for k in old:
            assert torch.equal(old[k].reshape(-1), new[k].reshape(-1)), k


@pytest.mark.parametrize("cid", ["6x7x33", "3x33x17"])
def test_seg_all_T_is_the_uniform_call_to_rounding(hip, cid):
    """seg_len = T everywhere masks nothing: the uniform call's numbers (the masked kernels' own arithmetic is the
    same, so these agree far inside the value bounds)"""
    import lvae_amd as la
    c = D.problem(cid)
    k0, k1, lik = D.modules_batched(c)
    X = c["X"].to(DEV)
    a = la.deviance_upper_bound_batched(L, k0, k1, lik, X, c["mu"].to(DEV), c["lv"].to(DEV), c["Z"].to(DEV), c["P"],
                                        c["T"], D.EPS)
    b = la.deviance_upper_bound_varying_T(L, k0, k1, lik, X, c["mu"].to(DEV), c["lv"].to(DEV), c["Z"].to(DEV), 2,
                                          D.EPS)
    assert D.rel(b, a) < 1e-12


# ---- 4. padding independence at the C ABI ----
@pytest.mark.parametrize("cid", ["abi2x8", "7x9", "3x33"])
def test_padding_independence(hip, cid):
    c = V.problem(cid)
    pad = ~c["valid"]
    assert bool(pad.any())
    for name, run, rows in (("dubo", V.abi_dubo, ("dmu", "dlogv")), ("elbo", V.abi_elbo, ("dy",))):
        clean, dirty = run(hip, cid, False), run(hip, cid, True)
        for k in clean:
            assert not torch.isnan(clean[k].double()).any(), (name, k)
            assert U.bit_equal(clean[k], dirty[k]), (name, k)
        assert not clean["info"].any()
        for k in rows:
            assert bool((clean[k][..., pad, :] == 0).all()), (name, k)
        # and the numbers are the oracle's (abi2x8 goes through no Python call)
        ref = V.oracle_dubo(cid) if name == "dubo" else V.oracle_elbo(cid, V.S_ABI)
        if name == "dubo":
            assert D.rel(clean["dubo"], ref["dubo"]) < V.DUBO_BOUND["dubo"]
            assert D.rel(clean["dmu"][c["valid"]], ref["dmu"]) < V.DUBO_BOUND["dmu"]
            assert D.rel(clean["dlogv"][c["valid"]], ref["dlogv"]) < V.DUBO_BOUND["dlogv"]
        else:
            assert D.rel(clean["elbo"], ref["elbo"]) < V.ELBO_BOUND["elbo"]
            assert D.rel(clean["dy"][:, c["valid"]], ref["dy"]) < V.ELBO_BOUND["dy"]
        assert D.rel(clean["dz"], ref["dz"]) < V.dz_bound(name, cid, 0 if name == "dubo" else V.S_ABI)


# ---- 5. reproducibility ----
def test_varying_reproducible(hip):
    cid = "9x16"
    a, b = V.gpu_dubo(cid), V.gpu_dubo(cid)
    for k in V.DUBO_QUANT:
        assert U.bit_equal(a[k], b[k]), k
    a, b = V.gpu_elbo(cid, 4), V.gpu_elbo(cid, 4)
    for k in V.ELBO_QUANT:
        assert U.bit_equal(a[k], b[k]), k


# ---- 6. the reference's golden vector, rows shuffled ----
def test_dubo_varying_reference_golden_shuffled(hip):
    """test_dubo_batched_reference_golden's fixture (gpapprox.npz: P = T = 16, M = 40, one dim) with its rows in a
    random order through deviance_upper_bound_varying_T: the reference's values, within that test's bounds"""
    import lvae_amd as la
    g = golden("gpapprox.npz")
    N = int(g["P"]) * int(g["T"])
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(4))
    X, Zi = torch.tensor(g["X"])[perm].to(DEV), torch.tensor(g["Z"], device=DEV)
    k0, k1 = la.generate_kernel_batched(1, **D.CFG, id_covariate=2)
    D.set_raw(k0, g["raw0"].T)
    D.set_raw(k1, g["raw1"].T)
    k0, k1 = k0.to(DEV), k1.to(DEV)
    lik = la.GaussianLikelihood(1, noise=float(g["noise"])).to(DEV)
    mu = torch.tensor(g["mu"])[perm].to(DEV)[:, None].requires_grad_()
    lv = torch.tensor(g["logv"])[perm].to(DEV)[:, None].requires_grad_()
    du = la.deviance_upper_bound_varying_T(1, k0, k1, lik, X, mu, lv, Zi[None], 2, float(g["eps"]))
    assert du.shape == (1,)
    du.sum().backward()
    errs = dict(dubo=D.rel(du[0], g["dubo"]), dmu=D.rel(mu.grad[:, 0].cpu(), torch.tensor(g["dubo_dmu"])[perm]),
                dlogv=D.rel(lv.grad[:, 0].cpu(), torch.tensor(g["dubo_dlogv"])[perm]),
                draw0=D.rel(torch.cat([p.grad for _, p in k0.named_parameters()]), g["dubo_draw0"][:, 0]),
                draw1=D.rel(torch.cat([p.grad for _, p in k1.named_parameters()]), g["dubo_draw1"][:, 0]))
    print("golden, shuffled rows", errs)
    assert errs["dubo"] < 1e-9
    assert errs["dmu"] < 1e-7
    assert errs["dlogv"] < 1e-7
    assert errs["draw0"] < 1e-6
    assert errs["draw1"] < 1e-6


# ---- 7. return codes ----
def test_seg_return_codes(hip):
    """-4 for a NULL or misaligned workspace, -3 for T = 129, checked before any launch: nothing is written"""
    from lvae_amd import _lib as P
    cid = "abi2x8"
    c, s0, s1, d = V._abi_common(cid, False)
    Q = c["X"].shape[1]
    st = P.stream_ptr()
    g = torch.ones(V.S_ABI * L, dtype=torch.float64, device=DEV)

    def calls(dims, elbo):
        nrow = c["P"] * c["T"] * L * (V.S_ABI if elbo else 1)
        data = (P.ptr(d["y"]),) if elbo else (P.ptr(d["mu"]), P.ptr(d["lv"]))
        common = (ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(dims), P.ptr(d["seg"]), P.ptr(d["x"]),
                  P.ptr(d["z"]), *data, P.ptr(d["p0"]), P.ptr(d["p1"]), P.ptr(d["noise"]))
        outs = [U.sentinel(V.S_ABI * L if elbo else L), U.sentinel(L, torch.int32)]
        grads = [U.sentinel(nrow) for _ in range(1 if elbo else 2)] + [U.sentinel(L * s0.n_params),
                                                                        U.sentinel(L * s1.n_params), U.sentinel(L)]
        fwd = hip.lvae_gp_elbo_fwd_seg_f64 if elbo else hip.lvae_dubo_fwd_seg_f64
        bwd = hip.lvae_gp_elbo_bwd_seg_f64 if elbo else hip.lvae_dubo_bwd_seg_f64
        return (lambda ws: fwd(*common, *[P.ptr(t) for t in outs], ws, st),
                lambda ws: bwd(*common, P.ptr(g), *[P.ptr(t) for t in grads], ws, st), outs + grads)
    for elbo in (False, True):
        good = (P.GpElboDims(L, c["M"], c["P"], c["T"], Q, V.S_ABI, V.EPS) if elbo
                else P.DuboDims(L, c["M"], c["P"], c["T"], Q, V.EPS))
        size = hip.lvae_gp_elbo_workspace_size if elbo else hip.lvae_dubo_workspace_size
        ws, tail = U.workspace(size(ctypes.byref(good)))
        fwd, bwd, bufs = calls(good, elbo)
        for call in (fwd, bwd):
            assert call(None) == -4
            assert call(ctypes.c_void_p(ws.data_ptr() + 8)) == -4
        long = (P.GpElboDims(L, c["M"], c["P"], 129, Q, V.S_ABI, V.EPS) if elbo
                else P.DuboDims(L, c["M"], c["P"], 129, Q, V.EPS))
        fwd3, bwd3, bufs3 = calls(long, elbo)
        assert fwd3(P.ptr(ws)) == -3 and bwd3(P.ptr(ws)) == -3
        torch.cuda.synchronize()
        assert U.all_sentinel(ws) and all(U.all_sentinel(t) for t in bufs + bufs3)


# ---- 8. drivers ----
def _step_problem():
    """7x9's ragged batch with images: (img, mask, X) of the rows kept, fp64"""
    from lvae_amd.data import health_mnist_batch
    c = V.problem("7x9")
    img, mask, _ = health_mnist_batch(c["P"], c["T"], seed=9, dtype=torch.float64)
    return c, img[c["valid"]], mask[c["valid"]], c["X"]


def _oracle_step(kind, loss_function, c, img, mask, X, eps, eps_gp, weight):
    ref = O.ConvVAE(L).double()
    ref.load_state_dict(O.vae_weights(ref, 23))
    raw0 = torch.tensor(c["raw0"], requires_grad=True)
    raw1 = torch.tensor(c["raw1"], requires_grad=True)
    mu, lv = ref.encode(img)
    recon = ref.decode(mu + eps * torch.exp(0.5 * lv))
    mse, nll = ref.loss_function(recon, img, mask)
    p0, p1 = O.constrain(raw0), O.constrain(raw1)
    if kind == "dubo":
        gp = sum(V.loop_dubo(c["s0"], p0[l], c["s1"], p1[l], 1.0, X, mu[:, l], lv[:, l], c["Z"][l], V.ID_COL, V.EPS)
                 for l in range(L))
    else:
        gp = 0.0
        for s in range(eps_gp.shape[0]):
            Zs = mu + eps_gp[s] * torch.exp(0.5 * lv)
            for l in range(L):
                gp = gp - V.loop_elbo(c["s0"], p0[l], c["s1"], p1[l], 1.0, X, Zs[:, l], c["Z"][l], V.ID_COL, V.EPS)
        gp = gp / eps_gp.shape[0]
    if loss_function == "mse":
        gp = gp / L
        net = mse.sum() + weight * gp
    else:
        net = nll.sum() + gp
    net.backward()
    return ref, dict(net=net.detach(), recon=mse.sum().detach(), nll=nll.sum().detach(), gp=gp.detach(),
                     raw0=raw0.grad, raw1=raw1.grad)


@pytest.mark.parametrize("kind", ["dubo", "elbo"])
def test_varying_step_vs_oracle(hip, kind):
    """One DuboStep / ElboStep with T=None on 7x9's ragged batch against oracle.ConvVAE in fp64 and the loop oracle,
    assembled as training.py:499-575 ('mse', then 'nll'); a second call with the same X keeps the layout"""
    import lvae_amd as la
    from lvae_amd.steps import DuboStep, ElboStep
    from lvae_amd.vae import ConvVAE
    c, img, mask, X = _step_problem()
    S, weight = 2, 0.15
    gen = torch.Generator().manual_seed(2)
    eps = torch.randn(c["N"], L, generator=gen, dtype=torch.float64)
    eps_gp = torch.randn(S, c["N"], L, generator=gen, dtype=torch.float64)
    for loss_function in ("mse", "nll"):
        ref, want = _oracle_step(kind, loss_function, c, img, mask, X, eps, eps_gp, weight)
        vae = ConvVAE(L, 1296, p_input=0.0, p=0.0).double()
        vae.load_state_dict(ref.state_dict())
        vae = vae.float().to(DEV)
        k0, k1 = la.generate_kernel_batched(L, **D.CFG, id_covariate=2)
        D.set_raw(k0, c["raw0"])
        D.set_raw(k1, c["raw1"])
        k0, k1 = k0.to(DEV), k1.to(DEV)
        lik = la.GaussianLikelihood(L, noise=1.0).to(DEV)
        opt = torch.optim.SGD(list(vae.parameters()) + list(k0.parameters()) + list(k1.parameters()), lr=0.0)
        kw = dict(weight=weight, loss_function=loss_function, eps=V.EPS, id_covariate=V.ID_COL)
        Xd = X.to(DEV)
        args = (img.float().to(DEV), mask.float().to(DEV), Xd, eps.float().to(DEV))
        if kind == "dubo":
            step = DuboStep(vae, k0, k1, lik, opt, c["Z"].to(DEV), None, **kw)
        else:
            step = ElboStep(vae, k0, k1, lik, opt, c["Z"].to(DEV), None, num_samples=S, **kw)
            args = args + (eps_gp.float().to(DEV),)
        net, rl, nl, gp = step(*args)
        got = dict(net=net, recon=rl, nll=nl, gp=gp,
                   raw0=torch.stack([p.grad for _, p in k0.named_parameters()], 1),
                   raw1=torch.stack([p.grad for _, p in k1.named_parameters()], 1))
        errs = {k: D.rel(got[k], want[k]) for k in want}
        print(f"{kind} step T=None {loss_function}:", {k: f"{e:.2e}" for k, e in errs.items()})
        for k, e in errs.items():
            assert e < 1e-4, (loss_function, k, e)
        if loss_function == "mse":
            for (name, p), (_, q) in zip(vae.named_parameters(), ref.named_parameters()):
                if q.grad is not None:   # (_log_vy has no gradient under loss='mse')
                    assert D.rel(p.grad, q.grad) < 1e-3, name
        assert step.layout.builds == 1
        lay = step.layout(Xd)
        net2 = step(*args)[0]            # lr = 0: the same step again
        assert step.layout.builds == 1 and step.layout(Xd) is lay
        assert D.rel(net2, net) < 1e-6
        step(args[0], args[1], Xd.clone(), *args[3:])   # another tensor: a new layout
        assert step.layout.builds == 2


def test_validate_varying_T(hip):
    """validate(varying_T=True) on the tiny on-disk set with three rows dropped == the sum of its parts (the
    network's losses over the whole set and the varying calls), for both bounds, both losses and both module forms"""
    import test_gpu_dubo_drivers as TD
    import lvae_amd as la
    from lvae_amd.evaluation import _whole_set
    from lvae_amd.validation import validate
    s = TD._tiny_setup()
    Lt, weight, seed = s["L"], 0.15, 11
    keep = torch.tensor([0, 1, 2, 3, 5, 8, 9, 10, 6])     # subjects of 4, 2 and 3 rows, the last row out of place

    class Sub:
        """the rows `keep` of the tiny data set, as a data set"""
        def __len__(self):
            return int(keep.numel())

        def batch(self, idx):
            return s["ds"].batch(keep[idx.cpu()])
    ds = Sub()
    z = s["z"].to(DEV)
    zl = [zi for zi in z]

    def by_hand(type_KL, mods, zz, num_samples):
        """validate's own order of work (and of random draws): the whole set as one batch, then the GP term"""
        with torch.no_grad():
            torch.manual_seed(seed)
            images, mask, labels = _whole_set(ds, s["vae"])
            assert labels.shape[0] == 9
            recon, mu, lv = s["vae"](images)
            mse, nll = s["vae"].loss_function(recon, images, mask)
            mu, lv = mu.double(), lv.double()
            if type_KL == "GPapprox_closed":
                gp = float(la.deviance_upper_bound_varying_T(Lt, *mods, labels, mu, lv, zz, 2, D.EPS).sum())
            else:
                gp = 0.0
                for _ in range(num_samples):
                    Zs = s["vae"].sample_latent(mu, lv)
                    gp -= float(la.elbo_varying_T(Lt, *mods, labels, Zs, zz, 2, D.EPS).sum())
                gp /= num_samples
        return dict(mse=weight * gp / Lt + float(mse.sum()), nll=gp + float(nll.sum()))

    def run(type_KL, mods, zz, num_samples, loss):
        torch.manual_seed(seed)
        got = validate(s["vae"], "conv", ds, type_KL, num_samples, Lt, *mods, zz, 999, weight, None, None, 2, loss,
                       eps=D.EPS, varying_T=True)
        assert isinstance(got, float)
        return got
    for type_KL, mods, zz, ns in (("GPapprox_closed", s["batched"], z, 1), ("GPapprox_closed", s["lists"], zl, 1),
                                  ("GPapprox", s["lists"], zl, 2)):
        want = by_hand(type_KL, mods, zz, ns)
        for loss in ("mse", "nll"):
            got = run(type_KL, mods, zz, ns, loss)
            print(f"validate varying_T {type_KL} {loss}: {got:.12e} by hand {want[loss]:.12e}")
            assert abs(got - want[loss]) <= 1e-12 * abs(want[loss]), (type_KL, loss, got, want[loss])
