"""The C ABI of the fused MLP VAE (lvae_mlp_*_f32, include/lvae_hip.h) at its edges: every argument check returns its
code before any launch (outputs keep their sentinels), and a direct call writes its logical extent only -- outputs
and workspace followed by sentinel tails -- and agrees with the autograd Functions' route bit for bit, with the
optional outputs given and with them NULL (h1 .. h4 forward, the six weight gradients of the decoder's backward).

Host-side argument checks only: no call here reaches a kernel with a bad argument."""
import ctypes

import pytest
import torch

import abi_util as U
import simple_vae_util as S
from lvae_amd import _lib

pytestmark = pytest.mark.gpu
DEV = S.DEV
B, D, L, H1, H2 = 33, 37, 4, 300, 30
TAIL = 64


def _buf(*shape):
    """(flat sentinel buffer with a tail, its logical view)"""
    n = 1
    for s in shape:
        n *= s
    buf = U.sentinel(n + TAIL, torch.float32)
    return buf, buf[:n].view(*shape)


def _filled(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) - 0.5).to(DEV)


def _calls(hip, b=B, d=D, l=L):
    """{entry: (function, input tensors, output buffers, positions among inputs + outputs that may be NULL)} with
    valid arguments for (b, d, l)"""
    w = dict(w1=_filled(H1, d), b1=_filled(H1), w21=_filled(H2, H1), b21=_filled(H2), w211=_filled(l, H2),
             b211=_filled(l), w221=_filled(l, H2, seed=1), b221=_filled(l, seed=1), w3=_filled(H2, l), b3=_filled(H2),
             w31=_filled(H1, H2), b31=_filled(H1), w4=_filled(d, H1), b4=_filled(d))
    x, z, eps = _filled(b, d), _filled(b, l), _filled(b, l, seed=2)
    h1, h2, h3, h4 = _filled(b, H1), _filled(b, H2), _filled(b, H2, seed=3), _filled(b, H1, seed=3)
    recon = torch.sigmoid(_filled(b, d, seed=4))
    g_recon, g_mu, g_lv = _filled(b, d, seed=5), _filled(b, l, seed=5), _filled(b, l, seed=6)
    ews, _ = U.workspace(hip.lvae_mlp_enc_bwd_workspace_size(b, d, l))
    dws, _ = U.workspace(hip.lvae_mlp_dec_bwd_workspace_size(b, d, l))
    o = lambda *shape: _buf(*shape)[0]
    return {
        "enc_fwd": (hip.lvae_mlp_enc_fwd_f32,
                    [x, w["w1"], w["b1"], w["w21"], w["b21"], w["w211"], w["b211"], w["w221"], w["b221"]],
                    [o(b, H1), o(b, H2), o(b, l), o(b, l)], (9, 10)),
        "dec_fwd": (hip.lvae_mlp_dec_fwd_f32,
                    [z, None, None, None, w["w3"], w["b3"], w["w31"], w["b31"], w["w4"], w["b4"]],
                    [None, o(b, H2), o(b, H1), o(b, d)], (11, 12)),
        "dec_bwd": (hip.lvae_mlp_dec_bwd_f32,
                    [g_recon, recon, h4, h3, z, None, None, w["w3"], w["w31"], w["w4"]],
                    [o(H2, l), o(H2), o(H1, H2), o(H1), o(d, H1), o(d), o(b, l), None, None, dws], ()),
        "enc_bwd": (hip.lvae_mlp_enc_bwd_f32,
                    [g_mu, g_lv, x, h1, h2, w["w21"], w["w211"], w["w221"]],
                    [o(H1, d), o(H1), o(H2, H1), o(H2), o(l, H2), o(l), o(l, H2), o(l), ews], ()),
    }


def _call(fn, ins, dims, outs):
    return fn(*(_lib.ptr(t) for t in ins), *dims, *(_lib.ptr(t) for t in outs), _lib.stream_ptr())


def _untouched(outs):
    torch.cuda.synchronize()
    return all(t is None or (U.all_sentinel(t) if t.dtype == torch.float32 else bool((t == 0x7F).all())) for t in outs)


@pytest.mark.parametrize("entry", ["enc_fwd", "dec_fwd", "dec_bwd", "enc_bwd"])
def test_argument_checks_return_before_any_launch(hip, entry):
    fn, ins, outs, optional = _calls(hip)[entry]
    dims = (B, D, H1, H2, L)
    args = ins + outs
    for i, t in enumerate(args):           # a required pointer NULL: -1
        if t is None or i in optional:
            continue
        a = list(args)
        a[i] = None
        assert _call(fn, a[:len(ins)], dims, a[len(ins):]) == -1, (entry, i)
    for i in range(5):                     # a non-positive dimension: -2
        for v in (0, -3):
            bad = list(dims)
            bad[i] = v
            assert _call(fn, ins, bad, outs) == -2, (entry, i, v)
    for bad in ((B, D, 64, 16, L), (B, D, 300, 32, L), (B, D, 256, 30, L), (B, D, H1, H2, 33)):   # widths: -3
        assert _call(fn, ins, bad, outs) == -3, (entry, bad)
    for bad_d in (64, 1296):               # beyond the LDS bound: -4 (the pointers are never read)
        assert hip.lvae_mlp_vae_fused_ok(bad_d, H1, H2, L) == 0
        assert _call(fn, ins, (B, bad_d, H1, H2, L), outs) == -4, (entry, bad_d)
    assert _untouched(outs)


def test_sampled_forms_require_their_pointers(hip):
    c = _calls(hip)
    fn, ins, outs, _ = c["dec_fwd"]
    mu, lv, eps = _filled(B, L), _filled(B, L, seed=1), _filled(B, L, seed=2)
    for miss in range(3):                  # z NULL: mu, log_var, eps and z_out all required
        lat = [mu, lv, eps]
        lat[miss] = None
        assert _call(fn, [None] + lat + ins[4:], (B, D, H1, H2, L), [_buf(B, L)[0]] + outs[1:]) == -1
    assert _call(fn, [None, mu, lv, eps] + ins[4:], (B, D, H1, H2, L), outs) == -1       # z_out NULL
    fn, ins, outs, _ = c["dec_bwd"]
    gm, gl = _buf(B, L)[0], _buf(B, L)[0]
    sampled_in = ins[:5] + [lv, eps] + ins[7:]
    assert _call(fn, sampled_in, (B, D, H1, H2, L), outs[:6] + [None, gm, None, outs[9]]) == -1
    assert _call(fn, ins[:5] + [lv, None] + ins[7:], (B, D, H1, H2, L), outs[:6] + [None, gm, gl, outs[9]]) == -1
    assert _call(fn, ins, (B, D, H1, H2, L), outs[:6] + [None, None, None, outs[9]]) == -1   # plain form: g_z required
    for k in range(6):                     # the six weight-gradient outputs: all or none
        some = [None] * 6
        some[k] = outs[k]
        assert _call(fn, ins, (B, D, H1, H2, L), some + outs[6:]) == -1, k
    ws = outs[9]
    assert _call(fn, ins, (B, D, H1, H2, L), outs[:9] + [ws[4:]]) == -5                      # misaligned workspace
    assert _untouched(outs) and _untouched([gm, gl])


def test_direct_calls_write_their_extent_only_and_match_the_model(hip):
    """A direct call of each entry with the model's weights: outputs equal the model's fused route bit for bit (the
    same kernels), and the sentinel tails of every output and of both workspaces survive"""
    (x, mask, eps), _ = S.reference(B, D, L)
    model = S.on_gpu(L, D, (H1, H2), 5)
    x, mask, eps = x.float().to(DEV), mask.float().to(DEV), eps.float().to(DEV)
    res = S.run(model, x, mask, eps)
    assert model.last_route == {"encode": "fused", "decode": "fused"}
    dims = (B, D, H1, H2, L)
    wb = lambda *fcs: [p.detach() for fc in fcs for p in (fc.weight, fc.bias)]
    bufs = {k: _buf(*s) for k, s in dict(h1=(B, H1), h2=(B, H2), mu=(B, L), lv=(B, L), z=(B, L), h3=(B, H2),
                                         h4=(B, H1), recon=(B, D)).items()}
    flat = lambda *ks: [bufs[k][0] for k in ks]
    view = lambda k: bufs[k][1]
    assert _call(hip.lvae_mlp_enc_fwd_f32, [x] + wb(model.fc1, model.fc21, model.fc211, model.fc221), dims,
                 flat("h1", "h2", "mu", "lv")) == 0
    assert _call(hip.lvae_mlp_dec_fwd_f32, [None, view("mu"), view("lv"), eps] + wb(model.fc3, model.fc31, model.fc4),
                 dims, flat("z", "h3", "h4", "recon")) == 0
    torch.cuda.synchronize()
    for k, name in (("mu", "mu"), ("lv", "logv"), ("recon", "recon")):
        assert torch.equal(view(k).double().cpu(), res[name]), k
    assert torch.equal(view("z"), view("mu") + eps * torch.exp(0.5 * view("lv"))) or S.rel(
        view("z"), view("mu") + eps * torch.exp(0.5 * view("lv"))) < 1e-6
    # the loss's gradients on recon, mu, log_var by autograd on the direct outputs
    recon = view("recon").clone().requires_grad_()
    mu, lv = view("mu").clone().requires_grad_(), view("lv").clone().requires_grad_()
    mse, nll = model.loss_function(recon, x, mask)
    (mse.sum() + 0.3 * nll.sum() + 0.1 * (mu ** 2).sum() + 0.05 * lv.sum()).backward()
    gshape = dict(dw3=(H2, L), db3=(H2,), dw31=(H1, H2), db31=(H1,), dw4=(D, H1), db4=(D,), g_mu=(B, L), g_lv=(B, L),
                  dw1=(H1, D), db1=(H1,), dw21=(H2, H1), db21=(H2,), dw211=(L, H2), db211=(L,), dw221=(L, H2),
                  db221=(L,))
    bufs.update({k: _buf(*s) for k, s in gshape.items()})
    dws, dtail = U.workspace(hip.lvae_mlp_dec_bwd_workspace_size(B, D, L))
    ews, etail = U.workspace(hip.lvae_mlp_enc_bwd_workspace_size(B, D, L))
    w = lambda fc: fc.weight.detach()
    assert _call(hip.lvae_mlp_dec_bwd_f32,
                 [recon.grad, view("recon"), view("h4"), view("h3"), view("z"), view("lv"), eps, w(model.fc3),
                  w(model.fc31), w(model.fc4)], dims,
                 flat("dw3", "db3", "dw31", "db31", "dw4", "db4") + [None] + flat("g_mu", "g_lv") + [dws]) == 0
    g_mu, g_lv = view("g_mu") + mu.grad, view("g_lv") + lv.grad
    assert _call(hip.lvae_mlp_enc_bwd_f32,
                 [g_mu, g_lv, x, view("h1"), view("h2"), w(model.fc21), w(model.fc211), w(model.fc221)], dims,
                 flat("dw1", "db1", "dw21", "db21", "dw211", "db211", "dw221", "db221") + [ews]) == 0
    torch.cuda.synchronize()
    names = dict(dw3="fc3.weight", db3="fc3.bias", dw31="fc31.weight", db31="fc31.bias", dw4="fc4.weight",
                 db4="fc4.bias", dw1="fc1.weight", db1="fc1.bias", dw21="fc21.weight", db21="fc21.bias",
                 dw211="fc211.weight", db211="fc211.bias", dw221="fc221.weight", db221="fc221.bias")
    for k, n in names.items():
        assert torch.equal(view(k).double().cpu(), res["g_" + n]), k
    # the optional outputs NULL: no saved activations forward (the no_grad form), no weight gradients backward (a
    # frozen decoder) -- everything else bit for bit as above
    nul = {k: _buf(*s) for k, s in dict(mu=(B, L), lv=(B, L), z=(B, L), recon=(B, D), g_mu=(B, L), g_lv=(B, L),
                                        g_z=(B, L), g_z_full=(B, L), recon_z=(B, D)).items()}
    assert _call(hip.lvae_mlp_enc_fwd_f32, [x] + wb(model.fc1, model.fc21, model.fc211, model.fc221), dims,
                 [None, None, nul["mu"][0], nul["lv"][0]]) == 0
    assert _call(hip.lvae_mlp_dec_fwd_f32, [None, view("mu"), view("lv"), eps] + wb(model.fc3, model.fc31, model.fc4),
                 dims, [nul["z"][0], None, None, nul["recon"][0]]) == 0
    assert _call(hip.lvae_mlp_dec_fwd_f32, [view("z"), None, None, None] + wb(model.fc3, model.fc31, model.fc4),
                 dims, [None, None, None, nul["recon_z"][0]]) == 0
    dec_in = [recon.grad, view("recon"), view("h4"), view("h3"), view("z")]
    dec_w = [w(model.fc3), w(model.fc31), w(model.fc4)]
    assert _call(hip.lvae_mlp_dec_bwd_f32, dec_in + [view("lv"), eps] + dec_w, dims,
                 [None] * 6 + [None, nul["g_mu"][0], nul["g_lv"][0], dws]) == 0
    assert _call(hip.lvae_mlp_dec_bwd_f32, dec_in + [None, None] + dec_w, dims,
                 [None] * 6 + [nul["g_z"][0], None, None, dws]) == 0
    full = {k: _buf(*s) for k, s in gshape.items() if k in ("dw3", "db3", "dw31", "db31", "dw4", "db4")}
    assert _call(hip.lvae_mlp_dec_bwd_f32, dec_in + [None, None] + dec_w, dims,
                 [full[k][0] for k in ("dw3", "db3", "dw31", "db31", "dw4", "db4")]
                 + [nul["g_z_full"][0], None, None, dws]) == 0
    torch.cuda.synchronize()
    for k in ("mu", "lv", "z", "recon", "g_mu", "g_lv"):
        assert torch.equal(nul[k][1], view(k)), k
    assert torch.equal(nul["recon_z"][1], view("recon"))
    assert torch.equal(nul["g_z"][1], view("g_mu")) and torch.equal(nul["g_z_full"][1], view("g_mu"))
    for k in full:
        assert torch.equal(full[k][1], view(k)), k
    bufs.update({"nul_" + k: v for k, v in nul.items()})
    bufs.update({"full_" + k: v for k, v in full.items()})
    for k, (buf, v) in bufs.items():
        assert U.all_sentinel(buf[v.numel():]), k
    assert U.tail_untouched(dtail) and U.tail_untouched(etail)
