"""Shared inputs, yardsticks and runners of the conditioned exact-KL tests (test_kl_cond_cpu.py, test_gpu_kl_cond.py,
test_gpu_kl_cond_abi.py): lvae_kl_cond_prepare_f64, lvae_dubo_cond_eval_f64 on its state, and condition_kl_closed
over them.

Problems: health_mnist_covariates rows, O.spec_full of dubo_util.CFG, L = 3, raw parameters log U(0.5, 2), noise
(0.8, 1.0, 1.2) -- so S >= noise I and both factors are well conditioned.  A case is (N training rows, Nn new rows);
the new rows are the leading whole subjects, except in 300+96, whose new rows are scattered over the subjects and
whose rows are shuffled.  The yardstick is oracle.lvae_oracle.kl_closed per dim under CPU autograd on the joint rows
cat(new, train), the new rows' (mu, logv) replaced by the point and differentiated alone, minus kl_closed on the
training rows.  ``closed_form`` restates the identity the kernels implement from O.gram / O.potrf / O.potrs:

    cond(m, l) = c + 1/2 (m^T A m - 2 r^T m + sum_i a_i e^{l_i} - sum_i l_i)
    W = K_tt^-1 K_tn    S = K_nn - K_nt W    A = S^-1    a = diag(A)    abar = W^T mu_t    r = A abar
    c = 1/2 (abar^T A abar - Nn + log|S| + tr(A W^T diag(v_t) W))

Bounds on the GPU: the project's rule min(max(10 x yardstick, 2e-12), 1e-6) (tests/test_gpu_predict_exact.py), the
yardstick being the change of closed_form / closed_eval under a relative 2^-50 perturbation of the hyper-parameters,
the noise and the training latents (abi_util.perturbed)."""
import ctypes
import functools

import numpy as np
import torch

import abi_util as U
import dubo_util as D
from oracle import lvae_oracle as O

DEV = D.DEV
L = D.L
SLAB = 512                      # kSyrkSlab of csrc/kl_cond.hip: panel rows per partial sum of the weighted SYRK
NOISE = (0.8, 1.0, 1.2)
COT = (1.0, -0.5, 2.0)
TAIL = 7
# id: (N, Nn, T rows per subject, scattered)
CASES = {
    "0+5": (0, 5, 5, False),                 # no training rows
    "1+1": (1, 1, 1, False),                 # the smallest shape
    "37+1": (37, 1, 1, False),               # one new row; N no multiple of 4 (the MFMA k step)
    "5+17": (5, 17, 17, False),              # Nn crosses a 16-tile; N smaller than a tile
    "70+33": (70, 33, 11, False),            # three tile rows, a ragged last tile, N crosses potrf's 64-block
    f"{SLAB + 3}+40": (SLAB + 3, 40, 10, False),   # two slabs, a 3-row tail: partials added in order
    "130+257": (130, 257, 1, False),         # Nn > N; the eval's second workgroup and sum launch; 15 SYRK blocks
    "300+96": (300, 96, 12, True),           # new rows scattered among the subjects, rows shuffled
}
CASE_IDS = list(CASES)
POINTS = ["zero", "own", "far"]
QUANT = ("val", "dm", "dlogv")
STATE = ("c", "r", "a", "A")
# GPU cases that miss the rule's bound would be held to 4 x their measured error here, with the cause:
# {(case, point or "state", quantity): 4 x measured}.  None was needed.
CASE_BOUND = {}


def spec():
    return O.spec_full(**D.CFG)


@functools.lru_cache(maxsize=None)
def problem(cid):
    from lvae_amd.data import health_mnist_covariates
    N, Nn, T, scattered = CASES[cid]
    seed = 700 + CASE_IDS.index(cid)
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    P = -(-(N + Nn) // T)
    X = torch.tensor(health_mnist_covariates(P, T, seed=seed))[:N + Nn]
    if scattered:
        perm = torch.tensor(rng.permutation(N + Nn))
        X = X[perm]          # shuffled: the first Nn rows are new, scattered over the subjects
    s = spec()
    mu = torch.randn(N + Nn, L, generator=gen, dtype=torch.float64)
    lv = 0.1 * torch.randn(N + Nn, L, generator=gen, dtype=torch.float64)
    return dict(cid=cid, N=N, Nn=Nn, spec=s, xn=X[:Nn].contiguous(), xt=X[Nn:].contiguous(),
                raw=np.log(rng.uniform(0.5, 2.0, (L, O.n_params(s)))), noise=np.array(NOISE),
                mu_n=mu[:Nn].contiguous(), lv_n=lv[:Nn].contiguous(), mu_t=mu[Nn:].contiguous(),
                lv_t=lv[Nn:].contiguous())


def hypers(c):
    """(constrained params [L, n_params], noise [L]) fp64 on the CPU"""
    return O.constrain(torch.tensor(c["raw"])), torch.tensor(c["noise"])


def point(cid, name):
    """(m [Nn, L], logv [Nn, L], cotangents [L]) of a named point"""
    c = problem(cid)
    m, lv = c["mu_n"], c["lv_n"]
    ones = torch.ones(L, dtype=torch.float64)
    if name == "zero":
        return torch.zeros_like(m), torch.zeros_like(lv), ones
    if name == "own":
        return m.clone(), lv.clone(), ones
    return m + 3.0, lv - 3.0, torch.tensor(COT, dtype=torch.float64)


def oracle_at(c, m, lv, cot):
    """kl_closed on cat(new, train) with the new rows at (m, lv), minus kl_closed on the training rows: values [L]
    and the gradients of sum_l cot_l val_l with respect to (m, lv)"""
    p, nz = hypers(c)
    s = c["spec"]
    m, lv = m.clone().requires_grad_(), lv.clone().requires_grad_()
    x = torch.cat([c["xn"], c["xt"]])
    mj, lj = torch.cat([m, c["mu_t"]]), torch.cat([lv, c["lv_t"]])
    vals = []
    for l in range(L):
        v = O.kl_closed(s, p[l], x, nz[l], mj[:, l], lj[:, l])
        if c["N"]:
            v = v - O.kl_closed(s, p[l], c["xt"], nz[l], c["mu_t"][:, l], c["lv_t"][:, l])
        vals.append(v)
    vals = torch.stack(vals)
    gm, gl = torch.autograd.grad(vals, (m, lv), cot)
    return dict(val=vals.detach(), dm=gm, dlogv=gl)


@functools.lru_cache(maxsize=None)
def oracle(cid, name):
    return oracle_at(problem(cid), *point(cid, name))


def closed_form_of(c, p, nz, mu_t, lv_t):
    """(c [L], r [L, Nn], a [L, Nn], A [L, Nn, Nn]) on the CPU from O.gram / O.potrf / O.potrs"""
    s, xn, xt, N, Nn = c["spec"], c["xn"], c["xt"], c["N"], c["Nn"]
    eye = torch.eye(Nn, dtype=torch.float64)
    out = []
    for l in range(L):
        S = O.gram(s, p[l], xn, xn) + nz[l] * eye
        abar = torch.zeros(Nn, dtype=torch.float64)
        Tm = torch.zeros(Nn, Nn, dtype=torch.float64)
        if N:
            Lt, _ = O.potrf(O.gram(s, p[l], xt, xt) + nz[l] * torch.eye(N, dtype=torch.float64))
            Ktn = O.gram(s, p[l], xt, xn)
            W = O.potrs(Ktn, Lt)
            S = S - Ktn.T @ W
            abar = W.T @ mu_t[:, l]
            Tm = (W * torch.exp(lv_t[:, l])[:, None]).T @ W
        Ls, logdet = O.potrf(S)
        A = O.potrs(eye, Ls)
        A = 0.5 * (A + A.T)
        r = A @ abar
        out.append((0.5 * (abar @ r - Nn + logdet + (A * Tm).sum()), r, torch.diagonal(A).clone(), A))
    return tuple(torch.stack([o[q] for o in out]) for q in range(4))


@functools.lru_cache(maxsize=None)
def closed_form(cid, perturb=False):
    """closed_form_of the case; perturb: from inputs perturbed by a relative 2^-50 (the tolerance yardstick)"""
    c = problem(cid)
    p, nz = hypers(c)
    v = [p, nz, c["mu_t"], c["lv_t"]]
    if perturb:
        gen = torch.Generator().manual_seed(80)
        v = [U.perturbed(t, gen) for t in v]
    return closed_form_of(c, *v)


def closed_eval(cf, m, lv, cot):
    """value, dm, dlogv of the closed form at (m, lv) [Nn, L] with cotangents cot [L]"""
    c0, r, a, A = cf
    mt, lt = m.T, lv.T                                         # [L, Nn]
    y = torch.einsum("lij,lj->li", A, mt)
    val = c0 + 0.5 * ((mt * y).sum(1) - 2 * (r * mt).sum(1) + (a * torch.exp(lt)).sum(1) - lt.sum(1))
    return dict(val=val, dm=(cot[:, None] * (y - r)).T, dlogv=(0.5 * cot[:, None] * (a * torch.exp(lt) - 1.0)).T)


def rule(yard):
    """the project's tolerance rule (tests/test_gpu_predict_exact.py)"""
    return min(max(10.0 * yard, 2e-12), 1e-6)


def point_bounds(cid, name):
    """{quantity: (bound, yardstick)}: the rule on the error of the perturbed closed form against the oracle"""
    ref = oracle(cid, name)
    got = closed_eval(closed_form(cid, True), *point(cid, name))
    out = {}
    for q in QUANT:
        yard = U.rel(got[q], ref[q])
        out[q] = (CASE_BOUND.get((cid, name, q), rule(yard)), yard)
    return out


def state_bounds(cid):
    ref, got = closed_form(cid), closed_form(cid, True)
    out = {}
    for q, r, g in zip(STATE, ref, got):
        yard = U.rel(g, r)
        out[q] = (CASE_BOUND.get((cid, "state", q), rule(yard)), yard)
    return out


# ------------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------------
class Lik:
    """a batched likelihood: .noise [L], taken as it stands (a GaussianLikelihood cannot hold a noise of 0)"""

    def __init__(self, noise, dev):
        self.noise = torch.as_tensor(noise, dtype=torch.float64).to(dev)

    def eval(self):
        return self


def modules(c, form="batched", dev=DEV, noise=None):
    """(kernel, likelihood) of the problem: one batched module + Lik, or per-dim lists"""
    import lvae_amd as la
    noise = c["noise"] if noise is None else noise
    if form == "batched":
        k = la.generate_kernel(**D.CFG, latent_dim=L).double()
        D.set_raw(k, c["raw"])
        return k.to(dev), Lik(noise, dev)
    ks, liks = [], []
    for l in range(L):
        k = la.generate_kernel(**D.CFG, latent_dim=1).double()
        D.set_raw(k, c["raw"][l:l + 1])
        ks.append(k.to(dev))
        liks.append(Lik(noise[l:l + 1], dev))
    return ks, liks


def condition(cid, form="batched", dev=DEV, **kw):
    import lvae_amd as la
    c = problem(cid)
    k, lik = modules(c, form, dev)
    return la.condition_kl_closed(k, lik, *(c[q].to(dev) for q in ("xn", "xt", "mu_t", "lv_t")), **kw)


def run_cond(cond, m, lv, cot, dev=DEV):
    m, lv = m.to(dev).requires_grad_(), lv.to(dev).requires_grad_()
    vals = cond(m, lv)
    gm, gl = torch.autograd.grad(vals, (m, lv), cot.to(dev))
    return dict(val=vals.detach().cpu(), dm=gm.cpu(), dlogv=gl.cpu())


def read_state(state, Nn, n_dims=L):
    """(c, r, a, A, mask) CPU tensors of a state buffer (cond_state.hpp: 256-byte aligned arrays in this order)"""
    al = lambda n: (8 * n + 255) // 256 * 256
    sizes = [n_dims, n_dims * Nn, n_dims * Nn, n_dims * Nn * Nn]
    shapes = [(n_dims,), (n_dims, Nn), (n_dims, Nn), (n_dims, Nn, Nn)]
    raw = state.cpu()
    out, off = [], 0
    for n, sh in zip(sizes, shapes):
        out.append(raw[off:off + 8 * n].view(torch.float64).reshape(sh).clone())
        off += al(n)
    out.append(raw[off:off + 4 * Nn].view(torch.int32).clone())
    return out


# ------------------------------------------------------------------------------------------------------
# the C ABI directly
# ------------------------------------------------------------------------------------------------------
def abi_inputs(cid, noise=None, params=None):
    from lvae_amd import _lib as P
    c = problem(cid) if isinstance(cid, str) else cid
    p, nz = hypers(c)
    t = dict(xn=c["xn"], xt=c["xt"], mu=c["mu_t"], lv=c["lv_t"], p=p if params is None else params,
             noise=nz if noise is None else torch.as_tensor(noise, dtype=torch.float64))
    return c, P.make_spec(c["spec"]), {k: v.to(DEV).contiguous() for k, v in t.items()}


def prepare(hip, cid, noise=None, params=None, group=None, state=None):
    """lvae_kl_cond_prepare_f64 on a sentinel-filled, sentinel-tailed state, workspace and info, the dims in groups
    of ``group`` (default: all at once); returns a dict with the state, info and the tails"""
    from lvae_amd import _lib as P
    c, s, d = abi_inputs(cid, noise, params)
    N, Nn = c["N"], c["Nn"]
    Q, n_par = d["xn"].shape[1], d["p"].shape[1]
    group = L if group is None else group
    nbytes = hip.lvae_dubo_cond_state_size(L, Nn, 1)
    st, stail = U.workspace(nbytes)
    ws, wtail = U.workspace(hip.lvae_kl_cond_workspace_size(N, Nn, group))
    info = U.sentinel(L + TAIL, torch.int32)
    at = lambda t, off: ctypes.c_void_p(t.data_ptr() + off * t.element_size())
    for l0 in range(0, L, group):
        g = min(group, L - l0)
        rc = hip.lvae_kl_cond_prepare_f64(ctypes.byref(s), P.ptr(d["xt"]) if N else None, Q, N, P.ptr(d["xn"]), Q, Nn, g,
                                          at(d["p"], l0 * n_par), at(d["noise"], l0), at(d["mu"], l0) if N else None, L,
                                          at(d["lv"], l0) if N else None, L, P.ptr(st), L, l0, at(info, l0), P.ptr(ws),
                                          P.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, rc
    assert U.tail_untouched(stail) and U.tail_untouched(wtail)
    assert U.all_sentinel(info[L:])
    return dict(c=c, state=st, state_bytes=nbytes, info=info[:L].cpu(), Nn=Nn, state_tail=stail)


def evaluate(hip, prep, m, lv, cot=None):
    """lvae_dubo_cond_eval_f64 (Pn = Nn, T = 1) on the prepared state; returns the logical CPU tensors"""
    from lvae_amd import _lib as P
    Nn = prep["Nn"]
    md, ld = m.to(DEV).contiguous(), lv.to(DEV).contiguous()
    g = None if cot is None else torch.as_tensor(cot, dtype=torch.float64).to(DEV)
    n = dict(val=L, dm=Nn * L, dlogv=Nn * L)
    o = {k: U.sentinel(v + TAIL) for k, v in n.items()}
    rc = hip.lvae_dubo_cond_eval_f64(L, Nn, 1, P.ptr(prep["state"]), P.ptr(md), P.ptr(ld), P.ptr(g), P.ptr(o["val"]),
                                     P.ptr(o["dm"]), P.ptr(o["dlogv"]), P.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    for k in o:
        assert U.all_sentinel(o[k][n[k]:]), k
    return dict(val=o["val"][:L].cpu(), dm=o["dm"][:Nn * L].reshape(Nn, L).cpu(),
                dlogv=o["dlogv"][:Nn * L].reshape(Nn, L).cpu())
