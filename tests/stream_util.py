"""The stream-order conformance suite's protocol and row table (test_gpu_stream_order.py, test_stream_rows_cpu.py).

The contract under test is the one include/lvae_hip.h opens with: every entry point enqueues all of its work on the
caller's stream, a side stream the library forks is joined back before the call returns, and the Python layer passes
the stream the caller made current.

A ROW is one public operation at one small shape: ``make(seed)`` gives a dict of device-resident tensors (keys that
start with "_" are not inputs: modules, specs, workspaces, streams), ``run(live)`` only enqueues, ``outputs(live)``
names the result tensors, ``reaches`` lists the lvae_* entry points the row must call.

The protocol (Trial): reference (twice on the real inputs on the default stream, bit-equal), decoy pass (the same
row on decoy inputs in the live buffers: every buffer then holds a consistent state of a valid problem, and the pass
is the warm-up), delayed pass (on a fresh non-blocking stream: a delay, the event ``released``, device copies of the
real inputs over the live ones, run, device copies of the outputs, the decoy restored; ``released`` must not have
fired when run returns, so every launch was enqueued while the inputs still held the decoy), verdict (bit-equal to
the reference).  A launch that is not ordered behind the caller's stream computes on the decoy: a wrong value, never
a wrong address, because decoy and real inputs share every integer array and every id / category covariate.

While a row runs, Recorder wraps each lvae_* attribute of the loaded library and notes the stream argument.

ROWS (name: case; held to bits unless the row says otherwise):
"""
import ctypes
import os
import re
import time
import zlib

import numpy as np
import torch

from conftest import ROOT

DEV = "cuda"
REAL, DECOY = 1, 2
MIN_DELAY_MS, MAX_DELAY_MS, HOST_FACTOR = 20.0, 250.0, 10.0
POWER = 1e-3       # bit-held rows (tolerance 0): the decoy's outputs must differ from the reference by this, relative
HEADER = os.path.join(ROOT, "include", "lvae_hip.h")

# entry points with a stream argument that no row calls, each with its reason
EXCLUDED = {
    "lvae_set_early_stream": "enqueues nothing: it stores the stream it is given (the rows that invert through the "
                             "blocked Cholesky run with a stream lent through it)",
}


# ------------------------------------------------------------------------------------------------------
# the header: which entry points take a stream, and where
# ------------------------------------------------------------------------------------------------------
def stream_entries():
    """{name: index of the parameter the header calls ``stream``} over include/lvae_hip.h"""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = {}
    for m in re.finditer(r"\b(lvae_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", src):
        names = []
        for p in m.group(2).split(","):
            ids = re.findall(r"[A-Za-z_]\w*", p)
            names.append(ids[-1] if ids else "")
        if "stream" in names:
            out[m.group(1)] = names.index("stream")
    return out


class Recorder:
    """While active, every lvae_* entry point with a stream argument is wrapped on the library object: ``calls`` gets
    (name, the stream argument as an int); the attributes are restored on exit."""

    def __init__(self, lib):
        self.lib, self.calls, self._saved = lib, [], {}

    def __enter__(self):
        for name, idx in stream_entries().items():
            fn = getattr(self.lib, name)
            self._saved[name] = fn
            setattr(self.lib, name, self._wrap(name, idx, fn))
        return self

    def _wrap(self, name, idx, fn):
        def call(*args):
            v = args[idx]
            v = v.value if isinstance(v, ctypes.c_void_p) else v
            self.calls.append((name, int(v or 0)))
            return fn(*args)
        return call

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(self.lib, name, fn)
        return False

    def names(self):
        return {n for n, _ in self.calls}

    def streams(self):
        return {s for n, s in self.calls if n not in EXCLUDED}


# ------------------------------------------------------------------------------------------------------
# the delay
# ------------------------------------------------------------------------------------------------------
class Delay:
    """A device-side delay of a given length on the current stream: torch.cuda._sleep, calibrated once with two timed
    events around a fixed cycle count; a chain of fp64 matmuls sized the same way where _sleep is unusable."""

    def __init__(self):
        self.kind, self.per_ms, self.note = "sleep", None, ""
        try:
            self.per_ms = self._calibrate(lambda c: torch.cuda._sleep(int(c)), 100_000)
        except Exception as e:  # noqa: BLE001 (whatever _sleep raises here: the fallback is the answer)
            self.note = f"_sleep unusable ({type(e).__name__}: {e}); "
        if self.per_ms is None:
            self.kind = "matmul"
            self._a = torch.full((512, 512), 1.0 / 512, dtype=torch.float64, device=DEV)
            self.per_ms = self._calibrate(self._chain, 8)
        print(f"delay calibration: {self.note}{self.kind}, {self.per_ms:.4g} units per ms")

    def _chain(self, n):
        a = self._a
        for _ in range(int(n)):
            a = torch.matmul(a, self._a)

    @staticmethod
    def _calibrate(fn, units):
        fn(units)
        torch.cuda.synchronize()
        while units < 4e10:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(units)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 4.0:
                return units / ms
            units *= 4
        return None

    def enqueue(self, ms):
        n = max(1, int(ms * self.per_ms))
        if self.kind == "sleep":
            torch.cuda._sleep(n)
        else:
            self._chain(n)


_DELAY = []


def delay():
    if not _DELAY:
        _DELAY.append(Delay())
    return _DELAY[0]


# ------------------------------------------------------------------------------------------------------
# the protocol
# ------------------------------------------------------------------------------------------------------
def tensors(d):
    return {k: v for k, v in d.items() if not k.startswith("_") and isinstance(v, torch.Tensor)}


def overwrite(dst, src):
    """device-to-device copies of src's input tensors over dst's, on the current stream"""
    with torch.no_grad():
        for k, v in tensors(src).items():
            dst[k].copy_(v)


def snapshot(outs):
    return {k: v.detach().clone() for k, v in outs.items()}


def bits_equal(a, b):
    import abi_util as U
    return a.dtype == b.dtype and U.bit_equal(a.detach(), b.detach())


def distance(got, ref):
    """{name: max |got - ref| / max |ref|} over the floating outputs"""
    out = {}
    for k, r in ref.items():
        if r.dtype.is_floating_point and r.numel():
            g, r = got[k].detach().double(), r.detach().double()
            out[k] = float((g - r).abs().max() / max(float(r.abs().max()), 1e-300))
    return out


def elbo_module():
    """lvae_amd.elbo, the module (the package's attribute of that name is gpapprox's function)"""
    import importlib
    return importlib.import_module("lvae_amd.elbo")


def settle():
    """after a synchronise: the deferred info checks of the calls just made (all zero, or it raises)"""
    elbo_module().check_pending()


def is_loose(row, key):
    """True for an output of a row off bit equality whose name is <prefix>.<w> for a w of the row's ``loose``: the
    whole parameter name is matched (conv1.weight.grad, never deconv1.weight.grad)"""
    return not row.bitwise and any(key.endswith("." + w) for w in row.loose)


class Trial:
    """One row through the protocol; the two-callers tests drive two of these side by side."""

    def __init__(self, row, lib):
        self.row, self.lib = row, lib

    def same(self, got, ref, what):
        row = self.row
        loose = {k for k in ref if is_loose(row, k)}
        for k, r in ref.items():
            if k not in loose:
                assert bits_equal(got[k], r), (f"{row.name}: {what}: output {k} is not bit-equal (relative distance "
                                               f"{distance({k: got[k]}, {k: r}).get(k)})")
        d = distance({k: got[k] for k in loose}, {k: ref[k] for k in loose})
        assert all(v <= row.tol for v in d.values()), f"{row.name}: {what}: {d} above {row.tol}"

    def reference(self):
        row, runs = self.row, []
        for _ in range(2):
            d = row.make(REAL)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            row.run(d)
            self.host_ms = 1e3 * (time.perf_counter() - t0)
            torch.cuda.synchronize()
            settle()
            runs.append(snapshot(row.outputs(d)))
        self.ref = runs[0]
        for k, v in self.ref.items():
            assert not v.dtype.is_floating_point or bool(torch.isfinite(v).all()), f"{row.name}: reference {k}"
        self.same(runs[1], runs[0], "the two reference runs")
        self.need_ms = max(MIN_DELAY_MS, HOST_FACTOR * self.host_ms)

    def decoy_pass(self):
        row = self.row
        self.live = row.make(DECOY)
        self._real = row.make(REAL)
        self.real = tensors(self._real)
        self.decoy = snapshot(tensors(self.live))
        for k, v in self.real.items():
            if v.dtype in (torch.int32, torch.int64):
                assert torch.equal(v, self.decoy[k]), f"{row.name}: integer input {k} differs between decoy and real"
        with Recorder(self.lib) as rec:
            row.run(self.live)
        torch.cuda.synchronize()
        settle()
        # every floating output must move under the decoy (else it could detect nothing), by 100 x its tolerance;
        # the row's ``no_power`` names the flags and state values that are exempt
        d = {k: v for k, v in distance(row.outputs(self.live), self.ref).items() if k not in row.no_power}
        need = {k: max(100.0 * row.tol, POWER) if is_loose(row, k) else POWER for k in d}
        weak = {k: v for k, v in d.items() if v < need[k]}
        self.power = min(d.values())
        print(f"{row.name}: decoy-to-real distance {self.power:.3g} .. {max(d.values()):.3g} over {len(d)} outputs "
              f"(each needs {POWER:g}; {100.0 * row.tol:g} where held to {row.tol:g}); entries {sorted(rec.names())}")
        assert not weak, f"{row.name}: the decoy leaves these outputs too close to the reference: {weak}"

    def enqueue(self, s, ms):
        """steps 3.1-3.6 on s (the caller has made s current); the premise is asserted by check()"""
        row = self.row
        delay().enqueue(ms)
        self.released = torch.cuda.Event()
        self.released.record(s)
        overwrite(self.live, self.real)
        if hasattr(row, "before_run"):
            row.before_run(self.live, ms)
        with Recorder(self.lib) as rec:
            t0 = time.perf_counter()
            row.run(self.live)
            self.enq_ms = 1e3 * (time.perf_counter() - t0)
            self.premise = not self.released.query()
        self.got = snapshot(row.outputs(self.live))
        overwrite(self.live, self.decoy)
        self.rec, self.stream, self.delay_ms = rec, s, ms

    def check(self):
        """after s.synchronize(): premise, streams, reach, verdict"""
        row, rec = self.row, self.rec
        allowed = {self.stream.cuda_stream} | {int(h) for h in row.declared(self.live)}
        seen = rec.streams()
        print(f"{row.name} [{row.case}]: host enqueue {self.host_ms:.2f} ms (reference) / {self.enq_ms:.2f} ms "
              f"(delayed), delay {self.delay_ms:.1f} ms, streams seen {sorted(hex(h) for h in seen)} of allowed "
              f"{sorted(hex(h) for h in allowed)}")
        assert self.premise, (f"{row.name}: the delay ({self.delay_ms:.1f} ms) ended before run returned "
                              f"({self.enq_ms:.2f} ms): the row's premise fails")
        assert 0 not in seen, f"{row.name}: an entry point was given the null stream: {rec.calls}"
        assert seen <= allowed, f"{row.name}: entry points ran on undeclared streams {seen - allowed}: {rec.calls}"
        missing = set(row.reaches) - rec.names()
        assert not missing, f"{row.name}: never called {sorted(missing)}"
        settle()
        self.same(self.got, self.ref, "the delayed pass against the reference")
        if hasattr(row, "verify"):
            row.verify(self.got)


def run_row(row, lib):
    t = Trial(row, lib)
    t.reference()
    t.decoy_pass()
    assert t.need_ms <= MAX_DELAY_MS, f"{row.name}: needs a {t.need_ms:.0f} ms delay: cut the row into smaller ones"
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t.enqueue(s, t.need_ms)
    s.synchronize()
    torch.cuda.synchronize()
    t.check()
    return t


def run_pair(row_a, row_b, lib):
    """Two rows on two streams behind delays that end together: the second's delay is shorter by the host time that
    has passed since the first's was enqueued."""
    ta, tb = Trial(row_a, lib), Trial(row_b, lib)
    for t in (ta, tb):
        t.reference()
        t.decoy_pass()
    total = ta.need_ms + tb.need_ms   # (the first row's enqueue falls inside its own share)
    assert total <= MAX_DELAY_MS, f"{row_a.name} + {row_b.name}: need a {total:.0f} ms delay"
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    t0 = time.perf_counter()
    with torch.cuda.stream(sa):
        ta.enqueue(sa, total)
    rest = total - 1e3 * (time.perf_counter() - t0)
    assert rest >= tb.need_ms, f"{row_a.name} took {total - rest:.1f} ms of host time, more than its share"
    with torch.cuda.stream(sb):
        tb.enqueue(sb, rest)
    sa.synchronize()
    sb.synchronize()
    torch.cuda.synchronize()
    ta.check()
    tb.check()


# ------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------
def vary(seed, key, t, kind="add", amp=0.3):
    """t itself for the real inputs; for the decoy a copy moved by amp * U(-1, 1) (add) or scaled by
    exp(amp * U(-1, 1)) (mul: stays positive), drawn from (key, seed) alone"""
    if seed == REAL:
        return t
    is_np = isinstance(t, np.ndarray)
    x = torch.as_tensor(t)
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()) + 7919 * seed)
    u = torch.rand(x.shape, generator=g, dtype=torch.float64) * 2.0 - 1.0
    y = (x.double() + amp * u) if kind == "add" else x.double() * torch.exp(amp * u)
    y = y.to(x.dtype)
    return y.numpy() if is_np else y


def decoy_x(seed, X, T):
    """health_mnist_covariates rows [.., 6] with the time reversed within 0 .. T-1 (and the disease time that follows
    it) for the decoy: integer-coded like the real ones, the same ids and categories"""
    if seed == REAL:
        return X
    X = X.clone()
    t = (T - 1) - X[..., 0]
    X[..., 0] = t
    X[..., 1] = torch.where(X[..., 4] == 1, t - 9.0, torch.zeros_like(t))
    return X


def spd_of(seed, key, L, n, cond=100.0):
    import abi_util as U
    A = U.spd(L, n, zlib.crc32(key.encode()) % 1000 + seed, cond)
    # (U.spd fixes the spectrum, and with it log|A|, whatever the seed: the decoy is scaled as well)
    return A if seed == REAL else 1.7 * A


def module_tensors(prefix, *mods):
    out = {}
    for j, mod in enumerate(mods):
        for n, p in mod.named_parameters():
            out[f"{prefix}{j}.{n}"] = p.data
    return out


def params_of(*mods):
    return [p for m in mods for p in m.parameters() if p.requires_grad]


def grads_of(out, ins, cot=None, names=None):
    """{name (default g<index>): gradient} of out with respect to the tensors ins (unused ones left out)"""
    g = torch.autograd.grad(out, ins, cot, allow_unused=True)
    return {(names[j] if names else f"g{j}"): t for j, t in enumerate(g) if t is not None}


def named_grads(out, mod, prefix, more=(), cot=None):
    """grads_of over the tensors ``more`` and then a module's parameters, those named <prefix>.<parameter>.grad"""
    named = [(n, p) for n, p in mod.named_parameters() if p.requires_grad]
    names = [f"g{j}" for j in range(len(more))] + [f"{prefix}.{n}.grad" for n, _ in named]
    return grads_of(out, list(more) + [p for _, p in named], cot, names)


# MIOpen's backward-weights convolution (aten.convolution_backward, the route vae._ConvReluMaxPool2 takes below 512
# images and for shapes outside the ConvVAE's): its result differs in the last bits between two synchronised
# default-stream runs on the same inputs, so these weight gradients are held to the ConvVAE tests' fp32 bar instead
class MiopenWgrad:
    bitwise, tol = False, 1e-4
    loose = ("conv1.weight.grad", "conv2.weight.grad")
    why = ("MIOpen's backward-weights convolution (aten.convolution_backward below 512 images) is not "
           "bit-reproducible between two reference runs")


def varied_problem(c, seed, T):
    """a dubo_util-style problem with its float values varied for the decoy (covariates through decoy_x)"""
    d = dict(c)
    d["raw0"], d["raw1"] = vary(seed, "raw0", c["raw0"]), vary(seed, "raw1", c["raw1"])
    d["noise"] = vary(seed, "noise", np.asarray(c["noise"], dtype=np.float64), "mul", 0.2)
    d["mu"], d["lv"] = vary(seed, "mu", c["mu"], amp=0.5), vary(seed, "lv", c["lv"], amp=0.1)
    d["X"], d["Z"] = decoy_x(seed, c["X"], T), decoy_x(seed, c["Z"], T).clone()
    # dubo_util draws the inducing rows from X, where rows of different subjects coincide in every covariate the
    # shared kernel reads: K0zz is then singular up to the jitter, and 1 / eps swamps what the hyper-parameters and
    # H contribute to grad_H.  A distinct sub-step offset per inducing point (fp64 covariates) removes the
    # coincidences; the decoy's offsets run the other way.
    M = d["Z"].shape[-2]
    ramp = 0.4 * torch.arange(M, dtype=torch.float64) / M
    d["Z"][..., 0] += (0.05 + ramp) if seed == REAL else (0.45 - ramp)
    return d


def split_modules(c):
    import dubo_util as D
    return D.modules_batched(c, DEV)


def full_modules(L, raw, noise):
    import dubo_util as D
    import lvae_amd as la
    k = la.generate_kernel(**D.CFG, latent_dim=L)
    D.set_raw(k, raw)
    lik = la.GaussianLikelihood(L, noise=1.0)
    lik.noise = torch.as_tensor(noise)
    return k.to(DEV), lik.to(DEV)


def full_raw(L, rng_seed):
    import dubo_util as D
    import lvae_amd as la
    n = len(list(la.generate_kernel(**D.CFG, latent_dim=L).parameters()))
    return np.log(np.random.default_rng(rng_seed).uniform(0.5, 2.0, (L, n)))


def vae_of(kind, L, seed, D=None):
    """a ConvVAE / SimpleVAE on the device in fp32 with the weights of simple_vae_util.weights(seed)"""
    import lvae_amd as la
    import simple_vae_util as S
    from lvae_amd.vae import ConvVAE
    m = ConvVAE(L, 1296, p_input=0.0, p=0.0) if kind == "conv" else la.SimpleVAE(L, D)
    m = m.double()
    m.load_state_dict(S.weights(m, 100 + seed, fp32_exact=True), strict=True)
    return m.float().to(DEV)


def images(seed, P, T, data_seed):
    from lvae_amd.data import health_mnist_batch
    img, mask, X = health_mnist_batch(P, T, seed=data_seed, dtype=torch.float32)
    if seed != REAL:
        img = 1.0 - img   # (the decoy's images: still in [0, 1])
    return img.to(DEV), mask.to(DEV), X


def step_outputs(losses, *mods):
    out = {f"loss{j}": t for j, t in enumerate(losses)}
    for j, m in enumerate(mods):
        for n, p in m.named_parameters():
            if p.grad is not None:
                out[f"m{j}.{n}.grad"] = p.grad
    return out


# ------------------------------------------------------------------------------------------------------
# the rows
# ------------------------------------------------------------------------------------------------------
ROWS = {}


class Row:
    case = ""
    reaches = ()
    # a row off bit equality: the outputs named <prefix>.<one of ``loose``> are compared at ``tol`` (max-norm,
    # relative), every other output still to the bits; ``why`` names the kernel responsible
    bitwise, tol, why, loose = True, 0.0, None, ()
    no_power = ()   # floating outputs that need not move under the decoy: flags and state values
    abi = False   # True: the row calls the C ABI itself, with buffers of its own

    def declared(self, live):
        return [s.cuda_stream for k, s in live.items() if k.startswith("_stream")]

    def outputs(self, live):
        return live["_out"]


def register(cls):
    row = cls()
    row.name = cls.__name__
    ROWS[row.name] = row
    return cls


def _spec_full():
    import dubo_util as D
    from lvae_amd import _lib as P
    from oracle import lvae_oracle as O
    s = O.spec_full(**D.CFG)
    return P.make_spec(s), O.n_params(s)


def _cov(P, T, seed):
    from lvae_amd.data import health_mnist_covariates
    return torch.tensor(health_mnist_covariates(P, T, seed=seed))


@register
class gram_py(Row):
    case = "kernels.gram forward + adjoint, [3, 70, 37]: n1 past a 64-tile, n2 ragged"
    reaches = ("lvae_gram_f64", "lvae_gram_bwd_f64")

    def make(self, seed):
        import abi_util as U
        spec, n = _spec_full()
        X = decoy_x(seed, _cov(5, 16, 3), 16)
        p = vary(seed, "p", U.draw_hypers(np.random.default_rng(1), 3, n), "mul", 0.2).to(DEV).requires_grad_()
        G = vary(seed, "G", torch.ones(3, 70, 37, dtype=torch.float64), amp=0.9).to(DEV)
        return dict(p=p, x1=X[:70].to(DEV).contiguous(), x2=X[40:77].to(DEV).contiguous(), G=G, _spec=spec)

    def run(self, d):
        from lvae_amd.kernels import gram
        K = gram(d["_spec"], d["p"], d["x1"], d["x2"])
        d["_out"] = dict(K=K, **grads_of(K, [d["p"]], d["G"]))


@register
class gram_abi(Row):
    abi = True
    case = "C ABI, L = 3, n1 = 70, n2 = 37, the reference kernel: fp32 Gram, x2 adjoint, mat-vec, mat-vec by component"
    reaches = ("lvae_gram_f32", "lvae_gram_bwd_x2_f64", "lvae_gram_matvec_f64", "lvae_gram_matvec_comp_f64")

    def make(self, seed):
        import abi_util as U
        from lvae_amd import _lib as P
        lib = P.load()
        spec, n = _spec_full()
        L, n1, n2, Q = 3, 70, 37, 6
        X = decoy_x(seed, _cov(5, 16, 3), 16)
        nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=DEV)
        ws = lambda b: torch.zeros(int(b) + 256, dtype=torch.uint8, device=DEV)
        R = int(spec.n_comp)
        return dict(p=vary(seed, "p", U.draw_hypers(np.random.default_rng(1), L, n), "mul", 0.2).to(DEV),
                    x1=X[:n1].to(DEV).contiguous(), x2=X[40:40 + n2].to(DEV).contiguous(),
                    G=vary(seed, "G", torch.ones(L, n1, n2, dtype=torch.float64), amp=0.9).to(DEV),
                    v=vary(seed, "v", torch.ones(n2, L, dtype=torch.float64), amp=0.9).to(DEV),
                    _spec=spec, _dims=(L, n1, n2, Q, R),
                    _out=dict(K32=torch.full((L, n1, n2), float("nan"), dtype=torch.float32, device=DEV),
                              dx2=nan(L, n2, Q), mv=nan(n1, L), mvc=nan(R, n1, L)),
                    _ws=[ws(lib.lvae_gram_bwd_x2_workspace_size(1, L, n1, n2, Q)),
                         ws(lib.lvae_gram_matvec_workspace_size(n1, n2, L)),
                         ws(lib.lvae_gram_matvec_comp_workspace_size(n1, n2, L, R))])

    def run(self, d):
        from lvae_amd import _lib as P
        lib, st, ptr, o = P.lib(), P.stream_ptr(), P.ptr, d["_out"]
        L, n1, n2, Q, R = d["_dims"]
        sp = ctypes.byref(d["_spec"])
        v1, v2 = P.XView(d["x1"].data_ptr(), 0, 0, Q), P.XView(d["x2"].data_ptr(), 0, 0, Q)
        P.check(lib.lvae_gram_f32(sp, v1, v2, 1, L, n1, n2, ptr(d["p"]), None, ptr(o["K32"]), L * n1 * n2, n1 * n2, n2,
                                  st), "gram_f32")
        P.check(lib.lvae_gram_bwd_x2_f64(sp, v1, v2, 1, L, n1, n2, Q, ptr(d["p"]), ptr(d["G"]), L * n1 * n2, n1 * n2,
                                         n2, 1, ptr(o["dx2"]), ptr(d["_ws"][0]), st), "gram_bwd_x2")
        P.check(lib.lvae_gram_matvec_f64(sp, ptr(d["x1"]), Q, n1, ptr(d["x2"]), Q, n2, L, ptr(d["p"]), None,
                                         ptr(d["v"]), L, ptr(o["mv"]), L, ptr(d["_ws"][1]), st), "gram_matvec")
        P.check(lib.lvae_gram_matvec_comp_f64(sp, ptr(d["x1"]), Q, n1, ptr(d["x2"]), Q, 0, n2, L, ptr(d["p"]),
                                              ptr(d["v"]), L, ptr(o["mvc"]), L, n1 * L, ptr(d["_ws"][2]), st),
                "gram_matvec_comp")


class _linalg(Row):
    dtype = torch.float64

    def make(self, seed):
        A = spd_of(seed, "A", 2, 70).to(self.dtype)
        B = vary(seed, "B", torch.ones(2, 70, 5, dtype=torch.float64), amp=0.9).to(self.dtype)
        return dict(A=A.to(DEV), B=B.to(DEV))

    def run(self, d):
        from lvae_amd import linalg
        Lf, logdet, info = linalg.cholesky_ex(d["A"])
        d["_out"] = dict(Lf=Lf, logdet=logdet, info=info, trsm=linalg.solve_triangular(Lf, d["B"]),
                         trsm_t=linalg.solve_triangular(Lf, d["B"], transpose=True),
                         potrs=linalg.cholesky_solve(d["B"], Lf))


@register
class linalg_f64(_linalg):
    case = "linalg.cholesky_ex + both triangular solves + cholesky_solve, [2, 70, 70] x 5 columns (n past the 64 block)"
    reaches = ("lvae_potrf_f64", "lvae_trsm_f64", "lvae_potrs_f64")


@register
class linalg_f32(_linalg):
    case = "the same in fp32 (the exact KL's factorisation, fp64 solves on fp32 storage)"
    reaches = ("lvae_potrf_f32", "lvae_trsm_f32", "lvae_potrs_f32")
    dtype = torch.float32


@register
class small_f64(Row):
    case = "gpapprox.spd_inverse [5, 70, 70] and the batched small GEMM (3 x 2) x [70, 33] @ [33, 9]"
    reaches = ("lvae_spd_inv_small_f64", "lvae_gemm_small_f64")

    def make(self, seed):
        one = lambda *s: torch.ones(*s, dtype=torch.float64)
        return dict(A=spd_of(seed, "A", 5, 70).to(DEV), Ga=vary(seed, "Ga", one(3, 2, 70, 33), amp=0.9).to(DEV),
                    Gb=vary(seed, "Gb", one(3, 2, 33, 9), amp=0.9).to(DEV),
                    _C=torch.full((3, 2, 70, 9), float("nan"), dtype=torch.float64, device=DEV))

    def run(self, d):
        from lvae_amd import _lib as P
        from lvae_amd.gpapprox import spd_inverse
        Ai, ld = spd_inverse(d["A"])
        P.check(P.lib().lvae_gemm_small_f64(0, 0, 70, 9, 33, 1.5, P.ptr(d["Ga"]), 33, 2 * 70 * 33, 70 * 33,
                                            P.ptr(d["Gb"]), 9, 2 * 33 * 9, 33 * 9, 0.0, P.ptr(d["_C"]), 9, 2 * 70 * 9,
                                            70 * 9, 3, 2, P.stream_ptr()), "gemm_small")
        d["_out"] = dict(Ai=Ai, logdet=ld, C=d["_C"])


@register
class chol_inv(Row):
    abi = True
    case = ("lvae_spd_inv_chol_f32 at (n, L) = (512, 3), the smallest split order of test_gpu_trtri_early, its stream "
            "lent; a second delay on the lent stream makes the early trtri finish late")
    reaches = ("lvae_spd_inv_chol_f32",)

    def make(self, seed):
        import test_gpu_trtri_early as T
        from lvae_amd import _lib as P
        lib = T.lend()
        P.check(lib.lvae_set_early_stream(ctypes.c_void_p(T._LENT[0].cuda_stream)), "set_early_stream")
        n, L = 512, 3
        c = T.Call(lib, n, L)
        c.A.copy_(T.spd_case(n, L, 40 + seed)[1])
        c.scr.zero_()
        return dict(A=c.A, _call=c, _lent=T._LENT[0])

    def before_run(self, d, ms):
        with torch.cuda.stream(d["_lent"]):
            delay().enqueue(ms + 5.0)

    def run(self, d):
        d["_call"].enqueue()

    def outputs(self, d):
        c = d["_call"]
        return dict(Ainv=c.Ai, logdet=c.logdet, info=c.info)


class _kl(Row):
    n, L = 300, 3

    def problem(self, seed):
        import test_gpu_kl_closed_abi as K
        n, L = self.n, self.L
        g = torch.Generator().manual_seed(17)
        k, lik = full_modules(L, vary(seed, "raw", full_raw(L, 5)),
                              vary(seed, "nz", np.linspace(0.6, 1.0, L), "mul", 0.2))
        mu = vary(seed, "mu", torch.randn(n, L, generator=g, dtype=torch.float64), amp=0.5)
        lv = vary(seed, "lv", 0.1 * torch.randn(n, L, generator=g, dtype=torch.float64), amp=0.1)
        cot = vary(seed, "cot", torch.ones(L, dtype=torch.float64), amp=0.5)
        d = dict(x=decoy_x(seed, K.x_std(n), 16).to(DEV), mu=mu.to(DEV).requires_grad_(),
                 lv=lv.to(DEV).requires_grad_(), cot=cot.to(DEV), _k=k, _lik=lik)
        d.update(module_tensors("mod", k, lik))
        return d

    def leaves(self, d):
        return [d["mu"], d["lv"]] + params_of(d["_k"], d["_lik"])


@register
class kl_closed_300x3(_kl):
    case = ("KL_closed_batched forward + autograd.grad, n = 300, L = 3 (Np = 512, schedule (a)): the binned residual "
            "plan runs on the side stream (its state is asserted in kl_prefactor, which holds the workspace); "
            "lvae_kl_closed_hyper_state reports the binned hyper route")
    reaches = ("lvae_kl_closed_fwd_f32", "lvae_kl_closed_bwd_latent_f32", "lvae_kl_closed_bwd_hyper_f32",
               "lvae_kl_closed_hyper_state", "lvae_kl_closed_refine_state", "lvae_param_pack_fwd_f64",
               "lvae_param_pack_bwd_f64")

    def make(self, seed):
        return self.problem(seed)

    def run(self, d):
        import lvae_amd as la
        E = elbo_module()
        with E.kl_closed_hyper_log() as hl, E.kl_closed_refine_log() as rl:
            kl = la.KL_closed_batched(d["_k"], d["x"], d["_lik"], d["mu"], d["lv"])
        d["_out"] = dict(kl=kl, hyper_on=hl[0], est=rl[0][0], refined=rl[0][1],
                         **grads_of(kl, self.leaves(d), d["cot"]))

    no_power = ("est",)   # (the refinement gate's estimate: a state value)

    def verify(self, got):
        assert int(got["hyper_on"]) == 1, "lvae_kl_closed_hyper_state: not the binned hyper route"


@register
class kl_closed_255x2(kl_closed_300x3):
    case = "the same at n = 255, L = 2 (one 256 block, the pipelined schedule's small end): the binned hyper route"
    n, L = 255, 2


@register
class kl_closed_abi(Row):
    abi = True
    case = ("C ABI: lvae_kl_closed_fwd_f32 then the one-call backward lvae_kl_closed_bwd_f32 (the Python layer takes "
            "its two halves) at n = 300, L = 3, positive hyper-parameters")
    reaches = ("lvae_kl_closed_fwd_f32", "lvae_kl_closed_bwd_f32")

    def make(self, seed):
        import abi_util as U
        import test_gpu_kl_closed_abi as K
        from lvae_amd import _lib as P
        n, L = 300, 3
        spec, npar = _spec_full()
        g = torch.Generator().manual_seed(17)
        nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=DEV)
        return dict(x=decoy_x(seed, K.x_std(n), 16).to(DEV),
                    p=vary(seed, "p", U.draw_hypers(np.random.default_rng(2), L, npar), "mul", 0.2).to(DEV),
                    nz=vary(seed, "nz", torch.linspace(0.6, 1.0, L, dtype=torch.float64), "mul", 0.2).to(DEV),
                    mu=vary(seed, "mu", torch.randn(n, L, generator=g, dtype=torch.float64), amp=0.5).to(DEV),
                    lv=vary(seed, "lv", 0.1 * torch.randn(n, L, generator=g, dtype=torch.float64), amp=0.1).to(DEV),
                    gkl=vary(seed, "gkl", torch.ones(L, dtype=torch.float64), amp=0.5).to(DEV), _spec=spec,
                    _out=dict(kl=nan(L), dmu=nan(n, L), dlv=nan(n, L), dp=nan(L, npar), dnz=nan(L),
                              info=torch.zeros(L, dtype=torch.int32, device=DEV)),
                    _ws=torch.zeros(int(P.load().lvae_kl_closed_workspace_size(n, L)), dtype=torch.uint8, device=DEV))

    def run(self, d):
        from lvae_amd import _lib as P
        lib, p, o, sp, st = P.lib(), P.ptr, d["_out"], ctypes.byref(d["_spec"]), P.stream_ptr()
        n, L = d["mu"].shape
        P.check(lib.lvae_kl_closed_fwd_f32(sp, p(d["x"]), 6, n, L, p(d["p"]), p(d["nz"]), p(d["mu"]), p(d["lv"]), L,
                                           p(o["kl"]), p(o["info"]), p(d["_ws"]), 1, st), "kl_closed_fwd")
        P.check(lib.lvae_kl_closed_bwd_f32(sp, p(d["x"]), 6, n, L, p(d["p"]), p(d["mu"]), p(d["lv"]), L, p(d["gkl"]),
                                           p(o["dmu"]), p(o["dlv"]), p(o["dp"]), p(o["dnz"]), p(d["_ws"]), st),
                "kl_closed_bwd")


@register
class kl_prefactor(_kl):
    case = ("kl_closed_prefactor(..., stream=s2) + KL_closed_batched(factor=) + autograd.grad at n = 300, L = 3; s2 "
            "declared; lvae_kl_closed_resid_state on the factor's workspace reports the binned plan")
    reaches = ("lvae_kl_closed_factor_f32", "lvae_kl_closed_reduce_f32", "lvae_kl_closed_bwd_latent_f32",
               "lvae_kl_closed_bwd_hyper_f32", "lvae_kl_closed_resid_state")

    def make(self, seed):
        d = self.problem(seed)
        d["_stream2"] = torch.cuda.Stream()
        d["_flags"] = torch.full((2,), -1, dtype=torch.int32, device=DEV)
        return d

    def run(self, d):
        import lvae_amd as la
        from lvae_amd import _lib as P
        f = la.kl_closed_prefactor(d["_k"], d["x"], d["_lik"], self.L, d["_stream2"])
        kl = la.KL_closed_batched(d["_k"], d["x"], d["_lik"], d["mu"], d["lv"], factor=f)
        fl = d["_flags"]
        P.check(P.lib().lvae_kl_closed_resid_state(self.n, self.L, P.ptr(f.ws), P.ptr(fl),
                                                   ctypes.c_void_p(fl.data_ptr() + 4), P.stream_ptr()), "resid_state")
        d["_out"] = dict(kl=kl, resid=fl, **grads_of(kl, self.leaves(d), d["cot"]))

    def verify(self, got):
        flags = got["resid"].tolist()
        assert flags == [2, 1], f"lvae_kl_closed_resid_state (covflag, binned) = {flags}"


class _inducing(Row):
    """the inducing-point bounds on a dubo_util case"""
    cid, T = "6x7x33", 7

    def problem(self, seed, z_grad=False):
        import dubo_util as D
        c = varied_problem(D.problem(self.cid), seed, self.T)
        k0, k1, lik = split_modules(c)
        d = dict(x=c["X"].to(DEV), z=c["Z"].to(DEV).requires_grad_(z_grad), mu=c["mu"].to(DEV).requires_grad_(),
                 lv=c["lv"].to(DEV).requires_grad_(),
                 cot=vary(seed, "cot", torch.ones(D.L, dtype=torch.float64), amp=0.5).to(DEV), _k0=k0, _k1=k1,
                 _lik=lik, _c=c)
        d.update(module_tensors("mod", k0, k1, lik))
        return d

    def leaves(self, d):
        return [d["mu"], d["lv"]] + ([d["z"]] if d["z"].requires_grad else []) + params_of(d["_k0"], d["_k1"],
                                                                                             d["_lik"])


def _ragged(c):
    """rows of a [P, T] problem with a few dropped, so that the subjects differ in length"""
    keep = torch.ones(c["P"] * c["T"], dtype=torch.bool)
    keep[[2, 9, 10, 11, 30]] = False
    return keep


@register
class hensman(_inducing):
    case = ("minibatch_KLD_upper_bound (natural gradient) forward + autograd.grad with a z that requires grad, then "
            "natural_gradient_update, on dubo_util 6x7x33 (M = 33 past two MFMA tiles)")
    reaches = ("lvae_hensman_fwd_part_f64", "lvae_hensman_bwd_f64", "lvae_hensman_bwd_z_f64",
               "lvae_natgrad_update_f64")
    prior, z_grad = False, True

    def make(self, seed):
        import dubo_util as D
        d = self.problem(seed, self.z_grad)
        M = d["_c"]["M"]
        d["m"] = vary(seed, "m", torch.zeros(D.L, M, 1, dtype=torch.float64), amp=0.7).to(DEV)
        d["H"] = spd_of(seed, "H", D.L, M, 10.0).to(DEV)
        d["cot"] = d["cot"][:1].reshape(()).clone()
        if self.prior:
            d["_stream2"] = torch.cuda.Stream()
        return d

    def run(self, d):
        import dubo_util as D
        import lvae_amd as la
        from lvae_amd.elbo import minibatch_KLD_upper_bound, natural_gradient_update
        c = d["_c"]
        args = (d["_k0"], d["_k1"], d["_lik"], D.L, d["m"], d["H"], d["x"])
        tail = dict(P_tot=2 * c["P"], P_batch=c["P"], T=c["T"], natural_gradient=True, eps=D.EPS)
        prior = la.HensmanPrior(*args, d["z"], **tail, stream=d["_stream2"]) if self.prior else None
        kld, gm, gH = minibatch_KLD_upper_bound(*args, d["mu"], d["lv"], d["z"], 2 * c["P"], c["P"], c["T"], True,
                                                D.EPS, prior=prior)
        m2, H2 = natural_gradient_update(d["m"], d["H"], gm, gH, 0.01)
        d["_out"] = dict(kld=kld, gm=gm, gH=gH, m2=m2, H2=H2, **grads_of(kld, self.leaves(d), d["cot"]))


@register
class hensman_prior(hensman):
    case = "the same with prior=HensmanPrior(..., stream=s2), s2 declared (parts 1 and 2 of the forward); z fixed"
    reaches = ("lvae_hensman_fwd_part_f64", "lvae_hensman_bwd_f64", "lvae_natgrad_update_f64")
    prior, z_grad = True, False


@register
class hensman_abi(Row):
    abi = True
    case = "lvae_hensman_fwd_f64 (the one-call forward, which the Python layer never takes) on dubo_util 6x7x33"
    reaches = ("lvae_hensman_fwd_f64",)

    def make(self, seed):
        import dubo_util as D
        from lvae_amd import _lib as P
        c, s0, s1, _, t = D.abi_inputs(varied_problem_abi(seed))
        L, M = D.L, c["M"]
        dims = P.HensmanDims(L, M, c["P"], c["T"], 6, 2.0 * c["P"], D.EPS, 1, 1.0)
        nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=DEV)
        t = dict(t, m=vary(seed, "m", torch.zeros(L, M, dtype=torch.float64), amp=0.7).to(DEV),
                 H=spd_of(seed, "H", L, M, 10.0).to(DEV))
        t.update(_spec=(s0, s1), _dims=dims, _out=dict(kld=nan(1), gm=nan(L, M), gH=nan(L, M, M)),
                 _info=torch.zeros(L, dtype=torch.int32, device=DEV),
                 _ws=torch.zeros(int(P.load().lvae_hensman_workspace_size(ctypes.byref(dims))) + 256,
                                 dtype=torch.uint8, device=DEV))
        return t

    def run(self, d):
        from lvae_amd import _lib as P
        p, o, (s0, s1) = P.ptr, d["_out"], d["_spec"]
        P.check(P.lib().lvae_hensman_fwd_f64(ctypes.byref(s0), ctypes.byref(s1), ctypes.byref(d["_dims"]), p(d["x"]),
                                             p(d["z"]), p(d["m"]), p(d["H"]), p(d["mu"]), p(d["lv"]), p(d["p0"]),
                                             p(d["p1"]), p(d["noise"]), p(o["kld"]), p(o["gm"]), p(o["gH"]),
                                             p(d["_info"]), p(d["_ws"]), P.stream_ptr()), "hensman_fwd")


def varied_problem_abi(seed, cid="6x7x33", T=7):
    """dubo_util.abi_inputs' problem form (positive p0 / p1) of a varied case"""
    import dubo_util as D
    from oracle import lvae_oracle as O
    c = varied_problem(D.problem(cid), seed, T)
    c["p0"], c["p1"] = O.constrain(torch.tensor(c["raw0"])), O.constrain(torch.tensor(c["raw1"]))
    return c


@register
class dubo(_inducing):
    case = "deviance_upper_bound_batched forward + autograd.grad (z requires grad) on dubo_util 6x7x33: the fused pass"
    reaches = ("lvae_dubo_fwd_f64", "lvae_dubo_bwd_f64", "lvae_dubo_bwd_z_f64")

    def make(self, seed):
        return self.problem(seed, True)

    def run(self, d):
        import dubo_util as D
        import lvae_amd as la
        c = d["_c"]
        v = la.deviance_upper_bound_batched(D.L, d["_k0"], d["_k1"], d["_lik"], d["x"], d["mu"], d["lv"], d["z"],
                                            c["P"], c["T"], D.EPS)
        d["_out"] = dict(dubo=v, **grads_of(v, self.leaves(d), d["cot"]))


@register
class dubo_T33(dubo):
    case = "the same on 3x33x17: T past the fused pass, the batched-product route"
    cid, T = "3x33x17", 33


class _seg(_inducing):
    def make(self, seed):
        from lvae_amd.gpapprox import subject_layout
        d = self.problem(seed, False)
        keep = _ragged(d["_c"])
        for k in ("x", "mu", "lv"):
            d[k] = d[k].detach()[keep.to(DEV)].contiguous().requires_grad_(k != "x")
        d["_layout"] = subject_layout(d["x"][:, 2])
        d["gather"], d["seg_len"] = d["_layout"].gather, d["_layout"].seg_len
        return d


@register
class dubo_seg(_seg):
    case = "deviance_upper_bound_varying_T on 6x7x33 with five rows dropped (subjects of 4 to 7 rows), its layout given"
    reaches = ("lvae_dubo_fwd_seg_f64", "lvae_dubo_bwd_seg_f64")

    def run(self, d):
        import dubo_util as D
        import lvae_amd as la
        v = la.gpapprox.deviance_upper_bound_varying_T(D.L, d["_k0"], d["_k1"], d["_lik"], d["x"], d["mu"], d["lv"],
                                                       d["z"], 2, D.EPS, layout=d["_layout"])
        d["_out"] = dict(dubo=v, **grads_of(v, self.leaves(d), d["cot"]))


@register
class elbo(_inducing):
    case = "elbo_batched with S = 3 samples, forward + autograd.grad (z requires grad), on dubo_util 6x7x33"
    reaches = ("lvae_gp_elbo_fwd_f64", "lvae_gp_elbo_bwd_f64", "lvae_gp_elbo_bwd_z_f64")
    S = 3

    def make(self, seed):
        d = self.problem(seed, True)
        self.samples(d, seed)
        return d

    def samples(self, d, seed):
        import dubo_util as D
        n = d["mu"].shape[0]
        g = torch.Generator().manual_seed(23)
        y = vary(seed, "y", torch.randn(self.S, n, D.L, generator=g, dtype=torch.float64), amp=0.5)
        d["y"] = y.to(DEV).requires_grad_()
        d["cot2"] = vary(seed, "cot2", torch.ones(self.S, D.L, dtype=torch.float64), amp=0.5).to(DEV)

    def run(self, d):
        import dubo_util as D
        import lvae_amd as la
        c = d["_c"]
        v = la.gpapprox.elbo_batched(D.L, d["_k0"], d["_k1"], d["_lik"], d["x"], d["y"], d["z"], c["P"], c["T"], D.EPS)
        d["_out"] = dict(elbo=v, **grads_of(v, [d["y"]] + self.leaves(d)[2:], d["cot2"]))


@register
class elbo_seg(_seg, elbo):
    case = "elbo_varying_T with S = 3 on the ragged 6x7x33, its layout given"
    reaches = ("lvae_gp_elbo_fwd_seg_f64", "lvae_gp_elbo_bwd_seg_f64")

    def make(self, seed):
        d = _seg.make(self, seed)
        self.samples(d, seed)
        return d

    def run(self, d):
        import dubo_util as D
        import lvae_amd as la
        v = la.gpapprox.elbo_varying_T(D.L, d["_k0"], d["_k1"], d["_lik"], d["x"], d["y"], d["z"], 2, D.EPS,
                                       layout=d["_layout"])
        d["_out"] = dict(elbo=v, **grads_of(v, [d["y"]] + self.leaves(d)[2:], d["cot2"]))


@register
class dubo_cond(Row):
    case = ("lvae_dubo_cond_prepare_f64 (gpapprox._condition, below condition_dubo's host work) then the conditioned "
            "bound and its gradient, dubo_util 6x7x33 with subjects 1 and 4 new")
    reaches = ("lvae_dubo_cond_prepare_f64", "lvae_dubo_cond_eval_f64")

    def make(self, seed):
        import dubo_util as D
        c, s0, s1, dims, t = D.abi_inputs(varied_problem_abi(seed))
        Pn, T = 2, c["T"]
        one = torch.ones(Pn * T, D.L, dtype=torch.float64)
        return dict(t, m_new=vary(seed, "mn", 0.0 * one, amp=0.8).to(DEV).requires_grad_(),
                    lv_new=vary(seed, "ln", 0.0 * one, amp=0.2).to(DEV).requires_grad_(),
                    cot=vary(seed, "cot", torch.ones(D.L, dtype=torch.float64), amp=0.5).to(DEV),
                    free=torch.tensor([1, 4], dtype=torch.int32, device=DEV), _spec=(s0, s1), _c=c)

    def run(self, d):
        import dubo_util as D
        from lvae_amd import gpapprox as G
        c, (s0, s1) = d["_c"], d["_spec"]
        state, Pn = G._condition(D.L, s0, d["p0"], s1, d["p1"], d["z"], d["noise"], d["x"], d["mu"], d["lv"], c["P"],
                                 c["T"], None, d["free"], D.EPS)
        v = G.DuboCondition(D.L, Pn, c["T"], Pn * c["T"], state)(d["m_new"], d["lv_new"])
        d["_out"] = dict(val=v, **grads_of(v, [d["m_new"], d["lv_new"]], d["cot"]))


def _kl_cond_problem(seed, cid="70+33"):
    """kl_cond_util's case with varied values: (modules, xn, xt, mu_t, lv_t, mu_n, lv_n)"""
    import kl_cond_util as C
    c = C.problem(cid)
    k, lik = full_modules(C.L, vary(seed, "raw", c["raw"]), vary(seed, "nz", c["noise"], "mul", 0.2))
    T = CASE_T[cid]
    f = lambda key, amp: vary(seed, key, c[key], amp=amp).to(DEV)
    d = dict(xn=decoy_x(seed, c["xn"], T).to(DEV), xt=decoy_x(seed, c["xt"], T).to(DEV), mu_t=f("mu_t", 0.5),
             lv_t=f("lv_t", 0.1), mu_n=f("mu_n", 0.5).requires_grad_(), lv_n=f("lv_n", 0.1).requires_grad_(),
             cot=vary(seed, "cot", torch.ones(C.L, dtype=torch.float64), amp=0.5).to(DEV), _k=k, _lik=lik)
    d.update(module_tensors("mod", k, lik))
    return d


CASE_T = {"70+33": 11}


@register
class kl_cond(Row):
    case = "condition_kl_closed (lvae_kl_cond_prepare_f64) then the conditioned KL and its gradient, kl_cond_util 70+33"
    reaches = ("lvae_kl_cond_prepare_f64", "lvae_dubo_cond_eval_f64")

    def make(self, seed):
        return _kl_cond_problem(seed)

    def run(self, d):
        from lvae_amd.kl_cond import condition_kl_closed
        cond = condition_kl_closed(d["_k"], d["_lik"], d["xn"], d["xt"], d["mu_t"], d["lv_t"])
        v = cond(d["mu_n"], d["lv_n"])
        d["_out"] = dict(val=v, **grads_of(v, [d["mu_n"], d["lv_n"]], d["cot"]))


@register
class predict_exact(Row):
    case = ("predict_exact (mean; variance in two test-row chunks) and predict_exact_components (means; covariance in "
            "two chunks) on kl_cond_util 70+33: 70 prediction rows, 33 test rows")
    reaches = ("lvae_predict_exact_f64", "lvae_predict_exact_var_f64", "lvae_predict_exact_comp_f64",
               "lvae_predict_exact_comp_cov_f64")

    def make(self, seed):
        from lvae_amd import _lib as P
        lib = P.load()
        d = _kl_cond_problem(seed)
        n, nt, L = 70, 33, 3
        R = int(_spec_full()[0].n_comp)
        d["_cap"] = (int(lib.lvae_predict_exact_var_workspace_size(n, nt, L, nt)) - 1,
                     int(lib.lvae_predict_exact_comp_cov_workspace_size(n, nt, L, R, nt)) - 1)
        return d

    def run(self, d):
        import lvae_amd.predict as Pr
        a = (d["_k"], d["_lik"], d["xt"], d["xn"], d["mu_t"])
        mean = Pr.predict_exact(*a)
        mean2, var = Pr.predict_exact(*a, return_var=True, add_noise=True, max_workspace_bytes=d["_cap"][0])
        mean3, comp = Pr.predict_exact_components(*a)
        mean4, cc = Pr.predict_exact_components(*a, return_cov=True, max_workspace_bytes=d["_cap"][1])
        d["_out"] = dict(mean=mean, mean2=mean2, var=var, mean3=mean3, comp=comp.values, mean4=mean4, comp4=cc.values,
                         ccov=cc.cov)


@register
class predict_exact_cov(Row):
    abi = True
    case = ("lvae_predict_exact_cov_f64 through predict._exact_run (below predict_exact's host grouping) in two chunks "
            "of whole groups, then lvae_predict_sample_f64 with S = 2 draws; 70 + 33 rows, the test subjects the "
            "groups")
    reaches = ("lvae_predict_exact_cov_f64", "lvae_predict_sample_f64")

    def make(self, seed):
        import lvae_amd.predict as Pr
        from lvae_amd import _lib as P
        lib = P.load()
        d = _kl_cond_problem(seed)
        nt, L, n = 33, 3, 70
        order, ids, counts, start, n_max = Pr._row_groups(d["xn"][:, 2].cpu(), "row")
        G = int(ids.numel())
        d["xn"] = d["xn"][order.to(DEV)].contiguous()
        d["eps"] = vary(seed, "eps", torch.zeros(2, nt, L, dtype=torch.float64), amp=1.0).to(DEV)
        d["index"] = Pr._group_index(torch.arange(nt), counts, start, n_max, DEV)
        d["_g"] = (G, n_max, (ctypes.c_int32 * (G + 1))(*start.tolist()))
        d["_cap"] = int(lib.lvae_predict_exact_cov_workspace_size(n, nt, L, nt)) - 1
        d["_ws"] = torch.zeros(int(lib.lvae_predict_sample_workspace_size(L, G, n_max)) + 256, dtype=torch.uint8,
                               device=DEV)
        return d

    def run(self, d):
        import lvae_amd.predict as Pr
        from lvae_amd import _lib as P
        lib, ptr = P.lib(), P.ptr
        G, n_max, start_h = d["_g"]
        a = Pr._exact_inputs(d["_k"], d["_lik"], d["xt"], d["xn"], d["mu_t"])
        L, nt, n = a.L, a.nt, a.n
        mean = torch.empty(nt, L, dtype=torch.float64, device=DEV)
        blocks = torch.empty(L, G, n_max, n_max, dtype=torch.float64, device=DEV)
        Pr._exact_run(lib, a, a.tx, d["_cap"], lambda g, c: int(lib.lvae_predict_exact_cov_workspace_size(n, nt, g, c)),
                      lib.lvae_predict_exact_cov_f64, "predict_exact_cov",
                      lambda at, l0, c: (G, ctypes.cast(start_h, ctypes.c_void_p), n_max, at(mean, l0), L,
                                         at(blocks, l0 * G * n_max * n_max), 1, c), floor=n_max)
        draws = torch.empty(2, nt, L, dtype=torch.float64, device=DEV)
        info = torch.empty(L * G, dtype=torch.int32, device=DEV)
        P.check(lib.lvae_predict_sample_f64(L, G, n_max, nt, 2, ptr(blocks), ptr(d["index"]), ptr(mean), ptr(d["eps"]),
                                            1e-8, ptr(draws), ptr(info), ptr(d["_ws"]), P.stream_ptr()),
                "predict_sample")
        d["_out"] = dict(mean=mean, blocks=blocks, draws=draws, info=info)


@register
class predict_inducing(Row):
    abi = True
    case = ("the five inducing-route predictors on predict._inducing_inputs' arguments (below the wrappers' host "
            "layout): ragged 6x7x33 as the prediction set, 14 test rows of three of its subjects and one unseen")
    reaches = ("lvae_predict_f64", "lvae_predict_var_f64", "lvae_predict_cov_f64", "lvae_predict_comp_f64",
               "lvae_predict_comp_cov_f64")
    KEYS = ("p0", "p1", "z", "noise", "x_pad", "mu_pad", "tx", "seg", "inc")

    def make(self, seed):
        import dubo_util as D
        import lvae_amd.predict as Pr
        c = varied_problem(D.problem("6x7x33"), seed, 7)
        k0, k1, lik = split_modules(c)
        keep = _ragged(c)
        x = c["X"][keep]
        tx = torch.cat([c["X"][[8, 12, 13, 15, 16, 29, 31, 34, 35, 36]], c["X"][[1, 3, 4, 5]]])
        tx[:, 0] += 0.5
        tx[-4:, 2] = 9.0
        with torch.no_grad():
            a = Pr._inducing_inputs(D.L, k0, k1, lik, x.to(DEV), tx.to(DEV), c["mu"][keep].to(DEV), c["Z"].to(DEV), 2,
                                    D.EPS)
        g = Pr._subject_groups(tx[:, 2], a.pred_ids, "row", Pr.MAX_GROUP_ROWS)
        a.tx = a.tx[g.order.to(DEV)].contiguous()
        d = {k: getattr(a, k) for k in self.KEYS}
        d.update(subj=g.subj.to(DEV), start=g.start.to(DEV), _a=a, _g=g, _mods=(k0, k1, lik))
        return d

    def run(self, d):
        from lvae_amd import _lib as P
        lib, ptr, a, g = P.lib(), P.ptr, d["_a"], d["_g"]
        L, M, Pp, T, Nt = a.L, a.M, a.P, a.T, a.Nt
        R0, R1 = int(a.spec0.n_comp), int(a.spec1.n_comp)
        R = R0 + R1
        new = lambda *s: torch.empty(*s, dtype=torch.float64, device=DEV)
        wsb = lambda b: torch.empty(int(b), dtype=torch.uint8, device=DEV)
        info = torch.empty(5, L, dtype=torch.int32, device=DEV)
        inf = lambda j: ctypes.c_void_p(info.data_ptr() + 4 * L * j)
        st = P.stream_ptr()
        head, par, groups = a.head(ptr(a.tx), Nt), a.params(), (g.G, ptr(d["subj"]), ptr(d["start"]))
        o = dict(mean=new(Nt, L), mean_v=new(Nt, L), var=new(Nt, L), mean_c=new(Nt, L),
                 blocks=new(L, g.G, g.n_max, g.n_max), mean_s=new(Nt, L), vals=new(R, Nt, L), mean_cc=new(Nt, L),
                 vals_cc=new(R, Nt, L), ccov=new(L, Nt, R, R), info=info)
        P.check(lib.lvae_predict_f64(*head, *par, ptr(o["mean"]), inf(0),
                                     ptr(wsb(lib.lvae_predict_workspace_size(L, M, Pp, T, Nt))), st), "predict")
        P.check(lib.lvae_predict_var_f64(*head, *groups, *par, ptr(o["mean_v"]), ptr(o["var"]), 1, inf(1),
                                         ptr(wsb(lib.lvae_predict_var_workspace_size(L, M, Pp, T, Nt))), st),
                "predict_var")
        P.check(lib.lvae_predict_cov_f64(*head, *groups, g.n_max, *par, ptr(o["mean_c"]), ptr(o["blocks"]), 0, inf(2),
                                         ptr(wsb(lib.lvae_predict_cov_workspace_size(L, M, Pp, T, Nt))), st),
                "predict_cov")
        P.check(lib.lvae_predict_comp_f64(*head, *par, ptr(o["mean_s"]), ptr(o["vals"]), L, Nt * L, inf(3),
                                          ptr(wsb(lib.lvae_predict_comp_workspace_size(L, M, Pp, T, Nt, R0, R1))), st),
                "predict_comp")
        P.check(lib.lvae_predict_comp_cov_f64(*head, *groups, *par, ptr(o["mean_cc"]), ptr(o["vals_cc"]), L, Nt * L,
                                              ptr(o["ccov"]), inf(4),
                                              ptr(wsb(lib.lvae_predict_comp_cov_workspace_size(L, M, Pp, T, Nt, R0,
                                                                                               R1))), st),
                "predict_comp_cov")
        d["_out"] = o


class _vae(Row):
    kind, L, B, Dm = "conv", 3, 5, None

    def make(self, seed):
        vae = vae_of(self.kind, self.L, seed, self.Dm)
        img, mask, _ = images(seed, 1, self.B, 31)
        if self.kind != "conv":
            flat = lambda t: t.reshape(self.B, -1)[:, :self.Dm].contiguous()
            img, mask = flat(img), flat(mask)
        eps = vary(seed, "eps", torch.zeros(self.B, self.L), amp=1.0).to(DEV)
        d = dict(img=img, mask=mask, eps=eps, _vae=vae)
        d.update(module_tensors("vae", vae))
        return d

    def run(self, d):
        import simple_vae_util as S
        vae = d["_vae"]
        loss, out = S.loss_of(vae, d["img"], d["mask"], d["eps"])
        d["_out"] = dict(loss=loss, **out, **named_grads(loss, vae, "vae"))


@register
class conv_vae(MiopenWgrad, _vae):
    case = "ConvVAE forward + backward of simple_vae_util.loss_of at B = 5 (below 512 images: MIOpen's conv backward)"
    reaches = ("lvae_conv1_relu_maxpool2_fwd_f32", "lvae_conv3x3_relu_maxpool2_fwd_f32", "lvae_bias_relu_fwd_f32",
               "lvae_act_bwd_f32", "lvae_deconv4s2_relu_fwd_f32", "lvae_deconv4s2_relu_bwd_f32",
               "lvae_deconv2_sigmoid_fwd_f32", "lvae_deconv2_sigmoid_bwd_f32", "lvae_relu_maxpool2_bias_bwd_f32",
               "lvae_reparam_fwd_f32", "lvae_reparam_bwd_f32", "lvae_vae_loss_fwd_f32", "lvae_vae_loss_bwd_f32")


@register
class simple_vae(_vae):
    case = "the fused SimpleVAE forward + backward of simple_vae_util.loss_of at B = 5, D = 48, L = 4, hidden (300, 30)"
    reaches = ("lvae_mlp_enc_fwd_f32", "lvae_mlp_dec_fwd_f32", "lvae_mlp_dec_bwd_f32", "lvae_mlp_enc_bwd_f32",
               "lvae_vae_loss_fwd_f32", "lvae_vae_loss_bwd_f32")
    kind, L, Dm = "mlp", 4, 48


@register
class pool_ops(MiopenWgrad, Row):
    loose = ("weight.grad",)   # (conv.weight.grad: the row's one module is the 8 -> 16 conv)
    case = ("vae.relu_maxpool2 on [5, 3, 10, 14] and vae.conv_relu_maxpool2 with an 8 -> 16 conv on [5, 8, 10, 14] "
            "(neither of the ConvVAE's fused shapes: MIOpen's conv + the bias / relu / pool pass), forward + backward")
    reaches = ("lvae_relu_maxpool2_fwd_f32", "lvae_relu_maxpool2_bwd_f32", "lvae_relu_maxpool2_bias_fwd_f32",
               "lvae_relu_maxpool2_bias_bwd_f32")

    def make(self, seed):
        import simple_vae_util as S
        conv = torch.nn.Conv2d(8, 16, 3, 1, 1).double()
        conv.load_state_dict(S.weights(conv, 60 + seed, fp32_exact=True))
        conv = conv.float().to(DEV)
        g = torch.Generator().manual_seed(3)
        xa = vary(seed, "xa", torch.randn(5, 3, 10, 14, generator=g), amp=0.7)
        xb = vary(seed, "xb", torch.randn(5, 8, 10, 14, generator=g), amp=0.7)
        d = dict(xa=xa.to(DEV).requires_grad_(), xb=xb.to(DEV).requires_grad_(), _conv=conv)
        d.update(module_tensors("conv", conv))
        return d

    def run(self, d):
        from lvae_amd import vae as V
        ya = V.relu_maxpool2(d["xa"])
        yb = V.conv_relu_maxpool2(d["_conv"], d["xb"])
        loss = (ya * ya).sum() + (yb * yb).sum()
        d["_out"] = dict(ya=ya, yb=yb, **named_grads(loss, d["_conv"], "conv", [d["xa"], d["xb"]]))


class _step(Row):
    """the training steps on dubo_util 6x7x33 with its images: losses and every gradient"""
    no_power = ("m0._log_vy.grad",)   # (exact zeros under the 'mse' loss, whatever the inputs)

    def base(self, seed, z_param=False):
        import dubo_util as D
        c = varied_problem(D.problem("6x7x33"), seed, 7)
        k0, k1, lik = split_modules(c)
        vae = vae_of("conv", D.L, seed)
        img, mask, _ = images(seed, c["P"], c["T"], 306)
        z = torch.nn.Parameter(c["Z"].to(DEV)) if z_param else c["Z"].to(DEV)
        eps = vary(seed, "eps", torch.zeros(c["N"], D.L), amp=1.0).to(DEV)
        d = dict(img=img, mask=mask, x=c["X"].to(DEV), eps=eps, z=z.data, _z=z, _vae=vae, _k0=k0, _k1=k1, _lik=lik,
                 _c=c)
        d.update(module_tensors("mod", vae, k0, k1, lik))
        return d

    def opt(self, d, extra=()):
        ps = params_of(d["_vae"], d["_k0"], d["_k1"], d["_lik"]) + list(extra)
        return torch.optim.SGD(ps, lr=0.0)


@register
class closed_step(Row):
    case = ("ClosedStep.forward_backward at test_closed_step_vs_oracle's shape (1024 images, L = 4): the factor from "
            "the worker thread on the caller's stream; its ConvVAE stream and the weight gradient's side stream "
            "declared")
    reaches = ("lvae_kl_closed_factor_f32", "lvae_kl_closed_reduce_f32", "lvae_kl_closed_bwd_latent_f32",
               "lvae_kl_closed_bwd_hyper_f32", "lvae_vae_loss_fwd_f32", "lvae_vae_loss_bwd_f32",
               "lvae_reparam_fwd_f32", "lvae_reparam_bwd_f32", "lvae_param_pack_fwd_f64", "lvae_param_pack_bwd_f64",
               "lvae_conv3x3_pool_wgrad_f32", "lvae_conv3x3_pool_dgrad_f32")

    no_power = ("m0._log_vy.grad",)   # (exact zeros under the 'mse' loss, whatever the inputs)

    def make(self, seed):
        from lvae_amd.steps import ClosedStep
        L, P, T = 4, 64, 16
        img, mask, X = images(seed, P, T, 8)
        vae = vae_of("conv", L, seed)
        k, lik = full_modules(L, vary(seed, "raw", full_raw(L, 8)), np.ones(L))
        eps = vary(seed, "eps", torch.zeros(P * T, L), amp=1.0).to(DEV)
        opt = torch.optim.SGD(params_of(vae, k, lik), lr=0.0)
        d = dict(img=img, mask=mask, x=decoy_x(seed, X, T).to(DEV), eps=eps, _vae=vae, _k=k, _lik=lik,
                 _step=ClosedStep(vae, k, lik, opt, weight=0.15, loss_function="mse"))
        d.update(module_tensors("mod", vae, k, lik))
        return d

    def run(self, d):
        d["_losses"] = d["_step"].forward_backward(d["img"], d["mask"], d["x"], d["eps"])

    def outputs(self, d):
        return step_outputs(d["_losses"], d["_vae"], d["_k"], d["_lik"])

    def declared(self, d):
        from lvae_amd import vae as V
        return [d["_step"]._vae_stream.cuda_stream, V._side_stream(d["img"].device).cuda_stream]


@register
class hensman_step(MiopenWgrad, _step):
    case = "HensmanStep.forward_backward + apply (natural-gradient update in place), 6 subjects x 7 rows, M = 33"
    reaches = ("lvae_hensman_fwd_part_f64", "lvae_hensman_bwd_f64", "lvae_natgrad_update_f64", "lvae_step_terms_fwd",
               "lvae_step_terms_bwd", "lvae_param_pack_fwd_f64", "lvae_param_pack_bwd_f64", "lvae_reparam_fwd_f32",
               "lvae_vae_loss_fwd_f32")

    def make(self, seed):
        import dubo_util as D
        from lvae_amd.steps import HensmanStep
        d = self.base(seed)
        M = d["_c"]["M"]
        d["m"] = vary(seed, "m", torch.zeros(D.L, M, 1, dtype=torch.float64), amp=0.7).to(DEV)
        d["H"] = spd_of(seed, "H", D.L, M, 10.0).to(DEV)
        d["_step"] = HensmanStep(d["_vae"], d["_k0"], d["_k1"], d["_lik"], self.opt(d), d["m"], d["H"], d["z"],
                                 2 * d["_c"]["P"], d["_c"]["T"])
        return d

    def run(self, d):
        st = d["_step"]
        losses = st.forward_backward(d["img"], d["mask"], d["x"], d["eps"])
        d["_o"] = step_outputs(losses, d["_vae"], d["_k0"], d["_k1"], d["_lik"])
        st.apply()
        d["_o"].update(m=st.m, H=st.H)

    def outputs(self, d):
        return d["_o"]


@register
class dubo_step(MiopenWgrad, _step):
    case = "DuboStep.forward_backward with z an nn.Parameter, 6 subjects x 7 rows, M = 33"
    reaches = ("lvae_dubo_fwd_f64", "lvae_dubo_bwd_f64", "lvae_dubo_bwd_z_f64", "lvae_vae_loss_bwd_f32",
               "lvae_reparam_bwd_f32")
    cls = "DuboStep"

    def make(self, seed):
        from lvae_amd import steps
        d = self.base(seed, True)
        d["_step"] = getattr(steps, self.cls)(d["_vae"], d["_k0"], d["_k1"], d["_lik"], self.opt(d, [d["_z"]]),
                                              d["_z"], d["_c"]["T"], **self.extra(d, seed))
        return d

    def extra(self, d, seed):
        return {}

    def call(self, d):
        return d["_step"].forward_backward(d["img"], d["mask"], d["x"], d["eps"])

    def run(self, d):
        d["_losses"] = self.call(d)

    def outputs(self, d):
        o = step_outputs(d["_losses"], d["_vae"], d["_k0"], d["_k1"], d["_lik"])
        o["z.grad"] = d["_z"].grad
        return o


@register
class elbo_step(dubo_step):
    case = "ElboStep.forward_backward with num_samples = 2 and z an nn.Parameter, the same problem"
    reaches = ("lvae_gp_elbo_fwd_f64", "lvae_gp_elbo_bwd_f64", "lvae_gp_elbo_bwd_z_f64")
    cls = "ElboStep"

    def extra(self, d, seed):
        import dubo_util as D
        d["eps_gp"] = vary(seed, "eps_gp", torch.zeros(2, d["_c"]["N"], D.L), amp=1.0).to(DEV)
        return dict(num_samples=2)

    def call(self, d):
        return d["_step"].forward_backward(d["img"], d["mask"], d["x"], d["eps"], d["eps_gp"])


@register
class latent_inference_step(Row):
    case = ("one LatentInferenceStep iteration (forward_backward; Adam's moments are host-side state, not inputs) on "
            "a condition_dubo state of 6x7x33 with its first two subjects new; the state is prepared beforehand and is one of the row's inputs")
    reaches = ("lvae_dubo_cond_eval_f64", "lvae_reparam_fwd_f32", "lvae_reparam_bwd_f32", "lvae_vae_loss_fwd_f32",
               "lvae_vae_loss_bwd_f32")

    def make(self, seed):
        import dubo_util as D
        import lvae_amd as la
        from lvae_amd.steps import LatentInferenceStep
        c = varied_problem(D.problem("6x7x33"), seed, 7)
        k0, k1, lik = split_modules(c)
        vae = vae_of("conv", D.L, seed)
        nn_ = 2 * c["T"]
        img, mask, _ = images(seed, 2, c["T"], 306)
        to = lambda t: t.to(DEV)
        with torch.no_grad():
            cond = la.gpapprox.condition_dubo(D.L, k0, k1, lik, to(c["X"][:nn_]), to(c["X"][nn_:]), to(c["mu"][nn_:]),
                                              to(c["lv"][nn_:]), to(c["Z"]), c["T"], D.EPS)
        torch.cuda.synchronize()
        mu, lv = torch.nn.Parameter(to(c["mu"][:nn_])), torch.nn.Parameter(to(c["lv"][:nn_]))
        opt = torch.optim.Adam([{"params": mu}, {"params": lv}], lr=1e-2)
        d = dict(img=img, mask=mask, eps=vary(seed, "eps", torch.zeros(nn_, D.L), amp=1.0).to(DEV), state=cond.state,
                 mu=mu.data, lv=lv.data, _mu=mu, _lv=lv, _vae=vae,
                 _step=LatentInferenceStep(vae, cond, mu, lv, opt))
        d.update(module_tensors("vae", vae))
        return d

    def run(self, d):
        st = d["_step"]
        losses = st.forward_backward(d["img"], d["mask"], d["eps"])
        d["_o"] = dict({f"loss{j}": t for j, t in enumerate(losses)}, gmu=d["_mu"].grad, glv=d["_lv"].grad)

    def outputs(self, d):
        return d["_o"]


# rows that run beside each other on two streams (test_two_callers)
PAIRS = [("kl_prefactor", "chol_inv"), ("predict_exact", "predict_inducing")]

__doc__ += "".join(f"  {name}: {row.case}"
                   + ("" if row.bitwise else f"  [outputs {row.loose} NOT held to bits, rel {row.tol:g}: {row.why}]")
                   + "\n" for name, row in ROWS.items())
