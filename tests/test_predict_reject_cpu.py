"""The latent predictors' argument checks, workspace-size queries and ctypes signatures against a recording of the
library as it stood before their host code was gathered into one check, carve and call path per route
(tests/golden/predict_reject_codes.json, written by tests/golden/gen_golden_predict_reject.py from that build).

Needs no GPU: every call here carries at least one bad argument and is rejected before any launch, and the size
queries are host code.  Per entry point the cases are a valid argument set on small host buffers (group_start of
lvae_predict_exact_cov_f64, which is read on the host, a real valid array), every single bad argument of the
return-code tests in tests/test_gpu_predict*.py, every pair of them (the order of the checks is part of the ABI: with
two bad arguments the same code must come back), and the few triples those tests hold.  The fully valid set is never
passed, and a case is called only where the recording says it is rejected.
"""
import ctypes
import itertools
import json
import os

import pytest
import torch

from lvae_amd import _lib as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_reject_codes.json")

# ---- host buffers and specs ----
_DBL = (ctypes.c_double * 2048)()
_INT = (ctypes.c_int32 * 256)()
_RAW = (ctypes.c_char * 8192)()
D, I = ctypes.addressof(_DBL), ctypes.addressof(_INT)
WS = (ctypes.addressof(_RAW) + 255) & ~255
Q = 4                                    # 1 + the specs' largest factor dim


def _variant(spec, **kw):
    s = P.KernelSpec.from_buffer_copy(spec)
    for k, v in kw.items():
        if k == "dim00":
            s.dim[0][0] = v
        else:
            setattr(s, k, v)
    return s


SPEC = P.make_spec([[("rbf", 0)], [("cat", 2), ("rbf", 1)], [("cat", 3)]])
S0 = P.make_spec([[("rbf", 0)], [("cat", 3), ("rbf", 1)]])
S1 = P.make_spec([[("cat", 2)], [("cat", 2), ("rbf", 0)]])
_KEEP = [SPEC, S0, S1]
r = ctypes.byref


def _spec_muts(name, spec, kinds):
    made = dict(comp17=dict(n_comp=17), dim32=dict(dim00=32), dimneg=dict(dim00=-1), comp0=dict(n_comp=0))
    out = {f"{name}=null": {name: None}}
    for k in kinds:
        v = _variant(spec, **made[k])
        _KEEP.append(v)
        out[f"{name}={k}"] = {name: r(v)}
    return out


def _ws_muts():
    return {"ws=null": dict(ws=None), "ws+8": dict(ws=WS + 8), "ws+128": dict(ws=WS + 128)}


# ---- exact route: n = 5, L = 2, nt = 3 (7 test rows in groups of 3, 1, 3 for the joint covariance) ----
def _starts(*v):
    a = (ctypes.c_int32 * len(v))(*v)
    _KEEP.append(a)
    return ctypes.addressof(a)


EX_HEAD = ["spec", "x", "ldx", "n", "L", "params", "noise", "mu", "ld_mu", "tx", "ldt", "nt"]
EX_BASE = dict(spec=r(SPEC), x=D, ldx=Q, n=5, L=2, params=D, noise=D, mu=D, ld_mu=2, tx=D, ldt=Q, nt=3, out=D,
               ld_out=2, info=I, ws=WS, stream=None)


def _exact_muts(spec_kinds):
    m = _spec_muts("spec", SPEC, spec_kinds)
    m.update({"x": dict(x=None), "ldx": dict(ldx=Q - 1), "n=0": dict(n=0), "n=-1": dict(n=-1), "L=0": dict(L=0),
              "params": dict(params=None), "noise": dict(noise=None), "mu": dict(mu=None), "ld_mu": dict(ld_mu=1),
              "tx": dict(tx=None), "ldt": dict(ldt=Q - 1), "nt=-1": dict(nt=-1), "ld_out": dict(ld_out=1),
              "info": dict(info=None)})
    m.update(_ws_muts())
    return m


_COMP = {"ld_comp": dict(ld_comp=1), "ld_comp=0": dict(ld_comp=0), "cs": dict(cs=3 * 2 - 1), "cs=0": dict(cs=0)}

ENTRIES = {}


def _entry(name, order, base, muts, skip=(), extra=()):
    ENTRIES[name] = dict(order=order, base=base, muts=muts, skip={frozenset(s) for s in skip}, extra=list(extra))


_entry("lvae_predict_exact_f64", EX_HEAD + ["out", "ld_out", "info", "ws", "stream"], EX_BASE,
       dict(_exact_muts(["comp17", "dim32", "dimneg"]), out=dict(out=None)))
_entry("lvae_predict_exact_comp_f64",
       EX_HEAD + ["out", "ld_out", "comp", "ld_comp", "cs", "info", "ws", "stream"],
       dict(EX_BASE, comp=D, ld_comp=2, cs=6),
       dict(_exact_muts(["dim32"]), out=dict(out=None), comp=dict(comp=None), **_COMP, **{"cs=-1": dict(cs=-1)}),
       extra=[("comp", "ld_comp=0", "cs=0")])
_entry("lvae_predict_exact_comp_cov_f64",
       EX_HEAD + ["out", "ld_out", "comp", "ld_comp", "cs", "chunk", "ccov", "info", "ws", "stream"],
       dict(EX_BASE, comp=D, ld_comp=2, cs=6, chunk=2, ccov=D),
       dict(_exact_muts(["dim32", "comp0"]), out=dict(out=None), **_COMP,
            **{"L=65536": dict(L=65536), "chunk=0": dict(chunk=0), "chunk=-3": dict(chunk=-3),
               "ccov": dict(ccov=None)}))
_entry("lvae_predict_exact_var_f64",
       EX_HEAD + ["out", "ld_out", "var", "ld_var", "add_noise", "chunk", "info", "ws", "stream"],
       dict(EX_BASE, var=D, ld_var=2, add_noise=0, chunk=2),
       dict(_exact_muts(["comp17"]), var=dict(var=None), ld_var=dict(ld_var=1),
            **{"add_noise=2": dict(add_noise=2), "add_noise=-1": dict(add_noise=-1), "chunk=0": dict(chunk=0)}))
_entry("lvae_predict_exact_cov_f64",
       EX_HEAD + ["G", "start", "n_max", "out", "ld_out", "cov", "add_noise", "chunk", "info", "ws", "stream"],
       dict(EX_BASE, nt=7, G=3, start=_starts(0, 3, 4, 7), n_max=3, cov=D, add_noise=0, chunk=4),
       dict(_exact_muts(["comp17"]), cov=dict(cov=None), start=dict(start=None),
            **{"L=65536": dict(L=65536), "G=-1": dict(G=-1), "G=0": dict(G=0), "G=65536": dict(G=65536),
               "nt=0": dict(nt=0, tx=None), "n_max=0": dict(n_max=0), "n_max=129": dict(n_max=129),
               "add_noise=2": dict(add_noise=2), "add_noise=-1": dict(add_noise=-1), "chunk<n_max": dict(chunk=2),
               "chunk=0": dict(chunk=0), "start shifted": dict(start=_starts(1, 3, 4, 7)),
               "start long": dict(start=_starts(0, 4, 4, 7)), "start empty": dict(start=_starts(0, 3, 3, 7)),
               "G-1": dict(G=2)}),
       skip=[("nt=0", "G=0")])   # (no test rows and no groups: together a valid set)

# ---- inducing-point route: L = 2, M = 3, P = 2, T = 4, Nt = 5 in 2 subject groups ----
IN_HEAD = ["s0", "s1", "L", "M", "Q", "P", "T", "seg", "inc", "x", "mu", "z", "Nt", "tx"]
IN_PAR = ["p0", "p1", "noise", "eps"]
IN_GRP = ["G", "gsub", "gstart"]
IN_BASE = dict(s0=r(S0), s1=r(S1), L=2, M=3, Q=Q, P=2, T=4, seg=I, inc=I, x=D, mu=D, z=D, Nt=5, tx=D, p0=D, p1=D,
               noise=D, eps=1e-3, out=D, info=I, ws=WS, stream=None, G=2, gsub=I, gstart=I)


def _inducing_muts(s1_kinds, pointers):
    m = _spec_muts("s0", S0, ["comp17"])
    m.update(_spec_muts("s1", S1, s1_kinds))
    m.update({"L=0": dict(L=0), "M=0": dict(M=0), "M=129": dict(M=129), "P=0": dict(P=0), "T=0": dict(T=0),
              "T=129": dict(T=129), "Q=0": dict(Q=0), "seg": dict(seg=None), "inc": dict(inc=None),
              "Nt=-1": dict(Nt=-1)})
    if pointers:   # (lvae_predict_f64 and lvae_predict_comp_f64 take null x, z, params*, noise: not bad there)
        m.update({"mu": dict(mu=None), "x": dict(x=None), "z": dict(z=None), "p0": dict(p0=None), "p1": dict(p1=None),
                  "noise": dict(noise=None), "tx": dict(tx=None), "G=-1": dict(G=-1), "gsub": dict(gsub=None),
                  "gstart": dict(gstart=None)})
    m.update(_ws_muts())
    return m


_ICOMP = {"ld_comp": dict(ld_comp=1), "ld_comp=0": dict(ld_comp=0), "cs": dict(cs=5 * 2 - 1), "cs=0": dict(cs=0)}

_entry("lvae_predict_f64", IN_HEAD + IN_PAR + ["out", "info", "ws", "stream"], IN_BASE,
       _inducing_muts(["comp17"], False))
_entry("lvae_predict_comp_f64", IN_HEAD + IN_PAR + ["out", "comp", "ld_comp", "cs", "info", "ws", "stream"],
       dict(IN_BASE, comp=D, ld_comp=2, cs=10),
       dict(_inducing_muts(["dim32"], False), comp=dict(comp=None), **_ICOMP, **{"Q<ld": dict(Q=Q - 1)}),
       extra=[("comp", "ld_comp=0", "cs=0")])
_entry("lvae_predict_var_f64",
       IN_HEAD + IN_GRP + IN_PAR + ["out", "var", "add_noise", "info", "ws", "stream"],
       dict(IN_BASE, var=D, add_noise=0),
       dict(_inducing_muts(["comp17"], True), var=dict(var=None), **{"add_noise=2": dict(add_noise=2)}))
_entry("lvae_predict_cov_f64",
       IN_HEAD + IN_GRP + ["n_max"] + IN_PAR + ["out", "cov", "add_noise", "info", "ws", "stream"],
       dict(IN_BASE, n_max=3, cov=D, add_noise=0),
       dict(_inducing_muts(["comp17"], True), cov=dict(cov=None),
            **{"L=65536": dict(L=65536), "G=65536": dict(G=65536), "add_noise=2": dict(add_noise=2),
               "add_noise=-1": dict(add_noise=-1), "n_max=0": dict(n_max=0), "n_max=129": dict(n_max=129)}))
_entry("lvae_predict_comp_cov_f64",
       IN_HEAD + IN_GRP + IN_PAR + ["out", "comp", "ld_comp", "cs", "ccov", "info", "ws", "stream"],
       dict(IN_BASE, comp=D, ld_comp=2, cs=10, ccov=D),
       dict(_inducing_muts(["dim32", "comp0"], True), out=dict(out=None), ccov=dict(ccov=None), **_ICOMP,
            **{"L=65536": dict(L=65536), "Q<ld": dict(Q=Q - 1), "Nt*R>int": dict(Nt=2 ** 31 // 4 + 1)}))

# ---- the draws: L = 2, G = 3, n_max = 4, Nt = 7, S = 5 ----
_entry("lvae_predict_sample_f64",
       ["L", "G", "n_max", "Nt", "S", "cov", "index", "mean", "eps", "jitter", "out", "info", "ws", "stream"],
       dict(L=2, G=3, n_max=4, Nt=7, S=5, cov=D, index=I, mean=D, eps=D, jitter=0.0, out=D, info=I, ws=WS, stream=None),
       {"L=0": dict(L=0), "G=-1": dict(G=-1), "LG>65535": dict(L=256, G=256), "n_max=0": dict(n_max=0),
        "n_max=129": dict(n_max=129), "Nt=-1": dict(Nt=-1), "Nt>G n_max": dict(Nt=13), "G=0": dict(G=0),
        "S=-1": dict(S=-1), "cov": dict(cov=None), "index": dict(index=None), "mean": dict(mean=None),
        "eps": dict(eps=None), "jitter<0": dict(jitter=-1e-9), "jitter=nan": dict(jitter=float("nan")),
        "out": dict(out=None), "info": dict(info=None), "ws=null": dict(ws=None), "ws+8": dict(ws=WS + 8)})


def cases(name):
    """[(case id, overrides)] of an entry: each single bad argument, each pair that touches different arguments
    (and does not add up to a valid set), and the entry's extra combinations"""
    e = ENTRIES[name]
    out = [(k, v) for k, v in e["muts"].items()]
    for (ka, va), (kb, vb) in itertools.combinations(e["muts"].items(), 2):
        if set(va) & set(vb) or frozenset((ka, kb)) in e["skip"]:
            continue
        out.append((f"{ka} + {kb}", {**va, **vb}))
    for combo in e["extra"]:
        kw = {}
        for k in combo:
            kw.update(e["muts"][k])
        out.append((" + ".join(combo), kw))
    return out


def call(lib, name, overrides):
    e = ENTRIES[name]
    assert overrides, "the fully valid set is never passed"
    a = dict(e["base"], **overrides)
    return int(getattr(lib, name)(*[a[k] for k in e["order"]]))


# ---- the size queries' grid ----
_BIG = (2 ** 31 - 1) // 4          # Nt with Nt * 4 just under INT32_MAX; _BIG + 1 is just over
# (L, M, P, T, Nt): the queries of lvae_predict_f64, _var_ and _cov_ (and _comp_ below) do not reject a size, and
# divide by L P T, so their grid holds Nt <= 0 and M outside 1 .. 128 but no L, P or T of 0
_IND5 = [(2, 3, 2, 4, 5), (1, 1, 1, 1, 1), (3, 128, 7, 128, 70), (2, 3, 2, 4, 0), (2, 3, 2, 4, -1), (2, 0, 2, 4, 5),
         (2, 129, 2, 4, 5), (16, 20, 40, 20, 4000), (1, 3, 5, 1, 37), (3, 20, 7, 20, 15), (2, 128, 1, 128, 1),
         (5, 7, 3, 9, 129)]
_IND7 = [s + (2, 2) for s in _IND5[:8]] + [
    (2, 3, 2, 4, 5, 1, 1), (2, 3, 2, 4, 5, 16, 16), (2, 3, 2, 4, 5, 0, 2), (2, 3, 2, 4, 5, 2, 17), (2, 3, 2, 4, 5, 0, 0)]
# lvae_predict_comp_cov_f64's query rejects: every bad size, and Nt R just under and just over INT32_MAX
_IND7V = _IND7 + [(0, 3, 2, 4, 5, 2, 2), (2, 3, 0, 4, 5, 2, 2), (2, 3, 2, 0, 5, 2, 2), (2, 3, 2, 129, 5, 2, 2),
                  (1, 1, 1, 1, _BIG, 2, 2), (1, 1, 1, 1, _BIG + 1, 2, 2)]
_EX3 = [(5, 3, 2), (1, 0, 1), (63, 17, 3), (65, 70, 1), (130, 1, 3), (513, 12, 2), (1200, 300, 16), (0, 3, 2), (5, -1, 2),
        (5, 3, 0), (-1, 3, 2), (4096, 1024, 4)]
_EX4 = [s + (c,) for s in _EX3[:6] for c in (1, 16)] + [
    (5, 3, 2, 3), (5, 3, 2, 4), (5, 3, 2, 100), (5, 3, 2, 0), (5, 3, 2, -1), (5, 0, 2, 0), (5, 0, 2, 7), (0, 3, 2, 2),
    (5, -1, 2, 2), (5, 3, 0, 2), (1200, 300, 16, 128), (513, 12, 2, 5)]
_EXC = [s + (rr,) for s in _EX3 for rr in (1, 5)] + [(5, 3, 2, 0), (5, 3, 2, 16), (5, 3, 2, 17), (5, 3, 2, -1)]
_EXCC = [s[:3] + (rr, s[3]) for s in _EX4 for rr in (1, 5)] + [(5, 3, 2, 0, 2), (5, 3, 2, 16, 2), (5, 3, 2, 17, 2)]
SIZE_GRID = {
    "lvae_predict_workspace_size": _IND5,
    "lvae_predict_var_workspace_size": _IND5,
    "lvae_predict_cov_workspace_size": _IND5,
    "lvae_predict_comp_workspace_size": _IND7,
    "lvae_predict_comp_cov_workspace_size": _IND7V,
    "lvae_predict_exact_workspace_size": _EX3,
    "lvae_predict_exact_comp_workspace_size": _EXC,
    "lvae_predict_exact_var_workspace_size": _EX4,
    "lvae_predict_exact_cov_workspace_size": _EX4,
    "lvae_predict_exact_comp_cov_workspace_size": _EXCC,
    "lvae_predict_sample_workspace_size": [(2, 3, 4), (1, 1, 1), (3, 0, 4), (0, 3, 4), (2, -1, 4), (2, 3, 0), (2, 3, 128),
                                           (16, 4000, 128), (255, 257, 3), (2, 3, -1), (1, 65535, 1), (7, 1, 129)],
}


def record(lib):
    """The table of a loaded library: {"codes": {entry: {case id: code}}, "sizes": {query: [[args, bytes]]}}"""
    codes = {name: {cid: call(lib, name, kw) for cid, kw in cases(name)} for name in ENTRIES}
    sizes = {name: [[list(s), int(getattr(lib, name)(*s))] for s in grid] for name, grid in SIZE_GRID.items()}
    return dict(codes=codes, sizes=sizes)


@pytest.fixture(scope="module")
def table():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_rejection_codes(table, name):
    lib = P.load()
    want = table["codes"][name]
    todo = cases(name)
    assert sorted(want) == sorted(cid for cid, _ in todo)
    for cid, kw in todo:
        assert -24 <= want[cid] <= -1, (name, cid)            # rejected in the recording: nothing can be launched
        assert call(lib, name, kw) == want[cid], (name, cid)


@pytest.mark.parametrize("name", list(SIZE_GRID))
def test_size_queries(table, name):
    lib = P.load()
    want = table["sizes"][name]
    assert [w[0] for w in want] == [list(s) for s in SIZE_GRID[name]]
    for args, size in want:
        assert int(getattr(lib, name)(*args)) == size, (name, args)


def test_signatures():
    """The predictor family's argtypes, element for element, as they were declared one flat list each"""
    I32, I64, DBL, VP, SZ = ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    SP = ctypes.POINTER(P.KernelSpec)
    want = {
        "lvae_predict_workspace_size": (SZ, [I32, I32, I32, I32, I32]),
        "lvae_predict_f64": (I32, [SP, SP, I32, I32, I32, I32, I32, VP, VP, VP, VP, VP, I32, VP, VP, VP, VP, DBL, VP,
                                   VP, VP, VP]),
        "lvae_predict_exact_workspace_size": (SZ, [I32, I32, I32]),
        "lvae_predict_exact_f64": (I32, [SP, VP, I64, I32, I32, VP, VP, VP, I64, VP, I64, I32, VP, I64, VP, VP, VP]),
        "lvae_predict_exact_comp_workspace_size": (SZ, [I32, I32, I32, I32]),
        "lvae_predict_exact_comp_f64": (I32, [SP, VP, I64, I32, I32, VP, VP, VP, I64, VP, I64, I32, VP, I64, VP, I64,
                                              I64, VP, VP, VP]),
        "lvae_predict_comp_workspace_size": (SZ, [I32, I32, I32, I32, I32, I32, I32]),
        "lvae_predict_comp_f64": (I32, [SP, SP, I32, I32, I32, I32, I32, VP, VP, VP, VP, VP, I32, VP, VP, VP, VP, DBL,
                                        VP, VP, I64, I64, VP, VP, VP]),
        "lvae_predict_exact_comp_cov_workspace_size": (SZ, [I32, I32, I32, I32, I32]),
        "lvae_predict_exact_comp_cov_f64": (I32, [SP, VP, I64, I32, I32, VP, VP, VP, I64, VP, I64, I32, VP, I64, VP,
                                                  I64, I64, I32, VP, VP, VP, VP]),
        "lvae_predict_comp_cov_workspace_size": (SZ, [I32, I32, I32, I32, I32, I32, I32]),
        "lvae_predict_comp_cov_f64": (I32, [SP, SP, I32, I32, I32, I32, I32, VP, VP, VP, VP, VP, I32, VP, I32, VP, VP,
                                            VP, VP, VP, DBL, VP, VP, I64, I64, VP, VP, VP, VP]),
        "lvae_predict_exact_var_workspace_size": (SZ, [I32, I32, I32, I32]),
        "lvae_predict_exact_var_f64": (I32, [SP, VP, I64, I32, I32, VP, VP, VP, I64, VP, I64, I32, VP, I64, VP, I64,
                                             I32, I32, VP, VP, VP]),
        "lvae_predict_var_workspace_size": (SZ, [I32, I32, I32, I32, I32]),
        "lvae_predict_var_f64": (I32, [SP, SP, I32, I32, I32, I32, I32, VP, VP, VP, VP, VP, I32, VP, I32, VP, VP, VP,
                                       VP, VP, DBL, VP, VP, I32, VP, VP, VP]),
        "lvae_predict_cov_workspace_size": (SZ, [I32, I32, I32, I32, I32]),
        "lvae_predict_cov_f64": (I32, [SP, SP, I32, I32, I32, I32, I32, VP, VP, VP, VP, VP, I32, VP, I32, VP, VP, I32,
                                       VP, VP, VP, DBL, VP, VP, I32, VP, VP, VP]),
        "lvae_predict_exact_cov_workspace_size": (SZ, [I32, I32, I32, I32]),
        "lvae_predict_exact_cov_f64": (I32, [SP, VP, I64, I32, I32, VP, VP, VP, I64, VP, I64, I32, I32, VP, I32, VP,
                                             I64, VP, I32, I32, VP, VP, VP]),
        "lvae_predict_sample_workspace_size": (SZ, [I32, I32, I32]),
        "lvae_predict_sample_f64": (I32, [I32, I32, I32, I32, I32, VP, VP, VP, VP, DBL, VP, VP, VP, VP]),
    }
    assert sorted(want) == sorted(k for k in P.SIGNATURES if k.startswith("lvae_predict_"))
    for name, (res, args) in want.items():
        assert P.SIGNATURES[name][0] is res and list(P.SIGNATURES[name][1]) == args, name


def test_subject_groups_cap_is_the_callers():
    """A subject with 129 test rows groups fine where no joint covariance of the group is formed (the variance and
    the components' covariance), and raises with the joint covariance's message where the caller sets the cap"""
    from lvae_amd.predict import MAX_GROUP_ROWS, _subject_groups
    labels = torch.cat([torch.full((129,), 7.0), torch.tensor([3.0, 9.0, 3.0])])
    pred_ids = torch.tensor([1.0, 3.0, 7.0], dtype=torch.float64)
    g = _subject_groups(labels, pred_ids, "test", max_rows=None)
    assert g.counts.tolist() == [2, 129, 1] and g.n_max == 129 and g.start.tolist() == [0, 2, 131, 132]
    assert g.start.dtype == torch.int32 and g.subj.dtype == torch.int32
    assert g.subj.tolist() == [1, 2, -1]                       # 9 is not in the prediction set
    assert g.order[:2].tolist() == [129, 131] and g.order[2:131].tolist() == list(range(129))
    with pytest.raises(ValueError) as err:
        _subject_groups(labels, pred_ids, "test", max_rows=MAX_GROUP_ROWS)
    assert str(err.value) == ("test: group 1 (label 7) has 129 test rows; a joint covariance is formed for groups of "
                              "at most 128")
