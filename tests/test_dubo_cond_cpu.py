"""The conditioned DUBO without a GPU: the golden of the reference's new-subject loss, the closed form the kernels
implement against the oracle's joint DUBO, and the host side of the C ABI (symbols, sizes)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dubo_cond_util as C
import dubo_util as D
from conftest import ROOT
from oracle import lvae_oracle as O

SYMBOLS = ("lvae_dubo_cond_state_size", "lvae_dubo_cond_prepare_f64", "lvae_dubo_cond_eval_f64")


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "dubo_cond.npz"))


def golden_oracle(g, q):
    """the oracle's joint DUBO on the golden's cat(pred, train) at point q: values [L], gradients wrt the pred rows"""
    s0, s1 = O.spec_split(**D.CFG, id_covariate=int(g["id_covariate"]))
    X, Z = torch.tensor(g["X"]), torch.tensor(g["Z"])
    Lg, P, Pn, T = int(g["L"]), int(g["P"]), int(g["Pn"]), int(g["T"])
    m = torch.tensor(g["m_pts"][q], requires_grad=True)
    lv = torch.tensor(g["lv_pts"][q], requires_grad=True)
    mj = torch.cat([m, torch.tensor(g["mu"][Pn * T:])], 0)
    lj = torch.cat([lv, torch.tensor(g["logv"][Pn * T:])], 0)
    vals = torch.stack([O.deviance_upper_bound(s0, O.constrain(torch.tensor(g["raw0"][l])), s1,
                                               O.constrain(torch.tensor(g["raw1"][l])), float(g["noise"][l]), X,
                                               mj[:, l], lj[:, l], Z[l], P + Pn, T, float(g["eps"]))
                        for l in range(Lg)])
    gm, gl = torch.autograd.grad(vals.sum(), (m, lv))
    return vals.detach(), gm, gl


@pytest.mark.parametrize("q", [0, 1])
def test_oracle_reproduces_golden(q):
    g = golden()
    vals, gm, gl = golden_oracle(g, q)
    assert C.U.rel(vals, torch.tensor(g["dubo"][q])) < 1e-10
    assert C.U.rel(gm, torch.tensor(g["dubo_dm"][q])) < 1e-8
    assert C.U.rel(gl, torch.tensor(g["dubo_dlogv"][q])) < 1e-8


@pytest.mark.parametrize("name", ["own", "far"])
@pytest.mark.parametrize("cid", C.CPU_CASES)
def test_closed_form_is_the_joint_dubo(cid, name):
    """6 x or more inside the bounds the GPU is held to"""
    m, lv, cot = C.point(cid, name)
    got = C.closed_eval(C.closed_form(cid), m, lv, cot)
    C.check(got, C.oracle(cid, name), f"{cid} {name}", {q: b / 6 for q, b in C.BOUND.items()})
    A = C.closed_form(cid)[3]
    assert float(torch.linalg.eigvalsh(0.5 * (A + A.transpose(1, 2))).min()) > 0.0


def test_symbols_declared_exported_and_bound():
    from lvae_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lvae_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", src), s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s


# lvae_dubo_workspace_size of the dubo_util cases (L = 3, Q = 6) as it was before the conditioned calls came
WORKSPACE_BYTES = {"6x7x33": 778240, "5x3x9": 98048, "1x4x3": 44544, "3x1x1": 40192, "9x16x120": 8904960,
                   "2x128x128": 19342848, "4x32x17": 1489664, "3x33x17": 1212928, "15x3x9": 170496, "16x3x9": 178944,
                   "17x3x9": 203008, "35x2x5": 179712}


@pytest.mark.parametrize("cid", D.CASE_IDS)
def test_dubo_workspace_size_unchanged(cid):
    """prepare runs in the DUBO's own workspace: its size stays what it was"""
    from lvae_amd import _lib
    P, T, M, _ = D.CASES[cid]
    dims = _lib.DuboDims(D.L, M, P, T, 6, D.EPS)
    assert _lib.load().lvae_dubo_workspace_size(ctypes.byref(dims)) == WORKSPACE_BYTES[cid]


def test_state_size_needs_no_gpu():
    from lvae_amd import _lib
    lib = _lib.load()
    for Lh, Pn, T in [(1, 1, 1), (3, 2, 7), (16, 8, 20), (3, 9, 32)]:
        n = lib.lvae_dubo_cond_state_size(Lh, Pn, T)
        Nn = Pn * T
        assert n % 256 == 0 and n >= 8 * (Lh + 2 * Lh * Nn + Lh * Nn * Nn) + 4 * Nn
    for bad in [(0, 2, 3), (3, 0, 3), (3, 2, 0), (-1, 2, 3)]:
        assert lib.lvae_dubo_cond_state_size(*bad) == 0
