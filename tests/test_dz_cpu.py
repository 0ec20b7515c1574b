"""Learnable inducing points, the part that needs no GPU: the yardstick of test_gpu_dz.py checked against central
differences, and the new entry points' exports and host-side size queries."""
import ctypes

import torch

import dubo_util as D
from oracle import lvae_oracle as O


def test_oracle_dz_matches_central_differences():
    """The oracle's dz of the DUBO (CPU autograd through O.gram with z.requires_grad_()) at the tiny case 5x3x9
    against central differences of the oracle itself over the continuous columns 0 and 1 of every inducing row.

    What central differences can resolve here: dubo_util draws the inducing rows from x, and rows of different
    subjects at the same time point are the same point to k0 (which has no id factor), so Kz is singular up to the
    jitter eps = 1e-6 (cond(Kz) ~ 2e7) and the bound bends on the scale h* = l sqrt(eps) ~ 1e-3 of a step in z.
    Truncation is then ~(h / h*)^2 of the gradient and rounding is the bound's evaluation error, ~cond 2^-53 |f|
    ~ 2e7 x 1e-16 x 10 = 2e-8, over 2h, against a largest entry of ~0.1: 1e-7 / h.  The two meet at h ~ 5e-5 with
    ~2.5e-3 each, ~5e-3 together; the test uses that h and allows 4x the estimate, 2e-2 of max |dz|: a check of
    signs, factors and structure, which is what the yardstick needs.  The categorical columns get exact zeros."""
    import lvae_amd as la
    cid = "5x3x9"
    c = D.problem(cid)
    k0, k1, lik = D.modules_batched(c, "cpu")
    _, p0 = la.kernel_spec_and_params(k0)
    _, p1 = la.kernel_spec_and_params(k1)
    p0, p1, nz = p0.detach(), p1.detach(), lik.noise.detach()

    def f(l, z):
        return O.deviance_upper_bound(c["s0"], p0[l], c["s1"], p1[l], nz[l], c["X"], c["mu"][:, l], c["lv"][:, l], z,
                                      c["P"], c["T"], D.EPS)
    h = 5e-5
    cont = sorted({d for comp in c["s0"] for k, d in comp if k in ("rbf", "per", "lin")})
    assert cont == [0, 1]
    worst = 0.0
    for l in range(D.L):
        z = c["Z"][l].clone().requires_grad_()
        f(l, z).backward()
        dz = z.grad
        other = [q for q in range(z.shape[1]) if q not in cont]
        assert bool((dz[:, other] == 0).all())
        fd = torch.zeros_like(dz)
        with torch.no_grad():
            for i in range(z.shape[0]):
                for q in cont:
                    zp, zm = c["Z"][l].clone(), c["Z"][l].clone()
                    zp[i, q] += h
                    zm[i, q] -= h
                    fd[i, q] = (f(l, zp) - f(l, zm)) / (2 * h)
        err = D.rel(dz, fd)
        print(f"dim {l}: max |dz| {float(dz.abs().max()):.3e} err vs central differences {err:.2e}")
        assert float(dz.abs().max()) > 0
        worst = max(worst, err)
    assert worst < 2e-2


def test_dz_exports_and_host_queries():
    """The new symbols are exported, bound with their signatures, and the two size queries answer on the host:
    multiples of 256 where a workspace is needed, 0 for arguments the calls reject."""
    from lvae_amd import _lib as P
    lib = P.load()
    names = ["lvae_gram_bwd_x2_workspace_size", "lvae_gram_bwd_x2_f64", "lvae_bound_dz_workspace_size",
             "lvae_dubo_bwd_z_f64", "lvae_gp_elbo_bwd_z_f64", "lvae_hensman_bwd_z_f64"]
    for n in names:
        assert n in P.SIGNATURES, n
        fn = getattr(lib, n)
        assert fn.restype is P.SIGNATURES[n][0] and list(fn.argtypes) == P.SIGNATURES[n][1]
    assert len(P.SIGNATURES["lvae_gram_bwd_x2_f64"][1]) == 17
    for n in names[3:]:
        assert len(P.SIGNATURES[n][1]) == 9
    for args in [(1, 1, 1, 1, 1), (1, 2, 63, 33, 8), (2, 3, 257, 128, 8), (1, 16, 4096, 120, 40), (1, 1, 0, 5, 3)]:
        b = lib.lvae_gram_bwd_x2_workspace_size(*args)
        assert b > 0 and b % 256 == 0, (args, b)
    nb, Lg, n1, n2, Q = 2, 3, 257, 128, 8
    # one partial [n2, Q] per block of 64 rows of every (b, l) slice
    assert lib.lvae_gram_bwd_x2_workspace_size(nb, Lg, n1, n2, Q) == nb * Lg * 5 * n2 * Q * 8
    # (columns past the 32 the kernels stage are zeros: no partials for them)
    assert lib.lvae_gram_bwd_x2_workspace_size(1, 1, 64, 4, 40) == lib.lvae_gram_bwd_x2_workspace_size(1, 1, 64, 4, 32)
    for args in [(0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, -1, 1, 1), (1, 1, 1, -1, 1), (1, 1, 1, 1, 0)]:
        assert lib.lvae_gram_bwd_x2_workspace_size(*args) == 0, args
    for args in [(1, 1, 1, 1), (3, 9, 15, 5), (3, 33, 42, 5), (16, 120, 4096, 5), (2, 128, 256, 40)]:
        b = lib.lvae_bound_dz_workspace_size(*args)
        assert b > 0 and b % 256 == 0, (args, b)
    Lh, M, N, Q = 16, 120, 4096, 5
    # the partials of the three jobs: k0(x, z) against dX (64 row blocks), k0(z, z) against dKz and against dKz^T
    # (2 each); then the re-formed dKz and its scratch: two [L, M, M] and two [L, N, M] arrays
    a256 = lambda b: (b + 255) // 256 * 256
    assert lib.lvae_bound_dz_workspace_size(Lh, M, N, Q) == (a256(Lh * (64 + 2 + 2) * M * Q * 8)
                                                             + 2 * a256(Lh * M * M * 8) + 2 * a256(Lh * N * M * 8))
    for args in [(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)]:
        assert lib.lvae_bound_dz_workspace_size(*args) == 0, args
    # the existing workspaces did not move (the z-adjoint has its own): at the workload shape the sizes DESIGN.md
    # recorded before the z-adjoint existed, 623.7 MiB (DUBO, section 4.3c) and 447.4 MiB (ELBO, section 4.3d)
    d = P.DuboDims(16, 120, 256, 16, 6, 1e-6)
    assert lib.lvae_dubo_workspace_size(ctypes.byref(d)) == 654036992
    g = P.GpElboDims(16, 120, 256, 16, 6, 4, 1e-6)
    assert lib.lvae_gp_elbo_workspace_size(ctypes.byref(g)) == 469156096
    assert abs(469156096 / 2 ** 20 - 447.4) < 0.05 and abs(654036992 / 2 ** 20 - 623.7) < 0.05
