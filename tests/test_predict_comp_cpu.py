"""CPU checks of the per-component predictions: the component oracles of predict_comp_util.py add up to the existing
total oracles, LatentComponents' bookkeeping (labels, module flags, explained_variance) on hand-made tensors, and the
GPU tests' cases are well posed (yardsticks <= 1e-7, references not zero, the slab case really slabbed).  No GPU
call: the size queries run on the host."""
import pytest
import torch

import abi_util as U
import predict_comp_util as C
import test_gpu_predict_exact_abi as E
from oracle import lvae_oracle as O


@pytest.mark.parametrize("cid", C.IND_IDS)
def test_inducing_components_sum_to_the_total_oracle(cid):
    """sum_r F[r] = O.batch_predict_varying_T within 1e-12 (ragged subjects, test subjects inside and outside the
    prediction set, none inside at all: the k1 components are then exactly zero)"""
    ref, _ = C.ind_ref(cid)
    if ref is None:
        assert C.ind_problem(cid)["Nt"] == 0
        return
    c = C.ind_problem(cid)
    total = C.ind_oracle(cid, total=True)
    assert ref.shape == (len(c["s0"]) + len(c["s1"]), c["Nt"], c["L"])
    err = U.rel(ref.sum(0), total)
    print(f"inducing components {cid}: |sum - total| / max|total| = {err:.2e}")
    assert err <= 1e-12
    if cid == "none-included":
        assert not bool(c["include"].any()) and bool((ref[len(c["s0"]):] == 0).all())
    if cid == "m3-mixed":
        assert 0 < int(c["include"].sum()) < c["P"] and float(ref[len(c["s0"]):].abs().max()) > 0


@pytest.mark.parametrize("cid", C.EXACT_IDS)
def test_exact_components_sum_to_the_total_oracle(cid):
    ref, _ = C.exact_ref(cid)
    if ref is None:
        assert E.problem(cid)["Nt"] == 0
        return
    total, _ = E.cpu_ref(cid)
    err = U.rel(ref.sum(0), total)
    print(f"exact components {cid}: |sum - total| / max|total| = {err:.2e}")
    assert err <= 1e-12


def test_component_oracle_is_the_gram_split():
    """The one-component Grams add up to O.gram of the whole spec (the parameter offsets are right), on a spec with
    rbf, per (two parameters) and parameter-free factors"""
    c = E.problem("ext")
    K = O.gram(c["spec"], c["params"], c["tx"], c["x"])
    parts = sum(C.comp_gram(c["spec"], c["params"], r, c["tx"], c["x"]) for r in range(len(c["spec"])))
    assert C.offsets(c["spec"]) == [0, 3, 4, 7, 8, 10] and C.offsets(c["spec"])[-1] == O.n_params(c["spec"])
    assert U.rel(parts, K) <= 1e-15


def test_gpu_cases_are_well_posed():
    """Every case of the two GPU modules: the perturbation yardstick is <= 1e-7 (10 x it stays under the 1e-6 cap),
    the reference is not zero, every component's own reference is non-zero unless it is zero by construction (the
    one-row "smallest" cases aside: a category that differs zeroes a component there), and the slab cases sit on
    either side of the host's threshold."""
    for cid in C.EXACT_IDS:
        ref, ya = C.exact_ref(cid)
        if ref is not None:
            assert ya <= 1e-7 and float(ref.abs().max()) > 0, (cid, ya)
            assert cid == "smallest" or float(ref.abs().amax((1, 2)).min()) > 0, cid
    for cid in C.IND_IDS:
        ref, ya = C.ind_ref(cid)
        if ref is None:
            continue
        c = C.ind_problem(cid)
        live = ref if bool(c["include"].any()) else ref[:len(c["s0"])]
        assert ya <= 1e-7 and float(ref.abs().max()) > 0, (cid, ya)
        assert cid == "smallest" or float(live.abs().amax((1, 2)).min()) > 0, cid
    for cid in C.MV_IDS:
        c = C.mv_problem(cid)
        ref, mag, full = C.mv_ref(cid)
        assert ref.shape == (c["R"], c["n1"], c["L"]) and float(full.min()) > 0
        ids = [r for r, comp in enumerate(c["spec"]) if ("cat", U.ID_COL) in comp]
        for r in range(c["R"]):
            if c["absent"] and r in ids:
                assert bool((ref[r] == 0).all()) and float(mag[r].max()) == 0.0
            else:
                assert float(ref[r].abs().max()) > 0, (cid, r)
    z = C.mv_problem("zero-id")
    assert len([1 for comp in z["spec"] if ("cat", U.ID_COL) in comp]) == 2
    s, s1 = C.mv_problem("slab"), C.mv_problem("slab-64")
    assert s["n1"] == 3 and C.slabs(3, s["n2"], s["L"], s["R"]) >= 2
    assert s1["n2"] == s["n2"] - 64 and C.slabs(3, s1["n2"], s1["L"], s1["R"]) == 1
    assert C.mv_problem("wide-cols")["x1"].shape[1] == 3 * U.QC and C.mv_problem("z128")["x2"].shape == (3, 128, U.QC)


def test_size_queries():
    """The component product's workspace is R times the summed product's (the same slabs), 0 on empty sides"""
    from lvae_amd import _lib
    lib = _lib.load()
    for n1, n2, L in ((3, 257, 2), (3, 193, 2), (70, 4096, 1), (1024, 4096, 16)):
        base = int(lib.lvae_gram_matvec_workspace_size(n1, n2, L))
        for R in (1, 5, 16):
            assert int(lib.lvae_gram_matvec_comp_workspace_size(n1, n2, L, R)) == R * base
    assert lib.lvae_gram_matvec_comp_workspace_size(0, 9, 2, 5) == 0
    assert lib.lvae_gram_matvec_comp_workspace_size(9, 0, 2, 5) == 0
    assert lib.lvae_gram_matvec_comp_workspace_size(9, 9, 2, 0) == 0
    assert lib.lvae_predict_exact_comp_workspace_size(0, 5, 2, 3) == 0
    assert lib.lvae_predict_exact_comp_workspace_size(70, 5, 2, 3) >= lib.lvae_predict_exact_workspace_size(70, 5, 2)
    assert (lib.lvae_predict_comp_workspace_size(2, 3, 4, 17, 9, 5, 4) >=
            lib.lvae_predict_workspace_size(2, 3, 4, 17, 9))


def test_latent_components_bookkeeping():
    """labels from kernel.components(), module flags, total() and explained_variance() on a hand-made tensor: an
    all-constant latent dim gives 0 shares, the shares of a live dim add up to 1"""
    import lvae_amd as la
    from lvae_amd.predict import LatentComponents, component_labels
    cfg = dict(cat_kernel=[2], bin_kernel=[], sqexp_kernel=[0],
               cat_int_kernel=[{'cont_covariate': 0, 'cat_covariate': 2}, {'cont_covariate': 0, 'cat_covariate': 3},
                               {'cont_covariate': 1, 'cat_covariate': 4}],
               bin_int_kernel=[], covariate_missing_val=[{'covariate': 3, 'mask': 5}])
    k0, k1 = la.generate_kernel_batched(2, **cfg, id_covariate=2)
    s0, s1 = O.spec_split(**cfg, id_covariate=2)
    assert component_labels(k0) == C.labels(s0) == ["rbf(0)", "cat(3)*bin(5)*rbf(0)", "cat(4)*rbf(1)"]
    assert component_labels(k1) == C.labels(s1) == ["cat(2)", "cat(2)*rbf(0)"]
    per_dim = [la.generate_kernel_batched(1, **cfg, id_covariate=2)[0] for _ in range(2)]
    assert component_labels(per_dim) == C.labels(s0)
    vals = torch.zeros(3, 4, 2, dtype=torch.float64)
    vals[0, :, 0] = torch.tensor([1.0, -1.0, 1.0, -1.0])      # variance 1
    vals[1, :, 0] = torch.tensor([3.0, 3.0, -3.0, -3.0])      # variance 9
    vals[2, :, 0] = 7.0                                        # constant: variance 0
    vals[:, :, 1] = torch.tensor([2.0, -5.0, 0.0])[:, None]    # dim 1: every component constant over the rows
    comps = LatentComponents(vals, ["a", "b", "c"], [0, 0, 1])
    assert comps.labels == ["a", "b", "c"] and comps.module == [0, 0, 1]
    assert torch.equal(comps.total(), vals.sum(0))
    ev = comps.explained_variance()
    assert ev.shape == (3, 2)
    assert torch.equal(ev[:, 0], torch.tensor([0.1, 0.9, 0.0], dtype=torch.float64))
    assert torch.equal(ev[:, 1], torch.zeros(3, dtype=torch.float64))
    assert "covariance" in LatentComponents.explained_variance.__doc__


def test_generate_component_sequences_cpu():
    """The cumulative decode on the CPU with a SimpleVAE: entry r decodes the sum of the first r + 1 components in
    the given order; the last entry of a full order is decode(total())"""
    import lvae_amd as la
    from lvae_amd.predict import LatentComponents
    torch.manual_seed(0)
    model = la.SimpleVAE(4, 36).eval()
    vals = torch.randn(3, 5, 4, dtype=torch.float64)
    comps = LatentComponents(vals, ["a", "b", "c"], [0, 0, 0])
    seq = la.generate_component_sequences(model, comps)
    with torch.no_grad():
        dec = lambda z: model.decode(z.to(torch.float32))
        assert seq.shape[:2] == (3, 5)
        assert torch.equal(seq[0], dec(vals[0])) and torch.equal(seq[-1], dec(comps.total()))
        rev = la.generate_component_sequences(model, comps, order=[2, 0])
        assert rev.shape[0] == 2 and torch.equal(rev[0], dec(vals[2])) and torch.equal(rev[1], dec(vals[[2, 0]].sum(0)))
    assert not seq.requires_grad
    with pytest.raises(ValueError):
        la.generate_component_sequences(model, comps, order=[3])
    assert "not additive" in la.generate_component_sequences.__doc__.lower().replace("not\n", "not ")
