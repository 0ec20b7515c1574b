"""The stream-order suite's row table covers the header (no GPU): every function of include/lvae_hip.h with a
parameter named ``stream`` is reached by a row of stream_util.ROWS or listed, with its reason, in
stream_util.EXCLUDED.  A new entry point fails here until it has a row."""
import stream_util as S
from test_abi import declared_symbols


def test_header_parse_finds_the_stream_argument():
    e = S.stream_entries()
    assert set(e) <= set(declared_symbols())
    # the last parameter nearly everywhere; lvae_set_early_stream's only one
    assert e["lvae_gram_f64"] == 13 and e["lvae_kl_closed_factor_f32"] == 9 and e["lvae_set_early_stream"] == 0
    assert not any(n.startswith("lvae_prof_") or n.endswith("_size") for n in e)
    from lvae_amd import _lib
    for name, idx in e.items():
        assert idx < len(_lib.SIGNATURES[name][1]), name


def test_rows_reach_every_entry_point_with_a_stream():
    entries = set(S.stream_entries())
    reached = set().union(*[set(r.reaches) for r in S.ROWS.values()])
    assert all(reason for reason in S.EXCLUDED.values())
    assert set(S.EXCLUDED) <= entries
    assert not (reached & set(S.EXCLUDED))
    assert reached - entries == set(), "a row names something that takes no stream"
    assert entries - set(S.EXCLUDED) - reached == set(), "entry points with a stream argument and no row"


def test_table_names_what_is_not_held_to_bits():
    """A row off bit equality carries its tolerance, the outputs it applies to and its reason, and is no C-ABI row."""
    for name, row in S.ROWS.items():
        assert row.case, name
        if not row.bitwise:
            assert row.tol > 0 and row.why and row.loose and not row.abi, name
        assert name in S.__doc__
    for a, b in S.PAIRS:
        assert a in S.ROWS and b in S.ROWS


def test_only_the_3x3_convs_weight_gradients_are_loose():
    """The outputs off bit equality are matched by their whole parameter name: of a ConvVAE's gradients, under the
    prefixes the rows use, conv1 / conv2's weights alone; nothing of the transposed convs (the project's own HIP
    kernels give those), no bias, no loss; in pool_ops the one conv's weight."""
    from lvae_amd.vae import ConvVAE
    names = [n for n, _ in ConvVAE(3).named_parameters()]
    assert "deconv1.weight" in names and "deconv2.weight" in names
    for name in ("conv_vae", "hensman_step", "dubo_step", "elbo_step"):
        row = S.ROWS[name]
        assert not row.bitwise
        for prefix in ("vae", "m0"):
            keys = [f"{prefix}.{n}.grad" for n in names] + ["loss", "loss0", "z.grad", "mu", "recon"]
            loose = {k for k in keys if S.is_loose(row, k)}
            assert loose == {f"{prefix}.conv1.weight.grad", f"{prefix}.conv2.weight.grad"}, (name, loose)
            assert not any("deconv" in k for k in loose)
    pool = S.ROWS["pool_ops"]
    assert [k for k in ("ya", "yb", "g0", "g1", "conv.weight.grad", "conv.bias.grad") if S.is_loose(pool, k)] == [
        "conv.weight.grad"]
    for name, row in S.ROWS.items():
        if row.bitwise:
            assert not S.is_loose(row, "vae.conv1.weight.grad"), name
