"""Stream-order conformance (stream_util.py holds the protocol and the row table): every public operation, run on a
fresh non-blocking stream behind a device-side delay while its inputs still hold a decoy problem, must give the bits
of its synchronised default-stream reference -- every launch, helper and nested call ordered behind the caller's
stream, every side stream forked after the caller's inputs and joined before the return -- and must hand the library
no stream but the caller's (or one the row declares), never the null stream.  No graph capture here."""
import pytest
import torch

import stream_util as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def deferred_info_checks(hip):
    """the rows only enqueue: the info arrays are read after the synchronise (stream_util.settle)"""
    elbo = S.elbo_module()
    elbo.take_pending()
    elbo.set_sync_checks(False)
    S.delay()
    yield
    torch.cuda.synchronize()
    elbo.take_pending()
    elbo.set_sync_checks(True)


@pytest.mark.parametrize("name", list(S.ROWS))
def test_row(hip, name):
    S.run_row(S.ROWS[name], hip)


@pytest.mark.parametrize("a,b", S.PAIRS)
def test_two_callers(hip, a, b):
    """Two rows on two streams behind delays that end together: each equals its own reference."""
    S.run_pair(S.ROWS[a], S.ROWS[b], hip)
