"""GPU parity of the device-resident forms of the Deneb state root, the ones
the benchmark times: big fields read from HBM (dev=), the registry root
handed in from the sharded composition (registry_root=), and a state whose
variable-length lists are empty. Bit-exact against the hashlib restatement."""
import pytest

import ssz_ref
from test_gpu_merkle_edges import emulated_sharded_root

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lighthouse_amd import _native

    return _native.default_ctx()


# 1000 is no multiple of 32: the participation lists end in a part-filled
# chunk; with 1 validator every per-validator list is one part-filled chunk
@pytest.fixture(scope="module", params=[1, 1000, 4096])
def state(request):
    """a synthetic state and its reference root, computed once"""
    from lighthouse_amd import beacon_state as bs

    st = bs.generate(request.param, seed=request.param)
    return st, ssz_ref.beacon_state_root_ref(st)


def with_uploaded_fields(st, ctx, fn):
    from lighthouse_amd import beacon_state as bs

    dev = bs.upload_fields(st, ctx)
    try:
        return fn(dev)
    finally:
        for p in dev.values():
            ctx.free(p)


def test_state_root_device_fields(ctx, state):
    from lighthouse_amd import beacon_state as bs

    st, want = state
    got = with_uploaded_fields(
        st, ctx, lambda dev: bs.state_root(st, ctx=ctx, dev=dev))
    assert got == want


def test_state_root_sharded_registry(ctx, state):
    """registry_root= from eight emulated ranks over 4096 leaves: shards of
    512 records that are full, part-filled and empty, depending on n"""
    from lighthouse_amd import beacon_state as bs

    st, want = state
    n = st["n_validators"]
    reg = emulated_sharded_root(ctx, st["validators_ssz"], n, 4096, 8)
    assert reg == ssz_ref.validator_registry_root(st["validators_ssz"], n)
    got = with_uploaded_fields(
        st, ctx,
        lambda dev: bs.state_root(st, ctx=ctx, dev=dev, registry_root=reg))
    assert got == want
    assert bs.state_root(st, ctx=ctx, registry_root=reg) == want


def test_state_root_empty_lists(ctx):
    from lighthouse_amd import beacon_state as bs

    st = bs.generate(33, seed=5)
    st["eth1_data_votes"] = []
    st["historical_roots"] = b""
    st["historical_summaries"] = []
    want = ssz_ref.beacon_state_root_ref(st)
    assert bs.state_root(st, ctx=ctx) == want
    got = with_uploaded_fields(
        st, ctx, lambda dev: bs.state_root(st, ctx=ctx, dev=dev))
    assert got == want
