"""GPU swap-or-not shuffle against the C oracle (which test_shuffle.py pins
to the hashlib restatement): the 256-position hash-window edges, both
directions, other round counts, inputs that are not range(n), the
device-resident entry, the error returns, and the scratch buffer the shuffle
shares with the merkle reduction on one context."""
import ctypes
import hashlib

import numpy as np
import pytest

import ssz_ref

pytestmark = pytest.mark.gpu

M3X_ERR_ARG = -2
SEED = hashlib.sha256(b"gpu-shuffle-edges").digest()


@pytest.fixture(scope="module")
def ctx():
    from lighthouse_amd import _native

    return _native.default_ctx()


def oracle_shuffle(oracle, values, rounds, seed, forwards):
    buf = np.array(values, dtype=np.uint32)
    rc = oracle.m3x_oracle_shuffle_list(
        buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(buf.size),
        ctypes.c_uint8(rounds), seed, ctypes.c_int(1 if forwards else 0))
    assert rc == 0
    return buf


def arbitrary_values(n):
    """seeded uint32 values with 0, 0xFFFFFFFF and repeated values among
    them: a kernel that wrote positions instead of moving values fails"""
    v = np.random.default_rng(n).integers(0, 1 << 32, size=n, dtype=np.uint32)
    v[0] = 0
    v[1] = 0xFFFFFFFF
    v[n // 2 :] = v[: n - n // 2][::-1]  # every value of the top half twice
    v[n - 1] = 0xFFFFFFFF
    v[n - 2] = 0
    return v


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 511, 512, 513, 65537])
def test_sizes_both_directions(ctx, oracle, n):
    from lighthouse_amd import shuffle as sh

    ident = np.arange(n, dtype=np.uint32)
    for fwd in [True, False]:
        want = oracle_shuffle(oracle, ident, 90, SEED, fwd)
        got = sh.shuffle_list(ident, 90, SEED, fwd, ctx=ctx)
        assert got.dtype == np.uint32 and got.tobytes() == want.tobytes(), (n, fwd)


@pytest.mark.parametrize("n", [257, 513])
@pytest.mark.parametrize("rounds", [1, 2, 255])
def test_round_counts(ctx, oracle, n, rounds):
    from lighthouse_amd import shuffle as sh

    ident = np.arange(n, dtype=np.uint32)
    for fwd in [True, False]:
        want = oracle_shuffle(oracle, ident, rounds, SEED, fwd)
        got = sh.shuffle_list(ident, rounds, SEED, fwd, ctx=ctx)
        assert got.tobytes() == want.tobytes(), (n, rounds, fwd)


@pytest.mark.parametrize("n", [513, 65537])
def test_values_are_moved_not_positions(ctx, oracle, n):
    from lighthouse_amd import shuffle as sh

    vals = arbitrary_values(n)
    for fwd in [True, False]:
        want = oracle_shuffle(oracle, vals, 90, SEED, fwd)
        got = sh.shuffle_list(vals, 90, SEED, fwd, ctx=ctx)
        assert got.tobytes() == want.tobytes(), (n, fwd)
        assert want.tobytes() != vals.tobytes()


def d2h(ctx, dev, nbytes):
    out = ctypes.create_string_buffer(nbytes)
    assert ctx._lib.m3x_d2h(ctx.handle, out, dev, nbytes) == 0
    return out.raw


@pytest.mark.parametrize("n", [513, 65537])
def test_device_resident_form(ctx, oracle, n):
    """upload, shuffle in device memory, read back: the host form's bytes;
    backwards over the same buffer brings the input back"""
    from lighthouse_amd import shuffle as sh

    lib = ctx._lib
    vals = arbitrary_values(n)
    want = sh.shuffle_list(vals, 90, SEED, True, ctx=ctx)
    assert want.tobytes() == oracle_shuffle(oracle, vals, 90, SEED, True).tobytes()
    dev = ctx.upload(vals.tobytes())
    try:
        assert lib.m3x_shuffle_list_dev(ctx.handle, dev, n, 90, SEED, 1) == 0
        assert d2h(ctx, dev, 4 * n) == want.tobytes()
        assert lib.m3x_shuffle_list_dev(ctx.handle, dev, n, 90, SEED, 0) == 0
        assert d2h(ctx, dev, 4 * n) == vals.tobytes()
    finally:
        ctx.free(dev)


def test_error_returns(ctx, oracle):
    from lighthouse_amd import shuffle as sh

    lib = ctx._lib
    n = 300
    vals = arbitrary_values(n)
    host = vals.copy()
    hp = host.ctypes.data_as(ctypes.c_void_p)
    dev = ctx.upload(vals.tobytes())
    try:
        # every one of these is refused before the list is touched
        for size, rounds in [(0, 90), ((1 << 24) + 1, 90), (n, 0), (n, 256)]:
            assert lib.m3x_shuffle_list(ctx.handle, hp, size, rounds, SEED, 1) \
                == M3X_ERR_ARG, (size, rounds)
            assert lib.m3x_shuffle_list_dev(ctx.handle, dev, size, rounds,
                                            SEED, 1) == M3X_ERR_ARG, (size, rounds)
        assert host.tobytes() == vals.tobytes()
        assert d2h(ctx, dev, 4 * n) == vals.tobytes()
        # rounds = 256 passes the host form's own check and is refused by
        # the device form it forwards to, after the temporary buffer was
        # made: repeated, the context still serves a valid call
        for _ in range(4):
            assert lib.m3x_shuffle_list(ctx.handle, hp, n, 256, SEED, 0) == M3X_ERR_ARG
        assert lib.m3x_shuffle_list(ctx.handle, hp, n, 255, SEED, 0) == 0
        assert host.tobytes() == oracle_shuffle(oracle, vals, 255, SEED, False).tobytes()
    finally:
        ctx.free(dev)
    # the wrapper's None for the reference's three conditions
    assert sh.shuffle_list([], 90, SEED, True, ctx=ctx) is None
    assert sh.shuffle_list([1, 2, 3], 0, SEED, True, ctx=ctx) is None
    too_long = np.zeros((1 << 24) + 1, dtype=np.uint32)
    assert sh.shuffle_list(too_long, 90, SEED, True, ctx=ctx) is None


def test_scratch_shared_with_merkle_reduction(oracle):
    """reduce_to_root and the shuffle carve the same growable buffer of a
    context; alternate them on a fresh one so that each growth (and the
    smaller uses after it) sits between calls of the other kind"""
    import os

    from lighthouse_amd import _native, shuffle as sh, tree_hash as th

    blob = ssz_ref.seeded_bytes(b"shared-scratch", 32 * 262145)
    small = ssz_ref.merkleize(ssz_ref.split_chunks(blob, 512), 9)
    large = ssz_ref.merkleize(ssz_ref.split_chunks(blob, 262145), 19)
    ctx = _native.Ctx(int(os.environ.get("M3X_DEVICE", "0")))
    try:
        assert th.merkleize_chunks(blob[: 32 * 512], 512, 9, -1, ctx=ctx) == small
        vals = arbitrary_values(65537)  # 257 hash windows: grows the buffer
        got = sh.shuffle_list(vals, 90, SEED, True, ctx=ctx)
        assert got.tobytes() == oracle_shuffle(oracle, vals, 90, SEED, True).tobytes()
        # 513 first-pass nodes, twice: grows it again
        assert th.merkleize_chunks(blob, 262145, 19, -1, ctx=ctx) == large
        vals = arbitrary_values(257)
        got = sh.shuffle_list(vals, 90, SEED, False, ctx=ctx)
        assert got.tobytes() == oracle_shuffle(oracle, vals, 90, SEED, False).tobytes()
        assert th.merkleize_chunks(blob[: 32 * 512], 512, 9, -1, ctx=ctx) == small
    finally:
        ctx.close()
