"""GPU merkleize at the kernels' staging boundaries, bit-exact against the
hashlib restatement (ssz_ref): the 9-level passes of k_reduce, the pooled /
allocated input switch, the high word of the mixed-in length, the sharded
registry root (subtree roots + finalize_root), the batched small-container
kernel over every group size, the registry cache at its capacity edges and
error returns, the registry root's host and device forms at the leaf-block
edges, the shared root slot under interleaved calls, and a refused context
create."""
import ctypes
import random

import pytest

import ssz_ref

pytestmark = pytest.mark.gpu

M3X_ERR_HIP = -1
M3X_ERR_ARG = -2
BIG_N = 262145  # first chunk count that needs three k_reduce passes


@pytest.fixture(scope="module")
def ctx():
    from lighthouse_amd import _native

    return _native.default_ctx()


@pytest.fixture(scope="module")
def blob():
    return ssz_ref.seeded_bytes(b"merkle-edges", 32 * BIG_N)


def both_forms(ctx, data, n, depth, mix):
    """root of the first n chunks of data through the host-copy entry and
    through the device-resident one"""
    from lighthouse_amd import tree_hash as th

    host = th.merkleize_chunks(data[: 32 * n], n, depth, mix, ctx=ctx)
    p = ctx.upload(data[: 32 * max(n, 1)])  # n = 0 reads nothing
    try:
        dev = th.merkleize_chunks_dev(p, n, depth, mix, ctx=ctx)
    finally:
        ctx.free(p)
    return host, dev


# ------------------------------------------------------------ 1. chunk trees

CHUNK_ROWS = [
    # depth < 9: one pass with levels = depth, ragged and full
    (1, 2), (3, 5), (8, 255), (8, 256),
    # exactly one full-span pass; zero padding inside a block; n = 1 skips it
    (9, 1), (9, 511), (9, 512),
    # second pass of 1, 3, 8 levels over 2 nodes padded with Z[9]
    (10, 513), (12, 513), (17, 513),
    # two full passes, ragged and exact
    (18, 262143), (18, 262144),
    # three passes 513 -> 2 -> 1, third one short, then a long zero cap
    (19, 262145), (40, 262145),
    # last pooled input, first allocated input
    (13, 8192), (14, 8193),
    # the top of the 65-entry zero ladder
    (64, 0), (64, 1), (63, 3),
]


@pytest.mark.parametrize("depth,n", CHUNK_ROWS)
def test_chunks_host_and_dev(ctx, blob, depth, n):
    want = ssz_ref.merkleize(ssz_ref.split_chunks(blob, n), depth)
    host, dev = both_forms(ctx, blob, n, depth, -1)
    assert host == want, ("host", depth, n)
    assert dev == want, ("dev", depth, n)


@pytest.mark.parametrize("depth,n", [(24, 100), (5, 0)])
def test_chunks_length_mix(ctx, blob, depth, n):
    root = ssz_ref.merkleize(ssz_ref.split_chunks(blob, n), depth)
    for mix in [-1, 0, 1, 2**32 - 1, 2**32, 2**32 + 5, 2**40]:
        want = root if mix < 0 else ssz_ref.mix_in_length(root, mix)
        host, dev = both_forms(ctx, blob, n, depth, mix)
        assert host == want, ("host", depth, n, mix)
        assert dev == want, ("dev", depth, n, mix)


def test_chunks_too_many_for_depth(ctx, blob):
    lib = ctx._lib
    out = ctypes.create_string_buffer(32)
    data = blob[: 32 * 9]
    assert lib.m3x_merkleize_chunks(ctx.handle, data, 9, 3, -1, out) == M3X_ERR_ARG
    p = ctx.upload(data)
    try:
        rc = lib.m3x_merkleize_chunks_dev(ctx.handle, p, 9, 3, -1, out)
    finally:
        ctx.free(p)
    assert rc == M3X_ERR_ARG
    # the context still works
    host, dev = both_forms(ctx, blob, 8, 3, -1)
    assert host == dev == ssz_ref.merkleize(ssz_ref.split_chunks(blob, 8), 3)


def test_depth_beyond_zero_ladder_rejected(ctx, blob):
    """the device ladder holds Z[0..64]; a deeper tree is refused on the
    host, before any launch"""
    lib = ctx._lib
    out = ctypes.create_string_buffer(32)
    data = blob[:64]
    assert lib.m3x_merkleize_chunks(ctx.handle, data, 2, 65, -1, out) == M3X_ERR_ARG
    p = ctx.upload(data)
    try:
        assert lib.m3x_merkleize_chunks_dev(ctx.handle, p, 2, 65, -1, out) == M3X_ERR_ARG
        assert lib.m3x_merkleize_chunks_dev(ctx.handle, p, 0, 65, -1, out) == M3X_ERR_ARG
    finally:
        ctx.free(p)
    assert lib.m3x_finalize_root(ctx.handle, data[:32], 0, 65, -1, out) == M3X_ERR_ARG
    assert ctx.finalize_root(data[:32], 64, 64, -1) == data[:32]


# --------------------------------------- 2. finalize_root, sharded registry

@pytest.mark.parametrize("a,b", [(0, 0), (0, 40), (20, 40), (40, 40), (63, 64)])
def test_finalize_root(ctx, a, b):
    node = ssz_ref.seeded_bytes(b"finalize-node", 32)
    for mix in [-1, 0, 2**32 + 5]:
        got = ctx.finalize_root(node, a, b, mix)
        assert got == ssz_ref.finalize(node, a, b, mix), (a, b, mix)


N_LEAVES = 1024


@pytest.fixture(scope="module")
def registry():
    """1024 records, and the reference root of every prefix asked for"""
    ssz = b"".join(ssz_ref.synthetic_validator_ssz(i) for i in range(N_LEAVES))
    roots = {}

    def root_of(n):
        if n not in roots:
            roots[n] = ssz_ref.validator_registry_root(ssz[: 121 * n], n)
        return roots[n]

    return ssz, root_of


def emulated_sharded_root(ctx, ssz, n_validators, n_leaves, world,
                          single_buffer=False):
    """The multi-GPU registry root with every rank emulated in this process:
    rank r hashes records [r*per, r*per + count) as a depth-log2(per) subtree
    (count = what is left of n_validators, 0..per), pairs of subtree roots
    are combined two-to-one, and finalize_root carries the result to depth 40
    and mixes in the length. With single_buffer the shards are read from one
    device buffer at byte offset start * 121."""
    lib = ctx._lib
    per = n_leaves // world
    assert per * world == n_leaves and per & (per - 1) == 0
    depth = per.bit_length() - 1
    out = ctypes.create_string_buffer(32)
    bufs = []
    base = None
    if single_buffer:
        base = ctx.upload(ssz[: 121 * n_validators] + b"\x00" * 4)
        bufs.append(base)
    nodes = []
    try:
        for rank in range(world):
            start = rank * per
            count = min(max(n_validators - start, 0), per)
            if base is not None:
                # an empty shard is never read; keep its pointer in bounds
                dev = ctypes.c_void_p(base.value + (121 * start if count else 0))
            else:
                dev = ctx.upload(ssz[121 * start : 121 * (start + count)]
                                 + b"\x00" * 4)
                bufs.append(dev)
            rc = lib.m3x_validator_subtree_root_dev(ctx.handle, dev, count,
                                                    depth, out)
            assert rc == 0, (rank, rc)
            nodes.append(out.raw)
    finally:
        for p in bufs:
            ctx.free(p)
    level = depth
    while len(nodes) > 1:
        nxt = []
        for i in range(0, len(nodes), 2):
            rc = lib.m3x_merkleize_chunks(ctx.handle, nodes[i] + nodes[i + 1],
                                          2, 1, -1, out)
            assert rc == 0, rc
            nxt.append(out.raw)
        nodes = nxt
        level += 1
    return ctx.finalize_root(nodes[0], level, 40, n_validators)


@pytest.mark.parametrize("n_validators", [1024, 700, 129, 1])
@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_sharded_registry_root(ctx, registry, world, n_validators):
    from lighthouse_amd import tree_hash as th

    ssz, root_of = registry
    want = root_of(n_validators)
    got = emulated_sharded_root(ctx, ssz, n_validators, N_LEAVES, world)
    assert got == want
    assert th.validator_registry_root(ssz[: 121 * n_validators], n_validators,
                                      ctx=ctx) == want


def test_sharded_registry_root_single_buffer(ctx, registry):
    ssz, root_of = registry
    # shards of 256, 256, 188 and 0 records out of one allocation
    got = emulated_sharded_root(ctx, ssz, 700, N_LEAVES, 4, single_buffer=True)
    assert got == root_of(700)


def test_subtree_root_too_many_for_depth(ctx, registry):
    ssz, _ = registry
    out = ctypes.create_string_buffer(32)
    p = ctx.upload(ssz[: 121 * 3] + b"\x00" * 4)
    try:
        rc = ctx._lib.m3x_validator_subtree_root_dev(ctx.handle, p, 3, 1, out)
    finally:
        ctx.free(p)
    assert rc == M3X_ERR_ARG


# ------------------------------------------------------- 3. merkleize_batch

def batch_want(groups):
    return [
        ssz_ref.merkleize(ssz_ref.split_chunks(g, len(g) // 32),
                          ssz_ref.ceil_log2(len(g) // 32))
        for g in groups
    ]


def cut_groups(blob, counts):
    groups, at = [], 0
    for c in counts:
        groups.append(blob[32 * at : 32 * (at + c)])
        at += c
    return groups


def test_batch_every_count(ctx, blob):
    """131 groups = two full waves and a ragged one; group i holds i % 33
    chunks, so every count 0..32 comes up several times"""
    from lighthouse_amd import tree_hash as th

    groups = cut_groups(blob, [i % 33 for i in range(131)])
    got = th.merkleize_batch(groups, ctx=ctx)
    want = batch_want(groups)
    for i in range(131):
        assert got[i] == want[i], (i, i % 33)
    assert got[0] == got[33] == ssz_ref.ZEROS[0]  # merkleize([], 0)


@pytest.mark.parametrize("count", [0, 1, 2, 3, 31, 32])
def test_batch_single_group(ctx, blob, count):
    from lighthouse_amd import tree_hash as th

    groups = cut_groups(blob, [count])
    assert th.merkleize_batch(groups, ctx=ctx) == batch_want(groups)


def test_batch_beyond_pool(ctx, blob):
    """300 groups of 32 chunks are 300 KiB of input: more than the pooled
    256 KiB buffer, so the call allocates"""
    from lighthouse_amd import tree_hash as th

    groups = cut_groups(blob, [32] * 300)
    assert th.merkleize_batch(groups, ctx=ctx) == batch_want(groups)


def test_batch_bad_offsets_rejected(ctx, blob):
    """counts above 32 and decreasing offsets are refused on the host,
    before any launch; the context is untouched"""
    from lighthouse_amd import tree_hash as th

    lib = ctx._lib
    data = blob[: 32 * 40]

    def call(offsets, n_elems):
        off = (ctypes.c_uint32 * len(offsets))(*offsets)
        out = ctypes.create_string_buffer(32 * max(n_elems, 1))
        return lib.m3x_merkleize_batch(ctx.handle, data, off, n_elems, out)

    assert call([0, 33], 1) == M3X_ERR_ARG
    assert call([0, 2, 35], 2) == M3X_ERR_ARG
    assert call([0, 5, 3], 2) == M3X_ERR_ARG
    assert call([4, 0], 1) == M3X_ERR_ARG
    assert call([0], 0) == M3X_ERR_ARG
    assert call([0, 32], 1) == 0
    groups = cut_groups(blob, [3, 0, 32, 17])
    assert th.merkleize_batch(groups, ctx=ctx) == batch_want(groups)


# ---------------------------------------------------------- 4. RegistryCache

@pytest.fixture(scope="module")
def recs():
    return [ssz_ref.synthetic_validator_ssz(i) for i in range(1100)]


def changed(rec: bytes, salt: int) -> bytes:
    """the record with another balance and the slashed flag flipped"""
    bal = (17_000_000_000 + salt).to_bytes(8, "little")
    return rec[:80] + bal + bytes([rec[88] ^ 1]) + rec[89:]


def model_root(leaves) -> bytes:
    """List[Validator, 2^40] root from leaf roots (zero chunks where a slot
    below the length was never written)"""
    return ssz_ref.mix_in_length(ssz_ref.merkleize(leaves, 40), len(leaves))


def make_cache(ctx, recs, n):
    from lighthouse_amd import tree_hash as th

    cache = th.RegistryCache(b"".join(recs[:n]), n, ctx=ctx)
    return cache, [ssz_ref.validator_leaf(r) for r in recs[:n]]


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_cache_build_and_append_at_capacity_edges(ctx, recs, n):
    """capacity is max(256, next power of two): n = 256 is a full cache,
    whose append at index 256 = capacity is refused"""
    cache, leaves = make_cache(ctx, recs, n)
    try:
        assert cache.root() == model_root(leaves)
        if n == 256:
            with pytest.raises(RuntimeError, match=f"rc={M3X_ERR_ARG}"):
                cache.update([n], recs[n])
            assert cache.root() == model_root(leaves)
        else:
            leaves.append(ssz_ref.validator_leaf(recs[n]))
            assert cache.update([n], recs[n]) == model_root(leaves)
            assert cache.root() == model_root(leaves)
    finally:
        cache.close()


def test_cache_append_five_from_empty(ctx, recs):
    cache, leaves = make_cache(ctx, recs, 0)
    try:
        leaves = [ssz_ref.validator_leaf(r) for r in recs[:5]]
        got = cache.update([0, 1, 2, 3, 4], b"".join(recs[:5]))
        assert got == model_root(leaves)
    finally:
        cache.close()


def test_cache_dirty_index_shapes(ctx, recs):
    n = 600  # capacity 1024
    cache, leaves = make_cache(ctx, recs, n)
    cur = list(recs[:n])
    salt = [0]

    def apply(indices):
        """change the records at indices (a repeated index gets the same
        record twice) and check the root"""
        new = {}
        for i in set(indices):
            salt[0] += 1
            new[i] = changed(cur[i], salt[0])
        for i, r in new.items():
            cur[i] = r
            leaves[i] = ssz_ref.validator_leaf(r)
        got = cache.update(list(indices), b"".join(new[i] for i in indices))
        assert got == model_root(leaves), indices

    try:
        assert cache.root() == model_root(leaves)
        apply([300, 301])  # both siblings of one parent
        apply([0, 599])  # first and last record
        apply([599, 598, 2, 3, 1])  # sibling pairs, out of order
        rng = random.Random(65)
        apply(rng.sample(range(n), 65))  # two blocks of the 64-thread kernels
        many = rng.sample(range(n), 100)
        apply(many + many[:40] + [many[0]])  # 141 entries, 41 of them repeats
        apply([7, 123, 7])
        # the last slot of the capacity as an append: the length becomes
        # 1024 and the slots never written count as zero chunks
        rec = changed(recs[1023], 9999)
        leaves += [ssz_ref.ZEROS[0]] * (1023 - n) + [ssz_ref.validator_leaf(rec)]
        assert cache.update([1023], rec) == model_root(leaves)
        assert cache.root() == model_root(leaves)
    finally:
        cache.close()


def test_cache_rejected_update_changes_nothing(ctx, recs):
    """indices [n, capacity]: the second one is out of range, so the call
    is refused, and the first one must not have grown the length"""
    n = 600
    cache, leaves = make_cache(ctx, recs, n)
    try:
        before = cache.root()
        assert before == model_root(leaves)
        with pytest.raises(RuntimeError, match=f"rc={M3X_ERR_ARG}"):
            cache.update([n, 1024], recs[n] + recs[n + 1])
        assert cache.root() == before
        # and the cache goes on from the old length
        leaves.append(ssz_ref.validator_leaf(recs[n]))
        assert cache.update([n], recs[n]) == model_root(leaves)
    finally:
        cache.close()


def test_cache_error_returns(ctx, recs):
    lib = ctx._lib
    out = ctypes.create_string_buffer(32)
    # more dirty indices than the dirty lists hold
    cache, leaves = make_cache(ctx, recs, 300)
    try:
        m = 65537
        idx = (ctypes.c_uint64 * m)()
        rc = lib.m3x_registry_cache_update(ctx.handle, cache._h, idx,
                                           bytes(121 * m), m, out)
        assert rc == M3X_ERR_ARG
        assert cache.root() == model_root(leaves)
    finally:
        cache.close()
    # a registry beyond 2^24 is refused before anything is read or built
    h = ctypes.c_void_p()
    rc = lib.m3x_registry_cache_create(ctx.handle, b"", (1 << 24) + 1,
                                       ctypes.byref(h))
    assert rc == M3X_ERR_ARG
    assert not h


# ------------------------------- 5. registry root forms, root slot, contexts

@pytest.mark.parametrize("n", [0, 1, 3, 256, 257])
def test_registry_root_host_and_dev(ctx, registry, n):
    """n = 0 is the ladder entry plus the length mix, 1 a single leaf with no
    reduce pass, 256 the exact leaf block, 257 a second block; 121 * 3 and
    121 * 257 are ragged modulo 4"""
    from lighthouse_amd import tree_hash as th

    ssz, root_of = registry
    want = root_of(n)
    if n == 0:
        assert want == ssz_ref.mix_in_length(ssz_ref.ZEROS[40], 0)
    assert th.validator_registry_root(ssz[: 121 * n], n, ctx=ctx) == want
    p = ctx.upload(ssz[: 121 * n] + b"\x00" * 4)
    try:
        dev = th.validator_registry_root_dev(p, n, ctx=ctx)
    finally:
        ctx.free(p)
    assert dev == want


def test_root_slot_interleaving(ctx, blob, registry, recs):
    """every call that ends in the context's root slot or its pooled input,
    back to back on one context in both orders: none may see another's
    leftovers"""
    from lighthouse_amd import tree_hash as th

    ssz, root_of = registry
    node = ssz_ref.seeded_bytes(b"interleave-node", 32)
    groups = cut_groups(blob, [3, 0, 32, 17])
    n_cache = 257

    def cache_root():
        cache, _ = make_cache(ctx, recs, n_cache)
        try:
            return cache.root()
        finally:
            cache.close()

    p = ctx.upload(ssz[: 121 * 257] + b"\x00" * 4)
    steps = [
        # 8192 chunks fill the whole pooled input
        ("chunks", lambda: th.merkleize_chunks(blob[: 32 * 8192], 8192, 13, ctx=ctx),
         ssz_ref.merkleize(ssz_ref.split_chunks(blob, 8192), 13)),
        ("registry_dev", lambda: th.validator_registry_root_dev(p, 257, ctx=ctx),
         root_of(257)),
        ("finalize", lambda: ctx.finalize_root(node, 20, 40, 5),
         ssz_ref.finalize(node, 20, 40, 5)),
        ("batch", lambda: th.merkleize_batch(groups, ctx=ctx), batch_want(groups)),
        ("cache", cache_root,
         model_root([ssz_ref.validator_leaf(r) for r in recs[:n_cache]])),
    ]
    try:
        for name, call, want in steps + steps[::-1]:
            assert call() == want, name
    finally:
        ctx.free(p)


def test_ctx_create_invalid_device(ctx, blob):
    """an ordinal the runtime rejects on the host: the half-built context is
    torn down, the out pointer stays null, other contexts are unaffected"""
    import torch

    h = ctypes.c_void_p()
    rc = ctx._lib.m3x_ctx_create(ctypes.byref(h), torch.cuda.device_count())
    assert rc == M3X_ERR_HIP
    assert not h
    host, dev = both_forms(ctx, blob, 8, 3, -1)
    assert host == dev == ssz_ref.merkleize(ssz_ref.split_chunks(blob, 8), 3)
