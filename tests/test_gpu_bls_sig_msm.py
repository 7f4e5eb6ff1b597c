"""m3x_bls_sig_sum_test: the batch pipeline's signature sum
sum_i r_i * sigma_i, by the bucket MSM (use_msm = 1) and by the per-set
multiplications with the two-stage reduction (use_msm = 0).

Both are compared, as 192 uncompressed bytes, with an exact-integer affine
G2 (tests/bls_g2_ref.py) fed by m3x_oracle_bls_sig_decompress. Signatures
come from m3x_oracle_bls_sign_batch; -sigma is the same encoding with the
sign flag (0x20) flipped. Nothing here depends on the MSM's window width.

Shapes:
  n = 1     rand 1, 2^64 - 1, 0 (sum at infinity), 2^56 (every digit below
            the top window zero)
  n = 2, 65 one sigma and one rand throughout: the doubling branch of the
            full add, then of the mixed add once a lane holds two equal
            points
  {s, -s}   equal rands, alone (sum at infinity) and beside a third set
  infinity  an infinity signature among valid ones
  n = 257   sort kernels of more than one block, mostly 0-2 entries per
            bucket
  n = 300   all rands equal: one bucket per window holds everything, more
            than a wave's 64 lanes, ragged
  300, 3    one context, for stale counters and index lists"""
import ctypes
import hashlib

import pytest

import bls_g2_ref as g2

pytestmark = pytest.mark.gpu

N_POOL = 300
M64 = 2**64 - 1
INF_SIG = bytes([0xC0]) + bytes(95)


def flip_sign(sig):
    return bytes([sig[0] ^ 0x20]) + sig[1:]


@pytest.fixture(scope="module")
def ctx():
    from lighthouse_amd import _native

    return _native.default_ctx()


class Pool:
    """N_POOL signatures, their exact affine points, and the reference sum
    of each case (computed once, shared by the tests)."""

    def __init__(self, oracle):
        self.oracle = oracle
        sks = ctypes.create_string_buffer(32 * N_POOL)
        pks = ctypes.create_string_buffer(96 * N_POOL)
        oracle.m3x_oracle_bls_keypool(ctypes.c_uint64(N_POOL), sks, pks)
        msgs = b"".join(
            hashlib.sha256(b"sigmsm%d" % i).digest() for i in range(N_POOL)
        )
        sigs = ctypes.create_string_buffer(96 * N_POOL)
        assert (
            oracle.m3x_oracle_bls_sign_batch(
                ctypes.c_uint64(N_POOL), sks.raw, msgs, sigs
            )
            == 0
        )
        self.sigs = [sigs.raw[96 * i : 96 * (i + 1)] for i in range(N_POOL)]
        self._pt = {}
        self._want = {}

    def point(self, sig):
        if sig not in self._pt:
            out = ctypes.create_string_buffer(192)
            assert self.oracle.m3x_oracle_bls_sig_decompress(sig, out) == 0
            self._pt[sig] = g2.from_uncompressed(out.raw)
        return self._pt[sig]

    def want(self, key, sigs, rands):
        if key not in self._want:
            total = g2.weighted_sum([self.point(s) for s in sigs], rands)
            self._want[key] = (g2.to_uncompressed(total), 1 if total is None else 0)
        return self._want[key]


@pytest.fixture(scope="module")
def pool(oracle):
    return Pool(oracle)


def gpu_sum(ctx, sigs, rands, use_msm):
    from lighthouse_amd import _native

    n = len(sigs)
    out = ctypes.create_string_buffer(192)
    rc = _native.load().m3x_bls_sig_sum_test(
        ctx.handle, b"".join(sigs), (ctypes.c_uint64 * n)(*rands), n, use_msm, out
    )
    return rc, out.raw


def check(ctx, pool, key, sigs, rands):
    want, want_inf = pool.want(key, sigs, rands)
    rc_msm, got_msm = gpu_sum(ctx, sigs, rands, 1)
    rc_old, got_old = gpu_sum(ctx, sigs, rands, 0)
    assert rc_msm == want_inf and got_msm == want
    assert rc_old == want_inf and got_old == want
    assert got_msm == got_old
    return want_inf


# the rands of tests/test_gpu_bls_perlane.py
def perlane_rands(n):
    return [((i * 0x9E3779B97F4A7C15 + 0xC0FFEE) | 1) & M64 for i in range(n)]


@pytest.mark.parametrize("rand", [1, M64, 0, 1 << 56])
def test_one_set(ctx, pool, rand):
    inf = check(ctx, pool, ("one", rand), pool.sigs[:1], [rand])
    assert inf == (1 if rand == 0 else 0)


@pytest.mark.parametrize("n", [2, 65])
def test_same_signature_same_rand(ctx, pool, n):
    r = 0xD1B54A32D192ED03
    assert check(ctx, pool, ("same", n), [pool.sigs[7]] * n, [r] * n) == 0


def test_opposite_pair(ctx, pool):
    s = pool.sigs[3]
    r = 0x8CB92BA72F3D8DD7
    assert check(ctx, pool, "pair", [s, flip_sign(s)], [r, r]) == 1
    assert (
        check(ctx, pool, "pair3", [s, pool.sigs[4], flip_sign(s)], [r, 0x1234567, r])
        == 0
    )


def test_infinity_signature_among_valid(ctx, pool):
    sigs = [pool.sigs[0], INF_SIG, pool.sigs[1], pool.sigs[2]]
    assert check(ctx, pool, "inf", sigs, perlane_rands(4)) == 0
    assert check(ctx, pool, "infonly", [INF_SIG], [5]) == 1


def test_n257_sparse_buckets(ctx, pool):
    assert check(ctx, pool, "n257", pool.sigs[:257], perlane_rands(257)) == 0


def test_n300_equal_rands_then_n3(ctx, pool):
    """Every set in one bucket per window (300 entries: four full strides
    of the wave and a ragged fifth), then three sets on the same context:
    counters, cursors or index lists left over from the first call would
    change the second sum."""
    r = 0xA5A5F00F3C3C0FF1
    assert check(ctx, pool, "n300", pool.sigs, [r] * N_POOL) == 0
    assert check(ctx, pool, "n3", pool.sigs[:3], perlane_rands(3)) == 0


def test_undecodable_signature(ctx, pool):
    bad = bytes([0x9F]) + bytes([0xFF]) * 95  # x.c1 >= p
    for use_msm in (1, 0):
        rc, _ = gpu_sum(ctx, [pool.sigs[0], bad], [3, 5], use_msm)
        assert rc == -4  # M3X_ERR_ENCODING
    assert check(ctx, pool, ("one", 1), pool.sigs[:1], [1]) == 0
