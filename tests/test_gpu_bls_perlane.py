"""Small batches forced through the LARGE-batch pipeline: with
M3X_SMALL_MILLER=0 every batch takes the per-lane k_bls_miller, the two-stage
reduce kernels and the two-stream tail (signature chain on the side stream,
GT chain on the main stream, joined by k_bls_finish) — paths the fixture
batches reach only above n = 2048.

Every verdict is compared with m3x_oracle_bls_verify_sets on the same
inputs and rands. Shapes are the smallest that can break something:
  n = 1    one partial, every other reduce thread empty
  n = 3    k = 1, 2 and 3 aggregates
  n = 65   two Miller blocks, ragged last wave; split h2c path (n > 64)
  n = 257  more stage-1 reduce blocks than one, a ragged last one, and
           reduce threads with no element in both stages
With M3X_LATENCY_MAX=0 as well, the batch also takes the kernels that the
dispatch otherwise keeps for n > 2^18: the fused k_bls_prepare and the
default-budget k_bls_h2c_map.
Set i carries k = 1 + i % 3 public keys and is signed with the sum of the
member secret keys."""
import ctypes
import hashlib
import os
from contextlib import contextmanager

import pytest

pytestmark = pytest.mark.gpu

ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N_MAX = 257
SHAPES = [1, 3, 65, 257]


@contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx():
    from lighthouse_amd import _native

    return _native.default_ctx()


class Workload:
    """The first n sets of one signed pool of N_MAX sets, plus the oracle's
    verdict for each variant (computed once, shared by the tests)."""

    def __init__(self, oracle):
        self.oracle = oracle
        pool = 3 * N_MAX
        sks = ctypes.create_string_buffer(32 * pool)
        pks = ctypes.create_string_buffer(96 * pool)
        oracle.m3x_oracle_bls_keypool(ctypes.c_uint64(pool), sks, pks)
        sk_int = [
            int.from_bytes(sks.raw[32 * j : 32 * (j + 1)], "big") for j in range(pool)
        ]
        self.msgs = b"".join(
            hashlib.sha256(b"perlane%d" % i).digest() for i in range(N_MAX)
        )
        sign_sks, pkb, self.offsets = bytearray(), bytearray(), [0]
        for i in range(N_MAX):
            k = 1 + i % 3
            members = range(3 * i, 3 * i + k)
            sign_sks += (sum(sk_int[j] for j in members) % ORDER).to_bytes(32, "big")
            for j in members:
                pkb += pks.raw[96 * j : 96 * (j + 1)]
            self.offsets.append(self.offsets[-1] + k)
        sigs = ctypes.create_string_buffer(96 * N_MAX)
        assert (
            oracle.m3x_oracle_bls_sign_batch(
                ctypes.c_uint64(N_MAX), bytes(sign_sks), self.msgs, sigs
            )
            == 0
        )
        self.sigs = sigs.raw
        self.pks = bytes(pkb)
        self.rands = [(i * 0x9E3779B97F4A7C15 + 0xC0FFEE) | 1 for i in range(N_MAX)]
        self._want = {}

    def args(self, n, msgs=None, sigs=None):
        msgs = self.msgs if msgs is None else msgs
        sigs = self.sigs if sigs is None else sigs
        offs = (ctypes.c_uint32 * (n + 1))(*self.offsets[: n + 1])
        rnds = (ctypes.c_uint64 * n)(*[r & (2**64 - 1) for r in self.rands[:n]])
        return (
            msgs[: 32 * n],
            sigs[: 96 * n],
            self.pks[: 96 * self.offsets[n]],
            offs,
            rnds,
        )

    def tampered(self, n):
        bad = bytearray(self.msgs[: 32 * n])
        j = n // 2
        bad[32 * j : 32 * (j + 1)] = hashlib.sha256(b"tampered").digest()
        return bytes(bad)

    def want(self, key, n, **kw):
        if key not in self._want:
            a = self.args(n, **kw)
            self._want[key] = self.oracle.m3x_oracle_bls_verify_sets(
                *a, ctypes.c_uint64(n)
            )
        return self._want[key]

    def gpu(self, ctx, n, **kw):
        from lighthouse_amd import _native

        a = self.args(n, **kw)
        return _native.load().m3x_bls_verify_sets(ctx.handle, *a, n)


@pytest.fixture(scope="module")
def wl(oracle):
    return Workload(oracle)


@pytest.mark.parametrize("n", SHAPES)
def test_perlane_valid_tampered_valid(ctx, wl, n):
    bad = wl.tampered(n)
    assert wl.want(("ok", n), n) == 1
    assert wl.want(("bad", n), n, msgs=bad) == 0
    with env(M3X_SMALL_MILLER="0"):
        assert wl.gpu(ctx, n) == wl.want(("ok", n), n)
        assert wl.gpu(ctx, n, msgs=bad) == wl.want(("bad", n), n, msgs=bad)
        # a rejection leaves nothing behind on the context
        assert wl.gpu(ctx, n) == wl.want(("ok", n), n)


def test_perlane_large_then_small_same_context(ctx, wl):
    """n = 257 followed at once by n = 3: a stale signature sum, side-stream
    slot or stage buffer, or a missing event wait, changes the second
    verdict."""
    bad3 = wl.tampered(3)
    with env(M3X_SMALL_MILLER="0"):
        assert wl.gpu(ctx, 257) == wl.want(("ok", 257), 257)
        assert wl.gpu(ctx, 3) == wl.want(("ok", 3), 3)
        assert wl.gpu(ctx, 257, msgs=wl.tampered(257)) == wl.want(
            ("bad", 257), 257, msgs=wl.tampered(257)
        )
        assert wl.gpu(ctx, 3) == wl.want(("ok", 3), 3)
        assert wl.gpu(ctx, 257) == wl.want(("ok", 257), 257)
        assert wl.gpu(ctx, 3, msgs=bad3) == wl.want(("bad", 3), 3, msgs=bad3)


def test_perlane_infinity_signature(ctx, wl):
    """One set whose signature is the infinity encoding: the signature sum
    is infinity, so the side chain's pairing is e(-g1, O) = 1."""
    inf_sig = bytes([0xC0]) + bytes(95)
    want = wl.want(("inf", 1), 1, sigs=inf_sig)
    with env(M3X_SMALL_MILLER="0"):
        assert wl.gpu(ctx, 1, sigs=inf_sig) == want
        assert wl.gpu(ctx, 1) == wl.want(("ok", 1), 1)


@pytest.mark.parametrize("n", [3, 65])
def test_large_batch_regime_valid_tampered_valid(ctx, wl, n):
    """M3X_LATENCY_MAX=0 sends a small batch through the kernels that
    otherwise run only above 2^18 sets: the fused k_bls_prepare and the
    default-budget k_bls_h2c_map. n = 3 has k = 1, 2, 3 and the fused
    k_bls_h2c; n = 65 has a ragged second wave and the three-pass h2c
    (k_bls_h2c_expand, k_bls_h2c_map, k_bls_h2c_fin)."""
    bad = wl.tampered(n)
    with env(M3X_LATENCY_MAX="0", M3X_SMALL_MILLER="0"):
        assert wl.gpu(ctx, n) == wl.want(("ok", n), n)
        assert wl.gpu(ctx, n, msgs=bad) == wl.want(("bad", n), n, msgs=bad)
        assert wl.gpu(ctx, n) == wl.want(("ok", n), n)


def test_large_batch_regime_infinity_signature(ctx, wl):
    """k_bls_prepare's sig.inf branch: the set contributes an infinite
    r*sigma and skips the psi subgroup check."""
    inf_sig = bytes([0xC0]) + bytes(95)
    want = wl.want(("inf", 1), 1, sigs=inf_sig)
    with env(M3X_LATENCY_MAX="0", M3X_SMALL_MILLER="0"):
        assert wl.gpu(ctx, 1, sigs=inf_sig) == want
        assert wl.gpu(ctx, 1) == wl.want(("ok", 1), 1)


def test_perlane_split_miller(ctx, wl):
    """The wave-split kernel shares the Miller step helpers; the switch is
    read on every call."""
    n = 65
    bad = wl.tampered(n)
    with env(M3X_SMALL_MILLER="0", M3X_MILLER_SPLIT="1"):
        assert wl.gpu(ctx, n) == wl.want(("ok", n), n)
        assert wl.gpu(ctx, n, msgs=bad) == wl.want(("bad", n), n, msgs=bad)
    with env(M3X_SMALL_MILLER="0", M3X_MILLER_SPLIT="0"):
        assert wl.gpu(ctx, n) == wl.want(("ok", n), n)
