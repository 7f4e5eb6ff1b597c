"""The batch pipeline with the signature sum formed by the bucket MSM, forced
at small n: M3X_SIG_MSM_MIN=1 sends every batch through the MSM on the side
stream and the two-class k_bls_prep_mults2, M3X_SMALL_MILLER=0 through the
per-lane Miller kernel and the two-stream tail, as a 64k-set batch goes.

Every verdict is compared with m3x_oracle_bls_verify_sets on the same
inputs and rands. The workload is the recipe of
tests/test_gpu_bls_perlane.py (copied): set i carries k = 1 + i % 3 public
keys and is signed with the sum of the member secret keys.
  n = 1    one entry per window
  n = 3    k = 1, 2 and 3 aggregates
  n = 65   a ragged second wave in the two-class prepare kernel
  n = 257  sort kernels of more than one block"""
import ctypes
import hashlib
import os
from contextlib import contextmanager

import pytest

pytestmark = pytest.mark.gpu

ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N_MAX = 257
SHAPES = [1, 3, 65, 257]
MSM = {"M3X_SIG_MSM_MIN": "1", "M3X_SMALL_MILLER": "0"}


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
            hashlib.sha256(b"msmpipe%d" % i).digest() for i in range(N_MAX)
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
def test_msm_valid_tampered_valid(ctx, wl, n):
    bad = wl.tampered(n)
    assert wl.want(("ok", n), n) == 1
    assert wl.want(("bad", n), n, msgs=bad) == 0
    with env(**MSM):
        assert wl.gpu(ctx, n) == 1
        assert wl.gpu(ctx, n, msgs=bad) == 0
        # a rejection leaves nothing behind on the context
        assert wl.gpu(ctx, n) == 1


def test_msm_infinity_signature(ctx, wl):
    """An infinity signature is skipped by the sort: alone the sum is
    infinity and the side chain's pairing is e(-g1, O) = 1; among valid
    sets the other signatures still add up."""
    inf_sig = bytes([0xC0]) + bytes(95)
    sigs3 = wl.sigs[:96] + inf_sig + wl.sigs[192:288]
    want1 = wl.want(("inf", 1), 1, sigs=inf_sig)
    want3 = wl.want(("inf", 3), 3, sigs=sigs3)
    assert want3 == 0  # set 1 no longer verifies
    with env(**MSM):
        assert wl.gpu(ctx, 1, sigs=inf_sig) == want1
        assert wl.gpu(ctx, 3, sigs=sigs3) == want3
        assert wl.gpu(ctx, 3) == 1


def test_msm_undecodable_signature(ctx, wl):
    """A signature that does not decode: verdict 0 and no error (the sort
    skips the placeholder), and a valid batch right after it."""
    n = 65
    bad_sig = bytes([0x9F]) + bytes([0xFF]) * 95  # x.c1 >= p
    sigs = wl.sigs[: 96 * 7] + bad_sig + wl.sigs[96 * 8 : 96 * n]
    assert wl.want(("undec", n), n, sigs=sigs) == 0
    with env(**MSM):
        assert wl.gpu(ctx, n, sigs=sigs) == 0
        assert wl.gpu(ctx, n) == 1


def test_msm_large_then_small_same_context(ctx, wl):
    """n = 257 followed at once by n = 3: stale counters, index lists,
    bucket sums or signature sum, or a missing event wait, change the
    second verdict."""
    bad3 = wl.tampered(3)
    bad257 = wl.tampered(257)
    assert wl.want(("bad", 3), 3, msgs=bad3) == 0
    assert wl.want(("bad", 257), 257, msgs=bad257) == 0
    with env(**MSM):
        assert wl.gpu(ctx, 257) == 1
        assert wl.gpu(ctx, 3) == 1
        assert wl.gpu(ctx, 257, msgs=bad257) == 0
        assert wl.gpu(ctx, 3) == 1
        assert wl.gpu(ctx, 257) == 1
        assert wl.gpu(ctx, 3, msgs=bad3) == 0


def test_msm_early_signature_pairing(ctx, wl):
    """M3X_SIGPAIR_EARLY=1 releases k_bls_sigpair right behind the MSM
    instead of behind the per-set Miller kernel (the measured alternative;
    read on every call)."""
    n = 65
    bad = wl.tampered(n)
    assert wl.want(("ok", n), n) == 1
    assert wl.want(("bad", n), n, msgs=bad) == 0
    with env(M3X_SIGPAIR_EARLY="1", **MSM):
        assert wl.gpu(ctx, n) == 1
        assert wl.gpu(ctx, n, msgs=bad) == 0
    with env(M3X_SIGPAIR_EARLY="0", **MSM):
        assert wl.gpu(ctx, n) == 1


def test_threshold_above_n_takes_old_path(ctx, wl):
    """M3X_SIG_MSM_MIN above n: the three-class prepare kernel and the
    two-stage signature reduction still answer, and the switch is read on
    every call."""
    n = 65
    bad = wl.tampered(n)
    assert wl.want(("ok", n), n) == 1
    assert wl.want(("bad", n), n, msgs=bad) == 0
    with env(M3X_SIG_MSM_MIN=str(n + 1), M3X_SMALL_MILLER="0"):
        assert wl.gpu(ctx, n) == 1
        assert wl.gpu(ctx, n, msgs=bad) == 0
    with env(**MSM):
        assert wl.gpu(ctx, n) == 1
    with env(M3X_SIG_MSM_MIN=str(n + 1), M3X_SMALL_MILLER="0"):
        assert wl.gpu(ctx, n) == 1
