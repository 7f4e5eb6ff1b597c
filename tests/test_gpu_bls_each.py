"""m3x_bls_verify_each: n signature sets in, n independent verdicts out, one
call (SignatureSet::verify per set, generic_signature_set.rs:111-120).

The expected value of every verdict is m3x_oracle_bls_verify_sets on that one
set alone (n = 1, rands = [1]); for a set without keys or with an empty
signature it is the host rule (False). Oracle verdicts are computed once per
distinct set and shared by the tests.

Workload as tests/test_gpu_bls_perlane.py: set i carries k = 1 + i % 3 public
keys and is signed with the sum of the member secret keys. Shapes:
  n = 1, 3   one wave, k = 1, 2, 3
  n = 65     ragged second wave in the lane-per-set stages; three-pass h2c
  n = 130    a third, two-lane wave
  k = 65, 130  more keys than lanes in k_bls_aggregate_w"""
import ctypes
import hashlib
import json
import os
from contextlib import contextmanager
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P_MOD = int(
    "1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f624"
    "1eabfffeb153ffffb9feffffffffaaab",
    16,
)
N_MAX = 257  # the interleave test's large batch
WIDE = (65, 130)
INF_SIG = bytes([0xC0]) + bytes(95)
M3X_ERR_ARG = -2
K_BLS_FINISH, K_BLS_EACH = 7, 20

GOLDEN = json.loads(
    (Path(__file__).parent / "golden" / "rfc9380_vectors.json").read_text()
)


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


def _compress_g2(uncomp):
    """96B compressed form of an uncompressed G2 point (ZCash flags), as
    tests/test_rfc9380.py does."""
    y_c1 = int.from_bytes(uncomp[96:144], "big")
    y_c0 = int.from_bytes(uncomp[144:192], "big")
    half = (P_MOD - 1) // 2
    big = y_c1 > half if y_c1 != 0 else y_c0 > half
    out = bytearray(uncomp[:96])
    out[0] |= 0x80
    if big:
        out[0] |= 0x20
    return bytes(out)


def _neg_pk(pk):
    y = int.from_bytes(pk[48:], "big")
    return pk[:48] + ((P_MOD - y) % P_MOD).to_bytes(48, "big")


def flatten(sets):
    """[(msg, sig, [pk, ...])] -> the C-ABI's flat buffers."""
    msgs = b"".join(s[0] for s in sets)
    sigs = b"".join(s[1] for s in sets)
    pks = b"".join(b"".join(s[2]) for s in sets)
    offs = [0]
    for s in sets:
        offs.append(offs[-1] + len(s[2]))
    return msgs, sigs, pks, (ctypes.c_uint32 * len(offs))(*offs)


class Workload:
    """A signed pool of N_MAX sets (k = 1 + i % 3) and two wide sets, each a
    (msg, sig, [pk, ...]) tuple, plus the oracle's verdict per distinct set."""

    def __init__(self, oracle):
        self.oracle = oracle
        pool = 3 * N_MAX + sum(WIDE)
        sks = ctypes.create_string_buffer(32 * pool)
        pks = ctypes.create_string_buffer(96 * pool)
        oracle.m3x_oracle_bls_keypool(ctypes.c_uint64(pool), sks, pks)
        sk = [int.from_bytes(sks.raw[32 * j : 32 * (j + 1)], "big") for j in range(pool)]
        self.pk = [pks.raw[96 * j : 96 * (j + 1)] for j in range(pool)]
        members = [list(range(3 * i, 3 * i + 1 + i % 3)) for i in range(N_MAX)]
        at = 3 * N_MAX
        for k in WIDE:
            members.append(list(range(at, at + k)))
            at += k
        total = len(members)
        msgs = [hashlib.sha256(b"each%d" % i).digest() for i in range(total)]
        sign_sks = b"".join(
            (sum(sk[j] for j in m) % ORDER).to_bytes(32, "big") for m in members
        )
        sigs = ctypes.create_string_buffer(96 * total)
        assert (
            oracle.m3x_oracle_bls_sign_batch(
                ctypes.c_uint64(total), sign_sks, b"".join(msgs), sigs
            )
            == 0
        )
        allsets = [
            (msgs[i], sigs.raw[96 * i : 96 * (i + 1)], [self.pk[j] for j in m])
            for i, m in enumerate(members)
        ]
        self.sets = allsets[:N_MAX]
        self.wide = allsets[N_MAX:]
        self._want = {}

    # -- defects: each returns a set derived from `s` that must not verify --
    def d_message(self, s):
        return (hashlib.sha256(b"replaced" + s[0]).digest(), s[1], s[2])

    def d_pubkey_swapped(self, s):
        return (s[0], s[1], s[2][:-1] + [self.pk[3 * N_MAX - 1]])

    def d_sig_off_curve(self, s):
        # smallest tweak of x.c0 for which x^3 + b has no square root
        unc = ctypes.create_string_buffer(192)
        for t in range(1, 64):
            sig = s[1][:95] + bytes([s[1][95] ^ t])
            if self.oracle.m3x_oracle_bls_sig_decompress(sig, unc) != 0:
                return (s[0], sig, s[2])
        raise AssertionError("no off-curve x found")

    def d_sig_noncanonical(self, s):
        return (s[0], s[1][:48] + P_MOD.to_bytes(48, "big"), s[2])

    def d_sig_non_subgroup(self, s):
        pt = bytes.fromhex(GOLDEN["non_subgroup_g2"]["uncompressed"])
        return (s[0], _compress_g2(pt), s[2])

    def d_sig_infinity(self, s):
        return (s[0], INF_SIG, s[2])

    def d_no_keys(self, s):
        return (s[0], s[1], [])

    def d_apk_infinity(self, s):
        return (s[0], s[1], [s[2][0], _neg_pk(s[2][0])])

    def d_pubkey_unparsable(self, s):
        bad = P_MOD.to_bytes(48, "big") + s[2][-1][48:]
        return (s[0], s[1], s[2][:-1] + [bad])

    DEFECTS = [
        "d_message", "d_pubkey_swapped", "d_sig_off_curve",
        "d_sig_noncanonical", "d_sig_non_subgroup", "d_sig_infinity",
        "d_no_keys", "d_apk_infinity", "d_pubkey_unparsable",
    ]

    def want(self, sets):
        out = []
        for s in sets:
            key = (s[0], s[1], tuple(s[2]))
            if key not in self._want:
                if not s[2]:
                    self._want[key] = 0  # host rule: no keys
                else:
                    rnd = (ctypes.c_uint64 * 1)(1)
                    self._want[key] = self.oracle.m3x_oracle_bls_verify_sets(
                        *flatten([s]), rnd, ctypes.c_uint64(1)
                    )
            out.append(self._want[key])
        return out

    def gpu(self, ctx, sets):
        from lighthouse_amd import _native

        n = len(sets)
        verdicts = (ctypes.c_int32 * n)(*([-7] * n))
        rc = _native.load().m3x_bls_verify_each(
            ctx.handle, *flatten(sets), n, verdicts
        )
        assert rc == 0
        return list(verdicts)

    def gpu_batch(self, ctx, sets):
        from lighthouse_amd import _native

        n = len(sets)
        rnds = (ctypes.c_uint64 * n)(
            *[((i * 0x9E3779B97F4A7C15 + 0xC0FFEE) | 1) & (2**64 - 1) for i in range(n)]
        )
        return _native.load().m3x_bls_verify_sets(
            ctx.handle, *flatten(sets), rnds, n
        )

    def defective(self, n=65):
        """n sets with one defect of each kind, at distinct indices that
        include 0, 63, 64 (= n - 1); index 33 is a k = 1 set with an
        unparsable key next to the k = 3 one at 50 (aggregate kernel)."""
        at = {
            0: "d_message", 7: "d_pubkey_swapped", 13: "d_sig_off_curve",
            21: "d_sig_noncanonical", 63: "d_sig_non_subgroup",
            30: "d_sig_infinity", 64: "d_no_keys", 40: "d_apk_infinity",
            50: "d_pubkey_unparsable", 33: "d_pubkey_unparsable",
        }
        sets = list(self.sets[:n])
        for i, d in at.items():
            sets[i] = getattr(self, d)(sets[i])
        return sets, sorted(at)


@pytest.fixture(scope="module")
def ctx():
    from lighthouse_amd import _native

    return _native.default_ctx()


@pytest.fixture(scope="module")
def wl(oracle):
    return Workload(oracle)


@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_each_all_valid(ctx, wl, n):
    sets = wl.sets[:n]
    want = wl.want(sets)
    assert want == [1] * n
    assert wl.gpu(ctx, sets) == want


def test_each_isolation(ctx, wl):
    """One call, nine kinds of defect: a verdict is 0 at exactly the
    defective indices. A flag shared between sets zeroes its neighbours."""
    n = 65
    sets, bad_at = wl.defective(n)
    want = wl.want(sets)
    assert want == [0 if i in bad_at else 1 for i in range(n)]
    assert wl.gpu(ctx, sets) == want
    # every set defective, the kinds cycling through the indices
    allbad = [
        getattr(wl, wl.DEFECTS[i % len(wl.DEFECTS)])(wl.sets[i]) for i in range(n)
    ]
    assert wl.want(allbad) == [0] * n
    assert wl.gpu(ctx, allbad) == [0] * n
    # nothing is left behind on the context
    assert wl.gpu(ctx, wl.sets[:n]) == [1] * n


def test_each_wide_aggregates(ctx, wl):
    w65, w130 = wl.wide
    sets = [wl.sets[0], w65, wl.sets[3], w130, wl.sets[6]]
    assert [len(s[2]) for s in sets] == [1, 65, 1, 130, 1]
    assert wl.want(sets) == [1] * 5
    assert wl.gpu(ctx, sets) == [1] * 5
    keys = list(w130[2])
    keys[97] = wl.pk[0]  # one member replaced by another valid key
    sets[3] = (w130[0], w130[1], keys)
    assert wl.want(sets) == [1, 1, 1, 0, 1]
    assert wl.gpu(ctx, sets) == [1, 1, 1, 0, 1]


@pytest.mark.parametrize("n", [3, 257])
def test_each_and_batch_interleaved(ctx, wl, n):
    """Both pipelines share the context's scratch: a fail flag, aggregate
    count or apk entry left by one changes the other's next result."""
    defects, _ = wl.defective(65)
    want = wl.want(defects)
    valid = wl.sets[:n]
    tampered = list(valid)
    tampered[n // 2] = wl.d_message(valid[n // 2])
    with env(M3X_SMALL_MILLER="0"):
        first = wl.gpu(ctx, defects)
        assert first == want
        assert wl.gpu_batch(ctx, valid) == 1
        assert wl.gpu(ctx, wl.sets[:65]) == [1] * 65
        assert wl.gpu_batch(ctx, tampered) == 0
        assert wl.gpu(ctx, defects) == first


def test_each_dev_entry(ctx, wl):
    from lighthouse_amd import _native

    lib = _native.load()
    n = 65
    sets = list(wl.sets[:n])
    sets[5] = wl.d_message(sets[5])
    sets[64] = wl.d_sig_non_subgroup(sets[64])
    host = wl.gpu(ctx, sets)
    assert host == wl.want(sets)
    msgs, sigs, pks, offs = flatten(sets)
    bufs = [ctx.upload(b) for b in (msgs, sigs, pks, bytes(offs))]
    out_d = ctx.alloc(4 * n)
    try:
        rc = lib.m3x_bls_verify_each_dev(ctx.handle, *bufs, n, out_d)
        assert rc == 0
        got = (ctypes.c_int32 * n)()
        assert lib.m3x_d2h(ctx.handle, got, out_d, 4 * n) == 0
        assert list(got) == host
    finally:
        for p in bufs + [out_d]:
            ctx.free(p)


def _bls_sets(wl, bls, n=8):
    return [
        bls.SignatureSet(
            bls.Signature.from_compressed(s[1]),
            [bls.PublicKey.from_uncompressed(p) for p in s[2]],
            s[0],
        )
        for s in wl.sets[:n]
    ]


def test_each_python_surface(ctx, wl):
    from lighthouse_amd import bls

    sets = _bls_sets(wl, bls)
    sets[1].signature = bls.Signature.empty()  # host short-circuit
    sets[4].signing_keys = []
    sets[6].message = hashlib.sha256(b"tampered").digest()
    got = bls.verify_signature_sets_each(sets, ctx=ctx)
    assert got == [i not in (1, 4, 6) for i in range(8)]


def test_fallback_runs_one_each_call(ctx, wl):
    """The batch-false fallback is one per-set call: one launch of the
    per-set pairing kernel, and one k_bls_finish (the batch attempt)."""
    from lighthouse_amd import bls

    sets = _bls_sets(wl, bls)
    sets[3].message = hashlib.sha256(b"tampered").digest()

    def launches(slot):
        ms, cnt = ctypes.c_double(), ctypes.c_uint64()
        assert ctx._lib.m3x_kernel_ms(
            ctx.handle, slot, ctypes.byref(ms), ctypes.byref(cnt)
        ) == 0
        return cnt.value

    ctx.timing_enable(True)
    try:
        got = bls.verify_signature_sets_with_fallback(sets, ctx=ctx)
        assert launches(K_BLS_EACH) == 1
        assert launches(K_BLS_FINISH) == 1
    finally:
        ctx.timing_enable(False)
    assert got == [i != 3 for i in range(8)]


def test_each_n_zero_and_null_ctx(ctx, wl):
    from lighthouse_amd import _native

    lib = _native.load()
    sentinel = 0x5A5A5A5A
    verdicts = (ctypes.c_int32 * 4)(*([sentinel] * 4))
    offs = (ctypes.c_uint32 * 1)(0)
    assert lib.m3x_bls_verify_each(ctx.handle, b"", b"", b"", offs, 0, verdicts) == 0
    assert list(verdicts) == [sentinel] * 4
    msgs, sigs, pks, offs = flatten(wl.sets[:1])
    assert (
        lib.m3x_bls_verify_each(None, msgs, sigs, pks, offs, 1, verdicts)
        == M3X_ERR_ARG
    )
    assert lib.m3x_bls_verify_each_dev(None, None, None, None, None, 1, None) == M3X_ERR_ARG
