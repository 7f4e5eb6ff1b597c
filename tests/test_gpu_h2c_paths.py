"""The hash-to-curve square roots on the GPU, through their test entries:

  m3x_bls_fp2_sqrt_test   fp2_sqrt alone: 0, Fp elements (a0, 0) residue and
                          non-residue, (0, a1), random squares of both signs
                          of t^2 = +-d, random non-squares
  m3x_bls_sswu_test       the two-pow SSWU + isogeny against the exact-integer
                          map (tests/h2c_sqrt_ref.py, itself checked against
                          RFC 9380's map with inversion): u = 0 (tv = 0),
                          (1, 0), (0, 1), (p-1, p-1) and 64 random u covering
                          gx1 square / non-square times either sign of t^2
  m3x_bls_h2c_batch_test  the pipeline's own kernels, fused / split / split
                          latency twins, against the oracle's hash_to_curve
                          with the product DST; n = 65 puts the role split of
                          the 2n-lane map kernel inside a wave, n = 130
                          crosses a block on both roles"""
import ctypes
import hashlib
import random

import pytest

import h2c_sqrt_ref as H

pytestmark = pytest.mark.gpu

G = H.G
P = H.P


@pytest.fixture(scope="module")
def ctx():
    from lighthouse_amd import _native

    return _native.default_ctx()


def _be(a):
    return a[0].to_bytes(48, "big") + a[1].to_bytes(48, "big")


def _fp2(b):
    return (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:96], "big"))


# ------------------------------------------------------------- fp2_sqrt
def _sqrt_cases():
    rng = random.Random(0x51)
    res = next(x for x in range(2, 50) if H.legendre(x) == 1)
    non = next(x for x in range(2, 50) if H.legendre(x) == -1)
    cases = [(0, 0), (res, 0), (non, 0), (P - res, 0), (0, 1), (0, non)]
    cases += [(0, rng.randrange(1, P)) for _ in range(2)]
    squares, nons = [], []
    while len(squares) < 62:
        a = G.f2sq((rng.randrange(P), rng.randrange(P)))
        if a[1]:
            squares.append(a)
    while len(nons) < 62:
        a = (rng.randrange(P), rng.randrange(1, P))
        if H.legendre(H.norm(a)) == -1:
            nons.append(a)
    return cases, squares, nons


def test_fp2_sqrt(ctx):
    from lighthouse_amd import _native

    special, squares, nons = _sqrt_cases()
    # the seed's squares take both branches of the root's select
    assert {H.sqrt_sign(a) for a in squares} == {1, -1}
    cases = special + squares + nons
    n = len(cases)
    assert n == 132  # three blocks, the last one ragged
    out = ctypes.create_string_buffer(96 * n)
    ok = ctypes.create_string_buffer(n)
    rc = _native.load().m3x_bls_fp2_sqrt_test(
        ctx.handle, b"".join(_be(a) for a in cases), n, out, ok
    )
    assert rc == 0
    for i, a in enumerate(cases):
        if a[1] == 0:
            want_ok = True  # every Fp element is a square in Fp2
        else:
            want_ok = H.legendre(H.norm(a)) == 1
        assert bool(ok.raw[i]) == want_ok, (i, a)
        r = _fp2(out.raw[96 * i : 96 * (i + 1)])
        if want_ok:
            assert r[0] < P and r[1] < P
            assert G.f2sq(r) == a, (i, a)
        else:
            assert r == (0, 0)


# ----------------------------------------------------------------- sswu
def test_sswu_matches_reference(ctx):
    from lighthouse_amd import _native

    rng = random.Random(0x52)
    rand_us = [(rng.randrange(P), rng.randrange(P)) for _ in range(64)]
    classes = {H.classify(u) for u in rand_us}
    assert classes == {(True, 1), (True, -1), (False, 1), (False, -1)}
    us = [(0, 0), (1, 0), (0, 1), (P - 1, P - 1)] + rand_us
    n = len(us)
    out = ctypes.create_string_buffer(192 * n)
    rc = _native.load().m3x_bls_sswu_test(
        ctx.handle, b"".join(_be(u) for u in us), n, out
    )
    assert rc == 0
    # the exceptional-input branch (sswu_g2_slow), which no ordinary u
    # reaches, run directly on the same inputs: it is the same map
    slow = ctypes.create_string_buffer(192 * n)
    rc = _native.load().m3x_bls_sswu_slow_test(
        ctx.handle, b"".join(_be(u) for u in us), n, slow
    )
    assert rc == 0
    for i, u in enumerate(us):
        want = G.g2_uncompressed(G.iso_map(G.sswu(u)))
        assert G.g2_uncompressed(H.h2c_point_no_clear(u)) == want
        assert out.raw[192 * i : 192 * (i + 1)] == want, (i, u)
        assert slow.raw[192 * i : 192 * (i + 1)] == want, (i, u)


# ------------------------------------------------------------ h2c batch
N_MAX = 130


@pytest.fixture(scope="module")
def h2c_ref(oracle):
    """N_MAX messages and the oracle's hash_to_curve of each (computed once)."""
    msgs = [hashlib.sha256(b"h2cpaths%d" % i).digest() for i in range(N_MAX)]
    want = []
    for m in msgs:
        out = ctypes.create_string_buffer(192)
        assert oracle.m3x_oracle_h2c_g2_dst(m, 32, G.DST, len(G.DST), out) == 0
        want.append(out.raw)
    return msgs, want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_h2c_batch_modes(ctx, h2c_ref, n):
    from lighthouse_amd import _native

    msgs, want = h2c_ref
    got = []
    for mode in (0, 1, 2):
        out = ctypes.create_string_buffer(192 * n)
        rc = _native.load().m3x_bls_h2c_batch_test(
            ctx.handle, b"".join(msgs[:n]), n, mode, out
        )
        assert rc == 0, mode
        got.append(out.raw)
    assert got[0] == got[1] == got[2]
    for i in range(n):
        assert got[0][192 * i : 192 * (i + 1)] == want[i], i
