"""GPU KZG commitments and proofs (blob_to_kzg_commitment, compute_kzg_proof,
compute_blob_kzg_proof): every comparison is bit-exact on bytes.

Three kinds of setup:
  ceremony     the real g1_lagrange list (tests/golden/ceremony_g1_lagrange.bin)
               with the fixture's [tau]G2; expected values are ceremony
               points and results already pinned in kzg_fixtures.json
  known tau    points [L_i(tau)]G1 made by the CPU oracle, so a commitment is
               [p(tau)]G1 and a proof [(p(tau) - y)/(tau - z)]G1: one oracle
               multiplication each, independent of the GPU's Lagrange-form
               quotient
  degenerate   every point +-G1, which forces the doubling, inverse and
               infinity branches of the MSM's additions"""
import ctypes
import hashlib
import json
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "tests" / "golden"))

import kzg_prover_ref as P  # noqa: E402
import kzg_ref as K  # noqa: E402

pytestmark = pytest.mark.gpu

R = K.BLS_MODULUS
N = K.FIELD_ELEMENTS_PER_BLOB
INF = K.G1_POINT_AT_INFINITY
SEEDS = [b"gpu-kzgp-%d" % i for i in range(7)]


def be32(v):
    return (v % R).to_bytes(32, "big")


def int_be(b):
    return int.from_bytes(b, "big")


def blob_of(elems):
    return b"".join(be32(v) for v in elems)


@pytest.fixture(scope="module")
def fx():
    return json.loads((REPO / "tests" / "golden" / "kzg_fixtures.json").read_text())


@pytest.fixture(scope="module")
def G():
    import gen_bls_fixtures

    return gen_bls_fixtures


@pytest.fixture(scope="module")
def kzg_mod():
    from lighthouse_amd import kzg

    return kzg


@pytest.fixture(scope="module")
def tau(fx):
    seed = fx["test_setup"]["tau_seed"].encode()
    return int.from_bytes(hashlib.sha256(seed).digest(), "big") % R


@pytest.fixture(scope="module")
def pt_mul(oracle, G):
    """[k]P compressed through the oracle; P an affine tuple."""

    def mul(k, p=None):
        k %= R
        if k == 0:
            return INF
        out = ctypes.create_string_buffer(96)
        base = G.g1_uncompressed(G.G1G if p is None else p)
        assert oracle.m3x_oracle_bls_g1_mul(base, be32(k), out) == 0
        raw = out.raw
        return G.g1_compress((int_be(raw[:48]), int_be(raw[48:])))

    return mul


# ------------------------------------------------------------------- setups
@pytest.fixture(scope="module")
def kz_ceremony(kzg_mod, fx):
    raw = (REPO / "tests" / "golden" / "ceremony_g1_lagrange.bin").read_bytes()
    k = kzg_mod.Kzg(bytes.fromhex(fx["ceremony"]["g2_tau"]), raw)
    yield k
    k.close()


@pytest.fixture(scope="module")
def tau_points(tau, pt_mul):
    """[L_k(tau)]G1 compressed, in trusted-setup file order (built once)."""
    return [pt_mul(s) for s in P.lagrange_scalars_file_order(tau)]


@pytest.fixture(scope="module")
def kz_tau(kzg_mod, fx, tau_points):
    # a sequence of 4096 48-byte strings, the other accepted form
    k = kzg_mod.Kzg(bytes.fromhex(fx["test_setup"]["g2_tau"]), tau_points)
    yield k
    k.close()


@pytest.fixture(scope="module")
def gen_pts(G):
    g = G.g1_compress(G.G1G)
    return g, G.g1_compress(G.g1_neg(G.G1G))


@pytest.fixture(scope="module")
def kz_all_gen(kzg_mod, fx, gen_pts):
    k = kzg_mod.Kzg(bytes.fromhex(fx["test_setup"]["g2_tau"]), gen_pts[0] * N)
    yield k
    k.close()


@pytest.fixture(scope="module")
def kz_alternating(kzg_mod, fx, gen_pts):
    """Blob order G, -G, G, -G, ...: element i pairs with file entry
    bitrev12(i), so odd elements are the file's upper half."""
    g, neg = gen_pts
    k = kzg_mod.Kzg(
        bytes.fromhex(fx["test_setup"]["g2_tau"]), g * (N // 2) + neg * (N // 2)
    )
    yield k
    k.close()


@pytest.fixture(scope="module")
def cases(tau, pt_mul):
    """7 seeded blobs with their known-tau commitments and proofs at the
    Fiat-Shamir z, computed once and shared (never mutated)."""
    out = []
    for seed in SEEDS:
        blob = K.blob_from_seed(seed)
        poly = K.blob_to_polynomial(blob)
        p_tau = K.poly_eval_at_secret(poly, tau)
        c = pt_mul(p_tau)
        z = K.compute_challenge(blob, c)
        y = K.evaluate_polynomial_in_evaluation_form(poly, z)
        q_tau = (p_tau - y) * pow((tau - z) % R, -1, R) % R
        out.append({"blob": blob, "poly": poly, "p_tau": p_tau, "c": c,
                    "z": be32(z), "y": be32(y), "proof": pt_mul(q_tau)})
    return out


def cols(ts, *keys):
    return [[t[k] for t in ts] for k in keys]


# ----------------------------------------------------------- ceremony setup
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_ceremony_monomial_blob(kz_ceremony, fx, k):
    mono = [bytes.fromhex(h) for h in fx["ceremony"]["g1_monomial"]]
    blob = P.monomial_blob(k)
    assert kz_ceremony.blob_to_kzg_commitment(blob) == mono[k]
    proof, y = kz_ceremony.compute_kzg_proof(blob, bytes(32))
    assert y == bytes(32)
    assert proof == mono[k - 1]


def test_ceremony_constant_blobs(kz_ceremony, gen_pts):
    g, neg = gen_pts
    assert kz_ceremony.blob_to_kzg_commitment(P.constant_blob(1)) == g
    # every scalar r - 1: the signed recoding's top window
    assert kz_ceremony.blob_to_kzg_commitment(P.constant_blob(R - 1)) == neg


def test_ceremony_fixture_blob(kz_ceremony, fx):
    c = fx["ceremony_blob"]
    blob = K.blob_from_seed(bytes.fromhex(c["seed_hex"]))
    commitment = bytes.fromhex(c["commitment"])
    assert kz_ceremony.blob_to_kzg_commitment(blob) == commitment
    assert kz_ceremony.compute_blob_kzg_proof(blob, commitment) == bytes.fromhex(c["proof"])
    proof, y = kz_ceremony.compute_kzg_proof(blob, bytes.fromhex(c["z"]))
    assert y == bytes.fromhex(c["y"])
    assert proof == bytes.fromhex(c["proof"])


@pytest.mark.parametrize("n", [1, 3])
def test_ceremony_round_trip(kz_ceremony, cases, n):
    blobs = [t["blob"] for t in cases[:n]]
    cs = kz_ceremony.blob_to_kzg_commitment_batch(blobs)
    proofs = kz_ceremony.compute_blob_kzg_proof_batch(blobs, cs)
    assert kz_ceremony.verify_blob_kzg_proof_batch(blobs, cs, proofs) is True
    bad = bytearray(blobs[n - 1])
    bad[32 * 11 + 31] ^= 0x01
    assert K.blob_to_polynomial(bytes(bad))  # still canonical
    blobs = blobs[: n - 1] + [bytes(bad)]
    assert kz_ceremony.verify_blob_kzg_proof_batch(blobs, cs, proofs) is False


# ---------------------------------------------------------- known-tau setup
@pytest.mark.parametrize("n", [1, 3, 7])
def test_known_tau_batches(kz_tau, cases, n):
    ts = cases[:n]
    blobs, cs, zs, ys, proofs = cols(ts, "blob", "c", "z", "y", "proof")
    assert kz_tau.blob_to_kzg_commitment_batch(blobs) == cs
    assert kz_tau.compute_blob_kzg_proof_batch(blobs, cs) == proofs
    assert kz_tau.compute_kzg_proof_batch(blobs, zs) == list(zip(proofs, ys))
    # the batch result equals the per-blob results
    for t in ts[-2:]:
        assert kz_tau.blob_to_kzg_commitment(t["blob"]) == t["c"]
        assert kz_tau.compute_blob_kzg_proof(t["blob"], t["c"]) == t["proof"]
        assert kz_tau.compute_kzg_proof(t["blob"], t["z"]) == (t["proof"], t["y"])
    assert kz_tau.verify_blob_kzg_proof_batch(blobs, cs, proofs) is True


def test_known_tau_device_resident_forms(kz_tau, cases):
    """The _dev entries over caller-owned device buffers."""
    ts = cases[:2]
    ctx = kz_tau._ctx
    blobs, cs, zs, ys, proofs = cols(ts, "blob", "c", "z", "y", "proof")
    blobs_d = ctx.upload(b"".join(blobs))
    cs_d = ctx.upload(b"".join(cs))
    zs_d = ctx.upload(b"".join(zs))
    out_d, ys_d = ctx.alloc(96), ctx.alloc(64)

    def fetch(dev, nbytes):
        buf = ctypes.create_string_buffer(nbytes)
        assert ctx._lib.m3x_d2h(ctx.handle, buf, dev, nbytes) == 0
        return buf.raw

    kz_tau.blob_to_kzg_commitment_batch_dev(blobs_d, 2, out_d)
    assert fetch(out_d, 96) == b"".join(cs)
    kz_tau.compute_blob_kzg_proof_batch_dev(blobs_d, cs_d, 2, out_d)
    assert fetch(out_d, 96) == b"".join(proofs)
    kz_tau.compute_kzg_proof_batch_dev(blobs_d, zs_d, 2, cs_d, ys_d)
    assert fetch(cs_d, 96) == b"".join(proofs)
    assert fetch(ys_d, 64) == b"".join(ys)
    for p in (blobs_d, cs_d, zs_d, out_d, ys_d):
        ctx.free(p)


@pytest.mark.parametrize("m", [5, 0])
def test_known_tau_z_in_domain(kz_tau, cases, tau, pt_mul, m):
    t = cases[1]
    z = K.roots_of_unity_brp()[m]
    assert m != 0 or z == 1
    proof, y = kz_tau.compute_kzg_proof(t["blob"], be32(z))
    assert y == t["blob"][32 * m : 32 * m + 32]
    q_tau = (t["p_tau"] - int_be(y)) * pow((tau - z) % R, -1, R) % R
    assert proof == pt_mul(q_tau)
    assert kz_tau.verify_kzg_proof(t["c"], be32(z), y, proof) is True


def test_known_tau_mixed_z_batch(kz_tau, cases, tau, pt_mul):
    """One call with z outside, inside and at zero: blocks do not share state."""
    ts = cases[:3]
    zs = [int_be(ts[0]["z"]), K.roots_of_unity_brp()[4095], 0]
    got = kz_tau.compute_kzg_proof_batch([t["blob"] for t in ts], [be32(z) for z in zs])
    for t, z, (proof, y) in zip(ts, zs, got):
        want_y = K.evaluate_polynomial_in_evaluation_form(t["poly"], z)
        assert y == be32(want_y)
        q_tau = (t["p_tau"] - want_y) * pow((tau - z) % R, -1, R) % R
        assert proof == pt_mul(q_tau)


@pytest.mark.parametrize("j", [0, 1, 4095])
def test_known_tau_sparse_blob_pins_ordering(kz_tau, tau_points, pt_mul, G, j):
    f = int_be(hashlib.sha256(b"sparse-%d" % j).digest()) % R
    blob = blob_of([f if i == j else 0 for i in range(N)])
    setup_point = G.g1_decompress(tau_points[K.bitrev(j)])
    assert kz_tau.blob_to_kzg_commitment(blob) == pt_mul(f, setup_point)


def test_known_tau_zero_blob(kz_tau):
    blob = bytes(K.BYTES_PER_BLOB)
    assert kz_tau.blob_to_kzg_commitment(blob) == INF
    assert kz_tau.compute_blob_kzg_proof(blob, INF) == INF
    assert kz_tau.compute_kzg_proof(blob, be32(5)) == (INF, bytes(32))


# -------------------------------------------------------- degenerate setups
def test_all_generator_setup_doublings(kz_all_gen, cases, pt_mul):
    poly = cases[0]["poly"]
    assert kz_all_gen.blob_to_kzg_commitment(cases[0]["blob"]) == pt_mul(sum(poly))
    # equal scalars everywhere: every pair of partial sums collides
    assert kz_all_gen.blob_to_kzg_commitment(P.constant_blob(3)) == pt_mul(3 * N)
    assert kz_all_gen.blob_to_kzg_commitment(P.constant_blob(R - 1)) == pt_mul(-N)


def test_alternating_setup_equal_pairs_cancel(kz_alternating, cases):
    poly = cases[0]["poly"]
    elems = [poly[i // 2] for i in range(N)]
    assert kz_alternating.blob_to_kzg_commitment(blob_of(elems)) == INF
    assert kz_alternating.blob_to_kzg_commitment(P.constant_blob(R - 1)) == INF


def test_alternating_setup_unequal_pairs(kz_alternating, cases, pt_mul):
    poly = cases[2]["poly"]
    signed = sum(f if i % 2 == 0 else -f for i, f in enumerate(poly))
    assert kz_alternating.blob_to_kzg_commitment(cases[2]["blob"]) == pt_mul(signed)


# ------------------------------------------------------------------- errors
def test_blob_element_equal_to_modulus(kz_tau, kzg_mod, cases):
    t = cases[0]
    for j in (9, 4095):
        bad = bytearray(t["blob"])
        bad[32 * j : 32 * j + 32] = R.to_bytes(32, "big")
        bad = bytes(bad)
        with pytest.raises(kzg_mod.KzgError):
            kz_tau.blob_to_kzg_commitment(bad)
        with pytest.raises(kzg_mod.KzgError):
            kz_tau.compute_kzg_proof(bad, t["z"])
        with pytest.raises(kzg_mod.KzgError):
            kz_tau.compute_blob_kzg_proof(bad, t["c"])
    # one bad blob fails the whole batch
    with pytest.raises(kzg_mod.KzgError):
        kz_tau.blob_to_kzg_commitment_batch([t["blob"], bad])
    # r - 1 is canonical
    ok = bytearray(t["blob"])
    ok[32 * 9 : 32 * 10] = be32(R - 1)
    assert len(kz_tau.blob_to_kzg_commitment(bytes(ok))) == 48


def test_z_out_of_range(kz_tau, kzg_mod, cases):
    t = cases[0]
    with pytest.raises(kzg_mod.KzgError):
        kz_tau.compute_kzg_proof(t["blob"], R.to_bytes(32, "big"))
    with pytest.raises(kzg_mod.KzgError):
        kz_tau.compute_kzg_proof(t["blob"], b"\xff" * 32)


def test_commitment_bad_flag_byte(kz_tau, kzg_mod, cases):
    t = cases[0]
    bad = bytes([t["c"][0] & 0x7F]) + t["c"][1:]  # compression bit cleared
    with pytest.raises(kzg_mod.KzgError):
        kz_tau.compute_blob_kzg_proof(t["blob"], bad)
    bad_inf = bytes([0xE0]) + bytes(47)  # infinity with the sign bit set
    with pytest.raises(kzg_mod.KzgError):
        kz_tau.compute_blob_kzg_proof(t["blob"], bad_inf)
    # infinity itself is a valid commitment: a proof comes back
    assert len(kz_tau.compute_blob_kzg_proof(t["blob"], INF)) == 48


@pytest.fixture(scope="module")
def off_subgroup(G):
    x = 0
    while True:
        y = G.fp_sqrt((x**3 + 4) % G.P)
        if y is not None and y != 0:
            break
        x += 1
    pt = (x, y)
    assert G.on_g1(pt)
    assert G.g1_mul(G.R, pt) is not None  # on the curve, not in the subgroup
    return G.g1_compress(pt)


def test_commitment_outside_subgroup(kz_tau, kzg_mod, cases, off_subgroup):
    t = cases[0]
    with pytest.raises(kzg_mod.KzgError):
        kz_tau.compute_blob_kzg_proof(t["blob"], off_subgroup)
    with pytest.raises(kzg_mod.KzgError):
        kz_tau.compute_blob_kzg_proof_batch(
            [t["blob"], cases[1]["blob"]], [t["c"], off_subgroup]
        )


def test_setup_problems(kzg_mod, fx, gen_pts, off_subgroup):
    g2_tau = bytes.fromhex(fx["test_setup"]["g2_tau"])
    g = gen_pts[0]
    with pytest.raises(kzg_mod.KzgError):  # an infinity point
        kzg_mod.Kzg(g2_tau, g * 7 + INF + g * (N - 8))
    with pytest.raises(kzg_mod.KzgError):  # a point outside the subgroup
        kzg_mod.Kzg(g2_tau, g * (N - 1) + off_subgroup)
    with pytest.raises(kzg_mod.KzgError):  # not an encoding
        kzg_mod.Kzg(g2_tau, bytes(48) + g * (N - 1))
    with pytest.raises(kzg_mod.KzgError):  # wrong lengths
        kzg_mod.Kzg(g2_tau, g * (N - 1))
    with pytest.raises(kzg_mod.KzgError):
        kzg_mod.Kzg(g2_tau, [g] * (N + 1))
    with pytest.raises(kzg_mod.KzgError):
        kzg_mod.Kzg(g2_tau, [g] * (N - 1) + [g[:47]])


def test_no_basis(kzg_mod, fx, cases):
    t = cases[0]
    k = kzg_mod.Kzg(bytes.fromhex(fx["test_setup"]["g2_tau"]))
    with pytest.raises(kzg_mod.KzgError):
        k.blob_to_kzg_commitment(t["blob"])
    with pytest.raises(kzg_mod.KzgError):
        k.compute_kzg_proof(t["blob"], t["z"])
    with pytest.raises(kzg_mod.KzgError):
        k.compute_blob_kzg_proof(t["blob"], t["c"])
    # the C entry itself refuses too (M3X_ERR_ARG), not only the wrapper
    out = ctypes.create_string_buffer(48)
    rc = k._lib.m3x_kzgp_blob_to_commitment(k._ctx.handle, k._h, t["blob"], 1, out)
    assert rc == -2
    # a verification-only handle still verifies
    assert k.verify_blob_kzg_proof(t["blob"], t["c"], t["proof"]) is True
    k.close()


def test_length_mismatch_and_empty(kz_tau, kzg_mod, cases):
    blobs, cs, zs = cols(cases[:3], "blob", "c", "z")
    with pytest.raises(kzg_mod.KzgError):
        kz_tau.compute_blob_kzg_proof_batch(blobs, cs[:2])
    with pytest.raises(kzg_mod.KzgError):
        kz_tau.compute_kzg_proof_batch(blobs, zs[:1])
    with pytest.raises(kzg_mod.KzgError):
        kz_tau.blob_to_kzg_commitment(blobs[0][:-1])
    with pytest.raises(kzg_mod.KzgError):
        kz_tau.compute_kzg_proof(blobs[0], zs[0][:-1])
    with pytest.raises(kzg_mod.KzgError):
        kz_tau.compute_blob_kzg_proof(blobs[0], cs[0] + b"\x00")
    assert kz_tau.blob_to_kzg_commitment_batch([]) == []
    assert kz_tau.compute_kzg_proof_batch([], []) == []
    assert kz_tau.compute_blob_kzg_proof_batch([], []) == []


# ---------------------------------------------------------------- threading
def test_two_contexts_two_threads(kzg_mod, fx, tau_points, cases):
    """Two threads, each with its own per-thread context and Kzg, commit
    different blobs three times: each gets its own right answers."""
    from concurrent.futures import ThreadPoolExecutor

    g2_tau = bytes.fromhex(fx["test_setup"]["g2_tau"])

    def worker(widx):
        k = kzg_mod.Kzg(g2_tau, tau_points)  # default_ctx() is per thread
        mine = cases[2 * widx : 2 * widx + 2]
        out = [
            k.blob_to_kzg_commitment_batch([t["blob"] for t in mine])
            for _ in range(3)
        ]
        k.close()
        return out

    with ThreadPoolExecutor(max_workers=2) as ex:
        outs = list(ex.map(worker, range(2)))
    assert outs[0] == [[cases[0]["c"], cases[1]["c"]]] * 3
    assert outs[1] == [[cases[2]["c"], cases[3]["c"]]] * 3
