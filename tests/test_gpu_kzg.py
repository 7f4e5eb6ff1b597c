"""GPU KZG blob proof verification vs the Python reference (tests/kzg_ref.py)
and the ceremony / test-setup fixture (tests/golden/kzg_fixtures.json).

Every check is bit-exact. Commitments and proofs for the batch tests are
made at run time under the insecure test setup (tau known): C = [p(tau)]G1,
pi = [(p(tau) - y)/(tau - z)]G1, two oracle scalar multiplications each."""
import ctypes
import hashlib
import json
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "tests" / "golden"))

import kzg_ref as K  # noqa: E402

pytestmark = pytest.mark.gpu

R = K.BLS_MODULUS
INF = K.G1_POINT_AT_INFINITY
SEEDS = [b"gpu-kzg-0", b"gpu-kzg-1", b"gpu-kzg-2"]


def be32(v):
    return v.to_bytes(32, "big")


@pytest.fixture(scope="module")
def fx():
    return json.loads((REPO / "tests" / "golden" / "kzg_fixtures.json").read_text())


@pytest.fixture(scope="module")
def G():
    import gen_bls_fixtures

    return gen_bls_fixtures


@pytest.fixture(scope="module")
def tau(fx):
    seed = fx["test_setup"]["tau_seed"].encode()
    return int.from_bytes(hashlib.sha256(seed).digest(), "big") % R


@pytest.fixture(scope="module")
def g1_mul(oracle, G):
    """[k]G1 compressed, through the oracle."""

    def mul(k):
        k %= R
        if k == 0:
            return INF
        out = ctypes.create_string_buffer(96)
        rc = oracle.m3x_oracle_bls_g1_mul(G.g1_uncompressed(G.G1G), be32(k), out)
        assert rc == 0
        raw = out.raw
        pt = (int.from_bytes(raw[:48], "big"), int.from_bytes(raw[48:], "big"))
        return G.g1_compress(pt)

    return mul


@pytest.fixture(scope="module")
def triples(tau, g1_mul):
    """3 distinct valid (blob, commitment, z, y, proof) under the test setup,
    computed once and shared (never mutated)."""
    out = []
    for seed in SEEDS:
        blob = K.blob_from_seed(seed)
        poly = K.blob_to_polynomial(blob)
        p_tau = K.poly_eval_at_secret(poly, tau)
        c = g1_mul(p_tau)
        z = K.compute_challenge(blob, c)
        y = K.evaluate_polynomial_in_evaluation_form(poly, z)
        q_tau = (p_tau - y) * pow((tau - z) % R, -1, R) % R
        out.append(
            {"blob": blob, "c": c, "z": be32(z), "y": be32(y), "proof": g1_mul(q_tau)}
        )
    return out


@pytest.fixture(scope="module")
def kzg_mod():
    from lighthouse_amd import kzg

    return kzg


@pytest.fixture(scope="module")
def kz(kzg_mod, fx):
    """Kzg under the insecure test setup."""
    return kzg_mod.Kzg(bytes.fromhex(fx["test_setup"]["g2_tau"]))


@pytest.fixture(scope="module")
def kz_ceremony(kzg_mod, fx):
    return kzg_mod.Kzg(bytes.fromhex(fx["ceremony"]["g2_tau"]))


def cols(ts, *keys):
    return [[t[k] for t in ts] for k in keys]


# ------------------------------------------------------------ ceremony cases
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_ceremony_known_answer(kz_ceremony, fx, k):
    mono = [bytes.fromhex(h) for h in fx["ceremony"]["g1_monomial"]]
    zero = bytes(32)
    assert kz_ceremony.verify_kzg_proof(mono[k], zero, zero, mono[k - 1]) is True


def test_ceremony_mismatched_pair(kz_ceremony, fx):
    mono = [bytes.fromhex(h) for h in fx["ceremony"]["g1_monomial"]]
    zero = bytes(32)
    assert kz_ceremony.verify_kzg_proof(mono[3], zero, zero, mono[1]) is False


def test_ceremony_blob_case(kz_ceremony, fx):
    c = fx["ceremony_blob"]
    blob = K.blob_from_seed(bytes.fromhex(c["seed_hex"]))
    commitment, proof = bytes.fromhex(c["commitment"]), bytes.fromhex(c["proof"])
    assert kz_ceremony.verify_blob_kzg_proof(blob, commitment, proof) is True
    assert (
        kz_ceremony.verify_kzg_proof(
            commitment, bytes.fromhex(c["z"]), bytes.fromhex(c["y"]), proof
        )
        is True
    )


def test_fixture_test_cases(kz, fx):
    for c in fx["test_cases"]:
        got = kz.verify_kzg_proof(
            bytes.fromhex(c["commitment"]),
            bytes.fromhex(c["z"]),
            bytes.fromhex(c["y"]),
            bytes.fromhex(c["proof"]),
        )
        assert got is c["verdict"], c["name"]


# ------------------------------------------------- challenge and evaluation
def test_challenge_eval_matches_reference(kzg_mod, triples):
    blobs, cs = cols(triples, "blob", "c")
    got = kzg_mod.blob_challenge_eval(blobs, cs)
    for t, (z, y) in zip(triples, got):
        assert z == t["z"]
        assert y == t["y"]


def test_eval_in_domain_returns_element(kzg_mod, triples):
    t = triples[0]
    z = be32(K.roots_of_unity_brp()[5])
    ((gz, gy),) = kzg_mod.blob_challenge_eval([t["blob"]], [t["c"]], zs=[z])
    assert gz == z
    assert gy == t["blob"][32 * 5 : 32 * 6]


def test_eval_at_zero(kzg_mod, triples):
    t = triples[1]
    want = K.challenge_and_eval(t["blob"], t["c"], z=0)
    ((gz, gy),) = kzg_mod.blob_challenge_eval([t["blob"]], [t["c"]], zs=[bytes(32)])
    assert (gz, gy) == want


# ------------------------------------------------ batch challenge and powers
@pytest.mark.parametrize("n", [1, 3])
def test_batch_challenge_matches_reference(kzg_mod, triples, n):
    cs, zs, ys, ps = cols(triples[:n], "c", "z", "y", "proof")
    want = be32(K.compute_batch_challenge(cs, zs, ys, ps))
    assert kzg_mod.batch_challenge(cs, zs, ys, ps) == want


def test_cancelling_pair_needs_r_powers(kz, triples, G):
    """C1+E and C2-E: the unweighted sum is unchanged, so an implementation
    that forgets the r powers would accept this batch."""
    a, b = triples[0], triples[1]
    e = G.g1_mul(7, G.G1G)
    c1 = G.g1_compress(G.g1_add(G.g1_decompress(a["c"]), e))
    c2 = G.g1_compress(G.g1_add(G.g1_decompress(b["c"]), G.g1_neg(e)))
    zs, ys, ps = cols([a, b], "z", "y", "proof")
    assert kz.verify_kzg_proof_batch([a["c"], b["c"]], zs, ys, ps) is True
    assert kz.verify_kzg_proof_batch([c1, c2], zs, ys, ps) is False


# ------------------------------------------------------------ valid batches
@pytest.mark.parametrize("n", [1, 2, 3])
def test_valid_blob_batch(kz, triples, n):
    blobs, cs, ps = cols(triples[:n], "blob", "c", "proof")
    assert kz.verify_blob_kzg_proof_batch(blobs, cs, ps) is True


def test_valid_blob_batch_crosses_wave(kz, triples):
    ts = [triples[i % 3] for i in range(65)]
    blobs, cs, ps = cols(ts, "blob", "c", "proof")
    assert kz.verify_blob_kzg_proof_batch(blobs, cs, ps) is True


def test_zero_blob_infinity_commitment_and_proof(kz):
    blob = bytes(K.BYTES_PER_BLOB)
    assert kz.verify_blob_kzg_proof(blob, INF, INF) is True
    assert kz.verify_kzg_proof(INF, be32(5), bytes(32), INF) is True
    assert kz.verify_kzg_proof(INF, be32(5), be32(1), INF) is False


def test_empty_batch(kz):
    assert kz.verify_blob_kzg_proof_batch([], [], []) is True
    assert kz.verify_kzg_proof_batch([], [], [], []) is True


# ---------------------------------------------------------- invalid batches
def test_flipped_blob_byte(kz, triples):
    blobs, cs, ps = cols(triples, "blob", "c", "proof")
    bad = bytearray(blobs[1])
    bad[32 * 7 + 31] ^= 0x01
    assert K.blob_to_polynomial(bytes(bad))  # still canonical
    blobs = [blobs[0], bytes(bad), blobs[2]]
    assert kz.verify_blob_kzg_proof_batch(blobs, cs, ps) is False


def test_swapped_proofs(kz, triples):
    blobs, cs, ps = cols(triples, "blob", "c", "proof")
    ps = [ps[1], ps[0], ps[2]]
    assert kz.verify_blob_kzg_proof_batch(blobs, cs, ps) is False


def test_wrong_y(kz, triples):
    t = triples[2]
    assert kz.verify_kzg_proof(t["c"], t["z"], t["y"], t["proof"]) is True
    wrong = be32((int.from_bytes(t["y"], "big") + 1) % R)
    assert kz.verify_kzg_proof(t["c"], t["z"], wrong, t["proof"]) is False


# ---------------------------------------------------------- encoding errors
def test_blob_element_equal_to_modulus(kz, kzg_mod, triples):
    t = triples[0]
    ok = bytearray(t["blob"])
    ok[32 * 9 : 32 * 10] = be32(R - 1)
    ok = bytes(ok)
    want = K.challenge_and_eval(ok, t["c"])
    assert kzg_mod.blob_challenge_eval([ok], [t["c"]]) == [want]
    assert kz.verify_blob_kzg_proof(ok, t["c"], t["proof"]) is False
    bad = bytearray(t["blob"])
    bad[32 * 9 : 32 * 10] = be32(R)
    with pytest.raises(kzg_mod.KzgError):
        kz.verify_blob_kzg_proof(bytes(bad), t["c"], t["proof"])
    with pytest.raises(kzg_mod.KzgError):
        kzg_mod.blob_challenge_eval([bytes(bad)], [t["c"]])


def test_scalar_out_of_range(kz, kzg_mod, triples):
    t = triples[0]
    with pytest.raises(kzg_mod.KzgError):
        kz.verify_kzg_proof(t["c"], be32(R), t["y"], t["proof"])
    with pytest.raises(kzg_mod.KzgError):
        kz.verify_kzg_proof(t["c"], t["z"], be32(R), t["proof"])


def test_commitment_bad_flag_byte(kz, kzg_mod, triples):
    t = triples[0]
    bad = bytes([t["c"][0] & 0x7F]) + t["c"][1:]  # compression bit cleared
    with pytest.raises(kzg_mod.KzgError):
        kz.verify_blob_kzg_proof(t["blob"], bad, t["proof"])
    bad_inf = bytes([0xE0]) + bytes(47)  # infinity with the sign bit set
    with pytest.raises(kzg_mod.KzgError):
        kz.verify_kzg_proof(bad_inf, t["z"], t["y"], t["proof"])


def test_commitment_outside_subgroup(kz, kzg_mod, triples, G):
    x = 0
    while True:
        y = G.fp_sqrt((x**3 + 4) % G.P)
        if y is not None and y != 0:
            break
        x += 1
    pt = (x, y)
    assert G.on_g1(pt)
    assert G.g1_mul(G.R, pt) is not None  # on the curve, not in the subgroup
    t = triples[0]
    with pytest.raises(kzg_mod.KzgError):
        kz.verify_kzg_proof(G.g1_compress(pt), t["z"], t["y"], t["proof"])
    with pytest.raises(kzg_mod.KzgError):
        kz.verify_kzg_proof(t["c"], t["z"], t["y"], G.g1_compress(pt))


def test_g2_tau_infinity_rejected(kzg_mod):
    with pytest.raises(kzg_mod.KzgError):
        kzg_mod.Kzg(bytes([0xC0]) + bytes(95))
    with pytest.raises(kzg_mod.KzgError):
        kzg_mod.Kzg(bytes(96))  # not a compressed encoding at all


def test_length_mismatch(kz, kzg_mod, triples):
    blobs, cs, ps = cols(triples, "blob", "c", "proof")
    with pytest.raises(kzg_mod.KzgError):
        kz.verify_blob_kzg_proof_batch(blobs, cs[:2], ps)
    with pytest.raises(kzg_mod.KzgError):
        kz.verify_blob_kzg_proof_batch(blobs, cs, ps[:1])
    with pytest.raises(kzg_mod.KzgError):
        kz.verify_blob_kzg_proof(blobs[0][:-1], cs[0], ps[0])
    with pytest.raises(kzg_mod.KzgError):
        kz.verify_kzg_proof_batch(cs, [triples[0]["z"]], [triples[0]["y"]], ps)


# ---------------------------------------------------------------- threading
def test_two_contexts_two_threads(kzg_mod, fx, triples):
    """Two threads, each with its own per-thread context and Kzg, one
    verifying a valid batch and one an invalid batch: no cross-talk."""
    from concurrent.futures import ThreadPoolExecutor

    g2_tau = bytes.fromhex(fx["test_setup"]["g2_tau"])
    blobs, cs, ps = cols(triples, "blob", "c", "proof")

    def worker(widx):
        k = kzg_mod.Kzg(g2_tau)  # default_ctx() is per thread
        out = []
        for _ in range(3):
            if widx == 0:
                out.append(k.verify_blob_kzg_proof_batch(blobs, cs, ps))
            else:
                out.append(
                    k.verify_blob_kzg_proof_batch(blobs, cs, [ps[2], ps[1], ps[0]])
                )
        k.close()
        return out

    with ThreadPoolExecutor(max_workers=2) as ex:
        outs = list(ex.map(worker, range(2)))
    assert outs[0] == [True] * 3
    assert outs[1] == [False] * 3
