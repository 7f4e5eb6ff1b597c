"""CPU-side KZG checks: the new C-ABI surface is declared and exported,
the Python reference (tests/kzg_ref.py) reproduces the committed fixture,
and the ceremony's own points pin the oracle's pairing with an external
known answer: e([tau^k]G1, G2) == e([tau^(k-1)]G1, [tau]G2)."""
import ctypes
import json
import re
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "tests" / "golden"))

import kzg_ref as K  # noqa: E402

KZG_SYMBOLS = [
    "m3x_kzg_create",
    "m3x_kzg_destroy",
    "m3x_kzg_verify_proof",
    "m3x_kzg_verify_proof_batch",
    "m3x_kzg_verify_blob_proof_batch",
    "m3x_kzg_verify_blob_proof_batch_dev",
    "m3x_kzg_blob_challenge_eval",
    "m3x_kzg_batch_challenge_test",
]


@pytest.fixture(scope="module")
def fx():
    return json.loads((REPO / "tests" / "golden" / "kzg_fixtures.json").read_text())


def test_header_declares_kzg_surface():
    hdr = (REPO / "include" / "m3x_consensus.h").read_text()
    declared = set(re.findall(r"\b(m3x_\w+)\s*\(", hdr))
    for sym in KZG_SYMBOLS:
        assert sym in declared, sym
    assert re.search(r"#define\s+M3X_ERR_ENCODING\s+-4\b", hdr)
    # every m3x_kzg_* the header declares is in the list the library test uses
    assert {s for s in declared if s.startswith("m3x_kzg_")} == set(KZG_SYMBOLS)


def test_library_exports_kzg_surface():
    import lighthouse_amd._native as native

    lib = native.load()
    for sym in KZG_SYMBOLS:
        assert hasattr(lib, sym), f"missing export {sym}"


def test_python_surface_constants():
    from lighthouse_amd import kzg

    assert kzg.BYTES_PER_BLOB == 131072 == K.BYTES_PER_BLOB
    assert kzg.FIELD_ELEMENTS_PER_BLOB == 4096
    assert kzg.BYTES_PER_COMMITMENT == kzg.BYTES_PER_PROOF == 48
    assert kzg.BLS_MODULUS == K.BLS_MODULUS
    assert issubclass(kzg.KzgError, Exception)


def test_domain_is_bit_reversed_roots():
    roots = K.roots_of_unity_brp()
    assert len(set(roots)) == 4096 and roots[0] == 1
    assert roots[1] == K.R - 1  # omega^2048
    w = pow(7, (K.R - 1) // 4096, K.R)
    assert roots[5] == pow(w, K.bitrev(5), K.R) and K.bitrev(5) == 0xA00
    assert all(pow(r, 4096, K.R) == 1 for r in roots[:64])


def test_reference_reproduces_fixture(fx):
    cases = [fx["ceremony_blob"]] + [
        c for c in fx["test_cases"] if c["name"].startswith("valid")
    ]
    for c in cases:
        blob = K.blob_from_seed(bytes.fromhex(c["seed_hex"]))
        z, y = K.challenge_and_eval(blob, bytes.fromhex(c["commitment"]))
        assert z.hex() == c["z"], c.get("name")
        assert y.hex() == c["y"], c.get("name")


def test_reference_in_domain_branch():
    blob = K.blob_from_seed(b"in-domain")
    poly = K.blob_to_polynomial(blob)
    roots = K.roots_of_unity_brp()
    for j in (0, 5, 4095):
        assert K.evaluate_polynomial_in_evaluation_form(poly, roots[j]) == poly[j]
    # p(X) = X in evaluation form evaluates to z anywhere
    assert K.evaluate_polynomial_in_evaluation_form(roots, 12345) == 12345


def test_ceremony_pins_oracle_pairing(fx, oracle):
    import gen_bls_fixtures as G

    mono = [G.g1_decompress(bytes.fromhex(h)) for h in fx["ceremony"]["g1_monomial"]]
    g2_tau = G.g2_decompress(bytes.fromhex(fx["ceremony"]["g2_tau"]))
    assert mono[0] == G.G1G

    def pairing(p, q):
        out = ctypes.create_string_buffer(576)
        rc = oracle.m3x_oracle_bls_pairing(
            G.g1_uncompressed(p), G.g2_uncompressed(q), out
        )
        assert rc == 0
        return out.raw

    lhs = {k: pairing(mono[k], G.G2G) for k in range(1, 5)}
    for k in range(1, 5):
        assert lhs[k] == pairing(mono[k - 1], g2_tau), k
    # the mismatched pair differs
    assert lhs[3] != pairing(mono[1], g2_tau)
