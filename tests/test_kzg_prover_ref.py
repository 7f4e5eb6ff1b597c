"""CPU-side checks for KZG commitment / proof computation: the m3x_kzgp_*
C-ABI surface is declared and exported, the Python reference's
Lagrange-form quotient (tests/kzg_prover_ref.py) agrees with the closed
form (p(tau) - y)/(tau - z) at the scalar level, and the ceremony
g1_lagrange fixture is the file its generator recorded."""
import hashlib
import json
import re
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tests"))

import kzg_prover_ref as P  # noqa: E402
import kzg_ref as K  # noqa: E402

R = K.BLS_MODULUS

KZGP_SYMBOLS = [
    "m3x_kzgp_load_g1_lagrange",
    "m3x_kzgp_blob_to_commitment",
    "m3x_kzgp_compute_proof",
    "m3x_kzgp_compute_blob_proof",
    "m3x_kzgp_blob_to_commitment_dev",
    "m3x_kzgp_compute_proof_dev",
    "m3x_kzgp_compute_blob_proof_dev",
]


def test_header_declares_kzgp_surface():
    hdr = (REPO / "include" / "m3x_consensus.h").read_text()
    declared = set(re.findall(r"\b(m3x_\w+)\s*\(", hdr))
    for sym in KZGP_SYMBOLS:
        assert sym in declared, sym
    assert {s for s in declared if s.startswith("m3x_kzgp_")} == set(KZGP_SYMBOLS)
    # each producing entry cites the lib.rs function it replaces
    for line in ("lib.rs:134", "lib.rs:141", "lib.rs:72"):
        assert line in hdr, line


def test_library_exports_kzgp_surface():
    import lighthouse_amd._native as native

    lib = native.load()
    for sym in KZGP_SYMBOLS:
        assert hasattr(lib, sym), f"missing export {sym}"
    names = native.Ctx.KERNEL_NAMES
    assert names[:16][-1] == "kzg_finish"  # existing ids keep their numbers
    assert names[16:] == ["kzgp_quotient", "kzgp_msm", "kzgp_finish"]


def test_python_surface():
    import inspect

    from lighthouse_amd import kzg

    params = list(inspect.signature(kzg.Kzg.__init__).parameters)
    assert params == ["self", "g2_tau", "g1_lagrange", "ctx"]
    for name in (
        "blob_to_kzg_commitment",
        "compute_kzg_proof",
        "compute_blob_kzg_proof",
        "blob_to_kzg_commitment_batch",
        "compute_kzg_proof_batch",
        "compute_blob_kzg_proof_batch",
    ):
        assert callable(getattr(kzg.Kzg, name)), name


@pytest.fixture(scope="module")
def tau():
    return int.from_bytes(hashlib.sha256(b"kzg-prover-ref-tau").digest(), "big") % R


@pytest.fixture(scope="module")
def lag(tau):
    return P.lagrange_scalars_blob_order(tau)


def test_lagrange_scalars(tau, lag):
    roots = K.roots_of_unity_brp()
    assert sum(lag) % R == 1  # the basis sums to the constant 1
    assert sum(l * w for l, w in zip(lag, roots)) % R == tau  # p(X) = X
    # the file order is the bit-reversal of the blob order
    assert K.bit_reversal_permutation(P.lagrange_scalars_file_order(tau)) == lag
    # one entry against the definition, no shared inversion
    i = 1234
    want = (pow(tau, 4096, R) - 1) * pow(4096, -1, R) % R
    want = want * roots[i] % R * pow((tau - roots[i]) % R, -1, R) % R
    assert lag[i] == want


@pytest.mark.parametrize("where", ["outside", "omega_5", "omega_0"])
def test_quotient_matches_closed_form(tau, lag, where):
    poly = K.blob_to_polynomial(K.blob_from_seed(b"prover-ref-" + where.encode()))
    roots = K.roots_of_unity_brp()
    z = {"outside": 0x1234567, "omega_5": roots[5], "omega_0": roots[0]}[where]
    quotient, y = P.compute_kzg_proof_impl(poly, z)
    if where != "outside":
        assert y == poly[roots.index(z)]
    p_tau = sum(f * l for f, l in zip(poly, lag)) % R
    assert p_tau == K.poly_eval_at_secret(poly, tau)
    got = sum(q * l for q, l in zip(quotient, lag)) % R
    assert got == (p_tau - y) * pow((tau - z) % R, -1, R) % R


def test_monomial_blob_quotient_is_previous_monomial():
    poly = K.blob_to_polynomial(P.monomial_blob(3))
    quotient, y = P.compute_kzg_proof_impl(poly, 0)
    assert y == 0
    assert quotient == K.blob_to_polynomial(P.monomial_blob(2))


def test_ceremony_lagrange_fixture():
    golden = REPO / "tests" / "golden"
    fx = json.loads((golden / "kzg_prover_fixtures.json").read_text())
    rec = fx["ceremony_g1_lagrange"]
    raw = (golden / rec["file"]).read_bytes()
    assert len(raw) == 4096 * 48 == rec["bytes"]
    assert rec["points"] == 4096
    assert hashlib.sha256(raw).hexdigest() == rec["sha256"]
    # every entry is a compressed, non-infinity encoding
    assert all(raw[48 * i] & 0xC0 == 0x80 for i in range(4096))
