"""CPU checks of the PeerDAS cell reference (tests/kzg_cells_ref.py), the
fixture file, and the presence of the cell-KZG surface. No GPU needed."""
import hashlib
import json
import re
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tests"))

import kzg_cells_ref as C  # noqa: E402
import kzg_ref as K  # noqa: E402

R = K.BLS_MODULUS
CELL_SYMBOLS = [
    "m3x_kzgc_compute_cells",
    "m3x_kzgc_compute_cells_dev",
    "m3x_kzgc_load_cell_setup",
    "m3x_kzgc_verify_cell_proof_batch",
    "m3x_kzgc_cell_batch_challenge_test",
]
FIXTURE_SHA256 = "7c08041ddd30842fc17df5f8d6391f92699bf2708961a1fedf318c351a25a879"
COLS = [0, 1, 2, 63, 64, 127]
TAU = int.from_bytes(hashlib.sha256(b"cells-ref-tau").digest(), "big") % R
CHALLENGE = int.from_bytes(hashlib.sha256(b"cells-ref-r").digest(), "big") % R


@pytest.fixture(scope="module")
def case():
    """One seeded blob with its coefficients and cells (never mutated)."""
    blob = K.blob_from_seed(b"cells-ref-0")
    coef = C.blob_coefficients(blob)
    return {"blob": blob, "poly": K.blob_to_polynomial(blob), "coef": coef,
            "cells": C.cells_from_coefficients(coef)}


def test_first_half_is_the_blob(case):
    cells = case["cells"]
    assert len(cells) == 128 and all(len(c) == 64 for c in cells)
    assert [v for c in cells[:64] for v in c] == case["poly"]
    assert b"".join(C.cell_to_bytes(c) for c in cells[:64]) == case["blob"]


def test_cells_are_the_polynomial_on_the_cosets(case):
    for c in COLS:
        pts = C.coset_points(c)
        assert [C.poly_eval(case["coef"], x) for x in pts] == case["cells"][c]


def test_second_half_by_a_4096_point_transform(case):
    """cells 64..127 = brp(FFT_4096(coef_j * omega_8192^j))"""
    w = C.root_of_unity(8192)
    shifted = [v * pow(w, j, R) % R for j, v in enumerate(case["coef"])]
    odd = K.bit_reversal_permutation(C.fft(shifted, C.root_of_unity(4096)))
    assert [v for c in case["cells"][64:] for v in c] == odd


def test_interpolant_reproduces_the_cell(case):
    for c in COLS:
        coef = C.interpolate_cell(c, case["cells"][c])
        assert len(coef) == 64
        assert [C.poly_eval(coef, x) for x in C.coset_points(c)] == case["cells"][c]


def test_quotient_identity(case):
    p_tau = C.poly_eval(case["coef"], TAU)
    for c in COLS:
        q_tau = C.poly_eval(C.cell_quotient(case["coef"], c), TAU)
        i_tau = C.poly_eval(C.interpolate_cell(c, case["cells"][c]), TAU)
        hc64 = pow(C.coset_shift(c), 64, R)
        assert hc64 == pow(C.root_of_unity(128), K.bitrev(c, 7), R)
        assert q_tau * (pow(TAU, 64, R) - hc64) % R == (p_tau - i_tau) % R


def test_scalar_batch_equation(case):
    p_tau = C.poly_eval(case["coef"], TAU)
    qs = [C.poly_eval(C.cell_quotient(case["coef"], c), TAU) for c in COLS]
    cells = [case["cells"][c] for c in COLS]
    rows = [0] * len(COLS)
    assert C.batch_equation_scalar(TAU, CHALLENGE, [p_tau], rows, COLS, cells, qs)
    bad = [list(c) for c in cells]
    bad[3][5] = (bad[3][5] + 1) % R
    assert not C.batch_equation_scalar(TAU, CHALLENGE, [p_tau], rows, COLS, bad, qs)
    # a column off by one fails too
    assert not C.batch_equation_scalar(
        TAU, CHALLENGE, [p_tau], rows, [1] + COLS[1:], cells, qs)


def test_transcript_layout():
    cs = [bytes([0xC0]) + bytes(47)] * 2
    cells = [bytes(2048), bytes([1]) * 2048]
    proofs = [bytes([0xC0]) + bytes(47)] * 2
    data = C.cell_batch_transcript(cs, [0, 1], [5, 127], cells, proofs)
    assert data[:16] == b"RCKZGCBATCH__V1_"
    assert data[16:48] == b"".join(
        v.to_bytes(8, "big") for v in (4096, 64, 2, 2))
    assert len(data) == 48 + 2 * 48 + 2 * (16 + 2048 + 48)
    second = 48 + 96 + 16 + 2048 + 48
    assert data[second : second + 16] == (1).to_bytes(8, "big") + (127).to_bytes(8, "big")
    assert C.cell_batch_challenge(cs, [0, 1], [5, 127], cells, proofs) < R


def test_fixture_file():
    path = REPO / "tests" / "golden" / "kzg_cell_fixtures.json"
    raw = path.read_bytes()
    assert hashlib.sha256(raw).hexdigest() == FIXTURE_SHA256
    fx = json.loads(raw)
    mono = fx["ceremony"]["g1_monomial"]
    assert len(mono) == 65 and all(len(bytes.fromhex(h)) == 48 for h in mono)
    assert len(bytes.fromhex(fx["ceremony"]["g2_monomial_64"])) == 96
    assert len(bytes.fromhex(fx["test_setup"]["g2_tau64"])) == 96
    old = json.loads((REPO / "tests" / "golden" / "kzg_fixtures.json").read_text())
    assert mono[:5] == old["ceremony"]["g1_monomial"]
    assert fx["test_setup"]["tau_seed"] == old["test_setup"]["tau_seed"]


def test_header_declares_cell_surface():
    hdr = (REPO / "include" / "m3x_consensus.h").read_text()
    declared = set(re.findall(r"\b(m3x_\w+)\s*\(", hdr))
    for sym in CELL_SYMBOLS:
        assert sym in declared, sym
    assert "lib.rs:171-216" in hdr
    for slot in ("21 kzgc_ntt", "22 kzgc_decode", "23 kzgc_combine"):
        assert slot in hdr, slot


def test_library_exports_cell_surface():
    import lighthouse_amd._native as native

    lib = native.load()
    for sym in CELL_SYMBOLS:
        assert hasattr(lib, sym), f"missing export {sym}"
    names = (native.Ctx.KERNEL_NAMES + native.Ctx.KERNEL_NAMES_BLS_TAIL
             + native.Ctx.KERNEL_NAMES_KZG_CELLS)
    assert names[21:] == ["kzgc_ntt", "kzgc_decode", "kzgc_combine"]


def test_python_surface():
    from lighthouse_amd import kzg

    for name in (
        "compute_cells",
        "compute_cells_batch",
        "compute_cells_batch_dev",
        "cells_to_blob",
        "verify_cell_proof_batch",
        "verify_cell_kzg_proof_batch",
        "load_cell_setup",
        "with_cell_setup",
    ):
        assert callable(getattr(kzg.Kzg, name)), name
    cells = [bytes([i]) * 2048 for i in range(128)]
    assert kzg.Kzg.cells_to_blob(cells) == b"".join(cells[:64])
    with pytest.raises(kzg.KzgError):
        kzg.Kzg.cells_to_blob(cells[:127])
    with pytest.raises(kzg.KzgError):
        kzg.Kzg.cells_to_blob(cells[:127] + [bytes(2047)])
