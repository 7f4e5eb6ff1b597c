"""CPU checks of the cell-proof method (tests/kzg_cell_proofs_ref.py): the
scalar-field identity the kernels rest on, the generated twiddle header, the
fixture, and the presence of the cell-proof surface. No GPU needed."""
import hashlib
import json
import re
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "tests" / "golden"))

import kzg_cell_proofs_ref as CP  # noqa: E402
import kzg_cells_ref as C  # noqa: E402
import kzg_ref as K  # noqa: E402

R = K.BLS_MODULUS
N = K.FIELD_ELEMENTS_PER_BLOB
PROOF_SYMBOLS = [
    "m3x_kzgc_load_g1_monomial",
    "m3x_kzgc_compute_cells_and_proofs",
    "m3x_kzgc_compute_cells_and_proofs_dev",
    "m3x_kzgc_recover_cells_and_proofs",
    "m3x_kzgc_recover_cells_and_proofs_dev",
]


def seeded(tag, count):
    return [
        int.from_bytes(hashlib.sha256(tag + i.to_bytes(4, "little")).digest(),
                       "big") % R
        for i in range(count)
    ]


# ----------------------------------------------------------------- identity
def test_dif_of_toeplitz_sums_is_every_cell_quotient():
    """A seeded p and tau, every [k]G1 replaced by k: the 128 outputs of the
    DIF over h equal q_c(tau), q_c = p // (X^64 - y_c), for all 128 cells."""
    coef = seeded(b"cell-proofs-ref-p", N)
    tau = seeded(b"cell-proofs-ref-tau", 1)[0]
    assert CP.cell_proof_scalars(coef, tau) == CP.cell_proof_scalars_direct(coef, tau)


@pytest.mark.parametrize("k", [63, 64, 127, 128, 4032, 4095])
def test_monomial_shapes(k):
    """X^k: q_c = sum_m y_c^m X^(k - 64(m+1)); what the GPU tests pin."""
    tau = seeded(b"cell-proofs-ref-tau", 1)[0]
    coef = [0] * k + [1] + [0] * (N - 1 - k)
    got = CP.cell_proof_scalars(coef, tau)
    for c in range(128):
        y = pow(C.coset_shift(c), 64, R)
        want = sum(pow(y, m, R) * pow(tau, k - 64 * (m + 1), R)
                   for m in range(k // 64)) % R
        assert got[c] == want, c
    if k == 63:
        assert got == [0] * 128
    if k == 64:
        assert got == [1] * 128


def test_signed_digits():
    for s in [0, 1, 8, 9, 15, 16, 0x88, 0x89, R - 1, (1 << 255) - 1,
              int("8" * 63, 16), int("8" * 63, 16) + 1] + seeded(b"digits", 8):
        d = CP.signed_digits(s)
        assert len(d) == 64 and all(-7 <= v <= 8 for v in d)
        assert sum(v << (4 * k) for k, v in enumerate(d)) == s


def test_block_numbering():
    assert CP.first_block(0) == 0 and CP.first_block(1) == 63
    assert CP.first_block(62) == 2015
    seen = [CP.first_block(m) + bx for m in range(63) for bx in range(63 - m)]
    assert seen == list(range(2016))


# ------------------------------------------------------------------ fixture
def test_fixture_matches_cell_fixtures():
    raw = (REPO / "tests" / "golden" / "ceremony_g1_monomial.bin").read_bytes()
    assert len(raw) == N * 48
    cfx = json.loads(
        (REPO / "tests" / "golden" / "kzg_cell_fixtures.json").read_text())
    mono = [bytes.fromhex(h) for h in cfx["ceremony"]["g1_monomial"]]
    assert len(mono) >= 65
    for j in range(65):
        assert raw[48 * j : 48 * j + 48] == mono[j], j
    # compressed, none infinity, all distinct
    pts = [raw[48 * j : 48 * j + 48] for j in range(N)]
    assert all(p[0] & 0x80 and not p[0] & 0x40 for p in pts)
    assert len(set(pts)) == N


# ------------------------------------------------------------------ surface
def test_generated_constants_header_is_current():
    import gen_kzg_cell_proof_consts as gen

    assert gen.HEADER.read_text() == gen.header_text()
    text = gen.HEADER.read_text()
    rows = re.findall(r"^    \{([^}]*)\},$", text, re.M)
    assert len(rows) == 64
    w128 = C.root_of_unity(128)
    for k, row in enumerate(rows):
        by = bytes(int(b, 16) for b in row.split(", "))
        assert len(by) == 32
        assert int.from_bytes(by, "big") == pow(w128, k, R), k


def test_header_declares_cell_proofs():
    hdr = (REPO / "include" / "m3x_consensus.h").read_text()
    declared = set(re.findall(r"\b(m3x_\w+)\s*\(", hdr))
    for sym in PROOF_SYMBOLS:
        assert sym in declared, sym
    assert "lib.rs:171-185" in hdr
    assert "27 kzgc_toeplitz" in hdr and "28 kzgc_proof_dft" in hdr
    assert "proofs are not computed" not in hdr
    assert "proofs are not recomputed" not in hdr
    for doc in ("README.md", "INTEGRATION.md"):
        text = " ".join((REPO / doc).read_text().split())
        assert "proofs are not computed" not in text, doc
        assert "compute_cells_and_kzg_proofs" in text, doc


def test_library_exports_cell_proofs():
    import lighthouse_amd._native as native

    lib = native.load()
    for sym in PROOF_SYMBOLS:
        assert hasattr(lib, sym), f"missing export {sym}"
        assert getattr(lib, sym).argtypes is not None, sym
    assert lib.m3x_abi_version() == 1
    assert native.Ctx.KERNEL_NAMES_KZG_CELL_PROOFS == [
        "kzgc_toeplitz", "kzgc_proof_dft"]
    assert native.Ctx.KERNEL_ID_KZG_CELL_PROOFS == 27


class _NoNative:
    """Stands in for the library: any native call fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the argument checks")


def _bare_kzg(kzg, monomial):
    k = object.__new__(kzg.Kzg)
    k._lib = _NoNative()
    k._ctx = None
    k._h = None
    k._has_basis = k._has_cell_setup = False
    k._has_monomial = monomial
    return k


def test_python_surface():
    from lighthouse_amd import kzg

    for name in ("load_g1_monomial", "compute_cells_and_kzg_proofs",
                 "compute_cells_and_kzg_proofs_batch",
                 "compute_cells_and_kzg_proofs_batch_dev",
                 "recover_cells_and_kzg_proofs",
                 "recover_cells_and_kzg_proofs_batch",
                 "recover_cells_and_kzg_proofs_batch_dev"):
        assert callable(getattr(kzg.Kzg, name)), name
    blob, cell = bytes(kzg.BYTES_PER_BLOB), bytes(kzg.BYTES_PER_CELL)
    ids = list(range(64))
    # no monomial load: every producing call raises before native code
    k = _bare_kzg(kzg, monomial=False)
    for call in (
        lambda: k.compute_cells_and_kzg_proofs(blob),
        lambda: k.compute_cells_and_kzg_proofs_batch([blob, blob]),
        lambda: k.compute_cells_and_kzg_proofs_batch_dev(None, 1, None, None),
        lambda: k.recover_cells_and_kzg_proofs(ids, [cell] * 64),
        lambda: k.recover_cells_and_kzg_proofs_batch(ids, [[cell] * 64]),
        lambda: k.recover_cells_and_kzg_proofs_batch_dev(ids, None, 1, None, None),
    ):
        with pytest.raises(kzg.KzgError):
            call()
    # wrong lengths in load_g1_monomial
    for bad in (bytes(48 * N - 1), [bytes(48)] * (N - 1),
                [bytes(48)] * (N - 1) + [bytes(47)]):
        with pytest.raises(kzg.KzgError):
            k.load_g1_monomial(bad)
    # with a load recorded: a second load, wrong lengths, the id rules
    k = _bare_kzg(kzg, monomial=True)
    with pytest.raises(kzg.KzgError):
        k.load_g1_monomial(bytes(48 * N))
    with pytest.raises(kzg.KzgError):
        k.compute_cells_and_kzg_proofs(blob[:-1])
    with pytest.raises(kzg.KzgError):
        k.compute_cells_and_kzg_proofs_batch_dev(None, 65536, None, None)
    for bad in (list(range(63)), list(range(63)) + [128], list(range(63)) + [0]):
        with pytest.raises(kzg.KzgError):
            k.recover_cells_and_kzg_proofs(bad, [cell] * len(bad))
        with pytest.raises(kzg.KzgError):
            k.recover_cells_and_kzg_proofs_batch_dev(bad, None, 1, None, None)
    with pytest.raises(kzg.KzgError):  # ids and cells disagree in number
        k.recover_cells_and_kzg_proofs(ids, [cell] * 65)
    with pytest.raises(kzg.KzgError):  # a short cell
        k.recover_cells_and_kzg_proofs(ids, [cell] * 63 + [cell[:-1]])
    assert k.compute_cells_and_kzg_proofs_batch([]) == []
    assert k.recover_cells_and_kzg_proofs_batch(ids, []) == []
