"""CPU checks of the PeerDAS recovery reference (tests/kzg_recover_ref.py),
the generated constants, and the presence of the recovery surface. No GPU
needed."""
import random
import re
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "tests" / "golden"))

import kzg_cells_ref as C  # noqa: E402
import kzg_recover_ref as RR  # noqa: E402
import kzg_ref as K  # noqa: E402

R = K.BLS_MODULUS
RECOVER_SYMBOLS = ["m3x_kzgc_recover_cells", "m3x_kzgc_recover_cells_dev"]
RNG = random.Random(20260101)
RANDOM_64 = RNG.sample(range(128), 64)
RANDOM_65 = RNG.sample(range(128), 65)
ID_SETS = {
    "first_half": list(range(64)),
    "second_half": list(range(64, 128)),
    "evens": list(range(0, 128, 2)),
    "random_64": RANDOM_64,
    "random_65": RANDOM_65,
    "all_but_77": [c for c in range(128) if c != 77],
    "all": list(range(128)),
}


@pytest.fixture(scope="module")
def cells():
    """The cells of one seeded blob (never mutated)."""
    return C.compute_cells(K.blob_from_seed(b"recover-ref-0"))


@pytest.mark.parametrize("name", list(ID_SETS))
def test_round_trip(cells, name):
    ids = ID_SETS[name]
    assert RR.recover_cells(ids, [cells[c] for c in ids]) == cells


def test_shuffled_ids(cells):
    ids = list(RANDOM_64)
    random.Random(7).shuffle(ids)
    assert ids != RANDOM_64 and sorted(ids) == sorted(RANDOM_64)
    assert RR.recover_cells(ids, [cells[c] for c in ids]) == cells


def test_inconsistent_65_raises(cells):
    known = [list(cells[c]) for c in RANDOM_65]
    known[17][40] = (known[17][40] + 1) % R
    with pytest.raises(ValueError):
        RR.recover_cells(RANDOM_65, known)


def test_changed_64_is_another_polynomial(cells):
    """64 cells always lie on exactly one polynomial of degree < 4096."""
    known = [list(cells[c]) for c in RANDOM_64]
    known[17][40] = (known[17][40] + 1) % R
    got = RR.recover_cells(RANDOM_64, known)
    assert got != cells
    assert [got[c] for c in RANDOM_64] == known


def test_argument_rules(cells):
    with pytest.raises(ValueError):  # k = 63
        RR.recover_cells(list(range(63)), cells[:63])
    with pytest.raises(ValueError):  # a repeated id
        RR.recover_cells(list(range(63)) + [5], cells[:63] + [cells[5]])
    with pytest.raises(ValueError):  # id 128
        RR.recover_cells(list(range(63)) + [128], cells[:64])
    with pytest.raises(ValueError):  # ids and cells disagree in number
        RR.recover_cells(list(range(64)), cells[:65])
    with pytest.raises(ValueError):  # an evaluation equal to r
        RR.recover_cells(list(range(64)), [[R] + list(cells[0][1:])] + cells[1:64])


def test_bytes_form(cells):
    ids = ID_SETS["second_half"]
    got = RR.recover_cells_bytes(ids, [C.cell_to_bytes(cells[c]) for c in ids])
    assert got == [C.cell_to_bytes(c) for c in cells]
    with pytest.raises(ValueError):
        RR.recover_cells_bytes(ids, [bytes(2047)] * 64)


# ------------------------------------------------------------------ surface
def test_header_declares_recovery():
    hdr = (REPO / "include" / "m3x_consensus.h").read_text()
    declared = set(re.findall(r"\b(m3x_\w+)\s*\(", hdr))
    for sym in RECOVER_SYMBOLS:
        assert sym in declared, sym
    assert "24 kzgc_recover" in hdr
    assert "lib.rs:208-216" in hdr


def test_library_exports_recovery():
    import lighthouse_amd._native as native

    lib = native.load()
    for sym in RECOVER_SYMBOLS:
        assert hasattr(lib, sym), f"missing export {sym}"
        assert getattr(lib, sym).argtypes is not None, sym
    assert lib.m3x_abi_version() == 1
    assert native.Ctx.KERNEL_NAMES_KZG_RECOVER == ["kzgc_recover"]
    names = (native.Ctx.KERNEL_NAMES + native.Ctx.KERNEL_NAMES_BLS_TAIL
             + native.Ctx.KERNEL_NAMES_KZG_CELLS
             + native.Ctx.KERNEL_NAMES_KZG_RECOVER)
    assert names.index("kzgc_recover") == 24 and len(names) == 25


def test_python_surface():
    from lighthouse_amd import kzg

    for name in ("recover_all_cells", "recover_all_cells_batch",
                 "recover_all_cells_batch_dev"):
        assert callable(getattr(kzg.Kzg, name)), name
    # the id rules are checked before anything native is touched
    for bad in (list(range(63)), list(range(129)), list(range(63)) + [128],
                list(range(63)) + [0], list(range(63)) + ["x"]):
        with pytest.raises(kzg.KzgError):
            kzg._pack_cell_ids(bad)
    ids = kzg._pack_cell_ids([127] + list(range(63)))
    assert list(ids) == [127] + list(range(63))


def test_generated_constants_header_is_current():
    import gen_kzg_recover_consts as gen

    assert gen.HEADER.read_text() == gen.header_text()
    text = gen.HEADER.read_text()
    mont = lambda v: v * (1 << 256) % R  # noqa: E731
    for name, value in (
        ("FRR_SHIFT_MONT", 7),
        ("FRR_SHIFT_INV_MONT", pow(7, -1, R)),
        ("FRR_SHIFT_POW64_MONT", pow(7, 64, R)),
        ("FRR_SHIFT_POW4096_MONT", pow(7, 4096, R)),
        ("FRR_INV8192_MONT", pow(8192, -1, R)),
        ("FRR_OMEGA128_MONT", C.root_of_unity(128)),
        ("FRR_QUOT_SCALE_MONT", pow(4096 * (pow(7, 8192, R) - 1), -1, R)),
    ):
        m = re.search(name + r"\[8\] = \{([^}]*)\}", text)
        assert m, name
        limbs = [int(w.rstrip("u"), 16) for w in m.group(1).split(", ")]
        assert sum(w << (32 * i) for i, w in enumerate(limbs)) == mont(value), name
