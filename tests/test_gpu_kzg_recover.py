"""GPU PeerDAS cell recovery (recover_all_cells) against the Python reference:
expected cells from tests/kzg_cells_ref.py, computed once for three seeded
blobs; the one recovery whose result is not a blob's own cells is compared
with tests/kzg_recover_ref.py. Every comparison is bit-exact."""
import ctypes
import json
import random
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tests"))

import kzg_cells_ref as C  # noqa: E402
import kzg_recover_ref as RR  # noqa: E402
import kzg_ref as K  # noqa: E402

pytestmark = pytest.mark.gpu

R = K.BLS_MODULUS
N = K.FIELD_ELEMENTS_PER_BLOB
SEEDS = [b"gpu-kzgr-0", b"gpu-kzgr-1", b"gpu-kzgr-2"]
RNG = random.Random(20260102)
RANDOM_64 = RNG.sample(range(128), 64)
RANDOM_65 = RNG.sample(range(128), 65)
PATTERNS = {
    "first_half": list(range(64)),
    "second_half": list(range(64, 128)),
    "evens": list(range(0, 128, 2)),
    "odds": list(range(1, 128, 2)),
    "random_64": RANDOM_64,
    "random_65": RANDOM_65,
    "missing_0": list(range(1, 128)),
    "missing_127": list(range(127)),
    "all": list(range(128)),
    "descending": list(range(127, 50, -1)),
    "shuffled": RNG.sample(RANDOM_65, 65),
}


def cell_bytes_of_coefficients(coef):
    coef = list(coef) + [0] * (N - len(coef))
    return [C.cell_to_bytes(c) for c in C.cells_from_coefficients(coef)]


def bump(cell, index):
    """The cell with evaluation `index` changed by 1 (still canonical)."""
    v = (int.from_bytes(cell[32 * index : 32 * index + 32], "big") + 1) % R
    return cell[: 32 * index] + v.to_bytes(32, "big") + cell[32 * index + 32 :]


@pytest.fixture(scope="module")
def kzg_mod():
    from lighthouse_amd import kzg

    return kzg


@pytest.fixture(scope="module")
def kz(kzg_mod):
    fx = json.loads((REPO / "tests" / "golden" / "kzg_fixtures.json").read_text())
    k = kzg_mod.Kzg(bytes.fromhex(fx["test_setup"]["g2_tau"]))  # no cell setup
    yield k
    k.close()


@pytest.fixture(scope="module")
def blobs():
    """[(blob, its 128 reference cells as bytes)], shared and never mutated."""
    out = []
    for seed in SEEDS:
        blob = K.blob_from_seed(seed)
        out.append((blob, cell_bytes_of_coefficients(C.blob_coefficients(blob))))
    return out


# -------------------------------------------------------------- round trips
@pytest.mark.parametrize("name", list(PATTERNS))
def test_round_trip(kz, blobs, name):
    ids = PATTERNS[name]
    _, want = blobs[0]
    got = kz.recover_all_cells(ids, [want[c] for c in ids])
    assert len(got) == 128
    for c in range(128):  # all 128 x 64 elements
        assert got[c] == want[c], c


def test_identity_paths(kz, blobs):
    """k = 64 with ids 0..63: the first half of the output is the input; k =
    128: the output is the input."""
    _, want = blobs[1]
    assert kz.recover_all_cells(range(64), want[:64])[:64] == want[:64]
    assert kz.recover_all_cells(range(128), want) == want


def test_three_blobs_one_id_set(kz, blobs):
    ids = RANDOM_64
    got = kz.recover_all_cells_batch(
        ids, [[want[c] for c in ids] for _, want in blobs])
    assert len(got) == 3
    for cells, (_, want) in zip(got, blobs):
        assert cells == want  # every blob's 128 x 64 elements


def test_zero_blob(kz):
    got = kz.recover_all_cells(PATTERNS["odds"], [bytes(2048)] * 64)
    assert got == [bytes(2048)] * 128


def test_top_monomial(kz):
    """X^4095: the highest coefficient survives the cut at degree 4096."""
    want = cell_bytes_of_coefficients([0] * 4095 + [1])
    for ids in (PATTERNS["second_half"], RANDOM_65):
        assert kz.recover_all_cells(ids, [want[c] for c in ids]) == want


def test_dev_matches_host(kz, blobs):
    ctx = kz._ctx
    ids = RANDOM_65
    raw = b"".join(b"".join(want[c] for c in ids) for _, want in blobs[:2])
    cells_d = ctx.upload(raw)
    out_d = ctx.alloc(2 * 128 * 2048)
    try:
        kz.recover_all_cells_batch_dev(ids, cells_d, 2, out_d)
        got = ctypes.create_string_buffer(2 * 128 * 2048)
        assert ctx._lib.m3x_d2h(ctx.handle, got, out_d, len(got)) == 0
    finally:
        ctx.free(cells_d)
        ctx.free(out_d)
    assert got.raw == b"".join(b"".join(want) for _, want in blobs[:2])


def test_recover_of_compute_cells(kz, blobs):
    blob, _ = blobs[2]
    cells = kz.compute_cells(blob)
    ids = PATTERNS["evens"]
    assert kz.recover_all_cells(ids, [cells[c] for c in ids]) == cells


# -------------------------------------------------------------------- errors
def test_inconsistent_cells(kz, kzg_mod, blobs):
    """One evaluation off by one: an error with 65 cells, another polynomial
    with 64. After each failure a valid call still returns the right cells."""
    _, want = blobs[0]
    _, other = blobs[1]

    def still_good():
        got = kz.recover_all_cells(RANDOM_64, [other[c] for c in RANDOM_64])
        assert got == other

    known = [want[c] for c in RANDOM_65]
    known[17] = bump(known[17], 40)
    with pytest.raises(kzg_mod.KzgError):
        kz.recover_all_cells(RANDOM_65, known)
    still_good()
    with pytest.raises(kzg_mod.KzgError):  # the bad blob is the second of two
        kz.recover_all_cells_batch(
            RANDOM_65, [[other[c] for c in RANDOM_65], known])
    still_good()
    known = [want[c] for c in RANDOM_64]
    known[17] = bump(known[17], 40)
    got = kz.recover_all_cells(RANDOM_64, known)
    assert got == RR.recover_cells_bytes(RANDOM_64, known)
    assert got != want and [got[c] for c in RANDOM_64] == known


def test_malformed_input_raises(kz, kzg_mod, blobs):
    _, want = blobs[0]
    E = kzg_mod.KzgError
    ids = list(range(64))
    good = want[:64]

    def still_good():
        assert kz.recover_all_cells(ids, good) == want

    bad = list(good)
    bad[9] = bad[9][: 32 * 63] + R.to_bytes(32, "big")  # evaluation == r
    with pytest.raises(E):
        kz.recover_all_cells(ids, bad)
    still_good()
    with pytest.raises(E):  # k = 63
        kz.recover_all_cells(ids[:63], good[:63])
    with pytest.raises(E):  # k = 129
        kz.recover_all_cells(list(range(128)) + [0], want + [want[0]])
    with pytest.raises(E):  # id 128
        kz.recover_all_cells(ids[:63] + [128], good)
    with pytest.raises(E):  # a repeated id
        kz.recover_all_cells(ids[:63] + [5], good)
    with pytest.raises(E):  # a cell of 2047 bytes
        kz.recover_all_cells(ids, good[:63] + [good[63][:-1]])
    with pytest.raises(E):  # ids and cells disagree in number
        kz.recover_all_cells(ids, want[:65])
    still_good()
    # the C entry refuses the same arguments before any launch
    raw = b"".join(want)
    out = ctypes.create_string_buffer(128 * 2048)

    def entry(id_list, n=1):
        arr = (ctypes.c_uint64 * len(id_list))(*id_list)
        return kz._lib.m3x_kzgc_recover_cells(
            kz._ctx.handle, arr, len(id_list), raw, n, out)

    assert entry(ids[:63]) == -2
    assert entry(list(range(128)) + [0]) == -2
    assert entry(ids[:63] + [128]) == -2
    assert entry(ids[:63] + [5]) == -2
    assert entry(ids, n=65536) == -2
    assert entry(ids[:63], n=0) == -2  # the checks apply to an empty call too
    assert entry(ids, n=0) == 0
    assert kz.recover_all_cells_batch(ids, []) == []
    assert entry(ids) == 0
    assert out.raw == raw
    still_good()


# --------------------------------------------------------------- timing slot
def test_timing_slot(kz, blobs):
    blob, want = blobs[0]
    ctx = kz._ctx
    ctx.timing_enable(True)
    try:
        kz.recover_all_cells(range(64, 128), want[64:])
        times = ctx.kernel_times()
        assert times["kzgc_recover"][1] > 0
        for name in ("kzgc_ntt", "kzgc_decode", "kzgc_combine"):
            assert times[name][1] == 0, name
        ms = ctypes.c_double()
        launches = ctypes.c_uint64()
        assert ctx._lib.m3x_kernel_ms(
            ctx.handle, 24, ctypes.byref(ms), ctypes.byref(launches)) == 0
        assert launches.value > 0 and ms.value > 0
        assert ctx._lib.m3x_kernel_ms(
            ctx.handle, 25, ctypes.byref(ms), ctypes.byref(launches)) == -2
        # compute_cells reports into slots 21..23 what it did before
        ctx.timing_enable(True)
        kz.compute_cells(blob)
        times = ctx.kernel_times()
        assert times["kzgc_ntt"][1] > 0
        assert times["kzgc_decode"][1] == 0 and times["kzgc_combine"][1] == 0
        assert times["kzgc_recover"][1] == 0
    finally:
        ctx.timing_enable(False)
