"""GPU PeerDAS cell KZG (compute_cells, verify_cell_proof_batch) against the
Python reference (tests/kzg_cells_ref.py). Every comparison is bit-exact.

Two setups:
  known tau   g1_monomial[j] = [tau^j]G1 from the CPU oracle and the
              fixture's [tau^64]G2; a commitment is [p(tau)]G1 and the proof
              of cell c is [q_c(tau)]G1 with q_c = p // (X^64 - h_c^64), one
              oracle multiplication each
  ceremony    the fixture's g1_monomial[0..64) and g2_monomial[64], with
              commitments from the existing Lagrange-basis handle; a blob
              X^64 + a(X), deg a < 64, has quotient 1 at every cell, so every
              proof is the G1 generator"""
import ctypes
import hashlib
import json
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "tests" / "golden"))

import kzg_cells_ref as C  # noqa: E402
import kzg_ref as K  # noqa: E402

pytestmark = pytest.mark.gpu

R = K.BLS_MODULUS
N = K.FIELD_ELEMENTS_PER_BLOB
INF = K.G1_POINT_AT_INFINITY
SEEDS = [b"gpu-kzgc-0", b"gpu-kzgc-1", b"gpu-kzgc-2"]


def be32(v):
    return (v % R).to_bytes(32, "big")


def int_be(b):
    return int.from_bytes(b, "big")


def blob_of_coefficients(coef):
    """The blob (evaluation form, blob order) of a coefficient list."""
    coef = list(coef) + [0] * (N - len(coef))
    cells = C.cells_from_coefficients(coef)
    return b"".join(C.cell_to_bytes(c) for c in cells[:64])


def seeded_scalars(tag, count):
    return [
        int_be(hashlib.sha256(tag + i.to_bytes(4, "little")).digest()) % R
        for i in range(count)
    ]


@pytest.fixture(scope="module")
def fx():
    return json.loads((REPO / "tests" / "golden" / "kzg_fixtures.json").read_text())


@pytest.fixture(scope="module")
def cfx():
    return json.loads(
        (REPO / "tests" / "golden" / "kzg_cell_fixtures.json").read_text())


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
    return int_be(hashlib.sha256(seed).digest()) % R


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
        return G.g1_compress((int_be(raw[:48]), int_be(raw[48:])))

    return mul


class BlobCase:
    """A blob with its reference cells and, under the known tau, its
    commitment and (computed on first use, then kept) its cell proofs."""

    def __init__(self, blob, tau, g1_mul):
        self.blob = blob
        self.coef = C.blob_coefficients(blob)
        self.cells = C.cells_from_coefficients(self.coef)
        self.cell_bytes = [C.cell_to_bytes(c) for c in self.cells]
        self._tau, self._mul, self._proofs = tau, g1_mul, {}
        self.c = g1_mul(C.poly_eval(self.coef, tau))

    def proof(self, col):
        if col not in self._proofs:
            q_tau = C.poly_eval(C.cell_quotient(self.coef, col), self._tau)
            self._proofs[col] = self._mul(q_tau)
        return self._proofs[col]


@pytest.fixture(scope="module")
def blobs(tau, g1_mul):
    """Three seeded blobs, computed once and shared (never mutated)."""
    return [BlobCase(K.blob_from_seed(s), tau, g1_mul) for s in SEEDS]


@pytest.fixture(scope="module")
def tau_setup(fx, cfx, tau, g1_mul):
    mono = b"".join(g1_mul(pow(tau, j, R)) for j in range(64))
    return mono, bytes.fromhex(cfx["test_setup"]["g2_tau64"])


@pytest.fixture(scope="module")
def kz(kzg_mod, fx, tau_setup):
    k = kzg_mod.Kzg.with_cell_setup(
        bytes.fromhex(fx["test_setup"]["g2_tau"]), tau_setup)
    yield k
    k.close()


def batch(cases, picks):
    """(cells, proofs, coordinates, commitments) for picks = [(row, col)]."""
    return (
        [cases[r].cell_bytes[c] for r, c in picks],
        [cases[r].proof(c) for r, c in picks],
        list(picks),
        [b.c for b in cases],
    )


# ------------------------------------------------------------ compute_cells
@pytest.mark.parametrize("n", [1, 3])
def test_compute_cells_matches_reference(kz, blobs, n):
    got = kz.compute_cells_batch([b.blob for b in blobs[:n]])
    assert len(got) == n
    for cells, want in zip(got, blobs):
        assert len(cells) == 128
        for c in range(128):  # all 128 x 64 elements
            assert cells[c] == want.cell_bytes[c], c
        assert b"".join(cells[:64]) == want.blob
        assert kz.cells_to_blob(cells) == want.blob


@pytest.mark.parametrize("k", [1, 4095])
def test_compute_cells_monomial(kz, k):
    blob = blob_of_coefficients([0] * k + [1])
    cells = kz.compute_cells(blob)
    for c in range(128):
        want = b"".join(be32(pow(x, k, R)) for x in C.coset_points(c))
        assert cells[c] == want, c


def test_compute_cells_zero_blob(kz):
    assert kz.compute_cells(bytes(K.BYTES_PER_BLOB)) == [bytes(2048)] * 128


def test_compute_cells_dev_matches_host(kz, blobs):
    ctx = kz._ctx
    raw = blobs[0].blob + blobs[1].blob
    blobs_d = ctx.upload(raw)
    out_d = ctx.alloc(2 * 128 * 2048)
    try:
        kz.compute_cells_batch_dev(blobs_d, 2, out_d)
        got = ctypes.create_string_buffer(2 * 128 * 2048)
        assert ctx._lib.m3x_d2h(ctx.handle, got, out_d, len(got)) == 0
    finally:
        ctx.free(blobs_d)
        ctx.free(out_d)
    assert got.raw == b"".join(blobs[0].cell_bytes + blobs[1].cell_bytes)


@pytest.mark.parametrize("index", [9, 4095])
def test_compute_cells_non_canonical(kz, kzg_mod, blobs, index):
    bad = bytearray(blobs[0].blob)
    bad[32 * index : 32 * index + 32] = R.to_bytes(32, "big")
    with pytest.raises(kzg_mod.KzgError):
        kz.compute_cells(bytes(bad))
    with pytest.raises(kzg_mod.KzgError):
        kz.compute_cells_batch([blobs[1].blob, bytes(bad)])
    # the next call is untouched by the failed one
    assert kz.compute_cells(blobs[1].blob) == blobs[1].cell_bytes


def test_compute_cells_lengths_and_empty(kz, kzg_mod, blobs):
    assert kz.compute_cells_batch([]) == []
    with pytest.raises(kzg_mod.KzgError):
        kz.compute_cells(blobs[0].blob[:-1])
    assert kz._lib.m3x_kzgc_compute_cells(kz._ctx.handle, None, 0, None) == 0


# ----------------------------------------------------------- challenge seam
@pytest.mark.parametrize("picks", [[(0, 5)], [(0, 0), (1, 127), (1, 64)]])
def test_challenge_matches_reference(kzg_mod, blobs, picks):
    cases = blobs[: max(r for r, _ in picks) + 1]
    cells, proofs, coords, cs = batch(cases, picks)
    want = C.cell_batch_challenge(
        cs, [r for r, _ in picks], [c for _, c in picks], cells, proofs)
    assert kzg_mod.cell_batch_challenge(cells, proofs, coords, cs) == be32(want)


# -------------------------------------------------------- verify: true cases
def test_verify_one_cell(kz, blobs):
    for col in (0, 77, 127):
        assert kz.verify_cell_proof_batch(*batch(blobs[:1], [(0, col)])) is True


def test_verify_sidecar_shape(kz, blobs):
    """one column, two blobs"""
    assert kz.verify_cell_proof_batch(*batch(blobs[:2], [(0, 70), (1, 70)])) is True


def test_verify_all_cells_of_a_blob(kz, blobs):
    picks = [(0, c) for c in range(128)]
    assert kz.verify_cell_proof_batch(*batch(blobs[:1], picks)) is True


def test_verify_65_cells_two_blobs(kz, blobs):
    """65 cells: one more than a wave of lanes"""
    picks = [(0, c) for c in range(40)] + [(1, 127 - c) for c in range(25)]
    assert len(picks) == 65
    assert kz.verify_cell_proof_batch(*batch(blobs[:2], picks)) is True


def test_verify_repeated_cell(kz, blobs):
    assert kz.verify_cell_proof_batch(*batch(blobs[:1], [(0, 3), (0, 3)])) is True


def test_verify_unreferenced_commitment(kz, blobs):
    cells, proofs, coords, cs = batch(blobs[:3], [(0, 1), (2, 100)])
    assert len(cs) == 3
    assert kz.verify_cell_proof_batch(cells, proofs, coords, cs) is True


def test_verify_empty(kz, blobs):
    assert kz.verify_cell_proof_batch([], [], [], []) is True
    assert kz.verify_cell_proof_batch([], [], [], [blobs[0].c]) is True
    assert kz.verify_cell_kzg_proof_batch([], [], [], []) is True
    rc = kz._lib.m3x_kzgc_verify_cell_proof_batch(
        kz._ctx.handle, kz._h, None, 0, None, None, None, None, 0)
    assert rc == 1


def test_verify_zero_blob(kz):
    """commitment, proofs and cells all infinity / zero"""
    picks = [0, 64, 127]
    assert kz.verify_cell_proof_batch(
        [bytes(2048)] * 3, [INF] * 3, [(0, c) for c in picks], [INF]) is True


def test_verify_low_degree_blob(kz, tau, g1_mul):
    """degree < 64: every quotient is zero, the interpolant is the polynomial"""
    coef = seeded_scalars(b"gpu-kzgc-low", 64)
    case = BlobCase(blob_of_coefficients(coef), tau, g1_mul)
    assert case.coef == coef + [0] * (N - 64)
    picks = [(0, 0), (0, 64), (0, 65), (0, 127)]
    cells, proofs, coords, cs = batch([case], picks)
    assert proofs == [INF] * 4
    assert kz.verify_cell_proof_batch(cells, proofs, coords, cs) is True


def test_spec_shape_agrees(kz, blobs):
    picks = [(1, 9), (0, 9), (1, 80), (0, 127)]
    cells, proofs, coords, cs = batch(blobs[:2], picks)
    per_cell = [blobs[r].c for r, _ in picks]
    idx = [c for _, c in picks]
    assert kz.verify_cell_kzg_proof_batch(per_cell, idx, cells, proofs) is True
    assert kz.verify_cell_proof_batch(cells, proofs, coords, cs) is True
    swapped = [proofs[1], proofs[0]] + proofs[2:]
    assert kz.verify_cell_kzg_proof_batch(per_cell, idx, cells, swapped) is False
    assert kz.verify_cell_proof_batch(cells, swapped, coords, cs) is False


# ------------------------------------------------------- verify: false cases
def test_verify_false_cases(kz, blobs):
    """After each negative case the same handle still accepts a valid batch."""
    picks = [(0, 2), (1, 2), (1, 90)]
    good = batch(blobs[:2], picks)
    cells, proofs, coords, cs = good

    def still_good():
        assert kz.verify_cell_proof_batch(*good) is True

    still_good()
    # one evaluation changed by 1, still canonical
    bad = bytearray(cells[1])
    v = (int_be(bad[32 * 63 :]) + 1) % R
    bad[32 * 63 :] = be32(v)
    assert kz.verify_cell_proof_batch(
        [cells[0], bytes(bad), cells[2]], proofs, coords, cs) is False
    still_good()
    # two cells' proofs swapped
    assert kz.verify_cell_proof_batch(
        cells, [proofs[0], proofs[2], proofs[1]], coords, cs) is False
    still_good()
    # column index off by one
    assert kz.verify_cell_proof_batch(
        cells, proofs, [(0, 2), (1, 2), (1, 91)], cs) is False
    still_good()
    # row pointing at the other blob's commitment
    assert kz.verify_cell_proof_batch(
        cells, proofs, [(1, 2), (1, 2), (1, 90)], cs) is False
    still_good()


def test_verify_one_bad_cell_among_128(kz, blobs):
    cells, proofs, coords, cs = batch(blobs[:1], [(0, c) for c in range(128)])
    bad = bytearray(cells[101])
    bad[31] ^= 0x01
    assert C.cell_from_bytes(bytes(bad))  # still canonical
    cells = cells[:101] + [bytes(bad)] + cells[102:]
    assert kz.verify_cell_proof_batch(cells, proofs, coords, cs) is False


# ----------------------------------------------------------- ceremony setup
@pytest.fixture(scope="module")
def kz_ceremony(kzg_mod, fx, cfx):
    raw = (REPO / "tests" / "golden" / "ceremony_g1_lagrange.bin").read_bytes()
    mono = [bytes.fromhex(h) for h in cfx["ceremony"]["g1_monomial"]]
    k = kzg_mod.Kzg.with_cell_setup(
        bytes.fromhex(fx["ceremony"]["g2_tau"]),
        (mono[:64], bytes.fromhex(cfx["ceremony"]["g2_monomial_64"])),
        g1_lagrange=raw,
    )
    yield k
    k.close()


def test_ceremony_quotient_one(kz_ceremony, cfx, G):
    mono = [bytes.fromhex(h) for h in cfx["ceremony"]["g1_monomial"]]
    gen = G.g1_compress(G.G1G)
    assert mono[0] == gen
    blob = blob_of_coefficients(seeded_scalars(b"gpu-kzgc-cer", 64) + [1])
    commitment = kz_ceremony.blob_to_kzg_commitment(blob)
    cells = kz_ceremony.compute_cells(blob)
    coords = [(0, c) for c in range(128)]
    assert kz_ceremony.verify_cell_proof_batch(
        cells, [gen] * 128, coords, [commitment]) is True
    proofs = [gen] * 77 + [mono[1]] + [gen] * 50
    assert kz_ceremony.verify_cell_proof_batch(
        cells, proofs, coords, [commitment]) is False


def test_ceremony_x64_commitment(kz_ceremony, cfx):
    mono64 = bytes.fromhex(cfx["ceremony"]["g1_monomial"][64])
    blob = blob_of_coefficients([0] * 64 + [1])
    assert kz_ceremony.blob_to_kzg_commitment(blob) == mono64


# ------------------------------------------------------------------- errors
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


def test_malformed_input_raises(kz, kzg_mod, blobs, off_subgroup):
    good = batch(blobs[:2], [(0, 4), (1, 66)])
    cells, proofs, coords, cs = good
    E = kzg_mod.KzgError
    bad_cell = bytearray(cells[1])
    bad_cell[32 * 17 : 32 * 18] = R.to_bytes(32, "big")  # evaluation == R
    with pytest.raises(E):
        kz.verify_cell_proof_batch([cells[0], bytes(bad_cell)], proofs, coords, cs)
    with pytest.raises(E):  # proof outside the subgroup
        kz.verify_cell_proof_batch(cells, [proofs[0], off_subgroup], coords, cs)
    with pytest.raises(E):  # commitment outside the subgroup
        kz.verify_cell_proof_batch(cells, proofs, coords, [cs[0], off_subgroup])
    cleared = bytes([proofs[0][0] & 0x7F]) + proofs[0][1:]  # compression bit
    with pytest.raises(E):
        kz.verify_cell_proof_batch(cells, [cleared, proofs[1]], coords, cs)
    with pytest.raises(E):  # wrong lengths
        kz.verify_cell_proof_batch([cells[0][:-1], cells[1]], proofs, coords, cs)
    with pytest.raises(E):
        kz.verify_cell_proof_batch(cells, [proofs[0], proofs[1] + b"\0"], coords, cs)
    with pytest.raises(E):
        kz.verify_cell_proof_batch(cells, proofs[:1], coords, cs)
    with pytest.raises(E):
        kz.verify_cell_proof_batch(cells, proofs, coords[:1], cs)
    with pytest.raises(E):
        kz.verify_cell_kzg_proof_batch(cs, [4], cells, proofs)
    with pytest.raises(E):  # col = 128
        kz.verify_cell_proof_batch(cells, proofs, [(0, 4), (1, 128)], cs)
    with pytest.raises(E):  # row = m
        kz.verify_cell_proof_batch(cells, proofs, [(0, 4), (2, 66)], cs)
    with pytest.raises(E):  # no commitments at all
        kz.verify_cell_proof_batch(cells, proofs, coords, [])
    # the C entry refuses the same coordinates before any launch
    packed = list(kzg_mod._pack_cell_batch(*good))
    u64 = ctypes.c_uint64 * 2
    for rows, cols_ in (((0, 2), (4, 66)), ((0, 1), (4, 128))):
        args = packed[:2] + [u64(*rows), u64(*cols_)] + packed[4:]
        assert kz._lib.m3x_kzgc_verify_cell_proof_batch(
            kz._ctx.handle, kz._h, *args) == -2
    args = [packed[0], 0] + packed[2:]
    assert kz._lib.m3x_kzgc_verify_cell_proof_batch(
        kz._ctx.handle, kz._h, *args) == -2
    # and the handle is as good as before
    assert kz.verify_cell_proof_batch(*good) is True


def test_handle_without_cell_setup(kzg_mod, fx, blobs):
    k = kzg_mod.Kzg(bytes.fromhex(fx["test_setup"]["g2_tau"]))
    good = batch(blobs[:1], [(0, 4)])
    with pytest.raises(kzg_mod.KzgError):
        k.verify_cell_proof_batch(*good)
    packed = kzg_mod._pack_cell_batch(*good)
    assert k._lib.m3x_kzgc_verify_cell_proof_batch(
        k._ctx.handle, k._h, *packed) == -2
    # compute_cells needs no setup
    assert k.compute_cells(blobs[0].blob) == blobs[0].cell_bytes
    k.close()


def test_bad_cell_setup_refused(kzg_mod, fx, tau_setup, blobs, off_subgroup, G):
    mono, g2_tau64 = tau_setup
    g2_tau = bytes.fromhex(fx["test_setup"]["g2_tau"])
    k = kzg_mod.Kzg(g2_tau)
    E = kzg_mod.KzgError
    pts = [mono[48 * j : 48 * j + 48] for j in range(64)]
    with pytest.raises(E):  # an infinity point among the 64
        k.load_cell_setup(pts[:9] + [INF] + pts[10:], g2_tau64)
    with pytest.raises(E):  # a point outside the subgroup
        k.load_cell_setup(pts[:63] + [off_subgroup], g2_tau64)
    with pytest.raises(E):  # a G2 point that does not decode
        k.load_cell_setup(mono, bytes(96))
    with pytest.raises(E):  # the G2 infinity
        k.load_cell_setup(mono, bytes([0xC0]) + bytes(95))
    with pytest.raises(E):  # wrong lengths
        k.load_cell_setup(mono[:-48], g2_tau64)
    with pytest.raises(E):
        k.load_cell_setup(pts[:63], g2_tau64)
    with pytest.raises(E):
        k.load_cell_setup(mono, g2_tau64[:-1])
    with pytest.raises(E):
        kzg_mod.Kzg.with_cell_setup(g2_tau, (mono,))
    # still without cell setup, and still verifying blobs
    with pytest.raises(E):
        k.verify_cell_proof_batch(*batch(blobs[:1], [(0, 4)]))
    kfx = fx["test_cases"][0]
    assert k.verify_kzg_proof(
        bytes.fromhex(kfx["commitment"]), bytes.fromhex(kfx["z"]),
        bytes.fromhex(kfx["y"]), bytes.fromhex(kfx["proof"])) is kfx["verdict"]
    # a good setup loads after the refused ones; a second load is refused
    k.load_cell_setup(mono, g2_tau64)
    assert k.verify_cell_proof_batch(*batch(blobs[:1], [(0, 4)])) is True
    with pytest.raises(E):
        k.load_cell_setup(mono, g2_tau64)
    assert k._lib.m3x_kzgc_load_cell_setup(
        k._ctx.handle, k._h, mono, g2_tau64) == -2
    k.close()


# ---------------------------------------------------------------- threading
def test_two_contexts_two_threads(kzg_mod, fx, tau_setup, blobs):
    """Two threads, each with its own per-thread context and Kzg: one checks
    a valid batch, the other an invalid one, three times each."""
    from concurrent.futures import ThreadPoolExecutor

    g2_tau = bytes.fromhex(fx["test_setup"]["g2_tau"])
    good = batch(blobs[:2], [(0, 8), (1, 8), (1, 120)])
    cells, proofs, coords, cs = good
    bad = (cells, [proofs[1], proofs[0], proofs[2]], coords, cs)

    def worker(widx):
        k = kzg_mod.Kzg.with_cell_setup(g2_tau, tau_setup)  # per-thread ctx
        args = good if widx == 0 else bad
        out = [k.verify_cell_proof_batch(*args) for _ in range(3)]
        k.close()
        return out

    with ThreadPoolExecutor(max_workers=2) as ex:
        outs = list(ex.map(worker, range(2)))
    assert outs == [[True] * 3, [False] * 3]
