"""GPU PeerDAS cell proofs (compute_cells_and_kzg_proofs,
recover_cells_and_kzg_proofs) against the Python reference. Every comparison
is bit-exact.

Two setups:
  known tau   g1_monomial[j] = [tau^j]G1 from the CPU oracle, built once; the
              proof of cell c is [q_c(tau)]G1 with q_c = p // (X^64 - y_c),
              one oracle multiplication each
  ceremony    tests/golden/ceremony_g1_monomial.bin; a blob X^(64+j) has
              quotient X^j at every cell, so every proof is g1_monomial[j],
              and the proofs of a seeded blob pass verify_cell_proof_batch
              against the Lagrange handle's commitment"""
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
SEEDS = [b"gpu-kzgcp-0", b"gpu-kzgcp-1", b"gpu-kzgcp-2"]
EXT = 128 * 2048
PROOFS = 128 * 48
SCATTERED_64 = [(5 * i + 3) % 128 for i in range(128)][:64]


def be32(v):
    return (v % R).to_bytes(32, "big")


def int_be(b):
    return int.from_bytes(b, "big")


def blob_of_coefficients(coef):
    """The blob (evaluation form, blob order) of a coefficient list."""
    coef = list(coef) + [0] * (N - len(coef))
    cells = C.cells_from_coefficients(coef)
    return b"".join(C.cell_to_bytes(c) for c in cells[:64])


def monomial_blob(k):
    return blob_of_coefficients([0] * k + [1])


def y_of(c):
    return pow(C.coset_shift(c), 64, R)


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


@pytest.fixture(scope="module")
def tau_mono(tau, g1_mul):
    """[tau^j]G1 compressed, j = 0..4095 (built once, never mutated)."""
    out, t = [], 1
    for _ in range(N):
        out.append(g1_mul(t))
        t = t * tau % R
    return out


class BlobCase:
    """A seeded blob with its reference cells and, under the known tau, its
    128 cell proofs."""

    def __init__(self, blob, tau, g1_mul):
        self.blob = blob
        self.coef = C.blob_coefficients(blob)
        self.cell_bytes = [
            C.cell_to_bytes(c) for c in C.cells_from_coefficients(self.coef)]
        self.proofs = [
            g1_mul(C.poly_eval(C.cell_quotient(self.coef, c), tau))
            for c in range(128)
        ]


@pytest.fixture(scope="module")
def blobs(tau, g1_mul):
    """Three seeded blobs, computed once and shared (never mutated)."""
    return [BlobCase(K.blob_from_seed(s), tau, g1_mul) for s in SEEDS]


@pytest.fixture(scope="module")
def kz(kzg_mod, fx, tau_mono):
    k = kzg_mod.Kzg(bytes.fromhex(fx["test_setup"]["g2_tau"]))
    k.load_g1_monomial(tau_mono)  # 4096 byte strings
    yield k
    k.close()


@pytest.fixture(scope="module")
def ceremony_mono():
    raw = (REPO / "tests" / "golden" / "ceremony_g1_monomial.bin").read_bytes()
    return [raw[48 * j : 48 * j + 48] for j in range(N)]


@pytest.fixture(scope="module")
def kz_ceremony(kzg_mod, fx, cfx, ceremony_mono):
    raw = (REPO / "tests" / "golden" / "ceremony_g1_lagrange.bin").read_bytes()
    k = kzg_mod.Kzg.with_cell_setup(
        bytes.fromhex(fx["ceremony"]["g2_tau"]),
        (ceremony_mono[:64], bytes.fromhex(cfx["ceremony"]["g2_monomial_64"])),
        g1_lagrange=raw,
    )
    k.load_g1_monomial(b"".join(ceremony_mono))  # one byte string
    yield k
    k.close()


# ---------------------------------------------------------------- known tau
@pytest.mark.parametrize("n", [1, 3])
def test_known_tau_all_proofs(kz, blobs, n):
    got = kz.compute_cells_and_kzg_proofs_batch([b.blob for b in blobs[:n]])
    assert len(got) == n
    for (cells, proofs), want in zip(got, blobs):
        assert len(cells) == 128 and len(proofs) == 128
        for c in range(128):
            assert proofs[c] == want.proofs[c], c
        assert cells == want.cell_bytes
    # the cells alongside are compute_cells' own
    assert [c for c, _ in got] == kz.compute_cells_batch(
        [b.blob for b in blobs[:n]])


def test_single_blob_form(kz, blobs):
    cells, proofs = kz.compute_cells_and_kzg_proofs(blobs[1].blob)
    assert cells == blobs[1].cell_bytes and proofs == blobs[1].proofs


# -------------------------------------------------- shapes that pin indexing
def test_monomial_63_every_proof_infinity(kz):
    _, proofs = kz.compute_cells_and_kzg_proofs(monomial_blob(63))
    assert proofs == [INF] * 128
    assert INF == bytes([0xC0]) + bytes(47)


def test_monomial_64_every_proof_generator(kz, G):
    _, proofs = kz.compute_cells_and_kzg_proofs(monomial_blob(64))
    assert proofs == [G.g1_compress(G.G1G)] * 128


@pytest.mark.parametrize("k", [127, 128, 4032, 4095])
def test_monomial_high(kz, tau, g1_mul, tau_mono, k):
    """X^k: q_c = sum_{m < k // 64} y_c^m X^(k - 64(m+1)). k = 128 is
    mono[64] + y_c mono[0]; k = 4032 and 4095 end in the last block of the
    m = 62 and m = 0 sums."""
    _, proofs = kz.compute_cells_and_kzg_proofs(monomial_blob(k))
    if k == 127:
        assert proofs == [tau_mono[63]] * 128
    for c in range(128):
        q_tau = sum(pow(y_of(c), m, R) * pow(tau, k - 64 * (m + 1), R)
                    for m in range(k // 64)) % R
        assert proofs[c] == g1_mul(q_tau), c


def test_zero_blob(kz):
    cells, proofs = kz.compute_cells_and_kzg_proofs(bytes(K.BYTES_PER_BLOB))
    assert proofs == [INF] * 128 and cells == [bytes(2048)] * 128


# ----------------------------------------------------------- ceremony setup
@pytest.mark.parametrize("j", [0, 1, 63])
def test_ceremony_monomial_quotient(kz_ceremony, ceremony_mono, j):
    _, proofs = kz_ceremony.compute_cells_and_kzg_proofs(monomial_blob(64 + j))
    assert proofs == [ceremony_mono[j]] * 128


def test_ceremony_proofs_verify(kz_ceremony, ceremony_mono):
    blob = K.blob_from_seed(b"gpu-kzgcp-ceremony")
    commitment = kz_ceremony.blob_to_kzg_commitment(blob)
    cells, proofs = kz_ceremony.compute_cells_and_kzg_proofs(blob)
    coords = [(0, c) for c in range(128)]
    assert kz_ceremony.verify_cell_proof_batch(
        cells, proofs, coords, [commitment]) is True
    # one proof changed to another valid point
    assert proofs[77] != ceremony_mono[1]
    bad = proofs[:77] + [ceremony_mono[1]] + proofs[78:]
    assert kz_ceremony.verify_cell_proof_batch(
        cells, bad, coords, [commitment]) is False


# ---------------------------------------------------------------- dev forms
def fetch(ctx, dev, nbytes):
    out = ctypes.create_string_buffer(nbytes)
    assert ctx._lib.m3x_d2h(ctx.handle, out, dev, nbytes) == 0
    return out.raw


def test_dev_forms_match_host(kz, blobs):
    ctx = kz._ctx
    blobs_d = ctx.upload(blobs[0].blob + blobs[1].blob)
    cells_d, proofs_d, proofs2_d = (
        ctx.alloc(2 * EXT), ctx.alloc(2 * PROOFS), ctx.alloc(2 * PROOFS))
    try:
        kz.compute_cells_and_kzg_proofs_batch_dev(blobs_d, 2, cells_d, proofs_d)
        kz.compute_cells_and_kzg_proofs_batch_dev(blobs_d, 2, None, proofs2_d)
        cells = fetch(ctx, cells_d, 2 * EXT)
        proofs = fetch(ctx, proofs_d, 2 * PROOFS)
        proofs2 = fetch(ctx, proofs2_d, 2 * PROOFS)
    finally:
        for p in (blobs_d, cells_d, proofs_d, proofs2_d):
            ctx.free(p)
    assert cells == b"".join(blobs[0].cell_bytes + blobs[1].cell_bytes)
    assert proofs == b"".join(blobs[0].proofs + blobs[1].proofs)
    assert proofs2 == proofs
    # the host form with cells_out = NULL
    out = ctypes.create_string_buffer(PROOFS)
    assert kz._lib.m3x_kzgc_compute_cells_and_proofs(
        ctx.handle, kz._h, blobs[2].blob, 1, None, out) == 0
    assert out.raw == b"".join(blobs[2].proofs)


# ----------------------------------------------------------------- recovery
@pytest.mark.parametrize("ids", [list(range(64, 128)), SCATTERED_64],
                         ids=["second_half", "scattered"])
def test_recover_cells_and_proofs(kz, blobs, ids):
    assert len(set(ids)) == 64
    known = [[b.cell_bytes[c] for c in ids] for b in blobs[:2]]
    got = kz.recover_cells_and_kzg_proofs_batch(ids, known)
    want = kz.compute_cells_and_kzg_proofs_batch([b.blob for b in blobs[:2]])
    assert got == want
    for (cells, proofs), b in zip(got, blobs):
        assert cells == b.cell_bytes and proofs == b.proofs


def test_recover_single_and_dev(kz, blobs):
    ids = SCATTERED_64
    known = [blobs[2].cell_bytes[c] for c in ids]
    cells, proofs = kz.recover_cells_and_kzg_proofs(ids, known)
    assert cells == blobs[2].cell_bytes and proofs == blobs[2].proofs
    ctx = kz._ctx
    in_d = ctx.upload(b"".join(known))
    cells_d, proofs_d = ctx.alloc(EXT), ctx.alloc(PROOFS)
    try:
        kz.recover_cells_and_kzg_proofs_batch_dev(ids, in_d, 1, cells_d, proofs_d)
        assert fetch(ctx, cells_d, EXT) == b"".join(cells)
        assert fetch(ctx, proofs_d, PROOFS) == b"".join(proofs)
    finally:
        for p in (in_d, cells_d, proofs_d):
            ctx.free(p)


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


def test_no_monomial_load(kzg_mod, fx, blobs):
    k = kzg_mod.Kzg(bytes.fromhex(fx["test_setup"]["g2_tau"]))
    E = kzg_mod.KzgError
    with pytest.raises(E):
        k.compute_cells_and_kzg_proofs(blobs[0].blob)
    ids = list(range(64))
    with pytest.raises(E):
        k.recover_cells_and_kzg_proofs(ids, blobs[0].cell_bytes[:64])
    # the C entries refuse the handle before any launch, n == 0 included
    out = ctypes.create_string_buffer(PROOFS)
    lib, h = k._lib, k._ctx.handle
    assert lib.m3x_kzgc_compute_cells_and_proofs(
        h, k._h, blobs[0].blob, 1, None, out) == -2
    assert lib.m3x_kzgc_compute_cells_and_proofs(h, k._h, None, 0, None, None) == -2
    cells_out = ctypes.create_string_buffer(EXT)
    assert lib.m3x_kzgc_recover_cells_and_proofs(
        h, k._h, (ctypes.c_uint64 * 64)(*ids), 64,
        b"".join(blobs[0].cell_bytes[:64]), 1, cells_out, out) == -2
    # compute_cells needs no setup
    assert k.compute_cells(blobs[0].blob) == blobs[0].cell_bytes
    k.close()


def test_c_argument_rules(kz, blobs):
    lib, h = kz._lib, kz._ctx.handle
    out = ctypes.create_string_buffer(PROOFS)
    assert lib.m3x_kzgc_compute_cells_and_proofs(h, kz._h, None, 0, None, None) == 0
    assert lib.m3x_kzgc_compute_cells_and_proofs(
        h, kz._h, blobs[0].blob, 65536, None, out) == -2
    cells_out = ctypes.create_string_buffer(EXT)
    known = b"".join(blobs[0].cell_bytes[:64])
    for bad in (list(range(63)) + [128], list(range(63)) + [0]):
        assert lib.m3x_kzgc_recover_cells_and_proofs(
            h, kz._h, (ctypes.c_uint64 * 64)(*bad), 64, known, 1, cells_out,
            out) == -2
    assert lib.m3x_kzgc_recover_cells_and_proofs(
        h, kz._h, (ctypes.c_uint64 * 63)(*range(63)), 63, known, 1, cells_out,
        out) == -2
    assert lib.m3x_kzgc_recover_cells_and_proofs(
        h, kz._h, (ctypes.c_uint64 * 64)(*range(64)), 64, None, 0, None,
        None) == 0
    assert kz.compute_cells_and_kzg_proofs(blobs[0].blob)[1] == blobs[0].proofs


def test_bad_monomial_setup_refused(kzg_mod, fx, tau_mono, blobs, off_subgroup):
    k = kzg_mod.Kzg(bytes.fromhex(fx["test_setup"]["g2_tau"]))
    E = kzg_mod.KzgError
    with pytest.raises(E):  # infinity among the 4096
        k.load_g1_monomial(tau_mono[:4000] + [INF] + tau_mono[4001:])
    with pytest.raises(E):  # a point outside the subgroup, last entry
        k.load_g1_monomial(tau_mono[:-1] + [off_subgroup])
    with pytest.raises(E):  # a point that does not decode, first entry
        k.load_g1_monomial([bytes(48)] + tau_mono[1:])
    with pytest.raises(E):  # wrong lengths
        k.load_g1_monomial(tau_mono[:-1])
    with pytest.raises(E):
        k.load_g1_monomial(b"".join(tau_mono)[:-1])
    # still refuses proofs, still verifies
    with pytest.raises(E):
        k.compute_cells_and_kzg_proofs(blobs[0].blob)
    out = ctypes.create_string_buffer(PROOFS)
    assert k._lib.m3x_kzgc_compute_cells_and_proofs(
        k._ctx.handle, k._h, blobs[0].blob, 1, None, out) == -2
    kfx = fx["test_cases"][0]
    assert k.verify_kzg_proof(
        bytes.fromhex(kfx["commitment"]), bytes.fromhex(kfx["z"]),
        bytes.fromhex(kfx["y"]), bytes.fromhex(kfx["proof"])) is kfx["verdict"]
    k.close()


def test_second_load_refused(kz, kzg_mod, tau_mono, blobs):
    with pytest.raises(kzg_mod.KzgError):
        kz.load_g1_monomial(tau_mono)
    assert kz._lib.m3x_kzgc_load_g1_monomial(
        kz._ctx.handle, kz._h, b"".join(tau_mono)) == -2
    assert kz.compute_cells_and_kzg_proofs(blobs[0].blob)[1] == blobs[0].proofs


@pytest.mark.parametrize("index", [0, 4095])
def test_blob_element_equal_to_modulus(kz, kzg_mod, blobs, index):
    bad = bytearray(blobs[0].blob)
    bad[32 * index : 32 * index + 32] = R.to_bytes(32, "big")
    bad = bytes(bad)
    E = kzg_mod.KzgError
    with pytest.raises(E):
        kz.compute_cells_and_kzg_proofs(bad)
    assert kz.compute_cells_and_kzg_proofs(blobs[1].blob)[1] == blobs[1].proofs
    with pytest.raises(E):  # as the second blob of a batch
        kz.compute_cells_and_kzg_proofs_batch([blobs[1].blob, bad])
    assert kz.compute_cells_and_kzg_proofs(blobs[1].blob)[1] == blobs[1].proofs
    # proofs only: the coefficient pass makes the check itself
    out = ctypes.create_string_buffer(2 * PROOFS)
    assert kz._lib.m3x_kzgc_compute_cells_and_proofs(
        kz._ctx.handle, kz._h, blobs[1].blob + bad, 2, None, out) == -4
    assert kz.compute_cells_and_kzg_proofs(blobs[0].blob) == (
        blobs[0].cell_bytes, blobs[0].proofs)


# -------------------------------------------------------------- timing slots
def test_timing_slots(kz, blobs):
    ctx = kz._ctx
    out = ctypes.create_string_buffer(PROOFS)
    ctx.timing_enable(True)
    try:
        assert kz._lib.m3x_kzgc_compute_cells_and_proofs(
            ctx.handle, kz._h, blobs[0].blob, 1, None, out) == 0
        times = ctx.kernel_times()
        assert times["kzgc_toeplitz"][1] == 1 and times["kzgc_toeplitz"][0] > 0
        assert times["kzgc_proof_dft"][1] == 1 and times["kzgc_proof_dft"][0] > 0
        # a proofs-only call: the coefficient pass counts into kzgc_toeplitz
        for name in ("kzgc_ntt", "kzgc_decode", "kzgc_combine", "kzgc_recover",
                     "bls_sigmsm"):
            assert times[name] == (0.0, 0), name
        for i in (27, 28):
            ms, cnt = ctypes.c_double(), ctypes.c_uint64()
            assert ctx._lib.m3x_kernel_ms(
                ctx.handle, i, ctypes.byref(ms), ctypes.byref(cnt)) == 0
            assert cnt.value == 1
        ms, cnt = ctypes.c_double(), ctypes.c_uint64()
        assert ctx._lib.m3x_kernel_ms(
            ctx.handle, 29, ctypes.byref(ms), ctypes.byref(cnt)) == -2
        # with the cells: compute_cells' passes count into kzgc_ntt
        kz.compute_cells_and_kzg_proofs(blobs[0].blob)
        times = ctx.kernel_times()
        assert times["kzgc_ntt"][1] == 1
        assert times["kzgc_toeplitz"][1] == 2 and times["kzgc_proof_dft"][1] == 2
    finally:
        ctx.timing_enable(False)
    assert out.raw == b"".join(blobs[0].proofs)


# ---------------------------------------------------------------- threading
def test_two_contexts_share_one_handle(kz, blobs):
    """Two threads, each with its own context, over the one handle."""
    from concurrent.futures import ThreadPoolExecutor

    from lighthouse_amd import _native

    def worker(widx):
        ctx = _native.Ctx()
        outs = []
        for _ in range(2):
            out = ctypes.create_string_buffer(PROOFS)
            rc = kz._lib.m3x_kzgc_compute_cells_and_proofs(
                ctx.handle, kz._h, blobs[widx].blob, 1, None, out)
            outs.append((rc, out.raw))
        ctx.close()
        return outs

    with ThreadPoolExecutor(max_workers=2) as ex:
        outs = list(ex.map(worker, range(2)))
    for widx in range(2):
        assert outs[widx] == [(0, b"".join(blobs[widx].proofs))] * 2
