"""KZG on the GPU — the reference's `Kzg` wrapper
(crypto/kzg/src/lib.rs:62-216): verify_kzg_proof, verify_blob_kzg_proof and
verify_blob_kzg_proof_batch, the producing half blob_to_kzg_commitment,
compute_kzg_proof and compute_blob_kzg_proof, and the PeerDAS cell functions
compute_cells, compute_cells_and_kzg_proofs, cells_to_blob,
verify_cell_proof_batch, recover_all_cells and recover_cells_and_kzg_proofs
(lib.rs:171-216).

Verification needs one trusted-setup point, [tau]G2 (entry 1 of the
ceremony's g2_monomial list, 96 bytes compressed). Producing commitments
and proofs also needs the 4096 g1_lagrange points, in the ceremony file's
order; without them the handle is verification-only. Cell verification
needs g1_monomial[0..64) and g2_monomial[64] (load_cell_setup, or the
with_cell_setup constructor); compute_cells and recover_all_cells need no
setup at all; cell proofs (compute_cells_and_kzg_proofs,
recover_cells_and_kzg_proofs) need the 4096 g1_monomial points
(load_g1_monomial). All byte strings are the spec's big-endian wire forms. Every verify method returns a bool: a
proof that does not verify is False; malformed input (bad point encoding, a
point outside the subgroup, a scalar >= the field modulus, wrong lengths)
or a producing call without the Lagrange basis raises KzgError, the
analogue of the reference's Error::Kzg / InconsistentArrayLength. No CPU
fallback (package rule)."""
import ctypes
from typing import Optional, Sequence

from . import _native

BYTES_PER_FIELD_ELEMENT = 32
FIELD_ELEMENTS_PER_BLOB = 4096
BYTES_PER_BLOB = BYTES_PER_FIELD_ELEMENT * FIELD_ELEMENTS_PER_BLOB
BYTES_PER_COMMITMENT = 48
BYTES_PER_PROOF = 48
BYTES_PER_G2_POINT = 96
FIELD_ELEMENTS_PER_CELL = 64
CELLS_PER_EXT_BLOB = 128
BYTES_PER_CELL = BYTES_PER_FIELD_ELEMENT * FIELD_ELEMENTS_PER_CELL
BLS_MODULUS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

_ERR_ARG = -2
_ERR_ENCODING = -4
_MAX_BATCH = 65535


class KzgError(ValueError):
    """Malformed input (the c_kzg::Error / InconsistentArrayLength analogue)."""


def _check_len(name, b, want):
    if not isinstance(b, (bytes, bytearray)) or len(b) != want:
        got = len(b) if hasattr(b, "__len__") else type(b).__name__
        raise KzgError(f"{name}: expected {want} bytes, got {got}")
    return bytes(b)


def _verdict(rc, what):
    if rc == 1:
        return True
    if rc == 0:
        return False
    if rc == _ERR_ENCODING:
        raise KzgError(f"{what}: malformed point or non-canonical field element")
    raise RuntimeError(f"{what} failed (rc={rc})")


def _join(name, items, want):
    return b"".join(_check_len(name, b, want) for b in items)


def _split(raw, size, n):
    return [raw[size * i : size * (i + 1)] for i in range(n)]


class Kzg:
    """Trusted setup bound to one GPU context: [tau]G2 for verification,
    plus (optionally) the Lagrange basis for commitments and proofs. The
    basis costs a one-time table build and about 200 MB of device memory;
    load_g1_monomial (cell proofs) builds a second table of the same shape
    over g1_monomial, about 200 MB more."""

    def __init__(self, g2_tau: bytes, g1_lagrange=None,
                 ctx: Optional[_native.Ctx] = None):
        g2_tau = _check_len("g2_tau", g2_tau, BYTES_PER_G2_POINT)
        if g1_lagrange is not None:
            if not isinstance(g1_lagrange, (bytes, bytearray)):
                if len(g1_lagrange) != FIELD_ELEMENTS_PER_BLOB:
                    raise KzgError(
                        f"g1_lagrange: expected {FIELD_ELEMENTS_PER_BLOB} "
                        f"points, got {len(g1_lagrange)}"
                    )
                g1_lagrange = _join("g1_lagrange point", g1_lagrange,
                                    BYTES_PER_COMMITMENT)
            g1_lagrange = _check_len(
                "g1_lagrange", g1_lagrange,
                FIELD_ELEMENTS_PER_BLOB * BYTES_PER_COMMITMENT,
            )
        self._has_basis = False
        self._has_cell_setup = False
        self._has_monomial = False
        self._ctx = ctx or _native.default_ctx()
        self._lib = _native.load()
        self._h = ctypes.c_void_p()
        rc = self._lib.m3x_kzg_create(
            self._ctx.handle, g2_tau, ctypes.byref(self._h)
        )
        if rc == _ERR_ENCODING:
            raise KzgError("g2_tau is not a valid non-infinity G2 subgroup point")
        if rc != 0:
            raise RuntimeError(f"m3x_kzg_create failed (rc={rc})")
        if g1_lagrange is not None:
            rc = self._lib.m3x_kzgp_load_g1_lagrange(
                self._ctx.handle, self._h, g1_lagrange
            )
            if rc != 0:
                self.close()
            if rc == _ERR_ENCODING:
                raise KzgError(
                    "g1_lagrange holds a point that is not a valid "
                    "non-infinity G1 subgroup point"
                )
            if rc != 0:
                raise RuntimeError(f"m3x_kzgp_load_g1_lagrange failed (rc={rc})")
            self._has_basis = True

    def close(self):
        if getattr(self, "_h", None):
            self._lib.m3x_kzg_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- lib.rs:152-167 ----
    def verify_kzg_proof(self, commitment: bytes, z: bytes, y: bytes,
                         proof: bytes) -> bool:
        commitment = _check_len("commitment", commitment, BYTES_PER_COMMITMENT)
        z = _check_len("z", z, BYTES_PER_FIELD_ELEMENT)
        y = _check_len("y", y, BYTES_PER_FIELD_ELEMENT)
        proof = _check_len("proof", proof, BYTES_PER_PROOF)
        rc = self._lib.m3x_kzg_verify_proof(
            self._ctx.handle, self._h, commitment, z, y, proof
        )
        return _verdict(rc, "verify_kzg_proof")

    def verify_kzg_proof_batch(self, commitments: Sequence[bytes],
                               zs: Sequence[bytes], ys: Sequence[bytes],
                               proofs: Sequence[bytes]) -> bool:
        n = len(commitments)
        if not (n == len(zs) == len(ys) == len(proofs)):
            raise KzgError(
                "inconsistent array length: "
                f"{n} commitments, {len(zs)} zs, {len(ys)} ys, {len(proofs)} proofs"
            )
        if n == 0:
            return True
        cs = b"".join(_check_len("commitment", c, BYTES_PER_COMMITMENT) for c in commitments)
        zb = b"".join(_check_len("z", z, BYTES_PER_FIELD_ELEMENT) for z in zs)
        yb = b"".join(_check_len("y", y, BYTES_PER_FIELD_ELEMENT) for y in ys)
        ps = b"".join(_check_len("proof", p, BYTES_PER_PROOF) for p in proofs)
        rc = self._lib.m3x_kzg_verify_proof_batch(
            self._ctx.handle, self._h, cs, zb, yb, ps, n
        )
        return _verdict(rc, "verify_kzg_proof_batch")

    # ---- lib.rs:83-103 ----
    def verify_blob_kzg_proof(self, blob: bytes, commitment: bytes,
                              proof: bytes) -> bool:
        return self.verify_blob_kzg_proof_batch([blob], [commitment], [proof])

    # ---- lib.rs:105-132 ----
    def verify_blob_kzg_proof_batch(self, blobs: Sequence[bytes],
                                    commitments: Sequence[bytes],
                                    proofs: Sequence[bytes]) -> bool:
        n = len(blobs)
        if not (n == len(commitments) == len(proofs)):
            raise KzgError(
                "inconsistent array length: "
                f"{n} blobs, {len(commitments)} commitments, {len(proofs)} proofs"
            )
        if n == 0:
            return True
        bl = b"".join(_check_len("blob", b, BYTES_PER_BLOB) for b in blobs)
        cs = b"".join(_check_len("commitment", c, BYTES_PER_COMMITMENT) for c in commitments)
        ps = b"".join(_check_len("proof", p, BYTES_PER_PROOF) for p in proofs)
        rc = self._lib.m3x_kzg_verify_blob_proof_batch(
            self._ctx.handle, self._h, bl, cs, ps, n
        )
        return _verdict(rc, "verify_blob_kzg_proof_batch")

    def verify_blob_kzg_proof_batch_dev(self, blobs_dev, commitments_dev,
                                        proofs_dev, n: int) -> bool:
        """Same check over inputs already resident in device memory
        (Ctx.upload): blobs n*131072, commitments n*48, proofs n*48."""
        rc = self._lib.m3x_kzg_verify_blob_proof_batch_dev(
            self._ctx.handle, self._h, blobs_dev, commitments_dev, proofs_dev, n
        )
        return _verdict(rc, "verify_blob_kzg_proof_batch_dev")


    # ---- producing half ----
    def _produced(self, rc, what):
        if rc == _ERR_ENCODING:
            raise KzgError(f"{what}: malformed point or non-canonical field element")
        if rc != 0:
            raise RuntimeError(f"{what} failed (rc={rc})")

    def _need_basis(self, what):
        if not self._has_basis:
            raise KzgError(f"{what}: this Kzg was built without g1_lagrange")

    # ---- lib.rs:134-139 ----
    def blob_to_kzg_commitment(self, blob: bytes) -> bytes:
        return self.blob_to_kzg_commitment_batch([blob])[0]

    def blob_to_kzg_commitment_batch(self, blobs: Sequence[bytes]):
        self._need_basis("blob_to_kzg_commitment")
        n = len(blobs)
        if n == 0:
            return []
        bl = _join("blob", blobs, BYTES_PER_BLOB)
        out = ctypes.create_string_buffer(BYTES_PER_COMMITMENT * n)
        rc = self._lib.m3x_kzgp_blob_to_commitment(
            self._ctx.handle, self._h, bl, n, out
        )
        self._produced(rc, "blob_to_kzg_commitment")
        return _split(out.raw, BYTES_PER_COMMITMENT, n)

    # ---- lib.rs:141-150 ----
    def compute_kzg_proof(self, blob: bytes, z: bytes):
        """(proof, y) with y = p(z)."""
        return self.compute_kzg_proof_batch([blob], [z])[0]

    def compute_kzg_proof_batch(self, blobs: Sequence[bytes],
                                zs: Sequence[bytes]):
        self._need_basis("compute_kzg_proof")
        n = len(blobs)
        if n != len(zs):
            raise KzgError(f"inconsistent array length: {n} blobs, {len(zs)} zs")
        if n == 0:
            return []
        bl = _join("blob", blobs, BYTES_PER_BLOB)
        zb = _join("z", zs, BYTES_PER_FIELD_ELEMENT)
        proofs = ctypes.create_string_buffer(BYTES_PER_PROOF * n)
        ys = ctypes.create_string_buffer(BYTES_PER_FIELD_ELEMENT * n)
        rc = self._lib.m3x_kzgp_compute_proof(
            self._ctx.handle, self._h, bl, zb, n, proofs, ys
        )
        self._produced(rc, "compute_kzg_proof")
        return list(zip(_split(proofs.raw, BYTES_PER_PROOF, n),
                        _split(ys.raw, BYTES_PER_FIELD_ELEMENT, n)))

    # ---- lib.rs:72-81 ----
    def compute_blob_kzg_proof(self, blob: bytes, commitment: bytes) -> bytes:
        return self.compute_blob_kzg_proof_batch([blob], [commitment])[0]

    def compute_blob_kzg_proof_batch(self, blobs: Sequence[bytes],
                                     commitments: Sequence[bytes]):
        self._need_basis("compute_blob_kzg_proof")
        n = len(blobs)
        if n != len(commitments):
            raise KzgError(
                f"inconsistent array length: {n} blobs, {len(commitments)} commitments"
            )
        if n == 0:
            return []
        bl = _join("blob", blobs, BYTES_PER_BLOB)
        cs = _join("commitment", commitments, BYTES_PER_COMMITMENT)
        out = ctypes.create_string_buffer(BYTES_PER_PROOF * n)
        rc = self._lib.m3x_kzgp_compute_blob_proof(
            self._ctx.handle, self._h, bl, cs, n, out
        )
        self._produced(rc, "compute_blob_kzg_proof")
        return _split(out.raw, BYTES_PER_PROOF, n)

    def blob_to_kzg_commitment_batch_dev(self, blobs_dev, n: int, out_dev):
        """Device-resident form: blobs n*131072 -> out_dev n*48."""
        self._need_basis("blob_to_kzg_commitment")
        rc = self._lib.m3x_kzgp_blob_to_commitment_dev(
            self._ctx.handle, self._h, blobs_dev, n, out_dev
        )
        self._produced(rc, "blob_to_kzg_commitment_dev")

    def compute_kzg_proof_batch_dev(self, blobs_dev, zs_dev, n: int,
                                    proofs_out_dev, ys_out_dev):
        """Device-resident form: blobs n*131072, zs n*32 -> proofs n*48
        and ys n*32."""
        self._need_basis("compute_kzg_proof")
        rc = self._lib.m3x_kzgp_compute_proof_dev(
            self._ctx.handle, self._h, blobs_dev, zs_dev, n, proofs_out_dev,
            ys_out_dev
        )
        self._produced(rc, "compute_kzg_proof_dev")

    def compute_blob_kzg_proof_batch_dev(self, blobs_dev, commitments_dev,
                                         n: int, out_dev):
        """Device-resident form: blobs n*131072, commitments n*48 -> n*48."""
        self._need_basis("compute_blob_kzg_proof")
        rc = self._lib.m3x_kzgp_compute_blob_proof_dev(
            self._ctx.handle, self._h, blobs_dev, commitments_dev, n, out_dev
        )
        self._produced(rc, "compute_blob_kzg_proof_dev")

    # ---- PeerDAS cells (lib.rs:171-216) ----
    @classmethod
    def with_cell_setup(cls, g2_tau: bytes, cell_setup, g1_lagrange=None,
                        ctx: Optional[_native.Ctx] = None):
        """Kzg(g2_tau, g1_lagrange, ctx) with cell_setup =
        (g1_monomial[0..64), g2_monomial[64]) loaded."""
        try:
            g1_monomial64, g2_tau64 = cell_setup
        except (TypeError, ValueError):
            raise KzgError(
                "cell_setup: expected (g1_monomial[0..64), g2_monomial[64])"
            ) from None
        k = cls(g2_tau, g1_lagrange, ctx)
        try:
            k.load_cell_setup(g1_monomial64, g2_tau64)
        except Exception:
            k.close()
            raise
        return k

    def load_cell_setup(self, g1_monomial64, g2_tau64: bytes):
        """Load g1_monomial[0..64) (64 * 48 bytes, or 64 byte strings) and
        g2_monomial[64] (96 bytes): what cell verification needs. A refused
        setup raises KzgError and leaves the handle as it was; one load per
        handle."""
        if not isinstance(g1_monomial64, (bytes, bytearray)):
            if len(g1_monomial64) != FIELD_ELEMENTS_PER_CELL:
                raise KzgError(
                    f"cell setup: expected {FIELD_ELEMENTS_PER_CELL} "
                    f"g1_monomial points, got {len(g1_monomial64)}"
                )
            g1_monomial64 = _join("g1_monomial point", g1_monomial64,
                                  BYTES_PER_COMMITMENT)
        g1_monomial64 = _check_len(
            "g1_monomial", g1_monomial64,
            FIELD_ELEMENTS_PER_CELL * BYTES_PER_COMMITMENT)
        g2_tau64 = _check_len("g2_tau64", g2_tau64, BYTES_PER_G2_POINT)
        if self._has_cell_setup:
            raise KzgError("cell setup already loaded")
        rc = self._lib.m3x_kzgc_load_cell_setup(
            self._ctx.handle, self._h, g1_monomial64, g2_tau64)
        if rc == _ERR_ENCODING:
            raise KzgError(
                "cell_setup holds a point that is not a valid non-infinity "
                "subgroup point"
            )
        if rc != 0:
            raise RuntimeError(f"m3x_kzgc_load_cell_setup failed (rc={rc})")
        self._has_cell_setup = True

    def load_g1_monomial(self, points):
        """Load the 4096 g1_monomial points (4096 * 48 bytes, or 4096 byte
        strings, the ceremony file's order): what cell proofs need. Builds a
        fixed-base table of about 200 MB of device memory once. A refused
        list raises KzgError and leaves the handle as it was; one load per
        handle."""
        if not isinstance(points, (bytes, bytearray)):
            if len(points) != FIELD_ELEMENTS_PER_BLOB:
                raise KzgError(
                    f"g1_monomial: expected {FIELD_ELEMENTS_PER_BLOB} "
                    f"points, got {len(points)}"
                )
            points = _join("g1_monomial point", points, BYTES_PER_COMMITMENT)
        points = _check_len("g1_monomial", points,
                            FIELD_ELEMENTS_PER_BLOB * BYTES_PER_COMMITMENT)
        if self._has_monomial:
            raise KzgError("g1_monomial already loaded")
        rc = self._lib.m3x_kzgc_load_g1_monomial(
            self._ctx.handle, self._h, points)
        if rc == _ERR_ENCODING:
            raise KzgError(
                "g1_monomial holds a point that is not a valid non-infinity "
                "G1 subgroup point"
            )
        if rc != 0:
            raise RuntimeError(f"m3x_kzgc_load_g1_monomial failed (rc={rc})")
        self._has_monomial = True

    def _need_monomial(self, what):
        if not self._has_monomial:
            raise KzgError(f"{what}: this Kzg has no g1_monomial loaded")

    # ---- lib.rs:171-185, cells and proofs ----
    def compute_cells_and_kzg_proofs(self, blob: bytes):
        """(cells, proofs): the blob's 128 cells and their 128 proofs of 48
        bytes."""
        return self.compute_cells_and_kzg_proofs_batch([blob])[0]

    def compute_cells_and_kzg_proofs_batch(self, blobs: Sequence[bytes]):
        self._need_monomial("compute_cells_and_kzg_proofs")
        n = len(blobs)
        if n == 0:
            return []
        if n > _MAX_BATCH:
            raise KzgError(
                f"compute_cells_and_kzg_proofs: at most {_MAX_BATCH} blobs a call")
        bl = _join("blob", blobs, BYTES_PER_BLOB)
        cells = ctypes.create_string_buffer(_BYTES_PER_EXT_BLOB * n)
        proofs = ctypes.create_string_buffer(_PROOF_BYTES_PER_BLOB * n)
        rc = self._lib.m3x_kzgc_compute_cells_and_proofs(
            self._ctx.handle, self._h, bl, n, cells, proofs)
        self._produced(rc, "compute_cells_and_kzg_proofs")
        return _split_cells_and_proofs(cells.raw, proofs.raw, n)

    def compute_cells_and_kzg_proofs_batch_dev(self, blobs_dev, n: int,
                                               cells_out_dev, proofs_out_dev):
        """Device-resident form: blobs n*131072 -> cells_out_dev n*262144
        (None: proofs only) and proofs_out_dev n*128*48."""
        self._need_monomial("compute_cells_and_kzg_proofs")
        if not 0 <= n <= _MAX_BATCH:
            raise KzgError(
                f"compute_cells_and_kzg_proofs: at most {_MAX_BATCH} blobs a call")
        rc = self._lib.m3x_kzgc_compute_cells_and_proofs_dev(
            self._ctx.handle, self._h, blobs_dev, n, cells_out_dev,
            proofs_out_dev)
        self._produced(rc, "compute_cells_and_kzg_proofs_dev")

    # ---- recover_cells_and_kzg_proofs: lib.rs:208-216 plus the proofs ----
    def recover_cells_and_kzg_proofs(self, cell_ids: Sequence[int],
                                     cells: Sequence[bytes]):
        """(cells, proofs) of a blob from at least 64 of its cells; the
        argument rules of recover_all_cells."""
        return self.recover_cells_and_kzg_proofs_batch(cell_ids, [cells])[0]

    def recover_cells_and_kzg_proofs_batch(
            self, cell_ids: Sequence[int],
            cells_per_blob: Sequence[Sequence[bytes]]):
        """The same for several blobs that share one set of known columns."""
        ids = _pack_cell_ids(cell_ids)
        self._need_monomial("recover_cells_and_kzg_proofs")
        k, n = len(cell_ids), len(cells_per_blob)
        if n > _MAX_BATCH:
            raise KzgError(
                f"recover_cells_and_kzg_proofs: at most {_MAX_BATCH} blobs a call")
        for cells in cells_per_blob:
            if len(cells) != k:
                raise KzgError(
                    f"inconsistent array length: {k} cell ids, {len(cells)} cells")
        if n == 0:
            return []
        ce = b"".join(_join("cell", cells, BYTES_PER_CELL)
                      for cells in cells_per_blob)
        out = ctypes.create_string_buffer(_BYTES_PER_EXT_BLOB * n)
        proofs = ctypes.create_string_buffer(_PROOF_BYTES_PER_BLOB * n)
        rc = self._lib.m3x_kzgc_recover_cells_and_proofs(
            self._ctx.handle, self._h, ids, k, ce, n, out, proofs)
        self._recovered(rc, "recover_cells_and_kzg_proofs")
        return _split_cells_and_proofs(out.raw, proofs.raw, n)

    def recover_cells_and_kzg_proofs_batch_dev(self, cell_ids: Sequence[int],
                                               cells_dev, n: int,
                                               cells_out_dev, proofs_out_dev):
        """Device-resident form: cells_dev n*k*2048, blob-major in the order
        of cell_ids (host) -> cells_out_dev n*262144, proofs_out_dev
        n*128*48."""
        ids = _pack_cell_ids(cell_ids)
        self._need_monomial("recover_cells_and_kzg_proofs")
        if not 0 <= n <= _MAX_BATCH:
            raise KzgError(
                f"recover_cells_and_kzg_proofs: at most {_MAX_BATCH} blobs a call")
        rc = self._lib.m3x_kzgc_recover_cells_and_proofs_dev(
            self._ctx.handle, self._h, ids, len(cell_ids), cells_dev, n,
            cells_out_dev, proofs_out_dev)
        self._recovered(rc, "recover_cells_and_kzg_proofs_dev")

    # ---- lib.rs:171-185, the cells only ----
    def compute_cells(self, blob: bytes):
        """The blob's 128 cells of 2048 bytes; cells 0..63 are the blob."""
        return self.compute_cells_batch([blob])[0]

    def compute_cells_batch(self, blobs: Sequence[bytes]):
        n = len(blobs)
        if n == 0:
            return []
        if n > _MAX_BATCH:
            raise KzgError(f"compute_cells: at most {_MAX_BATCH} blobs a call")
        bl = _join("blob", blobs, BYTES_PER_BLOB)
        per_blob = CELLS_PER_EXT_BLOB * BYTES_PER_CELL
        out = ctypes.create_string_buffer(per_blob * n)
        rc = self._lib.m3x_kzgc_compute_cells(self._ctx.handle, bl, n, out)
        self._produced(rc, "compute_cells")
        raw = out.raw
        return [
            _split(raw[per_blob * i : per_blob * (i + 1)], BYTES_PER_CELL,
                   CELLS_PER_EXT_BLOB)
            for i in range(n)
        ]

    def compute_cells_batch_dev(self, blobs_dev, n: int, cells_out_dev):
        """Device-resident form: blobs n*131072 -> cells_out_dev n*262144."""
        rc = self._lib.m3x_kzgc_compute_cells_dev(
            self._ctx.handle, blobs_dev, n, cells_out_dev
        )
        self._produced(rc, "compute_cells_dev")

    # ---- lib.rs:203-206 ----
    @staticmethod
    def cells_to_blob(cells: Sequence[bytes]) -> bytes:
        """The blob of a full set of 128 cells: cells 0..63 joined (host)."""
        if len(cells) != CELLS_PER_EXT_BLOB:
            raise KzgError(
                f"cells_to_blob: expected {CELLS_PER_EXT_BLOB} cells, "
                f"got {len(cells)}"
            )
        cells = [_check_len("cell", c, BYTES_PER_CELL) for c in cells]
        return b"".join(cells[: CELLS_PER_EXT_BLOB // 2])

    # ---- lib.rs:208-216 ----
    def recover_all_cells(self, cell_ids: Sequence[int],
                          cells: Sequence[bytes]):
        """All 128 cells of a blob from at least 64 of them: cells[t] is
        cell number cell_ids[t], in any order. KzgError for fewer than 64 or
        more than 128 cells, an id outside 0..127 or given twice, a
        non-canonical element, or cells that lie on no blob polynomial."""
        return self.recover_all_cells_batch(cell_ids, [cells])[0]

    def recover_all_cells_batch(self, cell_ids: Sequence[int],
                                cells_per_blob: Sequence[Sequence[bytes]]):
        """The same for several blobs that share one set of known columns:
        cells_per_blob[b][t] is cell cell_ids[t] of blob b."""
        ids = _pack_cell_ids(cell_ids)
        k, n = len(cell_ids), len(cells_per_blob)
        if n > _MAX_BATCH:
            raise KzgError(f"recover_all_cells: at most {_MAX_BATCH} blobs a call")
        for cells in cells_per_blob:
            if len(cells) != k:
                raise KzgError(
                    f"inconsistent array length: {k} cell ids, {len(cells)} cells")
        if n == 0:
            return []
        ce = b"".join(_join("cell", cells, BYTES_PER_CELL)
                      for cells in cells_per_blob)
        per_blob = CELLS_PER_EXT_BLOB * BYTES_PER_CELL
        out = ctypes.create_string_buffer(per_blob * n)
        rc = self._lib.m3x_kzgc_recover_cells(
            self._ctx.handle, ids, k, ce, n, out)
        self._recovered(rc, "recover_all_cells")
        raw = out.raw
        return [
            _split(raw[per_blob * i : per_blob * (i + 1)], BYTES_PER_CELL,
                   CELLS_PER_EXT_BLOB)
            for i in range(n)
        ]

    def recover_all_cells_batch_dev(self, cell_ids: Sequence[int], cells_dev,
                                    n: int, cells_out_dev):
        """Device-resident form: cells_dev n*k*2048, blob-major in the order
        of cell_ids (host) -> cells_out_dev n*262144."""
        ids = _pack_cell_ids(cell_ids)
        if not 0 <= n <= _MAX_BATCH:
            raise KzgError(f"recover_all_cells: at most {_MAX_BATCH} blobs a call")
        rc = self._lib.m3x_kzgc_recover_cells_dev(
            self._ctx.handle, ids, len(cell_ids), cells_dev, n, cells_out_dev)
        self._recovered(rc, "recover_all_cells_dev")

    @staticmethod
    def _recovered(rc, what):
        if rc == _ERR_ENCODING:
            raise KzgError(
                f"{what}: non-canonical field element, or cells that do not "
                "lie on one polynomial of degree < 4096")
        if rc == _ERR_ARG:
            raise KzgError(f"{what}: bad cell ids or count")
        if rc != 0:
            raise RuntimeError(f"{what} failed (rc={rc})")

    # ---- lib.rs:187-201 ----
    def verify_cell_proof_batch(self, cells: Sequence[bytes],
                                proofs: Sequence[bytes],
                                coordinates: Sequence[tuple],
                                commitments: Sequence[bytes]) -> bool:
        """The reference's shape: cell k sits at coordinates[k] = (row, col)
        of the blob matrix, row indexing `commitments`."""
        packed = self._pack_cell_batch(cells, proofs, coordinates, commitments)
        if packed is None:
            return True
        rc = self._lib.m3x_kzgc_verify_cell_proof_batch(
            self._ctx.handle, self._h, *packed
        )
        return _verdict(rc, "verify_cell_proof_batch")

    def verify_cell_kzg_proof_batch(self, commitments_per_cell: Sequence[bytes],
                                    cell_indices: Sequence[int],
                                    cells: Sequence[bytes],
                                    proofs: Sequence[bytes]) -> bool:
        """The spec's shape: one commitment per cell. Commitments are
        deduplicated by first appearance into the rows of the form above."""
        n = len(cells)
        if not (n == len(commitments_per_cell) == len(cell_indices) == len(proofs)):
            raise KzgError(
                "inconsistent array length: "
                f"{len(commitments_per_cell)} commitments, "
                f"{len(cell_indices)} cell indices, {n} cells, "
                f"{len(proofs)} proofs"
            )
        row_of, commitments, coordinates = {}, [], []
        for c, col in zip(commitments_per_cell, cell_indices):
            c = _check_len("commitment", c, BYTES_PER_COMMITMENT)
            if c not in row_of:
                row_of[c] = len(commitments)
                commitments.append(c)
            coordinates.append((row_of[c], col))
        return self.verify_cell_proof_batch(cells, proofs, coordinates, commitments)

    def _pack_cell_batch(self, cells, proofs, coordinates, commitments):
        """Checked ctypes arguments of a cell batch; None for the empty one."""
        if not self._has_cell_setup:
            raise KzgError("verify_cell_proof_batch: this Kzg has no cell "
                           "setup loaded")
        return _pack_cell_batch(cells, proofs, coordinates, commitments)


_BYTES_PER_EXT_BLOB = CELLS_PER_EXT_BLOB * BYTES_PER_CELL
_PROOF_BYTES_PER_BLOB = CELLS_PER_EXT_BLOB * BYTES_PER_PROOF


def _split_cells_and_proofs(cells_raw, proofs_raw, n):
    """[(cells, proofs)] of n blobs from the two output buffers."""
    return [
        (
            _split(cells_raw[_BYTES_PER_EXT_BLOB * i : _BYTES_PER_EXT_BLOB * (i + 1)],
                   BYTES_PER_CELL, CELLS_PER_EXT_BLOB),
            _split(proofs_raw[_PROOF_BYTES_PER_BLOB * i : _PROOF_BYTES_PER_BLOB * (i + 1)],
                   BYTES_PER_PROOF, CELLS_PER_EXT_BLOB),
        )
        for i in range(n)
    ]


def _pack_cell_ids(cell_ids):
    """Checked ctypes array of the known cells' numbers."""
    k = len(cell_ids)
    if not CELLS_PER_EXT_BLOB // 2 <= k <= CELLS_PER_EXT_BLOB:
        raise KzgError(
            f"recover_all_cells: {k} cells, need {CELLS_PER_EXT_BLOB // 2}.."
            f"{CELLS_PER_EXT_BLOB}")
    ids = []
    for c in cell_ids:
        try:
            c = int(c)
        except (TypeError, ValueError):
            raise KzgError(f"bad cell id {c!r}") from None
        if not 0 <= c < CELLS_PER_EXT_BLOB:
            raise KzgError(f"cell id {c} outside 0..{CELLS_PER_EXT_BLOB - 1}")
        ids.append(c)
    if len(set(ids)) != k:
        raise KzgError("recover_all_cells: repeated cell id")
    return (ctypes.c_uint64 * k)(*ids)


def _pack_cell_batch(cells, proofs, coordinates, commitments):
    n, m = len(cells), len(commitments)
    if not (n == len(proofs) == len(coordinates)):
        raise KzgError(
            "inconsistent array length: "
            f"{n} cells, {len(proofs)} proofs, {len(coordinates)} coordinates"
        )
    cs = _join("commitment", commitments, BYTES_PER_COMMITMENT)
    ce = _join("cell", cells, BYTES_PER_CELL)
    ps = _join("proof", proofs, BYTES_PER_PROOF)
    rows, cols = [], []
    for coord in coordinates:
        try:
            row, col = coord
            row, col = int(row), int(col)
        except (TypeError, ValueError):
            raise KzgError(f"bad coordinate {coord!r}") from None
        if not 0 <= row < m:
            raise KzgError(f"row {row} outside the {m} commitments")
        if not 0 <= col < CELLS_PER_EXT_BLOB:
            raise KzgError(f"column {col} outside 0..{CELLS_PER_EXT_BLOB - 1}")
        rows.append(row)
        cols.append(col)
    if n == 0:
        return None
    if n > _MAX_BATCH:
        raise KzgError(f"at most {_MAX_BATCH} cells a call")
    u64n = ctypes.c_uint64 * n
    return cs, m, u64n(*rows), u64n(*cols), ce, ps, n


# ---- test/introspection seams (parity tests; not on the import path) ----
def cell_batch_challenge(cells: Sequence[bytes], proofs: Sequence[bytes],
                         coordinates: Sequence[tuple],
                         commitments: Sequence[bytes],
                         ctx: Optional[_native.Ctx] = None) -> bytes:
    """The verify_cell_kzg_proof_batch challenge r, 32 bytes BE."""
    packed = _pack_cell_batch(cells, proofs, coordinates, commitments)
    if packed is None:
        raise KzgError("inconsistent array length")
    ctx = ctx or _native.default_ctx()
    out = ctypes.create_string_buffer(32)
    rc = _native.load().m3x_kzgc_cell_batch_challenge_test(
        ctx.handle, *packed, out)
    if rc != 0:
        raise RuntimeError(f"m3x_kzgc_cell_batch_challenge_test rc={rc}")
    return out.raw


def blob_challenge_eval(blobs: Sequence[bytes], commitments: Sequence[bytes],
                        zs: Optional[Sequence[bytes]] = None,
                        ctx: Optional[_native.Ctx] = None):
    """[(z_i, y_i)]: z_i = compute_challenge(blob_i, commitment_i), or
    zs[i] when given; y_i = the blob polynomial evaluated at z_i."""
    n = len(blobs)
    if n != len(commitments) or (zs is not None and n != len(zs)) or n == 0:
        raise KzgError("inconsistent array length")
    ctx = ctx or _native.default_ctx()
    bl = b"".join(_check_len("blob", b, BYTES_PER_BLOB) for b in blobs)
    cs = b"".join(_check_len("commitment", c, BYTES_PER_COMMITMENT) for c in commitments)
    zb = None
    if zs is not None:
        zb = b"".join(_check_len("z", z, BYTES_PER_FIELD_ELEMENT) for z in zs)
    out_z = ctypes.create_string_buffer(32 * n)
    out_y = ctypes.create_string_buffer(32 * n)
    rc = _native.load().m3x_kzg_blob_challenge_eval(
        ctx.handle, bl, cs, zb, n, out_z, out_y
    )
    if rc == _ERR_ENCODING:
        raise KzgError("non-canonical field element")
    if rc != 0:
        raise RuntimeError(f"m3x_kzg_blob_challenge_eval rc={rc}")
    return [
        (out_z.raw[32 * i : 32 * i + 32], out_y.raw[32 * i : 32 * i + 32])
        for i in range(n)
    ]


def batch_challenge(commitments: Sequence[bytes], zs: Sequence[bytes],
                    ys: Sequence[bytes], proofs: Sequence[bytes],
                    ctx: Optional[_native.Ctx] = None) -> bytes:
    """The verify_kzg_proof_batch Fiat-Shamir challenge r, 32 bytes BE."""
    n = len(commitments)
    if not (n == len(zs) == len(ys) == len(proofs)) or n == 0:
        raise KzgError("inconsistent array length")
    ctx = ctx or _native.default_ctx()
    out = ctypes.create_string_buffer(32)
    rc = _native.load().m3x_kzg_batch_challenge_test(
        ctx.handle,
        b"".join(_check_len("commitment", c, 48) for c in commitments),
        b"".join(_check_len("z", z, 32) for z in zs),
        b"".join(_check_len("y", y, 32) for y in ys),
        b"".join(_check_len("proof", p, 48) for p in proofs),
        n,
        out,
    )
    if rc == _ERR_ENCODING:
        raise KzgError("non-canonical field element")
    if rc != 0:
        raise RuntimeError(f"m3x_kzg_batch_challenge_test rc={rc}")
    return out.raw
