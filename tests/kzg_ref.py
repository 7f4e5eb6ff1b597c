"""Pure-integer restatement of the Deneb polynomial-commitments.md functions
that KZG proof *verification* needs (test infrastructure only).

Everything is big-endian, N = 4096, scalars live in the BLS12-381 scalar
field. Restated here: bit-reversal permutation and roots of unity,
compute_challenge, evaluate_polynomial_in_evaluation_form (with the
in-domain branch), the verify_kzg_proof_batch challenge and its powers.
Also the seed-derived blob used by the tests and fixtures."""
import hashlib

BLS_MODULUS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
PRIMITIVE_ROOT_OF_UNITY = 7
FIELD_ELEMENTS_PER_BLOB = 4096
BYTES_PER_FIELD_ELEMENT = 32
BYTES_PER_BLOB = FIELD_ELEMENTS_PER_BLOB * BYTES_PER_FIELD_ELEMENT
BYTES_PER_COMMITMENT = 48
BYTES_PER_PROOF = 48
FIAT_SHAMIR_PROTOCOL_DOMAIN = b"FSBLOBVERIFY_V1_"
RANDOM_CHALLENGE_KZG_BATCH_DOMAIN = b"RCKZGBATCH___V1_"
G1_POINT_AT_INFINITY = bytes([0xC0] + [0] * 47)

R = BLS_MODULUS
N = FIELD_ELEMENTS_PER_BLOB


def bitrev(j, bits=12):
    out = 0
    for _ in range(bits):
        out = (out << 1) | (j & 1)
        j >>= 1
    return out


def bit_reversal_permutation(seq):
    bits = (len(seq) - 1).bit_length()
    return [seq[bitrev(i, bits)] for i in range(len(seq))]


def compute_roots_of_unity(order=N):
    w = pow(PRIMITIVE_ROOT_OF_UNITY, (R - 1) // order, R)
    out = [1]
    for _ in range(order - 1):
        out.append(out[-1] * w % R)
    assert out[-1] * w % R == 1
    return out


_ROOTS_BRP = None


def roots_of_unity_brp():
    """omega^bitrev12(j) for j in 0..4095 (the order blob elements use)."""
    global _ROOTS_BRP
    if _ROOTS_BRP is None:
        _ROOTS_BRP = bit_reversal_permutation(compute_roots_of_unity())
    return _ROOTS_BRP


def blob_from_seed(seed: bytes) -> bytes:
    """element j = int_be(SHA256(seed || LE32(j))) mod r, 32 BE bytes."""
    out = bytearray()
    for j in range(N):
        h = hashlib.sha256(seed + j.to_bytes(4, "little")).digest()
        out += (int.from_bytes(h, "big") % R).to_bytes(32, "big")
    return bytes(out)


def blob_to_polynomial(blob: bytes):
    assert len(blob) == BYTES_PER_BLOB
    poly = []
    for j in range(N):
        v = int.from_bytes(blob[32 * j : 32 * j + 32], "big")
        if v >= R:
            raise ValueError("non-canonical field element %d" % j)
        poly.append(v)
    return poly


def hash_to_bls_field(data: bytes) -> int:
    return int.from_bytes(hashlib.sha256(data).digest(), "big") % R


def compute_challenge(blob: bytes, commitment: bytes) -> int:
    assert len(blob) == BYTES_PER_BLOB and len(commitment) == 48
    degree_poly = N.to_bytes(16, "big")
    return hash_to_bls_field(
        FIAT_SHAMIR_PROTOCOL_DOMAIN + degree_poly + blob + commitment
    )


def evaluate_polynomial_in_evaluation_form(poly, z: int) -> int:
    roots = roots_of_unity_brp()
    z %= R
    if z in roots:
        return poly[roots.index(z)]
    acc = 0
    for f, w in zip(poly, roots):
        acc += f * w % R * pow((z - w) % R, -1, R)
    return acc % R * ((pow(z, N, R) - 1) % R) % R * pow(N, -1, R) % R


def challenge_and_eval(blob: bytes, commitment: bytes, z=None):
    """(z, y) as 32-byte big-endian strings; z from Fiat-Shamir if None."""
    if z is None:
        z = compute_challenge(blob, commitment)
    y = evaluate_polynomial_in_evaluation_form(blob_to_polynomial(blob), z)
    return z.to_bytes(32, "big"), y.to_bytes(32, "big")


def compute_batch_challenge(commitments, zs, ys, proofs) -> int:
    """verify_kzg_proof_batch's r; zs/ys are 32-byte BE strings."""
    n = len(commitments)
    assert n == len(zs) == len(ys) == len(proofs)
    data = RANDOM_CHALLENGE_KZG_BATCH_DOMAIN
    data += N.to_bytes(8, "big") + n.to_bytes(8, "big")
    for c, z, y, p in zip(commitments, zs, ys, proofs):
        assert len(c) == 48 and len(z) == 32 and len(y) == 32 and len(p) == 48
        data += c + z + y + p
    return hash_to_bls_field(data)


def compute_powers(x: int, n: int):
    out, cur = [], 1
    for _ in range(n):
        out.append(cur)
        cur = cur * x % R
    return out


def poly_eval_at_secret(poly, tau: int) -> int:
    """p(tau) for an evaluation-form polynomial (insecure test setup)."""
    return evaluate_polynomial_in_evaluation_form(poly, tau)
