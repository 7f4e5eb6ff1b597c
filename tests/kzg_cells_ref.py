"""Pure-integer restatement of the PeerDAS cell functions of Fulu's
polynomial-commitments-sampling.md (test infrastructure only): the 2x
extension of a blob into 128 cells, the coset interpolant of a cell, the
cell quotient, the batch-verification transcript and the batch equation in
scalar form for a known tau.

Conventions (all big-endian, canonical): omega_N = 7^((R-1)/N); cell c is
the polynomial's 64 values on the coset h_c * <omega_64>, with
h_c = omega_8192^bitrev7(c), element i at h_c * omega_64^bitrev6(i). This is
bit_reversal_permutation(roots_of_unity(8192))[64c + i]."""
import kzg_ref as K

R = K.BLS_MODULUS
N = K.FIELD_ELEMENTS_PER_BLOB
FIELD_ELEMENTS_PER_EXT_BLOB = 2 * N
FIELD_ELEMENTS_PER_CELL = 64
CELLS_PER_EXT_BLOB = 128
BYTES_PER_CELL = 32 * FIELD_ELEMENTS_PER_CELL
RANDOM_CHALLENGE_KZG_CELL_BATCH_DOMAIN = b"RCKZGCBATCH__V1_"


def root_of_unity(order):
    assert (R - 1) % order == 0
    return pow(K.PRIMITIVE_ROOT_OF_UNITY, (R - 1) // order, R)


def fft(vals, w):
    """Recursive radix-2: out[k] = sum_j vals[j] * w^(jk), natural order."""
    n = len(vals)
    if n == 1:
        return list(vals)
    w2 = w * w % R
    even, odd = fft(vals[0::2], w2), fft(vals[1::2], w2)
    out, t = [0] * n, 1
    for k in range(n // 2):
        x = t * odd[k] % R
        out[k] = (even[k] + x) % R
        out[k + n // 2] = (even[k] - x) % R
        t = t * w % R
    return out


def ifft(vals, w):
    inv_n = pow(len(vals), -1, R)
    return [v * inv_n % R for v in fft(vals, pow(w, -1, R))]


def blob_coefficients(blob: bytes):
    """Monomial coefficients of the blob polynomial (degree < 4096)."""
    return ifft(K.bit_reversal_permutation(K.blob_to_polynomial(blob)),
                root_of_unity(N))


def cells_from_coefficients(coef):
    assert len(coef) == N
    ext = fft(list(coef) + [0] * N, root_of_unity(2 * N))
    ext = K.bit_reversal_permutation(ext)
    return [ext[64 * c : 64 * c + 64] for c in range(CELLS_PER_EXT_BLOB)]


def compute_cells(blob: bytes):
    """128 cells, each a list of 64 integers."""
    return cells_from_coefficients(blob_coefficients(blob))


def cell_to_bytes(cell):
    return b"".join(v.to_bytes(32, "big") for v in cell)


def cell_from_bytes(raw: bytes):
    assert len(raw) == BYTES_PER_CELL
    out = [int.from_bytes(raw[32 * i : 32 * i + 32], "big") for i in range(64)]
    if any(v >= R for v in out):
        raise ValueError("non-canonical cell element")
    return out


def compute_cells_bytes(blob: bytes):
    return [cell_to_bytes(c) for c in compute_cells(blob)]


def coset_shift(c):
    return pow(root_of_unity(2 * N), K.bitrev(c, 7), R)


def coset_points(c):
    """The 64 evaluation points of cell c, in cell order."""
    h, w64 = coset_shift(c), root_of_unity(64)
    return [h * pow(w64, K.bitrev(i, 6), R) % R for i in range(64)]


def interpolate_cell(c, cell):
    """Coefficients of the degree < 64 polynomial through cell c's values:
    J = IFFT_64(values in natural order), I[j] = J[j] * h_c^(-j)."""
    nat = K.bit_reversal_permutation(list(cell))
    j_coef = ifft(nat, root_of_unity(64))
    h_inv = pow(coset_shift(c), -1, R)
    return [v * pow(h_inv, j, R) % R for j, v in enumerate(j_coef)]


def poly_eval(coef, x):
    acc = 0
    for v in reversed(coef):
        acc = (acc * x + v) % R
    return acc


def cell_quotient(coef, c):
    """coef // (X^64 - h_c^64) by synthetic division (remainder dropped)."""
    hc64 = pow(coset_shift(c), 64, R)
    work = list(coef)
    q = [0] * (len(coef) - 64)
    for k in range(len(coef) - 1, 63, -1):
        q[k - 64] = work[k]
        work[k - 64] = (work[k - 64] + work[k] * hc64) % R
    return q


def cell_batch_transcript(commitments, rows, cols, cells, proofs) -> bytes:
    m, n = len(commitments), len(cells)
    assert n == len(rows) == len(cols) == len(proofs)
    data = RANDOM_CHALLENGE_KZG_CELL_BATCH_DOMAIN
    data += N.to_bytes(8, "big") + FIELD_ELEMENTS_PER_CELL.to_bytes(8, "big")
    data += m.to_bytes(8, "big") + n.to_bytes(8, "big")
    for c in commitments:
        assert len(c) == 48
        data += c
    for row, col, cell, proof in zip(rows, cols, cells, proofs):
        assert len(cell) == BYTES_PER_CELL and len(proof) == 48
        data += row.to_bytes(8, "big") + col.to_bytes(8, "big") + cell + proof
    return data


def cell_batch_challenge(commitments, rows, cols, cells, proofs) -> int:
    return K.hash_to_bls_field(
        cell_batch_transcript(commitments, rows, cols, cells, proofs))


def batch_equation_scalar(tau, r, commit_scalars, rows, cols, cells,
                          proof_scalars) -> bool:
    """The batch check with every point replaced by its discrete log:
    commitment i = [commit_scalars[i]]G1, proof k = [proof_scalars[k]]G1,
    g1_monomial[j] = [tau^j]G1, and e(LL, -[tau^64]G2) * e(RL, G2) == 1
    becomes RL - tau^64 * LL == 0 (mod R). cells are lists of integers."""
    n = len(cells)
    pw = K.compute_powers(r, n)
    ll = sum(pw[k] * proof_scalars[k] for k in range(n)) % R
    weights = [0] * len(commit_scalars)
    for k in range(n):
        weights[rows[k]] = (weights[rows[k]] + pw[k]) % R
    rlc = sum(w * s for w, s in zip(weights, commit_scalars)) % R
    agg = [0] * 64
    for k in range(n):
        for j, v in enumerate(interpolate_cell(cols[k], cells[k])):
            agg[j] = (agg[j] + pw[k] * v) % R
    rli = poly_eval(agg, tau)
    rlp = sum(pw[k] * pow(coset_shift(cols[k]), 64, R) % R * proof_scalars[k]
              for k in range(n)) % R
    return (rlc - rli + rlp - pow(tau, 64, R) * ll) % R == 0
