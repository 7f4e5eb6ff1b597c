"""Pure-integer restatement of PeerDAS cell recovery (Fulu
polynomial-commitments-sampling.md, recover_polynomialcoeff and the cell half
of recover_cells_and_kzg_proofs), on top of kzg_cells_ref. Test
infrastructure only: full 8192-point fft / ifft, the vanishing polynomial
formed coefficient by coefficient, nothing shared with the GPU pipeline."""
import kzg_cells_ref as C
import kzg_ref as K

R = C.R
N = C.N
EXT = C.FIELD_ELEMENTS_PER_EXT_BLOB
CELLS = C.CELLS_PER_EXT_BLOB
PER_CELL = C.FIELD_ELEMENTS_PER_CELL


def check_cell_ids(cell_ids):
    """The argument rules of recover_cells_and_kzg_proofs."""
    ids = [int(c) for c in cell_ids]
    if not CELLS // 2 <= len(ids) <= CELLS:
        raise ValueError(f"{len(ids)} cells: need {CELLS // 2}..{CELLS}")
    if any(not 0 <= c < CELLS for c in ids):
        raise ValueError("cell id outside 0..127")
    if len(set(ids)) != len(ids):
        raise ValueError("repeated cell id")
    return ids


def vanishing_poly_coeff(missing):
    """construct_vanishing_polynomial: Z(x) = S(x^64), S the product of
    (y - omega_128^bitrev7(c)) over the missing cells; 8192 coefficients."""
    w128 = C.root_of_unity(CELLS)
    short = [1]
    for c in missing:
        root = pow(w128, K.bitrev(c, 7), R)
        nxt = [0] * (len(short) + 1)
        for i, v in enumerate(short):
            nxt[i] = (nxt[i] - root * v) % R
            nxt[i + 1] = (nxt[i + 1] + v) % R
        short = nxt
    z = [0] * EXT
    for i, v in enumerate(short):
        z[i * PER_CELL] = v  # degree 64 * 64 = 4096 < 8192 at most
    return z


def coset_fft(vals, w, shift):
    return C.fft([v * pow(shift, i, R) % R for i, v in enumerate(vals)], w)


def coset_ifft(vals, w, shift):
    inv = pow(shift, -1, R)
    return [v * pow(inv, i, R) % R for i, v in enumerate(C.ifft(vals, w))]


def recover_polynomialcoeff(cell_ids, cells):
    """All 8192 coefficients of the recovered quotient (the upper 4096 are
    zero exactly when the cells lie on one polynomial of degree < 4096)."""
    w = C.root_of_unity(EXT)
    ext_rbo = [0] * EXT
    for c, cell in zip(cell_ids, cells):
        ext_rbo[PER_CELL * c : PER_CELL * (c + 1)] = cell
    ext = K.bit_reversal_permutation(ext_rbo)
    missing = [c for c in range(CELLS) if c not in set(cell_ids)]
    z_coef = vanishing_poly_coeff(missing)
    z_eval = C.fft(z_coef, w)
    ez_eval = [a * b % R for a, b in zip(z_eval, ext)]
    ez_coef = C.ifft(ez_eval, w)
    shift = K.PRIMITIVE_ROOT_OF_UNITY
    ez_coset = coset_fft(ez_coef, w, shift)
    z_coset = coset_fft(z_coef, w, shift)
    q_coset = [a * pow(b, -1, R) % R for a, b in zip(ez_coset, z_coset)]
    return coset_ifft(q_coset, w, shift)


def recover_cells(cell_ids, cells):
    """128 cells (lists of 64 integers) from k >= 64 distinct known ones,
    given as lists of integers in the order of cell_ids. ValueError on the
    argument rules and when the cells are inconsistent."""
    ids = check_cell_ids(cell_ids)
    if len(cells) != len(ids):
        raise ValueError(f"{len(ids)} ids but {len(cells)} cells")
    for cell in cells:
        if len(cell) != PER_CELL or any(not 0 <= v < R for v in cell):
            raise ValueError("malformed cell")
    coef = recover_polynomialcoeff(ids, cells)
    if any(coef[N:]):
        raise ValueError("cells do not lie on one polynomial of degree < 4096")
    return C.cells_from_coefficients(coef[:N])


def recover_cells_bytes(cell_ids, cells):
    ints = []
    for raw in cells:
        if len(raw) != C.BYTES_PER_CELL:
            raise ValueError("cell length")
        ints.append(C.cell_from_bytes(raw))
    return [C.cell_to_bytes(c) for c in recover_cells(cell_ids, ints)]
