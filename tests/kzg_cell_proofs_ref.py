"""Pure-integer restatement of what the cell-proof kernels do (test
infrastructure only), with every G1 point [k]G1 replaced by its scalar k:

  h_m     = sum_{j=0}^{4095-64(m+1)} p[j + 64(m+1)] * mono[j]     m = 0..62
  proof_c = sum_{m=0}^{62} y_c^m * h_m,  y_c = omega_128^bitrev7(c)

toeplitz_scalars is stage 1 (with the kernel's block decomposition),
dif128 stage 2: the radix-2 decimation-in-frequency transform with natural
input, a twiddle after each subtraction, and cell order on output.
signed_digits is the recoding the look-up kernel reads."""
import kzg_cells_ref as C
import kzg_ref as K

R = K.BLS_MODULUS
N = K.FIELD_ELEMENTS_PER_BLOB
SUMS = 63


def signed_digits(s):
    """64 digits d_k in [-7, 8] with s = sum d_k 16^k, for 0 <= s < 2^255."""
    out, carry = [], 0
    for k in range(64):
        d = ((s >> (4 * k)) & 15) + carry
        carry = 1 if d > 8 else 0
        if carry:
            d -= 16
        out.append(d)
    assert carry == 0
    return out


def first_block(m):
    """Index of h_m's first block sum: sums 0..m-1 have 63, 62, ... blocks."""
    return SUMS * m - m * (m - 1) // 2


def toeplitz_scalars(coef, mono):
    """h_0..h_62 over the scalars mono[j] (= tau^j for a real setup), summed
    block by block as the kernel does: block bx of h_m holds j = 64 bx ..
    64 bx + 63 and exists for bx + m <= 62."""
    assert len(coef) == N and len(mono) == N
    hs = []
    for m in range(SUMS):
        blocks = []
        for bx in range(SUMS - m):
            acc = 0
            for j in range(64 * bx, 64 * bx + 64):
                i = j + 64 * (m + 1)
                assert i < N
                acc += coef[i] * mono[j]
            blocks.append(acc % R)
        assert first_block(m) + len(blocks) == (
            first_block(m + 1) if m + 1 < SUMS else 2016)
        hs.append(sum(blocks) % R)
    return hs


def dif128(hs, twiddles):
    """128 outputs, position c holding sum_m y_c^m h_m. twiddles[k] =
    omega_128^k, k = 0..63 (the generated header's table)."""
    assert len(hs) == SUMS and len(twiddles) == 64
    p = list(hs) + [0] * (128 - SUMS)
    half = 64
    while half >= 1:
        for t in range(64):  # one butterfly per lane
            pos = t & (half - 1)
            lo = 2 * (t - pos) + pos
            hi = lo + half
            x, y = p[lo], p[hi]
            p[lo] = (x + y) % R
            d = (x - y) % R
            if half > 1:  # the last stage's twiddles are all 1
                d = d * twiddles[pos * (64 // half)] % R
            p[hi] = d
        half >>= 1
    return p


def cell_proof_scalars(coef, tau):
    """q_c(tau) for c = 0..127 by the kernels' route."""
    import gen_kzg_cell_proof_consts as GP

    mono = [pow(tau, j, R) for j in range(N)]
    return dif128(toeplitz_scalars(coef, mono), GP.twiddles())


def cell_proof_scalars_direct(coef, tau):
    """The definition: q_c = p // (X^64 - y_c) evaluated at tau."""
    return [C.poly_eval(C.cell_quotient(coef, c), tau) for c in range(128)]
