"""Pure-integer restatement of the Deneb polynomial-commitments.md functions
that KZG commitment and proof *computation* adds to tests/kzg_ref.py (test
infrastructure only).

Restated here: compute_kzg_proof_impl's quotient polynomial in evaluation
form, including compute_quotient_eval_within_domain for a z inside the
evaluation domain, and the Lagrange basis evaluated at a known secret,
L_i(tau) = (tau^4096 - 1)/4096 * w_i/(tau - w_i), which turns a 4096-point
setup into 4096 scalars for an insecure test setup."""
import kzg_ref as K

R = K.BLS_MODULUS
N = K.FIELD_ELEMENTS_PER_BLOB


def inv(x):
    return pow(x % R, -1, R)


def compute_quotient_eval_within_domain(z, poly, y):
    """The quotient's value at z when z is one of the roots of unity."""
    roots = K.roots_of_unity_brp()
    result = 0
    for f, w in zip(poly, roots):
        if w == z:
            continue
        result += (f - y) * w % R * inv(z * ((z - w) % R))
    return result % R


def compute_kzg_proof_impl(poly, z):
    """(quotient in evaluation form, y) — the spec's compute_kzg_proof_impl
    up to the final g1_lincomb over the Lagrange setup."""
    roots = K.roots_of_unity_brp()
    z %= R
    y = K.evaluate_polynomial_in_evaluation_form(poly, z)
    quotient = [0] * N
    for i, (f, w) in enumerate(zip(poly, roots)):
        if w == z:
            quotient[i] = compute_quotient_eval_within_domain(z, poly, y)
        else:
            quotient[i] = (f - y) * inv(w - z) % R
    return quotient, y


def lagrange_at(tau, roots):
    """[L_i(tau)] for the given ordering of the 4096 roots of unity."""
    tau %= R
    assert tau not in roots
    scale = (pow(tau, N, R) - 1) * inv(N) % R
    # one inversion for all 4096 denominators (Montgomery's trick)
    dens = [(tau - w) % R for w in roots]
    pre, run = [], 1
    for d in dens:
        run = run * d % R
        pre.append(run)
    acc = inv(run)
    out = [0] * len(roots)
    for i in range(len(roots) - 1, -1, -1):
        d_inv = acc * (pre[i - 1] if i else 1) % R
        acc = acc * dens[i] % R
        out[i] = scale * roots[i] % R * d_inv % R
    return out


def lagrange_scalars_blob_order(tau):
    """L_i(tau) paired with blob element i (bit-reversed roots)."""
    return lagrange_at(tau, K.roots_of_unity_brp())


def lagrange_scalars_file_order(tau):
    """L_k(tau) in the order a trusted-setup file lists g1_lagrange
    (natural powers of omega); bit-reversing it gives the blob order."""
    return lagrange_at(tau, K.compute_roots_of_unity())


def monomial_blob(k):
    """The blob of p(X) = X^k: f_i = w_i^k over the bit-reversed roots."""
    return b"".join(
        pow(w, k, R).to_bytes(32, "big") for w in K.roots_of_unity_brp()
    )


def constant_blob(v):
    return (v % R).to_bytes(32, "big") * N
