"""Exact-integer restatement of the two-pow hash-to-curve square roots in
lighthouse_amd/csrc/bls_device.hh (fp2_sqrt_from_norm_root, fp2_sqrt,
sswu_g2), over the arithmetic of tests/golden/gen_bls_fixtures.py.

Not a test module: tests/test_h2c_sqrt_formulas_ref.py checks these against
the by-definition forms, tests/test_gpu_h2c_paths.py uses them as the
reference and to classify its inputs."""
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tests" / "golden"))

import gen_bls_fixtures as G  # noqa: E402
import gen_h2c_consts as GH  # noqa: E402

P = G.P
E_M3 = (P - 3) // 4  # a^E_M3 = 1/sqrt(a) for a square a
INV2 = pow(2, P - 2, P)
SQRT_M5 = GH.SQRT_NEG5  # the generated constant
A, B, Z = G.A_P, G.B_P, G.Z_SSWU

POWS = {"n": 0}  # 381-bit Fp exponentiations executed


def fp_pow(a, e):
    POWS["n"] += 1
    return pow(a, e, P)


def legendre(a):
    a %= P
    return 0 if a == 0 else (1 if pow(a, (P - 1) // 2, P) == 1 else -1)


def norm(a):
    return (a[0] * a[0] + a[1] * a[1]) % P


def fp2_sqrt_from_norm_root(a, s):
    """a = a0 + a1 i with a1 != 0 and s^2 = N(a): one pow, one select.
    d = (a0+s)/2, u = d^((p-3)/4), t = u d. Then t^2 = +-d and the root is
    (t, a1 u/2) for "+", (-a1 u/2, t) for "-". Returns (root, sign)."""
    a0, a1 = a
    d = (a0 + s) * INV2 % P
    u = fp_pow(d, E_M3)
    t = u * d % P
    h = a1 * u % P * INV2 % P
    plus = t * t % P == d
    return ((t, h) if plus else ((-h) % P, t)), (1 if plus else -1)


def fp2_sqrt(a):
    """Two pows, no retry. None for a non-square."""
    a = (a[0] % P, a[1] % P)
    if a == (0, 0):
        return (0, 0)
    if a[1] == 0:  # rare: Fp element, always a square in Fp2
        s = fp_pow(a[0], (P + 1) // 4)
        if s * s % P == a[0]:
            return (s, 0)
        s = fp_pow((-a[0]) % P, (P + 1) // 4)
        return (0, s)
    n = norm(a)
    s = fp_pow(n, (P + 1) // 4)
    if s * s % P != n:
        return None
    cand, _ = fp2_sqrt_from_norm_root(a, s)
    return cand if G.f2sq(cand) == a else None


def sqrt_sign(a):
    """Which sign of t^2 = +-d the root of the square a (a1 != 0) takes."""
    s = pow(norm(a), (P + 1) // 4, P)
    assert s * s % P == norm(a)
    return fp2_sqrt_from_norm_root(a, s)[1]


def sswu_slow(u):
    """Exceptional inputs: the by-definition map with a real inversion."""
    zu2 = G.f2mul(Z, G.f2sq(u))
    tv = G.f2add(G.f2sq(zu2), zu2)
    if tv == (0, 0):
        x1 = G.f2mul(B, G.f2inv(G.f2mul(Z, A)))
    else:
        x1 = G.f2mul(G.f2mul(G.f2neg(B), G.f2inv(A)),
                     G.f2add((1, 0), G.f2inv(tv)))
    gx = lambda x: G.f2add(G.f2mul(G.f2sq(x), x), G.f2add(G.f2mul(A, x), B))
    x, y = x1, fp2_sqrt(gx(x1))
    if y is None:
        x = G.f2mul(zu2, x1)
        y = fp2_sqrt(gx(x))
    if G.sgn0_fp2(u) != G.sgn0_fp2(y):
        y = G.f2neg(y)
    return (x, y)


def sswu_two_pow(u, info=None):
    """Projective SSWU: x1 = xn/xd, a = gn*xd = g(x1)*xd^4. One pow on N(a)
    gives the square test, sqrt(N(a)) and 1/N(a); the failed test already
    holds sqrt(N(zu2^3 a)) for the second candidate; one more pow gives the
    Fp2 root. No inversion, no retry."""
    u = (u[0] % P, u[1] % P)
    zu2 = G.f2mul(Z, G.f2sq(u))
    tv = G.f2add(G.f2sq(zu2), zu2)
    xn = G.f2mul(B, G.f2add(tv, (1, 0)))
    xd = G.f2mul(Z, A) if tv == (0, 0) else G.f2neg(G.f2mul(A, tv))
    xd2 = G.f2sq(xd)
    gn = G.f2add(
        G.f2mul(G.f2add(G.f2sq(xn), G.f2mul(A, xd2)), xn),
        G.f2mul(B, G.f2mul(xd2, xd)),
    )
    a = G.f2mul(gn, xd)
    n = norm(a)
    u1 = fp_pow(n, E_M3)
    s1 = u1 * n % P
    is_sq = s1 * s1 % P == n  # gx1 square <=> N(a) a residue
    # second candidate: a2 = zu2^3 a = g(x2) xd^4, sqrt(N(a2)) from s1
    zu2_3 = G.f2mul(G.f2sq(zu2), zu2)
    a2 = G.f2mul(zu2_3, a)
    s2 = norm(zu2) * norm(u) % P * SQRT_M5 % P * s1 % P
    sel = a if is_sq else a2
    s = s1 if is_sq else s2
    if n == 0 or sel[1] == 0:
        if info is not None:
            info.update(slow=True)
        return sswu_slow(u)
    root, sign = fp2_sqrt_from_norm_root(sel, s)
    # 1/xd = conj(xd) N(gn) / N(a), 1/N(a) = +-u1^2 by the square test
    ninv = u1 * u1 % P
    if not is_sq:
        ninv = (-ninv) % P
    k = norm(gn) * ninv % P
    xdi = G.f2smul(G.f2conj(xd), k)
    x = G.f2mul(xn, xdi)
    if not is_sq:
        x = G.f2mul(x, zu2)
    y = G.f2mul(root, G.f2sq(xdi))
    if G.sgn0_fp2(u) != G.sgn0_fp2(y):
        y = G.f2neg(y)
    if info is not None:
        info.update(slow=False, gx1_square=is_sq, sign=sign)
    return (x, y)


def classify(u):
    """(gx1 is a square, sign of t^2 = +-d) for a non-exceptional u."""
    info = {}
    sswu_two_pow(u, info)
    assert not info["slow"]
    return info["gx1_square"], info["sign"]


def h2c_point_no_clear(u):
    """SSWU + 3-isogeny, affine, no cofactor clear (m3x_bls_sswu_test)."""
    return G.iso_map(sswu_two_pow(u))
