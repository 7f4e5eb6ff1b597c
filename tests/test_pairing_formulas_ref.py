"""The per-lane Miller loop's reduced-multiply formulas, restated literally
from lighthouse_amd/csrc/bls_device.hh over the exact-integer arithmetic of
tests/golden/gen_bls_fixtures.py and checked against its schoolbook /
generic forms (CPU only):

  * f6_mul       Karatsuba, 6 Fp2 products          == schoolbook (9)
  * f12_mul_nn / f12_sqr_nn over that f6_mul        == f12mul
  * f12_line_nn  sparse tower product, 14 products  == f12mul with the line
                                                       embedded densely
  * miller_raw   merged doubling+line step, xi-scaled lines, both points
                 Jacobian with Z != 1               == pairing(P, Q) after
                                                       the final exponentiation
  * the same loop gives one when either argument is infinity

The product counts are asserted too, so the test pins the multiply budget
the kernels are built on, not only the values."""
import random
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tests" / "golden"))

import gen_bls_fixtures as G  # noqa: E402

P = G.P
X_ABS = G.H_EFF_ABS

# ------------------------------------------------- counted Fp2 primitives
MULS = {"fp2_mul": 0, "fp": 0}


def fp2_mul(a, b):
    MULS["fp2_mul"] += 1
    MULS["fp"] += 3
    return G.f2mul(a, b)


def fp2_sqr(a):
    MULS["fp"] += 2
    return G.f2mul(a, a)


def fp2_mul_fp(a, k):
    MULS["fp"] += 2
    return G.f2smul(a, k)


def fp2_mul_xi(a):  # (c0 - c1) + (c0 + c1) u : adds only
    return ((a[0] - a[1]) % P, (a[0] + a[1]) % P)


def fp2_dbl(a):
    return G.f2add(a, a)


add, sub, neg = G.f2add, G.f2sub, G.f2neg


def reset():
    MULS["fp2_mul"] = 0
    MULS["fp"] = 0


# ------------------------------------------------------------ Fp6 / Fp12
# fp12m layout: 6 Fp2 coefficients of w; tower view A = (c0,c2,c4),
# B = (c1,c3,c5), f = A + w B, w^2 = v, v^3 = xi.


def f6_add(a, b):
    return [add(a[i], b[i]) for i in range(3)]


def f6_sub(a, b):
    return [sub(a[i], b[i]) for i in range(3)]


def f6_mul_v(a):
    return [fp2_mul_xi(a[2]), a[0], a[1]]


def f6_mul(a, b):
    v0 = fp2_mul(a[0], b[0])
    v1 = fp2_mul(a[1], b[1])
    v2 = fp2_mul(a[2], b[2])
    m12 = fp2_mul(add(a[1], a[2]), add(b[1], b[2]))
    m01 = fp2_mul(add(a[0], a[1]), add(b[0], b[1]))
    m02 = fp2_mul(add(a[0], a[2]), add(b[0], b[2]))
    c0 = add(v0, fp2_mul_xi(sub(sub(m12, v1), v2)))
    c1 = add(sub(sub(m01, v0), v1), fp2_mul_xi(v2))
    c2 = add(sub(sub(m02, v0), v2), v1)
    return [c0, c1, c2]


def f6_mul_schoolbook(a, b):
    acc = [G.F2_ZERO] * 5
    for i in range(3):
        for j in range(3):
            acc[i + j] = add(acc[i + j], G.f2mul(a[i], b[j]))
    return [
        add(acc[0], fp2_mul_xi(acc[3])),
        add(acc[1], fp2_mul_xi(acc[4])),
        acc[2],
    ]


def f6_mul_fp2(a, k):
    return [fp2_mul(a[0], k), fp2_mul(a[1], k), fp2_mul(a[2], k)]


def f6_mul_012s(a, b1, b2):
    v1 = fp2_mul(a[1], b1)
    v2 = fp2_mul(a[2], b2)
    s = fp2_mul(add(a[1], a[2]), add(b1, b2))
    c0 = fp2_mul_xi(sub(sub(s, v1), v2))
    c1 = add(fp2_mul(a[0], b1), fp2_mul_xi(v2))
    c2 = add(fp2_mul(a[0], b2), v1)
    return [c0, c1, c2]


def f12_split(f):
    return [f[0], f[2], f[4]], [f[1], f[3], f[5]]


def f12_join(A, B):
    return [A[0], B[0], A[1], B[1], A[2], B[2]]


def f12_mul_nn(a, b):
    A1, B1 = f12_split(a)
    A2, B2 = f12_split(b)
    aa = f6_mul(A1, A2)
    bb = f6_mul(B1, B2)
    cross = f6_mul(f6_add(A1, B1), f6_add(A2, B2))
    cross = f6_sub(f6_sub(cross, aa), bb)
    return f12_join(f6_add(aa, f6_mul_v(bb)), cross)


def f12_sqr_nn(a):
    A, B = f12_split(a)
    m1 = f6_mul(A, B)
    t = f6_mul(f6_add(A, B), f6_add(A, f6_mul_v(B)))
    t = f6_sub(t, m1)
    even = f6_sub(t, f6_mul_v(m1))
    return f12_join(even, f6_add(m1, m1))


def f12_line_nn(f, a0, a3, a5):
    A, B = f12_split(f)
    aa = f6_mul_fp2(A, a0)
    bb = f6_mul_012s(B, a3, a5)
    cross = f6_mul(f6_add(A, B), [a0, a3, a5])
    cross = f6_sub(f6_sub(cross, aa), bb)
    return f12_join(f6_add(aa, f6_mul_v(bb)), cross)


# ------------------------------------------------------------ Miller loop


def g2j_add(p, q):
    """add-2007-bl, as g2j_add (neither input infinite, p != +-q here)."""
    X1, Y1, Z1 = p
    X2, Y2, Z2 = q
    z1z1, z2z2 = fp2_sqr(Z1), fp2_sqr(Z2)
    u1, u2 = fp2_mul(X1, z2z2), fp2_mul(X2, z1z1)
    s1 = fp2_mul(Y1, fp2_mul(Z2, z2z2))
    s2 = fp2_mul(Y2, fp2_mul(Z1, z1z1))
    assert u1 != u2
    h = sub(u2, u1)
    i = fp2_sqr(fp2_dbl(h))
    j = fp2_mul(h, i)
    rr = fp2_dbl(sub(s2, s1))
    v = fp2_mul(u1, i)
    x3 = sub(sub(sub(fp2_sqr(rr), j), v), v)
    y3 = sub(fp2_mul(rr, sub(v, x3)), fp2_dbl(fp2_mul(s1, j)))
    z3 = fp2_mul(sub(sub(fp2_sqr(add(Z1, Z2)), z1z1), z2z2), h)
    return (x3, y3, z3)


def miller_precompute(Pj, Qj):
    Xp, Yp, Zp = Pj
    zp3 = Zp * Zp % P * Zp % P
    zq2 = fp2_sqr(Qj[2])
    return {
        "xp": Xp * Zp % P,
        "yp": Yp,
        "zp3": zp3,
        "zq2": zq2,
        "zq3": fp2_mul(zq2, Qj[2]),
    }


def miller_dbl_step(T, c):
    X, Y, Z = T
    A = fp2_sqr(X)
    B = fp2_sqr(Y)
    Z2 = fp2_sqr(Z)
    E = add(fp2_dbl(A), A)
    Z3 = fp2_dbl(fp2_mul(Y, Z))
    a0 = fp2_mul_xi(fp2_mul_fp(fp2_mul(Z3, Z2), c["yp"]))
    a3 = fp2_mul_fp(sub(fp2_mul(E, X), fp2_dbl(B)), c["zp3"])
    a5 = neg(fp2_mul_fp(fp2_mul(E, Z2), c["xp"]))
    C = fp2_sqr(B)
    D = fp2_dbl(sub(sub(fp2_sqr(add(X, B)), A), C))
    F = sub(sub(fp2_sqr(E), D), D)
    C8 = fp2_dbl(fp2_dbl(fp2_dbl(C)))
    Y3 = sub(fp2_mul(E, sub(D, F)), C8)
    return (F, Y3, Z3), (a0, a3, a5)


def miller_add_step(T, Qj, c):
    X, Y, Z = T
    Z2 = fp2_sqr(Z)
    Z3 = fp2_mul(Z2, Z)
    Hs = sub(fp2_mul(X, c["zq2"]), fp2_mul(Qj[0], Z2))
    Ms = sub(fp2_mul(Y, c["zq3"]), fp2_mul(Qj[1], Z3))
    HZq = fp2_mul(Hs, Qj[2])
    a0 = fp2_mul_xi(fp2_mul_fp(fp2_mul(Z3, HZq), c["yp"]))
    a3 = fp2_mul_fp(sub(fp2_mul(Ms, X), fp2_mul(Y, HZq)), c["zp3"])
    a5 = neg(fp2_mul_fp(fp2_mul(Ms, Z2), c["xp"]))
    return g2j_add(T, Qj), (a0, a3, a5)


def miller_raw(Pj, Qj):
    f = list(G.F12_ONE)
    if Pj[2] == 0 or Qj[2] == G.F2_ZERO:
        return f  # e(O, .) = e(., O) = 1
    c = miller_precompute(Pj, Qj)
    T = Qj
    for i in range(62, -1, -1):
        f = f12_sqr_nn(f)
        T, l = miller_dbl_step(T, c)
        f = f12_line_nn(f, *l)
        if (X_ABS >> i) & 1:
            T, l = miller_add_step(T, Qj, c)
            f = f12_line_nn(f, *l)
    return G.f12conj6(f)


# ------------------------------------------------------------------ tests


def rand_f2(rng):
    return (rng.randrange(P), rng.randrange(P))


def rand_f6(rng):
    return [rand_f2(rng) for _ in range(3)]


def rand_f12(rng):
    return [rand_f2(rng) for _ in range(6)]


def test_f6_mul_karatsuba_equals_schoolbook():
    rng = random.Random(0xF6)
    for _ in range(20):
        a, b = rand_f6(rng), rand_f6(rng)
        reset()
        got = f6_mul(a, b)
        assert MULS["fp2_mul"] == 6
        assert got == f6_mul_schoolbook(a, b)
    # edge operands: zero, one, a single v^2 term (exercises both xi folds)
    z, one = [G.F2_ZERO] * 3, [G.F2_ONE, G.F2_ZERO, G.F2_ZERO]
    v2 = [G.F2_ZERO, G.F2_ZERO, G.F2_ONE]
    a = rand_f6(rng)
    assert f6_mul(a, z) == z
    assert f6_mul(a, one) == a
    assert f6_mul(v2, v2) == f6_mul_schoolbook(v2, v2) == [G.F2_ZERO, G.XI, G.F2_ZERO]


def test_f12_tower_mul_and_sqr_equal_generic():
    rng = random.Random(0xF12)
    for _ in range(6):
        a, b = rand_f12(rng), rand_f12(rng)
        reset()
        assert f12_mul_nn(a, b) == G.f12mul(a, b)
        assert MULS["fp2_mul"] == 18
        reset()
        assert f12_sqr_nn(a) == G.f12mul(a, a)
        assert MULS["fp2_mul"] == 12


def test_line_product_14_equals_dense():
    rng = random.Random(0x11E)
    for _ in range(10):
        f = rand_f12(rng)
        a0, a3, a5 = rand_f2(rng), rand_f2(rng), rand_f2(rng)
        dense = [a0, G.F2_ZERO, G.F2_ZERO, a3, G.F2_ZERO, a5]
        reset()
        got = f12_line_nn(f, a0, a3, a5)
        assert MULS["fp2_mul"] == 14
        assert got == G.f12mul(f, dense)
    # a line with a vanishing coefficient (a5 = 0 happens for xp = 0)
    f = rand_f12(rng)
    a0, a3 = rand_f2(rng), rand_f2(rng)
    assert f12_line_nn(f, a0, a3, G.F2_ZERO) == G.f12mul(
        f, [a0, G.F2_ZERO, G.F2_ZERO, a3, G.F2_ZERO, G.F2_ZERO]
    )


def to_jac1(p, z):
    return (p[0] * z * z % P, p[1] * z * z * z % P, z)


def to_jac2(q, z):
    z2 = G.f2mul(z, z)
    return (G.f2mul(q[0], z2), G.f2mul(q[1], G.f2mul(z2, z)), z)


@pytest.fixture(scope="module")
def points():
    rng = random.Random(0xB15)
    pa = G.g1_mul(rng.randrange(1, G.R), G.G1G)
    qa = G.g2_mul(rng.randrange(1, G.R), G.G2G)
    return rng, pa, qa


def test_doubling_step_counts_and_point(points):
    """The merged step returns exactly 2T (checked in affine form) for 33 Fp
    products; the addition step returns T + Q."""
    rng, pa, qa = points
    Pj = to_jac1(pa, rng.randrange(2, P))
    Qj = to_jac2(qa, rand_f2(rng))
    c = miller_precompute(Pj, Qj)
    reset()
    T2, _ = miller_dbl_step(Qj, c)
    assert MULS["fp"] == 33

    def aff(t):
        zi = G.f2inv(t[2])
        zi2 = G.f2mul(zi, zi)
        return (G.f2mul(t[0], zi2), G.f2mul(t[1], G.f2mul(zi2, zi)))

    assert aff(T2) == G.g2_add(qa, qa)
    T3, _ = miller_add_step(T2, Qj, c)
    assert aff(T3) == G.g2_mul(3, qa)


def test_miller_loop_equals_pairing(points):
    rng, pa, qa = points
    Pj = to_jac1(pa, rng.randrange(2, P))
    Qj = to_jac2(qa, rand_f2(rng))
    got = G.f12pow(miller_raw(Pj, Qj), G.FINAL_EXP)
    assert got == G.pairing(pa, qa)
    assert got != G.F12_ONE
    # affine inputs (Z = 1) take the same path
    got1 = G.f12pow(miller_raw(to_jac1(pa, 1), to_jac2(qa, G.F2_ONE)), G.FINAL_EXP)
    assert got1 == got


def test_miller_loop_infinity_gives_one(points):
    rng, pa, qa = points
    Pj = to_jac1(pa, rng.randrange(2, P))
    Qj = to_jac2(qa, rand_f2(rng))
    inf1 = (0, 0, 0)
    inf2 = (G.F2_ZERO, G.F2_ZERO, G.F2_ZERO)
    for f in (miller_raw(inf1, Qj), miller_raw(Pj, inf2), miller_raw(inf1, inf2)):
        assert f == G.F12_ONE
        assert G.f12pow(f, G.FINAL_EXP) == G.F12_ONE
