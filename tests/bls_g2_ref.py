"""Exact-integer affine arithmetic on the BLS12-381 G2 curve
E'(Fp2): y^2 = x^3 + 4(1 + u), Fp2 = Fp[u]/(u^2 + 1), over Python ints.

A reference for tests only: textbook chord-and-tangent formulas and a
double-and-add, nothing shared with the device code. A point is None
(infinity) or ((x0, x1), (y0, y1)) with x = x0 + x1 u."""

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * d % P, -a[1] * d % P)


B2 = (4, 4)


def on_curve(pt):
    if pt is None:
        return True
    x, y = pt
    return f2_mul(y, y) == f2_add(f2_mul(f2_mul(x, x), x), B2)


def neg(pt):
    if pt is None:
        return None
    x, y = pt
    return (x, ((-y[0]) % P, (-y[1]) % P))


def add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if y1 != y2 or y1 == (0, 0):
            return None
        xx = f2_mul(x1, x1)
        lam = f2_mul(f2_add(f2_add(xx, xx), xx), f2_inv(f2_add(y1, y1)))
    else:
        lam = f2_mul(f2_sub(y2, y1), f2_inv(f2_sub(x2, x1)))
    x3 = f2_sub(f2_sub(f2_mul(lam, lam), x1), x2)
    y3 = f2_sub(f2_mul(lam, f2_sub(x1, x3)), y1)
    return (x3, y3)


def mul(k, pt):
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, pt)
    return acc


def from_uncompressed(b):
    """192 bytes x.c1 || x.c0 || y.c1 || y.c0, big-endian; infinity is the
    0x40 flag in the first byte."""
    assert len(b) == 192
    if b[0] & 0x40:
        return None
    v = [int.from_bytes(b[48 * i : 48 * (i + 1)], "big") for i in range(4)]
    pt = ((v[1], v[0]), (v[3], v[2]))
    assert on_curve(pt)
    return pt


def to_uncompressed(pt):
    """The device test entry's form: infinity is 192 zero bytes."""
    if pt is None:
        return bytes(192)
    (x0, x1), (y0, y1) = pt
    return b"".join(v.to_bytes(48, "big") for v in (x1, x0, y1, y0))


def weighted_sum(points, scalars):
    acc = None
    for pt, k in zip(points, scalars):
        acc = add(acc, mul(k, pt))
    return acc
