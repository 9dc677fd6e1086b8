"""tests/pyref/secp.py — TEST INFRASTRUCTURE: the secp256k1 group and its fields over Python integers, written from the
published definitions and on purpose with other algorithms than the kernels (lachain_amd/csrc/secp.hpp): a textbook
affine group law with None for infinity, plain modular arithmetic, and the Montgomery map of the scalar routines stated
as one multiplication by R^-1.  The yardstick of tests/test_secp_asm_sim.py, tests/test_secp_edges_emul.py and
tests/test_gpu_secp_edges.py; tests/pyref/ecies.py takes its curve from here.
"""
P = 2 ** 256 - 2 ** 32 - 977
C = 2 ** 32 + 977                       # 2^256 - p
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
     0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
RN = 2 ** 256 % N                       # the scalar routines' Montgomery radix


# ---------------------------------------------------------------- the group, affine
def pt_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def pt_mul(k, pt):
    acc = None
    while k:
        if k & 1:
            acc = pt_add(acc, pt)
        pt = pt_add(pt, pt)
        k >>= 1
    return acc


def pt_neg(pt):
    return None if pt is None else (pt[0], (P - pt[1]) % P)


def on_curve(pt):
    return pt is None or (0 <= pt[0] < P and 0 <= pt[1] < P and (pt[1] * pt[1] - pt[0] ** 3 - 7) % P == 0)


def lift_x(x):
    """both points with this x (the even y first), or None when x^3 + 7 is no square"""
    y2 = (pow(x, 3, P) + 7) % P
    y = pow(y2, (P + 1) // 4, P)
    if y * y % P != y2:
        return None
    y = y if y % 2 == 0 else P - y
    return (x % P, y), (x % P, P - y)


def compress(pt) -> bytes:
    return bytes([2 | (pt[1] & 1)]) + pt[0].to_bytes(32, "big")


def uncompressed(pt) -> bytes:
    return b"\x04" + pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


def from_jacobian(X, Y, Z):
    """(X, Y, Z) with x = X / Z^2, y = Y / Z^3 (any representatives) -> the affine point, None for Z = 0 mod p"""
    if Z % P == 0:
        return None
    zi = pow(Z, -1, P)
    return X * zi * zi % P, Y * zi * zi * zi % P


def to_jacobian(pt, lam):
    """the form (x lam^2, y lam^3, lam) of an affine point, canonical coordinates"""
    return pt[0] * lam * lam % P, pt[1] * pow(lam, 3, P) % P, lam % P


# ---------------------------------------------------------------- the fields
def fe_sqrt_candidate(a):
    """a^((p + 1) / 4): a square root when one exists"""
    return pow(a, (P + 1) // 4, P)


def sc_mont_mul(a, b):
    """a b R^-1 mod n (operands below n)"""
    return a * b * pow(RN, -1, N) % N


def sc_mont_inv(a):
    """a = x R -> x^-1 R; 0 -> 0"""
    x = a * pow(RN, -1, N) % N
    return pow(x, -1, N) * RN % N if x else 0
