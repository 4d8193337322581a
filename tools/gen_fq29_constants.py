"""Generates the constants of csrc/bn254_fq29.hip.h (29-bit-limb internal field representation).

Internal Montgomery radix rho = 2^261 (9 limbs x 29 bits).  External representation (what the host
libraries and the reference use) is Montgomery with R = 2^256 on 8 x 32-bit limbs.
"""
P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
B, L = 29, 9
M = (1 << B) - 1
RHO = 1 << (B * L)


def limbs(x):
    out = [(x >> (B * i)) & M for i in range(L - 1)]
    out.append(x >> (B * (L - 1)))
    return out


def fmt(name, arr, comment=""):
    return f"  // {comment}\n  {name} = {{" + ", ".join(f"0x{v:08X}u" for v in arr) + "};"


def lifted(k, e):
    c = limbs(k * P)
    bor = 1 << (e - B)
    out = [c[0] + (1 << e)] + [c[i] + (1 << e) - bor for i in range(1, L - 1)] + [c[L - 1] - bor]
    assert sum(v << (B * i) for i, v in enumerate(out)) == k * P
    assert all(0 <= v < (1 << 32) for v in out)
    return out


print("P29      ", [hex(v) for v in limbs(P)])
print("INV29     0x%08X   (-p^-1 mod 2^29)" % ((-pow(P, -1, 1 << B)) % (1 << B)))
print("PINV29    0x%08X   ( p^-1 mod 2^29)" % (pow(P, -1, 1 << B)))

def friendly(t):
    """INVF = INV29 + t 2^29 and NPP = (INVF p + 1) / 2^29: N = INVF p is a multiple of p that is -1 modulo 2^29, so a
    quotient digit m reduces column k by A[k] + m N = (A[k] - m) + 2^29 (m NPP) with m the column's own low bits -- no
    multiplication by INV29 (Fq29::reduce_columns, digits 0..6).  NPP must fit 9 limbs like p."""
    invf = INV29 + (t << B)
    assert (invf * P + 1) % (1 << B) == 0
    npp = (invf * P + 1) >> B
    return invf, limbs(npp)


INV29 = (-pow(P, -1, 1 << B)) % (1 << B)
# the t whose NPP has the smallest limb sum: the Montgomery terms of a column are digit * NPP_j, and their sum is what the
# 64-bit columns have to hold (tools/fq29_bounds.py).  t < 64 keeps INVF below 2^35 and NPP inside 9 limbs of 29 bits.
T_BEST = min(range(64), key=lambda t: sum(friendly(t)[1]))
INVF, NPP = friendly(T_BEST)
assert all(v <= M for v in NPP) and sum(v << (B * i) for i, v in enumerate(NPP)) == (INVF * P + 1) >> B
print("INVF      0x%08X   (INV29 + %d * 2^29; N = INVF p = -1 mod 2^29)" % (INVF, T_BEST))
print("NPP      ", [hex(v) for v in NPP], " (INVF p + 1) / 2^29; limb sum %d = 2^%.2f (p: %d = 2^%.2f; t = 0: %d)"
      % (sum(NPP), __import__("math").log2(sum(NPP)), sum(limbs(P)), __import__("math").log2(sum(limbs(P))),
         sum(friendly(0)[1])))
print("ONE29    ", [hex(v) for v in limbs(RHO % P)], " rho mod p (internal one)")
print("C_IN     ", [hex(v) for v in limbs(pow(2, 2 * B * L - 256, P))], " 2^(2*261-256) mod p: ext -> int")
print("D_OUT    ", [hex(v) for v in limbs(pow(2, 256, P))], " 2^256 mod p: int -> ext")
for k, e in ((4, 30), (8, 30), (8, 31), (16, 30), (16, 31), (12, 30)):
    print(f"K{k}E{e}  ", [hex(v) for v in lifted(k, e)], f" top-limb headroom {limbs(k*P)[8] - (1 << (e-B))}")
print("p/rho =", P / RHO, " p>>232 =", P >> 232, hex(P >> 232))
