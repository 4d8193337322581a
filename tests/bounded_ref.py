"""Big-integer model of the bounded-width calls (msm_amd_msm_bounded*, msm_amd_scalar_width*): the magnitude and the
sign fold of a residue, the width of a vector, the signed digits of a (c, bits) plan as the stage tap shows them, scalar
vectors of every pattern the tests use, and expected points from oracle/bn254_ref.py and g2_ref.py over bases with known
discrete logarithms (P_i = (a0 + i d) G: the expected sum is one scalar multiplication)."""
import functools
import random

from oracle import bn254_ref as o

import g2_ref as g

R = o.R_ORDER
HALF = (R - 1) // 2
UNSIGNED, SIGNED = 0, 1
MONT, CANON = 0, 1   # MSM_AMD_SCALAR_MONT_LE, MSM_AMD_SCALAR_CANON_LE
MAX_BITS = {UNSIGNED: 254, SIGNED: 253}


def magnitude(s, sign):
    """(magnitude, negative) of a residue s < r."""
    assert 0 <= s < R
    if sign == SIGNED and s > HALF:
        return R - s, True
    return s, False


def width(words, sign):
    """bits and the stats of a vector of raw 256-bit words (taken mod r): (bits, zeros, negatives, lowest widest index)"""
    bits = zeros = negatives = widest = 0
    for i, w in enumerate(words):
        m, neg = magnitude(w % R, sign)
        zeros += m == 0
        negatives += neg
        if m.bit_length() > bits:
            bits, widest = m.bit_length(), i
    return bits, {"zeros": zeros, "negatives": negatives, "widest": widest}


def fits(words, bits, sign):
    return all(magnitude(w % R, sign)[0] < (1 << bits) for w in words)


def num_windows(c, bits):
    return bits // c + 1


def digits(word, c, bits, sign):
    """The W = bits / c + 1 signed digits of one record: those of the magnitude, negated for a negative record."""
    m, neg = magnitude(word % R, sign)
    assert m < (1 << bits)
    d = o.signed_digits(m, c, num_windows(c, bits))
    assert sum(v << (c * w) for w, v in enumerate(d)) == m   # the top window took the last carry
    return [-v for v in d] if neg else d


def digit_matrix(words, c, bits, sign):
    """MSM_AMD_STAGE_DIGITS of a bounded call: [W][n] words, sign << 15 (c <= 15) or << 31 above, | magnitude"""
    shift = 15 if c <= 15 else 31
    rows = [digits(w, c, bits, sign) for w in words]
    return [[(abs(r[w]) | ((1 << shift) if r[w] < 0 else 0)) for r in rows] for w in range(num_windows(c, bits))]


def encode(words, layout):
    """records of a scalar layout: CANON_LE takes the raw words (they may exceed r), MONT_LE the residues"""
    if layout == CANON:
        return b"".join(w.to_bytes(32, "little") for w in words)
    return b"".join(o.encode_scalar_h2c(w % R) for w in words)


def signed_word(m, negative):
    return (R - m) % R if negative else m


def raw_above_r(s, rng):
    """a 256-bit word >= r with residue s (CANON_LE only)"""
    k = rng.randrange(1, ((1 << 256) - 1 - s) // R + 1)
    return s + k * R


# ---- scalar patterns: each returns n raw words whose magnitudes stay below 2^bits ---------------------------------------
def pattern(name, n, bits, sign, rng, layout=CANON):
    top = (1 << bits) - 1
    if sign == SIGNED and bits == 253:
        top = HALF   # the largest magnitude there is
    neg = (lambda: rng.random() < 0.5) if sign == SIGNED else (lambda: False)
    if name == "max":          # 2^bits - 1 everywhere: a carry through every window into the top one
        ws = [signed_word(top, neg()) for _ in range(n)]
    elif name == "top_bit":    # 2^(bits - 1) everywhere
        ws = [signed_word(1 << (bits - 1), neg()) for _ in range(n)]
    elif name == "random":
        ws = [signed_word(rng.randrange(top + 1), neg()) for _ in range(n)]
    elif name == "zero":
        ws = [0] * n
    elif name == "one_nonzero":
        ws = [0] * n
        ws[rng.randrange(n)] = signed_word(rng.randrange(1, top + 1), neg())
    elif name == "mixed":      # the edges and random records side by side, zeros among them
        edge = [top, 1 << (bits - 1), 1, 0, top - 1 if top > 1 else 1]
        ws = [signed_word(edge[i % len(edge)] if i % 3 == 0 else rng.randrange(top + 1), neg()) for i in range(n)]
    else:
        raise ValueError(name)
    if layout == CANON:        # every fourth record as a raw word >= r with the same residue
        ws = [raw_above_r(w, rng) if i % 4 == 1 else w for i, w in enumerate(ws)]
    assert fits(ws, bits, sign)
    return ws


PATTERNS = ("max", "top_bit", "random", "zero", "one_nonzero", "mixed")


def widths_for(c, sign=UNSIGNED):
    """every relation of the top digit to the window and the word edges of the 256-bit extraction"""
    cand = [1, c - 1, c, c + 1, 2 * c - 1, 2 * c, 31, 32, 33, 63, 64, 65, 127, 128, 253, 254]
    return sorted({b for b in cand if 1 <= b <= MAX_BITS[sign]})


# ---- bases with known discrete logarithms ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g1_progression(n, a0=0x1234567, d=0x9E3779B1):
    """(points as halo2curves affine bytes, discrete logs): P_i = (a0 + i d) G by n - 1 additions in the oracle"""
    step = o.to_jac(o.scalar_mul(d, o.GEN))
    cur = o.to_jac(o.scalar_mul(a0, o.GEN))
    out = []
    for _ in range(n):
        out.append(o.encode_affine_h2c(o.to_affine(cur)))
        cur = o.jac_add(cur, step)
    return b"".join(out), [a0 + i * d for i in range(n)]


def g1_expected(words, dl):
    """sum (w_i mod r) P_i as an affine oracle point (None: the identity)"""
    return o.scalar_mul(sum((w % R) * a for w, a in zip(words, dl)) % R, o.GEN)


def g1_decode(out96):
    return o.decode_jacobian_mont_le(out96)


def g2_expected(words, dl):
    return g.scalar_mul(sum((w % R) * a for w, a in zip(words, dl)) % R, g.GEN2)


def rng_for(*key):
    return random.Random("bounded" + repr(key))
