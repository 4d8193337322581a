"""Model side of the polynomial tests (msm_amd_fr_poly_eval*, msm_amd_fr_poly_div_linear*, msm_amd_fr_lincomb*): Python
integers on the record coders of tests/fr_ref.py.  A polynomial is n coefficients, lowest degree first; n_vec of them lie
back to back.  A model call takes records and returns records, so that a test compares bytes.  Nothing here calls the
library."""
import random

from fr_ref import CANON_LE, LAYOUTS, MONT_LE, R, decode, encode, first_difference, random_values, raw, words  # noqa: F401

# the special points: (name, residue, the raw word to encode -- None: the unique record of the residue)
SPECIAL_POINTS = (
    ("zero", 0, None),
    ("one", 1, None),
    ("minus_one", R - 1, None),
    ("r", 0, R),                                   # the raw word r reads as 0
    ("r_plus_1", 1, R + 1),
    ("all_ones", ((1 << 256) - 1) % R, (1 << 256) - 1),
)


def point_record(value, layout, word=None):
    """the record of a point: of the residue, or the raw word as it stands"""
    return raw([word]) if word is not None else encode([value], layout)


def point_value(rec, layout):
    return decode(rec, layout)[0]


def special_points(layout):
    """(name, record) of every special point and of a random one; a raw word means what the layout makes of it"""
    pts = [(name, point_record(v, layout, w)) for name, v, w in SPECIAL_POINTS]
    pts.append(("random", encode([random.Random(77).randrange(2, R - 1)], layout)))
    return pts


def vectors(data, layout, n_vec):
    vals = decode(data, layout)
    n = len(vals) // n_vec if n_vec else 0
    return [vals[v * n:(v + 1) * n] for v in range(n_vec)]


def eval_ints(coeffs, z):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % R
    return acc


def poly_eval(data, z_rec, layout, n_vec=1):
    """records of p_v(z)"""
    z = point_value(z_rec, layout)
    return encode([eval_ints(p, z) for p in vectors(data, layout, n_vec)], layout)


def div_linear_definition(coeffs, z):
    """from the definition: s_i = sum_{j >= i} c_j z^(j - i); (s_1 .. s_(n-1), 0) and s_0"""
    n = len(coeffs)
    zp = [1] * (n + 1)
    for j in range(1, n + 1):
        zp[j] = zp[j - 1] * z % R
    s = [sum(coeffs[j] * zp[j - i] for j in range(i, n)) % R for i in range(n)]
    return s[1:] + [0], s[0]


def div_linear_horner(coeffs, z):
    """the same by s_i = c_i + z s_(i+1), for sizes where the definition's n^2 / 2 products are too many
    (tests/test_poly_host.py holds the two against each other)"""
    s, run = [0] * (len(coeffs) + 1), 0
    for i in range(len(coeffs) - 1, -1, -1):
        run = (run * z + coeffs[i]) % R
        s[i] = run
    return s[1:], s[0]


def div_linear_ints(coeffs, z):
    return div_linear_definition(coeffs, z) if len(coeffs) <= 600 else div_linear_horner(coeffs, z)


def div_linear(data, z_rec, layout, n_vec=1):
    """(records of the padded quotients, records of the remainders)"""
    z = point_value(z_rec, layout)
    q, rem = [], []
    for p in vectors(data, layout, n_vec):
        qv, rv = div_linear_ints(p, z)
        q += qv
        rem.append(rv)
    return encode(q, layout), encode(rem, layout)


def lincomb(data, k_rec, layout, n_vec=1):
    """records of out[i] = sum_v k^v a_v[i]"""
    k = point_value(k_rec, layout)
    vecs = vectors(data, layout, n_vec)
    n = len(vecs[0]) if vecs else 0
    return encode([sum(pow(k, v, R) * vecs[v][i] for v in range(n_vec)) % R for i in range(n)], layout)
