"""Model side of the multilinear tests (msm_amd_fr_mle_bind*, msm_amd_fr_mle_eval*, msm_amd_fr_eq_table*,
msm_amd_fr_sumcheck_round*): Python integers on the record coders of tests/fr_ref.py.  A table is n = 2^m values f[i], the
value at x_j = bit j of i; n_vec tables lie `stride` records apart.  The record forms take records and return records, so
that a test compares bytes.  Nothing here calls the library."""
import random

from fr_ref import CANON_LE, LAYOUTS, MONT_LE, R, decode, encode, first_difference, random_values, raw, words  # noqa: F401

LOW, HIGH = 0, 1                 # MSM_AMD_MLE_*
ORDERS = (LOW, HIGH)
PRODUCT, EQ_AB_C = 0, 1          # MSM_AMD_SUMCHECK_*
SHAPES = ((PRODUCT, 1), (PRODUCT, 2), (PRODUCT, 3), (PRODUCT, 4), (EQ_AB_C, 4))    # (form, tables)
EDGE_WORDS = (0, 1, R - 1, R, R + 1, (1 << 256) - 1)                                # raw words of records and challenges


def degree(form, k):
    return 3 if form == EQ_AB_C else k


def pair(f, order, x):
    """the two values the next step of `order` combines at output index x"""
    return (f[2 * x], f[2 * x + 1]) if order == LOW else (f[x], f[x + len(f) // 2])


def bind_ints(f, order, rs):
    for r in rs:
        f = [(lo + r * (hi - lo)) % R for lo, hi in (pair(f, order, x) for x in range(len(f) // 2))]
    return f


def variable(order, s, m):
    """the variable that step s of `order` binds"""
    return s if order == LOW else m - 1 - s


def eq_ints(point, order):
    m = len(point)
    out = []
    for i in range(1 << m):
        acc = 1
        for s, p in enumerate(point):
            acc = acc * (p if i >> variable(order, s, m) & 1 else 1 - p) % R
        out.append(acc)
    return out


def eq_entry(point, order, i):
    m, acc = len(point), 1
    for s, p in enumerate(point):
        acc = acc * (p if i >> variable(order, s, m) & 1 else 1 - p) % R
    return acc


def evaluate_ints(f, order, point):
    return bind_ints(f, order, point)[0]


def combine(form, vals):
    """F of one value per table"""
    if form == EQ_AB_C:
        e, a, b, c = vals
        return e * (a * b - c) % R
    acc = 1
    for v in vals:
        acc = acc * v % R
    return acc


def round_ints(tabs, order, form):
    """g(0) .. g(d): t goes into every pair as an integer"""
    d, h = degree(form, len(tabs)), len(tabs[0]) // 2
    g = []
    for t in range(d + 1):
        acc = 0
        for x in range(h):
            acc += combine(form, [(lo + t * (hi - lo)) % R for lo, hi in (pair(f, order, x) for f in tabs)])
        g.append(acc % R)
    return g


def total(tabs, form):
    """sum of F over the whole tables: what g(0) + g(1) of the first round must be"""
    return sum(combine(form, [f[i] for f in tabs]) for i in range(len(tabs[0]))) % R


def interpolate(g, r):
    """the polynomial through (t, g[t]), t = 0 .. d, at r (Lagrange)"""
    acc = 0
    for t, y in enumerate(g):
        num = den = 1
        for u in range(len(g)):
            if u != t:
                num = num * (r - u) % R
                den = den * (t - u) % R
        acc = (acc + y * num * pow(den, -1, R)) % R
    return acc


def verifier_step(claim, g, r):
    """one round of the verifier: the check, then the next claim"""
    assert (g[0] + g[1]) % R == claim % R, "g(0) + g(1) differs from the claim"
    return interpolate(g, r)


def prove(tabs, order, form, challenges):
    """the model prover: [(g of round s)], and the tables after every bind"""
    rounds = []
    for r in challenges:
        rounds.append(round_ints(tabs, order, form))
        tabs = [bind_ints(f, order, [r]) for f in tabs]
    return rounds, tabs


# ---- records ---------------------------------------------------------------------------------------------------------------------
def span(n, n_vec, stride):
    return (n_vec - 1) * stride + n if n_vec else 0


def tables(data, layout, n, n_vec, stride=None):
    stride = n if stride is None else stride
    vals = decode(data, layout)
    return [vals[v * stride:v * stride + n] for v in range(n_vec)]


def pack(tabs, layout, stride=None, fill=b"\xEE" * 32):
    """tables -> records `stride` apart, the gaps filled"""
    n = len(tabs[0])
    stride = n if stride is None else stride
    out = b""
    for v, f in enumerate(tabs):
        out += encode(f, layout)
        if v + 1 < len(tabs):
            out += fill * (stride - n)
    return out


def bind(data, r_recs, layout, order, n, n_vec=1, stride=None):
    """the n >> n_bind records of every table"""
    rs = decode(r_recs, layout)
    return [encode(bind_ints(f, order, rs), layout) for f in tables(data, layout, n, n_vec, stride)]


def evaluate(data, point_recs, layout, order, n, n_vec=1, stride=None):
    p = decode(point_recs, layout)
    return encode([evaluate_ints(f, order, p) for f in tables(data, layout, n, n_vec, stride)], layout)


def eq_table(point_recs, layout, order):
    return encode(eq_ints(decode(point_recs, layout), order), layout)


def round_values(data, layout, order, form, n, n_vec, stride=None):
    return encode(round_ints(tables(data, layout, n, n_vec, stride), order, form), layout)


def edge_tables(seed, n, n_vec):
    """raw words: random values with 0, 1, r - 1 and the unreduced words r, r + 1, 2^256 - 1 strewn in"""
    rng = random.Random(seed)
    return [[rng.choice(EDGE_WORDS) if rng.randrange(3) == 0 else rng.randrange(R) for _ in range(n)] for _ in range(n_vec)]


def pack_raw(tabs, stride=None, fill=b"\xEE" * 32):
    n = len(tabs[0])
    stride = n if stride is None else stride
    out = b""
    for v, f in enumerate(tabs):
        out += raw(f)
        if v + 1 < len(tabs):
            out += fill * (stride - n)
    return out


def challenges(seed, count, layout, edge=False):
    """records of `count` challenges; edge: raw edge words among them"""
    rng = random.Random(seed)
    if not edge:
        return encode([rng.randrange(R) for _ in range(count)], layout)
    return raw([rng.choice(EDGE_WORDS) if s % 2 == 0 else rng.randrange(R) for s in range(count)])


def bind_outputs(out, n, n_bind, n_vec, stride):
    """what a bind call defines: the first n >> n_bind records of every output table"""
    return [out[32 * v * stride:32 * (v * stride + (n >> n_bind))] for v in range(n_vec)]


def bind_untouched(out, before, n, n_vec, stride):
    """nothing outside the first n/2 records of every output table may change"""
    for v in range(n_vec):
        lo, hi = 32 * (v * stride + n // 2), 32 * (v + 1) * stride if v + 1 < n_vec else len(out)
        if out[lo:hi] != before[lo:hi]:
            return "bytes behind the first n/2 records of table %d changed" % v
    return None
