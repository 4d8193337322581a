"""Model side of the term-list sumcheck tests (msm_amd_fr_sumcheck_round_terms*, msm_amd_fr_sumcheck_step_terms*): Python
integers on the table helpers of tests/mle_ref.py, which stays as it is.  A form is F = [f_outer] sum_k c_k prod_j
f_(factors[k][j]); the model gives F at one value per table, the round values g(0) .. g(d) and the step, which is by
definition one bind followed by the round over the bound tables.  The record forms take records and return records, so that
a test compares bytes.  Nothing here calls the library."""
import mle_ref as m
from mle_ref import HIGH, LAYOUTS, LOW, ORDERS, R  # noqa: F401

MAX_TABLES, MAX_TERMS, MAX_FACTORS = 16, 16, 6
EDGE_COEFF_WORDS = (0, 1, R - 1, R, (1 << 256) - 1)     # raw words of coefficient records: any 256-bit word is taken mod r


class Form:
    """terms: [(coefficient, [table indices])]; a coefficient is a value (an int, encoded as its unique record) or
    ("raw", word), the record holding that 256-bit word as it is; outer: a table index or None"""

    def __init__(self, name, n_vec, terms, outer=None):
        self.name, self.n_vec, self.terms, self.outer = name, n_vec, terms, outer

    def __repr__(self):
        return self.name

    @property
    def degree(self):
        return max(len(f) for _, f in self.terms) + (self.outer is not None)

    def coeff_records(self, layout):
        return [m.raw([c[1]]) if isinstance(c, tuple) else m.encode([c], layout) for c, _ in self.terms]

    def coeff_values(self, layout):
        return [m.decode(rec, layout)[0] for rec in self.coeff_records(layout)]

    def lib_terms(self, pkg, layout):
        """the library's view: pkg.SumcheckTerms"""
        return pkg.SumcheckTerms([(rec, f) for rec, (_, f) in zip(self.coeff_records(layout), self.terms)], self.outer)


def product(k):
    """the list that spells MSM_AMD_SUMCHECK_PRODUCT of k tables"""
    return Form("product-%d" % k, k, [(1, list(range(k)))])


EQ_AB_C = Form("eq-ab-c", 4, [(1, [1, 2]), (R - 1, [3])], outer=0)
# HyperPlonk's vanilla gate under eq: tables eq, q_L, q_R, q_M, q_O, q_C, w_1, w_2, w_3
VANILLA = Form("vanilla-gate", 9, [(1, [1, 6]), (1, [2, 7]), (1, [3, 6, 7]), (R - 1, [4, 8]), (1, [5])], outer=0)
GKR = Form("gkr-layer", 5, [(1, [1, 3]), (1, [1, 4]), (1, [2, 3, 4])], outer=0)       # eq (add (l + r) + mul l r)
# the shapes of the issue: every path of the body, and the edge coefficient words
FORMS = (
    Form("one-factor", 1, [(("raw", R), [0])]),                                         # coefficient word r: zero
    Form("one-factor-any", 2, [(12345, [1])]),
    Form("sixth-power", 1, [(7, [0] * 6)]),
    Form("sixteen-terms", 16, [(("raw", EDGE_COEFF_WORDS[k % 5]) if k < 10 else k * k + 1 if k % 2 else R - 1 if k % 4 else 1,
                                [k, (5 * k + 3) % 16][:1 + k % 2]) for k in range(16)]),
    Form("shared-table", 3, [(1, [0, 1]), (R - 1, [0, 2]), (("raw", (1 << 256) - 1), [0, 0, 1]), (0, [2])]),
    Form("outer-inside", 3, [(3, [0, 1]), (1, [2]), (R - 2, [0, 0])], outer=0),
    Form("degree-7", 4, [(R - 1, [0, 1, 2, 3, 1, 0]), (("raw", 1), [2])], outer=3),
    Form("degree-5", 3, [(1, [0, 1, 2, 2, 1]), (9, [1, 1])]),
    Form("degree-6-outer", 3, [(1, [0, 1, 2, 2, 1]), (R - 1, [1])], outer=2),
    product(1), product(2), product(3), product(4), EQ_AB_C, VANILLA, GKR,
)


def combine(form, coeffs, vals):
    """F of one value per table"""
    acc = 0
    for c, (_, factors) in zip(coeffs, form.terms):
        p = c
        for j in factors:
            p = p * vals[j] % R
        acc += p
    if form.outer is not None:
        acc *= vals[form.outer]
    return acc % R


def round_ints(tabs, order, form, coeffs):
    """g(0) .. g(d): t goes into every pair as an integer"""
    h = len(tabs[0]) // 2
    g = []
    for t in range(form.degree + 1):
        acc = 0
        for x in range(h):
            acc += combine(form, coeffs, [(lo + t * (hi - lo)) % R for lo, hi in (m.pair(f, order, x) for f in tabs)])
        g.append(acc % R)
    return g


def step_ints(tabs, order, r, form, coeffs):
    """the bound tables, and their round values"""
    bound = [m.bind_ints(f, order, [r]) for f in tabs]
    return bound, round_ints(bound, order, form, coeffs)


def total(tabs, form, coeffs):
    """the sum of F over the whole tables: what g(0) + g(1) of the first round must be"""
    return sum(combine(form, coeffs, [f[i] for f in tabs]) for i in range(len(tabs[0]))) % R


# ---- records ---------------------------------------------------------------------------------------------------------------------
def round_values(data, layout, order, form, n, stride=None):
    return m.encode(round_ints(m.tables(data, layout, n, form.n_vec, stride), order, form, form.coeff_values(layout)), layout)


def step(data, r_rec, layout, order, form, n, stride=None):
    """([the n / 2 records of every output table], the d + 1 records)"""
    bound, g = step_ints(m.tables(data, layout, n, form.n_vec, stride), order, m.decode(r_rec, layout)[0], form,
                         form.coeff_values(layout))
    return [m.encode(f, layout) for f in bound], m.encode(g, layout)


def round_plan(n, values, chunk_log, fold_log=10):
    """the closed form of the round plan: one wave per 2^min(C, log2 h) pairs, then folds of 2^10 partials per t"""
    h_log = n.bit_length() - 2
    count = 1 << (h_log - min(chunk_log, h_log))
    first = waves = count
    records, levels = count * values, 1
    while count > 1:
        count = (count + (1 << fold_log) - 1) >> fold_log
        waves += count * values
        records += count * values
        levels += 1
    return {"launches": levels, "waves": waves, "records": records, "bytes": 32 * records, "levels": levels,
            "first_waves": first, "values": values}


# ---- what every call refuses ---------------------------------------------------------------------------------------------------
def error_cases(pkg):
    """name -> (terms, n, n_vec, stride, order, layout): each is refused by the round and by the step"""
    one = m.encode([1], m.MONT_LE)
    T = pkg.SumcheckTerms
    n = 16
    good = T([(one, [0, 1])])

    def broken(field):
        x = T([(one, [0, 1])])
        setattr(x.c, field, None)
        return x

    many = T([(one, [0])] * 17)
    return {
        "n_terms == 0": (T([]), n, 2, n, 0, 0), "n_terms == 17": (many, n, 2, n, 0, 0),
        "term length 0": (T([(one, [0]), (one, [])]), n, 2, n, 0, 0),
        "term length 7": (T([(one, [0] * 7)]), n, 2, n, 0, 0),
        "index == n_vec": (T([(one, [0, 2])]), n, 2, n, 0, 0),
        "index in a later term": (T([(one, [0]), (one, [1, 0, 5])]), n, 2, n, 0, 0),
        "outer == n_vec": (T([(one, [0])], outer=2), n, 2, n, 0, 0),
        "n_vec == 17": (good, n, 17, n, 0, 0),
        "null list": (None, n, 2, n, 0, 0),
        "null coeff": (broken("coeff"), n, 2, n, 0, 0), "null term_len": (broken("term_len"), n, 2, n, 0, 0),
        "null factors": (broken("factors"), n, 2, n, 0, 0),
        "layout BE32": (good, n, 2, n, 0, pkg.SCALAR_CANON_BE32), "layout 7": (good, n, 2, n, 0, 7),
        "order 2": (good, n, 2, n, 2, 0), "order -1": (good, n, 2, n, -1, 0),
        "n == 12": (good, 12, 2, 12, 0, 0), "n == 1": (good, 1, 2, 1, 0, 0), "n == 0": (good, 0, 2, 0, 0, 0),
        "n == 2^32": (good, 1 << 32, 2, 1 << 32, 0, 0),
        "stride < n": (good, n, 2, n - 1, 0, 0), "n_vec stride >= 2^32": (good, n, 2, 1 << 31, 0, 0),
    }
