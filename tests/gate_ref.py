"""Model side of the gate-polynomial tests (msm_amd_fr_gate_eval, msm_amd_host_fr_gate_eval): Python integers, Python's %
for the row of a rotated read, and the packing helpers of tests/fr_ref.py and tests/mle_ref.py, which stay as they are.
    v[i]   = sum_k c_k prod_j col_(idx[k][j])[(i + rot[k][j] rot_step) % n]
    out[i] = v[i]   |   k_acc out[i] + v[i]   |   either, times scale[i % period]
The record forms take records and return records, so that a test compares bytes.  Nothing here calls the library."""
import random

import mle_ref as m
from mle_ref import CANON_LE, LAYOUTS, MONT_LE, R  # noqa: F401

MAX_COLUMNS, MAX_TERMS, MAX_FACTORS, MAX_OFFSETS, MAX_PERIOD = 256, 16, 8, 8, 256
ACCUMULATE = 1
INT32_MIN = -(1 << 31)
EDGE_COEFF_WORDS = (0, 1, R - 1, R, (1 << 256) - 1)     # raw words of coefficient records: any 256-bit word is taken mod r


class Gate:
    """terms: [(coefficient, [(column, rotation) or column])]; a coefficient is a value (an int, encoded as its unique
    record) or ("raw", word), the record holding that 256-bit word as it is"""

    def __init__(self, name, n_vec, terms, rot_step=1):
        self.name, self.n_vec, self.rot_step = name, n_vec, rot_step
        self.terms = [(c, [f if isinstance(f, tuple) else (f, 0) for f in fs]) for c, fs in terms]

    def __repr__(self):
        return self.name

    @property
    def degree(self):
        return max(len(f) for _, f in self.terms)

    @property
    def factors(self):
        return sum(len(f) for _, f in self.terms)

    def offsets(self, n):
        """the distinct effective offsets at n rows, in order of first use"""
        seen = []
        for _, fs in self.terms:
            for _, rot in fs:
                off = rot * self.rot_step % n
                if off not in seen:
                    seen.append(off)
        return seen

    def coeff_records(self, layout):
        return [m.raw([c[1]]) if isinstance(c, tuple) else m.encode([c], layout) for c, _ in self.terms]

    def coeff_values(self, layout):
        return [m.decode(rec, layout)[0] for rec in self.coeff_records(layout)]

    def products(self, layout, accumulate=False, scale=False):
        """field products per row: len - 1 per term, one for a coefficient that is neither 1 nor r - 1, one each for
        accumulate and scale"""
        return sum(len(f) - 1 + (c not in (1, R - 1)) for c, (_, f) in zip(self.coeff_values(layout), self.terms)) \
            + bool(accumulate) + bool(scale)

    def lib_terms(self, pkg, layout):
        """the library's view: pkg.GateTerms"""
        return pkg.GateTerms([(rec, f) for rec, (_, f) in zip(self.coeff_records(layout), self.terms)])


def rows_ints(cols, gate, coeffs):
    """v[i] of every row"""
    n = len(cols[0])
    out = []
    for i in range(n):
        acc = 0
        for c, (_, factors) in zip(coeffs, gate.terms):
            p = c
            for col, rot in factors:
                p = p * cols[col][(i + rot * gate.rot_step) % n] % R
            acc += p
        out.append(acc % R)
    return out


def eval_ints(cols, gate, coeffs, old=None, k_acc=None, scale=None):
    v = rows_ints(cols, gate, coeffs)
    if old is not None:
        v = [(k_acc * o + x) % R for o, x in zip(old, v)]
    if scale is not None:
        v = [x * scale[i % len(scale)] % R for i, x in enumerate(v)]
    return v


# ---- records ---------------------------------------------------------------------------------------------------------------------
def evaluate(data, layout, gate, n, stride=None, old=None, k_acc=None, scale=None):
    """the n output records; old (with k_acc): the records accumulated into; scale: the period records"""
    cols = m.tables(data, layout, n, gate.n_vec, stride)
    return m.encode(eval_ints(cols, gate, gate.coeff_values(layout),
                              None if old is None else m.decode(old, layout),
                              None if k_acc is None else m.decode(k_acc, layout)[0],
                              None if scale is None else m.decode(scale, layout)), layout)


def columns(seed, n, n_vec, layout, stride=None, edge=False):
    """n_vec random columns `stride` apart; edge (CANON_LE): raw words, some of them >= r"""
    if edge:
        return m.pack_raw(m.edge_tables(seed, n, n_vec), stride)
    return m.pack([m.random_values(seed + v, n) for v in range(n_vec)], layout, stride)


def records(seed, count, layout):
    return m.encode(m.random_values(seed, count), layout)


# ---- the shapes of the issue -------------------------------------------------------------------------------------------------------
_rng = random.Random(0x6A7E)
COPY = Gate("copy", 1, [(1, [0])])
POWER = Gate("eighth-power", 1, [(7, [0] * 8)])
NEIGHBOURS = Gate("neighbours", 2, [(1, [(0, -1), (1, 1)]), (R - 1, [(1, -1)]), (5, [(0, 1), 0])])   # rows 0 and n - 1 wrap
SIXTEEN = Gate("sixteen-terms", 5, [(("raw", EDGE_COEFF_WORDS[k % 5]) if k < 10 else _rng.randrange(R) if k % 2 else R - 1 if k % 4 else 1,
                                     [(k % 5, k % 3 - 1), ((3 * k + 1) % 5, 0)][:1 + k % 2]) for k in range(16)])
EIGHT_OFFSETS = Gate("eight-offsets", 3, [(1, [(0, 0), (1, 1), (2, 2), (0, 3)]), (R - 1, [(1, -1), (2, -2), (0, -3), (1, 4)]),
                                          (11, [(2, 4), (2, 0)])])
# |rot rot_step| >= n; a rotation that is 0 mod n at n = 1000 (rot_step 8: 125 * 8); INT32_MIN at rot_step 2^40
FAR = Gate("far-rotations", 2, [(1, [(0, 1000), (1, -777)]), (3, [(1, 125), (0, -125)])], rot_step=8)
HUGE = Gate("int32-min", 2, [(1, [(0, INT32_MIN), (1, (1 << 31) - 1)]), (R - 2, [(1, INT32_MIN)])], rot_step=1 << 40)
# q_L a + q_R b + q_M a b - q_O c + q_C over columns q_L, q_R, q_M, q_O, q_C, a, b, c
VANILLA = Gate("vanilla-gate", 8, [(1, [0, 5]), (1, [1, 6]), (1, [2, 5, 6]), (R - 1, [3, 7]), (1, [4])])
GATES = (COPY, POWER, NEIGHBOURS, SIXTEEN, EIGHT_OFFSETS, FAR, HUGE, VANILLA)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000)


def vanilla_next(rot_step):
    """the vanilla gate with c read one row on (the structural test)"""
    return Gate("vanilla-gate-next", 8, [(1, [0, 5]), (1, [1, 6]), (1, [2, 5, 6]), (R - 1, [3, (7, 1)]), (1, [4])], rot_step)


# ---- what every entry point refuses -------------------------------------------------------------------------------------------
def check_errors(pkg):
    """name -> (terms, n_vec, n, rot_step, text of msm_amd_fr_gate_check's refusal)"""
    one = m.encode([1], MONT_LE)
    T = pkg.GateTerms
    good = T([(one, [0, (1, 1)])])

    def broken(field):
        x = T([(one, [0, 1])])
        setattr(x.c, field, None)
        return x

    null = "null pointer in the term list"
    return {
        "null list": (None, 2, 16, 1, "null term list"),
        "n_vec == 0": (good, 0, 16, 1, "n_vec must be 1 .. 256 for a gate"),
        "n_vec == 257": (good, 257, 16, 1, "n_vec must be 1 .. 256 for a gate"),
        "n == 0": (good, 2, 0, 1, "n must be 1 .. 2^32 - 1"),
        "n == 2^32": (good, 2, 1 << 32, 1, "n must be 1 .. 2^32 - 1"),
        "n_terms == 0": (T([]), 2, 16, 1, "n_terms must be 1 .. 16"),
        "n_terms == 17": (T([(one, [0])] * 17), 2, 16, 1, "n_terms must be 1 .. 16"),
        "null coeff": (broken("coeff"), 2, 16, 1, null), "null term_len": (broken("term_len"), 2, 16, 1, null),
        "null factors": (broken("factors"), 2, 16, 1, null), "null rotations": (broken("rotations"), 2, 16, 1, null),
        "rot_step == 0": (good, 2, 16, 0, "rot_step must be at least 1"),
        "term length 0": (T([(one, [0]), (one, [])]), 2, 16, 1, "a term length must be 1 .. 8"),
        "term length 9": (T([(one, [0] * 9)]), 2, 16, 1, "a term length must be 1 .. 8"),
        "index == n_vec": (T([(one, [0, 2])]), 2, 16, 1, "a column index of a term is not below n_vec"),
        "index in a later term": (T([(one, [0]), (one, [1, 0, 5])]), 2, 16, 1, "a column index of a term is not below n_vec"),
        "nine offsets": (T([(one, [(0, r) for r in range(5)]), (one, [(1, r) for r in range(5, 9)])]), 2, 16, 1,
                         "more than MSM_AMD_GATE_MAX_OFFSETS (8) distinct offsets (rot * rot_step) mod n"),
    }
