"""The bound-limit corpus of the lazy 29-bit Fq12 tower and the pairing steps (csrc/bn254_fq12_29.hip.h): constructed raw
records at the edges of the bounds contract, one builder per raw op of msm_amd_test_fq12_ops, used by the host test
(tests/test_fq12_envelope_host.py) and the GPU test (tests/test_gpu_fq12_envelope.py) alike.  Pure Python, seeded.

corpus(op) returns records (name, class, a_words, b_words, check): 108 words each way, check(out_words) returns None or
what is wrong.  The expected values are computed once per process by the big-integer model pairing_ref on the VALUES of
the raw words (g2.fq2_of), so a record may hold any limbs the contract allows.  double_step / add_step are polynomial
maps: a T that is not on the curve has a defined answer.  So are the Granger-Scott squaring and the x-power chain built
on it (gs_sqr, gs_pow_x below: the header's formulas over Fq2, equal to the plain square and power on the cyclotomic
subgroup, which the host test checks), so the saturated records apply to CYCLO_SQR and POW_X too.

Operand bounds, from the header: elements and T at most 4 p; line coefficients (second operands) below 8 p; Q.x and P
canonical; Q.y at most 4 p.  A random residue r < p leaves room for r + 3 p under 4 p and r + 7 p under 8 p: the "top
multiple" of a non-zero residue is 3 (7 for a line coefficient); a zero can be written as 4 p itself.

Classes:
  saturated      limbs 0..7 = NORM_LIMB_MAX in every component of every operand, limb 8 the largest inside the bound;
                 and the same with limbs 0..7 = 2^29 - 1, which stay saturated when an operand is doubled or tripled
  saturated-one  one component saturated, the rest zero (localises a failure)
  edge-zero      zero written as j p, j = 0 .. 4 (0 .. 7 for line coefficients, and 8 p - 1)
  edge-one       one and minus one at every multiple
  edge-residue   the raw residues 0, 1, p - 1, (p - 1) / 2 in every component at the top multiple
  forms          one value as plain slices, with every borrow taken, and with random borrows
  grid           random residues, every component at its own multiple, every multiple in every position
  sparse         elements of Fq, Fq2, Fq6, a single w^k, line-shaped (w^0, w^1, w^3); zeros written as multiples of p
  cyclo          1, g, g^(r - 1), their conjugates and random cyclotomic elements at every multiple
  inv-shapes     Fq6-only, w-only and generic elements for INV
  zero           INV / FINAL_EXP of zero: the spec is only "returns, the output is an element"
  step-*         curve (T on the curve, random z), z0 (Z = 0), T=Q, T=-Q, negQy (Q.y = 4 p - y), P-edge (a coordinate of
                 P equal to 0 or p - 1)
"""
import functools

import g2_ref as g2
import pairing_ref as pr
from oracle import fq29_ref as f

P, RHO, RHO_INV = pr.P, g2.RHO, g2.RHO_INV
NLM = f.NORM_LIMB_MAX
ELEMENT, SECOND = 4, 8                     # the contract's bounds in multiples of p: elements; second operands (below)
MAX_RECORDS = {pr.FQ12_OP_POW_X: 128}      # every other op: 400
FINAL_EXP_MODEL_CHECKED = 32
HARD_EXPONENT = (P**4 - P**2 + 1) // pr.R_ORDER

OPS = {"fq6_mul": pr.FQ12_OP_FQ6_MUL, "mul": pr.FQ12_OP_MUL, "sqr": pr.FQ12_OP_SQR, "cyclo_sqr": pr.FQ12_OP_CYCLO_SQR,
       "line_mul": pr.FQ12_OP_LINE_MUL, "frob1": pr.FQ12_OP_FROB1, "frob2": pr.FQ12_OP_FROB2, "frob3": pr.FQ12_OP_FROB3,
       "conj": pr.FQ12_OP_CONJ, "inv": pr.FQ12_OP_INV, "pow_x": pr.FQ12_OP_POW_X, "double_step": pr.FQ12_OP_DOUBLE_STEP,
       "add_step": pr.FQ12_OP_ADD_STEP, "final_exp": pr.FQ12_OP_FINAL_EXP}
OP_NAMES = {v: k for k, v in OPS.items()}

_ELEMENT_CLASSES = ("saturated", "saturated-one", "edge-zero", "edge-one", "edge-residue", "forms", "grid", "sparse")
_STEP_CLASSES = _ELEMENT_CLASSES + ("step-curve", "step-z0", "step-P-edge")
# the coverage claim: every (op, class) pair the corpus holds; tests assert that each one is present
CLAIMED = set()
for _op in ("fq6_mul", "mul", "sqr", "line_mul", "frob1", "frob2", "frob3", "conj"):
    CLAIMED |= {(_op, c) for c in _ELEMENT_CLASSES}
CLAIMED |= {("cyclo_sqr", c) for c in _ELEMENT_CLASSES + ("cyclo",)}
CLAIMED |= {("pow_x", c) for c in _ELEMENT_CLASSES + ("cyclo",)}
CLAIMED |= {("inv", c) for c in _ELEMENT_CLASSES + ("inv-shapes", "zero")}
# FINAL_EXP: its edge-zero records are all zero, which is the class "zero" there (INV keeps a neighbour of each in edge-zero)
CLAIMED |= {("final_exp", c) for c in _ELEMENT_CLASSES + ("cyclo", "zero") if c != "edge-zero"}
CLAIMED |= {("double_step", c) for c in _STEP_CLASSES}
CLAIMED |= {("add_step", c) for c in _STEP_CLASSES + ("step-T=Q", "step-T=-Q", "step-negQy")}


# ---- limbs ---------------------------------------------------------------------------------------------------------------
def sat(bound):
    """limbs 0..7 at the normalised maximum, limb 8 the largest that keeps the value at most bound"""
    low = sum(NLM << (29 * i) for i in range(8))
    return [NLM] * 8 + [(bound - low) >> 232]


def sat_mask(bound):
    """limbs 0..7 = 2^29 - 1: k a (fq2_times, k = 2, 3, 6) of such a component has limbs of 2^29 - k .. 2^29 + k again,
    where the doubled NORM_LIMB_MAX wraps to small limbs -- the record that saturates the doubled first operands"""
    return [f.MASK] * 8 + [(bound - ((1 << 232) - 1)) >> 232]


SAT4, SAT8 = sat(ELEMENT * P), sat(SECOND * P - 1)
assert g2.value(SAT4) <= 4 * P < g2.value(SAT4) + (1 << 232) and g2.value(SAT8) < 8 * P <= g2.value(SAT8) + (1 << 232)


def limbs(x):
    """a component is an integer (plain slices) or a limb vector as it is"""
    return list(x) if isinstance(x, (list, tuple)) else g2.limbs_of(x)


def borrowed(v, rng=None):
    """every possible borrow taken (rng: each with probability 1/2): limb i takes 2^29 from limb i + 1 where it stays
    normalised, which needs limb i <= 7"""
    l = g2.limbs_of(v)
    for i in range(8):
        if l[i + 1] > 0 and l[i] + (1 << 29) <= NLM and (rng is None or rng.random() < 0.5):
            l[i] += 1 << 29
            l[i + 1] -= 1
    return l


def small_limbed(rng, bound):
    """a value at most bound whose plain limbs 0..7 are 1 .. 7, so that every borrow is possible"""
    top = rng.randrange(1, (bound >> 232))
    return sum(rng.randrange(1, 8) << (29 * i) for i in range(8)) + (top << 232)


def internal(x):
    return x * RHO % P


def words_w(comps):
    """12 components in the order of the powers of w (c[0].c0, c[0].c1, c[1].c0, ...) -> 108 words in the tower order"""
    pairs = [(comps[2 * i], comps[2 * i + 1]) for i in range(6)]
    out = []
    for c0, c1 in pr._tower_order(pairs):
        out += limbs(c0) + limbs(c1)
    return out


def words_flat(comps, pad=108):
    out = []
    for c in comps:
        out += limbs(c)
    return out + [0] * (pad - len(out))


# ---- component lists: (class, name, components), bound in multiples of p ---------------------------------------------------
def component_sets(n, bound, rng, tag):
    """the record classes over n components at most bound p (bound = 8: below 8 p)"""
    full = SAT4 if bound == ELEMENT else SAT8
    top = bound - 1                                     # the top multiple of a non-zero residue
    out = [("saturated", "all", [full] * n), ("saturated", "all, limbs 2^29 - 1", [sat_mask(bound * P - 1)] * n)]
    out += [("saturated-one", "component %d" % i, [full if k == i else 0 for k in range(n)]) for i in range(n)]
    zero_mults = list(range(bound + 1)) if bound == ELEMENT else list(range(bound))
    out += [("edge-zero", "zero as %d p" % j, [j * P] * n) for j in zero_mults]
    if bound == SECOND:
        out.append(("edge-zero", "8 p - 1", [8 * P - 1] * n))
        out.append(("edge-zero", "8 p - 1, borrows", [borrowed(8 * P - 1)] * n))
    out.append(("edge-zero", "zero, mixed multiples", [zero_mults[(3 * i + 1) % len(zero_mults)] * P for i in range(n)]))
    for j in range(bound):
        z = zero_mults[j % len(zero_mults)] * P
        out.append(("edge-one", "one + %d p" % j, [internal(1) + j * P] + [z] * (n - 1)))
        out.append(("edge-one", "minus one + %d p" % j, [internal(P - 1) + j * P] + [z] * (n - 1)))
    for r in (0, 1, P - 1, (P - 1) // 2):
        out.append(("edge-residue", "residue %s at the top" % {0: "0", 1: "1", P - 1: "p - 1"}.get(r, "(p - 1) / 2"),
                    [r + (bound if r == 0 and bound == ELEMENT else top) * P] * n))
    for k in range(3):
        vals = [small_limbed(rng, bound * P) for _ in range(n)]
        out.append(("forms", "value %d plain" % k, vals))
        out.append(("forms", "value %d every borrow" % k, [borrowed(v) for v in vals]))
        out.append(("forms", "value %d random borrows" % k, [borrowed(v, rng) for v in vals]))
    for k in range(2 * bound):                          # a Latin square of multiples, then a shifted second one
        res = [rng.randrange(1, P) for _ in range(n)]
        out.append(("grid", "multiples (i + %d) mod %d" % (k, bound),
                    [r + ((i * (1 + k // bound) + k) % bound) * P for i, r in enumerate(res)]))
    return [(cls, "%s %s" % (tag, name), comps) for cls, name, comps in out]


def sparse_sets(rng):
    """sparse Fq12 elements in the w order; a zero component is some multiple of p"""
    def fill(keep):
        return [(rng.randrange(1, P) + rng.randrange(4) * P) if i in keep else rng.randrange(5) * P for i in range(12)]
    out = [("sparse", "Fq", fill({0})), ("sparse", "Fq2", fill({0, 1})),
           ("sparse", "Fq6", fill({0, 1, 4, 5, 8, 9})), ("sparse", "line-shaped", fill({0, 1, 2, 3, 6, 7}))]
    out += [("sparse", "w^%d" % k, fill({2 * k, 2 * k + 1})) for k in range(6)]
    return out


@functools.lru_cache(maxsize=None)
def element_sets():
    """(class, name, 12 components in the w order) of the element records every Fq12 op takes"""
    rng = pr.rng_for(0xE12)
    return component_sets(12, ELEMENT, rng, "element") + sparse_sets(rng)


def dense_top(rng, n=12, bound=ELEMENT):
    return [rng.randrange(1, P) + (bound - 1) * P for _ in range(n)]


# ---- the polynomial maps of the cyclotomic squaring ------------------------------------------------------------------------
def gs_sqr(a):
    """fq12_cyclo_sqr as a map on any Fq12 (the header's Granger-Scott formulas); the square on the cyclotomic subgroup"""
    z0, z4, z3, z2, z1, z5 = a[0], a[2], a[4], a[1], a[3], a[5]
    three, two = (3, 0), (2, 0)

    def t(x, y):
        return pr.add2(pr.mul2(x, x), pr.mul2(pr.XI, pr.mul2(y, y))), pr.mul2(two, pr.mul2(x, y))
    t01, t01p = t(z0, z1)
    t23, t23p = t(z2, z3)
    t45, t45p = t(z4, z5)
    r = [None] * 6
    r[0] = pr.sub2(pr.mul2(three, t01), pr.mul2(two, z0))
    r[3] = pr.add2(pr.mul2(three, t01p), pr.mul2(two, z1))
    r[1] = pr.add2(pr.mul2(three, pr.mul2(pr.XI, t45p)), pr.mul2(two, z2))
    r[4] = pr.sub2(pr.mul2(three, t45), pr.mul2(two, z3))
    r[2] = pr.sub2(pr.mul2(three, t23), pr.mul2(two, z4))
    r[5] = pr.add2(pr.mul2(three, t23p), pr.mul2(two, z5))
    return tuple(r)


def gs_pow_x(a):
    """fq12_pow_x as a map on any Fq12: the square-and-multiply chain over gs_sqr"""
    r = a
    for bit in bin(pr.X_BN)[3:]:
        r = gs_sqr(r)
        if bit == "1":
            r = pr.mul12(r, a)
    return r


def final_exp_model(a):
    """a^((p^12 - 1) / r): the easy part by the Frobenius maps (tests/test_pairing_host.py checks that identity against
    the plain power), the hard part as the plain power by (p^4 - p^2 + 1) / r"""
    t = pr.mul12(pr.conj12(a), pr.inv12(a))
    return pr.pow12(pr.mul12(pr.frob12(t, 2), t), HARD_EXPONENT)


# ---- checks ----------------------------------------------------------------------------------------------------------------
def expect_fq12(want):
    def check(w):
        got = pr.fq12_of(w)
        if got != want:
            return "coefficients of w^%s differ from the model" % [i for i in range(6) if got[i] != want[i]]
    return check


def expect_fq2s(want, n_words):
    """want: Fq2 values of the first len(want) 18-word slots; every word from n_words on is zero"""
    def check(w):
        got = [g2.fq2_of(w[18 * k:18 * k + 18]) for k in range(len(want))]
        bad = [k for k in range(len(want)) if got[k] != tuple(want[k])]
        if bad:
            return "Fq2 slots %s differ from the model" % bad
        if any(w[n_words:]):
            return "words behind the result are not zero"
    return check


def twin_only(w):
    """no model: the spec is 'returns, the output is an element' (the tests compare device and twin, and the bounds)"""
    return None


def is_zero12(a):
    return all(c == pr.ZERO2 for c in a)


# ---- the builders ------------------------------------------------------------------------------------------------------------
def cyclo_sets():
    rng = pr.rng_for(0xC7C)
    g = pr.gt_generator()
    gm = pr.pow12(g, pr.R_ORDER - 1)
    named = [("1", pr.ONE12), ("g", g), ("g^(r-1)", gm), ("conj g", pr.conj12(g)), ("conj g^(r-1)", pr.conj12(gm)),
             ("random cyclotomic", pr.rand_cyclotomic(rng))]
    out = []
    for name, v in named:
        flat = [internal(x) for c in v for x in c]
        for j in range(ELEMENT + 1):
            # a non-zero residue goes up to 3 p, a zero component up to 4 p
            out.append(("cyclo", "%s at %d p" % (name, j), [x + (j if x == 0 else min(j, 3)) * P for x in flat]))
        out.append(("cyclo", "%s, mixed multiples" % name,
                    [x + rng.randrange(5 if x == 0 else 4) * P for x in flat]))
    return out


def _unary(model, sets):
    recs = []
    for cls, name, comps in sets:
        a = words_w(comps)
        recs.append((name, cls, a, [0] * 108, expect_fq12(model(pr.fq12_of(a)))))
    return recs


def _build_mul():
    rng = pr.rng_for(0x301)
    sets = element_sets()
    sat_w = words_w(sets[0][2])
    pairs = [("saturated", "saturated x saturated", sat_w, sat_w)]
    for cls, name, comps in sets[1:]:
        w = words_w(comps)
        other = sat_w if cls == "saturated-one" else w if cls == "saturated" else words_w(dense_top(rng))
        pairs.append((cls, name + " x dense", w, other))
        pairs.append((cls, "dense x " + name, other, w))
        if cls in ("edge-zero", "edge-one", "edge-residue", "forms"):
            pairs.append((cls, name + " x itself", w, w))
    return [(name, cls, a, b, expect_fq12(pr.mul12(pr.fq12_of(a), pr.fq12_of(b)))) for cls, name, a, b in pairs]


def _build_fq6_mul():
    rng = pr.rng_for(0x306)
    sets = component_sets(6, ELEMENT, rng, "fq6")
    for cls, name, comps in sparse_sets(rng):            # the even powers of w are the powers of v
        sets.append((cls, name + " (even part)", [comps[4 * k + h] for k in range(3) for h in range(2)]))
    sat_w = words_flat(sets[0][2])
    pairs = [("saturated", "saturated x saturated", sat_w, sat_w)]
    for cls, name, comps in sets[1:]:
        w = words_flat(comps)
        other = sat_w if cls == "saturated-one" else w if cls == "saturated" else words_flat(dense_top(rng, 6))
        pairs += [(cls, name + " x dense", w, other), (cls, "dense x " + name, other, w)]
    recs = []
    for cls, name, a, b in pairs:
        va = tuple(g2.fq2_of(a[18 * k:18 * k + 18]) for k in range(3))
        vb = tuple(g2.fq2_of(b[18 * k:18 * k + 18]) for k in range(3))
        z = pr.ZERO2
        want = pr.mul12((va[0], z, va[1], z, va[2], z), (vb[0], z, vb[1], z, vb[2], z))
        recs.append((name, cls, a, b, expect_fq2s([want[0], want[2], want[4]], 54)))
    return recs


def _build_line_mul():
    rng = pr.rng_for(0x304)
    sets = element_sets()
    lines = component_sets(6, SECOND, rng, "line")
    for k in range(3):                                   # a line with one coefficient only; zeros as multiples of p
        lines.append(("sparse", "line l%d only" % (k if k < 2 else 3),
                      [(rng.randrange(1, P) + 7 * P) if i // 2 == k else rng.randrange(8) * P for i in range(6)]))
    sat_e, sat_l = words_w(sets[0][2]), words_flat(lines[0][2])
    pairs = [("saturated", "saturated x saturated line", sat_e, sat_l)]
    for cls, name, comps in sets[1:]:
        pairs.append((cls, name + " x line", words_w(comps),
                      sat_l if cls == "saturated-one" else words_flat(lines[1][2]) if cls == "saturated" else
                      words_flat(dense_top(rng, 6, SECOND))))
    for cls, name, comps in lines[2:]:
        pairs.append((cls, "element x " + name, sat_e if cls == "saturated-one" else words_w(dense_top(rng)),
                      words_flat(comps)))
    recs = []
    for cls, name, a, b in pairs:
        l = [g2.fq2_of(b[18 * k:18 * k + 18]) for k in range(3)]
        recs.append((name, cls, a, b, expect_fq12(pr.mul12(pr.fq12_of(a), pr.line12(*l)))))
    return recs


def _build_inv():
    rng = pr.rng_for(0x309)
    recs = []
    for cls, name, comps in element_sets():
        a = words_w(comps)
        v = pr.fq12_of(a)
        if is_zero12(v):
            recs.append((name, "zero", a, [0] * 108, twin_only))
            if cls != "edge-zero":
                continue
            # keep the class populated with the smallest non-zero neighbour: the zero plus one in one component
            comps = [comps[0] + 1 if comps[0] < 4 * P else 1] + list(comps[1:])
            a, name = words_w(comps), name + ", plus one"
            v = pr.fq12_of(a)
        recs.append((name, cls, a, [0] * 108, expect_fq12(pr.inv12(v))))
    for k in range(4):
        mult = [rng.randrange(4) for _ in range(12)]
        shapes = (("Fq6-only", {0, 1, 4, 5, 8, 9}), ("w-only", {2, 3, 6, 7, 10, 11}), ("generic", set(range(12))))
        for name, keep in shapes:
            comps = [(rng.randrange(1, P) + mult[i] * P) if i in keep else rng.randrange(5) * P for i in range(12)]
            a = words_w(comps)
            recs.append(("%s %d" % (name, k), "inv-shapes", a, [0] * 108, expect_fq12(pr.inv12(pr.fq12_of(a)))))
    return recs


def _build_final_exp():
    """every element record and the cyclotomic ones; the model on a fixed subset of FINAL_EXP_MODEL_CHECKED: all the
    saturated records, then the first records of every other class in turn"""
    sets = element_sets() + cyclo_sets()
    vals = [pr.fq12_of(words_w(comps)) for _, _, comps in sets]
    chosen = [i for i, s in enumerate(sets) if s[0] in ("saturated", "saturated-one")]
    by_class = {}
    for i, s in enumerate(sets):
        if s[0] not in ("saturated", "saturated-one") and not is_zero12(vals[i]):
            by_class.setdefault(s[0], []).append(i)
    turn = 0
    while len(chosen) < FINAL_EXP_MODEL_CHECKED:
        for ids in by_class.values():
            if turn < len(ids) and len(chosen) < FINAL_EXP_MODEL_CHECKED:
                chosen.append(ids[turn])
        turn += 1
    chosen = set(chosen)
    recs = []
    for i, (cls, name, comps) in enumerate(sets):
        a = words_w(comps)
        if is_zero12(vals[i]):
            recs.append((name, "zero", a, [0] * 108, twin_only))
        elif i in chosen:
            recs.append((name + " [model]", cls, a, [0] * 108, expect_fq12(final_exp_model(vals[i]))))
        else:
            recs.append((name, cls, a, [0] * 108, twin_only))
    return recs


def _t_sets(rng):
    """T = (X, Y, Z): six components at most 4 p"""
    sets = component_sets(6, ELEMENT, rng, "T")
    for k, n in enumerate("XYZ"):
        sets.append(("sparse", "T with %s in Fq only, the rest zero" % n,
                     [(rng.randrange(1, P) + 3 * P) if i == 2 * k else rng.randrange(5) * P for i in range(6)]))
    for k in range(4):                                  # on the curve, a random projective form, every multiple
        t_aff, z = pr.g2_mul(rng.randrange(1, pr.R_ORDER)), g2.rand_fq2(rng)
        T = (pr.mul2(t_aff[0], z), pr.mul2(t_aff[1], z), z)
        sets.append(("step-curve", "T on the curve %d" % k,
                     [internal(x) + ((i + k) % 4) * P for i, x in enumerate(v for c in T for v in c)]))
    for j in range(5):
        sets.append(("step-z0", "Z = 0 as %d p" % j, dense_top(rng, 4) + [j * P, ((j + 2) % 5) * P]))
    return sets


P_MAX = [P - 1, P - 1]


def _p_sets(rng):
    p1 = pr.g1_mul(rng.randrange(1, pr.R_ORDER))
    on = [internal(p1[0]), internal(p1[1])]
    return on, [("step-P-edge", "P.x = 0", [0, on[1]]), ("step-P-edge", "P.y = 0", [on[0], 0]),
                ("step-P-edge", "P.x = p - 1", [P - 1, on[1]]), ("step-P-edge", "P.y = p - 1", [on[0], P - 1]),
                ("step-P-edge", "P = (0, 0)", [0, 0])]


def _step_records(cases, with_q):
    recs = []
    for cls, name, t, q, p in cases:
        a, b = words_flat(list(t) + list(q)), words_flat(p)
        T = tuple(g2.fq2_of(a[18 * k:18 * k + 18]) for k in range(3))
        p1 = tuple(g2.value(b[9 * k:9 * k + 9]) * RHO_INV % P for k in range(2))
        if with_q:
            Q = tuple(g2.fq2_of(a[54 + 18 * k:72 + 18 * k]) for k in range(2))
            T3, line = pr.add_step(T, Q, p1)
        else:
            T3, line = pr.double_step(T, p1)
        recs.append((name, cls, a, b, expect_fq2s(list(T3) + list(line), 108)))
    return recs


def _build_double_step():
    rng = pr.rng_for(0x30B)
    on, p_edges = _p_sets(rng)
    cases = [(cls, name, t, [], P_MAX if cls.startswith("saturated") else on) for cls, name, t in _t_sets(rng)]
    for cls, name, p in p_edges:
        cases.append((cls, name + ", T saturated", [SAT4] * 6, [], p))
        cases.append((cls, name + ", T random", dense_top(rng, 6), [], p))
    return _step_records(cases, False)


def _build_add_step():
    rng = pr.rng_for(0x30C)
    on, p_edges = _p_sets(rng)
    q_sat = [P - 1, P - 1, SAT4, SAT4]                   # Q.x canonical, Q.y at most 4 p

    def q_rand(mult=None):
        q = pr.g2_mul(rng.randrange(1, pr.R_ORDER))
        return [internal(q[0][0]), internal(q[0][1])] + \
               [internal(v) + (rng.randrange(4) if mult is None else mult) * P for v in q[1]]
    cases = []
    for cls, name, t in _t_sets(rng):
        sat_q = cls.startswith("saturated")
        cases.append((cls, name, t, q_sat if sat_q else q_rand(), P_MAX if sat_q else on))
    for cls, name, comps in component_sets(2, ELEMENT, rng, "Q.y"):   # the classes over Q.y, T saturated or random
        q = pr.g2_mul(rng.randrange(1, pr.R_ORDER))
        qx = [P - 1, P - 1] if cls.startswith("saturated") else [internal(q[0][0]), internal(q[0][1])]
        cases.append((cls, name + ", T saturated", [SAT4] * 6, qx + list(comps), P_MAX))
    for cls, name, p in p_edges:
        cases.append((cls, name + ", T and Q.y saturated", [SAT4] * 6, q_sat, p))
        cases.append((cls, name + ", T random", dense_top(rng, 6), q_rand(), p))
    for k in range(4):                                   # Q.y a negation 4 p - y, as the signed digits hand it over
        q = pr.g2_mul(rng.randrange(1, pr.R_ORDER))
        qw = [internal(q[0][0]), internal(q[0][1]), 4 * P - internal(q[1][0]), 4 * P - internal(q[1][1])]
        cases.append(("step-negQy", "Q.y = 4 p - y %d" % k, [SAT4] * 6 if k == 0 else dense_top(rng, 6), qw, on))
    for sign, cls in ((1, "step-T=Q"), (-1, "step-T=-Q")):   # T a projective form of +-Q at every multiple
        for j in range(5):
            q = pr.g2_mul(rng.randrange(1, pr.R_ORDER))
            z = pr.ONE2 if j == 0 else g2.rand_fq2(rng)
            y = q[1] if sign == 1 else pr.neg2(q[1])
            T = (pr.mul2(q[0], z), pr.mul2(y, z), z)
            t = [internal(v) + (min(j, 3) if internal(v) else j) * P for c in T for v in c]
            qw = [internal(q[0][0]), internal(q[0][1])] + [internal(v) + (j % 4) * P for v in q[1]]
            cases.append((cls, "T = %sQ, z %s, multiple %d" % ("-" if sign < 0 else "", "1" if j == 0 else "random", j),
                          t, qw, on))
    return _step_records(cases, True)


@functools.lru_cache(maxsize=None)
def corpus(op):
    """the records of one raw op: a list of (name, class, a_words, b_words, check); built once per process"""
    name = OP_NAMES[op]
    sets = element_sets()
    if name == "mul":
        recs = _build_mul()
    elif name == "fq6_mul":
        recs = _build_fq6_mul()
    elif name == "line_mul":
        recs = _build_line_mul()
    elif name == "sqr":
        recs = _unary(pr.sqr12, sets)
    elif name == "cyclo_sqr":
        recs = _unary(gs_sqr, sets) + _unary(pr.sqr12, cyclo_sets())
    elif name == "pow_x":
        recs = _unary(gs_pow_x, sets) + _unary(lambda v: pr.pow12(v, pr.X_BN), cyclo_sets())
    elif name in ("frob1", "frob2", "frob3"):
        recs = _unary(lambda v: pr.frob12(v, int(name[-1])), sets)
    elif name == "conj":
        recs = _unary(pr.conj12, sets)
    elif name == "inv":
        recs = _build_inv()
    elif name == "final_exp":
        recs = _build_final_exp()
    elif name == "double_step":
        recs = _build_double_step()
    else:
        recs = _build_add_step()
    assert len(recs) <= MAX_RECORDS.get(op, 400), (name, len(recs))
    assert all(len(r[2]) == 108 and len(r[3]) == 108 for r in recs)
    return recs


def flat(recs, which):
    return [w for r in recs for w in r[which]]


def split(words):
    return [words[108 * i:108 * i + 108] for i in range(len(words) // 108)]


# ---- what a figure of tools/fq12_bounds.py governs: (key, components of the output record it bounds) ---------------------
# An output record is twelve 9-limb components.  An Fq12 sits in the tower order: components 0..5 are the coefficients of
# w^0, w^2, w^4, components 6..11 those of w^1, w^3, w^5.  fq12_frob and fq12_conj pass the coefficient of w^0 (conj: every
# even one) through, and 4 p - c of a zero is 4 p: the frob figure governs the other five coefficients, conj has no figure
# of its own and is held to the element bound.  POW_X and FINAL_EXP end in an fq12_mul (x is odd).
ALL = tuple(range(12))
GOVERNS = {
    "fq6_mul": [("fq6_mul", (0, 1, 2, 3, 4, 5))], "mul": [("fq12_mul", ALL)], "sqr": [("fq12_sqr", ALL)],
    "cyclo_sqr": [("cyclo_even", (0, 1, 2, 3, 4, 5)), ("cyclo_odd", (6, 7, 8, 9, 10, 11))],
    "line_mul": [("fq12_mul_line", ALL)],
    "frob1": [("fq12_frob", ALL[2:])], "frob2": [("fq12_frob", ALL[2:])], "frob3": [("fq12_frob", ALL[2:])],
    "conj": [], "inv": [("fq12_inv", ALL)], "pow_x": [("fq12_mul", ALL)], "final_exp": [("fq12_mul", ALL)],
    "double_step": [("step_x", (0, 1)), ("step_y", (2, 3)), ("step_z", (4, 5)), ("line_l0", (6, 7)), ("line_l1", (8, 9)),
                    ("line_l3", (10, 11))],
}
GOVERNS["add_step"] = GOVERNS["double_step"]


def output_failures(op, w):
    """an output is normalised; every component at most 4 p (steps: T' at most 4 p, the lines below 8 p)"""
    comps = [g2.value(w[9 * i:9 * i + 9]) for i in range(12)]
    if not g2.normalised(w, 12):
        return "not normalised"
    step = OP_NAMES[op] in ("double_step", "add_step")
    for i, v in enumerate(comps):
        if v > (8 * P - 1 if step and i >= 6 else 4 * P):
            return "component %d is %.3f p" % (i, v / P)
    return None


def reached(op, outs):
    """{figure key: the largest governed component over outs, in multiples of p}, and the largest of all"""
    top = {key: 0.0 for key, _ in GOVERNS[OP_NAMES[op]]}
    top["largest"] = 0.0
    for w in outs:
        comps = [g2.value(w[9 * i:9 * i + 9]) / P for i in range(12)]
        top["largest"] = max(top["largest"], max(comps))
        for key, idx in GOVERNS[OP_NAMES[op]]:
            top[key] = max(top[key], max(comps[i] for i in idx))
    return top
