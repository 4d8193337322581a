"""Model side of the stage tests of the batch scalar multiplication (msm_amd_test_mul_stage, msm_amd_test_mul_stage_host):
the packed table format, the signed-digit walk over ANY table on the big-integer models with a log of the branches it
takes, tables constructed so that the walk skips identity entries, doubles and sees its sum vanish at chosen windows, and
XYZZ records at the edge of the point invariant for the shared normalisation.  Nothing here calls the library."""
import functools
import itertools
import random
import struct
from fractions import Fraction

import g2_ref as g
import g2_stage_ref as gs
import mul_ref as m
from oracle import fq29_ref as f

FIXED, NORMALISE, NORMALISE_RECORDS = 0, 1, 2               # MSM_AMD_MUL_STAGE_*
CW, W, HALF = 8, 32, 128                                    # asserted against msm_amd_test_mul_plan by the tests
WORDS = {1: 36, 2: 72}                                      # u32 per XYZZ record
K = 16                                                      # records per shared inversion (asserted likewise)


# ---- records -----------------------------------------------------------------------------------------------------------
def packed_entry(group, pt):
    """one table entry: canonical coordinates of the internal Montgomery domain (radix 2^261), 32 little-endian bytes
    each; None -> the identity marker (first coordinate 2^256 - 1, the rest zero)"""
    coords = 2 * group
    if pt is None:
        return b"\xff" * 32 + bytes(32 * (coords - 1))
    flat = pt if group == 1 else (pt[0][0], pt[0][1], pt[1][0], pt[1][1])
    return b"".join((v * f.RHO % f.P).to_bytes(32, "little") for v in flat)


def table_bytes(group, table):
    assert len(table) == W and all(len(row) == HALF for row in table)
    return b"".join(packed_entry(group, e) for row in table for e in row)


def unpack_words(raw, group):
    w = struct.unpack(f"<{len(raw) // 4}I", raw)
    return [list(w[i:i + WORDS[group]]) for i in range(0, len(w), WORDS[group])]


def pack_words(records):
    flat = [x for r in records for x in r]
    return struct.pack(f"<{len(flat)}I", *flat)


def decode_xyzz(group, words):
    """affine point of a raw record (None = identity).  G1: asserts ZZ^3 = ZZZ^2 and the curve as well."""
    return f.decode_point(words) if group == 1 else g.decode_xyzz(words)


def invariant_violations(group, words):
    return f.point_post(words) if group == 1 else gs.xyzz_post(words)


def intermediate_violations(group, words):
    """a record as mul_normalise leaves it -- X ZZZ, ZZ Y, a = ZZ ZZZ, the prefix product in the places of X, Y, ZZ, ZZZ
    -- against the bounds the header of mul_points.hip.h states for a record anywhere inside the invariant, taken from
    the tools that re-derive them (tools/fq29_bounds.py allows the rounding of the header's G1 figures; G2: the figures
    for all components at their maxima at once, MUL_NORM_AT_INV, strict)"""
    lim, slack = (f.FB.MUL_NORM, f.FB.MUL_NORM_SLACK) if group == 1 else (gs.BOUNDS.MUL_NORM_AT_INV, 0.0)
    bad = []
    for i in range(4 * group):
        name, fe = ("X*ZZZ", "ZZ*Y", "a", "pre")[i // group], words[9 * i:9 * i + 9]
        if f.value(fe) >= Fraction(str(lim[name] + slack)) * f.P:
            bad.append(f"{name} component {i % group} = {f.value(fe) / f.P:.3f} p, the header says < {lim[name]} p")
    return bad


# ---- the digit walk on the models -----------------------------------------------------------------------------------------
def digits(s):
    """the signed digits of s < r, least significant window first: a window value above 2^(c-1) becomes v - 2^c with a
    carry into the next window"""
    assert 0 <= s < m.R
    out, carry = [], 0
    for w in range(W):
        v = ((s >> (CW * w)) & ((1 << CW) - 1)) + carry
        carry = 1 if v > HALF else 0
        out.append(v - (1 << CW) if carry else v)
    assert carry == 0 and sum(d << (CW * w) for w, d in enumerate(out)) == s
    return out


def walk(group, table, s):
    """(sum, events) of mul_fixed over `table` (rows of HALF points, None = an identity entry) by affine additions of
    the model.  events: ("identity", w) an identity entry was skipped, ("start", w) the accumulator was (re)started,
    ("double", w) / ("vanish", w) the addition met acc == q / acc == -q."""
    acc, events = None, []
    for w, d in enumerate(digits(s)):
        if d == 0:
            continue
        e = table[w][abs(d) - 1]
        if e is None:
            events.append(("identity", w))
            continue
        q = e if d > 0 else m.neg(group, e)
        if acc is None:
            events.append(("start", w))
        elif acc == q:
            events.append(("double", w))
        elif acc == m.neg(group, q):
            events.append(("vanish", w))
        acc = m.add(group, acc, q)
    return acc, events


def model_table(group, pt):
    """the table the library builds for pt: T[w][d - 1] = [d 2^(8 w)] pt (fresh lists: the caller may replace entries)"""
    return [list(row[1:HALF + 1]) for row in m.multiples(group, pt, CW, W)]


# ---- constructed tables ---------------------------------------------------------------------------------------------------
def _scalar(rng, fixed=(), above=True, top=None):
    """random window values 1 .. 0x7e (positive digits, no carry), `fixed` {window: value} on top; above False: zero
    above the highest fixed window"""
    hi = max(fixed) if fixed else W - 1
    v = [rng.randrange(1, 0x7F) for _ in range(W)]
    v[W - 1] = rng.randrange(1, 0x2F)
    for w, b in dict(fixed).items():
        v[w] = b
    if not above:
        for w in range(hi + 1, W):
            v[w] = 0
    return sum(b << (CW * w) for w, b in enumerate(v))


def _build(group, seed):
    rng = random.Random(seed)
    table = model_table(group, m.random_base(group, 55))
    specials = []                                            # (name, scalar, events the walk must log)

    def partial(s, w):
        """the walk's accumulator of s before window w, on the table as it is now"""
        acc = None
        for j, d in enumerate(digits(s)[:w]):
            if d:
                e = table[j][abs(d) - 1]
                acc = m.add(group, acc, e if d > 0 else m.neg(group, e))
        return acc

    # identity entries at the first non-zero digit, a middle digit and the top digit.  The middle digit is 2^(c-1)
    # itself: the largest value that is NOT negated, so a digit rule that negates it reads the same (identity) entry
    # but carries into the next window
    for name, fixed in (("identity entries", {14: 0x80}), ("identity entries, low windows zero", {0: 0, 1: 0, 2: 0, 14: 0x80}),
                        ("identity entries, middle digit negated", {14: 0xC3})):
        s = _scalar(rng, fixed)
        dg = digits(s)
        first = next(w for w, d in enumerate(dg) if d)
        for w in (first, 14, W - 1):
            table[w][abs(dg[w]) - 1] = None
        specials.append((name, s, [("identity", first), ("identity", 14), ("identity", W - 1)]))
    for negated in (False, True):
        for w in (1, 15, 30 if negated else 31):             # the top window never holds a negated digit (s < r)
            for vanish in (False, True):
                fixed = {w: rng.randrange(0x82, 0xFF)} if negated else {}
                s = _scalar(rng, fixed)
                d = digits(s)[w]
                assert (d < 0) == negated
                p = partial(s, w)
                # the walk adds q = +-entry: q == acc doubles, q == -acc vanishes
                table[w][abs(d) - 1] = p if (d > 0) != vanish else m.neg(group, p)
                name = f"{'vanishing' if vanish else 'doubling'} at window {w}" + (", digit negated" if negated else "")
                want = [("vanish" if vanish else "double", w)]
                if vanish and w < W - 1:
                    want.append(("start", w + 1))             # the walk restarts from the next non-zero digit
                specials.append((name, s, want))
    s = _scalar(rng, {15: rng.randrange(1, 0x7F)}, above=False)
    table[15][digits(s)[15] - 1] = m.neg(group, partial(s, 15))
    specials.append(("vanishing at the last non-zero window", s, [("vanish", 15)]))
    ordinary = [rng.randrange(m.R) for _ in range(130)]
    return table, specials, ordinary


@functools.lru_cache(maxsize=None)
def constructed(group):
    """(table, specials, ordinary scalars, {scalar: (expected point, events)}).  Every special's events are verified on
    the finished table: a later replacement that disturbed an earlier special moves on to the next seed."""
    for seed in itertools.count(900 + group):
        table, specials, ordinary = _build(group, seed)
        expect = {s: walk(group, table, s) for _, s, _ in specials}
        if all(all(ev in expect[s][1] for ev in want) for _, s, want in specials):
            break
    for name, s, want in specials:
        if "vanishing" in name and ("31" in name or "last" in name):
            assert expect[s][0] is None, name                # the identity record
    for s in ordinary:
        expect[s] = walk(group, table, s)
    return table, specials, ordinary, expect


def placements(group):
    """(name, scalars) per call: each special as the only record, at lane 63 of a full wave and at lane 0 of the second
    wave among ordinary scalars; lane counts 1, 63, 64, 65 and 130"""
    _, specials, ordinary, _ = constructed(group)
    calls = []
    for c, (name, s, _) in enumerate(specials):
        calls.append((f"{name}: only record", [s]))
        arr = list(ordinary[:65 if c % 2 else 130])
        arr[63], arr[64] = s, specials[(c + 1) % len(specials)][1]
        calls.append((f"{name}: lane 63, next special at lane 64", arr))
    arr = list(ordinary[:63])
    arr[62], arr[0] = specials[0][1], specials[4][1]
    calls.append(("63 lanes", arr))
    arr = list(ordinary[:64])
    arr[63], arr[31] = specials[5][1], specials[6][1]
    calls.append(("64 lanes", arr))
    return calls


# ---- normalisation at the invariant ---------------------------------------------------------------------------------------
def lift_forms(group):
    """(name, lifts): all coordinates lifted at once, one coordinate at a time, G2: c0 and c1 separately; G1 also the
    two forms of fq29_ref.xyzz whose X / ZZ limbs all sit at the normalised maximum"""
    if group == 1:
        forms = [("all", (True,) * 4)] + [(nm, tuple(i == k for i in range(4))) for k, nm in enumerate(gs.COORDS)]
        return forms + [("all, X limbs at the maximum", "X"), ("all, ZZ limbs at the maximum", "ZZ")]
    forms = [("all", (True,) * 8)] + [(nm, tuple(i // 2 == k for i in range(8))) for k, nm in enumerate(gs.COORDS)]
    return forms + [("c0 of every coordinate", tuple(i % 2 == 0 for i in range(8))),
                    ("c1 of every coordinate", tuple(i % 2 == 1 for i in range(8)))]


def xyzz_record(group, pt, rng, lifts):
    if group == 2:
        return gs.xyzz_lifted(pt, rng, lifts)
    if isinstance(lifts, str):
        return [x for fe in f.xyzz(pt, rng, target=lifts) for x in fe]
    return [x for fe in f.xyzz(pt, rng, lifts=lifts) for x in fe]


def identity_record(group, pt, rng, plain):
    """ZZ (and ZZZ) limbs all zero; plain: X = Y = one as the additions write it, else X and Y of a lifted record"""
    n = WORDS[group] // 2
    if plain:
        one = f.canon(f.RHO % f.P)
        return (one + one if group == 1 else one + [0] * 9 + one + [0] * 9) + [0] * n
    return xyzz_record(group, pt, rng, (True,) * (4 * group))[:n] + [0] * n


IDENTITY_PATTERNS = ("none", "first of each group", "last of each group", "all", "all but one")


def _is_identity(pattern, i, n):
    return {"none": False, "first of each group": i % K == 0, "last of each group": i % K == K - 1 or i == n - 1,
            "all": True, "all but one": i != n // 2}[pattern]


@functools.lru_cache(maxsize=None)
def pool(group):
    return m.random_points(group, 33, 66)


@functools.lru_cache(maxsize=None)
def normalise_cases(group):
    """(name, output layout, records, expected points): groups of 1, 2, 15, 16 records and n = 17, 33 (a second lane, a
    tail group) under every identity pattern, cycling through the lift forms and both layouts; every lift form in a full
    group in both layouts"""
    rng = random.Random(70 + group)
    forms, pts, cases, idx = lift_forms(group), pool(group), [], 0
    plan = [(n, pat, None, None) for n in (1, 2, 15, 16, 17, 33) for pat in IDENTITY_PATTERNS]
    plan += [(K, "none", k, lo) for k in range(len(forms)) for lo in (0, 1)]
    for n, pat, k, lo in plan:
        name, lifts = forms[idx % len(forms) if k is None else k]
        layout = m.OUT_LAYOUTS[group][idx % 2 if lo is None else lo]
        recs, exp = [], []
        for i in range(n):
            ident = _is_identity(pat, i, n)
            recs.append(identity_record(group, pts[i], rng, i % 2 == 0) if ident else xyzz_record(group, pts[i], rng, lifts))
            exp.append(None if ident else pts[i])
        cases.append((f"n = {n}, identities: {pat}, lifted: {name}", layout, recs, exp))
        idx += 1
    return cases


@functools.lru_cache(maxsize=None)
def normalise_placement(group):
    """(records, expected points) of 65 groups: unlifted records everywhere, a maximal-lift group at lane 63 of the first
    wave (records 1008 .. 1023) and at lane 0 of the second (1024 .. 1039), each with one identity inside"""
    rng = random.Random(80 + group)
    pts, none, full = pool(group), (False,) * (4 * group), (True,) * (4 * group)
    recs, exp = [], []
    for i in range(65 * K):
        ident = i in (63 * K + 5, 64 * K)
        lifts = full if i >= 63 * K else none
        recs.append(identity_record(group, pts[i % 33], rng, False) if ident else xyzz_record(group, pts[i % 33], rng, lifts))
        exp.append(None if ident else pts[i % 33])
    return recs, exp
