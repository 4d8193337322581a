"""Stage reference of the G2 pipeline in pure Python (on tests/g2_ref.py; no C oracle of G2 exists or is needed).

Every test base is a_i G2 with a known small discrete log, so a bucket, a window partial or a work item is known as an
INTEGER (a signed sum of discrete logs) and becomes a point with one fixed-base multiplication; two points are equal
exactly when their discrete logs agree mod r.

  point_of(s)            s G2 for any integer s, from a byte-window table of G2 (cached)
  expected_buckets       signed sums of discrete logs per slot of a digit matrix, and their points
  expected_partials      bit-k subset sums over the slot index and the window total, the layout of reduce_bits_*
  horner                 the discrete log of the MSM result from the window partials (host_combine_g2)
  replay_items           the state machine of accumulate_g2_kernel on discrete logs, counting STEP_CLASSES
  sort_reference         sorted / bucket_start / bucket_size of a digit matrix on the CPU, any order inside a bucket
  constructed_instance   one-window input that reaches every class of the state machine and both combine kernels
  decode_records         tapped 192-byte Jacobian records -> affine points (None = identity)
  xyzz_lifted, xyzz_post 72-word XYZZ records at the edge of the point invariant, and the invariant as a checker"""
import importlib.util
import os
import random
from fractions import Fraction

import numpy as np

import g2_ref as g

R = g.R_ORDER


def _load_bounds():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "g2_bounds.py")
    spec = importlib.util.spec_from_file_location("g2_bounds", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BOUNDS = _load_bounds()
INV = BOUNDS.INV                 # the point invariant of bn254_ec2_29.hip.h, from the tool that proves it
COORDS = ("X", "Y", "ZZ", "ZZZ")

# ---- s G2 from a byte-window table --------------------------------------------------------------------------------
_ROWS = []     # _ROWS[j][b] = b 256^j G2, b = 0 .. 255 (None for b = 0); rows are built when first needed
_POINTS = {}   # non-negative integer -> point


def _row(j):
    while len(_ROWS) <= j:
        base = g.GEN2 if not _ROWS else g.add(_ROWS[-1][255], _ROWS[-1][1])   # 256^j G2 = (255 + 1) 256^(j-1) G2
        row = [None, base]
        for _ in range(254):
            row.append(g.add(row[-1], base))
        _ROWS.append(row)
    return _ROWS[j]


def point_of(s):
    """s G2 (None = identity) for any integer s: one table entry per non-zero byte of |s|.  s is NOT reduced mod r
    below 2^512, so the table itself is part of what a result that depends on r G2 = O checks."""
    if s < 0:
        return g.neg(point_of(-s))
    if s.bit_length() > 512:
        s %= R
    pt = _POINTS.get(s, False)
    if pt is not False:
        return pt
    acc, v, j = None, s, 0
    while v:
        b = v & 0xFF
        if b:
            acc = g.add(acc, _row(j)[b])
        v >>= 8
        j += 1
    _POINTS[s] = acc
    return acc


def decode_records(raw, which=None):
    """192-byte Jacobian records (the G2 stage tap's BUCKETS / PARTIAL, or a result) -> affine points, None for the
    identity (z all zero).  which: only these record indices (the others stay undecoded: `...`)."""
    count = len(raw) // 192
    assert len(raw) == 192 * count
    out = [...] * count
    for i in (range(count) if which is None else which):
        out[i] = g.decode_jacobian(raw[192 * i:192 * i + 192])
    return out


# ---- buckets and window partials ------------------------------------------------------------------------------------
def expected_buckets(digits, dlogs, lb):
    """digits [W][n] signed (slot = |digit| - 1), dlogs [n] -> (sums, points): per window a dict slot -> the signed
    integer sum of the discrete logs in that slot / its point.  Only slots that hold an entry appear (an entry with
    an identity base, dlog 0, included)."""
    d = np.asarray(digits)
    W, n = d.shape
    assert n == len(dlogs)
    sums = []
    for w in range(W):
        acc = {}
        for i in np.nonzero(d[w])[0]:
            v = int(d[w, i])
            assert abs(v) <= 1 << lb
            acc[abs(v) - 1] = acc.get(abs(v) - 1, 0) + (dlogs[i] if v > 0 else -dlogs[i])
        sums.append(acc)
    return sums, [{s: point_of(v) for s, v in acc.items()} for acc in sums]


def expected_partials(bucket_dlogs, W, lb):
    """bucket_dlogs: expected_buckets' sums -> (dlogs, points), each [W][lb + 1]: entry k < lb is the sum of the slots
    whose index has bit k set, entry lb the sum of all slots of the window."""
    assert len(bucket_dlogs) == W
    dl = []
    for acc in bucket_dlogs:
        row = [0] * (lb + 1)
        for s, v in acc.items():
            assert 0 <= s < 1 << lb
            row[lb] += v
            for k in range(lb):
                if (s >> k) & 1:
                    row[k] += v
        dl.append(row)
    return dl, [[point_of(v) for v in row] for row in dl]


def window_values(bucket_dlogs):
    """sum_s (s + 1) B[w][s] per window, as discrete logs"""
    return [sum((s + 1) * v for s, v in acc.items()) for acc in bucket_dlogs]


def horner(partial_dlogs, c, lb):
    """Discrete log of the MSM result: sum_w 2^(c w) (partial[w][lb] + sum_k 2^k partial[w][k])."""
    return sum((row[lb] + sum(row[k] << k for k in range(lb))) << (c * w) for w, row in enumerate(partial_dlogs))


# ---- the accumulate state machine on discrete logs --------------------------------------------------------------------
# One class per step of an item (a step = one entry of `sorted`); item_identity counts ITEMS whose state ends kEmpty.
STEP_CLASSES = ("identity_skip", "first_point", "one_generic", "one_double", "one_cancel", "many_generic",
                "many_double", "many_cancel", "restart_after_cancel", "item_identity")


def work_items(sorted_u32, bucket_start, bucket_size, n, W, lb, CH):
    """The work items of a plan, bucket by bucket and chunk by chunk: (bucket, chunk, entries of `sorted`)."""
    srt = np.asarray(sorted_u32, dtype=np.uint32).reshape(W, n)
    start = np.asarray(bucket_start, dtype=np.int64).reshape(-1)
    size = np.asarray(bucket_size, dtype=np.int64).reshape(-1)
    for b in np.nonzero(size)[0]:
        w = int(b) >> lb
        row = srt[w, start[b]:start[b] + size[b]]
        for j in range(0, int(size[b]), CH):
            yield int(b), j // CH, [int(e) for e in row[j:j + CH]]


def replay_item_dlog(entries, dlogs):
    """accumulate_g2_kernel's loop over one item on discrete logs mod r -> (class of every step, final dlog or None for
    the identity).  An entry is index | sign << 31; a base with dlog 0 is the identity."""
    EMPTY, ONE, MANY = 0, 1, 2
    state, acc, cancelled, classes = EMPTY, 0, False, []
    for e in entries:
        a = dlogs[e & 0x7FFFFFFF] % R
        if a == 0:
            classes.append("identity_skip")
            continue
        q = (R - a) if e >> 31 else a
        if state == EMPTY:
            classes.append("restart_after_cancel" if cancelled else "first_point")
            state, acc = ONE, q
            continue
        where = "one" if state == ONE else "many"
        if q == acc:
            classes.append(where + "_double")
            state, acc = MANY, 2 * acc % R
        elif (q + acc) % R == 0:
            classes.append(where + "_cancel")
            state, acc, cancelled = EMPTY, 0, True
        else:
            classes.append(where + "_generic")
            state, acc = MANY, (acc + q) % R
    return classes, (None if state == EMPTY else acc)


def replay_items(sorted_u32, bucket_start, bucket_size, n, W, lb, CH, dlogs):
    """Counts per class of STEP_CLASSES over every work item of a plan, in the order the tapped `sorted` gives."""
    counts = dict.fromkeys(STEP_CLASSES, 0)
    for _, _, entries in work_items(sorted_u32, bucket_start, bucket_size, n, W, lb, CH):
        classes, final = replay_item_dlog(entries, dlogs)
        for k in classes:
            counts[k] += 1
        if final is None:
            counts["item_identity"] += 1
    return counts


def sort_reference(digits, lb, rng=None):
    """(sorted [W][n], bucket_start [W][nb], bucket_size [W][nb]) of a digit matrix, as the sort stage leaves them:
    entries index | sign << 31 grouped by slot; inside a slot by index, or shuffled by rng."""
    d = np.asarray(digits)
    W, n = d.shape
    nb = 1 << lb
    srt = np.zeros((W, n), dtype=np.uint32)
    start = np.zeros((W, nb), dtype=np.uint32)
    size = np.zeros((W, nb), dtype=np.uint32)
    for w in range(W):
        slots = [[] for _ in range(nb)]
        for i in np.nonzero(d[w])[0]:
            v = int(d[w, i])
            slots[abs(v) - 1].append(int(i) | ((1 << 31) if v < 0 else 0))
        at = 0
        for s, ent in enumerate(slots):
            if rng is not None:
                rng.shuffle(ent)
            start[w, s], size[w, s] = at, len(ent)
            srt[w, at:at + len(ent)] = ent
            at += len(ent)
    return srt, start, size


# ---- instances ------------------------------------------------------------------------------------------------------
def distinct_dlogs(rng, count, bits=40):
    """distinct non-zero discrete logs below 2^bits"""
    seen = set()
    while len(seen) < count:
        seen.add(rng.randrange(1, 1 << bits))
    out = sorted(seen)
    rng.shuffle(out)
    return out


def encode_points(dlogs):
    """halo2curves G2Affine records of the bases dlog G2 (dlog 0 mod r: the identity, all zero)"""
    return b"".join(g.encode_h2c(point_of(a % R) if a % R else None) for a in dlogs)


CONSTRUCTED_C = 9


def constructed_instance(seed=7):
    """One-window (c = 9) input, the G2 twin of the G1 stage tests' constructed_instance: its buckets reach every class
    of STEP_CLASSES and both combine kernels.  Bucket v holds digit v (scalar v), a `negative` bucket digit -v (scalar
    512 - v, whose carry puts the point into slot 0 of window 1 as well: one large split bucket there).  Classes that
    depend on the order inside a bucket get enough buckets that some order reaches them.  Returns (scalars, dlogs);
    dlog 0 is an identity base, -(a + b) mod r the base -(P + Q)."""
    rng = random.Random(seed)
    pool = distinct_dlogs(rng, 400)
    nxt = iter(pool)
    ks, dl = [], []
    v = iter(range(1, 256))

    def bucket(bases, negative=False):
        val = next(v)
        for a in bases:
            ks.append(512 - val if negative else val)
            dl.append(a % R)

    P = lambda: next(nxt)
    p = P()
    bucket([p, p])                                          # doubling from kOne
    p = P()
    bucket([p, p], negative=True)                           # ... of a negated base (reload keeps the sign)
    p = P()
    bucket([p, p, p, p])                                    # a multiset of one base
    p = P()
    bucket([p, -p])                                         # cancellation from kOne
    for i in range(13):                                     # ... then a restart (in one order of three)
        p, q = P(), P()
        bucket([p, -p, q], negative=i == 0)
    for _ in range(3):
        p, q = P(), P()
        bucket([p, q, -(p + q)])                            # cancellation from kMany, in any order
        p, q, r = P(), P(), P()
        bucket([p, q, -(p + q), r], negative=True)          # ... then a restart (r last)
    for i in range(48):                                     # doubling from kMany in the order (P, P, 2P)
        p = P()
        bucket([p, p, 2 * p], negative=bool(i & 1))
    bucket([0, 0, P()])                                     # identity bases, before a finite base in one order
    bucket([0])                                             # ... and alone
    for size in (15, 16, 17):                               # CH - 1, CH, CH + 1 (CH = 16, asserted by the tests)
        bucket([rng.choice(pool) for _ in range(size)], negative=size == 17)
    bucket([0] * 32)                                        # split bucket whose items are the identity
    p, q = P(), P()
    bucket([p] * 16 + [q, -q] * 8)                          # split bucket: doublings and cancellations mixed
    p = P()
    bucket([p] * 32, negative=True)                         # split bucket, equal item sums: doubling in pt2_add
    p = P()
    bucket([p] * 128)                                       # 8 CH = kSerialItems items: combine_small
    bucket([rng.choice(pool) for _ in range(129)])          # 8 CH + 1: the first deferred bucket (combine_big)
    bucket([rng.choice(pool) for _ in range(1100)], negative=True)   # > 64 items: strided loop + LDS tree
    p = P()
    bucket([p] * 1040)                                      # 65 equal items: doubling inside the LDS tree
    return ks, dl


# ---- XYZZ records at the edge of the invariant ------------------------------------------------------------------------
def xyzz_post(words72):
    """the invariant of a stored / carried G2 point on the raw limbs: every component below INV[coordinate] p, limbs
    0..7 <= 2^29 + 7.  Returns a list of violations."""
    bad = []
    for i in range(8):
        name, fe = COORDS[i // 2], words72[9 * i:9 * i + 9]
        if g.value(fe) >= Fraction(str(INV[name])) * g.P:
            bad.append(f"{name}.c{i % 2} = {g.value(fe) / g.P:.3f} p, the invariant says < {INV[name]} p")
        if max(fe[:8]) > g.f.NORM_LIMB_MAX:
            bad.append(f"{name}.c{i % 2} has a limb {max(fe[:8]):#x} above 2^29 + 7")
    return bad


def xyzz_lifted(pt, rng, lifts=(True,) * 8):
    """72 words of the affine point pt with a random Z.  Component i of (X.c0, X.c1, Y.c0, ..., ZZZ.c1) with lifts[i]
    set carries the largest multiple of p that keeps it below its bound, in the limb form that borrows from the upper
    limbs (limbs 0..7 up to 2^29 + 7); the others are canonical.  X < 1.21 p has room for one p only above a residue
    below 0.21 p, so Z is drawn until every lifted component of X has such a residue."""
    room = (Fraction(str(INV["X"])) - 1) * g.P
    while True:
        z = g.rand_fq2(rng)
        zz = g.mul2(z, z)
        zzz = g.mul2(zz, z)
        comps = [v * g.RHO % g.P for c in (g.mul2(pt[0], zz), g.mul2(pt[1], zzz), zz, zzz) for v in c]
        if zz != g.ZERO2 and all(comps[i] < room for i in (0, 1) if lifts[i]):
            break
    out = []
    for i, v in enumerate(comps):
        out += g.f.borrowed(g.f.lift(v, INV[COORDS[i // 2]])) if lifts[i] else g.limbs_of(v)
    return out
