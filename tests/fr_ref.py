"""Model side of the Fr vector tests (msm_amd_fr_map*, msm_amd_fr_batch_inverse*, msm_amd_fr_prefix_product*): Python
integers only.  The six element-wise ops, the inverse with zeros, the inclusive and exclusive running products per
vector, and the record coders of the two scalar layouts.  A model call takes records and returns records, so that a test
compares bytes.  Nothing here calls the library."""
import random

from ntt_ref import CANON_BE32, CANON_LE, LAYOUTS, MONT, MONT_LE, R

ADD, SUB, MUL, SCALE, AXPY, MULSUB_SCALE = range(6)          # MSM_AMD_FR_*
OPS = (ADD, SUB, MUL, SCALE, AXPY, MULSUB_SCALE)
INCLUSIVE, EXCLUSIVE = 0, 1                                  # MSM_AMD_FR_PREFIX_*
MODES = (INCLUSIVE, EXCLUSIVE)
READS = {ADD: "ab", SUB: "ab", MUL: "ab", SCALE: "ak", AXPY: "abk", MULSUB_SCALE: "abck"}
UNREDUCED = (R, R + 1, (1 << 256) - 1, 2 * R - 1, 5 * R + 7)  # all < 2^256: 2^256 / r < 6
MONT_INV = pow(MONT, -1, R)


def raw(words):
    """records holding these 256-bit integers as they are"""
    return b"".join(w.to_bytes(32, "little") for w in words)


def words(data):
    return [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]


def encode(values, layout):
    """the unique records of these values: fully reduced"""
    return raw([v % R * MONT % R if layout == MONT_LE else v % R for v in values])


def decode(data, layout):
    """the values of any records: a 256-bit word is taken mod r"""
    return [w * MONT_INV % R if layout == MONT_LE else w % R for w in words(data)]


def fr_map(op, layout, a, b=None, c=None, k=None):
    A = decode(a, layout)
    B = decode(b, layout) if "b" in READS[op] else A
    C = decode(c, layout) if "c" in READS[op] else A
    K = decode(k, layout)[0] if "k" in READS[op] else 1
    fn = {ADD: lambda x, y, z: x + y, SUB: lambda x, y, z: x - y, MUL: lambda x, y, z: x * y, SCALE: lambda x, y, z: K * x,
          AXPY: lambda x, y, z: x + K * y, MULSUB_SCALE: lambda x, y, z: K * (x * y - z)}[op]
    return encode([fn(x, y, z) for x, y, z in zip(A, B, C)], layout)


def batch_inverse(data, layout):
    """(records, number of zeros): 0 for 0"""
    vals = decode(data, layout)
    return encode([pow(v, -1, R) if v else 0 for v in vals], layout), sum(1 for v in vals if not v)


def prefix_product(data, layout, mode, n_vec=1):
    vals = decode(data, layout)
    n = len(vals) // n_vec if n_vec else 0
    out = []
    for v in range(n_vec):
        run = 1
        for x in vals[v * n:(v + 1) * n]:
            if mode == EXCLUSIVE:
                out.append(run)
            run = run * x % R
            if mode == INCLUSIVE:
                out.append(run)
    return encode(out, layout)


def random_values(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


def first_difference(got, exp):
    assert len(got) == len(exp), (len(got), len(exp))
    for i in range(0, len(exp), 32):
        if got[i:i + 32] != exp[i:i + 32]:
            return "record %d: %s != %s" % (i // 32, got[i:i + 32].hex(), exp[i:i + 32].hex())
    return None
