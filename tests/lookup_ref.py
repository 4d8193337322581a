"""Model side of the lookup tests (msm_amd_fr_lookup_*, msm_amd_fr_prefix_sum*, msm_amd_fr_shift*): Python integers, and
at the end a numpy model of the multiplicities for CANON_LE records below 2^64 (pinned by tests/test_np_models_host.py).
A table is a dict from residue to the smallest row index that holds it; the multiplicities are credited to that row; the
row indices, the report, the running sums and the shift.  A model call takes records and returns records, so that a test
compares bytes.  Nothing here calls the library."""
import random

import numpy as np

from fr_ref import EXCLUSIVE, INCLUSIVE, decode, encode, first_difference, raw, words  # noqa: F401
from ntt_ref import CANON_LE, LAYOUTS, MONT, MONT_LE, R  # noqa: F401

STRICT, COUNT_MISSING = 0, 1                                 # MSM_AMD_LOOKUP_*
NOT_FOUND = 0xFFFFFFFF
NO_MISS = (1 << 64) - 1
EDGE_WORDS = (0, 1, R - 1, R, R + 5, (1 << 256) - 1)          # 256-bit words as they stand in a record
THREADS = 256                                                 # kLookupThreads: rows per workgroup of the insert launch
MANY_ROWS = ((1 << 16) + 1, 1 << 18)                          # tables of tests/test_gpu_many_workgroups.py: 257 and 1024 workgroups
CHAIN_BITS, CHAIN_ROWS = 8, 3 * (1 << 12) + 1                 # MSM_AMD_LOOKUP_HASH_BITS and the table of its long-chain test


def edge_records(layout):
    """records whose WORDS are the edge words: in MONT_LE the word w stands for w / MONT, in CANON_LE for w, both mod r"""
    return raw(EDGE_WORDS)


def representatives(table, layout):
    rep = {}
    for j, v in enumerate(decode(table, layout)):
        rep.setdefault(v, j)
    return rep


def multiplicities(table, data, layout, on_missing=COUNT_MISSING):
    """(m records or None, idx list, report dict): m is None for a miss under STRICT (the call fails and leaves m_out)"""
    rep = representatives(table, layout)
    n_rows = len(table) // 32
    counts = [0] * n_rows
    idx, missing, first = [], 0, NO_MISS
    for i, v in enumerate(decode(data, layout)):
        j = rep.get(v, NOT_FOUND)
        idx.append(j)
        if j == NOT_FOUND:
            missing += 1
            first = min(first, i)
        else:
            counts[j] += 1
    total = len(idx)
    report = dict(n_missing=missing, first_missing=first if total else 0, rows_hit=sum(1 for c in counts if c),
                  max_multiplicity=max(counts))
    m = None if (on_missing == STRICT and missing) else encode(counts, layout)
    return m, idx, report


def n_distinct(table, layout):
    return len(representatives(table, layout))


def prefix_sum(data, layout, mode, n_vec=1):
    vals = decode(data, layout)
    n = len(vals) // n_vec if n_vec else 0
    out = []
    for v in range(n_vec):
        run = 0
        for x in vals[v * n:(v + 1) * n]:
            if mode == EXCLUSIVE:
                out.append(run)
            run = (run + x) % R
            if mode == INCLUSIVE:
                out.append(run)
    return encode(out, layout)


def shift(a, k, layout):
    K = decode(k, layout)[0]
    return encode([x + K for x in decode(a, layout)], layout)


def random_table(seed, n_rows, layout, distinct=None):
    """n_rows records over `distinct` random values (default: all different), in random order"""
    rng = random.Random(seed)
    pool = [rng.randrange(R) for _ in range(distinct or n_rows)]
    vals = pool + [rng.choice(pool) for _ in range(n_rows - len(pool))]
    rng.shuffle(vals)
    return encode(vals, layout)


def draws(seed, table, layout, n, miss_at=()):
    """n records drawn from the rows of a table; the positions in miss_at hold values that are in no row"""
    rng = random.Random(seed)
    rows = decode(table, layout)
    have = set(rows)
    vals = [rng.choice(rows) for _ in range(n)]
    for i in miss_at:
        v = rng.randrange(R)
        while v in have:
            v = rng.randrange(R)
        vals[i] = v
    return encode(vals, layout)


# ---- the numpy model: CANON_LE records of values below 2^64 as (n, 8) uint32 arrays (sort_ref.np_records) -------------------------
def np_representatives(table_vals):
    """(sorted distinct uint64 values, the smallest row index of each)"""
    return np.unique(np.asarray(table_vals, dtype=np.uint64), return_index=True)


def np_multiplicities(table_vals, data_vals):
    """multiplicities() under COUNT_MISSING on uint64 values: (uint32 counters per row, uint32 idx, report dict)"""
    table_vals, data_vals = np.asarray(table_vals, dtype=np.uint64), np.asarray(data_vals, dtype=np.uint64)
    distinct, first = np_representatives(table_vals)
    at = np.minimum(np.searchsorted(distinct, data_vals), distinct.size - 1)
    hit = distinct[at] == data_vals
    idx = np.where(hit, first[at], NOT_FOUND).astype(np.uint32)
    counts = np.bincount(idx[hit], minlength=table_vals.size).astype(np.uint32)
    misses = np.flatnonzero(~hit)
    report = dict(n_missing=int(misses.size), first_missing=(int(misses[0]) if misses.size else NO_MISS) if idx.size else 0,
                  rows_hit=int(np.count_nonzero(counts)), max_multiplicity=int(counts.max()))
    return counts, idx, report


# ---- the hash of the index (csrc/fr_lookup.hip.h), for tests that read a handle's image ------------------------------------------
def _rotl(x, s):
    return ((x << s) | (x >> (32 - s))) & 0xFFFFFFFF


def home(word, capacity, home_bits):
    """the home slot of a reduced Montgomery residue given as a 256-bit integer: MurmurHash3 (x86, 32 bits, seed 0) over its
    eight words, the low home_bits bits of it counted down from the last slot"""
    h = 0
    for w in range(8):
        k = ((word >> (32 * w)) & 0xFFFFFFFF) * 0xCC9E2D51 & 0xFFFFFFFF
        k = _rotl(k, 15) * 0x1B873593 & 0xFFFFFFFF
        h = (_rotl(h ^ k, 13) * 5 + 0xE6546B64) & 0xFFFFFFFF
    h ^= 32
    h = (h ^ (h >> 16)) * 0x85EBCA6B & 0xFFFFFFFF
    h = (h ^ (h >> 13)) * 0xC2B2AE35 & 0xFFFFFFFF
    h ^= h >> 16
    return capacity - 1 - (h & ((1 << min(home_bits, 32)) - 1))


def np_home(rows, capacity, home_bits):
    """home() of every record of an (n, 8) uint32 array, as int64"""
    rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 8)
    u = np.uint32
    h = np.zeros(rows.shape[0], dtype=np.uint32)
    for w in range(8):
        k = rows[:, w] * u(0xCC9E2D51)
        k = ((k << u(15)) | (k >> u(17))) * u(0x1B873593)
        h ^= k
        h = ((h << u(13)) | (h >> u(19))) * u(5) + u(0xE6546B64)
    h ^= u(32)
    h = (h ^ (h >> u(16))) * u(0x85EBCA6B)
    h = (h ^ (h >> u(13))) * u(0xC2B2AE35)
    h ^= h >> u(16)
    return capacity - 1 - (h.astype(np.int64) & ((1 << min(home_bits, 32)) - 1))


def check_slots(slots, rows, rep_of_row, home_bits):
    """what a finished index must be, whatever the order in which its rows arrived.  slots: the uint32 slot words; rows: the
    (n_rows, 8) residues of the image; rep_of_row[j]: the smallest index of row j's class.  Every non-empty slot holds the
    smallest index of its class, every class has exactly one slot, and no empty slot lies between a class's home and its slot
    (upwards, wrapping), so that a probe finds it.  Returns (classes, longest): every member of a class looks at the slots
    from its home to the class's slot, so `longest` is what kLookupLongest must hold."""
    slots = np.asarray(slots, dtype=np.uint32)
    cap = slots.size
    assert cap & (cap - 1) == 0
    used = np.flatnonzero(slots != NOT_FOUND)
    occupant = slots[used].astype(np.int64)
    assert occupant.size and int(occupant.max()) < len(rep_of_row)
    rep_of_row = np.asarray(rep_of_row, dtype=np.int64)
    assert np.array_equal(rep_of_row[occupant], occupant), "a slot holds a row that is not the smallest of its class"
    assert np.array_equal(np.sort(occupant), np.unique(rep_of_row)), "a class has two slots or none"
    start = np_home(np.asarray(rows).reshape(-1, 8)[occupant], cap, home_bits)
    empties = np.concatenate(([0], np.cumsum(slots == NOT_FOUND)))                  # empties[i]: empty slots below i
    between = np.where(start <= used, empties[used] - empties[start], empties[cap] - empties[start] + empties[used])
    assert not between.any(), "an empty slot between a class's home and its slot"
    return int(occupant.size), int(((used - start) & (cap - 1)).max()) + 1


def spread_table(seed, n_rows, r_class_rows=None):
    """(256-bit words of n_rows rows, row indices of the class of 1024).  Rows from n_rows // 2 on repeat the row n_rows // 2
    places before them, so the members of a class sit n_rows // 2 rows apart; one class has 1024 members spread evenly from
    row 17 on; one class stands under the words v, v + r, v + 2r at r_class_rows (default: 0, n_rows // 2, the last row)."""
    rng = random.Random(seed)
    half = n_rows // 2
    words = [rng.randrange(R) for _ in range(half)]
    for i in range(half, n_rows):
        words.append(words[i - half])
    r_class_rows = r_class_rows or (0, half, n_rows - 1)
    stride = (n_rows - 18) // 1027
    many = [i for i in range(17, 17 + 1027 * stride, stride) if i not in r_class_rows][:1024]
    x = rng.randrange(R)
    for i in many:
        words[i] = x
    v = rng.randrange(1 << 200)
    for i, k in zip(r_class_rows, (2, 0, 1)):
        words[i] = v + k * R
    return words, many
