"""The numpy models of tests/sort_ref.py, tests/lookup_ref.py and tests/ntt_ref.py against the integer models of the same
modules, on the CPU and in bytes.  The numpy models exist for the columns of tests/test_gpu_many_workgroups.py, which are too
long for Python integers; they take CANON_LE records whose values are below 2^64.  The sizes are those of sort_ref.SIZES,
with and without duplicates."""
import random

import numpy as np
import pytest

import lookup_ref as lr
import ntt_ref as m
import sort_ref as sr

L = sr.CANON_LE


def columns(n):
    rng = random.Random(n)
    yield "below 2^64", [rng.randrange(1 << 64) for _ in range(n)]
    yield "below 2^32", [rng.randrange(1 << 32) for _ in range(n)]
    yield "duplicates", [rng.randrange(max(1, n // 3)) * 0x100000001 for _ in range(n)]
    yield "all equal", [(1 << 64) - 1] * n
    yield "edges", [(0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1)[rng.randrange(5)] for _ in range(n)]


@pytest.mark.parametrize("n", sr.SIZES)
def test_records_and_sort(n):
    for name, vals in columns(n):
        rec = sr.np_records(vals)
        data = sr.encode(vals, L)
        assert rec.tobytes() == data, name
        assert sr.np_values(rec).tolist() == vals and np.array_equal(sr.np_from_bytes(data), rec), name
        exp_out, exp_perm = sr.sort(data, L)
        out, perm = sr.np_sort(rec)
        assert out.dtype == np.uint32 and perm.dtype == np.uint32
        assert out.tobytes() == exp_out and perm.tolist() == exp_perm, name
        assert sr.np_digit_mask(rec) == sr.digit_mask(data, L), name
        sr.np_runs_ascend(rec, perm)
        sr.runs_ascend(data, perm.tolist(), L)


@pytest.mark.parametrize("n", [1, 65, 4097])
def test_sort_of_columns(n):
    cols = [vals for _, vals in columns(n)][:3]
    flat = [x for col in cols for x in col]
    exp_out, exp_perm = sr.sort(sr.encode(flat, L), L, 3)
    out, perm = sr.np_sort(sr.np_records(flat), 3)
    assert out.tobytes() == exp_out and perm.tolist() == exp_perm
    sr.np_runs_ascend(sr.np_records(flat), perm, 3)


def test_runs_ascend_refuses_an_unstable_order():
    rec = sr.np_records([5, 3, 5, 3])
    sr.np_runs_ascend(rec, [1, 3, 0, 2])
    for bad in ([3, 1, 0, 2], [0, 2, 1, 3], [1, 1, 0, 2]):
        with pytest.raises(AssertionError):
            sr.np_runs_ascend(rec, bad)
    with pytest.raises(AssertionError):
        sr.np_values(np.ones((2, 8), dtype=np.uint32))          # a value of 2^64 or more is no input of the model


@pytest.mark.parametrize("n_rows", sr.SIZES)
def test_multiplicities(n_rows):
    rng = random.Random(n_rows)
    for name, rows in columns(n_rows):
        table = sr.encode(rows, L)
        absent = next(v for v in range(7, 1 << 20) if v not in set(rows))
        for n, misses in ((1, ()), (n_rows, ()), (3 * n_rows + 1, ()), (n_rows + 2, (0, n_rows + 1)), (5, (3,))):
            vals = [rng.choice(rows) for _ in range(n)]
            for i in misses:
                vals[i] = absent
            data = sr.encode(vals, L)
            exp_m, exp_idx, exp_rep = lr.multiplicities(table, data, L)
            counts, idx, rep = lr.np_multiplicities(rows, vals)
            assert counts.dtype == np.uint32 and idx.dtype == np.uint32
            assert sr.np_records(counts).tobytes() == exp_m, (name, n)
            assert idx.tolist() == exp_idx and rep == exp_rep, (name, n)
        distinct, first = lr.np_representatives(rows)
        assert dict(zip(distinct.tolist(), first.tolist())) == lr.representatives(table, L), name
        assert distinct.size == lr.n_distinct(table, L)
    counts, idx, rep = lr.np_multiplicities(rows, [])
    assert rep == lr.multiplicities(table, b"", L)[2] and not counts.any() and idx.size == 0


@pytest.mark.parametrize("n", sr.SIZES)
def test_random_records_are_reduced_words(n):
    rec = m.np_random_records(n, n)
    assert rec.shape == (n, 8) and rec.dtype == np.uint32
    words = sr.words(rec.tobytes())
    assert all(w < m.R for w in words) and (n < 64 or len(set(words)) == n)
    assert m.encode(m.decode(rec.tobytes(), m.MONT_LE), m.MONT_LE) == rec.tobytes()      # the unique records of their values
    assert np.array_equal(m.np_random_records(n, n), rec)
    assert m.TOP_WORD_BELOW << 224 <= m.R


def test_home_and_check_slots():
    rng = random.Random(9)
    words = [0, 1, m.R - 1, (1 << 256) - 1] + [rng.randrange(1 << 256) for _ in range(300)]
    rec = sr.np_from_bytes(sr.raw(words))
    for cap, bits in ((2, 32), (1024, 32), (1024, 3), (1024, 0), (1 << 20, 13), (1 << 31, 32)):
        assert lr.np_home(rec, cap, bits).tolist() == [lr.home(w, cap, bits) for w in words], (cap, bits)
    assert lr.home(0, 1 << 31, 0) == (1 << 31) - 1 and {lr.home(w, 1024, 3) for w in words} == set(range(1016, 1024))
    # an index built in row order by the definition, then spoilt in the ways check_slots exists for
    rows, cap, bits = [5, 9, 5, 7, 9, 5], 16, 2
    rec = sr.np_records(rows)
    rep = [rows.index(v) for v in rows]
    slots = np.full(cap, lr.NOT_FOUND, dtype=np.uint32)
    longest = 0
    for j in sorted(set(rep)):
        at, steps = lr.home(rows[j], cap, bits), 1
        while slots[at] != lr.NOT_FOUND:
            at, steps = (at + 1) % cap, steps + 1
        slots[at], longest = j, max(longest, steps)
    assert lr.check_slots(slots, rec, rep, bits) == (3, longest)
    at = int(np.flatnonzero(slots == 1)[0])
    for spoil in ({at: 4}, {at: lr.NOT_FOUND}, {(at + 5) % cap: 1}):
        bad = slots.copy()
        for k, v in spoil.items():
            assert k == at or bad[k] == lr.NOT_FOUND
            bad[k] = v
        with pytest.raises(AssertionError):
            lr.check_slots(bad, rec, rep, bits)


def test_spread_table():
    for n_rows in (65537, 1 << 18):
        words, many = lr.spread_table(1, n_rows)
        rep = {}
        for j, w in enumerate(words):
            rep.setdefault(w % m.R, []).append(j)
        assert abs(len(rep) - n_rows // 2) < 1100 and len(many) == 1024
        assert sorted(len(v) for v in rep.values())[-2:] == [3, 1024]
        for members in rep.values():
            if len(members) != 1024:
                assert all(b - a >= 1 << 15 for a, b in zip(members, members[1:]))
        assert {w // m.R for w in (words[0], words[n_rows // 2], words[-1])} == {0, 1, 2}
