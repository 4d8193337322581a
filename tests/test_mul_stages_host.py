"""Host tests (no GPU) of the stage entry msm_amd_test_mul_stage_host: the signed-digit walk of mul_points.hip.h over
tables the test wrote (identity entries, an entry equal to the partial sum or to its negative, at a plain and at a
negated digit, on every wave position that matters on the GPU) and the shared normalisation on XYZZ records at the edge
of the point invariant.  Expected values come from mul_stage_ref (the big-integer models); every input record is
checked against the invariant before the library sees it, so a failure is a finding about the library."""
import ctypes

import pytest

import mul_ref as m
import mul_stage_ref as sr

GROUPS = [1, 2]


def host_run(msm_pkg):
    return msm_pkg.test_mul_stage_host


def test_constants_symbols_and_the_model_table(msm_pkg):
    L = msm_pkg.lib()
    for name in ("msm_amd_test_mul_stage", "msm_amd_test_mul_stage_host"):
        assert hasattr(L, name) and name in msm_pkg.EXPORTS
    assert (msm_pkg.MUL_STAGE_FIXED, msm_pkg.MUL_STAGE_NORMALISE, msm_pkg.MUL_STAGE_NORMALISE_RECORDS) == (
        sr.FIXED, sr.NORMALISE, sr.NORMALISE_RECORDS)
    for group in GROUPS:
        plan = msm_pkg.mul_plan(group)
        assert (plan["c"], plan["W"], plan["entries"], plan["K"]) == (sr.CW, sr.W, sr.W * sr.HALF, sr.K)
        assert msm_pkg.MUL_XYZZ_WORDS[group] == sr.WORDS[group]


def check_fixed_on_the_model_table(run, group):
    """the untouched model table under the stage entry gives what the public call gives: ties the table format down"""
    base = m.random_base(group, 55)
    tb = sr.table_bytes(group, sr.model_table(group, base))
    ks, names = m.planted_scalars(sr.CW, sr.W)
    exp = [m.from_rows(group, m.multiples(group, base, sr.CW, sr.W), k) for k in ks]
    for sl in m.SCALAR_LAYOUTS:
        raw = run(group, sr.FIXED, sl, m.scalars_bytes(ks, sl), tb, len(ks))
        for i, words in enumerate(sr.unpack_words(raw, group)):
            assert sr.decode_xyzz(group, words) == exp[i], (names[i], sl)
            assert not sr.invariant_violations(group, words), names[i]


def check_constructed_tables(run, group):
    table, specials, _, expect = sr.constructed(group)
    tb = sr.table_bytes(group, table)
    for name, ks in sr.placements(group):
        raw = run(group, sr.FIXED, 1, m.scalars_bytes(ks, 1), tb, len(ks))
        recs = sr.unpack_words(raw, group)
        assert len(recs) == len(ks)
        for i, (s, words) in enumerate(zip(ks, recs)):
            assert sr.decode_xyzz(group, words) == expect[s][0], (name, i, expect[s][1])
            assert not sr.invariant_violations(group, words), (name, i)
    return len(specials)


def check_normalise(run, group):
    for name, layout, recs, exp in sr.normalise_cases(group):
        for i, r in enumerate(recs):
            assert not sr.invariant_violations(group, r), (name, i)          # never an out-of-contract input
        data = sr.pack_words(recs)
        got = run(group, sr.NORMALISE, layout, data, None, len(recs))
        size = m.OUT_BYTES[(group, layout)]
        for i, pt in enumerate(exp):
            assert got[i * size:(i + 1) * size] == m.out_record(group, layout, pt), (name, i)
        # what the stage left in its copy of the records: the numerators, a_i and the prefix products inside the bounds
        # the header states (ZZ Y with Y as the second operand; the other order passes every output check above)
        left = sr.unpack_words(run(group, sr.NORMALISE_RECORDS, layout, data, None, len(recs)), group)
        for i, words in enumerate(left):
            assert not sr.intermediate_violations(group, words), (name, i)
            half = sr.WORDS[group] // 2
            assert (words[:half] == [0] * half) == (exp[i] is None), (name, i)      # an identity: exact zero numerators


def check_normalise_placement(run, group):
    recs, exp = sr.normalise_placement(group)
    for i, r in enumerate(recs):
        assert not sr.invariant_violations(group, r), i
    data = sr.pack_words(recs)
    for layout in m.OUT_LAYOUTS[group]:
        got = run(group, sr.NORMALISE, layout, data, None, len(recs))
        size = m.OUT_BYTES[(group, layout)]
        want = b"".join(m.out_record(group, layout, pt) for pt in exp)
        assert len(got) == len(want)
        for i in range(len(exp)):
            assert got[i * size:(i + 1) * size] == want[i * size:(i + 1) * size], i


@pytest.mark.parametrize("group", GROUPS)
def test_fixed_on_the_model_table(msm_pkg, group):
    check_fixed_on_the_model_table(host_run(msm_pkg), group)


@pytest.mark.parametrize("group", GROUPS)
def test_constructed_tables(msm_pkg, group):
    """identity entries, doubling and vanishing at windows 1, 15, 31 (30 for a negated digit), vanishing at the last
    window: each as the only record, at lane 63 and at lane 64 among ordinary scalars; the raw records decode to the
    model's sum and satisfy the point invariant"""
    assert check_constructed_tables(host_run(msm_pkg), group) == 16


@pytest.mark.parametrize("group", GROUPS)
def test_the_constructed_tables_reach_their_branches(group):
    """the model's own log: every special takes the branch it was built for, and a vanished sum at the last window is the
    identity"""
    _, specials, _, expect = sr.constructed(group)
    seen = set()
    for name, s, want in specials:
        pt, events = expect[s]
        assert all(ev in events for ev in want), (name, events)
        seen |= {kind for kind, _ in events}
        if want == [("vanish", 31)] or "last" in name:
            assert pt is None
    assert seen == {"identity", "start", "double", "vanish"}
    negated = [sr.digits(s)[want[0][1]] for name, s, want in specials if ", digit negated" in name]
    assert len(negated) == 6 and all(d < 0 for d in negated)
    middle = {name: sr.digits(s)[14] for name, s, _ in specials if name.startswith("identity entries")}
    assert sorted(middle.values()) == [0xC3 - 256, 128, 128]


@pytest.mark.parametrize("group", GROUPS)
def test_normalise_at_the_invariant(msm_pkg, group):
    check_normalise(host_run(msm_pkg), group)


@pytest.mark.parametrize("group", GROUPS)
def test_normalise_maximal_groups_on_lanes_63_and_64(msm_pkg, group):
    check_normalise_placement(host_run(msm_pkg), group)


@pytest.mark.parametrize("group", GROUPS)
def test_normalise_does_not_write_its_input(msm_pkg, group):
    recs, _ = sr.normalise_placement(group)
    data = ctypes.create_string_buffer(sr.pack_words(recs[:33]))
    before = data.raw
    msm_pkg.test_mul_stage_host(group, sr.NORMALISE, 0, data, None, 33)
    assert data.raw == before


def test_argument_errors(msm_pkg):
    L, IE, OK = msm_pkg.lib(), msm_pkg.INPUT_ERROR, msm_pkg.OK
    fn = L.msm_amd_test_mul_stage_host
    sc, tb = ctypes.create_string_buffer(32 * 4), ctypes.create_string_buffer(4096 * 128)
    recs, out = ctypes.create_string_buffer(288 * 4), ctypes.create_string_buffer(288 * 4)
    for group in GROUPS:
        assert fn(group, sr.FIXED, 1, sc, tb, 4, out) == OK
        assert fn(group, sr.NORMALISE, 0, recs, None, 4, out) == OK
        assert fn(group, sr.NORMALISE_RECORDS, 0, recs, None, 4, out) == OK
        assert fn(group, sr.NORMALISE_RECORDS, 9, recs, None, 4, out) == IE
        for which in (3, -1):
            assert fn(group, which, 0, sc, tb, 4, out) == IE
        for sl in (3, -1):
            assert fn(group, sr.FIXED, sl, sc, tb, 4, out) == IE
        for lo in (9, -1, msm_pkg.G2_POINT_PREPARED if group == 2 else msm_pkg.POINT_PREPARED):
            assert fn(group, sr.NORMALISE, lo, recs, None, 4, out) == IE
        assert fn(group, sr.FIXED, 1, None, tb, 4, out) == IE
        assert fn(group, sr.FIXED, 1, sc, None, 4, out) == IE
        assert fn(group, sr.FIXED, 1, sc, tb, 4, None) == IE
        assert fn(group, sr.NORMALISE, 0, None, None, 4, out) == IE
        assert fn(group, sr.NORMALISE, 0, recs, None, 4, None) == IE
        assert fn(group, sr.FIXED, 1, sc, tb, 1 << 32, out) == IE
        assert fn(group, sr.NORMALISE, 0, recs, None, 1 << 32, out) == IE
        assert fn(group, sr.FIXED, 1, None, None, 0, None) == OK               # n == 0 touches nothing
        assert fn(group, sr.FIXED, 3, None, None, 0, None) == IE               # ... but the enums are still judged
    for group in (0, 3):
        assert fn(group, sr.FIXED, 1, sc, tb, 4, out) == IE
