"""Inputs and expected outputs of the guard-band tests, shared by tests/test_guard_bands_host.py (the host twins, in a
HostArena) and tests/test_gpu_guard_bands.py (the _device forms, in a device Arena): the same table of calls and the same
shapes.  Every expected value comes from the big-integer models of the *_ref.py modules; nothing here calls the library.

The shapes are the smallest that cross each kernel's tail logic, W - 1, W, W + 1 for every unit W a launch uses; the units
were read from the launches (csrc/k_*.hip) and the headers they take their constants from:
  FR_MAP_N     kFrMapThreads = 256 (fr_vec.hip.h): the workgroup of fr_map_kernel, fr_lincomb_kernel and the shift; the
               inversion runs on tiles of 2^kFrInvTileLog = 256 records
  FR_SCAN_N    2^kFrTileLog = 512 records per scan tile (fr_vec.hip.h), one wave per tile; the polynomial calls run on the
               same tiles.  FR_SCAN_SMALL_TILE_N with MSM_AMD_FR_TILE_LOG = 2: 4^2 < 17, 4^3 < 65, 4^4 < 300, so three-,
               four- and five-level plans end in partial tiles
  MATVEC_ROWS  fr_mat_lane_kernel: one lane per short row, kFrMapThreads = 256 rows per workgroup, 64 per wave (k_fr.hip)
  MLE_N        fr_mle_bind_kernel and fr_eq_table_kernel: kFrMapThreads = 256; the round and eval kernels: one wave of 64
               lanes (kFrWave) over 2^kFrMleChunkLog = 256 pairs (fr_mle.hip.h)
  POSEIDON_N   fr_poseidon_kernel and fr_merkle_paths_kernel: one lane per state or record, kFrMapThreads = 256 per
               workgroup, 64 per wave (k_fr.hip)
  LOOKUP_ROWS / LOOKUP_TOTAL   kLookupThreads = 256 (rows, insert, probe, finish) and kLookupBlockThreads = 1024 (the
               probe of MSM_AMD_LOOKUP_COUNT = block) (fr_lookup.hip.h)
  POINT_N      one lane per record, 64 per wave; check_g1_kernel, the compress and decompress kernels of both groups and the
               G1 multiplication kernels launch 256 threads (check_sizes, COMPRESS_N, mul_sizes), check_g2_kernel and the G2
               multiplication kernels 64, convert_bases_kernel 128 (PREPARE_N) (k_check.hip, k_compress.hip, k_mul.hip,
               k_misc.hip)
  NTT_POINTS_LOGS   nttp_load / level / scale kernels: 256 threads, nttp_normalise_kernel 64 (k_nttp.hip)
  SORT_N       kSortThreads = 1024 (k_sort.hip), kRadixTile = 256 * kRadixItems = 4096 pairs (launch.h)
  PAIRING_SHAPES   (n_groups, group_size): 64 lanes per workgroup, one lane per pair in the Miller kernel, one per group in
               the final exponentiation (k_pairing.hip): 65 groups and a group of 65 pairs cross it
  MSM_N        the sizes the inputs of an MSM are held read-only at"""
import functools
import random

import fr_ref
import lookup_ref as lr
import matvec_ref
import mle_ref
import poly_ref
import poseidon_ref as ps

R = fr_ref.R
MONT_LE, CANON_LE = fr_ref.MONT_LE, fr_ref.CANON_LE
LAYOUTS = (MONT_LE, CANON_LE)

FR_MAP_N = (1, 255, 256, 257)
FR_SCAN_N = (1, 511, 512, 513)
FR_SCAN_SMALL_TILE_N = (17, 65, 300)
N_VEC = 3
MATVEC_ROWS = (63, 64, 65, 255, 256, 257)
MLE_N = (2, 64, 128, 256, 512, 1024)
POSEIDON_N = (1, 63, 64, 65, 255, 256, 257)
POSEIDON_T = (2, 3, 4, 5)
LOOKUP_ROWS = (63, 64, 65, 255, 256, 257)
LOOKUP_TOTAL = (1, 255, 256, 257, 1023, 1024, 1025)
POINT_N = (1, 3, 63, 65)
MUL_N = (1, 63, 65)
SORT_N = (1, 255, 256, 257, 1025, 4097)
PAIRING_SHAPES = ((1, 1), (3, 1), (3, 5), (5, 0), (65, 1), (1, 65))
MSM_N = (1, 65, 1000)


def check_sizes(group):
    return POINT_N + ((255, 256, 257) if group == 1 else ())            # check_g1_kernel: 256 threads, check_g2_kernel: 64


COMPRESS_N = POINT_N + (255, 257)                                      # both groups: 256 threads
PREPARE_N = MUL_N + (127, 129)                                         # convert_bases_kernel(_wide): 128 threads


def mul_sizes(group):
    return MUL_N + ((255, 257) if group == 1 else ())                   # the G1 kernels: 256 threads, the G2 kernels: 64


def layout_for(n):
    """both scalar layouts take turns over the sizes"""
    return LAYOUTS[n % 2]


@functools.lru_cache(maxsize=None)
def fr_records(n, layout, seed=0):
    """n records: the edge words (0, 1, r - 1, r, r + 5, 2^256 - 1 as they stand) first when there is room, then random"""
    rng = random.Random(1000 * n + seed)
    vals = fr_ref.encode([rng.randrange(R) for _ in range(n)], layout)
    edge = lr.raw(lr.EDGE_WORDS)
    return edge + vals[len(edge):] if n > len(lr.EDGE_WORDS) else vals


def fr_k(layout, seed=5):
    return fr_ref.encode([random.Random(seed).randrange(2, R)], layout)


# ---- Fr vectors ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fr_map_case(op, n):
    layout = layout_for(n)
    a, b, c, k = fr_records(n, layout, 1), fr_records(n, layout, 2), fr_records(n, layout, 3), fr_k(layout)
    return layout, a, b, c, k, fr_ref.fr_map(op, layout, a, b, c, k)


@functools.lru_cache(maxsize=None)
def fr_shift_case(n):
    layout = layout_for(n)
    a, k = fr_records(n, layout, 4), fr_k(layout, 6)
    return layout, a, k, lr.shift(a, k, layout)


@functools.lru_cache(maxsize=None)
def fr_lincomb_case(n):
    layout = layout_for(n)
    a, k = fr_records(n * N_VEC, layout, 7), fr_k(layout, 8)
    return layout, a, k, poly_ref.lincomb(a, k, layout, N_VEC)


@functools.lru_cache(maxsize=None)
def fr_inverse_case(n):
    layout = layout_for(n)
    a = fr_records(n, layout, 9)
    exp, zeros = fr_ref.batch_inverse(a, layout)
    return layout, a, exp, zeros


@functools.lru_cache(maxsize=None)
def fr_scan_case(kind, n, mode, n_vec=N_VEC):
    """kind: 'product' or 'sum'"""
    layout = layout_for(n)
    a = fr_records(n * n_vec, layout, 10)
    exp = fr_ref.prefix_product(a, layout, mode, n_vec) if kind == "product" else lr.prefix_sum(a, layout, mode, n_vec)
    return layout, a, exp


@functools.lru_cache(maxsize=None)
def fr_poly_case(n):
    layout = layout_for(n)
    a, z = fr_records(n * N_VEC, layout, 11), fr_k(layout, 12)
    q, rem = poly_ref.div_linear(a, z, layout, N_VEC)
    return layout, a, z, poly_ref.poly_eval(a, z, layout, N_VEC), q, rem


# ---- sparse matrix times vector -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matvec_case(n_rows):
    """row lengths 0 .. 9 and two long rows (40 and 300 entries: the wave path and a row of two segments)"""
    layout = layout_for(n_rows)
    rng = random.Random(300 + n_rows)
    lengths = [rng.randrange(10) for _ in range(n_rows)]
    lengths[n_rows // 2], lengths[-1] = 40, 300
    n_cols = 37
    mat = matvec_ref.from_lengths(n_rows, lengths, n_cols, layout)
    x = fr_records(n_cols, layout, 13)
    return layout, mat, x, matvec_ref.matvec(mat, x, layout, layout)


# ---- multilinear tables -------------------------------------------------------------------------------------------------------------
def mle_stride(n, strided):
    return n + 3 if strided else n


@functools.lru_cache(maxsize=None)
def mle_tables(n, n_vec, strided):
    """n_vec tables `stride` records apart as one input of (n_vec - 1) stride + n records; the gaps hold random bytes"""
    layout = layout_for(n.bit_length())
    stride = mle_stride(n, strided)
    rng = random.Random(17 * n + n_vec)
    data = b"".join(fr_records(n, layout, 20 + v) + (rng.randbytes(32 * (stride - n)) if v + 1 < n_vec else b"")
                    for v in range(n_vec))
    return layout, stride, data


@functools.lru_cache(maxsize=None)
def mle_bind_case(n, order, n_bind, strided):
    layout, stride, data = mle_tables(n, N_VEC, strided)
    r = mle_ref.challenges(40 + n, n_bind, layout)
    return layout, stride, data, r, mle_ref.bind(data, r, layout, order, n, N_VEC, stride)


def mle_bind_writable(n, stride, n_vec=N_VEC):
    """include/msm_amd.h: "The first n >> n_bind records of output table v (at out + 32 v stride) are the result; the call may
    also write the rest of that table's first n/2 records (unspecified content) and writes no other byte of out." """
    return [(32 * v * stride, 32 * (n // 2)) for v in range(n_vec)]


@functools.lru_cache(maxsize=None)
def mle_eval_case(n, order, strided):
    layout, stride, data = mle_tables(n, N_VEC, strided)
    point = mle_ref.challenges(50 + n, n.bit_length() - 1, layout)
    return layout, stride, data, point, mle_ref.evaluate(data, point, layout, order, n, N_VEC, stride)


@functools.lru_cache(maxsize=None)
def mle_eq_case(m, order):
    layout = layout_for(m)
    point = mle_ref.challenges(60 + m, m, layout)
    return layout, point, mle_ref.eq_table(point, layout, order)


@functools.lru_cache(maxsize=None)
def mle_round_case(n, order, form, n_vec, strided):
    layout, stride, data = mle_tables(n, n_vec, strided)
    return layout, stride, data, mle_ref.round_values(data, layout, order, form, n, n_vec, stride)


MLE_ROUND_SHAPES = ((mle_ref.PRODUCT, 1), (mle_ref.PRODUCT, 3), (mle_ref.EQ_AB_C, 4))     # 2, 4 and 4 records of g_out


# ---- Poseidon -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def poseidon_constants(t, layout):
    ark, mds = ps.constants(t)
    return ark, mds, ps.pack(ark, layout), ps.pack(mds, layout)


def _poseidon_inputs(count, layout, seed):
    vals = ps.random_values(seed, count)
    recs = [ps.enc(v, layout) for v in vals]
    for j, w in enumerate(ps.EDGE_WORDS):                   # raw edge words where there is room
        if 2 * j + 1 < count:
            recs[2 * j + 1] = ps.raw(w)
    return b"".join(recs)


@functools.lru_cache(maxsize=None)
def poseidon_permute_case(t, n):
    layout = layout_for(n + t)
    ark, mds, _, _ = poseidon_constants(t, layout)
    data = _poseidon_inputs(n * t, layout, 70 + n)
    vals = ps.unpack(data, layout)
    out = [x for k in range(n) for x in ps.permute(vals[k * t:(k + 1) * t], ark, mds, ps.R_F, ps.R_P[t])]
    return layout, data, ps.pack(out, layout)


@functools.lru_cache(maxsize=None)
def poseidon_hash_case(t, n):
    layout = layout_for(n + t)
    ark, mds, _, _ = poseidon_constants(t, layout)
    data, tag = _poseidon_inputs(n * (t - 1), layout, 80 + n), 0x1234 + t
    vals = ps.unpack(data, layout)
    out = [ps.hash_one(vals[k * (t - 1):(k + 1) * (t - 1)], ark, mds, ps.R_F, ps.R_P[t], tag) for k in range(n)]
    return layout, data, ps.enc(tag, layout), ps.pack(out, layout)


MERKLE_SHAPES = ((3, 2), (3, 64), (4, 27), (5, 16), (5, 64))      # (t, n_leaves): n_leaves a power of the arity t - 1
MERKLE_BAD_LEAVES = (3, 48)                                    # not a power of the arity: the header refuses it


@functools.lru_cache(maxsize=None)
def merkle_case(t, n_leaves):
    """leaves, tree records (root last), root, path indices (first, last, a repeated one) and their sibling records"""
    layout = layout_for(n_leaves + t)
    ark, mds, _, _ = poseidon_constants(t, layout)
    leaves = _poseidon_inputs(n_leaves, layout, 90 + n_leaves)
    tag = 7
    levels = ps.tree(ps.unpack(leaves, layout), t, ark, mds, ps.R_F, ps.R_P[t], tag)
    tree = ps.pack(ps.flat(levels), layout)
    idx = [0, n_leaves - 1, n_leaves // 2, n_leaves // 2]
    paths = b"".join(ps.pack(ps.path(ps.unpack(leaves, layout), levels, t - 1, i), layout) for i in idx)
    return layout, leaves, ps.enc(tag, layout), tree, tree[-32:], idx, paths


# ---- lookups ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lookup_case(n_rows, total, miss=False):
    """a table with duplicate rows, `total` inputs in N_VEC columns when total divides (else one); miss: one value in no row"""
    layout = layout_for(n_rows + total)
    table = lr.random_table(500 + n_rows, n_rows, layout, distinct=max(1, n_rows - 5))
    data = lr.draws(600 + total, table, layout, total, (total - 1,) if miss else ())
    n_vec = N_VEC if total % N_VEC == 0 else 1
    m, idx, rep = lr.multiplicities(table, data, layout)
    return layout, table, data, n_vec, m, idx, rep


# ---- points -------------------------------------------------------------------------------------------------------------------------
import struct                                  # noqa: E402

import check_ref as c                          # noqa: E402
import compress_ref as cr                      # noqa: E402
import g2_ref as g2                            # noqa: E402
import mul_ref as mr                           # noqa: E402
import ntt_points_ref as npr                   # noqa: E402
import ntt_ref                                 # noqa: E402
import pairing_ref as pr                       # noqa: E402
from oracle import bn254_ref as o              # noqa: E402

G1_LAYOUTS, G2_LAYOUTS = mr.IN_LAYOUTS[1], mr.IN_LAYOUTS[2]          # the host layouts of a point argument
G1_OUT, G2_OUT = mr.OUT_LAYOUTS[1], mr.OUT_LAYOUTS[2]                # the affine host layouts of a point output
PREPARED, G2_PREPARED = 4, 2                                         # MSM_AMD_POINT_PREPARED, MSM_AMD_G2_POINT_PREPARED
PREPARED_BYTES = {1: 64, 2: 128}
FORMATS = (cr.ARK, cr.PARITY)


@functools.lru_cache(maxsize=None)
def dlogs(n, seed):
    rng = random.Random(seed)
    return tuple(rng.randrange(1, pr.R_ORDER) for _ in range(n))


@functools.lru_cache(maxsize=None)
def g1_of(a):
    return npr.gmul(a)


@functools.lru_cache(maxsize=None)
def g2_of(a):
    return g2.scalar_mul(a % pr.R_ORDER, g2.GEN2) if a % pr.R_ORDER else None


@functools.lru_cache(maxsize=None)
def _progression(group, n, seed):
    """(discrete logs, points): (a0 + i d) G by n - 1 additions"""
    rng = random.Random(seed)
    a0, d = rng.randrange(1, pr.R_ORDER), rng.randrange(1, pr.R_ORDER)
    if group == 1:
        cur, step, pts = o.to_jac(g1_of(a0)), o.to_jac(g1_of(d)), []
        for _ in range(n):
            pts.append(o.to_affine(cur))
            cur = o.jac_add(cur, step)
    else:
        cur, step, pts = g2_of(a0), g2_of(d), []
        for _ in range(n):
            pts.append(cur)
            cur = g2.add(cur, step)
    return tuple((a0 + i * d) % pr.R_ORDER for i in range(n)), tuple(pts)


def group_points(group, n, seed):
    """n points of a group with known discrete logs (the identity at index 1 when there is room)"""
    dl, pts = _progression(group, n, seed)
    dl, pts = list(dl), list(pts)
    if n >= 3:
        dl[1], pts[1] = 0, None
    return dl, pts


def layout_of(group, k, out=False):
    """the layouts of a group take turns over k"""
    ls = (G1_OUT if group == 1 else G2_OUT) if out else (G1_LAYOUTS if group == 1 else G2_LAYOUTS)
    return ls[k % len(ls)]


@functools.lru_cache(maxsize=None)
def check_case(group, n):
    """n records with a not-reduced one first and one off the curve last (n >= 3); the expected reason bytes and report"""
    layout = layout_of(group, n)
    _, pts = group_points(group, n, 700 + n)
    recs = [c.g1_rec(layout, p, 1 + i) if group == 1 else c.g2_rec(layout, p) for i, p in enumerate(pts)]
    if n >= 3:
        recs[0] = c.non_reduced(recs[0], 0)
        recs[n - 1] = recs[n - 1].with_coord(1, (recs[n - 1].coords[1] + 1) % c.P)
    checks = 1 if group == 1 else 3
    report, reasons = c.expected_report(recs, checks)
    return layout, checks, c.encode_all(recs), reasons, report


@functools.lru_cache(maxsize=None)
def decompress_case(group, n, fmt):
    """n compressed records, the second-last one bad (n >= 3): (records, reasons, report, {affine layout: output})"""
    _, pts = group_points(group, n, 720 + n)
    recs = [cr.encode(group, fmt, p) for p in pts]
    if n >= 3:
        recs[n - 2] = b"\xff" * cr.SIZE[group]
    report, reasons = cr.expected_report(group, fmt, recs)
    outs = {lo: cr.expected_output(group, fmt, lo, recs) for lo in (G1_OUT if group == 1 else G2_OUT)}
    return b"".join(recs), recs, reasons, report, outs


@functools.lru_cache(maxsize=None)
def compress_case(group, n, fmt, layout):
    """n affine records, the last one not reduced (n >= 3): (points, compressed records, n_bad)"""
    _, pts = group_points(group, n, 740 + n)
    recs = [c.g1_rec(layout, p) if group == 1 else c.g2_rec(layout, p) for p in pts]
    if n >= 3:
        recs[n - 1] = c.non_reduced(recs[n - 1], 0)
    got = [cr.compress_expected(group, fmt, r) for r in recs]
    return c.encode_all(recs), b"".join(b for b, _ in got), sum(bad for _, bad in got)


@functools.lru_cache(maxsize=None)
def mul_case(group, n, mode):
    """(scalar layout, point layout in, scalars, base records, the expected affine points): a zero scalar at index 0"""
    sl, li = n % 3, layout_of(group, n + mode)
    ks = list(dlogs(n, 760 + n))
    ks[0] = 0
    dl, bases = group_points(group, n if mode == mr.EACH else 1, 780 + n)
    each = bases if mode == mr.EACH else bases * n
    if group == 1:                                                     # G1 has prime order: [k] [a] G = [k a] G from the table
        want = [g1_of(k * a % pr.R_ORDER) if k * a % pr.R_ORDER else None for k, a in zip(ks, dl if mode == mr.EACH else dl * n)]
    else:
        want = [mr.expected(group, k, p) for k, p in zip(ks, each)]
    pts = b"".join(mr.base_record(group, li, p, 3 + i) for i, p in enumerate(bases))
    return sl, li, mr.scalars_bytes(ks, sl), pts, want


def mul_out_layouts(group, n):
    """both affine output layouts at the largest size, one of them -- taking turns -- at the others"""
    los = G1_OUT if group == 1 else G2_OUT
    return los if n == MUL_N[-1] else (los[n % len(los)],)


def point_records(group, layout, pts):
    return b"".join(mr.out_record(group, layout, p) for p in pts)


@functools.lru_cache(maxsize=None)
def pairing_case(n_groups, group_size):
    """(G1 layout, G2 layout, G1 records, G2 records, expected GT values per group, is_one bytes): the last group of a
    product of several pairs cancels, so that is_one holds both values"""
    n = n_groups * group_size
    sp = [(a, b) for a, b in zip(dlogs(n, 800 + n), dlogs(n, 810 + n))]
    if group_size >= 2:
        a, b = sp[-2]
        sp[-1] = (pr.R_ORDER - a, b)
        for k in range(n - group_size, n - 2):
            sp[k] = (sp[k][0], 0)                                     # Q = O: the pair contributes 1
    l1, l2 = layout_of(1, n_groups), layout_of(2, group_size)
    a = b"".join(mr.base_record(1, l1, g1_of(x) if x % pr.R_ORDER else None, 5 + i) for i, (x, _) in enumerate(sp))
    b = b"".join(mr.base_record(2, l2, g2_of(y)) for _, y in sp)
    want = [pr.expected_by_dlog(sp[k * group_size:(k + 1) * group_size]) for k in range(n_groups)]
    return l1, l2, a, b, want, bytes(1 if w == pr.ONE12 else 0 for w in want)


def gt_records(values, layout):
    return b"".join(pr.encode_gt(v, layout) for v in values)


# ---- transforms -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ntt_case(log_n, n_vec, direction, shifted):
    layout, root, n = layout_for(log_n + n_vec), log_n & 1, 1 << log_n
    a = ntt_ref.random_vector(900 + log_n, n * n_vec)
    shift = 5 + log_n if shifted else 1
    exp = [x for v in range(n_vec) for x in ntt_ref.transform(a[v * n:(v + 1) * n], root, log_n, direction, shift)]
    return layout, root, ntt_ref.encode(a, layout), ntt_ref.shift_record(shift, layout) if shifted else None, ntt_ref.encode(exp, layout)


NTT_POINTS_LOGS = (1, 6, 7, 8, 9)


@functools.lru_cache(maxsize=None)
def ntt_points_case(log_n, direction):
    li, root = G1_LAYOUTS[log_n % 4], log_n & 1
    a = list(npr.random_logs(log_n))
    return li, root, npr.in_records(a, li), tuple(npr.gmul(v) for v in npr.transform(a, root, log_n, direction))


def ntt_points_inputs(log_n):
    """the points the cases of ntt_points_case transform"""
    return tuple(npr.gmul(v) for v in npr.random_logs(log_n))


# ---- MSM inputs with known discrete logs ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def msm_case(group, n, bits=254):
    """(scalar layout, scalars, H2C point records, expected affine point): bases (a0 + i d) G by additions"""
    rng = random.Random(950 + n + bits)
    dl, pts = _progression(group, n, 960 + n)
    ks = [rng.randrange(1 << bits) % pr.R_ORDER for _ in range(n)]
    if n >= 3:
        ks[2] = 0
    sl = n % 2
    total = sum(k * a for k, a in zip(ks, dl)) % pr.R_ORDER
    want = (g1_of if group == 1 else g2_of)(total)
    return sl, mr.scalars_bytes(ks, sl), point_records(group, 0, pts), want


def msm_result(group, out):
    """the affine point of a 96-byte (G1) or 192-byte (G2) Jacobian result"""
    return o.decode_jacobian_mont_le(out) if group == 1 else (None if out == g2.identity_bytes() else g2.decode_jacobian(out))


# ---- sort ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sort_case(n_pairs, key_bits):
    """(pairs as bytes, a checker): (key, payload) u32 pairs with keys below 2^key_bits and the index as payload"""
    rng = random.Random(n_pairs + key_bits)
    pairs = [(rng.randrange(1 << key_bits), i) for i in range(n_pairs)]
    data = struct.pack("<%dI" % (2 * n_pairs), *[w for p in pairs for w in p])
    return data, sorted(pairs, key=lambda p: p[0])


# ---- which calls of include/msm_amd.h the GPU file covers ---------------------------------------------------------------------------------
DEVICE_CALLS_COVERED = (
    "msm_device", "msm_batch_device", "msm_bounded_device", "msm_g2_device", "msm_g2_bounded_device", "scalar_width_device",
    "bases_prepare_device", "g2_bases_prepare_device", "sort_pairs_device",
    "check_points_device", "g2_check_points_device", "decompress_points_device", "g2_decompress_points_device",
    "compress_points_device", "g2_compress_points_device", "mul_points_device", "g2_mul_points_device",
    "ntt_device", "ntt_points_device",
    "fr_map_device", "fr_batch_inverse_device", "fr_prefix_product_device", "fr_prefix_sum_device", "fr_shift_device",
    "fr_poly_eval_device", "fr_poly_div_linear_device", "fr_lincomb_device", "fr_matvec_device",
    "fr_mle_bind_device", "fr_mle_eval_device", "fr_eq_table_device", "fr_sumcheck_round_device",
    "poseidon_permute_device", "poseidon_hash_device", "poseidon_merkle_build_device", "poseidon_merkle_paths_device",
    "fr_lookup_build_device", "fr_lookup_multiplicities_device", "pairing_product_device", "final_exponentiation_device")
DEVICE_CALLS_EXCLUDED = {
    "submit_batch_device": "the asynchronous twin of msm_batch_device: the same kernels on the same buffers",
    "submit_batch_bounded_device": "the asynchronous twin of msm_batch_bounded_device",
    "submit_batch_multi_device": "the asynchronous twin of msm_batch_multi_device",
    "msm_batch_bounded_device": "msm_batch_device at a bounded width; the bounded plan is covered by msm_bounded_device",
    "msm_batch_multi_device": "msm_batch_device over several ctxs",
    "tables_build_device": "writes only memory the library allocates itself",
    "g2_tables_build_device": "writes only memory the library allocates itself",
    "copy_to_device": "no compute call: the upload of the harness itself",
    "ctx_device": "no buffers: the device ordinal of a ctx",
    "pin_thread_to_device": "no buffers: binds the calling thread to a device",
}
