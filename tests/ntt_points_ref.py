"""Model side of the point-transform tests (msm_amd_ntt_points*, msm_amd_host_ntt_points): G1 has prime order r, so every
input is [a_j] G and the transform is linear -- the expected output is [ntt(a)_k] G with ntt(a) from ntt_ref on Python
integers, and the state of the library's network after some levels is that network run on the discrete logs.  Records
come from mul_ref.out_record / mul_ref.base_record.  Nothing here calls the library."""
import functools
import random

import check_ref as c
import mul_ref
import ntt_ref
from oracle import bn254_ref as o

R = ntt_ref.R
FORWARD, INVERSE = ntt_ref.FORWARD, ntt_ref.INVERSE
ARK, H2C = ntt_ref.ARK, ntt_ref.H2C
IN_LAYOUTS = mul_ref.IN_LAYOUTS[1]            # H2C, ARK_PROJECTIVE, ARK_AFFINE, JAC_BE32
OUT_LAYOUTS = mul_ref.OUT_LAYOUTS[1]          # H2C, ARK_AFFINE
PREPARED, TABLES = 4, 5                       # MSM_AMD_POINT_PREPARED, _TABLES
IN_BYTES, OUT_BYTES = c.G1_BYTES, {c.H2C: 64, c.ARK_AFFINE: 72}


# ---- [k] G, quickly: one Jacobian addition per non-zero byte of k from a table of [d 2^(8 w)] G -------------------------
@functools.lru_cache(maxsize=None)
def _rows():
    rows, base = [], o.to_jac(o.GEN)
    for _ in range(32):
        row, cur = [None], None
        for _ in range(255):
            cur = o.jac_add(cur, base)
            row.append(cur)
        rows.append(row)
        base = o.jac_add(row[255], row[1])                   # [256] base
    for k in (1, 2, 255, 256, R - 1, 0x1234567 << 200):       # the table against the model the other tests use
        assert _gmul(k, rows) == mul_ref.expected(1, k, o.GEN)
    return rows


def _gmul(k, rows):
    acc, w = None, 0
    while k:
        if k & 255:
            acc = o.jac_add(acc, rows[w][k & 255])
        k >>= 8
        w += 1
    return o.to_affine(acc)


@functools.lru_cache(maxsize=None)
def gmul(k):
    """[k mod r] G as an affine point, None = identity"""
    return _gmul(k % R, _rows())


def in_records(a, layout, seed=7):
    """[a_j] G as records of an input layout; the Jacobian layouts with a Z != 1 of their own per record"""
    rng = random.Random(seed)
    return b"".join(mul_ref.base_record(1, layout, gmul(x), rng.randrange(2, o.P)) for x in a)


def out_records(vals, layout):
    return b"".join(mul_ref.out_record(1, layout, gmul(v)) for v in vals)


def out_record(v, layout):
    return mul_ref.out_record(1, layout, gmul(v))


# ---- the transform and its network on the discrete logs --------------------------------------------------------------------
def transform(a, root, log_n, direction):
    """the contract: FORWARD out[k] = sum a_i w^(ik), INVERSE out[i] = n^-1 sum a_k w^(-ik)"""
    return ntt_ref.transform(a, root, log_n, direction)


def level_states(a, root, log_n, direction):
    """The network include/msm_amd.h states, on scalars: work[bitrev(j)] = a[j], then level l = 1 .. log_n: for every
    block base b (multiple of 2^l) and i < 2^(l-1): u = work[b+i], v = w^(+-i n / 2^l) work[b+i+2^(l-1)],
    work[b+i] = u + v, work[b+i+2^(l-1)] = u - v.  Yields the state after 0, 1, .. log_n levels (no scaling)."""
    n = 1 << log_n
    assert len(a) == n
    work = [0] * n
    for j, x in enumerate(a):
        work[ntt_ref.bitrev(j, log_n)] = x % R
    yield list(work)
    w = ntt_ref.omega(root, log_n)
    if direction == INVERSE:
        w = pow(w, -1, R)
    for l in range(1, log_n + 1):
        half = 1 << (l - 1)
        step = pow(w, n >> l, R)
        for b in range(0, n, 2 * half):
            t = 1
            for i in range(half):
                u, v = work[b + i], t * work[b + i + half] % R
                work[b + i], work[b + i + half] = (u + v) % R, (u - v) % R
                t = t * step % R
        yield list(work)


def lagrange_at(tau, root, log_n):
    """L_i(tau) for the domain {w^i}: L_i(X) = prod_{j != i} (X - w^j) / (w^i - w^j), term by term"""
    n, w = 1 << log_n, ntt_ref.omega(root, log_n)
    xs = [pow(w, i, R) for i in range(n)]
    out = []
    for i in range(n):
        num = den = 1
        for j in range(n):
            if j != i:
                num = num * (tau - xs[j]) % R
                den = den * (xs[i] - xs[j]) % R
        out.append(num * pow(den, -1, R) % R)
    return out


# ---- planted vectors --------------------------------------------------------------------------------------------------------
def planted(root, log_n, direction, seed=11):
    """name -> discrete logs.  delta: identity operands everywhere; constant: a doubling and a vanishing sum at every
    level, one point and n - 1 identities out; geometric c w^(-+j): one non-zero output; alternating a, -a; zeros;
    doubling: a_0 = w^(+-n/4) a_(n/2) and a_(n/4) chosen so that at level 2 the lane i = 1 of block 0, which walks the
    ladder of w^(+-n/4), meets T = u (log_n >= 2)."""
    n = 1 << log_n
    rng = random.Random(seed + 16 * log_n + root)
    cst, alt = rng.randrange(1, R), rng.randrange(1, R)
    w = ntt_ref.omega(root, log_n)
    ws = pow(w, -1, R) if direction == INVERSE else w          # the root the network of this direction multiplies by
    out = {
        "delta": [cst] + [0] * (n - 1),
        "constant": [cst] * n,
        "geometric": [cst * pow(ws, -j % n, R) % R for j in range(n)],
        "alternating": [alt if j % 2 == 0 else R - alt for j in range(n)],
        "zeros": [0] * n,
    }
    if log_n >= 2:
        a = [rng.randrange(1, R) for _ in range(n)]
        q = pow(ws, n // 4, R)
        a[0] = q * a[n // 2] % R
        a[n // 4] = (a[3 * n // 4] + pow(q, -1, R) * (a[0] - a[n // 2])) % R
        s1 = list(level_states(a, root, log_n, direction))[1]
        assert s1[1] != 0 and s1[1] == q * s1[3] % R           # u = T at level 2, block 0, i = 1
        out["doubling"] = a
    return out


@functools.lru_cache(maxsize=None)
def random_logs(log_n, seed=3):
    """n discrete logs with a zero (an identity input) among them when there is room"""
    rng = random.Random(seed + log_n)
    a = [rng.randrange(1, R) for _ in range(1 << log_n)]
    if log_n >= 2:
        a[rng.randrange(1 << log_n)] = 0
    return tuple(a)
