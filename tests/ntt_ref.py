"""Model side of the transform tests (msm_amd_ntt*, msm_amd_host_ntt): Python integers; np_random_records builds the
columns that are too long for them (pinned by tests/test_np_models_host.py).  The two 2^28-th roots as
g^t, a naive O(n^2) DFT, a recursive radix-2 transform for the sizes the naive one cannot reach, the closed form for
sparse inputs, the state of the library's network after some of its levels, and the record encoders of the two scalar
layouts.  Nothing here calls the library."""
import functools
import random

import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617   # BN254 scalar field
MONT = 1 << 256
MONT_LE, CANON_LE, CANON_BE32 = 0, 1, 2          # MSM_AMD_SCALAR_*
ARK, H2C = 0, 1                                  # MSM_AMD_NTT_ROOT_*
FORWARD, INVERSE = 0, 1                          # MSM_AMD_NTT_*
ROOTS, DIRECTIONS, LAYOUTS = (ARK, H2C), (FORWARD, INVERSE), (MONT_LE, CANON_LE)
TWO_ADICITY = 28
T_ODD = (R - 1) >> TWO_ADICITY
assert (R - 1) == T_ODD << TWO_ADICITY and T_ODD & 1
GENERATOR = {ARK: 5, H2C: 7}
# the values include/msm_amd.h prints (UNPINNED against the crates; pinned here against g^t)
RHO_LITERAL = {
    ARK: 19103219067921713944291392827692070036145651957329286315305642004821462161904,
    H2C: 0x03ddb9f5166d18b798865ea93dd31f743215cf6dd39329c8d34f1ed960c37c9c,
}


@functools.lru_cache(maxsize=None)
def rho(root):
    return pow(GENERATOR[root], T_ODD, R)


@functools.lru_cache(maxsize=None)
def omega(root, log_n):
    """the primitive 2^log_n-th root of the contract"""
    return pow(rho(root), 1 << (TWO_ADICITY - log_n), R)


def naive(a, root, log_n, direction, g=1):
    """the definition, term by term"""
    n = 1 << log_n
    assert len(a) == n
    w = omega(root, log_n)
    if direction == FORWARD:
        b = [x * pow(g, i, R) % R for i, x in enumerate(a)]
        return [sum(b[i] * pow(w, i * k % n, R) for i in range(n)) % R for k in range(n)]
    wi, gi, ni = pow(w, -1, R), pow(g, -1, R), pow(n, -1, R)
    return [sum(a[k] * pow(wi, i * k % n, R) for k in range(n)) * pow(gi, i, R) * ni % R for i in range(n)]


def _radix2(a, w):
    n = len(a)
    if n == 1:
        return a
    even, odd = _radix2(a[0::2], w * w % R), _radix2(a[1::2], w * w % R)
    out = [0] * n
    t = 1
    for k in range(n // 2):
        u = odd[k] * t % R
        out[k] = (even[k] + u) % R
        out[k + n // 2] = (even[k] - u) % R
        t = t * w % R
    return out


def transform(a, root, log_n, direction, g=1):
    """the same values by a recursive radix-2 transform (decimation in time: not the library's network)"""
    n = 1 << log_n
    assert len(a) == n
    a = [x % R for x in a]
    w = omega(root, log_n)
    if direction == FORWARD:
        t, b = 1, []
        for x in a:
            b.append(x * t % R)
            t = t * g % R
        return _radix2(b, w)
    out = _radix2(a, pow(w, -1, R))
    gi, t = pow(g, -1, R), pow(n, -1, R)
    for i in range(n):
        out[i] = out[i] * t % R
        t = t * gi % R
    return out


def sparse_forward(terms, root, log_n, k, g=1):
    """out[k] of FORWARD for an input with coefficient c at position i for (i, c) in terms"""
    w, n = omega(root, log_n), 1 << log_n
    return sum(c * pow(g, i, R) * pow(w, i * k % n, R) for i, c in terms) % R


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def level_states(a, root, log_n, direction, g=1):
    """the decimation-in-frequency network of csrc/ntt.hip.h's head comment on natural-order input: yields the state
    after 0, 1, .. log_n levels (a fresh list each).  a[i] g^i comes first when the direction is FORWARD (INVERSE scales
    after the network, so its states are those of the plain sums); level l pairs i with i + h, h = n >> (l + 1), for
    every i with bit log_n - 1 - l clear: a[i], a[i + h] <- a[i] + a[i + h], (a[i] - a[i + h]) w^((i mod h) << l)."""
    n = 1 << log_n
    assert len(a) == n
    a = [x % R for x in a]
    if direction == FORWARD:
        t = 1
        for i in range(n):
            a[i] = a[i] * t % R
            t = t * g % R
    yield list(a)
    w = omega(root, log_n)
    for level in range(log_n):
        h = n >> (level + 1)
        step = pow(w, 1 << level, R)          # w^((i mod h) << l) = step^(i mod h)
        tw, t = [], 1
        for _ in range(h):
            tw.append(t)
            t = t * step % R
        for base in range(0, n, 2 * h):
            for j in range(h):
                i = base + j
                x, y = a[i], a[i + h]
                a[i] = (x + y) % R
                a[i + h] = (x - y) * tw[j] % R
        yield list(a)


def levels_state(a, root, log_n, direction, g=1, levels=None):
    """the state of that network after `levels` levels (default: all).  After log_n levels position bitrev(k) holds
    sum_i a[i] w^(i k): transform(FORWARD)[k], and g^i n transform(INVERSE)[i] for k = (n - i) mod n."""
    levels = log_n if levels is None else levels
    assert 0 <= levels <= log_n
    for done, state in enumerate(level_states(a, root, log_n, direction, g)):
        if done == levels:
            return state


def encode(values, layout):
    """records of a scalar layout; values are stored as they are for CANON_LE (they may be >= r), mod r for MONT_LE"""
    if layout == MONT_LE:
        return b"".join((v % R * MONT % R).to_bytes(32, "little") for v in values)
    return b"".join(v.to_bytes(32, "little") for v in values)


def decode(data, layout):
    vals = [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]
    if layout == MONT_LE:
        inv = pow(MONT, -1, R)
        return [v * inv % R for v in vals]
    return vals


def shift_record(g, layout):
    return None if g is None else encode([g], layout)


def random_vector(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


# ---- numpy: columns too long for Python integers -----------------------------------------------------------------------------------
TOP_WORD_BELOW = 0x30000000      # r's top word is 0x30644e72: a record whose top word is below this is a reduced word


def np_random_records(seed, n):
    """(n, 8) uint32 records, every one a reduced 256-bit word; in MONT_LE the word w stands for w / MONT"""
    rec = np.random.default_rng(seed).integers(0, 1 << 32, size=(n, 8), dtype=np.uint32)
    rec[:, 7] %= np.uint32(TOP_WORD_BELOW)
    return rec

