"""Big-integer model of Poseidon over BN254 Fr (the circomlib / circomlibjs / iden3 family): the Grain generator of the
paper's generate_parameters_grain, the textbook permutation, the hash, Merkle trees, authentication paths and their
verifier.  Written from the paper's description, independently of the C text; tests/test_poseidon_host.py pins the
library's twins to it, tests/test_gpu_poseidon.py the kernels."""
import random

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % R
MONT_INV = pow(MONT, -1, R)
MONT_LE, CANON_LE = 0, 1
R_F = 8
R_P = {2: 56, 3: 57, 4: 56, 5: 60}
EDGE_WORDS = (0, R - 1, R, (1 << 256) - 1)


# ---- records -----------------------------------------------------------------------------------------------------------------
def enc(x, layout):
    """a value mod r as the library writes it: the fully reduced residue"""
    x %= R
    return ((x * MONT) % R if layout == MONT_LE else x).to_bytes(32, "little")


def raw(word):
    """any 256-bit word as it stands"""
    return word.to_bytes(32, "little")


def dec(rec, layout):
    """any 256-bit word is taken mod r"""
    w = int.from_bytes(rec, "little") % R
    return (w * MONT_INV) % R if layout == MONT_LE else w


def pack(values, layout):
    return b"".join(enc(v, layout) for v in values)


def unpack(data, layout):
    return [dec(data[k:k + 32], layout) for k in range(0, len(data), 32)]


def random_values(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


# ---- constants ----------------------------------------------------------------------------------------------------------------
class Grain:
    def __init__(self, t, r_f, r_p):
        bits = ""
        for value, width in ((1, 2), (0, 4), (254, 12), (t, 12), (r_f, 10), (r_p, 10)):
            bits += format(value, "0%db" % width)
        self.s = [int(b) for b in bits] + [1] * 30
        assert len(self.s) == 80
        for _ in range(160):
            self.update()

    def update(self):
        s = self.s
        b = s[62] ^ s[51] ^ s[38] ^ s[23] ^ s[13] ^ s[0]
        s.pop(0)
        s.append(b)
        return b

    def bit(self):
        while not self.update():
            self.update()
        return self.update()

    def integer(self):
        x = 0
        for _ in range(254):
            x = (x << 1) | self.bit()
        return x


_CONSTANTS = {}


def constants(t, r_f=R_F, r_p=None):
    """(ark, mds) as lists of integers: (r_f + r_p) t round constants, the t x t matrix row-major"""
    r_p = R_P[t] if r_p is None else r_p
    key = (t, r_f, r_p)
    if key not in _CONSTANTS:
        g = Grain(t, r_f, r_p)
        ark = []
        while len(ark) < (r_f + r_p) * t:
            x = g.integer()
            if x < R:
                ark.append(x)
        while True:
            xy = [g.integer() % R for _ in range(2 * t)]
            if len(set(xy)) == 2 * t and all((x + y) % R for x in xy[:t] for y in xy[t:]):
                break
        mds = [pow(xy[i] + xy[t + j], -1, R) for i in range(t) for j in range(t)]
        _CONSTANTS[key] = (ark, mds)
    return _CONSTANTS[key]


# ---- permutation, hash, tree -----------------------------------------------------------------------------------------------
def permute(state, ark, mds, r_f, r_p):
    t = len(state)
    s = [x % R for x in state]
    for rho in range(r_f + r_p):
        s = [(s[i] + ark[rho * t + i]) % R for i in range(t)]
        if rho < r_f // 2 or rho >= r_f // 2 + r_p:
            s = [pow(x, 5, R) for x in s]
        else:
            s[0] = pow(s[0], 5, R)
        s = [sum(mds[i * t + j] * s[j] for j in range(t)) % R for i in range(t)]
    return s


def hash_one(inputs, ark, mds, r_f, r_p, tag=0):
    return permute([tag] + list(inputs), ark, mds, r_f, r_p)[0]


def poseidon(inputs, tag=0):
    """circomlib's poseidon([...]) for 1 .. 4 inputs"""
    t = len(inputs) + 1
    ark, mds = constants(t)
    return hash_one(inputs, ark, mds, R_F, R_P[t], tag)


def depth(arity, n_leaves):
    d = 0
    while n_leaves > 1:
        assert n_leaves % arity == 0
        n_leaves, d = n_leaves // arity, d + 1
    return d


def tree(leaves, t, ark, mds, r_f, r_p, tag=0):
    """the levels above the leaves, the parents of the leaves first; the root is levels[-1][0]"""
    a, level, levels = t - 1, [x % R for x in leaves], []
    while len(level) > 1:
        level = [hash_one(level[k:k + a], ark, mds, r_f, r_p, tag) for k in range(0, len(level), a)]
        levels.append(level)
    return levels


def flat(levels):
    return [x for level in levels for x in level]


def path(leaves, levels, arity, index):
    """the siblings of leaf `index`, bottom level first, in child order without the node's own place"""
    out, pos = [], index
    for level in [[x % R for x in leaves]] + levels[:-1]:
        base = pos - pos % arity
        out += [level[base + c] for c in range(arity) if base + c != pos]
        pos //= arity
    return out


def verify(leaf, index, siblings, arity, root, ark, mds, r_f, r_p, tag=0):
    node, pos, at = leaf % R, index, 0
    while at < len(siblings):
        own = pos % arity
        group = siblings[at:at + arity - 1]
        node = hash_one(group[:own] + [node] + group[own:], ark, mds, r_f, r_p, tag)
        pos, at = pos // arity, at + arity - 1
    return node == root
