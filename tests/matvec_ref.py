"""Model side of the sparse-product tests (msm_amd_fr_matrix_*, msm_amd_fr_matvec*): Python integers on the record coders
of tests/fr_ref.py, and seeded generators of CSR matrices.  A matrix is a Csr: row_ptr and col_idx as lists of int (or
numpy arrays for the large shapes), values as records.  A model call takes records and returns records, so that a test
compares bytes.  Nothing here calls the library."""
import random

import numpy as np

from fr_ref import CANON_LE, LAYOUTS, MONT_LE, R, decode, encode, first_difference, random_values, raw, words  # noqa: F401

# the words a record may hold: (name, the raw word, or None for the unique record of the residue; the residue)
EDGE_WORDS = (("zero", None, 0), ("one", None, 1), ("minus_one", None, R - 1), ("raw_r", R, 0), ("r_plus_1", R + 1, 1),
              ("all_ones", (1 << 256) - 1, ((1 << 256) - 1) % R))


class Csr:
    def __init__(self, n_rows, n_cols, row_ptr, col_idx, values):
        self.n_rows, self.n_cols, self.row_ptr, self.col_idx, self.values = n_rows, n_cols, row_ptr, col_idx, values

    @property
    def nnz(self):
        return int(self.row_ptr[-1])

    def c_args(self):
        """(n_rows, n_cols, row_ptr, col_idx, values) as the bindings take them: packed bytes for numpy arrays"""
        rp = self.row_ptr.astype(np.uint64).tobytes() if isinstance(self.row_ptr, np.ndarray) else self.row_ptr
        ci = self.col_idx.astype(np.uint32).tobytes() if isinstance(self.col_idx, np.ndarray) else self.col_idx
        return self.n_rows, self.n_cols, rp, ci, self.values


def edge_records(layout, seed=5):
    """records of the edge words and of one random value; a raw word means what the layout makes of it"""
    recs = [raw([w]) if w is not None else encode([v], layout) for _, w, v in EDGE_WORDS]
    recs.append(encode([random.Random(seed).randrange(2, R - 1)], layout))
    return recs


def recode(data, layout, to_layout):
    """the unique records, in to_layout, of the values that `data` holds in `layout`"""
    return encode(decode(data, layout), to_layout)


def rows_model(mat, x, v_layout, layout, rows):
    """the values y[i] of the rows asked for: the definition with Python integers"""
    X = decode(x, layout)
    out = []
    for i in rows:
        lo, hi = int(mat.row_ptr[i]), int(mat.row_ptr[i + 1])
        V = decode(mat.values[32 * lo:32 * hi], v_layout)
        out.append(sum(v * X[int(mat.col_idx[lo + k])] for k, v in enumerate(V)) % R)
    return out


def matvec(mat, x, v_layout, layout):
    """records of y = M x in the layout of x"""
    return encode(rows_model(mat, x, v_layout, layout, range(mat.n_rows)), layout)


def n_distinct(mat, v_layout):
    """what the dictionary of a build holds: the distinct residues"""
    return len(set(decode(mat.values, v_layout)))


def from_lengths(seed, lengths, n_cols, v_layout, values=None):
    """a matrix of these row lengths, random columns (repeats inside a row happen), random values unless given as ints"""
    rng = random.Random(seed)
    row_ptr = [0]
    for ln in lengths:
        row_ptr.append(row_ptr[-1] + ln)
    nnz = row_ptr[-1]
    cols = [rng.randrange(n_cols) for _ in range(nnz)]
    vals = [rng.randrange(R) for _ in range(nnz)] if values is None else [values[k % len(values)] for k in range(nnz)]
    return Csr(len(lengths), n_cols, row_ptr, cols, encode(vals, v_layout))


def r1cs_shape(seed, n, v_layout=MONT_LE, ones=False):
    """The shape of an R1CS matrix, n rows and n columns: row lengths 1 + Poisson(2) (mean 3); one row in a thousand of
    1 000 entries; row n / 2 of n / 4 entries; nine values in ten are 1 or r - 1, the rest one of 30 constants; column 0
    leads a fifth of the rows.  ones: every value is 1 (the closed-form test).  The Csr carries value_ids and table (the
    32 residues) for models that sample rows."""
    rng = np.random.default_rng(seed)
    lengths = 1 + rng.poisson(2.0, n).astype(np.int64)
    lengths[rng.choice(n, max(1, n // 1000), replace=False)] = 1000
    lengths[n // 2] = n // 4
    row_ptr = np.zeros(n + 1, dtype=np.uint64)
    row_ptr[1:] = np.cumsum(lengths)
    nnz = int(row_ptr[-1])
    cols = rng.integers(0, n, nnz, dtype=np.uint32)
    lead = rng.random(n) < 0.2
    cols[row_ptr[:-1][lead].astype(np.int64)] = 0
    table = [1, R - 1] + random_values(seed + 1, 30)
    pick = rng.random(nnz)
    ids = np.where(pick < 0.45, 0, np.where(pick < 0.9, 1, 2 + rng.integers(0, 30, nnz))).astype(np.int64)
    if ones:
        ids[:] = 0
    recs = np.frombuffer(encode(table, v_layout), dtype=np.uint8).reshape(32, 32)
    mat = Csr(n, n, row_ptr, cols, recs[ids].tobytes())
    mat.value_ids, mat.table = ids, table
    return mat


def uniform_shape(seed, n, per_row=8):
    """exactly per_row entries per row, random columns, random 256-bit words as values (any word is a legal record)"""
    rng = np.random.default_rng(seed)
    row_ptr = np.arange(n + 1, dtype=np.uint64) * per_row
    cols = rng.integers(0, n, n * per_row, dtype=np.uint32)
    return Csr(n, n, row_ptr, cols, rng.bytes(32 * n * per_row))


def stack(mats, rows_each):
    """[A; B; C]: the matrices one under the other, each padded with empty rows to rows_each (lists only)"""
    row_ptr, cols, vals = [0], [], b""
    for mt in mats:
        base = row_ptr[-1]
        row_ptr += [base + p for p in mt.row_ptr[1:]] + [base + mt.row_ptr[-1]] * (rows_each - mt.n_rows)
        cols += list(mt.col_idx)
        vals += mt.values
    return Csr(rows_each * len(mats), mats[0].n_cols, row_ptr, cols, vals)
