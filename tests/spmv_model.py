"""Integer model of the sparse witness products (spmv_kernel, spmv_items_kernel, spmv_rows_kernel of csrc/spmv.hip) and the
fixtures their tests share.  Python integers, numpy and oracle.pyref only: nothing of the package is imported, so the cutter,
the products and the thresholds below are restated here and pinned against the package on the CPU (tests/test_spmv_model.py).

The three thresholds.  A row with more than LONG_ROW entries leaves the lane-per-row kernel; the host cuts it into work items
of at most ITEM entries.  One workgroup of THREADS lanes walks an item with stride THREADS, so an item of THREADS + 1 entries
is the first that makes a lane loop twice; one workgroup of THREADS lanes adds a row's partial sums with the same stride, so
a row of THREADS + 1 items (more than THREADS * ITEM = 2^20 entries under the production cut) is the first that strides."""

import random

import numpy as np

from oracle import pyref

LONG_ROW = 64      # zksnake_amd.spmv.LONG_ROW
ITEM = 4096        # zksnake_amd.spmv.ITEM
THREADS = 256      # SPMV_LONG_THREADS, and the block of the lane kernel


# ---- limbs <-> integers (four little-endian 64-bit words per element) ------------------------------------------------------
def to_limbs(values):
    return np.array([[(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in values], dtype=np.uint64).reshape(-1, 4)


def from_limbs(arr):
    return [sum(int(x) << (64 * i) for i, x in enumerate(row)) for row in np.asarray(arr).reshape(-1, 4)]


def row_ptr_of(lengths):
    rp = np.zeros(len(lengths) + 1, dtype=np.uint32)
    np.cumsum(np.asarray(lengths, dtype=np.int64), out=rp[1:])
    return rp


# ---- the product ------------------------------------------------------------------------------------------------------------
def dot_csr(row_ptr, cols, vals, w, r):
    """out[i] = sum_{k in [row_ptr[i], row_ptr[i+1])} vals[k] * w[cols[k]] mod r, everything as Python integers"""
    out = []
    for i in range(len(row_ptr) - 1):
        acc = 0
        for k in range(int(row_ptr[i]), int(row_ptr[i + 1])):
            acc += int(vals[k]) * int(w[int(cols[k])])
        out.append(acc % r)
    return out


def cut(row_ptr, long_row=LONG_ROW, item=ITEM):
    """(long_rows, item_ptr, items) as zk_spmv_long_dev takes them: the rows with more than `long_row` entries in row order,
    each tiled exactly by entry ranges [k0, k1) of at most `item` entries (all but a row's last one hold `item`);
    items[item_ptr[j]:item_ptr[j + 1]] belong to long_rows[j]"""
    long_rows, item_ptr, items = [], [0], []
    for i in range(len(row_ptr) - 1):
        k0, k1 = int(row_ptr[i]), int(row_ptr[i + 1])
        if k1 - k0 <= long_row:
            continue
        long_rows.append(i)
        while k0 < k1:
            items.append((k0, min(k0 + item, k1)))
            k0 += item
        item_ptr.append(len(items))
    return (np.array(long_rows, dtype=np.uint32), np.array(item_ptr, dtype=np.uint32),
            np.array(items, dtype=np.uint32).reshape(-1, 2))


# ---- matrices ---------------------------------------------------------------------------------------------------------------
def _value(rnd, r):
    return (1, r - 1, rnd.randrange(r))[rnd.randrange(3)]


def matrix(lengths, n_col, r, seed):
    """(row_ptr uint32, cols uint32, vals list of ints, w list of ints): rows of the given lengths, columns drawn with
    repetition (a row holds duplicate columns as soon as it is longer than a few entries), columns 0 and n_col - 1 forced to
    occur, values from {1, r - 1, random}; w holds 0, 1 and r - 1 among random elements"""
    rnd = random.Random(seed)
    row_ptr = row_ptr_of(lengths)
    nnz = int(row_ptr[-1])
    cols = [rnd.randrange(n_col) for _ in range(nnz)]
    if nnz:
        cols[0] = 0
        cols[-1] = n_col - 1
    vals = [_value(rnd, r) for _ in range(nnz)]
    w = [rnd.randrange(r) for _ in range(n_col)]
    for pos, v in zip(rnd.sample(range(n_col), min(3, n_col)), (0, 1, r - 1)):
        w[pos] = v
    return row_ptr, np.array(cols, dtype=np.uint32), vals, w


def periodic_row(n, r):
    """(row_ptr, cols, vals limbs (n, 4), w ints, expected): one row of n entries, entry k with value t[k % 5] and column
    k % 7.  The pair (k % 5, k % 7) has period 35, so the sum is the 35-term closed form sum_j count_j t[j % 5] w[j % 7] with
    count_j = #{k < n: k % 35 == j}; the arrays are tiled, 2^20 entries cost nothing"""
    rnd = random.Random(35)
    t = [1, r - 1, rnd.randrange(r), rnd.randrange(r), 2]
    w = [rnd.randrange(r), 1, r - 1, rnd.randrange(r), 0, rnd.randrange(r), rnd.randrange(r)]
    reps = -(-n // 35)
    j = np.arange(35)
    cols = np.tile((j % 7).astype(np.uint32), reps)[:n]
    vals = np.tile(to_limbs(t)[j % 5], (reps, 1))[:n]
    expected = sum((n // 35 + (1 if jj < n % 35 else 0)) * t[jj % 5] * w[jj % 7] for jj in range(35)) % r
    return np.array([0, n], dtype=np.uint32), np.ascontiguousarray(cols), np.ascontiguousarray(vals), w, expected


# ---- a satisfiable R1CS whose forward matrices have long rows, duplicate entries and unsorted triplets ----------------------
N_FREE = 300
SKEWED_LENGTHS = [0, 1, LONG_ROW, LONG_ROW + 1, ITEM, ITEM + 1, 2 * ITEM + 1, 2, THREADS - 1, THREADS, THREADS + 1]
SKEWED_ROWS = len(SKEWED_LENGTHS)      # 11 constraints, padded to 16 by QAP.from_r1cs
SKEWED_PADDED = 16
SKEWED_COLS = N_FREE + SKEWED_ROWS     # 311 wires
SKEWED_PUBLIC = 3
ZERO_WIRE, MINUS_ONE_WIRE = 5, 7


def skewed_circuit(r, seed=1):
    """(A, B, C, n_row, n_col, n_public, witness) in the shape of pyref.readme_circuit, with n_row = 11 (pass SKEWED_PADDED to
    the oracle's transforms).  300 free wires (wire 0 is the constant 1, wire 5 is 0, wire 7 is r - 1, the rest random); row j
    of A has SKEWED_LENGTHS[j] entries, B the same list rotated by three, columns drawn with repetition from the free wires and
    values from {1, r - 1, random}; row j of C is the single entry (j, 300 + j, r - 1) and wire 300 + j = -a_j b_j, so that
    a_j b_j = c_j.  The triplets are shuffled."""
    rnd = random.Random(seed)
    w = [rnd.randrange(r) for _ in range(N_FREE)]
    w[0], w[ZERO_WIRE], w[MINUS_ONE_WIRE] = 1, 0, r - 1

    def side(lengths):
        trip = []
        for j, n in enumerate(lengths):
            trip += [(j, rnd.randrange(N_FREE), _value(rnd, r)) for _ in range(n)]
        return trip

    A = side(SKEWED_LENGTHS)
    B = side(SKEWED_LENGTHS[3:] + SKEWED_LENGTHS[:3])
    a = pyref.sparse_dot(A, SKEWED_ROWS, w, r)
    b = pyref.sparse_dot(B, SKEWED_ROWS, w, r)
    C = [(j, N_FREE + j, r - 1) for j in range(SKEWED_ROWS)]
    w += [(-a[j] * b[j]) % r for j in range(SKEWED_ROWS)]
    for m in (A, B, C):
        rnd.shuffle(m)
    return A, B, C, SKEWED_ROWS, SKEWED_COLS, SKEWED_PUBLIC, w


def column_sums(triplets, n_col, x, r):
    """the transposed product: out[c] = sum over entries (row, c, v) of v * x[row] mod r"""
    out = [0] * n_col
    for row, col, v in triplets:
        out[col] += v * x[row]
    return [s % r for s in out]
