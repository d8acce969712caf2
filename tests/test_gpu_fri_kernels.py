"""GPU: the three entry points of csrc/fri.hip against the integer model (tests/fri_model.py) and direct evaluation, compared
with ==: the fold at every small size in full, at one and two workgroups, and at the first size where a thread takes a second
grid-stride item (closed form on a degree-3 polynomial); the low-degree extension against Horner's rule; the row gather on
repeated, first, last and out-of-range indices; and each of them on a busy stream, in the manner of
tests/test_gpu_stream_state_protocols.py.

The extension at and past the capped grid of 2^18 threads (1024 workgroups of 256), whole d_out and whole d_work against the CPU
oracle's transform of c[i] shift^i (a running product in Python integers), the reference itself spot-checked by Horner's rule.
Coefficients are uniform below r, with 0 and r - 1 at index 0, at 2^18 - 1, at 2^18 and at the last coefficient, and nonzero
elements lie behind the coefficients in device memory, which a loose guard would read.  One test item per field and size:
  N = 2^18, 2^17 - 3 coefficients   the largest size with one item per thread: a thread's seed power uses all 18 squarings, and the
                                    transform under the scale pass is a multi-pass one;
  N = 2^19, 2^18 coefficients       the first second item of the scale pass, stepped by shift^(2^18) for a random full-width
                                    shift; every second item is padding and must be written as zero (so the stepped
                                    power itself multiplies nothing here: the two sizes below are the ones that see it);
  N = 2^20, 2^18 + 5 coefficients   second items that hold a coefficient for threads 0..4 only, so the guard i < n_coeffs acts
                                    inside a second item; the first second trip of the permutation (N/2 = 2^19 pairs);
  N = 2^20, 2^19 - 1 coefficients   every second item but the last holds a coefficient.
(2^18 coefficients at blowup 4, N = 2^20, is the reference of tests/test_gpu_fri.py's end-to-end run and is built here too.)

The row gather past one grid and at both ends of row_bytes, with out-of-range indices, the first, the last and a repeated row
among the first eight and the last eight queries (the last ones are those a second item serves):
  row_bytes = 64, 300 rows, k = 2^16 + 1        2^18 + 4 chunks: threads 0..3 take a second item;
  row_bytes = 16, 1 and 5 rows, k = 2^18 + 3    the smallest row, one chunk per row, three second items;
  row_bytes = 65536, 3 rows, k = 65             the largest row: 266 240 chunks, e / chunks divides by 4096."""

import random
from collections import namedtuple

import numpy as np
import pytest

import fri_model as M
from oracle import corc
from stream_state_child import I, L, behind_spin, one, settle, staged, vals
from zksnake_amd import _native as N
from zksnake_amd.device import DeviceBuffer

pytestmark = pytest.mark.gpu

FIELDS = (("BN254", 0), ("BLS12_381", 1))
per_field = pytest.mark.parametrize("curve,cid", FIELDS, ids=[f[0] for f in FIELDS])


def field(curve):
    cv = M.CURVES[curve][1]
    return cv, cv.r


def read(buf, n):
    return I(buf.download((n, 4)))


def fold_dev(gpu, cid, r, s, w, alpha, layer_buf, log_m, out_buf, stream=None):
    N.check(gpu.zk_fri_fold_dev(cid, log_m, layer_buf.ptr, one(alpha * pow(2 * s, -1, r) % r), one(pow(w, -1, r)), out_buf.ptr, stream))


# ---- fold -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_m", [1, 2, 3, 9, 10])
@per_field
def test_fold_in_full(gpu, curve, cid, log_m):
    """every output of a layer with 0 and r - 1 among its values, for alpha in {0, 1, r - 1, random}; the output buffer is one
    element longer than the folded layer and that element must keep its pre-fill"""
    cv, r = field(curve)
    m = 1 << log_m
    s, w = cv.fr_gen, cv.root_of_unity(m)
    layer = vals(r, m, 40 + log_m)
    layer[0], layer[m - 1] = r - 1, 0
    if m >= 8:
        layer[2], layer[3] = r - 1, r - 1      # a pair of equal values, and one whose sum wraps
    d_layer = DeviceBuffer.from_numpy(L(layer))
    for alpha in (0, 1, r - 1, vals(r, 3, 50 + log_m)[0]):
        d_out = DeviceBuffer.from_numpy(L([7] * (m // 2 + 1)))
        fold_dev(gpu, cid, r, s, w, alpha, d_layer, log_m, d_out)
        assert read(d_out, m // 2 + 1) == M.fold_on(r, s, w, layer, alpha) + [7], f"alpha = {alpha}"
    assert read(d_layer, m) == layer, "the fold wrote to its input"


@per_field
def test_fold_at_the_first_second_item_per_thread(gpu, curve, cid):
    """log M = 20, h = 2^19: the layer is the extension of c0 + c1 X + c2 X^2 + c3 X^3 (from the CPU oracle's transform, not from
    this file's kernels), so the folded layer is (c0 + alpha c1) + (c2 + alpha c3) y at y_j = s^2 w^(2j)"""
    cv, r = field(curve)
    log_m, m = 20, 1 << 20
    h = m // 2
    s, w = cv.fr_gen, cv.root_of_unity(m)
    c = vals(r, 5, 60)[:4]
    alpha = vals(r, 3, 61)[0]
    scaled = np.zeros((m, 4), dtype=np.uint64)
    scaled[:4] = L([c[i] * pow(s, i, r) % r for i in range(4)])
    natural = corc.ntt(cid, scaled, threads=8)
    for i in (0, 1, h - 1, h, m - 1):
        assert I(natural[i:i + 1])[0] == M.poly_eval(c, s * pow(w, i, r) % r, r)
    pairs = np.empty_like(natural)
    pairs[0::2], pairs[1::2] = natural[:h], natural[h:]
    d_layer, d_out = DeviceBuffer.from_numpy(pairs), DeviceBuffer(h * 32)
    d_out.zero()
    fold_dev(gpu, cid, r, s, w, alpha, d_layer, log_m, d_out)
    got = d_out.download((h, 4))
    rnd = random.Random(62)
    a0, a1 = (c[0] + alpha * c[1]) % r, (c[2] + alpha * c[3]) % r
    for j in [0, 1, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, h // 2 - 1, h // 2, h - 1] + [rnd.randrange(h) for _ in range(4096)]:
        pos = 2 * j if j < h // 2 else 2 * (j - h // 2) + 1
        y = s * s % r * pow(w, 2 * j, r) % r
        assert I(got[pos:pos + 1])[0] == (a0 + a1 * y) % r, f"j = {j}"


# ---- low-degree extension -------------------------------------------------------------------------------------------------

def direct_lde(cv, coeffs, log_size):
    """pair order of the polynomial at g w^i, i < 2^log_size, by Horner's rule; also the natural order"""
    r, size = cv.r, 1 << log_size
    w = cv.root_of_unity(size)
    natural = [M.poly_eval(coeffs, cv.fr_gen * pow(w, i, r) % r, r) for i in range(size)]
    return M.pair_order(natural), natural


@pytest.mark.parametrize("log_b", [1, 2, 4])
@pytest.mark.parametrize("log_n", [0, 1, 4])
@per_field
def test_lde_against_direct_evaluation(gpu, curve, cid, log_n, log_b):
    cv, r = field(curve)
    n, log_size = 1 << log_n, log_n + log_b
    size = 1 << log_size
    full = vals(r, max(n, 3), 70 + log_n)[:n]
    for count in sorted({n, n - 1, n // 2, 0}):
        coeffs = full[:count]
        d_coeffs = DeviceBuffer.from_numpy(L(coeffs)) if count else None
        d_work, d_out = DeviceBuffer.from_numpy(L([9] * size)), DeviceBuffer.from_numpy(L([9] * (size + 1)))
        N.check(gpu.zk_fri_lde_dev(cid, log_n, log_b, count, d_coeffs.ptr if count else None, one(cv.fr_gen), d_work.ptr, d_out.ptr, None))
        want, natural = direct_lde(cv, coeffs, log_size)
        assert read(d_out, size + 1) == want + [9], f"{count} coefficients"
        assert read(d_work, size) == natural
        if count:
            assert read(d_coeffs, count) == coeffs


@per_field
def test_lde_equals_the_model_past_one_workgroup(gpu, curve, cid):
    """2^10 evaluations (four workgroups in the scale pass, two in the permutation) of 200 coefficients under log_n = 8"""
    cv, r = field(curve)
    P = M.Params(curve, 8, 2, 0, 1)
    coeffs = vals(r, 200, 80)
    d_coeffs, d_work, d_out = DeviceBuffer.from_numpy(L(coeffs)), DeviceBuffer(P.N * 32), DeviceBuffer(P.N * 32)
    N.check(gpu.zk_fri_lde_dev(cid, 8, 2, 200, d_coeffs.ptr, one(P.g), d_work.ptr, d_out.ptr, None))
    assert read(d_out, P.N) == M.lde(P, coeffs)


# ---- the extension at and past one grid -----------------------------------------------------------------------------------

EDGE = 1 << 18   # threads of the capped grid: the stride of a second item
# case: (log_n, log_b, coefficients, seed of a random shift or None for the field's generator)
LDE_CASES = {
    "one-item-2^18": (17, 1, (1 << 17) - 3, None),
    "padding-2^19": (18, 1, EDGE, 139),
    "guard-2^20": (19, 1, EDGE + 5, None),
    "full-2^20": (19, 1, (1 << 19) - 1, None),
    "commit-2^20": (18, 2, EDGE, None),   # tests/test_gpu_fri.py
}
LdeReference = namedtuple("LdeReference", "size shift coeffs limbs natural pairs")
_LDE_REFERENCES = {}   # (curve, case) -> LdeReference, built once and read-only


def lde_reference(curve, case):
    """the extension of the case's polynomial from Python integers and the CPU oracle's transform; nothing of csrc/fri.hip"""
    if (curve, case) in _LDE_REFERENCES:
        return _LDE_REFERENCES[curve, case]
    log_n, log_b, count, shift_seed = LDE_CASES[case]
    cid = M.CURVES[curve][0]
    cv, r = field(curve)
    size = 1 << (log_n + log_b)
    h = size // 2
    shift = cv.fr_gen if shift_seed is None else vals(r, 3, shift_seed)[0]
    assert shift % r not in (0, 1) and pow(shift, EDGE, r) != 1, "a step of 1 would hide a wrong step"
    coeffs = vals(r, count, 130 + list(LDE_CASES).index(case))
    marks = sorted(i for i in {0, EDGE - 1, EDGE, count - 1} if i < count)
    for pos, i in enumerate(reversed(marks)):   # the last coefficient is r - 1: nonzero, so a guard one short shows
        coeffs[i] = 0 if pos % 2 else r - 1
    scaled, t = [0] * count, 1
    for i, c in enumerate(coeffs):
        scaled[i] = c * t % r
        t = t * shift % r
    padded = np.zeros((size, 4), dtype=np.uint64)
    padded[:count] = L(scaled)
    natural = corc.ntt(cid, padded, threads=8)
    w = cv.root_of_unity(size)
    for i in (0, 1, h - 1, h, size - 1):
        assert I(natural[i:i + 1])[0] == M.poly_eval(coeffs, shift * pow(w, i, r) % r, r), f"the reference is wrong at {i}"
    pairs = np.empty_like(natural)
    pairs[0::2], pairs[1::2] = natural[:h], natural[h:]
    limbs = L(coeffs)
    for a in (limbs, natural, pairs):
        a.setflags(write=False)
    _LDE_REFERENCES[curve, case] = LdeReference(size, shift, coeffs, limbs, natural, pairs)
    return _LDE_REFERENCES[curve, case]


def same_limbs(got, want, what):
    diff = np.flatnonzero((got != want).any(axis=1))
    assert diff.size == 0, f"{what}: {diff.size} of {want.shape[0]} elements differ, the first at {diff[0]} (2^18 = {EDGE})"


@pytest.mark.parametrize("case", [c for c in LDE_CASES if c != "commit-2^20"])
@per_field
def test_lde_at_and_past_one_grid(gpu, curve, cid, case):
    """whole d_out (pair order) and whole d_work (natural order) against the oracle's transform; eight nonzero elements lie behind
    the coefficients, d_out is one element longer than the extension and that element keeps its pre-fill"""
    log_n, log_b, count, _ = LDE_CASES[case]
    r = field(curve)[1]
    ref = lde_reference(curve, case)
    size = ref.size
    behind = L([r - 1 - i for i in range(8)])
    held = np.concatenate([ref.limbs, behind])
    d_coeffs = DeviceBuffer.from_numpy(held)
    d_work = DeviceBuffer.from_numpy(np.full((size, 4), 9, dtype=np.uint64))
    d_out = DeviceBuffer.from_numpy(np.full((size + 1, 4), 9, dtype=np.uint64))
    N.check(gpu.zk_fri_lde_dev(cid, log_n, log_b, count, d_coeffs.ptr, one(ref.shift), d_work.ptr, d_out.ptr, None))
    got = d_out.download((size + 1, 4))
    same_limbs(got[:size], ref.pairs, "d_out")
    assert (got[size] == 9).all(), "the element behind d_out was written"
    same_limbs(d_work.download((size, 4)), ref.natural, "d_work")
    assert (d_coeffs.download(held.shape) == held).all(), "the extension wrote to its coefficients"


# ---- row gather -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row_bytes", [64, 48])
@pytest.mark.parametrize("k", [0, 1, 257])
def test_rows(gpu, k, row_bytes):
    n_rows = 300
    rng = np.random.default_rng(90 + k)
    rows = rng.integers(0, 256, size=(n_rows, row_bytes), dtype=np.uint8)
    idx = rng.integers(0, n_rows, size=k, dtype=np.uint64)
    if k == 1:
        idx[0] = n_rows - 1
    if k > 8:
        idx[:8] = [0, n_rows - 1, 5, 5, 5, n_rows, 1 << 63, 0]    # first, last, repeated, two out of range
    fill = np.full((k + 1, row_bytes), 0xEE, dtype=np.uint8)
    d_rows, d_out = DeviceBuffer.from_numpy(rows), DeviceBuffer.from_numpy(fill)
    d_idx = DeviceBuffer.from_numpy(idx if k else np.zeros(1, dtype=np.uint64))
    N.check(gpu.zk_fri_rows_dev(n_rows, row_bytes, d_rows.ptr, k, d_idx.ptr, d_out.ptr, None))
    got = d_out.download((k + 1, row_bytes), np.uint8)
    want = rows[np.minimum(idx, np.uint64(n_rows - 1)).astype(np.int64)]
    assert (got[:k] == want).all() and (got[k] == 0xEE).all()
    assert (d_rows.download((n_rows, row_bytes), np.uint8) == rows).all()


@pytest.mark.parametrize("row_bytes,rows_of,k", [(64, (300,), (1 << 16) + 1), (16, (1, 5), EDGE + 3), (65536, (3,), 65)],
                         ids=["64-bytes", "16-bytes", "65536-bytes"])
def test_rows_past_one_grid(gpu, row_bytes, rows_of, k):
    """k * chunks > 2^18: the last query (the last three at 16 bytes) is served by a thread's second item and is not row 0"""
    chunks = row_bytes // 16
    assert EDGE < k * chunks <= EDGE + 8 * chunks
    for n_rows in rows_of:
        rng = np.random.default_rng(95 + n_rows + row_bytes)
        rows = rng.integers(0, 256, size=(n_rows, row_bytes), dtype=np.uint8)
        idx = rng.integers(0, n_rows, size=k, dtype=np.uint64)
        last, mid = n_rows - 1, n_rows // 2
        idx[:8] = [0, last, mid, mid, mid, n_rows, 1 << 63, 0]      # first, last, repeated, two out of range
        idx[-8:] = [0, mid, mid, 0, n_rows, 1 << 63, mid, last]
        fill = np.full((k + 1, row_bytes), 0xEE, dtype=np.uint8)
        d_rows, d_out, d_idx = DeviceBuffer.from_numpy(rows), DeviceBuffer.from_numpy(fill), DeviceBuffer.from_numpy(idx)
        N.check(gpu.zk_fri_rows_dev(n_rows, row_bytes, d_rows.ptr, k, d_idx.ptr, d_out.ptr, None))
        got = d_out.download((k + 1, row_bytes), np.uint8)
        want = rows[np.minimum(idx, np.uint64(n_rows - 1)).astype(np.int64)]
        wrong = np.flatnonzero((got[:k] != want).any(axis=1))
        assert wrong.size == 0, f"{n_rows} rows: {wrong.size} of {k} queries differ, the first is query {wrong[0]}"
        assert (got[k] == 0xEE).all(), f"{n_rows} rows: the row behind the output was written"
        assert (d_rows.download((n_rows, row_bytes), np.uint8) == rows).all(), f"{n_rows} rows: the gather wrote to its rows"
        assert (d_idx.download((k,)) == idx).all()


# ---- on a busy stream -----------------------------------------------------------------------------------------------------

@per_field
def test_fold_on_a_busy_stream(gpu, curve, cid):
    cv, r = field(curve)
    log_m, m = 10, 1 << 10
    s, w, alpha = cv.fr_gen, cv.root_of_unity(m), vals(r, 3, 100)[0]
    stale, real = vals(r, m, 101), vals(r, m, 102)
    layer = staged(stale, real)
    d_out = DeviceBuffer.from_numpy(L([7] * (m // 2)))
    got = behind_spin(gpu, [layer], lambda st: fold_dev(gpu, cid, r, s, w, alpha, layer, log_m, d_out, st), lambda: read(d_out, m // 2))
    settle(got, M.fold_on(r, s, w, real, alpha), M.fold_on(r, s, w, stale, alpha))


@per_field
def test_lde_on_a_busy_stream(gpu, curve, cid):
    """the scale pass, the transform and the permutation all run behind the upload of the coefficients"""
    cv, r = field(curve)
    P = M.Params(curve, 8, 2, 0, 1)
    stale, real = vals(r, P.n, 110), vals(r, P.n, 111)
    coeffs = staged(stale, real)
    d_work, d_out = DeviceBuffer(P.N * 32), DeviceBuffer.from_numpy(L([7] * P.N))
    got = behind_spin(gpu, [coeffs], lambda st: N.check(gpu.zk_fri_lde_dev(cid, 8, 2, P.n, coeffs.ptr, one(P.g), d_work.ptr, d_out.ptr, st)),
                      lambda: read(d_out, P.N))
    settle(got, M.lde(P, real), M.lde(P, stale))


def test_rows_on_a_busy_stream(gpu):
    from stream_state_child import Staged
    rng = np.random.default_rng(120)
    n_rows, k = 300, 257
    rows = Staged(rng.integers(0, 256, size=(n_rows, 64), dtype=np.uint8), rng.integers(0, 256, size=(n_rows, 64), dtype=np.uint8))
    idx = Staged(rng.integers(0, n_rows, size=k, dtype=np.uint64), rng.integers(0, n_rows, size=k, dtype=np.uint64))
    d_out = DeviceBuffer.from_numpy(np.full((k, 64), 0xEE, dtype=np.uint8))
    got = behind_spin(gpu, [rows, idx], lambda st: N.check(gpu.zk_fri_rows_dev(n_rows, 64, rows.ptr, k, idx.ptr, d_out.ptr, st)),
                      lambda: d_out.download((k, 64), np.uint8))
    on_real = rows.pin.array[idx.pin.array.astype(np.int64)]
    assert (got == on_real).all(), "differs from the rows and indices uploaded behind the spin"
