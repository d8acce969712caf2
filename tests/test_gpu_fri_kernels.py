"""GPU: the three entry points of csrc/fri.hip against the integer model (tests/fri_model.py) and direct evaluation, compared
with ==: the fold at every small size in full, at one and two workgroups, and at the first size where a thread takes a second
grid-stride item (closed form on a degree-3 polynomial); the low-degree extension against Horner's rule; the row gather on
repeated, first, last and out-of-range indices; and each of them on a busy stream, in the manner of
tests/test_gpu_stream_state_protocols.py."""

import random

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
