"""GPU: the state AROUND the Fr kernels -- stream discipline of every entry point that takes a stream, twiddle-table growth
with work queued on the old table, per-stream scratch (regrow, two streams, destroyed streams), zk_shutdown.

Technique (no race is hoped for): streams of zk_stream_create are non-blocking, zk_debug_spin_dev parks one, and an input
that arrives by zk_dev_upload_async from page-locked memory behind the spin exists on the device only for work ordered on
that stream.  The device buffer holds another valid pattern P until then, so any launch, copy or memset that a wrapper
puts on another stream computes on P: a wrong value, never a fault.  Expectations are the CPU oracle (oracle/corc.py) or the
integer models of tests/, compared with ==.

"In flight" is asserted: parked() measures the spin alone (D); wherever another stream (or the host) works while a stream is
parked, the host time from queueing the spin to the end of that work must stay below D.
  Spin requests 200 ms and 20 ms (stream_state_child.SPIN_US, SPIN_SHORT_US); D for both on an MI355X is in EXPERIMENTS.md,
  "Stream-state tests".

Sizes: 2^12 = first size with scratch (two passes), 2^16 = largest on the initial 16-stage table (a QAP there needs stage
17), 2^17 = first growth for a plain transform and first three-pass plan (two scratch vectors).  Nothing is larger."""

import ctypes
import json
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

import mle_model as M
import stream_state_child as S
from oracle import corc
from stream_state_child import I, L, behind_spin, host4, one, settle, staged, vals
from zksnake_amd import _native as N
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD
from zksnake_amd.device import DeviceBuffer

pytestmark = pytest.mark.gpu

T = N.MLE_TILE_LOG
FIELDS = (("BN254", 0, BN254_SCALAR_FIELD), ("BLS12_381", 1, BLS12_381_SCALAR_FIELD))
FIELD_IDS = [f[0] for f in FIELDS]
per_field = pytest.mark.parametrize("name,cid,p", FIELDS, ids=FIELD_IDS)
_REF = {}


# ---- inputs and plumbing ------------------------------------------------------------------------------------------------

def ref_ntt(cid, log_n, seed, inverse=False):
    """(input limbs, oracle output): computed once, shared, never modified"""
    key = ("ntt", cid, log_n, seed, inverse)
    if key not in _REF:
        x = S.rand_limbs(1 << log_n, 1000 * log_n + 10 * seed + cid)
        _REF[key] = (x, corc.ntt(cid, x, inverse=inverse, threads=8))
    return _REF[key]


def ref_qap(cid, log_n, seed):
    key = ("qap", cid, log_n, seed)
    if key not in _REF:
        _REF[key] = S.qap_inputs(cid, log_n, 5000 + 100 * log_n + 10 * seed + cid)
    return _REF[key]


# ---- A.1: upload behind a spin, then compute ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 257, 4096, (1 << 16) + 1])
@per_field
def test_mle_sum_on_a_busy_stream(gpu, name, cid, p, n):
    """any n, not only powers of two; n = 0 reads nothing, so there only the value and the untouched stream are checked"""
    pv, qv = vals(p, max(n, 1), 1), vals(p, max(n, 1), 2)
    x = staged(pv, qv)
    out = host4()
    behind_spin(gpu, [x], lambda st: N.check(gpu.zk_mle_sum_dev(cid, n, x.ptr, N.u64p(out), st)))
    if n == 0:
        assert I(out) == [0]
    else:
        settle(I(out)[0], M.total(qv[:n], p), M.total(pv[:n], p))


@pytest.mark.parametrize("own_work", [True, False], ids=["d_work", "library work"])
@per_field
def test_mle_eval_on_a_busy_stream(gpu, name, cid, p, own_work):
    log_n = T + 4
    pv, qv, point = vals(p, 1 << log_n, 3), vals(p, 1 << log_n, 4), vals(p, log_n, 5)
    x = staged(pv, qv)
    work = DeviceBuffer(32 << (log_n - T + 1)) if own_work else None
    out = host4()
    behind_spin(gpu, [x], lambda st: N.check(gpu.zk_mle_eval_dev(cid, log_n, x.ptr, N.u64p(L(point)), N.u64p(out),
                                                                  work.ptr if work else None, st)))
    settle(I(out)[0], M.evaluate(qv, point, p), M.evaluate(pv, point, p))
    assert I(x.download()) == qv


@pytest.mark.parametrize("k", [1, T + 1], ids=["k=1", "k=9 (library work space)"])
@per_field
def test_mle_fix_on_a_busy_stream(gpu, name, cid, p, k):
    log_n = T + 4
    pv, qv, rs = vals(p, 1 << log_n, 6), vals(p, 1 << log_n, 7), vals(p, k, 8)
    x, out = staged(pv, qv), DeviceBuffer.from_numpy(L(vals(p, 1 << (log_n - k), 9)))
    got = behind_spin(gpu, [x], lambda st: N.check(gpu.zk_mle_fix_dev(cid, log_n, x.ptr, k, N.u64p(L(rs)), out.ptr, st)),
                      lambda: I(out.download((1 << (log_n - k), 4))))
    settle(got, M.fix(qv, rs, p), M.fix(pv, rs, p))


@pytest.mark.parametrize("in_place", [False, True], ids=["out of place", "in place"])
@per_field
def test_mle_coeffs_on_a_busy_stream(gpu, name, cid, p, in_place):
    log_n = T + 4
    pv, qv = vals(p, 1 << log_n, 10), vals(p, 1 << log_n, 11)
    x = staged(pv, qv)
    out = x.dev if in_place else DeviceBuffer.from_numpy(L(pv))
    got = behind_spin(gpu, [x], lambda st: N.check(gpu.zk_mle_coeffs_dev(cid, log_n, x.ptr, out.ptr, st)),
                      lambda: I(out.download((1 << log_n, 4))))
    settle(got, M.coefficients(qv, p), M.coefficients(pv, p))


@per_field
def test_mle_permute_on_a_busy_stream(gpu, name, cid, p):
    log_n = T + 2
    pv, qv = vals(p, 1 << log_n, 12), vals(p, 1 << log_n, 13)
    perm = list(range(log_n))
    random.Random(3).shuffle(perm)
    x, out = staged(pv, qv), DeviceBuffer.from_numpy(L(pv))
    got = behind_spin(gpu, [x], lambda st: N.check(gpu.zk_mle_permute_dev(cid, log_n, x.ptr, N.u8p(np.array(perm, dtype=np.uint8)), out.ptr, st)),
                      lambda: I(out.download((1 << log_n, 4))))
    settle(got, M.permute(qv, perm), M.permute(pv, perm))


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused with the fold"])
@per_field
def test_sumcheck_round_with_eight_tables_and_eight_terms_on_a_busy_stream(gpu, name, cid, p, fused):
    """the ABI maximum of tables and of terms, degrees 1, 2, 3, every table used, one table twice in a term"""
    log_n, nt = T + 1, 8
    n = 1 << log_n
    pt, qt = [vals(p, n, 20 + i) for i in range(nt)], [vals(p, n, 40 + i) for i in range(nt)]
    coeffs = [1, p - 1, 0] + vals(p, 5, 60)
    terms = [(coeffs[t], tuple((t + 3 * j) % nt for j in range(1 + t % 3))) for t in range(nt - 1)] + [(coeffs[7], (7, 7, 0))]
    assert {tb for _, w in terms for tb in w} == set(range(nt))
    r = vals(p, 1, 61)[0]
    tabs = [staged(a, b) for a, b in zip(pt, qt)]
    outs = [DeviceBuffer.from_numpy(L(pt[i][: n // 2])) for i in range(nt)] if fused else None
    arr = ctypes.c_void_p * nt
    deg = (ctypes.c_int * nt)(*[len(w) for _, w in terms])
    idx = (ctypes.c_int * (3 * nt))()
    for t, (_, w) in enumerate(terms):
        for j, tb in enumerate(w):
            idx[3 * t + j] = tb
    s = host4(4)

    def call(st):
        N.check(gpu.zk_sumcheck_round_dev(cid, log_n, nt, arr(*[t.ptr for t in tabs]), nt, N.u64p(L([c for c, _ in terms])), deg, idx,
                                          one(r) if fused else None, arr(*[o.ptr for o in outs]) if fused else None, N.u64p(s), st))

    def model(tables):
        if not fused:
            return M.round_sums(tables, terms, p), None
        folded = [M.fix(t, [r], p) for t in tables]
        return M.round_sums(folded, terms, p), folded

    got = behind_spin(gpu, tabs, call, lambda: (I(s), [I(o.download((n // 2, 4))) for o in outs] if fused else None))
    settle(got, model(qt), model(pt))
    assert all(I(t.download()) == q for t, q in zip(tabs, qt)), "an input table was modified"


def horner(c, x, p):
    acc = 0
    for v in reversed(c):
        acc = (acc * x + v) % p
    return acc


@per_field
def test_poly_eval_and_eval_many_on_a_busy_stream(gpu, name, cid, p):
    counts = [1000, 37, 1]
    pv, qv = [vals(p, c, 70 + i) for i, c in enumerate(counts)], [vals(p, c, 80 + i) for i, c in enumerate(counts)]
    xs = vals(p, 3, 90)
    cs = [staged(a, b) for a, b in zip(pv, qv)]
    out = host4()
    behind_spin(gpu, cs[:1], lambda st: N.check(gpu.zk_poly_eval_dev(cid, counts[0], cs[0].ptr, one(xs[0]), N.u64p(out), st)))
    settle(I(out)[0], horner(qv[0], xs[0], p), horner(pv[0], xs[0], p))
    for c, a in zip(cs, pv):
        c.dev.upload(L(a))
    outs = host4(3)
    behind_spin(gpu, cs, lambda st: N.check(gpu.zk_poly_eval_many_dev(cid, 3, N.u64p(np.array(counts, dtype=np.uint64)),
                                                                       (N._vp * 3)(*[c.ptr for c in cs]), N.u64p(L(xs)), N.u64p(outs), st)))
    settle(I(outs), [horner(c, x, p) for c, x in zip(qv, xs)], [horner(c, x, p) for c, x in zip(pv, xs)])


def grand_product(num, den, p):
    acc, out = 1, [1]
    for a, b in zip(num, den):
        acc = acc * a * pow(b, -1, p) % p
        out.append(acc)
    return out


@per_field
def test_grand_product_on_a_busy_stream(gpu, name, cid, p):
    n = 1000
    nz = lambda v: [x or 1 for x in v]  # noqa: E731
    pn, qn, pd, qd = nz(vals(p, n, 100)), nz(vals(p, n, 101)), nz(vals(p, n, 102)), nz(vals(p, n, 103))
    num, den, out = staged(pn, qn), staged(pd, qd), DeviceBuffer.from_numpy(L(vals(p, n + 1, 104)))
    got = behind_spin(gpu, [num, den], lambda st: N.check(gpu.zk_plonk_grand_product_dev(cid, n, num.ptr, den.ptr, out.ptr, st)),
                      lambda: I(out.download((n + 1, 4))))
    settle(got, grand_product(qn, qd, p), grand_product(pn, pd, p))


def div_linear(c, root, p):
    q, carry = [0] * (len(c) - 1), 0
    for i in range(len(c) - 1, 0, -1):
        carry = (c[i] + carry * root) % p
        q[i - 1] = carry
    return q, (c[0] + carry * root) % p


@pytest.mark.parametrize("zero_root", [False, True], ids=["root", "root 0"])
@per_field
def test_div_linear_on_a_busy_stream(gpu, name, cid, p, zero_root):
    n = 1000
    pv, qv = vals(p, n, 110), vals(p, n, 111)
    root = 0 if zero_root else vals(p, 1, 112)[0]
    c, q = staged(pv, qv), DeviceBuffer.from_numpy(L(vals(p, n - 1, 113)))
    rem = host4()
    got = behind_spin(gpu, [c], lambda st: N.check(gpu.zk_poly_div_linear_dev(cid, n, c.ptr, one(root), q.ptr, N.u64p(rem), st)),
                      lambda: (I(q.download((n - 1, 4))), I(rem)[0]))
    settle(got, div_linear(qv, root, p), div_linear(pv, root, p))


@pytest.mark.parametrize("real_is_zero", [False, True], ids=["zero until the upload", "non-zero until the upload"])
@per_field
def test_is_zero_on_a_busy_stream(gpu, name, cid, p, real_is_zero):
    n = 1000
    zero, other = [0] * n, [0] * (n - 1) + [1]
    x = staged(other, zero) if real_is_zero else staged(zero, other)
    flag = ctypes.c_int(-1)
    behind_spin(gpu, [x], lambda st: N.check(gpu.zk_vec_is_zero_dev(cid, n, x.ptr, ctypes.byref(flag), st)))
    settle(flag.value, int(real_is_zero), int(not real_is_zero))


@per_field
def test_axpby_vec_op_and_gather_on_a_busy_stream(gpu, name, cid, p):
    n = 1000
    px, qx, py, qy = vals(p, n, 120), vals(p, n, 121), vals(p, n, 122), vals(p, n, 123)
    a, b, c = vals(p, 3, 124)
    x, y, out = staged(px, qx), staged(py, qy), DeviceBuffer.from_numpy(L(px))
    read = lambda: I(out.download((n, 4)))  # noqa: E731
    got = behind_spin(gpu, [x, y], lambda st: N.check(gpu.zk_vec_axpby_dev(cid, n, one(a), x.ptr, one(b), y.ptr, one(c), out.ptr, st)), read)
    settle(got, [(a * u + b * v + c) % p for u, v in zip(qx, qy)], [(a * u + b * v + c) % p for u, v in zip(px, py)])
    for op, f in enumerate((lambda u, v: u * v % p, lambda u, v: (u + v) % p, lambda u, v: (u - v) % p)):
        x.dev.upload(L(px))
        y.dev.upload(L(py))
        got = behind_spin(gpu, [x, y], lambda st: N.check(gpu.zk_vec_op_dev(cid, op, n, x.ptr, y.ptr, out.ptr, st)), read)
        settle(got, [f(u, v) for u, v in zip(qx, qy)], [f(u, v) for u, v in zip(px, py)])
    x.dev.upload(L(px))
    m = n // 3
    got = behind_spin(gpu, [x], lambda st: N.check(gpu.zk_vec_gather_dev(cid, m, x.ptr, 3, 1, out.ptr, st)), lambda: I(out.download((m, 4))))
    settle(got, qx[1::3][:m], px[1::3][:m])


@per_field
def test_lincomb_on_a_busy_stream(gpu, name, cid, p):
    n, counts = 1000, [1000, 999, 37]
    pa, qa = vals(p, n, 130), vals(p, n, 131)
    pxs, qxs = [vals(p, c, 132 + i) for i, c in enumerate(counts)], [vals(p, c, 136 + i) for i, c in enumerate(counts)]
    sc, at = [p - 1] + vals(p, 2, 140), [(0, p - 1), (n - 1, 5)]
    acc, xs = staged(pa, qa), [staged(a, b) for a, b in zip(pxs, qxs)]

    def call(st):
        N.check(gpu.zk_vec_lincomb_dev(cid, n, acc.ptr, 3, N.u64p(np.array(counts, dtype=np.uint64)), (N._vp * 3)(*[v.ptr for v in xs]),
                                       N.u64p(L(sc)), 2, N.u64p(np.array([i for i, _ in at], dtype=np.uint64)), N.u64p(L([v for _, v in at])), st))

    def model(a, terms):
        out = list(a)
        for c, s, x in zip(counts, sc, terms):
            for i in range(c):
                out[i] = (out[i] + s * x[i]) % p
        for i, v in at:
            out[i] = (out[i] + v) % p
        return out

    settle(behind_spin(gpu, [acc] + xs, call, lambda: I(acc.download())), model(qa, qxs), model(pa, pxs))


@per_field
def test_perm_terms_and_quotient_on_a_busy_stream(gpu, name, cid, p):
    n = 257
    pv, qv = [vals(p, n, 150 + i) for i in range(6)], [vals(p, n, 160 + i) for i in range(6)]
    beta, gamma, alpha = vals(p, 3, 170)
    cols, out = [staged(a, b) for a, b in zip(pv, qv)], DeviceBuffer.from_numpy(L(pv[0]))
    arr = ctypes.c_void_p * 3
    got = behind_spin(gpu, cols, lambda st: N.check(gpu.zk_plonk_perm_terms_dev(cid, n, arr(*[c.ptr for c in cols[:3]]), arr(*[c.ptr for c in cols[3:]]),
                                                                                 one(beta), one(gamma), out.ptr, st)),
                      lambda: I(out.download((n, 4))))

    def terms(v):
        return [(v[0][i] + beta * v[3][i] + gamma) * (v[1][i] + beta * v[4][i] + gamma) * (v[2][i] + beta * v[5][i] + gamma) % p for i in range(n)]

    settle(got, terms(qv), terms(pv))
    # the quotient on a coset of m = 4n points (the formula of include/zkmi.h, k_j = 1, 2, 3)
    nq, k = 128, 4
    m = k * nq
    pq, qq = [vals(p, m, 200 + i) for i in range(15)], [vals(p, m, 220 + i) for i in range(15)]
    zh = vals(p, k, 240)
    qcols, qout = [staged(a, b) for a, b in zip(pq, qq)], DeviceBuffer.from_numpy(L(pq[0]))
    got = behind_spin(gpu, qcols, lambda st: N.check(gpu.zk_plonk_quotient_dev(cid, m, nq, (ctypes.c_void_p * 15)(*[c.ptr for c in qcols]), N.u64p(L(zh)),
                                                                                one(beta), one(gamma), one(alpha), qout.ptr, st)),
                      lambda: I(qout.download((m, 4))))

    def quotient(v):
        a, b, c, z, pi, ql, qr, qo, qm, qc, s1, s2, s3, x, l1 = v
        out = []
        for i in range(m):
            gate = a[i] * ql[i] + b[i] * qr[i] + c[i] * qo[i] + a[i] * b[i] * qm[i] + qc[i] + pi[i]
            left = (a[i] + beta * x[i] + gamma) * (b[i] + 2 * beta * x[i] + gamma) * (c[i] + 3 * beta * x[i] + gamma) * z[i]
            right = (a[i] + beta * s1[i] + gamma) * (b[i] + beta * s2[i] + gamma) * (c[i] + beta * s3[i] + gamma) * z[(i + k) % m]
            out.append((gate + alpha * (left - right) + alpha * alpha * (z[i] - 1) * l1[i]) * zh[i % k] % p)
        return out

    settle(got, quotient(qq), quotient(pq))


@per_field
def test_powers_and_canon_on_a_busy_stream(gpu, name, cid, p):
    """zk_vec_powers_dev reads no device input: here an upload of another pattern INTO ITS OUTPUT is queued behind the spin
    first, so a launch on another stream would be overwritten by it"""
    n = 1000
    g = vals(p, 1, 250)[0]
    pattern = vals(p, n, 251)
    out = staged(vals(p, n, 252), pattern)
    got = behind_spin(gpu, [out], lambda st: N.check(gpu.zk_vec_powers_dev(cid, n, one(g), out.ptr, st)), lambda: I(out.download()))
    settle(got, [pow(g, i, p) for i in range(n)], pattern)
    lift = lambda v: [x + p if i % 2 == 0 and x + p < 1 << 256 else x for i, x in enumerate(v)]  # noqa: E731
    pv, qv = lift(vals(p, n, 253)), lift(vals(p, n, 254))
    qv[5] = (1 << 256) - 1
    x = staged(pv, qv)
    got = behind_spin(gpu, [x], lambda st: N.check(gpu.zk_vec_canon_dev(cid, n, x.ptr, st)), lambda: I(x.download()))
    settle(got, [v % p for v in qv], [v % p for v in pv])


@pytest.mark.parametrize("log_n,inverse", [(12, 0), (12, 1), (16, 0)])
@per_field
def test_ntt_on_a_busy_stream(gpu, name, cid, p, log_n, inverse):
    (px, want_p), (qx, want_q) = ref_ntt(cid, log_n, 1, bool(inverse)), ref_ntt(cid, log_n, 2, bool(inverse))
    x = S.Staged(px, qx)
    got = behind_spin(gpu, [x], lambda st: S.ntt_dev(gpu, cid, inverse, log_n, x.ptr, st), x.download)
    settle(got.tolist(), want_q.tolist(), want_p.tolist())


@pytest.mark.parametrize("form", ["one call", "begin / end", "u and v only"])
@per_field
def test_qap_chain_on_a_busy_stream(gpu, name, cid, p, form):
    log_n = 12
    n = 1 << log_n
    (pabc, puvh), (qabc, quvh) = ref_qap(cid, log_n, 1), ref_qap(cid, log_n, 2)
    a, b, c = (S.Staged(x, y) for x, y in zip(pabc, qabc))
    h, work = DeviceBuffer.from_numpy(pabc[0]), DeviceBuffer(4 * n * 32)
    ok, ev = N._i(-1), N._vp()

    def call(st):
        if form == "one call":
            N.check(gpu.zk_qap_h_dev(cid, log_n, a.ptr, b.ptr, c.ptr, h.ptr, work.ptr, ok, st))
        elif form == "begin / end":
            N.check(gpu.zk_qap_h_dev_begin(cid, log_n, a.ptr, b.ptr, c.ptr, h.ptr, work.ptr, st, ctypes.byref(ev)))
            N.check(gpu.zk_qap_h_dev_end(cid, log_n, work.ptr, ok, st))
        else:
            N.check(gpu.zk_qap_uv_dev(cid, log_n, a.ptr, b.ptr, st, ctypes.byref(ev)))

    k = 2 if form == "u and v only" else 3
    got = behind_spin(gpu, [a, b, c], call, lambda: [a.download().tolist(), b.download().tolist(), h.download((n, 4)).tolist()][:k])
    settle(got, [x.tolist() for x in quvh[:k]], [x.tolist() for x in puvh[:k]])
    assert (c.download() == qabc[2]).all(), "c was modified"
    if k == 3:
        assert ok.value == 1


@per_field
def test_spmv_short_and_long_rows_on_a_busy_stream(gpu, name, cid, p):
    """the matrix of test_spmv_long_rows (rows of 10000, 65, 64, 2 and 0 entries: both kernels of the long-row path and the
    lane-per-row kernel); the values and the vector arrive behind the spin"""
    from zksnake_amd.array import SparseArray
    from zksnake_amd.spmv import LONG_ROW, DeviceCsr
    rnd = random.Random(11)
    n_row, n_col = 9, 12000
    where = [(0, c) for c in range(10000)] + [(3, c) for c in rnd.sample(range(n_col), LONG_ROW + 1)]
    where += [(5, c) for c in rnd.sample(range(n_col), LONG_ROW)] + [(7, 0), (7, 1)]
    pm, qm = vals(p, len(where), 260), vals(p, len(where), 261)
    pw, qw = vals(p, n_col, 262), vals(p, n_col, 263)
    rows, cols = [r for r, _ in where], [c for _, c in where]
    mats = [SparseArray.from_triplets(rows, cols, v, n_row, n_col, p) for v in (pm, qm)]
    csr_p, csr_q = mats[0].to_csr(), mats[1].to_csr()
    assert (csr_p[0] == csr_q[0]).all() and (csr_p[1] == csr_q[1]).all()
    csr = DeviceCsr(cid, *csr_p)
    assert csr.n_long == 2
    pin = S.PinnedArray(csr_q[2].shape, np.uint64)
    pin.array[...] = csr_q[2]
    w, out = staged(pw, qw), DeviceBuffer.from_numpy(np.full((n_row, 4), 7, dtype=np.uint64))

    class Values:
        def send(self, lib, st):
            N.check(lib.zk_dev_upload_async(csr.vals.ptr, pin.ptr, pin.nbytes, st))

    got = behind_spin(gpu, [Values(), w], lambda st: csr.apply(w.ptr, out.ptr, st), lambda: I(out.download((n_row, 4))))
    settle(got, mats[1].dot(qw), mats[0].dot(pw))


# ---- A.3 - A.5: scratch and tables with work in flight -----------------------------------------------------------------

def warm(gpu, cid, log_n):
    """the twiddle table reaches log_n stages and the default stream's scratch that size, before anything is parked"""
    x, want = ref_ntt(cid, log_n, 9)
    d = DeviceBuffer.from_numpy(x)
    S.ntt_dev(gpu, cid, 0, log_n, d.ptr, None)
    S.sync(gpu, None)
    assert (d.download(x.shape) == want).all()


@per_field
def test_scratch_regrows_on_a_busy_stream(gpu, name, cid, p):
    """a 2^12 transform queued behind a spin holds the stream's first scratch vector; the 2^17 transform queued after it makes
    get_scratch synchronise the stream, free that vector and allocate two larger ones.  Both results are the oracle's, and
    the stream then serves 2^12 again from the larger scratch."""
    warm(gpu, cid, 17)
    (x12, want12), (x17, want17) = ref_ntt(cid, 12, 3), ref_ntt(cid, 17, 3)
    d12, d17 = DeviceBuffer.from_numpy(x12), DeviceBuffer.from_numpy(x17)
    a = S.new_stream(gpu)
    try:
        d, t0 = S.parked(gpu, a)
        S.ntt_dev(gpu, cid, 0, 12, d12.ptr, a)
        t1 = time.perf_counter()
        S.ntt_dev(gpu, cid, 0, 17, d17.ptr, a)      # waits for the spin inside: the regrow synchronises the stream
        S.sync(gpu, a)
        msg = S.in_flight(d, t0, t1, "queueing the 2^12 transform")
        assert msg is None, msg
        assert (d12.download(x12.shape) == want12).all(), "2^12 behind the spin"
        assert (d17.download(x17.shape) == want17).all(), "2^17 after the regrow"
        d12.upload(x12)
        S.ntt_dev(gpu, cid, 0, 12, d12.ptr, a)
        S.sync(gpu, a)
        assert (d12.download(x12.shape) == want12).all(), "2^12 on the grown scratch"
    finally:
        N.check(gpu.zk_stream_destroy(a))


@per_field
def test_transforms_on_two_streams_and_the_default_stream(gpu, name, cid, p):
    """a forward 2^17 on A is still queued behind the spin while B runs a forward and an inverse 2^17 and the default stream a
    forward one, to completion; then both streams are kept busy AT ONCE (16 transforms each, issued alternately, no
    synchronisation in between), which is where scratch shared between streams would be overwritten mid-transform."""
    warm(gpu, cid, 17)
    (x, want_x), (y, want_y), (z, want_zi) = ref_ntt(cid, 17, 4), ref_ntt(cid, 17, 5), ref_ntt(cid, 17, 6, True)
    want_z = ref_ntt(cid, 17, 6)[1]
    dx, dy, dzi, dz = (DeviceBuffer.from_numpy(v) for v in (x, y, z, z))
    a, b = S.new_stream(gpu), S.new_stream(gpu)
    try:
        d, t0 = S.parked(gpu, a)
        S.ntt_dev(gpu, cid, 0, 17, dx.ptr, a)
        S.ntt_dev(gpu, cid, 0, 17, dy.ptr, b)
        S.ntt_dev(gpu, cid, 1, 17, dzi.ptr, b)
        S.ntt_dev(gpu, cid, 0, 17, dz.ptr, None)
        S.sync(gpu, b)
        S.sync(gpu, None)
        t1 = time.perf_counter()
        S.sync(gpu, a)
        msg = S.in_flight(d, t0, t1, "three 2^17 transforms on the other streams")
        print(f"spin {1e3 * d:.2f} ms, other streams done after {1e3 * (t1 - t0):.3f} ms")
        assert msg is None, msg
        for buf, want, what in ((dx, want_x, "A, behind the spin"), (dy, want_y, "B forward"), (dzi, want_zi, "B inverse"), (dz, want_z, "default stream")):
            assert (buf.download(x.shape) == want).all(), what
        # both streams busy at once: 8 x (inverse, forward) brings each vector back to its forward transform
        for _ in range(8):
            for buf, st in ((dx, a), (dy, b)):
                S.ntt_dev(gpu, cid, 1, 17, buf.ptr, st)
                S.ntt_dev(gpu, cid, 0, 17, buf.ptr, st)
        S.sync(gpu, a)
        S.sync(gpu, b)
        assert (dx.download(x.shape) == want_x).all() and (dy.download(x.shape) == want_y).all(), "concurrent transforms"
    finally:
        N.check(gpu.zk_stream_destroy(a))
        N.check(gpu.zk_stream_destroy(b))


@pytest.mark.parametrize("log_n", [12, 16])
@per_field
def test_qap_chains_on_two_streams(gpu, name, cid, p, log_n):
    """_begin on A behind the spin, the one-call form on B with another witness to completion, then _end on A"""
    (abc1, uvh1), (abc2, uvh2) = ref_qap(cid, log_n, 1), ref_qap(cid, log_n, 2)
    S.QapRun(abc2).one_call(gpu, cid, None)     # tables for (curve, log_n) and stage log_n + 1 exist before anything is parked
    r1, r2 = S.QapRun(abc1), S.QapRun(abc2)
    a, b = S.new_stream(gpu), S.new_stream(gpu)
    try:
        d, t0 = S.parked(gpu, a)
        assert r1.begin(gpu, cid, a).value
        r2.one_call(gpu, cid, b)
        t1 = time.perf_counter()
        r1.end(gpu, cid, a)
        msg = S.in_flight(d, t0, t1, f"the QAP chain at 2^{log_n} on the other stream")
        print(f"spin {1e3 * d:.2f} ms, other stream done after {1e3 * (t1 - t0):.3f} ms")
        assert msg is None, msg
        assert r2.matches(uvh2), "one-call form on B"
        assert r1.matches(uvh1), "begin / end on A"
    finally:
        N.check(gpu.zk_stream_destroy(a))
        N.check(gpu.zk_stream_destroy(b))


@per_field
def test_streams_created_after_one_was_destroyed(gpu, name, cid, p):
    """a stream that ran a 2^12 transform and a QAP chain (scratch and an event are kept under its handle) is destroyed; one of
    the next eight streams may be handed the same handle value.  Each runs 2^17, one after another."""
    warm(gpu, cid, 17)
    (x12, want12), (x17, want17) = ref_ntt(cid, 12, 3), ref_ntt(cid, 17, 3)
    abc, uvh = ref_qap(cid, 12, 1)
    old = S.new_stream(gpu)
    d12, run = DeviceBuffer.from_numpy(x12), S.QapRun(abc)
    S.ntt_dev(gpu, cid, 0, 12, d12.ptr, old)
    run.begin(gpu, cid, old)
    run.end(gpu, cid, old)
    assert (d12.download(x12.shape) == want12).all() and run.matches(uvh)
    N.check(gpu.zk_stream_destroy(old))
    streams = [S.new_stream(gpu) for _ in range(8)]
    d17 = DeviceBuffer.from_numpy(x17)
    try:
        for i, st in enumerate(streams):
            d17.upload(x17)
            S.ntt_dev(gpu, cid, 0, 17, d17.ptr, st)
            S.sync(gpu, st)
            assert (d17.download(x17.shape) == want17).all(), f"stream {i} (handle reused: {st.value == old.value})"
        run2 = S.QapRun(abc)
        assert run2.begin(gpu, cid, streams[0]).value
        run2.end(gpu, cid, streams[0])
        assert run2.matches(uvh)
    finally:
        for st in streams:
            N.check(gpu.zk_stream_destroy(st))


# ---- B: scenarios in a process of their own ----------------------------------------------------------------------------

_CHILDREN = {"died": None}
CHILD_TIMEOUT = {"retired_by_ntt": 120, "retired_by_qap": 120, "qap_first": 90, "inverse_first": 90, "shutdown": 150}


def run_child(scenario):
    if _CHILDREN["died"]:
        pytest.fail(f"not started: an earlier child died ({_CHILDREN['died']})")
    cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "stream_state_child.py"), scenario]
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT[scenario])
    except subprocess.TimeoutExpired:
        _CHILDREN["died"] = f"{scenario} hung: no result within {CHILD_TIMEOUT[scenario]} s"
        pytest.fail(_CHILDREN["died"])
    if res.returncode < 0 or res.returncode in (134, 139):
        _CHILDREN["died"] = f"{scenario} exited with {res.returncode}"
        pytest.fail(_CHILDREN["died"] + "\n" + res.stderr[-2000:])
    assert res.returncode == 0, f"{scenario} exited with {res.returncode}\n{res.stderr[-4000:]}"
    report = json.loads(res.stdout.strip().splitlines()[-1])
    assert report["scenario"] == scenario and report["checks"]
    print(json.dumps(report["timing"]))
    failed = [k for k, v in report["checks"].items() if v is not True]
    assert not failed, failed
    return report


@pytest.mark.parametrize("scenario", ["retired_by_ntt", "retired_by_qap"])
def test_child_retired_twiddle_table_stays_readable(gpu, scenario):
    """the table is known to hold 16 stages; a 2^16 transform queued behind a spin on A carries its address while B makes it
    grow (a 2^17 transform / a QAP chain at 2^16) and retires it"""
    run_child(scenario)


def test_child_first_call_is_a_qap_chain(gpu):
    run_child("qap_first")


def test_child_first_call_is_an_inverse_transform_on_a_created_stream(gpu):
    run_child("inverse_first")


def test_child_shutdown_frees_what_it_promises_and_nothing_the_caller_owns(gpu):
    """NTT 2^12 and 2^17, QAP 2^12, a fixed-base batch of 50, an MSM plan of 1500 points; zk_shutdown; everything again: same
    bits, equal to the oracle.  A buffer and a pooled DevVec from before keep their content, the old plan handle is refused
    with ZK_ERR_ARG (the handle table is host memory and handle values are never reused: msm.hip), a second shutdown is a
    no-op, and frvec.release_pool() leaves the pool usable."""
    run_child("shutdown")
