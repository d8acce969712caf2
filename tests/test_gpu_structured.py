"""GPU: structured inputs at the ends of the scalar field through the public entry points -- values r - 1, r - 2, deltas,
alternating vectors -- whose results are closed forms (every expected zero must be all four limbs zero), for every NTT plan
shape up to 2^22 (plain and coset forms), the fused QAP chain including its one-point and negative-size edges, the element-wise
device kernels (vec_op, vec_canon, vec_is_zero, vec_powers, poly_eval, poly_eval_many) at their block and chunk edges, the PlonK
kernels (axpby, lincomb, grand product, div_linear, perm_terms, quotient with its period refusals), SpMV rows of r - 1, and a
BN254 G1 MSM over bases with edge coordinates in both plan modes."""

import ctypes

import numpy as np
import pytest

from helpers import CURVES, rand_limbs
from oracle import corc, pyref
from zksnake_amd import _native as N

pytestmark = pytest.mark.gpu


def const(v, n):
    return np.tile(N.ints_to_limbs([v], 4), (n, 1))


def delta(v, n, at=0):
    a = np.zeros((n, 4), dtype=np.uint64)
    a[at] = N.ints_to_limbs([v], 4)[0]
    return a


def host_ntt(lib, cid, a, inverse=0, coset=0):
    out = np.zeros_like(a)
    N.check(lib.zk_ntt(cid, inverse, coset, a.shape[0], N.u64p(a), a.shape[0], N.u64p(out)))
    return out


def dev_ntt(lib, cid, a, inverse=0):
    from zksnake_amd.device import DeviceBuffer
    d = DeviceBuffer.from_numpy(np.ascontiguousarray(a))
    N.check(lib.zk_ntt_dev(cid, inverse, a.shape[0].bit_length() - 1, d.ptr, None))
    lib.zk_dev_synchronize()
    out = d.download(a.shape)
    d.free()
    return out


@pytest.mark.parametrize("name,cid", CURVES)
@pytest.mark.parametrize("log_n", list(range(23)))
def test_ntt_structured_inputs_every_plan_shape(gpu, name, cid, log_n):
    cv = pyref.curve_by_name(name)
    r, n = cv.r, 1 << log_n
    m1 = const(r - 1, n)
    inv_n = pow(n, -1, r)
    for run in (lambda a, inv: host_ntt(gpu, cid, a, inv), lambda a, inv: dev_ntt(gpu, cid, a, inv)):
        # all r - 1: the output is a delta
        assert (run(m1, 0) == delta((r - n) % r, n)).all()
        assert (run(m1, 1) == delta(r - 1, n)).all()
        # a delta of r - 1 at index 0: a constant
        assert (run(delta(r - 1, n), 0) == m1).all()
        assert (run(delta(r - 1, n), 1) == const((r - 1) * inv_n % r, n)).all()
        # alternating r - 1 and 0: nonzero only at k = 0 mod n/2
        if n >= 2:
            alt = np.zeros((n, 4), dtype=np.uint64)
            alt[0::2] = m1[0::2]
            want = np.zeros((n, 4), dtype=np.uint64)
            want[0] = want[n // 2] = N.ints_to_limbs([(r - 1) * (n // 2) % r], 4)[0]
            assert (run(alt, 0) == want).all()
    # coset forms: a delta at 0 maps to a constant and back (the offset's power 0); a delta at 1 is scaled by the offset g
    # itself (pyref.coset_ntt: g = the n-th root of unity w), forward out[k] = (r - 1) g w^k
    assert (host_ntt(gpu, cid, delta(r - 1, n), 0, 1) == m1).all()
    assert (host_ntt(gpu, cid, m1, 1, 1) == delta(r - 1, n)).all()
    w = cv.root_of_unity(n)
    if n >= 2:
        g = w
        geo = geometric(r, (r - 1) * g % r, w, n)
        assert (host_ntt(gpu, cid, delta(r - 1, n, 1), 0, 1) == geo).all()
        assert (host_ntt(gpu, cid, geo, 1, 1) == delta(r - 1, n, 1)).all()
    # a delta of r - 1 at n - 1: forward out[k] = -w^(k (n - 1)) = -w^(-k), inverse out[k] = -w^(-k (n - 1)) / n = -w^k / n
    wi = pow(w, -1, r)
    d = delta(r - 1, n, n - 1)
    fwd = geometric(r, r - 1, wi, n)
    assert (host_ntt(gpu, cid, d, 0) == fwd).all()
    assert (dev_ntt(gpu, cid, d, 0) == fwd).all()
    assert (dev_ntt(gpu, cid, d, 1) == geometric(r, (r - 1) * inv_n % r, w, n)).all()
    # half the entries in {0, 1, r - 1, r - 2}, the rest random below 2^252: element by element against the oracle
    rng = np.random.default_rng(log_n)
    mix = rand_limbs(n, log_n)
    edge = N.ints_to_limbs([0, 1, r - 1, r - 2], 4)
    mix[0::2] = edge[rng.integers(0, 4, size=(n + 1) // 2)]
    assert (host_ntt(gpu, cid, mix, 0) == corc.ntt(cid, mix, threads=16)).all()
    assert (dev_ntt(gpu, cid, mix, 1) == corc.ntt(cid, mix, inverse=True, threads=16)).all()


def geometric(r, first, ratio, n):
    """(first * ratio^k mod r for k < n) as (n, 4) limbs"""
    out, x = [], first
    for _ in range(n):
        out.append(x)
        x = x * ratio % r
    return N.ints_to_limbs(out, 4)


def _qap(lib, cid, log_n, a, b, c, form):
    """run the QAP chain in one of its three forms; returns (rc, u, v, h, divisible)"""
    from zksnake_amd.device import DeviceBuffer
    n = 1 << max(log_n, 0)
    da, db, dc = DeviceBuffer.from_numpy(a), DeviceBuffer.from_numpy(b), DeviceBuffer.from_numpy(c)
    dh, dw = DeviceBuffer(n * 32), DeviceBuffer(4 * n * 32)
    dh.upload(const(12345, n))    # h must be written, not left as it was
    ok = N._i(-1)
    if form == "one_call":
        rc = lib.zk_qap_h_dev(cid, log_n, da.ptr, db.ptr, dc.ptr, dh.ptr, dw.ptr, ok, None)
    elif form == "two_step":
        ev = N._vp()
        rc = lib.zk_qap_h_dev_begin(cid, log_n, da.ptr, db.ptr, dc.ptr, dh.ptr, dw.ptr, None, ctypes.byref(ev))
        if rc == 0:
            N.check(lib.zk_qap_h_dev_end(cid, log_n, dw.ptr, ok, None))
    else:
        rc = lib.zk_qap_uv_dev(cid, log_n, da.ptr, db.ptr, None, None)
    lib.zk_dev_synchronize()
    res = (rc, da.download((n, 4)), db.download((n, 4)), dh.download((n, 4)), ok.value)
    for buf in (da, db, dc, dh, dw):
        buf.free()
    return res


@pytest.mark.parametrize("name,cid", CURVES)
@pytest.mark.parametrize("log_n", [0, 1, 11, 12, 17])
@pytest.mark.parametrize("form", ["one_call", "two_step", "uv_only"])
def test_qap_chain_structured(gpu, name, cid, log_n, form):
    cv = pyref.curve_by_name(name)
    r, n = cv.r, 1 << log_n
    zero = np.zeros((n, 4), dtype=np.uint64)
    m1 = const(r - 1, n)
    # a = b = all r - 1, c = all 1: divisible, u = v = delta(r - 1), h exactly zero
    rc, u, v, h, ok = _qap(gpu, cid, log_n, m1, m1, const(1, n), form)
    assert rc == 0
    assert (u == delta(r - 1, n)).all() and (v == delta(r - 1, n)).all()
    if form != "uv_only":
        assert ok == 1 and (h == zero).all()
    # a = all r - 1, b = c = 0: divisible, v = 0, h = 0
    rc, u, v, h, ok = _qap(gpu, cid, log_n, m1, zero, zero, form)
    assert rc == 0 and (u == delta(r - 1, n)).all() and (v == zero).all()
    if form != "uv_only":
        assert ok == 1 and (h == zero).all()
        # one wrong entry: not divisible
        c = const(1, n)
        c[n - 1] = N.ints_to_limbs([2], 4)[0]
        rc, u, v, h, ok = _qap(gpu, cid, log_n, m1, m1, c, form)
        assert rc == 0 and ok == 0


@pytest.mark.parametrize("form", ["one_call", "two_step", "uv_only"])
def test_qap_chain_rejects_a_negative_size(gpu, form):
    one = np.zeros((1, 4), dtype=np.uint64)
    for cid in (0, 1):
        rc = _qap(gpu, cid, -1, one, one, one, form)[0]
        assert rc == N.ZK_ERR_DOMAIN


EDGE = lambda r: (0, 1, r - 1, r - 2)  # noqa: E731


@pytest.mark.parametrize("name,cid", CURVES)
def test_vec_op_on_edge_pairs(gpu, name, cid):
    from zksnake_amd.device import DeviceBuffer
    r = pyref.curve_by_name(name).r
    pairs = [(x, y) for x in EDGE(r) for y in EDGE(r)] * 20   # 320 elements: a partial second block
    a = N.ints_to_limbs([x for x, _ in pairs], 4)
    b = N.ints_to_limbs([y for _, y in pairs], 4)
    n = a.shape[0]
    da, db, do = DeviceBuffer.from_numpy(a), DeviceBuffer.from_numpy(b), DeviceBuffer(n * 32)
    for op, fn in ((0, lambda x, y: x * y), (1, lambda x, y: x + y), (2, lambda x, y: x - y)):
        want = N.ints_to_limbs([fn(x, y) % r for x, y in pairs], 4)
        out = np.zeros_like(a)
        N.check(gpu.zk_vec_op(cid, op, n, n, N.u64p(a), n, N.u64p(b), N.u64p(out)))
        assert (out == want).all(), op
        N.check(gpu.zk_vec_op_dev(cid, op, n, da.ptr, db.ptr, do.ptr, None))
        gpu.zk_dev_synchronize()
        assert (do.download((n, 4)) == want).all(), op


@pytest.mark.parametrize("name,cid", CURVES)
def test_vec_canon_is_zero_and_powers(gpu, name, cid):
    from zksnake_amd.device import DeviceBuffer
    cv = pyref.curve_by_name(name)
    r = cv.r
    xs = [0, r - 1, r, 2 * r, (1 << 256) - 1, r + 1, 2 * r - 1] * 41   # 287 elements
    d = DeviceBuffer.from_numpy(N.ints_to_limbs(xs, 4))
    N.check(gpu.zk_vec_canon_dev(cid, len(xs), d.ptr, None))
    gpu.zk_dev_synchronize()
    assert (d.download((len(xs), 4)) == N.ints_to_limbs([x % r for x in xs], 4)).all()
    # is_zero: n at the block edges, and one nonzero bit in the last word of the last element
    for n in (1, 255, 256, 257):
        z = DeviceBuffer.from_numpy(np.zeros((n, 4), dtype=np.uint64))
        flag = ctypes.c_int(-1)
        N.check(gpu.zk_vec_is_zero_dev(cid, n, z.ptr, ctypes.byref(flag), None))
        assert flag.value == 1
        last = np.zeros((n, 4), dtype=np.uint64)
        last[n - 1, 3] = np.uint64(1)
        z.upload(last)
        N.check(gpu.zk_vec_is_zero_dev(cid, n, z.ptr, ctypes.byref(flag), None))
        assert flag.value == 0, n
        z.free()
    # powers past the order of g wrap to exactly 1
    n = 256
    w = cv.root_of_unity(n)
    for g in (0, 1, r - 1, w):
        cnt = n + 37
        p = DeviceBuffer(cnt * 32)
        N.check(gpu.zk_vec_powers_dev(cid, cnt, N.u64p(N.ints_to_limbs([g], 4)), p.ptr, None))
        gpu.zk_dev_synchronize()
        assert (p.download((cnt, 4)) == N.ints_to_limbs([pow(g, k, r) for k in range(cnt)], 4)).all(), g
        p.free()


@pytest.mark.parametrize("name,cid", CURVES)
def test_poly_eval_at_roots_and_eval_many_at_chunk_edges(gpu, name, cid):
    from zksnake_amd.device import DeviceBuffer
    cv = pyref.curve_by_name(name)
    r = cv.r
    # X^n - 1 vanishes at every n-th root of unity: exactly zero
    n = 4096
    zh = np.zeros((n + 1, 4), dtype=np.uint64)
    zh[0] = N.ints_to_limbs([r - 1], 4)[0]
    zh[n] = N.ints_to_limbs([1], 4)[0]
    d = DeviceBuffer.from_numpy(zh)
    w = cv.root_of_unity(n)
    out = np.zeros(4, dtype=np.uint64)
    for x in (1, w, pow(w, n - 1, r), r - 1):
        N.check(gpu.zk_poly_eval_dev(cid, n + 1, d.ptr, N.u64p(N.ints_to_limbs([x], 4)), N.u64p(out), None))
        assert (out == 0).all(), x
    d.free()
    # 64 jobs, all coefficients r - 1, counts at the chunk and block edges, x in {1, r - 1, 2}
    counts = [0, 1, 31, 32, 33, 8191, 8192, 8193] * 8
    xs = [(1, r - 1, 2)[i % 3] for i in range(64)]
    buf = DeviceBuffer.from_numpy(const(r - 1, 8193))
    cs = np.array(counts, dtype=np.uint64)
    ptrs = (N._vp * 64)(*([buf.ptr] * 64))
    xl = N.ints_to_limbs(xs, 4)
    outs = np.zeros((64, 4), dtype=np.uint64)
    N.check(gpu.zk_poly_eval_many_dev(cid, 64, N.u64p(cs), ptrs, N.u64p(xl), N.u64p(outs), None))

    def expect(c, x):
        if x == 1:
            return (-c) % r
        if x == r - 1:
            return (r - 1) * (c % 2) % r
        return (r - 1) * (pow(2, c, r) - 1) % r
    assert (outs == N.ints_to_limbs([expect(c, x) for c, x in zip(counts, xs)], 4)).all()
    buf.free()


def _dev(limbs):
    from zksnake_amd.device import DeviceBuffer
    return DeviceBuffer.from_numpy(np.ascontiguousarray(limbs, dtype=np.uint64))


def _get(buf, n):
    N.load().zk_dev_synchronize()
    return buf.download((n, 4))


def _edge_vec(r, n, seed):
    """n values from {0, 1, r - 1, r - 2} (seeded) as ints"""
    rng = np.random.default_rng(seed)
    return [EDGE(r)[int(i)] for i in rng.integers(0, 4, size=n)]


@pytest.mark.parametrize("name,cid", CURVES)
def test_axpby_lincomb_and_grand_product_at_r_minus_1(gpu, name, cid):
    from zksnake_amd.device import DeviceBuffer
    from zksnake_amd.frvec import FrOps
    r = pyref.curve_by_name(name).r
    ops = FrOps(r)
    n = 1000
    m1l = N.ints_to_limbs([r - 1], 4)
    # axpby with a = b = c = x = y = r - 1: (-1)(-1) + (-1)(-1) - 1 = 1
    x, out = _dev(const(r - 1, n)), DeviceBuffer(n * 32)
    N.check(gpu.zk_vec_axpby_dev(cid, n, N.u64p(m1l), x.ptr, N.u64p(m1l), x.ptr, N.u64p(m1l), out.ptr, None))
    assert (_get(out, n) == const(1, n)).all()
    # lincomb: 16 terms of scalar r - 1 times all r - 1 over counts n - t, then 8 updates of r - 1 to one index
    acc = ops.d_from(const(r - 1, n))
    counts = [n - t for t in range(16)]
    ops.d_lincomb(acc, terms=[(c, r - 1, x.ptr) for c in counts], at=[(n - 3, r - 1)] * 8)
    want = [(-1 + sum(1 for c in counts if i < c)) % r for i in range(n)]
    want[n - 3] = (want[n - 3] - 8) % r
    assert (_get(acc.buf, n) == N.ints_to_limbs(want, 4)).all()
    # grand product: num = den gives exactly 1 everywhere; num all r - 1 over den 1 alternates -1, 1; and over den r - 1 is 1
    for num, den, f in (([(1, r - 1, r - 2)[i % 3] for i in range(n)], None, lambda i: 1),
                        ([r - 1] * n, [1] * n, lambda i: (-1) ** i % r),
                        ([r - 1] * n, [r - 1] * n, lambda i: 1)):
        den = num if den is None else den
        dn, dd, go = _dev(N.ints_to_limbs(num, 4)), _dev(N.ints_to_limbs(den, 4)), DeviceBuffer((n + 1) * 32)
        ops.d_grand_product(n, dn.ptr, dd.ptr, go.ptr)
        assert (_get(go, n + 1) == N.ints_to_limbs([f(i) for i in range(n + 1)], 4)).all()
        for b in (dn, dd, go):
            b.free()
    for b in (x, out):
        b.free()


@pytest.mark.parametrize("name,cid", CURVES)
def test_div_linear_leaves_no_remainder_at_edge_roots(gpu, name, cid):
    from zksnake_amd.device import DeviceBuffer
    from zksnake_amd.frvec import FrOps
    cv = pyref.curve_by_name(name)
    r = cv.r
    ops = FrOps(r)
    n = 1000
    q = _edge_vec(r, n - 1, 3)
    for root in (r - 1, 1, cv.root_of_unity(1024)):
        # coeffs of (X - root) q
        co = [(-root * q[0]) % r] + [(q[i - 1] - root * q[i]) % r for i in range(1, n - 1)] + [q[n - 2]]
        dc, dq = _dev(N.ints_to_limbs(co, 4)), DeviceBuffer((n - 1) * 32)
        rem = ops.d_div_linear(n, dc.ptr, root, dq.ptr)
        assert rem == 0 and (_get(dq, n - 1) == N.ints_to_limbs(q, 4)).all(), root
        # plus one: the remainder is exactly 1
        co[0] = (co[0] + 1) % r
        dc.upload(N.ints_to_limbs(co, 4))
        assert ops.d_div_linear(n, dc.ptr, root, dq.ptr) == 1
        dc.free(); dq.free()


@pytest.mark.parametrize("name,cid", CURVES)
def test_perm_terms_at_edge_values(gpu, name, cid):
    from zksnake_amd.device import DeviceBuffer
    from zksnake_amd.frvec import FrOps
    r = pyref.curve_by_name(name).r
    ops = FrOps(r)
    n = 777
    # every input r - 1: each factor is -1 + 1 - 1 = -1, the product -1
    m1 = _dev(const(r - 1, n))
    out = DeviceBuffer(n * 32)
    ops.d_perm_terms(n, [m1.ptr] * 3, [m1.ptr] * 3, r - 1, r - 1, out.ptr)
    assert (_get(out, n) == const(r - 1, n)).all()
    # edge values in every column and scalar
    cols = [_edge_vec(r, n, 10 + j) for j in range(6)]
    bufs = [_dev(N.ints_to_limbs(c, 4)) for c in cols]
    for beta, gamma in ((r - 1, r - 2), (1, 0), (0, r - 1)):
        ops.d_perm_terms(n, [b.ptr for b in bufs[:3]], [b.ptr for b in bufs[3:]], beta, gamma, out.ptr)
        want = []
        for i in range(n):
            v = 1
            for j in range(3):
                v = v * (cols[j][i] + beta * cols[3 + j][i] + gamma) % r
            want.append(v)
        assert (_get(out, n) == N.ints_to_limbs(want, 4)).all()


def _quotient_ref(r, m, n, cols, zh_inv, beta, gamma, alpha):
    a, b, c, z, pi, ql, qr, qo, qm, qc, s1, s2, s3, x, l1 = cols
    k = m // n
    out = []
    for i in range(m):
        gate = a[i] * ql[i] + b[i] * qr[i] + c[i] * qo[i] + a[i] * b[i] * qm[i] + qc[i] + pi[i]
        left = (a[i] + beta * x[i] + gamma) * (b[i] + 2 * beta * x[i] + gamma) * (c[i] + 3 * beta * x[i] + gamma) * z[i]
        right = (a[i] + beta * s1[i] + gamma) * (b[i] + beta * s2[i] + gamma) * (c[i] + beta * s3[i] + gamma) * z[(i + k) % m]
        t = gate + alpha * (left - right) + alpha * alpha * (z[i] - 1) * l1[i]
        out.append(t * zh_inv[i % k] % r)
    return out


@pytest.mark.parametrize("name,cid", CURVES)
def test_quotient_periods_and_refusals(gpu, name, cid):
    """m not a multiple of 256 (n = 5), period 2, 4 and 16: z(omega x) wraps around the end of the vector; period 1 and 17 are
    refused"""
    from zksnake_amd.device import DeviceBuffer
    from zksnake_amd.frvec import FrOps
    r = pyref.curve_by_name(name).r
    ops = FrOps(r)
    n = 5
    for k in (2, 4, 16):
        m = k * n
        cols = [_edge_vec(r, m, 100 * k + j) for j in range(15)]
        zh_inv = _edge_vec(r, k, 7 * k)
        bufs = [_dev(N.ints_to_limbs(c, 4)) for c in cols]
        out = DeviceBuffer(m * 32)
        for beta, gamma, alpha in ((r - 1, r - 1, r - 1), (r - 2, 1, 0)):
            ops.d_quotient(m, n, [b.ptr for b in bufs], N.ints_to_limbs(zh_inv, 4), beta, gamma, alpha, out.ptr)
            want = _quotient_ref(r, m, n, cols, zh_inv, beta, gamma, alpha)
            assert (_get(out, m) == N.ints_to_limbs(want, 4)).all(), k
        # all r - 1
        allm1 = _dev(const(r - 1, m))
        ops.d_quotient(m, n, [allm1.ptr] * 15, const(r - 1, k), r - 1, r - 1, r - 1, out.ptr)
        want = _quotient_ref(r, m, n, [[r - 1] * m] * 15, [r - 1] * k, r - 1, r - 1, r - 1)
        assert (_get(out, m) == N.ints_to_limbs(want, 4)).all(), k
    arr = ctypes.c_void_p * 15
    one = N.ints_to_limbs([1], 4)
    for m in (n, 17 * n):
        buf = DeviceBuffer(m * 32)
        rc = gpu.zk_plonk_quotient_dev(cid, m, n, arr(*([buf.ptr] * 15)), N.u64p(const(1, 17)), N.u64p(one), N.u64p(one),
                                       N.u64p(one), buf.ptr, None)
        assert rc == N.ZK_ERR_ARG, m
        buf.free()


@pytest.mark.parametrize("name,cid", CURVES)
def test_spmv_rows_of_r_minus_1(gpu, name, cid):
    """entries r - 1 times a witness of r - 1: every row is nnz mod r, for lane-per-row rows (64 entries) and a long row
    (10000 entries, several work items)"""
    from zksnake_amd.array import SparseArray
    from zksnake_amd.device import DeviceBuffer
    from zksnake_amd.spmv import DeviceCsr
    r = pyref.curve_by_name(name).r
    n_col = 12000
    lens = [64, 1, 0, 63, 10000, 64, 2]
    trip = [(row, c, r - 1) for row, ln in enumerate(lens) for c in range(ln)]
    m = SparseArray.from_triplets(*zip(*trip), len(lens), n_col, r)
    csr = DeviceCsr(cid, *m.to_csr())
    assert csr.n_long == 1
    dw, out = _dev(const(r - 1, n_col)), DeviceBuffer(len(lens) * 32)
    csr.apply(dw.ptr, out.ptr)
    assert (_get(out, len(lens)) == N.ints_to_limbs([ln % r for ln in lens], 4)).all()


def _edge_g1_bases():
    """BN254 G1 points (cofactor 1: every solution of y^2 = x^3 + 3 is in the group) with edge coordinates: x = p - 1, small x,
    y = p - small, and coordinates whose Montgomery form (R = 2^261) is within 2^20 of 0 or p"""
    p = pyref.BN254_P
    rinv = pow(1 << 261, -1, p)

    def lift(x):
        rhs = (x * x * x + 3) % p
        y = pow(rhs, (p + 1) // 4, p)
        return (x, y) if y * y % p == rhs else None

    cands = [p - 1 - i for i in range(64)] + list(range(64))
    cands += [(k * rinv) % p for k in range(1, 64)] + [((p - k) * rinv) % p for k in range(1, 64)]
    cands += [((1 << 20) - k) * rinv % p for k in range(8)] + [(p - (1 << 20) + k) * rinv % p for k in range(8)]
    pts = []
    for x in cands:
        pt = lift(x)
        if pt:
            pts += [pt, (pt[0], (p - pt[1]) % p)]   # y and p - y: one of them is a large "p - small" or a small y
    return pts


@pytest.mark.parametrize("flags", [0, N.MSM_PRECOMPUTE])
def test_msm_bn254_g1_bases_with_edge_coordinates(gpu, flags):
    pts = _edge_g1_bases()
    assert len(pts) >= 100
    n = len(pts)
    bases = corc.points_to_limbs(pts, 0, 1)
    r = pyref.BN254_R
    rng = np.random.default_rng(5)
    vals = [r - 1 if i % 2 == 0 else int(rng.integers(0, 2**62)) * (r // 2**62) for i in range(n)]
    sc = N.ints_to_limbs(vals, 4)
    exp = corc.msm(0, 1, sc, bases, threads=8)
    h = N._u64(0)
    N.check(gpu.zk_msm_plan_create(0, 1, n, bases.ctypes.data, 0, flags, 0, h))
    try:
        out = np.zeros(N.point_limbs(0, 1), dtype=np.uint64)
        N.check(gpu.zk_msm_plan_run(h, n, sc.ctypes.data, 0, 0, 0, N.u64p(out), None))
        assert (out == exp).all()
        # all scalars r - 1: the negated sum
        sc1 = const(r - 1, n)
        N.check(gpu.zk_msm_plan_run(h, n, sc1.ctypes.data, 0, 0, 0, N.u64p(out), None))
        assert (out == corc.msm(0, 1, sc1, bases, threads=8)).all()
    finally:
        N.check(gpu.zk_msm_plan_destroy(h))
