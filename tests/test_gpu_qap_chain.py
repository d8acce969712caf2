"""GPU: the fused QAP chain (zk_qap_h_dev, _begin / _end, zk_qap_uv_dev; csrc/ntt.hip, qap_h_dev_impl) at every transform plan
shape from 2^1 to 2^22, both scalar fields, with a nonzero quotient compared element by element, by == on limbs.

The chain's element-wise work rides on ntt_pass_kernel (NttFuse: in_v on a first pass; scale_tab, out2, add_tab on a last pass),
and each hook indexes its table with the pass's own physical index, which depends on the plan: one pass to 2^11, two to 2^16
(6+6, 7+6, 8+6, 8+7, 8+8), three above (6+5+6, 6+6+6, 7+6+6, 8+6+6, 8+6+7, 8+6+8 for 2^17 .. 2^22).  The inputs are the three
families of tests/qap_model.py (pinned on the CPU by tests/test_qap_model.py):

  A  random with edge values against the CPU oracle's whole chain, 2^1 .. 2^17 (the oracle takes seconds above);
  B  dense times a monomial, 2^1 .. 2^22: a dense h over up to 7/8 of the vector from ONE oracle transform per (curve, size),
     exact zeros above, both role orders (the dense vector through out2 = U1 or V1);
  C  sparse times its reflection, 2^3 .. 2^22: nonzero h at both ends and either side of the last pass's run length, of 2048 and
     of n/2, and an index where two products cancel.

Every run fills h and the work area with 0xA5 first (every element of h, zeros included, must be written), gives both eight guard
elements behind their documented sizes (n and 4n), and checks u, v, h, the divisibility flag, that c is untouched and that the
guards kept their fill.  One combination per size also runs in the two-step form on a stream of its own and through
zk_qap_uv_dev (both pointers, and each alone).  The oracle transforms are built once per (curve, size) and shared."""

import ctypes

import numpy as np
import pytest

import qap_model as M
from oracle import corc
from zksnake_amd import _native as N
from zksnake_amd.device import DeviceBuffer

pytestmark = pytest.mark.gpu

GUARD, FILL = 8, 0xA5
THREADS = 16
LOGS = list(range(1, 23))
ORACLE_LOGS = list(range(1, 18))
FLIP_LOGS = (9, 12, 17)
_SHARED = {}


@pytest.fixture(scope="module", autouse=True)
def shared_inputs():
    """the module's oracle transforms (never modified) are dropped when its last test has run"""
    yield
    _SHARED.clear()


def dense(name, cid, log_n):
    """(u, a = NTT(u)) of family B"""
    key = ("dense", cid, log_n)
    if key not in _SHARED:
        u = M.mixed(M.curve(name), 1 << log_n, 7000 + 10 * log_n + cid)
        _SHARED[key] = (u, corc.ntt(cid, u, threads=THREADS))
    return _SHARED[key]


def monomial(name, cid, log_n, f):
    """(a, b, c, u, v, h) of family B for the shift f"""
    cv, n = M.curve(name), 1 << log_n
    u, a = dense(name, cid, log_n)
    b, c, v, h = M.monomial_case(cid, cv, u, a, f, M.monomial_beta(cv, n, f))
    return a, b, c, u, v, h


def reflection(name, cid, log_n):
    """(a, b, c, u, v, h) of family C (one test's, so not kept)"""
    m = M.Reflection(M.curve(name), log_n)
    a = corc.ntt(cid, m.coefficients(), threads=THREADS)
    return (a,) + m.case(cid, a)


class Chain:
    """one run of the chain: a, b, c on the device, h and the work area filled with 0xA5 with guard elements behind them"""

    def __init__(self, gpu, cid, log_n, a, b, c):
        self.gpu, self.cid, self.log_n, self.n = gpu, cid, log_n, 1 << log_n
        n = self.n
        self.a, self.b, self.c = DeviceBuffer.from_numpy(a), DeviceBuffer.from_numpy(b), DeviceBuffer.from_numpy(c)
        self.h, self.work = DeviceBuffer((n + GUARD) * 32), DeviceBuffer((4 * n + GUARD) * 32)
        for buf in (self.h, self.work):
            N.check(gpu.zk_dev_memset(buf.ptr, FILL, buf.nbytes))
        gpu.zk_dev_synchronize()      # the fill runs on the default stream, which a stream of zk_stream_create does not wait for
        self.ok = N._i(-1)

    def one_call(self):
        N.check(self.gpu.zk_qap_h_dev(self.cid, self.log_n, self.a.ptr, self.b.ptr, self.c.ptr, self.h.ptr, self.work.ptr, self.ok, None))

    def two_step(self):
        st, ev = N._vp(), N._vp()
        N.check(self.gpu.zk_stream_create(0, ctypes.byref(st)))
        try:
            N.check(self.gpu.zk_qap_h_dev_begin(self.cid, self.log_n, self.a.ptr, self.b.ptr, self.c.ptr, self.h.ptr, self.work.ptr, st,
                                                ctypes.byref(ev)))
            assert ev.value
            N.check(self.gpu.zk_qap_h_dev_end(self.cid, self.log_n, self.work.ptr, self.ok, st))
        finally:
            N.check(self.gpu.zk_stream_destroy(st))

    def uv(self, with_a=True, with_b=True):
        N.check(self.gpu.zk_qap_uv_dev(self.cid, self.log_n, self.a.ptr if with_a else None, self.b.ptr if with_b else None, None, None))
        self.gpu.zk_dev_synchronize()

    def check(self, u, v, h, c, divisible=1, what=""):
        n = self.n
        self.gpu.zk_dev_synchronize()
        assert divisible is None or self.ok.value == divisible, f"divisible {what}"
        assert (self.a.download((n, 4)) == u).all(), f"u {what}"
        assert (self.b.download((n, 4)) == v).all(), f"v {what}"
        if h is not None:
            got = self.h.download((n, 4))
            bad = np.flatnonzero((got != h).any(axis=1))
            assert bad.size == 0, f"h {what}: {bad.size} elements differ, first at {bad[:8].tolist()}, last at {int(bad[-1])}"
        assert (self.c.download((n, 4)) == c).all(), f"c was written {what}"
        assert (self.h.download((GUARD * 32,), np.uint8, offset=n * 32) == FILL).all(), f"written behind h {what}"
        assert (self.work.download((GUARD * 32,), np.uint8, offset=4 * n * 32) == FILL).all(), f"written behind the work area {what}"

    def free(self):
        for buf in (self.a, self.b, self.c, self.h, self.work):
            buf.free()


def run(gpu, cid, log_n, a, b, c, u, v, h, form="one_call", what=""):
    ch = Chain(gpu, cid, log_n, a, b, c)
    try:
        getattr(ch, form)()
        ch.check(u, v, h, c, what=what)
    finally:
        ch.free()


# ---- A: random with edge values against the oracle's whole chain --------------------------------------------------------------
@pytest.mark.parametrize("log_n", ORACLE_LOGS)
@pytest.mark.parametrize("name,cid", M.CURVES)
def test_random_with_edge_values_matches_the_oracle_chain(gpu, name, cid, log_n):
    cv, n = M.curve(name), 1 << log_n
    a, b = M.mixed(cv, n, 100 + log_n), M.mixed(cv, n, 200 + log_n)
    c = corc.vec_op(cid, "mul", a, b)
    u, v, h = corc.qap_h(cid, a, b, c, threads=THREADS)
    run(gpu, cid, log_n, a, b, c, u, v, h)


# ---- B: dense times a monomial ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,eighths", [(x, e) for x in LOGS for e in (4, 6, 7)[:x]], ids=lambda x: str(x))
@pytest.mark.parametrize("name,cid", M.CURVES)
def test_dense_times_monomial(gpu, name, cid, log_n, eighths):
    """f = n/2, 3n/4, 7n/8 (eighths of n), as far as they are integers"""
    f = (eighths << log_n) // 8
    assert f in M.monomial_shifts(1 << log_n)
    a, b, c, u, v, h = monomial(name, cid, log_n, f)
    run(gpu, cid, log_n, a, b, c, u, v, h, what="dense first")
    run(gpu, cid, log_n, b, a, c, v, u, h, what="dense second")


# ---- C: sparse times its reflection ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [x for x in LOGS if x >= 3])
@pytest.mark.parametrize("name,cid", M.CURVES)
def test_sparse_times_reflection(gpu, name, cid, log_n):
    a, b, c, u, v, h = reflection(name, cid, log_n)
    run(gpu, cid, log_n, a, b, c, u, v, h, what="sparse first")
    run(gpu, cid, log_n, b, a, c, v, u, h, what="reflection first")


# ---- the other two forms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", LOGS)
@pytest.mark.parametrize("name,cid", M.CURVES)
def test_two_step_and_uv_forms(gpu, name, cid, log_n):
    """family B with f = n/2, dense vector second (its one-call run is in test_dense_times_monomial)"""
    n = 1 << log_n
    b, a, c, v, u, h = monomial(name, cid, log_n, n // 2)
    run(gpu, cid, log_n, a, b, c, u, v, h, form="two_step", what="two-step")
    for with_a, with_b in ((True, True), (True, False), (False, True)):
        ch = Chain(gpu, cid, log_n, a, b, c)
        try:
            ch.uv(with_a, with_b)
            ch.check(u if with_a else a, v if with_b else b, None, c, divisible=None, what=f"uv form {with_a} {with_b}")
            if with_a and with_b:   # this form has no use for h and the work area: both keep their fill altogether
                assert (ch.h.download((n * 32,), np.uint8) == FILL).all() and (ch.work.download((4 * n * 32,), np.uint8) == FILL).all()
        finally:
            ch.free()


# ---- divisibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", FLIP_LOGS)
@pytest.mark.parametrize("name,cid", M.CURVES)
def test_one_wrong_entry_is_not_divisible(gpu, name, cid, log_n):
    cv, n = M.curve(name), 1 << log_n
    a, b, c, u, v, h = monomial(name, cid, log_n, 3 * n // 4)
    for form, index in (("one_call", 0), ("one_call", 255), ("two_step", 256), ("one_call", n // 2), ("two_step", n - 1)):
        bad = M.flip_limb(c, index, cv.r)
        ch = Chain(gpu, cid, log_n, a, b, bad)
        try:
            getattr(ch, form)()
            ch.check(u, v, None, bad, divisible=0, what=f"c[{index}] flipped")
        finally:
            ch.free()
    # an entry of a instead: u is another vector now, v is not
    index = n // 2 + 1
    bad = M.flip_limb(a, index, cv.r)
    ch = Chain(gpu, cid, log_n, bad, b, c)
    try:
        ch.one_call()
        ch.check(corc.ntt(cid, bad, inverse=True, threads=THREADS), v, None, c, divisible=0, what=f"a[{index}] flipped")
    finally:
        ch.free()
