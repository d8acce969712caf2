"""Helper of tests/test_gpu_stream_state.py and tests/test_gpu_stream_state_protocols.py: the stream primitives and the
upload-behind-a-spin plumbing both use, and the scenarios that need a process of their own (a twiddle table known to hold 16
stages, a first call of a given kind, zk_shutdown).

Run as `python stream_state_child.py <scenario>`: prints ONE JSON line {"scenario", "checks": {name: bool}, "timing": {..}}.
Every expectation is the CPU oracle (oracle/corc.py), compared with ==.  Not a test module: pytest does not collect it."""

import ctypes
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

from oracle import corc  # noqa: E402
from zksnake_amd import _native as N  # noqa: E402
from zksnake_amd.device import DeviceBuffer, PinnedArray  # noqa: E402

CURVES = (("BN254", 0), ("BLS12_381", 1))
# Spin requests (microseconds).  SPIN_US parks a stream in the scenarios that assert "still in flight"; what both last on an
# MI355X, and the slowest step SPIN_US has to outlast, are in EXPERIMENTS.md "Stream-state tests".
SPIN_US = 200_000
SPIN_SHORT_US = 20_000   # upload-behind-a-spin cases: only has to outlast the host's enqueueing of one call


def rand_limbs(n, seed):
    """(n, 4) uint64 values below 2^252: canonical in both scalar fields"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    v[:, 3] &= np.uint64((1 << 60) - 1)
    return v


def new_stream(lib):
    st = N._vp()
    N.check(lib.zk_stream_create(0, ctypes.byref(st)))
    return st


def sync(lib, st):
    N.check(lib.zk_stream_synchronize(st))


def parked(lib, st, us=SPIN_US):
    """(D, t0): D = the measured duration of one spin of `us` alone on `st` (enqueue + synchronise, after a one-microsecond
    spin that takes the first-launch costs), t0 = the host time at which the spin that now parks `st` was queued"""
    N.check(lib.zk_debug_spin_dev(st, 1))
    sync(lib, st)
    t = time.perf_counter()
    N.check(lib.zk_debug_spin_dev(st, us))
    sync(lib, st)
    d = time.perf_counter() - t
    t0 = time.perf_counter()
    N.check(lib.zk_debug_spin_dev(st, us))
    return d, t0


def in_flight(d, t0, t1, what):
    """the message of a failed "still in flight" assertion, or None"""
    if t1 - t0 < d:
        return None
    return (f"timing: {what} took {1e3 * (t1 - t0):.2f} ms from the moment the spin was queued, the spin alone lasts "
            f"{1e3 * d:.2f} ms: the parked stream's work was no longer provably pending")


class Staged:
    """a device vector that holds `stale` now and receives `real` (same shape) by an asynchronous upload from page-locked
    memory when send() is called: behind a spin, `real` is there only for work ordered on that stream"""

    def __init__(self, stale, real):
        stale, real = np.ascontiguousarray(stale), np.ascontiguousarray(real)
        assert stale.shape == real.shape and stale.dtype == real.dtype and real.nbytes > 0
        self.dev = DeviceBuffer.from_numpy(stale)
        self.pin = PinnedArray(real.shape, real.dtype)
        self.pin.array[...] = real
        self.shape, self.dtype, self.nbytes = real.shape, real.dtype, real.nbytes

    @property
    def ptr(self):
        return self.dev.ptr

    def send(self, lib, st):
        N.check(lib.zk_dev_upload_async(self.dev.ptr, self.pin.ptr, self.nbytes, st))

    def download(self):
        return self.dev.download(self.shape, self.dtype)


# ---- inputs and plumbing of the upload-behind-a-spin tests (test_gpu_stream_state.py, test_gpu_stream_state_protocols.py) ----

def vals(p, n, seed):
    """n field elements with 0 and r-1 among them"""
    rnd = random.Random(seed * 7919 + (p & 0xFFFF))
    v = [rnd.randrange(p) for _ in range(n)]
    if n > 2:
        v[1], v[n - 1] = 0, p - 1
    return v


def L(ints):
    return N.ints_to_limbs(ints, 4)


def I(limbs):
    return N.limbs_to_ints(np.ascontiguousarray(limbs).reshape(-1, 4))


def one(v):
    return N.u64p(N.ints_to_limbs([v], 4))


def staged(stale, real):
    return Staged(L(stale), L(real))


def behind_spin(gpu, inputs, call, read=None):
    """park a fresh stream, queue the uploads of the real inputs behind the spin, issue `call(stream)` on it, synchronise;
    returns read() (or what call returned).  The uploads must have been queued while the spin was provably running."""
    st = new_stream(gpu)
    try:
        d, t0 = parked(gpu, st, SPIN_SHORT_US)
        for s in inputs:
            s.send(gpu, st)
        msg = in_flight(d, t0, time.perf_counter(), "queueing the uploads")
        got = call(st)
        sync(gpu, st)
        assert msg is None, msg
        return read() if read else got
    finally:
        N.check(gpu.zk_stream_destroy(st))


def settle(got, on_real, on_stale):
    assert on_real != on_stale, "the case does not distinguish the real input from the stale one"
    assert got == on_real, "differs from the model on the uploaded input"
    assert got != on_stale, "equals the model on the STALE device content: part of the call ran on another stream"


def host4(k=1):
    return np.full((k, 4), 0xA5A5A5A5, dtype=np.uint64)


def ntt_dev(lib, cid, inverse, log_n, ptr, st):
    N.check(lib.zk_ntt_dev(cid, inverse, log_n, ptr, st))


def qap_inputs(cid, log_n, seed):
    """a, b random and c = a b on the domain (a satisfied witness), with the oracle's u, v, h"""
    n = 1 << log_n
    a, b = rand_limbs(n, seed), rand_limbs(n, seed + 1)
    c = corc.vec_op(cid, "mul", a, b)
    return (a, b, c), corc.qap_h(cid, a, b, c, threads=8)


class QapRun:
    """device side of one QAP chain"""

    def __init__(self, abc):
        n = abc[0].shape[0]
        self.n, self.log_n, self.c = n, n.bit_length() - 1, abc[2]
        self.a, self.b, self.dc = (DeviceBuffer.from_numpy(x) for x in abc)
        self.h, self.work = DeviceBuffer(n * 32), DeviceBuffer(4 * n * 32)
        self.ok = N._i(-1)

    def one_call(self, lib, cid, st):
        N.check(lib.zk_qap_h_dev(cid, self.log_n, self.a.ptr, self.b.ptr, self.dc.ptr, self.h.ptr, self.work.ptr, self.ok, st))

    def begin(self, lib, cid, st):
        ev = N._vp()
        N.check(lib.zk_qap_h_dev_begin(cid, self.log_n, self.a.ptr, self.b.ptr, self.dc.ptr, self.h.ptr, self.work.ptr, st, ctypes.byref(ev)))
        return ev

    def end(self, lib, cid, st):
        N.check(lib.zk_qap_h_dev_end(cid, self.log_n, self.work.ptr, self.ok, st))

    def matches(self, uvh):
        n = self.n
        return bool(self.ok.value == 1 and (self.a.download((n, 4)) == uvh[0]).all() and (self.b.download((n, 4)) == uvh[1]).all()
                    and (self.h.download((n, 4)) == uvh[2]).all() and (self.dc.download((n, 4)) == self.c).all())


# ---- scenarios ---------------------------------------------------------------------------------------------------------

def _retired(lib, grower):
    """A transform at 2^16 is queued behind a spin on A with the 16-stage table's address in its arguments; B then makes the
    table grow (a 2^17 transform, or a QAP chain at 2^16, which needs stage 17).  The old table must stay readable."""
    checks, timing = {}, {}
    for name, cid in CURVES:
        a, b = new_stream(lib), new_stream(lib)
        x16, y17 = rand_limbs(1 << 16, 10 + cid), rand_limbs(1 << 17, 20 + cid)
        want_x = corc.ntt(cid, x16, threads=8)
        dx = DeviceBuffer.from_numpy(x16)
        # A's scratch and the 16-stage table exist before the spin: the queued call only enqueues
        ntt_dev(lib, cid, 0, 16, dx.ptr, a)
        sync(lib, a)
        checks[f"{name} warm-up"] = bool((dx.download((1 << 16, 4)) == want_x).all())
        dx.upload(x16)
        if grower == "ntt":
            dy = DeviceBuffer.from_numpy(y17)
            want_y = corc.ntt(cid, y17, threads=8)
        else:
            abc, uvh = qap_inputs(cid, 16, 30 + cid)
            run = QapRun(abc)
        d, t0 = parked(lib, a)
        ntt_dev(lib, cid, 0, 16, dx.ptr, a)
        if grower == "ntt":
            ntt_dev(lib, cid, 0, 17, dy.ptr, b)
            sync(lib, b)
        else:
            run.one_call(lib, cid, b)
        t1 = time.perf_counter()
        sync(lib, a)
        timing[name] = {"spin_ms": 1e3 * d, "grow_ms": 1e3 * (t1 - t0)}
        msg = in_flight(d, t0, t1, f"growing the table on the other stream ({grower})")
        checks[f"{name} in flight" + (": " + msg if msg else "")] = msg is None
        checks[f"{name} queued 2^16 transform on the retired table"] = bool((dx.download((1 << 16, 4)) == want_x).all())
        if grower == "ntt":
            checks[f"{name} 2^17 transform that grew the table"] = bool((dy.download((1 << 17, 4)) == want_y).all())
        else:
            checks[f"{name} QAP chain that grew the table"] = run.matches(uvh)
        # and the grown table serves the small size
        dx.upload(x16)
        ntt_dev(lib, cid, 0, 16, dx.ptr, b)
        sync(lib, b)
        checks[f"{name} 2^16 on the grown table"] = bool((dx.download((1 << 16, 4)) == want_x).all())
        N.check(lib.zk_stream_destroy(a))
        N.check(lib.zk_stream_destroy(b))
    return checks, timing


def retired_by_ntt(lib):
    return _retired(lib, "ntt")


def retired_by_qap(lib):
    return _retired(lib, "qap")


def qap_first(lib):
    """the process's first call is a QAP chain: BLS12-381 at 2^16 (builds a 17-stage table in one go), then BN254 at 2^12"""
    checks = {}
    for name, cid, log_n in (("BLS12_381", 1, 16), ("BN254", 0, 12)):
        abc, uvh = qap_inputs(cid, log_n, 40 + cid)
        run = QapRun(abc)
        run.one_call(lib, cid, None)
        checks[f"{name} 2^{log_n}"] = run.matches(uvh)
    return checks, {}


def inverse_first(lib):
    """the process's first call is an inverse transform at 2^17 on a created stream, then the host API at size 4"""
    checks = {}
    for name, cid in CURVES:
        st = new_stream(lib)
        x = rand_limbs(1 << 17, 50 + cid)
        dx = DeviceBuffer.from_numpy(x)
        ntt_dev(lib, cid, 1, 17, dx.ptr, st)
        sync(lib, st)
        checks[f"{name} inverse 2^17"] = bool((dx.download((1 << 17, 4)) == corc.ntt(cid, x, inverse=True, threads=8)).all())
        small = rand_limbs(4, 60 + cid)
        out = np.zeros((4, 4), dtype=np.uint64)
        N.check(lib.zk_ntt(cid, 0, 0, 4, N.u64p(small), 4, N.u64p(out)))
        checks[f"{name} host size 4"] = bool((out == corc.ntt(cid, small)).all())
        N.check(lib.zk_stream_destroy(st))
    return checks, {}


def shutdown(lib):
    """everything zk_shutdown promises to free is rebuilt on demand; what the caller still owns stays valid"""
    from zksnake_amd import frvec
    from zksnake_amd.constant import BN254_SCALAR_FIELD
    checks = {}
    cid, grp = 0, 1
    st = new_stream(lib)   # lives across the shutdown
    x12, x17 = rand_limbs(1 << 12, 70), rand_limbs(1 << 17, 71)
    abc, uvh = qap_inputs(cid, 12, 72)
    gen = np.zeros(8, dtype=np.uint64)
    N.check(lib.zk_point_generator(cid, grp, N.u64p(gen)))
    k50, k1500, sc = rand_limbs(50, 73), rand_limbs(1500, 74), rand_limbs(1500, 75)
    bases = corc.batch_mul(cid, grp, k1500, gen)
    want = {"ntt12": corc.ntt(cid, x12), "ntt17": corc.ntt(cid, x17, threads=8), "batch": corc.batch_mul(cid, grp, k50, gen),
            "msm": corc.msm(cid, grp, sc, bases, threads=8)}

    def compute():
        got = {}
        for key, x, log_n in (("ntt12", x12, 12), ("ntt17", x17, 17)):
            d = DeviceBuffer.from_numpy(x)
            ntt_dev(lib, cid, 0, log_n, d.ptr, st)
            sync(lib, st)
            got[key] = d.download(x.shape)
        run = QapRun(abc)
        run.one_call(lib, cid, st)
        got["qap"] = run.matches(uvh)
        out = np.zeros((50, 8), dtype=np.uint64)
        N.check(lib.zk_batch_mul(cid, grp, 50, N.u64p(k50), N.u64p(gen), 1, N.u64p(out)))
        got["batch"] = out
        h = ctypes.c_uint64(0)
        N.check(lib.zk_msm_plan_create(cid, grp, 1500, bases.ctypes.data, 0, 0, 0, ctypes.byref(h)))
        pt = np.zeros(8, dtype=np.uint64)
        N.check(lib.zk_msm_plan_run(h.value, 1500, sc.ctypes.data, 0, 0, 0, N.u64p(pt), None))
        got["msm"] = pt
        return got, h.value

    def same(got, label):
        for key in ("ntt12", "ntt17", "batch", "msm"):
            checks[f"{label}: {key} equals the oracle"] = bool((got[key] == want[key]).all())
        checks[f"{label}: qap equals the oracle"] = got["qap"]

    first, plan = compute()
    same(first, "before shutdown")
    pattern = rand_limbs(1000, 76)
    buf = DeviceBuffer.from_numpy(pattern)
    ops = frvec.FrOps(BN254_SCALAR_FIELD)
    del_me = frvec.DevVec(1000)
    del del_me                                  # into the pool ...
    vec = frvec.DevVec(1000, zero=False)        # ... and out of it again
    checks["the DevVec came from the pool"] = not frvec._POOL.get(32 * 1000)
    vec.upload(pattern)

    checks["zk_shutdown returns ZK_OK"] = lib.zk_shutdown() == N.ZK_OK
    second, plan2 = compute()
    same(second, "after shutdown")
    checks["results before and after are the same bits"] = all(bool((first[k] == second[k]).all()) for k in want)
    checks["a buffer from before the shutdown keeps its content"] = bool((buf.download(pattern.shape) == pattern).all())
    checks["a DevVec from before the shutdown keeps its content"] = bool((vec.download() == pattern).all())
    checks["the buffer can be freed"] = lib.zk_dev_free(buf.ptr) == N.ZK_OK
    buf.ptr = None
    pt = np.zeros(8, dtype=np.uint64)
    checks["plan_run refuses the handle from before the shutdown"] = \
        lib.zk_msm_plan_run(plan, 1500, sc.ctypes.data, 0, 0, 0, N.u64p(pt), None) == N.ZK_ERR_ARG and not pt.any()
    checks["plan_destroy refuses the handle from before the shutdown"] = lib.zk_msm_plan_destroy(plan) == N.ZK_ERR_ARG
    checks["the new plan is destroyed normally"] = lib.zk_msm_plan_destroy(plan2) == N.ZK_OK
    checks["two shutdowns in a row return ZK_OK"] = lib.zk_shutdown() == N.ZK_OK and lib.zk_shutdown() == N.ZK_OK
    del vec
    checks["the pool holds the released DevVec"] = bool(frvec._POOL.get(32 * 1000))
    frvec.release_pool()
    checks["release_pool empties the pool"] = not frvec._POOL and frvec._POOL_BYTES[0] == 0
    v = ops.d_from(x12)
    ops.d_ntt(v, 1 << 12)
    checks["DevVec work after release_pool equals the oracle"] = bool((v.download() == want["ntt12"]).all())
    third, plan3 = compute()
    same(third, "after the second shutdown")
    checks["the last plan is destroyed normally"] = lib.zk_msm_plan_destroy(plan3) == N.ZK_OK
    N.check(lib.zk_stream_destroy(st))
    return checks, {}


SCENARIOS = {"retired_by_ntt": retired_by_ntt, "retired_by_qap": retired_by_qap, "qap_first": qap_first,
             "inverse_first": inverse_first, "shutdown": shutdown}


def main(argv):
    scenario = argv[1]
    lib = N.ensure_gpu()
    checks, timing = SCENARIOS[scenario](lib)
    print(json.dumps({"scenario": scenario, "checks": checks, "timing": timing}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
