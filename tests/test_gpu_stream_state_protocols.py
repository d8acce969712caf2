"""GPU: stream discipline of the twelve entry points of csrc/ipa.hip, csrc/rangeproof.hip and csrc/gkr.hip, with the technique of
tests/test_gpu_stream_state.py, unchanged: a fresh non-blocking stream is parked behind zk_debug_spin_dev, the real inputs
arrive from page-locked memory behind the spin (the device buffers hold another valid pattern until then), the call is issued
on that stream, and after the synchronisation the result must equal the integer model on the real input and differ from the
model on the stale one.  A kernel or copy that a wrapper put on another stream computes on the stale pattern: a wrong value,
never a fault.  Several of these calls queue two or three kernels and a copy back to the host; every one of them is covered
by an output that only comes out right when each link ran behind the uploads.

Three calls read no device memory (zk_ipa_verify_scalars_dev, zk_rp_verify_scalars_dev, zk_gkr_eq_table_dev).  For them the
output buffer is downloaded on the default stream while the stream is still parked and must still hold its pre-fill: a launch
that left the stream has written by then.

Expectations: tests/ipa_model.py, tests/range_proof_model.py, tests/gkr_model.py, compared with ==.  Outputs are pre-filled with
valid field elements that differ from what is expected, so that "written, and on this stream" shows."""

import random
import time

import pytest

import gkr_model as G
import ipa_model as IM
import range_proof_model as RM
import stream_state_child as S
from stream_state_child import I, L, behind_spin, host4, one, settle, staged, vals
from test_gpu_gkr import _skewed_layer, arrays
from zksnake_amd import _native as N
from zksnake_amd.arithmetization.layered_circuit import CompiledLayer
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD
from zksnake_amd.device import DeviceBuffer
from zksnake_amd.spmv import ITEM, LONG_ROW

pytestmark = pytest.mark.gpu

FIELDS = (("BN254", 0, BN254_SCALAR_FIELD), ("BLS12_381", 1, BLS12_381_SCALAR_FIELD))
per_field = pytest.mark.parametrize("name,cid,p", FIELDS, ids=[f[0] for f in FIELDS])


def untouched_host():
    """what a host result of host4() holds when the call wrote nothing to it"""
    return I(host4())[0]


def pattern(p, n, seed):
    """n field elements between 2 and r - 2: none of them is a 0, 1 or r - 1 that a result holds for a reason"""
    return [2 + x % (p - 3) for x in vals(p, n, seed)]


def filled(p, n, seed):
    """(device buffer of n valid field elements, the elements)"""
    fill = pattern(p, n, seed)
    return DeviceBuffer.from_numpy(L(fill)), fill


def read(buf, n):
    return I(buf.download((n, 4)))


def settle_parts(names, got, on_real, on_stale, same=()):
    """settle() on every named part of a result; the parts in `same` do not depend on the staged input, so there only the value
    is checked -- and that the model says so"""
    assert len(names) == len(got) == len(on_real) == len(on_stale)
    for name, g, r, s in zip(names, got, on_real, on_stale):
        if name in same:
            assert r == s, f"{name}: expected not to depend on the staged input"
            assert g == r, f"{name}: differs from the model"
        else:
            try:
                settle(g, r, s)
            except AssertionError as e:
                raise AssertionError(f"{name}: {e}") from None


def held_back(gpu, out, n, call):
    """for a call without device inputs: park a fresh stream, issue `call(stream)`, download the n elements of `out` on the default
    stream BEFORE the spin ends (asserted), synchronise; returns (what the early download saw, the output afterwards)"""
    st = S.new_stream(gpu)
    try:
        d, t0 = S.parked(gpu, st, S.SPIN_SHORT_US)
        call(st)
        early = read(out, n)
        msg = S.in_flight(d, t0, time.perf_counter(), "issuing the call and downloading its output on the default stream")
        S.sync(gpu, st)
        assert msg is None, msg
        return early, read(out, n)
    finally:
        N.check(gpu.zk_stream_destroy(st))


def settle_held_back(early, late, prefill, want):
    assert prefill != want and not set(prefill) & set(want), "the pre-fill does not distinguish itself from the result"
    assert early == prefill, "the output was written while the stream was still parked: the launch ran on another stream"
    assert late == want, "differs from the model"


# ---- csrc/ipa.hip ---------------------------------------------------------------------------------------------------------------

IPA_LOG = 9
IPA_PARTS = ("a", "b", "s", "s_inv", "scal_L", "scal_R", "cross")


def ipa_model(k, a, b, s, s_inv, weight, u, p, untouched):
    """the round's contract on copies: (a, b, s, s_inv, scal_L, scal_R, cross); `untouched` stands where a round writes nothing"""
    a, b, s, s_inv = list(a), list(b), list(s), list(s_inv)
    out = RM.seeded_round_contract(IPA_LOG, k, a, b, s, s_inv, weight, u, None if u is None else pow(u, -1, p), p)
    return (a, b, s, s_inv) + (tuple(out) if out else untouched)


@pytest.mark.parametrize("k", [0, 1, IPA_LOG], ids=["k=0", "k=1 (in-place fold)", "k=log_n (last round)"])
@per_field
def test_ipa_round_on_a_busy_stream(gpu, name, cid, p, k):
    """fold, scalars, cross products, their combine and the copy back: a and b after the fold, s and s_inv, the 2n scalars of L
    and of R and the two cross products on the host.  k = 0 reads a and b only (s, s_inv are initialised); later rounds read
    all four.  The last round writes neither scalar buffer nor cross product: both must keep their content."""
    n = 1 << IPA_LOG
    stale = [vals(p, n, 300 + i) for i in range(4)]
    real = [vals(p, n, 310 + i) for i in range(4)]
    u = None if k == 0 else vals(p, 3, 320)[0]
    bufs = [staged(x, y) for x, y in zip(stale, real)]
    (d_l, fill_l), (d_r, fill_r) = filled(p, 2 * n, 321), filled(p, 2 * n, 322)
    cross = host4(2)
    untouched = (fill_l, fill_r, (untouched_host(), untouched_host()))

    def call(st):
        N.check(gpu.zk_ipa_round_dev(cid, IPA_LOG, k, *[x.ptr for x in bufs], None if u is None else one(u), None if u is None else one(pow(u, -1, p)),
                                     d_l.ptr, d_r.ptr, N.u64p(cross), st))

    got = behind_spin(gpu, bufs if k else bufs[:2], call,
                      lambda: tuple(I(x.download()) for x in bufs) + (read(d_l, 2 * n), read(d_r, 2 * n), tuple(I(cross))))
    on_real, on_stale = ipa_model(k, *real, None, u, p, untouched), ipa_model(k, *stale, None, u, p, untouched)
    if k == 0:
        same = ("s", "s_inv")
        assert on_real[4] != fill_l and on_real[5] != fill_r
    elif k == IPA_LOG:
        same = ("scal_L", "scal_R", "cross")
    else:
        same = ()
    settle_parts(IPA_PARTS, got, on_real, on_stale, same)


@per_field
def test_ipa_round_seeded_on_a_busy_stream(gpu, name, cid, p):
    """k = 0 with the weights of s_inv staged: s_inv is the REAL weights, and so is everything multiplied by them"""
    n = 1 << IPA_LOG
    stale = [vals(p, n, 330 + i) for i in range(3)]      # a, b, h_weight
    real = [vals(p, n, 340 + i) for i in range(3)]
    a, b, w = (staged(x, y) for x, y in zip(stale, real))
    (d_s, _), (d_si, _) = filled(p, n, 350), filled(p, n, 351)
    (d_l, _), (d_r, _) = filled(p, 2 * n, 352), filled(p, 2 * n, 353)
    cross = host4(2)

    def call(st):
        N.check(gpu.zk_ipa_round_seeded_dev(cid, IPA_LOG, 0, a.ptr, b.ptr, d_s.ptr, d_si.ptr, w.ptr, None, None, d_l.ptr, d_r.ptr, N.u64p(cross), st))

    got = behind_spin(gpu, [a, b, w], call, lambda: (I(a.download()), I(b.download()), read(d_s, n), read(d_si, n), read(d_l, 2 * n),
                                                      read(d_r, 2 * n), tuple(I(cross))))
    blank = [0] * n
    on_real = ipa_model(0, real[0], real[1], blank, blank, real[2], None, p, None)
    on_stale = ipa_model(0, stale[0], stale[1], blank, blank, stale[2], None, p, None)
    settle_parts(IPA_PARTS, got, on_real, on_stale, same=("s",))
    assert got[3] == real[2], "s_inv is not the uploaded weights"
    assert I(w.download()) == real[2], "the weights were modified"


def round_challenges(p, count, seed):
    """1, r - 1, a value >= r, then random ones, as handed in"""
    return ([1, p - 1, p + 5] + [x or 1 for x in vals(p, count, seed)])[:count]


@per_field
def test_ipa_verify_scalars_on_a_busy_stream(gpu, name, cid, p):
    n = 1 << IPA_LOG
    us = round_challenges(p, IPA_LOG, 360)
    a, b = vals(p, 3, 361)[0], p - 1
    out, prefill = filled(p, 2 * n, 362)
    early, late = held_back(gpu, out, 2 * n, lambda st: N.check(gpu.zk_ipa_verify_scalars_dev(
        cid, IPA_LOG, N.u64p(L(us)), N.u64p(L([pow(u, -1, p) for u in us])), one(a), one(b), out.ptr, st)))
    settle_held_back(early, late, prefill, IM.verify_scalars(IPA_LOG, [u % p for u in us], a, b, p))


# ---- csrc/rangeproof.hip -----------------------------------------------------------------------------------------------------

RP_BITS_LOG, RP_LOG = 3, 8
RP_N = 1 << RP_LOG


def rp_values(seed):
    """(values, their device form of m x 2 limbs): random 128-bit integers, 0 and 2^n - 1 among the bits that count"""
    rnd = random.Random(seed)
    m = 1 << (RP_LOG - RP_BITS_LOG)
    values = [rnd.getrandbits(128) for _ in range(m)]
    values[1] &= ~0xFF
    values[m - 1] |= 0xFF
    return values, N.ints_to_limbs(values, 2)


def rp_inputs(p, seed):
    """(stale values, real values, Staged values, stale s, real s, Staged s)"""
    (pv, pl), (qv, ql) = rp_values(seed), rp_values(seed + 1)
    assert [v & 0xFF for v in pv] != [v & 0xFF for v in qv]
    ps, qs = vals(p, 2 * RP_N, seed + 2), vals(p, 2 * RP_N, seed + 3)
    return pv, qv, S.Staged(pl, ql), ps, qs, staged(ps, qs)


def values_of(st):
    return N.limbs_to_ints(st.download())


@per_field
def test_rp_bits_on_a_busy_stream(gpu, name, cid, p):
    pv, qv, values, _, _, _ = rp_inputs(p, 400)
    out, prefill = filled(p, 2 * RP_N, 404)
    got = behind_spin(gpu, [values], lambda st: N.check(gpu.zk_rp_bits_dev(cid, RP_BITS_LOG, RP_LOG, values.ptr, out.ptr, st)),
                      lambda: read(out, 2 * RP_N))
    assert not set(prefill) & {0, 1, p - 1}
    settle(got, RM.bits_contract(RP_BITS_LOG, RP_LOG, qv, p), RM.bits_contract(RP_BITS_LOG, RP_LOG, pv, p))
    assert values_of(values) == qv, "the values were modified"


@per_field
def test_rp_poly_on_a_busy_stream(gpu, name, cid, p):
    """the three sums, their combine and the copy back: the three coefficients on the host"""
    pv, qv, values, ps, qs, s = rp_inputs(p, 410)
    y, z = vals(p, 4, 414)[2:]
    t = host4(3)
    behind_spin(gpu, [values, s], lambda st: N.check(gpu.zk_rp_poly_dev(cid, RP_BITS_LOG, RP_LOG, values.ptr, s.ptr, one(y), one(z), N.u64p(t), st)))
    on_real, on_stale = (RM.poly_contract(RP_BITS_LOG, RP_LOG, v, x, y, z, p) for v, x in ((qv, qs), (pv, ps)))
    settle_parts(("t0", "t1", "t2"), tuple(I(t)), on_real, on_stale)
    assert values_of(values) == qv and I(s.download()) == qs, "an input table was modified"


@per_field
def test_rp_eval_on_a_busy_stream(gpu, name, cid, p):
    """l || r at x depend on the values and on s; the weights y_inv^k on neither, so for them the pre-fill is what shows the write"""
    pv, qv, values, ps, qs, s = rp_inputs(p, 420)
    y, z, x = vals(p, 5, 424)[2:]
    y_inv = pow(y, -1, p)
    (ab, _), (w, fill_w) = filled(p, 2 * RP_N, 425), filled(p, RP_N, 426)
    got = behind_spin(gpu, [values, s], lambda st: N.check(gpu.zk_rp_eval_dev(cid, RP_BITS_LOG, RP_LOG, values.ptr, s.ptr, one(y), one(y_inv), one(z),
                                                                               one(x), ab.ptr, w.ptr, st)),
                      lambda: (read(ab, 2 * RP_N), read(w, RP_N)))
    on_real, on_stale = (RM.eval_contract(RP_BITS_LOG, RP_LOG, v, t, y, y_inv, z, x, p) for v, t in ((qv, qs), (pv, ps)))
    assert not set(fill_w) & set(on_real[1])
    settle_parts(("ab", "h_weight"), got, on_real, on_stale, same=("h_weight",))
    assert values_of(values) == qv and I(s.download()) == qs, "an input table was modified"


@per_field
def test_rp_verify_scalars_on_a_busy_stream(gpu, name, cid, p):
    us = round_challenges(p, RP_LOG, 430)
    a, b, y_inv, z = vals(p, 6, 431)[2:]
    out, prefill = filled(p, 2 * RP_N, 432)
    early, late = held_back(gpu, out, 2 * RP_N, lambda st: N.check(gpu.zk_rp_verify_scalars_dev(
        cid, RP_BITS_LOG, RP_LOG, N.u64p(L(us)), N.u64p(L([pow(u, -1, p) for u in us])), one(a), one(b), one(y_inv), one(z), out.ptr, st)))
    settle_held_back(early, late, prefill, RM.verify_scalars_contract(RP_BITS_LOG, RP_LOG, us, a, b, y_inv, z, p))


# ---- csrc/gkr.hip ---------------------------------------------------------------------------------------------------------------

@per_field
def test_gkr_eq_table_on_a_busy_stream(gpu, name, cid, p):
    k = 10
    r = vals(p, k, 500)
    out, prefill = filled(p, 1 << k, 501)
    early, late = held_back(gpu, out, 1 << k, lambda st: N.check(gpu.zk_gkr_eq_table_dev(cid, k, N.u64p(L(r)), out.ptr, st)))
    settle_held_back(early, late, prefill, G.eq_table(r, p))


@per_field
def test_gkr_layer_eval_on_a_busy_stream(gpu, name, cid, p):
    n_prev, n = 300, 257
    kp, k = G.num_vars(n_prev), G.num_vars(n)
    rnd = random.Random(510)
    gates = [(rnd.randrange(2), rnd.randrange(n_prev), rnd.randrange(n_prev)) for _ in range(n)]
    t, b, c = (DeviceBuffer.from_numpy(a) for a in arrays(gates))
    pw, qw = G.pad(vals(p, n_prev, 511), kp), G.pad(vals(p, n_prev, 512), kp)
    w = staged(pw, qw)
    out, prefill = filled(p, 1 << k, 513)
    got = behind_spin(gpu, [w], lambda st: N.check(gpu.zk_gkr_layer_eval_dev(cid, n, t.ptr, b.ptr, c.ptr, kp, w.ptr, k, out.ptr, st)),
                      lambda: read(out, 1 << k))
    on_real, on_stale = (G.pad(G.evaluate_circuit([gates], x, p)[1], k) for x in (qw, pw))
    assert 0 not in prefill[n:], "the pre-fill hides an unwritten padding entry"
    settle(got, on_real, on_stale)
    assert I(w.download()) == qw, "the wires below were modified"


def skewed(p):
    """the "skewed rows" layer of test_gpu_gkr.py: short rows, long rows of one, two and three items -- all three kernels of a pass"""
    n_prev, gates = _skewed_layer(random.Random("skewed rows"))
    layer = CompiledLayer(n_prev, *arrays(gates))
    for csr in (layer.by_b, layer.by_c):
        assert csr.n_long == 4 and csr.n_items == 7 and csr.n_entries == len(gates) == 2 * LONG_ROW + 4 * ITEM + 6
    return gates, layer


@pytest.mark.parametrize("phase", [1, 2])
@per_field
def test_gkr_phases_on_a_busy_stream(gpu, name, cid, p, phase):
    """rows, items and long rows: E and W (phase 1) or E and E2 (phase 2) arrive behind the spin; the partial sums of the items
    and both outputs hold other field elements until the pass writes them, so a long-rows kernel that left the stream adds up
    the pre-fill"""
    gates, layer = skewed(p)
    k, kp = layer.k, layer.k_prev
    csr = layer.by_b if phase == 1 else layer.by_c
    pe, qe = vals(p, 1 << k, 520), vals(p, 1 << k, 521)
    py, qy = vals(p, 1 << kp, 522), vals(p, 1 << kp, 523)
    e, y = staged(pe, qe), staged(py, qy)
    fill_part = pattern(p, 2 * csr.n_items, 524)
    csr.d_partials.upload(L(fill_part))
    (o0, fill0), (o1, fill1) = filled(p, 1 << kp, 525), filled(p, 1 << kp, 526)
    fn = gpu.zk_gkr_phase1_dev if phase == 1 else gpu.zk_gkr_phase2_dev
    got = behind_spin(gpu, [e, y], lambda st: N.check(fn(cid, *csr.args(), k, e.ptr, y.ptr, o0.ptr, o1.ptr, st)),
                      lambda: (read(o0, 1 << kp), read(o1, 1 << kp)))
    model = (lambda te, ty: G.phase1_tables(gates, kp, ty, te, p)) if phase == 1 else (lambda te, ty: G.phase2_tables(gates, kp, te, ty, p))
    on_real, on_stale = tuple(model(qe, qy)), tuple(model(pe, py))
    assert not set(fill0 + fill1 + fill_part) & set(on_real[0] + on_real[1] + on_stale[0] + on_stale[1])
    settle_parts(("P", "Q") if phase == 1 else ("Aadd", "Amul"), got, on_real, on_stale)
    assert (I(e.download()), I(y.download())) == (qe, qy), "an input table was modified"


@per_field
def test_gkr_wiring_eval_on_a_busy_stream(gpu, name, cid, p):
    """the sums over the gates, their combine and the copy back: the two results on the host"""
    gates, layer = skewed(p)
    k, kp = layer.k, layer.k_prev
    stale_pt, real_pt = [[vals(p, m, s + i) for i, m in enumerate((k, kp, kp))] for s in (530, 540)]
    stale, real = [[G.eq_table(x, p) for x in pts] for pts in (stale_pt, real_pt)]
    er, eu, ev = (staged(x, y) for x, y in zip(stale, real))
    out = host4(2)
    behind_spin(gpu, [er, eu, ev], lambda st: N.check(gpu.zk_gkr_wiring_eval_dev(cid, layer.n, layer.d_types.ptr, layer.d_in1.ptr, layer.d_in2.ptr, k,
                                                                                 er.ptr, kp, eu.ptr, ev.ptr, N.u64p(out), st)))
    settle_parts(("add", "mul"), tuple(I(out)), G.wiring(gates, *real_pt, p), G.wiring(gates, *stale_pt, p))
    assert [I(x.download()) for x in (er, eu, ev)] == real, "an input table was modified"
