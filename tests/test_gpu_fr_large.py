"""GPU: the multilinear and sumcheck kernels (csrc/mle.hip) at the sizes where a launch shape starts that the integer model
cannot reach in test time: the capped grid's second stride, the fourth fix pass, the fourth coefficient pass.

The inputs are geometric tables T[i] = c g^i with random full-width c and g, so every entry is a distinct full-width field
element, and one table T[i] = r - 1 - i.  A geometric table stays geometric under every operation of these kernels, so exact
expectations cost O(log n) Python integer operations (the closed forms of tests/mle_model.py, which tests/test_mle_model.py
holds to the definitions on the CPU).  An expected TABLE is the closed form's triple expanded by the sequential host recurrence
zk_fr_grand_product, never by a GPU kernel.  Every comparison is == on integers or np.array_equal on limbs.

Each test names the constant of csrc/mle.hip its size sits on; when one of them changes, the test moves with it."""

import ctypes
import os
import random
import re

import numpy as np
import pytest

import mle_model as M
from test_gpu_mle import challenges
from test_gpu_sumcheck import shapes
from zksnake_amd import _native as N
from zksnake_amd import frvec
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD
from zksnake_amd.frvec import DevVec, FrOps
from zksnake_amd.mle import MLE_OBJECT, sumcheck_round
from zksnake_amd.subprotocol import ProductPolynomial, Sumcheck

pytestmark = pytest.mark.gpu

FIELDS = (("BN254", BN254_SCALAR_FIELD), ("BLS12_381", BLS12_381_SCALAR_FIELD))
T = N.MLE_TILE_LOG
TILE = 1 << T
with open(os.path.join(os.path.dirname(os.path.abspath(N.__file__)), "csrc", "mle.hip")) as _f:
    MAX_PARTIALS = int(re.search(r"constexpr unsigned MLE_MAX_PARTIALS = (\d+);", _f.read()).group(1))   # read from the source
GRID = MAX_PARTIALS * TILE     # elements (or pairs) one sweep of the capped grid covers

# sumcheck_round_kernel strides when pairs > MLE_MAX_PARTIALS * MLE_TILE.  The fused form has 2^(log_n - 2) pairs, the unfused
# form 2^(log_n - 1); 21 is the smallest log_n at which the fused form takes a second pair (the unfused then takes four)
ROUND_LOG = (GRID.bit_length() - 1) + 3
# fix_chain makes ceil(k / MLE_TILE_LOG) passes: 3 T + 1 is the smallest k with a fourth
FIX_LOG = 3 * T + 1
# mle_coeffs_impl: nb = min(left, MLE_TILE_LOG - lc) with lc = 0 on the first pass and 2 later, so T + 2 (T - 2) + 1 is the
# smallest log_n with a fourth pass, which has nb = 1: 8 active threads per workgroup
COEFF_LOG = T + 2 * (T - 2) + 1
assert (ROUND_LOG, FIX_LOG, COEFF_LOG) == (21, 25, 21)   # the sizes the issue names; a changed constant fails here, then move the tests

_INPUTS = {}
_EXPANDED = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_the_shared_tables():
    """the shared inputs (512 MiB of HBM) and whatever this file left in the vector pool go back to the device afterwards"""
    yield
    _INPUTS.clear()
    _EXPANDED.clear()
    frvec.release_pool()


def one_limbs(value):
    return np.ascontiguousarray(N.ints_to_limbs([value], 4))


def scalar(out):
    return int.from_bytes(out.tobytes(), "little")


def geo_inputs(p, count, log_n, seed):
    rnd = random.Random(seed + (p & 0xFFFF))
    return [(rnd.randrange(1 << 250, p), rnd.randrange(1 << 250, p), log_n) for _ in range(count)]


def pin_indices(n, seed):
    """about 64 indices: first, last, workgroup edges, the edges of one sweep of the capped grid, random ones"""
    rnd = random.Random(seed)
    fixed = {0, 1, 2, n - 2, n - 1, n // 2 - 1, n // 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, n - TILE - 1, n - TILE,
             GRID - 1, GRID, GRID + 1, 2 * GRID - 1, 2 * GRID, 2 * GRID + TILE, n - GRID - 1, n - GRID}
    fixed = {i for i in fixed if 0 <= i < n}
    while len(fixed) < 64:
        fixed.add(rnd.randrange(n))
    return sorted(fixed)


def build_geo(ops, tab):
    """the table on the device: powers of g times c; pinned at pin_indices against c g^i before anyone uses it"""
    c, g, log_n = tab
    n = 1 << log_n
    vec = ops.d_powers(g, n)
    N.check(N.load().zk_vec_axpby_dev(ops.cid, n, N.u64p(one_limbs(c)), vec.ptr(), None, None, None, vec.ptr(), None))
    for i in pin_indices(n, log_n):
        assert scalar(vec.download(1, i)) == c * pow(g, i, ops.r) % ops.r, f"input table, index {i}"
    return vec


def inputs(p):
    """four geometric tables of 2^ROUND_LOG elements per field on the device (shared by the tests, never modified)"""
    if p not in _INPUTS:
        ops = FrOps(p)
        tabs = geo_inputs(p, 4, ROUND_LOG, seed=1)
        _INPUTS[p] = (tabs, [build_geo(ops, t) for t in tabs])
    return _INPUTS[p]


def expand(ops, tab):
    """the table of a triple as limbs, by the sequential host recurrence: rows 1 .. n of zk_fr_grand_product with num = (c, g, g, ..)
    and den = 1 are c, c g, c g^2, ..  (kept per triple: the two shapes of the chain share their tables)"""
    c, g, log_n = tab
    key = (ops.r, c, g, log_n)
    if key not in _EXPANDED:
        n = 1 << log_n
        num = ops.const(g, n)
        num[0] = one_limbs(c)[0]
        _EXPANDED[key] = ops.grand_product(num, ops.const(1, n))[1:]
    return _EXPANDED[key]


def device_sum(gpu, ops, vec, n):
    out = np.zeros(4, dtype=np.uint64)
    N.check(gpu.zk_mle_sum_dev(ops.cid, n, vec.ptr(), N.u64p(out), None))
    return scalar(out)


def fused_round(gpu, ops, log_n, src, terms, r):
    """zk_sumcheck_round_dev with the challenge as the caller's raw limbs (not reduced): (folded tables, [s(0) .. s(3)])"""
    out = [DevVec(1 << (log_n - 1), zero=False) for _ in src]
    arr = ctypes.c_void_p * len(src)
    deg = (ctypes.c_int * len(terms))(*[len(w) for _, w in terms])
    idx = (ctypes.c_int * (3 * len(terms)))()
    for t_i, (_, which) in enumerate(terms):
        for j, tb in enumerate(which):
            idx[3 * t_i + j] = tb
    coeff = N.ints_to_limbs([c for c, _ in terms], 4)
    s = np.zeros((4, 4), dtype=np.uint64)
    N.check(gpu.zk_sumcheck_round_dev(ops.cid, log_n, len(src), arr(*[v.ptr() for v in src]), len(terms), N.u64p(coeff), deg, idx,
                                      N.u64p(one_limbs(r)), arr(*[v.ptr() for v in out]), N.u64p(s), None))
    return out, N.limbs_to_ints(s)


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_fused_rounds_from_the_strided_grid_down(gpu, name, p):
    """sumcheck_round_kernel at log_n = ROUND_LOG = 21 (threshold: pairs > MLE_MAX_PARTIALS * MLE_TILE) and every level below.
    r == NULL at 21: the unfused kernel over 2^20 pairs, four sweeps of the capped grid, with several tables and terms, and
    mle_combine_kernel over 1024 partials x 4 sums.  r != NULL at 21: 2^19 pairs, a thread takes a second pair and writes a second
    folded pair.  Then one fused round per level down to single elements; at every round s(0 .. 3) equals the closed form, and at
    levels 20, 19, 18 (above, at and below one sweep) and every level <= 10 the folded tables are compared whole."""
    ops = FrOps(p)
    tabs, vecs = inputs(p)
    rnd = random.Random(5)
    rs = [p - 1, p + 5, 0] + [rnd.randrange(p) for _ in range(ROUND_LOG - 3)]
    for label, used in (("gkr", 4), ("degree 2", 2)):       # "degree 2" on two tables is the shape of tools/sumcheck_bench.py
        terms = shapes(p)[label]
        cur_tabs, cur = tabs[:used], vecs[:used]
        assert sumcheck_round(ops, ROUND_LOG, [v.ptr() for v in cur], terms) == M.geo_round_sums(cur_tabs, terms, p), label
        for level in range(ROUND_LOG, 0, -1):
            r = rs[ROUND_LOG - level]
            cur, s = fused_round(gpu, ops, level, cur, terms, r)
            cur_tabs = [M.geo_fix(t, [r % p], p) for t in cur_tabs]
            assert s == M.geo_round_sums(cur_tabs, terms, p), (label, level)
            if level - 1 in (20, 19, 18) or level - 1 <= 10:
                for tb in range(used):
                    assert np.array_equal(cur[tb].download(1 << (level - 1)), expand(ops, cur_tabs[tb])), (label, level - 1, tb)
    for tab, vec in zip(tabs, vecs):
        assert device_sum(gpu, ops, vec, 1 << ROUND_LOG) == M.geo_total(tab, p), "an input table was modified"
    _EXPANDED.clear()


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_prover_at_the_strided_grid(gpu, name, p):
    """Sumcheck.prove_arbitrary and Sumcheck.prove at ROUND_LOG = 21 variables: round 0 is the unfused strided launch, round 1
    the fused one (threshold as above); the verifier's last check runs zk_mle_eval_dev at 21 variables (three fix passes)"""
    tabs, vecs = inputs(p)
    ops = FrOps(p)
    polys = [MLE_OBJECT[p]._wrap(ROUND_LOG, v) for v in vecs]
    sc = Sumcheck(ROUND_LOG, p)
    for label, used in (("degree 2", 2), ("gkr", 4)):
        terms = shapes(p)[label]
        poly = ProductPolynomial(polys[:used], terms, p)
        claim, proof, rs = sc.prove_arbitrary(poly)
        assert (claim, [u.coeffs() for u in proof], rs) == M.geo_prove(tabs[:used], terms, p), label
        assert sc.verify(claim, proof, poly.degree(), mlpoly=poly) == rs
        assert poly.evaluate(rs) == M.geo_f_value(tabs[:used], terms, rs, p)
    claim, proof, rs = sc.prove(polys[3])
    assert (claim, [u.coeffs() for u in proof], rs) == M.geo_prove(tabs[3:], [(1, (0,))], p)
    assert sc.verify(claim, proof, 1, mlpoly=polys[3]) == rs
    assert polys[3].evaluate(rs) == M.geo_evaluate(tabs[3], rs, p)
    for tab, vec in zip(tabs, vecs):
        assert device_sum(gpu, ops, vec, 1 << ROUND_LOG) == M.geo_total(tab, p), "the prover modified an input polynomial"


def fix_work_elems(log_n, k):
    """fix_work_elems of csrc/mle.hip: the first pass's survivors and, with more than two passes, the second pass's"""
    passes = -(-k // T)
    if passes < 2:
        return 0
    return (1 << (log_n - T)) + ((1 << (log_n - 2 * T)) if passes > 2 else 0)


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_four_fix_passes(gpu, name, p):
    """fix_chain with k = FIX_LOG = 25 = 3 MLE_TILE_LOG + 1 (threshold: ceil(k / MLE_TILE_LOG) = 4 passes): pass 2 writes tmp[0]
    again, which pass 0 filled, while pass 1's output in the other half of `work` is its input; zk_mle_eval_dev keeps its result
    slot behind both halves.  k = 24 on the same table is the last three-pass chain and leaves two survivors."""
    ops = FrOps(p)
    log_n = FIX_LOG
    n = 1 << log_n
    tab = geo_inputs(p, 1, log_n, seed=3)[0]
    vec = build_geo(ops, tab)
    special = challenges(p, 6)                                  # 0, 1, r-1, r+5, 2^256-1, r
    assert [special[i] % p for i in (0, 1, 5)] == [0, 1, 0]
    rnd = random.Random(9)
    # The special values on the first and on the last pass.  A challenge of 0 or 1 drops one element of every pair from the result,
    # so on the last passes they come first and the last two challenges are 2^256 - 1 (k = 25) and r + 5 (k = 24): the one-launch
    # fourth pass then depends on both survivors of the third.  The second list is random throughout: with it every element of
    # the table reaches the result, which the 0 and 1 at the head of the first list prevent.
    tail = [special[i] for i in (0, 1, 5, 2, 3, 4)]
    lists = {"special": special + [rnd.randrange(p) for _ in range(log_n - 12)] + tail,
             "random": [rnd.randrange(2, p) for _ in range(log_n)]}
    need = fix_work_elems(log_n, log_n) + 1
    assert need == (1 << 17) + (1 << 9) + 1
    for label, rs in lists.items():
        assert len(rs) == log_n and all(r % p not in (0, 1) for r in rs[-2:])
        raw = N.ints_to_limbs(rs, 4)
        reduced = [r % p for r in rs]
        for k in (log_n, log_n - 1):
            out = DevVec(n >> k, zero=False)
            N.check(gpu.zk_mle_fix_dev(ops.cid, log_n, vec.ptr(), k, N.u64p(raw), out.ptr(), None))
            assert N.limbs_to_ints(out.download(n >> k)) == M.geo_table(M.geo_fix(tab, reduced[:k], p), p), f"fix k={k}, {label}"
        want = M.geo_evaluate(tab, reduced, p)
        for work in (DevVec(need, zero=False), None):
            out = np.zeros(4, dtype=np.uint64)
            N.check(gpu.zk_mle_eval_dev(ops.cid, log_n, vec.ptr(), N.u64p(raw), N.u64p(out), work.ptr() if work else None, None))
            assert scalar(out) == want, f"eval with {'the caller' if work else 'its own'} work buffer, {label}"
    assert device_sum(gpu, ops, vec, n) == M.geo_total(tab, p), "the input table is not c g^i everywhere, or was modified"


def spot_indices(log_n):
    """4096 indices: 0, every 2^b, the last, both sides of the edges of the 256-element tiles of the first coefficient pass and
    of the 64-element segments of the later ones (4 x 64 per tile) near both ends, the rest random"""
    n = 1 << log_n
    idx = {0, n - 1} | {1 << b for b in range(log_n)}
    for step in (256, 64):
        for m in range(1, 17):
            idx |= {m * step - 1, m * step, n - m * step - 1, n - m * step}
    rnd = random.Random(log_n)
    while len(idx) < 4096:
        idx.add(rnd.randrange(n))
    return sorted(idx)


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_four_coefficient_passes(gpu, name, p):
    """mle_coeffs_impl at log_n = COEFF_LOG = 21 (threshold: nb = min(left, MLE_TILE_LOG - lc), lc = 0 then 2, so the passes take
    8 + 6 + 6 + 1 bits): the fourth pass has 8 active threads in each of 2^18 workgroups, and works in place like the second and
    third.  The table r - 1 - i has the coefficients r - 1 at 0, r - 2^b at 2^b and zero elsewhere and is compared whole; a
    geometric table is compared at 4096 indices."""
    ops = FrOps(p)
    log_n = COEFF_LOG
    n = 1 << log_n
    table, want = M.descending_limbs(p, log_n), M.descending_coefficient_limbs(p, log_n)
    d_in, d_out = ops.d_from(table), DevVec(n, zero=False)
    N.check(gpu.zk_mle_coeffs_dev(ops.cid, log_n, d_in.ptr(), d_out.ptr(), None))
    assert np.array_equal(d_out.download(n), want)
    assert np.array_equal(d_in.download(n), table), "the input table was modified"
    N.check(gpu.zk_mle_coeffs_dev(ops.cid, log_n, d_in.ptr(), d_in.ptr(), None))   # in place
    assert np.array_equal(d_in.download(n), want)
    tab, vec = inputs(p)[0][0], inputs(p)[1][0]
    assert tab[2] == log_n
    N.check(gpu.zk_mle_coeffs_dev(ops.cid, log_n, vec.ptr(), d_out.ptr(), None))
    idx = spot_indices(log_n)
    got = N.limbs_to_ints(d_out.download(n)[idx])
    assert got == [M.geo_coefficient(tab, i, p) for i in idx]
    assert device_sum(gpu, ops, vec, n) == M.geo_total(tab, p), "the input table was modified"
