"""The setup-side group kernels (csrc/setup_impl.hip.h) at their lane, block and digit edges, through the public C ABI only:
normalize_kernel (both output forms), dbl_rows_kernel, fixed_table_kernel, fixed_mul_kernel and varbase_mul_kernel.

  A  canonical normalisation through zk_batch_mul: every size around a lane (4), a block of varbase_mul_kernel (128), a workgroup
     of the normalisation (1024) and the threshold of the table path (2048), under every infinity pattern of
     setup_model.infinity_patterns -- made by the scalars 0, r, 2r and, with per-element bases, by an all-zero base
  B  Montgomery-form normalisation and dbl_rows_kernel through ZK_MSM_PRECOMPUTE plans over bases with the same patterns: whole
     runs, one run per window (a wrong table row names its window) and plans for a window range (row 0 after c w doublings)
  C  every row of the fixed table, read with both signs: a random linear combination per window against the closed form
  D  digit, reduction and window edges, and on BN254 the scalar k* whose top-window addition meets its own row (the doubling
     branch of the mixed addition, setup_model's docstring), through the table path and through varbase_mul_kernel
  E  the cache of the fixed table over a sequence of bases

Every comparison is == on limbs.  Expected points come from the CPU oracle (corc.batch_mul / corc.msm), for the reduction and
doubling edges also from oracle/pyref.py in Python integers; no expected point comes from the GPU.  Output buffers start as 0xA5
bytes, so a row the library does not write, or an infinity that is not all zeros, fails the comparison."""

import functools
import random

import numpy as np
import pytest

import setup_model as M
from helpers import window_range_scalars
from oracle import corc, pyref
from zksnake_amd import _native as N

pytestmark = pytest.mark.gpu

GROUPS = [(0, 1), (0, 2), (1, 1), (1, 2)]
IDS = ["BN254_G1", "BN254_G2", "BLS12_381_G1", "BLS12_381_G2"]
VARBASE_SIZES = [1, 2, 3, 4, 5, 7, 8, 127, 128, 129, 1023, 1024, 1025, 2047]
FIXED_SIZES = [2048, 2049, 4095, 4096, 4097]
PLAN_SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 2049]
NMAX = max(FIXED_SIZES)
FILL = 0xA5A5A5A5A5A5A5A5


def _curve(cid):
    return pyref.BN254 if cid == 0 else pyref.BLS12_381


def _limbs(vals):
    return N.ints_to_limbs([int(v) for v in vals], 4)


class _Group:
    """per group, computed once and never changed: NMAX non-zero scalars k_i and a second vector m_i, the oracle's rows k_i G
    and, for the per-element form, m_i (k_i G)"""

    def __init__(self, cid, grp):
        self.cid, self.grp, self.r = cid, grp, _curve(cid).r
        self.g = pyref.Group(_curve(cid), grp)
        self.gen = corc.points_to_limbs([self.g.gen], cid, grp)[0]
        rnd = random.Random(0x5E7 + 2 * cid + grp)
        self.k = [rnd.randrange(1, self.r) for _ in range(NMAX)]
        self.m = [rnd.randrange(1, self.r) for _ in range(max(VARBASE_SIZES))]
        self.k_limbs, self.m_limbs = _limbs(self.k), _limbs(self.m)
        self.rows = corc.batch_mul(cid, grp, self.k_limbs, self.gen, threads=8)
        self.rows2 = corc.batch_mul(cid, grp, self.m_limbs, self.rows[:len(self.m)], threads=8)
        assert self.rows.any(axis=1).all() and self.rows2.any(axis=1).all()
        for a in (self.gen, self.k_limbs, self.m_limbs, self.rows, self.rows2):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _group(cid, grp):
    return _Group(cid, grp)


def _batch_mul(gpu, cid, grp, sc, bases, broadcast):
    sc, bases = np.ascontiguousarray(sc), np.ascontiguousarray(bases)
    n = sc.shape[0]
    out = np.full((n, N.point_limbs(cid, grp)), FILL, dtype=np.uint64)
    N.check(gpu.zk_batch_mul(cid, grp, n, N.u64p(sc), N.u64p(bases), broadcast, N.u64p(out)))
    return out


def _patterns(n):
    return dict({"no infinity": []}, **M.infinity_patterns(n))


# ---- A: canonical normalisation through zk_batch_mul ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,broadcast", [(n, b) for n in VARBASE_SIZES for b in (1, 0)] + [(n, 1) for n in FIXED_SIZES])
@pytest.mark.parametrize("cid,grp", GROUPS, ids=IDS)
def test_batch_mul_sizes_and_infinity_patterns(gpu, cid, grp, n, broadcast):
    G = _group(cid, grp)
    assert (n >= M.FIXED_BASE_MIN) == (n in FIXED_SIZES)
    zero_scalars = _limbs([0, G.r, 2 * G.r])
    base_sc = G.k_limbs[:n] if broadcast else G.m_limbs[:n]
    want = G.rows[:n] if broadcast else G.rows2[:n]
    failed = []
    for name, idx in _patterns(n).items():
        sc = base_sc.copy()
        bases = G.gen if broadcast else G.rows[:n].copy()
        for t, i in enumerate(idx):
            kind = t % (3 if broadcast else 4)
            if kind < 3:
                sc[i] = zero_scalars[kind]
            else:
                bases[i] = 0            # the point at infinity under a non-zero scalar
        exp = want.copy()
        exp[idx] = 0
        got = _batch_mul(gpu, cid, grp, sc, bases, broadcast)
        bad = np.flatnonzero((got != exp).any(axis=1))
        if bad.size:
            failed.append(f"{name}: rows {bad[:8].tolist()} of {bad.size} differ")
    assert not failed, f"n = {n}, broadcast = {broadcast}: " + "; ".join(failed)


# ---- B: Montgomery-form normalisation and dbl_rows_kernel through fixed-base plans -------------------------------------------
def _plan_scalars(G, n, seed):
    rnd = random.Random(seed)
    vals = [rnd.randrange(G.r) for _ in range(n)]
    vals[-1] = G.r - 1
    if n >= 3:
        vals[0], vals[n // 2] = 1, 0
    return vals


def _plan_run(gpu, h, cid, grp, sc, first=0, count=0):
    out = np.full(N.point_limbs(cid, grp), FILL, dtype=np.uint64)
    N.check(gpu.zk_msm_plan_run(h, sc.shape[0], sc.ctypes.data, 0, first, count, N.u64p(out), None))
    return out


def _mixed_bases(G, n):
    """the oracle's rows under the lane subsets (at the start and across the workgroup boundary) and the edge lanes at once"""
    pats = M.infinity_patterns(n)
    bases = G.rows[:n].copy()
    for name in ("lane subsets", "lane subsets across workgroups", "edge lanes"):
        bases[pats.get(name, [])] = 0
    return bases


@pytest.mark.parametrize("c", [0, 9])
@pytest.mark.parametrize("n", PLAN_SIZES)
@pytest.mark.parametrize("cid,grp", GROUPS, ids=IDS)
def test_precompute_plan_over_infinity_patterns(gpu, cid, grp, n, c):
    G = _group(cid, grp)
    sc = _limbs(_plan_scalars(G, n, 300 + n))
    failed = []
    for name, idx in _patterns(n).items():
        bases = G.rows[:n].copy()
        bases[idx] = 0
        exp = corc.msm(cid, grp, sc, bases, threads=8)
        h = N._u64(0)
        N.check(gpu.zk_msm_plan_create(cid, grp, n, bases.ctypes.data, 0, N.MSM_PRECOMPUTE, c, h))
        try:
            if not (_plan_run(gpu, h, cid, grp, sc) == exp).all():
                failed.append(name)
        finally:
            N.check(gpu.zk_msm_plan_destroy(h))
    assert not failed, f"n = {n}, window bits {c}: wrong under " + "; ".join(failed)


@pytest.mark.parametrize("c", [0, 9])
@pytest.mark.parametrize("n", [1025, 2049])
@pytest.mark.parametrize("cid,grp", GROUPS, ids=IDS)
def test_precompute_plan_window_by_window(gpu, cid, grp, n, c):
    """scalars a_i 2^(c w) with 0 < a_i < 2^(c-1): one positive digit in window w and none elsewhere, so the run reads table row
    w alone and a wrong row names its window"""
    G = _group(cid, grp)
    bases = _mixed_bases(G, n)
    rng = np.random.default_rng(400 + n + c)
    h = N._u64(0)
    N.check(gpu.zk_msm_plan_create(cid, grp, n, bases.ctypes.data, 0, N.MSM_PRECOMPUTE, c, h))
    try:
        cb, nw = N._i(0), N._i(0)
        N.check(gpu.zk_msm_plan_windows(h, cb, nw))
        cw, nwin = cb.value, nw.value
        assert (c == 0 or cw == c) and cw * nwin > G.r.bit_length()
        tested = 0
        for w in range(nwin):
            hi = min((1 << (cw - 1)) - 1, (G.r - 1) >> (cw * w))
            if hi < 1:
                assert w == nwin - 1        # above r: the window only ever holds the carry of the one below
                continue
            vals = [int(a) << (cw * w) for a in rng.integers(1, hi + 1, size=n)]
            sc = _limbs(vals)
            assert (_plan_run(gpu, h, cid, grp, sc) == corc.msm(cid, grp, sc, bases, threads=8)).all(), f"window {w} of {nwin} x {cw} bits"
            tested += 1
        assert tested >= nwin - 1
    finally:
        N.check(gpu.zk_msm_plan_destroy(h))


@pytest.mark.parametrize("c", [0, 9])
@pytest.mark.parametrize("cid,grp", GROUPS, ids=IDS)
def test_precompute_plan_for_a_window_range(gpu, cid, grp, c):
    """plans that start at window 1 and at the last window: row 0 of their table is the bases after c w_first doublings, normalised"""
    G, n = _group(cid, grp), 1025
    bases = _mixed_bases(G, n)
    vals = _plan_scalars(G, n, 500 + c)
    sc = _limbs(vals)
    lc, ln = N._i(0), N._i(0)
    N.check(gpu.zk_msm_window_layout(cid, grp, n, N.MSM_PRECOMPUTE, c, lc, ln))
    cw, nwin = lc.value, ln.value
    assert (c == 0 or cw == c) and nwin >= 3
    for first, count in ((1, nwin - 1), (1, 2), (nwin - 1, 1)):
        part = window_range_scalars(cid, grp, vals, cw, nwin, False, first, count)
        exp = corc.msm(cid, grp, _limbs(part), bases, threads=8)
        h = N._u64(0)
        N.check(gpu.zk_msm_plan_create_range(cid, grp, n, bases.ctypes.data, 0, N.MSM_PRECOMPUTE, cw, first, count, h))
        try:
            assert (_plan_run(gpu, h, cid, grp, sc) == exp).all(), f"windows [{first}, {first + count}) of {nwin} x {cw} bits"
            assert (_plan_run(gpu, h, cid, grp, sc, first + count - 1, 1) ==
                    corc.msm(cid, grp, _limbs(window_range_scalars(cid, grp, vals, cw, nwin, False, first + count - 1, 1)), bases, threads=8)).all()
        finally:
            N.check(gpu.zk_msm_plan_destroy(h))


# ---- C: every row of the fixed table, both signs -------------------------------------------------------------------------------
def _table_row_scalars(r, j, negative):
    """(d values, (count, 4) limbs) of the scalars that read the rows of window j: d 2^(16 j) while below r, or (2^16 - d) 2^(16 j),
    whose digits are -d at j and +1 at j + 1"""
    top = (r - 1) >> (16 * j)
    d = np.arange(1, min(M.FIXED_HALF, top) + 1, dtype=np.uint64)
    sc = np.zeros((d.size, 4), dtype=np.uint64)
    field = (np.uint64(1 << 16) - d) if negative else d
    sc[:, j // 4] = field << np.uint64(16 * (j % 4))
    return d, sc


@pytest.mark.parametrize("negative", [0, 1], ids=["positive", "negative"])
@pytest.mark.parametrize("cid,grp", GROUPS, ids=IDS)
def test_every_fixed_table_row(gpu, cid, grp, negative):
    """one zk_batch_mul over the scalars that read each row of each window alone (about 2^19 of them).  Per window the oracle's MSM
    of the returned points under random 128-bit coefficients a_d must be (sum a_d s_d mod r) G: one wrong row survives with
    probability 2^-128.  A seeded sample and the rows 1, 2, 2^15 - 1, 2^15 are also compared one by one.
    (Up to 3 s per case on an MI355X host, nearly all of it the oracle's sixteen MSMs.)"""
    G = _group(cid, grp)
    windows = list(range(15 if negative else 16))        # a negative digit in window 15 would need a window 16
    parts = [_table_row_scalars(G.r, j, negative) for j in windows]
    assert all(d.size == M.FIXED_HALF for (d, _), j in zip(parts, windows) if j < 15)
    if not negative:
        assert parts[-1][0].size == G.r >> 240
    sc = np.ascontiguousarray(np.concatenate([s for _, s in parts]))
    got = _batch_mul(gpu, cid, grp, sc, G.gen, 1)
    rng = np.random.default_rng(600 + negative)
    off = 0
    for j, (d, s) in zip(windows, parts):
        rows = got[off:off + d.size]
        coef = np.zeros((d.size, 4), dtype=np.uint64)
        coef[:, :2] = rng.integers(0, 1 << 63, size=(d.size, 2), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(d.size, 2), dtype=np.uint64)
        a = [lo + (hi << 64) for lo, hi in coef[:, :2].tolist()]
        fields = [(1 << 16) - int(v) if negative else int(v) for v in d.tolist()]
        dot = (sum(x * f for x, f in zip(a, fields)) << (16 * j)) % G.r
        want = corc.batch_mul(cid, grp, _limbs([dot]), G.gen)[0]
        assert (corc.msm(cid, grp, coef, rows, threads=8) == want).all(), f"window {j}: some row differs"
        pick = sorted(set(int(v) for v in rng.integers(1, d.size + 1, size=64)) | {v for v in (1, 2, M.FIXED_HALF - 1, M.FIXED_HALF) if v <= d.size})
        at = np.array(pick) - 1
        assert (rows[at] == corc.batch_mul(cid, grp, s[at], G.gen, threads=8)).all(), f"window {j}: a sampled row differs"
        off += d.size
    assert off == got.shape[0]


# ---- D: digits, reduction and the doubling scalar --------------------------------------------------------------------------------
def _edge_vector(G, n, offsets, seed):
    edges = M.edge_scalars(G.r)
    rnd = random.Random(seed)
    vals = [rnd.randrange(G.r) for _ in range(n)]
    for o in offsets:
        assert o + len(edges) <= n
        vals[o:o + len(edges)] = edges
    return edges, vals


def _check_python_integers(G, vals, got, which):
    for s in which:
        i = vals.index(s)
        assert corc.limbs_to_points(got[i:i + 1], G.cid, G.grp)[0] == G.g.mul(G.g.gen, s % G.r), hex(s)


@pytest.mark.parametrize("cid,grp", GROUPS, ids=IDS)
def test_edge_scalars_through_the_fixed_table(gpu, cid, grp):
    G, n = _group(cid, grp), 2048
    offsets = (0, 257, 1026, 1539)               # each edge scalar at every index residue mod 4 and on both sides of 1024
    edges, vals = _edge_vector(G, n, offsets, 700)
    assert sorted(o % 4 for o in offsets) == [0, 1, 2, 3] and offsets[1] + len(edges) <= 1024 <= offsets[2]
    if cid == 0:
        assert M.top_window_doubling_scalars(G.r)[0] in edges
    sc = _limbs(vals)
    got = _batch_mul(gpu, cid, grp, sc, G.gen, 1)
    exp = corc.batch_mul(cid, grp, sc, G.gen, threads=8)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, f"scalars {[hex(vals[i]) for i in bad[:4]]} at rows {bad[:8].tolist()} differ"
    _check_python_integers(G, vals, got, M.reduction_edges(G.r) + M.doubling_edges(G.r))


@pytest.mark.parametrize("broadcast", [1, 0])
@pytest.mark.parametrize("cid,grp", GROUPS, ids=IDS)
def test_edge_scalars_through_double_and_add(gpu, cid, grp, broadcast):
    G, n = _group(cid, grp), 129
    edges, vals = _edge_vector(G, n, (0,), 701)
    sc = _limbs(vals)
    bases = G.gen if broadcast else G.rows[:n]
    got = _batch_mul(gpu, cid, grp, sc, bases, broadcast)
    exp = corc.batch_mul(cid, grp, sc, bases, threads=8)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, f"scalars {[hex(vals[i]) for i in bad[:4]]} at rows {bad[:8].tolist()} differ"
    if broadcast:
        _check_python_integers(G, vals, got, M.reduction_edges(G.r) + M.doubling_edges(G.r))


# ---- E: the cache of the fixed table -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,grp", GROUPS, ids=IDS)
def test_fixed_table_follows_the_base(gpu, cid, grp):
    """bases A, B, A, -A (same x as A), infinity, A in turn: each call answers for the base it was given"""
    G, n = _group(cid, grp), 2048
    pts = corc.limbs_to_points(G.rows[1:3], cid, grp)
    rows = corc.points_to_limbs([pts[0], pts[1], G.g.neg(pts[0]), None], cid, grp)
    A, B, negA, inf = rows
    assert (A[:A.size // 2] == negA[:A.size // 2]).all() and (A != negA).any() and not inf.any()
    vals = [random.Random(800).randrange(G.r) for _ in range(n)]
    vals[:4] = [0, 1, G.r - 1, G.r + 1]
    sc = _limbs(vals)
    want = {}
    for name, base in (("A", A), ("B", B), ("-A", negA)):
        want[name] = corc.batch_mul(cid, grp, sc, base, threads=8)
    want["infinity"] = np.zeros_like(want["A"])
    for step, (name, base) in enumerate((("A", A), ("B", B), ("A", A), ("-A", negA), ("infinity", inf), ("A", A))):
        got = _batch_mul(gpu, cid, grp, sc, base, 1)
        assert (got == want[name]).all(), f"call {step}: base {name}"
