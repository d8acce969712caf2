"""Integer models and expected-value builders for the MSM reduction stages (tests/test_gpu_msm_reduce_stages.py): pair_add and
the XYZZ doubling on Montgomery representatives (add-2008-s / dbl-2008-s-1, extending StepRef of test_field_edges.py), the SumJob
index expression of strided_sum_kernel with the job shapes of reduce_plan (csrc/msm_reduce_plan.h; tests/test_host_lib.py holds
one_step_jobs / two_step_jobs against the C++ word for word), the run profiles of combine_kernel with the tier rule
of the run-offset scan, and pools of input points whose discrete logarithms are known (expected sums are then (sum of logs) G,
checked against chains of pyref.Group.add by the CPU tests).  Nothing here needs a GPU."""

import random

import numpy as np

from oracle import pyref
from test_field_edges import FQ, StepRef, edges, rand_below

COMBINE_SMALL_MAX, COMBINE_WAVE_MAX, COMBINE_WAVE_BLOCKS, COMBINE_BIG_BLOCKS, COMBINE_THREADS, WS_BLOCK = 16, 2048, 128, 64, 256, 128


class Grp:
    def __init__(self, gid, name, f, d, curve, which):
        self.gid, self.name, self.f, self.d, self.curve, self.which = gid, name, f, d, curve, which
        self.g = pyref.Group(curve, which)
        self.p, self.r = f.p, curve.r
        self.ref = PairRef(f, d)
        self.REGS = d * f.N            # registers per coordinate
        self.LIMBS = d * f.W           # 32-bit words per coordinate in memory
        self.XW = 4 * self.LIMBS       # words per XYZZ row

    def __repr__(self):
        return self.name

    # ---- field elements: a coordinate is a tuple of d component integers (Montgomery representatives unless said otherwise)
    def comp(self, x):
        return (x,) if self.d == 1 else tuple(x)

    def plain(self, c):
        return c[0] if self.d == 1 else tuple(c)

    def to_mont(self, x):
        return tuple(v * self.f.R % self.p for v in self.comp(x))

    def rand_elt(self, rnd):
        while True:
            t = tuple(rnd.randrange(self.p) for _ in range(self.d))
            if any(t):
                return t

    def is_zero(self, c):
        return all(v % self.p == 0 for v in c)

    def is_inf(self, pt):
        return self.is_zero(pt[2])

    # ---- points
    def xyzz(self, aff, rnd, lift=None):
        """an XYZZ representative (Montgomery) of the affine point with a random Z: X = x t^2, Y = y t^3, ZZ = t^2, ZZZ = t^3, every
        component then shifted by a random multiple of p inside its range (X: [0, 4p), the rest [0, 2p)); lift = "x_high" puts
        every component of X into [2p, 4p); None (infinity) gives zeros"""
        if aff is None:
            return ((0,) * self.d,) * 4
        m = self.ref.mul
        t = self.rand_elt(rnd)
        t2 = m(t, t)
        t3 = m(t2, t)
        pt = (m(self.to_mont(aff[0]), t2), m(self.to_mont(aff[1]), t3), t2, t3)
        return self.shift(pt, rnd, lift)

    def shift(self, pt, rnd, lift=None):
        p = self.p
        out = []
        for k, c in enumerate(pt):
            hi = 4 if k == 0 else 2
            if k == 0 and lift == "x_high":
                out.append(tuple(v % p + rnd.choice((2, 3)) * p for v in c))
            else:
                out.append(tuple(v % p + rnd.randrange(hi) * p for v in c))
        return tuple(out)

    def to_affine(self, pt):
        """the affine point of an XYZZ representative (the Montgomery factors cancel in X / ZZ and Y / ZZZ), None for ZZ = 0"""
        if self.is_inf(pt):
            return None
        F = self.g.F
        red = lambda c: self.plain(tuple(v % self.p for v in c))  # noqa: E731
        return (F.mul(red(pt[0]), F.inv(red(pt[2]))), F.mul(red(pt[1]), F.inv(red(pt[3]))))

    def neg_pt(self, pt):
        return (pt[0], tuple((-v) % self.p for v in pt[1]), pt[2], pt[3])

    def mul_gen(self, k):
        k %= self.r
        if k == 0:
            return None
        if k > self.r // 2:
            return self.g.neg(pyref.ec_mul(self.g.F, self.g.gen, self.r - k))
        return pyref.ec_mul(self.g.F, self.g.gen, k)

    # ---- encodings
    def regs(self, pt):
        """register form: 29-bit limbs, 4 REGS words"""
        return [l for c in pt for v in c for l in self.f.limbs(v)]

    def unregs(self, words):
        N, d = self.f.N, self.d
        from test_field_edges import val
        return tuple(tuple(val(words[(k * d + j) * N:(k * d + j + 1) * N]) for j in range(d)) for k in range(4))

    def row(self, pt):
        """memory form: packed 32-bit words, XW words"""
        W = self.f.W
        out = []
        for c in pt:
            for v in c:
                assert 0 <= v < 1 << (32 * W)
                out += [(v >> (32 * i)) & 0xFFFFFFFF for i in range(W)]
        return out

    def unrow(self, words):
        W, d = self.f.W, self.d
        ws = [int(x) for x in words]
        comp = lambda i: sum(ws[i * W + j] << (32 * j) for j in range(W))  # noqa: E731
        return tuple(tuple(comp(k * d + j) for j in range(d)) for k in range(4))

    def check_row_range(self, pt):
        """what every stage promises the next one for a stored row: X < 4p, Y / ZZ / ZZZ < 2p, per component"""
        for k, c in enumerate(pt):
            for v in c:
                assert v < (4 if k == 0 else 2) * self.p, (k, hex(v))


class PairRef(StepRef):
    """StepRef plus the XYZZ + XYZZ sum (add-2008-s) and the XYZZ doubling (dbl-2008-s-1, a = 0), with the branch pair_add takes"""

    BRANCHES = ("ordinary", "double", "cancel", "r_zero_only", "left_inf", "right_inf")

    def dbl(self, P):
        X, Y, ZZ, ZZZ = P
        if self.zero(ZZ) or self.zero(Y):
            return None
        U = self.add(Y, Y)
        V = self.mul(U, U)
        W = self.mul(U, V)
        S = self.mul(X, V)
        xx = self.mul(X, X)
        M = self.add(self.add(xx, xx), xx)
        X3 = self.sub(self.mul(M, M), self.add(S, S))
        Y3 = self.sub(self.mul(M, self.sub(S, X3)), self.mul(W, Y))
        return X3, Y3, self.mul(V, ZZ), self.mul(W, ZZZ)

    def pair_add(self, P, Q):
        """(branch, result): result is "P" / "Q" (that operand, unchanged), None (infinity, written as zeros) or the four
        coordinates mod p.  half_is_inf tests the lane's second component (ZZ in the even lane, ZZZ in the odd one) with
        F::is_zero, which takes 0 and p (per component) for zero: both lanes agree only if ZZ and ZZZ vanish together"""
        assert self.zero(P[2]) == self.zero(P[3]) and self.zero(Q[2]) == self.zero(Q[3]), "ZZ = 0 <=> ZZZ = 0 is an input contract"
        if self.zero(Q[2]):
            return "right_inf", "P"
        if self.zero(P[2]):
            return "left_inf", "Q"
        U1, U2 = self.mul(P[0], Q[2]), self.mul(Q[0], P[2])
        S1, S2 = self.mul(P[1], Q[3]), self.mul(Q[1], P[3])
        Pd, Rr = self.sub(U2, U1), self.sub(S2, S1)
        if self.zero(Pd):
            if self.zero(Rr):
                return "double", self.dbl(tuple(tuple(v % self.p for v in c) for c in P))
            return "cancel", None
        PP = self.mul(Pd, Pd)
        PPP = self.mul(Pd, PP)
        Qq = self.mul(U1, PP)
        X3 = self.sub(self.sub(self.mul(Rr, Rr), PPP), self.add(Qq, Qq))
        Y3 = self.sub(self.mul(Rr, self.sub(Qq, X3)), self.mul(S1, PPP))
        ZZ3 = self.mul(self.mul(P[2], Q[2]), PP)
        ZZZ3 = self.mul(self.mul(P[3], Q[3]), PPP)
        return ("r_zero_only" if self.zero(Rr) else "ordinary"), (X3, Y3, ZZ3, ZZZ3)


GROUPS = [Grp(0, "BN254_G1", FQ[0], 1, pyref.BN254, 1), Grp(1, "BN254_G2", FQ[0], 2, pyref.BN254, 2),
          Grp(2, "BLS12_381_G1", FQ[1], 1, pyref.BLS12_381, 1), Grp(3, "BLS12_381_G2", FQ[1], 2, pyref.BLS12_381, 2)]


def cube_root_of_unity(p):
    """a primitive cube root of unity of F_p (p = 1 mod 3 for both base fields: the curves have a = 0 and order-3 automorphisms)"""
    assert p % 3 == 1
    for g in range(2, 50):
        w = pow(g, (p - 1) // 3, p)
        if w != 1:
            assert pow(w, 3, p) == 1
            return w
    raise AssertionError


# ---- pair_add records ----------------------------------------------------------------------------------------------------------
def real_points(G, n, seed):
    """n distinct affine points a_i G with their a_i (a_0 random, then steps of a fixed random difference: one affine addition each)"""
    rnd = random.Random(seed)
    a0, dlt = rnd.randrange(1 << 40, 1 << 41), rnd.randrange(1 << 40, 1 << 41)
    P, D = G.mul_gen(a0), G.mul_gen(dlt)
    out = []
    for i in range(n):
        out.append((P, a0 + i * dlt))
        P = G.g.add(P, D)
    return out


def disguise(G, pt, rnd):
    """another representative of the same point: other Z (ZZ t^2, ZZZ t^3, X t^2, Y t^3), then shifts by multiples of p"""
    m = G.ref.mul
    t = G.rand_elt(rnd)
    t2 = m(t, t)
    t3 = m(t2, t)
    return G.shift((m(pt[0], t2), m(pt[1], t3), m(pt[2], t2), m(pt[3], t3)), rnd)


def pair_add_records(G, seed, n_ordinary=400, n_special=24):
    """list of (P, Q, wanted branch or None): every branch of pair_add by construction.  Ordinary records draw every coordinate at
    its documented bound with the generators of test_field_edges (X: 4p; Y, ZZ, ZZZ: 2p; 20 % on an edge) -- the formulas are
    polynomial identities, the operands need not be curve points; the special cases are built from curve points"""
    rnd = random.Random(seed)
    f, d, p, ref = G.f, G.d, G.p, G.ref
    e4, e2 = edges(f, 4), edges(f, 2)

    def rv(k):
        return rnd.choice(e4 if k == 4 else e2) if rnd.random() < 0.2 else rand_below(rnd, k * p)

    def rand_pt():
        while True:
            pt = tuple(tuple(rv(4 if k == 0 else 2) for _ in range(d)) for k in range(4))
            if ref.zero(pt[2]) == ref.zero(pt[3]):
                return pt

    recs = [(rand_pt(), rand_pt(), None) for _ in range(n_ordinary)]
    pts = real_points(G, n_special, seed + 1)
    w = cube_root_of_unity(p)
    zero = ((0,) * d,) * 4
    p_inf = lambda pt: (pt[0], pt[1], (p,) * d, (p,) * d)  # noqa: E731  "infinity" as ZZ = ZZZ = p (every component)
    for aff, _ in pts:
        P = G.xyzz(aff, rnd)
        recs.append((P, disguise(G, P, rnd), "double"))
        recs.append((P, disguise(G, G.neg_pt(P), rnd), "cancel"))
        x2 = tuple(v * w % p for v in G.comp(aff[0]))                      # (w x, y) is on the curve too: same y, other x
        recs.append((P, G.xyzz((G.plain(x2), aff[1]), rnd), "r_zero_only"))
        recs.append((zero, P, "left_inf"))
        recs.append((P, zero, "right_inf"))
        recs.append((zero, zero, "right_inf"))
        recs.append((p_inf(rand_pt()), P, "left_inf"))
        recs.append((P, p_inf(rand_pt()), "right_inf"))
        # coordinates equal to p as representatives of zero elsewhere than ZZ: an ordinary addition
        recs.append(((tuple(p for _ in range(d)),) + rand_pt()[1:], rand_pt(), None))
    return recs


def wave_layouts(G, seed):
    """two blocks of 32 records (one wave each): every pair doubles; exactly one pair (in the middle of the wave) doubles"""
    rnd = random.Random(seed)
    pts = [G.xyzz(aff, rnd) for aff, _ in real_points(G, 64, seed + 1)]
    all_dbl = [(pts[i], disguise(G, pts[i], rnd), "double") for i in range(32)]
    one_dbl = [(pts[i], disguise(G, pts[i], rnd), "double") if i == 13 else (pts[i], pts[32 + i], "ordinary") for i in range(32)]
    return all_dbl, one_dbl


def check_pair_add(G, P, Q, got_words):
    """the output record against the model: branch taken, exact coordinates mod p, ranges and limb normalisation"""
    from test_field_edges import is_norm
    N, d, p = G.f.N, G.d, G.p
    got = G.unregs(got_words)
    branch, e = G.ref.pair_add(P, Q)
    if e == "P" or e == "Q":
        assert got == (P if e == "P" else Q), f"{branch}: the other operand must come back unchanged"
        return branch, got
    for k in range(4):
        for j in range(d):
            base = (k * d + j) * N
            assert is_norm(got_words[base:base + N]), (k, j)
    G.check_row_range(got)
    if e is None:
        assert all(v == 0 for c in got for v in c), f"{branch}: infinity is written as zeros"
    else:
        assert tuple(tuple(v % p for v in c) for c in got) == e, branch
    return branch, got


# ---- pools of input points for the kernels ----------------------------------------------------------------------------------------
KINDS = ("random", "all_equal", "alternating", "mostly_inf", "small_multiples", "x_high")


class Pool:
    """encoded rows with known discrete logarithms; inputs of a kernel are index arrays into the pool"""

    def __init__(self, G, kind, seed, size=96):
        rnd = random.Random(seed)
        self.G, self.kind = G, kind
        self.affine, self.scalar, pts = [], [], []

        def put(aff, a, lift=None, pt=None):
            self.affine.append(aff)
            self.scalar.append(a)
            pts.append(pt if pt is not None else G.xyzz(aff, rnd, lift))

        if kind in ("random", "x_high", "mostly_inf"):
            for aff, a in real_points(G, size, seed + 1):
                put(aff, a, "x_high" if kind == "x_high" else None)
            if kind == "mostly_inf":
                put(None, 0)
                junk = G.xyzz(self.affine[0], rnd)
                put(None, 0, pt=(junk[0], junk[1], (G.p,) * G.d, (G.p,) * G.d))   # infinity as ZZ = ZZZ = p
        elif kind == "all_equal":
            aff, a = real_points(G, 1, seed + 1)[0]
            for _ in range(8):
                put(aff, a)
        elif kind == "alternating":
            aff, a = real_points(G, 1, seed + 1)[0]
            for i in range(8):
                put(aff if i % 2 == 0 else G.g.neg(aff), a if i % 2 == 0 else -a)
        elif kind == "small_multiples":
            for a in (1, -1, 2, -2, 3, -3):
                for _ in range(2):
                    put(G.mul_gen(a), a)
            put(None, 0)
        else:
            raise AssertionError(kind)
        self.points = pts
        self.rows = np.array([G.row(pt) for pt in pts], dtype=np.uint32)
        self.n_real = size if kind == "mostly_inf" else len(pts)

    def draw(self, n, seed):
        """n pool indices of this kind's pattern"""
        rng = np.random.default_rng(seed)
        k = len(self.points)
        if self.kind == "alternating":
            return (np.arange(n) % 2 + 2 * rng.integers(0, k // 2, size=n)).astype(np.int64)   # P, -P, P, .. in random representatives
        if self.kind == "mostly_inf":
            idx = self.n_real + rng.integers(0, 2, size=n)
            hit = rng.random(n) < 0.08
            idx[hit] = rng.integers(0, self.n_real, size=int(hit.sum()))
            return idx.astype(np.int64)
        return rng.integers(0, k, size=n).astype(np.int64)

    def expected(self, idx, weights=None):
        """sum_j w_j X_{idx_j} as an affine point (None = infinity), from the logarithms"""
        s = 0
        for t, i in enumerate(idx):
            s += self.scalar[int(i)] * (1 if weights is None else int(weights[t]))
        return self.G.mul_gen(s)

    def expected_by_addition(self, idx, weights=None):
        """the same by a chain of pyref additions (the definition; the CPU tests hold `expected` against it)"""
        g, acc = self.G.g, None
        for t, i in enumerate(idx):
            for _ in range(1 if weights is None else int(weights[t])):
                acc = g.add(acc, self.affine[int(i)])
        return acc


def check_out_row(G, words, want):
    """a stored output row: its range promise, and the same group element as `want`"""
    pt = G.unrow(words)
    G.check_row_range(pt)
    got = G.to_affine(pt)
    assert got == want, (got, want)


# ---- strided_sum_kernel ----------------------------------------------------------------------------------------------------------
class SumJob:
    FIELDS = ("n_out", "per_group", "group_stride", "outer", "inner", "count", "out_offset", "split", "outer2", "in_offset")

    def __init__(self, n_out, per_group, group_stride, outer, inner, count, out_offset, split=1, outer2=0, in_offset=0):
        self.n_out, self.per_group, self.group_stride, self.outer, self.inner, self.count = n_out, per_group, group_stride, outer, inner, count
        self.out_offset, self.split, self.outer2, self.in_offset = out_offset, split, outer2, in_offset

    def words(self):
        return np.array([getattr(self, k) for k in self.FIELDS], dtype=np.uint32)

    def index(self, o, j):
        """the point strided_sum_kernel reads as term j of output o (msm_reduce.hip.h)"""
        x = o % self.per_group
        return self.in_offset + (o // self.per_group) * self.group_stride + (x // self.split) * self.outer + (x % self.split) * self.outer2 + j * self.inner

    def max_index(self):
        return max((self.index(o, self.count - 1) for o in range(self.n_out)), default=-1)


def one_step_jobs(groups, R, C):
    """rows and columns of `groups` bucket sets of R x C buckets (the one-step form of reduce_plan, csrc/msm_reduce_plan.h)"""
    Bk = R * C
    n_rows, n_cols = groups * R, groups * C
    return SumJob(n_rows, R, Bk, C, 1, C, 0), SumJob(n_cols, C, Bk, 1, C, R, n_rows)


def two_step_jobs(groups, R, C, K):
    """(prow, pcol), (frow, fcol), lpo2: partial sums over runs of K buckets, then the sums of the partial sums (the two-step form
    of reduce_plan)"""
    assert K >= 2 and C % K == 0 and R % K == 0 and C // K >= 2 and R // K >= 2
    Bk = R * C
    n_rows, n_cols = groups * R, groups * C
    pr, pc = C // K, R // K
    prow = SumJob(n_rows * pr, R * pr, Bk, C, 1, K, 0, pr, K)
    pcol = SumJob(n_cols * pc, C * pc, Bk, 1, C, K, n_rows * pr, pc, K * C)
    frow = SumJob(n_rows, n_rows, 0, pr, 1, pr, 0)
    fcol = SumJob(n_cols, n_cols, 0, pc, 1, pc, n_rows, 1, 0, n_rows * pr)
    return (prow, pcol), (frow, fcol), 2 * min(32, max(pr, pc) // 2)


def job_terms(job):
    """per output: the input indices it sums"""
    return [[job.index(o, j) for j in range(job.count)] for o in range(job.n_out)]


# ---- weighted_sum_kernel -------------------------------------------------------------------------------------------------------------
def weighted_blocks(m0, n0, m1):
    """per launched block: (array 0 / 1, array index, first point, length), in the kernel's block order"""
    out = []
    for which, m in ((0, m0), (1, m1)):
        for a in range(n0):
            for b in range(0, m, WS_BLOCK):
                out.append((which, a, b, min(WS_BLOCK, m - b)))
    return out


# ---- combine_kernel ---------------------------------------------------------------------------------------------------------------------
def tier_of(runs):
    if runs == 0:
        return "empty"
    if runs == 1:
        return "single"
    if runs <= COMBINE_SMALL_MAX:
        return "small"
    return "wave" if runs <= COMBINE_WAVE_MAX else "big"


def combine_profile(run_counts):
    """run_start (n_keys + 1), big_list (n_keys), big_count (2) for the given runs per key, by the rule of the run-offset scan
    (msm_sort.hip.h): more than COMBINE_WAVE_MAX runs -> listed from the back, more than COMBINE_SMALL_MAX -> from the front"""
    n_keys = len(run_counts)
    run_start = np.zeros(n_keys + 1, dtype=np.uint32)
    run_start[1:] = np.cumsum(np.asarray(run_counts, dtype=np.uint64)).astype(np.uint32)
    big_list = np.zeros(n_keys, dtype=np.uint32)
    big_count = np.zeros(2, dtype=np.uint32)
    for key, r in enumerate(run_counts):
        if r > COMBINE_WAVE_MAX:
            big_list[n_keys - 1 - int(big_count[1])] = key
            big_count[1] += 1
        elif r > COMBINE_SMALL_MAX:
            big_list[int(big_count[0])] = key
            big_count[0] += 1
    return run_start, big_list, big_count
