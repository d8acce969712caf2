"""Integer model of the setup-side group kernels (csrc/setup_impl.hip.h): the signed 16-bit digits fixed_mul_kernel cuts a scalar
into, the one scalar whose top-window addition meets its own table row, the index sets of infinite points that the batched
normalisation is tested on, and the edge scalars of tests/test_gpu_setup_kernels.py.  Python integers only: no point, no oracle.

The collision argument.  fixed_mul_kernel adds table row |d_j| 2^(16 j) G (negated for d_j < 0) per window, lowest first.  Before
window j the accumulator holds L_j G with L_j = sum_{i<j} d_i 2^(16 i), and |L_j| <= 2^15 (2^(16 j) - 1) / (2^16 - 1) < 2^(16 j).
The mixed addition takes its same-x branch when L_j = +-d_j 2^(16 j) (mod r), d_j != 0.  As integers that cannot be
(|d_j| 2^(16 j) >= 2^(16 j) > |L_j|); a multiple of r between them needs |L_j| + 2^15 2^(16 j) >= r, and the left side is below
2^(16 j + 16) <= 2^240 < r for j < 15.  So only the top window can collide.  There the digit d is positive and
L - d 2^240 = -r (doubling) or L + d 2^240 = +r (cancellation).  The second is the scalar r itself, which is reduced to 0
before the digits are cut and adds nothing; the first is s = L + d 2^240 = 2 d 2^240 - r, which is below r for every d up to the
top digit of r, but its lower windows must be able to hold L = d 2^240 - r: that leaves d = r >> 240 and asks that r mod 2^240
is at most 2^15 (2^240 - 1) / (2^16 - 1), the most negative value fifteen windows can spell."""

FIXED_C = 16
FIXED_HALF = 1 << (FIXED_C - 1)
NORM_E = 4                 # points per lane of normalize_kernel
NORM_GROUP = 1024          # points per workgroup (256 lanes), i.e. per field inversion
VARBASE_BLOCK = 128
FIXED_BASE_MIN = 2048      # zk_batch_mul with one base: the table path from here on


def fixed_windows(r):
    return (r.bit_length() + 1 + FIXED_C - 1) // FIXED_C


def fixed_bias(nwin):
    return sum(FIXED_HALF << (FIXED_C * j) for j in range(nwin))


def fixed_digits(s, r):
    """the signed digits of s mod r as fixed_mul_kernel takes them: 16-bit fields of (s mod r) + bias, each minus 2^15"""
    nwin = fixed_windows(r)
    t = s % r + fixed_bias(nwin)
    assert t >> (FIXED_C * nwin) == 0, "the top field overflows"
    return [((t >> (FIXED_C * j)) & 0xFFFF) - FIXED_HALF for j in range(nwin)]


def lower_sum_range(j):
    """(min, max) of L_j = sum_{i<j} d_i 2^(16 i) over all digit vectors"""
    ones = sum(1 << (FIXED_C * i) for i in range(j))
    return -FIXED_HALF * ones, (FIXED_HALF - 1) * ones


def window_can_collide(j, r):
    """the bound argument for window j: can L_j = +-d_j 2^(16 j) (mod r) hold for some d_j != 0 at all?"""
    lo, hi = lower_sum_range(j)
    reach = max(-lo, hi)
    as_integers = reach >= 1 << (FIXED_C * j)                       # |L_j| against the smallest non-zero |d_j| 2^(16 j)
    around_r = reach + (FIXED_HALF << (FIXED_C * j)) >= r           # |L_j -+ d_j 2^(16 j)| against r
    return as_integers or around_r


def top_window_doubling_scalars(r):
    """every s in [0, r) for which the last addition of fixed_mul_kernel adds a point to itself"""
    nwin = fixed_windows(r)
    top = FIXED_C * (nwin - 1)
    lo, hi = lower_sum_range(nwin - 1)
    out = []
    for d in range(1, (r >> top) + 2):                   # the top digit of s < r is at most (r >> top) + 1
        low = (d << top) - r                             # what the lower windows must sum to
        if not lo <= low <= hi:
            continue
        s = low + (d << top)
        if 0 <= s < r:
            dg = fixed_digits(s, r)
            assert dg[-1] == d and sum(v << (FIXED_C * i) for i, v in enumerate(dg[:-1])) == low
            out.append(s)
    return out


def top_window_cancelling_scalar(r):
    """the smallest positive integer whose lower windows sum to minus its top row: L + d 2^top = 0 (mod r) with d > 0"""
    return r


def doubling_control(k, r):
    """the lower windows of k under a top digit one less: the same accumulator meets the neighbouring row"""
    top = FIXED_C * (fixed_windows(r) - 1)
    return k - (1 << top)


# ---- infinity patterns of the batched normalisation -------------------------------------------------------------------------
def infinity_patterns(n):
    """name -> sorted indices below n that are made infinite; only the patterns that exist at n (never an empty one)"""
    pats = {}

    def put(name, idx):
        idx = sorted(set(i for i in idx if 0 <= i < n))
        if idx:
            pats[name] = idx

    for e in range(NORM_E):
        # every third lane, so that both neighbours of each infinity stay finite; a neighbour must exist on both sides
        put(f"e={e} with finite neighbours", [i for i in range(e, n - 1, NORM_E) if (i // NORM_E) % 3 == 0 and i >= 1])
    if n >= 16 * NORM_E:
        put("lane subsets", [NORM_E * lane + e for lane in range(16) for e in range(NORM_E) if lane >> e & 1])
    if n >= NORM_GROUP + 8 * NORM_E:
        first = NORM_GROUP // NORM_E - 8   # sixteen lanes, eight on each side of the workgroup boundary
        put("lane subsets across workgroups", [NORM_E * (first + lane) + e for lane in range(16) for e in range(NORM_E) if lane >> e & 1])
    if n > NORM_E:
        put("edge lanes", list(range(0, 4)) + list(range(NORM_GROUP - 4, NORM_GROUP)) + list(range(NORM_GROUP, NORM_GROUP + 4)))
    if n > NORM_GROUP:
        put("first workgroup", range(NORM_GROUP))
    if n > 2 * NORM_GROUP:
        put("whole workgroup between finite ones", range(NORM_GROUP, 2 * NORM_GROUP))
    put("everything", range(n))
    put("everything but the last", range(n - 1))
    if n % NORM_E:
        lane = range(n - n % NORM_E, n)
        put("ragged lane, last point finite", lane[:-1])
        put("ragged lane, last point infinite", lane)
    return pats


# ---- edge scalars -----------------------------------------------------------------------------------------------------------
def reduction_edges(r):
    q = (1 << 256) // r
    return [0, 1, 2, r - 2, r - 1, r, r + 1, 2 * r - 1, 2 * r, 2 * r + 1, q * r - 1, q * r, (1 << 256) - 1]


def window_edges():
    out = []
    for j in range(16):
        for b in (FIXED_C * j, FIXED_C * j + FIXED_C - 1):
            out += [v for v in ((1 << b) - 1, 1 << b, (1 << b) + 1) if 0 <= v < 1 << 256]
    return out


def digit_patterns():
    return [sum(f << (16 * j) for j in range(16)) for f in (0x8000, 0x7FFF, 0x8001, 0xFFFF)]


def doubling_edges(r):
    out = []
    for k in top_window_doubling_scalars(r):
        out += [k, k - 1, k + 1, k + r, r - k, doubling_control(k, r)]
    return out


def edge_scalars(r):
    """family D: every scalar below 2^256, duplicates kept (the list is placed, not deduplicated)"""
    out = reduction_edges(r) + window_edges() + digit_patterns() + doubling_edges(r)
    assert all(0 <= v < 1 << 256 for v in out)
    return out


def subtractions_needed(s, r):
    return s // r
