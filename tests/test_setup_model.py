"""CPU: tests/setup_model.py pinned -- the digit model of fixed_mul_kernel on every edge scalar, the one BN254 scalar whose top
window meets its own table row (and why BLS12-381 has none, no lower window can, and the cancelling twin is r itself), and the
infinity patterns against what their names promise."""

import random

import pytest

import setup_model as M
from oracle import pyref

CURVES = (("BN254", pyref.BN254.r), ("BLS12_381", pyref.BLS12_381.r))
K_STAR_BN254 = 0x3063b18d1ece5fd647afba497e7ea7a2d7cc17b786468f6ebc1e0a6c0fffffff
SIZES = [1, 2, 3, 4, 5, 7, 8, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097]


def _digits_ok(s, r):
    d = M.fixed_digits(s, r)
    assert len(d) == 16
    assert all(-(1 << 15) <= v < 1 << 15 for v in d)
    assert sum(v << (16 * j) for j, v in enumerate(d)) == s % r
    return d


@pytest.mark.parametrize("name,r", CURVES)
def test_fixed_digits_spell_the_reduced_scalar(name, r):
    rnd = random.Random(5)
    for s in M.edge_scalars(r) + [rnd.randrange(1 << 256) for _ in range(2000)]:
        _digits_ok(s, r)
    assert M.fixed_digits(0, r) == [0] * 16 and M.fixed_digits(r, r) == [0] * 16 and M.fixed_digits(2 * r, r) == [0] * 16
    assert M.fixed_digits(1 << 15, r)[:2] == [-(1 << 15), 1]                     # the carry boundary
    assert M.fixed_digits((1 << 15) - 1, r)[:2] == [(1 << 15) - 1, 0]
    assert M.fixed_windows(r) == 16 and M.fixed_bias(16) >> 255 == 1


@pytest.mark.parametrize("name,r", CURVES)
def test_table_row_scalars_read_the_row_they_name(name, r):
    """family C: d 2^(16 j) reads row d of window j alone; (2^16 - d) 2^(16 j) reads it negated, with +1 in the next window"""
    for j in range(16):
        for d in (1, 2, 12345, (1 << 15) - 1, 1 << 15):
            if (d << (16 * j)) < r:
                # d = 2^15 is spelt -2^15 with a carry: the same point through the negated read of row 2^15 and row 1 above
                want = [0] * 16
                if d < 1 << 15:
                    want[j] = d
                else:
                    want[j] = -(1 << 15)
                    want[j + 1] = 1
                assert M.fixed_digits(d << (16 * j), r) == want
            if j < 15:
                neg = M.fixed_digits(((1 << 16) - d) << (16 * j), r)
                assert neg[j] == -d and neg[j + 1] == 1 and not any(v for i, v in enumerate(neg) if i not in (j, j + 1))
    assert (r - 1) >> 240 == r >> 240      # the top window's rows run up to d = r >> 240


def test_the_doubling_scalar_of_bn254():
    r = pyref.BN254.r
    assert M.top_window_doubling_scalars(r) == [K_STAR_BN254]
    k, v = K_STAR_BN254, r >> 240
    assert v == 0x3064 and (r >> 224) & 0xFFFF == 0x4E72 < 0x8000
    assert k == 2 * (v << 240) - r and 0 < k < r
    d = _digits_ok(k, r)
    assert d[15] == v
    low = sum(x << (16 * j) for j, x in enumerate(d[:15]))
    assert low == -(r - (v << 240)) and low % r == (v << 240) % r        # the accumulator IS the row it is about to add
    # r - k* = 2 (r - v 2^240): neither equal nor opposite to its top row; the control differs from k* in the top digit only
    dn = _digits_ok(r - k, r)
    lown = sum(x << (16 * j) for j, x in enumerate(dn[:15]))
    assert dn[15] != 0 and (lown - (dn[15] << 240)) % r != 0 and (lown + (dn[15] << 240)) % r != 0
    c = M.doubling_control(k, r)
    dc = _digits_ok(c, r)
    assert dc[:15] == d[:15] and dc[15] == v - 1
    assert M.doubling_edges(r) == [k, k - 1, k + 1, k + r, r - k, c] and k + r < 1 << 256


def test_bls12_381_has_no_doubling_scalar():
    r = pyref.BLS12_381.r
    assert M.top_window_doubling_scalars(r) == [] and M.doubling_edges(r) == []
    assert r >> 240 == 0x73ED and (r >> 224) & 0xFFFF == 0xA753 >= 0x8000
    # the lower windows cannot reach -(r mod 2^240)
    assert -(r % (1 << 240)) < M.lower_sum_range(15)[0]


@pytest.mark.parametrize("name,r", CURVES)
def test_no_lower_window_can_collide(name, r):
    for j in range(16):
        lo, hi = M.lower_sum_range(j)
        # the extreme digit vectors really are the extremes of the model
        if j:
            s_lo = -M.fixed_bias(j) % (1 << (16 * j))                 # biased fields all zero: every digit -2^15, carry above
            assert sum(v << (16 * i) for i, v in enumerate(M.fixed_digits(s_lo, r)[:j])) == lo
            s_hi = sum(0x7FFF << (16 * i) for i in range(j))
            assert sum(v << (16 * i) for i, v in enumerate(M.fixed_digits(s_hi, r)[:j])) == hi
        if j < 15:
            assert max(-lo, hi) < 1 << (16 * j)                       # never equal as integers ..
            assert max(-lo, hi) + (1 << (16 * j + 15)) < r            # .. and never r apart
            assert not M.window_can_collide(j, r)
    assert M.window_can_collide(15, r)


@pytest.mark.parametrize("name,r", CURVES)
def test_the_cancelling_twin_is_r_itself(name, r):
    """L + d 2^240 = 0 (mod r) with d > 0 and 0 <= L + d 2^240 < 2r leaves r alone, and r is reduced to 0 before the digits are
    cut: every digit is zero, nothing is added, so the cancelling branch of the top-window addition cannot be reached"""
    assert M.top_window_cancelling_scalar(r) == r
    assert M.fixed_digits(r, r) == [0] * 16
    lo, hi = M.lower_sum_range(15)
    top_max = (r >> 240) + 1
    assert 0 < hi + (top_max << 240) < 2 * r                          # so the only multiple of r in reach is r (0 has d = 0)
    for s in (r - 1, r + 1):
        d = M.fixed_digits(s, r)
        assert (sum(v << (16 * j) for j, v in enumerate(d[:15])) + (d[15] << 240)) % r != 0


@pytest.mark.parametrize("name,r", CURVES)
def test_edge_scalar_list(name, r):
    e = M.edge_scalars(r)
    assert len(e) <= M.VARBASE_BLOCK + 1                              # the whole list fits the n = 129 runs
    assert {0, r, 2 * r, (1 << 256) - 1, 1 << 255, (1 << 240) - 1} <= set(e)
    assert max(M.subtractions_needed(s, r) for s in e) == (5 if name == "BN254" else 2)
    q = (1 << 256) // r
    assert M.subtractions_needed(q * r, r) == q and M.subtractions_needed(q * r - 1, r) == q - 1
    for f in (0x8000, 0x7FFF, 0x8001, 0xFFFF):
        assert sum(f << (16 * j) for j in range(16)) in e
    # what the subtractions are for: s - k r spells the same point for every k, as long as the bias does not carry out of the top
    # field.  On BN254 2^256 - 1 needs three of its five subtractions for that (so a loop cut to three still gives the right
    # point and a loop cut to two does not); on BLS12-381 both of its two.
    top, bias = (1 << 256) - 1, M.fixed_bias(16)
    need = 3 if name == "BN254" else 2
    assert top - (need - 1) * r + bias >= 1 << 256 > top - need * r + bias and top - need * r >= 0


@pytest.mark.parametrize("n", SIZES)
def test_infinity_patterns_contain_what_their_names_say(n):
    pats = M.infinity_patterns(n)
    for name, idx in pats.items():
        assert idx and idx == sorted(set(idx)) and 0 <= idx[0] and idx[-1] < n, name
    inf = {name: set(idx) for name, idx in pats.items()}
    for e in range(4):
        name = f"e={e} with finite neighbours"
        assert (name in pats) == (n >= e + 2 and (e > 0 or n >= 14)), name
        for i in pats.get(name, []):
            assert i % 4 == e and 0 <= i - 1 and i + 1 < n and i - 1 not in inf[name] and i + 1 not in inf[name]
    for name, first in (("lane subsets", 0), ("lane subsets across workgroups", 1024 // 4 - 8)):
        if name in pats:
            seen = set()
            for lane in range(first, first + 16):
                seen.add(tuple(4 * lane + e in inf[name] for e in range(4)))
            assert len(seen) == 16 and max(pats[name]) < 4 * (first + 16) and min(pats[name]) >= 4 * first
    assert ("lane subsets" in pats) == (n >= 64) and ("lane subsets across workgroups" in pats) == (n >= 1056)
    if "lane subsets across workgroups" in pats:
        assert min(pats["lane subsets across workgroups"]) < 1024 <= max(pats["lane subsets across workgroups"])
    if n > 4:
        want = set(range(4)) | set(range(1020, 1028))
        assert inf["edge lanes"] == {i for i in want if i < n}
    if n > 1024:
        assert pats["first workgroup"] == list(range(1024))
    assert ("whole workgroup between finite ones" in pats) == (n > 2048)
    if n > 2048:
        assert pats["whole workgroup between finite ones"] == list(range(1024, 2048))
    assert pats["everything"] == list(range(n))
    assert pats.get("everything but the last", []) == list(range(n - 1))
    if n % 4:
        lane = list(range(n - n % 4, n))
        assert pats["ragged lane, last point infinite"] == lane
        assert pats.get("ragged lane, last point finite", []) == lane[:-1]
    else:
        assert not any(name.startswith("ragged") for name in pats)
    # every lane position and the lanes at both ends of a workgroup are met by some pattern with a finite point beside it
    if n >= 1025:
        assert {0, 1023, 1024} <= inf["edge lanes"]
