"""CPU: the host side of csrc/spartan.hip under sanitizers, the new symbols' bindings, and the rules of the Spartan package that
need no GPU: sizes, the merged CSR and its long-segment items against the integer model, and the proof's byte layout."""

import os
import random

import numpy as np
import pytest

import spartan_model as S
from helpers import CURVES, run_host_program
from zksnake_amd import _native as N
from zksnake_amd.ecc import EllipticCurve
from zksnake_amd.spartan import Spartan, SpartanProof
from zksnake_amd.spartan import protocol as SP
from zksnake_amd.spmv import ITEM, LONG_ROW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spartan_host_side_refuses_bad_arguments_under_sanitizers(tmp_path):
    """tests/native/spartan_args_check.cpp, built by the recipe in the header of pcs_args_check.cpp (helpers.run_host_program): a
    host-only compile, an EMPTY offload bundle, link, run.  The sanitizer runtimes are linked into the program; nothing is loaded
    into Python.  The program sees no device on any machine, so the calls that pass the checks fail in the launch with
    ZK_ERR_HIP, which is what it expects."""
    res = run_host_program("spartan_args_check", tmp_path)
    assert res.returncode == 0 and "spartan_args_check: all ok" in res.stdout, res.stdout + res.stderr


def test_symbols_are_bound(lib):
    for name in ("zk_r1cs_products_dev", "zk_r1cs_bind_dev"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    with open(os.path.join(ROOT, "include", "zkmi.h")) as f:
        text = f.read()
    assert f"#define ZK_R1CS_MAX_LOG {N.R1CS_MAX_LOG}\n" in text and f"#define ZK_R1CS_LONG_ROW {N.R1CS_LONG_ROW}\n" in text
    assert N.R1CS_LONG_ROW == LONG_ROW and Spartan is SP.Spartan


def test_sizes_and_column_permutation():
    for n_row, n_col, n_public in ((1, 2, 1), (2, 3, 1), (5, 9, 3), (5, 7, 5), (5, 11, 9), (300, 302, 2), (1 << 24, 3, 2)):
        inst = {"n_row": n_row, "n_col": n_col, "n_public": n_public}
        assert SP.sizes(n_row, n_col, n_public) == S.sizes(inst)
    for bad in ((0, 2, 1), (2, 2, 0), (2, 2, 3), ((1 << 24) + 1, 3, 1), (2, (1 << 24) + 2, 1), (2, (1 << 24) + 2, (1 << 24) + 1)):
        with pytest.raises(ValueError):
            SP.sizes(*bad)


def test_merged_csr_and_long_segments_against_the_model():
    rnd = random.Random(5)
    n_seg, log_seg = 8, 3
    lengths = {(1, 0): LONG_ROW, (2, 1): LONG_ROW + 1, (5, 0): ITEM, (5, 2): ITEM + 1, (5, 1): 3, (7, 2): 2 * ITEM + 5}
    mats = [[], [], []]
    for (seg, m), count in lengths.items():
        mats[m] += [(seg, rnd.randrange(16), rnd.randrange(1, 100)) for _ in range(count)]
    mats[0] += [(0, 1, 7), (0, 1, 8)]                    # a repeated (segment, idx) keeps both entries
    for m in mats:
        rnd.shuffle(m)
    ptr, idx, val = S.merged_csr(n_seg, mats)
    cols = [(np.array([e[0] for e in m], dtype=np.int64), np.array([e[1] for e in m], dtype=np.int64),
             N.ints_to_limbs([e[2] for e in m], 4)) for m in mats]
    g_ptr, g_idx, g_val = SP.merged_csr(log_seg, cols)
    assert g_ptr.dtype == np.uint32 and g_ptr.tolist() == ptr and g_idx.tolist() == idx and N.limbs_to_ints(g_val) == val
    long_segs, item_ptr, items = SP.long_segments(g_ptr)
    assert long_segs.tolist() == [2, 5, 7]               # 64 entries stay short, 65 go long
    # per (long segment, matrix): no item for a short sub-segment, ceil(len / ITEM) items that tile the sub-segment otherwise
    assert item_ptr.shape[0] == 3 * 3 + 1 and item_ptr[0] == 0 and int(item_ptr[-1]) == items.shape[0]
    for j, seg in enumerate(long_segs.tolist()):
        for m in range(3):
            k0, k1 = ptr[3 * seg + m], ptr[3 * seg + m + 1]
            mine = items[item_ptr[3 * j + m]:item_ptr[3 * j + m + 1]].tolist()
            if k1 - k0 <= LONG_ROW:
                assert mine == []
                continue
            assert len(mine) == -(-(k1 - k0) // ITEM) and mine[0][0] == k0 and mine[-1][1] == k1
            assert all(0 < b - a <= ITEM for a, b in mine) and all(x[1] == y[0] for x, y in zip(mine, mine[1:]))
    counts = {(5, 0): 1, (5, 2): 2, (7, 2): 3, (2, 1): 1}
    assert items.shape[0] == sum(counts.values())
    # nothing long: empty arrays of the right shapes
    long_segs, item_ptr, items = SP.long_segments(np.array([0, 1, 1, 2, 2, 2, 2], dtype=np.uint32))
    assert long_segs.shape == (0,) and item_ptr.tolist() == [0] and items.shape == (0, 2)


@pytest.mark.parametrize("name,cid", CURVES, ids=[c[0] for c in CURVES])
def test_proof_bytes_round_trip_and_rejections(name, cid):
    E = EllipticCurve(name)
    p, G = E.order, E.G1()
    nb = 32 if cid == 0 else 48
    rnd = random.Random(9 + cid)
    s_x, s = 3, 4
    draw = lambda k: [rnd.randrange(p) for _ in range(k)]  # noqa: E731
    proof = SpartanProof(G * 5, [draw(4) for _ in range(s_x)], draw(3), [[p - 1, 0, 1] for _ in range(s)], p - 1,
                         [G * 7, E.curve.PointG1.identity(), G * 9], name)
    data = proof.to_bytes()
    assert len(data) == SpartanProof.size(s_x, s, name) == 2 + 4 * nb + 32 * (4 * s_x + 3 + 3 * s + 1) and data[:2] == bytes([s_x, s])
    back = SpartanProof.from_bytes(data, name)
    assert back.to_bytes() == data and back.outer == proof.outer and back.inner == proof.inner and back.evals == proof.evals
    assert back.v_w == p - 1 and back.commitment == proof.commitment and back.opening == proof.opening
    # a wrong length, a header that does not fit the length, a scalar that is not below r, a point that does not decode
    for bad in (data[:-1], data + b"\0", b"", data[:1], bytes([s_x + 1, s]) + data[2:], bytes([s_x, s - 1]) + data[2:],
                bytes([0, s]) + data[2:]):
        with pytest.raises(ValueError):
            SpartanProof.from_bytes(bad, name)
    first = 2 + nb
    for at in (first, first + 32 * (4 * s_x), len(data) - 3 * nb - 32):
        with pytest.raises(ValueError):
            SpartanProof.from_bytes(data[:at] + p.to_bytes(32, "little") + data[at + 32:], name)
    for at in (2, len(data) - nb):
        with pytest.raises(ValueError):
            SpartanProof.from_bytes(data[:at] + b"\xff" * nb + data[at + nb:], name)
