"""GPU: the Python front of the QAP stage (QAP.from_r1cs, evaluate_witness, evaluate_witness_device of groth16/qap.py) and
the sparse products as the prover and the setup use them, on the skewed circuit of tests/spmv_model.py: forward rows of up to
8193 entries, mostly duplicate (row, col) pairs, shuffled triplets, 11 constraints padded to 16, transposes that mix short, long
and empty rows.  Everything by == against Python integers and oracle/pyref.py."""

import random

import numpy as np
import pytest

import spmv_model as S
from oracle import pyref
from zksnake_amd import _native as N
from zksnake_amd.arithmetization import R1CS
from zksnake_amd.device import DeviceBuffer
from zksnake_amd.groth16 import Groth16
from zksnake_amd.groth16.qap import QAP
from zksnake_amd.spmv import LONG_ROW, DeviceCsr

pytestmark = pytest.mark.gpu

CURVES = (("BN254", 0), ("BLS12_381", 1))
TOXIC = (0x1234567, 0x2345678, 0x3456789, 0x456789A, 0x56789AB)     # as tests/test_gpu_groth16.py pins them
BLIND = (0x6789ABC, 0x789ABCD)
NP = S.SKEWED_PADDED
REMAINDER = r"\(U \* V - W\) did not divided by Z to zero"


def _r1cs(trip, curve):
    A, B, C, n_row, n_col, n_pub, _ = trip
    unz = lambda m: tuple(list(t) for t in zip(*m))  # noqa: E731
    return R1CS.from_triplets(unz(A), unz(B), unz(C), n_row, n_col, n_pub, curve)


def _pad(coeffs, n):
    return S.to_limbs(list(coeffs) + [0] * (n - len(coeffs)))


class Case:
    """the skewed circuit over one field with the oracle's answer, computed once and never changed"""

    def __init__(self, name, cid):
        self.name, self.cid = name, cid
        self.cv = pyref.curve_by_name(name)
        self.r = self.cv.r
        self.trip = S.skewed_circuit(self.r)
        self.A, self.B, self.C, self.n_row, self.n_col, self.n_pub, self.w = self.trip
        self.polys = pyref.qap_evaluate_witness(self.A, self.B, self.C, NP, self.w, self.cv)
        u, v, _, h = self.polys
        self.uvh = (_pad(u, NP), _pad(v, NP), _pad(h, NP))
        self.w_limbs = S.to_limbs(self.w)
        self.bad = list(self.w)
        self.bad[S.N_FREE + 4] = (self.bad[S.N_FREE + 4] + 1) % self.r           # one output wire raised by 1

    def qap(self):
        q = QAP(self.r)
        q.from_r1cs(_r1cs(self.trip, self.name))
        return q

    def check(self, res, which="uvh"):
        for key, want in zip("uvh", self.uvh):
            buf = getattr(res, key)
            if key in which:
                assert (buf.download((NP, 4)) == want).all(), f"{key} differs from the oracle's"
            else:
                assert buf is None
        assert res.n == NP and (res.witness.download((self.n_col, 4)) == self.w_limbs).all()


@pytest.fixture(scope="module", params=CURVES, ids=[c[0] for c in CURVES])
def case(request):
    return Case(*request.param)


def garbage(n, seed):
    g = np.random.default_rng(seed).integers(1, 2**64, size=(n, 4), dtype=np.uint64)
    g[:, 3] |= np.uint64(0xF << 60)                                  # above both moduli: no field element
    return g


def _apply(csr, x, seed):
    """csr.apply into n_rows + 1 rows of garbage; the guard row must survive"""
    stale = garbage(csr.n_rows + 1, seed)
    out, dx = DeviceBuffer.from_numpy(stale), DeviceBuffer.from_numpy(S.to_limbs(x))
    csr.apply(dx.ptr, out.ptr)
    got = out.download((csr.n_rows + 1, 4))
    assert (got[-1] == stale[-1]).all(), "the guard row was written"
    assert (dx.download((len(x), 4)) == S.to_limbs(x)).all()
    return S.from_limbs(got[:-1])


# ---- the sparse products as prove() and setup() build them ------------------------------------------------------------------
def test_padded_products(gpu, case):
    r1cs = _r1cs(case.trip, case.name)
    stale = [m.to_csr() for m in (r1cs.A, r1cs.B, r1cs.C)]            # cached at 11 rows: from_r1cs has to drop these
    assert all(rp.shape == (case.n_row + 1,) for rp, _, _ in stale)
    q = QAP(case.r)
    q.from_r1cs(r1cs)
    for k, (m, trip) in enumerate(zip((q.a, q.b, q.c), (case.A, case.B, case.C))):
        assert m.n_row == NP
        row_ptr, cols, vals = m.to_csr()
        assert row_ptr.shape == (NP + 1,)
        csr = DeviceCsr(case.cid, row_ptr, cols, vals)
        assert csr.n_rows == NP and csr.n_long == (7, 7, 0)[k]        # rows above LONG_ROW: 65, 4096, 4097, 8193, 255, 256, 257
        got = _apply(csr, case.w, 70 + k)
        assert got == S.dot_csr(row_ptr, cols, S.from_limbs(vals), case.w, case.r) == pyref.sparse_dot(trip, NP, case.w, case.r)
        assert got[case.n_row:] == [0] * (NP - case.n_row)


def test_transposes_as_setup_uses_them(gpu, case):
    q = case.qap()
    rnd = random.Random(81)
    x = [rnd.randrange(case.r) for _ in range(NP)]
    x[2], x[6] = 0, case.r - 1
    for k, (m, trip) in enumerate(zip((q.a, q.b, q.c), (case.A, case.B, case.C))):
        csc = DeviceCsr(case.cid, *m.to_csc())
        lengths = np.diff(m.to_csc()[0].astype(np.int64))
        assert csc.n_rows == case.n_col and csc.n_long == int((lengths > LONG_ROW).sum()) and (csc.n_long > 0) == (k < 2)
        assert (lengths == 0).any() and (lengths > 0).any()
        assert _apply(csc, x, 80 + k) == S.column_sums(trip, case.n_col, x, case.r)


# ---- the reference-shaped API -----------------------------------------------------------------------------------------------
def test_evaluate_witness_returns_the_four_polynomials(gpu, case):
    polys = case.qap().evaluate_witness(list(case.w))
    assert len(polys) == 4
    for got, want in zip(polys, case.polys):
        assert pyref.strip_zeros(got.coeffs()) == want


# ---- every witness form -----------------------------------------------------------------------------------------------------
def _forms(case):
    r, w, n_pub = case.r, case.w, case.n_pub
    lifted = list(w)
    for i, k in ((0, 1), (3, 5), (S.ZERO_WIRE, 1), (S.MINUS_ONE_WIRE, 5), (len(w) - 1, 1), (150, 5)):
        lifted[i] += k * r
    limbs = case.w_limbs
    above = [v + r if i % 3 == 0 else v for i, v in enumerate(w)]    # w + r < 2r < 2^256 in both fields
    assert max(above) < 1 << 256
    raised = S.to_limbs(above)
    return {
        "ints": list(w),
        "ints_above_r": lifted,
        "limbs": limbs.copy(),
        "limbs_above_r": raised.copy(),
        "ints_limbs": (list(w[:n_pub]), raised[n_pub:].copy()),
        "limbs_ints": (raised[:n_pub].copy(), lifted[n_pub:]),
        "limbs_limbs": (limbs[:n_pub].copy(), raised[n_pub:].copy()),
        "empty_list_part": ([], raised.copy()),
        "empty_limb_part": (lifted, np.zeros((0, 4), dtype=np.uint64)),
    }


FORMS = ["ints", "ints_above_r", "limbs", "limbs_above_r", "ints_limbs", "limbs_ints", "limbs_limbs", "empty_list_part", "empty_limb_part"]


def test_every_witness_form(gpu, case):
    q = case.qap()
    forms = _forms(case)
    assert sorted(forms) == sorted(FORMS)
    for form in FORMS:
        seen = []
        res = q.evaluate_witness_device(forms[form], after_upload=lambda buf: seen.append((buf, buf.download((case.n_col, 4)))))
        assert len(seen) == 1 and seen[0][0] is res.witness, form
        assert (seen[0][1] == case.w_limbs).all(), f"{form}: the witness was not canonical and resident when after_upload ran"
        case.check(res)


# ---- needs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("needs", [{"u"}, {"v"}, {"u", "v"}], ids=["u", "v", "uv"])
def test_needs_without_h(gpu, case, needs):
    q = case.qap()
    res = q.evaluate_witness_device(case.w_limbs, needs=needs)
    case.check(res, which="".join(sorted(needs)))
    assert [d is not None for d in q._dev] == ["u" in needs, "v" in needs, False]
    # without h the witness is not checked against the constraints; u and v of the bad witness are the good ones (only an
    # output wire differs, and those occur in C alone)
    res = q.evaluate_witness_device(list(case.bad), needs=needs)
    for key, want in zip("uv", case.uvh):
        assert (getattr(res, key) is None) == (key not in needs)
        assert key not in needs or (getattr(res, key).download((NP, 4)) == want).all()
    assert res.h is None and [d is not None for d in q._dev] == ["u" in needs, "v" in needs, False]


@pytest.mark.parametrize("needs", [{"u", "h"}, None], ids=["uh", "all"])
def test_needs_with_h_runs_and_checks_the_whole_chain(gpu, case, needs):
    q = case.qap()
    case.check(q.evaluate_witness_device(list(case.w), needs=needs))
    assert all(d is not None for d in q._dev)
    with pytest.raises(ValueError, match=REMAINDER):
        q.evaluate_witness_device(list(case.bad), needs=needs)


# ---- errors leave the object usable -----------------------------------------------------------------------------------------
def test_errors_leave_the_object_usable(gpu, case):
    q = case.qap()
    w = case.w
    case.check(q.evaluate_witness_device(list(w)))
    with pytest.raises(OverflowError) as negative:
        N.ints_to_limbs([1, -1], 4)

    with pytest.raises(ValueError, match=REMAINDER):
        q.evaluate_witness_device(list(case.bad))
    case.check(q.evaluate_witness_device(list(w)))
    with pytest.raises(ValueError, match=REMAINDER):
        q.evaluate_witness_device(S.to_limbs(case.bad))
    case.check(q.evaluate_witness_device(case.w_limbs))
    for wrong in (list(w[:-1]), list(w) + [1], case.w_limbs[:-1], (list(w[:3]), case.w_limbs[2:])):
        with pytest.raises(ValueError, match="witness length does not match"):
            q.evaluate_witness_device(wrong)
        case.check(q.evaluate_witness_device(list(w)))
    with pytest.raises(negative.type):
        q.evaluate_witness_device(list(w[:-1]) + [-1])
    case.check(q.evaluate_witness_device(list(w)))
    with pytest.raises(negative.type):
        q.evaluate_witness_device((case.w_limbs[:3], list(w[3:-1]) + [-1]))
    case.check(q.evaluate_witness_device((case.w_limbs[:3], list(w[3:]))))
    # a one-constraint system: 1 * 1 = 1 over the wire [1]
    one = R1CS.from_triplets(([0], [0], [1]), ([0], [0], [1]), ([0], [0], [1]), 1, 1, 1, case.name)
    q.from_r1cs(one)
    with pytest.raises(ValueError, match="at least 2 rows"):
        q.evaluate_witness_device([1])
    q.from_r1cs(_r1cs(case.trip, case.name))
    case.check(q.evaluate_witness_device(list(w)))


# ---- one QAP object, several circuits ---------------------------------------------------------------------------------------
def test_reuse_across_circuits(gpu, case):
    q = case.qap()
    case.check(q.evaluate_witness_device(list(case.w)))
    A, B, C, n_row, n_col, n_pub, w = chain = pyref.chain_circuit(4, case.r)
    assert (n_row, n_col) != (NP, case.n_col)
    q.from_r1cs(_r1cs(chain, case.name))
    res = q.evaluate_witness_device(S.to_limbs(w))
    u, v, _, h = pyref.qap_evaluate_witness(A, B, C, n_row, w, case.cv)
    assert res.n == n_row
    for buf, want in ((res.u, u), (res.v, v), (res.h, h)):
        assert (buf.download((n_row, 4)) == _pad(want, n_row)).all()
    assert (res.witness.download((n_col, 4)) == S.to_limbs(w)).all()
    q.from_r1cs(_r1cs(case.trip, case.name))
    case.check(q.evaluate_witness_device(case.w_limbs))


# ---- the whole prover -------------------------------------------------------------------------------------------------------
def test_whole_prover_on_the_skewed_circuit(gpu, case):
    """the first proof in the suite whose forward matrices have long rows and duplicate entries and whose transposes mix the
    lane kernel with the long-row kernels"""
    cv, w, n_pub = case.cv, case.w, case.n_pub
    r1cs = _r1cs(case.trip, case.name)
    assert r1cs.is_sat(w[:n_pub], w[n_pub:])
    g = Groth16(r1cs, case.name)
    g._toxic, g._blinding = TOXIC, BLIND
    g.setup()
    proof = g.prove(w[:n_pub], w[n_pub:])
    a, b, c = pyref.groth16_closed_form(case.A, case.B, case.C, NP, case.n_col, n_pub, w, cv, TOXIC, BLIND)
    g1, g2 = pyref.G1(cv), pyref.G2(cv)
    assert proof.to_bytes() == pyref.proof_bytes(cv, (g1.mul(g1.gen, a), g2.mul(g2.gen, b), g1.mul(g1.gen, c)))
    assert g.verify(proof, w[:n_pub])
    forged = list(w[:n_pub])
    forged[1] = (forged[1] + 1) % cv.r
    assert not g.verify(proof, forged)
