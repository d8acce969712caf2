"""GPU: PointArray.msm / msm_enqueue / msm_finish, the one way from a PointArray's plan to a point.

Bases of 1, 2, 3 and 70 points (one point, below and at the smallest plans, more than one wave), G1 on both curves and G2 on
BN254; base 1 repeats base 0 and the scalars start r - 1, 1, 0.  Two references that share no code with the plan: the sum of
host scalar multiplications, and `E.multiexp` over the plain list of points (zk_msm, no plan)."""

import random

import pytest

from zksnake_amd import _native as N
from zksnake_amd._algebra import PointArray
from zksnake_amd.ecc import EllipticCurve
from zksnake_amd.frvec import FrOps

pytestmark = pytest.mark.gpu

GROUPS = [("BN254", 1), ("BLS12_381", 1), ("BN254", 2)]
SIZES = [1, 2, 3, 70]


class Case:
    def __init__(self, curve, group, n):
        self.E, self.group, self.n = EllipticCurve(curve), group, n
        rnd = random.Random(100 * n + 10 * self.E.curve_id + group)
        g, r = (self.E.G1() if group == 1 else self.E.G2()), self.E.order
        self.points = [g * rnd.randrange(1, r) for _ in range(n)]
        if n > 1:
            self.points[1] = self.points[0]
        self.ops = FrOps(r)
        self.scalars = [([r - 1, 1, 0] + [rnd.randrange(r) for _ in range(n)])[:n],      # what every case multiplies
                        [rnd.randrange(r) for _ in range(n)]]                              # the second MSM of a pair
        self.limbs = [self.ops.limbs(s) for s in self.scalars]
        self.zero = g * 0

    def array(self):
        return PointArray.from_points(self.E.curve_id, self.group, self.points)

    def host_sum(self, scalars):
        acc = self.zero
        for p, s in zip(self.points, scalars):
            acc = acc + p * s
        return acc


_CASES = {}


@pytest.fixture(params=[(c, g, n) for c, g in GROUPS for n in SIZES], ids=lambda p: f"{p[0]}-G{p[1]}-{p[2]}")
def case(request, gpu):
    if request.param not in _CASES:
        _CASES[request.param] = Case(*request.param)
    return _CASES[request.param]


def test_host_limbs_and_device_vector_agree_with_multiexp(case):
    arr, want = case.array(), case.host_sum(case.scalars[0])
    assert case.E.multiexp(case.points, case.scalars[0]) == want
    assert arr.msm(case.limbs[0]) == want
    vec = case.ops.d_from(case.limbs[0])
    assert arr.msm(vec) == want
    assert arr.msm(vec.ptr(), case.n) == want
    for s in (0, 1, case.E.order - 1):
        assert arr.msm(case.ops.limbs([s] * case.n)) == case.host_sum([s] * case.n)
    assert len(arr._plans) == 1


def test_count_takes_the_prefix(case):
    arr, vec = case.array(), case.ops.d_from(case.limbs[0])
    for count in sorted({1, case.n - 1} - {0, case.n}):
        want = case.E.multiexp(case.points[:count], case.scalars[0][:count])
        assert want == case.host_sum(case.scalars[0][:count])
        assert arr.msm(case.limbs[0], count) == want
        assert arr.msm(vec, count) == want
        assert arr.msm(case.limbs[0][:count]) == want


def test_no_scalars_give_the_identity_without_a_plan(case):
    arr = case.array()
    timings = []
    for point in (arr.msm(case.limbs[0], 0, timings=timings), arr.msm(case.limbs[0][:0]), arr.msm(case.ops.d_from(case.limbs[0]), 0)):
        assert point.is_zero() and type(point) is type(case.zero)
    assert arr._plans == {} and timings == []


def test_more_scalars_than_bases_fail_with_the_length_status(case):
    """zk_msm_plan_run and zk_msm_plan_enqueue end in enqueue_phase: `n_scalars > n_api` is ZK_ERR_LENGTH (csrc/msm_impl.hip.h)"""
    arr = case.array()
    longer = case.ops.limbs(case.scalars[0] + [5])
    for scalars in (longer, case.ops.d_from(longer)):
        with pytest.raises(N.ZkError) as err:
            arr.msm(scalars)
        assert err.value.status == N.ZK_ERR_LENGTH
    with pytest.raises(N.ZkError) as err:
        arr.msm_enqueue(longer)
    assert err.value.status == N.ZK_ERR_LENGTH
    assert arr.msm(case.limbs[0]) == case.host_sum(case.scalars[0])      # the plan is idle and usable afterwards


def test_two_slots_in_flight_finished_in_reverse_order(case):
    arr = case.array()
    first = arr.msm_enqueue(case.ops.d_from(case.limbs[0]), case.n)
    second = arr.msm_enqueue(case.limbs[1], slot=1, concurrent=True)
    assert first[0] != second[0] and len(arr._plans) == 2
    assert arr.msm_finish(second) == case.host_sum(case.scalars[1])
    assert arr.msm_finish(first) == case.host_sum(case.scalars[0])


def test_timings_get_one_float_per_call(case):
    arr, timings = case.array(), []
    arr.msm(case.limbs[0], timings=timings)
    assert len(timings) == 1 and isinstance(timings[0], float) and timings[0] >= 0.0
    arr.msm(case.ops.d_from(case.limbs[1]), timings=timings)
    assert len(timings) == 2 and isinstance(timings[1], float)
