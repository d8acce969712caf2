"""CPU: the closed forms of tests/qap_model.py are pinned by two references that share nothing with them -- the CPU oracle's whole
QAP chain (corc.qap_h: transforms over the doubled domain) and a schoolbook product of the coefficient vectors in Python
integers -- and the properties the builders promise (support positions, the cancelling index, h[n-1] = 0, the pass plan) hold at
every size the GPU tests use."""

import pytest

import qap_model as M
from oracle import corc

LOGS = list(range(1, 11))


def ints(x):
    return corc.limbs_to_ints(x)


@pytest.mark.parametrize("log_n", LOGS)
@pytest.mark.parametrize("name,cid", M.CURVES)
def test_monomial_family_equals_the_oracle_chain(name, cid, log_n):
    cv, n = M.curve(name), 1 << log_n
    u = M.mixed(cv, n, 10 + log_n)
    a = corc.ntt(cid, u)
    for f in M.monomial_shifts(n):
        b, c, v, h = M.monomial_case(cid, cv, u, a, f, M.monomial_beta(cv, n, f))
        eu, ev, eh = corc.qap_h(cid, a, b, c)
        assert (eu == u).all() and (ev == v).all() and (eh == h).all(), f
        eu, ev, eh = corc.qap_h(cid, b, a, c)
        assert (eu == v).all() and (ev == u).all() and (eh == h).all(), f
        # dense where it may be: at most the edge zeros of u are zero below f, and nothing is nonzero from f on
        assert not h[f:].any() and h[:f].any(axis=1).sum() >= f - (u[n - f:].any(axis=1) == 0).sum()


@pytest.mark.parametrize("log_n", [x for x in LOGS if x >= 3])
@pytest.mark.parametrize("name,cid", M.CURVES)
def test_reflection_family_equals_the_oracle_chain(name, cid, log_n):
    cv = M.curve(name)
    m = M.Reflection(cv, log_n)
    a = corc.ntt(cid, m.coefficients())
    b, c, u, v, h = m.case(cid, a)
    eu, ev, eh = corc.qap_h(cid, a, b, c)
    assert (eu == u).all() and (ev == v).all() and (eh == h).all()


@pytest.mark.parametrize("log_n", [3, 6])
@pytest.mark.parametrize("name,cid", M.CURVES)
def test_both_families_equal_a_schoolbook_product(name, cid, log_n):
    cv, n = M.curve(name), 1 << log_n
    r, w = cv.r, cv.root_of_unity(n)
    evals = lambda coef: [sum(x * pow(w, e * k, r) for e, x in enumerate(coef)) % r for k in range(n)]  # noqa: E731
    u = M.mixed(cv, n, 20 + log_n)
    a = corc.ntt(cid, u)
    assert ints(a) == evals(ints(u))
    for f in M.monomial_shifts(n):
        beta = M.monomial_beta(cv, n, f)
        b, c, v, h = M.monomial_case(cid, cv, u, a, f, beta)
        assert ints(b) == evals(ints(v)) and ints(v) == [beta if i == f else 0 for i in range(n)]
        assert ints(c) == [x * y % r for x, y in zip(ints(a), ints(b))]
        assert ints(h) == M.schoolbook_high(ints(u), ints(v), r)
    m = M.Reflection(cv, log_n)
    a = corc.ntt(cid, m.coefficients())
    b, c, u, v, h = m.case(cid, a)
    assert ints(a) == evals(ints(u)) and ints(b) == evals(ints(v))
    assert ints(c) == [x * y % r for x, y in zip(ints(a), ints(b))]
    assert ints(h) == M.schoolbook_high(ints(u), ints(v), r)


@pytest.mark.parametrize("name,cid", M.CURVES)
def test_builders_keep_their_promises_at_every_size(name, cid):
    cv = M.curve(name)
    r = cv.r
    for log_n in range(1, 23):
        n = 1 << log_n
        shifts = M.monomial_shifts(n)
        assert shifts == [n // 2, 3 * n // 4, 7 * n // 8][:min(log_n, 3)] and all(0 < f < n for f in shifts)
        betas = [M.monomial_beta(cv, n, f) for f in shifts]
        assert betas.count(r - 1) == 1 and all(0 < x < r for x in betas)
        if log_n < 3:
            continue
        m = M.Reflection(cv, log_n)   # asserts its own promises
        assert set(m.targets) <= set(m.h) and m.h[m.cancel] == 0 and m.cancel not in m.targets
        assert {0, 1, n - 2, n // 2 - 1, n // 2} <= set(m.targets)
        if log_n > 11:
            q = M.plan(log_n)[-1][1]
            assert {2047, 2048, (1 << q) - 1, 1 << q} <= set(m.targets)
        assert n - 1 not in m.h and all(0 <= t < n - 1 for t in m.h)
        assert len(m.v) == len(m.alpha) and m.v[0] == m.alpha[0]
        wrong = M.Reflection(cv, log_n, seed=1)
        assert wrong.alpha != m.alpha    # the seed reaches the coefficients


def test_plan_is_the_digit_table_of_the_transform():
    assert [M.plan(x) for x in (1, 10, 11)] == [[(1, 0)], [(10, 0)], [(11, 0)]]
    assert [[m for m, _ in M.plan(x)] for x in range(12, 17)] == [[6, 6], [7, 6], [8, 6], [8, 7], [8, 8]]
    assert [[m for m, _ in M.plan(x)] for x in range(17, 23)] == [[6, 5, 6], [6, 6, 6], [7, 6, 6], [8, 6, 6], [8, 6, 7], [8, 6, 8]]
    assert [[m for m, _ in M.plan(x)] for x in (23, 24)] == [[8, 7, 8], [8, 8, 8]]
    for log_n in range(12, 25):
        assert sum(m for m, _ in M.plan(log_n)) == log_n
        assert all(q == min(11 - m, log_n - m) for m, q in M.plan(log_n))


def test_flip_limb_changes_one_element_and_stays_canonical():
    cv = M.curve("BN254")
    c = M.limbs([cv.r - 1, 0, 5, cv.r - 2])
    for i in range(4):
        out = M.flip_limb(c, i, cv.r)
        diff = (out != c).any(axis=1)
        assert diff.sum() == 1 and diff[i] and (out[i] != c[i]).sum() == 1 and ints(out)[i] < cv.r
