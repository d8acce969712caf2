"""CPU: the host side of csrc/mlpcs.hip under sanitizers, the new symbol's binding, and the rules of MultilinearKZG that need no
GPU: constructor limits, size errors (raised before anything moves to the device) and the verifier, which runs on the host and
needs `G2_tau` only."""

import os
import random

import pytest

import mlpcs_model as M
from helpers import CURVES, run_host_program
from zksnake_amd import _native as N
from zksnake_amd.commitment.polynomial import MultilinearKZG
from zksnake_amd.ecc import EllipticCurve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mlpcs_host_side_refuses_bad_arguments_under_sanitizers(tmp_path):
    """tests/native/mlpcs_args_check.cpp, built by the recipe in the header of pcs_args_check.cpp (helpers.run_host_program, as
    test_host_lib.py builds ipa_args_check): a host-only compile, an EMPTY offload bundle, link, run.  The sanitizer runtimes are
    linked into the program; nothing is loaded into Python.  The program sees no device on any machine, so the calls that pass
    the checks fail in the launch with ZK_ERR_HIP, which is what it expects."""
    res = run_host_program("mlpcs_args_check", tmp_path)
    assert res.returncode == 0 and "mlpcs_args_check: all ok" in res.stdout, res.stdout + res.stderr


def test_symbol_is_bound(lib):
    assert "zk_mlpcs_quotients_dev" in N.SIGNATURES and hasattr(lib, "zk_mlpcs_quotients_dev")
    with open(os.path.join(ROOT, "include", "zkmi.h")) as f:
        assert f"#define ZK_MLPCS_MAX_LOG {N.MLPCS_MAX_LOG}\n" in f.read()


def test_constructor_limits():
    with pytest.raises(ValueError):
        MultilinearKZG(N.MLPCS_MAX_LOG + 1, "BN254")
    with pytest.raises(ValueError):
        MultilinearKZG(-1, "BLS12_381")
    with pytest.raises(KeyError):
        MultilinearKZG(4, "no such curve")
    for name, _ in CURVES:
        s = MultilinearKZG(N.MLPCS_MAX_LOG, name)
        assert s.num_vars == 24 and not s.is_setup and s.G2_tau is None and s.name == "MultilinearKZG"
        assert MultilinearKZG(0, name).num_vars == 0
        for call in (lambda: s.commit([1, 2]), lambda: s.open([1, 2], [3]), lambda: s.batch_open([[1, 2]], [3]),
                     lambda: s.verify(None, [], [], 0)):
            with pytest.raises(RuntimeError):
                call()
        s.release()   # nothing to free: a no-op


def verifier(name, n, tau):
    """a scheme that can only verify: tau_k G2 by host scalar multiplications"""
    s = MultilinearKZG(n, name)
    s.G2_tau = [s.E.G2() * t for t in tau]
    return s


@pytest.mark.parametrize("name,cid", CURVES, ids=[c[0] for c in CURVES])
def test_size_errors_come_before_any_device_work(name, cid):
    s = verifier(name, 3, [5, 6, 7])
    s._levels, s.is_setup = [], True     # past the setup check only: every call below must raise before it touches a level
    with pytest.raises(ValueError):
        s.commit(list(range(16)))                 # m = 4 > num_vars
    with pytest.raises(ValueError):
        s.open(list(range(16)), [1, 2, 3, 4])
    with pytest.raises(ValueError):
        s.open([1, 2, 3, 4], [1])                 # len(point) != m
    with pytest.raises(ValueError):
        s.open([1, 2, 3, 4], [1, 2, 3])
    with pytest.raises(ValueError):
        s.open([7], [1])                          # m = 0 takes the empty point
    with pytest.raises(ValueError):
        s.commit([1, 2, 3])                       # not a power of two
    with pytest.raises(ValueError):
        s.commit([])
    with pytest.raises(ValueError):
        s.batch_open([[1, 2], [1, 2, 3, 4]], [1])
    with pytest.raises(ValueError):
        s.batch_open([[1, 2], [3, 4]], [1, 2])
    with pytest.raises(ValueError):
        s.batch_open([], [])
    with pytest.raises(TypeError):
        s.commit("table")
    s._levels = None


@pytest.mark.parametrize("name,cid", CURVES, ids=[c[0] for c in CURVES])
def test_verifier_on_the_host_against_the_model(name, cid):
    """commitment and proof built from the integer model by host scalar multiplications: accepted, also for m < n and with
    identity points; malformed or wrong input gives False and never raises"""
    E = EllipticCurve(name)
    p, G = E.order, E.G1()
    rnd = random.Random(11 + cid)
    n = 3
    tau = [rnd.randrange(p) for _ in range(n)]
    s = verifier(name, n, tau)
    for m, table in ((3, [rnd.randrange(p) for _ in range(8)]), (2, [p - 1, 0, 1, 5]), (0, [9]), (2, [7, 7, 7, 7]), (1, [0, 0])):
        z = [rnd.randrange(p) for _ in range(m)]
        c = G * M.commit(table, tau, p)
        qs, v = M.open_(table, z, tau, p)
        proof = [G * q for q in qs]
        assert s.verify(c, proof, z, v)
        assert s.verify(c, proof, [x + p for x in z], v + p)          # scalars are reduced on entry
        assert not s.verify(c, proof, z, (v + 1) % p)
        if m:
            assert all(q.is_zero() for q in proof) == (len(set(table)) == 1)
            assert not s.verify(c, proof[:-1], z, v) and not s.verify(c, proof + [G], z, v)
            assert not s.verify(c, [proof[0] + G] + proof[1:], z, v)
            # a constant polynomial takes the same value, with the same proof, at every point
            assert s.verify(c, proof, [(z[0] + 1) % p] + z[1:], v) == (len(set(table)) == 1)
            assert not s.verify(c, tuple(proof), z[:-1], v)
        assert not s.verify(c, proof + [G], z + [1], v)
        assert not s.verify(c, None, z, v) and not s.verify(None, proof, z, v)
        assert m == 0 or not s.verify(c, [None] * m, z, v)
    assert not s.verify(G, [G] * 4, [1, 2, 3, 4], 0)                  # more coordinates than the scheme has variables
    # the batch verifier is the same check on the combination
    tables = [[rnd.randrange(p) for _ in range(4)] for _ in range(3)]
    z = [rnd.randrange(p), 1]
    cs = [G * M.commit(t, tau, p) for t in tables]
    vs = [M.evaluate(t, z, p) for t in tables]
    rho = s._challenge(None, cs, z, vs)
    qs, v = M.open_(M.combine(tables, rho, p), z, tau, p)
    assert v == M.combine_scalars(vs, rho, p)
    proof = [G * q for q in qs]
    assert s.batch_verify(cs, proof, z, vs)
    assert not s.batch_verify(cs[::-1], proof, z, vs) and not s.batch_verify(cs, proof, z, [vs[0] + 1] + vs[1:])
    assert not s.batch_verify(cs[:2], proof, z, vs) and not s.batch_verify([], proof, z, [])
