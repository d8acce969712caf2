"""CPU: the host side of csrc/pcs.hip under sanitizers, the new symbols' bindings, and the package's argument rules that need no
GPU."""

import os

import pytest

from helpers import run_host_program
from zksnake_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pcs_host_side_refuses_bad_arguments_under_sanitizers(tmp_path):
    """tests/native/pcs_args_check.cpp, built by the recipe in its header (helpers.run_host_program, as test_host_lib.py builds
    ipa_args_check): a host-only compile, an EMPTY offload bundle for the __hip_fatbin_<hash> symbol the object refers to, link, run.
    The sanitizer runtimes are linked into the program; nothing is loaded into Python.  The program sees no device on any machine, so the calls
    that pass the checks fail in the launch with ZK_ERR_HIP, which is what it expects."""
    res = run_host_program("pcs_args_check", tmp_path)
    assert res.returncode == 0 and "pcs_args_check: all ok" in res.stdout, res.stdout + res.stderr


def test_symbols_are_bound(lib):
    for name in ("zk_pcs_round_dev", "zk_pcs_verify_scalars_dev"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    with open(os.path.join(ROOT, "include", "zkmi.h")) as f:
        assert f"#define ZK_PCS_MAX_LOG {N.PCS_MAX_LOG}\n" in f.read()


def test_sizes_are_refused_before_any_allocation():
    from zksnake_amd.commitment.polynomial import IPA, KZG
    from zksnake_amd.commitment.polynomial import kzg
    with pytest.raises(ValueError):
        IPA((1 << 21) + 1, "BN254")
    assert IPA(1 << 21, "BLS12_381").log_n == 21 and IPA(1, "BN254").n == 1 and IPA(5, "BN254").n == 8
    with pytest.raises(ValueError):
        KZG(kzg.MAX_BASES, "BN254")
    assert KZG(kzg.MAX_BASES - 1, "BN254").degree == kzg.MAX_BASES - 1
    with pytest.raises(KeyError):
        KZG(4, "no such curve")


def test_random_vector_has_one_home():
    """RangeProof.random_vector and IPA.random draw through the same FrOps.random_vector"""
    import inspect
    from zksnake_amd.commitment.polynomial import IPA
    from zksnake_amd.frvec import FrOps
    from zksnake_amd.subprotocol import RangeProof
    assert "random_vector" in inspect.getsource(RangeProof.random_vector) and "urandom" not in inspect.getsource(RangeProof)
    assert "urandom" not in inspect.getsource(IPA) and "urandom" in inspect.getsource(FrOps.random_vector)
    ipa = IPA(8, "BN254")
    rnd = ipa.random(multi=True)
    assert set(rnd) == {"poly_r", "t_bar", "f_blind"} and rnd["poly_r"].shape == (8, 4)
    assert max(N.limbs_to_ints(rnd["poly_r"])) < ipa.order
