"""CPU: the host side of csrc/pcs.hip under sanitizers, the new symbols' bindings, and the package's argument rules that need no
GPU."""

import os
import re
import shutil
import subprocess

import pytest

from zksnake_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pcs_host_side_refuses_bad_arguments_under_sanitizers(tmp_path):
    """tests/native/pcs_args_check.cpp, built by the recipe in its header the way test_host_lib.py builds ipa_args_check: a
    host-only compile, an EMPTY offload bundle for the __hip_fatbin_<hash> symbol the object refers to, link, run.  The sanitizer
    runtimes are linked into the program; nothing is loaded into Python.  The program sees no device on any machine, so the calls
    that pass the checks fail in the launch with ZK_ERR_HIP, which is what it expects."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    magic = ",".join(f"'{c}'" for c in "__CLANG_OFFLOAD_BUNDLE__")
    supp = tmp_path / "lsan.supp"      # the HSA runtime's own 144 bytes at exit on a machine with a GPU driver
    supp.write_text("leak:libhsa-runtime64\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", LSAN_OPTIONS=f"suppressions={supp}:print_suppressions=0")
    name = "pcs_args_check"
    obj, stub, exe = str(tmp_path / f"{name}.o"), str(tmp_path / f"{name}_stub"), str(tmp_path / name)
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-mbmi2", "-madx",
                           "-DZK_NOINLINE_MUL", *san, "-c", os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", obj], timeout=600)
    undefined = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout
    syms = sorted(set(re.findall(r"__hip_fatbin_[0-9a-f]+", undefined)))
    assert syms, "the host-only object names no device image"
    with open(stub + ".cpp", "w") as f:   # the magic string and a bundle count of zero: registered at load time, never looked into
        f.write("#include <stdint.h>\nstruct bundle { char magic[24]; uint64_t count; };\n")
        for sym in syms:
            f.write(f'extern "C" __attribute__((aligned(4096))) const bundle {sym} = {{{{{magic}}}, 0}};\n')
    subprocess.check_call(["g++", "-O0", "-c", stub + ".cpp", "-o", stub + ".o"], timeout=600)
    subprocess.check_call([hipcc, "--offload-host-only", *san, "-o", exe, obj, stub + ".o"], timeout=600)
    res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and f"{name}: all ok" in res.stdout, res.stdout + res.stderr


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
