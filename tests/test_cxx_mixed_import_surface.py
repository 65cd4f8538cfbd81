"""The cxx mixed-owner batches are reachable under the reference's import paths
(heartbeat.Heartbeat, heartbeat.Swizzle.Swizzle: one class object) and listed
in the native binding."""
import importlib

import pytest


def test_prove_and_verify_mixed_reexported(monkeypatch):
    from heartbeat_amd import multi
    monkeypatch.setattr(multi, "_devices", [0])          # no device enumeration: this test opens no GPU
    amd = importlib.import_module("heartbeat_amd.Swizzle")
    hb_mod = importlib.import_module("heartbeat.Swizzle")
    import heartbeat
    assert heartbeat.Heartbeat is amd.Swizzle and hb_mod.Swizzle is amd.Swizzle
    assert heartbeat.Heartbeat.prove_mixed is amd.Swizzle.prove_mixed
    assert heartbeat.Heartbeat.verify_mixed is amd.Swizzle.verify_mixed
    assert heartbeat.Swizzle.Swizzle.prove_mixed is amd.Swizzle.prove_mixed
    assert heartbeat.Swizzle.Swizzle.verify_mixed is amd.Swizzle.verify_mixed
    # static: callable without an instance
    assert amd.Swizzle.prove_mixed([]) == [] and amd.Swizzle.verify_mixed([]) == []
    # the module functions beside prove_files and verify_rhs_many
    assert amd.prove_files_mixed([]) == [] and amd.verify_rhs_mixed([]) == []


def test_native_binding_lists_the_cxx_mixed_calls():
    from heartbeat_amd import _native
    sig = {s[0]: s for s in _native.SIGNATURES}
    assert "hb_cxx_prove_mixed" in sig and "hb_cxx_verify_rhs_mixed" in sig
    # the descriptors of the PySwizzle mixed calls, unchanged
    assert sig["hb_cxx_prove_mixed"][1:] == sig["hb_prove_mixed"][1:]
    assert sig["hb_cxx_verify_rhs_mixed"][1:] == sig["hb_verify_rhs_mixed"][1:]


def test_many_helpers_take_the_native_name_and_the_mu_policy():
    import inspect
    from heartbeat_amd import _many
    from heartbeat_amd.exc import HeartbeatError
    assert inspect.signature(_many.prove_files_mixed).parameters["native"].default == "hb_prove_mixed"
    sig = inspect.signature(_many.verify_rhs_mixed).parameters
    assert sig["native"].default == "hb_verify_rhs_mixed" and sig["exact_mu"].default is False
    # exact_mu is checked before any native call
    item = (257, 2, b"f" * 32, b"a" * 32, 3, b"c" * 32, 1, 257, [1, 2, 3])
    with pytest.raises(HeartbeatError) as e:
        _many.verify_rhs_mixed([item], native="hb_cxx_verify_rhs_mixed", exact_mu=True)
    assert str(e.value) == "proof has 3 mu values, not 2"
