"""The mixed-owner batches are reachable under the reference's import paths
(heartbeat.PySwizzle, as heartbeat/PySwizzle/__init__.py exports the class)."""
import importlib


def test_prove_and_verify_mixed_reexported():
    amd = importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")
    hb_mod = importlib.import_module("heartbeat.PySwizzle.PySwizzle")
    hb_pkg = importlib.import_module("heartbeat.PySwizzle")
    import heartbeat
    import heartbeat_amd
    assert hb_mod.PySwizzle.prove_mixed is amd.PySwizzle.prove_mixed
    assert hb_mod.PySwizzle.verify_mixed is amd.PySwizzle.verify_mixed
    assert hb_pkg.PySwizzle.prove_mixed is amd.PySwizzle.prove_mixed
    assert hb_pkg.PySwizzle.verify_mixed is amd.PySwizzle.verify_mixed
    assert heartbeat.PySwizzle.PySwizzle.prove_mixed is heartbeat_amd.PySwizzle.PySwizzle.prove_mixed
    assert heartbeat.PySwizzle.PySwizzle.verify_mixed is heartbeat_amd.PySwizzle.PySwizzle.verify_mixed
    # static: callable without an instance
    assert amd.PySwizzle.prove_mixed([]) == [] and amd.PySwizzle.verify_mixed([]) == []


def test_native_binding_lists_the_mixed_calls():
    from heartbeat_amd import _native
    names = [s[0] for s in _native.SIGNATURES]
    assert "hb_prove_mixed" in names and "hb_verify_rhs_mixed" in names
