"""The mixed-owner encode under the reference's own package names, without a
GPU: in a fresh interpreter outside the repo, the names reached through
``heartbeat.*`` are the GPU build's objects."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_encode_mixed_names_in_a_fresh_interpreter(tmp_path):
    check = """
import heartbeat
from heartbeat import Heartbeat, PySwizzle, Swizzle
import heartbeat_amd
import heartbeat_amd.Swizzle
import importlib
from heartbeat_amd import _many, _native
# the modules (the packages' attribute of that name is the class)
amd_pys = importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")
hb_pys = importlib.import_module("heartbeat.PySwizzle.PySwizzle")

# the classes' static methods, callable without an instance
assert heartbeat.PySwizzle.PySwizzle.encode_mixed is amd_pys.PySwizzle.encode_mixed
assert PySwizzle.PySwizzle.encode_mixed([]) == []
assert heartbeat.Heartbeat.encode_mixed is heartbeat_amd.Swizzle.Swizzle.encode_mixed
assert Heartbeat.encode_mixed is Swizzle.Swizzle.encode_mixed
assert Heartbeat.encode_mixed([]) == []
# the module-level twins with explicit keys
assert hb_pys.encode_files_mixed is amd_pys.encode_files_mixed
assert callable(heartbeat_amd.Swizzle.encode_files_mixed)
assert heartbeat_amd.Swizzle.encode_files_mixed is not amd_pys.encode_files_mixed
assert amd_pys.ENCODE_MIXED_MIN >= 1 and heartbeat_amd.Swizzle.CXX_ENCODE_MIXED_MIN >= 1
# the shared layer and the ABI's names
assert callable(_many.encode_files_mixed)
names = [s[0] for s in _native.SIGNATURES]
assert "hb_encode_mixed" in names and "hb_cxx_encode_mixed" in names
assert _native.EncodeMixedDesc._fields_[:4] == _native.ProveMixedDesc._fields_[:4]
print("ok")
"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", check], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "ok"
