"""The listed-block update's names are reachable through the reference's
package paths (heartbeat.PySwizzle), as the other additions are."""
import importlib


def test_update_names_through_heartbeat_pyswizzle():
    import heartbeat.PySwizzle as pkg
    mod = importlib.import_module("heartbeat.PySwizzle.PySwizzle")
    amd = importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")
    for cls in (pkg.PySwizzle, mod.PySwizzle):
        assert cls is amd.PySwizzle
        for name in ("encode_blocks", "patch_tag", "update", "update_file", "update_many"):
            assert callable(getattr(cls, name)), name
    assert isinstance(amd.PySwizzle.__dict__["patch_tag"], staticmethod)
    assert mod.encode_blocks_many is amd.encode_blocks_many
    assert isinstance(amd.UPDATE_MANY_MIN, int) and amd.UPDATE_MANY_MIN >= 1


def test_native_signatures_name_the_new_entry_points():
    from heartbeat_amd import _native
    names = [s[0] for s in _native.SIGNATURES]
    assert "hb_encode_blocks_many" in names and "hb_encode_blocks" in names
    assert [f[0] for f in _native.BlocksDesc._fields_] == ["f_key", "alpha_key", "indices", "nblocks", "data", "len",
                                                           "tags"]
