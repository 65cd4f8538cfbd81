"""The cxx Swizzle's listed-block update is reachable through the reference's
names (heartbeat.Heartbeat, heartbeat.Swizzle), as the other additions are."""


def test_update_names_on_heartbeat():
    import heartbeat
    import heartbeat.Swizzle as pkg
    import heartbeat_amd.Swizzle as amd
    for cls in (heartbeat.Heartbeat, pkg.Swizzle):
        assert cls is amd.Swizzle
        for name in ("encode_blocks", "patch_tag", "update", "update_file", "update_many"):
            assert callable(getattr(cls, name)), name
    assert isinstance(amd.Swizzle.__dict__["patch_tag"], staticmethod)
    assert callable(amd.encode_blocks_many)
    assert isinstance(amd.CXX_UPDATE_MANY_MIN, int) and amd.CXX_UPDATE_MANY_MIN >= 1


def test_native_signatures_name_the_new_entry_points():
    from heartbeat_amd import _native
    sigs = {s[0]: s for s in _native.SIGNATURES}
    assert "hb_cxx_encode_blocks_many" in sigs and "hb_cxx_encode_blocks" in sigs
    # the descriptors and arguments of the PySwizzle twins
    assert sigs["hb_cxx_encode_blocks_many"][1:] == sigs["hb_encode_blocks_many"][1:]
    assert sigs["hb_cxx_encode_blocks"][1:] == sigs["hb_encode_blocks"][1:]
