"""heartbeat.OneHash.OneHash (reference heartbeat/OneHash/OneHash.py): the
scheme's classes from heartbeat_amd.OneHash.OneHash, whose responses and seed
chains run on the GPU."""
from heartbeat_amd.OneHash.OneHash import Challenge, OneHash  # NOQA

__all__ = ["Challenge", "OneHash"]
