"""heartbeat.PySwizzle.PySwizzle (reference heartbeat/PySwizzle/PySwizzle.py):
the scheme's classes from heartbeat_amd.PySwizzle.PySwizzle, whose encode /
prove / verify run on the GPU."""
from ..util import KeyedPRF  # NOQA  (as the reference module: heartbeat.util)
from heartbeat_amd.PySwizzle.PySwizzle import (  # NOQA
    Challenge, Proof, PySwizzle, State, Tag, encode_blocks_many, encode_file, encode_files, encode_files_mixed,
    getPrime, getPrimes, prove_files, verify_rhs_many)

__all__ = ["KeyedPRF", "Challenge", "Tag", "State", "Proof", "PySwizzle", "getPrime", "getPrimes"]
