"""The OneHash heartbeat (heartbeat/OneHash): Challenge and OneHash with the
reference package's names; GPU responses, seed chains and batches (OneHash.py)."""
from .OneHash import Challenge, OneHash  # NOQA
