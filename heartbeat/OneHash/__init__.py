"""heartbeat.OneHash (reference heartbeat/OneHash/__init__.py).  As there,
``heartbeat.OneHash.OneHash`` is the class once the package is imported; the
module stays reachable as sys.modules entry (pickles use it).  As in the
reference, ``import heartbeat`` does not import this package."""
from .OneHash import Challenge, OneHash  # NOQA
