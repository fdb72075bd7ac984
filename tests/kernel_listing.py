"""The per-kernel figures of the product build's assembly listing (photonbend_amd.build: build_listing compiles it, parse_listing reads it;
DESIGN 3.4).  The six tests/test_isa_*.py modules share ONE compile per test process (stats()); experiments/r6/isa_stats.py prints the same
rows for any build."""

import os
import tempfile

from photonbend_amd import build

parse = build.parse_listing  # (in the package, next to build_listing: experiments/r6/isa_stats.py reads listings with it too, and must not need tests/)

_stats = None  # {name: row} of the product build, or the exception its compile ended with: made once per process


def stats():
    """{name: row} of the product build's listing.  The compile (minutes, a 50 MB file) happens at most once per process, in a temporary
    directory that does not outlive it; a failure is remembered and raised again, so the other modules fail at once with the same message."""
    global _stats
    import pytest

    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("needs hipcc")
    if _stats is None:
        try:
            with tempfile.TemporaryDirectory(prefix="pb_listing_") as tmp:
                with open(build.build_listing(os.path.join(tmp, "pb.s"))) as f:
                    _stats = {r["name"]: r for r in parse(f.read())}
        except Exception as e:
            _stats = e
    if isinstance(_stats, Exception):
        raise _stats
    return _stats
