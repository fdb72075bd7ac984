#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY - writes tests/golden/eac.npz from tests/eac_ref.py, the written NumPy definition of the equi-angular cube map
(DESIGN 3.14).  There is no reference class to run: the definition is the cube map's (tests/cubemap_ref.py, pinned to the reference by
tests/make_cubemap_goldens.py) with two functions of a face coordinate in between, and tests/test_eac_host.py shows that with those two
replaced by the identity it IS the cube's, bit for bit.  Run it on the goldens' platform (tests/helpers.live_numpy_is_the_goldens_numpy):
the file holds NumPy's result bits there.  Per small case: the float64 map after get_coordinate_map and after every rotation (bits; a cube
destination's unrotated map once per mapping and face size), the integer source-index map(s) (and a double source's blend weights) and the
output bytes on the synthetic frame.

Usage:  python tests/make_eac_goldens.py
"""

from __future__ import annotations

import os
import sys
import warnings

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from tests import eac_cases as ec  # noqa: E402
from tests import helpers as H  # noqa: E402



def arrays():
    """{key: array} of every small case, from the definition."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return _arrays()


def _arrays():
    out = {}
    for case in ec.small_cases():
        n = case.name
        frame = ec.case_frame(case)
        stages = ec.ref_stages(case)
        for k, st in enumerate(stages):
            key = ec.map_key(case, k)
            if key in out:
                assert np.array_equal(out[key], H.bits(st)), key
            out[key] = H.bits(st)
        idx = ec.ref_index(case, stages[-1])
        if case.src[0] == "double":
            out[f"{n}/idx_l"], out[f"{n}/idx_r"] = idx[0], idx[1]
            out[f"{n}/w_l"], out[f"{n}/w_r"] = H.bits(idx[2]), H.bits(idx[3])
        else:
            out[f"{n}/idx"] = idx
        out[f"{n}/u8"] = ec.ref_remap(case, frame, stages[-1])
    return out


def main():
    assert H.live_numpy_is_the_goldens_numpy(), "this host's NumPy does not return the goldens' bits: run where tests/golden/npmath.npz was made"
    out = arrays()
    path = os.path.join(H.GOLD, "eac.npz")
    np.savez_compressed(path, **out)
    print(f"eac.npz written, {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
