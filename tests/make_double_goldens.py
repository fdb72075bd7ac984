#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY - writes tests/golden/double_tiles.npz: for every case of tests/double_cases.EDGES the CPU oracle's two taps
(il, ir: int32) and two blend factors (fl, fr: float64, stored as their bits) of the double-fisheye source
(oracle.reference_path.remap_index).  Run it on the goldens' platform (tests/helpers.live_numpy_is_the_goldens_numpy): the file holds
NumPy's result bits there, so the edge comparisons of tests/test_hip_double_tiles.py are exact on any host.  The archive's members carry
a fixed date: a second run writes the same bytes.

Usage:  python tests/make_double_goldens.py [output path]
"""

from __future__ import annotations

import io
import os
import sys
import zipfile

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from tests import double_cases as dc  # noqa: E402
from tests import helpers as H  # noqa: E402


def arrays():
    """{key: array} of every edge case, from the oracle."""
    out = {}
    for case in dc.EDGES:
        il, ir, fl, fr = dc.oracle_taps(case)
        assert il.dtype == ir.dtype == np.int32 and fl.dtype == fr.dtype == np.float64 and il.shape == fl.shape == (case.dst[1], case.dst[2])
        out[f"{case.name}/il"], out[f"{case.name}/ir"] = il, ir
        out[f"{case.name}/fl"], out[f"{case.name}/fr"] = H.bits(fl), H.bits(fr)
    return out


def write(path, out):
    """np.savez_compressed's format with every member dated 1980-01-01 (NumPy stamps the time of the run)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(out[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    assert H.live_numpy_is_the_goldens_numpy(), "this host's NumPy does not return the goldens' bits: run where tests/golden/npmath.npz was made"
    out = arrays()
    path = sys.argv[1] if len(sys.argv) > 1 else dc.FIXTURE
    write(path, out)
    print(f"{os.path.basename(path)} written, {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
