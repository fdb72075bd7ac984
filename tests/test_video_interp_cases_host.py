"""The condition on the cases of tests/video_interp_cases.py, from the oracle alone (no GPU): the band in which a GPU test may excuse a
sample that is fill in one result and sampled in the other - interp_cases.edge_band(case, final, 1/512) - holds under 0.5 % of each case's
output pixels, and nothing for a panorama source.  Every size is even, so 4:2:0 applies to all of them."""

import pytest

from tests import interp_cases as ic
from tests import video_interp_cases as vc


def test_the_case_list_is_the_issue_s():
    names = [c.name for c in vc.CASES]
    assert names[:4] == ["sweep3", "sweep5", "sweep10", "sweep12"] and names[4:8] == [c.name for c in ic.MAGNIFIED] and len(names) == 13
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("case", vc.CASES, ids=lambda c: c.name)
def test_sizes_are_even_and_the_edge_band_is_small(case):
    for p in (case.dst, case.src):
        assert not (p[1] | p[2]) & 1, (case.name, p)
    assert case.src[0] in ("camera", "pano"), case.src
    final = ic.final_map(case)
    band = ic.edge_band(case, final, vc.BAND)
    share = float(band.mean())
    print(f"{case.name}: {int(band.sum())} of {band.size} output pixels in the edge band ({100 * share:.3f} %)")
    assert share < vc.BAND_SHARE, (case.name, share)
    if case.src[0] == "pano":
        assert not band.any(), case.name
