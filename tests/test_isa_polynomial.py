"""The float64 kernels that gained the polynomial lens (its Horner chains and the rolled Newton loop sit in the lens switch of
csrc/pb_stages.hpp, which every kernel of the float64 chain inlines), read from the compiler's listing of the product build like
test_isa_budget.py: no scratch, and no fewer waves per SIMD than before the lens was added.  The hot kernels never evaluate a lens;
their budgets are pinned by test_isa_budget.py, test_isa_supersample.py and test_isa_catmull_rom.py."""

import pytest

from tests import kernel_listing

# waves per SIMD ("Occupancy" in the listing) of every kernel that inlines pb_lens_forward / pb_lens_inverse, read from the listing of
# commit 34dda95 ("Share one sampler path between bilinear and Catmull-Rom"), the last one without the polynomial lens - same flags
# (photonbend_amd/build.py), same compiler.  A fact of that commit, not of the code under test.
PARENT_OCCUPANCY = {
    "pb_coordmap_kernel": 8,
    "pb_threshold_kernel": 8,
    "pb_sep_tables_kernel": 8,
    "pb_sep_check_kernel": 8,
    "pb_double_tables_kernel": 8,
    "pb_double_pair_kernel": 7,
    "pb_double_lat_kernel": 8,
    "pb_bilinear_double_fix_kernel": 3,
    "pb_bilinear_coord_kernel<3>": 8,
    "pb_bilinear_coord_kernel<4>": 8,
    "pb_bilinear_fix_coord_kernel<3>": 8,
    "pb_bilinear_fix_coord_kernel<4>": 8,
    "pb_bilinear_coord_kernel<2>": 8,
    "pb_bilinear_fix_coord_kernel<2>": 8,
    "pb_bilinear_coord_kernel<0>": 8,
    "pb_bilinear_fix_coord_kernel<0>": 8,
    "pb_model_kernel<3>": 8,
    "pb_certify_kernel<3, 0>": 4,
    "pb_certify_kernel<3, 1>": 4,
    "pb_certify_kernel<3, -1>": 4,
    "pb_model_kernel<4>": 8,
    "pb_certify_kernel<4, 0>": 4,
    "pb_certify_kernel<4, 1>": 4,
    "pb_certify_kernel<4, -1>": 4,
    "pb_model_kernel<2>": 8,
    "pb_certify_kernel<2, 0>": 5,
    "pb_certify_kernel<2, 1>": 4,
    "pb_certify_kernel<2, -1>": 4,
    "pb_model_kernel<0>": 8,
    "pb_certify_kernel<0, 0>": 4,
    "pb_certify_kernel<0, 1>": 4,
    "pb_certify_kernel<0, -1>": 4,
    "pb_fix_tables_kernel<2>": 8,
    "pb_fix_tables_kernel<0>": 8,
    "pb_remap_kernel<1, 0>": 7,
    "pb_remap_kernel<1, 1>": 7,
    "pb_remap_kernel<1, -1>": 7,
    "pb_remap_kernel<2, 0>": 8,
    "pb_remap_kernel<2, 1>": 7,
    "pb_remap_kernel<2, -1>": 8,
    "pb_remap_kernel<0, 0>": 8,
    "pb_remap_kernel<0, 1>": 7,
    "pb_remap_kernel<0, -1>": 7,
    "pb_interp_double_kernel<PbCatmullRom>": 2,
    "pb_interp_double_kernel<PbBilinear>": 3,
    "pb_interp_fix_kernel<PbCatmullRom, 2>": 5,
    "pb_interp_fix_kernel<PbBilinear, 2>": 8,
    "pb_interp_fix_kernel<PbCatmullRom, 0>": 4,
    "pb_interp_fix_kernel<PbBilinear, 0>": 8,
    "pb_index_kernel<1, 0>": 8,
    "pb_index_kernel<1, 1>": 8,
    "pb_index_kernel<1, -1>": 8,
    "pb_index_kernel<2, 0>": 8,
    "pb_index_kernel<2, 1>": 8,
    "pb_index_kernel<2, -1>": 8,
    "pb_index_kernel<0, 0>": 8,
    "pb_index_kernel<0, 1>": 8,
    "pb_index_kernel<0, -1>": 8,
    "pb_sample_map_interp_kernel<PbCatmullRom, 1, unsigned char>": 4,
    "pb_sample_map_interp_kernel<PbBilinear, 1, unsigned char>": 8,
    "pb_sample_map_interp_kernel<PbCatmullRom, 0, unsigned char>": 7,
    "pb_sample_map_interp_kernel<PbBilinear, 0, unsigned char>": 8,
    "pb_sample_map_interp_kernel<PbCatmullRom, 1, unsigned short>": 4,
    "pb_sample_map_interp_kernel<PbBilinear, 1, unsigned short>": 8,
    "pb_sample_map_interp_kernel<PbCatmullRom, 0, unsigned short>": 7,
    "pb_sample_map_interp_kernel<PbBilinear, 0, unsigned short>": 8,
    "pb_sample_map_kernel<1>": 8,
    "pb_sample_map_kernel<0>": 8,
    "pb_index_from_map_kernel<1>": 8,
    "pb_index_from_map_kernel<0>": 8,
}
# ... and the instruction counts of two small kernels that hold exactly one inverse lens (same listing)
PARENT_INSTRUCTIONS = {"pb_coordmap_kernel": 1449, "pb_threshold_kernel": 1511}


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def test_float64_kernels_keep_their_occupancy_and_have_no_scratch(stats):
    missing = sorted(set(PARENT_OCCUPANCY) - set(stats))
    assert not missing, missing
    bad = {k: (stats[k]["occupancy"], want, stats[k]["scratch"]) for k, want in PARENT_OCCUPANCY.items()
           if stats[k]["occupancy"] < want or stats[k]["scratch"] != 0}
    for k in sorted(PARENT_OCCUPANCY):
        r = stats[k]
        print(f"{k:64s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} scratch {r['scratch']} waves {r['occupancy']} (before: {PARENT_OCCUPANCY[k]})")
    assert not bad, f"(waves per SIMD, before, scratch bytes): {bad}"


def test_the_issue_s_kernels_are_among_them():
    for prefix, n in (("pb_remap_kernel", 9), ("pb_certify_kernel", 12), ("pb_coordmap", 1), ("pb_index_kernel", 9), ("pb_threshold_kernel", 1),
                      ("pb_interp_", 6)):
        assert sum(k.startswith(prefix) for k in PARENT_OCCUPANCY) == n, prefix


def test_the_newton_loop_is_rolled(stats):
    """One Newton step is two Horner chains (19 float64 multiplies and adds), a float64 division (about a dozen instructions) and a
    subtraction: unrolled ten times it would add 300-400 instructions to a kernel that inverts one lens; rolled, with the forward and
    inverse cases of the switch around it, well under 200."""
    for name, before in PARENT_INSTRUCTIONS.items():
        grown = stats[name]["instr"] - before
        print(f"{name}: {before} -> {stats[name]['instr']} instructions")
        assert 0 < grown < 200, (name, before, stats[name]["instr"])
