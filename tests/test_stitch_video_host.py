"""CPU-only checks of the double-fisheye video stitch (pb_stitch_planar / pb_stitch_nv12): the header's declarations and the
library's exports, the argument checks - the nearest calls' own, cell by cell of tests/test_video_calls_host.py's grid -, the refusals of
plans the kernel does not serve, the Python keywords and the ``stitch-yuv`` command's usage errors.  Every plan is deferred: it has no
device, so nothing here could start a launch."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
from click.testing import CliRunner

from photonbend_amd import _native as nat
from photonbend_amd.scripts import cli
from tests import test_video_calls_host as grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE, INVALID, UNSUPPORTED = grid.FAKE, grid.INVALID, grid.UNSUPPORTED
TWINS = {"pb_stitch_planar": "pb_remap_planar", "pb_stitch_nv12": "pb_remap_nv12"}


def test_the_header_declares_the_five_functions_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "photonbend_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(pb_(?:plan_)?stitch\w*)\s*\(([^)]*)\)\s*;", text)}
    near = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(pb_remap_(?:planar|nv12)(?:_supported)?)\s*\(([^)]*)\)\s*;", text)}
    assert decl == {
        "pb_stitch_planar": near["pb_remap_planar"], "pb_stitch_nv12": near["pb_remap_nv12"],  # the arguments of the nearest calls
        "pb_stitch_planar_supported": near["pb_remap_planar_supported"], "pb_stitch_nv12_supported": near["pb_remap_nv12_supported"],
        "pb_plan_stitch_tile_mix": "const pb_plan* plan, long long mix[9]",
    }
    assert re.search(r"#define PB_ABI_VERSION 5\b", text)  # additive
    for name, twin in list(TWINS.items()) + [(n + "_supported", t + "_supported") for n, t in TWINS.items()]:
        assert nat.SIGNATURES[name] == nat.SIGNATURES[twin], name
    assert nat.SIGNATURES["pb_plan_stitch_tile_mix"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)])
    lib = nat.load()
    assert all(hasattr(lib, n) for n in decl) and lib.pb_abi_version() == 5


def _cells(name):
    family = "planar" if name.endswith("planar") else "nv12"
    for S in (1, 2):
        for sub in (grid.SUBS.values() if family == "planar" else (None,)):
            for p, kw in grid.call_cases(family, False, False, S, sub):
                yield S, sub, p, kw


@pytest.mark.parametrize("name", sorted(TWINS))
def test_every_argument_check_of_the_nearest_call_comes_back_with_the_same_status_and_message(name, monkeypatch):
    lib = nat.load()
    monkeypatch.setitem(grid.CALLS, name, grid.CALLS[TWINS[name]])  # (the grid's runner looks the family up by name)
    n_invalid = n_none = n_refused = 0
    with grid.plans() as made:
        for S, sub, p, kw in _cells(name):
            want = grid.run_c_cell(lib, made, TWINS[name], S, sub, p, kw)
            got = grid.run_c_cell(lib, made, name, S, sub, p, kw)
            if want[1] == INVALID:
                assert got == want, (S, sub, p, kw)
                n_invalid += 1
            elif want[1] == 0:  # no frames: PB_OK, nothing to launch
                assert got == want and want[0] == 0, (S, sub, p, kw)
                n_none += 1
            else:  # the arguments pass (or a layout member reaches 2^31): the plan - deferred - is refused, nothing else
                assert want[1] == UNSUPPORTED and got[1] == UNSUPPORTED, (S, sub, p, kw, got)
                if "planes span less than 2^31 bytes (" in want[2]:
                    assert got == want  # (the shared resolver's refusal, before anything is multiplied)
                else:
                    assert got[2].startswith(name + " takes "), got
                n_refused += 1
    assert n_invalid > 100 and n_none > 10 and n_refused > 20, (n_invalid, n_none, n_refused)


def test_a_deferred_double_plan_and_a_panorama_source_are_refused_with_their_own_messages():
    lib = nat.load()
    with grid.plans() as made:
        for name, twin in TWINS.items():
            sub = (nat.PLANAR_420,) if name.endswith("planar") else ()
            for S in (1, 2):
                args = lambda h: [h, FAKE, FAKE, 1, None, None, *sub, S, None, None]  # noqa: E731
                assert getattr(lib, name)(*args(made["double"])) == UNSUPPORTED
                msg = lib.pb_last_error().decode()
                assert msg.startswith(name + " takes prepared double-fisheye plans in a tile mode (not deferred, not PB_MODE_FAITHFUL") and "pb_gather_blend_u8" in msg
                assert getattr(lib, name + "_supported")(made["double"], *sub, S) == 0
                for single in ("base", "cube", "eac", "tall"):
                    assert getattr(lib, name)(*args(made[single])) == UNSUPPORTED, single
                    assert lib.pb_last_error().decode() == f"{name} takes double-fisheye sources: use {twin} for a single source"
                    assert getattr(lib, name + "_supported")(made[single], *sub, S) == 0
                # the nearest calls keep refusing the double plan, as before
                assert getattr(lib, twin)(*args(made["double"])) == UNSUPPORTED and "double-fisheye" in lib.pb_last_error().decode()
            assert getattr(lib, name + "_supported")(None, *sub, 1) == INVALID and lib.pb_last_error() == b"null argument"
            assert getattr(lib, name + "_supported")(made["double"], *sub, 3) == INVALID and b"bytes_per_sample" in lib.pb_last_error()
            assert getattr(lib, name + "_supported")(made["odd_5x8_4x8"], *sub, 1) == INVALID and b"even" in lib.pb_last_error()
        mix = (C.c_longlong * 9)(*([7] * 9))
        assert lib.pb_plan_stitch_tile_mix(made["double"], mix) == 0 and list(mix) == [0] * 9  # no tables: all zero
        assert lib.pb_plan_stitch_tile_mix(None, mix) == INVALID and lib.pb_plan_stitch_tile_mix(made["double"], None) == INVALID


def test_the_python_keywords_and_the_checks_before_any_device():
    P = nat.Plan
    assert list(inspect.signature(P.stitch_planar).parameters) == ["self", "src", "subsampling", "out", "fill", "src_layout", "dst_layout", "stream"]
    assert list(inspect.signature(P.stitch_nv12).parameters) == ["self", "src", "out", "fill", "src_layout", "dst_layout", "stream"]
    assert list(inspect.signature(P.launch_stitch_planar).parameters) == list(inspect.signature(P.launch_planar).parameters)[:-1]
    assert list(inspect.signature(P.launch_stitch_nv12).parameters) == list(inspect.signature(P.launch_nv12).parameters)[:-1]
    assert list(inspect.signature(P.stitch_planar_supported).parameters) == ["self", "subsampling", "bytes_per_sample"]
    assert list(inspect.signature(P.stitch_nv12_supported).parameters) == ["self", "bytes_per_sample"]
    assert all(p.default is None for n, p in inspect.signature(P.stitch_planar).parameters.items() if n not in ("self", "src", "subsampling"))
    double = nat.Plan(nat.make_proj(nat.KIND_PANO, *grid.DST_HW), [], nat.make_proj(*grid.DOUBLE), defer=True)
    assert double.stitch_planar_supported("420", 1) is False and double.stitch_nv12_supported(2) is False and double.stitch_planar_supported(nat.PLANAR_444) is False
    assert set(double.stitch_tile_mix()) == {"solo", "unit", "row", "lat", "failed", "fix_tiles", "fix_pixels", "fix_anchors_422", "fix_anchors_420"}
    assert all(v == 0 for v in double.stitch_tile_mix().values())
    with pytest.raises(nat.PbError, match="bytes_per_sample"):
        double.stitch_nv12_supported(3)
    with pytest.raises(ValueError):
        double.stitch_planar_supported("411")
    with pytest.raises(nat.PbError, match="device arrays"):
        double.stitch_planar(np.zeros(48, np.uint8), "420")
    with pytest.raises(nat.PbError, match="device arrays"):
        double.stitch_nv12(np.zeros((6, 8), np.uint8))
    with grid.stand_ins():
        (h, w), (Hd, Wd) = grid.SRC_HW, grid.DST_HW
        with pytest.raises(nat.PbError, match="packed source frames"):
            double.stitch_planar(grid.FakeDevice((7,), np.uint8), "420")
        with pytest.raises(nat.PbError, match="uint8"):
            double.stitch_nv12(grid.FakeDevice((3 * h // 2, w), np.float32))
        with pytest.raises(nat.PbError, match="out must be"):
            double.stitch_nv12(grid.FakeDevice((3 * h // 2, w), np.uint8), out=grid.FakeDevice((1,), np.uint8))
        # every argument passes: the library refuses the deferred plan - no fallback
        with pytest.raises(nat.PbError, match="pb_stitch_planar takes prepared double-fisheye plans"):
            double.stitch_planar(grid.FakeDevice((h * w * 3 // 2,), np.uint16), "420", fill=(1, 2, 3))
        with pytest.raises(nat.PbError, match="pb_stitch_nv12 takes prepared double-fisheye plans"):
            double.launch_stitch_nv12(FAKE, FAKE)
        double.launch_stitch_planar(FAKE, FAKE, "444", 0)  # no frames: nothing to launch


# ---- the command's usage errors: raised before any input is read ---------------------------------------------------------------------------
def run(*args, **kw):
    return CliRunner().invoke(cli.main, ["stitch-yuv", *map(str, args)], **kw)


def test_the_command_s_usage_errors_exit_before_any_input_is_read_and_write_nothing(tmp_path):
    inp, out = tmp_path / "in.yuv", tmp_path / "out.yuv"
    inp.write_bytes(bytes(40 * 80 * 3 // 2))
    ok = ("--width", 80, "--height", 40, "--lens", "equidistant", "--fov", 195)
    for args, word in ((("--height", 40, "--lens", "equidistant", "--fov", 195), "--width"), (("--width", 80, "--lens", "equidistant", "--fov", 195), "--height"),
                       (("--width", 80, "--height", 40, "--fov", 195), "--lens"), (("--width", 80, "--height", 40, "--lens", "equidistant"), "--fov"),
                       ((*ok, "--pix-fmt", "yuva420p"), "yuva420p"), ((*ok, "--lens-max-theta", 90), "polynomial"), ((*ok, "--type", "double"), "--type"),
                       ((*ok, "--rotations", inp), "--rotations"), ((*ok, "--interpolation", "bilinear"), "--interpolation")):
        res = run(inp, out, *args)
        assert res.exit_code == 2 and word in res.output and not out.exists(), (args, res.output)
    for args, message in ((("--width", 81, "--height", 40, "--lens", "equidistant", "--fov", 195), "4:2:0 frames have even dimensions, got --width 81 --height 40"),
                          (("--width", 80, "--height", 41, "--lens", "equidistant", "--fov", 195, "--pix-fmt", "yuv420p"), "yuv420p frames have even widths and heights"),
                          (("--width", 81, "--height", 41, "--lens", "equidistant", "--fov", 195, "--pix-fmt", "yuv422p10le"), "yuv422p10le frames have even widths"),
                          ((*ok, "--out-height", 33), "4:2:0 frames have even dimensions: the output would be 33 x 66"),
                          ((*ok, "--pix-fmt", "yuv422p", "--out-height", 33, "--out-width", 65), "yuv422p frames have even widths: the output would be 33 x 65"),
                          ((*ok, "--out-width", 0), "the output would be 40 x 0"), ((*ok, "--chunk", 6), "--chunk is a multiple of 4, got 6"),
                          (("--width", 80, "--height", 40, "--lens", "equidistant", "--fov", 170), "can't be smaller than 180"),
                          (("--width", 80, "--height", 40, "--lens", "equidistant", "--fov", 361), "can't be higher than 360")):
        # stdin would be read if the command got that far: it is given none, and an absent input file is not noticed either
        res = run(tmp_path / "absent.yuv", out, *args)
        assert res.exit_code == 1 and message in res.stderr and not out.exists(), (args, res.output)
    res = run(tmp_path / "absent.yuv", out, *ok)
    assert res.exit_code == 1 and "absent.yuv" in res.stderr and not out.exists(), res.output
    inp.write_bytes(bytes(40 * 80 * 3 // 2 + 10))
    res = run(inp, out, *ok)
    assert res.exit_code == 1 and "1 frames of 4800 bytes and a truncated one of 10" in res.stderr and not out.exists(), res.output
    assert set(nat.VIDEO_FORMATS) == set(next(p for p in cli.stitch_yuv.params if p.name == "pix_fmt").type.choices)
    # the nearest commands keep refusing a double fisheye
    res = CliRunner().invoke(cli.main, ["remap-nv12", str(inp), str(out), "--width", "80", "--height", "40", "--type", "double", "--lens", "equidistant", "--fov", "190"])
    assert res.exit_code == 2 and "double" in res.output
