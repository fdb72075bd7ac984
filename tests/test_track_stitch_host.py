"""CPU-only checks of the tracked double-fisheye video stitch (pb_track_stitch_planar / pb_track_stitch_nv12): the header's
declarations and the library's exports, the argument checks - the nearest tracked calls' own, cell by cell of
tests/test_video_calls_host.py's grid, the table checks among them -, the refusals, the Python keywords and the ``stitch-track-yuv``
command's usage errors.  Every plan is deferred and every call that passes its argument checks goes to a plan of a SINGLE source, which
these calls refuse (or spans 2^31 bytes): nothing here could start a launch."""

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
TWINS = {"pb_track_stitch_planar": "pb_remap_track_planar", "pb_track_stitch_nv12": "pb_remap_track_nv12"}


def refusal(name):
    return f"{name} takes double-fisheye sources: use {TWINS[name]} for a single source"


def test_the_header_declares_the_two_functions_with_their_twins_arguments_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "photonbend_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(pb_track_stitch\w*)\s*\(([^)]*)\)\s*;", text)}
    near = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(pb_remap_track_(?:planar|nv12))\s*\(([^)]*)\)\s*;", text)}
    assert decl == {name: near[twin] for name, twin in TWINS.items()}
    assert re.search(r"#define PB_ABI_VERSION 5\b", text)  # additive
    for name, twin in TWINS.items():
        assert nat.SIGNATURES[name] == nat.SIGNATURES[twin], name
    lib = nat.load()
    assert all(hasattr(lib, n) for n in TWINS) and lib.pb_abi_version() == 5 == nat.ABI_VERSION


def _cells(name):
    family = "planar" if name.endswith("planar") else "nv12"
    for S in (1, 2):
        for sub in (grid.SUBS.values() if family == "planar" else (None,)):
            for p, kw in grid.call_cases(family, True, False, S, sub):
                yield S, sub, p, kw


@pytest.mark.parametrize("name", sorted(TWINS))
def test_every_argument_and_table_check_of_the_nearest_tracked_call_comes_back_with_the_same_status_and_message(name, monkeypatch):
    """The twin gets the grid's plan; the new call gets the panorama plan of the same shapes wherever the grid names the double fisheye -
    the one plan the new call would serve -, so every cell that passes the checks ends in its single-source refusal."""
    lib = nat.load()
    monkeypatch.setitem(grid.CALLS, name, grid.CALLS[TWINS[name]])  # (the grid's runner looks the family up by name)
    assert grid.PLANS["double"][1:] == grid.PLANS["base"][1:] and grid.PLANS["double"][0][1:3] == grid.PLANS["base"][0][1:3]
    n_invalid = n_table = n_none = n_refused = 0
    with grid.plans() as made:
        assert all(grid.is_deferred(h) for h in made.values())
        for S, sub, p, kw in _cells(name):
            want = grid.run_c_cell(lib, made, TWINS[name], S, sub, p, kw)
            got = grid.run_c_cell(lib, made, name, S, sub, "base" if p == "double" else p, kw)
            if want[1] == INVALID:
                assert got == want, (S, sub, p, kw)
                n_invalid += 1
                n_table += any(w in want[2] for w in ("rotation table", "n_rot_per_frame", "PB_MAX_ROTATIONS"))
            elif want[1] == 0:  # no frames: PB_OK, nothing to launch
                assert got == want and want[0] == 0, (S, sub, p, kw)
                n_none += 1
            else:  # the arguments pass (or a layout member reaches 2^31): the plan - a single source - is refused, nothing else
                assert want[1] == UNSUPPORTED and got[1] == UNSUPPORTED, (S, sub, p, kw, got)
                if "planes span less than 2^31 bytes (" in want[2]:
                    assert got == want  # (the shared resolver's refusal, before anything is multiplied)
                else:
                    assert got[2] == refusal(name), got
                n_refused += 1
    assert n_invalid > 100 and n_table > 10 and n_none > 10 and n_refused > 20, (n_invalid, n_table, n_none, n_refused)


def test_single_sources_and_frames_of_two_to_the_31_bytes_are_refused_and_no_frames_is_ok():
    lib = nat.load()
    with grid.plans() as made:
        for name, twin in TWINS.items():
            family = "planar" if name.endswith("planar") else "nv12"
            sub = (nat.PLANAR_420,) if family == "planar" else ()
            zeros = (0,) * (4 if family == "planar" else 2)
            cls = nat.pb_planar_layout if family == "planar" else nat.pb_nv12_layout
            for S in (1, 2):
                args = lambda h, n=1, k=1, dl=None: [h, FAKE, k, FAKE, FAKE, n, None, None if dl is None else C.addressof(dl), *sub, S, None, None]  # noqa: E731
                for single in ("base", "cube", "eac", "tall", "rot1"):
                    assert getattr(lib, name)(*args(made[single])) == UNSUPPORTED, single
                    assert lib.pb_last_error().decode() == refusal(name)
                    assert getattr(lib, name)(*args(made[single], k=0)) == INVALID  # (the argument checks come first)
                # the double fisheye: what the call serves - no frames: PB_OK, no launch, no device; a span of 2^31 bytes: refused
                for k in (1, 2, 8):
                    assert getattr(lib, name)(*args(made["double"], n=0, k=k)) == 0
                assert getattr(lib, name)(*args(made["double"], n=0, k=9)) == INVALID and b"PB_MAX_ROTATIONS" in lib.pb_last_error()
                huge = cls(1 << 30, *zeros)
                assert getattr(lib, name)(*args(made["double"], dl=huge)) == UNSUPPORTED
                msg = lib.pb_last_error().decode()
                assert msg.startswith(name + " takes frames whose planes span less than 2^31 bytes and sources below 32768 px a side"), msg
                assert getattr(lib, name)(*args(made["double"], dl=huge, k=0)) == INVALID and b"n_rot_per_frame" in lib.pb_last_error()
                # the nearest tracked calls keep refusing the double plan, word for word
                assert getattr(lib, twin)(*args(made["double"])) == UNSUPPORTED
                assert lib.pb_last_error().decode() == f"{twin} takes single sources (a double fisheye's blend is sample-typed): convert to RGB8 and use pb_remap_track_u8"


def test_the_python_keywords_and_the_checks_before_any_device():
    P = nat.Plan
    assert list(inspect.signature(P.stitch_track_planar).parameters) == ["self", "src", "rotations", "subsampling", "out", "fill", "src_layout", "dst_layout", "stream"]
    assert list(inspect.signature(P.stitch_track_nv12).parameters) == ["self", "src", "rotations", "out", "fill", "src_layout", "dst_layout", "stream"]
    # the tracked calls' keywords without `interpolation`
    assert list(inspect.signature(P.stitch_track_planar).parameters) == list(inspect.signature(P.remap_track_planar).parameters)[:-1]
    assert list(inspect.signature(P.stitch_track_nv12).parameters) == list(inspect.signature(P.remap_track_nv12).parameters)[:-1]
    assert list(inspect.signature(P.launch_stitch_track_planar).parameters) == list(inspect.signature(P.launch_track_planar).parameters)[:-1]
    assert list(inspect.signature(P.launch_stitch_track_nv12).parameters) == list(inspect.signature(P.launch_track_nv12).parameters)[:-1]
    for m, t in ((P.stitch_track_planar, P.remap_track_planar), (P.stitch_track_nv12, P.remap_track_nv12), (P.launch_stitch_track_planar, P.launch_track_planar),
                 (P.launch_stitch_track_nv12, P.launch_track_nv12)):
        twin = inspect.signature(t).parameters
        assert all(p.default == twin[n].default and p.kind == twin[n].kind for n, p in inspect.signature(m).parameters.items()), m.__name__
    (h, w), (Hd, Wd) = grid.SRC_HW, grid.DST_HW
    pano = nat.Plan(nat.make_proj(nat.KIND_PANO, *grid.DST_HW), [], nat.make_proj(nat.KIND_PANO, *grid.SRC_HW), defer=True)
    double = nat.Plan(nat.make_proj(nat.KIND_PANO, *grid.DST_HW), [], nat.make_proj(*grid.DOUBLE), defer=True)
    mats = np.tile(np.eye(3), (2, 1, 1))
    with pytest.raises(nat.PbError, match="device arrays"):
        double.stitch_track_planar(np.zeros(48, np.uint8), mats[:1], "420")
    with pytest.raises(nat.PbError, match="device arrays"):
        double.stitch_track_nv12(np.zeros((6, 8), np.uint8), mats[:1])
    with grid.stand_ins():
        with pytest.raises(nat.PbError, match="packed source frames"):
            double.stitch_track_planar(grid.FakeDevice((7,), np.uint8), mats[:1], "420")
        with pytest.raises(nat.PbError, match="uint8"):
            double.stitch_track_nv12(grid.FakeDevice((3 * h // 2, w), np.float32), mats[:1])
        with pytest.raises(ValueError, match="1 frames need 1 rotations, the table holds 2"):
            double.stitch_track_nv12(grid.FakeDevice((3 * h // 2, w), np.uint8), mats)
        with pytest.raises(ValueError, match="2 frames need 2 rotations, the table holds 1"):
            double.stitch_track_planar(grid.FakeDevice((2, h * w * 3 // 2), np.uint8), mats[:1], "420")
        with pytest.raises(ValueError, match="PB_MAX_ROTATIONS"):
            double.stitch_track_nv12(grid.FakeDevice((3 * h // 2, w), np.uint8), np.zeros((1, 9, 3, 3)))
        with pytest.raises(ValueError):
            double.stitch_track_planar(grid.FakeDevice((h * w * 3 // 2,), np.uint8), mats[:1], "411")
        # every argument passes: the library refuses the single source - no fallback
        with pytest.raises(nat.PbError, match="pb_track_stitch_planar takes double-fisheye sources: use pb_remap_track_planar"):
            pano.launch_stitch_track_planar(FAKE, 1, FAKE, FAKE, "420", bytes_per_sample=2, fill=(1, 2, 3))
        with pytest.raises(nat.PbError, match="pb_track_stitch_nv12 takes double-fisheye sources: use pb_remap_track_nv12"):
            pano.launch_stitch_track_nv12(FAKE, 1, FAKE, FAKE)
        double.launch_stitch_track_planar(FAKE, 2, FAKE, FAKE, "444", 0)  # no frames: nothing to launch
        double.launch_stitch_track_nv12(FAKE, 1, FAKE, FAKE, 0, bytes_per_sample=2)
        # the tracked calls of a single source keep refusing the double plan
        with pytest.raises(nat.PbError, match="pb_remap_track_nv12 takes single sources"):
            double.launch_track_nv12(FAKE, 1, FAKE, FAKE)


# ---- the command's usage errors: raised before any input is read ---------------------------------------------------------------------------
def run(*args, **kw):
    return CliRunner().invoke(cli.main, ["stitch-track-yuv", *map(str, args)], **kw)


def test_the_command_s_usage_errors_exit_before_any_input_is_read_and_write_nothing(tmp_path):
    inp, out, track = tmp_path / "in.yuv", tmp_path / "out.yuv", tmp_path / "track.txt"
    inp.write_bytes(bytes(40 * 80 * 3 // 2 * 3))  # three frames
    track.write_text("0 0 0\n# a comment\n10 20 30\n")  # two lines
    ok = ("--width", 80, "--height", 40, "--lens", "equidistant", "--fov", 195, "--rotations", track)
    assert "stitch-track-yuv" in cli.main.commands and "stitch-yuv" in cli.main.commands
    # click's own: a missing required option - --rotations among them -, an unknown format, an option of another command
    for args, word in ((ok[:-2], "--rotations"), (ok[2:], "--width"), (("--width", 80, *ok[4:]), "--height"), ((*ok[:4], *ok[6:]), "--lens"), ((*ok[:6], *ok[8:]), "--fov"),
                       ((*ok[:-2], "--rotations", tmp_path / "absent.txt"), "absent.txt"), ((*ok, "--pix-fmt", "yuva420p"), "yuva420p"),
                       ((*ok, "--interpolation", "bilinear"), "--interpolation"), ((*ok, "--type", "double"), "--type")):
        res = run(inp, out, *args)
        assert res.exit_code == 2 and word in res.output and not out.exists(), (args, res.output)
    rest = ("--lens", "equidistant", "--fov", 195, "--rotations", track)
    for args, message in ((("--width", 81, "--height", 40, *rest), "4:2:0 frames have even dimensions, got --width 81 --height 40"),
                          (("--width", 80, "--height", 41, *rest, "--pix-fmt", "yuv420p"), "yuv420p frames have even widths and heights"),
                          (("--width", 81, "--height", 41, *rest, "--pix-fmt", "yuv422p10le"), "yuv422p10le frames have even widths"),
                          ((*ok, "--out-height", 33), "4:2:0 frames have even dimensions: the output would be 33 x 66"),
                          ((*ok, "--pix-fmt", "yuv422p", "--out-height", 33, "--out-width", 65), "yuv422p frames have even widths: the output would be 33 x 65"),
                          ((*ok, "--out-width", 0), "the output would be 40 x 0"), ((*ok, "--chunk", 6), "--chunk is a multiple of 4, got 6"),
                          (("--width", 80, "--height", 40, "--lens", "equidistant", "--fov", 170, "--rotations", track), "can't be smaller than 180"),
                          (("--width", 80, "--height", 40, "--lens", "equidistant", "--fov", 361, "--rotations", track), "can't be higher than 360")):
        # stdin would be read if the command got that far: it is given none, and an absent input file is not noticed either
        res = run(tmp_path / "absent.yuv", out, *args)
        assert res.exit_code == 1 and message in res.stderr and not out.exists(), (args, res.output)
    bad = tmp_path / "bad.txt"
    bad.write_text("0 0\n")
    res = run(tmp_path / "absent.yuv", out, *ok[:-1], bad)
    assert res.exit_code == 1 and "three numbers" in res.stderr and not out.exists(), res.output
    res = run(tmp_path / "absent.yuv", out, *ok)
    assert res.exit_code == 1 and "absent.yuv" in res.stderr and not out.exists(), res.output
    # a track shorter than the file, and a truncated frame: refused before anything is written
    res = run(inp, out, *ok)
    assert res.exit_code == 1 and "holds 3 frames, the rotation track 2 lines" in res.stderr and not out.exists(), res.output
    inp.write_bytes(bytes(40 * 80 * 3 // 2 + 10))
    res = run(inp, out, *ok)
    assert res.exit_code == 1 and "1 frames of 4800 bytes and a truncated one of 10" in res.stderr and not out.exists(), res.output
    assert set(nat.VIDEO_FORMATS) == set(next(p for p in cli.stitch_track_yuv.params if p.name == "pix_fmt").type.choices)
    assert next(p for p in cli.stitch_track_yuv.params if p.name == "track").required
    # the two commands share every other option; stitch-yuv keeps rejecting --rotations
    names = lambda c: [p.name for p in c.params]  # noqa: E731
    assert [n for n in names(cli.stitch_track_yuv) if n != "track"] == names(cli.stitch_yuv)
    res = CliRunner().invoke(cli.main, ["stitch-yuv", str(inp), str(out), *map(str, ok)])
    assert res.exit_code == 2 and "--rotations" in res.output and not out.exists()
