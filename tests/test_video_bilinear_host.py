"""CPU-only checks of the bilinear video calls (pb_remap_planar_bilinear / pb_remap_nv12_bilinear): the header and the
library's exports, the argument checks - which are the nearest calls', message for message -, the plans the calls refuse before anything
could be launched (a deferred plan and a double-fisheye source have no device state), the ``interpolation`` keyword of the ``Plan``
methods and the ``--interpolation`` option of the two raw-video commands."""

import ctypes as C
import os
import re

import numpy as np
import pytest
from click.testing import CliRunner

from photonbend_amd import _native as nat
from photonbend_amd.scripts import cli
from tests import planar_ref
from tests.test_planar_host import FAKE, INVALID, SUBS, UNSUPPORTED, FakeDevice, packed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_four_functions_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "photonbend_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(pb_remap_(?:planar|nv12)_bilinear\w*)\s*\(([^)]*)\)\s*;", text)}
    assert decl == {
        "pb_remap_planar_bilinear": "const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_planar_layout* src_layout, "
                                    "const pb_planar_layout* dst_layout, int subsampling, int bytes_per_sample, const uint16_t fill[3], void* stream",
        "pb_remap_nv12_bilinear": "const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_nv12_layout* src_layout, "
                                  "const pb_nv12_layout* dst_layout, int bytes_per_sample, const uint16_t fill_yuv[3], void* stream",
        "pb_remap_planar_bilinear_supported": "const pb_plan* plan, int subsampling, int bytes_per_sample",
        "pb_remap_nv12_bilinear_supported": "const pb_plan* plan, int bytes_per_sample",
    }
    # the signatures of their nearest twins
    for name in decl:
        assert nat.SIGNATURES[name] == nat.SIGNATURES[name.replace("_bilinear", "")], name
    lib = nat.load()
    assert all(hasattr(lib, n) for n in decl)
    assert lib.pb_abi_version() == 5  # additive


def _plan(src, dst, flags=nat.PLAN_DEFER):
    lib = nat.load()
    handle = C.c_void_p()
    assert lib.pb_plan_create_ex(C.byref(dst), None, 0, C.byref(src), flags, 0, C.byref(handle)) == 0
    return lib, handle


def _pano_plan(h, w, H, W):
    return _plan(nat.make_proj(nat.KIND_PANO, h, w), nat.make_proj(nat.KIND_PANO, H, W))


def _planar(fn, lib, plan, sub, S=1, src=FAKE, dst=FAKE, n=1, sl=None, dl=None, fill=None):
    sl = None if sl is None else nat.pb_planar_layout(*sl)
    dl = None if dl is None else nat.pb_planar_layout(*dl)
    rc = getattr(lib, fn)(plan, src, dst, n, None if sl is None else C.addressof(sl), None if dl is None else C.addressof(dl), sub, S,
                          None if fill is None else C.addressof((C.c_uint16 * 3)(*fill)), None)
    return rc, lib.pb_last_error()


def _nv12(fn, lib, plan, S=1, src=FAKE, dst=FAKE, n=1, sl=None, dl=None, fill=None):
    sl = None if sl is None else nat.pb_nv12_layout(*sl)
    dl = None if dl is None else nat.pb_nv12_layout(*dl)
    rc = getattr(lib, fn)(plan, src, dst, n, None if sl is None else C.addressof(sl), None if dl is None else C.addressof(dl), S,
                          None if fill is None else C.addressof((C.c_uint16 * 3)(*fill)), None)
    return rc, lib.pb_last_error()


def _planar_bad_calls(sub):
    """Keyword sets of calls on a (4 x 8) -> (6 x 12) plan that fail an argument check of pb_remap_planar: one per check and side."""
    calls = [dict(plan=None), dict(src=None), dict(dst=None), dict(n=-1)]
    calls += [dict(S=S) for S in (-1, 0, 3, 4, 8)] + [dict(sub=bad) for bad in (-1, 3, 420)]
    for S in (1, 2):
        for which, dims in (("sl", (4, 8)), ("dl", (6, 12))):
            base = packed(*dims, S, sub)
            ce = base[3] - base[2]
            for broken in ((base[0] - S, 0, 0, 0, 0), (0, base[1] - S, 0, 0, 0), (0, 0, base[2] - S, 0, 0), (0, 0, 0, base[2] - S, 0), (0, 0, 0, base[3] - S, 0),
                           (0, 0, base[3] + ce - S, base[3], 0), (0, 0, 0, 0, base[4] - S), (0, 0, 0, base[3] + S, base[4]), (0, 0, base[4], 0, base[4] + ce - S)):
                calls.append({"S": S, which: broken})
            if S == 2:
                calls += [{"S": S, which: b} for b in ((base[0] + 1, 0, 0, 0, 0), (0, base[1] + 1, 0, 0, 0), (0, 0, 0, base[3] + 1, 0), (0, 0, 0, 0, base[4] + 1))]
    calls += [dict(S=2, src=FAKE + 1), dict(S=2, dst=FAKE + 1)]
    return calls


@pytest.mark.parametrize("sub", planar_ref.SUBSAMPLINGS)
def test_every_invalid_argument_of_pb_remap_planar_comes_back_with_the_same_message(sub):
    lib, plan = _pano_plan(4, 8, 6, 12)
    try:
        calls = _planar_bad_calls(sub)
        for kw in calls:
            kw = dict(kw)
            p = kw.pop("plan", plan)
            sid = kw.pop("sub", SUBS[sub])
            near = _planar("pb_remap_planar", lib, p, sid, **kw)
            bil = _planar("pb_remap_planar_bilinear", lib, p, sid, **kw)
            assert near[0] == INVALID and bil == near, (kw, near, bil)
        assert len(calls) > 50
        for S in (3, 0):
            assert lib.pb_remap_planar_bilinear_supported(plan, SUBS[sub], S) == INVALID and b"bytes_per_sample" in lib.pb_last_error()
        assert lib.pb_remap_planar_bilinear_supported(plan, 7, 1) == INVALID and b"subsampling" in lib.pb_last_error()
        assert lib.pb_remap_planar_bilinear_supported(None, SUBS[sub], 1) == INVALID and lib.pb_last_error() == b"null argument"
        # a layout member of 2^31 or more: the nearest call's refusal (the message names the nearest call: it is its check)
        huge = (1 << 31, 0, 0, 0, 0)
        assert _planar("pb_remap_planar_bilinear", lib, plan, SUBS[sub], sl=huge) == _planar("pb_remap_planar", lib, plan, SUBS[sub], sl=huge)
        assert _planar("pb_remap_planar_bilinear", lib, plan, SUBS[sub], sl=huge)[0] == UNSUPPORTED
        # no frames: nothing to launch, whatever the plan
        assert _planar("pb_remap_planar_bilinear", lib, plan, SUBS[sub], n=0)[0] == 0
    finally:
        lib.pb_plan_destroy(plan)
    # the dimension rule
    lib, odd = _pano_plan(3, 7, 4, 8)
    try:
        near, bil = _planar("pb_remap_planar", lib, odd, SUBS[sub]), _planar("pb_remap_planar_bilinear", lib, odd, SUBS[sub])
        assert (bil == near and near[0] == INVALID) if sub != "444" else (bil[0] == near[0] == UNSUPPORTED), (sub, near, bil)
        if sub != "444":
            assert lib.pb_remap_planar_bilinear_supported(odd, SUBS[sub], 1) == INVALID and b"even" in lib.pb_last_error()
    finally:
        lib.pb_plan_destroy(odd)


def test_every_invalid_argument_of_pb_remap_nv12_comes_back_with_the_same_message():
    lib, plan = _pano_plan(4, 8, 6, 12)
    try:
        calls = [dict(plan=None), dict(src=None), dict(dst=None), dict(n=-1)] + [dict(S=S) for S in (-1, 0, 3, 4)]
        for S in (1, 2):
            for which, (h, w) in (("sl", (4, 8)), ("dl", (6, 12))):
                p = S * w
                calls += [{"S": S, which: v} for v in ((p - 2 * S, 0, 0), (0, p * h - 2 * S, 0), (0, 0, p * h * 3 // 2 - 2 * S), (p + S, 0, 0), (0, p * h + S, 0),
                                                        (0, 0, p * h * 3 // 2 + S))]
            calls += [dict(S=S, src=FAKE + S), dict(S=S, dst=FAKE + S)]
        for kw in calls:
            kw = dict(kw)
            p = kw.pop("plan", plan)
            near, bil = _nv12("pb_remap_nv12", lib, p, **kw), _nv12("pb_remap_nv12_bilinear", lib, p, **kw)
            assert near[0] == INVALID and bil == near, (kw, near, bil)
        assert lib.pb_remap_nv12_bilinear_supported(plan, 3) == INVALID and b"bytes_per_sample" in lib.pb_last_error()
        assert lib.pb_remap_nv12_bilinear_supported(None, 1) == INVALID and lib.pb_last_error() == b"null argument"
        assert _nv12("pb_remap_nv12_bilinear", lib, plan, n=0)[0] == 0
    finally:
        lib.pb_plan_destroy(plan)
    lib, odd = _pano_plan(4, 8, 5, 10)
    try:
        near, bil = _nv12("pb_remap_nv12", lib, odd), _nv12("pb_remap_nv12_bilinear", lib, odd)
        assert near[0] == INVALID and b"even" in near[1] and bil == near
        assert lib.pb_remap_nv12_bilinear_supported(odd, 1) == INVALID and b"even" in lib.pb_last_error()
    finally:
        lib.pb_plan_destroy(odd)


def test_a_deferred_plan_and_a_double_fisheye_source_are_unsupported_and_nothing_is_launched():
    """Neither plan has device state (a deferred plan never looks at a device): a refusal here cannot have launched anything, and the frame
    "pointers" are not addresses."""
    double = nat.make_proj(nat.KIND_DOUBLE, 8, 16, lens=0, fov=np.deg2rad(190.0), f_distance=4.0)
    for src in (nat.make_proj(nat.KIND_PANO, 8, 16), double):
        lib, plan = _plan(src, nat.make_proj(nat.KIND_PANO, 6, 12))
        try:
            for S in (1, 2):
                for sid in SUBS.values():
                    rc, msg = _planar("pb_remap_planar_bilinear", lib, plan, sid, S)
                    assert rc == UNSUPPORTED and msg.startswith(b"pb_remap_planar_bilinear takes prepared plans"), msg
                    assert lib.pb_remap_planar_bilinear_supported(plan, sid, S) == 0
                rc, msg = _nv12("pb_remap_nv12_bilinear", lib, plan, S)
                assert rc == UNSUPPORTED and msg.startswith(b"pb_remap_nv12_bilinear takes prepared plans"), msg
                assert lib.pb_remap_nv12_bilinear_supported(plan, S) == 0
                # the nearest calls refuse the same plans
                assert _planar("pb_remap_planar", lib, plan, nat.PLANAR_420, S)[0] == UNSUPPORTED and _nv12("pb_remap_nv12", lib, plan, S)[0] == UNSUPPORTED
        finally:
            lib.pb_plan_destroy(plan)


# ---- Python ------------------------------------------------------------------------------------------------------------------------------
def test_the_interpolation_keyword_of_the_plan_methods(monkeypatch):
    monkeypatch.setattr(nat, "is_device_array", lambda a: isinstance(a, FakeDevice))
    monkeypatch.setattr(nat, "is_tensor", lambda a: False)
    p = nat.make_proj(nat.KIND_PANO, 4, 8)
    plan = nat.Plan(p, [], p, defer=True)
    for bad in ("cubic", "", "BILINEAR", "catmull-rom"):
        with pytest.raises(ValueError, match="one of"):
            plan.remap_planar(FakeDevice((48,), np.uint8), "420", interpolation=bad)
        with pytest.raises(ValueError, match="one of"):
            plan.remap_nv12(FakeDevice((6, 8), np.uint8), interpolation=bad)
        with pytest.raises(ValueError, match="one of"):
            plan.planar_supported("420", interpolation=bad)
        with pytest.raises(ValueError, match="one of"):
            plan.nv12_supported(interpolation=bad)
    with pytest.raises(ValueError) as exc:  # the RGB methods' error for an unknown mode
        plan.remap_planar(FakeDevice((48,), np.uint8), "420", interpolation="cubic")
    with pytest.raises(ValueError) as rgb:
        plan.remap(FakeDevice((4, 8, 3), np.uint8), interpolation="cubic")
    assert str(exc.value) == str(rgb.value)
    with pytest.raises(TypeError):  # keyword-only
        plan.planar_supported("420", 1, "bilinear")
    for sub in SUBS:
        assert not plan.planar_supported(sub, interpolation="bilinear") and not plan.planar_supported(sub, 2, interpolation="nearest")
    assert not plan.nv12_supported(interpolation="bilinear") and not plan.nv12_supported(2, interpolation="bilinear")
    with pytest.raises(nat.PbError, match="pb_remap_planar_bilinear takes prepared plans"):
        plan.launch_planar(FAKE, FAKE, "422", 1, 0, interpolation="bilinear")
    with pytest.raises(nat.PbError, match="pb_remap_nv12_bilinear takes prepared plans"):
        plan.launch_nv12(FAKE, FAKE, 1, 0, interpolation="bilinear")
    with pytest.raises(nat.PbError, match="pb_index_map_i32"):  # the default is the nearest call, as before
        plan.launch_planar(FAKE, FAKE, "422", 1, 0)


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("command", ["remap-yuv", "remap-nv12"])
def test_bilinear_with_a_rotation_track_is_a_usage_error_before_any_input_is_read(tmp_path, command):
    track = tmp_path / "track.txt"
    track.write_text("0 0 0\n")
    out = tmp_path / "out.yuv"
    # (the input does not exist and the sizes are odd: neither is looked at)
    res = CliRunner().invoke(cli.main, [command, str(tmp_path / "absent.yuv"), str(out), "--width", "31", "--height", "15", "--interpolation", "bilinear",
                                        "--rotations", str(track)])
    assert res.exit_code != 0 and "--rotations" in res.output and "bilinear" in res.output and "absent.yuv" not in res.output and not out.exists(), res.output
    res = CliRunner().invoke(cli.main, [command, str(tmp_path / "absent.yuv"), str(out), "--width", "32", "--height", "16", "--interpolation", "cubic"])
    assert res.exit_code != 0 and "cubic" in res.output and not out.exists(), res.output
    # the default is nearest: with a track, the usual errors
    res = CliRunner().invoke(cli.main, [command, str(tmp_path / "absent.yuv"), str(out), "--width", "32", "--height", "16", "--rotations", str(track)])
    assert res.exit_code != 0 and "absent.yuv" in res.output, res.output
