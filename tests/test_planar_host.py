"""CPU-only checks of the planar remap (pb_remap_planar / pb_remap_track_planar): the header and the library's exports, the
argument checks that come before any device is looked at - layout defaults, the dimension rule per subsampling, overlapping planes -, the
Python checks of ``Plan.remap_planar``, the ``pixel_format`` table and the host pipeline over the stand-ins of tests/test_host_memory.py,
and the ``utils`` helpers.  A deferred plan has no device and every library call here fails its checks: none could start a launch."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import photonbend_amd as pb
from photonbend_amd import _native as nat
from photonbend_amd import batch
from tests import planar_ref
from tests.test_host_memory import FakePlan, pipe_env  # noqa: F401  (the stand-ins of the streaming pipeline's tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000  # a non-null "device pointer" for calls that must be refused before anything reads it
INVALID, UNSUPPORTED = -1, -3
SUBS = {"444": nat.PLANAR_444, "422": nat.PLANAR_422, "420": nat.PLANAR_420}


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_three_functions_the_struct_and_the_constants_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "photonbend_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (pb_remap(?:_track)?_planar\w*)\s*\(([^)]*)\)\s*;", text)}
    assert decl == {
        "pb_remap_planar": "const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_planar_layout* src_layout, "
                           "const pb_planar_layout* dst_layout, int subsampling, int bytes_per_sample, const uint16_t fill[3], void* stream",
        "pb_remap_planar_supported": "const pb_plan* plan, int subsampling, int bytes_per_sample",
        "pb_remap_track_planar": "const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames, "
                                 "const pb_planar_layout* src_layout, const pb_planar_layout* dst_layout, int subsampling, int bytes_per_sample, "
                                 "const uint16_t fill[3], void* stream",
    }
    assert re.search(r"typedef struct pb_planar_layout \{ size_t pitch, chroma_pitch, offset1, offset2, frame_stride; \} pb_planar_layout;", text)
    consts = dict(re.findall(r"#define (PB_PLANAR_4\d\d) (\d+)", text))
    assert consts == {"PB_PLANAR_444": str(nat.PLANAR_444), "PB_PLANAR_422": str(nat.PLANAR_422), "PB_PLANAR_420": str(nat.PLANAR_420)}
    assert len({nat.PLANAR_444, nat.PLANAR_422, nat.PLANAR_420}) == 3
    vp = C.c_void_p
    assert nat.SIGNATURES["pb_remap_planar"] == (C.c_int, [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp])
    assert nat.SIGNATURES["pb_remap_planar_supported"] == (C.c_int, [vp, C.c_int, C.c_int])
    assert nat.SIGNATURES["pb_remap_track_planar"] == (C.c_int, [vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp])
    assert [f[0] for f in nat.pb_planar_layout._fields_] == ["pitch", "chroma_pitch", "offset1", "offset2", "frame_stride"]
    assert C.sizeof(nat.pb_planar_layout) == 5 * C.sizeof(C.c_size_t)
    lib = nat.load()
    assert all(hasattr(lib, n) for n in decl)
    assert lib.pb_abi_version() == 5  # additive


def _deferred(h, w, H=None, W=None):
    lib = nat.load()
    handle = C.c_void_p()
    src, dst = nat.make_proj(nat.KIND_PANO, h, w), nat.make_proj(nat.KIND_PANO, H or h, W or w)
    assert lib.pb_plan_create_ex(C.byref(dst), None, 0, C.byref(src), nat.PLAN_DEFER, 0, C.byref(handle)) == 0
    return lib, handle


def _call(lib, plan, sub, S=1, src=FAKE, dst=FAKE, n=1, sl=None, dl=None, fill=None):
    sl = None if sl is None else nat.pb_planar_layout(*sl)
    dl = None if dl is None else nat.pb_planar_layout(*dl)
    rc = lib.pb_remap_planar(plan, src, dst, n, None if sl is None else C.addressof(sl), None if dl is None else C.addressof(dl), sub, S,
                             None if fill is None else C.addressof((C.c_uint16 * 3)(*fill)), None)
    return rc, lib.pb_last_error()


def _track_call(lib, plan, sub, S=1, table=FAKE, k=1, src=FAKE, dst=FAKE, n=1, sl=None):
    sl = None if sl is None else nat.pb_planar_layout(*sl)
    rc = lib.pb_remap_track_planar(plan, table, k, src, dst, n, None if sl is None else C.addressof(sl), None, sub, S, None, None)
    return rc, lib.pb_last_error()


def packed(h, w, S, sub):
    """The packed defaults of the header, spelled out: (pitch, chroma_pitch, offset1, offset2, frame_stride)."""
    cx, cy = planar_ref.SHIFTS[sub]
    p, cp = S * w, S * (w >> cx)
    o1 = p * h
    o2 = o1 + cp * (h >> cy)
    return p, cp, o1, o2, o2 + cp * (h >> cy)


@pytest.mark.parametrize("sub", planar_ref.SUBSAMPLINGS)
def test_argument_checks_come_before_any_device_and_say_what_is_wrong(sub):
    lib, plan = _deferred(4, 8, 6, 12)  # source 4 x 8, destination 6 x 12
    sid = SUBS[sub]
    try:
        assert _call(lib, None, sid) == (INVALID, b"null argument")
        assert _call(lib, plan, sid, src=None) == (INVALID, b"null argument") and _call(lib, plan, sid, dst=None) == (INVALID, b"null argument")
        assert _call(lib, plan, sid, n=-1) == (INVALID, b"negative frame count")
        for S in (-1, 0, 3, 4, 8):
            rc, msg = _call(lib, plan, sid, S)
            assert rc == INVALID and b"bytes_per_sample" in msg, (S, msg)
            assert lib.pb_remap_planar_supported(plan, sid, S) == INVALID and b"bytes_per_sample" in lib.pb_last_error()
        for bad in (-1, 3, 420):
            rc, msg = _call(lib, plan, bad)
            assert rc == INVALID and b"subsampling" in msg, (bad, msg)
            assert lib.pb_remap_planar_supported(plan, bad, 1) == INVALID and b"subsampling" in lib.pb_last_error()
        assert lib.pb_remap_planar_supported(None, sid, 1) == INVALID and lib.pb_last_error() == b"null argument"
        for S in (1, 2):
            ok_s, ok_d = packed(4, 8, S, sub), packed(6, 12, S, sub)
            assert ok_s[4] == S * planar_ref.frame_samples(4, 8, sub)
            # the defaults and their spelled-out form pass every argument check: what is left is the plan (deferred)
            yv12 = (ok_s[0], ok_s[1], ok_s[3], ok_s[2], ok_s[4])  # planes 1 and 2 swapped
            for sl, dl in ((None, None), (ok_s, ok_d), ((0,) * 5, (0,) * 5), (yv12, None), ((S * 8 + S, S * 8, S * 9 * 4 + S, 1024, 0), (256, 128, 256 * 9, 256 * 16, 256 * 32))):
                rc, msg = _call(lib, plan, sid, S, sl=sl, dl=dl)
                assert rc == UNSUPPORTED and b"pb_index_map_i32" in msg, (S, sl, dl, msg)
            # a 1-byte plane may start anywhere; a 2-byte one at any even address
            assert _call(lib, plan, sid, S, src=FAKE + S, dst=FAKE + 3 * S)[0] == UNSUPPORTED
            assert lib.pb_remap_planar_supported(plan, sid, S) == 0
            assert _call(lib, plan, sid, S, n=0)[0] == 0  # no frames: nothing to launch
            for which in ("sl", "dl"):
                base = ok_s if which == "sl" else ok_d
                name = b"source" if which == "sl" else b"destination"
                ce = base[3] - base[2]  # a packed chroma plane's bytes
                for broken, rule in (((base[0] - S, 0, 0, 0, 0), b"pitch smaller than a row"),
                                     ((0, base[1] - S, 0, 0, 0), b"chroma_pitch smaller than a row"),
                                     ((0, 0, base[2] - S, 0, 0), b"planes overlap"),  # plane 1 starts inside plane 0
                                     ((0, 0, 0, base[2] - S, 0), b"planes overlap"),  # plane 2 starts inside plane 0
                                     ((0, 0, 0, base[3] - S, 0), b"planes overlap"),  # plane 2 starts inside plane 1
                                     ((0, 0, base[3] + ce - S, base[3], 0), b"planes overlap"),  # swapped: plane 1 starts inside plane 2
                                     ((0, 0, 0, 0, base[4] - S), b"frame_stride smaller than a frame"),
                                     ((0, 0, 0, base[3] + S, base[4]), b"frame_stride smaller than a frame"),  # plane 2 ends beyond the stride
                                     ((0, 0, base[4], 0, base[4] + ce - S), b"frame_stride smaller than a frame")):  # plane 1 behind plane 2, beyond it
                    rc, msg = _call(lib, plan, sid, S, **{which: broken})
                    assert rc == INVALID and name in msg and rule in msg, (S, which, broken, msg)
                if S == 2:  # by one byte: not a multiple of one sample
                    for broken in ((base[0] + 1, 0, 0, 0, 0), (0, base[1] + 1, 0, 0, 0), (base[0], base[1], base[2] + 1, base[3] + 2, 0), (0, 0, 0, base[3] + 1, 0), (0, 0, 0, 0, base[4] + 1)):
                        rc, msg = _call(lib, plan, sid, S, **{which: broken})
                        assert rc == INVALID and b"multiples of 2" in msg and name in msg, (which, broken, msg)
                # a member no frame below 2^31 bytes can have - wrapping products included - is refused before anything is multiplied
                for pos in range(4):
                    for v in (1 << 31, (1 << 63) + (1 << 20), (1 << 64) - 2):
                        huge = tuple(v if i == pos else 0 for i in range(5))
                        rc, msg = _call(lib, plan, sid, S, **{which: huge})
                        assert rc == UNSUPPORTED and b"2^31" in msg, (S, which, huge, msg)
            if S == 2:
                for kw in ({"src": FAKE + 1}, {"dst": FAKE + 1}):
                    rc, msg = _call(lib, plan, sid, S, **kw)
                    assert rc == INVALID and b"multiples of" in msg, (kw, msg)
            # the track entry point: the same checks first, then the table's; n_frames == 0 needs no device
            assert _track_call(lib, plan, sid, S, sl=(ok_s[0] - S, 0, 0, 0, 0))[1].endswith(b"pitch smaller than a row")
            assert _track_call(lib, plan, sid, S, table=None) == (INVALID, b"null rotation table")
            assert _track_call(lib, plan, sid, S, table=FAKE + 4)[0] == INVALID and _track_call(lib, plan, sid, S, k=0)[0] == INVALID
            assert _track_call(lib, plan, sid, S, k=nat.PB_MAX_ROTATIONS + 1)[0] == INVALID
            assert _track_call(lib, plan, sid, S, n=0)[0] == 0
    finally:
        lib.pb_plan_destroy(plan)


@pytest.mark.parametrize("dims,ok", [((5, 8, 4, 8), ("444", "422")), ((4, 8, 3, 8), ("444", "422")), ((4, 7, 4, 8), ("444",)), ((4, 8, 4, 9), ("444",)),
                                     ((3, 5, 7, 9), ("444",)), ((4, 8, 6, 12), ("444", "422", "420"))])
def test_the_dimension_rule_per_subsampling(dims, ok):
    lib, plan = _deferred(*dims)
    try:
        for sub, sid in SUBS.items():
            for S in (1, 2):
                rc, msg = _call(lib, plan, sid, S)
                if sub in ok:
                    assert rc == UNSUPPORTED and lib.pb_remap_planar_supported(plan, sid, S) == 0, (dims, sub, msg)  # (deferred: the only refusal left)
                else:
                    assert rc == INVALID and b"even" in msg and (b"4:2:2" if sub == "422" else b"4:2:0") in msg, (dims, sub, msg)
                    assert lib.pb_remap_planar_supported(plan, sid, S) == INVALID and b"even" in lib.pb_last_error()
                    assert _track_call(lib, plan, sid, S)[0] == INVALID
    finally:
        lib.pb_plan_destroy(plan)


# ---- Plan.remap_planar's own checks -----------------------------------------------------------------------------------------------------
class FakeDevice:
    """Passes nat.is_device_array's test without a device: the checks under test run before anything touches it."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, np.dtype(dtype)

    def data_ptr(self):
        return FAKE


def test_plan_remap_planar_checks_its_arguments_without_a_gpu(monkeypatch):
    monkeypatch.setattr(nat, "is_device_array", lambda a: isinstance(a, FakeDevice))
    monkeypatch.setattr(nat, "is_tensor", lambda a: False)
    p = nat.make_proj(nat.KIND_PANO, 4, 8)
    plan = nat.Plan(p, [], p, defer=True)
    for sub in ("444", "422", "420", nat.PLANAR_420):
        assert not plan.planar_supported(sub) and not plan.planar_supported(sub, 2)
    with pytest.raises(nat.PbError, match="bytes_per_sample"):
        plan.planar_supported("420", 3)
    with pytest.raises(ValueError, match="subsampling"):
        plan.planar_supported("411")
    with pytest.raises(ValueError, match="subsampling"):
        plan.remap_planar(FakeDevice((48,), np.uint8), 7)
    with pytest.raises(nat.PbError, match="device arrays"):
        plan.remap_planar(np.zeros(48, np.uint8), "420")
    with pytest.raises(nat.PbError, match="pb_index_map_i32"):  # (the raw calls: refused by the library, a deferred plan)
        plan.launch_planar(FAKE, FAKE, "422", 1, 0)
    with pytest.raises(nat.PbError, match="uint8 or uint16"):
        plan._video_source(nat.video_family(nat.PLANAR_420), FakeDevice((48,), np.float32), None)
    # shapes: flat or (N, flat); 4:4:4 also (3, h, w) / (N, 3, h, w); nothing else
    for sub, good, bad in (("420", [(48,), (3, 48)], [(6, 8), (47,), (3, 4, 8), (96,)]), ("422", [(64,), (2, 64)], [(8, 8), (48,), (3, 4, 8)]),
                           ("444", [(96,), (5, 96), (3, 4, 8), (2, 3, 4, 8)], [(12, 8), (4, 8, 3), (3, 8, 4), (64,)])):
        sid = SUBS[sub]
        for shp in good:
            src, fam, got, dt, sl, n = plan._video_source(nat.video_family(sid), FakeDevice(shp, np.uint16), None)
            assert (fam.sub, got, dt, sl) == (sid, shp, np.dtype(np.uint16), None) and n == (shp[0] if len(shp) in (2, 4) else 1)
        for shp in bad:
            with pytest.raises(nat.PbError, match="packed source frames"):
                plan._video_source(nat.video_family(sid), FakeDevice(shp, np.uint8), None)
    # frames at a layout: a 1-D buffer, counted by the stride
    l = (16, 8, 80, 128, 256)
    assert plan._video_source(nat.video_family(nat.PLANAR_420), FakeDevice((256 * 2 + 140,), np.uint8), l)[-1] == 3  # (a frame ends with plane 2's last sample: 128 + 8 + 4)
    with pytest.raises(nat.PbError, match="1-D"):
        plan._video_source(nat.video_family(nat.PLANAR_420), FakeDevice((3, 256), np.uint8), l)
    with pytest.raises(nat.PbError, match="spans 140"):
        plan._video_source(nat.video_family(nat.PLANAR_420), FakeDevice((139,), np.uint8), l)
    # the dimension rule per subsampling
    for dims, refused in (((3, 8), ("420",)), ((4, 7), ("422", "420")), ((3, 7), ("422", "420"))):
        odd = nat.Plan(nat.make_proj(nat.KIND_PANO, *dims), [], p, defer=True)
        for sub, sid in SUBS.items():
            n = planar_ref.frame_samples(4, 8, sub)
            if sub in refused:
                with pytest.raises(nat.PbError, match="even"):
                    odd._video_source(nat.video_family(sid), FakeDevice((n,), np.uint8), None)
                with pytest.raises(nat.PbError, match="even"):
                    odd.planar_supported(sub)
            else:
                assert not odd.planar_supported(sub)
    with pytest.raises(ValueError, match="rotations"):
        plan.remap_track_planar(FakeDevice((2, 48), np.uint8), np.eye(3)[None], "420")  # two frames, one rotation


def test_layout_defaults_and_refusals():
    assert nat.planar_layout(None) is None
    l = nat.planar_layout((256, 128, 1024, 2048, 0))
    assert (l.pitch, l.chroma_pitch, l.offset1, l.offset2, l.frame_stride) == (256, 128, 1024, 2048, 0) and nat.planar_layout(l) is l
    l = nat.planar_layout({"chroma_pitch": 64})
    assert (l.pitch, l.chroma_pitch, l.offset1, l.offset2, l.frame_stride) == (0, 64, 0, 0, 0)
    with pytest.raises(ValueError):
        nat.planar_layout({"uv_offset": 64})
    for sub, sid in SUBS.items():
        for S in (1, 2):
            p = packed(4, 8, S, sub)
            assert nat.planar_frame_bytes(None, 4, 8, S, sid) == p[:4] + (p[4], p[4])
            assert nat.planar_frame_samples(4, 8, sid) * S == p[4]
            # the planes swapped (YV12): the same span; a stride of its own
            assert nat.planar_frame_bytes(nat.planar_layout((0, 0, p[3], p[2], 512)), 4, 8, S, sid)[2:] == (p[3], p[2], p[4], 512)
            for broken, rule in (((p[0] - S, 0, 0, 0, 0), "pitch"), ((0, p[1] - S, 0, 0, 0), "pitch"), ((0, 0, p[2] - S, 0, 0), "overlap"), ((0, 0, 0, p[3] - S, 0), "overlap"),
                                 ((0, 0, p[3], p[3] + S, 0), "overlap"), ((0, 0, 0, 0, p[4] - S), "frame_stride")):
                with pytest.raises(nat.PbError, match=rule):
                    nat.planar_frame_bytes(nat.planar_layout(broken), 4, 8, S, sid)
    with pytest.raises(nat.PbError, match="multiples of 2"):
        nat.planar_frame_bytes(nat.planar_layout((17, 0, 0, 0, 0)), 4, 8, 2, nat.PLANAR_420)
    # padding after a plane's last row belongs to nobody: plane 1 may start right behind plane 0's last sample
    assert nat.planar_frame_bytes(nat.planar_layout((16, 0, 16 * 3 + 8, 0, 0)), 4, 8, 1, nat.PLANAR_420)[2:4] == (56, 64)


# ---- the pixel_format table and the host pipeline ---------------------------------------------------------------------------------------
FORMATS = {
    "yuv420p": (np.uint8, "420", (16, 128, 128)), "yuv422p": (np.uint8, "422", (16, 128, 128)), "yuv444p": (np.uint8, "444", (16, 128, 128)),
    "yuv420p10le": (np.uint16, "420", (64, 512, 512)), "yuv422p10le": (np.uint16, "422", (64, 512, 512)), "yuv444p10le": (np.uint16, "444", (64, 512, 512)),
    "yuv420p16le": (np.uint16, "420", (4096, 32768, 32768)), "yuv444p16le": (np.uint16, "444", (4096, 32768, 32768)),
    "gbrp": (np.uint8, "444", (0, 0, 0)), "gbrp16le": (np.uint16, "444", (0, 0, 0)),
}


def test_the_pixel_format_table():
    assert set(nat.PLANAR_FORMATS) == set(FORMATS) and len(FORMATS) == 10
    for name, (dt, sub, fill) in FORMATS.items():
        assert nat.PLANAR_FORMATS[name] == (np.dtype(dt), SUBS[sub], fill), name
    assert not set(nat.PLANAR_FORMATS) & {"nv12", "p010"}


class FakePlanarPlan(FakePlan):
    """... with the planar launch: 'remaps' a flat frame by reversing it, and records subsampling, sample size and fill."""

    def launch_planar(self, src_ptr, dst_ptr, subsampling, n_frames, stream, bytes_per_sample, fill):
        n = nat.planar_frame_samples(self.src.height, self.src.width, subsampling) * bytes_per_sample
        a = np.frombuffer((C.c_ubyte * n).from_address(src_ptr), np.uint8)
        np.frombuffer((C.c_ubyte * n).from_address(dst_ptr), np.uint8)[...] = a[::-1]
        self.launches.append((int(stream), "planar", subsampling, bytes_per_sample, tuple(fill)))
        self.lib.log.append(("run", int(stream)))

    def launch_nv12(self, *a):
        raise AssertionError("a planar format took the semi-planar launch")


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_planar_frames_take_the_same_pipeline(pipe_env, fmt):  # noqa: F811
    lib, hp = pipe_env
    dt, sub, fill = FORMATS[fmt]
    S = np.dtype(dt).itemsize
    rng = np.random.default_rng(11)
    n = planar_ref.frame_samples(24, 40, sub)
    frames = [rng.integers(0, 256, n).astype(dt) for _ in range(3)]
    plan = FakePlanarPlan(24, 40, lib)
    outs = list(batch.remap_frames(plan, frames, pixel_format=fmt))
    assert [l[1:] for l in plan.launches] == [("planar", SUBS[sub], S, fill)] * 3
    assert all(o.dtype == np.dtype(dt) and o.shape == (n,) and np.array_equal(o.view(np.uint8), f.view(np.uint8)[::-1]) for f, o in zip(frames, outs))
    one = hp.remap_ndarray(plan, frames[1], pixel_format=fmt)
    assert one.dtype == np.dtype(dt) and one.shape == (n,) and np.array_equal(one.view(np.uint8), frames[1].view(np.uint8)[::-1])
    if sub == "444":  # also as (3, h, w)
        cube = hp.remap_ndarray(plan, frames[1].reshape(3, 24, 40), pixel_format=fmt)
        assert cube.shape == (3, 24, 40) and np.array_equal(cube.ravel(), one)
    # what is not such a frame, or not such a call, is a ValueError - before anything is launched
    count = len(plan.launches)
    for bad in (frames[0][:-1], frames[0].astype(np.float32), frames[0].reshape(-1, 40), frames[0].astype(np.uint16 if S == 1 else np.uint8)):
        with pytest.raises(ValueError):
            hp.remap_ndarray(plan, bad, pixel_format=fmt)
    if sub != "444":
        with pytest.raises(ValueError):
            hp.remap_ndarray(plan, np.zeros((3, 24, 40), dt), pixel_format=fmt)
    for kw in ({"interpolation": "bilinear"}, {"supersample": 2}, {"rotations": np.eye(3)[None]}):
        with pytest.raises(ValueError):
            batch.remap_frames(plan, frames, pixel_format=fmt, **kw)
    # the dimension rule names the format
    for dims, refused in (((25, 40), ("420",)), ((24, 39), ("420", "422"))):
        odd = FakePlanarPlan(*dims, lib)
        a = np.zeros(planar_ref.frame_samples(dims[0] & ~1, dims[1] & ~1, sub), dt)
        if sub in refused:
            with pytest.raises(ValueError, match=f"{fmt} frames have even"):
                hp.remap_ndarray(odd, a, pixel_format=fmt)
    assert len(plan.launches) == count
    del outs, one


def test_the_dimension_messages_name_the_rule():
    assert nat.planar_dims_rule(nat.PLANAR_422, "yuv422p") == "yuv422p frames have even widths"
    assert nat.planar_dims_rule(nat.PLANAR_420, "yuv420p") == "yuv420p frames have even widths and heights"
    assert nat.planar_dims_ok(nat.PLANAR_444, (33, 35)) and nat.planar_dims_ok(nat.PLANAR_422, (33, 36)) and not nat.planar_dims_ok(nat.PLANAR_422, (33, 35))
    assert not nat.planar_dims_ok(nat.PLANAR_420, (33, 36)) and nat.planar_dims_ok(nat.PLANAR_420, (34, 36), (2, 2))


# ---- utils ------------------------------------------------------------------------------------------------------------------------------
def test_the_plane_helpers_are_views_and_inverse_to_each_other():
    assert "planar_planes" in pb.utils.__all__ and "planar_frame" in pb.utils.__all__
    for sub, (h, w) in (("444", (3, 5)), ("422", (3, 6)), ("420", (4, 6)), (nat.PLANAR_420, (4, 6))):
        cx, cy = nat.PLANAR_SHIFTS[nat.planar_subsampling(sub)]
        for dt in (np.uint8, np.uint16):
            n = h * w + 2 * (h >> cy) * (w >> cx)
            frame = np.arange(n).astype(dt)
            p0, p1, p2 = pb.utils.planar_planes(frame, h, w, sub)
            assert p0.shape == (h, w) and p1.shape == p2.shape == (h >> cy, w >> cx)
            assert all(np.shares_memory(p, frame) for p in (p0, p1, p2))
            assert p0[0, 0] == 0 and p1[0, 0] == h * w and p2[-1, -1] == n - 1
            want = planar_ref.planes(frame, h, w, {0: "444", 1: "422", 2: "420"}[nat.planar_subsampling(sub)])
            assert all(np.array_equal(a, b) for a, b in zip((p0, p1, p2), want))
            back = pb.utils.planar_frame(p0, p1, p2)
            assert back.dtype == frame.dtype and np.array_equal(back, frame) and not np.shares_memory(back, frame)
    cube = np.arange(3 * 3 * 5, dtype=np.uint8).reshape(3, 3, 5)
    assert all(np.array_equal(p, cube[k]) for k, p in enumerate(pb.utils.planar_planes(cube, 3, 5, "444")))
    for bad in (((29,), 3, 5, "420"), ((29,), 3, 5, "422"), ((44,), 3, 5, "444"), ((3, 3, 6), 3, 6, "422"), ((6, 6), 4, 6, "420")):
        with pytest.raises(ValueError):
            pb.utils.planar_planes(np.zeros(bad[0], np.uint8), *bad[1:])
    with pytest.raises(ValueError):
        pb.utils.planar_planes(np.zeros(36, np.uint8), 4, 6, "411")
    with pytest.raises(ValueError):
        pb.utils.planar_frame(np.zeros((4, 6), np.uint8), np.zeros((2, 3), np.uint16), np.zeros((2, 3), np.uint16))
    with pytest.raises(ValueError):
        pb.utils.planar_frame(np.zeros((4, 6), np.uint8), np.zeros((2, 3), np.uint8), np.zeros((4, 3), np.uint8))
    with pytest.raises(ValueError):
        pb.utils.planar_frame(np.zeros((4, 6), np.uint8), np.zeros((3, 3), np.uint8), np.zeros((3, 3), np.uint8))
