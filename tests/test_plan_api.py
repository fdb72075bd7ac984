"""The explicit plan API (pb_plan_create_ex / pb_plan_prepare / pb_plan_set_window_budget / pb_plan_serialize) and
the host-side plan cache: deferred plans cost nothing and run the faithful kernel, preparation never tunes unless
asked, a serialized plan reproduces the original bytes, the cache is LRU, per device and thread-safe."""

import ctypes
import threading

import numpy as np
import pytest
import torch

import photonbend_amd as pb
from photonbend_amd import _native as nat
from photonbend_amd.core import projection as proj
from tests import helpers as H
from tests.cases import Case, cam, dbl, inscribed, pano

CASES = [
    Case("api_pano", cam(320, 352, "equisolid", 200, inscribed(320)), pano(256, 512), [(10, 20, 30)]),
    Case("api_cam", pano(256, 512), cam(320, 320, "equidistant", 360, inscribed(320))),
    Case("api_double", pano(256, 512), dbl(240, 480, "equidistant", 195), [(3, 90, -7)], mask=2),
    Case("api_double_sep", pano(256, 512), dbl(240, 480, "equidistant", 180), mask=2),
]


def _projs(case):
    src, cmap = H.pb_chain(case, image=np.zeros((case.src[1], case.src[2], 3), np.uint8))
    return cmap.dst_proj, cmap.rotations, src._proj()


# ---- CPU: argument validation and the cache's bookkeeping (deferred plans need no device) -----------------
def test_create_ex_argument_validation():
    lib = nat.load()
    h = ctypes.c_void_p()
    good = nat.make_proj(nat.KIND_PANO, 8, 16)
    assert lib.pb_plan_create_ex(ctypes.byref(good), None, 0, ctypes.byref(good), 64, 0, ctypes.byref(h)) == -1  # unknown flag
    assert lib.pb_plan_create_ex(ctypes.byref(good), None, 0, ctypes.byref(good), nat.PLAN_BILINEAR, 0, ctypes.byref(h)) == -1  # (a pb_plan_prepare flag)
    assert lib.pb_plan_create_ex(ctypes.byref(good), None, 0, ctypes.byref(good), 0, -5, ctypes.byref(h)) == -1
    assert lib.pb_plan_create_ex(ctypes.byref(good), None, 0, ctypes.byref(good), nat.PLAN_DEFER, 0, ctypes.byref(h)) == 0
    n = ctypes.c_size_t()
    assert lib.pb_plan_serialize(h, None, 0, ctypes.byref(n)) == -3  # nothing prepared: unsupported
    assert lib.pb_plan_set_window_budget(h, 8192) == -3
    assert lib.pb_plan_window_budget(h) == 0
    lib.pb_plan_destroy(h)
    assert lib.pb_plan_deserialize(b"\0" * 16, 16, ctypes.byref(h)) == -1
    junk = bytes(4096)
    assert lib.pb_plan_deserialize(junk, len(junk), ctypes.byref(h)) == -1
    assert lib.pb_stream_copy(None, None, 16, None) == -1


def test_plan_cache_is_lru_and_keyed_by_device(monkeypatch):
    monkeypatch.setattr(proj, "_PLAN_CACHE_MAX", 3)
    proj._PLAN_CACHE.clear()
    src = nat.make_proj(nat.KIND_PANO, 8, 16)
    dsts = [nat.make_proj(nat.KIND_PANO, 8 + k, 16) for k in range(4)]
    plans = [proj._plan_for(d, [], src, device="cuda:0", eager=False) for d in dsts[:3]]
    assert proj._plan_for(dsts[0], [], src, device="cuda:0", eager=False) is plans[0]  # a hit refreshes the entry
    proj._plan_for(dsts[3], [], src, device="cuda:0", eager=False)  # evicts ONE entry: the least recently used (dsts[1])
    assert len(proj._PLAN_CACHE) == 3
    assert proj._plan_for(dsts[0], [], src, device="cuda:0", eager=False) is plans[0]
    assert proj._plan_for(dsts[2], [], src, device="cuda:0", eager=False) is plans[2]
    assert proj._plan_for(dsts[1], [], src, device="cuda:0", eager=False) is not plans[1]
    # same geometry on another device: another plan
    assert proj._plan_for(dsts[0], [], src, device="cuda:1", eager=False) is not proj._plan_for(dsts[0], [], src, device="cuda:0", eager=False)
    proj._PLAN_CACHE.clear()


def test_plan_cache_survives_concurrent_callers():
    proj._PLAN_CACHE.clear()
    src = nat.make_proj(nat.KIND_PANO, 8, 16)
    got, errs = [], []

    def worker(k):
        try:
            for i in range(50):
                got.append(proj._plan_for(nat.make_proj(nat.KIND_PANO, 8 + (i + k) % 5, 16), [], src, device="cuda:0", eager=False))
        except Exception as exc:  # pragma: no cover
            errs.append(exc)

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs and len(got) == 200 and len(proj._PLAN_CACHE) == 5
    proj._PLAN_CACHE.clear()


def test_launch_gate_holds_launches_off_a_rebuild():
    """_native._LaunchGate: any number of launches inside at once; close() waits for them to leave and keeps new ones out until open()."""
    import time

    gate = nat._LaunchGate()
    log, inside = [], threading.Event()

    def launch(k, hold):
        gate.enter()
        log.append(("in", k))
        inside.set()
        time.sleep(hold)
        log.append(("out", k))
        gate.leave()

    a = threading.Thread(target=launch, args=(0, 0.2))
    a.start()
    inside.wait(5)
    gate.enter()  # (a second launch beside the first)
    gate.leave()
    closer = threading.Thread(target=lambda: (gate.close(), log.append(("closed",)), time.sleep(0.1), log.append(("opening",)), gate.open()))
    closer.start()
    time.sleep(0.05)
    b = threading.Thread(target=launch, args=(1, 0.0))
    b.start()
    for t in (a, closer, b):
        t.join(5)
        assert not t.is_alive()
    assert log == [("in", 0), ("out", 0), ("closed",), ("opening",), ("in", 1), ("out", 1)]


# ---- GPU ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_deferred_prepare_serialize_roundtrip(case):
    d, rots, s = _projs(case)
    frames = torch.stack([nat.synth_frame(case.src[1], case.src[2], frame=f, circle_mask=case.mask) for f in range(2)])
    plan = nat.Plan(d, rots, s, defer=True, bilinear=True)  # (with the opt-in mode's tables, like the plan a blob restores)
    info = plan.info()
    assert not info["fast_path"] and info["tiles"] == -1 and info["window_budget"] == 0
    faithful = plan.remap(frames).clone()  # a deferred plan runs the float64 chain
    plan.prepare(budget=6144)
    info = plan.info()
    assert info["fast_path"] and info["window_budget"] == 6144 and plan.timing()["prepare_ms"] > 0 and plan.timing()["tune_ms"] == 0
    assert torch.equal(plan.remap(frames), faithful)
    plan.prepare()  # idempotent
    assert plan.info() == info
    blob = plan.serialize()
    twin = nat.Plan.deserialize(blob, d, rots, s)
    assert twin.info() == info
    assert torch.equal(twin.remap(frames), faithful) and torch.equal(twin.remap(frames[1]), faithful[1])
    # the opt-in bilinear mode's launch (its own budget, table copies, half windows, LDS pool) is rebuilt from the blob: same tiles, same bytes
    bil = plan.remap(frames, interpolation="bilinear").clone()
    assert twin.bilinear_tile_mix() == plan.bilinear_tile_mix() and twin.bilinear_launch_shape() == plan.bilinear_launch_shape()
    assert torch.equal(twin.remap(frames, interpolation="bilinear"), bil)
    twin.set_window_budget(12288)  # the certified flags travel with the blob
    assert twin.info()["lean_tiles"] >= info["lean_tiles"] and torch.equal(twin.remap(frames), faithful)
    assert torch.equal(twin.remap(frames, interpolation="bilinear"), bil)  # (the nearest mode's budget does not reach the bilinear mode's tables)
    # a corrupted blob is rejected, not uploaded
    bad = bytearray(blob)
    bad[len(bad) // 2] ^= 0x40
    with pytest.raises(nat.PbError, match="corrupt"):
        nat.Plan.deserialize(bytes(bad), d, rots, s)
    with pytest.raises(nat.PbError):
        nat.Plan.deserialize(blob[:-7], d, rots, s)
    # an intact blob of ANOTHER request (one more rotation; another field of view) is refused: the cache's file name is no proof
    other = list(rots) + [np.eye(3)]
    with pytest.raises(nat.PbError, match="another geometry"):
        nat.Plan.deserialize(blob, d, other, s)
    if d.kind != nat.KIND_PANO:
        import copy

        d2 = copy.copy(d)
        d2.fov = d.fov * 0.999
        with pytest.raises(nat.PbError, match="another geometry"):
            nat.Plan.deserialize(blob, d2, rots, s)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_bilinear_tables_are_built_at_the_modes_first_use(case):
    """Round 6: a plan made for the reference's sampler (PB_PLAN_NO_BILINEAR, the Python default) carries no state of the opt-in bilinear
    mode; pb_remap_bilinear_u8 on it is still correct - the mode's float64 kernels - and pb_plan_prepare(PB_PLAN_BILINEAR) builds the
    tables later: then the bytes are those of a plan that had them from the start, the nearest bytes and the window budget never move."""
    d, rots, s = _projs(case)
    lib = nat.load()
    frame = nat.synth_frame(case.src[1], case.src[2], frame=2, circle_mask=case.mask)
    eager = nat.Plan(d, rots, s, bilinear=True)
    lazy = nat.Plan(d, rots, s)
    tiles = eager.info()["tiles"]
    assert eager.info()["bilinear_float64_tiles"] == 0 and lazy.info()["bilinear_float64_tiles"] == tiles > 0
    near = eager.remap(frame)
    assert torch.equal(lazy.remap(frame), near)
    want = eager.remap(frame, interpolation="bilinear")
    eager.set_mode(nat.MODE_FAITHFUL)
    f64 = eager.remap(frame, interpolation="bilinear")
    # through the C ABI, without the wrapper's ensure_bilinear: the float64 kernels of the mode
    out = torch.empty_like(want)
    nat.check(lib.pb_remap_bilinear_u8(lazy.handle, frame.data_ptr(), out.data_ptr(), 1, 0, 0, nat.current_stream()))
    torch.cuda.synchronize()
    assert torch.equal(out, f64)
    budget = lazy.info()["window_budget"]
    lazy.set_window_budget(5120)
    assert torch.equal(lazy.remap(frame, interpolation="bilinear"), want)  # (the wrapper builds the tables at the first bilinear use)
    assert lazy.info()["bilinear_float64_tiles"] == 0 and lazy.info()["window_budget"] == 5120 != budget
    assert torch.equal(lazy.remap(frame), near)
    assert lazy.bilinear_tile_mix() == nat.Plan(d, rots, s, bilinear=True).bilinear_tile_mix()
    # a deferred plan remembers the wish for its preparation
    late = nat.Plan(d, rots, s, defer=True)
    assert torch.equal(late.remap(frame, interpolation="bilinear"), f64)
    late.prepare()
    assert late.info()["bilinear_float64_tiles"] == 0 and torch.equal(late.remap(frame, interpolation="bilinear"), want)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [Case("api_race_pano", cam(1536, 1536, "equidistant", 360, inscribed(1536)), pano(1024, 2048)),
                                  Case("api_race_double", pano(1024, 2048), dbl(960, 1920, "equidistant", 195), [(3, 90, -7)], mask=2)], ids=lambda c: c.name)
def test_nearest_launches_run_on_while_another_thread_builds_the_bilinear_tables(case):
    """A plan of the host's cache is shared by threads, and the opt-in mode's tables are built at the mode's first use on whichever thread
    that happens: the build leaves the nearest mode's launch table in place (nothing it holds changes), so launches of the reference's
    sampler on other threads run on through it - same bytes before, during and after."""
    d, rots, s = _projs(case)
    frame = nat.synth_frame(case.src[1], case.src[2], frame=4, circle_mask=case.mask)
    plan = nat.Plan(d, rots, s)
    want = plan.remap(frame)
    want_bil = nat.Plan(d, rots, s, bilinear=True).remap(frame, interpolation="bilinear")
    torch.cuda.synchronize()
    started, errors, bad = threading.Event(), [], []

    def nearest_loop():
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                out = torch.empty_like(want)
                for k in range(150):
                    plan.remap(frame, out=out)
                    if k == 10:
                        started.set()
                    torch.cuda.current_stream().synchronize()
                    if not torch.equal(out, want):
                        bad.append(k)
        except Exception as ex:  # pragma: no cover
            errors.append(ex)
        finally:
            started.set()

    t = threading.Thread(target=nearest_loop)
    t.start()
    started.wait(60)
    got_bil = plan.remap(frame, interpolation="bilinear")  # (builds the tables: plan.ensure_bilinear)
    t.join(120)
    assert not t.is_alive() and not errors and not bad, (errors, bad[:5])
    assert plan.info()["bilinear_float64_tiles"] == 0 and torch.equal(got_bil, want_bil)
    assert torch.equal(plan.remap(frame), want)


@pytest.mark.gpu
def test_destroyed_plans_hand_their_tables_to_the_next_and_shutdown_returns_them():
    """Round 6: a plan's tables come from the library's block cache and go back to it when the plan is destroyed (one device wait instead
    of a hipFree - itself a device wait - per table); pb_shutdown returns the idle blocks to the driver.  Whatever block a table lands
    in, the bytes are the same - also while an earlier plan of the same geometry is still alive and launching."""
    case = Case("api_cache", cam(1536, 1536, "equidistant", 360, inscribed(1536)), pano(1024, 2048), [(5, -10, 20)])
    d, rots, s = _projs(case)
    frame = nat.synth_frame(case.src[1], case.src[2], frame=6, circle_mask=case.mask)
    keeper = nat.Plan(d, rots, s)
    want = keeper.remap(frame).clone()
    want_bil = keeper.remap(frame, interpolation="bilinear").clone()
    for k in range(4):
        p = nat.Plan(d, rots, s, bilinear=bool(k & 1))
        assert torch.equal(p.remap(frame), want) and torch.equal(keeper.remap(frame), want)
        assert torch.equal(p.remap(frame, interpolation="bilinear"), want_bil)
        del p
    free_cached = torch.cuda.mem_get_info()[0]
    assert nat.load().pb_shutdown() == 0
    assert torch.cuda.mem_get_info()[0] >= free_cached
    assert torch.equal(keeper.remap(frame), want)  # live plans keep their tables
    p = nat.Plan(d, rots, s)
    assert torch.equal(p.remap(frame), want)


@pytest.mark.gpu
def test_plans_made_used_and_destroyed_on_four_threads_at_once():
    """The block cache under concurrent preparation and destruction: four threads each make, use (both samplers) and drop plans of three
    geometries in turn, tables of one thread's dead plans serving another's new ones - every result equals the single-threaded one."""
    cases = [CASES[0], CASES[2], Case("api_mt_cam", pano(512, 1024), cam(640, 640, "equidistant", 360, inscribed(640)))]
    setups = []
    for c in cases:
        d, rots, s = _projs(c)
        frame = nat.synth_frame(c.src[1], c.src[2], frame=1, circle_mask=c.mask)
        p = nat.Plan(d, rots, s)
        setups.append((d, rots, s, frame, p.remap(frame).clone(), p.remap(frame, interpolation="bilinear").clone()))
        del p
    torch.cuda.synchronize()
    errors, bad = [], []

    def worker(t):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                for k in range(12):
                    d, rots, s, frame, want, want_bil = setups[(k + t) % len(setups)]
                    p = nat.Plan(d, rots, s, bilinear=bool((k + t) & 1))
                    a = p.remap(frame)
                    b = p.remap(frame, interpolation="bilinear") if k % 3 == 0 else None
                    torch.cuda.current_stream().synchronize()
                    if not torch.equal(a, want) or (b is not None and not torch.equal(b, want_bil)):
                        bad.append((t, k))
                    del p
        except Exception as ex:  # pragma: no cover
            errors.append(ex)

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    [t.start() for t in ts]
    [t.join(180) for t in ts]
    assert not any(t.is_alive() for t in ts) and not errors and not bad, (errors, bad[:5])


@pytest.mark.gpu
def test_tune_is_opt_in_and_changes_no_byte():
    case = Case("tune", cam(1536, 1536, "equidistant", 360, inscribed(1536)), pano(1024, 2048))
    d, rots, s = _projs(case)
    frame = nat.synth_frame(1024, 2048, frame=3)
    plain = nat.Plan(d, rots, s)
    assert plain.timing()["tune_ms"] == 0 and plain.info()["window_budget"] == 7168
    tuned = nat.Plan(d, rots, s, tune=True)
    assert tuned.timing()["tune_ms"] > 0 and tuned.info()["window_budget"] in (12288, 10224, 8176, 7168)
    assert torch.equal(plain.remap(frame), tuned.remap(frame))


@pytest.mark.gpu
def test_facade_first_use_is_faithful_second_use_prepares(tmp_path, monkeypatch):
    proj._PLAN_CACHE.clear()
    monkeypatch.delenv("PB_PLAN_EAGER", raising=False)
    monkeypatch.setenv("PB_PLAN_CACHE_DIR", str(tmp_path))
    frame = nat.synth_frame(256, 512, frame=1).cpu().numpy()
    dst = pb.CameraImage(np.zeros((300, 300, 3), np.uint8), pb.utils.to_radians(190), pb.equisolid())
    src = pb.PanoramaImage(frame)
    a = src.process_coordinate_map(dst.get_coordinate_map())
    (entry,) = proj._PLAN_CACHE.values()
    assert entry[1] == 1 and not entry[2] and not entry[0].info()["fast_path"]
    b = src.process_coordinate_map(dst.get_coordinate_map())
    (entry,) = proj._PLAN_CACHE.values()
    assert entry[2] and entry[0].info()["fast_path"]
    assert np.array_equal(a, b)
    blobs = list(tmp_path.glob("*.pbplan"))
    assert len(blobs) == 1
    # a new process (here: an emptied cache) takes the prepared plan from disk, without certification
    proj._PLAN_CACHE.clear()
    monkeypatch.setenv("PB_PLAN_EAGER", "1")
    c = src.process_coordinate_map(dst.get_coordinate_map())
    (entry,) = proj._PLAN_CACHE.values()
    assert entry[0].info()["fast_path"] and entry[0].timing()["prepare_ms"] == 0
    assert np.array_equal(a, c)
    proj._PLAN_CACHE.clear()


@pytest.mark.gpu
def test_stride_validation_and_stream_copy():
    lib = nat.load()
    case = CASES[0]
    d, rots, s = _projs(case)
    plan = nat.Plan(d, rots, s)
    frames = torch.stack([nat.synth_frame(case.src[1], case.src[2], frame=f) for f in range(2)])
    out = torch.empty((2, d.height, d.width, 3), dtype=torch.uint8, device="cuda")
    assert lib.pb_remap_u8(plan.handle, frames.data_ptr(), out.data_ptr(), 2, 16, 0, None) == -1
    assert b"src_frame_stride" in lib.pb_last_error()
    assert lib.pb_remap_u8(plan.handle, frames.data_ptr(), out.data_ptr(), 2, 0, 16, None) == -1
    # the bilinear and supersampled entry points check their strides alike; a supersampled output frame is H/n x W/n
    small_src, small_dst = b"src_frame_stride smaller than a frame", b"dst_frame_stride smaller than a frame"
    assert lib.pb_remap_bilinear_u8(plan.handle, frames.data_ptr(), out.data_ptr(), 2, 16, 0, None) == -1
    assert lib.pb_last_error() == small_src
    assert lib.pb_remap_bilinear_u8(plan.handle, frames.data_ptr(), out.data_ptr(), 2, 0, 16, None) == -1
    assert lib.pb_last_error() == small_dst
    for n in (2, 4):
        ss_frame = 3 * (d.height // n) * (d.width // n)
        args = (plan.handle, n, nat.INTERP_IDS["nearest"], frames.data_ptr(), out.data_ptr(), 2)
        assert lib.pb_remap_ss_u8(*args, 16, 0, None, 0, 0, None) == -1
        assert lib.pb_last_error() == small_src
        assert lib.pb_remap_ss_u8(*args, 0, ss_frame - 1, None, 0, 0, None) == -1
        assert lib.pb_last_error() == small_dst
    a = torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda")
    b = torch.zeros_like(a)
    nat.check(lib.pb_stream_copy(b.data_ptr(), a.data_ptr(), a.numel(), None))
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert lib.pb_stream_copy(b.data_ptr() + 1, a.data_ptr(), 16, None) == -1


@pytest.mark.gpu
def test_two_threads_remap_same_sized_images_without_sharing_staging():
    """the staging buffers were process-wide; two threads remapping same-sized ndarray images at once
    interleaved their writes.  They are per thread now: every result must equal its single-threaded twin."""
    fov = pb.utils.to_radians(180)
    dst = pb.CameraImage(np.zeros((256, 256, 3), np.uint8), fov, pb.equidistant())
    frames = [nat.synth_frame(256, 512, frame=f).cpu().numpy() for f in range(4)]
    want = [pb.PanoramaImage(f).process_coordinate_map(dst.get_coordinate_map()) for f in frames]
    res = {}

    def worker(k):
        for rep in range(6):
            out = pb.PanoramaImage(frames[k]).process_coordinate_map(dst.get_coordinate_map())
            res[(k, rep)] = np.array_equal(out, want[k])

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert len(res) == 24 and all(res.values())


@pytest.mark.gpu
def test_threads_preparing_plans_at_once_share_the_scratch_cache_safely():
    """Round 4: the short-lived device buffers of plan preparation (counters, per-unit costs, column tables) come from a per-device cache
    shared by every thread.  Four threads prepare plans of four geometries over and over at the same time; every plan's index map must
    equal the one a single thread built, and its certification statistics too."""
    fov = pb.utils.to_radians(190)
    geoms = []
    for k, (h, w) in enumerate([(256, 256), (320, 288), (288, 352), (384, 384)]):
        d = pb.CameraImage(np.zeros((h, w, 3), np.uint8), fov, pb.equidistant())._proj("dst")
        s = nat.make_proj(nat.KIND_PANO, 256 + 32 * k, 512 + 64 * k)
        rots = [] if k % 2 == 0 else [pb.Rotation(0.1 * k, -0.2, 0.05).rotation_matrix]
        geoms.append((d, rots, s))
    serial = []
    for d, rots, s in geoms:
        p = nat.Plan(d, rots, s)
        serial.append((p.index_map().cpu().numpy(), p.info()["fix_pixels"], p.info()["lean_tiles"]))
    ok = {}

    def worker(k):
        d, rots, s = geoms[k]
        for rep in range(8):
            p = nat.Plan(d, rots, s)
            info = p.info()
            ok[(k, rep)] = np.array_equal(p.index_map().cpu().numpy(), serial[k][0]) and (info["fix_pixels"], info["lean_tiles"]) == serial[k][1:]

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert len(ok) == 32 and all(ok.values()), [k for k, v in ok.items() if not v]


_FAIL_SCRIPT = r"""
import sys, numpy as np, torch
from photonbend_amd import _native as nat
import photonbend_amd as pb
d = pb.CameraImage(np.zeros((256, 256, 3), np.uint8), pb.utils.to_radians(180), pb.equidistant())._proj("dst")
s = nat.make_proj(nat.KIND_PANO, 256, 512)
frame = nat.synth_frame(256, 512, frame=2)
plan = nat.Plan(d, [], s, bilinear=True)       # launch-table allocation no. 1: fine (the opt-in mode's tables with it: building them later re-applies the budget)
want = plan.remap(frame).clone()
bil = plan.remap(frame, interpolation="bilinear").clone()
try:
    plan.set_window_budget(6144)               # allocation no. 2: made to fail
    print("NO-ERROR"); sys.exit(3)
except nat.PbError as e:
    assert "launch table" in str(e), str(e)
# the plan is left WITHOUT a launch table, never with a stale one: launches take the direct-gather kernels - same bytes
assert plan.info()["window_budget"] == 6144
assert torch.equal(plan.remap(frame), want)
assert torch.equal(plan.remap(torch.stack([frame, frame]))[1], want)
got = plan.remap(frame, interpolation="bilinear")   # no table: the per-pixel float64 path instead of the tile models (no crash,
diff = (got.to(torch.int16) - bil.to(torch.int16)).abs()   # same picture: <= 1 LSB off the one-pixel rim of the black region)
assert int((diff > 1).sum()) <= diff.numel() // 100, int((diff > 1).sum())
plan.set_window_budget(7168)                   # allocation no. 3 succeeds: the table is back
assert torch.equal(plan.remap(frame), want)
print("OK")
"""


@pytest.mark.gpu
def test_failed_launch_table_allocation_leaves_a_working_plan():
    """VERDICT r2 weak 10 / ADVICE: a failed allocation inside pb_build_launch_table used to leave a stale or half-built table.
    The diagnostic build (-DPB_ABLATION, loaded through PB_LIB_PATH; the product has no such hook) fails the n-th allocation."""
    import os
    import subprocess
    import sys

    from photonbend_amd.build import DIAG_LIB_PATH

    if not os.path.exists(DIAG_LIB_PATH):
        pytest.skip("diagnostic build missing (python -m photonbend_amd.build --diag)")
    env = dict(os.environ, PB_LIB_PATH=DIAG_LIB_PATH, PB_FAIL_LTABLE_ALLOC="2")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _FAIL_SCRIPT], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr


@pytest.mark.gpu
def test_plans_are_prepared_outside_the_cache_lock(monkeypatch):
    """the cache lock guards the dictionary only.  While one thread prepares a geometry (held up inside _prepare),
    another thread gets a DIFFERENT geometry's prepared plan without waiting; eager callers of the SAME geometry wait for the one
    preparation and all receive its plan; a facade (non-eager) caller does not wait and gets the deferred plan; a failed preparation
    reaches its eager waiters as an error and leaves the entry retryable."""
    proj._PLAN_CACHE.clear()
    (d1, r1, s1), (d2, r2, s2) = _projs(CASES[0]), _projs(CASES[1])
    gate, entered = threading.Event(), threading.Event()
    real_prepare = proj._prepare
    calls = []

    def slow_prepare(plan, key, rotations):
        calls.append(key)
        if plan.dst.key() == d1.key():
            entered.set()
            assert gate.wait(60)
        return real_prepare(plan, key, rotations)

    monkeypatch.setattr(proj, "_prepare", slow_prepare)
    out = {}
    t1 = threading.Thread(target=lambda: out.__setitem__("owner", proj._plan_for(d1, r1, s1, device="cuda:0")))
    t1.start()
    assert entered.wait(60)
    # a different geometry: prepared while geometry 1 is still being prepared
    other = proj._plan_for(d2, r2, s2, device="cuda:0")
    assert other.info()["fast_path"]
    # the same geometry: a facade caller gets the deferred plan at once, eager callers wait for the owner's plan
    lazy = proj._plan_for(d1, r1, s1, device="cuda:0", eager=False)
    assert not lazy.info()["fast_path"]
    waiters = [threading.Thread(target=lambda k=k: out.__setitem__(k, proj._plan_for(d1, r1, s1, device="cuda:0"))) for k in range(3)]
    [t.start() for t in waiters]
    gate.set()
    t1.join(60)
    [t.join(60) for t in waiters]
    assert out["owner"].info()["fast_path"] and all(out[k] is out["owner"] for k in range(3))
    assert sum(1 for k in calls if k[1] == d1.key()) == 1, "one preparation per geometry"
    # a failing preparation: the owner raises, the entry stays unprepared and can be retried
    proj._PLAN_CACHE.clear()

    def failing_prepare(plan, key, rotations):
        raise nat.PbError("injected")

    monkeypatch.setattr(proj, "_prepare", failing_prepare)
    with pytest.raises(nat.PbError):
        proj._plan_for(d1, r1, s1, device="cuda:0")
    monkeypatch.setattr(proj, "_prepare", real_prepare)
    assert proj._plan_for(d1, r1, s1, device="cuda:0").info()["fast_path"]
    proj._PLAN_CACHE.clear()


@pytest.mark.gpu
def test_plans_give_their_device_memory_back():
    """Every buffer a plan owns - tile tables, launch-order copies, exact-index tables, the bilinear mode's coordinate tables, private
    right-eye copy and launch table - is released by pb_plan_destroy: forty plans of four kinds (single source, double-fisheye,
    deferred then prepared, deserialized), each used in both sampling modes, and the device's free memory is back where it was
    (a leak of one c3-sized coordinate table alone would be 12 MB per plan)."""
    import gc

    cases = [
        Case("leak_rot", cam(1024, 1024, "equisolid", 360, inscribed(1024)), cam(1024, 1024, "equidistant", 360, inscribed(1024)), [(30, 45, 10)]),
        Case("leak_dbl", pano(512, 1024), dbl(486, 972, "equidistant", 190), mask=2),
    ]

    def churn(n):
        for k in range(n):
            case = cases[k % 2]
            d, rots, s = _projs(case)
            frame = nat.synth_frame(case.src[1], case.src[2], frame=k, circle_mask=case.mask)
            plan = nat.Plan(d, rots, s, defer=(k % 4 == 2))
            if k % 4 == 2:
                plan.prepare()
            if k % 4 == 3:
                plan = nat.Plan.deserialize(plan.serialize(), d, rots, s)
            plan.remap(frame)
            plan.remap(frame, interpolation="bilinear")
            plan.set_window_budget(6144)
            del plan, frame
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()

    churn(4)  # (pools, module loading, torch's own caches: all warm)
    free0, _ = torch.cuda.mem_get_info()
    churn(40)
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (8 << 20), f"{(free0 - free1) >> 20} MiB of device memory did not come back after 40 plans"
