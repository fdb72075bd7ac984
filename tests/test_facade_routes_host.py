"""Which path a ``process_coordinate_map`` call takes, on the CPU: every cell of a grid of image layouts, residencies, maps,
sources, interpolations and supersample factors runs against stand-ins at the facade's boundary - ``_plan_for``, the host pipe, the
plan's launches, the map kernels, uploads and downloads - that record their name and the arguments that matter and return arrays of the
right shape and dtype on malloc'd "device" memory.  The expected traces (``tests/golden/facade_routes.json``, grouped by distinct trace)
were recorded by this very recorder from the facade as it was before it had a routing function: a difference is a behaviour change.

``python tests/test_facade_routes_host.py OUT.json`` records the grid of the package on the path into OUT.json."""

import contextlib
import gc
import itertools
import json
import os
import sys

import numpy as np
import pytest

from photonbend_amd import _device, _hostpipe
from photonbend_amd import _native as nat
from photonbend_amd.core import lens as lenses
from photonbend_amd.core import projection as pj
from photonbend_amd.core._coordmap import CoordinateMap
from tests.test_host_memory import FakePipeLib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "facade_routes.json")
MARK = -7.0  # what a stand-in kernel that "zeroes invalid pixels" leaves in a device map's first element

LAYOUTS = {  # name -> (trailing shape, dtype)
    "rgb8": ((3,), np.uint8), "grey8": ((), np.uint8), "grey16": ((), np.uint16), "rgba8": ((4,), np.uint8), "rgb16": ((3,), np.uint16),
    "rgba16": ((4,), np.uint16), "rgb_f32": ((3,), np.float32), "px5": ((5,), np.uint8), "u8_1x3": ((1, 3), np.uint8),
}
AXES = {
    "layout": list(LAYOUTS),
    "image": ["host", "device", "device_misaligned"],
    "map": ["lazy0", "lazy1", "lazy9", "coordmap", "ndarray", "ndarray_odd", "device", "ndarray_f32"],
    "source": ["pano", "camera", "camera_custom", "double", "double_custom", "cube"],
    "interpolation": ["nearest", "bilinear", "catmull-rom"],
    "supersample": [1, 2],
    "px_supported": [False, True],
}
IMAGE_HW = (4, 6)  # every source's image: (2N, 3N), which a cube map has to be and the others may be
ROTATIONS = [np.roll(np.eye(3), k % 3, axis=0) for k in range(9)]
DST_HW = (4, 8)  # the destination panorama (a supersampled map: n x this; the odd map: one row and column less)


def _dev(shape, dtype, zeroed=False):
    d = _device.DeviceArray(tuple(int(v) for v in shape), dtype)
    if zeroed:
        d.copy_from_host(np.zeros(d.shape, d.dtype))
    return d


def _sd(x):
    """[shape, dtype] of an array, with the running cell's image layout written as symbols (``Cell.symbols``) so that cells of different
    layouts that take the same path share a trace.  A symbol stands for one value per layout and a value that has a symbol is always
    written as it: two cells of one layout have the same symbolic trace exactly when they have the same trace."""
    shape, dt, sym = [int(v) for v in x.shape], np.dtype(x.dtype).name, Cell.symbols
    if shape[2:] == sym["T"] and dt == sym["D"]:
        return [shape[:2] + ["T"], "D"]
    if shape[2:] == [sym["B"]] and dt == "uint8":
        return [shape[:2] + ["B"], "uint8"]
    return [shape, dt]


def _s(value, symbol):
    return symbol if value == Cell.symbols[symbol] else value


def _mark(cmap):
    cmap.view(np.float64, (cmap.size,))[0:1].copy_from_host(np.array([MARK]))


class FakePlan:
    def __init__(self, dst, src, px_ok):
        self.dst, self.src, self.px_ok = dst, src, px_ok  # (px_ok: Plan.px_supported's answer, a parameter of the cell)

    def px_supported(self, bpp):
        return self.px_ok  # (a pure question: asked, not recorded)

    def remap(self, img, out=None, interpolation="nearest", supersample=1):
        Cell.log.append(["Plan.remap", _sd(img), interpolation, supersample])
        return _dev((self.dst.height // supersample, self.dst.width // supersample, 3), np.uint8)

    def remap_px(self, img):
        Cell.log.append(["Plan.remap_px", _sd(img), img.data_ptr() % 4])
        return _dev((self.dst.height, self.dst.width) + tuple(img.shape[2:]), img.dtype)

    def index_map(self, weights=False, device=None):
        Cell.log.append(["Plan.index_map", bool(weights), device is None])
        two = self.src.kind == nat.KIND_DOUBLE
        idx = _dev(((2,) if two else ()) + (self.dst.height, self.dst.width), np.int32)
        return (idx, _dev(idx.shape, np.float64) if two else None) if weights else idx


class Cell:
    """What the stand-ins of the running cell write to and answer from."""

    log: list = []
    px_ok = False
    symbols: dict = {}  # of its image layout: "T" trailing shape, "D" dtype, "B" bytes per pixel, "C" channels, "S" bytes per sample
    images: dict = {}  # (layout, residency) -> the image every cell of that kind shares: the facade only reads it


@contextlib.contextmanager
def stand_ins():
    """The facade's boundary, replaced: each stand-in appends [name, arguments that matter] to the running cell's log."""
    mp = pytest.MonkeyPatch()

    def plan_for(dst, rotations, src, device=None, eager=True):
        rotations = list(rotations)
        Cell.log.append(["_plan_for", len(rotations), bool(eager), device is None])
        if len(rotations) > nat.PB_MAX_ROTATIONS:
            raise nat.PbError(f"at most {nat.PB_MAX_ROTATIONS} rotations fit one fused plan")
        return FakePlan(dst, src, Cell.px_ok)

    def remap_ndarray(plan, image, interpolation="nearest", device=None, supersample=1):
        bpp = _hostpipe._px_format(plan, image, interpolation, supersample)[2]
        Cell.log.append(["remap_ndarray", _sd(image), bool(image.flags.c_contiguous), interpolation, supersample, _s(bpp, "B")])
        return np.zeros((plan.dst.height // supersample, plan.dst.width // supersample) + tuple(image.shape[2:]), image.dtype)

    def upload(a, device=None):
        Cell.log.append(["_upload", _sd(a)])
        return _dev(a.shape, a.dtype).copy_from_host(a)

    def to_host(t):
        Cell.log.append(["_to_host", _sd(t)])
        return t.numpy()

    def coordmap(dst, device=None):
        Cell.log.append(["coordmap"])
        return _dev((dst.height, dst.width, 3), np.float64, zeroed=True)

    def rotate(matrix, cmap):
        Cell.log.append(["rotate"])
        return _dev(cmap.shape, np.float64, zeroed=True)

    def sample_map(src, cmap, image):
        Cell.log.append(["sample_map", _sd(cmap), _sd(image)])
        _mark(cmap)
        return _dev(tuple(cmap.shape[:2]) + (3,), np.uint8)

    def sample_map_interp(interpolation, src, cmap, img, channels, dt, dist_l=None, dist_r=None):
        Cell.log.append(["sample_map_interp", interpolation, _sd(cmap), _sd(img), _s(int(channels), "C"), _s(np.dtype(dt).name, "D"), dist_l is not None, dist_r is not None])
        _mark(cmap)
        return _dev(tuple(cmap.shape[:2]) + (channels,), np.uint8 if src.kind == nat.KIND_DOUBLE else dt)

    def index_from_map(src, cmap, dist_l=None, dist_r=None):
        Cell.log.append(["index_from_map", _sd(cmap), dist_l is not None, dist_r is not None])
        _mark(cmap)
        two = src.kind == nat.KIND_DOUBLE
        idx = _dev(((2,) if two else ()) + tuple(cmap.shape[:2]), np.int32)
        return idx, (_dev(idx.shape, np.float64) if two else None)

    def gather_px(idx, img_bytes):
        Cell.log.append(["gather_px", _sd(idx), _sd(img_bytes)])
        return _dev(tuple(idx.shape) + (img_bytes.shape[2],), np.uint8)

    def gather_blend(idx2, w2, img_bytes, channels, sample_bytes):
        Cell.log.append(["gather_blend", _sd(idx2), _sd(img_bytes), _s(int(channels), "C"), _s(int(sample_bytes), "S")])
        return _dev((idx2.shape[1] * idx2.shape[2] * channels,), np.uint8)

    def box_reduce(x, n):
        Cell.log.append(["box_reduce", _sd(x), int(n)])
        return _dev((x.shape[0] // n, x.shape[1] // n) + tuple(x.shape[2:]), x.dtype)

    lib = FakePipeLib()  # 'device' memory is malloc'd, copies are memmoves
    mp.setattr(_device, "_lib", lambda: lib)
    mp.setattr(nat, "require_gpu", lambda: None)
    mp.setattr(nat, "on_device", lambda d: contextlib.nullcontext())
    mp.setattr(pj, "_plan_for", plan_for)
    mp.setattr(pj, "_upload", upload)
    mp.setattr(pj, "_to_host", to_host)
    mp.setattr(_hostpipe, "remap_ndarray", remap_ndarray)
    for fn in (coordmap, rotate, sample_map, sample_map_interp, index_from_map, gather_px, gather_blend, box_reduce):
        mp.setattr(nat, fn.__name__, fn)
    try:
        yield
    finally:
        Cell.images.clear()
        gc.collect()  # (no stand-in device array may outlive the stand-in library that frees it)
        mp.undo()


def _custom_lens():
    return lenses.Lens(lambda theta: theta * 1.0, lambda r: r * 1.0)


def _source(kind, image):
    if kind == "pano":
        return pj.PanoramaImage(image)
    if kind == "cube":
        return pj.CubemapImage(image)
    lens = _custom_lens() if kind.endswith("_custom") else lenses.equidistant()
    if kind.startswith("camera"):
        return pj.CameraImage(image, 3.0, lens)
    return pj.DoubleCameraImage(image, 3.3, lens)


def _image(layout, residency):
    if (layout, residency) not in Cell.images:
        Cell.images[layout, residency] = _new_image(layout, residency)
    return Cell.images[layout, residency]


def _new_image(layout, residency):
    tail, dt = LAYOUTS[layout]
    a = (np.arange(int(np.prod(IMAGE_HW + tail)), dtype=np.int64) % 251).astype(dt).reshape(IMAGE_HW + tail)
    if residency == "host":
        return a
    block = _dev((a.nbytes + 8,), np.uint8)  # (malloc's blocks are 16-byte aligned; one byte in, the view is misaligned for every pixel of 2^k bytes)
    view = _device.DeviceArray(a.shape, a.dtype, _ptr=block.data_ptr() + (1 if residency == "device_misaligned" else 0), _owner=block._owner)
    return view.copy_from_host(a)


def _map(kind, n):
    """(the map, what to pass as ``supersample``): a CoordinateMap carries its own factor, an array needs it said."""
    H, W = n * DST_HW[0], n * DST_HW[1]
    proj = nat.make_proj(nat.KIND_PANO, H, W)
    if kind.startswith("lazy"):
        return CoordinateMap(proj, ROTATIONS[:int(kind[4:])], supersample=n), None
    if kind == "coordmap":
        return CoordinateMap.from_array(proj, np.zeros((H, W, 3)), supersample=n), None
    if kind == "ndarray_odd":
        return np.zeros((H - 1, W - 1, 3)), n
    if kind == "ndarray_f32":
        return np.zeros((H, W, 3), np.float32), n
    if kind == "device":
        return _dev((H, W, 3), np.float64, zeroed=True), n
    return np.zeros((H, W, 3)), n


def run_cell(layout, residency, map_kind, source, interpolation, n, px_ok):
    """One call of the facade over the stand-ins (installed by the caller) -> its trace: [the ordered calls (how often ``_plan_for`` was
    asked is how often it is among them), the result's [type, shape, dtype] or the exception's [type, message], whether the map noted
    its invalid pixels zeroed, whether a host map was written back]."""
    log = Cell.log = []
    Cell.px_ok = px_ok
    tail, dt = LAYOUTS[layout][0], np.dtype(LAYOUTS[layout][1])
    Cell.symbols = {"T": list(tail), "D": dt.name, "C": int(np.prod(tail, dtype=int)), "S": dt.itemsize, "B": int(np.prod(tail, dtype=int)) * dt.itemsize}
    image = _image(layout, residency)
    cmap, ss = _map(map_kind, n)
    try:
        out = _source(source, image).process_coordinate_map(cmap, interpolation, ss)
        outcome = {"result": [type(out).__name__] + _sd(out)}
    except Exception as exc:  # (the facade's argument errors are part of its behaviour)
        outcome = {"raised": [type(exc).__name__, str(exc).replace(f"got {dt.name}", "got D")]}
    host = cmap._array if isinstance(cmap, CoordinateMap) else cmap
    return [log, outcome, bool(getattr(cmap, "_zero_invalid", False)), bool(isinstance(host, np.ndarray) and host.flat[0] == MARK)]


def cells():
    return itertools.product(*AXES.values())


def record():
    """The trace of every cell, in the order of ``cells()``."""
    with stand_ins():
        return [run_cell(*cell) for cell in cells()]


# The fixture: every level holds each distinct value once and the level above refers to it by index - calls, call sequences and outcomes;
# traces [sequence, outcome, noted, written back]; blocks, the traces of one (image, map, source, px_supported) over BLOCK_AXES; and
# "cells", the block of every (image, map, source, px_supported).  74 blocks serve the 288 of them.
BLOCK_AXES = ["layout", "interpolation", "supersample"]
_DIMS = [len(v) for v in AXES.values()]
_ORDER = [k for k, a in enumerate(AXES) if a not in BLOCK_AXES] + [list(AXES).index(a) for a in BLOCK_AXES]
_INNER = int(np.prod([len(AXES[a]) for a in BLOCK_AXES]))


def _intern(table, value):
    return table.setdefault(json.dumps(value), len(table))


def encode(traces):
    calls, sequences, outcomes, distinct, blocks = {}, {}, {}, {}, {}
    ids = [_intern(distinct, [_intern(sequences, [_intern(calls, c) for c in log]), _intern(outcomes, outcome), int(noted), int(written)])
           for log, outcome, noted, written in traces]
    rows = np.array(ids).reshape(_DIMS).transpose(_ORDER).reshape(-1, _INNER)
    cell_blocks = [_intern(blocks, row.tolist()) for row in rows]
    tables = {"calls": calls, "sequences": sequences, "outcomes": outcomes, "traces": distinct, "blocks": blocks}
    return {"axes": AXES, "block_axes": BLOCK_AXES, **{k: [json.loads(v) for v in t] for k, t in tables.items()}, "cells": cell_blocks}


def decode(rec):
    """The fixture -> the trace of every cell, in the order of ``cells()``."""
    assert rec["axes"] == AXES and rec["block_axes"] == BLOCK_AXES and len(rec["cells"]) * _INNER == int(np.prod(_DIMS))  # no cell dropped or added
    rows = np.array([rec["blocks"][b] for b in rec["cells"]]).reshape([_DIMS[k] for k in _ORDER])
    ids = rows.transpose(np.argsort(_ORDER)).reshape(-1)
    return [[[rec["calls"][c] for c in rec["sequences"][s]], rec["outcomes"][o], bool(noted), bool(written)]
            for s, o, noted, written in (rec["traces"][i] for i in ids)]


def test_every_cell_of_the_grid_takes_the_recorded_path():
    want = decode(json.load(open(GOLDEN)))
    got = json.loads(json.dumps(record()))
    wrong = [(cell, g, w) for cell, g, w in zip(cells(), got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(want)} cells differ; the first: {wrong[0][0]}\n got  {wrong[0][1]}\n want {wrong[0][2]}"


def _facts(**kw):
    base = dict(src=nat.make_proj(nat.KIND_CAMERA, 6, 6, nat.LENS_IDS["equidistant"], 3.0, 3.0, 2.0), height=6, width=6, tail=(3,),
                dt=np.dtype(np.uint8), bpp=3, on_device=False, map_kind="lazy", map_shape=(4, 8, 3), rotations=(), interpolation="nearest",
                supersample=1)
    base.update(kw)
    src = base["src"]
    return pj._Call(custom_src=src.kind not in nat.LENSLESS_KINDS and src.lens == nat.LENS_CUSTOM, **base)


def test_the_decision_function_names_the_routes_of_the_design_table():
    """``_route`` alone, no stand-in: the rows of DESIGN 3.12, their fallbacks, the plan's eagerness, the folded rotations, the errors."""
    grey16 = dict(tail=(), dt=np.dtype(np.uint16), bpp=2)
    double = nat.make_proj(nat.KIND_DOUBLE, 6, 12, nat.LENS_IDS["equidistant"], 3.3, 3.0, 2.0)
    custom = nat.make_proj(nat.KIND_CAMERA, 6, 6, nat.LENS_CUSTOM, 3.0, 3.0, 2.0)
    nine = tuple(np.roll(np.eye(3), k % 3, axis=0) for k in range(9))
    for facts, name, fallback, eager, device_out in (
        (_facts(), "HOST_RGB8", None, False, False),
        (_facts(interpolation="bilinear", supersample=2, map_shape=(8, 16, 3)), "HOST_RGB8", None, True, False),
        (_facts(**grey16), "HOST_PX", "PLAN_GATHER", False, False),
        (_facts(on_device=True), "DEV_RGB8", None, False, True),
        (_facts(on_device=True, interpolation="catmull-rom"), "DEV_RGB8", None, True, True),
        (_facts(on_device=True, **grey16), "DEV_PX", "PLAN_GATHER", False, True),
        (_facts(on_device=True, tail=(1, 3)), "DEV_PX", "PLAN_GATHER", False, True),
        (_facts(tail=(5,), bpp=5), "PLAN_GATHER", None, False, False),
        (_facts(src=double, width=12, **grey16), "PLAN_GATHER", None, False, False),
        (_facts(map_kind="ndarray"), "MAP_RGB8", None, False, False),
        (_facts(map_kind="coordmap", **grey16), "MAP_GATHER", None, False, False),
        (_facts(src=custom), "MAP_GATHER", None, False, False),
        (_facts(rotations=nine), "MAP_RGB8", None, False, False),
        (_facts(map_kind="device", interpolation="bilinear"), "MAP_INTERP", None, False, False),
        (_facts(interpolation="bilinear", **grey16), "MAP_INTERP", None, False, False),
        (_facts(on_device=True, supersample=2, map_shape=(8, 16, 3)), "SS_FUSED", None, False, True),
        (_facts(supersample=2, map_shape=(8, 16, 3), **grey16), "SS_GENERIC", None, False, False),
    ):
        r = pj._route(facts)
        assert (r.name, r.fallback, r.eager, r.device_out) == (name, fallback, eager, device_out), (facts, r)
        assert len(r.rotations) == len(facts.rotations)
    # the supersampled generic route is the n = 1 route with its result on the device, then the box filter
    r = pj._route(_facts(supersample=2, map_shape=(8, 16, 3), **grey16))
    assert (r.inner.name, r.inner.fallback, r.inner.device_out) == ("DEV_PX", "PLAN_GATHER", True)
    # an interpolating call folds a chain longer than one plan takes into one matrix R_9 ... R_1; a nearest call keeps the reference's bits
    r = pj._route(_facts(rotations=nine, interpolation="bilinear"))
    folded = np.eye(3)
    for m in nine:
        folded = m @ folded
    assert r.name == "HOST_RGB8" and len(r.rotations) == 1 and np.array_equal(r.rotations[0], folded)
    r = pj._route(_facts(rotations=nine, interpolation="bilinear", supersample=2, map_shape=(8, 16, 3)))
    assert r.name == "SS_GENERIC" and r.inner.name == "DEV_RGB8" and len(r.inner.rotations) == 1
    # the argument errors, before any device work and in this order
    f32 = dict(dt=np.dtype(np.float32), bpp=12)
    with pytest.raises(NotImplementedError, match="supersampling takes 8- or 16-bit unsigned samples, got float32"):
        pj._route(_facts(supersample=2, map_shape=(7, 15, 3), interpolation="bilinear", **f32))
    with pytest.raises(ValueError, match=r"a \(7, 15\) coordinate map is not divisible by supersample=2"):
        pj._route(_facts(supersample=2, map_shape=(7, 15, 3), src=double, tail=(), bpp=1, interpolation="bilinear"))
    with pytest.raises(NotImplementedError, match="bilinear sampling takes 8- or 16-bit unsigned samples, got float32"):
        pj._route(_facts(interpolation="bilinear", src=double, tail=(), **{**f32, "bpp": 4}))
    with pytest.raises(ValueError, match=r"operands could not be broadcast together with shapes \(4,8\) \(4,8,1\)"):
        pj._route(_facts(interpolation="catmull-rom", src=double, width=12, tail=(), bpp=1))


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(encode(json.loads(json.dumps(record()))), f, separators=(",", ":"))
        f.write("\n")
