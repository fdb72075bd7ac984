"""NumPy frames <-> device: the host side of the drop-in's REAL path - the reference's contract is ndarray in, fresh
ndarray out (core/__init__.py:66-92), so for a user who just swaps imports a remap is upload + kernel + download.

What each direction costs and how it is kept down (measured on the MI355X box, c2 = 100.7 MB in, 50.3 MB out):
  download  the result ndarray IS page-locked memory from a recycling pool (``_device.PINNED``): the DMA writes it directly, no
            staging copy; the block returns to the pool when the caller drops the array.
  upload    memory the caller owns is pageable.  A frame-sized array (>= 32 MiB) is page-locked in place at its first sighting, a
            smaller one at its second (pb_host_register, tied to the owning object's lifetime: 0.2-0.35 ms for a c2 frame), and
            uploads with ONE DMA straight out of the caller's memory.  Anything else (views, small arrays seen once) is copied
            through page-locked staging buffers in 16 MiB chunks on a few threads, each chunk's DMA running while the next chunk
            is being copied.
  streams   (remap_frames) the two DMA directions do not run at full rate side by side on this box (1.77 ms up + 0.89 ms down take
            2.41 ms on two streams), but an upload DMA and a KERNEL that stores over PCIe do (2.06 ms): the remap kernel of frame k
            writes its output straight into the page-locked result ndarray while frame k + 1 uploads - no device output buffer,
            no download (experiments/r6/pcie_paths.py).
No PyTorch anywhere in this module.
"""

from __future__ import annotations

import threading
from collections import OrderedDict
from typing import Iterable, Iterator

import numpy as np

from . import _native as nat
from ._device import PINNED, REGISTERED, DeviceArray, Event, Stream
from .utils.hostcopy import par_copy

CHUNK = 16 << 20
_TLS = threading.local()


class HostPipe:
    """One thread's streams, staging buffers and cached device buffers on one device."""

    def __init__(self, device: int):
        self.device = device
        self.stream = Stream()
        self._stage = []  # [pinned uint8 ndarray, Event or None]
        self._dev = OrderedDict()  # (slot, nbytes) -> DeviceArray
        self._ring = {}  # nbytes -> idle DeviceArrays of remap_frames
        self._ws_idle = None  # the supersampled generic path's workspace between calls (at most one kept: the largest)
        self._k = 0

    # -- device buffers kept between calls (hipMalloc of a 100 MB frame costs about a millisecond) ------------------------
    def device_buffer(self, slot: str, nbytes: int) -> DeviceArray:
        key = (slot, nbytes)
        buf = self._dev.get(key)
        if buf is None:
            while len(self._dev) >= 8:
                self._dev.popitem(last=False)
            buf = self._dev[key] = DeviceArray((nbytes,), np.uint8)
        self._dev.move_to_end(key)
        return buf

    # -- the streaming pipeline's rotating input buffers: checked out for one remap_frames call, kept for the next (three hipMallocs and
    #    hipFrees of 100 MB were 1.5 ms of every call - a tenth of a millisecond per frame of a 16-frame batch)
    def take_ring(self, nbytes: int, count: int) -> list:
        idle = self._ring.setdefault(nbytes, [])
        out = [idle.pop() for _ in range(min(count, len(idle)))]
        while len(out) < count:
            out.append(DeviceArray((nbytes,), np.uint8))
        return out

    def give_ring(self, nbytes: int, bufs: list) -> None:
        idle = self._ring.setdefault(nbytes, [])
        idle.extend(bufs[: max(0, 4 - len(idle))])  # (at most four per size stay)
        for key in [k for k in self._ring if k != nbytes][1:]:  # (and two sizes)
            del self._ring[key]

    # -- the supersampled generic path's workspace (one n x frame): checked out for one call, like the ring, so that a streamed batch
    #    and a single frame of the same thread never share one; at most one idle buffer stays
    def take_workspace(self, nbytes: int):
        ws = self._ws_idle
        if not nbytes:
            return None
        if ws is not None and ws.nbytes >= nbytes:
            self._ws_idle = None
            return ws
        return DeviceArray((int(nbytes),), np.uint8)

    def give_workspace(self, ws) -> None:
        """Returns a workspace whose work has completed."""
        if ws is not None and (self._ws_idle is None or ws.nbytes > self._ws_idle.nbytes):
            self._ws_idle = ws

    def _staging(self):
        """The next page-locked staging chunk, free of its previous DMA."""
        if len(self._stage) < 3:
            ent = [PINNED.ndarray((CHUNK,), np.uint8), None]
            self._stage.append(ent)
        else:
            ent = self._stage[self._k % 3]
        self._k += 1
        if ent[1] is not None:
            ent[1].sync()
        return ent

    def upload(self, a: np.ndarray, dst: DeviceArray, stream: Stream | None = None) -> bool:
        """Queues the upload of `a`'s bytes into `dst` on `stream`.  Returns False when `a` has been read completely on return
        (staged copy), True when the DMA reads the caller's (page-locked) memory until the stream has passed this point."""
        st = stream or self.stream
        a = np.ascontiguousarray(a)
        flat = a.reshape(-1).view(np.uint8)
        n = flat.nbytes
        if n != dst.nbytes:
            raise ValueError(f"upload of {n} bytes into a device buffer of {dst.nbytes}")
        lib = nat.load()
        if REGISTERED.is_registered(a):
            nat.check(lib.pb_memcpy_h2d(dst.data_ptr(), flat.ctypes.data, n, st.handle))
            return True
        for off in range(0, n, CHUNK):
            m = min(CHUNK, n - off)
            ent = self._staging()
            par_copy(ent[0][:m], flat[off : off + m])
            nat.check(lib.pb_memcpy_h2d(dst.data_ptr() + off, ent[0].ctypes.data, m, st.handle))
            if ent[1] is None:
                ent[1] = Event()
            ent[1].record(st)
        return False

    def download(self, src: DeviceArray, shape, dtype, stream: Stream | None = None) -> np.ndarray:
        """Queues the download of `src` into a fresh page-locked ndarray on `stream`; valid once the stream has been synchronised."""
        st = stream or self.stream
        out = PINNED.ndarray(shape, dtype)
        nat.check(nat.load().pb_memcpy_d2h(out.ctypes.data, src.data_ptr(), out.nbytes, st.handle))
        return out


def pipe_for(device: int | None = None) -> HostPipe:
    dev = nat.current_device() if device is None else int(device)
    pipes = getattr(_TLS, "pipes", None)
    if pipes is None:
        pipes = _TLS.pipes = {}
    p = pipes.get(dev)
    if p is None:
        with nat.on_device(dev):
            p = pipes[dev] = HostPipe(dev)
    return p


def _out_shape(plan, supersample: int) -> tuple:
    """(H, W) of a result: the plan's destination, or its n x n block grid (Plan.out_shape) when supersampled."""
    if nat.check_supersample(supersample) == 1:
        return plan.dst.height, plan.dst.width
    return plan.out_shape(supersample)


def _ss_kw(supersample: int, ws=None) -> dict:
    """Plan.launch's supersample arguments - passed only when supersampling, so that n = 1 is exactly the plain launch."""
    return {} if supersample == 1 else {"supersample": supersample, "workspace": ws}


def _ss_bytes(plan, supersample: int, interpolation: str, src_ptr: int) -> int:
    return 0 if supersample == 1 else plan.supersample_workspace_bytes(supersample, interpolation, src_ptr=src_ptr)


def _px_format(plan, a: np.ndarray, interpolation: str, supersample: int) -> tuple:
    """(trailing shape, dtype, bytes per pixel) of a frame (h, w, *tail) for `plan`: uint8 (h, w, 3), or - nearest, not supersampled - any
    dtype and tail whose pixel is one of nat.PX_SIZES bytes (Plan.launch's bytes_per_px: pb_remap_px).  ValueError otherwise."""
    sh = (plan.src.height, plan.src.width)
    tail, dt = tuple(a.shape[2:]), a.dtype
    if a.ndim < 2 or tuple(a.shape[:2]) != sh:
        raise ValueError(f"frames must be {sh + (3,)} uint8 (or {sh} + trailing dimensions with pixels of {nat.PX_SIZES} bytes), got {dt} {tuple(a.shape)}")
    if dt == np.uint8 and tail == (3,):
        return tail, dt, 3
    bpp = nat.tail_bytes(tail, dt)
    if bpp not in nat.PX_SIZES or interpolation != "nearest" or supersample != 1:
        raise ValueError(f"frames must be uint8 {sh + (3,)} - or, for nearest sampling without supersampling, {sh} + trailing dimensions with "
                         f"pixels of {nat.PX_SIZES} bytes -, got {dt} {tuple(a.shape)}")
    return tail, dt, bpp


def _px_kw(bpp: int) -> dict:
    """Plan.launch's pixel size - passed only when it is not the uint8 RGB call."""
    return {} if bpp == 3 else {"bytes_per_px": bpp}


VIDEO_FORMATS = {name: dt for name, (dt, fam, _) in nat.VIDEO_FORMATS.items() if fam.pairs}  # 4:2:0 semi-planar frames (3h/2, w): Plan.launch_nv12


def check_video_call(pixel_format: str, interpolation: str, supersample: int, track=None) -> np.dtype:
    """The sample type of a video pixel format, for a call it can be part of: nearest, not supersampled, no rotation track (pb_remap_nv12).
    ValueError otherwise.  THE place that says so: ``_video_format`` and ``batch.remap_frames`` (before its first frame) ask here."""
    if pixel_format not in nat.VIDEO_FORMATS:
        raise ValueError(f"pixel_format must be None or one of {sorted(VIDEO_FORMATS) + sorted(nat.PLANAR_FORMATS)}, got {pixel_format!r}")
    if interpolation != "nearest" or supersample != 1 or track is not None:
        raise ValueError(f"{pixel_format} frames take nearest sampling without supersampling or a rotation track")
    return nat.VIDEO_FORMATS[pixel_format][0]


def _video_format(plan, a: np.ndarray, pixel_format: str, interpolation: str, supersample: int, track=None) -> tuple:
    """(result shape, dtype, bytes per sample) of a packed video frame for `plan`: (3h/2, w) for the semi-planar formats; a flat array of the
    three planes' samples - at 4:4:4 also (3, h, w) - for the planar ones.  The keyword is needed: such an array is indistinguishable from a
    grey image.  ValueError otherwise."""
    dt = check_video_call(pixel_format, interpolation, supersample, track)
    fam = nat.VIDEO_FORMATS[pixel_format][1]
    h, w, H, W = plan.src.height, plan.src.width, plan.dst.height, plan.dst.width
    if not nat.planar_dims_ok(fam.sub, (h, w), (H, W)):
        rule = f"{pixel_format} frames need even dimensions" if fam.pairs else nat.planar_dims_rule(fam.sub, pixel_format)
        raise ValueError(f"{rule}, the plan maps {h} x {w} to {H} x {W}")
    frames = fam.packed(h, w)
    if a.dtype != dt or tuple(a.shape) not in frames:
        raise ValueError(f"{pixel_format} frames must be {dt} {' or '.join(map(str, frames))}, got {a.dtype} {tuple(a.shape)}")
    return fam.packed(H, W)[frames.index(tuple(a.shape))], dt, dt.itemsize


def _launch_video(plan, pixel_format: str, src_ptr: int, dst_ptr: int, stream: int, bps: int) -> None:
    """One packed video frame: pb_remap_nv12 for the semi-planar formats, pb_remap_planar with the format's black for the planar ones."""
    _, fam, fill = nat.VIDEO_FORMATS[pixel_format]
    if fam.pairs:
        plan.launch_nv12(src_ptr, dst_ptr, 1, stream, bps)
    else:
        plan.launch_planar(src_ptr, dst_ptr, fam.sub, 1, stream, bps, fill)


def remap_ndarray(plan: nat.Plan, image: np.ndarray, interpolation: str = "nearest", device: int | None = None, supersample: int = 1,
                  pixel_format: str | None = None) -> np.ndarray:
    """One frame: uint8 (h, w, 3) ndarray -> fresh uint8 (H, W, 3) ndarray (upload, ONE kernel launch, download).  ``supersample`` n: `plan`
    is the n x destination's and the result (H / n, W / n, 3) holds the n x n block means (``Plan.launch``).  ``interpolation``: "nearest",
    "bilinear" or "catmull-rom" (not supersampled).  Nearest without supersampling also takes (h, w, *tail) frames of any dtype whose
    pixel is 1, 2, 4, 6 or 8 bytes - grey, RGBA, 16-bit samples - and returns (H, W, *tail) of that dtype (pb_remap_px: a plan
    ``Plan.px_supported`` refuses is a PbError).  ``pixel_format`` "nv12" (uint8) or "p010" (uint16): the frame is a 4:2:0 semi-planar
    video frame (3h/2, w) and the result (3H/2, W) (pb_remap_nv12, DESIGN 3.15: a plan ``Plan.nv12_supported`` refuses is a PbError).
    ``pixel_format`` one of ``nat.PLANAR_FORMATS`` - ffmpeg's "yuv420p", "yuv422p", "yuv444p", their "10le" / "16le" forms, "gbrp",
    "gbrp16le": the frame is a planar frame, a flat array of its three planes' samples (``utils.planar_planes``; 4:4:4 also (3, h, w)),
    and the result one of the destination's, black pixels the format's black (pb_remap_planar)."""
    nat.check_interpolation(interpolation, supersample)
    if pixel_format is None:
        oh, ow = _out_shape(plan, supersample)
        tail, dt, bpp = _px_format(plan, image, interpolation, supersample)
        oshape, out_bytes = (oh, ow) + tail, bpp * oh * ow
    else:
        oshape, dt, bpp = _video_format(plan, image, pixel_format, interpolation, supersample)  # (bpp: bytes per sample)
        out_bytes = bpp * int(np.prod(oshape))
    nat.require_gpu()
    pipe = pipe_for(device)
    with nat.on_device(pipe.device):
        d_in = pipe.device_buffer("in", image.nbytes)
        d_out = pipe.device_buffer("out", out_bytes)
        ws = pipe.take_workspace(_ss_bytes(plan, supersample, interpolation, d_in.data_ptr()))
        pipe.upload(image, d_in)
        if pixel_format is None:
            plan.launch(d_in.data_ptr(), d_out.data_ptr(), 1, pipe.stream.handle, interpolation, **_ss_kw(supersample, ws), **_px_kw(bpp))
        else:
            _launch_video(plan, pixel_format, d_in.data_ptr(), d_out.data_ptr(), pipe.stream.handle, bpp)
        out = pipe.download(d_out, oshape, dt)
        pipe.stream.sync()
        pipe.give_workspace(ws)
    return out


def remap_frames(plan: nat.Plan, frames: Iterable[np.ndarray], depth: int = 3, interpolation: str = "nearest",
                 supersample: int = 1, track=None, pixel_format: str | None = None) -> Iterator[np.ndarray]:
    """Streams host-resident frames through one plan: while frame k + 1 uploads on the H2D stream, the remap kernel of frame k stores its
    output over PCIe straight into frame k's result ndarray (page-locked, device-visible), through `depth` rotating device input
    buffers.  Yields uint8 (H, W, 3) ndarrays in order (page-locked, recycled when dropped).  ``supersample`` n: `plan` is the n x
    destination's, the results are (H / n, W / n, 3) block means - the fused kernel stores only those over PCIe.  Nearest without
    supersampling also takes frames (h, w, *tail) of any dtype whose pixel is 1, 2, 4, 6 or 8 bytes (``remap_ndarray``): all frames of a
    call share the first frame's format, and the results are (H, W, *tail) of that dtype.  ``track``: ``nat.rotation_table``'s result - a
    rotation per frame (uint8 RGB, not supersampled): the table is uploaded once before the first frame (a device array is used in place)
    and frame f is a one-frame ``Plan.launch_track`` that points at entry f; a frame beyond the table is a ValueError at that frame.
    ``pixel_format`` "nv12" / "p010": the frames are 4:2:0 semi-planar video frames (3h/2, w) of uint8 / uint16 and the results (3H/2, W)
    (``remap_ndarray``) - the same pipeline, page-locking and ring; a planar format of ``nat.PLANAR_FORMATS``: flat planar frames
    (``remap_ndarray``); None: everything above."""
    nat.check_interpolation(interpolation, supersample)
    if pixel_format is not None:
        check_video_call(pixel_format, interpolation, supersample, track)
    if track is not None and supersample != 1:
        raise ValueError("a rotation track is not supersampled: pass supersample=1")
    oh, ow = _out_shape(plan, supersample)
    nat.require_gpu()
    tab = n_tab = k_tab = None
    if track is not None:
        tab, n_tab, k_tab = track
        if isinstance(tab, np.ndarray):  # (synchronous, once: every launch below finds the whole table on the device)
            tab = DeviceArray(tab.shape, np.float64).copy_from_host(tab)
    depth = max(2, int(depth))
    dev = nat.current_device()
    pipe = pipe_for(dev)
    fmt = sh = dh = d_in = ws = None  # the call's pixel format, frame shapes, ring and workspace: known with the first frame
    n_in = bpp = 0
    s_up, s_run = Stream(), Stream()
    uploaded = [Event() for _ in range(depth)]
    computed = [Event() for _ in range(depth)]
    results = [None] * depth
    sources = [None] * depth  # a sequence's frames whose DMA may still be reading them
    pending: list = []  # slots whose kernel has been queued, oldest first

    def drain_one():
        slot = pending.pop(0)
        computed[slot].sync()  # (the kernel has completed: its stores into the host array are visible, the upload before it is through)
        out, results[slot], sources[slot] = results[slot], None, None
        return out

    ahead = frames if isinstance(frames, (list, tuple)) else None
    k = 0
    try:
        for frame in frames:
            a = np.asarray(frame)
            if fmt is None and pixel_format is not None:
                dh, dt, bpp = _video_format(plan, a, pixel_format, interpolation, supersample, track)  # (bpp: bytes per sample)
                fmt, sh = ((), dt, bpp), tuple(a.shape)
                n_in = a.nbytes
                d_in = pipe.take_ring(n_in, depth)
            elif fmt is None:
                tail, dt, bpp = fmt = _px_format(plan, a, interpolation, supersample)
                sh, dh = (plan.src.height, plan.src.width) + tail, (oh, ow) + tail
                n_in = a.nbytes
                d_in = pipe.take_ring(n_in, depth)
                ws = pipe.take_workspace(_ss_bytes(plan, supersample, interpolation, d_in[0].data_ptr()))  # (used in s_run's order, frame after frame)
            if a.dtype != fmt[1] or tuple(a.shape) != sh:
                raise ValueError(f"frames must be {fmt[1]} {sh}, got {a.dtype} {tuple(a.shape)}")
            slot = k % depth  # (free: the previous turn delivered its result, below)
            direct = pipe.upload(a, d_in[slot], s_up)
            uploaded[slot].record(s_up)
            s_run.wait(uploaded[slot])
            out = results[slot] = PINNED.ndarray(dh, fmt[1])
            if pixel_format is not None:
                _launch_video(plan, pixel_format, d_in[slot].data_ptr(), out.ctypes.data, s_run.handle, bpp)
            elif tab is None:
                plan.launch(d_in[slot].data_ptr(), out.ctypes.data, 1, s_run.handle, interpolation, **_ss_kw(supersample, ws), **_px_kw(bpp))
            else:
                if k >= n_tab:
                    raise ValueError(f"frame {k} has no rotation: the table holds {n_tab}")
                if bpp != 3:
                    raise ValueError(f"a rotation track takes uint8 {sh[:2] + (3,)} frames, got {a.dtype} {tuple(a.shape)}")
                plan.launch_track(tab.data_ptr() + k * k_tab * nat.TRACK_MATRIX_BYTES, k_tab, d_in[slot].data_ptr(), out.ctypes.data, 1, s_run.handle, interpolation)
            computed[slot].record(s_run)
            pending.append(slot)
            if direct and ahead is not None:
                # frames that already exist (a list, a tuple): nothing waits for this DMA - the next frame's is queued behind it at once;
                # the frame is held until its kernel has run.  The NEXT frame is page-locked meanwhile (0.2-0.35 ms off the critical path).
                sources[slot] = a
                if k + 1 < len(ahead) and isinstance(ahead[k + 1], np.ndarray):
                    REGISTERED.is_registered(ahead[k + 1])
            # everything that does not need the next frame happens HERE, while this frame's DMA runs: the oldest result is handed over (the
            # caller's turn with it included) and frees the slot the next frame takes.  What was left between the end of one upload and the
            # start of the next - the link idle - used to hold all of this: 0.15-0.2 ms of a 2.25 ms frame.
            if len(pending) == depth:
                yield drain_one()
            if direct and ahead is None:
                # an iterator may refill the buffer the DMA is reading as soon as it is asked for the next frame: the DMA must be through
                uploaded[slot].sync()
            k += 1
        while pending:
            yield drain_one()
    finally:
        # (a caller that stops early: nothing of the pipeline may still be reading its frames or writing the results it was not given)
        s_up.sync()
        s_run.sync()
        if d_in is not None:
            pipe.give_ring(n_in, d_in)
        pipe.give_workspace(ws)
