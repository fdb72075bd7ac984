"""The three photonbend commands on top of the GPU core - SURVEY 8 f-2 - and three of our own beside them: pano-to-cubemap,
cubemap-to-pano and cubemap-to-cubemap (the cube map is a (2N, 3N) image of six faces: left, front, right over up, back, down).

Same command names, options and rules as the reference CLI (photonbend/scripts/main.py:28-35,
commands/make_photo.py:52-141, alter_photo.py:51-162, make_pano.py:54-149, commands/__init__.py:53-191):
image type -> class and magnitude, output size, fov validation, any number of ``-r pitch yaw roll``
applied in order, the .jpg/.jpeg/.png suffix rule and the overwrite prompt.  Everything here is host
plumbing (Pillow decode/encode dominates its wall time); the remap is one pb_remap_u8 call.
"""

from __future__ import annotations

import math
import sys
from pathlib import Path
from typing import Optional, Sequence, Tuple

import click
import numpy as np
from PIL import Image

from .. import core
from .. import _native as nat
from ..core.lens import equidistant, equisolid, orthographic, polynomial, rectilinear, stereographic
from ..core.projection import CameraImage, CubemapImage, DoubleCameraImage, PanoramaImage
from ..core.rotation import Rotation
from ..utils import to_radians

LENSES = {
    "equidistant": equidistant,
    "equisolid": equisolid,
    "orthographic": orthographic,
    "rectilinear": rectilinear,
    "stereographic": stereographic,
}
POLYNOMIAL = "polynomial"  # a --lens choice with parameters (lens_object)
TYPES = ("inscribed", "double", "cropped", "full")
INTERPOLATIONS = nat.INTERPOLATIONS

TYPE_HELP = """

    \b
    The choices are:
    - inscribed: The valid data is on a inscribed circle.
    - double: The valid data is on two inscribed side-by-side circles.
    - cropped: The valid data is on a inscribed circle, top-and-bottom cropped.
    - full: The whole area of the image is valid data.
    """
DOUBLE_FOV_NOTE = "\n\n    IMPORTANT: FoV for double images are the value for one of the sensors and > 180."
ROTATION_HELP = "The rotation that should be applied to the camera: <pitch yaw roll> in degrees. Repeatable."


# ---- rules ------------------------------------------------------------------------------------
def checked_output(path: Path) -> Path:
    """Suffix rule and overwrite prompt (commands/__init__.py:53-70)."""
    out = Path(path)
    if out.suffix.lower() not in (".jpg", ".jpeg", ".png"):
        print("The desired output image should be a JPG or PNG file.")
        print("Provide an output filename ending in either JPG, JPEG or PNG (case insensitive)")
        print("Exiting!")
        sys.exit(1)
    if out.exists():
        answer = ""
        while answer not in ("y", "n"):
            answer = input("File already exists. Overwrite? (y/n) ")
        if answer == "n":
            print("Exiting!")
            sys.exit(0)
    return out


def open_image(path: Path) -> np.ndarray:
    """The decoded pixels exactly as Pillow hands them over (commands/__init__.py:135-143): RGB, RGBA, grey
    ("L" -> (H, W)), 16-bit - nothing is converted, the remap gathers whatever the array holds, like the reference."""
    try:
        with Image.open(path) as im:
            return np.asarray(im)
    except IOError:
        print("Error: Input image could not be opened!")
        print("Exiting!")
        sys.exit(1)


def magnitude_for(image_type: str, shape: Sequence[int]) -> float:
    """Pixels from the centre to where the full fov is reached (commands/__init__.py:91-109)."""
    if len(shape) > 3:
        raise ValueError("Can't calculate magnitude of images with more than 3 dimensions")
    height, width, _ = shape  # like the reference (:96): a grey (H, W) array does not unpack - ValueError
    if image_type == "double":
        return height / 2 - 0.5
    if image_type == "full":
        return math.sqrt((width / 2.0 - 0.5) ** 2 + (height / 2.0 - 0.5) ** 2)
    return width / 2 - 0.5  # inscribed, cropped


def radians_fov(fov: float, image_type: str) -> float:
    """fov rules (commands/__init__.py:171-177)."""
    if image_type == "double" and fov < 180:
        raise ValueError("The fov of a double image can't be smaller than 180 degrees.")
    if fov > 360:
        raise ValueError("The fov of an image can't be higher than 360 degrees.")
    return to_radians(fov)


def camera_shape(image_type: str, source: np.ndarray, height: Optional[int]) -> Tuple[int, int, int]:
    """Shape of a fisheye destination (commands/__init__.py:180-191)."""
    h = source.shape[0] if height is None else height
    return (h, 2 * h, 3) if image_type == "double" else (h, h, 3)


def lens_object(lens: str, coefficients=None, max_theta=None, prefix: str = "--lens"):
    """The Lens of a --lens choice.  ``polynomial`` (no reference counterpart: a calibrated Kannala-Brandt lens, core.lens.polynomial)
    takes its K1 K2 K3 K4 from ``<prefix>-coefficients`` and the end of its domain, in degrees, from ``<prefix>-max-theta``; either
    option without ``polynomial``, and ``polynomial`` without coefficients, are usage errors."""
    coefficients = tuple(coefficients) if coefficients else None
    if lens != POLYNOMIAL:
        if coefficients is not None or max_theta is not None:
            raise click.UsageError(f"{prefix}-coefficients / {prefix}-max-theta belong to `{prefix} {POLYNOMIAL}`, not to `{prefix} {lens}`")
        return LENSES[lens]()
    if coefficients is None:
        raise click.UsageError(f"`{prefix} {POLYNOMIAL}` needs {prefix}-coefficients K1 K2 K3 K4")
    try:
        return polynomial(*coefficients, max_theta=None if max_theta is None else to_radians(max_theta))
    except ValueError as exc:
        raise click.BadParameter(str(exc), param_hint=f"{prefix}-coefficients")


def camera_object(image_type: str, pixels: np.ndarray, fov: float, lens, magnitude: float):
    """CameraImage or DoubleCameraImage for the type (commands/__init__.py:84-88); ``lens``: a built-in's name or a Lens."""
    cls = DoubleCameraImage if image_type == "double" else CameraImage
    return cls(pixels, fov, LENSES[lens]() if isinstance(lens, str) else lens, magnitude=magnitude)


def run_chain(source, destiny, rotations, out: Path, supersample: int = 1, interpolation: str = "nearest") -> None:
    """dst.get_coordinate_map() -> rotations in order -> src.process_coordinate_map() -> save.  ``supersample`` n > 1: the map of the n x
    destination, each output pixel the mean of its n x n samples (the output size stays what the size rules gave).  ``interpolation``:
    the sampler - "nearest" (the reference's), or the opt-in "bilinear" / "catmull-rom" (the latter not supersampled)."""
    try:
        nat.check_interpolation(interpolation, supersample)
    except ValueError as exc:
        raise click.BadParameter(str(exc), param_hint="--interpolation")
    if supersample == 1:
        cmap = destiny.get_coordinate_map()
    else:
        try:
            cmap = destiny.get_coordinate_map(supersample=supersample)
        except ValueError as exc:
            raise click.BadParameter(str(exc), param_hint="--supersample")
    for rot in rotations:
        cmap = Rotation(*map(to_radians, rot)).rotate_coordinate_map(cmap)
    mapped = source.process_coordinate_map(cmap) if interpolation == "nearest" else source.process_coordinate_map(cmap, interpolation=interpolation)
    try:
        Image.fromarray(np.ascontiguousarray(mapped)).save(out)
    except IOError:
        print("Could not save to the specified location!")
        print("Exiting!")
        sys.exit(1)


def _sampler(interpolation: str) -> dict:
    """run_chain's keyword for --interpolation: none at the default, so that a plain call is exactly what it was."""
    return {} if interpolation == "nearest" else {"interpolation": interpolation}


# ---- commands -----------------------------------------------------------------------------------
_lens_choice = click.Choice(list(LENSES) + [POLYNOMIAL])


def _lens_parameters(prefix: str, dest: str):
    """``<prefix>-coefficients K1 K2 K3 K4`` and ``<prefix>-max-theta DEGREES`` of a polynomial lens choice."""

    def deco(fn):
        fn = click.option(f"{prefix}-coefficients", f"{dest}_coefficients", type=click.FLOAT, nargs=4, default=None, metavar="K1 K2 K3 K4",
                          help=f"With `{prefix} polynomial`: r(theta) = theta + K1 theta^3 + K2 theta^5 + K3 theta^7 + K4 theta^9 "
                               "(a fisheye calibration's k1..k4, r in focal lengths).")(fn)
        fn = click.option(f"{prefix}-max-theta", f"{dest}_max_theta", type=click.FLOAT, default=None, metavar="DEGREES",
                          help=f"With `{prefix} polynomial`: the largest incidence angle the lens images, in degrees (default 180).")(fn)
        return fn

    return deco


_type_choice = click.Choice(list(TYPES))


def _common(fn):
    fn = click.option("-s", "--size", type=click.INT, default=None, help="The vertical size of the destiny image")(fn)
    fn = click.option("-r", "--rotation", type=click.FLOAT, nargs=3, multiple=True, default=[], help=ROTATION_HELP)(fn)
    fn = click.option("--supersample", type=click.Choice(["1", "2", "4"]), default="1", show_default=True,
                      help="Antialiasing: each output pixel is the mean of n x n samples (1 = off).")(fn)
    fn = click.option("--interpolation", type=click.Choice(list(INTERPOLATIONS)), default="nearest", show_default=True,
                      help="The sampler: nearest (the reference's), bilinear or catmull-rom (sharp when magnifying; not with --supersample).")(fn)
    return fn


@click.group()
def main():
    """photonbend commands on the MI355X remapper."""


@main.command("make-photo")
@click.argument("input_image", type=click.Path(exists=True, path_type=Path))
@click.option("--type", "otype", required=True, type=_type_choice, help="The type of the output image. " + TYPE_HELP)
@click.option("--lens", required=True, type=_lens_choice, help="The lens type to be used on the output photo.")
@_lens_parameters("--lens", "lens")
@click.option("--fov", required=True, type=click.FLOAT, help="The lens field of view of the output photo in degrees. " + DOUBLE_FOV_NOTE)
@_common
@click.argument("output_image", type=click.Path(exists=False, path_type=Path))
def make_photo(input_image, otype, lens, fov, output_image, rotation, size, supersample, interpolation, lens_coefficients, lens_max_theta):
    """Make a photo out of a panorama.

    \b
    INPUT is the path to the source panorama.
    OUTPUT is the desired path of the destiny photo.
    """
    lens = lens_object(lens, lens_coefficients, lens_max_theta)
    out = checked_output(output_image)
    pano = open_image(input_image)
    _, _, _ = pano.shape  # make_photo.py:112 unpacks three dimensions: grey inputs are a ValueError in the reference CLI
    shape = camera_shape(otype, pano, size)
    destiny = camera_object(otype, np.zeros(shape, np.uint8), radians_fov(fov, otype), lens, magnitude_for(otype, shape))
    run_chain(PanoramaImage(pano), destiny, rotation, out, int(supersample), **_sampler(interpolation))


@main.command("alter-photo")
@click.argument("input_image", type=click.Path(exists=True, path_type=Path))
@click.option("--itype", required=True, type=_type_choice, help="The type of the input image. " + TYPE_HELP)
@click.option("--ilens", required=True, type=_lens_choice, help="The lens type that was used on the input photo.")
@_lens_parameters("--ilens", "ilens")
@click.option("--ifov", required=True, type=click.FLOAT, help="The lens field of view of the input photo in degrees. " + DOUBLE_FOV_NOTE)
@click.option("--otype", required=True, type=_type_choice, help="The type of the output image." + TYPE_HELP)
@click.option("--olens", required=True, type=_lens_choice, help="The lens type of the output photo. " + DOUBLE_FOV_NOTE)
@_lens_parameters("--olens", "olens")
@click.option("--ofov", required=True, type=click.FLOAT, help="The lens field of view of the output photo in degrees.")
@click.argument("output_image", type=click.Path(exists=False, path_type=Path))
@_common
def alter_photo(input_image, itype, ilens, ifov, otype, olens, ofov, output_image, rotation, size, supersample, interpolation,
                ilens_coefficients, ilens_max_theta, olens_coefficients, olens_max_theta):
    """Change the the lens and FoV of a photo.

    \b
    INPUT is the path to the source photo.
    OUTPUT is the desired path of the destiny photo.
    """
    ilens = lens_object(ilens, ilens_coefficients, ilens_max_theta, "--ilens")
    olens = lens_object(olens, olens_coefficients, olens_max_theta, "--olens")
    out = checked_output(output_image)
    photo = open_image(input_image)
    source = camera_object(itype, photo, radians_fov(ifov, itype), ilens, magnitude_for(itype, photo.shape))
    shape = camera_shape(otype, photo, size)
    # the destination magnitude comes from the SOURCE shape (alter_photo.py:142): only visible when --size differs
    destiny = camera_object(otype, np.zeros(shape, np.uint8), radians_fov(ofov, otype), olens, magnitude_for(otype, photo.shape))
    run_chain(source, destiny, rotation, out, int(supersample), **_sampler(interpolation))


@main.command("make-pano")
@click.argument("input_image", type=click.Path(exists=True, path_type=Path))
@click.option("--type", "itype", required=True, type=_type_choice, help="The type of the input image. " + TYPE_HELP)
@click.option("--lens", required=True, type=_lens_choice, help="The lens type that was used on the input photo.")
@_lens_parameters("--lens", "lens")
@click.option("--fov", required=True, type=click.FLOAT, help="The lens field of view of the input photo in degrees. " + DOUBLE_FOV_NOTE)
@_common
@click.argument("output_image", type=click.Path(exists=False, path_type=Path))
def make_pano(input_image, itype, lens, fov, output_image, rotation, size, supersample, interpolation, lens_coefficients, lens_max_theta):
    """Make a panorama out of a photo.

    \b
    INPUT is the path to the source photo.
    OUTPUT is the desired path of the destiny panorama.
    """
    lens = lens_object(lens, lens_coefficients, lens_max_theta)
    out = checked_output(output_image)
    photo = open_image(input_image)
    source = camera_object(itype, photo, radians_fov(fov, itype), lens, magnitude_for(itype, photo.shape))
    h = photo.shape[0] if size is None else size
    destiny = PanoramaImage(np.zeros((h, int(h * 2), 3), np.uint8))  # make_pano.py:142-149
    run_chain(source, destiny, rotation, out, int(supersample), **_sampler(interpolation))


def _cubemap_common(fn):
    """-r, --interpolation and --supersample of the two cube map commands: the existing options under the existing rules."""
    fn = click.option("-r", "--rotation", type=click.FLOAT, nargs=3, multiple=True, default=[], help=ROTATION_HELP)(fn)
    fn = click.option("--supersample", type=click.Choice(["1", "2", "4"]), default="1", show_default=True,
                      help="Antialiasing: each output pixel is the mean of n x n samples (1 = off).")(fn)
    fn = click.option("--interpolation", type=click.Choice(list(INTERPOLATIONS)), default="nearest", show_default=True,
                      help="The sampler: nearest, bilinear or catmull-rom (sharp when magnifying; not with --supersample).  From a cube map "
                           "the interpolating samplers stay on one face: seams are not filtered, and the half texel along each face's top and "
                           "left edge comes out black (thin dark seam lines; nearest has none).")(fn)
    return fn


MAPPINGS = tuple(CubemapImage.MAPPINGS)
MAPPING_HELP = ("How a face is laid out: gnomonic (the plain cube map: position proportional to the tangent of the angle from the face centre) or "
                "equiangular (the equi-angular cube map of 360-degree video: position proportional to the angle itself).")


def _mapping_option(*names):
    return click.option(*names, type=click.Choice(list(MAPPINGS)), default="gnomonic", show_default=True, help=MAPPING_HELP)


@main.command("pano-to-cubemap")
@click.argument("input_image", type=click.Path(exists=True, path_type=Path))
@click.option("--face-size", type=click.INT, default=None, help="The side N of a face in pixels; the output is 3N wide and 2N high. [default: input height // 2]")
@_mapping_option("--mapping")
@_cubemap_common
@click.argument("output_image", type=click.Path(exists=False, path_type=Path))
def pano_to_cubemap(input_image, face_size, output_image, rotation, supersample, interpolation, mapping):
    """Make a cube map out of a panorama.

    \b
    INPUT is the path to the source panorama.
    OUTPUT is the desired path of the cube map: six faces in a 3 x 2 grid, left, front, right over up, back, down.
    """
    out = checked_output(output_image)
    pano = open_image(input_image)
    n = pano.shape[0] // 2 if face_size is None else face_size
    if n < 1:
        raise click.BadParameter("a face needs at least one pixel", param_hint="--face-size")
    destiny = CubemapImage(np.zeros((2 * n, 3 * n, 3), np.uint8), mapping=mapping)
    run_chain(PanoramaImage(pano), destiny, rotation, out, int(supersample), **_sampler(interpolation))


@main.command("cubemap-to-pano")
@click.argument("input_image", type=click.Path(exists=True, path_type=Path))
@click.option("--height", type=click.INT, default=None, help="The vertical size of the panorama (its width is twice that). [default: 2 x the face size]")
@_mapping_option("--mapping")
@_cubemap_common
@click.argument("output_image", type=click.Path(exists=False, path_type=Path))
def cubemap_to_pano(input_image, height, output_image, rotation, supersample, interpolation, mapping):
    """Make a panorama out of a cube map.

    \b
    INPUT is the path to the source cube map: a 3N x 2N image of six faces, left, front, right over up, back, down.
    OUTPUT is the desired path of the destiny panorama.
    """
    out = checked_output(output_image)
    cube = open_image(input_image)
    try:
        source = CubemapImage(cube, mapping=mapping)
    except ValueError as exc:
        raise click.UsageError(f"{input_image}: {exc}")
    h = 2 * source.face_size if height is None else height
    if h < 1:
        raise click.BadParameter("a panorama needs at least one row", param_hint="--height")
    destiny = PanoramaImage(np.zeros((h, 2 * h, 3), np.uint8))
    run_chain(source, destiny, rotation, out, int(supersample), **_sampler(interpolation))


@main.command("cubemap-to-cubemap")
@click.argument("input_image", type=click.Path(exists=True, path_type=Path))
@_mapping_option("--input-mapping")
@_mapping_option("--output-mapping")
@click.option("--face-size", type=click.INT, default=None, help="The side N of an output face in pixels. [default: the input's face size]")
@_cubemap_common
@click.argument("output_image", type=click.Path(exists=False, path_type=Path))
def cubemap_to_cubemap(input_image, input_mapping, output_mapping, face_size, output_image, rotation, supersample, interpolation):
    """Convert a cube map between the gnomonic and the equi-angular mapping, resize it or re-orient it.

    \b
    INPUT is the path to the source cube map: a 3N x 2N image of six faces, left, front, right over up, back, down.
    OUTPUT is the desired path of the destiny cube map, in the same arrangement.
    """
    out = checked_output(output_image)
    cube = open_image(input_image)
    try:
        source = CubemapImage(cube, mapping=input_mapping)
    except ValueError as exc:
        raise click.UsageError(f"{input_image}: {exc}")
    n = source.face_size if face_size is None else face_size
    if n < 1:
        raise click.BadParameter("a face needs at least one pixel", param_hint="--face-size")
    destiny = CubemapImage(np.zeros((2 * n, 3 * n, 3), np.uint8), mapping=output_mapping)
    run_chain(source, destiny, rotation, out, int(supersample), **_sampler(interpolation))


# ---- raw video frames ---------------------------------------------------------------------------
PIX_FMTS = {name: dt.type for name, (dt, fam, _) in nat.VIDEO_FORMATS.items() if fam.pairs}  # ffmpeg's -pix_fmt names of the two 4:2:0 semi-planar layouts
TRACK_FRAMES = 4  # PB_TRACK_FRAMES (csrc/pb_kernels_track.hpp): --chunk is a multiple of it


def _fail(message: str):
    """A usage error of remap-nv12: the message on stderr (stdout may be the frame pipe), exit status 1."""
    click.echo(f"Error: {message}", err=True)
    sys.exit(1)


def _read_track(path: Path) -> np.ndarray:
    """A rotation track file: one `pitch yaw roll` line in degrees per frame (blank lines and # comments skipped) -> radians (N, 3)."""
    rows = []
    for n, line in enumerate(Path(path).read_text().splitlines(), 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        try:
            vals = [float(v) for v in line.split()]
        except ValueError:
            vals = []
        if len(vals) != 3:
            _fail(f"{path}:{n}: a rotation track line holds three numbers: pitch yaw roll in degrees")
        rows.append([to_radians(v) for v in vals])
    return np.array(rows, np.float64).reshape(-1, 3)


def _read_exact(stream, nbytes: int) -> bytes:
    """Up to nbytes from a file or a pipe: short only at the end of the input."""
    parts, got = [], 0
    while got < nbytes:
        b = stream.read(nbytes - got)
        if not b:
            break
        parts.append(b)
        got += len(b)
    return b"".join(parts)


def _video_chain(width, height, otype, lens, fov, size, rotation, lens_coefficients, lens_max_theta):
    """The coordinate map of a raw-video command (remap-nv12, remap-yuv): by default a panorama of the input's size (--size H: H x 2H), with
    --type, --lens and --fov the photo make-photo would make; every -r applied in order."""
    if otype is None:
        if lens is not None or fov is not None or lens_coefficients or lens_max_theta is not None:
            raise click.UsageError("--lens / --fov and the lens parameters belong to a photo: give --type too")
        h_out = height if size is None else size
        destiny = PanoramaImage(np.zeros((h_out, width if size is None else 2 * h_out, 3), np.uint8))
    else:
        if lens is None or fov is None:
            raise click.UsageError("a photo needs --type, --lens and --fov")
        shape = camera_shape(otype, np.zeros((height, width, 3), np.uint8), size)
        destiny = camera_object(otype, np.zeros(shape, np.uint8), radians_fov(fov, otype), lens_object(lens, lens_coefficients, lens_max_theta), magnitude_for(otype, shape))
    cmap = destiny.get_coordinate_map()
    for rot in rotation:
        cmap = Rotation(*map(to_radians, rot)).rotate_coordinate_map(cmap)
    return cmap


def _video_sampler(interpolation: str, track) -> bool:
    """--interpolation of a raw-video command -> whether the plan carries the bilinear mode's tables.  With a rotation track it is a usage
    error, raised before any input is read: the track kernels sample nearest."""
    if interpolation != "nearest" and track is not None:
        _fail(f"--interpolation {interpolation} does not go with --rotations: a rotation track is sampled nearest")
    return interpolation == "bilinear"


def _stream_frames(input_frames, output_frames, frame_in: int, dt, chunk: int, mats, remap) -> None:
    """The frame loop of a raw-video command: `chunk` packed frames of frame_in bytes at a time from a file or stdin through
    remap(host (n, samples of a frame), index of the first frame) -> device frames, written to a file or stdout.  A truncated frame and a
    rotation track (`mats`, or None) shorter than the input are usage errors - for a file, before anything is written."""
    piped = str(input_frames) == "-"
    if not piped:  # a file's length is known: refuse before anything is written
        if not input_frames.is_file():
            _fail(f"{input_frames}: no such file")
        total = input_frames.stat().st_size
        if total % frame_in:
            _fail(f"{input_frames}: {total} bytes are {total // frame_in} frames of {frame_in} bytes and a truncated one of {total % frame_in}")
        if mats is not None and total // frame_in > len(mats):
            _fail(f"{input_frames} holds {total // frame_in} frames, the rotation track {len(mats)} lines")
    fin = sys.stdin.buffer if piped else open(input_frames, "rb")
    fout = sys.stdout.buffer if str(output_frames) == "-" else open(output_frames, "wb")
    done = 0
    try:
        while True:
            data = _read_exact(fin, chunk * frame_in)
            n, rest = divmod(len(data), frame_in)
            if mats is not None and done + n + (1 if rest else 0) > len(mats):
                _fail(f"the input holds more than {len(mats)} frames, the rotation track {len(mats)} lines")
            if n:
                host = np.frombuffer(data, dt, n * frame_in // dt.itemsize).reshape(n, frame_in // dt.itemsize)
                fout.write(nat.to_host(remap(host, done)).tobytes())
                done += n
            if rest:
                _fail(f"the input ends with a truncated frame: {rest} of {frame_in} bytes after {done} whole frames")
            if len(data) < chunk * frame_in:
                break
        fout.flush()
    finally:
        if fin is not sys.stdin.buffer:
            fin.close()
        if fout is not sys.stdout.buffer:
            fout.close()


def _remap_video(pix_fmt, input_frames, output_frames, width, height, otype, lens, fov, size, rotation, track, chunk, interpolation, lens_coefficients, lens_max_theta):
    """The body of remap-nv12 and remap-yuv: frames of the pixel format `pix_fmt` (``nat.VIDEO_FORMATS``)."""
    bilinear = _video_sampler(interpolation, track)
    dt, fam, fill = nat.VIDEO_FORMATS[pix_fmt]
    rule, least = ("4:2:0 frames have even dimensions", 2) if fam.pairs else (nat.planar_dims_rule(fam.sub, pix_fmt), 1)
    if width < least or height < least or not nat.planar_dims_ok(fam.sub, (height, width)):
        _fail(f"{rule}, got --width {width} --height {height}")
    if size is not None and (size < least or not nat.planar_dims_ok(fam.sub, (size, 2))):
        _fail(f"{rule}, got --size {size}")
    if chunk < TRACK_FRAMES or chunk % TRACK_FRAMES:
        _fail(f"--chunk is a multiple of {TRACK_FRAMES}, got {chunk}")
    cmap = _video_chain(width, height, otype, lens, fov, size, rotation, lens_coefficients, lens_max_theta)
    dstp, srcp = cmap.dst_proj, PanoramaImage(np.zeros((height, width, 3), np.uint8))._proj("src")
    if dstp.width & 1 if fam.pairs else not nat.planar_dims_ok(fam.sub, (dstp.height, dstp.width)):  # (a semi-planar output's height is --size or the input's)
        _fail(f"{rule}: the output would be {dstp.height} x {dstp.width}")
    mats = None if track is None else core.rotation_track(_read_track(track))
    frame = fam.packed(height, width)[0]  # a packed frame as the plan's methods take it: (3h/2, w), or flat
    # without a track: a prepared plan and the tile kernel; with one: a deferred plan (its tables are never read) and the track kernel
    plan = None

    def remap(host, first):  # upload, ONE launch, download
        nonlocal plan
        if plan is None:  # (made with the first frames: the usage errors of the input come before any plan is prepared)
            plan = nat.Plan(dstp, list(cmap.rotations), srcp, bilinear=bilinear) if mats is None else nat.Plan(dstp, list(cmap.rotations), srcp, defer=True)
        s = nat.to_device(host.reshape((len(host),) + frame))
        if fam.pairs:
            return plan.remap_nv12(s, **_sampler(interpolation)) if mats is None else plan.remap_track_nv12(s, mats[first : first + len(host)])
        return plan.remap_planar(s, fam.sub, fill=fill, **_sampler(interpolation)) if mats is None else plan.remap_track_planar(s, mats[first : first + len(host)], fam.sub, fill=fill)

    _stream_frames(input_frames, output_frames, int(np.prod(frame)) * dt.itemsize, dt, chunk, mats, remap)


@main.command("remap-nv12")
@click.argument("input_frames", metavar="INPUT", type=click.Path(path_type=Path, allow_dash=True))
@click.argument("output_frames", metavar="OUTPUT", type=click.Path(path_type=Path, allow_dash=True))
@click.option("--width", required=True, type=click.INT, help="The width of an input frame in pixels (even).")
@click.option("--height", required=True, type=click.INT, help="The height of an input frame in pixels (even).")
@click.option("--pix-fmt", type=click.Choice(list(PIX_FMTS)), default="nv12", show_default=True, help="The frames' layout, as ffmpeg names it.")
@click.option("--type", "otype", type=click.Choice([t for t in TYPES if t != "double"]), default=None,
              help="Make a photo: the type of the output image (with --lens and --fov). " + TYPE_HELP)
@click.option("--lens", type=_lens_choice, default=None, help="With --type: the lens type of the output photo.")
@_lens_parameters("--lens", "lens")
@click.option("--fov", type=click.FLOAT, default=None, help="With --type: the lens field of view of the output photo in degrees.")
@click.option("-s", "--size", type=click.INT, default=None, help="The vertical size of an output frame (even). [default: the input's]")
@click.option("-r", "--rotation", type=click.FLOAT, nargs=3, multiple=True, default=[], help=ROTATION_HELP)
@click.option("--rotations", "track", type=click.Path(exists=True, dir_okay=False, path_type=Path), default=None,
              help="A rotation track: a text file of one `pitch yaw roll` line in degrees per frame, applied after every -r.")
@click.option("--chunk", type=click.INT, default=8, show_default=True, help=f"Frames per launch, a multiple of {TRACK_FRAMES}.")
@click.option("--interpolation", type=click.Choice(list(nat.VIDEO_INTERPOLATIONS)), default="nearest", show_default=True,
              help="The sampler: nearest (the reference's) or bilinear (chroma co-sited with its block's top-left pixel; not with --rotations).")
def remap_nv12(input_frames, output_frames, width, height, pix_fmt, otype, lens, fov, size, rotation, track, chunk, interpolation, lens_coefficients, lens_max_theta):
    """Remap raw NV12 / P010 video frames of an equirectangular panorama, e.g. between two `ffmpeg -f rawvideo -pix_fmt nv12` pipes.

    \b
    INPUT is a file of packed frames, HEIGHT x WIDTH each; - is stdin.
    OUTPUT receives the packed output frames; - is stdout.
    By default the output is a panorama of the same size (--size H: H x 2H); with --type, --lens and --fov it is the photo make-photo would make.
    """
    _remap_video(pix_fmt, input_frames, output_frames, width, height, otype, lens, fov, size, rotation, track, chunk, interpolation, lens_coefficients, lens_max_theta)


@main.command("remap-yuv")
@click.argument("input_frames", metavar="INPUT", type=click.Path(path_type=Path, allow_dash=True))
@click.argument("output_frames", metavar="OUTPUT", type=click.Path(path_type=Path, allow_dash=True))
@click.option("--width", required=True, type=click.INT, help="The width of an input frame in pixels.")
@click.option("--height", required=True, type=click.INT, help="The height of an input frame in pixels.")
@click.option("--pix-fmt", type=click.Choice(list(nat.PLANAR_FORMATS)), default="yuv420p", show_default=True, help="The frames' planar layout, as ffmpeg names it.")
@click.option("--type", "otype", type=click.Choice([t for t in TYPES if t != "double"]), default=None,
              help="Make a photo: the type of the output image (with --lens and --fov). " + TYPE_HELP)
@click.option("--lens", type=_lens_choice, default=None, help="With --type: the lens type of the output photo.")
@_lens_parameters("--lens", "lens")
@click.option("--fov", type=click.FLOAT, default=None, help="With --type: the lens field of view of the output photo in degrees.")
@click.option("-s", "--size", type=click.INT, default=None, help="The vertical size of an output frame. [default: the input's]")
@click.option("-r", "--rotation", type=click.FLOAT, nargs=3, multiple=True, default=[], help=ROTATION_HELP)
@click.option("--rotations", "track", type=click.Path(exists=True, dir_okay=False, path_type=Path), default=None,
              help="A rotation track: a text file of one `pitch yaw roll` line in degrees per frame, applied after every -r.")
@click.option("--chunk", type=click.INT, default=8, show_default=True, help=f"Frames per launch, a multiple of {TRACK_FRAMES}.")
@click.option("--interpolation", type=click.Choice(list(nat.VIDEO_INTERPOLATIONS)), default="nearest", show_default=True,
              help="The sampler: nearest (the reference's) or bilinear (chroma co-sited with its block's top-left pixel; not with --rotations).")
def remap_yuv(input_frames, output_frames, width, height, pix_fmt, otype, lens, fov, size, rotation, track, chunk, interpolation, lens_coefficients, lens_max_theta):
    """Remap raw PLANAR video frames of an equirectangular panorama - yuv420p, yuv422p, yuv444p, their 10- and 16-bit forms, gbrp - e.g.
    between two `ffmpeg -f rawvideo -pix_fmt yuv420p` pipes.

    \b
    INPUT is a file of packed frames, three planes each: HEIGHT x WIDTH, then two of the format's chroma size; - is stdin.
    OUTPUT receives the packed output frames; - is stdout.
    By default the output is a panorama of the same size (--size H: H x 2H); with --type, --lens and --fov it is the photo make-photo would make.
    4:2:0 formats have even widths and heights, 4:2:2 formats even widths, 4:4:4 formats (gbrp among them) take any size.
    """
    _remap_video(pix_fmt, input_frames, output_frames, width, height, otype, lens, fov, size, rotation, track, chunk, interpolation, lens_coefficients, lens_max_theta)


def _stitch_video(input_frames, output_frames, width, height, pix_fmt, lens, fov, out_width, out_height, rotation, track, chunk, lens_coefficients, lens_max_theta):
    """The body of stitch-yuv and stitch-track-yuv (`track`: the file of a rotation track, or None)."""
    dt, fam, fill = nat.VIDEO_FORMATS[pix_fmt]
    rule, least = ("4:2:0 frames have even dimensions", 2) if fam.pairs else (nat.planar_dims_rule(fam.sub, pix_fmt), 1)
    if width < max(least, 2) or height < least or not nat.planar_dims_ok(fam.sub, (height, width)):
        _fail(f"{rule}, got --width {width} --height {height}")
    h_out = height if out_height is None else out_height
    w_out = 2 * h_out if out_width is None else out_width
    if h_out < least or w_out < least or not nat.planar_dims_ok(fam.sub, (h_out, w_out)):
        _fail(f"{rule}: the output would be {h_out} x {w_out}")
    if chunk < TRACK_FRAMES or chunk % TRACK_FRAMES:
        _fail(f"--chunk is a multiple of {TRACK_FRAMES}, got {chunk}")
    try:
        source = camera_object("double", np.zeros((height, width, 3), np.uint8), radians_fov(fov, "double"), lens_object(lens, lens_coefficients, lens_max_theta),
                               magnitude_for("double", (height, width, 3)))
    except ValueError as exc:
        _fail(str(exc))
    cmap = PanoramaImage(np.zeros((h_out, w_out, 3), np.uint8)).get_coordinate_map()
    for rot in rotation:
        cmap = Rotation(*map(to_radians, rot)).rotate_coordinate_map(cmap)
    dstp, srcp = cmap.dst_proj, source._proj()
    mats = None if track is None else core.rotation_track(_read_track(track))
    frame = fam.packed(height, width)[0]
    # without a track: a prepared plan and the tile kernel; with one: a deferred plan (its tables are never read) and the track kernel
    plan = None

    def remap(host, first):  # upload, ONE launch, download
        nonlocal plan
        if plan is None:  # (made with the first frames: the usage errors of the input come before any plan is prepared)
            plan = nat.Plan(dstp, list(cmap.rotations), srcp, bilinear=False) if mats is None else nat.Plan(dstp, list(cmap.rotations), srcp, defer=True)
        s = nat.to_device(host.reshape((len(host),) + frame))
        if mats is None:
            return plan.stitch_nv12(s) if fam.pairs else plan.stitch_planar(s, fam.sub, fill=fill)
        rots = mats[first : first + len(host)]
        return plan.stitch_track_nv12(s, rots) if fam.pairs else plan.stitch_track_planar(s, rots, fam.sub, fill=fill)

    _stream_frames(input_frames, output_frames, int(np.prod(frame)) * dt.itemsize, dt, chunk, mats, remap)


def _stitch_options(command):
    """The arguments and options the two stitch commands share."""
    for decorate in reversed([
        click.argument("input_frames", metavar="INPUT", type=click.Path(path_type=Path, allow_dash=True)),
        click.argument("output_frames", metavar="OUTPUT", type=click.Path(path_type=Path, allow_dash=True)),
        click.option("--width", required=True, type=click.INT, help="The width of an input frame in pixels: both fisheye circles side by side."),
        click.option("--height", required=True, type=click.INT, help="The height of an input frame in pixels."),
        click.option("--pix-fmt", type=click.Choice(list(nat.VIDEO_FORMATS)), default="nv12", show_default=True, help="The frames' layout, as ffmpeg names it."),
        click.option("--lens", type=_lens_choice, required=True, help="The lens type of the two fisheye cameras."),
        _lens_parameters("--lens", "lens"),
        click.option("--fov", type=click.FLOAT, required=True, help="The field of view of each fisheye camera in degrees (180 to 360)."),
        click.option("--out-width", type=click.INT, default=None, help="The width of an output frame. [default: twice the output height]"),
        click.option("--out-height", type=click.INT, default=None, help="The height of an output frame. [default: the input's]"),
        click.option("-r", "--rotation", type=click.FLOAT, nargs=3, multiple=True, default=[], help=ROTATION_HELP),
        click.option("--chunk", type=click.INT, default=8, show_default=True, help=f"Frames per launch, a multiple of {TRACK_FRAMES}."),
    ]):
        command = decorate(command)
    return command


@main.command("stitch-yuv")
@_stitch_options
def stitch_yuv(input_frames, output_frames, width, height, pix_fmt, lens, fov, out_width, out_height, rotation, chunk, lens_coefficients, lens_max_theta):
    """Stitch raw video frames of a side-by-side DOUBLE FISHEYE - NV12, P010, yuv420p, yuv422p, yuv444p, their 10- and 16-bit forms, gbrp -
    into an equirectangular panorama of the same pixel format, e.g. between two `ffmpeg -f rawvideo` pipes.  One launch per chunk, both
    planes, no RGB detour; every sample is the reference's blend of the two eyes' samples.

    \b
    INPUT is a file of packed frames, HEIGHT x WIDTH each; - is stdin.
    OUTPUT receives the packed panorama frames, OUT-HEIGHT x OUT-WIDTH each; - is stdout.
    4:2:0 formats have even widths and heights, 4:2:2 formats even widths, 4:4:4 formats (gbrp among them) take any size.
    """
    _stitch_video(input_frames, output_frames, width, height, pix_fmt, lens, fov, out_width, out_height, rotation, None, chunk, lens_coefficients, lens_max_theta)


@main.command("stitch-track-yuv")
@_stitch_options
@click.option("--rotations", "track", type=click.Path(exists=True, dir_okay=False, path_type=Path), required=True,
              help="A rotation track: a text file of one `pitch yaw roll` line in degrees per frame, applied after every -r.")
def stitch_track_yuv(input_frames, output_frames, width, height, pix_fmt, lens, fov, out_width, out_height, rotation, track, chunk, lens_coefficients, lens_max_theta):
    """Stitch raw video frames of a side-by-side DOUBLE FISHEYE with a ROTATION PER FRAME - a gyro track: a stabilised, horizon-levelled
    panorama of the same pixel format.  stitch-yuv's formats, sizes and options; one launch per chunk, every plane, no RGB detour and no
    plan per frame; every sample is the reference's blend of the two eyes' samples for that frame's rotations.

    \b
    INPUT is a file of packed frames, HEIGHT x WIDTH each; - is stdin.
    OUTPUT receives the packed panorama frames, OUT-HEIGHT x OUT-WIDTH each; - is stdout.
    --rotations holds at least one line per input frame.
    """
    _stitch_video(input_frames, output_frames, width, height, pix_fmt, lens, fov, out_width, out_height, rotation, track, chunk, lens_coefficients, lens_max_theta)


if __name__ == "__main__":
    main()
