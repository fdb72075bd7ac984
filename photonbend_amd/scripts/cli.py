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


if __name__ == "__main__":
    main()
