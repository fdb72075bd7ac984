"""What tests/test_hip_pxf_interp.py runs pb_remap_interp_pxf on, the frames it draws, and how far a sample may lie from the definition's
float64 value, shared with the CPU conditions on all three (tests/test_pxf_host.py)."""

import numpy as np

from tests import px_interp_cases as pc

# pb_remap_interp_px's cases without the one this call refuses: a source of two pixels has no coordinate tables, and float samples have no
# per-pixel route
REFUSED = "tiny_pano_1x2"
CASES = [c for c in pc.CASES if c.name != REFUSED]
ALL_FORMAT_CASES = pc.ALL_FORMAT_CASES
FORMATS = [(C, S) for S in (2, 4) for C in (1, 2, 3, 4)]  # (channels, sample_bytes): binary16 and binary32
BAND = pc.BAND
PINNED_BANDS = pc.PINNED_BANDS
DTYPE = {2: np.float16, 4: np.float32}
U_OUT = {2: 2.0**-11, 4: 2.0**-24}  # the unit roundoff of the narrowing
# The draws: independent random samples, all normal numbers.  (name, L, U) - the range the tolerance is worked out for.
DRAWS = {
    4: (("unit", 0.25, 1.0), ("signed", -1000.0, 1000.0), ("hdr", 2.0**-8, 2.0**12)),
    2: (("unit", 0.25, 1.0), ("signed", -64.0, 64.0), ("hdr", 2.0**-8, 2.0**12)),  # 1.5625 x 4096 = 6400: inside 65504 after the cubic's overshoot
}


def draw(h, w, C, S, k, seed, squeeze=True):
    """Draw k of sample size S: an (h, w, C) frame - (h, w) for one channel - and its (L, U)."""
    name, L, U = DRAWS[S][k]
    rng = np.random.default_rng(seed)
    if name == "hdr":
        a = np.exp2(rng.uniform(-8.0, 12.0, size=(h, w, C)))
    else:
        a = rng.uniform(L, U, size=(h, w, C))
        if name == "signed":  # (no sample so near zero that it is subnormal in the sample type: 2^-14 is the smallest normal half)
            a = np.where(np.abs(a) < 2.0**-10, 1.0, a)
    a = np.clip(a.astype(DTYPE[S]), DTYPE[S](L), DTYPE[S](U))  # (the narrowing may not leave [L, U])
    assert np.isfinite(a).all() and (np.abs(a) >= np.finfo(DTYPE[S]).tiny).all()
    return (a[:, :, 0].copy() if C == 1 and squeeze else a), (L, U)


POISON_PANO, POISON_TEXEL = "mag_pano_pole_and_seam", (12, 16)  # NaN containment: the panorama-source case and its poisoned texel
POISON_CAM = "mag_stereo_from_cal"  # ... and the camera-source case (its centre output pixel is live): the texel under that pixel


def poison_mask(src_proj, final, texel):
    """The output pixels a non-finite sample at `texel` may spoil: those whose tap base (i0, j0) lies within 3 texels of it per axis -
    texel - 3 <= base <= texel + 2, a panorama's columns modulo w.  The 4 x 4 footprint reaches base - 1 .. base + 2, so it holds the texel
    for texel - 2 <= base <= texel + 1, and a tile kernel's tap base is the definition's or its neighbour (coordinates certified to 1/1024
    px): every footprint that can hold the texel is inside.  Dead pixels never count."""
    from tests import pxf_ref

    i0, j0, _, _, live = pxf_ref.tap_base(src_proj, np.copy(final))
    dy, dx = i0 - texel[0], j0 - texel[1]
    if src_proj.kind == "pano":
        w = src_proj.width
        dx = (dx + w // 2) % w - w // 2
    return live & (dy >= -3) & (dy <= 2) & (dx >= -3) & (dx <= 2)


def centre_texel(src_proj, final):
    """The texel under the centre output pixel (which must be live)."""
    from tests import pxf_ref

    fy, fx, live = pxf_ref.positions(src_proj, np.copy(final))
    cy, cx = final.shape[0] // 2, final.shape[1] // 2
    assert live[cy, cx]
    return int(np.floor(fy[cy, cx])), int(np.floor(fx[cy, cx]))


def tolerance(filt: str, L: float, U: float, S: int) -> float:
    """How far a sample may lie from the definition's float64 V when the frame's samples lie in [L, U]: D = U - L, M = max(|L|, |U|),
    u_out = 2^-24 (float32) or 2^-11 (float16).  The tile coordinates are certified to 1/1024 px per axis.
      bilinear      D / 512 + M 2^-20 + M u_out: V moves by at most D per unit of tx and of ty (video_bilinear_ref.tolerance's R / 512); the
                    three float32 lerps have at most 4 u D + 4 u M <= 12 u M < 16 u M, u = 2^-24; one narrowing of a value of at most M.
      catmull-rom   15 D / 4096 + M 2^-18 + 1.5625 M u_out: DESIGN 3.8's coordinate budget with D for R (taps at most D / 2 from mid-range,
                    sum |w| <= 1.25, sum |w'| <= 3); DESIGN 3.23's arithmetic ceiling 33.125 u M < 64 u M; one narrowing of a value of at
                    most 1.25^2 M."""
    D, M = float(U) - float(L), max(abs(float(L)), abs(float(U)))
    if filt == "bilinear":
        return D / 512.0 + M * 2.0**-20 + M * U_OUT[S]
    assert filt == "catmull-rom", filt
    return 15.0 * D / 4096.0 + M * 2.0**-18 + 1.5625 * M * U_OUT[S]
