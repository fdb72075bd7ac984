/*
 * photonbend_hip.h - C ABI of the MI355X (gfx950) per-pixel lens remapper.
 *
 * This is the drop-in boundary for photonbend's core remap path.  Every entry
 * point is extern "C", takes plain pointers and sizes, returns 0 on success or
 * a negative pb_status (message via pb_last_error()), never throws, never
 * allocates or synchronises inside a launch function (so a caller may capture
 * launches into a hipGraph), and works on caller-owned DEVICE buffers on a
 * caller-chosen HIP stream (passed as void*; NULL = the default stream).
 *
 * Reference interfaces replaced (all paths under /root/reference/photonbend):
 *   pb_proj            the state of CameraImage (core/projection.py:86-121),
 *                      DoubleCameraImage (:296-316) and PanoramaImage (:477-485)
 *   pb_plan_create     dst.get_coordinate_map() -> Rotation.rotate_coordinate_map()*
 *                      -> src.process_coordinate_map()  chained lazily
 *                      (core/__init__.py:66-92)
 *   pb_remap_u8        that chain, fused: one work-item per output pixel
 *   pb_remap_px        the same for the other arrays the reference's fancy indexing takes - grey (H, W),
 *                      RGBA, 16-bit samples: pixels of 1, 2, 4, 6 or 8 bytes - in one launch
 *                      (image[positions], projection.py:234-243, :545-546)
 *   pb_index_map_i32   the integer coordinate map inside process_coordinate_map
 *                      (projection.py:254-259, :545)
 *   pb_coordmap_f64    get_coordinate_map()  (projection.py:147, :341, :487)
 *   pb_rotate_f64      Rotation.rotate_coordinate_map()  (core/rotation.py:102-176)
 *   pb_sample_map_u8   process_coordinate_map(ndarray)  (projection.py:197, :408, :515)
 *
 * Images are uint8 (H, W, 3) RGB, row-major, tightly packed (core/__init__.py:31-36); pb_remap_px, pb_gather_px and
 * pb_gather_blend_u8 take the other layouts the reference accepts.
 * Coordinate maps are float64 (H, W, 3) = (latitude, longitude, invalid flag)
 * (core/__init__.py:42-49).  Angles are radians.
 */
#ifndef PHOTONBEND_HIP_H
#define PHOTONBEND_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define PB_ABI_VERSION 5
#define PB_MAX_ROTATIONS 8

typedef enum pb_status {
    PB_OK = 0,
    PB_ERR_INVALID = -1,   /* bad argument (null pointer, size, enum value) */
    PB_ERR_HIP = -2,       /* a HIP runtime call failed */
    PB_ERR_UNSUPPORTED = -3,
    PB_ERR_NO_DEVICE = -4
} pb_status;

/* projection.py class -> kind */
typedef enum pb_kind {
    PB_KIND_CAMERA = 0, /* CameraImage        projection.py:69  */
    PB_KIND_DOUBLE = 1, /* DoubleCameraImage  projection.py:277 */
    PB_KIND_PANO = 2,   /* PanoramaImage      projection.py:465 */
    /* (3 and 4 are taken inside the library: the two eyes of a double-fisheye source as sources of their own) */
    PB_KIND_CUBE = 5,   /* a cube map (additive, ABI 5): no reference class - six rectilinear CameraImage faces of 120
                           degrees with f_distance N / 2, each behind a fixed rotation, in one (2N, 3N) frame: top row left, front,
                           right - bottom row up, back, down.  height = 2N, width = 3N; lens, fov, magnitude and f_distance are
                           ignored, as for a panorama.  A destination and a source wherever the other kinds are. */
    /* (6 and 7 stay refused, as they always were) */
    PB_KIND_EAC = 8     /* an equi-angular cube map (additive, ABI 5): PB_KIND_CUBE's frame, faces, face selection and
                           truncation, but the position on a face is proportional to the ANGLE from the face centre, not to its
                           tangent: with half = N / 2 a centred face coordinate c of this kind is the plain cube's
                           tan((c / half) * (pi / 4)) * half, and back (atan(c / half) * (4 / pi)) * half.  Same shape rule, same
                           ignored fields; a destination and a source wherever PB_KIND_CUBE is. */
} pb_kind;

/* core/lens.py factories :341-401 */
typedef enum pb_lens {
    PB_LENS_EQUIDISTANT = 0,
    PB_LENS_EQUISOLID = 1,
    PB_LENS_RECTILINEAR = 2,
    PB_LENS_STEREOGRAPHIC = 3,
    PB_LENS_ORTHOGRAPHIC = 4,
    PB_LENS_THOBY = 5,
    PB_LENS_CUSTOM = 6 /* Lens(forward_function, reverse_function) of arbitrary Python callables (lens.py:48-64): the HOST
                          evaluates them; accepted only by pb_index_from_map_i32 together with its distance planes */
} pb_lens;

/* One end of a remap.  f_distance is computed by the HOST with the reference
 * formula magnitude / forward_lens(fov / 2) (projection.py:141-144) so that its
 * bits are the caller's; the kernels never recompute it. */
typedef struct pb_proj {
    int32_t kind;      /* pb_kind */
    int32_t lens;      /* pb_lens (ignored for PB_KIND_PANO, PB_KIND_CUBE and PB_KIND_EAC) */
    int32_t height;
    int32_t width;
    double fov;        /* radians; the per-sensor fov for PB_KIND_DOUBLE */
    double magnitude;  /* informational (already folded into f_distance) */
    double f_distance; /* focal distance in pixels */
} pb_proj;

/* POLYNOMIAL (KANNALA-BRANDT) LENSES (ABI 5, additive): the odd polynomial a fisheye calibration yields, the k1..k4 of
 * OpenCV's fisheye module,
 *     r(theta) = theta + k1 theta^3 + k2 theta^5 + k3 theta^7 + k4 theta^9        (r in focal-length units)
 * on [0, max_theta] (radians, 0 < max_theta <= pi), +inf beyond; its inverse is ten Newton steps from t = r, +inf beyond r(max_theta).
 * Evaluated by the float64 chain with + - * / only, each rounded on its own: bit-reproducible by any IEEE host, the same in both math
 * flavours.  pb_proj does not grow: a lens is REGISTERED once and the id it gets (PB_LENS_POLYNOMIAL_BASE upwards) is a pb_proj.lens every
 * entry point accepts, in either role, wherever it accepts a built-in lens.
 *   pb_lens_polynomial       validates (finite coefficients; max_theta in range; r increasing on [0, max_theta]; the Newton steps invert it
 *                            there - PB_ERR_INVALID otherwise) and registers.  Entries are immutable; the same coefficients and max_theta
 *                            give the same id; thread-safe; at most 4096 distinct lenses per process, then PB_ERR_UNSUPPORTED.
 *   pb_lens_polynomial_info  the coefficients and max_theta of a registered id (either pointer may be NULL).
 * An id means something in THIS process only.  Nothing that outlives the process holds one: plans, their blobs (pb_plan_serialize),
 * pb_plan_matches and pb_bcast_params carry and compare the coefficients.  The caller computes pb_proj.f_distance as for every lens:
 * magnitude / r(fov / 2), with fov / 2 <= max_theta.  (The parameter block inside a plan blob grew with this addition: blobs written by
 * earlier builds are refused by the size check, like blobs of any other build.) */
#define PB_LENS_POLYNOMIAL_BASE 16
int pb_lens_polynomial(const double k[4], double max_theta, int* lens_out);
int pb_lens_polynomial_info(int lens, double k[4], double* max_theta);

typedef struct pb_plan pb_plan; /* opaque, immutable after creation */

/* ---- library / device ------------------------------------------------- */
int pb_abi_version(void);
/* 0: the float64 chain runs NumPy's AVX-512 arcsin / arccos / arctan / tan (hosts with AVX512_SKX); 1: glibc's (hosts without).  See
 * PB_PLAN_MATH_SVML / PB_PLAN_MATH_LIBM. */
int pb_math_flavour(void);
const char* pb_last_error(void); /* thread-local, valid until the next failing call */
int pb_init(int device);         /* hipSetDevice + sanity checks (gfx950 expected) */
int pb_shutdown(void);           /* returns the idle blocks of the plan-preparation cache (<= 96 MiB of device memory) to the driver; plans stay valid */
int pb_device_name(char* buf, size_t buflen);

/* ---- the fused hot path ------------------------------------------------ */
/* rot3x3: n_rot row-major 3x3 float64 matrices = Rotation.rotation_matrix
 * (core/rotation.py:100), applied in order; n_rot in [0, PB_MAX_ROTATIONS].
 * When a HIP device is visible, creation prepares the plan on the CURRENT device (synchronously,
 * about the cost of two faithful frames): destination-validity thresholds, per-tile models (one
 * table per eye for a double-fisheye source), the exhaustive comparison with the faithful chain, and
 * the exact lookup tables for everything the models miss (source indices of failed tiles and fix
 * pixels; for double sources also their blend factors and the latitudes of merge-band tiles).  The
 * plan then owns device memory on that device (256 B per 32x32 output tile and eye + the tables)
 * until pb_plan_destroy. */
int pb_plan_create(const pb_proj* dst, const double* rot3x3, int n_rot, const pb_proj* src, pb_plan** out);
void pb_plan_destroy(pb_plan* plan);

/* Explicit form of pb_plan_create (which is pb_plan_create_ex(..., 0, 0, out)).
 *   flags       PB_PLAN_DEFER  no device work at creation: the plan is a parameter block and its launches run the
 *                              faithful float64 kernel (the cheapest way to remap ONE image of a geometry, the
 *                              reference CLI's case) until pb_plan_prepare builds the fast path;
 *               PB_PLAN_TUNE   after preparation, pick the LDS window budget (four candidates) and then the launch order
 *                              (the policy's walk against plain / heaviest rows first / heaviest super-tiles first) by
 *                              timing launches on scratch frames (allocates frame-sized scratch, about a hundred frames'
 *                              worth of GPU time; opt-in).  Both decide paths and order only, never a byte; a serialized
 *                              plan remembers them.
 *   win_budget  bytes of LDS window per wave for the hot kernels (multiple of 16 in [4224, 12288]; clamped);
 *               0 = the library default (7168).  It decides which PATH a tile takes, never its pixels.
 * Creation never times anything or allocates frame-sized memory unless PB_PLAN_TUNE is given. */
#define PB_PLAN_DEFER 1u
#define PB_PLAN_TUNE 2u
/* MATH FLAVOURS (ABI 5).  The reference's float64 results depend on which code NumPy dispatches to on the HOST it runs on: with
 * AVX512_SKX np.arcsin / arccos / arctan / tan (core/lens.py:71-307, core/rotation.py:158) are NumPy's own AVX-512 kernels, without it
 * they are libm's (glibc 2.35: asin / acos / atan / tan) - 7-8 % of the arcsin / arccos results differ in the last bit, and with them
 * whole texels of identity-type remaps.  The library comes in both flavours, built from the same sources: libphotonbend_hip.so
 * (pb_math_flavour() == 0: the AVX-512 kernels' bits, the platform of tests/golden/) and libphotonbend_hip_libm.so (== 1: libm's bits,
 * tests/golden/npmath_libm.npz, libm_flavour.json); a host loads the one that matches ITS reference (photonbend_amd/_native.py does:
 * NumPy's own dispatch decides, PB_MATH_FLAVOUR=svml|libm overrides).  The two flags below let a caller STATE which flavour a plan must
 * have: pb_plan_create_ex returns PB_ERR_UNSUPPORTED from the library of the other flavour instead of silently giving other bits. */
#define PB_PLAN_MATH_SVML 4u
#define PB_PLAN_MATH_LIBM 8u
/* THE OPT-IN BILINEAR MODE'S TABLES (flag values added in round 6; ABI 5 unchanged).  A prepared plan carries, besides what the reference's
 * nearest sampler needs, the opt-in bilinear mode's state (exact coordinate tables, its own launch table and LDS pool: 0.2-0.3 ms of a
 * c2 plan's 0.85 ms).  PB_PLAN_NO_BILINEAR (pb_plan_create_ex) leaves it out - for callers of pb_remap_u8, the reference's path;
 * PB_PLAN_BILINEAR (pb_plan_prepare, synchronous, no launch of the plan in flight) builds it later.  pb_remap_bilinear_u8 on a plan
 * without it is still correct - it runs the mode's per-pixel float64 kernels, several times slower - and pb_plan_bilinear_float64_tiles
 * says so (every tile).  A deferred plan (PB_PLAN_DEFER) remembers either choice for its preparation.  Default (neither flag): as before.
 * A double-fisheye source whose field of view lies within one degree of 180 (180 itself excepted) never gets the tables: the reference's blend factor
 * past the end of so narrow a merge band (projection.py:440-444) multiplies any sampler's rounding; the mode's float64 kernels serve it. */
#define PB_PLAN_NO_BILINEAR 16u
#define PB_PLAN_BILINEAR 32u
int pb_plan_create_ex(const pb_proj* dst, const double* rot3x3, int n_rot, const pb_proj* src, unsigned flags,
                      int win_budget, pb_plan** out);
/* Builds the fast path of a deferred plan on the current device (flags: 0, PB_PLAN_TUNE, PB_PLAN_BILINEAR).  On a prepared plan
 * it applies win_budget (when > 0) and, with PB_PLAN_BILINEAR, builds the bilinear mode's tables if the plan lacks them.  Synchronous. */
int pb_plan_prepare(pb_plan* plan, unsigned flags, int win_budget);
/* Re-classifies the tiles of a prepared plan under another window budget (synchronous, cheap: one small kernel). */
int pb_plan_set_window_budget(pb_plan* plan, int win_budget);
/* Host wall time (ms) of the device preparation and of the optional tuning; either pointer may be NULL. */
int pb_plan_timing(const pb_plan* plan, double* prepare_ms, double* tune_ms);
/* A prepared plan as a host blob and back, so that a process (the CLI's one-image case) need not pay the
 * per-pixel certification again for a geometry it has seen: pass buf = NULL to query the size.  The blob is
 * valid for this library build only (checked) and carries a checksum; deserialisation uploads the tables to
 * the CURRENT device.  The blob names the math flavour that made its exact tables: the library of the other flavour
 * refuses it with PB_ERR_UNSUPPORTED (a blob cache shared by hosts with and without AVX-512 keeps one blob per flavour). */
int pb_plan_serialize(const pb_plan* plan, void* buf, size_t capacity, size_t* size_out);
int pb_plan_deserialize(const void* buf, size_t size, pb_plan** out);
/* Execution mode of a plan.  AUTO (default) and FAST: ONE launch of the hot kernel per call (per-tile
 * float32 polynomial models of the coordinate field; what the models miss is looked up in the plan's
 * exact tables), when the plan was prepared on a device; otherwise, and under FAITHFUL, the per-pixel
 * float64 chain for every pixel.  Both produce identical bytes: the tables hold, by construction at
 * plan creation, the faithful result for every pixel whose model index differs from the faithful one. */
#define PB_MODE_AUTO 0
#define PB_MODE_FAITHFUL 1
#define PB_MODE_FAST 2
#define PB_MODE_FAST_DIRECT 3 /* FAST without LDS windows: direct-gather hot kernel + fix kernel, the path of frames that are
                                 not 16-byte aligned (double sources: the separable / faithful kernels) */
int pb_plan_set_mode(pb_plan* plan, int mode);
/* fast_path_enabled: 0/1 under the current mode; stats7: {32x32 tiles, tiles handled whole by the
 * tables ("failed"), single pixels on the fix list, pixels where model and faithful index differed,
 * tiles on the lean LDS-window path, all-black tiles, tiles on the lean direct-gather path} (-1 when the
 * plan has no device state; a double-fisheye source counts both eyes' tables in the last four);
 * thresholds4:
 * {invalid_lo, invalid_hi} on (2x)^2+(2y)^2 for the left/single and the right eye of the
 * destination.  Any pointer may be NULL. */
int pb_plan_info(const pb_plan* plan, int* fast_path_enabled, long long* stats7, long long* thresholds4);
int pb_plan_dst_shape(const pb_plan* plan, int* height, int* width);
int pb_plan_src_shape(const pb_plan* plan, int* height, int* width);
/* bytes of LDS window per wave the plan's hot launches use (it decides which path a tile takes, never its
 * pixels); 0 without device state */
int pb_plan_window_budget(const pb_plan* plan);
/* How many 32x32 tiles of a prepared plan the opt-in bilinear mode (pb_remap_bilinear_u8) recomputes with the float64 chain per
 * pixel instead of the tile models: failed tiles, tiles whose model is further than 1/1024 px from the faithful coordinate
 * somewhere (fine for the reference's truncating sampler, whose exceptions are tabulated; too coarse to interpolate at), and
 * - double-fisheye sources - tiles that are not plain for an eye that sees them.  0 for a deferred plan. */
int pb_plan_bilinear_float64_tiles(const pb_plan* plan);
/* Diagnostics of the opt-in bilinear mode (ABI 5; synchronous, not for the hot loop): how its launch serves the tile entries its waves
 * read - mix[0] LDS-window entries, [1] direct-gather entries, [2] entries read from the exact coordinate table, [3] black entries,
 * [4] window / direct entries whose coordinate is evaluated on the certified low-degree part of the tile model (PB_TILE_TD3),
 * [5] entries counted (one per tile; a double-fisheye plan's two-eye tiles have one per eye), [6] of the window entries [0], those
 * staged as two half windows (their source box exceeds the budget, its top and bottom halves do not), [7] of the table entries [2],
 * those whose taps all lie inside the frame (read without clamps or wrap).  All zero without tile tables. */
int pb_plan_bilinear_tile_mix(const pb_plan* plan, long long mix[8]);
/* ... and the shape of its launch (ABI 5): the dynamic LDS of a workgroup (the pool its four waves' windows are packed into: 40 448 bytes -
 * four workgroups per CU - where at most 2 % of the tiles lose their window to it, else four full-budget regions) and the workgroups
 * of one frame (four waves = four tiles each; the grid of an n-frame launch is n times that); both 0 without tile tables. */
int pb_plan_bilinear_launch_shape(const pb_plan* plan, int* lds_bytes, int* workgroups_per_frame);

/* 1 when `plan` was made for exactly this request (same projections, same rotation bits), 0 when not, negative on bad
 * arguments (ABI 3).  What a cache of serialized plans checks after pb_plan_deserialize: the blob's checksum says it is
 * intact, not that it belongs to the geometry the caller has in mind. */
int pb_plan_matches(const pb_plan* plan, const pb_proj* dst, const double* rot3x3, int n_rot, const pb_proj* src);

/* Remap n_frames frames that share the plan's geometry.  Frame f is read at
 * src_dev + f * src_frame_stride and written at dst_dev + f * dst_frame_stride
 * (strides in bytes, at least a frame; pass 0 for tightly packed frames).  ONE kernel launch whatever n_frames:
 * the frames of a batch are a dimension of the grid, so the launch ramp and drain are paid once per call
 * (measured on MI355X: 8 frames per call run 1.3x faster per frame than 8 calls).  Asynchronous on `stream`;
 * never allocates or synchronises (graph-capture safe).  A deferred plan (PB_PLAN_DEFER, not yet prepared) runs
 * the faithful float64 kernel.  (A double-fisheye -> unrotated panorama plan keeps a second, separable fast path for frames the windowed
 * kernel cannot take - source pointer or stride not a multiple of 16 bytes, PB_MODE_FAST_DIRECT; its tables are verified against the
 * float64 chain by a kernel the FIRST such launch enqueues on `stream`: that launch, launches inside a stream capture, and any launch
 * issued before the verification has finished run the float64 kernel instead - same bytes, slower.) */
int pb_remap_u8(const pb_plan* plan, const uint8_t* src_dev, uint8_t* dst_dev, int n_frames,
                size_t src_frame_stride, size_t dst_frame_stride, void* stream);

/* The same batch launch for frames that are NOT at a uniform stride - a ring of separately allocated buffers (ABI 5).
 * src_dev / dst_dev are HOST arrays of n_frames DEVICE pointers (tightly packed frames); frame f is read at src_dev[f] and
 * written at dst_dev[f].  ONE kernel launch per 64 frames on `stream`: the pointers travel in the kernel-argument segment
 * (read at launch: the arrays may be reused when the call returns), so the call stays allocation- and synchronisation-free
 * (graph-capture safe) like pb_remap_u8, whose bytes it reproduces.  Frames the windowed kernels cannot take (a source
 * pointer not 16-byte aligned), deferred plans and PB_MODE_FAITHFUL / PB_MODE_FAST_DIRECT run as n_frames single launches.
 * Replaces: a host loop over process_coordinate_map() (core/__init__.py:66-92) on separately allocated arrays. */
int pb_remap_u8v(const pb_plan* plan, const uint8_t* const* src_dev, uint8_t* const* dst_dev, int n_frames, void* stream);

/* pb_remap_u8 for frames whose pixel is not three bytes (ABI 5, additive): grey (bytes_per_px 1), 16-bit grey or two
 * uint8 channels (2), RGBA (4), 16-bit RGB (6), 16-bit RGBA (8).  The reference's nearest sampler never looks inside a pixel - it copies
 * bytes_per_px bytes from the plan's certified source index - so the bytes are those of pb_index_map_i32 + pb_gather_px, in ONE launch
 * of the tile kernel pb_px_hot_kernel whatever n_frames, without an index map in memory.  pb_remap_u8's contract: the same argument
 * checks and messages, strides in bytes (0: packed frames of bytes_per_px * h * w), asynchronous on `stream`, never allocates or
 * synchronises (graph-capture safe).
 *   bytes_per_px == 3            exactly pb_remap_u8 (same route, same bytes);
 *   outside {1, 2, 3, 4, 6, 8}   PB_ERR_INVALID;
 *   alignment                    frame pointers and strides must be multiples of min(4, bytes_per_px & -bytes_per_px) bytes - 1, 2, 4, 2, 4
 *                                for 1, 2, 4, 6, 8 - else PB_ERR_INVALID, before any launch;
 *   PB_ERR_UNSUPPORTED           (nothing is written; use pb_index_map_i32 + pb_gather_px) for plans the tile kernel does not serve:
 *                                deferred plans, PB_MODE_FAITHFUL, double-fisheye sources (their blend is sample-typed:
 *                                pb_gather_blend_u8), plans without device state, sources of 32768 px a side or more, and frames of
 *                                bytes_per_px * h * w >= 2^31 bytes (the kernel's source byte offsets are 32-bit).
 * pb_remap_px_supported: 1 when pb_remap_px takes `plan` with this pixel size, 0 when it would return PB_ERR_UNSUPPORTED, negative on
 * bad arguments - a caller chooses its path without provoking the error. */
int pb_remap_px(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, size_t src_frame_stride,
                size_t dst_frame_stride, int bytes_per_px, void* stream);
int pb_remap_px_supported(const pb_plan* plan, int bytes_per_px);

/* 4:2:0 semi-planar video frames - NV12 (bytes_per_sample 1) and P010 / P016 (2) - in ONE launch of the tile kernel pb_video_hot_kernel
 * whatever n_frames (ABI 5, additive).  A frame is a plane of height x width luma samples and, uv_offset bytes after its
 * start, a plane of height/2 x width/2 interleaved (U, V) pairs; the rows of both planes are `pitch` bytes apart - the surface a hardware
 * video decoder writes.  With idx the plan's index map (pb_index_map_i32):
 *   luma     Y_out[y][x] = Y_src[r][c], (r, c) = divmod(idx[y][x], w); fill_yuv[0] where idx[y][x] < 0;
 *   chroma   UV_out[i][j] = UV_src[r >> 1][c >> 1], (r, c) = divmod(idx[2i][2j], w) - the ANCHOR, the top-left pixel of the 2 x 2 block;
 *            (fill_yuv[1], fill_yuv[2]) where idx[2i][2j] < 0.  Only the anchor decides, whatever the block's other pixels are.
 * This is a NEAREST sample of chroma at the anchor's position: it can lie up to one luma pixel off the chroma sample's nominal siting,
 * the order of what truncation does to luma.  No chroma interpolation is done.  The bytes are exact: those of the definition with
 * the reference's own index map.
 *   layouts (bytes; NULL, or a 0 member: the packed default)   pitch = S * width; uv_offset = pitch * height; frame_stride = uv_offset +
 *                                pitch * height / 2.  Padding bytes are neither read nor written.
 *   fill_yuv                     the samples of black pixels; NULL: video black, (16, 128, 128) << 8 * (S - 1).
 *   PB_ERR_INVALID               before any launch, nothing is written: null plan or frames, bytes_per_sample outside {1, 2}, an odd
 *                                dimension of source or destination, pitch < S * width, uv_offset < pitch * height, a frame_stride
 *                                smaller than a frame, a pointer, pitch, offset or stride that is not a multiple of 2 * S (one pair).
 *   PB_ERR_UNSUPPORTED           nothing is written - exactly the plans pb_remap_px refuses: deferred plans, PB_MODE_FAITHFUL,
 *                                double-fisheye sources, plans without device state, sources of 32768 px a side or more; and frames
 *                                whose byte span (uv_offset + pitch * height / 2) reaches 2^31 (the kernel's byte offsets are 32-bit) - a pitch
 *                                or uv_offset of 2^31 or more among them, refused before any product is formed.
 * Asynchronous on `stream`, never allocates or synchronises (graph-capture safe).
 * pb_remap_nv12_supported: 1 when pb_remap_nv12 takes `plan` with packed frames of this sample size, 0 when it would return
 * PB_ERR_UNSUPPORTED, negative on bad arguments. */
typedef struct pb_nv12_layout { size_t pitch, uv_offset, frame_stride; } pb_nv12_layout;   /* bytes; 0 = packed default */
int pb_remap_nv12(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_nv12_layout* src_layout,
                  const pb_nv12_layout* dst_layout, int bytes_per_sample, const uint16_t fill_yuv[3], void* stream);
int pb_remap_nv12_supported(const pb_plan* plan, int bytes_per_sample);

/* PLANAR video frames - yuv420p / yuv422p / yuv444p, their 10- and 16-bit forms, gbrp - in ONE launch of the tile kernel
 * pb_video_hot_kernel whatever n_frames (ABI 5, additive).  A frame is three planes of S-byte samples, S = bytes_per_sample:
 * plane 0 of height x width samples at the frame's start, rows `pitch` bytes apart; planes 1 and 2 of (height >> cy) x (width >> cx)
 * samples each, offset1 and offset2 bytes after the frame's start, rows `chroma_pitch` bytes apart.  (cx, cy) is (0, 0) for PB_PLANAR_444,
 * (1, 0) for PB_PLANAR_422 and (1, 1) for PB_PLANAR_420.  With idx the plan's index map (pb_index_map_i32):
 *   plane 0       P0_out[y][x] = P0_src[r][c], (r, c) = divmod(idx[y][x], w); fill[0] where idx[y][x] < 0 - pb_remap_px of the plane;
 *   planes 1, 2   Pk_out[i][j] = Pk_src[r >> cy][c >> cx], (r, c) = divmod(idx[i << cy][j << cx], w) - the ANCHOR, the top-left pixel of
 *                 the sample's block; fill[k] where the anchor's index is negative.  Only the anchor decides.
 * A NEAREST sample of chroma at the anchor's position, as for pb_remap_nv12; no chroma interpolation.  At PB_PLANAR_420 planes 1 and 2,
 * interleaved, are pb_remap_nv12's pairs.  At PB_PLANAR_444 every plane is a grey remap: gbrp is PB_PLANAR_444 with fill (0, 0, 0).  The
 * bytes are exact: those of the definition with the reference's own index map.  Plane order (I420 against YV12, G-B-R) is a matter of
 * offset1 and offset2 alone.
 *   dimensions                   source and destination widths are multiples of 1 << cx, heights of 1 << cy: PB_PLANAR_444 takes any
 *                                size, PB_PLANAR_422 odd heights.
 *   layouts (bytes; NULL, or a 0 member: the packed default)   pitch = S * width; chroma_pitch = S * (width >> cx); offset1 = pitch *
 *                                height; offset2 = offset1 + chroma_pitch * (height >> cy); frame_stride = the end of plane 2.  The planes
 *                                may come in any order.  Padding bytes are neither read nor written.
 *   fill                         the samples of black pixels, per plane; NULL: pb_remap_nv12's video black, (16, 128, 128) << 8 * (S - 1).
 *   PB_ERR_INVALID               before any launch, nothing is written: null plan or frames, a negative count, bytes_per_sample outside
 *                                {1, 2}, a subsampling outside the three, a dimension that breaks the rule above, a pitch smaller than a
 *                                row, planes that overlap each other or plane 0, a plane that ends beyond frame_stride, a pointer, pitch,
 *                                offset or stride that is not a multiple of S (a 1-byte plane may start anywhere).
 *   PB_ERR_UNSUPPORTED           nothing is written - exactly the plans pb_remap_px and pb_remap_nv12 refuse: deferred plans,
 *                                PB_MODE_FAITHFUL, double-fisheye sources, plans without device state, sources of 32768 px a side or more;
 *                                and frames whose byte span (the end of the last plane) reaches 2^31 - a layout member of 2^31 or more
 *                                among them, refused before any product is formed.
 * Asynchronous on `stream`, never allocates or synchronises (graph-capture safe).
 * pb_remap_planar_supported: 1 when pb_remap_planar takes `plan` with packed frames of this subsampling and sample size, 0 when it would
 * return PB_ERR_UNSUPPORTED, negative on bad arguments.
 * pb_remap_track_planar: ROTATION TRACKS for these frames - pb_remap_track_nv12's contract with the definition above: frame f receives it
 * with idx the index map of the chain "this plan's own n_rot rotations followed by the n_rot_per_frame matrices of table entry f";
 * equivalently what pb_remap_planar writes for frame f alone from a prepared plan of that whole chain, wherever pb_remap_planar_supported.
 * The plan's tables are never read: a deferred plan, a prepared one and any mode are served alike.  PB_ERR_INVALID before any launch, in
 * this order: pb_remap_planar's checks, then pb_remap_track_u8's table checks.  PB_ERR_UNSUPPORTED, nothing written: a double-fisheye
 * source, frames whose byte span reaches 2^31, sources of 32768 px a side or more.  n_frames == 0: PB_OK, no launch, no device. */
#define PB_PLANAR_444 0
#define PB_PLANAR_422 1
#define PB_PLANAR_420 2
typedef struct pb_planar_layout { size_t pitch, chroma_pitch, offset1, offset2, frame_stride; } pb_planar_layout;  /* bytes; 0 = packed default */
int pb_remap_planar(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_planar_layout* src_layout,
                    const pb_planar_layout* dst_layout, int subsampling, int bytes_per_sample, const uint16_t fill[3], void* stream);
int pb_remap_planar_supported(const pb_plan* plan, int subsampling, int bytes_per_sample);
int pb_remap_track_planar(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames,
                          const pb_planar_layout* src_layout, const pb_planar_layout* dst_layout, int subsampling, int bytes_per_sample,
                          const uint16_t fill[3], void* stream);

/* OPT-IN: BILINEAR sampling of the same video frames in ONE launch of the tile kernel pb_planar_bilinear_kernel whatever n_frames
 * (ABI 5, additive).  No reference counterpart: the definition is written down in tests/video_bilinear_ref.py.  With f the
 * reference's pre-truncation source coordinate of an output pixel and "live" as for pb_remap_bilinear_u8:
 *   plane 0       pb_remap_bilinear_u8's definition on a grey plane: s = f - 0.5, taps floor(s), floor(s) + 1 per axis, rows clamped, a
 *                 panorama's columns wrapped, a camera's clamped, round half to even; fill[0] where the pixel is not live.
 *   planes 1, 2   sample (i, j) is decided by its ANCHOR (i << cy, j << cx) as in the nearest calls.  Chroma is co-sited with the top-left
 *                 luma pixel of its block (source and destination alike): the anchor's coordinate in chroma samples is s / (1 << c) per
 *                 axis, and the same bilinear expression runs on the (height >> cy) x (width >> cx) plane - rows clamped to it, a
 *                 panorama's columns wrapped modulo width >> cx; fill[k] where the anchor is not live.
 * Precision: the tile models' coordinates are certified to 1/1024 px per axis, so a sample is within T(R) = 1 + floor(R / 512) of the
 * definition, R the largest sample value of the source frame and the fills: 1 LSB for 8-bit samples, 2 for 10-bit samples stored low,
 * 128 for full 16-bit or high-aligned (P010) samples.  At the rim of a camera source a pixel within 1/512 px of the liveness edge may
 * be fill where the definition samples, or the reverse.
 * Arguments, layouts, defaults, PB_ERR_INVALID (checks, order and messages) and n_frames == 0: exactly pb_remap_planar's / pb_remap_nv12's.
 *   PB_ERR_UNSUPPORTED   nothing is written: whatever the nearest call refuses; plans without the bilinear mode's tables (created with
 *                        PB_PLAN_NO_BILINEAR and not given pb_plan_prepare(plan, PB_PLAN_BILINEAR) since, or whose coordinate table did
 *                        not fit); cube and equi-angular-cube sources (no interpolating tile kernel).
 * Asynchronous on `stream`, never allocates or synchronises (graph-capture safe).  The _supported calls: 1 / 0 / negative as above.
 * (The return type stands on a line of its own: tools that read the nearest calls' declarations as `int pb_remap_planar...(` and
 * `int pb_remap_nv12...(` keep finding exactly those.) */
int
pb_remap_planar_bilinear(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_planar_layout* src_layout,
                             const pb_planar_layout* dst_layout, int subsampling, int bytes_per_sample, const uint16_t fill[3], void* stream);
int
pb_remap_nv12_bilinear(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_nv12_layout* src_layout,
                           const pb_nv12_layout* dst_layout, int bytes_per_sample, const uint16_t fill_yuv[3], void* stream);
int
pb_remap_planar_bilinear_supported(const pb_plan* plan, int subsampling, int bytes_per_sample);
int
pb_remap_nv12_bilinear_supported(const pb_plan* plan, int bytes_per_sample);
/* Diagnostic, synchronous: what the fix-pixel path of pb_planar_bilinear_kernel meets in `plan`.  mix[0] = modelled tiles with fix pixels,
 * mix[1] = their fix pixels, mix[2] = of those the chroma anchors at PB_PLANAR_422 (an even column), mix[3] = at PB_PLANAR_420 (an even
 * row too).  All zero for a plan without the bilinear mode's tables. */
int pb_plan_video_bilinear_mix(const pb_plan* plan, long long mix[4]);

/* STITCHING video frames of a DOUBLE-FISHEYE source in ONE launch of the tile kernel pb_stitch_video_kernel whatever n_frames (ABI 5,
 * additive): the side-by-side double fisheye as NV12 / P010 (pb_stitch_nv12) or planar frames (pb_stitch_planar), the
 * destination in the same format.  The definition is written down in tests/stitch_video_ref.py.  With (il, ir, fl, fr) the reference's
 * taps and factors of an output pixel (DoubleCameraImage.process_coordinate_map; pb_index_map_i32 with weights: indices r * width + c
 * into the full frame, the right eye's already mirrored, -1 = that eye is black there) and
 *   blend(a_l, a_r) = cast((il < 0 ? 0.0 : a_l) * fl + (ir < 0 ? 0.0 : a_r) * fr) in float64, the cast NumPy's astype widened to the
 *                     sample: non-finite or |v| >= 2^31 gives 0, else truncate toward zero and keep the low 8 * S bits,
 *   plane 0       out[y][x] = blend(P0[r_l][c_l], P0[r_r][c_r]); fill[0] where both taps are -1.
 *   planes 1, 2   sample (i, j) (or the two members of a pair) is decided by its ANCHOR, output pixel (i << cy, j << cx), as in the nearest
 *                 calls: blend(Pk[r_l >> cy][c_l >> cx], Pk[r_r >> cy][c_r >> cx]) with the anchor's taps and factors; fill[k] where both
 *                 of the anchor's taps are -1.
 * Exact: with S = 1, 4:4:4 and fill (0, 0, 0) the three planes are the three channels of pb_remap_u8's output for the RGB image whose
 * channels are the source planes.  An eye that is black where the other is live contributes 0.0, as in the reference; the fill is used
 * only where nothing is live.  In the reference's half-degree safety zone beside the merge band a factor slightly exceeds 1: a bright
 * sample may wrap modulo 2^(8 * S) there (a 10-bit sample stored low wraps at 2^16) - the reference's quirk, reproduced.
 * Arguments, layouts, defaults, PB_ERR_INVALID (checks, order and messages) and n_frames == 0: exactly pb_remap_planar's / pb_remap_nv12's.
 * Frames need no alignment beyond one sample (one chroma pair for pb_stitch_nv12).
 *   PB_ERR_UNSUPPORTED   nothing is written: a source that is not a double fisheye (use pb_remap_planar / pb_remap_nv12); deferred plans,
 *                        PB_MODE_FAITHFUL, plans without both eyes' tile tables and a launch-order table (a geometry whose plan got
 *                        none), sources of 32768 px a side or more; frames whose byte span reaches 2^31.
 * Asynchronous on `stream`, never allocates or synchronises (graph-capture safe).  The _supported calls: 1 / 0 / negative as above. */
int
pb_stitch_planar(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_planar_layout* src_layout,
                 const pb_planar_layout* dst_layout, int subsampling, int bytes_per_sample, const uint16_t fill[3], void* stream);
int
pb_stitch_nv12(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_nv12_layout* src_layout,
               const pb_nv12_layout* dst_layout, int bytes_per_sample, const uint16_t fill_yuv[3], void* stream);
int
pb_stitch_planar_supported(const pb_plan* plan, int subsampling, int bytes_per_sample);
int
pb_stitch_nv12_supported(const pb_plan* plan, int bytes_per_sample);
/* Diagnostic, synchronous: what the waves of a stitch launch meet in `plan`, slot by slot of its launch-order table.  mix[0] = one-eye
 * (SOLO) slots, mix[1] / mix[2] / mix[3] = two-eye tiles of weight class UNIT / ROW / LAT, mix[4] = failed tiles, mix[5] = two-eye
 * tiles with fix pixels, mix[6] = their fix pixels, mix[7] = of those the chroma anchors at PB_PLANAR_422 (an even column), mix[8] = at
 * PB_PLANAR_420 (an even row too).  All zero for a plan without the double-fisheye tile tables. */
int pb_plan_stitch_tile_mix(const pb_plan* plan, long long mix[9]);

/* OPT-IN extension with no reference counterpart (the reference samples nearest-by-truncation only):
 * bilinear interpolation at the reference's pre-truncation coordinate (pixel k covers [k, k+1), centre
 * k + 0.5; taps clamped to the image, panorama columns wrap; round half to even).  Pixels the nearest mode
 * paints black stay black.  A double-fisheye source is the reference's blend (projection.py:439-460) of the two eyes'
 * bilinear samples (each eye sampled like a camera source on its half, rounded to uint8, then blended and cast as the
 * nearest mode does); it runs through the per-eye tile models like the nearest mode (ABI 3; pixels the models cannot serve
 * are recomputed by the float64 chain in the same call). */
int pb_remap_bilinear_u8(const pb_plan* plan, const uint8_t* src_dev, uint8_t* dst_dev, int n_frames,
                         size_t src_frame_stride, size_t dst_frame_stride, void* stream);

/* OPT-IN Catmull-Rom sampling (ABI 5, additive), no reference counterpart: the bilinear definition above with a 4 x 4
 * footprint.  s = f - 0.5, i0 = floor(s), t = s - i0; taps rows i0 - 1 .. i0 + 2 x columns j0 - 1 .. j0 + 2, clamped like bilinear's
 * (panorama columns wrap, an eye's taps stay in its half); Keys' cubic weights with a = -0.5; row sums, then the column sum; round half to
 * even, clipped to [0, 255] (the cubic overshoots).  Black exactly where the bilinear mode is black; a double-fisheye source blends the two
 * eyes' rounded samples like the reference.  pb_remap_bilinear_u8's contract: pb_remap_u8's argument checks and messages, asynchronous,
 * no allocation, no synchronisation (graph-capture safe).  Prepared single-source plans (AUTO / FAST, built with the bilinear mode's tables
 * - PB_PLAN_BILINEAR) take one tile-kernel launch per batch, float32 arithmetic on coordinates certified to 1/1024 px: within 1 LSB of the
 * definition.  Deferred plans, PB_MODE_FAITHFUL, plans without those tables and double-fisheye sources evaluate the definition per pixel in
 * float64 (its bytes exactly).  The supersampled entry points do not take this mode. */
int pb_remap_catmull_rom_u8(const pb_plan* plan, const uint8_t* src_dev, uint8_t* dst_dev, int n_frames,
                            size_t src_frame_stride, size_t dst_frame_stride, void* stream);

/* ROTATION TRACKS (ABI 5, additive): a batch in which every frame has rotations of its own - stabilising or reframing a
 * 360-degree video, a turntable - in ONE launch.  Frame f receives exactly the bytes the matching single-plan call (pb_remap_u8,
 * pb_remap_bilinear_u8, pb_remap_catmull_rom_u8 by `interpolation`) writes for frame f alone from a plan of the same dst and src in
 * PB_MODE_FAITHFUL whose rotation chain is this plan's own n_rot rotations followed by frame f's n_rot_per_frame.  Rotations are applied
 * one after another, arccos / atan2 between them, as Rotation.rotate_coordinate_map does (core/rotation.py:102-176); nothing is folded.
 * Nearest: the reference's own output for that chain; the interpolating modes: their float64 per-pixel definition.
 *   rot3x3_dev       DEVICE memory, 8-byte aligned: float64 [n_frames][n_rot_per_frame][9], row-major 3 x 3 = Rotation.rotation_matrix.
 *                    The kernel reads it when the stream runs the launch: it must stay alive and unchanged until then.
 *   interpolation    PB_INTERP_NEAREST, PB_INTERP_BILINEAR or PB_INTERP_CATMULL_ROM.
 * The plan's tables are never read (they are certified for another chain): a deferred plan, a prepared one, any mode, with or without the
 * bilinear mode's tables or device state are served alike - the float64 chain per pixel, the part no frame changes (the destination's
 * inverse projection, a cube destination's face rotation, the plan's own rotations) once per pixel and chunk of frames.  All source and
 * destination kinds.  pb_remap_u8's contract: its argument checks and messages, strides in bytes (0: packed), asynchronous on `stream`;
 * never allocates, never synchronises, never copies the table (graph-capture safe).  PB_ERR_INVALID before any launch: a null or misaligned
 * table, n_rot_per_frame < 1, n_rot + n_rot_per_frame > PB_MAX_ROTATIONS, an interpolation outside the three.  n_frames == 0: PB_OK, no launch. */
#define PB_INTERP_NEAREST 0
#define PB_INTERP_BILINEAR 1
#define PB_INTERP_CATMULL_ROM 2
int pb_remap_track_u8(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, int interpolation, const uint8_t* src_dev, uint8_t* dst_dev,
                      int n_frames, size_t src_frame_stride, size_t dst_frame_stride, void* stream);

/* ROTATION TRACKS OF GREY, RGBA AND 16-BIT FRAMES (ABI 5, additive): pb_remap_track_u8 for frames of `channels` samples of
 * `sample_bytes` bytes a pixel, channels in {1, 2, 3, 4}, sample_bytes in {1, 2} - a pixel of B = channels * sample_bytes bytes, B in
 * {1, 2, 3, 4, 6, 8} like pb_remap_px's.  Frame f receives exactly the bytes the materialised-map calls write for that frame alone:
 * pb_coordmap_f64, pb_rotate_f64 by this plan's own n_rot rotations and then by the n_rot_per_frame matrices of table entry f (one after
 * another, nothing folded), then by `interpolation`
 *   PB_INTERP_NEAREST       pb_index_from_map_i32 + pb_gather_px - for a single source the reference's own image[positions], whatever the
 *                           pixel holds; a double fisheye: pb_gather_blend_u8, the reference's blend per byte;
 *   PB_INTERP_BILINEAR      pb_sample_map_bilinear_px;
 *   PB_INTERP_CATMULL_ROM   pb_sample_map_catmull_rom_px - the float64 definitions per channel, rounded half to even and clamped to the
 *                           sample type's range; a double fisheye samples each eye on its half and blends to uint8.
 * All single source kinds and all destination kinds; a double-fisheye source with sample_bytes == 1.  channels == 3 with sample_bytes == 1
 * is exactly pb_remap_track_u8 (same kernels, same bytes).  Like every track call it reads nothing of the plan but its parameters: deferred,
 * prepared, any mode are served alike.  pb_remap_track_u8's contract with the pixel size: pb_remap_px's frame checks and messages first
 * (frame pointers and strides multiples of min(4, B & -B) bytes), then pb_remap_track_u8's table checks, then the interpolation's;
 * then PB_ERR_INVALID for channels or sample_bytes outside their sets; then PB_ERR_UNSUPPORTED, nothing written, for a double-fisheye
 * source with sample_bytes == 2 (the reference narrows that blend to uint8 modulo 256: use pb_sample_map_*_px / pb_gather_blend_u8 per
 * frame).  n_frames == 0: PB_OK, no launch.  Asynchronous on `stream`; never allocates, never synchronises, never copies the table
 * (graph-capture safe).  Byte offsets inside a frame are 64-bit: no frame size is refused.
 * pb_remap_track_px_supported: 1 when pb_remap_track_px takes `plan` with this format, 0 when it would return PB_ERR_UNSUPPORTED, negative
 * on bad arguments. */
int pb_remap_track_px(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, int interpolation, const void* src_dev, void* dst_dev,
                      int n_frames, size_t src_frame_stride, size_t dst_frame_stride, int channels, int sample_bytes, void* stream);
int pb_remap_track_px_supported(const pb_plan* plan, int channels, int sample_bytes);

/* BILINEAR AND CATMULL-ROM SAMPLING OF GREY, RGBA AND 16-BIT FRAMES (ABI 5, additive): the interpolating modes of
 * pb_remap_bilinear_u8 / pb_remap_catmull_rom_u8 for frames of `channels` samples of `sample_bytes` bytes a pixel - channels in {1, 2, 3, 4},
 * sample_bytes in {1, 2} (uint8 / uint16, native byte order), tightly packed rows - in ONE launch of the tile kernel pb_px_interp_kernel
 * whatever n_frames, without a coordinate map.  The definitions are those modes' own on an image of that layout (per channel; the cubic
 * clipped to the sample type's range; zeros where the pixel is not live); the tile kernel's coordinates are certified to 1/1024 px per
 * axis, so with R the largest sample value of the source frame every sample is within 1 + R / 512 (bilinear) or
 * 1 + floor(15 R / 4096 + R / 2^18) (Catmull-Rom) of the definition, as for uint8 RGB with R = 255.
 * interpolation is PB_INTERP_BILINEAR or PB_INTERP_CATMULL_ROM.  channels 3 of one byte is pb_remap_bilinear_u8 / pb_remap_catmull_rom_u8
 * itself, on every plan those take.  The checks, in this order:
 *   pb_remap_px's frame checks and messages with bytes_per_px = channels * sample_bytes (frame pointers and strides multiples of
 *   min(4, B & -B) bytes; the weakest alignment while the format is not known to be valid);
 *   PB_ERR_INVALID        an interpolation other than the two (PB_INTERP_NEAREST: the message names pb_remap_px);
 *   PB_ERR_INVALID        channels or sample_bytes outside their sets;
 *   PB_ERR_UNSUPPORTED    nothing is written and nothing launched - the plans pb_remap_px refuses (deferred plans, PB_MODE_FAITHFUL,
 *                         double-fisheye sources, plans without device state, sources of 32768 px a side or more, frames of 2^31 bytes or
 *                         more); plans without the bilinear mode's tables (call pb_plan_prepare(plan, PB_PLAN_BILINEAR)); cube and
 *                         equi-angular-cube sources (use pb_sample_map_bilinear_px / pb_sample_map_catmull_rom_px).
 * A plan that WAS prepared with PB_PLAN_BILINEAR and whose coordinate tables cannot exist (a source of one or two pixels, of 2^18 px a
 * side or more, a GiB of coordinates) is served per pixel from the plan's float64 chain - the definition itself, in one launch.
 * n_frames == 0 is PB_OK and launches nothing.  Asynchronous on `stream`; never allocates or synchronises, so it can be captured into a graph.
 * pb_remap_interp_px_supported: 1 when pb_remap_interp_px takes `plan` with this format and interpolation, 0 when it would return
 * PB_ERR_UNSUPPORTED, negative on bad arguments. */
int
pb_remap_interp_px(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, size_t src_frame_stride,
                   size_t dst_frame_stride, int channels, int sample_bytes, int interpolation, void* stream);
int
pb_remap_interp_px_supported(const pb_plan* plan, int channels, int sample_bytes, int interpolation);
/* Diagnostic: what a pb_remap_interp_px call with these arguments launches on `plan` - 1 the tile kernel pb_px_interp_kernel, 2 the float64
 * chain per pixel (a prepared plan whose coordinate tables cannot exist), 3 the uint8 RGB call it delegates to, 0 nothing
 * (PB_ERR_UNSUPPORTED); negative on bad arguments, as pb_remap_interp_px_supported. */
int
pb_plan_px_interp_route(const pb_plan* plan, int channels, int sample_bytes, int interpolation);

/* BILINEAR AND CATMULL-ROM SAMPLING OF FLOAT16 AND FLOAT32 FRAMES (ABI 5, additive): HDR panoramas, depth and disparity
 * planes, flow fields, float mattes - frames of `channels` IEEE samples a pixel, channels in {1, 2, 3, 4}, sample_bytes 2 (binary16) or 4
 * (binary32), native byte order, tightly packed rows - in ONE launch of the tile kernel pb_pxf_interp_kernel whatever n_frames, without a
 * coordinate map.  The pixel is B = channels * sample_bytes bytes: {2, 4, 6, 8} or {4, 8, 12, 16}.
 * The definition (tests/pxf_ref.py) is the integer modes' up to the sum: per channel V = top + ty (bot - top) with top = a + tx (b - a)
 * (bilinear), or Keys' cubic with a = -0.5 over the 4 x 4 footprint, row sums first (Catmull-Rom); rows clamped, a panorama's columns
 * wrapped, a camera's clamped.  V is NOT rounded to an integer and NOT clipped - the cubic's overshoot and negative lobes are kept - and is
 * narrowed once to the sample type, round to nearest even (a half result beyond 65504 is infinity, as IEEE says).  A pixel that is not
 * live is +0.0 in every channel (all bytes zero).  A NaN or an infinity among a pixel's taps (its clamped and wrapped 2 x 2 or 4 x 4
 * footprint) leaves that pixel's value unspecified; it affects no other pixel and never makes a dead pixel anything but +0.0.
 * Precision: the tile coordinates are certified to 1/1024 px per axis and all arithmetic is float32.  With a frame's samples in [L, U],
 * D = U - L, M = max(|L|, |U|), u = 2^-24 for float32 and 2^-11 for float16 frames, every sample is within D / 512 + M 2^-20 + M u
 * (bilinear) or 15 D / 4096 + M 2^-18 + 1.5625 M u (Catmull-Rom) of the definition's exact value.
 * The checks, in pb_remap_interp_px's order:
 *   pb_remap_px's frame checks and messages with bytes_per_px = channels * sample_bytes, 12 and 16 being pixel sizes for this call only
 *   (frame pointers and strides multiples of min(4, B & -B) bytes - 4 for 12 and 16; the weakest alignment while the format is not known
 *   to be valid);
 *   PB_ERR_INVALID        an interpolation other than PB_INTERP_BILINEAR / PB_INTERP_CATMULL_ROM (PB_INTERP_NEAREST: the message names
 *                         pb_remap_px, which moves float pixels of up to 8 bytes as bytes);
 *   PB_ERR_INVALID        channels or sample_bytes outside their sets;
 *   n_frames == 0         PB_OK, no launch;
 *   PB_ERR_UNSUPPORTED    nothing is written and nothing launched - the plans pb_remap_px refuses (deferred plans, PB_MODE_FAITHFUL,
 *                         double-fisheye sources, plans without device state, sources of 32768 px a side or more); frames of 2^31 bytes
 *                         or more; plans never prepared for the bilinear mode (call pb_plan_prepare(plan, PB_PLAN_BILINEAR)); cube and
 *                         equi-angular-cube sources; and plans that WERE prepared for it whose coordinate tables cannot exist (a source
 *                         of one or two pixels, of 2^18 px a side or more, a GiB of coordinates): pb_remap_interp_px serves those from
 *                         the float64 chain, and no such per-pixel kernel exists for float samples.
 * Asynchronous on `stream`; never allocates or synchronises, so it can be captured into a graph.
 * pb_remap_interp_pxf_supported: 1 when pb_remap_interp_pxf takes `plan` with this format and interpolation, 0 when it would return
 * PB_ERR_UNSUPPORTED, negative on bad arguments.
 * PB_INTERP_PXF is defined (empty) by every header that declares the two: a caller that must also build against an earlier header of
 * ABI 5 can test for it. */
#define PB_INTERP_PXF
int PB_INTERP_PXF pb_remap_interp_pxf(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, size_t src_frame_stride,
                                      size_t dst_frame_stride, int channels, int sample_bytes, int interpolation, void* stream);
int PB_INTERP_PXF pb_remap_interp_pxf_supported(const pb_plan* plan, int channels, int sample_bytes, int interpolation);

/* ROTATION TRACKS FOR 4:2:0 SEMI-PLANAR VIDEO FRAMES (ABI 5, additive): NV12 / P010 / P016 frames, every frame with rotations
 * of its own, both planes of all frames in as many launches as pb_remap_track_u8 makes.  Frame f receives exactly pb_remap_nv12's
 * definition above with idx the index map of the chain "this plan's own n_rot rotations followed by the n_rot_per_frame matrices of table
 * entry f", applied one after another as for pb_remap_track_u8 (nothing folded): luma like a grey image, the pair of an output 2 x 2 block
 * from the source position of the block's top-left pixel, and only that anchor decides between pair and fill.  Equivalently: what
 * pb_remap_nv12 writes for frame f alone from a prepared plan of that whole chain, wherever pb_remap_nv12_supported.
 *   rot3x3_dev, n_rot_per_frame   pb_remap_track_u8's table: device memory, 8-byte aligned, read when the stream runs the launch.
 *   layouts, bytes_per_sample, fill_yuv   pb_remap_nv12's.  Padding bytes are neither read nor written.
 * The plan's tables are never read: a deferred plan, a prepared one and any mode are served alike.
 *   PB_ERR_INVALID       before any launch, in this order: pb_remap_nv12's checks (null plan or frames, a negative count, bytes_per_sample,
 *                        odd dimensions, the layouts, pointer alignment), then pb_remap_track_u8's (a null or misaligned table,
 *                        n_rot_per_frame < 1, n_rot + n_rot_per_frame > PB_MAX_ROTATIONS).  n_frames == 0: PB_OK, no launch, no device.
 *   PB_ERR_UNSUPPORTED   nothing is written: a double-fisheye source (its blend is sample-typed: convert to RGB8 and use
 *                        pb_remap_track_u8); frames whose byte span reaches 2^31 or sources of 32768 px a side or more (a plan per frame,
 *                        pb_index_map_i32 and a gather of the two planes).
 * Asynchronous on `stream`; never allocates, never synchronises, never copies the table (graph-capture safe). */
int pb_remap_track_nv12(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames,
                        const pb_nv12_layout* src_layout, const pb_nv12_layout* dst_layout, int bytes_per_sample, const uint16_t fill_yuv[3],
                        void* stream);

/* OPT-IN: BILINEAR ROTATION TRACKS FOR VIDEO FRAMES (ABI 5, additive): pb_remap_track_nv12's and pb_remap_track_planar's
 * arguments and launches, sampled bilinearly - smooth stabilised, levelled or reframed video without a plan per frame.  Frame f receives
 * the definition of pb_remap_planar_bilinear / pb_remap_nv12_bilinear above (tests/video_bilinear_ref.py: plane 0 the grey bilinear sample,
 * planes 1 and 2 decided by their anchor, chroma co-sited top-left, the anchor's coordinate halved where the plane is subsampled) with f and
 * "live" those of the float64 chain "this plan's own n_rot rotations followed by the n_rot_per_frame matrices of table entry f", applied
 * one after another as for pb_remap_track_u8 (nothing folded).  A panorama source is live where the entry is not invalid and finite, a
 * camera source additionally where 0 <= fy < height and 0 <= fx < width.
 * Precision: the kernel (pb_track_video_bilinear_kernel) holds the chain's float64 coordinate itself, not a certified model, and evaluates
 * the three lerps in float64 in the definition's order: every sample is the definition's bytes exactly, for 8-, 10- and 16-bit samples
 * alike.  There is no tolerance and no edge band.
 * The plan's tables are never read: a deferred plan, a prepared one, with or without the bilinear mode's tables, and any mode are served
 * alike.
 *   PB_ERR_INVALID       checks, order and messages are the nearest tracked calls': pb_remap_nv12's / pb_remap_planar's, then
 *                        pb_remap_track_u8's table checks.  n_frames == 0: PB_OK, no launch, no device.
 *   PB_ERR_UNSUPPORTED   nothing is written: a double-fisheye source; cube and equi-angular-cube sources (the definition covers panorama
 *                        and camera sources, as for the untracked bilinear video calls); frames whose byte span reaches 2^31 or sources
 *                        of 32768 px a side or more.
 * Asynchronous on `stream`; never allocates, never synchronises, never copies the table (graph-capture safe); one launch per 65535 chunks
 * of frames.  (The return type stands on a line of its own, as for the bilinear video calls above.) */
int
pb_remap_track_nv12_bilinear(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames,
                                 const pb_nv12_layout* src_layout, const pb_nv12_layout* dst_layout, int bytes_per_sample, const uint16_t fill_yuv[3],
                                 void* stream);
int
pb_remap_track_planar_bilinear(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames,
                                   const pb_planar_layout* src_layout, const pb_planar_layout* dst_layout, int subsampling, int bytes_per_sample,
                                   const uint16_t fill[3], void* stream);

/* ROTATION TRACKS FOR DOUBLE-FISHEYE VIDEO FRAMES (ABI 5, additive): a batch of NV12 / P010 (pb_track_stitch_nv12) or planar
 * frames (pb_track_stitch_planar) of a side-by-side double fisheye, every frame with rotations of its own, stitched in ONE launch of
 * pb_track_stitch_kernel per 65535 chunks of frames, every plane written - a stabilised, horizon-levelled panorama straight from a
 * decoder's surfaces.  The argument lists are pb_remap_track_planar's and pb_remap_track_nv12's.  Frame f receives the definition of
 * pb_stitch_planar / pb_stitch_nv12 above (tests/stitch_video_ref.py), unchanged, with (il, ir, fl, fr) the taps and factors of the float64
 * chain "this plan's own n_rot rotations followed by the n_rot_per_frame matrices of table entry f", applied one after another as for
 * pb_remap_track_u8 (nothing folded).  Equivalently: what pb_stitch_planar / pb_stitch_nv12 write for frame f alone from a prepared plan of
 * that whole chain, byte for byte; and with S = 1, 4:4:4 and fill (0, 0, 0) the three planes are the three channels of pb_remap_track_u8's
 * frame f.  There is no tolerance.  An invalid destination pixel has both taps -1 and takes the fill; a black eye contributes 0.0; only
 * the anchor decides a chroma sample, with the anchor's factors.
 * The plan's tables are never read: a deferred plan, a prepared one and any mode are served alike.
 *   PB_ERR_INVALID       before any launch, in this order: pb_remap_planar's / pb_remap_nv12's checks, then pb_remap_track_u8's table
 *                        checks, with their messages.  n_frames == 0: PB_OK, no launch, no device.
 *   PB_ERR_UNSUPPORTED   nothing is written: a source that is not a double fisheye (use pb_remap_track_planar / pb_remap_track_nv12);
 *                        frames whose byte span reaches 2^31; sources of 32768 px a side or more.
 * Asynchronous on `stream`; never allocates, never synchronises, never copies the table (graph-capture safe). */
int pb_track_stitch_planar(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames,
                           const pb_planar_layout* src_layout, const pb_planar_layout* dst_layout, int subsampling, int bytes_per_sample,
                           const uint16_t fill[3], void* stream);
int pb_track_stitch_nv12(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames,
                         const pb_nv12_layout* src_layout, const pb_nv12_layout* dst_layout, int bytes_per_sample, const uint16_t fill_yuv[3],
                         void* stream);

/* SUPERSAMPLED REMAPPING (ABI 5, additive).  Output pixel (i, j) is, per channel, the round-half-to-even mean of the n x n block
 * S[n i : n i + n, n j : n j + n] of S = the remap of the n x destination: the same kind and lens with image (n H, n W) and, for a camera,
 * magnitude n x (a double fisheye's magnitude = height / 2 scales by itself); n in {2, 4}, a power of two, so its f_distance is exactly
 * n x f_distance.  In integers (N = n^2, k = log2 N): q = sum >> k, r = sum & (N - 1), out = q + (r > N/2 || (r == N/2 && (q & 1))).
 *   pb_remap_ss_u8        `plan` is an ordinary plan of the n x destination (dimensions divisible by n); dst receives (H, W, 3) frames.
 *                         interpolation: PB_INTERP_NEAREST (pb_remap_u8's samples) or PB_INTERP_BILINEAR (pb_remap_bilinear_u8's).  Prepared
 *                         single-source plans in nearest mode (AUTO / FAST, 16-byte aligned frames) take the FUSED kernel: one launch per
 *                         batch, the n x n blocks reduced in registers, only the H x W output stored.  Everything else (double-fisheye
 *                         sources, bilinear mode, deferred plans, PB_MODE_FAITHFUL / PB_MODE_FAST_DIRECT, unaligned frames, PB_SS_GENERIC)
 *                         takes the GENERIC path: frame by frame, the n x remap into `workspace_dev`, then pb_box_reduce.  Never allocates,
 *                         never synchronises (graph-capture safe): the caller provides the workspace.
 *   pb_remap_ss_workspace the workspace bytes a call needs: 0 when the fused kernel takes it (source pointer and stride - a packed frame's
 *                         size when 0 - multiples of 16 bytes), else one n x frame.
 *   pb_box_reduce         the generic kernel on its own: (n_frames, n height, n width, channels) samples of sample_bytes (1 or 2) bytes ->
 *                         (n_frames, height, width, channels), tightly packed.
 * n outside {2, 4}, indivisible dimensions and n x frames beyond the projection limit (n^2 h w < 2^29) are PB_ERR_INVALID. */
#define PB_SS_GENERIC 1u /* (PB_INTERP_NEAREST, PB_INTERP_BILINEAR: above) */
int pb_remap_ss_workspace(const pb_plan* plan, int n, int interpolation, unsigned flags, size_t* bytes);
int pb_remap_ss_u8(const pb_plan* plan, int n, int interpolation, const uint8_t* src_dev, uint8_t* dst_dev, int n_frames, size_t src_frame_stride,
                   size_t dst_frame_stride, void* workspace_dev, size_t workspace_bytes, unsigned flags, void* stream);
int pb_box_reduce(const void* src_dev, void* dst_dev, int height, int width, int channels, int sample_bytes, int n, int n_frames, void* stream);

/* Integer coordinate map: for camera / pano sources idx_dev is int32 [H*W], the
 * linear source pixel index (row * src_width + col) or -1 where the output is
 * black.  For a double source idx_dev is int32 [2][H*W] (left-eye index, then
 * right-eye index, both into the full side-by-side frame) and, when weights_dev
 * is not NULL, float64 [2][H*W] receives the two blend factors
 * (projection.py:439-457). */
int pb_index_map_i32(const pb_plan* plan, int32_t* idx_dev, double* weights_dev, void* stream);

/* ---- multi-GPU: one process per GPU (SURVEY 8 e; ABI 3) ------------------------------------------------------------------
 * Frames are independent: a batch shards contiguously over the ranks and no pixel crosses a link.  The ONE data-path collective
 * is the RCCL broadcast (ncclBroadcast over xGMI inside a node) of the parameter block - both projections with the host-side
 * f_distance bits, the rotation matrices - from the root rank, so every device computes with identical bits; each rank then
 * creates its own plan (pb_plan_create on its device).  The reference has no counterpart (single process, no collective);
 * these entry points are what a non-Python host binds where the Python package uses torch.distributed
 * (photonbend_amd/parallel.py: same block layout).  librccl.so.1 is loaded at first use; PB_ERR_UNSUPPORTED without it.
 *   pb_comm_unique_id   rank 0 makes the 128-byte rendezvous id (ncclGetUniqueId); the launcher hands it to the other ranks
 *   pb_comm_init        collective: every rank, on ITS current device (ncclCommInitRank)
 *   pb_bcast_params     collective: root's dst / rot3x3[9 * n_rot] / n_rot / src overwrite everyone else's (rot3x3 must hold
 *                       9 * PB_MAX_ROTATIONS doubles); synchronises `stream`.  A polynomial lens travels as its coefficients: every rank
 *                       registers them and finds its OWN id in the pb_proj it gets back.  PRECONDITION: non-null pointers and a root inside
 *                       [0, n_ranks) on EVERY rank - those are checked before anyone enters the collective and must not differ
 *                       between ranks; everything only the root can know (its n_rot, its upload) travels WITH the broadcast: an
 *                       invalid root request makes every rank return PB_ERR_INVALID together, none is left waiting
 *   pb_shard_range      first = rank * q + min(rank, r), count = q + (rank < r)  (q, r = divmod(n_items, n_ranks))
 *   pb_remap_batch_sharded  remaps THIS rank's share of a batch of n_frames_total frames: its count frames, resident in its own
 *                       buffers from src_dev / dst_dev on (frame k of the share = batch frame first + k); one pb_remap_u8 */
typedef struct pb_comm pb_comm;
int pb_comm_unique_id(void* id128);
int pb_comm_init(int n_ranks, int rank, const void* id128, pb_comm** out);
int pb_comm_destroy(pb_comm* comm);
int pb_comm_rank(const pb_comm* comm, int* n_ranks, int* rank);
int pb_bcast_params(pb_comm* comm, pb_proj* dst, double* rot3x3, int* n_rot, pb_proj* src, int root, void* stream);
int pb_shard_range(int n_items, int n_ranks, int rank, int* first, int* count);
int pb_remap_batch_sharded(const pb_comm* comm, const pb_plan* plan, const uint8_t* src_dev, uint8_t* dst_dev, int n_frames_total,
                           size_t src_frame_stride, size_t dst_frame_stride, int* first_out, int* count_out, void* stream);

/* ---- materialised coordinate-map API (protocol compatibility) ---------
 * The float64 values are the reference's BITS as computed on x86-64 with FMA and AVX512_SKX, glibc 2.35, NumPy 2.2.6 (the platform of
 * tests/golden/): the device runs that platform's sin / cos / sincos / atan2 and NumPy's arcsin / arccos / arctan / tan restated bit
 * for bit (csrc/pb_math_glibc.hpp, csrc/pb_math_np.hpp); the same functions define every index map and remap. */
int pb_coordmap_f64(const pb_proj* dst, double* map_dev, void* stream);
/* Zeroes lat/lon of invalid pixels IN map_in_dev (rotation.py:119-125), like the
 * reference; map_out_dev must not alias map_in_dev. */
int pb_rotate_f64(const double* rot3x3, double* map_in_dev, double* map_out_dev, int height, int width,
                  void* stream);
/* map is (height, width, 3); PB_KIND_PANO zeroes invalid lat/lon in map_dev
 * (projection.py:534-536). */
int pb_sample_map_u8(const pb_proj* src, double* map_dev, int height, int width, const uint8_t* src_dev,
                     uint8_t* dst_dev, void* stream);

/* The sampling half of process_coordinate_map without the gather (projection.py:197-260 camera, :408-462 double,
 * :515-547 panorama): coordinate map (height, width, 3) -> int32 source index per pixel (-1 = black; a double source:
 * [2][height*width], left eye then right eye, and weights_dev float64 [2][height*width] when not NULL).  PB_KIND_PANO
 * zeroes invalid lat/lon in map_dev like the reference.  dist_l_dev / dist_r_dev (float64 [height*width], optional):
 * forward_lens(latitude) * f_distance evaluated by the host for a PB_LENS_CUSTOM source (the right eye's plane is
 * forward_lens(pi - latitude) * f_distance); with them the built-in forward lens is not used.
 * Together with pb_gather_px / pb_gather_blend_u8 this serves every image the reference accepts but the fused
 * uint8 RGB path does not: grey (H, W), RGBA (H, W, 4), 16-bit samples - the reference fancy-indexes whatever array
 * it is given (projection.py:234-243, :545-546). */
int pb_index_from_map_i32(const pb_proj* src, double* map_dev, int height, int width, const double* dist_l_dev,
                          const double* dist_r_dev, int32_t* idx_dev, double* weights_dev, void* stream);
/* The opt-in bilinear mode on a MATERIALISED map and on ANY image (ABI 5): what process_coordinate_map(map, interpolation="bilinear")
 * runs when the map is an array (looked at or edited between the stages; a destination Lens of user callables), when the image is not
 * uint8 RGB (grey, RGBA, 16-bit samples) or when the source Lens is made of user callables (dist_l_dev / dist_r_dev as in
 * pb_index_from_map_i32).  The definition of pb_remap_bilinear_u8, evaluated per pixel in float64 from the map's (lat, lon, invalid):
 * taps floor(f - 0.5), + 1 clamped to the image (a panorama's columns wrap, an eye's taps stay in its half), round half to even,
 * clamped to the sample range; PB_KIND_PANO zeroes invalid lat/lon in map_dev like the reference.  img_dev: (h, w, channels)
 * samples of sample_bytes (1 or 2) bytes; out_dev: (height, width, channels) of the same sample type - a double-fisheye source
 * returns uint8 like the reference's (left * fl + right * fr).astype(np.uint8) (projection.py:447-460).
 * Replaces: nothing in the reference (it truncates: projection.py:254-259, :545); completes the ProjectionImage protocol
 * (projection.py:40-66, :197-245, :515-547) for the opt-in mode.  pb_sample_map_bilinear_u8 = 3 channels of 1 byte. */
int pb_sample_map_bilinear_px(const pb_proj* src, double* map_dev, int height, int width, const double* dist_l_dev, const double* dist_r_dev,
                              const void* img_dev, void* out_dev, int channels, int sample_bytes, void* stream);
int pb_sample_map_bilinear_u8(const pb_proj* src, double* map_dev, int height, int width, const uint8_t* src_dev, uint8_t* dst_dev, void* stream);
/* The opt-in Catmull-Rom mode (pb_remap_catmull_rom_u8's definition) on a MATERIALISED map and on ANY image: pb_sample_map_bilinear_px's
 * arguments, checks and side effects, evaluated per pixel in float64 in the definition's order - its bytes exactly. */
int pb_sample_map_catmull_rom_px(const pb_proj* src, double* map_dev, int height, int width, const double* dist_l_dev, const double* dist_r_dev,
                                 const void* img_dev, void* out_dev, int channels, int sample_bytes, void* stream);
/* dst[p] = idx[p] < 0 ? 0 : src[idx[p]], bytes_per_px bytes each (1..64). */
int pb_gather_px(const int32_t* idx_dev, const void* src_dev, void* dst_dev, size_t n_px, int bytes_per_px, void* stream);
/* The double-fisheye blend for `channels` interleaved samples of 1 or 2 bytes (unsigned): per channel
 * (left * fl + right * fr).astype(uint8) - uint8 output whatever the input width, like the reference
 * (projection.py:447-460).  idx2_dev / weights2_dev as written by pb_index_map_i32 / pb_index_from_map_i32. */
int pb_gather_blend_u8(const int32_t* idx2_dev, const double* weights2_dev, const void* src_dev, uint8_t* dst_dev,
                       size_t n_px, int channels, int sample_bytes, void* stream);

/* map_projection (projection.py:550-599): coordinate map -> colour map (red = latitude stretched to
 * 0..255 over the valid pixels, green = longitude * 255 / 2pi, blue = invalid * 255).  Zeroes invalid
 * lat/lon in map_dev like the reference.  workspace24_dev: 24 bytes of device scratch; after the call it
 * holds {min key, max key, number of valid pixels} (uint64 each). */
int pb_map_projection_u8(double* map_dev, int height, int width, uint8_t* out_dev, void* workspace24_dev, void* stream);

/* ---- deterministic synthetic frames (bench + tests) -------- */
/* circle_mask: 0 none, 1 black outside the inscribed circle, 2 black outside
 * the two side-by-side inscribed circles. */
int pb_synth_frame_u8(uint8_t* frame_dev, int height, int width, uint32_t frame, uint32_t seed, int circle_mask,
                      void* stream);

/* ---- plumbing for hosts without their own device allocator ------------ */
int pb_malloc(void** dev_ptr, size_t bytes);
int pb_free(void* dev_ptr);
int pb_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream);
int pb_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream);
int pb_memset(void* dst_dev, int value, size_t bytes, void* stream);
int pb_stream_create(void** stream);
int pb_stream_destroy(void* stream);
int pb_stream_sync(void* stream);
int pb_event_create(void** event);
int pb_event_destroy(void* event);
int pb_event_record(void* event, void* stream);
int pb_event_sync(void* event);
int pb_event_elapsed_ms(void* start, void* stop, float* ms);
/* ABI 4: what a host that moves frames between ITS memory and the device needs beyond the above (the reference's contract is
 * ndarray in, fresh ndarray out: core/__init__.py:66-92; the Python package's NumPy path is built on these, without PyTorch).
 *   pb_device_count / pb_set_device / pb_get_device   the device ordinals pb_init takes
 *   pb_device_sync          hipDeviceSynchronize
 *   pb_stream_wait_event    work queued on `stream` after this call waits for `event` (cross-stream ordering: upload -> remap -> download)
 *   pb_host_alloc / _free   page-locked host memory (hipHostMalloc): DMA reads / writes it without a staging copy
 *   pb_host_register / _unregister   page-lock memory the CALLER allocated (hipHostRegister) for as long as it is registered; the
 *                           caller must unregister before the memory is freed or unmapped */
int pb_device_count(int* n);
int pb_set_device(int device);
int pb_get_device(int* device);
int pb_device_sync(void);
int pb_stream_wait_event(void* stream, void* event);
int pb_host_alloc(void** host_ptr, size_t bytes);
int pb_host_free(void* host_ptr);
int pb_host_register(void* host_ptr, size_t bytes);
int pb_host_unregister(void* host_ptr);
/* measurement utility: a plain 16-byte-per-lane device copy (pointers and size multiples of 16) - the practical
 * HBM ceiling bench.py reports next to the remap kernel */
int pb_stream_copy(void* dst_dev, const void* src_dev, size_t bytes, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* PHOTONBEND_HIP_H */
