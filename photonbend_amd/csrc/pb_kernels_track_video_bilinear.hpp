// pb_kernels_track_video_bilinear.hpp - BILINEAR ROTATION TRACKS FOR VIDEO FRAMES (pb_remap_track_planar_bilinear,
// pb_remap_track_nv12_bilinear): planar 4:4:4 / 4:2:2 / 4:2:0 frames and NV12 / P010, every frame with rotations of its own,
// the three planes of every frame in one launch, sampled bilinearly.
//
// The definition is tests/video_bilinear_ref.py's with, for frame f, the (fy, fx, live) of the float64 chain "the plan's own
// rotations followed by frame f's" (pb_kernels_track.hpp: one after another, nothing folded):
//   live          not invalid and finite; a camera source additionally 0 <= fy < h and 0 <= fx < w.
//   plane 0       s = f - 0.5, i0 = floor(s), t = s - i0, taps i0, i0 + 1 per axis, rows clamped, a panorama's columns wrapped, a camera's
//                 clamped; top = a + tx (b - a), bot likewise, rint(top + ty (bot - top)); fill[0] where the pixel is not live.
//   planes 1, 2   sample (i, j) belongs to its ANCHOR, output pixel (i << cy, j << cx); chroma is co-sited top-left, so the anchor's
//                 coordinate in chroma sample units is s / (1 << c) per axis: the same expression on the (h >> cy, w >> cx) plane;
//                 fill[k] where the anchor is not live.  Only the anchor decides.
// The kernel holds the chain's float64 coordinate itself - no certified model - and evaluates the three lerps in float64 in the
// definition's order under the build's -ffp-contract=off: the result is the definition's bytes exactly, for 8-, 10- and 16-bit samples
// alike (the uint8 routes' float32 taps are not exact for 16-bit samples and are not used).  The plan's tables are never read.
//
// pb_track_video_bilinear_kernel<S, SRC_KIND, PAIRS> has pb_track_video_kernel's structure - the skeleton of pb_kernels_track.hpp, a
// work-item owns PB_PX = 4 consecutive pixels of ONE row.
//   coordinate    a panorama's through pb_src_pretrunc; a camera's through pb_src_pretrunc_sc with the sine and cosine of pb_expi_np -
//                 np.exp(lon * 1j), the definition's own (pb_sample_map_interp_px computes it so): pb_src_pretrunc's plain sincos is the
//                 model builders' and differs from it in the last bit.
//   PAIRS false   three planes; the subsampling is a RUN-TIME, wave-uniform (cx, cy), for pb_track_video_kernel's reason.
//   PAIRS true    NV12 / P010 at 4:2:0: planes 1 and 2 are the interleaved (U, V) plane, one 2 * S-byte load per chroma tap, pair stores.
//                 The layout travels in the same PbPlanar: o1 = the pair plane's offset, cpitch = its pitch, o2 unused.
//   taps          each loaded with exactly its S (or 2 * S) bytes.  Rows and columns are clamped for EVERY tap, a panorama's columns
//                 wrapped first (pb_vbil_rc: once suffices - the chain ends in a rotation, so lon comes from atan2 and a live s lies
//                 in [-0.5, w - 0.5], on the chroma plane in [-0.25, w / 2 - 0.25]): no load leaves its plane.  A pixel that is not live
//                 samples at s = (0, 0) and takes the fill after the loads.
//   chroma        a quad starts at a multiple of four, so on a row with (y & cy) == 0 its pixels k with (k & cx) == 0 are anchors, and the
//                 work-item already holds their coordinate: chroma costs no second chain.
//   stores        pb_track_video_store's, U in p1 and V in p2.  Padding between rows, planes and frames is neither read nor written.
//
// Limits: the nearest track kernels' (32-bit byte offsets inside a frame, sources below 32768 px a side).
// grid: (quads of a frame / PB_BLOCK, chunks of fpc frames).
#pragma once
#include "pb_kernels_planar_bilinear.hpp"
#include "pb_kernels_track_video.hpp"

// waves per SIMD the kernel is compiled for.  What the build gave at each bound tried, quads of four pixels throughout:
//   8       panorama source 63 VGPRs, 78 scalar registers, no scratch, eight waves; camera source 63 VGPRs and 20 bytes of scratch
//   6, 4    no scratch for either: 63 (panorama) and 67 (camera) VGPRs, 106 scalar registers, the compiler takes seven waves
// So a panorama source is held to eight and a camera source gets the budget of four: no frame-loop kernel of this library spills.
#ifndef PB_TVB_WPE
#define PB_TVB_WPE(kind) ((kind) == PB_KIND_PANO ? 8 : 4)
#endif

// the four tap offsets (in samples of `step` bytes) and the two fractions of tap coordinate (sy, sx) on a plane (hp, wp) of pitch `pitch`
template <bool WRAP>
__device__ __forceinline__ void pb_tvb_taps(const double sy, const double sx, const int hp, const int wp, const unsigned pitch, const unsigned step,
                                            unsigned o[4], double& ty, double& tx) {
    const double ry = floor(sy), rx = floor(sx);
    ty = sy - ry;
    tx = sx - rx;
    unsigned r[2], c[2];
    pb_vbil_rc<WRAP>((int)ry, (int)rx, hp, wp, r, c);
    o[0] = r[0] * pitch + c[0] * step;
    o[1] = r[0] * pitch + c[1] * step;
    o[2] = r[1] * pitch + c[0] * step;
    o[3] = r[1] * pitch + c[1] * step;
}
// the definition's three lerps, in its order, float64 (samples are below 2^16: the result is too)
__device__ __forceinline__ unsigned pb_tvb_mix(const unsigned a, const unsigned b, const unsigned c, const unsigned d, const double tx, const double ty) {
    const double fa = (double)a, fb = (double)b, fc = (double)c, fd = (double)d;
    const double top = fa + tx * (fb - fa), bot = fc + tx * (fd - fc);
    return (unsigned)rint(top + ty * (bot - top));
}

// (the sample size comes first, for the reason pb_kernels_track_video.hpp gives)
template <int S, int SRC_KIND, bool PAIRS>
__global__ __launch_bounds__(PB_BLOCK, PB_TVB_WPE(SRC_KIND)) void pb_track_video_bilinear_kernel(const PbParams P, const double* __restrict__ rot, int k_rot, int fpc,
                                                                                     const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n_frames,
                                                                                     unsigned long long src_stride, unsigned long long dst_stride, const PbPlanar L,
                                                                                     const int cx_arg, const int cy_arg) {
    static_assert(SRC_KIND == PB_KIND_PANO || SRC_KIND == PB_KIND_CAMERA, "the sources the definition covers (tests/video_bilinear_ref.py)");
    constexpr bool WRAP = SRC_KIND == PB_KIND_PANO;
    const int cx = PAIRS ? 1 : cx_arg, cy = PAIRS ? 1 : cy_arg;  // (each 0 or 1)
    const int W = P.dst.width, H = P.dst.height;
    const unsigned qpr = ((unsigned)W + PB_PX - 1) / PB_PX;  // quads per row
    const unsigned g = blockIdx.x * PB_BLOCK + threadIdx.x;
    unsigned y = g / qpr;
    if (y >= (unsigned)H) return;
    int x0 = (int)(g - y * qpr) * PB_PX;

    const int count = (W - x0 >= PB_PX) ? PB_PX : W - x0;
    double lat[PB_PX], lon[PB_PX];
    bool inv[PB_PX];
    pb_track_fill_row(P, y, x0, count, lat, lon, inv);
    const int h = P.src.height, w = P.src.width;
    const PbTrackChunk ch = pb_track_chunk(fpc, n_frames);
    for (int f = ch.f0; f < ch.f1; ++f) {
        const uint8_t* __restrict__ s = src + (unsigned long long)f * src_stride;
        uint8_t* __restrict__ d = dst + (unsigned long long)f * dst_stride;
        pb_track_reask(y, x0);
        const unsigned yy = y;
        const int xx = x0;
        const bool anchor_row = !(yy & (unsigned)cy);
        unsigned pa[PB_PX / 2] = {0u, 0u}, p1[PB_PX / 2] = {0u, 0u}, p2[PB_PX / 2] = {0u, 0u};  // (pb_track_pack)
        PB_UNROLL(PB_FAITHFUL_UNROLL)
        for (int k = 0; k < PB_PX; ++k) {
            if (k < count) {
                const PbCoord c = pb_track_quad_coord(lat, lon, inv, k, rot, k_rot, f);
                double fy, fx;
                if (WRAP) {
                    pb_src_pretrunc<PB_KIND_PANO>(P, c, fy, fx);
                } else {
                    double sl, cl;
                    pb_expi_np(c.lon, &sl, &cl);  // np.exp(lon * 1j)
                    pb_src_pretrunc_sc<PB_KIND_CAMERA>(P, c, sl, cl, fy, fx);
                }
                const bool live = !c.inv && (WRAP ? pb_live(fy, fx, 1.0e300) : pb_live_in(fy, fx, 1.0e300, h, w));
                const double sy = live ? fy - 0.5 : 0.0, sx = live ? fx - 0.5 : 0.0;
                unsigned o[4];
                double ty, tx;
                pb_tvb_taps<WRAP>(sy, sx, h, w, L.src_pitch, (unsigned)S, o, ty, tx);
                const unsigned v0 = pb_tvb_mix(pb_nv12_load_y<S>(s, o[0]), pb_nv12_load_y<S>(s, o[1]), pb_nv12_load_y<S>(s, o[2]), pb_nv12_load_y<S>(s, o[3]), tx, ty);
                pb_track_pack(pa, k, live ? v0 : L.fill[0]);
                if (anchor_row && !(k & cx)) {  // an anchor: its coordinate in chroma sample units, s / 2 where subsampled (exact)
                    pb_tvb_taps<WRAP>(cy ? sy * 0.5 : sy, cx ? sx * 0.5 : sx, h >> cy, w >> cx, L.src_cpitch, (unsigned)(PAIRS ? 2 * S : S), o, ty, tx);
                    unsigned u[4], v[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) pb_video_load_c<S, PAIRS>(s, L, o[t], u[t], v[t]);
                    const unsigned v1 = pb_tvb_mix(u[0], u[1], u[2], u[3], tx, ty), v2 = pb_tvb_mix(v[0], v[1], v[2], v[3], tx, ty);
                    pb_track_pack(p1, k, live ? v1 : L.fill[1]);
                    pb_track_pack(p2, k, live ? v2 : L.fill[2]);
                }
            }
        }
        pb_track_video_store<S, PAIRS, false>(d, L, W, H, xx, yy, cx, cy, anchor_row, L.dst_cpitch, pa, p1, p2);
    }
}
