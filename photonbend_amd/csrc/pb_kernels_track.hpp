// pb_kernels_track.hpp - ROTATION TRACKS (pb_remap_track_u8): one launch remaps a batch in which every frame has rotations
// of its own - a stabilised or reframed 360-degree video, a turntable.  Frame f is the float64 chain of pb_stages.hpp for the plan's own
// rotations FOLLOWED BY frame f's, applied one after another as the reference applies Rotation objects (rotation.py:102-176: arccos /
// atan2 between them, nothing folded): for nearest sampling the reference's own output of that chain, for the interpolating modes their
// float64 per-pixel definition.  The plan's tables are certified for another chain and are never read: the kernels take the parameter
// block and nothing else of a plan.
//
// What a work-item computes ONCE is the part of the chain no frame changes - pb_dst_coord, a cube destination's face rotation, the plan's
// own rotations (pb_chain): two float64 and a flag per pixel stay live across the frame loop, nothing of the transcendental kernels
// (the build's switched-off machine LICM keeps their constants inside the loop body: pb_stages.hpp, pb_rotate_all).  Per frame of its chunk
// it rotates by the frame's matrices, evaluates the source, gathers and stores.  Frames are chunked over blockIdx.y, `fpc` frames per
// chunk (PB_TRACK_FRAMES; the last chunk may be short).  The matrix address depends on the frame alone - uniform across the workgroup -
// so the nine entries of a matrix arrive as scalar operands; the table is only ever loaded from.
//
// The pieces of that structure which the track kernels share - this file's, pb_kernels_track_px.hpp's, pb_kernels_track_video.hpp's,
// pb_kernels_track_video_bilinear.hpp's and pb_kernels_track_stitch.hpp's - are written ONCE, in the skeleton below, as __forceinline__
// functions: pb_track_chunk and pb_track_quad_coord for all of them, and for the three kernels of video frames the fill of a row quad,
// the re-asked row and column, the packed samples and the three planes' stores.  What was observed of the forms (gfx950 listing):
//   pb_track_chunk, pb_track_quad_coord, pb_track_pack   leave every kernel's instruction stream as it was.
//   pb_track_fill_row, pb_track_video_store              reorder the instruction stream of the video kernels; registers, scratch and
//                                                        waves stay (a cube source's PAIRS kernels take one VGPR fewer), and so does
//                                                        their rate (experiments/README.md).  pb_track_stitch_kernel keeps the fill's
//                                                        text by the letter of the rate criterion: with the function its PAIRS forms
//                                                        measured 0.3 - 0.4 % above the parent's own range, which is also what one
//                                                        process differs from the next by with the same instructions.
//   a fill function for the linear quad                  moves pb_track_eac_kernel and pb_track_kernel<cube> from 7 to 8 waves: the
//                                                        pb_chain block stays in pb_track_body and pb_track_px_body.
//   the frame loop with the sample as a closure          moved registers of every nearest kernel (the stitch kernels to 65 VGPRs): the
//                                                        frame loops stay in the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "pb_kernels_bilinear.hpp"
#include "pb_kernels_catmull_rom.hpp"
#include "pb_kernels_faithful.hpp"
#include "pb_video.hpp"

// frames per chunk: chosen by measurement on MI355X (experiments/rotation_track_rate.py; the table in DESIGN 3.13)
#ifndef PB_TRACK_FRAMES
#define PB_TRACK_FRAMES 4
#endif
// waves per SIMD the nearest kernel is compiled for.  A panorama and a camera source are held to eight (at most 64 VGPRs and 96 scalar
// registers: no scratch); a cube and a double-fisheye source get the budget of four, under which the compiler takes seven (64-65 VGPRs,
// 106 scalar registers) - held to eight they spill 12 bytes of scratch.  Measured on MI355X, eight against the budget of four, A / B / A / B,
// 16 frames, us per frame: panorama source 116.3 -> 110.7 (panorama destination) and 267.6 -> 263.1 (c2), fisheye 148.0 -> 140.4; with the
// spill cube 249.3 -> 238.6 and double fisheye 153.1 -> 148.9, not taken: no frame-loop kernel of this library spills
#ifndef PB_TRACK_WPE
#define PB_TRACK_WPE(kind) (((kind) == PB_KIND_PANO || (kind) == PB_KIND_CAMERA) ? 8 : 4)
#endif

// frame f's rotations: k_rot matrices at rot + 9 * k_rot * f (f is uniform: scalar loads)
__device__ __forceinline__ PbCoord pb_track_rotate(const double* __restrict__ rot, int k_rot, int f, PbCoord c) {
    const double* __restrict__ R = rot + 9ull * (unsigned)k_rot * (unsigned)f;
    for (int r = 0; r < k_rot; ++r) c = pb_rotate(R + 9 * r, c);
    return c;
}

// ---- the skeleton --------------------------------------------------------------------------------------------------------------------
// the frames of this workgroup's chunk, [f0, f1): chunks of fpc frames over blockIdx.y, the last one may be short
struct PbTrackChunk {
    int f0, f1;
};
__device__ __forceinline__ PbTrackChunk pb_track_chunk(int fpc, int n_frames) {
    const int f0 = (int)blockIdx.y * fpc;
    return {f0, (n_frames - f0 < fpc) ? n_frames : f0 + fpc};
}

// A quad's frame-invariant state is the coordinate of each of its `count` pixels (1 to PB_PX) behind the plan's own rotations, in three
// arrays of the kernel: double lat[PB_PX], lon[PB_PX]; bool inv[PB_PX].
// pb_track_quad_coord: pixel k's coordinate under frame f's rotations
__device__ __forceinline__ PbCoord pb_track_quad_coord(const double lat[PB_PX], const double lon[PB_PX], const bool inv[PB_PX], int k, const double* rot, int k_rot,
                                                       int f) {
    PbCoord c;
    c.lat = lat[k];
    c.lon = lon[k];
    c.inv = inv[k];
    c.face = 0;
    return pb_track_rotate(rot, k_rot, f, c);
}
// the fill of a row quad (video frames: rows are pitched, so a quad is `count` pixels of ONE row y from column x0 on)
__device__ __forceinline__ void pb_track_fill_row(const PbParams& P, unsigned y, int x0, int count, double lat[PB_PX], double lon[PB_PX], bool inv[PB_PX]) {
    PB_UNROLL(PB_FAITHFUL_UNROLL)
    for (int k = 0; k < PB_PX; ++k) {
        lat[k] = lon[k] = 0.0;
        inv[k] = true;
        if (k < count) {
            const PbCoord c = pb_chain<PB_ROT_ANY>(P, (int)y, x0 + k);
            lat[k] = c.lat;
            lon[k] = c.lon;
            inv[k] = c.inv;
        }
    }
}
// A video kernel asks its row and column anew in every frame, IN PLACE, from values the compiler cannot trace: what it would otherwise
// compute once from them - three planes' store offsets, the anchor tests - stays live across the float64 chains of the whole frame loop
// and puts the panorama and camera instantiations into scratch at their eight waves.
__device__ __forceinline__ void pb_track_reask(unsigned& y, int& x0) { asm volatile("" : "+v"(y), "+v"(x0)); }
// A frame's samples of one quad are 16 bits each at the most: packed two pixels to a register (unsigned pa[PB_PX / 2], p1[], p2[], zeroed
// per frame) while the other pixels' chains run.  pa: plane 0; p1, p2: planes 1 and 2, of the quad's ANCHORS - a quad starts at a multiple
// of four, so on a row with (y & cy) == 0 its pixels k with (k & cx) == 0 own the chroma sample at (y >> cy, x >> cx); cx and cy, each 0
// or 1, are RUN-TIME and wave-uniform.
__device__ __forceinline__ void pb_track_pack(unsigned p[PB_PX / 2], int k, unsigned v) { p[k >> 1] |= v << (16 * (k & 1)); }
// ... and their stores: pb_nv12_store_y for four samples of a row, pb_planar_store2 for two, pb_nv12_store_uv for two pairs - one store where
// the address allows, else one by one, clipped to the plane.  Padding between rows, planes and frames is never written.
//   AS_STORED   false: p1 holds plane 1's samples and p2 plane 2's, joined here where the planes are interleaved (PAIRS: U first; the
//               anchors are the pixels k = 0, 2: the low halves).
//               true: the kernel packed what it loaded as it lies in memory - with PAIRS the whole pair in p1 (it belongs to an even
//               pixel and takes the register whole: 32 bits at S == 2), and where cx == 1 the odd halves are empty: nothing to mask.
//   dst_cpitch  the pitch of the destination's planes 1 and 2 (of the pair plane)
template <int S, bool PAIRS, bool AS_STORED>
__device__ __forceinline__ void pb_track_video_store(uint8_t* d, const PbPlanar& L, const int W, const int H, const int xx, const unsigned yy, const int cx, const int cy,
                                                     const bool anchor_row, const unsigned dst_cpitch, const unsigned pa[PB_PX / 2], const unsigned p1[PB_PX / 2],
                                                     const unsigned p2[PB_PX / 2]) {
    const unsigned a[PB_PX] = {pa[0] & 0xFFFFu, pa[0] >> 16, pa[1] & 0xFFFFu, pa[1] >> 16};
    pb_nv12_store_y<S, false>(d, L.dst_pitch, W, H, xx, (int)yy, a);
    if (!anchor_row) return;
    if constexpr (PAIRS && AS_STORED) {
        pb_nv12_store_uv<S, false>(d + L.dst_o1, dst_cpitch, W, H, xx, (int)yy, p1);
    } else if constexpr (PAIRS) {
        const unsigned uv[2] = {(p1[0] & 0xFFFFu) | ((p2[0] & 0xFFFFu) << (8 * S)), (p1[1] & 0xFFFFu) | ((p2[1] & 0xFFFFu) << (8 * S))};
        pb_nv12_store_uv<S, false>(d + L.dst_o1, dst_cpitch, W, H, xx, (int)yy, uv);
    } else if (cx == 0) {
        const unsigned c1[PB_PX] = {p1[0] & 0xFFFFu, p1[0] >> 16, p1[1] & 0xFFFFu, p1[1] >> 16};
        const unsigned c2[PB_PX] = {p2[0] & 0xFFFFu, p2[0] >> 16, p2[1] & 0xFFFFu, p2[1] >> 16};
        pb_nv12_store_y<S, false>(d + L.dst_o1, dst_cpitch, W, H, xx, (int)yy, c1);
        pb_nv12_store_y<S, false>(d + L.dst_o2, dst_cpitch, W, H, xx, (int)yy, c2);
    } else if constexpr (AS_STORED) {
        pb_planar_store2<S, false>(d + L.dst_o1, dst_cpitch, W >> 1, H >> cy, xx >> 1, (int)(yy >> cy), p1);
        pb_planar_store2<S, false>(d + L.dst_o2, dst_cpitch, W >> 1, H >> cy, xx >> 1, (int)(yy >> cy), p2);
    } else {
        const unsigned h1[2] = {p1[0] & 0xFFFFu, p1[1] & 0xFFFFu}, h2[2] = {p2[0] & 0xFFFFu, p2[1] & 0xFFFFu};
        pb_planar_store2<S, false>(d + L.dst_o1, dst_cpitch, W >> 1, H >> cy, xx >> 1, (int)(yy >> cy), h1);
        pb_planar_store2<S, false>(d + L.dst_o2, dst_cpitch, W >> 1, H >> cy, xx >> 1, (int)(yy >> cy), h2);
    }
}

// ---- the RGB8 kernels ----------------------------------------------------------------------------------------------------------------
// one nearest pixel of a frame from its map entry: process_coordinate_map's sample (pb_remap_kernel's, per frame)
template <int SRC_KIND>
__device__ __forceinline__ unsigned pb_track_px(const PbParams& P, const PbCoord& c, const uint8_t* __restrict__ s) {
    if (SRC_KIND == PB_KIND_PANO) return pb_load_px(s, pb_src_pano_index(P, c));
    if (SRC_KIND == PB_KIND_CAMERA) return pb_load_px(s, pb_src_camera_index(P, c));
    if (pb_is_cube(SRC_KIND)) return pb_load_px(s, pb_src_cube_index<SRC_KIND == PB_KIND_EAC>(P, c));
    const PbDoubleTap t = pb_src_double_taps(P, c);
    const unsigned l = pb_load_px(s, t.il), r = pb_load_px(s, t.ir);
    if (c.inv) return 0u;  // final_image[invalid_map] = 0, projection.py:460
    return pb_blend_u8(l & 0xFF, r & 0xFF, t.fl, t.fr) | (pb_blend_u8((l >> 8) & 0xFF, (r >> 8) & 0xFF, t.fl, t.fr) << 8) |
           (pb_blend_u8((l >> 16) & 0xFF, (r >> 16) & 0xFF, t.fl, t.fr) << 16);
}

// pb_remap_kernel's layout: PB_PX consecutive output pixels per work-item, three dword stores where the frame is 4-byte aligned, bytes
// otherwise, every store clipped to the image.  grid: (quads of the image / PB_BLOCK, chunks of fpc frames).
template <int SRC_KIND>
__device__ __forceinline__ void pb_track_body(const PbParams& P, const double* __restrict__ rot, int k_rot, int fpc, const uint8_t* __restrict__ src,
                                              uint8_t* __restrict__ dst, int n_frames, unsigned long long src_stride, unsigned long long dst_stride, int aligned) {
    const unsigned total = (unsigned)P.dst.height * (unsigned)P.dst.width;
    const unsigned g = blockIdx.x * PB_BLOCK + threadIdx.x;
    const unsigned p0 = g * PB_PX;
    if (p0 >= total) return;
    const int count = (total - p0 >= PB_PX) ? PB_PX : (int)(total - p0);
    const unsigned W = (unsigned)P.dst.width;
    unsigned i = p0 / W, j = p0 - i * W;

    double lat[PB_PX], lon[PB_PX];
    bool inv[PB_PX];
    PB_UNROLL(PB_FAITHFUL_UNROLL)
    for (int k = 0; k < PB_PX; ++k) {
        lat[k] = lon[k] = 0.0;
        inv[k] = true;
        if (k < count) {
            const PbCoord c = pb_chain<PB_ROT_ANY>(P, (int)i, (int)j);
            lat[k] = c.lat;
            lon[k] = c.lon;
            inv[k] = c.inv;
            if (++j == W) {
                j = 0;
                ++i;
            }
        }
    }
    const PbTrackChunk ch = pb_track_chunk(fpc, n_frames);
    for (int f = ch.f0; f < ch.f1; ++f) {
        const uint8_t* s = src + (unsigned long long)f * src_stride;
        uint8_t* d = dst + (unsigned long long)f * dst_stride;
        unsigned a[PB_PX];
        PB_UNROLL(PB_FAITHFUL_UNROLL)
        for (int k = 0; k < PB_PX; ++k) {
            a[k] = 0u;
            if (k < count) a[k] = pb_track_px<SRC_KIND>(P, pb_track_quad_coord(lat, lon, inv, k, rot, k_rot, f), s);
        }
        pb_store_px4(d, p0, a, count, aligned != 0);
    }
}
template <int SRC_KIND>
__global__ __launch_bounds__(PB_BLOCK, PB_TRACK_WPE(SRC_KIND)) void pb_track_kernel(const PbParams P, const double* __restrict__ rot, int k_rot, int fpc,
                                                                                   const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n_frames,
                                                                                   unsigned long long src_stride, unsigned long long dst_stride, int aligned) {
    pb_track_body<SRC_KIND>(P, rot, k_rot, fpc, src, dst, n_frames, src_stride, dst_stride, aligned);
}
// ... of an equi-angular cube source (a kernel of its own name: the instantiations of the one above are listed per source kind by
// tests/test_isa_track.py)
__global__ __launch_bounds__(PB_BLOCK, PB_TRACK_WPE(PB_KIND_EAC)) void pb_track_eac_kernel(const PbParams P, const double* __restrict__ rot, int k_rot, int fpc,
                                                                                          const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n_frames,
                                                                                          unsigned long long src_stride, unsigned long long dst_stride, int aligned) {
    pb_track_body<PB_KIND_EAC>(P, rot, k_rot, fpc, src, dst, n_frames, src_stride, dst_stride, aligned);
}

// The interpolating modes: one pixel, its pb_chain and pb_track_chunk's frames around the definition's own device functions - FILTER::prepare / FILTER::sample as
// pb_interp_fix_kernel and pb_interp_cube_kernel run them over every pixel, pb_interp_double_at as pb_interp_double_kernel does.  One
// pixel per work-item, like those.
template <int SRC_KIND, class FILTER>
__device__ __forceinline__ void pb_track_interp_body(const PbParams& P, const double* __restrict__ rot, int k_rot, int fpc, const uint8_t* __restrict__ src,
                                                     uint8_t* __restrict__ dst, int n_frames, unsigned long long src_stride, unsigned long long dst_stride) {
    PbPixelPick k;
    if (!pb_pick_pixel(P, true, nullptr, 0, nullptr, 0, nullptr, 0, k)) return;
    const PbCoord base = pb_chain<PB_ROT_ANY>(P, k.i, k.j);
    const PbTrackChunk ch = pb_track_chunk(fpc, n_frames);
    for (int f = ch.f0; f < ch.f1; ++f) {
        const uint8_t* s = src + (unsigned long long)f * src_stride;
        const PbCoord c = pb_track_rotate(rot, k_rot, f, base);
        unsigned v;
        if constexpr (SRC_KIND == PB_KIND_DOUBLE) {
            v = pb_interp_double_at<FILTER>(P, c, s);
        } else {
            const typename FILTER::Px q = FILTER::template prepare<SRC_KIND>(P, c);
            v = FILTER::template sample<SRC_KIND>(P, q, s);
        }
        pb_store_px(dst + (unsigned long long)f * dst_stride + 3ull * k.p, v);
    }
}
template <int SRC_KIND, class FILTER>
__global__ __launch_bounds__(PB_BLOCK) void pb_track_interp_kernel(const PbParams P, const double* __restrict__ rot, int k_rot, int fpc,
                                                                   const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n_frames,
                                                                   unsigned long long src_stride, unsigned long long dst_stride) {
    pb_track_interp_body<SRC_KIND, FILTER>(P, rot, k_rot, fpc, src, dst, n_frames, src_stride, dst_stride);
}
template <class FILTER>
__global__ __launch_bounds__(PB_BLOCK) void pb_track_interp_eac_kernel(const PbParams P, const double* __restrict__ rot, int k_rot, int fpc,
                                                                       const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n_frames,
                                                                       unsigned long long src_stride, unsigned long long dst_stride) {
    pb_track_interp_body<PB_KIND_EAC, FILTER>(P, rot, k_rot, fpc, src, dst, n_frames, src_stride, dst_stride);
}
