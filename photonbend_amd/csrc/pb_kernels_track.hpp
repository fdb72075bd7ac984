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
#pragma once
#include <hip/hip_runtime.h>

#include "pb_kernels_bilinear.hpp"
#include "pb_kernels_catmull_rom.hpp"
#include "pb_kernels_faithful.hpp"

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
    const int f0 = (int)blockIdx.y * fpc;
    const int f1 = (n_frames - f0 < fpc) ? n_frames : f0 + fpc;
    for (int f = f0; f < f1; ++f) {
        const uint8_t* s = src + (unsigned long long)f * src_stride;
        uint8_t* d = dst + (unsigned long long)f * dst_stride;
        unsigned a[PB_PX];
        PB_UNROLL(PB_FAITHFUL_UNROLL)
        for (int k = 0; k < PB_PX; ++k) {
            a[k] = 0u;
            if (k < count) {
                PbCoord c;
                c.lat = lat[k];
                c.lon = lon[k];
                c.inv = inv[k];
                c.face = 0;
                a[k] = pb_track_px<SRC_KIND>(P, pb_track_rotate(rot, k_rot, f, c), s);
            }
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

// The interpolating modes: the same structure around the definition's own device functions - FILTER::prepare / FILTER::sample as
// pb_interp_fix_kernel and pb_interp_cube_kernel run them over every pixel, pb_interp_double_at as pb_interp_double_kernel does.  One
// pixel per work-item, like those.
template <int SRC_KIND, class FILTER>
__device__ __forceinline__ void pb_track_interp_body(const PbParams& P, const double* __restrict__ rot, int k_rot, int fpc, const uint8_t* __restrict__ src,
                                                     uint8_t* __restrict__ dst, int n_frames, unsigned long long src_stride, unsigned long long dst_stride) {
    PbPixelPick k;
    if (!pb_pick_pixel(P, true, nullptr, 0, nullptr, 0, nullptr, 0, k)) return;
    const PbCoord base = pb_chain<PB_ROT_ANY>(P, k.i, k.j);
    const int f0 = (int)blockIdx.y * fpc;
    const int f1 = (n_frames - f0 < fpc) ? n_frames : f0 + fpc;
    for (int f = f0; f < f1; ++f) {
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
