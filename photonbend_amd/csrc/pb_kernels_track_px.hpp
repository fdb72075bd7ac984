// pb_kernels_track_px.hpp - ROTATION TRACKS OF GREY, RGBA AND 16-BIT FRAMES (pb_remap_track_px): pb_kernels_track.hpp's
// launch - every frame of a batch with rotations of its own, the part of the float64 chain no frame changes once per pixel and chunk of
// frames - for pixels of B = channels * sample_bytes bytes, B in {1, 2, 4, 6, 8} (three bytes are pb_remap_track_u8's own kernels).
// Frame f receives the bytes of the materialised-map route for that frame alone: the destination's map, the plan's rotations, frame f's
// (pb_rotate_f64 each, nothing folded), then
//   nearest       pb_index_from_map_i32 + pb_gather_px (a double fisheye: pb_gather_blend_u8) - the sampler never looks inside a pixel;
//   interpolating pb_sample_map_bilinear_px / pb_sample_map_catmull_rom_px - FILTER::sample64<SAMPLE, WRAP> per channel.
//
// pb_track_px_kernel<SRC_KIND>: pb_track_body's frame loop, on the skeleton of pb_kernels_track.hpp.  The pixel size is a RUN-TIME
// kernel argument, uniform across the launch: the body is the float64 chain (some 19 000 instructions per source kind), which is what the kernel costs; a copy per pixel size would
// multiply that by five and buy nothing.  A pixel is loaded with exactly its own bytes (pb_px_load of pb_kernels_px.hpp: u8, u16, dword,
// dword + u16, 2 x dword; frames aligned to A = min(4, B & -B)) and held in two dwords, so no load touches a byte outside the frame; four
// pixels leave as dwords where their first byte is 4-byte aligned, else in units of A, every store clipped to the image.  Byte offsets
// inside a frame are 64-bit.
// pb_track_px_interp_kernel<SRC_KIND, FILTER, SAMPLE>: pb_track_interp_body's structure around what pb_sample_map_interp_px does from a
// map entry onward (pb_track_px_sample below, written beside it: splitting that function moves its kernels' registers).
#pragma once
#include <hip/hip_runtime.h>

#include "pb_kernels_px.hpp"
#include "pb_kernels_track.hpp"

// waves per SIMD the nearest kernels are compiled for.  A panorama and a camera source are held to eight, as PB_TRACK_WPE holds the RGB8
// kernel (63 VGPRs, 78 scalar registers, no scratch: what is live across the chains is an index per pixel, as there); a cube and a
// double-fisheye source get the budget of four, under which the compiler takes seven - they fit eight without scratch too (62-63 VGPRs)
// but move 140-370 scalars through vector lanes, and the RGB8 kernel's measurement of that trade is not repeated here
#ifndef PB_TRACK_PX_WPE
#define PB_TRACK_PX_WPE(kind) (((kind) == PB_KIND_PANO || (kind) == PB_KIND_CAMERA) ? 8 : 4)
#endif

// The four pixels of a single source move AFTER their four chains, from their source indices: one index per pixel is live across the
// chains (as the RGB8 kernel's packed pixel is), the pixel's two dwords only between its load and its store.  (Loaded inside the chain
// loop - behind a branch on the run-time size in every pixel's divergent region - the panorama and camera kernels spill 12 bytes of
// scratch at eight waves.)  The movement itself is pb_kernels_px.hpp's: pb_px_load takes exactly the pixel's bytes, a black pixel reads
// pixel 0 and is zeroed; pb_px_store4 where all four exist and their first byte is 4-byte aligned, else pb_px_store1 in units of A.
template <int BPP>
__device__ __forceinline__ void pb_track_px_move4(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, unsigned long long p0, const int idx[PB_PX], int count) {
    PbPx<BPP> a[PB_PX];
#pragma unroll
    for (int k = 0; k < PB_PX; ++k)  // (k >= count: index -1)
        a[k] = pb_px_zero_if<BPP>(pb_px_load<BPP>(s + (unsigned long long)(unsigned)(idx[k] < 0 ? 0 : idx[k]) * (unsigned)BPP, 0u), idx[k] < 0);
    uint8_t* p = d + p0 * (unsigned)BPP;
    if (count == PB_PX && ((uintptr_t)p & 3u) == 0) {
        pb_px_store4<BPP, false>(p, a);
    } else {
#pragma unroll
        for (int k = 0; k < PB_PX; ++k)
            if (k < count) pb_px_store1<BPP>(p + BPP * k, a[k]);
    }
}
__device__ __forceinline__ void pb_track_px_move4(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, unsigned long long p0, const int idx[PB_PX], int count, int B) {
    switch (B) {  // (uniform: a scalar branch)
        case 1: pb_track_px_move4<1>(s, d, p0, idx, count); break;
        case 2: pb_track_px_move4<2>(s, d, p0, idx, count); break;
        case 4: pb_track_px_move4<4>(s, d, p0, idx, count); break;
        case 6: pb_track_px_move4<6>(s, d, p0, idx, count); break;
        default: pb_track_px_move4<8>(s, d, p0, idx, count); break;
    }
}
template <int SRC_KIND>
__device__ __forceinline__ int pb_track_px_index(const PbParams& P, const PbCoord& c) {
    if (SRC_KIND == PB_KIND_PANO) return pb_src_pano_index(P, c);
    if (SRC_KIND == PB_KIND_CAMERA) return pb_src_camera_index(P, c);
    return pb_src_cube_index<SRC_KIND == PB_KIND_EAC>(P, c);
}

// A double fisheye (uint8 samples: B = 1, 2 or 4, the pixel one dword) blends inside the chain loop - two indices and two float64
// factors per pixel would be live across the chains otherwise: byte-wise (l * fl + r * fr) through pb_cvt_u8, zeros where the entry is
// invalid - pb_gather_blend_u8's bytes
__device__ __forceinline__ unsigned pb_track_px_load_lo(const uint8_t* __restrict__ s, int idx, int B) {
    if (idx < 0) return 0u;
    const uint8_t* p = s + (unsigned long long)(unsigned)idx * (unsigned)B;
    return B == 1 ? (unsigned)*p : (B == 2 ? (unsigned)*reinterpret_cast<const uint16_t*>(p) : *reinterpret_cast<const unsigned*>(p));
}
__device__ __forceinline__ unsigned pb_track_px_blend(const PbParams& P, const PbCoord& c, const uint8_t* __restrict__ s, int B) {
    const PbDoubleTap t = pb_src_double_taps(P, c);
    const unsigned l = pb_track_px_load_lo(s, t.il, B), r = pb_track_px_load_lo(s, t.ir, B);
    if (c.inv) return 0u;  // final_image[invalid_map] = 0, projection.py:460
    unsigned v = 0u;
    for (int b = 0; b < B; ++b) v |= pb_blend_u8((l >> (8 * b)) & 0xFF, (r >> (8 * b)) & 0xFF, t.fl, t.fr) << (8 * b);
    return v;
}
template <int BPP>
__device__ __forceinline__ void pb_track_px_store4_lo(uint8_t* __restrict__ d, unsigned long long p0, const int v[PB_PX], int count) {
    uint8_t* p = d + p0 * (unsigned)BPP;
    PbPx<BPP> a[PB_PX];
#pragma unroll
    for (int k = 0; k < PB_PX; ++k) a[k].w[0] = (unsigned)v[k];
    if (count == PB_PX && ((uintptr_t)p & 3u) == 0) {
        pb_px_store4<BPP, false>(p, a);
    } else {
#pragma unroll
        for (int k = 0; k < PB_PX; ++k)
            if (k < count) pb_px_store1<BPP>(p + BPP * k, a[k]);
    }
}
__device__ __forceinline__ void pb_track_px_store4_lo(uint8_t* __restrict__ d, unsigned long long p0, const int v[PB_PX], int count, int B) {
    if (B == 1) pb_track_px_store4_lo<1>(d, p0, v, count);
    else if (B == 2) pb_track_px_store4_lo<2>(d, p0, v, count);
    else pb_track_px_store4_lo<4>(d, p0, v, count);
}

// grid: (quads of the image / PB_BLOCK, chunks of fpc frames) - pb_track_body's; what is carried per pixel differs from it (above)
template <int SRC_KIND>
__device__ __forceinline__ void pb_track_px_body(const PbParams& P, const double* __restrict__ rot, int k_rot, int fpc, const uint8_t* __restrict__ src,
                                                 uint8_t* __restrict__ dst, int n_frames, unsigned long long src_stride, unsigned long long dst_stride, int B) {
    const unsigned total = (unsigned)P.dst.height * (unsigned)P.dst.width;
    const unsigned g = blockIdx.x * PB_BLOCK + threadIdx.x;
    if (g >= (total + PB_PX - 1) / PB_PX) return;
    const unsigned p0 = g * PB_PX;
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
        int a[PB_PX];  // a single source: the pixel's source index; a double fisheye: its blended bytes
        PB_UNROLL(PB_FAITHFUL_UNROLL)
        for (int k = 0; k < PB_PX; ++k) {
            a[k] = SRC_KIND == PB_KIND_DOUBLE ? 0 : -1;
            if (k < count) {
                const PbCoord c = pb_track_quad_coord(lat, lon, inv, k, rot, k_rot, f);
                if constexpr (SRC_KIND == PB_KIND_DOUBLE) a[k] = (int)pb_track_px_blend(P, c, s, B);
                else a[k] = pb_track_px_index<SRC_KIND>(P, c);
            }
        }
        if constexpr (SRC_KIND == PB_KIND_DOUBLE) pb_track_px_store4_lo(d, p0, a, count, B);
        else pb_track_px_move4(s, d, p0, a, count, B);
    }
}
template <int SRC_KIND>
__global__ __launch_bounds__(PB_BLOCK, PB_TRACK_PX_WPE(SRC_KIND)) void pb_track_px_kernel(const PbParams P, const double* __restrict__ rot, int k_rot, int fpc,
                                                                                const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n_frames,
                                                                                unsigned long long src_stride, unsigned long long dst_stride, int B) {
    pb_track_px_body<SRC_KIND>(P, rot, k_rot, fpc, src, dst, n_frames, src_stride, dst_stride, B);
}
// ... of an equi-angular cube source (a kernel of its own name, as pb_track_eac_kernel is: tests/test_isa_track_px.py lists per source kind)
__global__ __launch_bounds__(PB_BLOCK, PB_TRACK_PX_WPE(PB_KIND_EAC)) void pb_track_px_equiangular_kernel(const PbParams P, const double* __restrict__ rot, int k_rot, int fpc,
                                                                                    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n_frames,
                                                                                    unsigned long long src_stride, unsigned long long dst_stride, int B) {
    pb_track_px_body<PB_KIND_EAC>(P, rot, k_rot, fpc, src, dst, n_frames, src_stride, dst_stride, B);
}

// One interpolated pixel of a frame from its map entry: what pb_sample_map_interp_px computes from the entry onward - the source stage,
// liveness (bound 1.0e300), FILTER::sample64 per channel, a cube's face rectangle, a double fisheye's two eyes on their halves and the
// reference's blend (uint8 whatever the samples: instantiated for uint8_t alone).  o: the pixel's first sample.
template <int SRC_KIND, class FILTER, typename SAMPLE>
__device__ __forceinline__ void pb_track_px_sample(const PbParams& P, const PbCoord& c, const SAMPLE* __restrict__ img, SAMPLE* __restrict__ o, int channels) {
    const bool inv = c.inv;
    const double lat = c.lat, lon = c.lon;  // (an invalid entry is (0, 0) behind a rotation: pb_rotate)
    const int h = P.src.height, w = P.src.width;
    if (SRC_KIND == PB_KIND_PANO) {
        const double fy = lat / P.src_hseg, fx = lon / P.src_wseg + P.src_half_w;
        const bool live = !inv && pb_live(fy, fx, 1.0e300);
        for (int ch = 0; ch < channels; ++ch)
            o[ch] = live ? (SAMPLE)FILTER::template sample64<SAMPLE, true>(img, fy, fx, h, w, 0, w, false, channels, ch) : (SAMPLE)0;
        return;
    }
    if (pb_is_cube(SRC_KIND)) {
        const PbCubePos q = pb_src_cube_pos<SRC_KIND == PB_KIND_EAC>(P, c);
        const int n = pb_cube_n(P.src);
        const bool live = !inv && pb_live_in(q.fy, q.fx, 1.0e300, n, n);
        const SAMPLE* face = img + ((unsigned long long)pb_cube_row0(q.face, n) * (unsigned)w + (unsigned)pb_cube_col0(q.face, n)) * (unsigned)channels;
        for (int ch = 0; ch < channels; ++ch)
            o[ch] = live ? (SAMPLE)FILTER::template sample64<SAMPLE, false>(face, q.fy, q.fx, n, w, 0, n, false, channels, ch) : (SAMPLE)0;
        return;
    }
    double sl, cl;
    pb_expi_np(lon, &sl, &cl);  // np.exp(lon * 1j), projection.py:252
    if (SRC_KIND == PB_KIND_CAMERA) {
        const double dist = pb_lens_forward(P, lat) * P.src.f_distance;
        const double fy = ((sl * dist) * -1.0) + P.src_cy, fx = (cl * dist) + P.src_cx;
        const bool live = !inv && pb_live_in(fy, fx, 1.0e300, h, w);
        for (int ch = 0; ch < channels; ++ch)
            o[ch] = live ? (SAMPLE)FILTER::template sample64<SAMPLE, false>(img, fy, fx, h, w, 0, w, false, channels, ch) : (SAMPLE)0;
        return;
    }
    const double lat_r = (lat * -1.0) + PB_PI;
    const double dl = pb_lens_forward(P, lat) * P.src.f_distance, dr = pb_lens_forward(P, lat_r) * P.src.f_distance;
    const int wl = P.src_eye_w, wr = P.src_eye_w_right;
    const double fyl = ((sl * dl) * -1.0) + P.src_cy, fxl = (cl * dl) + P.src_cx;
    const double fyr = ((sl * dr) * -1.0) + P.src_cy, fxr = (cl * dr) + P.src_cx_r;
    const bool live_l = !inv && pb_live_in(fyl, fxl, 1.0e300, h, wl), live_r = !inv && pb_live_in(fyr, fxr, 1.0e300, h, wr);
    const double fl = pb_merge_factor(P, lat), fr = pb_merge_factor(P, lat_r);
    for (int ch = 0; ch < channels; ++ch) {
        const double l = live_l ? FILTER::template sample64<SAMPLE, false>(img, fyl, fxl, h, w, 0, wl, false, channels, ch) : 0.0;
        const double r = live_r ? FILTER::template sample64<SAMPLE, false>(img, fyr, fxr, h, w, wl, wl + wr, true, channels, ch) : 0.0;
        o[ch] = inv ? (SAMPLE)0 : (SAMPLE)pb_cvt_u8(l * fl + r * fr);
    }
}

// one pixel per work-item; grid: (pixels of the image / PB_BLOCK, chunks of fpc frames) - pb_track_interp_body's
template <int SRC_KIND, class FILTER, typename SAMPLE>
__device__ __forceinline__ void pb_track_px_interp_body(const PbParams& P, const double* __restrict__ rot, int k_rot, int fpc, const uint8_t* __restrict__ src,
                                                        uint8_t* __restrict__ dst, int n_frames, unsigned long long src_stride, unsigned long long dst_stride,
                                                        int channels) {
    static_assert(SRC_KIND != PB_KIND_DOUBLE || sizeof(SAMPLE) == 1, "the double-fisheye blend writes uint8");
    PbPixelPick k;
    if (!pb_pick_pixel(P, true, nullptr, 0, nullptr, 0, nullptr, 0, k)) return;
    const PbCoord base = pb_chain<PB_ROT_ANY>(P, k.i, k.j);
    const unsigned long long off = (unsigned long long)k.p * (unsigned)channels * sizeof(SAMPLE);
    const PbTrackChunk ch = pb_track_chunk(fpc, n_frames);
    for (int f = ch.f0; f < ch.f1; ++f) {
        const SAMPLE* img = reinterpret_cast<const SAMPLE*>(src + (unsigned long long)f * src_stride);
        SAMPLE* o = reinterpret_cast<SAMPLE*>(dst + (unsigned long long)f * dst_stride + off);
        pb_track_px_sample<SRC_KIND, FILTER, SAMPLE>(P, pb_track_rotate(rot, k_rot, f, base), img, o, channels);
    }
}
template <int SRC_KIND, class FILTER, typename SAMPLE>
__global__ __launch_bounds__(PB_BLOCK) void pb_track_px_interp_kernel(const PbParams P, const double* __restrict__ rot, int k_rot, int fpc,
                                                                      const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n_frames,
                                                                      unsigned long long src_stride, unsigned long long dst_stride, int channels) {
    pb_track_px_interp_body<SRC_KIND, FILTER, SAMPLE>(P, rot, k_rot, fpc, src, dst, n_frames, src_stride, dst_stride, channels);
}
template <class FILTER, typename SAMPLE>
__global__ __launch_bounds__(PB_BLOCK) void pb_track_px_interp_equiangular_kernel(const PbParams P, const double* __restrict__ rot, int k_rot, int fpc,
                                                                          const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n_frames,
                                                                          unsigned long long src_stride, unsigned long long dst_stride, int channels) {
    pb_track_px_interp_body<PB_KIND_EAC, FILTER, SAMPLE>(P, rot, k_rot, fpc, src, dst, n_frames, src_stride, dst_stride, channels);
}
