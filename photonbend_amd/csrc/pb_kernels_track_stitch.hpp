// pb_kernels_track_stitch.hpp - ROTATION TRACKS FOR DOUBLE-FISHEYE VIDEO FRAMES (pb_track_stitch_planar, pb_track_stitch_nv12):
// NV12 / P010 and planar 4:4:4 / 4:2:2 / 4:2:0 frames of a side-by-side double fisheye, every frame with rotations of its own, every plane
// of every frame in one launch.  Frame f is the definition of pb_kernels_stitch_video.hpp - blend, anchors, fills, cast - with the taps
// and factors (il, ir, fl, fr) of the float64 chain "the plan's own rotations followed by frame f's" (pb_kernels_track.hpp).  No arithmetic
// is new: the chain is pb_track_body's, the taps are pb_src_double_taps' (one pb_expi_np for both eyes, as in pb_track_px), the blend is
// pb_sv_blend, the loads and stores are the stitch kernel's.  The plan's tables are never read.
//
// pb_track_stitch_kernel<S, PAIRS> has pb_track_video_kernel's structure: pb_chain<PB_ROT_ANY> once per pixel, two float64 and a flag per
// pixel live across the frame loop, frames chunked over blockIdx.y (`fpc` per chunk, a short last chunk), the frame's matrices through
// pb_track_rotate (scalar loads), a work-item owns PB_PX = 4 consecutive pixels of ONE row (a row's last quad holds 1 to 4 pixels).
//   PAIRS         planes 1 and 2 as one plane of interleaved pairs (NV12 / P010), 4:2:0.  Otherwise three planes, the subsampling a
//                 RUN-TIME, wave-uniform (cx, cy) for pb_track_video_kernel's reason.
//   taps          each tap comes apart through pb_nv12_divmod; each eye's plane-0 sample is loaded with exactly S bytes and, on anchors,
//                 its two chroma samples (PAIRS: one 2 * S-byte pair) at (r >> cy, c >> cx).  A black tap reads its plane's first sample
//                 and is zeroed after the load: branch-free, never out of bounds.  The anchor's factors serve its chroma.
//   fills         where both taps are black (an invalid destination pixel has both).
//   stores        pb_nv12_store_y, pb_planar_store2 and pb_nv12_store_uv, clipped to their planes.  Padding between rows, planes and
//                 frames is neither read nor written.
//   registers     a pixel's three samples are packed two to a register while the other pixels' chains run; the row and column are asked
//                 anew in every frame behind an empty asm (pb_track_video_kernel's reason).
//
// Limits.  Byte offsets inside a frame are 32-bit: the calls refuse frames whose span reaches 2^31 bytes and sources of 32768 px a side
// or more before any launch.  grid: (quads of a frame / PB_BLOCK, chunks of fpc frames).
#pragma once
#include "pb_kernels_stitch_video.hpp"
#include "pb_kernels_track.hpp"

template <int S, bool PAIRS>
__global__ __launch_bounds__(PB_BLOCK, PB_TRACK_WPE(PB_KIND_DOUBLE)) void pb_track_stitch_kernel(const PbParams P, const double* __restrict__ rot, int k_rot, int fpc,
                                                                                                const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n_frames,
                                                                                                unsigned long long src_stride, unsigned long long dst_stride,
                                                                                                const PbPlanar L, const int cx_arg, const int cy_arg) {
    static_assert(S == 1 || S == 2, "sample sizes of pb_track_stitch_planar / pb_track_stitch_nv12");
    const int cx = PAIRS ? 1 : cx_arg, cy = PAIRS ? 1 : cy_arg;  // (each 0 or 1; interleaved pairs are 4:2:0)
    const int W = P.dst.width, H = P.dst.height;
    const unsigned qpr = ((unsigned)W + PB_PX - 1) / PB_PX;  // quads per row
    const unsigned g = blockIdx.x * PB_BLOCK + threadIdx.x;
    unsigned y = g / qpr;
    if (y >= (unsigned)H) return;
    int x0 = (int)(g - y * qpr) * PB_PX;

    const int count = (W - x0 >= PB_PX) ? PB_PX : W - x0;
    double lat[PB_PX], lon[PB_PX];
    bool inv[PB_PX];
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
    const unsigned sw = (unsigned)P.src.width;
    const float inv_sw = __builtin_amdgcn_rcpf((float)sw);
    const int f0 = (int)blockIdx.y * fpc;
    const int f1 = (n_frames - f0 < fpc) ? n_frames : f0 + fpc;
    for (int f = f0; f < f1; ++f) {
        const uint8_t* __restrict__ s = src + (unsigned long long)f * src_stride;
        uint8_t* __restrict__ d = dst + (unsigned long long)f * dst_stride;
        // (the row and column are asked anew in every frame, in place: pb_track_video_kernel's reason)
        asm volatile("" : "+v"(y), "+v"(x0));
        const unsigned yy = y;
        const int xx = x0;
        const bool anchor_row = !(yy & (unsigned)cy);
        // (a pixel's three samples are 16 bits each at the most: packed two to a register while the other pixels' chains run)
        unsigned pa[PB_PX / 2] = {0u, 0u}, p1[PB_PX / 2] = {0u, 0u}, p2[PB_PX / 2] = {0u, 0u};
        PB_UNROLL(PB_FAITHFUL_UNROLL)
        for (int k = 0; k < PB_PX; ++k) {
            if (k < count) {
                PbCoord c;
                c.lat = lat[k];
                c.lon = lon[k];
                c.inv = inv[k];
                c.face = 0;
                const PbDoubleTap t = pb_src_double_taps(P, pb_track_rotate(rot, k_rot, f, c));
                const bool bl = t.il < 0, br = t.ir < 0, none = bl && br;
                unsigned rl, cl, rr, cr;
                pb_nv12_divmod((unsigned)(bl ? 0 : t.il), sw, inv_sw, rl, cl);
                pb_nv12_divmod((unsigned)(br ? 0 : t.ir), sw, inv_sw, rr, cr);
                const unsigned yl = pb_nv12_load_y<S>(s, rl * L.src_pitch + cl * (unsigned)S), yr = pb_nv12_load_y<S>(s, rr * L.src_pitch + cr * (unsigned)S);
                const unsigned v0 = none ? L.fill[0] : pb_sv_blend<S>(bl ? 0u : yl, br ? 0u : yr, t.fl, t.fr);
                pa[k >> 1] |= v0 << (16 * (k & 1));
                if (anchor_row && !(k & cx)) {  // (an anchor: its taps and factors serve the two chroma samples)
                    constexpr unsigned CS = PAIRS ? 2 * S : S;
                    unsigned c1l, c2l, c1r, c2r;
                    pb_video_load_c<S, PAIRS>(s, L, (rl >> cy) * L.src_cpitch + (cl >> cx) * CS, c1l, c2l);
                    pb_video_load_c<S, PAIRS>(s, L, (rr >> cy) * L.src_cpitch + (cr >> cx) * CS, c1r, c2r);
                    const unsigned v1 = none ? L.fill[1] : pb_sv_blend<S>(bl ? 0u : c1l, br ? 0u : c1r, t.fl, t.fr);
                    const unsigned v2 = none ? L.fill[2] : pb_sv_blend<S>(bl ? 0u : c2l, br ? 0u : c2r, t.fl, t.fr);
                    p1[k >> 1] |= v1 << (16 * (k & 1));
                    p2[k >> 1] |= v2 << (16 * (k & 1));
                }
            }
        }
        const unsigned a[PB_PX] = {pa[0] & 0xFFFFu, pa[0] >> 16, pa[1] & 0xFFFFu, pa[1] >> 16};
        pb_nv12_store_y<S, false>(d, L.dst_pitch, W, H, xx, (int)yy, a);
        if (anchor_row) {
            if constexpr (PAIRS) {  // (the anchors are the pixels k = 0, 2: the low halves)
                const unsigned uv[2] = {(p1[0] & 0xFFFFu) | ((p2[0] & 0xFFFFu) << (8 * S)), (p1[1] & 0xFFFFu) | ((p2[1] & 0xFFFFu) << (8 * S))};
                pb_nv12_store_uv<S, false>(d + L.dst_o1, L.dst_cpitch, W, H, xx, (int)yy, uv);
            } else if (cx == 0) {
                const unsigned c1[PB_PX] = {p1[0] & 0xFFFFu, p1[0] >> 16, p1[1] & 0xFFFFu, p1[1] >> 16};
                const unsigned c2[PB_PX] = {p2[0] & 0xFFFFu, p2[0] >> 16, p2[1] & 0xFFFFu, p2[1] >> 16};
                pb_nv12_store_y<S, false>(d + L.dst_o1, L.dst_cpitch, W, H, xx, (int)yy, c1);
                pb_nv12_store_y<S, false>(d + L.dst_o2, L.dst_cpitch, W, H, xx, (int)yy, c2);
            } else {
                const unsigned h1[2] = {p1[0] & 0xFFFFu, p1[1] & 0xFFFFu}, h2[2] = {p2[0] & 0xFFFFu, p2[1] & 0xFFFFu};
                pb_planar_store2<S, false>(d + L.dst_o1, L.dst_cpitch, W >> 1, H >> cy, xx >> 1, (int)(yy >> cy), h1);
                pb_planar_store2<S, false>(d + L.dst_o2, L.dst_cpitch, W >> 1, H >> cy, xx >> 1, (int)(yy >> cy), h2);
            }
        }
    }
}
