// pb_kernels_track_stitch.hpp - ROTATION TRACKS FOR DOUBLE-FISHEYE VIDEO FRAMES (pb_track_stitch_planar, pb_track_stitch_nv12):
// NV12 / P010 and planar 4:4:4 / 4:2:2 / 4:2:0 frames of a side-by-side double fisheye, every frame with rotations of its own, every plane
// of every frame in one launch.  Frame f is the definition of pb_kernels_stitch_video.hpp - blend, anchors, fills, cast - with the taps
// and factors (il, ir, fl, fr) of the float64 chain "the plan's own rotations followed by frame f's" (pb_kernels_track.hpp).  No arithmetic
// is new: the chain is pb_track_body's, the taps are pb_src_double_taps' (one pb_expi_np for both eyes, as in pb_track_px), the blend is
// pb_sv_blend, the loads and stores are the stitch kernel's.  The plan's tables are never read.
//
// pb_track_stitch_kernel<S, PAIRS> has pb_track_video_kernel's structure - the skeleton of pb_kernels_track.hpp, a work-item owns
// PB_PX = 4 consecutive pixels of ONE row (a row's last quad holds 1 to 4 pixels).
//   PAIRS         planes 1 and 2 as one plane of interleaved pairs (NV12 / P010), 4:2:0.  Otherwise three planes, the subsampling a
//                 RUN-TIME, wave-uniform (cx, cy) for pb_track_video_kernel's reason.
//   taps          each tap comes apart through pb_nv12_divmod; each eye's plane-0 sample is loaded with exactly S bytes and, on anchors,
//                 its two chroma samples (PAIRS: one 2 * S-byte pair) at (r >> cy, c >> cx).  A black tap reads its plane's first sample
//                 and is zeroed after the load: branch-free, never out of bounds.  The anchor's factors serve its chroma.
//   fills         where both taps are black (an invalid destination pixel has both).
//   stores        pb_track_video_store's, U in p1 and V in p2.  Padding between rows, planes and frames is neither read nor written.
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
    PB_UNROLL(PB_FAITHFUL_UNROLL)  // (pb_track_fill_row's text, kept by the letter of the rate criterion: experiments/README.md)
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
                const PbDoubleTap t = pb_src_double_taps(P, pb_track_quad_coord(lat, lon, inv, k, rot, k_rot, f));
                const bool bl = t.il < 0, br = t.ir < 0, none = bl && br;
                unsigned rl, cl, rr, cr;
                pb_nv12_divmod((unsigned)(bl ? 0 : t.il), sw, inv_sw, rl, cl);
                pb_nv12_divmod((unsigned)(br ? 0 : t.ir), sw, inv_sw, rr, cr);
                const unsigned yl = pb_nv12_load_y<S>(s, rl * L.src_pitch + cl * (unsigned)S), yr = pb_nv12_load_y<S>(s, rr * L.src_pitch + cr * (unsigned)S);
                const unsigned v0 = none ? L.fill[0] : pb_sv_blend<S>(bl ? 0u : yl, br ? 0u : yr, t.fl, t.fr);
                pb_track_pack(pa, k, v0);
                if (anchor_row && !(k & cx)) {  // (an anchor: its taps and factors serve the two chroma samples)
                    constexpr unsigned CS = PAIRS ? 2 * S : S;
                    unsigned c1l, c2l, c1r, c2r;
                    pb_video_load_c<S, PAIRS>(s, L, (rl >> cy) * L.src_cpitch + (cl >> cx) * CS, c1l, c2l);
                    pb_video_load_c<S, PAIRS>(s, L, (rr >> cy) * L.src_cpitch + (cr >> cx) * CS, c1r, c2r);
                    const unsigned v1 = none ? L.fill[1] : pb_sv_blend<S>(bl ? 0u : c1l, br ? 0u : c1r, t.fl, t.fr);
                    const unsigned v2 = none ? L.fill[2] : pb_sv_blend<S>(bl ? 0u : c2l, br ? 0u : c2r, t.fl, t.fr);
                    pb_track_pack(p1, k, v1);
                    pb_track_pack(p2, k, v2);
                }
            }
        }
        pb_track_video_store<S, PAIRS, false>(d, L, W, H, xx, yy, cx, cy, anchor_row, L.dst_cpitch, pa, p1, p2);
    }
}
