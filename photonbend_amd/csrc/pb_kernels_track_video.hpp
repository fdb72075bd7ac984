// pb_kernels_track_video.hpp - ROTATION TRACKS FOR VIDEO FRAMES (pb_remap_track_planar; pb_remap_track_nv12):
// planar 4:4:4 / 4:2:2 / 4:2:0 frames and NV12 / P010 / P016, every frame with rotations of its own, every plane of every frame in one
// launch.  Frame f is the definition of pb_kernels_video.hpp with the index map of the float64 chain "the plan's own rotations followed by
// frame f's" (pb_kernels_track.hpp).  No arithmetic is new: the chain is pb_track_body's, the loads, fills and stores are
// pb_video_hot_kernel's.  The plan's tables are never read.
//
// pb_track_video_kernel<S, SRC_KIND, PAIRS> is built on the skeleton of pb_kernels_track.hpp (what is live across the frame loop, the
// chunks, the matrices as scalar operands, the row and column asked anew per frame, the packed samples, the stores).  What differs from
// pb_track_body:
//   quads         rows are pitched, so a work-item owns PB_PX = 4 consecutive pixels of ONE row; quads are counted per row (a row's last
//                 quad holds 1 to 4 pixels: 4:4:4 takes odd widths).
//   subsampling   a RUN-TIME, wave-uniform argument (cx, cy - the shifts of the chroma planes), not a template parameter: the kernel is
//                 bound by float64 transcendentals, and three times the float64 instantiations would cost build time for nothing.
//   PAIRS         NV12 / P010: planes 1 and 2 as one plane of interleaved pairs, 4:2:0 - (cx, cy) = (1, 1) whatever the arguments.  An
//                 anchor's pair is loaded whole and held as stored.
//   chroma        a quad starts at a multiple of four, so on a row with y & ((1 << cy) - 1) == 0 its pixels k with k & ((1 << cx) - 1) == 0
//                 are anchors, and the work-item already holds their source index: it gathers the two source samples (the pair) and
//                 stores them in row y >> cy of planes 1 and 2 (of the pair plane).  Chroma costs no float64.  Consecutive work-items walk
//                 along a row, so whether the row holds anchors is uniform across every wave that does not straddle a row's end.
//   index         the chain's index r * w + c comes apart through pb_nv12_divmod - exact for the sources this call takes (below 32768 px a
//                 side: a row number far below 2^22).
//   loads         exactly S or 2 * S bytes, branch-free, the fill applied after the load; the stores are pb_track_video_store's, with
//                 the samples as stored (AS_STORED).  Padding between rows, planes and frames is neither read nor written.
//
// Limits.  Byte offsets inside a frame are 32-bit: the calls refuse frames whose span reaches 2^31 bytes before any launch.
// grid: (quads of a frame / PB_BLOCK, chunks of fpc frames).
#pragma once
#include "pb_video.hpp"
#include "pb_kernels_track.hpp"

// (the sample size comes first: tests/test_isa_eac.py lists, by their first template argument, the kernels of an equi-angular source that
//  existed when it was written; this kernel's instantiations are pinned per source kind by tests/test_isa_track_nv12.py and test_isa_planar.py)
template <int S, int SRC_KIND, bool PAIRS>
__global__ __launch_bounds__(PB_BLOCK, PB_TRACK_WPE(SRC_KIND)) void pb_track_video_kernel(const PbParams P, const double* __restrict__ rot, int k_rot, int fpc,
                                                                                         const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n_frames,
                                                                                         unsigned long long src_stride, unsigned long long dst_stride, const PbPlanar L,
                                                                                         const int cx_arg, const int cy_arg) {
    static_assert(SRC_KIND == PB_KIND_PANO || SRC_KIND == PB_KIND_CAMERA || pb_is_cube(SRC_KIND), "a single source (a double fisheye's blend is sample-typed)");
    const int cx = PAIRS ? 1 : cx_arg, cy = PAIRS ? 1 : cy_arg;  // (each 0 or 1; interleaved pairs are 4:2:0)
    const unsigned fill1 = PAIRS ? L.fill[1] | (L.fill[2] << (8 * S)) : L.fill[1];  // (the pair as stored)
    // (the pair plane's rows are the luma rows' distance apart: two scalar registers fewer across the frame loop)
    const unsigned src_cpitch = PAIRS ? L.src_pitch : L.src_cpitch, dst_cpitch = PAIRS ? L.dst_pitch : L.dst_cpitch;
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
    const unsigned sw = (unsigned)P.src.width;
    const float inv_sw = __builtin_amdgcn_rcpf((float)sw);
    const PbTrackChunk ch = pb_track_chunk(fpc, n_frames);
    for (int f = ch.f0; f < ch.f1; ++f) {
        const uint8_t* __restrict__ s = src + (unsigned long long)f * src_stride;
        uint8_t* __restrict__ d = dst + (unsigned long long)f * dst_stride;
        pb_track_reask(y, x0);
        const unsigned yy = y;
        const int xx = x0;
        const bool anchor_row = !(yy & (unsigned)cy);  // (cy is 0 or 1)
        unsigned pa[PB_PX / 2] = {0u, 0u}, p1[PB_PX / 2] = {0u, 0u}, p2[PB_PX / 2] = {0u, 0u};  // (pb_track_pack)
        PB_UNROLL(PB_FAITHFUL_UNROLL)
        for (int k = 0; k < PB_PX; ++k) {
            if (k < count) {
                const int id = pb_exact_index_of<SRC_KIND>(P, pb_track_quad_coord(lat, lon, inv, k, rot, k_rot, f));
                unsigned r, col;
                pb_nv12_divmod((unsigned)(id < 0 ? 0 : id), sw, inv_sw, r, col);
                const unsigned v0 = pb_nv12_load_y<S>(s, id < 0 ? 0u : r * L.src_pitch + col * (unsigned)S);
                pb_track_pack(pa, k, id < 0 ? L.fill[0] : v0);
                if (anchor_row && !(k & cx)) {  // (an anchor; cx is 0 or 1)
                    unsigned v1, v2 = 0u;
                    pb_video_load_stored<S, PAIRS>(s, L, id < 0 ? 0u : (r >> cy) * src_cpitch + (col >> cx) * (unsigned)(PAIRS ? 2 * S : S), v1, v2);
                    pb_track_pack(p1, k, id < 0 ? fill1 : v1);
                    if constexpr (!PAIRS) pb_track_pack(p2, k, id < 0 ? L.fill[2] : v2);
                }
            }
        }
        pb_track_video_store<S, PAIRS, true>(d, L, W, H, xx, yy, cx, cy, anchor_row, dst_cpitch, pa, p1, p2);
    }
}
