// pb_kernels_track_nv12.hpp - ROTATION TRACKS FOR 4:2:0 SEMI-PLANAR VIDEO FRAMES (pb_remap_track_nv12): NV12 and P010 / P016
// frames, every frame with rotations of its own, both planes of every frame in one launch.  Frame f is the definition of
// pb_kernels_nv12.hpp with the index map of the float64 chain "the plan's own rotations followed by frame f's" (pb_kernels_track.hpp):
//   luma     Y_out[y][x] = Y_src[r][c], (r, c) the chain's source pixel of (y, x); fill_y where that pixel is black.
//   chroma   the pair of output block (i, j) is UV_src[r >> 1][c >> 1] with (r, c) the source pixel of the block's ANCHOR (2i, 2j);
//            (fill_u, fill_v) where the anchor is black.  Only the anchor decides.
// No arithmetic is new: the chain is pb_track_body's, the planes, loads, fills and stores are pb_nv12_hot_kernel's.  The plan's tables
// are never read.
//
// pb_track_nv12_kernel<S, SRC_KIND> has pb_track_body's structure: pb_chain<PB_ROT_ANY> once per pixel, two float64 and a flag per pixel
// live across the frame loop, frames chunked over blockIdx.y (`fpc` per chunk), the frame's matrices through pb_track_rotate (a uniform
// address: scalar loads).  What differs:
//   quads    rows are pitched, so a work-item owns PB_PX = 4 consecutive luma pixels of ONE row; quads are counted per row, ceil(W / 4)
//            of them.  W is even: the last quad of a row holds 4 pixels or 2, never 1 or 3.
//   chroma   a quad starts at an even column, so on an even row its pixels k = 0 and k = 2 are the anchors of two adjacent output pairs,
//            and the work-item already holds their source index: it gathers the two source pairs and stores them at the same column byte
//            offset as its luma, in row y >> 1 of the chroma plane.  Work-items of odd rows touch no chroma; chroma costs no float64.
//            Consecutive work-items walk along a row, so whether the row is even is uniform across every wave that does not straddle
//            a row's end (all but at most one wave per row): the chroma branch is a scalar one nearly everywhere.
//   index    the chain's index r * w + c comes apart through pb_nv12_divmod - exact for the sources this call takes (below 32768 px a
//            side: a row number far below 2^22).
//   stores   pb_nv12_store_y / pb_nv12_store_uv: four luma samples, or two pairs, in one 4 * S-byte store where the address allows, else
//            sample by sample / pair by pair, clipped to the row.  Loads take exactly S or 2 * S bytes (pb_nv12_y_rc / pb_nv12_uv_rc:
//            branch-free, the fill applied after the load).  Padding between rows, planes and frames is neither read nor written.
//
// Limits.  Byte offsets inside a frame are 32-bit: pb_remap_track_nv12 refuses frames whose span reaches 2^31 bytes before any launch.
// grid: (quads of a frame / PB_BLOCK, chunks of fpc frames).
#pragma once
#include "pb_kernels_nv12.hpp"
#include "pb_kernels_track.hpp"

// (the sample size comes first: tests/test_isa_eac.py lists, by their first template argument, the kernels of an equi-angular source that
//  existed when it was written; this kernel's instantiations are pinned per source kind by tests/test_isa_track_nv12.py)
template <int S, int SRC_KIND>
__global__ __launch_bounds__(PB_BLOCK, PB_TRACK_WPE(SRC_KIND)) void pb_track_nv12_kernel(const PbParams P, const double* __restrict__ rot, int k_rot, int fpc,
                                                                                        const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n_frames,
                                                                                        unsigned long long src_stride, unsigned long long dst_stride, const PbNv12 L) {
    static_assert(SRC_KIND == PB_KIND_PANO || SRC_KIND == PB_KIND_CAMERA || pb_is_cube(SRC_KIND), "a single source (a double fisheye's blend is sample-typed)");
    const int W = P.dst.width, H = P.dst.height;
    const unsigned qpr = ((unsigned)W + PB_PX - 1) / PB_PX;  // quads per row
    const unsigned g = blockIdx.x * PB_BLOCK + threadIdx.x;
    const unsigned y = g / qpr;
    if (y >= (unsigned)H) return;
    const int x0 = (int)(g - y * qpr) * PB_PX;
    const int count = (W - x0 >= PB_PX) ? PB_PX : W - x0;  // 4 or 2
    const bool even_row = !(y & 1u);

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
        unsigned a[PB_PX], uv[2];
        PB_UNROLL(PB_FAITHFUL_UNROLL)
        for (int k = 0; k < PB_PX; ++k) {
            a[k] = 0u;
            if (!(k & 1)) uv[k >> 1] = 0u;
            if (k < count) {
                PbCoord c;
                c.lat = lat[k];
                c.lon = lon[k];
                c.inv = inv[k];
                c.face = 0;
                const int id = pb_exact_index_of<SRC_KIND>(P, pb_track_rotate(rot, k_rot, f, c));
                unsigned r, col;
                pb_nv12_divmod((unsigned)(id < 0 ? 0 : id), sw, inv_sw, r, col);
                a[k] = pb_nv12_y_rc<S>(s, L, (int)r, (int)col, id < 0);
                if (!(k & 1) && even_row) uv[k >> 1] = pb_nv12_uv_rc<S>(s, L, (int)r, (int)col, id < 0);  // (an anchor)
            }
        }
        pb_nv12_store_y<S, false>(d, L.dst_pitch, W, H, x0, (int)y, a);
        if (even_row) pb_nv12_store_uv<S, false>(d + L.dst_uv, L.dst_pitch, W, H, x0, (int)y, uv);
    }
}
