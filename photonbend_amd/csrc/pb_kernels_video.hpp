// pb_kernels_video.hpp - the nearest tile kernel for VIDEO frames (pb_video.hpp's frame model): planar 4:4:4 / 4:2:2 / 4:2:0 - yuv420p /
// yuv422p / yuv444p, their 10- and 16-bit forms, gbrp (pb_remap_planar) - and, as PAIRS, NV12 and P010 / P016
// (pb_remap_nv12).
//   plane 0   P0_out[y][x] = P0_src[r][c], (r, c) the plan's certified source pixel of (y, x); fill0 where that pixel is black.
//   chroma    Pk_out[i][j] = Pk_src[r >> CY][c >> CX] with (r, c) the source pixel of the sample's ANCHOR (i << CY, j << CX); fillk where
//             the anchor is black.  PAIRS: the pair of block (i, j) is UV_src[r >> 1][c >> 1], (fill_u, fill_v) where the anchor is black.
//             Only the anchor decides.  A nearest sample, no interpolation.
// So the tile models, certification, the exact-index tables, the fix lists and the launch-order table are those of the RGB8 plan,
// unchanged, as for pb_px_hot_kernel; this file adds the kernel that writes EVERY plane of a tile in one launch.  The 32 x 32 tile is
// even-aligned: a chroma block never straddles tiles.
//
// pb_video_hot_kernel<SRC_KIND, S, SUB, PAIRS> has pb_px_hot_kernel's launch shape: one wave per slot of the plan's nearest launch-order
// table, the entry in SGPRs (pb_load_entry), frames of a batch as a grid dimension, the parameter block behind a pointer, PbHot by value,
// static LDS.  A chroma value is held AS STORED: c1 and c2 the samples of planes 1 and 2, or (PAIRS) c1 the pair as loaded - one
// 2 * S-byte load - and c2 nothing; the fill of c1 is then the packed pair.
//   BLACK           fills.
//   LEAN / DIRECT   pb_px_hot_kernel's direct-gather path in the two certified evaluation orders (pb_gather_front), `dead` bits for
//   / MASKED        MASKED.  A lane holds 16 pixels of one line before the regrouping: p = lane & 31 is fixed and q = (2n + hh + shift) & 31
//                   has a parity that does not depend on n.  So the lanes that hold anchors hold nothing else: all 64 at 4:4:4, the 32
//                   with an even COLUMN at 4:2:2 (p or q, by the evaluation order), the 16 with an even p and q at 4:2:0.  THOSE LANES
//                   GATHER THE CHROMA of each of their pixels next to the plane-0 sample - every gather of a tile is in flight at once,
//                   which is what a gather-bound tile kernel wants - and the planes go through the regrouping buffer one after another,
//                   each stored as soon as it has been read back: three passes, two with PAIRS.  (The other way - the anchors' offsets
//                   through the buffer, the chroma gathered in the store shape - puts a second memory round trip behind the LDS pass.)
//   generic         pb_model_row / pb_model_px_rc; row and column stay apart (rows are pitched).  The lane is in the store shape, four
//                   pixels of a row: its anchors are the pixels k = 0 .. 3 (4:4:4) or k = 0, 2 (4:2:2, 4:2:0).  Every lane loads them (no
//                   load inside a branch); at 4:2:0 the lanes of even rows store them.
//   FAILED          the plan's exact indices (idx_tab); a stored index r * w + c is taken apart by pb_nv12_divmod (few pixels).  The
//                   loads of one row of a lane's pixels are in flight together, of all four rows with PAIRS (a pair plane is a third of
//                   the values).
//   fix pixels      re-copied through fix_px / fix_idx after the wave's own stores have completed (s_waitcnt vmcnt(0)); a fix pixel that
//                   is an anchor re-copies its chroma too.
//
// Movement, the scalar-register rule (layouts and fills in vector registers, fills applied after the loads from values the compiler
// cannot trace, pb_nv12_even asked anew at each use) and the limits: pb_video.hpp.  LDS: the regrouping buffer only, 4224 bytes per wave.
#pragma once
#include "pb_video.hpp"

template <int SRC_KIND, int S, int SUB, bool PAIRS>
__global__ __launch_bounds__(64 * PB_TILE_WAVES) void pb_video_hot_kernel(const PbParams* __restrict__ Pp, const PbHot Hd, const PbTileEntry* __restrict__ table,
                                                                           const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                           const unsigned groups_per_frame, unsigned long long src_stride,
                                                                           unsigned long long dst_stride, const int32_t* __restrict__ idx_tab,
                                                                           const int32_t* __restrict__ fix_px, const int32_t* __restrict__ fix_idx, const PbPlanar Ls) {
    static_assert(SUB == PB_SUB_444 || SUB == PB_SUB_422 || SUB == PB_SUB_420, "the subsamplings of pb_remap_planar");
    static_assert(!PAIRS || SUB == PB_SUB_420, "interleaved pairs are NV12 / P010: 4:2:0");
    constexpr int CX = pb_planar_cx(SUB), CY = pb_planar_cy(SUB);
    constexpr int NC = 4 >> CX;          // chroma values of a lane's four pixels of a row: at pixels k = j << CX
    constexpr int NP = PAIRS ? 1 : 2;    // chroma planes
    constexpr int NR = PAIRS ? 4 : 1;    // rows of a lane's pixels whose loads the failed path keeps in flight together
    PbPlanar L = pb_video_in_vgprs(Ls);  // (pb_video.hpp, "Scalar registers")
    if constexpr (PAIRS) {               // c1 is the pair as stored and c2 nothing
        L.fill[1] |= L.fill[2] << (8 * S);
        L.fill[2] = 0u;
    }
    constexpr bool NT = PB_NT_DEFAULT(SRC_KIND);  // (the RGB8 kernel's store policy, for its reasons: pb_store3)
    __shared__ unsigned lds[PB_TILE_WAVES][PB_PX_PLANE];
    const PbParams& P = *Pp;
    asm volatile("" ::"s"(table), "s"(Hd.dst_w), "s"(Hd.dst_h), "s"(Hd.src_w), "s"(Hd.src_h), "s"(groups_per_frame));
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned wg = blockIdx.x;
    if (wg >= groups_per_frame) {  // a batch: which frame
        const unsigned f = wg / groups_per_frame;
        wg -= f * groups_per_frame;
        src += (unsigned long long)f * src_stride;
        dst += (unsigned long long)f * dst_stride;
    }
    PbTileEntry entry;
    pb_load_entry(table + (wg * 4u + (unsigned)wave), entry);
    const PbTileEntry* __restrict__ e = &entry;
    const int flags = e->flags;
    if (flags & PB_TILE_SKIP) return;
    const int tx = e->tile_xy & 0xFFFF, ty = (int)((unsigned)e->tile_xy >> 16);
    const int X0 = tx * PB_TILE, Y0 = ty * PB_TILE;
    const int W = Hd.dst_w, H = Hd.dst_h;
    const unsigned sw = (unsigned)Hd.src_w;
    const float inv_sw = __builtin_amdgcn_rcpf((float)sw);
    const int xg = lane & 7, yb = lane >> 3;
    const int x = X0 + 4 * xg;  // the lane's store shape: columns x .. x + 3 of rows Y0 + yb + 8 * jr (Y0 and 8 * jr are even: yb decides a row's parity)
    // (the chroma planes are addressed from the frame's start, by 32-bit offsets: four plane pointers would be eight more live registers)

    if (flags & PB_TILE_FAILED) {
        const int32_t* __restrict__ slot = idx_tab + (size_t)e->aux_off * (PB_TILE * PB_TILE);
#pragma unroll
        for (int j0 = 0; j0 < 4; j0 += NR) {
            unsigned a[NR][4], c1[NR][4], c2[NR][4] = {}, black = 0u;
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int jr = j0 + i;
                const int4 v = *reinterpret_cast<const int4*>(slot + (yb + 8 * jr) * PB_TILE + 4 * xg);
                const int id[4] = {v.x, v.y, v.z, v.w};
                const bool row_in = Y0 + yb + 8 * jr < H;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    // (black or outside the image: a bit per pixel, for the fills after the loads - pb_video.hpp, "Scalar registers")
                    const int idk = (row_in && x + k < W) ? id[k] : -1;
                    black |= (unsigned)(idk < 0) << (4 * i + k);
                    unsigned r, c;
                    pb_nv12_divmod((unsigned)(idk < 0 ? 0 : idk), sw, inv_sw, r, c);
                    a[i][k] = pb_nv12_load_y<S>(src, r * L.src_pitch + c * (unsigned)S);
                    if (!(k & CX))  // (every lane loads - no load inside a branch, they are all in flight together; at 4:2:0 the lanes of even rows store)
                        pb_video_load_stored<S, PAIRS>(src, L, pb_video_coff<S, SUB, PAIRS>(L.src_cpitch, r, c), c1[i][k >> CX], c2[i][k >> CX]);
                }
            }
            asm volatile("" : "+v"(black));
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool b = (black >> (4 * i + k)) & 1u;
                    a[i][k] = b ? L.fill[0] : a[i][k];
                    if (!(k & CX)) {
                        c1[i][k >> CX] = b ? L.fill[1] : c1[i][k >> CX];
                        c2[i][k >> CX] = b ? L.fill[2] : c2[i][k >> CX];
                    }
                }
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                pb_nv12_store_y<S, true>(dst, L.dst_pitch, W, H, x, Y0 + yb + 8 * (j0 + i), a[i]);
                if (!CY || pb_nv12_even(yb)) pb_video_store_stored<S, SUB, PAIRS, true>(dst, L, W, H, x, Y0 + yb + 8 * (j0 + i), c1[i], c2[i]);
            }
        }
        return;  // (a failed tile has no fix pixels: its table slot holds them all)
    }
    if (flags & PB_TILE_BLACK) {
        const unsigned z0[4] = {L.fill[0], L.fill[0], L.fill[0], L.fill[0]}, z1[4] = {L.fill[1], L.fill[1], L.fill[1], L.fill[1]},
                       z2[4] = {L.fill[2], L.fill[2], L.fill[2], L.fill[2]};
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            pb_nv12_store_y<S, false>(dst, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, z0);
            if (!CY || pb_nv12_even(yb)) pb_video_store_stored<S, SUB, PAIRS, false>(dst, L, W, H, x, Y0 + yb + 8 * jr, z1, z2);
        }
    } else if (flags & (PB_TILE_LEAN | PB_TILE_DIRECT)) {
        // pb_px_hot_kernel's direct-gather path (its comments and pb_win_tile's hold here): every pixel of such a tile lies inside the
        // image and samples inside the tile's source box, in both evaluation orders (pb_certify_kernel)
        unsigned* win = lds[wave];
        unsigned rc[16];  // the certified source pixel: row << 16 | column (both below 32768)
        const PbGather g = pb_gather_front(e, lane, rc);
        // this lane's 16 pixels are all anchors (else none is): its column is p (along_x) or q, its row the other
        const int colpar = g.along_x ? g.p : g.hh + g.shift, rowpar = g.along_x ? g.hh + g.shift : g.p;
        const bool anchors = !(((colpar & CX) | (rowpar & CY)) & 1);
        unsigned t0[16], t1[16], t2[16];
        if (flags & PB_TILE_MASKED) {
            const unsigned dead = pb_gather_dead(P, g, X0, Y0);
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                t0[n] = L.fill[0];
                t1[n] = L.fill[1];
                t2[n] = L.fill[2];
                if (!((dead >> n) & 1u)) {  // (a dead pixel's address is not a certified one: no load)
                    t0[n] = pb_nv12_load_y<S>(src, (rc[n] >> 16) * L.src_pitch + (rc[n] & 0xFFFFu) * (unsigned)S);
                    if (anchors) pb_video_load_stored<S, PAIRS>(src, L, pb_video_coff<S, SUB, PAIRS>(L.src_cpitch, rc[n] >> 16, rc[n] & 0xFFFFu), t1[n], t2[n]);
                }
            }
        } else {
#pragma unroll
            for (int n = 0; n < 16; ++n) t0[n] = pb_nv12_load_y<S>(src, (rc[n] >> 16) * L.src_pitch + (rc[n] & 0xFFFFu) * (unsigned)S);
            if (anchors) {
#pragma unroll
                for (int n = 0; n < 16; ++n) pb_video_load_stored<S, PAIRS>(src, L, pb_video_coff<S, SUB, PAIRS>(L.src_cpitch, rc[n] >> 16, rc[n] & 0xFFFFu), t1[n], t2[n]);
            }
        }
        // park as [y][x], read back in the store shape and store: plane 0, then - through the same buffer - the chroma at its anchors
        {
            unsigned a[4][4];
#pragma unroll
            for (int n = 0; n < 16; ++n) win[g.at(n)] = t0[n];
            pb_wave_sync();
#pragma unroll
            for (int jr = 0; jr < 4; ++jr)
#pragma unroll
                for (int k = 0; k < 4; ++k) a[jr][k] = win[(yb + 8 * jr) * 33 + 4 * xg + k];
            pb_wave_sync();  // (the buffer's previous contents have been read)
#pragma unroll
            for (int jr = 0; jr < 4; ++jr) pb_nv12_store_y<S, NT>(dst, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, a[jr]);
        }
#pragma unroll
        for (int pl = 1; pl <= NP; ++pl) {
            unsigned c[4][4];
            if (anchors) {
#pragma unroll
                for (int n = 0; n < 16; ++n) win[g.at(n)] = (pl == 1) ? t1[n] : t2[n];
            }
            pb_wave_sync();
            if (!CY || pb_nv12_even(yb)) {
#pragma unroll
                for (int jr = 0; jr < 4; ++jr)
#pragma unroll
                    for (int j = 0; j < NC; ++j) c[jr][j] = win[(yb + 8 * jr) * 33 + 4 * xg + (j << CX)];
            }
            pb_wave_sync();
            if (!CY || pb_nv12_even(yb)) {
#pragma unroll
                for (int jr = 0; jr < 4; ++jr) {
                    if constexpr (PAIRS) pb_nv12_store_uv<S, NT>(dst + L.dst_o1, L.dst_cpitch, W, H, x, Y0 + yb + 8 * jr, c[jr]);
                    else pb_planar_store_c<S, SUB, NT>(dst + (pl == 1 ? L.dst_o1 : L.dst_o2), L.dst_cpitch, W, H, x, Y0 + yb + 8 * jr, c[jr]);
                }
            }
        }
    } else {
        // generic tile: validity, wrap and truncation edge per pixel; a packed (row << 16 | column), or -1 = black
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            PbRowModel R;
            pb_model_row(P, e, X0, Y0, yb + 8 * jr, 4 * xg, R);
            unsigned a[4], c1[4], c2[4] = {};
            int v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = pb_model_px_rc<SRC_KIND>(P, R, 4 * xg, k);
                const unsigned r = (unsigned)v[k] >> 16, c = (unsigned)v[k] & 0xFFFFu;
                a[k] = pb_nv12_load_y<S>(src, v[k] < 0 ? 0u : r * L.src_pitch + c * (unsigned)S);
                if (!(k & CX))  // (every lane loads; at 4:2:0 the lanes of even rows store)
                    pb_video_load_stored<S, PAIRS>(src, L, v[k] < 0 ? 0u : pb_video_coff<S, SUB, PAIRS>(L.src_cpitch, r, c), c1[k >> CX], c2[k >> CX]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // (the fills after the loads, from values the compiler cannot trace)
                asm volatile("" : "+v"(v[k]));
                a[k] = v[k] < 0 ? L.fill[0] : a[k];
                if (!(k & CX)) {
                    c1[k >> CX] = v[k] < 0 ? L.fill[1] : c1[k >> CX];
                    c2[k >> CX] = v[k] < 0 ? L.fill[2] : c2[k >> CX];
                }
            }
            pb_nv12_store_y<S, NT>(dst, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, a);
            if (!CY || pb_nv12_even(yb)) pb_video_store_stored<S, SUB, PAIRS, NT>(dst, L, W, H, x, Y0 + yb + 8 * jr, c1, c2);
        }
    }
    // this tile's fix pixels (where the model's truncation differs from the faithful one): re-copied through their exact indices
    // after the wave's own stores have completed; an anchor among them re-copies its chroma
    const int n_fix = e->fix_cnt;
    if (n_fix > 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane < n_fix) {
            const unsigned p = (unsigned)fix_px[e->fix_off + lane];
            const int id = fix_idx[e->fix_off + lane];
            unsigned y, xx, r, c;
            pb_nv12_divmod(p, (unsigned)W, __builtin_amdgcn_rcpf((float)W), y, xx);
            pb_nv12_divmod((unsigned)(id < 0 ? 0 : id), sw, inv_sw, r, c);
            const unsigned v0 = pb_nv12_load_y<S>(src, id < 0 ? 0u : r * L.src_pitch + c * (unsigned)S);
            pb_nv12_store_y1<S>(dst + (y * L.dst_pitch + xx * (unsigned)S), id < 0 ? L.fill[0] : v0);
            if (!(((xx & CX) | (y & CY)) & 1u)) {
                unsigned v1, v2 = 0u;
                pb_video_load_stored<S, PAIRS>(src, L, id < 0 ? 0u : pb_video_coff<S, SUB, PAIRS>(L.src_cpitch, r, c), v1, v2);
                // (with PAIRS v1 is the whole pair and v2 and its fill are 0: the pair goes out as it came in)
                pb_video_store_c1<S, SUB, PAIRS>(dst, L, y, xx, id < 0 ? L.fill[1] : v1, id < 0 ? L.fill[2] : v2);
            }
        }
    }
}
