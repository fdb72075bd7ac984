// pb_kernels_stitch_video.hpp - the nearest tile kernel for DOUBLE-fisheye video frames: NV12 / P010 and planar 4:4:4 / 4:2:2 / 4:2:0
// (pb_stitch_nv12, pb_stitch_planar).
//
// The frame is pb_video.hpp's: three planes of S-byte samples or, with PAIRS, planes 1 and 2 as one plane of interleaved pairs at
// 4:2:0; the plan is pb_kernels_double.hpp's, unchanged: two certified tile tables, the weight class of every tile
// (UNIT / ROW / LAT), the latitude table, the faithful taps and factors of failed tiles and fix pixels (PbDoubleFix), the launch-order
// table with its SOLO entries.  With (il, ir, fl, fr) the reference's taps and factors of an output pixel
//   blend(a_l, a_r) = cast((il < 0 ? 0.0 : a_l) * fl + (ir < 0 ? 0.0 : a_r) * fr), the cast pb_cvt_u8's widened to the sample: non-finite
//                     or |v| >= 2^31 gives 0, else truncate and keep the low 8 * S bits;
//   plane 0           out[y][x] = blend(P0[r_l][c_l], P0[r_r][c_r]), fill0 where both taps are black;
//   planes 1, 2       sample (i, j) has the ANCHOR (i << CY, j << CX): blend(Pk[r_l >> CY][c_l >> CX], Pk[r_r >> CY][c_r >> CX]) with the
//                     anchor's taps and factors, fillk where both of the anchor's taps are black.  Only the anchor decides.
//
// pb_stitch_video_kernel<S, SUB, PAIRS> has pb_hot_double_kernel's single-frame launch shape: one wave per slot of the double plan's
// launch-order table, frames of a batch as a grid dimension, the layouts and fills in vector registers (pb_video.hpp's rule).
//   SOLO slot       one eye at weight exactly 1, nothing on a fix list: the slot's entry is that eye's, in scalar registers, and the tile
//                   is a camera-source tile - pb_video_hot_kernel's BLACK and LEAN / DIRECT paths (an eye's tile is never MASKED), with
//                   the regrouping through LDS and the anchor lanes, the pair gathered whole with PAIRS.
//   two-eye tile    both entries lane-held (pb_desc_of_lanes, pb_coefs_of_lanes).  Per eye the certified source pixel of the lane's
//                   sixteen pixels (store shape: four pixels of four rows): pb_collapse_row_lanes + pb_eval_row + the entry's anchor for
//                   LEAN and DIRECT alike - no LDS windows, the RGB kernel's are laid out in 3-byte pixels -, pb_model_px_rc<EYE_L / _R>
//                   for generic tiles, black for a BLACK eye.  Each eye's plane-0 sample and, at the anchors, its chroma samples (or its
//                   pair) are gathered with exactly their S or 2 * S bytes; a black tap reads its plane's first sample and is zeroed
//                   after the load.  The weight mode is a wave-uniform run-time decision from the left entry's flags: UNIT the integer
//                   sum, ROW pb_blend_u8's float64 on rows[y], LAT on pb_merge_factor of the stored latitude; the anchor's factors
//                   serve its chroma.  The fills go where both taps are black.
//   FAILED tile     every pixel through tile_fix's PbDoubleFix (indices taken apart by pb_nv12_divmod); anchors redo their chroma.
//   fix pixels      behind s_waitcnt vmcnt(0) through px_fix; a fix pixel that is an anchor redoes its two chroma samples.
// Stores go through pb_nv12_store_y, pb_planar_store_c and pb_nv12_store_uv, clipped to their planes (plain stores, as for every double
// source).  Padding between rows, planes and frames is neither read nor written.  Byte offsets inside a frame are 32-bit: the calls
// refuse frames that span 2^31 bytes or more and sources of 32768 px a side or more.  LDS: the regrouping buffer, 4224 bytes per wave.
#pragma once
#include "pb_kernels_double.hpp"
#include "pb_video.hpp"

template <int S>
__device__ __forceinline__ unsigned pb_sv_cvt(double v) {  // pb_cvt_u8, keeping the low 8 * S bits
    if (!(fabs(v) < 2147483648.0)) return 0u;
    return ((unsigned)(int)v) & (S == 1 ? 0xFFu : 0xFFFFu);
}
template <int S>
__device__ __forceinline__ unsigned pb_sv_blend(unsigned l, unsigned r, double fl, double fr) {  // pb_blend_u8 on a sample
    return pb_sv_cvt<S>((double)l * fl + (double)r * fr);
}
// One output pixel through its stored faithful taps and factors: the plane-0 sample and, with CHROMA, the two chroma samples of the
// block it anchors.  Every load is issued before the first blend.
template <int S, int SUB, bool PAIRS, bool CHROMA>
__device__ __forceinline__ void pb_sv_tap(const uint8_t* __restrict__ src, const PbPlanar& L, const unsigned sw, const float inv_sw, const PbDoubleFix& t, unsigned& y,
                                          unsigned& c1, unsigned& c2) {
    const bool bl = t.il < 0, br = t.ir < 0;
    unsigned rl, cl, rr, cr;
    pb_nv12_divmod((unsigned)(bl ? 0 : t.il), sw, inv_sw, rl, cl);
    pb_nv12_divmod((unsigned)(br ? 0 : t.ir), sw, inv_sw, rr, cr);
    unsigned yl = pb_nv12_load_y<S>(src, rl * L.src_pitch + cl * (unsigned)S), yr = pb_nv12_load_y<S>(src, rr * L.src_pitch + cr * (unsigned)S);
    unsigned c1l = 0u, c2l = 0u, c1r = 0u, c2r = 0u;
    if constexpr (CHROMA) {
        pb_video_load_c<S, PAIRS>(src, L, pb_video_coff<S, SUB, PAIRS>(L.src_cpitch, rl, cl), c1l, c2l);
        pb_video_load_c<S, PAIRS>(src, L, pb_video_coff<S, SUB, PAIRS>(L.src_cpitch, rr, cr), c1r, c2r);
    }
    yl = bl ? 0u : yl;
    yr = br ? 0u : yr;
    y = (bl && br) ? L.fill[0] : pb_sv_blend<S>(yl, yr, t.fl, t.fr);
    if constexpr (CHROMA) {
        c1 = (bl && br) ? L.fill[1] : pb_sv_blend<S>(bl ? 0u : c1l, br ? 0u : c1r, t.fl, t.fr);
        c2 = (bl && br) ? L.fill[2] : pb_sv_blend<S>(bl ? 0u : c2l, br ? 0u : c2r, t.fl, t.fr);
    }
}

// one eye's certified source pixel of the lane's sixteen pixels (store shape), q[jr * 4 + k] = row << 16 | column, or -1 = black
template <int SRC_KIND>
__device__ __forceinline__ void pb_sv_eye_rc(const PbParams& P, const PbDesc& D, const PbTileEntry* __restrict__ e, const unsigned ve, const int X0, const int Y0,
                                             const int xg, const int yb, int q[16]) {
    if (PB_D_PLAIN(D.flags)) {
        const PbCoefs K = pb_coefs_of_lanes(ve);
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            pb_f2 a[5];
            pb_collapse_row_lanes(K, yb + 8 * jr, a);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const pb_f2 fv = pb_eval_row(a, pb_tile_coord(4 * xg + k));
                q[jr * 4 + k] = ((D.anchor_r + (int)fv.x) << 16) | (D.anchor_c + (int)fv.y);  // (>= 0: truncation == floor; both below 32768)
            }
        }
    } else if (PB_D_GENERIC(D.flags)) {
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            PbRowModel R;
            pb_model_row(P, e, X0, Y0, yb + 8 * jr, 4 * xg, R);
#pragma unroll
            for (int k = 0; k < 4; ++k) q[jr * 4 + k] = pb_model_px_rc<SRC_KIND>(P, R, 4 * xg, k);
        }
    } else {
#pragma unroll
        for (int n = 0; n < 16; ++n) q[n] = -1;  // BLACK: this eye contributes nothing to the tile
    }
}

// A SOLO slot: a camera-source tile of the live eye (entry in scalar registers) - pb_video_hot_kernel's BLACK and LEAN / DIRECT paths
template <int S, int SUB, bool PAIRS>
__device__ __forceinline__ void pb_sv_solo(const PbTileEntry* __restrict__ e, const int flags, const int X0, const int Y0, const int lane, unsigned* win,
                                           const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const PbPlanar& L, const int W, const int H) {
    constexpr int CX = pb_planar_cx(SUB), CY = pb_planar_cy(SUB);
    constexpr int NC = 4 >> CX;
    const int xg = lane & 7, yb = lane >> 3;
    const int x = X0 + 4 * xg;
    if (flags & PB_TILE_BLACK) {
        const unsigned z0[4] = {L.fill[0], L.fill[0], L.fill[0], L.fill[0]}, z1[4] = {L.fill[1], L.fill[1], L.fill[1], L.fill[1]},
                       z2[4] = {L.fill[2], L.fill[2], L.fill[2], L.fill[2]};
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            pb_nv12_store_y<S, false>(dst, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, z0);
            if (!CY || pb_nv12_even(yb)) pb_video_store_c<S, SUB, PAIRS>(dst, L, W, H, x, Y0 + yb + 8 * jr, z1, z2);
        }
        return;
    }
    // the direct-gather path in the two certified evaluation orders (pb_video_hot_kernel's comments hold): every pixel lies inside the
    // image and samples inside the tile's source box
    unsigned rc[16];  // the certified source pixel: row << 16 | column (both below 32768)
    const PbGather g = pb_gather_front(e, lane, rc);
    const int colpar = g.along_x ? g.p : g.hh + g.shift, rowpar = g.along_x ? g.hh + g.shift : g.p;
    const bool anchors = !(((colpar & CX) | (rowpar & CY)) & 1);  // this lane's 16 pixels are all anchors (else none is)
    unsigned t0[16], t1[16], t2[16];  // (PAIRS: t1 holds the pair as stored, t2 nothing)
#pragma unroll
    for (int n = 0; n < 16; ++n) t0[n] = pb_nv12_load_y<S>(src, (rc[n] >> 16) * L.src_pitch + (rc[n] & 0xFFFFu) * (unsigned)S);
    if (anchors) {
#pragma unroll
        for (int n = 0; n < 16; ++n) pb_video_load_stored<S, PAIRS>(src, L, pb_video_coff<S, SUB, PAIRS>(L.src_cpitch, rc[n] >> 16, rc[n] & 0xFFFFu), t1[n], t2[n]);
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
        for (int jr = 0; jr < 4; ++jr) pb_nv12_store_y<S, false>(dst, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, a[jr]);
    }
#pragma unroll
    for (int pl = 1; pl <= (PAIRS ? 1 : 2); ++pl) {
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
                if constexpr (PAIRS) pb_nv12_store_uv<S, false>(dst + L.dst_o1, L.dst_cpitch, W, H, x, Y0 + yb + 8 * jr, c[jr]);
                else pb_planar_store_c<S, SUB, false>(dst + (pl == 1 ? L.dst_o1 : L.dst_o2), L.dst_cpitch, W, H, x, Y0 + yb + 8 * jr, c[jr]);
            }
        }
    }
}

template <int S, int SUB, bool PAIRS>
__global__ __launch_bounds__(64 * PB_TILE_WAVES) void pb_stitch_video_kernel(const PbParams P, const PbTileEntry* __restrict__ table_l,
                                                                              const PbTileEntry* __restrict__ table_r, const PbTileEntry* __restrict__ ltable,
                                                                              const PbSepRow* __restrict__ rows, const double* __restrict__ lat_tab,
                                                                              const int32_t* __restrict__ fix_px, const PbDoubleFix* __restrict__ px_fix,
                                                                              const PbDoubleFix* __restrict__ tile_fix, const uint8_t* __restrict__ src,
                                                                              uint8_t* __restrict__ dst, const unsigned groups_per_frame,
                                                                              unsigned long long src_stride, unsigned long long dst_stride, const PbPlanar Ls) {
    static_assert(S == 1 || S == 2, "sample sizes of pb_stitch_planar / pb_stitch_nv12");
    static_assert(SUB == PB_SUB_444 || SUB == PB_SUB_422 || SUB == PB_SUB_420, "the subsamplings of pb_stitch_planar");
    static_assert(!PAIRS || SUB == PB_SUB_420, "interleaved pairs are 4:2:0");
    constexpr int CX = pb_planar_cx(SUB), CY = pb_planar_cy(SUB);
    const PbPlanar L = pb_video_in_vgprs(Ls);  // (pb_video.hpp, "Scalar registers")
    __shared__ unsigned lds[PB_TILE_WAVES][PB_PX_PLANE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned wg = blockIdx.x;
    if (wg >= groups_per_frame) {  // a batch: which frame
        const unsigned f = wg / groups_per_frame;
        wg -= f * groups_per_frame;
        src += (unsigned long long)f * src_stride;
        dst += (unsigned long long)f * dst_stride;
    }
    const int W = P.dst.width, H = P.dst.height;
    const unsigned vslot = (unsigned)__builtin_amdgcn_readfirstlane((int)(wg * (unsigned)PB_TILE_WAVES + (unsigned)wave));
    int tx, ty;
    {
        PbTileEntry entry;
        pb_load_entry(ltable + vslot, entry);
        if (entry.flags & PB_TILE_SKIP) return;
        tx = entry.tile_xy & 0xFFFF;
        ty = (int)((unsigned)entry.tile_xy >> 16);
        if (entry.flags & PB_TILE_SOLO) {
            pb_sv_solo<S, SUB, PAIRS>(&entry, entry.flags, tx * PB_TILE, ty * PB_TILE, lane, lds[wave], src, dst, L, W, H);
            return;
        }
    }
    const int X0 = tx * PB_TILE, Y0 = ty * PB_TILE;
    const int xg = lane & 7, yb = lane >> 3;
    const int x = X0 + 4 * xg;
    const unsigned sw = (unsigned)P.src.width;
    const float inv_sw = __builtin_amdgcn_rcpf((float)sw);
    const size_t tile = (size_t)ty * pb_tiles_x(P) + tx;
    const PbTileEntry* __restrict__ el = table_l + tile;
    const PbTileEntry* __restrict__ er = table_r + tile;
    // both entries: one coalesced 256-byte vector load each, in flight together
    const unsigned vl = reinterpret_cast<const unsigned*>(el)[lane], vr = reinterpret_cast<const unsigned*>(er)[lane];
    const PbDesc DL = pb_desc_of_lanes(vl), DR = pb_desc_of_lanes(vr);
    if ((DL.flags | DR.flags) & PB_TILE_FAILED) {
        // failed tile: every pixel through its stored faithful taps and factors (a tile's pixels beyond the image hold the taps of a
        // clamped pixel and are never stored)
        const PbDoubleFix* __restrict__ slot = tile_fix + (size_t)pb_lane_i(vr, PB_E_DWORD(aux_off)) * (PB_TILE * PB_TILE);
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            unsigned a[4], c1[4], c2[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const PbDoubleFix t = slot[(yb + 8 * jr) * PB_TILE + 4 * xg + k];
                if (!(k & CX)) {  // (every lane gathers its anchors' chroma; at 4:2:0 the lanes of even rows store it)
                    pb_sv_tap<S, SUB, PAIRS, true>(src, L, sw, inv_sw, t, a[k], c1[k >> CX], c2[k >> CX]);
                } else {
                    unsigned n1, n2;
                    pb_sv_tap<S, SUB, PAIRS, false>(src, L, sw, inv_sw, t, a[k], n1, n2);
                }
            }
            pb_nv12_store_y<S, false>(dst, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, a);
            if (!CY || pb_nv12_even(yb)) pb_video_store_c<S, SUB, PAIRS>(dst, L, W, H, x, Y0 + yb + 8 * jr, c1, c2);
        }
        return;  // (a failed tile has no fix pixels: its slot holds them all)
    }
    // the weight mode of the tile (pb_double_pair_kernel): wave-uniform
    const bool by_row = (DL.flags & PB_TILE_W_ROW) != 0, by_lat = (DL.flags & PB_TILE_W_LAT) != 0;
    int ql[16], qr[16];
    pb_sv_eye_rc<PB_KIND_EYE_L>(P, DL, el, vl, X0, Y0, xg, yb, ql);
    pb_sv_eye_rc<PB_KIND_EYE_R>(P, DR, er, vr, X0, Y0, xg, yb, qr);
    const double* __restrict__ lt = lat_tab + (by_lat ? (size_t)pb_lane_i(vl, PB_E_DWORD(aux_off)) * PB_LAT_TILE_DOUBLES : (size_t)0);
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) {
        unsigned yl[4], yr[4], c1l[4], c2l[4], c1r[4], c2r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int vL = ql[jr * 4 + k], vR = qr[jr * 4 + k];
            const unsigned rl = (unsigned)vL >> 16, cl = (unsigned)vL & 0xFFFFu, rr = (unsigned)vR >> 16, cr = (unsigned)vR & 0xFFFFu;
            yl[k] = pb_nv12_load_y<S>(src, vL < 0 ? 0u : rl * L.src_pitch + cl * (unsigned)S);
            yr[k] = pb_nv12_load_y<S>(src, vR < 0 ? 0u : rr * L.src_pitch + cr * (unsigned)S);
            if (!(k & CX)) {  // (every lane gathers its anchors' chroma - no load inside a branch; at 4:2:0 the lanes of even rows store it)
                pb_video_load_c<S, PAIRS>(src, L, vL < 0 ? 0u : pb_video_coff<S, SUB, PAIRS>(L.src_cpitch, rl, cl), c1l[k >> CX], c2l[k >> CX]);
                pb_video_load_c<S, PAIRS>(src, L, vR < 0 ? 0u : pb_video_coff<S, SUB, PAIRS>(L.src_cpitch, rr, cr), c1r[k >> CX], c2r[k >> CX]);
            }
        }
        double wl[4], wr[4];
        if (by_lat) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double t = lt[(yb + 8 * jr) * PB_TILE + 4 * xg + k];
                wl[k] = pb_merge_factor(P, t);
                wr[k] = pb_merge_factor(P, (t * -1.0) + PB_PI);  // the right eye's latitude, projection.py:426-427
            }
        } else if (by_row) {
            const PbSepRow R = rows[min(Y0 + yb + 8 * jr, H - 1)];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                wl[k] = R.f_l;
                wr[k] = R.f_r;
            }
        }
        unsigned a[4], c1[4], c2[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int vL = ql[jr * 4 + k], vR = qr[jr * 4 + k];
            asm volatile("" : "+v"(vL));  // (the blacks after the loads, from values the compiler cannot trace: pb_video.hpp)
            asm volatile("" : "+v"(vR));
            const bool bl = vL < 0, br = vR < 0, none = bl && br;
            constexpr unsigned mask = S == 1 ? 0xFFu : 0xFFFFu;
            const unsigned l0 = bl ? 0u : yl[k], r0 = br ? 0u : yr[k];
            if (by_lat || by_row) a[k] = pb_sv_blend<S>(l0, r0, wl[k], wr[k]);
            else a[k] = (l0 + r0) & mask;  // UNIT: l * 1.0 + r * 1.0 is the exact integer l + r, the cast keeps its low bits
            a[k] = none ? L.fill[0] : a[k];
            if (!(k & CX)) {
                const int j = k >> CX;
                const unsigned l1 = bl ? 0u : c1l[j], r1 = br ? 0u : c1r[j], l2 = bl ? 0u : c2l[j], r2 = br ? 0u : c2r[j];
                if (by_lat || by_row) {
                    c1[j] = pb_sv_blend<S>(l1, r1, wl[k], wr[k]);
                    c2[j] = pb_sv_blend<S>(l2, r2, wl[k], wr[k]);
                } else {
                    c1[j] = (l1 + r1) & mask;
                    c2[j] = (l2 + r2) & mask;
                }
                c1[j] = none ? L.fill[1] : c1[j];
                c2[j] = none ? L.fill[2] : c2[j];
            }
        }
        pb_nv12_store_y<S, false>(dst, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, a);
        if (!CY || pb_nv12_even(yb)) pb_video_store_c<S, SUB, PAIRS>(dst, L, W, H, x, Y0 + yb + 8 * jr, c1, c2);
    }
    // the tile's fix pixels (either eye's list; a pixel listed by both is written twice): through their stored taps, after the wave's own
    // stores have completed; an anchor among them redoes its two chroma samples
    const int nl = pb_lane_i(vl, PB_E_DWORD(fix_cnt)), nr = pb_lane_i(vr, PB_E_DWORD(fix_cnt));  // <= PB_TILE_FAIL_LIMIT each
    if (nl + nr > 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        for (int base = 0; base < nl + nr; base += 64) {
            const int n = base + lane;
            if (n < nl + nr) {
                const int item = n < nl ? pb_lane_i(vl, PB_E_DWORD(fix_off)) + n : pb_lane_i(vr, PB_E_DWORD(fix_off)) + (n - nl);
                const unsigned p = (unsigned)fix_px[item];
                const PbDoubleFix t = px_fix[item];
                unsigned y, xx, v0, v1, v2;
                pb_nv12_divmod(p, (unsigned)W, __builtin_amdgcn_rcpf((float)W), y, xx);
                if (!(((xx & CX) | (y & CY)) & 1u)) {
                    pb_sv_tap<S, SUB, PAIRS, true>(src, L, sw, inv_sw, t, v0, v1, v2);
                    pb_video_store_c1<S, SUB, PAIRS>(dst, L, y, xx, v1, v2);
                } else {
                    pb_sv_tap<S, SUB, PAIRS, false>(src, L, sw, inv_sw, t, v0, v1, v2);
                }
                pb_nv12_store_y1<S>(dst + (y * L.dst_pitch + xx * (unsigned)S), v0);
            }
        }
    }
}

// Diagnostic (pb_plan_stitch_tile_mix): what the waves of a stitch launch meet, slot by slot of the launch-order table.  counters:
// [0] SOLO slots, [1] / [2] / [3] two-eye tiles of weight class UNIT / ROW / LAT, [4] failed tiles, [5] two-eye tiles with fix pixels,
// [6] their fix pixels, [7] / [8] of those the chroma anchors at 4:2:2 / at 4:2:0
__global__ void pb_stitch_mix_kernel(const PbTileEntry* __restrict__ ltable, unsigned n_slots, const PbTileEntry* __restrict__ table_l,
                                     const PbTileEntry* __restrict__ table_r, int tiles_x, const int32_t* __restrict__ fix_px, int W,
                                     unsigned* __restrict__ counters) {
    const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_slots) return;
    const PbTileEntry& s = ltable[v];
    if (s.flags & PB_TILE_SKIP) return;
    if (s.flags & PB_TILE_SOLO) {
        atomicAdd(&counters[0], 1u);
        return;
    }
    const size_t tile = (size_t)((unsigned)s.tile_xy >> 16) * tiles_x + (s.tile_xy & 0xFFFF);
    const PbTileEntry &l = table_l[tile], &r = table_r[tile];
    if ((l.flags | r.flags) & PB_TILE_FAILED) {
        atomicAdd(&counters[4], 1u);
        return;
    }
    atomicAdd(&counters[(l.flags & PB_TILE_W_LAT) ? 3 : (l.flags & PB_TILE_W_ROW) ? 2 : 1], 1u);
    const int n = l.fix_cnt + r.fix_cnt;
    if (n <= 0) return;
    unsigned a422 = 0, a420 = 0;
    for (int k = 0; k < n; ++k) {
        const int p = fix_px[k < l.fix_cnt ? l.fix_off + k : r.fix_off + (k - l.fix_cnt)], y = p / W, x = p - y * W;
        a422 += !(x & 1);
        a420 += !((x | y) & 1);
    }
    atomicAdd(&counters[5], 1u);
    atomicAdd(&counters[6], (unsigned)n);
    atomicAdd(&counters[7], a422);
    atomicAdd(&counters[8], a420);
}
