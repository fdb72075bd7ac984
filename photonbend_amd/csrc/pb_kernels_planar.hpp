// pb_kernels_planar.hpp - the nearest tile kernel for PLANAR video frames: three planes of S-byte samples, 4:4:4, 4:2:2 or 4:2:0
// (pb_remap_planar) - yuv420p / yuv422p / yuv444p, their 10- and 16-bit forms, gbrp.
//
// Plane 0 is full resolution, (h, w); planes 1 and 2 are (h >> CY, w >> CX) each, (CX, CY) = (0, 0) at 4:4:4, (1, 0) at 4:2:2, (1, 1) at
// 4:2:0.  Plane 0's rows are `pitch` bytes apart, the rows of planes 1 and 2 `cpitch`; the planes start at byte offsets 0, o1, o2 of the
// frame, in any order.  Widths are multiples of 1 << CX and heights of 1 << CY, source and destination alike.
//   plane 0       P0_out[y][x] = P0_src[r][c], (r, c) the plan's certified source pixel of (y, x); fill0 where that pixel is black.
//   planes 1, 2   Pk_out[i][j] = Pk_src[r >> CY][c >> CX] with (r, c) the source pixel of the sample's ANCHOR, the top-left pixel
//                 (i << CY, j << CX) of its block; fillk where the anchor is black.  Only the anchor decides.  A nearest sample.
// This is pb_kernels_nv12.hpp's definition with the pair taken apart into two planes and the block's shape a parameter, so the tile
// models, certification, the exact-index tables, the fix lists and the launch-order table are those of the RGB8 plan, unchanged.
//
// pb_planar_hot_kernel<SRC_KIND, S, SUB> has pb_nv12_hot_kernel's launch shape (one wave per slot of the nearest launch-order table, the
// entry in SGPRs, frames as a grid dimension, PbHot by value, the static regrouping LDS) and its paths:
//   BLACK           fills.
//   LEAN / DIRECT   the direct-gather path in the two certified evaluation orders, `dead` bits for MASKED.  A lane holds 16 pixels of one
//   / MASKED        line before the regrouping: p = lane & 31 is fixed and q = (2n + hh + shift) & 31 has a parity that does not depend on
//                   n.  So the lanes that hold anchors hold nothing else: all 64 at 4:4:4, the 32 with an even COLUMN at 4:2:2 (p or q,
//                   by the evaluation order), the 16 with an even p and q at 4:2:0.  Those lanes gather the two chroma samples of each of
//                   their pixels next to the plane-0 sample - every gather of a tile is in flight at once - and the three planes go
//                   through the regrouping buffer one after another, each stored as soon as it has been read back.
//   generic         pb_model_row / pb_model_px_rc.  The lane is in the store shape, four pixels of a row: its anchors are the pixels
//                   k = 0 .. 3 (4:4:4) or k = 0, 2 (4:2:2, 4:2:0).  Every lane loads them (no load inside a branch); at 4:2:0 the
//                   lanes of even rows store them.
//   FAILED          the plan's exact indices (idx_tab), taken apart by pb_nv12_divmod.
//   fix pixels      re-copied through fix_px / fix_idx behind s_waitcnt vmcnt(0); a fix pixel that is an anchor re-copies its two
//                   chroma samples.
//
// Movement.  Pointers, pitches, offsets and strides are multiples of S and nothing more.  Every sample is loaded with exactly its S bytes,
// so no load touches a byte outside its plane; a black pixel reads its plane's first sample and takes the fill after the load.  A lane's
// four plane-0 samples of a row - at 4:4:4 its four samples of a chroma plane too - leave in one 4 * S-byte store where the address is
// 4-byte aligned, its two chroma samples at 4:2:2 / 4:2:0 in one 2 * S-byte store where the address is 2 * S-byte aligned; else sample by
// sample.  Stores are clipped to the plane.  Padding between rows, planes and frames is neither read nor written.
//
// Scalar registers: pb_kernels_nv12.hpp's rule - the layouts and fills live in vector registers, fills of black pixels are applied after
// the loads from values the compiler cannot trace.
//
// Limits.  Byte offsets inside a frame are 32-bit: pb_remap_planar refuses frames whose span reaches 2^31 bytes before any launch, and
// sources of 32768 px a side or more.  LDS: the regrouping buffer only, 4224 bytes per wave.
#pragma once
#include "pb_kernels_nv12.hpp"

// SUB: the subsampling of planes 1 and 2 (the values of PB_PLANAR_444 / _422 / _420 in include/photonbend_hip.h)
#define PB_SUB_444 0
#define PB_SUB_422 1
#define PB_SUB_420 2
__host__ __device__ constexpr int pb_planar_cx(int sub) { return sub != PB_SUB_444; }
__host__ __device__ constexpr int pb_planar_cy(int sub) { return sub == PB_SUB_420; }

// the layouts and fills of one launch, in bytes; the fills are samples
struct PbPlanar {
    unsigned src_pitch, src_cpitch, src_o1, src_o2;
    unsigned dst_pitch, dst_cpitch, dst_o1, dst_o2;
    unsigned fill[3];
};

// two adjacent samples of a chroma plane, (cy, cx) and (cy, cx + 1) of a plane (CH, CW) with rows `pitch` bytes apart
template <int S, bool NT>
__device__ __forceinline__ void pb_planar_store2(uint8_t* __restrict__ d, const unsigned pitch, const int CW, const int CH, const int cx, const int cy,
                                                 const unsigned v[2]) {
    if (cy >= CH) return;
    uint8_t* p = d + ((unsigned)cy * pitch + (unsigned)cx * (unsigned)S);
    if (cx + 1 < CW && ((uintptr_t)p & (unsigned)(2 * S - 1)) == 0) {
        if constexpr (S == 1) pb_px_store_vec<NT>((uint16_t)(v[0] | (v[1] << 8)), p);
        else pb_px_store_vec<NT>(v[0] | (v[1] << 16), p);
    } else {
        if (cx < CW) pb_nv12_store_y1<S>(p, v[0]);
        if (cx + 1 < CW) pb_nv12_store_y1<S>(p + S, v[1]);
    }
}
// the lane's samples of one chroma plane that belong to output row y, columns x .. x + 3 (x a multiple of 4): c[0 .. (4 >> CX) - 1].
// The caller has established that row y holds anchors (CY == 0, or y even)
template <int S, int SUB, bool NT>
__device__ __forceinline__ void pb_planar_store_c(uint8_t* __restrict__ d, const unsigned cpitch, const int W, const int H, const int x, const int y,
                                                  const unsigned c[4]) {
    constexpr int CX = pb_planar_cx(SUB), CY = pb_planar_cy(SUB);
    if constexpr (CX == 0) pb_nv12_store_y<S, NT>(d, cpitch, W, H, x, y, c);
    else pb_planar_store2<S, NT>(d, cpitch, W >> CX, H >> CY, x >> CX, y >> CY, c);
}
// the byte offset of the chroma sample of source pixel (r, c) inside its plane
template <int S, int SUB>
__device__ __forceinline__ unsigned pb_planar_coff(const unsigned cpitch, const unsigned r, const unsigned c) {
    return (r >> pb_planar_cy(SUB)) * cpitch + (c >> pb_planar_cx(SUB)) * (unsigned)S;
}

template <int SRC_KIND, int S, int SUB>
__global__ __launch_bounds__(64 * PB_TILE_WAVES) void pb_planar_hot_kernel(const PbParams* __restrict__ Pp, const PbHot Hd, const PbTileEntry* __restrict__ table,
                                                                            const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                            const unsigned groups_per_frame, unsigned long long src_stride,
                                                                            unsigned long long dst_stride, const int32_t* __restrict__ idx_tab,
                                                                            const int32_t* __restrict__ fix_px, const int32_t* __restrict__ fix_idx, const PbPlanar Ls) {
    static_assert(SUB == PB_SUB_444 || SUB == PB_SUB_422 || SUB == PB_SUB_420, "the subsamplings of pb_remap_planar");
    constexpr int CX = pb_planar_cx(SUB), CY = pb_planar_cy(SUB);
    constexpr int NC = 4 >> CX;  // chroma samples of a lane's four pixels of a row: at pixels k = j << CX
    // the layouts and fills live in VECTOR registers (pb_kernels_nv12.hpp, "Scalar registers")
    PbPlanar L;
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.src_pitch) : "s"(Ls.src_pitch));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.src_cpitch) : "s"(Ls.src_cpitch));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.src_o1) : "s"(Ls.src_o1));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.src_o2) : "s"(Ls.src_o2));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.dst_pitch) : "s"(Ls.dst_pitch));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.dst_cpitch) : "s"(Ls.dst_cpitch));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.dst_o1) : "s"(Ls.dst_o1));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.dst_o2) : "s"(Ls.dst_o2));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.fill[0]) : "s"(Ls.fill[0]));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.fill[1]) : "s"(Ls.fill[1]));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.fill[2]) : "s"(Ls.fill[2]));
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
    // (planes 1 and 2 are addressed from the frame's start, by 32-bit offsets: four plane pointers would be eight more live registers)

    if (flags & PB_TILE_FAILED) {
        const int32_t* __restrict__ slot = idx_tab + (size_t)e->aux_off * (PB_TILE * PB_TILE);
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            const int4 v = *reinterpret_cast<const int4*>(slot + (yb + 8 * jr) * PB_TILE + 4 * xg);
            const int id[4] = {v.x, v.y, v.z, v.w};
            const bool row_in = Y0 + yb + 8 * jr < H;
            unsigned a[4], c1[4], c2[4], black = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // (black or outside the image: a bit per pixel, for the fills after the loads)
                const int idk = (row_in && x + k < W) ? id[k] : -1;
                black |= (unsigned)(idk < 0) << k;
                unsigned r, c;
                pb_nv12_divmod((unsigned)(idk < 0 ? 0 : idk), sw, inv_sw, r, c);
                a[k] = pb_nv12_load_y<S>(src, r * L.src_pitch + c * (unsigned)S);
                if (!(k & CX)) {  // (every lane loads - no load inside a branch; at 4:2:0 the lanes of even rows store)
                    const unsigned off = pb_planar_coff<S, SUB>(L.src_cpitch, r, c);
                    c1[k >> CX] = pb_nv12_load_y<S>(src, L.src_o1 + off);
                    c2[k >> CX] = pb_nv12_load_y<S>(src, L.src_o2 + off);
                }
            }
            asm volatile("" : "+v"(black));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool b = (black >> k) & 1u;
                a[k] = b ? L.fill[0] : a[k];
                if (!(k & CX)) {
                    c1[k >> CX] = b ? L.fill[1] : c1[k >> CX];
                    c2[k >> CX] = b ? L.fill[2] : c2[k >> CX];
                }
            }
            pb_nv12_store_y<S, true>(dst, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, a);
            if (!CY || pb_nv12_even(yb)) {
                pb_planar_store_c<S, SUB, true>(dst + L.dst_o1, L.dst_cpitch, W, H, x, Y0 + yb + 8 * jr, c1);
                pb_planar_store_c<S, SUB, true>(dst + L.dst_o2, L.dst_cpitch, W, H, x, Y0 + yb + 8 * jr, c2);
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
            if (!CY || pb_nv12_even(yb)) {
                pb_planar_store_c<S, SUB, false>(dst + L.dst_o1, L.dst_cpitch, W, H, x, Y0 + yb + 8 * jr, z1);
                pb_planar_store_c<S, SUB, false>(dst + L.dst_o2, L.dst_cpitch, W, H, x, Y0 + yb + 8 * jr, z2);
            }
        }
    } else if (flags & (PB_TILE_LEAN | PB_TILE_DIRECT)) {
        // pb_px_hot_kernel's direct-gather path (its comments and pb_win_tile's hold here): every pixel of such a tile lies inside the
        // image and samples inside the tile's source box, in both evaluation orders (pb_certify_kernel)
        unsigned* win = lds[wave];
        const int ar = e->anchor_r, ac = e->anchor_c;
        const bool along_x = fabsf(e->c[1][0]) <= fabsf(e->c[5][0]);  // |d row / du| <= |d row / dv|
        const int p = lane & 31, hh = lane >> 5;
        const float num = along_x ? e->c[1][0] : e->c[5][0], den = along_x ? e->c[5][0] : e->c[1][0];
        const float slope = (den != 0.0f) ? -num / den : 0.0f;
        const int shift = (int)rintf(slope * ((float)p - 15.5f));
        // this lane's 16 pixels are all anchors (else none is): its column is p (along_x) or q, its row the other
        const int colpar = along_x ? p : hh + shift, rowpar = along_x ? hh + shift : p;
        const bool anchors = !(((colpar & CX) | (rowpar & CY)) & 1);
        unsigned dead = 0u;
        if (flags & PB_TILE_MASKED) {
            const int side = (P.dst.kind == PB_KIND_DOUBLE) && (X0 >= P.dst_half_w);
            const int wc = (P.dst.kind == PB_KIND_DOUBLE) ? P.dst_half_w : P.dst.width;
            const long long lo = P.inv_lo[side], hi = P.inv_hi[side];
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                const int q = (2 * n + hh + shift) & 31;
                const int px = along_x ? p : q, py = along_x ? q : p;
                const long long x2 = 2ll * (X0 + px - (side ? P.dst_half_w : 0)) - (wc - 1), y2 = (long long)(P.dst.height - 1) - 2ll * (Y0 + py);
                const long long n4 = x2 * x2 + y2 * y2;
                dead |= (unsigned)(n4 >= lo && n4 < hi) << n;
            }
        }
        unsigned rc[16];  // the certified source pixel: row << 16 | column (both below 32768)
        if (along_x) {
            pb_f2 bcol[5];
            pb_collapse_col(e, p, bcol);
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                const pb_f2 fv = pb_eval_row(bcol, pb_tile_coord((2 * n + hh + shift) & 31));
                rc[n] = ((unsigned)(ar + (int)fv.x) << 16) | (unsigned)(ac + (int)fv.y);
            }
        } else {
            pb_f2 a[5];
            pb_collapse_row(e, p, a);
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                const pb_f2 fv = pb_eval_row(a, pb_tile_coord((2 * n + hh + shift) & 31));
                rc[n] = ((unsigned)(ar + (int)fv.x) << 16) | (unsigned)(ac + (int)fv.y);
            }
        }
        unsigned t0[16], t1[16], t2[16];
        if (flags & PB_TILE_MASKED) {
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                t0[n] = L.fill[0];
                t1[n] = L.fill[1];
                t2[n] = L.fill[2];
                if (!((dead >> n) & 1u)) {  // (a dead pixel's address is not a certified one: no load)
                    t0[n] = pb_nv12_load_y<S>(src, (rc[n] >> 16) * L.src_pitch + (rc[n] & 0xFFFFu) * (unsigned)S);
                    if (anchors) {
                        const unsigned off = pb_planar_coff<S, SUB>(L.src_cpitch, rc[n] >> 16, rc[n] & 0xFFFFu);
                        t1[n] = pb_nv12_load_y<S>(src, L.src_o1 + off);
                        t2[n] = pb_nv12_load_y<S>(src, L.src_o2 + off);
                    }
                }
            }
        } else {
#pragma unroll
            for (int n = 0; n < 16; ++n) t0[n] = pb_nv12_load_y<S>(src, (rc[n] >> 16) * L.src_pitch + (rc[n] & 0xFFFFu) * (unsigned)S);
            if (anchors) {
#pragma unroll
                for (int n = 0; n < 16; ++n) {
                    const unsigned off = pb_planar_coff<S, SUB>(L.src_cpitch, rc[n] >> 16, rc[n] & 0xFFFFu);
                    t1[n] = pb_nv12_load_y<S>(src, L.src_o1 + off);
                    t2[n] = pb_nv12_load_y<S>(src, L.src_o2 + off);
                }
            }
        }
        // park as [y][x], read back in the store shape and store: plane 0, then - through the same buffer - planes 1 and 2 at their anchors
        {
            unsigned a[4][4];
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                const int q = (2 * n + hh + shift) & 31;
                win[along_x ? q * 33 + p : p * 33 + q] = t0[n];
            }
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
        for (int pl = 1; pl <= 2; ++pl) {
            unsigned c[4][4];
            if (anchors) {
#pragma unroll
                for (int n = 0; n < 16; ++n) {
                    const int q = (2 * n + hh + shift) & 31;
                    win[along_x ? q * 33 + p : p * 33 + q] = (pl == 1) ? t1[n] : t2[n];
                }
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
                for (int jr = 0; jr < 4; ++jr)
                    pb_planar_store_c<S, SUB, NT>(dst + (pl == 1 ? L.dst_o1 : L.dst_o2), L.dst_cpitch, W, H, x, Y0 + yb + 8 * jr, c[jr]);
            }
        }
    } else {
        // generic tile: validity, wrap and truncation edge per pixel; a packed (row << 16 | column), or -1 = black
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            PbRowModel R;
            pb_model_row(P, e, X0, Y0, yb + 8 * jr, 4 * xg, R);
            unsigned a[4], c1[4], c2[4];
            int v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = pb_model_px_rc<SRC_KIND>(P, R, 4 * xg, k);
                const unsigned r = (unsigned)v[k] >> 16, c = (unsigned)v[k] & 0xFFFFu;
                a[k] = pb_nv12_load_y<S>(src, v[k] < 0 ? 0u : r * L.src_pitch + c * (unsigned)S);
                if (!(k & CX)) {  // (every lane loads; at 4:2:0 the lanes of even rows store)
                    const unsigned off = v[k] < 0 ? 0u : pb_planar_coff<S, SUB>(L.src_cpitch, r, c);
                    c1[k >> CX] = pb_nv12_load_y<S>(src, L.src_o1 + off);
                    c2[k >> CX] = pb_nv12_load_y<S>(src, L.src_o2 + off);
                }
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
            if (!CY || pb_nv12_even(yb)) {
                pb_planar_store_c<S, SUB, NT>(dst + L.dst_o1, L.dst_cpitch, W, H, x, Y0 + yb + 8 * jr, c1);
                pb_planar_store_c<S, SUB, NT>(dst + L.dst_o2, L.dst_cpitch, W, H, x, Y0 + yb + 8 * jr, c2);
            }
        }
    }
    // this tile's fix pixels (where the model's truncation differs from the faithful one): re-copied through their exact indices
    // after the wave's own stores have completed; an anchor among them re-copies its two chroma samples
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
                const unsigned off = id < 0 ? 0u : pb_planar_coff<S, SUB>(L.src_cpitch, r, c);
                const unsigned v1 = pb_nv12_load_y<S>(src, L.src_o1 + off), v2 = pb_nv12_load_y<S>(src, L.src_o2 + off);
                const unsigned doff = (y >> CY) * L.dst_cpitch + (xx >> CX) * (unsigned)S;
                pb_nv12_store_y1<S>(dst + (L.dst_o1 + doff), id < 0 ? L.fill[1] : v1);
                pb_nv12_store_y1<S>(dst + (L.dst_o2 + doff), id < 0 ? L.fill[2] : v2);
            }
        }
    }
}
