// pb_kernels_px.hpp - the nearest tile kernel for pixels that are not three bytes (pb_remap_px).
//
// The nearest sampler never looks inside a pixel: it copies bytes_per_px bytes from a certified source index.  Tile models,
// certification, the exact-index tables, the fix lists and the launch-order table are those of the RGB8 plan, unchanged; this file adds
// the kernel that moves B-byte pixels, B in {1, 2, 4, 6, 8}: grey8, grey16 (or two uint8 channels), RGBA8, RGB16, RGBA16.
//
// pb_px_hot_kernel<SRC_KIND, BPP> is launched like pb_hot_win_kernel: one wave per slot of the plan's nearest launch-order table, the
// entry in SGPRs (pb_load_entry), frames of a batch as a grid dimension, the parameter block behind a pointer, PbHot by value.
//   BLACK           zeros.
//   LEAN / DIRECT   the direct-gather path of pb_win_tile (a LEAN entry carries the same model and anchors as the DIRECT entry
//   / MASKED        pb_budget_kernel would make of it): lanes along the line of constant source row, the shear, `dead` bits for MASKED,
//                   regrouping through the wave's LDS to four consecutive pixels x four rows per lane.  The model is evaluated in the two
//                   certified orders only (pb_collapse_row / pb_collapse_col + pb_eval_row).
//   generic         pb_model_row / pb_model_px_rc, global loads only (no LDS window).
//   FAILED          the plan's exact indices (idx_tab), as pb_failed_tile.
//   fix pixels      re-copied through fix_px / fix_idx after the wave's own stores have completed.
//
// Pixel movement.  A frame pointer and stride are multiples of A = min(4, B & -B) bytes (pb_remap_px checks): 1, 2, 4, 2, 4 for B = 1, 2,
// 4, 6, 8.  A pixel is loaded with EXACTLY its own bytes - u8, u16, dword, dword + u16, dwordx2 - so no load can touch a byte outside the
// frame, the very last pixel included (the RGB8 kernels read four bytes for a three-byte pixel and special-case it; nothing of the kind
// is needed here).  Four output pixels leave in one 4-, 8-, 16-, 24- or 32-byte store where their address is 4-byte aligned, else
// sample by sample (a partial tile's edge, an odd row start of 1-, 2- and 6-byte pixels).  pb_px_load, pb_px_store1 and pb_px_store4 also
// move pixels of 12 and 16 bytes - three and four float32 channels, A = 4: three and four dwords, 48- and 64-byte stores as three and four
// 16-byte ones - for pb_pxf_interp_kernel (pb_kernels_pxf_interp.hpp); pb_px_hot_kernel has no instantiation for them.
//
// Limits.  Source byte offsets are 32-bit: pb_remap_px refuses frames of B * h * w >= 2^31 bytes (source or destination) with
// PB_ERR_UNSUPPORTED before any launch.  Sources of 32768 px a side or more are refused like the window routes (generic tiles pack row
// and column in 16 bits each).  LDS: the regrouping buffer only, 4224 bytes per wave.
#pragma once
#include "pb_kernels_tile.hpp"

#define PB_PX_PLANE (33 * 32)  // dwords of the regrouping buffer: [y][x] with a 33-dword pitch
typedef unsigned pb_px_u32x2 __attribute__((ext_vector_type(2), aligned(4)));
typedef unsigned pb_px_u32x4 __attribute__((ext_vector_type(4), aligned(4)));

template <int BPP>
struct PbPx {
    static constexpr int NW = (BPP + 3) / 4;
    unsigned w[NW];  // the pixel's bytes, little endian, zero above them
};

// exactly BPP bytes at byte offset `off` of the frame (a multiple of BPP; the frame is aligned to min(4, BPP & -BPP))
template <int BPP>
__device__ __forceinline__ PbPx<BPP> pb_px_load(const uint8_t* __restrict__ s, unsigned off) {
    static_assert(BPP == 1 || BPP == 2 || BPP == 4 || BPP == 6 || BPP == 8 || BPP == 12 || BPP == 16,
                  "pixel sizes of pb_remap_px, and three and four float32 channels (pb_remap_interp_pxf)");
    PbPx<BPP> v;
    const uint8_t* p = s + off;
    if constexpr (BPP == 1) {
        v.w[0] = *p;
    } else if constexpr (BPP == 2) {
        v.w[0] = *reinterpret_cast<const uint16_t*>(p);
    } else if constexpr (BPP == 4) {
        v.w[0] = *reinterpret_cast<const unsigned*>(p);
    } else if constexpr (BPP == 6) {
        __builtin_memcpy(&v.w[0], p, 4);  // (2-byte aligned: an unaligned dword, like the RGB8 kernels' gathers)
        v.w[1] = *reinterpret_cast<const uint16_t*>(p + 4);
    } else if constexpr (BPP == 8) {
        pb_px_u32x2 t = *reinterpret_cast<const pb_px_u32x2*>(p);
        v.w[0] = t.x;
        v.w[1] = t.y;
    } else if constexpr (BPP == 12) {
        __builtin_memcpy(&v.w[0], __builtin_assume_aligned(p, 4), 12);  // (three dwords, 4-byte aligned: a vector of three would be read as sixteen bytes)
    } else {
        pb_px_u32x4 t = *reinterpret_cast<const pb_px_u32x4*>(p);
        v.w[0] = t.x;
        v.w[1] = t.y;
        v.w[2] = t.z;
        v.w[3] = t.w;
    }
    return v;
}
template <int BPP>
__device__ __forceinline__ PbPx<BPP> pb_px_zero_if(PbPx<BPP> v, bool black) {
#pragma unroll
    for (int i = 0; i < PbPx<BPP>::NW; ++i) v.w[i] = black ? 0u : v.w[i];
    return v;
}
// the pixel of source index `id` (-1: black).  Branch-free, so that a lane's gathers are in flight together: a black pixel reads pixel 0
template <int BPP>
__device__ __forceinline__ PbPx<BPP> pb_px_load_idx(const uint8_t* __restrict__ s, int id) {
    return pb_px_zero_if<BPP>(pb_px_load<BPP>(s, id < 0 ? 0u : (unsigned)id * (unsigned)BPP), id < 0);
}

// one pixel, sample by sample (p aligned like the frame)
template <int BPP>
__device__ __forceinline__ void pb_px_store1(uint8_t* p, const PbPx<BPP>& v) {
    if constexpr (BPP == 1) {
        *p = (uint8_t)v.w[0];
    } else if constexpr (BPP == 2) {
        *reinterpret_cast<uint16_t*>(p) = (uint16_t)v.w[0];
    } else if constexpr (BPP == 4) {
        *reinterpret_cast<unsigned*>(p) = v.w[0];
    } else if constexpr (BPP == 6) {
        uint16_t* q = reinterpret_cast<uint16_t*>(p);
        q[0] = (uint16_t)v.w[0];
        q[1] = (uint16_t)(v.w[0] >> 16);
        q[2] = (uint16_t)v.w[1];
    } else {  // 8, 12, 16: dword by dword
        unsigned* q = reinterpret_cast<unsigned*>(p);
#pragma unroll
        for (int i = 0; i < PbPx<BPP>::NW; ++i) q[i] = v.w[i];
    }
}
template <bool NT, class V>
__device__ __forceinline__ void pb_px_store_vec(const V v, uint8_t* p) {
    if (NT)
        __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
    else
        *reinterpret_cast<V*>(p) = v;
}
// four consecutive pixels in one 4 * BPP-byte store (p 4-byte aligned)
template <int BPP, bool NT>
__device__ __forceinline__ void pb_px_store4(uint8_t* p, const PbPx<BPP> a[4]) {
    if constexpr (BPP == 1) {
        pb_px_store_vec<NT>(a[0].w[0] | (a[1].w[0] << 8) | (a[2].w[0] << 16) | (a[3].w[0] << 24), p);
    } else if constexpr (BPP == 2) {
        const pb_px_u32x2 o = {a[0].w[0] | (a[1].w[0] << 16), a[2].w[0] | (a[3].w[0] << 16)};
        pb_px_store_vec<NT>(o, p);
    } else if constexpr (BPP == 4) {
        const pb_px_u32x4 o = {a[0].w[0], a[1].w[0], a[2].w[0], a[3].w[0]};
        pb_px_store_vec<NT>(o, p);
    } else if constexpr (BPP == 6) {
        const pb_px_u32x4 o = {a[0].w[0], a[0].w[1] | (a[1].w[0] << 16), (a[1].w[0] >> 16) | (a[1].w[1] << 16), a[2].w[0]};
        const pb_px_u32x2 q = {a[2].w[1] | (a[3].w[0] << 16), (a[3].w[0] >> 16) | (a[3].w[1] << 16)};
        pb_px_store_vec<NT>(o, p);
        pb_px_store_vec<NT>(q, p + 16);
    } else if constexpr (BPP == 8) {
        const pb_px_u32x4 o = {a[0].w[0], a[0].w[1], a[1].w[0], a[1].w[1]};
        const pb_px_u32x4 q = {a[2].w[0], a[2].w[1], a[3].w[0], a[3].w[1]};
        pb_px_store_vec<NT>(o, p);
        pb_px_store_vec<NT>(q, p + 16);
    } else if constexpr (BPP == 12) {  // 48 bytes
        const pb_px_u32x4 o = {a[0].w[0], a[0].w[1], a[0].w[2], a[1].w[0]};
        const pb_px_u32x4 q = {a[1].w[1], a[1].w[2], a[2].w[0], a[2].w[1]};
        const pb_px_u32x4 r = {a[2].w[2], a[3].w[0], a[3].w[1], a[3].w[2]};
        pb_px_store_vec<NT>(o, p);
        pb_px_store_vec<NT>(q, p + 16);
        pb_px_store_vec<NT>(r, p + 32);
    } else {  // 64 bytes
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const pb_px_u32x4 o = {a[k].w[0], a[k].w[1], a[k].w[2], a[k].w[3]};
            pb_px_store_vec<NT>(o, p + 16 * k);
        }
    }
}
// the lane's four pixels of output row y, columns x .. x + 3: clipped at the image's edge, one wide store where the address allows
template <int BPP, bool NT>
__device__ __forceinline__ void pb_px_store_row(uint8_t* __restrict__ d, const int W, const int H, const int x, const int y, const PbPx<BPP> a[4]) {
    if (y >= H) return;
    uint8_t* p = d + (unsigned long long)BPP * ((unsigned long long)y * (unsigned)W + (unsigned)x);
    if (x + 3 < W && ((uintptr_t)p & 3u) == 0) {
        pb_px_store4<BPP, NT>(p, a);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x + k < W) pb_px_store1<BPP>(p + BPP * k, a[k]);
    }
}

// The front end of the direct-gather path of a LEAN / DIRECT tile (pb_win_tile's, its comments hold): which sixteen pixels of the tile a
// lane gathers, and where they come from.  Lanes lie along the line of constant source row: lane (p, hh) holds the pixels n = 0 .. 15 at
// q = (2 n + hh + shift) & 31 of line p - pixel (y, x) = (q, p) with along_x, else (p, q) -, `shift` the line's shear.
struct PbGather {
    bool along_x;  // |d row / du| <= |d row / dv|
    int p, hh, shift;
    __device__ __forceinline__ int q(const int n) const { return (2 * n + hh + shift) & 31; }
    __device__ __forceinline__ int at(const int n) const { return along_x ? q(n) * 33 + p : p * 33 + q(n); }  // pixel n's dword of a [y][x] regrouping plane
};
__device__ __forceinline__ PbGather pb_gather_lanes(const PbTileEntry* __restrict__ e, const int lane) {
    PbGather g;
    g.along_x = fabsf(e->c[1][0]) <= fabsf(e->c[5][0]);
    g.p = lane & 31;
    g.hh = lane >> 5;
    const float num = g.along_x ? e->c[1][0] : e->c[5][0], den = g.along_x ? e->c[5][0] : e->c[1][0];
    const float slope = (den != 0.0f) ? -num / den : 0.0f;
    g.shift = (int)rintf(slope * ((float)g.p - 15.5f));
    return g;
}
// rc[n] = pixel n's certified source pixel, row << 16 | column (both below 32768): the model from the SGPR-resident entry, evaluated in the
// two certified orders only (pb_collapse_col / pb_collapse_row + pb_eval_row)
__device__ __forceinline__ PbGather pb_gather_front(const PbTileEntry* __restrict__ e, const int lane, unsigned rc[16]) {
    const PbGather g = pb_gather_lanes(e, lane);
    const int ar = e->anchor_r, ac = e->anchor_c;
    if (g.along_x) {
        pb_f2 bcol[5];
        pb_collapse_col(e, g.p, bcol);
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            const pb_f2 fv = pb_eval_row(bcol, pb_tile_coord(g.q(n)));
            rc[n] = ((unsigned)(ar + (int)fv.x) << 16) | (unsigned)(ac + (int)fv.y);
        }
    } else {
        pb_f2 a[5];
        pb_collapse_row(e, g.p, a);
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            const pb_f2 fv = pb_eval_row(a, pb_tile_coord(g.q(n)));
            rc[n] = ((unsigned)(ar + (int)fv.x) << 16) | (unsigned)(ac + (int)fv.y);
        }
    }
    return g;
}
// the `dead` bits of a MASKED tile at (X0, Y0): bit n is set where the lane's pixel n is black by the destination's mask
__device__ __forceinline__ unsigned pb_gather_dead(const PbParams& P, const PbGather& g, const int X0, const int Y0) {
    const int side = (P.dst.kind == PB_KIND_DOUBLE) && (X0 >= P.dst_half_w);
    const int wc = (P.dst.kind == PB_KIND_DOUBLE) ? P.dst_half_w : P.dst.width;
    const long long lo = P.inv_lo[side], hi = P.inv_hi[side];
    unsigned dead = 0u;
#pragma unroll
    for (int n = 0; n < 16; ++n) {
        const int q = g.q(n);
        const int px = g.along_x ? g.p : q, py = g.along_x ? q : g.p;
        const long long x2 = 2ll * (X0 + px - (side ? P.dst_half_w : 0)) - (wc - 1), y2 = (long long)(P.dst.height - 1) - 2ll * (Y0 + py);
        const long long n4 = x2 * x2 + y2 * y2;
        dead |= (unsigned)(n4 >= lo && n4 < hi) << n;
    }
    return dead;
}

template <int SRC_KIND, int BPP>
__global__ __launch_bounds__(64 * PB_TILE_WAVES) void pb_px_hot_kernel(const PbParams* __restrict__ Pp, const PbHot Hd, const PbTileEntry* __restrict__ table,
                                                                        const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                        const unsigned groups_per_frame, unsigned long long src_stride,
                                                                        unsigned long long dst_stride, const int32_t* __restrict__ idx_tab,
                                                                        const int32_t* __restrict__ fix_px, const int32_t* __restrict__ fix_idx) {
    typedef PbPx<BPP> Px;
    constexpr int NW = Px::NW;
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
    // the wave's slot of the launch-order table (four waves per workgroup: pb_hot_win_kernel's vslot)
    PbTileEntry entry;
    pb_load_entry(table + (wg * 4u + (unsigned)wave), entry);
    const PbTileEntry* __restrict__ e = &entry;
    const int flags = e->flags;
    if (flags & PB_TILE_SKIP) return;
    const int tx = e->tile_xy & 0xFFFF, ty = (int)((unsigned)e->tile_xy >> 16);
    const int X0 = tx * PB_TILE, Y0 = ty * PB_TILE;
    const int W = Hd.dst_w, H = Hd.dst_h;
    const int xg = lane & 7, yb = lane >> 3;
    const int x = X0 + 4 * xg;  // the lane's store shape: columns x .. x + 3 of rows Y0 + yb + 8 * jr

    if (flags & PB_TILE_FAILED) {
        const int32_t* __restrict__ slot = idx_tab + (size_t)e->aux_off * (PB_TILE * PB_TILE);
        Px a[4][4];
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            const int4 v = *reinterpret_cast<const int4*>(slot + (yb + 8 * jr) * PB_TILE + 4 * xg);
            const int id[4] = {v.x, v.y, v.z, v.w};
            const bool row_in = Y0 + yb + 8 * jr < H;
#pragma unroll
            for (int k = 0; k < 4; ++k) a[jr][k] = pb_px_load_idx<BPP>(src, (row_in && x + k < W) ? id[k] : -1);
        }
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) pb_px_store_row<BPP, true>(dst, W, H, x, Y0 + yb + 8 * jr, a[jr]);
        return;  // (a failed tile has no fix pixels: its table slot holds them all)
    }
    if (flags & PB_TILE_BLACK) {
        Px z[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int i = 0; i < NW; ++i) z[k].w[i] = 0u;
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) pb_px_store_row<BPP, false>(dst, W, H, x, Y0 + yb + 8 * jr, z);
    } else if (flags & (PB_TILE_LEAN | PB_TILE_DIRECT)) {
        // pb_win_tile's direct-gather path (its comments hold here): every pixel of such a tile lies inside the image and samples
        // inside the tile's source box, in both evaluation orders (pb_certify_kernel)
        unsigned* win = lds[wave];
        const unsigned rowbytes = (unsigned)BPP * (unsigned)Hd.src_w;
        const unsigned gbase = (unsigned)e->anchor_r * rowbytes + (unsigned)BPP * (unsigned)e->anchor_c;
        // (of the shared front end this kernel takes the lanes' geometry alone: its source offsets are bytes of BPP-byte pixels, and with
        //  the `dead` loop behind pb_gather_dead the compiler allocates its registers differently - tests/test_isa_pixel_formats.py pins them)
        const PbGather g = pb_gather_lanes(e, lane);
        const bool along_x = g.along_x;
        const int p = g.p, hh = g.hh, shift = g.shift;
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
        unsigned go[16];
        if (along_x) {
            pb_f2 bcol[5];
            pb_collapse_col(e, p, bcol);
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                const pb_f2 fv = pb_eval_row(bcol, pb_tile_coord((2 * n + hh + shift) & 31));
                go[n] = gbase + (unsigned)(int)fv.x * rowbytes + __umul24((unsigned)(int)fv.y, (unsigned)BPP);
            }
        } else {
            pb_f2 a[5];
            pb_collapse_row(e, p, a);
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                const pb_f2 fv = pb_eval_row(a, pb_tile_coord((2 * n + hh + shift) & 31));
                go[n] = gbase + (unsigned)(int)fv.x * rowbytes + __umul24((unsigned)(int)fv.y, (unsigned)BPP);
            }
        }
        Px t[16];
        if (flags & PB_TILE_MASKED) {
#pragma unroll
            for (int n = 0; n < 16; ++n) {
#pragma unroll
                for (int i = 0; i < NW; ++i) t[n].w[i] = 0u;
                if (!((dead >> n) & 1u)) t[n] = pb_px_load<BPP>(src, go[n]);  // (a dead pixel's address is not a certified one: no load)
            }
        } else {
#pragma unroll
            for (int n = 0; n < 16; ++n) t[n] = pb_px_load<BPP>(src, go[n]);
        }
        // park as [y][x], read back as 4 consecutive pixels x 4 rows per lane - one pixel dword at a time through the one plane (a second
        // plane for 6- and 8-byte pixels would be 33 KiB a workgroup: four waves per SIMD by LDS alone)
        Px a[4][4];
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            if (i) pb_wave_sync();  // (the plane's previous contents have been read)
#pragma unroll
            for (int n = 0; n < 16; ++n) win[g.at(n)] = t[n].w[i];
            pb_wave_sync();
#pragma unroll
            for (int jr = 0; jr < 4; ++jr)
#pragma unroll
                for (int k = 0; k < 4; ++k) a[jr][k].w[i] = win[(yb + 8 * jr) * 33 + 4 * xg + k];
        }
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) pb_px_store_row<BPP, NT>(dst, W, H, x, Y0 + yb + 8 * jr, a[jr]);
    } else {
        // generic tile: validity, wrap and truncation edge per pixel; a packed (row << 16 | column), or -1 = black
        const unsigned sw = (unsigned)Hd.src_w;
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            PbRowModel R;
            pb_model_row(P, e, X0, Y0, yb + 8 * jr, 4 * xg, R);
            Px a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int v = pb_model_px_rc<SRC_KIND>(P, R, 4 * xg, k);
                a[k] = pb_px_load_idx<BPP>(src, v < 0 ? -1 : (int)(((unsigned)v >> 16) * sw + ((unsigned)v & 0xFFFFu)));
            }
            pb_px_store_row<BPP, NT>(dst, W, H, x, Y0 + yb + 8 * jr, a);
        }
    }
    // this tile's fix pixels (where the model's truncation differs from the faithful one): re-copied through their exact indices
    // after the wave's own stores have completed
    const int n_fix = e->fix_cnt;
    if (n_fix > 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane < n_fix) {
            const unsigned p = (unsigned)fix_px[e->fix_off + lane];
            const Px v = pb_px_load_idx<BPP>(src, fix_idx[e->fix_off + lane]);
            pb_px_store1<BPP>(dst + (unsigned long long)BPP * p, v);
        }
    }
}
