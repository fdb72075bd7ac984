// pb_kernels_px_interp.hpp - OPT-IN bilinear and Catmull-Rom sampling of grey, RGBA and 16-bit frames (pb_remap_interp_px):
// the interpolating tile kernel for pixels of C channels of S-byte samples, (C, S) in {1, 2, 3, 4} x {1, 2} without (3, 1) - uint8 RGB is
// pb_bilinear_hot_kernel's / pb_catmull_rom_hot_kernel's.  The pixel is B = C * S bytes: pb_kernels_px.hpp's {1, 2, 4, 6, 8}, the two-byte
// pixel both as grey16 (1, 2) and as two uint8 channels (2, 1).
//
// The definitions are the RGB8 modes' own, on an image of any layout: oracle/reference_path.py: remap_bilinear and
// tests/catmull_rom_ref.py: remap.  f is the reference's pre-truncation source coordinate, s = f - 0.5, i0 = floor(s), t = s - i0 per axis.
//   bilinear      taps i0, i0 + 1 per axis; per channel top = a + tx (b - a), bot likewise, rint(top + ty (bot - top)).
//   Catmull-Rom   taps i0 - 1 .. i0 + 2 per axis, Keys' weights with a = -0.5 (pb_kernels_catmull_rom.hpp); per channel the four row sums,
//                 then the column sum, rounded half to even and clipped to [0, 2^(8 S) - 1].
// Rows clamped, a panorama's columns wrapped modulo w, a camera's clamped; zeros where the pixel is not live.
//
// pb_px_interp_kernel<SRC_KIND, FILTER, C, S> has pb_planar_bilinear_kernel's launch shape and coordinates to the letter: one wave per slot
// of the bilinear mode's launch-order table, four waves per workgroup through pb_bil_slot_of<4>, frames of a batch a grid dimension with
// 64-bit frame offsets, the tile entry in SGPRs; table tiles walk their bil_xy slot in its stored order (pb_cr_of_q), LEAN / DIRECT tiles
// evaluate the certified tile model (pb_bil_collapse / pb_bil_eval, TD3 where flagged) in the orientation they were certified in, BLACK
// tiles store zeros, fix pixels are redone from bil_fix_xy behind s_waitcnt vmcnt(0).  No plan state, no preparation pass.  The walk is
// written out here, beside pb_planar_bilinear_kernel's and pb_cr_vals': a shared walk with the sampler as a parameter moved the
// registers of those kernels, whose listings are pinned.
//
// Sampling.  Every tap is ONE pb_px_load<B> of exactly the pixel's own bytes - u8, u16, dword, dword + u16, 2 x dword - so no load leaves
// the frame, the last pixel's included.  Tap rows and columns are clamped for EVERY pixel, without a branch: inside the image that changes
// nothing, and the pixels of a partial tile that lie outside the destination - whose model coordinates are anything - cannot leave the
// frame either.  A panorama's columns are wrapped ONCE first: a live coordinate has j0 in [-1, w - 1], so the bilinear taps lie in
// [-1, w] and the four Catmull-Rom taps in [-2, w + 1], which one addition or subtraction of w brings into [0, w - 1] for w >= 2.  At
// w = 1 a tap at -2 or 2 is still outside after it and the clamp puts it on column 0 - the only column, which is what modulo 1 gives.
// A dead pixel reads pixel 0 and is zeroed after the loads.  Channels are unpacked from the loaded dwords.  The Catmull-Rom footprint is
// walked row by row - four taps, their row sum per channel, the column sum's next term - so one row of taps is live per pixel.  No float64.
//
// Catmull-Rom in float32: the bound on this file's order of operations.  u = 2^-24, so a rounding moves x by at most u |x| and by at most
// half an ulp; R the largest sample value (below 2^16: exact as a float); t in [0, 1).
//   weights   pb_pxi_weights, rounding by rounding (an inner error is carried on through factors t, t^2 <= 1):
//             w-1 = ((1 - 0.5 t) t - 0.5) t   in (0.5, 1]: u / 2; in [-0.5, 0.5): u / 4; the product, below 0.5: u / 4            <= 1 u
//             w0  = (1.5 t - 2.5) t^2 + 1     in [-2.5, -1): 2 u; t^2 below 1: u / 2, times 2.5; the sum, in [0, 1]: u / 2       <= 3.75 u
//             w1  = ((2 - 1.5 t) t + 0.5) t   in (0.5, 2]: u; in [0.5, 1.17]: u; the product, in [0, 1]: u / 2                   <= 2.5 u
//             w2  = (0.5 t - 0.5) t^2         in [-0.5, 0): u / 4; t^2: u / 2, times 0.5; the product, below 0.08: u / 16        <= 1 u
//             sum |dw| <= 8.25 u.
//   row sum   r = wx0 a0, then three fused multiply-adds: sum |dw| R <= 8.25 u R, and four roundings of partial sums of at most
//             sum |w| R <= 1.25 R: 5 u R.  |dr| <= 13.25 u R.
//   column    v = wy0 r0, then three fused multiply-adds: sum |wy| |dr| <= 1.25 x 13.25 u R, sum |dwy| |r| <= 8.25 u x 1.25 R, four
//             roundings of partial sums of at most 1.25 x 1.25 R: 6.25 u R.  |dv| <= 33.125 u R < 64 u R = R 2^-18,
// the share the budget T_cr(R) = 1 + floor(15 R / 4096 + R 2^-18) leaves the arithmetic: 0.13 LSB against 0.25 at R = 65535, 0.0005 against
// 0.001 at R = 255.  The clip (v_med3_f32) is exact and the 1.5 x 2^23 addend IS the rounding half to even.  Bilinear: pb_vbil_mix, whose
// bound is video_bilinear_ref's T(R).
//
// Stores.  A packed pixel is parked in the wave's regrouping plane(s) - [y][x], 33-dword pitch; one dword for pixels of up to 4 bytes, the
// second plane for the upper dword of 6- and 8-byte pixels - and read back in the store shape (four pixels of a row).  They leave through
// pb_kernels_px.hpp's pb_px_store_row: pb_px_store4 where all four exist and their first byte is 4-byte aligned, else pb_px_store1 in
// units of A = min(4, B & -B), clipped to the image.  Fix pixels: pb_px_store1.
//
// Limits: pb_remap_px's (32-bit byte offsets inside a frame, sources below 32768 px a side).  LDS: 4224 bytes per wave and plane - 8448
// for 6- and 8-byte pixels, what the video kernel uses.
#pragma once
#include "pb_kernels_planar_bilinear.hpp"
#include "pb_kernels_px.hpp"

#define PB_PXI_BILINEAR 1     // FILTER: PB_INTERP_BILINEAR
#define PB_PXI_CATMULL_ROM 2  //         PB_INTERP_CATMULL_ROM
#define PB_PXI_WAVES 4
// waves per SIMD the kernel is compiled for: pb_planar_bilinear_kernel's (128 VGPRs) and pb_catmull_rom_hot_kernel's (168)
#define PB_PXI_WPE(filter) ((filter) == PB_PXI_BILINEAR ? PB_VBIL_WPE : PB_CR_WPE)

// channel k of a loaded pixel
template <int C, int S>
__device__ __forceinline__ unsigned pb_pxi_channel(const PbPx<C * S>& v, const int k) {
    return S == 1 ? ((v.w[0] >> (8 * k)) & 0xFFu) : ((v.w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
}
// ... into a pixel whose dwords start as zero (val is below 2^(8 S))
template <int C, int S>
__device__ __forceinline__ void pb_pxi_put(PbPx<C * S>& v, const int k, const unsigned val) {
    if (S == 1) v.w[0] |= val << (8 * k);
    else v.w[k >> 1] |= val << (16 * (k & 1));
}
// the four Catmull-Rom weights of a fraction, float32, in the definition's Horner order
__device__ __forceinline__ void pb_pxi_weights(const float t, float w[4]) {
    const float t2 = t * t;
    w[0] = fmaf(fmaf(-0.5f, t, 1.0f), t, -0.5f) * t;
    w[1] = fmaf(fmaf(1.5f, t, -2.5f), t2, 1.0f);
    w[2] = fmaf(fmaf(-1.5f, t, 2.0f), t, 0.5f) * t;
    w[3] = fmaf(0.5f, t, -0.5f) * t2;
}

// One output pixel from its tap base (i0, j0) and fractions (ty, tx); dead: zeros.
template <int FILTER, int C, int S, bool WRAP>
__device__ __forceinline__ PbPx<C * S> pb_pxi_px(const uint8_t* __restrict__ s, const int h, const int w, int i0, int j0, const float ty, const float tx,
                                                 const bool dead) {
    constexpr int B = C * S;
    typedef PbPx<B> Px;
    if (dead) i0 = j0 = 0;
    Px o;
#pragma unroll
    for (int i = 0; i < Px::NW; ++i) o.w[i] = 0u;
    if constexpr (FILTER == PB_PXI_BILINEAR) {
        unsigned r[2], c[2];
        pb_vbil_rc<WRAP>(i0, j0, h, w, r, c);
        const unsigned o0 = r[0] * (unsigned)w, o1 = r[1] * (unsigned)w;
        const Px a0 = pb_px_load<B>(s, (o0 + c[0]) * (unsigned)B), a1 = pb_px_load<B>(s, (o0 + c[1]) * (unsigned)B);
        const Px a2 = pb_px_load<B>(s, (o1 + c[0]) * (unsigned)B), a3 = pb_px_load<B>(s, (o1 + c[1]) * (unsigned)B);
#pragma unroll
        for (int k = 0; k < C; ++k)
            pb_pxi_put<C, S>(o, k, pb_vbil_mix(pb_pxi_channel<C, S>(a0, k), pb_pxi_channel<C, S>(a1, k), pb_pxi_channel<C, S>(a2, k), pb_pxi_channel<C, S>(a3, k), tx, ty));
    } else {
        float wx[4], wy[4], acc[C];
        pb_pxi_weights(tx, wx);
        pb_pxi_weights(ty, wy);
        unsigned c[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            int x = j0 - 1 + l;
            if (WRAP) x = x < 0 ? x + w : (x >= w ? x - w : x);  // (once: the header's note)
            c[l] = (unsigned)min(max(x, 0), w - 1);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned row = (unsigned)min(max(i0 - 1 + k, 0), h - 1) * (unsigned)w;
            Px t[4];
#pragma unroll
            for (int l = 0; l < 4; ++l) t[l] = pb_px_load<B>(s, (row + c[l]) * (unsigned)B);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                float sum = wx[0] * (float)pb_pxi_channel<C, S>(t[0], ch);
#pragma unroll
                for (int l = 1; l < 4; ++l) sum = fmaf(wx[l], (float)pb_pxi_channel<C, S>(t[l], ch), sum);
                acc[ch] = k == 0 ? wy[0] * sum : fmaf(wy[k], sum, acc[ch]);
            }
        }
        constexpr float top = S == 1 ? 255.0f : 65535.0f;
#pragma unroll
        for (int ch = 0; ch < C; ++ch)  // clipped, then rounded half to even by the 1.5 x 2^23 addend: the value is the low bits of the sum
            pb_pxi_put<C, S>(o, ch, __float_as_uint(__builtin_amdgcn_fmed3f(acc[ch], 0.0f, top) + 12582912.0f) & 0xFFFFu);
    }
    return pb_px_zero_if<B>(o, dead);
}

template <int SRC_KIND, int FILTER, int C, int S>
__global__ __launch_bounds__(64 * PB_PXI_WAVES, PB_PXI_WPE(FILTER)) void pb_px_interp_kernel(const PbHot Hd, const PbTileEntry* __restrict__ table,
                                                                                             const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                                             const unsigned groups_per_frame, unsigned long long src_stride,
                                                                                             unsigned long long dst_stride, const PbBilCoord* __restrict__ bil_xy,
                                                                                             const int32_t* __restrict__ fix_px, const PbBilCoord* __restrict__ fix_xy) {
    static_assert(SRC_KIND == PB_KIND_CAMERA || SRC_KIND == PB_KIND_PANO, "single sources with an interpolating tile kernel");
    static_assert(FILTER == PB_PXI_BILINEAR || FILTER == PB_PXI_CATMULL_ROM, "the two interpolating filters");
    static_assert(C >= 1 && C <= 4 && (S == 1 || S == 2) && C * S != 3, "1 to 4 channels of 8- or 16-bit samples; uint8 RGB has tile kernels of its own");
    constexpr int B = C * S;
    typedef PbPx<B> Px;
    constexpr int NW = Px::NW;
    constexpr bool WRAP = SRC_KIND == PB_KIND_PANO;
    constexpr bool NT = PB_NT_DEFAULT(SRC_KIND);
    __shared__ unsigned park[PB_PXI_WAVES][NW][PB_PX_PLANE];
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
    const unsigned vslot = (unsigned)__builtin_amdgcn_readfirstlane((int)pb_bil_slot_of<PB_PXI_WAVES>(wg, (unsigned)wave));
    pb_load_entry(table + vslot, entry);
    const PbTileEntry* __restrict__ e = &entry;
    const int flags = e->flags;
    if (flags & PB_TILE_SKIP) return;
    const int X0 = (e->tile_xy & 0xFFFF) * PB_TILE, Y0 = (int)((unsigned)e->tile_xy >> 16) * PB_TILE;
    const int W = Hd.dst_w, H = Hd.dst_h, h = Hd.src_h, w = Hd.src_w;
    const int xg = lane & 7, yb = lane >> 3;
    const int x = X0 + 4 * xg;  // the lane's store shape: columns x .. x + 3 of rows Y0 + yb + 8 * jr
    unsigned* p0 = park[wave][0];
    unsigned* p1 = park[wave][NW - 1];  // (the upper dword's plane of 6- and 8-byte pixels)

    if (e->bil_off < 0 && !(flags & (PB_TILE_LEAN | PB_TILE_DIRECT))) {  // BLACK (every other class has a table slot)
        Px z[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int i = 0; i < NW; ++i) z[k].w[i] = 0u;
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) pb_px_store_row<B, false>(dst, W, H, x, Y0 + yb + 8 * jr, z);
    } else if (e->bil_off >= 0) {
        // a table tile: the slot's exact coordinates, walked as pb_cr_vals walks them
        const PbBilCoord* __restrict__ t = bil_xy + (size_t)(e->bil_off & PB_BIL_SLOT_MASK) * (PB_TILE * PB_TILE);
        const int p = lane & 31, hh = lane >> 5;
        const bool by_rows = (flags & PB_TILE_TAB_Y) != 0;
        const int shift = pb_bil_slot_shift(e->bil_off, p);
#pragma unroll 1
        for (int g = 0; g < 4; ++g) {  // the lane's coordinates 4 g .. 4 g + 3: entries [2 n + hh][p] of the slot
            int2 c[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) c[m] = *reinterpret_cast<const int2*>(t + (2 * (4 * g + m) + hh) * PB_TILE + p);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                int i0, j0;
                float ty, tx;
                bool dead;
                pb_cr_of_q(c[m].x, c[m].y, i0, j0, ty, tx, dead);
                const int a = (2 * (4 * g + m) + hh + shift) & 31;  // (the slot is stored in walk order)
                const int py = by_rows ? p : a, px = by_rows ? a : p;
                const Px v = pb_pxi_px<FILTER, C, S, WRAP>(src, h, w, i0, j0, ty, tx, dead);
                p0[py * 33 + px] = v.w[0];
                if (NW > 1) p1[py * 33 + px] = v.w[NW - 1];
            }
        }
    } else {
        // a model tile: the tile model per pixel, evaluated as pb_cr_vals evaluates it; every pixel of such a tile inside the image is live
        const bool td3 = (flags & PB_TILE_TD3) != 0;
        const bool along_x = fabsf(e->c[1][0]) <= fabsf(e->c[5][0]);  // |d row / du| <= |d row / dv|
        const pb_f2 half = {0.5f, 0.5f};
        const int ar = e->anchor_r, ac = e->anchor_c;
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {
            // along_x: column 4 xg + q at rows yb + 8 m; else row yb + 8 q at columns 4 xg + m
            pb_f2 b[5], sv[4];
            if (td3) pb_bil_collapse<true>(e, along_x, along_x ? 4 * xg + q : yb + 8 * q, b);
            else pb_bil_collapse<false>(e, along_x, along_x ? 4 * xg + q : yb + 8 * q, b);
            b[0] = b[0] - half;  // s = f - 0.5, relative to the tile's anchor
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float tc = pb_tile_coord(along_x ? yb + 8 * m : 4 * xg + m);
                sv[m] = td3 ? pb_bil_eval<true>(b, tc) : pb_bil_eval<false>(b, tc);
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float fy = floorf(sv[m].x), fx = floorf(sv[m].y);
                const int py = along_x ? yb + 8 * m : yb + 8 * q, px = along_x ? 4 * xg + q : 4 * xg + m;
                const Px v = pb_pxi_px<FILTER, C, S, WRAP>(src, h, w, ar + (int)fy, ac + (int)fx, sv[m].x - fy, sv[m].y - fx, false);
                p0[py * 33 + px] = v.w[0];
                if (NW > 1) p1[py * 33 + px] = v.w[NW - 1];
            }
        }
    }
    if (e->bil_off >= 0 || (flags & (PB_TILE_LEAN | PB_TILE_DIRECT))) {  // (a black tile parked nothing)
        pb_wave_sync();
        // read back in the store shape and store
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            Px a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a[k].w[0] = p0[(yb + 8 * jr) * 33 + 4 * xg + k];
                if (NW > 1) a[k].w[NW - 1] = p1[(yb + 8 * jr) * 33 + 4 * xg + k];
            }
            pb_px_store_row<B, NT>(dst, W, H, x, Y0 + yb + 8 * jr, a);
        }
    }
    // this tile's fix pixels (where the model's coordinate is not certified): redone from their exact coordinates after the wave's own
    // stores have completed
    const int n_fix = e->fix_cnt;
    if (n_fix > 0 && e->bil_off < 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane < n_fix) {
            const unsigned p = (unsigned)fix_px[e->fix_off + lane];
            const PbBilCoord q = fix_xy[e->fix_off + lane];
            int i0, j0;
            float fty, ftx;
            bool dead;
            pb_cr_of_q(q.y, q.x, i0, j0, fty, ftx, dead);
            const Px v = pb_pxi_px<FILTER, C, S, WRAP>(src, h, w, i0, j0, fty, ftx, dead);
            pb_px_store1<B>(dst + (unsigned long long)B * p, v);
        }
    }
}
