// pb_kernels_pxf_interp.hpp - OPT-IN bilinear and Catmull-Rom sampling of float16 and float32 frames (pb_remap_interp_pxf):
// the interpolating tile kernel for pixels of C channels of S-byte IEEE samples, (C, S) in {1, 2, 3, 4} x {2, 4} - binary16 and binary32.
// The pixel is B = C * S bytes: {2, 4, 6, 8} for half samples, {4, 8, 12, 16} for single ones.
//
// The definition is tests/pxf_ref.py: the integer modes'  up to the sum, and no further.  f is the reference's
// pre-truncation source coordinate, s = f - 0.5, i0 = floor(s), t = s - i0 per axis.
//   bilinear      taps i0, i0 + 1 per axis; per channel top = a + tx (b - a), bot likewise, V = top + ty (bot - top).
//   Catmull-Rom   taps i0 - 1 .. i0 + 2 per axis, Keys' weights with a = -0.5; per channel the four row sums, then the column sum V.
// Rows clamped, a panorama's columns wrapped modulo w, a camera's clamped.  V is narrowed ONCE to the sample type, round to nearest even:
// no rounding to an integer and no clip - the cubic's overshoot and negative lobes are kept, a half result beyond 65504 is IEEE's infinity.
// A pixel that is not live is +0.0 in every channel: all bytes zero.
//
// pb_pxf_interp_kernel<SRC_KIND, FILTER, C, S> has pb_px_interp_kernel's launch shape, tile walk, coordinates, fix pixels, BLACK tiles
// and stores (pb_kernels_px_interp.hpp, whose comments hold): one wave per slot of the bilinear mode's launch-order table, four waves per
// workgroup through pb_bil_slot_of<4>, frames of a batch a grid dimension with 64-bit frame offsets, the tile entry in SGPRs, table tiles
// through pb_cr_of_q, LEAN / DIRECT tiles through pb_bil_collapse / pb_bil_eval in their certified orientation, fix pixels from bil_fix_xy
// behind s_waitcnt vmcnt(0).  No plan state, no preparation pass.  The walk is written out here, beside pb_px_interp_kernel's, as that one
// is beside pb_planar_bilinear_kernel's: the 28 pb_px_interp_kernel listings are pinned and a shared walk was not tried against them.
//
// Sampling.  Every tap is ONE pb_px_load<B> of exactly the pixel's own bytes, rows and columns clamped for EVERY pixel without a branch, a
// panorama's columns wrapped once first - pb_pxi_px's rules, for its reasons.  A dead pixel reads pixel 0 and is zeroed by a SELECT
// (pb_px_zero_if), never by a multiplication: a NaN or an infinity at pixel 0 reaches no dead pixel.  A sample enters the sums of the
// pixels whose footprint holds it and of no other, so a non-finite sample spoils those pixels alone.  Half samples are widened with
// v_cvt_f32_f16, which is exact; all arithmetic is float32 - no float64, no packed-half arithmetic -; the result is narrowed once
// (v_cvt_f16_f32, round to nearest even; single: the sum itself).  Catmull-Rom walks its footprint row by row with pb_pxi_weights, as
// pb_pxi_px does: one row of taps is live per pixel.
//
// Float32 arithmetic, rounding by rounding.  u = 2^-24; a frame's samples lie in [L, U], D = U - L, M = max(|L|, |U|); t in [0, 1).
//   bilinear      b - a: exact difference at most D, rounded: u D.  top = fmaf(tx, b - a, a): the carried u D, and one rounding of a value
//                 in [L, U]: u M.  |d top|, |d bot| <= u D + u M.  bot - top: at most D, rounded: u D, and the carried 2 (u D + u M).
//                 fmaf(ty, bot - top, top) = (1 - ty) top + ty bot: carries at most max(|d top|, |d bot|) + ty u D, one rounding u M.
//                 |dV| <= 3 u D + 2 u M to first order in u; with room for the second-order terms, 4 u D + 4 u M <= 12 u M (D <= 2 M)
//                 < 16 u M = M 2^-20, the arithmetic's share of T_bil.
//   Catmull-Rom   pb_kernels_px_interp.hpp's bound with M for R - the same weights, the same products and fused multiply-adds in the same
//                 order, on taps that are exact floats of magnitude at most M: sum |dw| <= 8.25 u, |d row| <= 13.25 u M,
//                 |dV| <= 33.125 u M < 64 u M = M 2^-18, the arithmetic's share of T_cr.
//   narrowing     one rounding of V: at most u_out |V|, u_out = 2^-11 for half (single: none beyond the last rounding above), |V| <= M
//                 bilinear and <= 1.25^2 M Catmull-Rom.
// tests/test_pxf_host.py emulates both orders in float32 on worst-case and random taps and holds them inside these shares.
//
// Stores.  A pixel is parked in the wave's regrouping planes - [y][x], 33-dword pitch, ONE PLANE PER DWORD of the pixel: one for pixels of
// up to 4 bytes, two for 6 and 8, three for 12, four for 16 - and read back in the store shape (four pixels of a row); they leave through
// pb_px_store_row: pb_px_store4 (up to 48 and 64 bytes as three and four 16-byte stores) where all four exist and their first byte is 4-byte
// aligned, else pb_px_store1 in units of A = min(4, B & -B), clipped to the image.  Fix pixels: pb_px_store1.
//
// Limits: pb_remap_px's (32-bit byte offsets inside a frame, sources below 32768 px a side).  LDS: 4224 bytes per wave and plane - 16896
// a workgroup for one plane, 67584 for four.  Three and four planes hold a CU's 160 KiB to three and two workgroups; those rows are
// compiled for two waves per SIMD, which is what their LDS allows (DESIGN 3.24 has the choice and its reason).
#pragma once
#include "pb_kernels_px_interp.hpp"

// waves per SIMD the kernel is compiled for: pb_px_interp_kernel's for pixels of up to two dwords; pixels of three and four are held to
// two by their planes, so the compiler may as well have the registers
#define PB_PXF_WPE(filter, bytes) ((bytes) > 8 ? 2 : PB_PXI_WPE(filter))

// channel k of a loaded pixel, widened to float32 (exact)
template <int C, int S>
__device__ __forceinline__ float pb_pxf_channel(const PbPx<C * S>& v, const int k) {
    if constexpr (S == 4) return __uint_as_float(v.w[k]);
    else return (float)__builtin_bit_cast(_Float16, (unsigned short)(v.w[k >> 1] >> (16 * (k & 1))));
}
// ... narrowed once (round to nearest even) into a pixel whose dwords start as zero.  The float32 value is pinned in a register first:
// left to itself the compiler folds the last fused multiply-add and the narrowing into v_fma_mixlo_f16, which rounds the exact sum to
// binary16 in ONE step - not the float32 result narrowed, and so not float16(the float32 frame's result), which is what a half frame's
// result is defined as (tests/test_hip_pxf_interp.py holds the two kernels to each other bit for bit).
template <int C, int S>
__device__ __forceinline__ void pb_pxf_put(PbPx<C * S>& v, const int k, float val) {
    if constexpr (S == 4) {
        v.w[k] = __float_as_uint(val);
    } else {
        asm("" : "+v"(val));
        v.w[k >> 1] |= (unsigned)__builtin_bit_cast(unsigned short, (_Float16)val) << (16 * (k & 1));
    }
}

// One output pixel from its tap base (i0, j0) and fractions (ty, tx); dead: +0.0 in every channel, by a select.
template <int FILTER, int C, int S, bool WRAP>
__device__ __forceinline__ PbPx<C * S> pb_pxf_px(const uint8_t* __restrict__ s, const int h, const int w, int i0, int j0, const float ty, const float tx,
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
        for (int k = 0; k < C; ++k) {
            const float fa = pb_pxf_channel<C, S>(a0, k), fc = pb_pxf_channel<C, S>(a2, k);
            const float top = fmaf(tx, pb_pxf_channel<C, S>(a1, k) - fa, fa), bot = fmaf(tx, pb_pxf_channel<C, S>(a3, k) - fc, fc);
            pb_pxf_put<C, S>(o, k, fmaf(ty, bot - top, top));
        }
    } else {
        float wx[4], wy[4], acc[C];
        pb_pxi_weights(tx, wx);
        pb_pxi_weights(ty, wy);
        unsigned c[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            int x = j0 - 1 + l;
            if (WRAP) x = x < 0 ? x + w : (x >= w ? x - w : x);  // (once: pb_kernels_px_interp.hpp's note)
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
                float sum = wx[0] * pb_pxf_channel<C, S>(t[0], ch);
#pragma unroll
                for (int l = 1; l < 4; ++l) sum = fmaf(wx[l], pb_pxf_channel<C, S>(t[l], ch), sum);
                acc[ch] = k == 0 ? wy[0] * sum : fmaf(wy[k], sum, acc[ch]);
            }
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) pb_pxf_put<C, S>(o, ch, acc[ch]);
    }
    return pb_px_zero_if<B>(o, dead);
}

template <int SRC_KIND, int FILTER, int C, int S>
__global__ __launch_bounds__(64 * PB_PXI_WAVES, PB_PXF_WPE(FILTER, C * S)) void pb_pxf_interp_kernel(const PbHot Hd, const PbTileEntry* __restrict__ table,
                                                                                                      const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                                                      const unsigned groups_per_frame, unsigned long long src_stride,
                                                                                                      unsigned long long dst_stride,
                                                                                                      const PbBilCoord* __restrict__ bil_xy,
                                                                                                      const int32_t* __restrict__ fix_px,
                                                                                                      const PbBilCoord* __restrict__ fix_xy) {
    static_assert(SRC_KIND == PB_KIND_CAMERA || SRC_KIND == PB_KIND_PANO, "single sources with an interpolating tile kernel");
    static_assert(FILTER == PB_PXI_BILINEAR || FILTER == PB_PXI_CATMULL_ROM, "the two interpolating filters");
    static_assert(C >= 1 && C <= 4 && (S == 2 || S == 4), "1 to 4 channels of binary16 or binary32 samples");
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
    unsigned* pl = park[wave][0];  // dword i of pixel (py, px): pl[i * PB_PX_PLANE + py * 33 + px]

    if (e->bil_off < 0 && !(flags & (PB_TILE_LEAN | PB_TILE_DIRECT))) {  // BLACK (every other class has a table slot)
        Px z[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int i = 0; i < NW; ++i) z[k].w[i] = 0u;
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) pb_px_store_row<B, false>(dst, W, H, x, Y0 + yb + 8 * jr, z);
    } else if (e->bil_off >= 0) {
        // a table tile: the slot's exact coordinates, walked as pb_px_interp_kernel walks them
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
                const Px v = pb_pxf_px<FILTER, C, S, WRAP>(src, h, w, i0, j0, ty, tx, dead);
#pragma unroll
                for (int i = 0; i < NW; ++i) pl[i * PB_PX_PLANE + py * 33 + px] = v.w[i];
            }
        }
    } else {
        // a model tile: the tile model per pixel, evaluated as pb_px_interp_kernel evaluates it; every pixel of such a tile inside the image is live
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
                const Px v = pb_pxf_px<FILTER, C, S, WRAP>(src, h, w, ar + (int)fy, ac + (int)fx, sv[m].x - fy, sv[m].y - fx, false);
#pragma unroll
                for (int i = 0; i < NW; ++i) pl[i * PB_PX_PLANE + py * 33 + px] = v.w[i];
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
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int i = 0; i < NW; ++i) a[k].w[i] = pl[i * PB_PX_PLANE + (yb + 8 * jr) * 33 + 4 * xg + k];
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
            const Px v = pb_pxf_px<FILTER, C, S, WRAP>(src, h, w, i0, j0, fty, ftx, dead);
            pb_px_store1<B>(dst + (unsigned long long)B * p, v);
        }
    }
}
