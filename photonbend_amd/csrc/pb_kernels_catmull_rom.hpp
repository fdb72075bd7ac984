// pb_kernels_catmull_rom.hpp - OPT-IN Catmull-Rom sampling: the bilinear mode's definition with a 4 x 4 footprint.
//
// Like bilinear (pb_kernels_bilinear.hpp) this mode has no reference behaviour: its oracle is our own written definition
// (tests/catmull_rom_ref.py).  f is the reference's pre-truncation source coordinate; s = f - 0.5, i0 = floor(s), t = s - i0 (columns
// alike: j0, u).  The taps are rows i0 - 1 .. i0 + 2 x columns j0 - 1 .. j0 + 2: rows clamped to the image, a panorama's columns wrapped
// modulo w, a camera's clamped, an eye of a double fisheye clamped to its own half (the right eye mirrored).  The weights are Keys' cubic
// with a = -0.5, in float64 and in exactly this order:
//   w-1 = ((-0.5 t + 1.0) t - 0.5) t      w0 = (1.5 t - 2.5) t t + 1.0      w1 = ((-1.5 t + 2.0) t + 0.5) t      w2 = (0.5 t - 0.5) t t
// Per channel the four row sums r_k = sum_l wx_l tap(k, l) (l = -1 .. 2, plain sequential adds), then v = sum_k wy_k r_k the same way,
// rounded half to even and clipped to the sample type's range (the cubic overshoots).  Black exactly where the bilinear mode is black.
// A double-fisheye source blends the two eyes' rounded samples like the reference, (l fl + r fr).astype(uint8).
//
//   PbCatmullRom                       the FILTER of the shared sampler kernels of pb_kernels_bilinear.hpp: with it
//                                      pb_sample_map_interp_kernel is the definition per pixel from a materialised map, any image (C channels
//                                      of 8- or 16-bit samples); pb_interp_fix_kernel the definition per pixel from the plan's float64 chain -
//                                      every pixel (PB_MODE_FAITHFUL, deferred plans, plans without the bilinear mode's tables) or the tiles
//                                      and fix pixels the tile kernel leaves to it; pb_interp_double_kernel the same for double-fisheye sources
//   pb_catmull_rom_hot_kernel          THE hot path, single sources: one wave per tile over the bilinear mode's launch-order table,
//                                      coordinates from its certified tile models and exact coordinate tables, float32 arithmetic
// The float64 kernels evaluate the definition's own expressions under the build's -ffp-contract=off: their bytes are the definition's.
#pragma once
#include "pb_kernels_bilinear.hpp"

// ---- the definition, float64 -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pb_cr64_weights(double t, double w[4]) {
    w[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
    w[1] = (1.5 * t - 2.5) * t * t + 1.0;
    w[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
    w[3] = (0.5 * t - 0.5) * t * t;
}
// The FILTER (pb_kernels_bilinear.hpp) of this mode: PbBilinear's 4 x 4 sibling.  Its per-pixel routes ARE the definition: the coordinate as
// the map kernel computes it from the chain's (lat, lon), liveness bound 1.0e300, sample64 per channel.
struct PbCatmullRom {
    template <typename SAMPLE, bool WRAP>
    static __device__ __forceinline__ double sample64(const SAMPLE* __restrict__ img, double fy, double fx, int h, int w, int cmin, int cmax, bool mirror,
                                                      int channels, int ch) {
        const double sy = fy - 0.5, sx = fx - 0.5;
        const double ry = floor(sy), rx = floor(sx);
        double wy[4], wx[4];
        pb_cr64_weights(sy - ry, wy);
        pb_cr64_weights(sx - rx, wx);
        long long r[4], g[4];
        pb_tap_addr<4, WRAP>((long long)ry - 1, (long long)rx - 1, h, cmin, cmax, mirror, r, g);
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double s = wx[0] * pb_bil64_tap(img, r[k], g[0], w, channels, ch);
            s = s + wx[1] * pb_bil64_tap(img, r[k], g[1], w, channels, ch);
            s = s + wx[2] * pb_bil64_tap(img, r[k], g[2], w, channels, ch);
            s = s + wx[3] * pb_bil64_tap(img, r[k], g[3], w, channels, ch);
            v = (k == 0) ? wy[0] * s : v + wy[k] * s;
        }
        v = rint(v);
        const double vmax = (double)(SAMPLE)~(SAMPLE)0;
        return v < 0.0 ? 0.0 : (v > vmax ? vmax : v);
    }
    // one source's (or eye's) uint8 RGB pixel
    template <bool WRAP>
    static __device__ __forceinline__ unsigned rgb(const uint8_t* __restrict__ s, double fy, double fx, int h, int w, int cmin, int cmax, bool mirror) {
        unsigned out = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out |= (unsigned)sample64<uint8_t, WRAP>(s, fy, fx, h, w, cmin, cmax, mirror, 3, ch) << (8 * ch);
        return out;
    }
    struct Px {
        bool live;
        double fy, fx;
        int face;  // a cube source: the selected face ((fy, fx) is the position on it)
    };
    template <int SRC_KIND>
    static __device__ __forceinline__ Px prepare(const PbParams& P, const PbCoord& c) {
        Px q;
        q.face = 0;
        if (pb_is_cube(SRC_KIND)) {
            q.fy = q.fx = 0.0;
            q.live = false;
            if (c.inv) return q;
            const PbCubePos h = pb_src_cube_pos<SRC_KIND == PB_KIND_EAC>(P, c);
            q.face = h.face;
            q.fy = h.fy;
            q.fx = h.fx;
            q.live = pb_live_in(h.fy, h.fx, 1.0e300, pb_cube_n(P.src), pb_cube_n(P.src));
            return q;
        }
        if (SRC_KIND == PB_KIND_PANO) {
            q.fy = c.lat / P.src_hseg;
            q.fx = c.lon / P.src_wseg + P.src_half_w;
            q.live = !c.inv && pb_live(q.fy, q.fx, 1.0e300);
        } else {
            double sl, cl;
            pb_expi_np(c.lon, &sl, &cl);
            const double dist = pb_lens_forward(P, c.lat) * P.src.f_distance;
            q.fy = ((sl * dist) * -1.0) + P.src_cy;
            q.fx = (cl * dist) + P.src_cx;
            q.live = !c.inv && pb_live_in(q.fy, q.fx, 1.0e300, P.src.height, P.src.width);
        }
        return q;
    }
    template <int SRC_KIND>
    static __device__ __forceinline__ unsigned sample(const PbParams& P, const Px& q, const uint8_t* __restrict__ s) {
        if (pb_is_cube(SRC_KIND)) {  // the face as an image of its own (N rows of pitch w): the taps stay on it
            const int n = pb_cube_n(P.src);
            const uint8_t* face = s + 3ull * ((unsigned long long)pb_cube_row0(q.face, n) * (unsigned)P.src.width + (unsigned)pb_cube_col0(q.face, n));
            return q.live ? rgb<false>(face, q.fy, q.fx, n, P.src.width, 0, n, false) : 0u;
        }
        return q.live ? rgb<SRC_KIND == PB_KIND_PANO>(s, q.fy, q.fx, P.src.height, P.src.width, 0, P.src.width, false) : 0u;
    }
    static __device__ __forceinline__ unsigned eye(const PbParams& P, const uint8_t* __restrict__ s, double lat, double sl, double cl, int we, double cx,
                                                   int cmin, bool mirror) {
        const double dist = pb_lens_forward(P, lat) * P.src.f_distance;
        const double fy = ((sl * dist) * -1.0) + P.src_cy, fx = (cl * dist) + cx;
        return pb_live_in(fy, fx, 1.0e300, P.src.height, we) ? rgb<false>(s, fy, fx, P.src.height, P.src.width, cmin, cmin + we, mirror) : 0u;
    }
};

// ---- the tile kernel: float32 arithmetic -------------------------------------------------------------------------------------------
// Precision budget.  The tile models are certified to PB_COARSE_PX = 1/1024 px per axis against the faithful coordinate; the
// coordinate tables hold it to 2^-13 px.  On the steepest content (taps 127.5 from their mean) the cubic's sum of |w'| <= 3 and sum of
// |w| <= 1.25 (both at t = 1/2) turn 1/1024 px per axis into at most 127.5 (1.25 x 3 + 3 x 1.25) / 1024 = 0.93 LSB before rounding: a
// pixel may move by 1.  The float32 arithmetic below adds rounding of order 1e-4 LSB (weights to 2^-24 relative, sixteen products of at
// most 255 and their running sums, each rounded to 2^-24 relative) - far inside the remaining 0.07 LSB.

// The weights of two pixels at once (packed float32: v_pk_fma_f32 / v_pk_mul_f32).
__device__ __forceinline__ void pb_cr_w2(const pb_f2 t, pb_f2 w[4]) {
    const pb_f2 t2 = t * t;
    const pb_f2 a = {-0.5f, -0.5f}, one = {1.0f, 1.0f}, b = {1.5f, 1.5f}, c = {-2.5f, -2.5f}, d = {-1.5f, -1.5f}, e = {2.0f, 2.0f}, h = {0.5f, 0.5f};
    w[0] = __builtin_elementwise_fma(__builtin_elementwise_fma(a, t, one), t, a) * t;
    w[1] = __builtin_elementwise_fma(__builtin_elementwise_fma(b, t, c), t2, one);
    w[2] = __builtin_elementwise_fma(__builtin_elementwise_fma(d, t, e), t, h) * t;
    w[3] = __builtin_elementwise_fma(h, t, a) * t2;
}
// byte b (0..11) of a 12-byte tap row as a float
__device__ __forceinline__ float pb_cr_byte(const unsigned r[3], int b) { return (float)((r[b >> 2] >> (8 * (b & 3))) & 0xFFu); }
// Two pixels' values from their four 12-byte tap rows (tap l's channel c at byte 3 l + c), packed RGB.  Row sums first, then the column
// sum, per channel; clipped to [0, 255] and rounded half to even by the 1.5 x 2^23 addend (the value is then the low byte of the sum's bits).
__device__ __forceinline__ void pb_cr_mix2(const unsigned ra[4][3], const unsigned rb[4][3], const pb_f2 tx, const pb_f2 ty, unsigned out[2]) {
    pb_f2 wx[4], wy[4];
    pb_cr_w2(tx, wx);
    pb_cr_w2(ty, wy);
    pb_f2 acc[3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            pb_f2 s = wx[0] * (pb_f2){pb_cr_byte(ra[k], ch), pb_cr_byte(rb[k], ch)};
#pragma unroll
            for (int l = 1; l < 4; ++l) s = __builtin_elementwise_fma(wx[l], (pb_f2){pb_cr_byte(ra[k], 3 * l + ch), pb_cr_byte(rb[k], 3 * l + ch)}, s);
            acc[ch] = k == 0 ? wy[0] * s : __builtin_elementwise_fma(wy[k], s, acc[ch]);
        }
    unsigned m[2][3];
    const pb_f2 magic = {12582912.0f, 12582912.0f};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const pb_f2 v = {__builtin_amdgcn_fmed3f(acc[ch].x, 0.0f, 255.0f), __builtin_amdgcn_fmed3f(acc[ch].y, 0.0f, 255.0f)};
        const pb_f2 r = v + magic;
        m[0][ch] = __float_as_uint(r.x);
        m[1][ch] = __float_as_uint(r.y);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)  // v_perm_b32(S0, S1, sel): selector 0-3 = bytes of S1, 4-7 = bytes of S0, 0x0c = 0x00
        out[i] = __builtin_amdgcn_perm(m[i][2], __builtin_amdgcn_perm(m[i][1], m[i][0], 0x0c0c0400u), 0x0c040100u);
}

// A pixel's four tap rows: (i0, j0) = floor(s), the footprint rows i0 - 1 .. i0 + 2 and columns j0 - 1 .. j0 + 2.  INSIDE the image
// (no tap clamped or wrapped): one 12-byte load per row, which ends at the footprint's last byte and so never passes the frame's end.
// Anywhere else (an image edge, the panorama's seam): each tap by itself, rows clamped, columns wrapped (WRAP) or clamped, three byte
// loads per tap - any frame size.
template <bool WRAP>
__device__ __forceinline__ void pb_cr_rows(const uint8_t* __restrict__ s, int i0, int j0, int h, int w, unsigned r[4][3]) {
    const bool inside = i0 >= 1 && i0 + 2 <= h - 1 && j0 >= 1 && j0 + 2 <= w - 1;
    if (inside) {
        const unsigned rowbytes = 3u * (unsigned)w;
        const unsigned o = (unsigned)(i0 - 1) * rowbytes + 3u * (unsigned)(j0 - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) __builtin_memcpy(r[k], s + o + (unsigned)k * rowbytes, 12);
    } else {
        int c[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            int x = j0 - 1 + l;
            if (WRAP) {
                x %= w;
                if (x < 0) x += w;
            }
            c[l] = min(max(x, 0), w - 1);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = min(max(i0 - 1 + k, 0), h - 1);
            unsigned p[4];
#pragma unroll
            for (int l = 0; l < 4; ++l) p[l] = pb_load_px(s, y * w + c[l]);
            r[k][0] = p[0] | (p[1] << 24);
            r[k][1] = (p[1] >> 8) | (p[2] << 16);
            r[k][2] = (p[2] >> 16) | (p[3] << 8);
        }
    }
}

// Two pixels from their tap bases (i0, j0) and fractions (ty, tx); dead[n]: black.  Their eight row loads are in flight together before
// the arithmetic (four pixels at a time spilled at 128 VGPRs).
template <bool WRAP>
__device__ __forceinline__ void pb_cr_px2(const uint8_t* __restrict__ s, const int i0[2], const int j0[2], const float ty[2], const float tx[2],
                                          const bool dead[2], int h, int w, unsigned out[2]) {
    unsigned r[2][4][3];
#pragma unroll
    for (int n = 0; n < 2; ++n) pb_cr_rows<WRAP>(s, i0[n], j0[n], h, w, r[n]);
    const pb_f2 tx2 = {tx[0], tx[1]}, ty2 = {ty[0], ty[1]};
    pb_cr_mix2(r[0], r[1], tx2, ty2, out);
#pragma unroll
    for (int n = 0; n < 2; ++n)
        if (dead[n]) out[n] = 0u;
}

// a PbBilCoord (1/4096 px, s = f - 0.5) as the tap base and fractions
__device__ __forceinline__ void pb_cr_of_q(int qy, int qx, int& i0, int& j0, float& ty, float& tx, bool& dead) {
    dead = qy == PB_BIL_DEAD;
    if (dead) qy = qx = 0;
    i0 = qy >> PB_BIL_SHIFT;  // (arithmetic shifts: floor)
    j0 = qx >> PB_BIL_SHIFT;
    ty = (float)(qy & ((1 << PB_BIL_SHIFT) - 1)) * (1.0f / (float)(1 << PB_BIL_SHIFT));
    tx = (float)(qx & ((1 << PB_BIL_SHIFT) - 1)) * (1.0f / (float)(1 << PB_BIL_SHIFT));
}

// v[jr * 4 + k] = the sample of pixel (4 xg + k, yb + 8 jr) of the tile (the lane's four 12-byte stores), packed RGB.
//   table   the entry names a slot of the exact coordinate table: walked as pb_bil_vals walks it (lane = a column or row of the tile,
//           sheared along the line of constant source row);
//   black   nothing of the tile samples this source;
//   model   LEAN / DIRECT tiles: the tile model per pixel, evaluated exactly as the bilinear window path evaluates it (column-first when
//           the source row changes least along x), taps straight from global memory (no LDS windows: a bilinear window carries one texel
//           of margin, the 4 x 4 footprint needs two on the far side).
// Both paths park each pixel in the wave's LDS `park` ([y][x], 33-dword pitch) and the lane reads its sixteen back for the stores: the
// loops stay rolled (unrolled, the compiler hoisted every pixel's tap loads to the top and spilled them).
template <bool WRAP>
__device__ __forceinline__ void pb_cr_vals(const PbHot& Hd, const PbTileEntry* __restrict__ e, const int flags, const int lane, unsigned* park,
                                           const uint8_t* __restrict__ s, const PbBilCoord* __restrict__ bil_xy, unsigned v[16]) {
    const int xg = lane & 7, yb = lane >> 3;
    const int h = Hd.src_h, w = Hd.src_w;
    if (e->bil_off < 0 && !(flags & (PB_TILE_LEAN | PB_TILE_DIRECT))) {  // BLACK (every other class has a table slot)
#pragma unroll
        for (int n = 0; n < 16; ++n) v[n] = 0u;
        return;
    }
    if (e->bil_off >= 0) {
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
            for (int m0 = 0; m0 < 4; m0 += 2) {
                int i0[2], j0[2];
                float ty[2], tx[2];
                bool dead[2];
                unsigned o[2];
#pragma unroll
                for (int n = 0; n < 2; ++n) pb_cr_of_q(c[m0 + n].x, c[m0 + n].y, i0[n], j0[n], ty[n], tx[n], dead[n]);
                pb_cr_px2<WRAP>(s, i0, j0, ty, tx, dead, h, w, o);
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const int a = (2 * (4 * g + m0 + n) + hh + shift) & 31;  // (the slot is stored in walk order)
                    park[by_rows ? p * 33 + a : a * 33 + p] = o[n];
                }
            }
        }
    } else {
        const bool td3 = (flags & PB_TILE_TD3) != 0;
        const bool along_x = fabsf(e->c[1][0]) <= fabsf(e->c[5][0]);  // |d row / du| <= |d row / dv|
        const pb_f2 half = {0.5f, 0.5f};
        const int ar = e->anchor_r, ac = e->anchor_c;
        const bool dead[2] = {false, false};
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
            for (int m0 = 0; m0 < 4; m0 += 2) {
                int i0[2], j0[2];
                float ty[2], tx[2];
                unsigned o[2];
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const float fy = floorf(sv[m0 + n].x), fx = floorf(sv[m0 + n].y);
                    i0[n] = ar + (int)fy;
                    j0[n] = ac + (int)fx;
                    ty[n] = sv[m0 + n].x - fy;
                    tx[n] = sv[m0 + n].y - fx;
                }
                pb_cr_px2<WRAP>(s, i0, j0, ty, tx, dead, h, w, o);
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const int m = m0 + n;
                    park[along_x ? (yb + 8 * m) * 33 + 4 * xg + q : (yb + 8 * q) * 33 + 4 * xg + m] = o[n];
                }
            }
        }
    }
    pb_wave_sync();
#pragma unroll
    for (int jr = 0; jr < 4; ++jr)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[jr * 4 + k] = park[(yb + 8 * jr) * 33 + 4 * xg + k];
}

// One wave per tile over the bilinear mode's launch-order table, four waves per workgroup (pb_bil_slot_of<4>), frames of a batch a grid
// dimension.  The tile's fix pixels are redone from their exact coordinates after the tile's stores, like pb_bilinear_hot_kernel's.
// bil_xy == nullptr: the plan has no coordinate table; its table tiles and fix pixels are left to pb_interp_fix_kernel<PbCatmullRom>.
#define PB_CR_WAVES 4
#define PB_CR_WPE 3  // waves per SIMD the tile kernel is compiled for (its register budget: 168 VGPRs; at 128 it spills)
template <int SRC_KIND>
__global__ __launch_bounds__(64 * PB_CR_WAVES, PB_CR_WPE) void pb_catmull_rom_hot_kernel(const PbHot Hd, const PbTileEntry* __restrict__ table,
                                                                               const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                               const unsigned groups_per_frame, unsigned long long src_stride,
                                                                               unsigned long long dst_stride, const PbBilCoord* __restrict__ bil_xy,
                                                                               const int32_t* __restrict__ fix_px, const PbBilCoord* __restrict__ fix_xy) {
    __shared__ unsigned park[PB_CR_WAVES][PB_TILE * 33];
    constexpr bool WRAP = SRC_KIND == PB_KIND_PANO;
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
    const unsigned vslot = (unsigned)__builtin_amdgcn_readfirstlane((int)pb_bil_slot_of<PB_CR_WAVES>(wg, (unsigned)wave));
    pb_load_entry(table + vslot, entry);
    const PbTileEntry* __restrict__ e = &entry;
    const int flags = e->flags;
    if (flags & PB_TILE_SKIP) return;
    if (e->bil_off >= 0 && !bil_xy) return;  // (no coordinate table: the float64 kernel owns the tile)
    const int tx = e->tile_xy & 0xFFFF, ty = (int)((unsigned)e->tile_xy >> 16);
    unsigned v[16];
    pb_cr_vals<WRAP>(Hd, e, flags, lane, park[wave], src, bil_xy, v);
    pb_bil_store<SRC_KIND == PB_KIND_CAMERA>(v, dst, tx * PB_TILE, ty * PB_TILE, lane, Hd.dst_w, Hd.dst_h);
    const int n_fix = e->fix_cnt;
    if (n_fix > 0 && fix_xy && e->bil_off < 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the wave's own stores have completed
        if (lane < n_fix) {
            const unsigned p = (unsigned)fix_px[e->fix_off + lane];
            const PbBilCoord q = fix_xy[e->fix_off + lane];
            int i0, j0;
            float fty, ftx;
            bool dead;
            pb_cr_of_q(q.y, q.x, i0, j0, fty, ftx, dead);
            unsigned r[4][3], o[2];
            pb_cr_rows<WRAP>(src, i0, j0, Hd.src_h, Hd.src_w, r);
            pb_cr_mix2(r, r, (pb_f2){ftx, ftx}, (pb_f2){fty, fty}, o);
            const unsigned px = dead ? 0u : o[0];
            uint8_t* d = dst + 3ull * p;
            pb_store_px(d, px);
        }
    }
}
