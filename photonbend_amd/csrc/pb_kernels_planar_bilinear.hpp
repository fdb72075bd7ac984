// pb_kernels_planar_bilinear.hpp - OPT-IN bilinear sampling of video frames (pb_remap_planar_bilinear, pb_remap_nv12_bilinear):
// planar 4:4:4 / 4:2:2 / 4:2:0 frames and NV12 / P010, three planes of a tile in ONE launch.
//
// The definition is written down in tests/video_bilinear_ref.py.  f is the reference's pre-truncation source coordinate of an output pixel.
//   plane 0       the bilinear mode's definition on a grey image: s = f - 0.5, i0 = floor(s), t = s - i0, taps i0, i0 + 1 per axis, rows
//                 clamped, a panorama's columns wrapped, a camera's clamped; top = a + tx (b - a), bot likewise, rint(top + ty (bot - top));
//                 fill[0] where the pixel is not live.
//   planes 1, 2   sample (i, j) belongs to its ANCHOR, output pixel (i << CY, j << CX) - the nearest kernels' rule.  Chroma is co-sited
//                 with the top-left luma pixel of its block, in source and destination alike, so the anchor's coordinate in chroma sample
//                 units is s_c = s / (1 << C) per axis: the same expression on the (h >> CY, w >> CX) plane, rows clamped to that plane, a
//                 panorama's columns wrapped modulo w >> CX; fill[k] where the anchor is not live.  Only the anchor decides.
//
// pb_planar_bilinear_kernel<SRC_KIND, S, SUB, PAIRS> has pb_catmull_rom_hot_kernel's launch shape (one wave per slot of the bilinear
// mode's launch-order table, four waves per workgroup through pb_bil_slot_of<4>, frames of a batch a grid dimension, the entry in SGPRs)
// and pb_cr_vals' coordinates: table tiles walk their bil_xy slot in its stored order, LEAN / DIRECT tiles evaluate the certified tile
// model (pb_bil_collapse / pb_bil_eval, TD3 where flagged), BLACK tiles store fills, fix pixels are redone from bil_fix_xy behind
// s_waitcnt vmcnt(0) - an anchor among them redoes its two chroma samples.  It adds no plan state and no preparation pass.
//   PAIRS   (with SUB = 4:2:0 only) planes 1 and 2 are the interleaved (U, V) plane of NV12 / P010: one 2 * S-byte load per chroma tap,
//           pair stores.  The layout travels in the same PbPlanar: o1 = the pair plane's offset, cpitch = its pitch, o2 unused.
//
// Sampling.  Four taps per sample straight from global memory, each loaded with exactly its S (or 2 * S) bytes: no load leaves its plane.
// The tap rows and columns are clamped (and a panorama's wrapped once: a live coordinate lies in [-0.5, w - 0.5]) for EVERY sample, in
// six integer instructions per axis and without a branch: inside the image that changes nothing, and the pixels of a tile that lie
// outside the destination - whose model coordinates are anything - cannot leave the plane either.  A dead pixel reads its plane's first
// sample and takes the fill after the loads.  Weights and sums are float32 (differences of samples are exact, three fused multiply-adds
// per sample); the result is rounded half to even by the 1.5 x 2^23 addend.  The chroma coordinate comes from the anchor's luma tap
// base and fraction, halved where subsampled: i_c = i0 >> C, t_c = ((i0 & 1) + t) / 2 - exact in float32 - computed by the lane that
// owns the anchor.
//
// Stores.  A pixel's plane-0 sample is parked in the wave's first regrouping plane ([y][x], 33-dword pitch), an anchor's two chroma
// samples as U | V << 16 at the anchor's place of the second; the lanes read them back in the store shape (four pixels of a row) and
// they leave through pb_nv12_store_y, pb_planar_store_c and pb_nv12_store_uv, clipped to their planes.  Padding is never read or written.
//
// Scalar registers: pb_video.hpp's rule - the layouts and fills live in vector registers, the tile entry stays in SGPRs.
// Limits: pb_remap_planar's (32-bit byte offsets inside a frame, sources below 32768 px a side).  LDS: 8448 bytes per wave.
#pragma once
#include "pb_kernels_catmull_rom.hpp"
#include "pb_video.hpp"

#define PB_VBIL_WAVES 4
#define PB_VBIL_WPE 4  // waves per SIMD the kernel is compiled for (128 VGPRs)

// the four taps' rows and columns on a plane (h, w)
template <bool WRAP>
__device__ __forceinline__ void pb_vbil_rc(const int i0, const int j0, const int h, const int w, unsigned r[2], unsigned c[2]) {
    r[0] = (unsigned)min(max(i0, 0), h - 1);
    r[1] = (unsigned)min(max(i0 + 1, 0), h - 1);
    int c0 = j0, c1 = j0 + 1;
    if (WRAP) {
        c0 = c0 < 0 ? c0 + w : (c0 >= w ? c0 - w : c0);
        c1 = c1 < 0 ? c1 + w : (c1 >= w ? c1 - w : c1);
    }
    c[0] = (unsigned)min(max(c0, 0), w - 1);
    c[1] = (unsigned)min(max(c1, 0), w - 1);
}
// top = a + tx (b - a), bot likewise, top + ty (bot - top), rounded half to even (samples are below 2^16: the low bits of the sum)
__device__ __forceinline__ unsigned pb_vbil_mix(const unsigned a, const unsigned b, const unsigned c, const unsigned d, const float tx, const float ty) {
    const float fa = (float)a, fc = (float)c;
    const float top = fmaf(tx, (float)b - fa, fa), bot = fmaf(tx, (float)d - fc, fc);
    return __float_as_uint(fmaf(ty, bot - top, top) + 12582912.0f) & 0xFFFFu;
}

// One output pixel from its tap base (i0, j0) and fractions (ty, tx) on plane 0: y = its plane-0 sample; anchor: uv = the two chroma
// samples of its block, U | V << 16.  dead: the fills.
template <int S, int SUB, bool PAIRS, bool WRAP>
__device__ __forceinline__ void pb_vbil_px(const uint8_t* __restrict__ s, const PbPlanar& L, const int h, const int w, int i0, int j0, const float ty,
                                           const float tx, const bool dead, const bool anchor, unsigned& y, unsigned& uv) {
    constexpr int CX = pb_planar_cx(SUB), CY = pb_planar_cy(SUB);
    if (dead) i0 = j0 = 0;
    unsigned r[2], c[2];
    pb_vbil_rc<WRAP>(i0, j0, h, w, r, c);
    const unsigned o0 = r[0] * L.src_pitch, o1 = r[1] * L.src_pitch;
    const unsigned a0 = pb_nv12_load_y<S>(s, o0 + c[0] * (unsigned)S), a1 = pb_nv12_load_y<S>(s, o0 + c[1] * (unsigned)S);
    const unsigned a2 = pb_nv12_load_y<S>(s, o1 + c[0] * (unsigned)S), a3 = pb_nv12_load_y<S>(s, o1 + c[1] * (unsigned)S);
    unsigned u[4], v[4];
    float tyc = ty, txc = tx;
    if (anchor) {
        // the anchor's coordinate in chroma sample units: s / 2 where subsampled
        if (CY) tyc = ((float)(i0 & 1) + ty) * 0.5f;
        if (CX) txc = ((float)(j0 & 1) + tx) * 0.5f;
        unsigned rc[2], cc[2];
        pb_vbil_rc<WRAP>(i0 >> CY, j0 >> CX, h >> CY, w >> CX, rc, cc);  // (arithmetic shifts: floor)
#pragma unroll
        for (int k = 0; k < 4; ++k) pb_video_load_c<S, PAIRS>(s, L, rc[k >> 1] * L.src_cpitch + cc[k & 1] * (unsigned)(PAIRS ? 2 * S : S), u[k], v[k]);
    }
    const unsigned vy = pb_vbil_mix(a0, a1, a2, a3, tx, ty);
    y = dead ? L.fill[0] : vy;
    if (anchor) {
        const unsigned vu = pb_vbil_mix(u[0], u[1], u[2], u[3], txc, tyc), vv = pb_vbil_mix(v[0], v[1], v[2], v[3], txc, tyc);
        uv = dead ? (L.fill[1] | (L.fill[2] << 16)) : (vu | (vv << 16));
    }
}
// (x, y) of a tile holds an anchor
template <int SUB>
__device__ __forceinline__ bool pb_vbil_anchor(const int x, const int y) {
    return !(((x & pb_planar_cx(SUB)) | (y & pb_planar_cy(SUB))) & 1);
}
// U | V << 16 as the pair lies in memory (U in the low S bytes)
template <int S>
__device__ __forceinline__ unsigned pb_vbil_pair(const unsigned uv) {
    return S == 1 ? ((uv & 0xFFu) | (uv >> 8)) : uv;
}

template <int SRC_KIND, int S, int SUB, bool PAIRS>
__global__ __launch_bounds__(64 * PB_VBIL_WAVES, PB_VBIL_WPE) void pb_planar_bilinear_kernel(const PbHot Hd, const PbTileEntry* __restrict__ table,
                                                                                           const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                                           const unsigned groups_per_frame, unsigned long long src_stride,
                                                                                           unsigned long long dst_stride, const PbBilCoord* __restrict__ bil_xy,
                                                                                           const int32_t* __restrict__ fix_px,
                                                                                           const PbBilCoord* __restrict__ fix_xy, const PbPlanar Ls) {
    static_assert(SUB == PB_SUB_444 || SUB == PB_SUB_422 || SUB == PB_SUB_420, "the subsamplings of pb_remap_planar_bilinear");
    static_assert(!PAIRS || SUB == PB_SUB_420, "interleaved pairs are NV12 / P010: 4:2:0");
    static_assert(SRC_KIND == PB_KIND_CAMERA || SRC_KIND == PB_KIND_PANO, "single sources with an interpolating tile kernel");
    constexpr int CX = pb_planar_cx(SUB), CY = pb_planar_cy(SUB);
    constexpr int NC = 4 >> CX;
    constexpr bool WRAP = SRC_KIND == PB_KIND_PANO;
    constexpr bool NT = PB_NT_DEFAULT(SRC_KIND);
    const PbPlanar L = pb_video_in_vgprs(Ls);  // (pb_video.hpp, "Scalar registers")
    __shared__ unsigned park[PB_VBIL_WAVES][2][PB_PX_PLANE];
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
    const unsigned vslot = (unsigned)__builtin_amdgcn_readfirstlane((int)pb_bil_slot_of<PB_VBIL_WAVES>(wg, (unsigned)wave));
    pb_load_entry(table + vslot, entry);
    const PbTileEntry* __restrict__ e = &entry;
    const int flags = e->flags;
    if (flags & PB_TILE_SKIP) return;
    const int X0 = (e->tile_xy & 0xFFFF) * PB_TILE, Y0 = (int)((unsigned)e->tile_xy >> 16) * PB_TILE;
    const int W = Hd.dst_w, H = Hd.dst_h, h = Hd.src_h, w = Hd.src_w;
    const int xg = lane & 7, yb = lane >> 3;
    const int x = X0 + 4 * xg;  // the lane's store shape: columns x .. x + 3 of rows Y0 + yb + 8 * jr (Y0 and 8 * jr are even: yb decides a row's parity)
    unsigned* p0 = park[wave][0];
    unsigned* p1 = park[wave][1];

    if (e->bil_off < 0 && !(flags & (PB_TILE_LEAN | PB_TILE_DIRECT))) {  // BLACK (every other class has a table slot)
        const unsigned z0[4] = {L.fill[0], L.fill[0], L.fill[0], L.fill[0]}, z1[4] = {L.fill[1], L.fill[1], L.fill[1], L.fill[1]},
                       z2[4] = {L.fill[2], L.fill[2], L.fill[2], L.fill[2]};
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            const int y = Y0 + yb + 8 * jr;
            pb_nv12_store_y<S, false>(dst, L.dst_pitch, W, H, x, y, z0);
            if (!CY || pb_nv12_even(yb)) pb_video_store_c<S, SUB, PAIRS>(dst, L, W, H, x, y, z1, z2);
        }
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
                const bool anchor = pb_vbil_anchor<SUB>(px, py);
                unsigned vy, vuv = 0u;
                pb_vbil_px<S, SUB, PAIRS, WRAP>(src, L, h, w, i0, j0, ty, tx, dead, anchor, vy, vuv);
                p0[py * 33 + px] = vy;
                if (anchor) p1[py * 33 + px] = vuv;
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
                const bool anchor = pb_vbil_anchor<SUB>(px, py);
                unsigned vy, vuv = 0u;
                pb_vbil_px<S, SUB, PAIRS, WRAP>(src, L, h, w, ar + (int)fy, ac + (int)fx, sv[m].x - fy, sv[m].y - fx, false, anchor, vy, vuv);
                p0[py * 33 + px] = vy;
                if (anchor) p1[py * 33 + px] = vuv;
            }
        }
    }
    if (e->bil_off >= 0 || (flags & (PB_TILE_LEAN | PB_TILE_DIRECT))) {  // (a black tile parked nothing)
        pb_wave_sync();
        // read back in the store shape and store: plane 0, then planes 1 and 2 at their anchors
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            unsigned a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = p0[(yb + 8 * jr) * 33 + 4 * xg + k];
            pb_nv12_store_y<S, NT>(dst, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, a);
        }
        if (!CY || pb_nv12_even(yb)) {
#pragma unroll
            for (int jr = 0; jr < 4; ++jr) {
                const int y = Y0 + yb + 8 * jr;
                unsigned c1[4], c2[4];
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    const unsigned uv = p1[(yb + 8 * jr) * 33 + 4 * xg + (j << CX)];
                    c1[j] = PAIRS ? pb_vbil_pair<S>(uv) : (uv & 0xFFFFu);
                    c2[j] = uv >> 16;
                }
                pb_video_store_stored<S, SUB, PAIRS, NT>(dst, L, W, H, x, y, c1, c2);  // (PAIRS: c1 holds the pairs)
            }
        }
    }
    // this tile's fix pixels (where the model's coordinate is not certified): redone from their exact coordinates after the wave's own
    // stores have completed; an anchor among them redoes its two chroma samples
    const int n_fix = e->fix_cnt;
    if (n_fix > 0 && e->bil_off < 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane < n_fix) {
            const unsigned p = (unsigned)fix_px[e->fix_off + lane];
            const PbBilCoord q = fix_xy[e->fix_off + lane];
            unsigned y, xx;
            pb_nv12_divmod(p, (unsigned)W, __builtin_amdgcn_rcpf((float)W), y, xx);
            int i0, j0;
            float fty, ftx;
            bool dead;
            pb_cr_of_q(q.y, q.x, i0, j0, fty, ftx, dead);
            const bool anchor = pb_vbil_anchor<SUB>((int)xx, (int)y);
            unsigned vy, vuv = 0u;
            pb_vbil_px<S, SUB, PAIRS, WRAP>(src, L, h, w, i0, j0, fty, ftx, dead, anchor, vy, vuv);
            pb_nv12_store_y1<S>(dst + (y * L.dst_pitch + xx * (unsigned)S), vy);
            if (anchor) pb_video_store_c1<S, SUB, PAIRS>(dst, L, y, xx, vuv & 0xFFFFu, vuv >> 16);
        }
    }
}

// Diagnostic (pb_plan_video_bilinear_mix): what pb_planar_bilinear_kernel's fix-pixel path meets in a plan, over the bilinear mode's
// launch-order table.  counters[0] = model tiles with fix pixels, [1] = their fix pixels, [2] = of those the anchors at 4:2:2 (an even
// column), [3] = the anchors at 4:2:0 (an even row too).  At 4:4:4 every fix pixel is an anchor.
__global__ void pb_video_bilinear_mix_kernel(const PbTileEntry* __restrict__ ltable, unsigned n_slots, const int32_t* __restrict__ fix_px, int W,
                                             unsigned* __restrict__ counters) {
    const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_slots) return;
    const PbTileEntry& e = ltable[v];
    if ((e.flags & PB_TILE_SKIP) || e.bil_off >= 0 || e.fix_cnt <= 0 || !(e.flags & (PB_TILE_LEAN | PB_TILE_DIRECT))) return;
    unsigned a422 = 0, a420 = 0;
    for (int k = 0; k < e.fix_cnt; ++k) {
        const int p = fix_px[e.fix_off + k], y = p / W, x = p - y * W;
        a422 += !(x & 1);
        a420 += !((x | y) & 1);
    }
    atomicAdd(&counters[0], 1u);
    atomicAdd(&counters[1], (unsigned)e.fix_cnt);
    atomicAdd(&counters[2], a422);
    atomicAdd(&counters[3], a420);
}
