// pb_video.hpp - THE FRAME MODEL OF THE VIDEO KERNELS: what every kernel that moves video frames knows about a frame.
//
// A frame is plane 0 - full resolution, (h, w), S-byte samples, rows `pitch` bytes apart - plus two chroma planes of (h >> CY, w >> CX)
// samples each, (CX, CY) = (0, 0) at 4:4:4, (1, 0) at 4:2:2, (1, 1) at 4:2:0, rows `cpitch` bytes apart.  The planes start at byte offsets
// 0, o1, o2 of the frame, in any order.  Widths are multiples of 1 << CX and heights of 1 << CY, source and destination alike.
//   PAIRS   NV12 and P010 / P016 store the two chroma planes as ONE plane of interleaved (U, V) pairs, at 4:2:0: o1 is the pair plane's
//           offset, cpitch its pitch (the luma pitch), o2 is unused; a pair is 2 * S bytes, U in the low S.  A kernel template takes the
//           form as `bool PAIRS` beside the subsampling; everything else of the frame model is the same.
// A chroma sample (or pair) belongs to its ANCHOR, the top-left pixel (i << CY, j << CX) of its block: whatever a kernel computes for the
// anchor's plane-0 sample - a source pixel, taps and factors - serves the block's chroma.  Only the anchor decides.
//
// Movement.  Pointers, pitches, offsets and strides are multiples of S (PAIRS: of 2 * S) and nothing more (the calls check).  A sample is
// loaded with exactly its S bytes and a pair with exactly its 2 * S, so no load touches a byte outside its plane - the last sample or
// pair of the source included.  A lane's four plane-0 samples of a row - at 4:4:4 its four samples of a chroma plane too, with PAIRS its
// two adjacent pairs - leave in one 4 * S-byte store where the address is 4-byte aligned, its two chroma samples at 4:2:2 / 4:2:0 in one
// 2 * S-byte store where the address is 2 * S-byte aligned; else sample by sample or pair by pair (a pair's address is always
// pair-aligned).  Stores are clipped to their plane.  Padding between rows, planes and frames is neither read nor written.
//
// Scalar registers.  A tile kernel's entry takes 64 of the 102 and must stay there (tests/test_isa_nv12.py).  What a video tile kernel
// adds is kept out of them: the layouts and fills live in vector registers (pb_video_in_vgprs), and the fills of black pixels in the
// failed and generic paths are applied AFTER the loads, from values the compiler cannot trace back (asm volatile("" : "+v"(x))) - as
// lane masks kept alive across sixteen loads they pushed a quarter of the entry into vector lanes.  pb_nv12_even is asked anew at each
// use for the same reason.
//
// Limits.  Byte offsets inside a frame are 32-bit: the calls refuse frames whose span reaches 2^31 bytes with PB_ERR_UNSUPPORTED before
// any launch, and sources of 32768 px a side or more like pb_remap_px.
#pragma once
#include "pb_kernels_px.hpp"

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
// ... in VECTOR registers: the tile entry takes 64 scalar registers, and eleven more live values beside the exec masks of the plane and
// alignment branches would push it out of them ("Scalar registers" above)
__device__ __forceinline__ PbPlanar pb_video_in_vgprs(const PbPlanar& Ls) {
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
    return L;
}

template <int S>
__device__ __forceinline__ unsigned pb_nv12_load_y(const uint8_t* __restrict__ s, unsigned off) {
    static_assert(S == 1 || S == 2, "sample sizes of the video calls");
    if constexpr (S == 1) return s[off];
    else return *reinterpret_cast<const uint16_t*>(s + off);
}
template <int S>
__device__ __forceinline__ unsigned pb_nv12_load_uv(const uint8_t* __restrict__ s, unsigned off) {
    if constexpr (S == 1) return *reinterpret_cast<const uint16_t*>(s + off);
    else return *reinterpret_cast<const unsigned*>(s + off);
}

// (r, c) = divmod(id, w) for a stored source or destination index, inv_w = 1 / w to a few ulp.  What it needs is a QUOTIENT below 2^22
// - a row number: below 2^15 for a source, 2^14 for a destination, whatever the width - and id < 2^31: the float quotient's relative
// error is below 2^-22, so it is within one of the true one, and it is corrected by arithmetic on the remainder's sign - no comparison,
// so no lane mask: the failed path runs sixteen of these side by side.
__device__ __forceinline__ void pb_nv12_divmod(unsigned id, unsigned w, float inv_w, unsigned& r, unsigned& c) {
    int q = (int)((float)id * inv_w);
    int rem = (int)id - q * (int)w;
    const int neg = rem >> 31;  // -1: the quotient was one too large
    q += neg;
    rem += (int)w & neg;
    const int over = ((int)w - 1 - rem) >> 31;  // -1: one too small
    q -= over;
    rem -= (int)w & over;
    r = (unsigned)q;
    c = (unsigned)rem;
}

// v is even - asked anew at every use: a lane mask kept for the whole kernel costs the scalar registers the tile entry needs
__device__ __forceinline__ bool pb_nv12_even(int v) {
    int b = v & 1;
    asm volatile("" : "+v"(b));
    return b == 0;
}

template <int S>
__device__ __forceinline__ void pb_nv12_store_y1(uint8_t* p, unsigned v) {
    if constexpr (S == 1) *p = (uint8_t)v;
    else *reinterpret_cast<uint16_t*>(p) = (uint16_t)v;
}
template <int S>
__device__ __forceinline__ void pb_nv12_store_uv1(uint8_t* p, unsigned v) {
    if constexpr (S == 1) *reinterpret_cast<uint16_t*>(p) = (uint16_t)v;
    else *reinterpret_cast<unsigned*>(p) = v;
}
// the lane's four samples of output row y, columns x .. x + 3, of a full-resolution plane d
template <int S, bool NT>
__device__ __forceinline__ void pb_nv12_store_y(uint8_t* __restrict__ d, const unsigned pitch, const int W, const int H, const int x, const int y,
                                                const unsigned a[4]) {
    if (y >= H) return;
    uint8_t* p = d + ((unsigned)y * pitch + (unsigned)x * (unsigned)S);
    if (x + 3 < W && ((uintptr_t)p & 3u) == 0) {
        if constexpr (S == 1) {
            pb_px_store_vec<NT>(a[0] | (a[1] << 8) | (a[2] << 16) | (a[3] << 24), p);
        } else {
            const pb_px_u32x2 o = {a[0] | (a[1] << 16), a[2] | (a[3] << 16)};
            pb_px_store_vec<NT>(o, p);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x + k < W) pb_nv12_store_y1<S>(p + S * k, a[k]);
    }
}
// the lane's two adjacent pairs of the blocks anchored at (y, x) and (y, x + 2), y and x even (d: the pair plane).  W is even: a block
// is inside the image or outside it
template <int S, bool NT>
__device__ __forceinline__ void pb_nv12_store_uv(uint8_t* __restrict__ d, const unsigned pitch, const int W, const int H, const int x, const int y,
                                                 const unsigned uv[2]) {
    if (y >= H) return;
    uint8_t* p = d + (((unsigned)y >> 1) * pitch + (unsigned)x * (unsigned)S);  // (pair x / 2 is 2 * S bytes wide)
    if (x + 3 < W && ((uintptr_t)p & 3u) == 0) {
        if constexpr (S == 1) {
            pb_px_store_vec<NT>(uv[0] | (uv[1] << 16), p);
        } else {
            const pb_px_u32x2 o = {uv[0], uv[1]};
            pb_px_store_vec<NT>(o, p);
        }
    } else {
        if (x < W) pb_nv12_store_uv1<S>(p, uv[0]);
        if (x + 2 < W) pb_nv12_store_uv1<S>(p + 2 * S, uv[1]);
    }
}
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

// ---- either form of the chroma: two planes of samples, or (PAIRS) one plane of pairs
// the byte offset of the chroma sample (PAIRS: the pair) of source pixel (r, c) inside its plane
template <int S, int SUB, bool PAIRS>
__device__ __forceinline__ unsigned pb_video_coff(const unsigned cpitch, const unsigned r, const unsigned c) {
    return (r >> pb_planar_cy(SUB)) * cpitch + (c >> pb_planar_cx(SUB)) * (unsigned)(PAIRS ? 2 * S : S);
}
// the chroma at byte offset `off` of its plane AS STORED: c1 and c2 the two samples, or (PAIRS: one load) c1 the pair and c2 untouched
template <int S, bool PAIRS>
__device__ __forceinline__ void pb_video_load_stored(const uint8_t* __restrict__ s, const PbPlanar& L, const unsigned off, unsigned& c1, unsigned& c2) {
    if constexpr (PAIRS) {
        c1 = pb_nv12_load_uv<S>(s, L.src_o1 + off);
    } else {
        c1 = pb_nv12_load_y<S>(s, L.src_o1 + off);
        c2 = pb_nv12_load_y<S>(s, L.src_o2 + off);
    }
}
// ... as its two samples (PAIRS: the pair taken apart)
template <int S, bool PAIRS>
__device__ __forceinline__ void pb_video_load_c(const uint8_t* __restrict__ s, const PbPlanar& L, const unsigned off, unsigned& c1, unsigned& c2) {
    if constexpr (PAIRS) {
        const unsigned v = pb_nv12_load_uv<S>(s, L.src_o1 + off);
        c1 = v & (S == 1 ? 0xFFu : 0xFFFFu);
        c2 = v >> (8 * S);
    } else {
        pb_video_load_stored<S, false>(s, L, off, c1, c2);
    }
}
// the lane's chroma of output row y, columns x .. x + 3, AS STORED: c1[j] and c2[j] the samples at pixels j << CX, or (PAIRS) c1[0 .. 1]
// the two pairs.  The caller has established that row y holds anchors
template <int S, int SUB, bool PAIRS, bool NT>
__device__ __forceinline__ void pb_video_store_stored(uint8_t* __restrict__ d, const PbPlanar& L, const int W, const int H, const int x, const int y,
                                                      const unsigned c1[4], const unsigned c2[4]) {
    if constexpr (PAIRS) {
        pb_nv12_store_uv<S, NT>(d + L.dst_o1, L.dst_cpitch, W, H, x, y, c1);
    } else {
        pb_planar_store_c<S, SUB, NT>(d + L.dst_o1, L.dst_cpitch, W, H, x, y, c1);
        pb_planar_store_c<S, SUB, NT>(d + L.dst_o2, L.dst_cpitch, W, H, x, y, c2);
    }
}
// ... from its samples c1[j], c2[j] (PAIRS: put together)
template <int S, int SUB, bool PAIRS>
__device__ __forceinline__ void pb_video_store_c(uint8_t* __restrict__ d, const PbPlanar& L, const int W, const int H, const int x, const int y, const unsigned c1[4],
                                                 const unsigned c2[4]) {
    if constexpr (PAIRS) {
        const unsigned uv[2] = {c1[0] | (c2[0] << (8 * S)), c1[1] | (c2[1] << (8 * S))};
        pb_video_store_stored<S, SUB, true, false>(d, L, W, H, x, y, uv, uv);
    } else {
        pb_video_store_stored<S, SUB, false, false>(d, L, W, H, x, y, c1, c2);
    }
}
// one chroma sample pair of the destination, at the block of the anchor pixel (y, x)
template <int S, int SUB, bool PAIRS>
__device__ __forceinline__ void pb_video_store_c1(uint8_t* __restrict__ d, const PbPlanar& L, const unsigned y, const unsigned x, const unsigned c1, const unsigned c2) {
    const unsigned off = (y >> pb_planar_cy(SUB)) * L.dst_cpitch + (x >> pb_planar_cx(SUB)) * (unsigned)(PAIRS ? 2 * S : S);
    if constexpr (PAIRS) {
        pb_nv12_store_uv1<S>(d + (L.dst_o1 + off), c1 | (c2 << (8 * S)));
    } else {
        pb_nv12_store_y1<S>(d + (L.dst_o1 + off), c1);
        pb_nv12_store_y1<S>(d + (L.dst_o2 + off), c2);
    }
}
