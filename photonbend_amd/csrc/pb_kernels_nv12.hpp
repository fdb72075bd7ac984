// pb_kernels_nv12.hpp - the nearest tile kernel for 4:2:0 semi-planar video frames: NV12 and P010 / P016 (pb_remap_nv12).
//
// A frame is a full-resolution plane of luma samples followed, at uv_offset, by a half-resolution plane of interleaved (U, V) pairs;
// rows of both planes are `pitch` bytes apart.  S = 1 (NV12) or 2 (P010 / P016) bytes per sample.  All four dimensions are even.
//   luma     Y_out[y][x] = Y_src[r][c], (r, c) the plan's certified source pixel of (y, x); fill_y where that pixel is black.
//   chroma   the pair of output block (i, j) is UV_src[r >> 1][c >> 1] with (r, c) the source pixel of the block's ANCHOR, its top-left
//            pixel (2i, 2j); (fill_u, fill_v) where the anchor is black.  Only the anchor decides.  A nearest sample, no interpolation.
// So the tile models, certification, the exact-index tables, the fix lists and the launch-order table are those of the RGB8 plan,
// unchanged, as for pb_px_hot_kernel; this file adds the kernel that writes BOTH planes of a tile in one launch.  The 32 x 32 tile is
// even-aligned: a chroma block never straddles tiles, and a tile owns 16 x 16 pairs.
//
// pb_nv12_hot_kernel<SRC_KIND, S> has pb_px_hot_kernel's launch shape: one wave per slot of the plan's nearest launch-order table, the
// entry in SGPRs (pb_load_entry), frames of a batch as a grid dimension, the parameter block behind a pointer, PbHot by value, static LDS.
//   BLACK           fills.
//   LEAN / DIRECT   pb_px_hot_kernel's direct-gather path in the two certified evaluation orders, `dead` bits for MASKED.  Before the
//   / MASKED        regrouping a lane holds 16 pixels of one line: p = lane & 31 is fixed and q = (2n + hh + shift) & 31 has a parity
//                   that does not depend on n, so 16 of the 64 lanes hold nothing but anchors and the other 48 hold none.  THOSE 16
//                   LANES GATHER THE PAIRS, next to their luma gathers, and the pairs go through the regrouping plane in a second pass.
//                   (The other way - the anchors' offsets through the plane, the pairs gathered in the store shape - spreads the
//                   gathers over 32 lanes but puts a second memory round trip behind the LDS pass; here every gather of a tile is in
//                   flight at once, which is what a gather-bound tile kernel wants.)
//   generic         pb_model_row / pb_model_px_rc; row and column stay apart (rows are pitched).  The lane is in the store shape:
//                   lanes with even yb hold the anchors at k = 0, 2 of their four rows.  Every lane loads those two pairs (no load
//                   inside a branch), the lanes of even rows store them.
//   FAILED          the plan's exact indices (idx_tab); a stored index r * w + c is taken apart by pb_nv12_divmod (few pixels).
//   fix pixels      re-copied through fix_px / fix_idx after the wave's own stores have completed; a fix pixel on an even row and even
//                   column is an anchor and re-copies its pair too.
//
// Movement.  Pointers, pitches, offsets and strides are multiples of one pair, 2 * S bytes (pb_remap_nv12 checks).  A luma sample is
// loaded with exactly its S bytes and a pair with exactly its 2 * S, so no load touches a byte outside its plane - the last pair of
// the source included.  Four luma samples, or two adjacent pairs, leave in one 4 * S-byte store where their address is 4-byte aligned,
// else luma sample by sample and chroma pair by pair (a pair's address is always pair-aligned); stores are clipped to the image.
//
// Scalar registers.  The tile entry takes 64 of the 102 and must stay there (tests/test_isa_nv12.py).  What this kernel adds is kept
// out of them: the layouts and fills live in vector registers, and the fills of black pixels in the failed and generic paths are
// applied AFTER the loads, from values the compiler cannot trace back (asm volatile("" : "+v"(x))) - as lane masks kept alive across
// sixteen loads they pushed a quarter of the entry into vector lanes.
//
// Limits.  Byte offsets inside a frame are 32-bit: pb_remap_nv12 refuses frames whose span (uv_offset + pitch * height / 2) reaches
// 2^31 bytes with PB_ERR_UNSUPPORTED before any launch, and sources of 32768 px a side or more like pb_remap_px.  LDS: the regrouping
// buffer only, 4224 bytes per wave.
#pragma once
#include "pb_kernels_px.hpp"

// the layouts and fills of one launch, in bytes and in stored form: fill_uv is the pair as it lies in memory (U in the low S bytes)
struct PbNv12 {
    unsigned src_pitch, src_uv, dst_pitch, dst_uv;
    unsigned fill_y, fill_uv;
};

template <int S>
__device__ __forceinline__ unsigned pb_nv12_load_y(const uint8_t* __restrict__ s, unsigned off) {
    static_assert(S == 1 || S == 2, "sample sizes of pb_remap_nv12");
    if constexpr (S == 1) return s[off];
    else return *reinterpret_cast<const uint16_t*>(s + off);
}
template <int S>
__device__ __forceinline__ unsigned pb_nv12_load_uv(const uint8_t* __restrict__ s, unsigned off) {
    if constexpr (S == 1) return *reinterpret_cast<const uint16_t*>(s + off);
    else return *reinterpret_cast<const unsigned*>(s + off);
}
// the luma sample / the pair of source pixel (r, c), or the fill.  Branch-free, so that a lane's gathers are in flight together: a
// black pixel reads the plane's first sample / pair
template <int S>
__device__ __forceinline__ unsigned pb_nv12_y_rc(const uint8_t* __restrict__ s, const PbNv12& L, int r, int c, bool black) {
    const unsigned v = pb_nv12_load_y<S>(s, black ? 0u : (unsigned)r * L.src_pitch + (unsigned)c * (unsigned)S);
    return black ? L.fill_y : v;
}
template <int S>
__device__ __forceinline__ unsigned pb_nv12_uv_rc(const uint8_t* __restrict__ s, const PbNv12& L, int r, int c, bool black) {
    const unsigned v = pb_nv12_load_uv<S>(s, L.src_uv + (black ? 0u : ((unsigned)r >> 1) * L.src_pitch + ((unsigned)c & ~1u) * (unsigned)S));
    return black ? L.fill_uv : v;
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
// the lane's four luma samples of output row y, columns x .. x + 3 (d: the luma plane)
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
// the lane's two adjacent pairs of the blocks anchored at (y, x) and (y, x + 2), y and x even (d: the chroma plane).  W is even: a
// block is inside the image or outside it
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

template <int SRC_KIND, int S>
__global__ __launch_bounds__(64 * PB_TILE_WAVES) void pb_nv12_hot_kernel(const PbParams* __restrict__ Pp, const PbHot Hd, const PbTileEntry* __restrict__ table,
                                                                          const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                          const unsigned groups_per_frame, unsigned long long src_stride,
                                                                          unsigned long long dst_stride, const int32_t* __restrict__ idx_tab,
                                                                          const int32_t* __restrict__ fix_px, const int32_t* __restrict__ fix_idx, const PbNv12 Ls) {
    // the layouts and fills live in VECTOR registers: the tile entry takes 64 scalar registers, and six more live values beside the
    // exec masks of the plane and alignment branches would push it out of them
    PbNv12 L;
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.src_pitch) : "s"(Ls.src_pitch));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.src_uv) : "s"(Ls.src_uv));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.dst_pitch) : "s"(Ls.dst_pitch));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.dst_uv) : "s"(Ls.dst_uv));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.fill_y) : "s"(Ls.fill_y));
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.fill_uv) : "s"(Ls.fill_uv));
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
    const int x = X0 + 4 * xg;  // the lane's store shape: columns x .. x + 3 of rows Y0 + yb + 8 * jr; yb even: pixels k = 0, 2 are anchors
    uint8_t* __restrict__ duv = dst + L.dst_uv;

    if (flags & PB_TILE_FAILED) {
        const int32_t* __restrict__ slot = idx_tab + (size_t)e->aux_off * (PB_TILE * PB_TILE);
        unsigned a[4][4], uv[4][2], black = 0u;
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            const int4 v = *reinterpret_cast<const int4*>(slot + (yb + 8 * jr) * PB_TILE + 4 * xg);
            const int id[4] = {v.x, v.y, v.z, v.w};
            const bool row_in = Y0 + yb + 8 * jr < H;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // (black or outside the image: a bit per pixel, for the fills after the loads - see "Scalar registers" above)
                const int idk = (row_in && x + k < W) ? id[k] : -1;
                black |= (unsigned)(idk < 0) << (4 * jr + k);
                unsigned r, c;
                pb_nv12_divmod((unsigned)(idk < 0 ? 0 : idk), sw, inv_sw, r, c);
                a[jr][k] = pb_nv12_load_y<S>(src, r * L.src_pitch + c * (unsigned)S);
                if (!(k & 1))  // (every lane loads - no load inside a branch, they are all in flight together; the lanes of even rows store)
                    uv[jr][k >> 1] = pb_nv12_load_uv<S>(src, L.src_uv + (r >> 1) * L.src_pitch + (c & ~1u) * (unsigned)S);
            }
        }
        asm volatile("" : "+v"(black));
#pragma unroll
        for (int jr = 0; jr < 4; ++jr)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a[jr][k] = ((black >> (4 * jr + k)) & 1u) ? L.fill_y : a[jr][k];
                if (!(k & 1)) uv[jr][k >> 1] = ((black >> (4 * jr + k)) & 1u) ? L.fill_uv : uv[jr][k >> 1];
            }
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            pb_nv12_store_y<S, true>(dst, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, a[jr]);
            if (pb_nv12_even(yb)) pb_nv12_store_uv<S, true>(duv, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, uv[jr]);
        }
        return;  // (a failed tile has no fix pixels: its table slot holds them all)
    }
    if (flags & PB_TILE_BLACK) {
        const unsigned z[4] = {L.fill_y, L.fill_y, L.fill_y, L.fill_y}, zuv[2] = {L.fill_uv, L.fill_uv};
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            pb_nv12_store_y<S, false>(dst, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, z);
            if (pb_nv12_even(yb)) pb_nv12_store_uv<S, false>(duv, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, zuv);
        }
    } else if (flags & (PB_TILE_LEAN | PB_TILE_DIRECT)) {
        // pb_px_hot_kernel's direct-gather path (its comments and pb_win_tile's hold here): every pixel of such a tile lies inside the
        // image and samples inside the tile's source box, in both evaluation orders (pb_certify_kernel)
        unsigned* win = lds[wave];
        const unsigned pitch = L.src_pitch;
        const int ar = e->anchor_r, ac = e->anchor_c;
        const bool along_x = fabsf(e->c[1][0]) <= fabsf(e->c[5][0]);  // |d row / du| <= |d row / dv|
        const int p = lane & 31, hh = lane >> 5;
        const float num = along_x ? e->c[1][0] : e->c[5][0], den = along_x ? e->c[5][0] : e->c[1][0];
        const float slope = (den != 0.0f) ? -num / den : 0.0f;
        const int shift = (int)rintf(slope * ((float)p - 15.5f));
        const bool anchors = !((p | (hh + shift)) & 1);  // this lane's 16 pixels are all anchors (else none is)
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
        unsigned t[16], tuv[16];
        if (flags & PB_TILE_MASKED) {
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                t[n] = L.fill_y;
                tuv[n] = L.fill_uv;
                if (!((dead >> n) & 1u)) {  // (a dead pixel's address is not a certified one: no load)
                    t[n] = pb_nv12_load_y<S>(src, (rc[n] >> 16) * pitch + (rc[n] & 0xFFFFu) * (unsigned)S);
                    if (anchors) tuv[n] = pb_nv12_load_uv<S>(src, L.src_uv + (rc[n] >> 17) * pitch + (rc[n] & 0xFFFEu) * (unsigned)S);
                }
            }
        } else {
#pragma unroll
            for (int n = 0; n < 16; ++n) t[n] = pb_nv12_load_y<S>(src, (rc[n] >> 16) * pitch + (rc[n] & 0xFFFFu) * (unsigned)S);
            if (anchors) {
#pragma unroll
                for (int n = 0; n < 16; ++n) tuv[n] = pb_nv12_load_uv<S>(src, L.src_uv + (rc[n] >> 17) * pitch + (rc[n] & 0xFFFEu) * (unsigned)S);
            }
        }
        // park as [y][x], read back in the store shape: the luma plane, then - through the same buffer - the pairs at their anchors
        unsigned a[4][4], uv[4][2];
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            const int q = (2 * n + hh + shift) & 31;
            win[along_x ? q * 33 + p : p * 33 + q] = t[n];
        }
        pb_wave_sync();
#pragma unroll
        for (int jr = 0; jr < 4; ++jr)
#pragma unroll
            for (int k = 0; k < 4; ++k) a[jr][k] = win[(yb + 8 * jr) * 33 + 4 * xg + k];
        pb_wave_sync();  // (the plane's previous contents have been read)
        if (anchors) {
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                const int q = (2 * n + hh + shift) & 31;
                win[along_x ? q * 33 + p : p * 33 + q] = tuv[n];
            }
        }
        pb_wave_sync();
        if (pb_nv12_even(yb)) {
#pragma unroll
            for (int jr = 0; jr < 4; ++jr)
#pragma unroll
                for (int k = 0; k < 2; ++k) uv[jr][k] = win[(yb + 8 * jr) * 33 + 4 * xg + 2 * k];
        }
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            pb_nv12_store_y<S, NT>(dst, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, a[jr]);
            if (pb_nv12_even(yb)) pb_nv12_store_uv<S, NT>(duv, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, uv[jr]);
        }
    } else {
        // generic tile: validity, wrap and truncation edge per pixel; a packed (row << 16 | column), or -1 = black
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            PbRowModel R;
            pb_model_row(P, e, X0, Y0, yb + 8 * jr, 4 * xg, R);
            unsigned a[4], uv[2];
            int v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = pb_model_px_rc<SRC_KIND>(P, R, 4 * xg, k);
                const unsigned r = (unsigned)v[k] >> 16, c = (unsigned)v[k] & 0xFFFFu;
                a[k] = pb_nv12_load_y<S>(src, v[k] < 0 ? 0u : r * L.src_pitch + c * (unsigned)S);
                if (!(k & 1))  // (every lane loads, the lanes of even rows store)
                    uv[k >> 1] = pb_nv12_load_uv<S>(src, L.src_uv + (v[k] < 0 ? 0u : (r >> 1) * L.src_pitch + (c & ~1u) * (unsigned)S));
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // (the fills after the loads, from values the compiler cannot trace: "Scalar registers" above)
                asm volatile("" : "+v"(v[k]));
                a[k] = v[k] < 0 ? L.fill_y : a[k];
                if (!(k & 1)) uv[k >> 1] = v[k] < 0 ? L.fill_uv : uv[k >> 1];
            }
            pb_nv12_store_y<S, NT>(dst, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, a);
            if (pb_nv12_even(yb)) pb_nv12_store_uv<S, NT>(duv, L.dst_pitch, W, H, x, Y0 + yb + 8 * jr, uv);
        }
    }
    // this tile's fix pixels (where the model's truncation differs from the faithful one): re-copied through their exact indices
    // after the wave's own stores have completed; an anchor among them re-copies its pair
    const int n_fix = e->fix_cnt;
    if (n_fix > 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane < n_fix) {
            const unsigned p = (unsigned)fix_px[e->fix_off + lane];
            const int id = fix_idx[e->fix_off + lane];
            unsigned y, xx, r, c;
            pb_nv12_divmod(p, (unsigned)W, __builtin_amdgcn_rcpf((float)W), y, xx);
            pb_nv12_divmod((unsigned)(id < 0 ? 0 : id), sw, inv_sw, r, c);
            pb_nv12_store_y1<S>(dst + (y * L.dst_pitch + xx * (unsigned)S), pb_nv12_y_rc<S>(src, L, (int)r, (int)c, id < 0));
            if (!((y | xx) & 1u))
                pb_nv12_store_uv1<S>(duv + ((y >> 1) * L.dst_pitch + xx * (unsigned)S), pb_nv12_uv_rc<S>(src, L, (int)r, (int)c, id < 0));
        }
    }
}
