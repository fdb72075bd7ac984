// Supersampled remapping: output pixel (i, j) is the round-half-to-even mean of the n x n block
// S[n i : n i + n, n j : n j + n] of the remap S of the n x destination (image n H x n W, camera magnitude n x), n in {2, 4}.
//
//   pb_box_reduce_kernel  the generic path: (F, n H, n W, C) samples of 1 or 2 bytes -> (F, H, W, C); what every remap the fused
//                         kernel does not take (double-fisheye sources, bilinear mode, grey / RGBA / 16-bit images, materialised maps,
//                         deferred plans, PB_MODE_FAITHFUL / PB_MODE_FAST_DIRECT, frames that are not 16-byte aligned) writes to a
//                         workspace first.
//   pb_ss_win_kernel      the fused path: the n x plan's tiles exactly as pb_hot_win_kernel runs them (same models, windows, exact
//                         tables, failed-tile lookups: the same subsample bytes), but each wave reduces its 32 x 32 tile's n x n blocks
//                         in registers and stores only the H x W output - never the n^2 intermediate.
//
// Rounding, in integers (N = n^2, k = log2 N):  q = sum >> k, r = sum & (N - 1), out = q + (r > N/2 || (r == N/2 && (q & 1))).
#pragma once

#include <type_traits>

template <int K>
__device__ __forceinline__ unsigned pb_ss_round(unsigned sum) {
    constexpr unsigned N = 1u << K, HALF = N >> 1;
    const unsigned q = sum >> K, r = sum & (N - 1u);
    return q + ((r > HALF || (r == HALF && (q & 1u))) ? 1u : 0u);
}

// ---- generic path --------------------------------------------------------------------------------------------------------------
// One thread per output pixel: n rows of n * channels consecutive samples (neighbouring threads read neighbouring pieces of the same
// rows), integer sums, whole output pixel written by its thread.
template <int NS, int SB>
__global__ __launch_bounds__(256) void pb_box_reduce_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const unsigned W,
                                                            const int channels, const unsigned long long n_px) {
    typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type T;
    constexpr int K = NS == 2 ? 2 : 4;
    const T* __restrict__ s = reinterpret_cast<const T*>(src);
    T* __restrict__ d = reinterpret_cast<T*>(dst);
    const unsigned long long row_len = (unsigned long long)NS * W * channels;  // samples per n x row
    for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < n_px; t += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long fi = t / W;  // frame * H + output row
        const unsigned j = (unsigned)(t - fi * W);
        const T* __restrict__ b = s + fi * NS * row_len + (unsigned long long)NS * j * channels;
        T* __restrict__ o = d + t * channels;
        for (int c = 0; c < channels; ++c) {
            unsigned sum = 0;
#pragma unroll
            for (int r = 0; r < NS; ++r)
#pragma unroll
                for (int q = 0; q < NS; ++q) sum += b[r * row_len + q * channels + c];
            o[c] = (T)pb_ss_round<K>(sum);
        }
    }
}

// ---- fused path ----------------------------------------------------------------------------------------------------------------
// The subsample values of one tile of the n x plan, in pb_win_tile's lane layout: a[jr][k] = the RGB bytes (low 24 bits) of pixel
// (X0 + 4 xg + k, Y0 + yb + 8 jr), xg = lane & 7, yb = lane >> 3.  The four tile classes compute exactly what pb_win_tile stores (its
// code, one frame, the stores replaced by registers); pixels outside the n x image hold anything - their whole blocks lie outside too.
template <int SRC_KIND>
__device__ __forceinline__ void pb_ss_tile_vals(const PbParams& P, const PbHot& Hd, const PbTileEntry* __restrict__ e, const int flags,
                                                const int tx, const int ty, const int lane, unsigned* win, const uint8_t* __restrict__ src,
                                                unsigned (&a)[4][4]) {
    const int X0 = tx * PB_TILE, Y0 = ty * PB_TILE;
    const unsigned rowbytes = 3u * (unsigned)Hd.src_w;
    const unsigned frame_bytes = rowbytes * (unsigned)Hd.src_h;
    const unsigned safe_len = frame_bytes & ~15u;
    const int xg = lane & 7, yb = lane >> 3;
    if (flags & PB_TILE_BLACK) {
#pragma unroll
        for (int jr = 0; jr < 4; ++jr)
#pragma unroll
            for (int k = 0; k < 4; ++k) a[jr][k] = 0u;
        return;
    }
    if (flags & PB_TILE_DIRECT) {
        const unsigned gbase = (unsigned)e->anchor_r * rowbytes + 3u * (unsigned)e->anchor_c;
        const bool along_x = fabsf(e->c[1][0]) <= fabsf(e->c[5][0]);
        const int p = lane & 31, hh = lane >> 5;
        const float num = along_x ? e->c[1][0] : e->c[5][0], den = along_x ? e->c[5][0] : e->c[1][0];
        const float slope = (den != 0.0f) ? -num / den : 0.0f;
        const int shift = (int)rintf(slope * ((float)p - 15.5f));
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
                go[n] = gbase + (unsigned)(int)fv.x * rowbytes + __umul24((unsigned)(int)fv.y, 3u);
            }
        } else {
            pb_f2 b[5];
            pb_collapse_row(e, p, b);
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                const pb_f2 fv = pb_eval_row(b, pb_tile_coord((2 * n + hh + shift) & 31));
                go[n] = gbase + (unsigned)(int)fv.x * rowbytes + __umul24((unsigned)(int)fv.y, 3u);
            }
        }
        unsigned t[16];
        if (flags & PB_TILE_MASKED) {
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                t[n] = 0u;
                if (!((dead >> n) & 1u)) __builtin_memcpy(&t[n], src + go[n], 4);
            }
        } else {
#pragma unroll
            for (int n = 0; n < 16; ++n) __builtin_memcpy(&t[n], src + go[n], 4);
        }
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            const int q = (2 * n + hh + shift) & 31;
            win[along_x ? q * 33 + p : p * 33 + q] = t[n];
        }
        pb_wave_sync();
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            const unsigned* r = win + (yb + 8 * jr) * 33 + 4 * xg;
#pragma unroll
            for (int k = 0; k < 4; ++k) a[jr][k] = r[k];
        }
        return;
    }
    if (flags & PB_TILE_LEAN) {
        const int nrows = e->win_rows, n16 = e->win_n16;
        const unsigned a0 = (unsigned)e->win_a0, pitch = 16u * (unsigned)n16;
        const unsigned gbase = (unsigned)e->anchor_r * rowbytes + 3u * (unsigned)e->anchor_c;
        float u[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = pb_tile_coord(4 * xg + k);
        unsigned la[4][4];
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
            pb_f2 b[5];
            pb_collapse_row(e, yb + 8 * jr, b);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const pb_f2 fv = pb_eval_row(b, u[k]);
                const unsigned dr = (unsigned)(int)fv.x, dc = (unsigned)(int)fv.y;
                la[jr][k] = __umul24(dr, pitch) + (__umul24(dc, 3u) + a0);
            }
        }
        asm volatile("" ::: "memory");
        pb_issue_window_loads(src, win, lane, gbase, rowbytes, nrows, n16, safe_len);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        pb_wave_sync();
#pragma unroll
        for (int jr = 0; jr < 4; ++jr)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned l = la[jr][k];
                a[jr][k] = __builtin_amdgcn_alignbyte(win[(l >> 2) + 1], win[l >> 2], l);
            }
        return;
    }
    // generic tile
    const int r0 = e->win_r0, c0 = e->win_c0;
    int nrows = e->win_rows;
    const unsigned gbase = (unsigned)r0 * rowbytes + 3u * (unsigned)c0;
    const unsigned a0 = gbase & 15u;
    int n16 = 1;
    if (nrows > 0) {
        n16 = (3 * e->win_cols + 15 + 1 + 15) >> 4;
        if (n16 > 64) n16 = 64;
        const int cap = Hd.win_budget / (16 * n16);
        if (nrows > cap) nrows = cap;
    }
    const unsigned pitch = 16u * (unsigned)n16;
    const unsigned rb16 = rowbytes & 15u;
    if (nrows > 0) pb_issue_window_loads(src, win, lane, gbase, rowbytes, nrows, n16, safe_len);
    int rc[4][4];
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) {
        PbRowModel R;
        pb_model_row(P, e, X0, Y0, yb + 8 * jr, 4 * xg, R);
#pragma unroll
        for (int k = 0; k < 4; ++k) rc[jr][k] = pb_model_px_rc<SRC_KIND>(P, R, 4 * xg, k);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    pb_wave_sync();
#pragma unroll
    for (int jr = 0; jr < 4; ++jr)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int v = rc[jr][k];
            unsigned px = 0;
            if (v >= 0) {
                const unsigned r = (unsigned)v >> 16, c = (unsigned)v & 0xFFFFu;
                const unsigned row = r - (unsigned)r0;
                const unsigned g = r * rowbytes + 3u * c;
                const unsigned off = 3u * (c - (unsigned)c0) + ((a0 + row * rb16) & 15u);
                if (row < (unsigned)nrows && off + 4u <= pitch && g + 4u <= safe_len) {
                    const unsigned l = row * pitch + off;
                    px = __builtin_amdgcn_alignbyte(win[(l >> 2) + 1], win[l >> 2], l);
                } else if (g + 4u <= frame_bytes) {
                    __builtin_memcpy(&px, src + g, 4);
                } else {
                    px = (unsigned)src[g] | ((unsigned)src[g + 1] << 8) | ((unsigned)src[g + 2] << 16);
                }
            }
            a[jr][k] = px;
        }
}

// A failed tile's values through the plan's exact indices (pb_failed_tile's gathers, one frame).
__device__ __forceinline__ void pb_ss_failed_vals(const PbHot& Hd, const PbTileEntry* __restrict__ e, const int lane,
                                                  const uint8_t* __restrict__ src, const int32_t* __restrict__ idx_tab, unsigned (&a)[4][4]) {
    const int xg = lane & 7, yb = lane >> 3;
    const int32_t* __restrict__ slot = idx_tab + (size_t)e->aux_off * (PB_TILE * PB_TILE);
    const unsigned last_px = (unsigned)Hd.src_h * (unsigned)Hd.src_w - 1u;
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) {
        const int4 v4 = *reinterpret_cast<const int4*>(slot + (yb + 8 * jr) * PB_TILE + 4 * xg);
        const int id[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int v = id[k];
            const bool last = (unsigned)v == last_px;
            const unsigned off = v < 0 ? 0u : 3u * (unsigned)v - (last ? 1u : 0u);
            unsigned t;
            __builtin_memcpy(&t, src + off, 4);
            a[jr][k] = v < 0 ? 0u : (last ? t >> 8 : t);
        }
    }
}

// Up to four output pixels (low 24 bits of v[0..3]) at pixel p of the output frame; `count` of them exist.
template <bool NT>
__device__ __forceinline__ void pb_ss_put(uint8_t* __restrict__ d, const unsigned long long p, const unsigned (&v)[4], const int count) {
    uint8_t* o = d + 3ull * p;
    if (count >= 4 && (((uintptr_t)o) & 3u) == 0) {
        pb_store3<NT>(pb_pack_px4(v[0], v[1], v[2], v[3]), o);
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < count) {
            o[3 * k + 0] = (uint8_t)(v[k] & 0xFF);
            o[3 * k + 1] = (uint8_t)((v[k] >> 8) & 0xFF);
            o[3 * k + 2] = (uint8_t)((v[k] >> 16) & 0xFF);
        }
}

// Cross-lane moves of the reduction, without the LDS crossbar where DPP can do it: lane ^ 8 is a rotation by 8 inside a 16-lane row
// (DPP row_ror:8), the quad moves are DPP quad_perm; lane ^ 16 crosses rows: ds_swizzle in bit mode (and 0x1f, xor 0x10), no LDS access.
__device__ __forceinline__ unsigned pb_ss_xor8(unsigned v) { return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, false); }
__device__ __forceinline__ unsigned pb_ss_xor16(unsigned v) { return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0x401F); }
template <int QUAD_PERM>
__device__ __forceinline__ unsigned pb_ss_quad(unsigned v) { return (unsigned)__builtin_amdgcn_mov_dpp((int)v, QUAD_PERM, 0xF, 0xF, false); }

// The n x n block means of a tile's values, stored as the H x W output.  Channels 0 and 2 are summed as two 16-bit fields of one
// register, channel 1 in another (at most 16 x 255 per field).  The horizontal part of a block is inside the lane; the vertical part
// comes from the lanes +-8 (and +-16 for n = 4: rows yb .. yb + 3) by butterfly moves (pb_ss_xor8 / pb_ss_xor16).  The finished pixels are then collected four
// to a lane, so that the output leaves in 12-byte stores like pb_win_tile's.
template <int NS, bool NT>
__device__ __forceinline__ void pb_ss_reduce_store(const unsigned (&a)[4][4], const int tx, const int ty, const int lane, const int Wn,
                                                   const int Hn, uint8_t* __restrict__ dst) {
    constexpr int K = NS == 2 ? 2 : 4;
    const int xg = lane & 7, yb = lane >> 3;
    const int Wo = Wn / NS;
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) {
        const int y = ty * PB_TILE + yb + 8 * jr;  // the lane's n x row; its block's first row when yb % n == 0
        unsigned px[4];
        if (NS == 2) {
            unsigned ev[2], od[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                ev[h] = (a[jr][2 * h] & 0xFF00FFu) + (a[jr][2 * h + 1] & 0xFF00FFu);
                od[h] = ((a[jr][2 * h] >> 8) & 0xFFu) + ((a[jr][2 * h + 1] >> 8) & 0xFFu);
                ev[h] += pb_ss_xor8(ev[h]);
                od[h] += pb_ss_xor8(od[h]);
            }
            const unsigned p0 = pb_ss_round<K>(ev[0] & 0xFFFFu) | (pb_ss_round<K>(od[0]) << 8) | (pb_ss_round<K>(ev[0] >> 16) << 16);
            const unsigned p1 = pb_ss_round<K>(ev[1] & 0xFFFFu) | (pb_ss_round<K>(od[1]) << 8) | (pb_ss_round<K>(ev[1] >> 16) << 16);
            // lane xg (even) takes its neighbour's two pixels: four consecutive output pixels
            const unsigned q0 = pb_ss_quad<0xB1>(p0), q1 = pb_ss_quad<0xB1>(p1);  // quad_perm [1, 0, 3, 2]: lane ^ 1
            px[0] = p0; px[1] = p1; px[2] = q0; px[3] = q1;
            if ((yb & 1) == 0 && (xg & 1) == 0 && y < Hn) {
                const int xo = (tx * PB_TILE + 4 * xg) / 2;
                if (xo < Wo) pb_ss_put<NT>(dst, (unsigned long long)(y / 2) * Wo + xo, px, min(4, Wo - xo));
            }
        } else {
            unsigned ev = 0, od = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ev += a[jr][k] & 0xFF00FFu;
                od += (a[jr][k] >> 8) & 0xFFu;
            }
            ev += pb_ss_xor8(ev);
            od += pb_ss_xor8(od);
            ev += pb_ss_xor16(ev);
            od += pb_ss_xor16(od);
            const unsigned p0 = pb_ss_round<K>(ev & 0xFFFFu) | (pb_ss_round<K>(od) << 8) | (pb_ss_round<K>(ev >> 16) << 16);
            // lane xg (0 or 4) takes the pixels of xg + 1 .. xg + 3
            px[0] = p0;
            px[1] = pb_ss_quad<0xF9>(p0);  // quad_perm [1, 2, 3, 3]: the quad's lane 0 reads lane 1
            px[2] = pb_ss_quad<0xFE>(p0);  // [2, 3, 3, 3]
            px[3] = pb_ss_quad<0xFF>(p0);  // [3, 3, 3, 3]
            if ((yb & 3) == 0 && (xg & 3) == 0 && y < Hn) {
                const int xo = (tx * PB_TILE + 4 * xg) / 4;
                if (xo < Wo) pb_ss_put<NT>(dst, (unsigned long long)(y / 4) * Wo + xo, px, min(4, Wo - xo));
            }
        }
    }
}

// The fused supersampled hot kernel: pb_hot_win_kernel's grid, workgroups, launch-order table and LDS windows over the n x plan
// (frames are a grid dimension: one launch per batch), each tile reduced before it is stored.  A tile's fix pixels (where the model's
// truncation differs from the faithful chain) are patched into the registers of the lanes that own them BEFORE the reduction: their
// exact values are loaded by lanes 0 .. n_fix - 1 and handed round one at a time (n_fix <= PB_TILE_FAIL_LIMIT, uniform loop).
template <int SRC_KIND, int NS>
__global__ __launch_bounds__(64 * PB_TILE_WAVES) void pb_ss_win_kernel(const PbParams* __restrict__ Pp, const PbHot Hd, const PbTileEntry* __restrict__ table,
                                                                        const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                        const unsigned groups_per_frame, unsigned long long src_stride,
                                                                        unsigned long long dst_stride, const int32_t* __restrict__ idx_tab,
                                                                        const int32_t* __restrict__ fix_px, const int32_t* __restrict__ fix_idx) {
    static_assert(NS == 2 || NS == 4, "n x n blocks of n = 2 or 4 lie inside one 32 x 32 tile");
    const PbParams& P = *Pp;
    asm volatile("" ::"s"(table), "s"(Hd.dst_w), "s"(Hd.dst_h), "s"(Hd.src_w), "s"(Hd.src_h), "s"(Hd.win_budget), "s"(groups_per_frame));
    const int lane = threadIdx.x & 63;
    const int wave_in_wg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr unsigned wpw = PB_TILE_WAVES;
    unsigned wg = blockIdx.x;
    const unsigned wgs_per_frame = groups_per_frame * (4u / wpw);
    if (wg >= wgs_per_frame) {
        const unsigned f = wg / wgs_per_frame;
        wg -= f * wgs_per_frame;
        src += (unsigned long long)f * src_stride;
        dst += (unsigned long long)f * dst_stride;
    }
    const unsigned flat = (wg >> 3) * wpw + (unsigned)wave_in_wg;
    const unsigned vslot = ((flat >> 2) * 8u + (wg & 7u)) * 4u + (flat & 3u);
    PbTileEntry entry;
    pb_load_entry(table + vslot, entry);
    const int tx = entry.tile_xy & 0xFFFF, ty = (int)((unsigned)entry.tile_xy >> 16);
    if (entry.flags & PB_TILE_SKIP) return;
    const PbTileEntry* __restrict__ e = &entry;
    const int flags = e->flags;
    unsigned a[4][4];
    if (flags & PB_TILE_FAILED) {
        pb_ss_failed_vals(Hd, e, lane, src, idx_tab, a);
    } else {
        pb_ss_tile_vals<SRC_KIND>(P, Hd, e, flags, tx, ty, lane, pb_dyn_lds + (size_t)wave_in_wg * ((Hd.win_budget >> 2) + 4), src, a);
        const int n_fix = e->fix_cnt;
        if (n_fix > 0) {
            unsigned fv = 0u;
            int fp = 0;
            if (lane < n_fix) {
                fp = fix_px[e->fix_off + lane];
                fv = pb_load_px(src, fix_idx[e->fix_off + lane]);
            }
            const int X0 = tx * PB_TILE, Y0 = ty * PB_TILE;
            for (int i = 0; i < n_fix; ++i) {
                const int p = __builtin_amdgcn_readlane(fp, i);
                const unsigned v = (unsigned)__builtin_amdgcn_readlane((int)fv, i);
                const int py = p / Hd.dst_w, px = p - py * Hd.dst_w;
                const int ly = py - Y0, lx = px - X0;  // inside this tile
                if (lane == (ly & 7) * 8 + (lx >> 2)) {
#pragma unroll
                    for (int jr = 0; jr < 4; ++jr)
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if ((ly >> 3) == jr && (lx & 3) == k) a[jr][k] = v;
                }
            }
        }
    }
    pb_ss_reduce_store<NS, PB_NT_DEFAULT(SRC_KIND)>(a, tx, ty, lane, Hd.dst_w, Hd.dst_h, dst);
}
