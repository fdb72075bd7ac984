// photonbend_hip.hip - the C ABI declared in include/photonbend_hip.h over the HIP kernels
// (gfx950 / CDNA4):
//   pb_kernels_faithful.hpp  per-pixel float64 chain (the reference semantics on the device; map API; PB_MODE_FAITHFUL)
//   pb_kernels_tile.hpp      hot kernel for pano / camera sources (per-tile float32 models, LDS windows, exact
//                            lookup tables), plan builders
//   pb_kernels_double.hpp    hot kernel for double-fisheye sources (one tile table per eye, weight classes)
//   pb_kernels_sep.hpp       separable tables for the unrotated stitch (row factors; unaligned-frame fallback)
//   pb_kernels_bilinear.hpp  opt-in bilinear sampling
//   pb_kernels_track.hpp     rotation tracks: a rotation per frame in one launch of the float64 chain
//   pb_kernels_track_video_bilinear.hpp  ... of video frames, sampled bilinearly
//   pb_kernels_track_stitch.hpp          ... of double-fisheye video frames, stitched
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared ...
// (-ffp-contract=off is REQUIRED: the reference rounds every multiply and add
// separately; fused multiply-adds appear only where written as fma()/fmaf()).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <algorithm>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "pb_params.hpp"
#include "pb_stages.hpp"
#include "pb_kernels_faithful.hpp"
#include "pb_tile.hpp"
#include "pb_kernels_tile.hpp"
#include "pb_kernels_sep.hpp"
#include "pb_kernels_double.hpp"
#include "pb_kernels_bilinear.hpp"
#include "pb_kernels_supersample.hpp"
#include "pb_kernels_catmull_rom.hpp"
#include "pb_kernels_px.hpp"
#include "pb_kernels_video.hpp"
#include "pb_kernels_track.hpp"
#include "pb_kernels_track_video.hpp"
#include "pb_kernels_planar_bilinear.hpp"
#include "pb_kernels_track_video_bilinear.hpp"
#include "pb_kernels_stitch_video.hpp"
#include "pb_kernels_track_stitch.hpp"
#include "pb_kernels_track_px.hpp"
#include "pb_kernels_px_interp.hpp"
#include "pb_kernels_pxf_interp.hpp"

#define PB_DOUBLE_FRAMES_PER_WAVE 1  // frames a double-source wave loops over (the rest of a batch is a grid dimension)

// Experiment knobs (environment variables) exist in the -DPB_ABLATION diagnostic build only (experiments/); the product
// library reads no environment.
#ifdef PB_ABLATION
static int pb_knob(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
#else
static inline int pb_knob(const char*, int dflt) { return dflt; }
#endif

// -DPB_ABLATION only: PB_PLAN_STAGES=1 prints where a plan preparation's host time goes (experiments/r6/plan_stages.py): PB_STAGE("name")
// stamps the host clock when the code reaches it, pb_stage_report prints the intervals.  Nothing in the product build.
#ifdef PB_ABLATION
#include <vector>
static std::vector<std::pair<const char*, double>> g_stages;
static void pb_stage_mark(const char* name) {
    static const int on = pb_knob("PB_PLAN_STAGES", 0);
    if (!on) return;
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    g_stages.emplace_back(name, ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6);
}
static void pb_stage_report() {
    if (g_stages.size() > 1) {
        fprintf(stderr, "[plan stages]");
        for (size_t k = 1; k < g_stages.size(); ++k) fprintf(stderr, " %s %.0f", g_stages[k].first, 1e3 * (g_stages[k].second - g_stages[k - 1].second));
        fprintf(stderr, " | total %.0f us\n", 1e3 * (g_stages.back().second - g_stages.front().second));
    }
    g_stages.clear();
}
#define PB_STAGE(name) pb_stage_mark(name)
#else
#define PB_STAGE(name) ((void)0)
static inline void pb_stage_report() {}
#endif

// -DPB_ABLATION only: PB_FAIL_LTABLE_ALLOC=n makes the n-th launch-table allocation of the process fail (tests of the error path)
static bool pb_test_alloc_fails() {
#ifdef PB_ABLATION
    static int countdown = pb_knob("PB_FAIL_LTABLE_ALLOC", 0);
    if (countdown > 0 && --countdown == 0) return true;
#endif
    return false;
}

// -DPB_ABLATION only: PB_BIL_OFF=<bits> switches SPEED-ONLY features of the opt-in bilinear mode off at plan creation (tests: the pixels
// must not depend on them) - 1 half windows, 2 unguarded table tiles, 4 the table tiles' walk, 8 half windows in pair slots, 16 the small LDS pool
static inline bool pb_bil_off(int bit) { return (pb_knob("PB_BIL_OFF", 0) & bit) != 0; }

static thread_local std::string g_err;
static int pb_fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define PB_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            return pb_fail(PB_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));   \
    } while (0)

// THE BLOCK CACHE AND WHO OWNS ITS BLOCKS.  Every device buffer of plan preparation - the temporaries of a few launches (counters, per-unit
// costs, a column table) and a plan's own tables (tile tables, fix lists, launch tables, parameter block) - comes from a per-device cache:
// a hipFree costs ~35 us on this stack (it synchronises the device) and a hipMalloc ~5; a released block is kept (up to 96 MiB in blocks
// of up to 16 MiB: the tables of a 33-Mpx plan) and handed to the next request it fits.  A block has ONE owner, a PbBlock: a local of the
// function that needs a temporary, a member of one of pb_plan's groups for a table; nothing else calls pb_tmp_alloc / pb_tmp_free.  When
// a block may go back depends on who may still be reading it - two rules:
//   temporaries  every user works on the NULL stream, which orders a block's next kernel behind its last one device-wide: a local PbBlock
//                goes out of scope after a synchronising copy or a hipDeviceSynchronize (error paths wait explicitly before they return),
//                or behind kernels whose results only later NULL-stream work reads.
//   plan tables  launches read them on the CALLER's streams, which the NULL stream does not order: ONE wait for the plan's device, then
//                the blocks go back - pb_drain_and_drop for a group or a launch table that is replaced, pb_plan_destroy for all of them.
namespace {
struct PbTmpCache {
    struct Block { int device; size_t bytes; void* ptr; };
    std::mutex lock;
    std::vector<Block> idle;
    std::unordered_map<void*, std::pair<int, size_t>> live;
    size_t held = 0;
} g_tmp;
}  // namespace
static hipError_t pb_tmp_alloc(void** out, size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    {
        std::lock_guard<std::mutex> g(g_tmp.lock);
        size_t best = g_tmp.idle.size();
        for (size_t k = 0; k < g_tmp.idle.size(); ++k) {
            const PbTmpCache::Block& b = g_tmp.idle[k];
            if (b.device == device && b.bytes >= bytes && b.bytes <= 4 * bytes + 4096 && (best == g_tmp.idle.size() || b.bytes < g_tmp.idle[best].bytes)) best = k;
        }
        if (best != g_tmp.idle.size()) {
            const PbTmpCache::Block b = g_tmp.idle[best];
            g_tmp.idle.erase(g_tmp.idle.begin() + (long)best);
            g_tmp.held -= b.bytes;
            g_tmp.live[b.ptr] = {b.device, b.bytes};
            *out = b.ptr;
            return hipSuccess;
        }
    }
    e = hipMalloc(out, bytes);
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> g(g_tmp.lock);
        g_tmp.live[*out] = {device, bytes};
    }
    return e;
}
static void pb_tmp_free(void* ptr) {
    if (!ptr) return;
    {
        std::lock_guard<std::mutex> g(g_tmp.lock);
        const auto it = g_tmp.live.find(ptr);
        if (it != g_tmp.live.end()) {
            const std::pair<int, size_t> info = it->second;
            g_tmp.live.erase(it);
            if (info.second <= ((size_t)16 << 20) && g_tmp.held + info.second <= ((size_t)96 << 20)) {
                g_tmp.idle.push_back({info.first, info.second, ptr});
                g_tmp.held += info.second;
                return;
            }
        }
    }
    (void)hipFree(ptr);
}
// The owner of one block of the cache: move-only, gives the block back when it dies or is reset().  Move assignment swaps - the block
// held before leaves with the source (`x = PbBlock<T>()` releases at once).  PbBlockAny is the untyped part (the blob code walks a
// plan's tables as bytes); PbBlock<T> converts to the T* the kernels take.
class PbBlockAny {
public:
    PbBlockAny() = default;
    PbBlockAny(const PbBlockAny&) = delete;
    PbBlockAny& operator=(const PbBlockAny&) = delete;
    PbBlockAny(PbBlockAny&& o) noexcept { swap(o); }
    PbBlockAny& operator=(PbBlockAny&& o) noexcept { swap(o); return *this; }
    ~PbBlockAny() { pb_tmp_free(p_); }
    void reset() { PbBlockAny().swap(*this); }
    void swap(PbBlockAny& o) noexcept { std::swap(p_, o.p_); }
    bool holds() const { return p_ != nullptr; }
    void* bytes() const { return p_; }
    hipError_t alloc_bytes(size_t n) {
        if (p_) return hipErrorInvalidValue;  // (a bug of the caller: reported, and the block it holds is not leaked)
        const hipError_t e = pb_tmp_alloc(&p_, n);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }

protected:
    void* p_ = nullptr;
};
template <class T>
class PbBlock : public PbBlockAny {
public:
    hipError_t alloc(size_t count) { return alloc_bytes(count * sizeof(T)); }
    T* get() const { return static_cast<T*>(p_); }
    operator T*() const { return get(); }
};

// Waits for `device` (< 0: the current one): a plan's launches may still be reading its tables on the caller's streams when a block goes
// back to the cache - what the hipFree of rounds 1-5 did by itself, once per table.
static void pb_wait_device(int device) {
    int cur = -1;
    if (device < 0 || hipGetDevice(&cur) != hipSuccess || cur == device) {
        (void)hipDeviceSynchronize();
        return;
    }
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    (void)hipSetDevice(cur);
}

// The separable tables' taps against the faithful chain, every pixel, once per plan: enqueued by the first launch that wants
// pb_sep_double_kernel, its verdict read - without waiting - by the launches after it.  The verdict lands in a word of a page of pinned,
// device-mapped host memory the process allocates once (the check kernel counts mismatches straight into it).
namespace {
struct PbSepPage {
    std::mutex lock;
    unsigned* host = nullptr;  // 1024 words
    unsigned* dev = nullptr;
    std::vector<int> idle;
} g_sep;
}  // namespace
// a plan's word of that page and the event recorded behind its check (pb_sep_setup hands them out; an empty one touches neither HIP
// nor the page); move-only, moves by swapping like PbBlock
struct PbSepSlot {
    int slot = -1;
    hipEvent_t event = nullptr;
    mutable int checked = 0;  // 0 not started, 2 in flight, 1 passed, -1 failed
    PbSepSlot() = default;
    PbSepSlot(PbSepSlot&& o) noexcept { swap(o); }
    PbSepSlot& operator=(PbSepSlot&& o) noexcept { swap(o); return *this; }
    void swap(PbSepSlot& o) noexcept { std::swap(slot, o.slot); std::swap(event, o.event); std::swap(checked, o.checked); }
    ~PbSepSlot() {
        if (slot < 0 && !event) return;
        std::lock_guard<std::mutex> g(g_sep.lock);
        if (event) {
            (void)hipEventSynchronize(event);  // (a check still in flight writes its word: the slot must not be handed on before)
            (void)hipEventDestroy(event);
        }
        if (slot >= 0) g_sep.idle.push_back(slot);
    }
};

// ---- a plan's device state, grouped by what builds it: each group owns its blocks and the counters that describe them, so
// "drop this state" is one assignment of a fresh group (pb_drain_and_drop where launches may be reading it) ---------------------------
// a launch-order copy of the tile tables and its size: set together, dropped together (a non-null table comes with groups >= 8)
struct PbLaunchTable {
    PbBlock<PbTileEntry> entries;
    unsigned groups = 0;  // virtual workgroups (of four waves) per frame, a multiple of 8
    bool holds() const { return entries.holds(); }
};
// CERTIFIED TABLES: built by pb_plan_prepare_on_device, completed by the first pb_classify_under_budget (saved_l / saved_r), written to
// blobs (pb_plan_sections) and restored from them
struct PbCertified {
    int fast_ready = 0;  // models + fix list built and certified on the plan's device
    PbBlock<PbTileEntry> table;
    PbBlock<int32_t> fail_tiles, fix_px;
    PbBlock<int32_t> idx_tab;  // exact source indices of the pixels of failed tiles (4 KiB per tile) ...
    PbBlock<int32_t> fix_idx;  // ... and of the fix list's pixels: looked up per frame instead of recomputed
    unsigned n_tiles = 0, n_fail_tiles = 0, n_fix_px = 0, n_lean_tiles = 0, n_black_tiles = 0, n_direct_tiles = 0;
    long long diff_pixels = -1;  // pixels (outside failed tiles) where model and faithful index differed
    // separable path (double source, unrotated pano destination): row / column tables.  sep_ready: the tables exist (their row weights
    // are exact by construction and serve the tile kernels); sep.checked: the exhaustive check of their TAPS against the faithful ones.
    // The check (one float64 chain per pixel: 0.27 ms of c5's 1.3 ms preparation) is only needed by pb_sep_double_kernel, the fallback
    // for frames the windowed two-eye kernel cannot take; the first launch that wants the fallback ENQUEUES it (pb_sep_usable: no
    // allocation, no synchronisation - the launch functions' contract) and takes the float64 kernel, later launches take the fallback
    // once the check has been seen to pass.
    int sep_ready = 0;
    PbSepSlot sep;
    PbBlock<PbSepRow> sep_rows;
    PbBlock<PbSepCol> sep_cols;
    // double-fisheye source: one certified tile table per eye (pb_kernels_double.hpp); `table` is the left eye's
    int dbl_ready = 0;
    PbBlock<PbTileEntry> table_r;
    PbBlock<PbDoubleFix> dbl_tile_fix, dbl_px_fix;  // faithful taps + factors of failed tiles' pixels / of the fix list's pixels
    PbBlock<double> lat_tab;  // faithful latitudes of the pixels of merge-band tiles (PB_TILE_W_LAT), 8 KiB per tile
    unsigned n_row_weight_tiles = 0, n_lat_tiles = 0;
    // the tile flags as classified and certified with the largest window budget: pb_apply_budget derives the flags
    // in use from them, so the budget can be changed at any time without touching a pixel
    PbBlock<int32_t> saved_l, saved_r;
    bool holds() const {
        return table.holds() || fail_tiles.holds() || fix_px.holds() || idx_tab.holds() || fix_idx.holds() || sep_rows.holds() || sep_cols.holds() ||
               table_r.holds() || dbl_tile_fix.holds() || dbl_px_fix.holds() || lat_tab.holds() || saved_l.holds() || saved_r.holds();
    }
};
// NEAREST LAUNCH STATE: rebuilt by pb_apply_budget with every budget change; derived, never serialized
struct PbNearestLaunch {
    PbLaunchTable lt;         // the hot kernel's launch-order copy of `table`
    PbBlock<PbParams> P_dev;  // device copy of P as the hot launches see it
    bool holds() const { return lt.holds() || P_dev.holds(); }
};
// BILINEAR-MODE STATE (pb_kernels_bilinear.hpp): built by pb_build_bilinear_list + pb_build_bilinear_launch from the certified tables;
// derived, never serialized, untouched by pb_plan_set_window_budget
struct PbBilinearState {
    PbBlock<int32_t> tiles;  // tiles the bilinear tile kernels leave to the float64 pass: PB_TILE_COARSE models; double-fisheye plans also tiles an eye sees but that are not plain for it
    unsigned n_tiles = 0;
    // the mode's exact coordinate tables: 8 KiB per slot (PbTileEntry::bil_off), and the fix list's coordinates (two per pixel for a
    // double-fisheye source); empty = the tables would not fit, those tiles take the float64 pass
    PbBlock<PbBilCoord> xy, fix_xy;
    unsigned n_slots = 0;
    // ... and its own launch-order table, classified under ITS window budget (PB_BIL_WIN_BUDGET: a direct-gather tile costs the
    // bilinear mode two 8-byte loads per pixel, the nearest mode one dword - its best budget is larger) and ordered by its own costs
    PbLaunchTable lt;
    int budget = 0;
    PbBlock<PbDblTables> dbl_tables;  // double-fisheye plans: what only some waves of the bilinear launch need, behind one pointer
    int waves = 4;                    // waves per REAL workgroup of a bilinear launch (4 or 2: chosen with the pool, pb_build_bilinear_launch)
    unsigned pool_bytes = 0;          // dynamic LDS of a bilinear launch's workgroup: the slots' regions are packed into it (pb_bilinear_pool_kernel)
    bool holds() const { return tiles.holds() || xy.holds() || fix_xy.holds() || lt.holds() || dbl_tables.holds(); }
};

struct pb_plan {
    PbParams P;
    int mode = PB_MODE_AUTO;  // PB_MODE_AUTO / PB_MODE_FAITHFUL / PB_MODE_FAST
    int device = -1;          // device that owns the blocks below
    PbCertified cert;
    PbNearestLaunch nearest;
    PbBilinearState bil;
    int bil_wanted = 1;  // 0: created with PB_PLAN_NO_BILINEAR - the opt-in mode's tables are built when pb_plan_prepare(PB_PLAN_BILINEAR) asks for them
    int walk = 0;        // launch-order rule: 0 = by policy (pb_build_launch_table), 1 = plain, 2 = rows from the heaviest outwards,
                         // 3 = super-tiles heaviest first; PB_PLAN_TUNE may pick 1-3 by timing, a serialized plan remembers it
    double prepare_ms = 0.0, tune_ms = 0.0;  // host wall time of the device preparation / of the optional budget tuning
    bool holds() const { return cert.holds() || nearest.holds() || bil.holds(); }
};
// The plan-table rule in one place: `state` (a group, a launch table, a single block) may be read by launches on the caller's streams, so
// the plan's device is waited for ONCE - only if there is a block to give back - and then the state is a fresh one, counters included.
template <class State>
static void pb_drain_and_drop(const pb_plan* pl, State& state) {
    if (state.holds()) pb_wait_device(pl->device);
    state = State();
}

static inline unsigned pb_blocks(unsigned long long items);
// plan preparation / deserialisation: a result word and an event for the plan (failure = the fallback stays unverified, i.e. unused)
static void pb_sep_setup(PbCertified& c) {
    if (!c.sep_ready || c.sep.slot >= 0) return;
    std::lock_guard<std::mutex> g(g_sep.lock);
    if (!g_sep.host) {
        void* h = nullptr;
        void* d = nullptr;
        if (hipHostMalloc(&h, 1024 * sizeof(unsigned), hipHostMallocMapped) != hipSuccess) return;
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
            (void)hipHostFree(h);
            return;
        }
        g_sep.host = (unsigned*)h;
        g_sep.dev = (unsigned*)d;
        for (int k = 1023; k >= 0; --k) g_sep.idle.push_back(k);
    }
    if (g_sep.idle.empty()) return;
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return;
    c.sep.slot = g_sep.idle.back();
    g_sep.idle.pop_back();
    c.sep.event = ev;
    c.sep.checked = 0;
}
// launch path: may pb_sep_double_kernel run?  Never waits, never allocates.
static bool pb_sep_usable(const pb_plan* plan, hipStream_t st) {
    if (!plan->cert.sep_ready || plan->cert.sep.slot < 0 || !plan->cert.sep.event || !plan->cert.sep_rows || !plan->cert.sep_cols) return false;
    std::lock_guard<std::mutex> g(g_sep.lock);
    if (plan->cert.sep.checked == 1) return true;
    if (plan->cert.sep.checked == -1) return false;
    if (plan->cert.sep.checked == 2) {
        if (hipEventQuery(plan->cert.sep.event) != hipSuccess) return false;  // still running (or the query failed): not yet
        plan->cert.sep.checked = g_sep.host[plan->cert.sep.slot] == 0u ? 1 : -1;
        return plan->cert.sep.checked == 1;
    }
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;  // (an event recorded inside a capture could not be queried afterwards)
    if (st && hipStreamIsCapturing(st, &capturing) == hipSuccess && capturing != hipStreamCaptureStatusNone) return false;
    const PbParams& P = plan->P;
    g_sep.host[plan->cert.sep.slot] = 0u;
    hipLaunchKernelGGL(pb_sep_check_kernel, dim3(pb_blocks((unsigned long long)P.dst.height * P.dst.width)), dim3(PB_BLOCK), 0, st, P, plan->cert.sep_rows,
                       plan->cert.sep_cols, g_sep.dev + plan->cert.sep.slot);
    if (hipEventRecord(plan->cert.sep.event, st) == hipSuccess) plan->cert.sep.checked = 2;
    return false;
}

// ----------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------
// ---- polynomial (Kannala-Brandt) lenses: the process-wide registry behind pb_lens_polynomial --------------------------
// Immutable entries; the same coefficients and max_theta (bit for bit) give the same id; ids are PB_LENS_POLYNOMIAL_BASE + slot and
// mean something in THIS process only - a plan's PbParams, its blob and the broadcast block carry the coefficients, never an id.
enum { PB_POLY_MAX_ENTRIES = 4096 };
static struct {
    std::mutex lock;
    std::vector<PbPoly> entries;
} g_poly;

static bool pb_poly_lookup(int lens, PbPoly* out) {
    if (lens < PB_LENS_POLYNOMIAL_BASE) return false;
    std::lock_guard<std::mutex> g(g_poly.lock);
    const size_t slot = (size_t)(lens - PB_LENS_POLYNOMIAL_BASE);
    if (slot >= g_poly.entries.size()) return false;
    if (out) *out = g_poly.entries[slot];
    return true;
}

// real roots in [lo, hi] of the polynomial c[0] + c[1] x + ... + c[n] x^n (n <= 4): between consecutive roots of the derivative the
// polynomial is monotonic, so every sign change brackets exactly one root, found by bisection
static void pb_poly_roots(const double* c, int n, double lo, double hi, std::vector<double>& roots) {
    while (n > 0 && c[n] == 0.0) --n;
    if (n == 0) return;
    if (n == 1) {
        const double r = -c[0] / c[1];
        if (r >= lo && r <= hi) roots.push_back(r);
        return;
    }
    double dc[4];
    for (int i = 1; i <= n; ++i) dc[i - 1] = (double)i * c[i];
    std::vector<double> pts;
    pts.push_back(lo);
    pb_poly_roots(dc, n - 1, lo, hi, pts);
    pts.push_back(hi);
    std::sort(pts.begin(), pts.end());
    const auto f = [&](double x) {
        double v = c[n];
        for (int i = n - 1; i >= 0; --i) v = v * x + c[i];
        return v;
    };
    for (size_t i = 0; i + 1 < pts.size(); ++i) {
        double a = pts[i], b = pts[i + 1];
        const double fa = f(a), fb = f(b);
        if (fa == 0.0) roots.push_back(a);
        if (!((fa < 0.0 && fb > 0.0) || (fa > 0.0 && fb < 0.0))) continue;
        for (int it = 0; it < 200; ++it) {
            const double m = 0.5 * (a + b);
            if (!(m > a && m < b)) break;
            if ((f(m) < 0.0) == (fa < 0.0)) a = m;
            else b = m;
        }
        roots.push_back(0.5 * (a + b));
    }
    if (f(hi) == 0.0) roots.push_back(hi);
}

// the checks of core/lens.py's polynomial(): finite coefficients, 0 < max_theta <= pi, dp > 0 on [0, max_theta] (its minimum is at an end
// or at a real root of the derivative of the quartic in t^2), and ten Newton steps invert p on a grid of 4097 angles to 2^-40
static bool pb_poly_make(const double k[4], double max_theta, PbPoly& L, std::string& why) {
    memset(&L, 0, sizeof(L));
    for (int i = 0; i < 4; ++i) {
        if (!std::isfinite(k[i])) {
            why = "polynomial lens: the coefficients must be finite";
            return false;
        }
        L.k[i] = k[i];
        L.d[i] = (double)(2 * i + 3) * k[i];
    }
    if (!(max_theta > 0.0 && max_theta <= PB_PI)) {
        why = "polynomial lens: max_theta must lie in (0, pi]";
        return false;
    }
    L.max_theta = max_theta;
    L.r_max = pb_poly_p(L, max_theta);
    const double U = max_theta * max_theta;
    const double q[5] = {1.0, L.d[0], L.d[1], L.d[2], L.d[3]}, dq[4] = {q[1], 2.0 * q[2], 3.0 * q[3], 4.0 * q[4]};
    std::vector<double> at;
    at.push_back(0.0);
    pb_poly_roots(dq, 3, 0.0, U, at);
    at.push_back(U);
    for (double u : at) {
        const double v = q[0] + u * (q[1] + u * (q[2] + u * (q[3] + u * q[4])));
        if (!(v > 0.0)) {
            why = "polynomial lens: r(theta) is not increasing on [0, max_theta] (a non-monotonic model folds the image); a calibration holds on the lens's own field only - pass a smaller max_theta";
            return false;
        }
    }
    if (!(L.r_max > 0.0) || !std::isfinite(L.r_max)) {
        why = "polynomial lens: r(max_theta) is not a positive finite number";
        return false;
    }
    for (int i = 0; i <= 4096; ++i) {
        const double theta = (i == 4096) ? max_theta : (double)i * (max_theta / 4096.0);
        const double r = pb_poly_p(L, theta);
        double t = r;
        for (int s = 0; s < PB_POLY_NEWTON_STEPS; ++s) t = t - (pb_poly_p(L, t) - r) / pb_poly_dp(L, t);
        if (!(fabs(t - theta) <= 9.094947017729282e-13)) {  // 2^-40
            why = "polynomial lens: ten Newton steps from t = r do not invert r(theta) on [0, max_theta]";
            return false;
        }
    }
    return true;
}

static int pb_poly_register(const PbPoly& L, int* lens_out) {
    std::lock_guard<std::mutex> g(g_poly.lock);
    for (size_t i = 0; i < g_poly.entries.size(); ++i)
        if (memcmp(&g_poly.entries[i], &L, sizeof(PbPoly)) == 0) {
            *lens_out = PB_LENS_POLYNOMIAL_BASE + (int)i;
            return PB_OK;
        }
    if (g_poly.entries.size() >= PB_POLY_MAX_ENTRIES) return PB_ERR_UNSUPPORTED;
    g_poly.entries.push_back(L);
    *lens_out = PB_LENS_POLYNOMIAL_BASE + (int)g_poly.entries.size() - 1;
    return PB_OK;
}

enum { PB_ROLE_DST = 1, PB_ROLE_SRC = 2, PB_ROLE_CUSTOM_OK = 4 };
static bool pb_has_lens(int kind) { return kind != PB_KIND_PANO && !pb_is_cube(kind); }  // (their pb_proj.lens / fov / f_distance are ignored)
static bool pb_end_ok(const pb_proj* p, std::string& why, int role = PB_ROLE_DST | PB_ROLE_SRC) {
    if (!p) {
        why = "null pb_proj";
        return false;
    }
    if ((p->kind < PB_KIND_CAMERA || p->kind > PB_KIND_PANO) && !pb_is_cube(p->kind)) {
        why = "pb_proj.kind out of range";
        return false;
    }
    if (pb_has_lens(p->kind) && (p->lens < PB_LENS_EQUIDISTANT || p->lens > PB_LENS_THOBY) && !pb_poly_lookup(p->lens, nullptr) &&
        !((role & PB_ROLE_CUSTOM_OK) && p->lens == PB_LENS_CUSTOM)) {
        why = p->lens == PB_LENS_CUSTOM ? "PB_LENS_CUSTOM is valid only where the host supplies the lens values (pb_index_from_map_i32 with distance planes)"
                                        : p->lens >= PB_LENS_POLYNOMIAL_BASE ? "pb_proj.lens is not a registered polynomial lens of this process (pb_lens_polynomial)"
                                        : "pb_proj.lens out of range";
        return false;
    }
    if (p->height < 1 || p->width < 1 || (long long)p->height * p->width > 0x7FFFFFFFll / 4) {
        why = "pb_proj height/width out of range (need 1 <= h*w < 2^29)";
        return false;
    }
    if (p->kind == PB_KIND_DOUBLE && (p->width & 1) && (role & PB_ROLE_DST)) {
        // the reference's map of an odd-width double DESTINATION is 2 * (W // 2) wide (projection.py:389-397): pass that width;
        // an odd-width double SOURCE is fine (eyes of W // 2 and W - W // 2 columns, projection.py:429-431)
        why = "a double-fisheye destination needs an even width (the reference's map is 2 * (W // 2) wide)";
        return false;
    }
    if (p->kind == PB_KIND_DOUBLE && p->width < 2) {
        why = "a double-fisheye frame needs at least two columns";
        return false;
    }
    if (pb_is_cube(p->kind) && ((p->height & 1) || p->width != 3 * (p->height / 2))) {
        why = "a cube map is a (2N, 3N) frame: six N x N faces in a 3 x 2 grid";
        return false;
    }
    return true;
}

// one end of a request as the parameter block holds it: a registered polynomial id resolves into PB_LENS_POLYNOMIAL + its coefficients
// (pb_end_ok and this function are the only places that know the registry)
struct PbEndX {
    PbEnd e;
    PbPoly poly;  // zero unless e.lens == PB_LENS_POLYNOMIAL
};
static PbEndX pb_to_end(const pb_proj* p) {
    PbEndX x;
    memset(&x, 0, sizeof(x));
    PbEnd& e = x.e;
    e.kind = p->kind;
    e.lens = (p->kind == PB_KIND_PANO) ? PB_LENS_EQUIDISTANT : p->lens;
    if (pb_has_lens(p->kind) && pb_poly_lookup(p->lens, &x.poly)) e.lens = PB_LENS_POLYNOMIAL;
    e.height = p->height;
    e.width = p->width;
    e.fov = p->fov;
    e.f_distance = p->f_distance;
    if (pb_is_cube(p->kind)) {
        // a face IS CameraImage(N x N, fov = 2 pi / 3, rectilinear()) with f_distance set to exactly N / 2: the block holds
        // that camera, whatever the caller left in the ignored fields
        e.lens = PB_LENS_RECTILINEAR;
        e.fov = 2 * PB_PI / 3;
        e.f_distance = (double)(p->height / 2) / 2;
    }
    return x;
}

static inline unsigned pb_blocks(unsigned long long items) { return (unsigned)((items + PB_BLOCK - 1) / PB_BLOCK); }


static inline unsigned pb_hot_blocks(const PbParams& P) {
    const unsigned tx = (P.dst.width + PB_TILE - 1) / PB_TILE, ty = (P.dst.height + PB_TILE - 1) / PB_TILE;
    return ((tx + 1) / 2) * ((ty + 1) / 2);
}
static inline unsigned pb_num_tiles(const PbParams& P) {
    return ((P.dst.width + PB_TILE - 1) / PB_TILE) * ((P.dst.height + PB_TILE - 1) / PB_TILE);
}

static_assert(16384 / PB_TILE < 65536, "PbTileEntry::tile_xy packs tile coordinates in 16 bits each");
static bool pb_fast_possible_dims(const PbParams& P) {
    // the tile models need 32-bit squares of the doubled pixel offsets and u24 index arithmetic
    return P.dst.width <= 16384 && P.dst.height <= 16384 && P.src.width < 32768 && P.src.height < 32768;
}
static bool pb_fast_possible(const PbParams& P) {
    return P.src.kind != PB_KIND_DOUBLE && P.dst.width <= 16384 && P.dst.height <= 16384 && P.src.width < (1 << 24) &&
           P.src.height < (1 << 24);
}

// the bilinear mode's plan state (pb_kernels_bilinear.hpp): which tiles the models cannot serve, their slots in the exact coordinate
// table, the table itself and the fix list's coordinates - all from the faithful float64 chain, once per plan; derived state, not
// serialized (rebuilt from the tile tables).  Synchronous.
// A double-fisheye source whose field of view is within one degree of 180 (not 180 itself): the reference keeps blending for half a degree past the merge
// band's end with the band's own slope (projection.py:416-418, :440-444), so the factor there reaches -0.5 deg / (fov - 180 deg) - minus
// 45 at 180.011 degrees - and multiplies whatever an eye's sample is off by.  The tile kernels' eye samples may be the neighbouring integer
// (1 LSB); with a band of a degree or more the factor stays within [-0.5, 1] and the sum within 2 LSB; below that the mode
// runs its per-pixel float64 kernels, whose eye samples are the definition's.  (Exactly 180 degrees: the factor is infinite or NaN and
// the cast gives 0 whatever the sample - no restriction.)
static bool pb_bilinear_tiles_allowed(const PbParams& P) {
    // (below 180 degrees the band turns inside out; it exists down to 179.5 degrees, with factors from 1 up to 0.5 deg / (180 deg - fov))
    // THE place that says a cube source has no tile tables in the interpolated modes (the definition per pixel on the selected face, DESIGN
    // 3.10): the table builders ask here, and pb_route follows from the tables' absence
    if (pb_is_cube(P.src.kind)) return false;
    return !(P.src.kind == PB_KIND_DOUBLE && P.mrg_range != 0.0 && fabs(P.mrg_range) < 0.999 * (PB_PI / 180.0));  // (181 / 179 degrees themselves: tiles)
}
// (PB_INTERP_CATMULL_ROM: the third id, which pb_remap_track_u8 takes; the supersampled entry points take PB_INTERP_NEAREST and PB_INTERP_BILINEAR)
// Template arguments from run-time values: f(PbInt<A>()) if `first`, else f(PbInt<B>()) - the kernel's KIND, its waves per workgroup,
// the supersample factor.
template <int V>
using PbInt = std::integral_constant<int, V>;
template <int A, int B, class F>
static void pb_pick(bool first, F&& f) {
    if (first) f(PbInt<A>());
    else f(PbInt<B>());
}
// pb_px_hot_kernel's BPP (PB_PX_SIZES without 3, which is pb_hot_win_kernel's)
template <class F>
static void pb_pick_px_size(int bpp, F&& f) {
    switch (bpp) {
        case 1: f(PbInt<1>()); break;
        case 2: f(PbInt<2>()); break;
        case 4: f(PbInt<4>()); break;
        case 6: f(PbInt<6>()); break;
        default: f(PbInt<8>()); break;
    }
}
// pb_px_interp_kernel's (C, S): 1 to 4 channels of 1 or 2 bytes without (3, 1), which is the RGB8 tile kernels'
template <class F>
static void pb_pick_px_format(int channels, int sample_bytes, F&& f) {
    static_assert(PB_PXI_BILINEAR == PB_INTERP_BILINEAR && PB_PXI_CATMULL_ROM == PB_INTERP_CATMULL_ROM, "the kernel's FILTER is the header's constant");
    switch (channels * 4 + sample_bytes) {
        case 1 * 4 + 1: f(PbInt<1>(), PbInt<1>()); break;
        case 2 * 4 + 1: f(PbInt<2>(), PbInt<1>()); break;
        case 4 * 4 + 1: f(PbInt<4>(), PbInt<1>()); break;
        case 1 * 4 + 2: f(PbInt<1>(), PbInt<2>()); break;
        case 2 * 4 + 2: f(PbInt<2>(), PbInt<2>()); break;
        case 3 * 4 + 2: f(PbInt<3>(), PbInt<2>()); break;
        default: f(PbInt<4>(), PbInt<2>()); break;
    }
}
// pb_pxf_interp_kernel's (C, S): 1 to 4 channels of binary16 or binary32 samples
template <class F>
static void pb_pick_pxf_format(int channels, int sample_bytes, F&& f) {
    pb_pick<2, 4>(sample_bytes == 2, [&](auto S) {
        switch (channels) {
            case 1: f(PbInt<1>(), S); break;
            case 2: f(PbInt<2>(), S); break;
            case 3: f(PbInt<3>(), S); break;
            default: f(PbInt<4>(), S); break;
        }
    });
}
// pb_video_hot_kernel's SUB (PB_PLANAR_444 / _422 / _420; pb_video_fmt_check has refused everything else)
template <class F>
static void pb_pick_subsampling(int sub, F&& f) {
    static_assert(PB_PLANAR_444 == PB_SUB_444 && PB_PLANAR_422 == PB_SUB_422 && PB_PLANAR_420 == PB_SUB_420, "the kernel's SUB is the header's constant");
    switch (sub) {
        case PB_PLANAR_444: f(PbInt<PB_SUB_444>()); break;
        case PB_PLANAR_422: f(PbInt<PB_SUB_422>()); break;
        default: f(PbInt<PB_SUB_420>()); break;
    }
}
// The SRC_KIND of the MODEL-evaluating kernels (hot, window, supersampled, interpolated tile kernels) of a single source.  A cube source
// runs the camera's: what those kernels evaluate is a certified tile model, a frame-wide bounds test and the camera's truncation edge, and
// pb_certify_kernel<PB_KIND_CUBE> compares that very evaluation with the cube's float64 chain for every pixel.
template <class F>
static void pb_pick_kind(const PbParams& P, F&& f) {
    pb_pick<PB_KIND_PANO, PB_KIND_CAMERA>(P.src.kind == PB_KIND_PANO, f);
}
// a cube source's mapping (P.src.kind is one of the two: pb_is_cube)
template <class F>
static void pb_pick_cube_kind(const PbParams& P, F&& f) {
    pb_pick<PB_KIND_EAC, PB_KIND_CUBE>(P.src.kind == PB_KIND_EAC, f);
}
// ... and of the kernels that run the float64 chain of a single source: a cube's own, of either mapping
template <class F>
static void pb_pick_exact_kind(const PbParams& P, F&& f) {
    if (pb_is_cube(P.src.kind)) pb_pick_cube_kind(P, f);
    else pb_pick_kind(P, f);
}
template <class F>
static void pb_pick_lensed_kind(const PbParams& P, F&& f) {  // (every source but a cube, whose kernels of the caller have names of their own)
    if (P.src.kind == PB_KIND_DOUBLE) f(PbInt<PB_KIND_DOUBLE>());
    else pb_pick_kind(P, f);
}
template <class F>
static void pb_pick_any_kind(const PbParams& P, F&& f) {  // (float64 chain, any source)
    if (P.src.kind == PB_KIND_DOUBLE) f(PbInt<PB_KIND_DOUBLE>());
    else pb_pick_exact_kind(P, f);
}
// Kernels that carry a NAME per cube mapping instead of a template argument (the listing tests count the other sources' instantiations
// per kind: pb_kernels_bilinear.hpp, pb_kernels_track.hpp) - the one place that maps a kind to them
template <int KIND, class FILTER>
static constexpr auto pb_interp_cube_kernel_of() {
    if constexpr (KIND == PB_KIND_EAC) return &pb_interp_eac_kernel<FILTER>;
    else return &pb_interp_cube_kernel<FILTER>;
}
template <int KIND, class FILTER, typename SAMPLE>
static constexpr auto pb_sample_map_interp_cube_kernel_of() {
    if constexpr (KIND == PB_KIND_EAC) return &pb_sample_map_interp_eac_kernel<FILTER, SAMPLE>;
    else return &pb_sample_map_interp_cube_kernel<FILTER, SAMPLE>;
}
template <int KIND>
static constexpr auto pb_track_kernel_of() {
    if constexpr (KIND == PB_KIND_EAC) return &pb_track_eac_kernel;
    else return &pb_track_kernel<KIND>;
}
template <int KIND, class FILTER>
static constexpr auto pb_track_interp_kernel_of() {
    if constexpr (KIND == PB_KIND_EAC) return &pb_track_interp_eac_kernel<FILTER>;
    else return &pb_track_interp_kernel<KIND, FILTER>;
}
template <int KIND>
static constexpr auto pb_track_px_kernel_of() {
    if constexpr (KIND == PB_KIND_EAC) return &pb_track_px_equiangular_kernel;
    else return &pb_track_px_kernel<KIND>;
}
template <int KIND, class FILTER, typename SAMPLE>
static constexpr auto pb_track_px_interp_kernel_of() {
    if constexpr (KIND == PB_KIND_EAC) return &pb_track_px_interp_equiangular_kernel<FILTER, SAMPLE>;
    else return &pb_track_px_interp_kernel<KIND, FILTER, SAMPLE>;
}
template <class F>
static void pb_pick_filter(int filter, F&& f) {  // (the FILTER of the shared sampler kernels, pb_kernels_bilinear.hpp)
    if (filter == PB_INTERP_CATMULL_ROM) f(PbCatmullRom());
    else f(PbBilinear());
}
static int pb_build_bilinear_list(pb_plan* pl) {
    const PbParams& P = pl->P;
    pb_drain_and_drop(pl, pl->bil);  // (the whole mode's state: pb_build_bilinear_launch follows and builds the rest)
    if (!pb_bilinear_tiles_allowed(P)) return PB_OK;  // (no tables: pb_remap_bilinear_u8 takes the float64 kernels)
    unsigned res[2] = {0u, 0u};
    hipError_t e;
    {
        PbBlock<unsigned> cnt;  // (its scope: back in the cache before the coordinate tables ask for their blocks)
        PB_HIP(cnt.alloc(2));
        e = hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned), 0);
        if (e == hipSuccess) e = pl->bil.tiles.alloc(pl->cert.n_tiles ? pl->cert.n_tiles : 1);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(pb_bilinear_tile_list_kernel, dim3((pl->cert.n_tiles + 255) / 256), dim3(256), 0, 0, pl->cert.table, pl->cert.table_r, pl->cert.n_tiles,
                               P.src_eye_w, P.src.width, pl->bil.tiles, cnt);
            e = hipMemcpy(res, cnt, sizeof(res), hipMemcpyDeviceToHost);
        } else {
            (void)hipDeviceSynchronize();
        }
    }
    const bool dbl = pl->cert.table_r.holds();
    // the tables: sources the 1/4096-px fixed point holds, and at most 1 GiB of coordinates (a geometry the models mostly cannot
    // follow keeps the float64 pass)
    const bool tables = e == hipSuccess && P.src.width < PB_BIL_MAX_DIM && P.src.height < PB_BIL_MAX_DIM && (size_t)P.src.width * P.src.height >= 3 &&
                        (size_t)res[1] * PB_TILE * PB_TILE * sizeof(PbBilCoord) <= ((size_t)1 << 30);
    if (tables) {
        const unsigned np = pl->cert.n_fix_px, stride = dbl ? 2u : 1u;
        e = pl->bil.xy.alloc((size_t)(res[1] ? res[1] : 1u) * PB_TILE * PB_TILE);
        if (e == hipSuccess) e = pl->bil.fix_xy.alloc((size_t)(np ? np : 1u) * stride);
        if (e == hipSuccess) {
            const dim3 grid(4u * pl->cert.n_tiles), block(PB_BLOCK), fgrid((np + PB_BLOCK - 1) / PB_BLOCK);
            if (dbl) {
                hipLaunchKernelGGL(pb_bilinear_coord_kernel<PB_KIND_EYE_L>, grid, block, 0, 0, P, pl->cert.table, pl->bil.xy);
                hipLaunchKernelGGL(pb_bilinear_coord_kernel<PB_KIND_EYE_R>, grid, block, 0, 0, P, pl->cert.table_r, pl->bil.xy);
                if (np) {
                    hipLaunchKernelGGL(pb_bilinear_fix_coord_kernel<PB_KIND_EYE_L>, fgrid, block, 0, 0, P, pl->cert.fix_px, (int)np, pl->bil.fix_xy, 2, 0);
                    hipLaunchKernelGGL(pb_bilinear_fix_coord_kernel<PB_KIND_EYE_R>, fgrid, block, 0, 0, P, pl->cert.fix_px, (int)np, pl->bil.fix_xy, 2, 1);
                }
            } else {
                pb_pick_kind(P, [&](auto K) {
                    hipLaunchKernelGGL(pb_bilinear_coord_kernel<K.value>, grid, block, 0, 0, P, pl->cert.table, pl->bil.xy);
                    if (np) hipLaunchKernelGGL(pb_bilinear_fix_coord_kernel<K.value>, fgrid, block, 0, 0, P, pl->cert.fix_px, (int)np, pl->bil.fix_xy, 1, 0);
                });
            }
            // which way each slot is walked (lanes along the direction the source position moves least), slots walked by rows transposed
            // ... and whether its taps need the guards at all (PB_TILE_TAB_PLAIN); an eye's taps stay in its half of the frame
            hipLaunchKernelGGL(pb_bilinear_orient_kernel, dim3(pl->cert.n_tiles), dim3(256), 0, 0, pl->cert.table, pl->bil.xy, P.src.height, P.src.width, 0,
                               dbl ? P.src_eye_w : P.src.width, pb_knob("PB_BIL_OFF", 0), pl->cert.saved_l);
            if (dbl)
                hipLaunchKernelGGL(pb_bilinear_orient_kernel, dim3(pl->cert.n_tiles), dim3(256), 0, 0, pl->cert.table_r, pl->bil.xy, P.src.height, P.src.width, P.src_eye_w,
                                   P.src.width, pb_knob("PB_BIL_OFF", 0), pl->cert.saved_r);
            e = hipGetLastError();  // (not waited for: the launch builder's read-backs follow on the same stream and report a failure)
        }
    }
    if (e != hipSuccess) {
        pb_drain_and_drop(pl, pl->bil);  // (the kernels above may be running)
        return pb_fail(PB_ERR_HIP, std::string("bilinear tables: ") + hipGetErrorString(e));
    }
    pl->bil.n_tiles = res[0];
    pl->bil.n_slots = res[1];
    return PB_OK;
}

// Runs once per plan on the current device (synchronously, default stream):
//  1. validity thresholds of a camera / double destination by bisection with the exact predicate;
//  2. per-tile polynomial models (pb_model_kernel);
//  3. certification: the hot path's index is compared with the faithful one for EVERY pixel; differing
//     pixels / tiles become the plan's fix list (pb_certify_kernel).
static int pb_plan_prepare_on_device(pb_plan* pl) {
    PbParams& P = pl->P;
    PbCertified& c = pl->cert;
    PbBlock<long long> scratch;
    PB_HIP(hipGetDevice(&pl->device));
    PB_HIP(scratch.alloc(16));
    int rc = PB_OK;
    do {
        if (pb_is_cube(P.dst.kind)) {
            // no pixel of a cube is invalid (the largest incidence angle on a face is below 54.74 degrees, fov / 2 is 60): thresholds no
            // (2x)^2 + (2y)^2 reaches, so that the tile code's integer validity test never fires
            for (int sd = 0; sd < 2; ++sd) P.inv_lo[sd] = P.inv_hi[sd] = (int64_t)1 << 62;
        } else if (P.dst.kind != PB_KIND_PANO) {
            hipLaunchKernelGGL(pb_threshold_kernel, dim3(1), dim3(128), 0, 0, P, scratch);
            // (a chain of ~10 dependent square roots and arcsines, and the kernel's launch: a single source's tile tables are allocated meanwhile)
            if (P.src.kind != PB_KIND_DOUBLE && pb_fast_possible(P)) {
                const unsigned nt0 = pb_num_tiles(P);
                if (c.table.alloc(nt0) != hipSuccess ||
                    c.fail_tiles.alloc(nt0) != hipSuccess ||
                    c.fix_px.alloc((size_t)nt0 * PB_TILE_FAIL_LIMIT) != hipSuccess) { rc = PB_ERR_HIP; break; }
            }
            long long thr[4];
            if (hipMemcpy(thr, scratch, sizeof(thr), hipMemcpyDeviceToHost) != hipSuccess) { rc = PB_ERR_HIP; break; }
            P.inv_lo[0] = thr[0]; P.inv_hi[0] = thr[1];
            P.inv_lo[1] = thr[2]; P.inv_hi[1] = thr[3];
        }
        P.thresholds_ready = 1;
        if (P.src.kind == PB_KIND_DOUBLE && P.dst.kind == PB_KIND_PANO && P.n_rot == 0) {
            // separable path: the row / column tables (their taps are checked against the faithful ones when first needed: pb_sep_verified)
            if (c.sep_rows.alloc(P.dst.height) != hipSuccess ||
                c.sep_cols.alloc(P.dst.width) != hipSuccess) { rc = PB_ERR_HIP; break; }
            hipLaunchKernelGGL(pb_sep_tables_kernel, dim3(pb_blocks((unsigned long long)P.dst.height + P.dst.width)), dim3(PB_BLOCK), 0, 0,
                               P, c.sep_rows, c.sep_cols);
            c.sep_ready = 1;
            c.sep.checked = 0;
            pb_sep_setup(pl->cert);
        }
        if (P.src.kind == PB_KIND_DOUBLE) {
            // two certified tile tables (one per eye) + the weight class of every tile
            if (!pb_fast_possible_dims(P)) break;
            const unsigned ntiles = pb_num_tiles(P);
            const unsigned cap = 2u * ntiles * PB_TILE_FAIL_LIMIT;
            if (c.table.alloc(ntiles) != hipSuccess ||
                c.table_r.alloc(ntiles) != hipSuccess ||
                c.fail_tiles.alloc((size_t)2 * ntiles) != hipSuccess ||
                c.fix_px.alloc(cap) != hipSuccess) { rc = PB_ERR_HIP; break; }
            unsigned* counters = reinterpret_cast<unsigned*>(scratch + 4);
            if (hipMemsetAsync(counters, 0, 12 * sizeof(unsigned), 0) != hipSuccess) { rc = PB_ERR_HIP; break; }
            const dim3 grid(pb_hot_blocks(P)), block(64 * PB_TILE_WAVES);
            // (unrotated panorama destination: the separable path's column table holds the sine / cosine of every column's longitude)
            const double* col_sc = (P.dst.kind == PB_KIND_PANO && P.n_rot == 0 && c.sep_cols) ? reinterpret_cast<const double*>(c.sep_cols.get()) : nullptr;
            hipLaunchKernelGGL(pb_model_kernel<PB_KIND_EYE_L>, grid, block, 0, 0, P, c.table);
            hipLaunchKernelGGL(pb_window_kernel<PB_KIND_EYE_L>, grid, block, 0, 0, P, c.table);
            PB_LAUNCH_BY_ROT(P, pb_certify_kernel, PB_KIND_EYE_L, grid, block, 0, 0, P, c.table, c.fail_tiles, c.fix_px, cap, counters, col_sc);
            hipLaunchKernelGGL(pb_model_kernel<PB_KIND_EYE_R>, grid, block, 0, 0, P, c.table_r);
            hipLaunchKernelGGL(pb_window_kernel<PB_KIND_EYE_R>, grid, block, 0, 0, P, c.table_r);
            PB_LAUNCH_BY_ROT(P, pb_certify_kernel, PB_KIND_EYE_R, grid, block, 0, 0, P, c.table_r, c.fail_tiles, c.fix_px, cap, counters, col_sc);
            hipLaunchKernelGGL(pb_count_flags_kernel, dim3((ntiles + 255) / 256), dim3(256), 0, 0, c.table, ntiles, counters);
            hipLaunchKernelGGL(pb_count_flags_kernel, dim3((ntiles + 255) / 256), dim3(256), 0, 0, c.table_r, ntiles, counters);
            const unsigned lat_capacity = ntiles < 65536u ? ntiles : 65536u;  // <= 512 MiB of latitudes
            hipLaunchKernelGGL(pb_double_pair_kernel, grid, block, 0, 0, P, c.table, c.table_r, c.sep_ready ? c.sep_rows : nullptr,
                               c.fail_tiles, counters, lat_capacity);
            unsigned res[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            if (hipMemcpy(res, counters, sizeof(res), hipMemcpyDeviceToHost) != hipSuccess) { rc = PB_ERR_HIP; break; }
            c.n_lat_tiles = res[8] < lat_capacity ? res[8] : lat_capacity;
            if (c.n_lat_tiles) {
                if (c.lat_tab.alloc((size_t)c.n_lat_tiles * PB_LAT_TILE_DOUBLES) != hipSuccess) { rc = PB_ERR_HIP; break; }
                hipLaunchKernelGGL(pb_double_lat_kernel, grid, block, 0, 0, P, c.table, c.lat_tab);
                if (hipGetLastError() != hipSuccess) { rc = PB_ERR_HIP; break; }  // (not waited for: see the fix tables below)
            }
            {   // faithful taps of failed tiles and fix pixels, looked up per frame
                const unsigned nf = res[1], np = res[0] > cap ? cap : res[0];
                // a geometry the models mostly cannot follow is not worth gigabytes of stored taps: faithful kernel
                if ((size_t)nf * PB_TILE * PB_TILE * sizeof(PbDoubleFix) > ((size_t)1 << 30)) break;
                if (c.dbl_tile_fix.alloc((size_t)(nf ? nf : 1) * PB_TILE * PB_TILE) != hipSuccess ||
                    c.dbl_px_fix.alloc((size_t)(np ? np : 1)) != hipSuccess) { rc = PB_ERR_HIP; break; }
                const unsigned blocks = 4u * nf + (np + PB_BLOCK - 1) / PB_BLOCK;
                if (blocks) {
                    hipLaunchKernelGGL(pb_double_tables_kernel, dim3(blocks), dim3(PB_BLOCK), 0, 0, P, c.table_r, c.fail_tiles, (int)nf, c.fix_px,
                                       (int)np, c.dbl_tile_fix, c.dbl_px_fix);
                    // (not waited for: the budget pass and the launch-order pass queue up behind it, and their readback reports a failure)
                    if (hipGetLastError() != hipSuccess) { rc = PB_ERR_HIP; break; }
                }
            }
            c.n_tiles = ntiles;
            c.n_lean_tiles = res[4];
            c.n_black_tiles = res[5];
            c.n_direct_tiles = res[6];
            c.n_row_weight_tiles = res[7];
            c.n_fix_px = res[0] > cap ? cap : res[0];
            c.n_fail_tiles = res[1];
            c.diff_pixels = res[2];
            if (pl->bil_wanted && pb_build_bilinear_list(pl) != PB_OK) { rc = PB_ERR_HIP; break; }
            c.dbl_ready = 1;
            break;
        }
        PB_STAGE("thresholds");
        if (!pb_fast_possible(P)) break;
        const unsigned ntiles = pb_num_tiles(P);
        const unsigned cap = ntiles * PB_TILE_FAIL_LIMIT;
        if (!c.table &&  // (not allocated beside the threshold kernel above)
            (c.table.alloc(ntiles) != hipSuccess ||
             c.fail_tiles.alloc(ntiles) != hipSuccess ||
             c.fix_px.alloc(cap) != hipSuccess)) { rc = PB_ERR_HIP; break; }
        PB_STAGE("malloc3");
        unsigned* counters = reinterpret_cast<unsigned*>(scratch + 4);
        if (hipMemsetAsync(counters, 0, 8 * sizeof(unsigned), 0) != hipSuccess) { rc = PB_ERR_HIP; break; }
        const dim3 grid(pb_hot_blocks(P)), block(64 * PB_TILE_WAVES);
        if (P.src.kind == PB_KIND_PANO) {
            hipLaunchKernelGGL(pb_model_kernel<PB_KIND_PANO>, grid, block, 0, 0, P, c.table);
            hipLaunchKernelGGL(pb_window_kernel<PB_KIND_PANO>, grid, block, 0, 0, P, c.table);
            PB_LAUNCH_BY_ROT(P, pb_certify_kernel, PB_KIND_PANO, grid, block, 0, 0, P, c.table, c.fail_tiles, c.fix_px, cap, counters);
        } else if (pb_is_cube(P.src.kind)) {
            // tiles whose pixels fall on more than one face get no usable model from their 25 nodes and fail certification by themselves
            pb_pick_cube_kind(P, [&](auto K) {
                hipLaunchKernelGGL(pb_model_kernel<K.value>, grid, block, 0, 0, P, c.table);
                hipLaunchKernelGGL(pb_window_kernel<K.value>, grid, block, 0, 0, P, c.table);
                PB_LAUNCH_BY_ROT(P, pb_certify_kernel, K.value, grid, block, 0, 0, P, c.table, c.fail_tiles, c.fix_px, cap, counters);
            });
        } else {
            PbBlock<double> col_sc;  // (unrotated panorama destination: one sine / cosine per column instead of one per pixel)
            if (P.dst.kind == PB_KIND_PANO && P.n_rot == 0 && col_sc.alloc((size_t)P.dst.width * 2) == hipSuccess)
                hipLaunchKernelGGL(pb_col_sincos_kernel, dim3((P.dst.width + 255) / 256), dim3(256), 0, 0, P, col_sc);
            hipLaunchKernelGGL(pb_model_kernel<PB_KIND_CAMERA>, grid, block, 0, 0, P, c.table);
            hipLaunchKernelGGL(pb_window_kernel<PB_KIND_CAMERA>, grid, block, 0, 0, P, c.table);
            PB_LAUNCH_BY_ROT(P, pb_certify_kernel, PB_KIND_CAMERA, grid, block, 0, 0, P, c.table, c.fail_tiles, c.fix_px, cap, counters, (const double*)col_sc);
            if (col_sc) (void)hipDeviceSynchronize();  // (the block goes back at the end of this scope)
        }
        PB_STAGE("enqueue+colsync");
        hipLaunchKernelGGL(pb_count_flags_kernel, dim3((ntiles + 255) / 256), dim3(256), 0, 0, c.table, ntiles, counters);
        unsigned res[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpy(res, counters, sizeof(res), hipMemcpyDeviceToHost) != hipSuccess) { rc = PB_ERR_HIP; break; }
        PB_STAGE("certify-readback");
        c.n_lean_tiles = res[4];
        c.n_black_tiles = res[5];
        c.n_direct_tiles = res[6];
        c.n_fix_px = res[0] > cap ? cap : res[0];
        c.n_fail_tiles = res[1];
        c.diff_pixels = res[2];
        c.n_tiles = ntiles;
        {   // exact-index tables for the windowed hot kernel
            const unsigned nf = c.n_fail_tiles, np = c.n_fix_px;
            if (c.idx_tab.alloc((size_t)(nf ? nf : 1) * PB_TILE * PB_TILE) != hipSuccess ||
                c.fix_idx.alloc((size_t)(np ? np : 1)) != hipSuccess) { rc = PB_ERR_HIP; break; }
            const unsigned blocks = 4u * nf + (np + PB_BLOCK - 1) / PB_BLOCK;
            if (blocks) {
                pb_pick_exact_kind(P, [&](auto K) {
                    hipLaunchKernelGGL(pb_fix_tables_kernel<K.value>, dim3(blocks), dim3(PB_BLOCK), 0, 0, P, c.table, c.fail_tiles, (int)nf, c.fix_px,
                                       (int)np, c.idx_tab, c.fix_idx);
                });
                // (not waited for: the budget pass and the launch-order pass queue up behind it, and their readback reports a failure)
                if (hipGetLastError() != hipSuccess) { rc = PB_ERR_HIP; break; }
            }
        }
        PB_STAGE("fix-tables");
        if (pl->bil_wanted && pb_build_bilinear_list(pl) != PB_OK) { rc = PB_ERR_HIP; break; }
        c.fast_ready = 1;
    } while (0);
    if (rc != PB_OK) {
        g_err = std::string("plan preparation on device failed: ") + hipGetErrorString(hipGetLastError());
        (void)hipDeviceSynchronize();
        // the failed attempt's state goes as a whole, counters and readiness included: the plan reads as never prepared
        pl->cert = PbCertified();
        pl->bil = PbBilinearState();
    }
    PB_STAGE("bil-list");
    // (the scratch block's next user is ordered behind these kernels by the NULL stream; pb_plan_prepare_full's budget pass ends the
    //  preparation with the wait - a failed one waits here, its tables have just been freed)
    if (rc != PB_OK || !(c.fast_ready || c.dbl_ready)) (void)hipDeviceSynchronize();
    PB_STAGE("final-sync");
    return rc;
}

static bool pb_use_fast(const pb_plan* plan) { return plan->cert.fast_ready && plan->mode != PB_MODE_FAITHFUL; }

// ---- what a remap call launches ------------------------------------------------------------------------------------
// The plan's tables live on the device it was prepared on (a deferred plan has none yet).
static int pb_check_device(const pb_plan* plan) {
    if (plan->device < 0) return PB_OK;
    int dev = -1;
    PB_HIP(hipGetDevice(&dev));
    if (dev != plan->device) return pb_fail(PB_ERR_INVALID, "plan was prepared on another device; create one plan per device");
    return PB_OK;
}

// The arguments of every frame-launching entry point, in this order: null plan / frames, the frame count (0: PB_OK and nothing to
// launch - callers return), the plan's device, the frame strides (0: tightly packed; the defaults are filled in here and nowhere
// else).  n: the supersample factor - an output frame is H/n x W/n of the plan's destination.  tables: src / dst are pb_remap_u8v's
// pointer tables, which may be null when there are no frames.  bpp: bytes per pixel (pb_remap_px; 3 everywhere else) - one of
// PB_PX_SIZES, frames and strides aligned to pb_px_align(bpp).  wide: 12 and 16 are pixel sizes too (three and four float32 channels:
// pb_remap_interp_pxf alone).
static bool pb_px_size_ok(int bpp) { return bpp == 1 || bpp == 2 || bpp == 3 || bpp == 4 || bpp == 6 || bpp == 8; }
static unsigned pb_px_align(int bpp) { return (unsigned)std::min(4, bpp & -bpp); }
static int pb_check_frames(const pb_plan* plan, const void* src, const void* dst, int n_frames, int n, size_t& src_stride, size_t& dst_stride,
                           bool tables = false, int bpp = 3, bool wide = false) {
    if (!plan || ((!src || !dst) && (n_frames > 0 || !tables))) return pb_fail(PB_ERR_INVALID, "null argument");
    if (n_frames < 0) return pb_fail(PB_ERR_INVALID, "negative frame count");
    if (!pb_px_size_ok(bpp) && !(wide && (bpp == 12 || bpp == 16))) return pb_fail(PB_ERR_INVALID, "bytes_per_px outside {1, 2, 3, 4, 6, 8}");
    if (n_frames == 0) return PB_OK;
    const int rc = pb_check_device(plan);
    if (rc != PB_OK) return rc;
    const PbParams& P = plan->P;
    const unsigned long long B = (unsigned long long)bpp;
    const unsigned long long src_bytes = B * P.src.height * P.src.width, dst_bytes = B * ((unsigned)P.dst.height / n) * ((unsigned)P.dst.width / n);
    if (!src_stride) src_stride = src_bytes;
    if (!dst_stride) dst_stride = dst_bytes;
    if (dst_stride < dst_bytes) return pb_fail(PB_ERR_INVALID, "dst_frame_stride smaller than a frame");
    if (n_frames > 1 && src_stride < src_bytes) return pb_fail(PB_ERR_INVALID, "src_frame_stride smaller than a frame");
    const unsigned a = pb_px_align(bpp);  // (1 for three-byte pixels)
    if (!tables && ((((uintptr_t)src | (uintptr_t)dst) | src_stride | dst_stride) & (a - 1u)))
        return pb_fail(PB_ERR_INVALID, "frame pointers and strides must be multiples of " + std::to_string(a) + " bytes for " + std::to_string(bpp) + "-byte pixels");
    return PB_OK;
}

// The one routing decision: which kernels a remap call of `pl` launches (the table in DESIGN §3.7).  aligned: the source frames and
// their stride are 16-byte aligned (the window kernels' LDS-DMA row segments); n: the supersample factor (1: a plain call).
// What the plan builders guarantee, and the conditions below rely on: fast_ready is set for single sources only (pb_fast_possible),
// dbl_ready and sep_ready for double-fisheye sources only, dbl_ready for sources below 32768 px a side only (pb_fast_possible_dims);
// a launch table (nearest.lt / bil.lt) that holds its entries comes with groups >= 8 (PbLaunchTable: pb_build_launch_table moves both in together).
// What distinguishes the families of video entry points: NV12 / P010 frames - 4:2:0, planes 1 and 2 as one plane of
// interleaved pairs, laid out by a pb_nv12_layout - and planar frames at a subsampling (pb_planar_layout).  The words are the messages'.
struct PbVideoFmt {
    bool pairs = false;       // planes 1 and 2 are interleaved pairs
    int sub = PB_PLANAR_420;  // PB_PLANAR_* (pairs: 4:2:0)
    int S = 1;                // bytes per sample
    bool stitch = false;      // the stitch calls (pb_stitch_nv12 / pb_stitch_planar): a double-fisheye source, blended
    int cx() const { return pb_planar_cx(sub); }  // planes 1 and 2 are (h >> cy, w >> cx)
    int cy() const { return pb_planar_cy(sub); }
    unsigned long long unit() const { return (unsigned long long)(pairs ? 2 * S : S); }  // what pointers, pitches and offsets are multiples of
    const char* unit_name() const { return pairs ? "one chroma pair" : "one sample"; }
    const char* planes() const { return pairs ? "two" : "three"; }                       // "... and gather the two planes"
    std::string nearest() const { return pairs ? "pb_remap_nv12" : "pb_remap_planar"; }  // the nearest call, which the layout messages cite
    std::string stitch_name() const { return pairs ? "pb_stitch_nv12" : "pb_stitch_planar"; }
};
struct PbRoute {
    enum Kind {
        DOUBLE,              // nearest: pb_hot_double_kernel
        SEP,                 // nearest: pb_sep_double_kernel once its tables' check has passed (pb_sep_usable), else as FLOAT64
        WIN,                 // nearest: pb_hot_win_kernel
        DIRECT,              // nearest: pb_hot_kernel + pb_fix_kernel
        FLOAT64,             // nearest: pb_remap_kernel
        BIL_DOUBLE,          // bilinear: pb_bilinear_double_hot_kernel (+ pb_bilinear_double_fix_kernel without coordinate tables)
        INTERP_TILES,           // bilinear / catmull-rom: pb_bilinear_hot_kernel / pb_catmull_rom_hot_kernel (+ pb_interp_fix_kernel<filter> over the
                                // listed tiles and the fix pixels without coordinate tables)
        INTERP_FLOAT64,         // bilinear / catmull-rom: pb_interp_fix_kernel<filter> over every pixel
        INTERP_DOUBLE_FLOAT64,  // bilinear / catmull-rom: pb_interp_double_kernel<filter>
        SS_FUSED,            // supersampled: pb_ss_win_kernel
        SS_GENERIC,          // supersampled: frame by frame the route of n = 1 into a workspace, then pb_box_reduce_kernel
        PX,                  // nearest, pixels of bpp != 3 bytes (pb_remap_px): pb_px_hot_kernel
        PX_NONE,             // ... on a plan that kernel does not serve: nothing is launched (PB_ERR_UNSUPPORTED)
        PX_INTERP,           // bilinear / catmull-rom, pixels of (channels, sample_bytes) != (3, 1) (pb_remap_interp_px): pb_px_interp_kernel
        PX_INTERP_NEAREST_NONE,  // ... on a plan the nearest call refuses too - the plans of PX_NONE: nothing is launched (PB_ERR_UNSUPPORTED)
        PX_INTERP_FLOAT64,   // ... on a plan prepared for the bilinear mode whose coordinate tables cannot exist (a source of one or two pixels, of 2^18 px a side
                             // or more, a GiB of coordinates): the definition per pixel, pb_track_px_interp_kernel without a rotation per frame
        PX_INTERP_NONE,      // ... on a plan never prepared for the bilinear mode (a cube source never is): nothing is launched
        PXF_INTERP,          // bilinear / catmull-rom, pixels of 1 to 4 float16 or float32 samples (pb_remap_interp_pxf): pb_pxf_interp_kernel
        PXF_INTERP_NEAREST_NONE,  // ... on a plan the nearest call refuses too - the plans of PX_NONE: nothing is launched (PB_ERR_UNSUPPORTED)
        PXF_INTERP_NO_TABLES,     // ... on a plan prepared for the bilinear mode whose coordinate tables cannot exist (PX_INTERP_FLOAT64's plans): there is
                                  // no float64 per-pixel kernel for float samples, so nothing is launched
        PXF_INTERP_NONE,     // ... on a plan never prepared for the bilinear mode (a cube source never is): nothing is launched
        VIDEO,               // nearest, video frames: planar 4:4:4 / 4:2:2 / 4:2:0 (pb_remap_planar) and, as PAIRS, 4:2:0 semi-planar
                             // (pb_remap_nv12): pb_video_hot_kernel
        VIDEO_NONE,          // ... on a plan those kernels do not serve - the plans of PX_NONE: nothing is launched (PB_ERR_UNSUPPORTED)
        VIDEO_STITCH,        // nearest, video frames of a double-fisheye source (pb_stitch_nv12, pb_stitch_planar): pb_stitch_video_kernel
        VIDEO_STITCH_NONE,   // ... on a plan that kernel does not serve: nothing is launched (PB_ERR_UNSUPPORTED)
        VIDEO_BIL,           // bilinear, planar or 4:2:0 semi-planar frames (pb_remap_planar_bilinear, pb_remap_nv12_bilinear): pb_planar_bilinear_kernel
        VIDEO_BIL_NEAREST_NONE,  // ... on a plan the nearest call refuses too - the plans of PX_NONE: nothing is launched (PB_ERR_UNSUPPORTED)
        VIDEO_BIL_NONE,      // ... on a plan without the bilinear mode's tile and coordinate tables (a cube source never has them): nothing is launched
    } kind;
    bool windows;                    // BIL_DOUBLE / bilinear INTERP_TILES: LEAN tiles gather from LDS windows
    int filter = PB_INTERP_NEAREST;  // the INTERP_* routes: PB_INTERP_BILINEAR or PB_INTERP_CATMULL_ROM
    int bpp = 3;                     // PX, PX_INTERP: bytes per pixel
    PbVideoFmt video = {};           // VIDEO*: the frames' format
    int sample_bytes = 1;            // PX_INTERP, PXF_INTERP: bytes per sample (bpp / sample_bytes channels)
};
static bool pb_aligned16(const void* src, unsigned long long stride) { return ((((uintptr_t)src) | stride) & 15u) == 0; }
// video: the format of a video call's frames, null everywhere else; sample_bytes: of a pixel of bpp != 3 bytes that an interpolating call looks into;
// float_samples: those samples are IEEE binary16 / binary32 (pb_remap_interp_pxf; a pixel of three bytes cannot be one)
static PbRoute pb_route(const pb_plan* pl, int interpolation, int n, unsigned flags, bool aligned, int bpp = 3, const PbVideoFmt* video = nullptr,
                        int sample_bytes = 1, bool float_samples = false) {
    const PbParams& P = pl->P;
    if (bpp != 3 || video || float_samples) {
        // the tile kernel of the nearest plan's launch-order table, or nothing: no window, so no alignment beyond the pixel's own
        // (pb_check_frames); fast_ready says single source, prepared, device state; generic tiles pack row and column in 16 bits each
        const bool served = n == 1 && pb_use_fast(pl) && pl->nearest.lt.entries && pl->nearest.P_dev && P.src.width < 32768 && P.src.height < 32768;
        const bool px = interpolation == PB_INTERP_NEAREST && served;
        if (video && video->stitch) {
            // the double plan's own state, as pb_hot_double_kernel takes it - without the LDS windows, so no alignment and no window mode
            const bool stitched = n == 1 && interpolation == PB_INTERP_NEAREST && P.src.kind == PB_KIND_DOUBLE && pl->mode != PB_MODE_FAITHFUL && pl->cert.dbl_ready &&
                                  pl->nearest.lt.entries && P.src.width < 32768 && P.src.height < 32768;
            return {stitched ? PbRoute::VIDEO_STITCH : PbRoute::VIDEO_STITCH_NONE, false, PB_INTERP_NEAREST, 3, *video};
        }
        if (video && interpolation == PB_INTERP_BILINEAR) {
            // the nearest call's plans, and of those the ones with the bilinear mode's launch-order, tile and exact coordinate tables (no
            // second kernel picks up what a plan without coordinate tables leaves; a cube source never has bil.tiles: pb_bilinear_tiles_allowed)
            const bool tabs = pl->bil.lt.entries && pl->bil.tiles && pl->bil.xy && pl->bil.fix_xy && !pb_is_cube(P.src.kind);
            return {!served ? PbRoute::VIDEO_BIL_NEAREST_NONE : tabs ? PbRoute::VIDEO_BIL : PbRoute::VIDEO_BIL_NONE, false, PB_INTERP_BILINEAR, 3, *video};
        }
        if (video) return {px ? PbRoute::VIDEO : PbRoute::VIDEO_NONE, false, PB_INTERP_NEAREST, 3, *video};
        if (interpolation != PB_INTERP_NEAREST) {
            // the video frames' rule: the nearest call's plans, and of those the ones with the bilinear mode's tables.  A plan that was
            // prepared for the mode (its tile list exists) and holds no coordinate tables cannot have them (pb_build_bilinear_list): float64
            const bool prepared = pl->bil.tiles && !pb_is_cube(P.src.kind), tabs = prepared && pl->bil.lt.entries && pl->bil.xy && pl->bil.fix_xy;
            if (float_samples)  // the same plans; where the integer samples take the float64 chain, nothing
                return {!served ? PbRoute::PXF_INTERP_NEAREST_NONE : tabs ? PbRoute::PXF_INTERP : (prepared && !pl->bil.xy) ? PbRoute::PXF_INTERP_NO_TABLES : PbRoute::PXF_INTERP_NONE,
                        false, interpolation, bpp, {}, sample_bytes};
            return {!served ? PbRoute::PX_INTERP_NEAREST_NONE : tabs ? PbRoute::PX_INTERP : (prepared && !pl->bil.xy) ? PbRoute::PX_INTERP_FLOAT64 : PbRoute::PX_INTERP_NONE,
                    false, interpolation, bpp, {}, sample_bytes};
        }
        return {px ? PbRoute::PX : PbRoute::PX_NONE, false, PB_INTERP_NEAREST, bpp};
    }
    if (n > 1) {
        const bool fused = interpolation == PB_INTERP_NEAREST && !(flags & PB_SS_GENERIC) && pb_route(pl, interpolation, 1, 0, aligned).kind == PbRoute::WIN;
        return {fused ? PbRoute::SS_FUSED : PbRoute::SS_GENERIC, false};
    }
    const bool tiled = pl->mode != PB_MODE_FAITHFUL;
    const bool windows = pl->mode != PB_MODE_FAST_DIRECT && P.src.width < 32768 && P.src.height < 32768 && aligned;
    if (interpolation == PB_INTERP_BILINEAR || interpolation == PB_INTERP_CATMULL_ROM) {
        // (catmull-rom runs on the bilinear mode's tables: no LDS windows, no tile kernel for two eyes)
        const bool bil = interpolation == PB_INTERP_BILINEAR;
        if (P.src.kind == PB_KIND_DOUBLE)
            return (bil && tiled && pl->cert.dbl_ready && pl->bil.lt.entries && pl->bil.tiles && pl->bil.dbl_tables)
                       ? PbRoute{PbRoute::BIL_DOUBLE, windows, interpolation}
                       : PbRoute{PbRoute::INTERP_DOUBLE_FLOAT64, false, interpolation};
        // (a cube source never has bil.tiles - pb_bilinear_tiles_allowed - and so takes INTERP_FLOAT64: the definition per pixel on the selected face)
        return (pb_use_fast(pl) && pl->bil.lt.entries && pl->bil.tiles) ? PbRoute{PbRoute::INTERP_TILES, bil && windows, interpolation}
                                                                    : PbRoute{PbRoute::INTERP_FLOAT64, false, interpolation};
    }
    if (tiled && pl->cert.dbl_ready && pl->nearest.lt.entries && windows) return {PbRoute::DOUBLE, true};
    if (tiled && pl->cert.sep_ready) return {PbRoute::SEP, false};
    if (pb_use_fast(pl) && pl->nearest.lt.entries && pl->nearest.P_dev && windows) return {PbRoute::WIN, true};
    if (pb_use_fast(pl)) return {PbRoute::DIRECT, false};
    return {PbRoute::FLOAT64, false};
}

// the double-fisheye kernels' WMODE: 1 the separable path's exact row weights, 2 stored merge-band latitudes, 0 neither
static const PbSepRow* pb_sep_rows(const pb_plan* pl) { return pl->cert.sep_ready ? pl->cert.sep_rows : nullptr; }
template <class F>
static void pb_pick_wmode(const pb_plan* pl, F&& f) {
    if (pb_sep_rows(pl)) f(PbInt<1>());
    else if (pl->cert.n_lat_tiles) f(PbInt<2>());
    else f(PbInt<0>());
}
// Frames are a grid dimension of the tile launches: a batch goes in launches of at most 0x7FFFFFFF / gpf frames (gpf: workgroups per
// frame), launch(src, dst, frames) with the pointers of each piece's first frame.
template <class F>
static void pb_each_launch(const uint8_t* src, uint8_t* dst, int n_frames, unsigned long long ss, unsigned long long ds, unsigned gpf, F&& launch) {
    const int per_launch = (int)(0x7FFFFFFFu / gpf);
    for (int f0 = 0; f0 < n_frames; f0 += per_launch)
        launch(src + (unsigned long long)f0 * ss, dst + (unsigned long long)f0 * ds, n_frames - f0 < per_launch ? n_frames - f0 : per_launch);
}
// the rotation tracks' launch loop (defined with them, below): PX_INTERP_FLOAT64 launches through it
extern "C++" template <class LAUNCH>
static int pb_track_launch(int n_frames, const double* rot3x3_dev, int n_rot_per_frame, const void* src, void* dst, size_t src_stride, size_t dst_stride, LAUNCH launch);
// real workgroups per frame of a bilinear tile launch
static unsigned pb_bil_groups(const pb_plan* pl) { return pl->bil.lt.groups * (4u / (unsigned)pl->bil.waves); }

// the direct-gather hot kernel + the fix kernel; OUT 0 = frames, OUT 1 = int32 index map
template <int OUT>
static void pb_launch_direct(const pb_plan* pl, const uint8_t* src, uint8_t* dst, int n_frames, unsigned long long ss, unsigned long long ds,
                             int32_t* idx_out, hipStream_t st) {
    const PbParams& P = pl->P;
    pb_pick_kind(P, [&](auto K) {
        hipLaunchKernelGGL((pb_hot_kernel<K.value, OUT>), dim3(pb_hot_blocks(P)), dim3(64 * PB_TILE_WAVES), 0, st, P, pl->cert.table, src, dst, n_frames, ss, ds, idx_out);
    });
    const unsigned fix_blocks = 4u * pl->cert.n_fail_tiles + (pl->cert.n_fix_px + PB_BLOCK - 1) / PB_BLOCK;
    if (fix_blocks)
        hipLaunchKernelGGL((pb_fix_kernel<OUT>), dim3(fix_blocks), dim3(PB_BLOCK), 0, st, P, pl->cert.fail_tiles, (int)pl->cert.n_fail_tiles, pl->cert.fix_px,
                           (int)pl->cert.n_fix_px, pl->cert.idx_tab, pl->cert.fix_idx, src, dst, n_frames, ss, ds, idx_out);
}

// Launches a nearest or bilinear route (n = 1) for n_frames frames at strides ss / ds (pb_check_frames has filled them in).
// video: the plane layouts and fills of the VIDEO and VIDEO_BIL routes (an NV12 layout travels as a PbPlanar: pb_video.hpp), null everywhere else.
static int pb_launch(const pb_plan* pl, PbRoute r, const uint8_t* src, uint8_t* dst, int n_frames, unsigned long long ss, unsigned long long ds,
                     hipStream_t st, const PbPlanar* video = nullptr) {
    const PbParams& P = pl->P;
    const unsigned long long npx = (unsigned long long)P.dst.height * P.dst.width;
    switch (r.kind) {
        case PbRoute::DOUBLE: {
            // failed tiles and fix pixels go through the plan's stored faithful taps
            static const int fpw_env = pb_knob("PB_DOUBLE_FPW", 0);
            const int fpw = fpw_env > 0 ? fpw_env : PB_DOUBLE_FRAMES_PER_WAVE;
            const unsigned gpf = pl->nearest.lt.groups;  // workgroups per frame of the plan's launch-order table
            const dim3 grid(gpf * (unsigned)((n_frames + fpw - 1) / fpw));  // (h*w < 2^29 and n_frames an int: far below the grid limit for any batch that fits memory)
            pb_pick_wmode(pl, [&](auto W) {
                pb_pick<1, 0>(n_frames == 1 || fpw == 1, [&](auto ONE) {
                    hipLaunchKernelGGL((pb_hot_double_kernel<W.value, ONE.value != 0>), grid, dim3(64 * PB_TILE_WAVES), pb_window_lds_bytes(P, 8), st, P, pl->cert.table,
                                       pl->cert.table_r, pl->nearest.lt.entries, pb_sep_rows(pl), pl->cert.lat_tab, pl->cert.fix_px, pl->cert.dbl_px_fix, pl->cert.dbl_tile_fix, src, dst, n_frames, ss,
                                       ds, gpf, fpw, PbNoFrameTab{0});
                });
            });
            break;
        }
        case PbRoute::SEP:
            if (pb_sep_usable(pl, st)) {
                hipLaunchKernelGGL(pb_sep_double_kernel, dim3(pb_hot_blocks(P)), dim3(64 * PB_TILE_WAVES), 0, st, P, pl->cert.sep_rows, pl->cert.sep_cols, src, dst,
                                   n_frames, ss, ds);
                break;
            }
            [[fallthrough]];
        case PbRoute::FLOAT64: {
            const int dst_aligned = (((uintptr_t)dst | ds) & 3u) == 0;
            pb_pick_any_kind(P, [&](auto K) {
                PB_LAUNCH_BY_ROT(P, pb_remap_kernel, K.value, dim3(pb_blocks((npx + PB_PX - 1) / PB_PX)), dim3(PB_BLOCK), 0, st, P, src, dst, n_frames,
                                 ss, ds, dst_aligned);
            });
            break;
        }
        case PbRoute::WIN: {
            // failed tiles and fix pixels are looked up in the plan's exact-index tables by the hot waves themselves (pb_kernels_tile.hpp);
            // a frame's share of the grid is a multiple of 8 workgroups so that a tile group keeps its XCD residue in every frame
            const unsigned gpf = pl->nearest.lt.groups;
            pb_each_launch(src, dst, n_frames, ss, ds, gpf, [&](const uint8_t* sf, uint8_t* df, int nf) {
                pb_pick_kind(P, [&](auto K) {
                    hipLaunchKernelGGL((pb_hot_win_kernel<K.value>), dim3(gpf * (unsigned)nf), dim3(64 * PB_TILE_WAVES), pb_window_lds_bytes(P), st,
                                       (const PbParams*)pl->nearest.P_dev, pb_hot_of_host(P), pl->nearest.lt.entries, sf, df, gpf, ss, ds, pl->cert.idx_tab, pl->cert.fix_px, pl->cert.fix_idx,
                                       (unsigned)nf, PbNoFrameTab{0});
                });
            });
            break;
        }
        case PbRoute::DIRECT:
            pb_launch_direct<0>(pl, src, dst, n_frames, ss, ds, nullptr, st);
            break;
        case PbRoute::PX: {
            // launched like WIN: the nearest launch-order table, frames of a batch as a grid dimension; static LDS (the regrouping buffer)
            const unsigned gpf = pl->nearest.lt.groups;
            pb_each_launch(src, dst, n_frames, ss, ds, gpf, [&](const uint8_t* sf, uint8_t* df, int nf) {
                pb_pick_kind(P, [&](auto K) {
                    pb_pick_px_size(r.bpp, [&](auto B) {
                        hipLaunchKernelGGL((pb_px_hot_kernel<K.value, B.value>), dim3(gpf * (unsigned)nf), dim3(64 * PB_TILE_WAVES), 0, st,
                                           (const PbParams*)pl->nearest.P_dev, pb_hot_of_host(P), pl->nearest.lt.entries, sf, df, gpf, ss, ds, pl->cert.idx_tab,
                                           pl->cert.fix_px, pl->cert.fix_idx);
                    });
                });
            });
            break;
        }
        case PbRoute::PX_NONE:
            return pb_fail(PB_ERR_UNSUPPORTED, "pb_remap_px takes prepared plans of a single source in a tile mode (not deferred, not PB_MODE_FAITHFUL, not "
                                               "double-fisheye, sources below 32768 px a side): use pb_index_map_i32 + pb_gather_px");
        case PbRoute::PX_INTERP: {
            // launched like VIDEO_BIL: the bilinear mode's launch-order table read with four waves per workgroup; static LDS (the regrouping planes)
            const unsigned gpf = pl->bil.lt.groups;
            pb_each_launch(src, dst, n_frames, ss, ds, gpf, [&](const uint8_t* sf, uint8_t* df, int nf) {
                pb_pick_kind(P, [&](auto K) {
                    pb_pick<PB_PXI_BILINEAR, PB_PXI_CATMULL_ROM>(r.filter == PB_INTERP_BILINEAR, [&](auto F) {
                        pb_pick_px_format(r.bpp / r.sample_bytes, r.sample_bytes, [&](auto C, auto S) {
                            hipLaunchKernelGGL((pb_px_interp_kernel<K.value, F.value, C.value, S.value>), dim3(gpf * (unsigned)nf), dim3(64 * PB_PXI_WAVES), 0, st,
                                               pb_hot_of_host(P), pl->bil.lt.entries, sf, df, gpf, ss, ds, pl->bil.xy, pl->cert.fix_px, pl->bil.fix_xy);
                        });
                    });
                });
            });
            break;
        }
        case PbRoute::PX_INTERP_NEAREST_NONE:
            return pb_fail(PB_ERR_UNSUPPORTED, "pb_remap_interp_px takes prepared plans of a single source in a tile mode (not deferred, not PB_MODE_FAITHFUL, not "
                                               "double-fisheye, sources below 32768 px a side): use pb_sample_map_bilinear_px / pb_sample_map_catmull_rom_px");
        case PbRoute::PX_INTERP_NONE:
            if (pb_is_cube(P.src.kind))
                return pb_fail(PB_ERR_UNSUPPORTED, "pb_remap_interp_px takes camera and panorama sources (a cube source has no interpolating tile kernel): use "
                                                   "pb_sample_map_bilinear_px / pb_sample_map_catmull_rom_px");
            return pb_fail(PB_ERR_UNSUPPORTED, "pb_remap_interp_px needs the bilinear mode's tile and coordinate tables: call pb_plan_prepare(plan, PB_PLAN_BILINEAR) first");
        case PbRoute::PX_INTERP_FLOAT64: {
            // the float64 chain per pixel: pb_remap_track_px's interpolating launch with no rotation per frame (no table is read), frames
            // chunked over the grid's y by the rotation tracks' launch loop
            const int channels = r.bpp / r.sample_bytes;
            return pb_track_launch(n_frames, nullptr, 0, src, dst, ss, ds, [&](const double* rot, const uint8_t* sf, uint8_t* df, int nf, unsigned chunks, int fpc) {
                const auto launch = [&](auto K, auto* sample) {  // (the sample type: uint8_t or uint16_t)
                    using SAMPLE = std::remove_pointer_t<decltype(sample)>;
                    pb_pick_filter(r.filter, [&](auto F) {
                        hipLaunchKernelGGL((pb_track_px_interp_kernel<K.value, decltype(F), SAMPLE>), dim3(pb_blocks(npx), chunks), dim3(PB_BLOCK), 0, st, P, rot, 0, fpc, sf, df, nf,
                                           ss, ds, channels);
                    });
                };
                if (r.sample_bytes == 1) pb_pick_kind(P, [&](auto K) { launch(K, (uint8_t*)nullptr); });
                else pb_pick_kind(P, [&](auto K) { launch(K, (uint16_t*)nullptr); });
            });
        }
        case PbRoute::PXF_INTERP: {
            // launched like PX_INTERP; static LDS: one regrouping plane per dword of the pixel
            const unsigned gpf = pl->bil.lt.groups;
            pb_each_launch(src, dst, n_frames, ss, ds, gpf, [&](const uint8_t* sf, uint8_t* df, int nf) {
                pb_pick_kind(P, [&](auto K) {
                    pb_pick<PB_PXI_BILINEAR, PB_PXI_CATMULL_ROM>(r.filter == PB_INTERP_BILINEAR, [&](auto F) {
                        pb_pick_pxf_format(r.bpp / r.sample_bytes, r.sample_bytes, [&](auto C, auto S) {
                            hipLaunchKernelGGL((pb_pxf_interp_kernel<K.value, F.value, C.value, S.value>), dim3(gpf * (unsigned)nf), dim3(64 * PB_PXI_WAVES), 0, st,
                                               pb_hot_of_host(P), pl->bil.lt.entries, sf, df, gpf, ss, ds, pl->bil.xy, pl->cert.fix_px, pl->bil.fix_xy);
                        });
                    });
                });
            });
            break;
        }
        case PbRoute::PXF_INTERP_NEAREST_NONE:
            return pb_fail(PB_ERR_UNSUPPORTED, "pb_remap_interp_pxf takes prepared plans of a single source in a tile mode (not deferred, not PB_MODE_FAITHFUL, not "
                                               "double-fisheye, sources below 32768 px a side): float frames have no other device route");
        case PbRoute::PXF_INTERP_NO_TABLES:
            return pb_fail(PB_ERR_UNSUPPORTED, "pb_remap_interp_pxf needs the bilinear mode's coordinate tables, and the tables cannot exist for this source (one or two "
                                               "pixels, 2^18 px a side or more, or a GiB of coordinates): float frames have no per-pixel route");
        case PbRoute::PXF_INTERP_NONE:
            if (pb_is_cube(P.src.kind))
                return pb_fail(PB_ERR_UNSUPPORTED, "pb_remap_interp_pxf takes camera and panorama sources (a cube source has no interpolating tile kernel)");
            return pb_fail(PB_ERR_UNSUPPORTED, "pb_remap_interp_pxf needs the bilinear mode's tile and coordinate tables: call pb_plan_prepare(plan, PB_PLAN_BILINEAR) first");
        case PbRoute::VIDEO: {
            // launched like PX: every plane of a tile by the tile's wave
            const unsigned gpf = pl->nearest.lt.groups;
            pb_each_launch(src, dst, n_frames, ss, ds, gpf, [&](const uint8_t* sf, uint8_t* df, int nf) {
                pb_pick_kind(P, [&](auto K) {
                    pb_pick<1, 2>(r.video.S == 1, [&](auto S) {
                        auto go = [&](auto SUB, auto PAIRS) {
                            hipLaunchKernelGGL((pb_video_hot_kernel<K.value, S.value, SUB.value, PAIRS.value != 0>), dim3(gpf * (unsigned)nf), dim3(64 * PB_TILE_WAVES), 0, st,
                                               (const PbParams*)pl->nearest.P_dev, pb_hot_of_host(P), pl->nearest.lt.entries, sf, df, gpf, ss, ds, pl->cert.idx_tab,
                                               pl->cert.fix_px, pl->cert.fix_idx, *video);
                        };
                        if (r.video.pairs) go(PbInt<PB_SUB_420>(), PbInt<1>());
                        else pb_pick_subsampling(r.video.sub, [&](auto SUB) { go(SUB, PbInt<0>()); });
                    });
                });
            });
            break;
        }
        case PbRoute::VIDEO_NONE:
            return pb_fail(PB_ERR_UNSUPPORTED, r.video.nearest() + " takes prepared plans of a single source in a tile mode (not deferred, not PB_MODE_FAITHFUL, not "
                                               "double-fisheye, sources below 32768 px a side): use pb_index_map_i32 and gather the " + r.video.planes() + " planes");
        case PbRoute::VIDEO_STITCH: {
            // launched like DOUBLE's single-frame form, frames of a batch as a grid dimension; static LDS (the regrouping buffer)
            const unsigned gpf = pl->nearest.lt.groups;
            pb_each_launch(src, dst, n_frames, ss, ds, gpf, [&](const uint8_t* sf, uint8_t* df, int nf) {
                pb_pick<1, 2>(r.video.S == 1, [&](auto S) {
                    auto go = [&](auto SUB, auto PAIRS) {
                        hipLaunchKernelGGL((pb_stitch_video_kernel<S.value, SUB.value, PAIRS.value != 0>), dim3(gpf * (unsigned)nf), dim3(64 * PB_TILE_WAVES), 0, st, P,
                                           pl->cert.table, pl->cert.table_r, pl->nearest.lt.entries, pb_sep_rows(pl), pl->cert.lat_tab, pl->cert.fix_px, pl->cert.dbl_px_fix,
                                           pl->cert.dbl_tile_fix, sf, df, gpf, ss, ds, *video);
                    };
                    if (r.video.pairs) go(PbInt<PB_SUB_420>(), PbInt<1>());
                    else pb_pick_subsampling(r.video.sub, [&](auto SUB) { go(SUB, PbInt<0>()); });
                });
            });
            break;
        }
        case PbRoute::VIDEO_STITCH_NONE:
            if (P.src.kind != PB_KIND_DOUBLE)
                return pb_fail(PB_ERR_UNSUPPORTED, r.video.stitch_name() + " takes double-fisheye sources: use " + r.video.nearest() + " for a single source");
            return pb_fail(PB_ERR_UNSUPPORTED, r.video.stitch_name() + " takes prepared double-fisheye plans in a tile mode (not deferred, not PB_MODE_FAITHFUL, with both eyes' "
                                               "tile tables and a launch-order table, sources below 32768 px a side): use pb_index_map_i32 with weights and "
                                               "pb_gather_blend_u8 per plane");
        case PbRoute::VIDEO_BIL: {
            // launched like the Catmull-Rom tile kernel: the bilinear mode's launch-order table read with four waves per workgroup
            const unsigned gpf = pl->bil.lt.groups;
            pb_each_launch(src, dst, n_frames, ss, ds, gpf, [&](const uint8_t* sf, uint8_t* df, int nf) {
                pb_pick_kind(P, [&](auto K) {
                    pb_pick<1, 2>(r.video.S == 1, [&](auto S) {
                        auto go = [&](auto SUB, auto PAIRS) {
                            hipLaunchKernelGGL((pb_planar_bilinear_kernel<K.value, S.value, SUB.value, PAIRS.value != 0>), dim3(gpf * (unsigned)nf), dim3(64 * PB_VBIL_WAVES),
                                               0, st, pb_hot_of_host(P), pl->bil.lt.entries, sf, df, gpf, ss, ds, pl->bil.xy, pl->cert.fix_px, pl->bil.fix_xy, *video);
                        };
                        if (r.video.pairs) go(PbInt<PB_SUB_420>(), PbInt<1>());
                        else pb_pick_subsampling(r.video.sub, [&](auto SUB) { go(SUB, PbInt<0>()); });
                    });
                });
            });
            break;
        }
        case PbRoute::VIDEO_BIL_NEAREST_NONE:
        case PbRoute::VIDEO_BIL_NONE: {
            const std::string name = r.video.nearest() + "_bilinear";
            if (r.kind == PbRoute::VIDEO_BIL_NEAREST_NONE)
                return pb_fail(PB_ERR_UNSUPPORTED, name + " takes prepared plans of a single source in a tile mode (not deferred, not PB_MODE_FAITHFUL, not "
                                                          "double-fisheye, sources below 32768 px a side): convert to RGB and use pb_remap_bilinear_u8");
            if (pb_is_cube(P.src.kind))
                return pb_fail(PB_ERR_UNSUPPORTED, name + " takes camera and panorama sources (a cube source has no interpolating tile kernel): convert to RGB and use "
                                                          "pb_remap_bilinear_u8");
            return pb_fail(PB_ERR_UNSUPPORTED, name + " needs the bilinear mode's tile and coordinate tables: call pb_plan_prepare(plan, PB_PLAN_BILINEAR) first");
        }
        case PbRoute::BIL_DOUBLE: {
            // the per-eye tile models of the nearest mode's plan + the exact coordinate tables: one wave per tile
            const unsigned gpf = pb_bil_groups(pl);
            PbHot Hb = pb_hot_of_host(P);  // (the bilinear mode's window budget travels in it)
            Hb.win_budget = pl->bil.budget;
            pb_each_launch(src, dst, n_frames, ss, ds, gpf, [&](const uint8_t* sf, uint8_t* df, int nf) {
                pb_pick_wmode(pl, [&](auto W) {
                    pb_pick<2, 4>(pl->bil.waves == 2, [&](auto WAVES) {
                        hipLaunchKernelGGL((pb_bilinear_double_hot_kernel<W.value, WAVES.value>), dim3(gpf * (unsigned)nf), dim3(64 * pl->bil.waves),
                                           (size_t)pl->bil.pool_bytes, st, Hb, P.src_eye_w, pl->bil.lt.entries, pl->bil.dbl_tables, sf, df, gpf, ss, ds,
                                           (int)r.windows, pl->bil.xy);
                    });
                });
            });
            if (!pl->bil.xy) {  // no coordinate tables (they would not fit): the failed / listed tiles and the fix pixels from the float64 chain
                const unsigned n_tiles64 = pl->cert.n_fail_tiles + pl->bil.n_tiles;
                const unsigned fix_blocks = 4u * n_tiles64 + (pl->cert.n_fix_px + PB_BLOCK - 1) / PB_BLOCK;
                if (fix_blocks)
                    hipLaunchKernelGGL(pb_bilinear_double_fix_kernel, dim3(fix_blocks), dim3(PB_BLOCK), 0, st, P, pl->cert.fail_tiles, (int)pl->cert.n_fail_tiles,
                                       pl->bil.tiles, (int)n_tiles64, pl->cert.fix_px, (int)pl->cert.n_fix_px, src, dst, n_frames, ss, ds);
            }
            break;
        }
        case PbRoute::INTERP_DOUBLE_FLOAT64:
            pb_pick_filter(r.filter, [&](auto F) {
                hipLaunchKernelGGL(pb_interp_double_kernel<decltype(F)>, dim3(pb_blocks(npx)), dim3(PB_BLOCK), 0, st, P, src, dst, n_frames, ss, ds);
            });
            break;
        case PbRoute::INTERP_TILES:
            // launched like the nearest hot kernel: the bilinear mode's launch-order table, frames of a batch as a grid dimension
            pb_pick_kind(P, [&](auto K) {
                if (r.filter == PB_INTERP_CATMULL_ROM) {  // the table read with four waves per workgroup: bil.lt.groups workgroups per frame
                    const unsigned gpf = pl->bil.lt.groups;
                    pb_each_launch(src, dst, n_frames, ss, ds, gpf, [&](const uint8_t* sf, uint8_t* df, int nf) {
                        hipLaunchKernelGGL((pb_catmull_rom_hot_kernel<K.value>), dim3(gpf * (unsigned)nf), dim3(64 * PB_CR_WAVES), 0, st, pb_hot_of_host(P),
                                           pl->bil.lt.entries, sf, df, gpf, ss, ds, pl->bil.xy, pl->cert.fix_px, pl->bil.fix_xy);
                    });
                } else {
                    const unsigned gpf = pb_bil_groups(pl);
                    PbParams Pb = P;
                    Pb.win_budget = pl->bil.budget;
                    pb_each_launch(src, dst, n_frames, ss, ds, gpf, [&](const uint8_t* sf, uint8_t* df, int nf) {
                        pb_pick<2, 4>(pl->bil.waves == 2, [&](auto WAVES) {
                            hipLaunchKernelGGL((pb_bilinear_hot_kernel<K.value, WAVES.value>), dim3(gpf * (unsigned)nf), dim3(64 * pl->bil.waves),
                                               (size_t)pl->bil.pool_bytes, st, pb_hot_of_host(Pb), pl->bil.lt.entries, sf, df, gpf, ss, ds, (int)r.windows,
                                               pl->bil.xy, pl->cert.fix_px, pl->bil.fix_xy);
                        });
                    });
                }
                const unsigned n64 = pl->cert.n_fail_tiles + pl->bil.n_tiles;  // failed + listed tiles
                if (!pl->bil.xy && (n64 || pl->cert.n_fix_px))  // no coordinate tables (they would not fit): the float64 chain
                    pb_pick_filter(r.filter, [&](auto F) {
                        hipLaunchKernelGGL((pb_interp_fix_kernel<decltype(F), K.value>), dim3(4u * n64 + (pl->cert.n_fix_px + PB_BLOCK - 1) / PB_BLOCK),
                                           dim3(PB_BLOCK), 0, st, P, pl->cert.fail_tiles, 0, src, dst, n_frames, ss, ds, (int)n64, pl->cert.fix_px, (int)pl->cert.n_fix_px,
                                           pl->bil.tiles, (int)pl->cert.n_fail_tiles);
                    });
            });
            break;
        case PbRoute::INTERP_FLOAT64:
            if (pb_is_cube(P.src.kind)) {
                pb_pick_cube_kind(P, [&](auto K) {
                    pb_pick_filter(r.filter, [&](auto F) {
                        hipLaunchKernelGGL((pb_interp_cube_kernel_of<K.value, decltype(F)>()), dim3(pb_blocks(npx)), dim3(PB_BLOCK), 0, st, P, src, dst, n_frames, ss, ds);
                    });
                });
                break;
            }
            pb_pick_kind(P, [&](auto K) {
                pb_pick_filter(r.filter, [&](auto F) {
                    hipLaunchKernelGGL((pb_interp_fix_kernel<decltype(F), K.value>), dim3(pb_blocks(npx)), dim3(PB_BLOCK), 0, st, P, nullptr, 1, src, dst,
                                       n_frames, ss, ds);
                });
            });
            break;
        default:
            return pb_fail(PB_ERR_INVALID, "not a route of one frame");  // (the supersampled routes: pb_remap_ss_u8)
    }
    PB_HIP(hipGetLastError());
    return PB_OK;
}

// The LDS window budget of a plan (bytes per wave).  Smaller windows let more workgroups share a CU (the hot
// kernels are latency x concurrency bound) but push tiles with larger windows onto the direct-gather path; which
// side wins depends on the geometry.  The classification only decides the PATH a tile takes, never its pixels
// (same model, same anchors, same tables), so a budget change cannot change a byte.
#define PB_DEFAULT_EXP 0
#define PB_DEFAULT_WIN_BUDGET 7168  // 5 workgroups per CU: fastest or within noise of the fastest on every BASELINE geometry (round-2 sweep r2o / r2p:
                                    // c1 14.3 us vs 15.1-16 elsewhere, c3 38.4, c5 86.4, c2 flat 44.1-44.6 from 7 to 12 KiB, batches 33.0-33.5 vs 34.9 at 12 KiB)
static int pb_clamp_budget(int budget) {
    budget &= ~15;
    if (budget < PB_DIRECT_LDS_BYTES) budget = PB_DIRECT_LDS_BYTES;
    if (budget > PB_WINLDS_MAX) budget = PB_WINLDS_MAX;
    return budget;
}

// The hot kernel's launch order: the tile entries copied into the order the waves of a launch take them, so that a
// wave's entry is found by its slot (no tile arithmetic) and the order is the plan's to choose.  Workgroup ids keep
// their XCD residue (round-robin dispatch); where the grid divides into 256x256-px super-tiles (16 workgroups), XCD x
// takes the super-tiles x, x + 8, ... of a ROW of super-tiles, and the chip walks through the rows together (every
// order that gave each XCD its own compact region - row bands, column strips, a Hilbert curve cut into eight - measured
// 5-15 % slower, in batches too, and so did every order that broke a column's vertical neighbours apart).  Which row comes
// next is the plan's choice: a launch that ENDS on its cheapest rows drains faster.  Where the rows differ (a fisheye
// output: black corners above and below, the dense centre between), the walk starts at the heaviest row and moves
// outwards on two fronts, heavier neighbour first: c2 44.1 -> 41.8 us (ending on the centre rows instead: 46.7).  Rows
// of even cost keep the plain top-to-bottom order (two fronts cost c3 10 %, c1 2 %) unless their SUPER-TILES differ (clusters of
// failed and direct-gather tiles): then the super-tiles go heaviest first, dealt round-robin (c3 37.9 -> 35.1 us).  Double-fisheye
// plans walk top to bottom and let columns of super-tiles change XCD when one XCD runs ahead (the policy is spelled out where it
// is applied, below).  -DPB_ABLATION builds: PB_ORDER=1 forces top-to-bottom.  Synchronous.
// class_dev / class_out: the budget pass's counters still on the device (pb_classify_under_budget keep_dev) and where their first two
// words go - fetched with the cost pass's readback when there is one, by themselves otherwise.
static int pb_build_launch_table(pb_plan* pl, const bool bil = false, const unsigned* class_dev = nullptr, unsigned* class_out = nullptr) {
    PbParams& P = pl->P;
    PbLaunchTable& out = bil ? pl->bil.lt : pl->nearest.lt;
    // every failure exit: the plan's old table goes (it may be classified under another budget), the error is reported
    const auto fail = [&](const std::string& msg) {
        pb_drain_and_drop(pl, out);
        return pb_fail(PB_ERR_HIP, msg);
    };
    if (!pl->cert.fast_ready && !pl->cert.dbl_ready) return PB_OK;  // (a double-fisheye plan: the left eye's table + PB_TILE_SOLO entries)
    const unsigned tiles_x = (P.dst.width + PB_TILE - 1) / PB_TILE, tiles_y = (P.dst.height + PB_TILE - 1) / PB_TILE;
    const unsigned gx = (tiles_x + 1) / 2, gy = (tiles_y + 1) / 2;
    static const unsigned U = [] { const int v = pb_knob("PB_UNIT", 4); return (v == 2 || v == 8 || v == 16) ? (unsigned)v : 4u; }();  // workgroups per unit side
    static const unsigned UYk = [] { const int v = pb_knob("PB_UNIT_Y", 0); return (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) ? (unsigned)v : 0u; }();  // experiments: unit height in workgroups (0: square)
    const unsigned UY = UYk ? UYk : U;
    const bool units = gx % U == 0 && gy % UY == 0 && (gx / U) * (gy / UY) >= 16u;
    static const int order_mode = pb_knob("PB_ORDER", 0);
    std::vector<int> unit_of;
    int units_per_xcd = 0;
    unsigned n_groups = (gx * gy + 7u) & ~7u;
    if (units) {
        const unsigned sgx = gx / U, sgy = gy / UY, ns = sgx * sgy;
        units_per_xcd = (int)((ns + 7u) / 8u);
        n_groups = 8u * (unsigned)units_per_xcd * U * UY;
        // the walk: rows of super-tiles top to bottom, XCD = position in the walk mod 8 (plain), unless the plan's tiles say
        // that work is unevenly spread - then the launch starts on its heaviest part and ENDS on its cheapest, which drains fast:
        //   rows differ (max / min > 1.45; a fisheye output's black-cornered edges against its dense centre, a panorama's
        //   pole rows against its rim rows): from the heaviest row outwards on two fronts, heavier neighbour first - the chip
        //   still walks through whole rows together (c2 44.1 -> 41.8 us, c1 14.1 -> 13.0);
        //   rows alike but super-tiles differ (max / mean > 1.7; clusters of failed and direct-gather tiles): super-tiles
        //   heaviest first, dealt round-robin (c3 37.9 -> 35.1 us, batches 32.0 -> 30.7).
        // Cost of a tile from its class and window: a wave's measured life (experiments/diag_trace.py) is 3 us on a black tile,
        // 4.2 + 0.4 per KiB of window on a window tile, 9.5 + 0.03 per source column on a direct-gather tile.
        std::vector<unsigned> seq(ns);  // the walk: super-tile ids in launch order
        for (unsigned S = 0; S < ns; ++S) seq[S] = S;
        std::vector<float> unit_cost;
        bool row_walk = true;  // seq is a sequence of whole rows
        const int walk = (order_mode >= 1 && order_mode <= 3) ? order_mode : pl->walk;  // (PB_ORDER=1 / 2 / 3, diagnostic build: force the plain walk / rows outwards / heaviest first)
        if (walk != 1 && sgy >= 4 && (ns >= 128u || walk != 0)) {  // (fewer than 16 super-tiles per XCD: too coarse to reorder - a 3072x2048 output measured 3-4 % slower)
            std::vector<unsigned> fixed(ns + 4u, 0u);
            PbBlock<unsigned> cost_dev;
            if (cost_dev.alloc(ns + 4u) != hipSuccess) return fail("launch table: out of device memory");
            (void)hipMemsetAsync(cost_dev, 0, ns * sizeof(unsigned), 0);
            hipLaunchKernelGGL(pb_unit_cost_kernel, dim3((pl->cert.n_tiles + 255) / 256), dim3(256), 0, 0, pl->cert.table, pl->cert.n_tiles, tiles_x, 2u * U, sgx, cost_dev,
                               pl->cert.dbl_ready ? pl->cert.table_r : nullptr, 2u * UY, bil ? 1 : 0, class_dev, ns);
            PB_STAGE("lt-host0");
            const hipError_t ce = hipMemcpy(fixed.data(), cost_dev, (ns + (class_dev ? 4u : 0u)) * sizeof(unsigned), hipMemcpyDeviceToHost);
            if (class_dev && class_out && ce == hipSuccess) {
                class_out[0] = fixed[ns];
                class_out[1] = fixed[ns + 1];
                class_dev = nullptr;  // (delivered)
            }
            PB_STAGE("lt-cost-readback");
            if (ce != hipSuccess) {
                (void)hipDeviceSynchronize();
                return fail(std::string("launch table: ") + hipGetErrorString(ce));
            }
            std::vector<float> row_cost(sgy, 0.f);
            unit_cost.assign(ns, 0.f);
            for (unsigned S = 0; S < ns; ++S) {
                unit_cost[S] = (float)fixed[S] / 1024.0f;
                row_cost[S / sgx] += unit_cost[S];
            }
            const float rmax = *std::max_element(row_cost.begin(), row_cost.end()), rmin = *std::min_element(row_cost.begin(), row_cost.end());
            const float umax = *std::max_element(unit_cost.begin(), unit_cost.end());
            float usum = 0.f;
            for (float c : unit_cost) usum += c;
            if (walk == 0 && pl->cert.dbl_ready) {
                // double-fisheye sources keep the plain walk (two fronts measured 1.5 % slower on c5); their problem is another one, below
            } else if (walk == 2 || (walk == 0 && rmax > 1.45f * rmin)) {
                const unsigned top = (unsigned)(std::max_element(row_cost.begin(), row_cost.end()) - row_cost.begin());
                int up = (int)top - 1;
                unsigned down = top + 1, k = 0;
                std::vector<unsigned> row_seq(sgy);
                row_seq[k++] = top;
                while (k < sgy) {
                    const bool take_down = down < sgy && (up < 0 || row_cost[down] >= row_cost[(unsigned)up]);
                    row_seq[k++] = take_down ? down++ : (unsigned)up--;
                }
                for (unsigned k2 = 0; k2 < sgy; ++k2)
                    for (unsigned i = 0; i < sgx; ++i) seq[k2 * sgx + i] = row_seq[k2] * sgx + i;
            } else if (walk == 3 || (walk == 0 && umax * (float)ns > 1.7f * usum)) {
                row_walk = false;
                std::stable_sort(seq.begin(), seq.end(), [&](unsigned a, unsigned b) { return unit_cost[a] > unit_cost[b]; });
            }
        }
        unit_of.assign((size_t)8 * units_per_xcd, -1);
        std::vector<int> filled(8, 0);
        float imbalance = 1.f;  // busiest / idlest XCD if every column of super-tiles kept "XCD = column mod 8"
        if (!unit_cost.empty() && sgx % 8 == 0) {
            float tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (unsigned S = 0; S < ns; ++S) tot[(S % sgx) & 7u] += unit_cost[S];
            imbalance = *std::max_element(tot, tot + 8) / std::max(1e-6f, *std::min_element(tot, tot + 8));
        }
        if (walk == 0 && row_walk && sgx % 8 == 0 && !unit_cost.empty() && (pl->cert.dbl_ready || imbalance > 1.15f)) {
            // A stitch's expensive tiles - the seams where both eyes contribute, the eyes' rims - stand in COLUMNS of the
            // output, and "XCD = column mod 8" hands whole seams to the same XCDs row after row: the chip waits for them
            // (c5 76.5 us; super-tiles dealt at random 66.6).  Rows are still walked together and a column keeps its XCD from
            // row to row (vertical neighbours share an L2), but after every row the busiest XCD hands a column to the idlest
            // when it is more than half a super-tile ahead: c5 76.5 -> 64.6 us, c5shard 68.9 -> 54.7.  Single sources get the
            // exchange only when their columns are that uneven too (busiest / idlest XCD > 1.15 under "column mod 8": a panorama
            // from a 200-degree fisheye, black columns beyond the field of view, 26.7 -> 25.8 us); on even columns it measured
            // +-0 (c2, c3) or worse (c1 +6 % under the plain walk).
            std::vector<int> owner(sgx);
            for (unsigned i = 0; i < sgx; ++i) owner[i] = (int)(i & 7u);
            float total[8] = {0, 0, 0, 0, 0, 0, 0, 0}, all = 0.f;
            for (float c : unit_cost) all += c;
            const float thresh = 0.5f * all / (float)ns;
            for (unsigned r = 0; r < sgy; ++r) {
                for (unsigned i = 0; i < sgx; ++i) {
                    const int x = owner[i];
                    const unsigned S = (seq[r * sgx] / sgx) * sgx + i;  // row r of the walk, column i
                    unit_of[(size_t)x * units_per_xcd + filled[x]++] = (int)S;
                    total[x] += unit_cost[S];
                }
                if (r + 1 == sgy) break;
                float ahead[8];  // totals as they will stand after the exchanges decided so far
                for (unsigned x = 0; x < 8; ++x) ahead[x] = total[x];
                for (int pass = 0; pass < 4; ++pass) {
                    const int a = (int)(std::max_element(ahead, ahead + 8) - ahead), b = (int)(std::min_element(ahead, ahead + 8) - ahead);
                    if (ahead[a] - ahead[b] <= thresh) break;
                    float best = 0.f;
                    int bi = -1, bj = -1;
                    for (unsigned i = 0; i < sgx; ++i)
                        for (unsigned j = 0; j < sgx; ++j)
                            if (owner[i] == a && owner[j] == b) {
                                const unsigned nr = seq[(r + 1) * sgx] / sgx;
                                const float gain = unit_cost[nr * sgx + i] - unit_cost[nr * sgx + j];  // what `a` sheds next row
                                if (gain > best) { best = gain; bi = (int)i; bj = (int)j; }
                            }
                    if (bi < 0) break;
                    std::swap(owner[bi], owner[bj]);
                    ahead[a] -= best;
                    ahead[b] += best;
                }
            }
        } else {
            for (unsigned p = 0; p < ns; ++p) unit_of[(size_t)(p & 7u) * units_per_xcd + filled[p & 7u]++] = (int)seq[p];  // XCD = position in the walk, mod 8
        }
    }
    // the new table is built aside (`fresh`) and moved into the plan only when it is complete: a failure leaves the plan WITHOUT a
    // launch table (no entries, groups == 0 - its launches then take the direct-gather kernels), never with a half-written one or
    // one classified under another budget
    pb_drain_and_drop(pl, out);
    PbLaunchTable fresh;
    PbBlock<int> unit_dev;
    hipError_t e = hipSuccess;
    if (class_dev && class_out) {  // (no cost pass has brought the budget pass's class counters along)
        unsigned r4[4] = {0, 0, 0, 0};
        e = hipMemcpy(r4, class_dev, sizeof(r4), hipMemcpyDeviceToHost);
        class_out[0] = r4[0];
        class_out[1] = r4[1];
    }
    if (units && e == hipSuccess) {
        e = unit_dev.alloc(unit_of.size());
        PB_STAGE("lt-host-order");
        if (e == hipSuccess) {
            if (unit_of.size() <= 1024) {  // (up to four launches that nothing waits for)
                for (size_t o = 0; o < unit_of.size(); o += 256) {
                    PbWordChunk c;
                    const size_t n = std::min<size_t>(256, unit_of.size() - o);
                    memcpy(c.v, unit_of.data() + o, n * sizeof(int));
                    hipLaunchKernelGGL(pb_store_words_kernel, dim3(1), dim3(256), 0, 0, c, unit_dev + o, (int)n);
                }
                e = hipGetLastError();
            } else {
                e = hipMemcpy(unit_dev, unit_of.data(), unit_of.size() * sizeof(int), hipMemcpyHostToDevice);
            }
        }
        PB_STAGE("lt-unit-upload");
    }
    if (bil && pl->cert.dbl_ready) {
        // the PAIR layout (pb_kernels_tile.hpp): a two-eye tile takes two slots of a pair workgroup, so the XCDs' lists grow by what
        // their tile groups need - counted, scanned per XCD and written in place of the plain layout's one workgroup per group
        PbBlock<unsigned> scan;  // n_wgs[n_groups], start[n_groups], totals[8]
        unsigned totals[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (e == hipSuccess) e = scan.alloc(2 * (size_t)n_groups + 8);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(pb_pair_count_kernel, dim3((n_groups + 255) / 256), dim3(256), 0, 0, P, pl->cert.table, pl->cert.table_r, unit_dev, units_per_xcd, n_groups, (int)U, (int)UY, scan);
            hipLaunchKernelGGL(pb_pair_scan_kernel, dim3(1), dim3(512), 0, 0, scan, n_groups, scan + n_groups, scan + 2 * (size_t)n_groups);
            e = hipMemcpy(totals, scan + 2 * (size_t)n_groups, sizeof(totals), hipMemcpyDeviceToHost);
        }
        const unsigned per_xcd = *std::max_element(totals, totals + 8), pair_groups = 8u * per_xcd;
        if (e == hipSuccess && pair_groups == 0) e = hipErrorInvalidValue;  // (a plan without tiles does not get here)
        if (e == hipSuccess) e = fresh.entries.alloc((size_t)pair_groups * 4u);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(pb_skip_fill_kernel, dim3(pair_groups), dim3(256), 0, 0, fresh.entries, 4u * pair_groups);
            hipLaunchKernelGGL(pb_pair_table_kernel, dim3(n_groups), dim3(64), 0, 0, P, pl->cert.table, pl->cert.table_r, fresh.entries, unit_dev, units_per_xcd, n_groups, (int)U, (int)UY,
                               scan + n_groups);
            e = hipDeviceSynchronize();
        }
        n_groups = pair_groups;
    } else {
        const unsigned n_slots = 4u * n_groups;
        if (e == hipSuccess) e = (!bil && pb_test_alloc_fails()) ? hipErrorOutOfMemory : fresh.entries.alloc(n_slots);  // (the test hook counts the nearest mode's tables)
        if (e == hipSuccess) {
            PB_STAGE("lt-malloc");
            hipLaunchKernelGGL(pb_launch_table_kernel, dim3(n_groups), dim3(256), 0, 0, P, pl->cert.table, fresh.entries, unit_dev, units_per_xcd, n_slots, (int)U,
                               pl->cert.dbl_ready ? pl->cert.table_r : nullptr, (int)UY);
            e = hipDeviceSynchronize();
            PB_STAGE("lt-kernel-sync");
        }
    }
    if (e != hipSuccess) {
        pb_drain_and_drop(pl, fresh);  // (its kernels may be running)
        (void)hipGetLastError();
        return pb_fail(PB_ERR_HIP, std::string("launch table: ") + hipGetErrorString(e));
    }
    fresh.groups = n_groups;
    out = std::move(fresh);
    return PB_OK;
}

// keeps the certified flags (once) and writes the flags under `budget` into the tile tables; counts = {LEAN, DIRECT} tiles (nullptr: not
// wanted - then the call does not wait for the device).
// keep_dev: the class counters stay on the device in that block (4 words, zeroed here) for the caller to fetch with something else.
static int pb_classify_under_budget(pb_plan* pl, int budget, unsigned counts[2], unsigned* keep_dev = nullptr) {
    const unsigned nt = pl->cert.n_tiles;
    const dim3 g((nt + 255) / 256), b(256);
    if (!pl->cert.saved_l) {
        PB_HIP(pl->cert.saved_l.alloc(nt));
        hipLaunchKernelGGL(pb_save_flags_kernel, g, b, 0, 0, pl->cert.table, pl->cert.saved_l, nt);
        if (pl->cert.dbl_ready) {
            PB_HIP(pl->cert.saved_r.alloc(nt));
            hipLaunchKernelGGL(pb_save_flags_kernel, g, b, 0, 0, pl->cert.table_r, pl->cert.saved_r, nt);
        }
    }
    PbBlock<unsigned> own;  // (the class counters, unless the caller keeps them)
    if (!keep_dev) PB_HIP(own.alloc(4));
    unsigned* const counters = keep_dev ? keep_dev : own.get();
    (void)hipMemsetAsync(counters, 0, 4 * sizeof(unsigned), 0);
    if (pl->cert.dbl_ready)
        hipLaunchKernelGGL(pb_budget_double_kernel, g, b, 0, 0, pl->cert.table, pl->cert.table_r, pl->cert.saved_l, pl->cert.saved_r, nt, budget, counters);
    else
        hipLaunchKernelGGL(pb_budget_kernel, g, b, 0, 0, pl->cert.table, pl->cert.saved_l, nt, budget, counters);
    if (keep_dev || !counts) {  // (the caller fetches the counts, or nobody reads them: no round trip - a block's next user is ordered behind the kernel by the stream)
        PB_HIP(hipGetLastError());
        return PB_OK;
    }
    unsigned res[4] = {0, 0, 0, 0};
    const hipError_t e = hipMemcpy(res, counters, sizeof(res), hipMemcpyDeviceToHost);
    if (e != hipSuccess) (void)hipDeviceSynchronize();
    PB_HIP(e);
    counts[0] = res[0];
    counts[1] = res[1];
    return PB_OK;
}

// The bilinear mode's launch-order table: the tiles classified under PB_BIL_WIN_BUDGET, ordered by the bilinear mode's costs.  Leaves
// the tile tables' flags under THAT budget: pb_apply_budget (the nearest mode's) must follow.  A failure leaves the plan without the
// table (the bilinear launches then take the float64 kernels), never with a stale one.  Synchronous.
#define PB_BIL_WIN_BUDGET PB_WINLDS_MAX
#define PB_BIL_POOL_RULE 50u  // a pool is accepted when at most 1 / PB_BIL_POOL_RULE of the tiles lose their window to it
#ifndef PB_BIL_POOL_SMALL
#define PB_BIL_POOL_SMALL 40448u  // a four-wave bilinear workgroup's small LDS pool: four of them, sixteen waves, per CU (160 KiB of LDS); two waves: half
#endif
//  // measured on MI355X (experiments/r4/budget_bil.sh): c1 28.7 us at 7 KiB, 25.2 at 12; c2 68.9 / 62.0; c5 109.8 / 103.4; c3 58.3 / 58.9
static int pb_build_bilinear_launch(pb_plan* pl) {
    if (!(pl->cert.fast_ready || pl->cert.dbl_ready)) return PB_OK;
    const auto fail = [&](const std::string& msg) {  // every failure exit behind the table's construction: no table, the error reported
        pb_drain_and_drop(pl, pl->bil.lt);
        return pb_fail(PB_ERR_HIP, msg);
    };
    pb_drain_and_drop(pl, pl->bil.lt);
    if (!pb_bilinear_tiles_allowed(pl->P)) return PB_OK;
    pl->bil.budget = pb_clamp_budget(PB_BIL_WIN_BUDGET);
    int rc = pb_classify_under_budget(pl, pl->bil.budget, nullptr);
    if (rc == PB_OK) rc = pb_build_launch_table(pl, true);
    if (rc != PB_OK) return rc;
    // Workgroup size and LDS pool, chosen together (a pool is accepted when at most 2 % of the tiles lose their window to it), best first:
    //   two waves, 19.75 KiB   sixteen waves per CU (four per SIMD: what the tile code's 117-120 VGPRs allow) in eight workgroups
    //   four waves, 39.5 KiB   sixteen waves in four workgroups: regions pooled over four slots fit where two slots do not (c1)
    //   two waves, 22.8 KiB    fourteen waves per CU
    //   two waves, 2 x budget  always fits: twelve waves per CU
    PbBlock<unsigned> counters;
    const unsigned ng = pl->bil.lt.groups;
    unsigned res[2] = {0u, 0u};
    hipError_t e = counters.alloc(8);
    if (e == hipSuccess) e = hipMemsetAsync(counters, 0, 8 * sizeof(unsigned), 0);
    if (e == hipSuccess && !pb_bil_off(1))  // direct-gather slots that can be served as two half windows
    {
        hipLaunchKernelGGL(pb_bilinear_halves_kernel, dim3(ng), dim3(256), 0, 0, pl->bil.lt.entries, 4u * ng, pl->bil.budget, pl->P.src.height, pl->P.src.width,
                           pb_bil_off(8) ? 1 : 0, counters);
    }
    const unsigned budget32 = (unsigned)pl->bil.budget + 32u;
    int waves = 2;
    unsigned pool = 2u * budget32;
    if (e == hipSuccess && !pb_bil_off(16)) {
        // (the one-eye slots of a virtual workgroup dealt to its two halves so that their LDS needs balance: largest with smallest)
        hipLaunchKernelGGL(pb_bilinear_balance_kernel, dim3(ng), dim3(64), 0, 0, pl->bil.lt.entries, ng);
        const struct { int waves; unsigned bytes; } tiers[3] = {{2, PB_BIL_POOL_SMALL / 2u}, {4, PB_BIL_POOL_SMALL}, {2, (163840u / 7u) & ~15u}};
        // the three dry passes back to back, ONE read-back (a round trip is ~25 us; a plan that takes the third tier made three)
        unsigned dry[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        e = hipMemsetAsync(counters, 0, 6 * sizeof(unsigned), 0);
        for (int t = 0; t < 3 && e == hipSuccess; ++t) {
            if (tiers[t].bytes >= (unsigned)tiers[t].waves * budget32) continue;
            hipLaunchKernelGGL(pb_bilinear_pool_kernel, dim3((ng * (4u / (unsigned)tiers[t].waves) + 127) / 128), dim3(128), 0, 0, pl->bil.lt.entries, ng, tiers[t].bytes, 1,
                               counters + 2 * t, tiers[t].waves);
        }
        if (e == hipSuccess) e = hipMemcpy(dry, counters, sizeof(dry), hipMemcpyDeviceToHost);
        for (int t = 0; t < 3 && e == hipSuccess; ++t) {
            if (tiers[t].bytes >= (unsigned)tiers[t].waves * budget32) continue;
            if (dry[2 * t + 1] == 0u && dry[2 * t] * PB_BIL_POOL_RULE <= pl->cert.n_tiles) {
                waves = tiers[t].waves;
                pool = tiers[t].bytes;
                break;
            }
        }
    } else {
        waves = 4;  // (the diagnostic build's "no small pool": round 4's shape)
        pool = 4u * budget32;
    }
    if (e == hipSuccess) e = hipMemsetAsync(counters, 0, 2 * sizeof(unsigned), 0);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pb_bilinear_pool_kernel, dim3((ng * (4u / (unsigned)waves) + 127) / 128), dim3(128), 0, 0, pl->bil.lt.entries, ng, pool, 0, counters, waves);
        e = hipMemcpy(res, counters, sizeof(res), hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) (void)hipDeviceSynchronize();
    counters.reset();  // (read back; a two-eye plan's table block below is of its size)
    if (e != hipSuccess || res[1] != 0u) return fail(std::string("bilinear LDS pool: ") + (e != hipSuccess ? hipGetErrorString(e) : "a workgroup does not fit"));
    if (pl->cert.dbl_ready) {
        const PbDblTables T = {pl->P.mrg_min, pl->P.mrg_max_safe, pl->P.mrg_max, pl->P.mrg_range, pl->cert.sep_ready ? pl->cert.sep_rows : nullptr, pl->cert.lat_tab, pl->cert.fix_px,
                               pl->bil.fix_xy, pl->cert.dbl_tile_fix, pl->cert.dbl_px_fix};
        if ((!pl->bil.dbl_tables && pl->bil.dbl_tables.alloc(1) != hipSuccess) ||
            hipMemcpy(pl->bil.dbl_tables, &T, sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
            return fail("bilinear launch: out of device memory");
    }
    pl->bil.pool_bytes = pool;
    pl->bil.waves = waves;
    return PB_OK;
}

// applies `budget` to the certified flags and rebuilds the nearest mode's launch-order table; synchronous on the default stream
static int pb_apply_budget(pb_plan* pl, int budget) {
    PbParams& P = pl->P;
    if (!(pl->cert.fast_ready || pl->cert.dbl_ready)) return PB_OK;
    budget = pb_clamp_budget(budget);
    // the parameter block as the launches will see it goes up BEFORE anything of the plan changes (a failure used to
    // leave the old launch table, classified under the old budget, next to the new budget)
    PbParams Q = P;
    Q.win_budget = budget;
    if (!pl->nearest.P_dev) PB_HIP(pl->nearest.P_dev.alloc(1));
    // Nothing here waits for the device by itself (a round trip is 12-25 us of a 0.5 ms plan): the class counters of the budget pass stay
    // on the device and come back with the launch-order pass's costs, the parameter block is stored by a kernel from its own arguments.
    unsigned counts[2] = {pl->cert.n_lean_tiles, pl->cert.n_direct_tiles};
    PbBlock<unsigned> class_dev;
    PB_HIP(class_dev.alloc(4));
    PB_STAGE("ab-pdev-malloc");
    int rc = pb_classify_under_budget(pl, budget, nullptr, class_dev);
    PB_STAGE("ab-classify");
    if (rc == PB_OK) {
        hipLaunchKernelGGL(pb_store_params_kernel, dim3(1), dim3(64), 0, 0, Q, pl->nearest.P_dev);
        if (hipGetLastError() != hipSuccess) rc = pb_fail(PB_ERR_HIP, "parameter block upload failed");
    }
    PB_STAGE("ab-pdev-upload");
    if (rc != PB_OK) {
        // the table may be half reclassified: no launch table at all (launches take the direct-gather kernels, which read no budget)
        (void)hipDeviceSynchronize();  // (the counter block goes back idle)
        pl->nearest.lt = PbLaunchTable();  // (waited for just above)
        return rc;
    }
    P.win_budget = budget;
    rc = pb_build_launch_table(pl, false, class_dev, counts);
    if (rc != PB_OK) (void)hipDeviceSynchronize();  // (a success: pb_build_launch_table has waited for the device - class_dev may go back)
    pl->cert.n_lean_tiles = counts[0];
    pl->cert.n_direct_tiles = counts[1];
    return rc;
}

// OPT-IN (PB_PLAN_TUNE): picks the budget by measurement - four candidates x a few launches on scratch frames
// (allocates and fills frame-sized scratch; tens of frames' worth of GPU time).  Returns the winner.
static int pb_tune_window_budget(pb_plan* pl) {
    PbParams& P = pl->P;
    int best = P.win_budget;
    if (!(pl->cert.fast_ready || pl->cert.dbl_ready)) return best;
    const size_t sb = 3ull * P.src.height * P.src.width, db = 3ull * P.dst.height * P.dst.width;
    if (sb + db > (1ull << 30)) return best;
    struct Scratch {  // frame-sized and once per tuned plan: plain hipMalloc, not the cache's business; released behind the wait below
        uint8_t *src = nullptr, *dst = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Scratch() {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            (void)hipFree(src), (void)hipFree(dst);
        }
    } scratch;
    uint8_t *&src = scratch.src, *&dst = scratch.dst;
    hipEvent_t &e0 = scratch.e0, &e1 = scratch.e1;
    do {
        // scratch frames in rotation, more than the 256 MiB Infinity Cache in total: the launches being timed
        // must stream from HBM like real frames do, not hit a cache-resident copy
        const size_t sb16 = (sb + 255) & ~(size_t)255, db16 = (db + 255) & ~(size_t)255;
        int n_scratch = (int)(((size_t)320 << 20) / (sb16 + db16)) + 1;
        if (n_scratch < 2) n_scratch = 2;
        if (n_scratch > 8) n_scratch = 8;
        if (hipMalloc((void**)&src, n_scratch * sb16) != hipSuccess || hipMalloc((void**)&dst, n_scratch * db16) != hipSuccess) break;
        if (hipMemsetAsync(src, 0x55, n_scratch * sb16, 0) != hipSuccess) break;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) break;
        // one frame of scratch slot `slot`, launched as pb_remap_u8 launches it
        const auto launch = [&](int slot) {
            const uint8_t* s = src + slot * sb16;
            return pb_launch(pl, pb_route(pl, PB_INTERP_NEAREST, 1, 0, pb_aligned16(s, sb)), s, dst + slot * db16, 1, sb, db, 0);
        };
        const int cand[4] = {PB_WINLDS_MAX, 10224, 8176, 7168};  // 3, 4, 5 and 5 workgroups per CU (LDS-wise)
        float t_min[4] = {1e30f, 1e30f, 1e30f, 1e30f};
        bool failed = false;
        int launch_no = 0;
        for (int pass = 0; pass < 2 && !failed; ++pass)  // two interleaved passes: clock ramps and noise hit all alike
            for (int c = 0; c < 4 && !failed; ++c) {
                if (pb_apply_budget(pl, cand[c]) != PB_OK) { failed = true; break; }
                for (int rep = 0; rep < 4; ++rep) {  // the first launch after a reclassification is not counted
                    (void)hipEventRecord(e0, 0);
                    const int slot = launch_no++ % n_scratch;
                    if (launch(slot) != PB_OK) { failed = true; break; }
                    (void)hipEventRecord(e1, 0);
                    if (hipEventSynchronize(e1) != hipSuccess) { failed = true; break; }
                    float ms = 0.f;
                    (void)hipEventElapsedTime(&ms, e0, e1);
                    if (rep > 0 && ms < t_min[c]) t_min[c] = ms;
                }
            }
        // the library default unless another budget is at least 3 % faster (a handful of launches is a noisy yardstick)
        int bi = 3;
        for (int c = 0; c < 3; ++c)
            if (t_min[c] < t_min[3] * 0.97f && t_min[c] < t_min[bi]) bi = c;
        if (!failed) best = cand[bi];
        // then the launch order under the chosen budget: the policy's walk against the three fixed ones
        if (!failed && pb_apply_budget(pl, best) == PB_OK) {
            std::vector<float> t_walk[4];
            for (int pass = 0; pass < 3 && !failed; ++pass)
                for (int wk = 0; wk < 4 && !failed; ++wk) {
                    pl->walk = wk;
                    if (pb_build_launch_table(pl) != PB_OK) { failed = true; break; }
                    for (int rep = 0; rep < 7; ++rep) {
                        (void)hipEventRecord(e0, 0);
                        const int slot = launch_no++ % n_scratch;
                        if (launch(slot) != PB_OK) { failed = true; break; }
                        (void)hipEventRecord(e1, 0);
                        if (hipEventSynchronize(e1) != hipSuccess) { failed = true; break; }
                        float ms = 0.f;
                        (void)hipEventElapsedTime(&ms, e0, e1);
                        if (rep > 0) t_walk[wk].push_back(ms);
                    }
                }
            // medians (a launch in isolation varies by several per cent); a fixed walk must beat the policy's by 5 %
            float med[4] = {1e30f, 1e30f, 1e30f, 1e30f};
            for (int wk = 0; wk < 4 && !failed; ++wk) {
                std::sort(t_walk[wk].begin(), t_walk[wk].end());
                if (!t_walk[wk].empty()) med[wk] = t_walk[wk][t_walk[wk].size() / 2];
            }
            int bw = 0;
            for (int wk = 1; wk < 4; ++wk)
                if (med[wk] < med[0] * 0.95f && med[wk] < med[bw]) bw = wk;
            pl->walk = failed ? 0 : bw;
        }
    } while (0);
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    return best;
}

// the parameter block of a request, as pb_plan_create_ex fills it before any device work
static void pb_params_of_request(PbParams& P, const PbEndX& dst, const double* rot3x3, int n_rot, const PbEndX& src) {
    memset(&P, 0, sizeof(PbParams));
    P.dst = dst.e;
    P.src = src.e;
    P.poly_dst = dst.poly;
    P.poly_src = src.poly;
    P.n_rot = n_rot;
    for (int k = 0; k < n_rot; ++k)
        for (int e = 0; e < 9; ++e) P.R[k][e] = rot3x3[9 * k + e];
    pb_derive(P);
}
// everything of a parameter block that follows from the request alone (not: budget, experiment flags, validity thresholds)
static bool pb_same_request(const PbParams& a, const PbParams& b) {
    PbParams x = a, y = b;
    for (PbParams* p : {&x, &y}) {
        p->win_budget = 0;
        p->exp_flags = 0;
        p->thresholds_ready = 0;
        p->fast_tiles = 0;
        for (int i = 0; i < 2; ++i) p->inv_lo[i] = p->inv_hi[i] = 0;
    }
    return memcmp(&x, &y, sizeof(PbParams)) == 0;
}

static double pb_now_ms() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

// device preparation of a plan on the current device + its window budget (0 = default; PB_WIN_BUDGET overrides
// the default for experiments); PB_PLAN_TUNE times candidates instead
static int pb_plan_prepare_full(pb_plan* pl, unsigned flags, int win_budget) {
    if (pl->cert.fast_ready || pl->cert.dbl_ready || pl->cert.sep_ready || pl->device >= 0) {
        // already prepared: the budget may change, and the opt-in bilinear mode's tables may be asked for (PB_PLAN_BILINEAR) by a plan
        // that was created without them
        if ((flags & PB_PLAN_BILINEAR) && (pl->cert.fast_ready || pl->cert.dbl_ready) && !pl->bil.tiles && pb_bilinear_tiles_allowed(pl->P)) {
            pl->bil_wanted = 1;
            int rc = pb_build_bilinear_list(pl);
            if (rc == PB_OK) rc = pb_build_bilinear_launch(pl);
            // pb_build_bilinear_launch leaves the tile tables' flags under the MODE's budget: the nearest mode's classification is written
            // back (one small kernel).  Its launch table is NOT rebuilt - nothing it holds has changed, and no device memory a launch may
            // hold a pointer to is freed here.  The tile tables do pass through the other classification on the way, and a double-fisheye
            // plan's nearest kernel reads them: hence the header's rule - no launch of the plan in flight (the Python host, which builds
            // the mode's tables at its first use on whichever thread that happens, holds its own launches off: _native.py _LaunchGate).
            const int rc2 = win_budget > 0 ? pb_apply_budget(pl, win_budget) : pb_classify_under_budget(pl, pl->P.win_budget, nullptr);
            if (rc != PB_OK) return rc;
            if (rc2 != PB_OK) return rc2;
            PB_HIP(hipDeviceSynchronize());
            return PB_OK;
        }
        if (win_budget > 0) return pb_apply_budget(pl, win_budget);
        return PB_OK;
    }
    PB_STAGE("begin");
    const double t0 = pb_now_ms();
    int rc = pb_plan_prepare_on_device(pl);
    if (rc != PB_OK) {
        pl->device = -1;  // (pb_plan_prepare_on_device has dropped its state): the plan is unprepared again and may be retried
        return rc;
    }
    int budget = win_budget > 0 ? win_budget : PB_DEFAULT_WIN_BUDGET;
    if (win_budget <= 0 && pb_knob("PB_WIN_BUDGET", 0) > 0) budget = pb_knob("PB_WIN_BUDGET", 0);
    if (pl->bil_wanted) rc = pb_build_bilinear_launch(pl);
    if (rc != PB_OK) return rc;
    PB_STAGE("bil-launch");
    rc = pb_apply_budget(pl, budget);
    if (rc != PB_OK) return rc;
    PB_HIP(hipDeviceSynchronize());
    PB_STAGE("apply-budget-end");
    pb_stage_report();
    pl->prepare_ms = pb_now_ms() - t0;
    if ((flags & PB_PLAN_TUNE) && win_budget <= 0) {
        const double t1 = pb_now_ms();
        const int best = pb_tune_window_budget(pl);
        rc = pb_apply_budget(pl, best);
        pl->tune_ms = pb_now_ms() - t1;
    }
    return rc;
}

// a plan under construction (pb_plan_create_ex, pb_plan_deserialize): destroyed like any other unless it is released into *out
struct PbPlanDestroy {
    void operator()(pb_plan* pl) const { pb_plan_destroy(pl); }
};
using PbPlanOwner = std::unique_ptr<pb_plan, PbPlanDestroy>;

extern "C" {

int pb_abi_version(void) { return PB_ABI_VERSION; }
int pb_math_flavour(void) { return PB_MATH_FLAVOUR; }
const char* pb_last_error(void) { return g_err.c_str(); }

int pb_init(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return pb_fail(PB_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return pb_fail(PB_ERR_INVALID, "device ordinal out of range");
    PB_HIP(hipSetDevice(device));
    return PB_OK;
}
int pb_shutdown(void) {
    // the idle blocks of the plan-preparation cache (at most 96 MiB) go back to the driver; live plans keep theirs
    std::vector<void*> idle;
    {
        std::lock_guard<std::mutex> g(g_tmp.lock);
        for (const auto& b : g_tmp.idle) idle.push_back(b.ptr);
        g_tmp.idle.clear();
        g_tmp.held = 0;
    }
    for (void* p : idle) (void)hipFree(p);
    return PB_OK;
}

int pb_device_name(char* buf, size_t buflen) {
    if (!buf || !buflen) return pb_fail(PB_ERR_INVALID, "null buffer");
    int dev = 0;
    PB_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    PB_HIP(hipGetDeviceProperties(&prop, dev));
    snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return PB_OK;
}

int pb_plan_create_ex(const pb_proj* dst, const double* rot3x3, int n_rot, const pb_proj* src, unsigned flags, int win_budget,
                      pb_plan** out) {
    std::string why;
    if (!out) return pb_fail(PB_ERR_INVALID, "null out pointer");
    *out = nullptr;
    if (!pb_end_ok(dst, why, PB_ROLE_DST) || !pb_end_ok(src, why, PB_ROLE_SRC)) return pb_fail(PB_ERR_INVALID, why);
    if (n_rot < 0 || n_rot > PB_MAX_ROTATIONS) return pb_fail(PB_ERR_INVALID, "n_rot outside [0, PB_MAX_ROTATIONS]");
    if (n_rot > 0 && !rot3x3) return pb_fail(PB_ERR_INVALID, "null rotation matrices");
    if (flags & ~(unsigned)(PB_PLAN_DEFER | PB_PLAN_TUNE | PB_PLAN_MATH_SVML | PB_PLAN_MATH_LIBM | PB_PLAN_NO_BILINEAR)) return pb_fail(PB_ERR_INVALID, "unknown plan flags");
    if ((flags & PB_PLAN_MATH_SVML) && (flags & PB_PLAN_MATH_LIBM)) return pb_fail(PB_ERR_INVALID, "a plan has one math flavour");
    if (((flags & PB_PLAN_MATH_SVML) && PB_MATH_FLAVOUR != 0) || ((flags & PB_PLAN_MATH_LIBM) && PB_MATH_FLAVOUR != 1))
        return pb_fail(PB_ERR_UNSUPPORTED, PB_MATH_FLAVOUR ? "this is libphotonbend_hip_libm.so (the float64 chain runs glibc's asin / acos / atan / tan): load libphotonbend_hip.so for the AVX-512 (SVML) flavour"
                                                           : "this is libphotonbend_hip.so (the float64 chain runs NumPy's AVX-512 arcsin / arccos / arctan / tan): load libphotonbend_hip_libm.so for the libm flavour");
    flags &= ~(unsigned)(PB_PLAN_MATH_SVML | PB_PLAN_MATH_LIBM);
    if (win_budget < 0) return pb_fail(PB_ERR_INVALID, "negative window budget");
    PbPlanOwner pl(new (std::nothrow) pb_plan());
    if (!pl) return pb_fail(PB_ERR_INVALID, "out of host memory");
    pb_params_of_request(pl->P, pb_to_end(dst), rot3x3, n_rot, pb_to_end(src));
    pl->P.win_budget = PB_WINLDS_MAX;
    pl->P.exp_flags = PB_DEFAULT_EXP;
    pl->P.exp_flags = pb_knob("PB_EXP", PB_DEFAULT_EXP);
    pl->mode = PB_MODE_AUTO;
    pl->bil_wanted = (flags & PB_PLAN_NO_BILINEAR) ? 0 : 1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
    (void)hipGetLastError();
    if (ndev > 0 && !(flags & PB_PLAN_DEFER)) {
        const int rc = pb_plan_prepare_full(pl.get(), flags, win_budget);
        if (rc != PB_OK) return rc;
    }
    *out = pl.release();
    return PB_OK;
}

int pb_plan_matches(const pb_plan* plan, const pb_proj* dst, const double* rot3x3, int n_rot, const pb_proj* src) {
    std::string why;
    if (!plan) return pb_fail(PB_ERR_INVALID, "null argument");
    if (!pb_end_ok(dst, why, PB_ROLE_DST) || !pb_end_ok(src, why, PB_ROLE_SRC)) return pb_fail(PB_ERR_INVALID, why);
    if (n_rot < 0 || n_rot > PB_MAX_ROTATIONS || (n_rot > 0 && !rot3x3)) return pb_fail(PB_ERR_INVALID, "bad rotation arguments");
    PbParams Q;
    pb_params_of_request(Q, pb_to_end(dst), rot3x3, n_rot, pb_to_end(src));
    return pb_same_request(Q, plan->P) ? 1 : 0;
}

int pb_lens_polynomial(const double k[4], double max_theta, int* lens_out) {
    if (!k || !lens_out) return pb_fail(PB_ERR_INVALID, "null argument");
    PbPoly L;
    std::string why;
    if (!pb_poly_make(k, max_theta, L, why)) return pb_fail(PB_ERR_INVALID, why);
    const int rc = pb_poly_register(L, lens_out);
    if (rc != PB_OK) return pb_fail(rc, "the polynomial lens registry is full (4096 distinct lenses per process)");
    return PB_OK;
}

int pb_lens_polynomial_info(int lens, double k[4], double* max_theta) {
    PbPoly L;
    if (!pb_poly_lookup(lens, &L)) return pb_fail(PB_ERR_INVALID, "not a registered polynomial lens of this process");
    if (k)
        for (int i = 0; i < 4; ++i) k[i] = L.k[i];
    if (max_theta) *max_theta = L.max_theta;
    return PB_OK;
}

int pb_plan_create(const pb_proj* dst, const double* rot3x3, int n_rot, const pb_proj* src, pb_plan** out) {
    return pb_plan_create_ex(dst, rot3x3, n_rot, src, 0u, 0, out);
}

int pb_plan_prepare(pb_plan* plan, unsigned flags, int win_budget) {
    if (!plan) return pb_fail(PB_ERR_INVALID, "null argument");
    if (flags & ~(unsigned)(PB_PLAN_TUNE | PB_PLAN_BILINEAR)) return pb_fail(PB_ERR_INVALID, "unknown plan flags");
    if (win_budget < 0) return pb_fail(PB_ERR_INVALID, "negative window budget");
    if (flags & PB_PLAN_BILINEAR) plan->bil_wanted = 1;  // (a deferred plan: its preparation now includes the mode's tables)
    const int rc = pb_check_device(plan);
    if (rc != PB_OK) return rc;
    return pb_plan_prepare_full(plan, flags, win_budget);
}

int pb_plan_set_window_budget(pb_plan* plan, int win_budget) {
    if (!plan || win_budget <= 0) return pb_fail(PB_ERR_INVALID, "null plan or non-positive budget");
    if (!(plan->cert.fast_ready || plan->cert.dbl_ready)) return pb_fail(PB_ERR_UNSUPPORTED, "the plan has no tile tables (not prepared, or a geometry without a fast path)");
    int dev = -1;
    PB_HIP(hipGetDevice(&dev));
    if (dev != plan->device) return pb_fail(PB_ERR_INVALID, "plan was prepared on another device; create one plan per device");
    return pb_apply_budget(plan, win_budget);
}

int pb_plan_timing(const pb_plan* plan, double* prepare_ms, double* tune_ms) {
    if (!plan) return pb_fail(PB_ERR_INVALID, "null argument");
    if (prepare_ms) *prepare_ms = plan->prepare_ms;
    if (tune_ms) *tune_ms = plan->tune_ms;
    return PB_OK;
}

void pb_plan_destroy(pb_plan* plan) {
    if (!plan) return;
    // ONE wait (launches of the plan may still be in flight on the caller's streams), then its groups give their blocks back to the
    // cache; a plan that owns none (deferred and never prepared, or without tables) touches no HIP call
    if (plan->holds()) pb_wait_device(plan->device);
    delete plan;
}

int pb_plan_dst_shape(const pb_plan* plan, int* height, int* width) {
    if (!plan || !height || !width) return pb_fail(PB_ERR_INVALID, "null argument");
    *height = plan->P.dst.height;
    *width = plan->P.dst.width;
    return PB_OK;
}
int pb_plan_bilinear_float64_tiles(const pb_plan* plan) {
    if (!plan || !(plan->cert.fast_ready || plan->cert.dbl_ready)) return 0;
    if (!plan->bil.tiles) return (int)plan->cert.n_tiles;  // (created with PB_PLAN_NO_BILINEAR and not asked since: pb_remap_bilinear_u8 runs the per-pixel float64 kernels)
    if (plan->bil.xy) return 0;  // every tile the models cannot serve has its exact coordinates in the plan's table
    return (int)(plan->cert.n_fail_tiles + (plan->bil.tiles ? plan->bil.n_tiles : 0u));
}
int pb_plan_bilinear_tile_mix(const pb_plan* plan, long long mix[8]) {
    if (!plan || !mix) return pb_fail(PB_ERR_INVALID, "null argument");
    for (int k = 0; k < 8; ++k) mix[k] = 0;
    if (!(plan->cert.fast_ready || plan->cert.dbl_ready) || !plan->bil.lt.entries || plan->bil.lt.groups == 0) return PB_OK;
    if (plan->device >= 0) {
        int dev = -1;
        PB_HIP(hipGetDevice(&dev));
        if (dev != plan->device) return pb_fail(PB_ERR_INVALID, "plan was prepared on another device");
    }
    // the entries the bilinear launch's waves read, classified as the kernel takes them (pb_bilinear_mix_kernel)
    PbBlock<unsigned> counters;
    PB_HIP(counters.alloc(8));
    hipError_t e = hipMemsetAsync(counters, 0, 8 * sizeof(unsigned), 0);
    if (e == hipSuccess) {
        const unsigned n_slots = 4u * plan->bil.lt.groups;
        hipLaunchKernelGGL(pb_bilinear_mix_kernel, dim3((n_slots + 255) / 256), dim3(256), 0, 0, plan->bil.lt.entries, n_slots, counters);
        unsigned res[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        e = hipMemcpy(res, counters, sizeof(res), hipMemcpyDeviceToHost);
        for (int k = 0; k < 8; ++k) mix[k] = res[k];
    }
    if (e != hipSuccess) (void)hipDeviceSynchronize();
    PB_HIP(e);
    return PB_OK;
}
int pb_plan_video_bilinear_mix(const pb_plan* plan, long long mix[4]) {
    if (!plan || !mix) return pb_fail(PB_ERR_INVALID, "null argument");
    for (int k = 0; k < 4; ++k) mix[k] = 0;
    if (!plan->cert.fast_ready || !plan->bil.lt.entries || plan->bil.lt.groups == 0 || !plan->cert.n_fix_px) return PB_OK;
    if (int rc = pb_check_device(plan)) return rc;
    PbBlock<unsigned> counters;
    PB_HIP(counters.alloc(4));
    hipError_t e = hipMemsetAsync(counters, 0, 4 * sizeof(unsigned), 0);
    if (e == hipSuccess) {
        const unsigned n_slots = 4u * plan->bil.lt.groups;
        hipLaunchKernelGGL(pb_video_bilinear_mix_kernel, dim3((n_slots + 255) / 256), dim3(256), 0, 0, plan->bil.lt.entries, n_slots, plan->cert.fix_px, plan->P.dst.width,
                           counters);
        unsigned res[4] = {0, 0, 0, 0};
        e = hipMemcpy(res, counters, sizeof(res), hipMemcpyDeviceToHost);
        for (int k = 0; k < 4; ++k) mix[k] = res[k];
    }
    if (e != hipSuccess) (void)hipDeviceSynchronize();
    PB_HIP(e);
    return PB_OK;
}
int pb_plan_stitch_tile_mix(const pb_plan* plan, long long mix[9]) {
    if (!plan || !mix) return pb_fail(PB_ERR_INVALID, "null argument");
    for (int k = 0; k < 9; ++k) mix[k] = 0;
    if (!plan->cert.dbl_ready || !plan->nearest.lt.entries || plan->nearest.lt.groups == 0) return PB_OK;
    if (int rc = pb_check_device(plan)) return rc;
    // the slots a stitch launch's waves read, classified as pb_stitch_video_kernel takes them (pb_stitch_mix_kernel)
    PbBlock<unsigned> counters;
    PB_HIP(counters.alloc(9));
    hipError_t e = hipMemsetAsync(counters, 0, 9 * sizeof(unsigned), 0);
    if (e == hipSuccess) {
        const unsigned n_slots = 4u * plan->nearest.lt.groups;
        hipLaunchKernelGGL(pb_stitch_mix_kernel, dim3((n_slots + 255) / 256), dim3(256), 0, 0, plan->nearest.lt.entries, n_slots, plan->cert.table, plan->cert.table_r,
                           (plan->P.dst.width + PB_TILE - 1) / PB_TILE, plan->cert.fix_px, plan->P.dst.width, counters);
        unsigned res[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        e = hipMemcpy(res, counters, sizeof(res), hipMemcpyDeviceToHost);
        for (int k = 0; k < 9; ++k) mix[k] = res[k];
    }
    if (e != hipSuccess) (void)hipDeviceSynchronize();
    PB_HIP(e);
    return PB_OK;
}
int pb_plan_bilinear_launch_shape(const pb_plan* plan, int* lds_bytes, int* workgroups_per_frame) {
    if (!plan || !lds_bytes || !workgroups_per_frame) return pb_fail(PB_ERR_INVALID, "null argument");
    const bool tiles = (plan->cert.fast_ready || plan->cert.dbl_ready) && plan->bil.lt.entries && plan->bil.lt.groups > 0;
    *lds_bytes = tiles ? (int)plan->bil.pool_bytes : 0;
    *workgroups_per_frame = tiles ? (int)pb_bil_groups(plan) : 0;
    return PB_OK;
}
int pb_plan_window_budget(const pb_plan* plan) {
    return (plan && (plan->cert.fast_ready || plan->cert.dbl_ready)) ? plan->P.win_budget : 0;
}
int pb_plan_src_shape(const pb_plan* plan, int* height, int* width) {
    if (!plan || !height || !width) return pb_fail(PB_ERR_INVALID, "null argument");
    *height = plan->P.src.height;
    *width = plan->P.src.width;
    return PB_OK;
}

int pb_remap_u8(const pb_plan* plan, const uint8_t* src_dev, uint8_t* dst_dev, int n_frames, size_t src_frame_stride,
                size_t dst_frame_stride, void* stream) {
    const int rc = pb_check_frames(plan, src_dev, dst_dev, n_frames, 1, src_frame_stride, dst_frame_stride);
    if (rc != PB_OK || n_frames == 0) return rc;
    return pb_launch(plan, pb_route(plan, PB_INTERP_NEAREST, 1, 0, pb_aligned16(src_dev, src_frame_stride)), src_dev, dst_dev, n_frames,
                     src_frame_stride, dst_frame_stride, (hipStream_t)stream);
}

// pixels of bytes_per_px != 3 on plans the tile kernel serves; 3 is pb_remap_u8 itself
static bool pb_px_frames_fit(const pb_plan* plan, int bpp) {  // 32-bit source byte offsets (pb_kernels_px.hpp)
    const PbParams& P = plan->P;
    const unsigned long long B = (unsigned long long)bpp;
    return B * P.src.height * P.src.width < (1ull << 31) && B * P.dst.height * P.dst.width < (1ull << 31);
}
int pb_remap_px(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, size_t src_frame_stride, size_t dst_frame_stride,
                int bytes_per_px, void* stream) {
    const int rc = pb_check_frames(plan, src_dev, dst_dev, n_frames, 1, src_frame_stride, dst_frame_stride, false, bytes_per_px);
    if (rc != PB_OK || n_frames == 0) return rc;
    const uint8_t* s = static_cast<const uint8_t*>(src_dev);
    uint8_t* d = static_cast<uint8_t*>(dst_dev);
    if (bytes_per_px != 3 && !pb_px_frames_fit(plan, bytes_per_px))
        return pb_fail(PB_ERR_UNSUPPORTED, "pb_remap_px takes frames below 2^31 bytes: use pb_index_map_i32 + pb_gather_px");
    return pb_launch(plan, pb_route(plan, PB_INTERP_NEAREST, 1, 0, pb_aligned16(s, src_frame_stride), bytes_per_px), s, d, n_frames, src_frame_stride,
                     dst_frame_stride, (hipStream_t)stream);
}
int pb_remap_px_supported(const pb_plan* plan, int bytes_per_px) {
    if (!plan) return pb_fail(PB_ERR_INVALID, "null argument");
    if (!pb_px_size_ok(bytes_per_px)) return pb_fail(PB_ERR_INVALID, "bytes_per_px outside {1, 2, 3, 4, 6, 8}");
    if (bytes_per_px == 3) return 1;
    return pb_route(plan, PB_INTERP_NEAREST, 1, 0, false, bytes_per_px).kind == PbRoute::PX && pb_px_frames_fit(plan, bytes_per_px);
}

// Video frames: one path through the checks, the route and the launch for every family (PbVideoFmt).  Every check comes
// before the device is looked at and before any launch.
struct PbVideoFrame {  // a resolved layout, in bytes (semi-planar: cpitch = pitch, o1 = uv_offset, o2 = 0)
    unsigned long long pitch, cpitch, o1, o2, span, stride;
};
static int pb_nv12_resolve(const char* what, const pb_nv12_layout* l, unsigned long long S, unsigned long long h, unsigned long long w, PbVideoFrame& f) {
    const std::string n(what);
    // (a frame must span less than 2^31 bytes to be served: a pitch or an offset at or beyond that is refused here, before anything is
    //  multiplied - no product below can wrap, whatever the caller passes)
    if (l && (l->pitch >= (1ull << 31) || l->uv_offset >= (1ull << 31)))
        return pb_fail(PB_ERR_UNSUPPORTED, "pb_remap_nv12 takes frames whose planes span less than 2^31 bytes (" + n + " pitch or uv_offset): use pb_index_map_i32 and gather the two planes");
    f.pitch = f.cpitch = (l && l->pitch) ? l->pitch : S * w;
    if (f.pitch < S * w) return pb_fail(PB_ERR_INVALID, n + " pitch smaller than a row");
    f.o1 = (l && l->uv_offset) ? l->uv_offset : f.pitch * h;
    f.o2 = 0;
    if (f.o1 < f.pitch * h) return pb_fail(PB_ERR_INVALID, n + " uv_offset smaller than the luma plane");
    f.span = f.o1 + f.pitch * (h / 2);  // (whole pitches: the pair plane's last row counts to its pitch)
    f.stride = (l && l->frame_stride) ? l->frame_stride : f.span;
    if (f.stride < f.span) return pb_fail(PB_ERR_INVALID, n + " frame_stride smaller than a frame");
    if ((f.pitch | f.o1 | f.stride) % (2 * S))
        return pb_fail(PB_ERR_INVALID, n + " pitch, uv_offset and frame_stride must be multiples of " + std::to_string(2 * S) + " bytes (one chroma pair)");
    return PB_OK;
}
static int pb_planar_resolve(const char* what, const pb_planar_layout* l, unsigned long long S, unsigned long long h, unsigned long long w, int cx, int cy,
                             PbVideoFrame& f) {
    const std::string n(what);
    // (a frame must span less than 2^31 bytes to be served: a member at or beyond that is refused here, before anything is multiplied -
    //  no product below can wrap, whatever the caller passes)
    if (l && (l->pitch >= (1ull << 31) || l->chroma_pitch >= (1ull << 31) || l->offset1 >= (1ull << 31) || l->offset2 >= (1ull << 31)))
        return pb_fail(PB_ERR_UNSUPPORTED, "pb_remap_planar takes frames whose planes span less than 2^31 bytes (" + n + " pitch, chroma_pitch, offset1 or offset2): use pb_index_map_i32 and gather the three planes");
    const unsigned long long cw = w >> cx, ch = h >> cy;
    f.pitch = (l && l->pitch) ? l->pitch : S * w;
    if (f.pitch < S * w) return pb_fail(PB_ERR_INVALID, n + " pitch smaller than a row");
    f.cpitch = (l && l->chroma_pitch) ? l->chroma_pitch : S * cw;
    if (f.cpitch < S * cw) return pb_fail(PB_ERR_INVALID, n + " chroma_pitch smaller than a row of planes 1 and 2");
    // a plane occupies [start, start + pitch * (rows - 1) + S * samples of a row): the padding after its last row belongs to nobody
    const unsigned long long e0 = h ? f.pitch * (h - 1) + S * w : 0, ce = ch ? f.cpitch * (ch - 1) + S * cw : 0;
    f.o1 = (l && l->offset1) ? l->offset1 : f.pitch * h;
    f.o2 = (l && l->offset2) ? l->offset2 : f.o1 + f.cpitch * ch;
    if (f.o1 < e0 || f.o2 < e0) return pb_fail(PB_ERR_INVALID, n + " planes overlap: plane 1 or 2 starts inside plane 0");
    if (ce && (f.o1 < f.o2 ? f.o1 + ce > f.o2 : f.o2 + ce > f.o1)) return pb_fail(PB_ERR_INVALID, n + " planes overlap: planes 1 and 2");
    f.span = std::max(f.o1, f.o2) + ce;
    // (the packed default is the end of plane 2 when the planes come in order; in any order, the end of the last plane)
    f.stride = (l && l->frame_stride) ? l->frame_stride : std::max(f.span, f.o2 + f.cpitch * ch);
    if (f.stride < f.span) return pb_fail(PB_ERR_INVALID, n + " frame_stride smaller than a frame: a plane ends beyond it");
    if ((f.pitch | f.cpitch | f.o1 | f.o2 | f.stride) % S)
        return pb_fail(PB_ERR_INVALID, n + " pitch, chroma_pitch, offsets and frame_stride must be multiples of " + std::to_string(S) + " bytes (one sample)");
    return PB_OK;
}
// layout: a pb_nv12_layout (pairs) or a pb_planar_layout, null for the packed defaults
static int pb_video_resolve(const PbVideoFmt& v, const char* what, const void* layout, const PbEnd& p, PbVideoFrame& f) {
    const unsigned long long S = (unsigned long long)v.S, h = (unsigned long long)p.height, w = (unsigned long long)p.width;
    return v.pairs ? pb_nv12_resolve(what, static_cast<const pb_nv12_layout*>(layout), S, h, w, f)
                   : pb_planar_resolve(what, static_cast<const pb_planar_layout*>(layout), S, h, w, v.cx(), v.cy(), f);
}
// the sample size, the subsampling and the dimension rule of a format: what the calls and the _supported questions check alike
static int pb_video_fmt_check(const pb_plan* plan, const PbVideoFmt& v) {
    if (v.S != 1 && v.S != 2) return pb_fail(PB_ERR_INVALID, "bytes_per_sample outside {1, 2}");
    if (v.sub != PB_PLANAR_444 && v.sub != PB_PLANAR_422 && v.sub != PB_PLANAR_420)
        return pb_fail(PB_ERR_INVALID, "subsampling outside {PB_PLANAR_444, PB_PLANAR_422, PB_PLANAR_420}");
    const PbParams& P = plan->P;
    if (((P.src.width | P.dst.width) & v.cx()) || ((P.src.height | P.dst.height) & v.cy()))
        return pb_fail(PB_ERR_INVALID, v.sub == PB_PLANAR_420 ? "4:2:0 frames need even source and destination dimensions" : "4:2:2 frames need even source and destination widths");
    return PB_OK;
}
// The arguments of every video entry point, in this order: null plan / frames, the frame count, the sample size, the subsampling, the
// dimension rule, the two layouts (source first), the pointers' alignment.  Resolves the layouts, and the fills in stored form.
struct PbVideoCall {
    PbVideoFmt fmt;
    PbVideoFrame fs, fd;
    PbPlanar L;
    bool span_fits() const { return fs.span < (1ull << 31) && fd.span < (1ull << 31); }
};
static int pb_video_check(const pb_plan* plan, const void* src_dev, const void* dst_dev, int n_frames, const void* src_layout, const void* dst_layout,
                          const PbVideoFmt& v, const uint16_t fill[3], PbVideoCall& c) {
    if (!plan || !src_dev || !dst_dev) return pb_fail(PB_ERR_INVALID, "null argument");
    if (n_frames < 0) return pb_fail(PB_ERR_INVALID, "negative frame count");
    int rc = pb_video_fmt_check(plan, v);
    if (rc == PB_OK) rc = pb_video_resolve(v, "source", src_layout, plan->P.src, c.fs);
    if (rc == PB_OK) rc = pb_video_resolve(v, "destination", dst_layout, plan->P.dst, c.fd);
    if (rc != PB_OK) return rc;
    if (((uintptr_t)src_dev | (uintptr_t)dst_dev) % v.unit())
        return pb_fail(PB_ERR_INVALID, "frame pointers must be multiples of " + std::to_string(v.unit()) + " bytes (" + v.unit_name() + ")");
    const unsigned sh = 8u * ((unsigned)v.S - 1u), smask = v.S == 1 ? 0xFFu : 0xFFFFu;
    // (pitches and offsets are below 2^31: the resolvers; they are used only when the span is, too)
    c.fmt = v;
    c.L = {(unsigned)c.fs.pitch, (unsigned)c.fs.cpitch, (unsigned)c.fs.o1, (unsigned)c.fs.o2, (unsigned)c.fd.pitch, (unsigned)c.fd.cpitch, (unsigned)c.fd.o1, (unsigned)c.fd.o2,
           {fill ? fill[0] & smask : 16u << sh, fill ? fill[1] & smask : 128u << sh, fill ? fill[2] & smask : 128u << sh}};
    return PB_OK;
}
// the plain calls: nearest (pb_video_hot_kernel) and bilinear (pb_planar_bilinear_kernel, with pairs for NV12)
static int pb_video_call(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const void* src_layout, const void* dst_layout, const PbVideoFmt& v,
                         const uint16_t fill[3], void* stream, int interpolation, const char* name) {
    PbVideoCall c;
    int rc = pb_video_check(plan, src_dev, dst_dev, n_frames, src_layout, dst_layout, v, fill, c);
    if (rc != PB_OK || n_frames == 0) return rc;
    rc = pb_check_device(plan);
    if (rc != PB_OK) return rc;
    const PbRoute r = pb_route(plan, interpolation, 1, 0, false, 3, &v);
    if ((r.kind == PbRoute::VIDEO || r.kind == PbRoute::VIDEO_BIL || r.kind == PbRoute::VIDEO_STITCH) && !c.span_fits())
        return pb_fail(PB_ERR_UNSUPPORTED, std::string(name) + " takes frames whose planes span less than 2^31 bytes: use pb_index_map_i32 and gather the " + v.planes() + " planes");
    return pb_launch(plan, r, static_cast<const uint8_t*>(src_dev), static_cast<uint8_t*>(dst_dev), n_frames, c.fs.stride, c.fd.stride, (hipStream_t)stream, &c.L);
}
// (packed frames; a pitched layout's span is the call's to check)
static int pb_video_supported(const pb_plan* plan, const PbVideoFmt& v, int interpolation) {
    if (!plan) return pb_fail(PB_ERR_INVALID, "null argument");
    if (int rc = pb_video_fmt_check(plan, v)) return rc;
    PbVideoCall c;
    if (pb_video_resolve(v, "source", nullptr, plan->P.src, c.fs) != PB_OK || pb_video_resolve(v, "destination", nullptr, plan->P.dst, c.fd) != PB_OK) return 0;
    const PbRoute::Kind k = pb_route(plan, interpolation, 1, 0, false, 3, &v).kind;
    return (k == PbRoute::VIDEO || k == PbRoute::VIDEO_BIL || k == PbRoute::VIDEO_STITCH) && c.span_fits();
}
static PbVideoFmt pb_fmt_nv12(int bytes_per_sample) { return {true, PB_PLANAR_420, bytes_per_sample}; }
static PbVideoFmt pb_fmt_planar(int subsampling, int bytes_per_sample) { return {false, subsampling, bytes_per_sample}; }
static PbVideoFmt pb_fmt_stitch(PbVideoFmt v) {
    v.stitch = true;
    return v;
}
int pb_stitch_nv12(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_nv12_layout* src_layout, const pb_nv12_layout* dst_layout,
                   int bytes_per_sample, const uint16_t fill_yuv[3], void* stream) {
    return pb_video_call(plan, src_dev, dst_dev, n_frames, src_layout, dst_layout, pb_fmt_stitch(pb_fmt_nv12(bytes_per_sample)), fill_yuv, stream, PB_INTERP_NEAREST, "pb_stitch_nv12");
}
int pb_stitch_planar(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_planar_layout* src_layout, const pb_planar_layout* dst_layout,
                     int subsampling, int bytes_per_sample, const uint16_t fill[3], void* stream) {
    return pb_video_call(plan, src_dev, dst_dev, n_frames, src_layout, dst_layout, pb_fmt_stitch(pb_fmt_planar(subsampling, bytes_per_sample)), fill, stream, PB_INTERP_NEAREST,
                         "pb_stitch_planar");
}
int pb_stitch_nv12_supported(const pb_plan* plan, int bytes_per_sample) { return pb_video_supported(plan, pb_fmt_stitch(pb_fmt_nv12(bytes_per_sample)), PB_INTERP_NEAREST); }
int pb_stitch_planar_supported(const pb_plan* plan, int subsampling, int bytes_per_sample) {
    return pb_video_supported(plan, pb_fmt_stitch(pb_fmt_planar(subsampling, bytes_per_sample)), PB_INTERP_NEAREST);
}
int pb_remap_nv12_bilinear(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_nv12_layout* src_layout, const pb_nv12_layout* dst_layout,
                           int bytes_per_sample, const uint16_t fill_yuv[3], void* stream) {
    return pb_video_call(plan, src_dev, dst_dev, n_frames, src_layout, dst_layout, pb_fmt_nv12(bytes_per_sample), fill_yuv, stream, PB_INTERP_BILINEAR, "pb_remap_nv12_bilinear");
}
int pb_remap_nv12(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_nv12_layout* src_layout, const pb_nv12_layout* dst_layout,
                  int bytes_per_sample, const uint16_t fill_yuv[3], void* stream) {
    return pb_video_call(plan, src_dev, dst_dev, n_frames, src_layout, dst_layout, pb_fmt_nv12(bytes_per_sample), fill_yuv, stream, PB_INTERP_NEAREST, "pb_remap_nv12");
}
int pb_remap_nv12_supported(const pb_plan* plan, int bytes_per_sample) { return pb_video_supported(plan, pb_fmt_nv12(bytes_per_sample), PB_INTERP_NEAREST); }
int pb_remap_nv12_bilinear_supported(const pb_plan* plan, int bytes_per_sample) { return pb_video_supported(plan, pb_fmt_nv12(bytes_per_sample), PB_INTERP_BILINEAR); }
int pb_remap_planar(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_planar_layout* src_layout, const pb_planar_layout* dst_layout,
                    int subsampling, int bytes_per_sample, const uint16_t fill[3], void* stream) {
    return pb_video_call(plan, src_dev, dst_dev, n_frames, src_layout, dst_layout, pb_fmt_planar(subsampling, bytes_per_sample), fill, stream, PB_INTERP_NEAREST, "pb_remap_planar");
}
int pb_remap_planar_bilinear(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_planar_layout* src_layout, const pb_planar_layout* dst_layout,
                             int subsampling, int bytes_per_sample, const uint16_t fill[3], void* stream) {
    return pb_video_call(plan, src_dev, dst_dev, n_frames, src_layout, dst_layout, pb_fmt_planar(subsampling, bytes_per_sample), fill, stream, PB_INTERP_BILINEAR,
                         "pb_remap_planar_bilinear");
}
int pb_remap_planar_supported(const pb_plan* plan, int subsampling, int bytes_per_sample) {
    return pb_video_supported(plan, pb_fmt_planar(subsampling, bytes_per_sample), PB_INTERP_NEAREST);
}
int pb_remap_planar_bilinear_supported(const pb_plan* plan, int subsampling, int bytes_per_sample) {
    return pb_video_supported(plan, pb_fmt_planar(subsampling, bytes_per_sample), PB_INTERP_BILINEAR);
}

int pb_remap_u8v(const pb_plan* plan, const uint8_t* const* src_dev, uint8_t* const* dst_dev, int n_frames, void* stream) {
    size_t ss = 0, ds = 0;
    const int rc = pb_check_frames(plan, src_dev, dst_dev, n_frames, 1, ss, ds, true);
    if (rc != PB_OK || n_frames == 0) return rc;
    bool aligned = true;
    for (int f = 0; f < n_frames; ++f) {
        if (!src_dev[f] || !dst_dev[f]) return pb_fail(PB_ERR_INVALID, "null frame pointer");
        aligned = aligned && pb_aligned16(src_dev[f], 0);
    }
    hipStream_t st = (hipStream_t)stream;
    const PbRoute r = pb_route(plan, PB_INTERP_NEAREST, 1, 0, aligned);
    if (r.kind != PbRoute::DOUBLE && r.kind != PbRoute::WIN) {
        // frames LDS-DMA cannot address, deferred plans, the float64 mode: the frames one by one (same bytes, n launches)
        for (int f = 0; f < n_frames; ++f) {
            const int rf = pb_launch(plan, pb_route(plan, PB_INTERP_NEAREST, 1, 0, pb_aligned16(src_dev[f], ss)), src_dev[f], dst_dev[f], 1, ss, ds, st);
            if (rf != PB_OK) return rf;
        }
        return PB_OK;
    }
    // the VEC instantiations of the two windowed kernels: frame f's pointers from a by-value table, at most PB_MAX_VFRAMES per launch
    const PbParams& P = plan->P;
    const unsigned gpf = plan->nearest.lt.groups;
    for (int f0 = 0; f0 < n_frames; f0 += PB_MAX_VFRAMES) {
        const int nf = n_frames - f0 < PB_MAX_VFRAMES ? n_frames - f0 : PB_MAX_VFRAMES;
        PbFrameTab tab;
        for (int f = 0; f < PB_MAX_VFRAMES; ++f) {
            tab.src[f] = src_dev[f0 + (f < nf ? f : 0)];
            tab.dst[f] = dst_dev[f0 + (f < nf ? f : 0)];
        }
        const dim3 grid(gpf * (unsigned)nf), block(64 * PB_TILE_WAVES);
        if (r.kind == PbRoute::DOUBLE)
            pb_pick_wmode(plan, [&](auto W) {
                hipLaunchKernelGGL((pb_hot_double_kernel<W.value, true, true>), grid, block, pb_window_lds_bytes(P, 8), st, P, plan->cert.table, plan->cert.table_r,
                                   plan->nearest.lt.entries, pb_sep_rows(plan), plan->cert.lat_tab, plan->cert.fix_px, plan->cert.dbl_px_fix, plan->cert.dbl_tile_fix, tab.src[0], tab.dst[0], nf,
                                   0ull, 0ull, gpf, 1, tab);
            });
        else
            pb_pick_kind(P, [&](auto K) {
                hipLaunchKernelGGL((pb_hot_win_kernel<K.value, true>), grid, block, pb_window_lds_bytes(P), st, (const PbParams*)plan->nearest.P_dev, pb_hot_of_host(P),
                                   plan->nearest.lt.entries, tab.src[0], tab.dst[0], gpf, 0ull, 0ull, plan->cert.idx_tab, plan->cert.fix_px, plan->cert.fix_idx, (unsigned)nf, tab);
            });
    }
    PB_HIP(hipGetLastError());
    return PB_OK;
}

int pb_remap_bilinear_u8(const pb_plan* plan, const uint8_t* src_dev, uint8_t* dst_dev, int n_frames, size_t src_frame_stride,
                         size_t dst_frame_stride, void* stream) {
    const int rc = pb_check_frames(plan, src_dev, dst_dev, n_frames, 1, src_frame_stride, dst_frame_stride);
    if (rc != PB_OK || n_frames == 0) return rc;
    return pb_launch(plan, pb_route(plan, PB_INTERP_BILINEAR, 1, 0, pb_aligned16(src_dev, src_frame_stride)), src_dev, dst_dev, n_frames,
                     src_frame_stride, dst_frame_stride, (hipStream_t)stream);
}

int pb_remap_catmull_rom_u8(const pb_plan* plan, const uint8_t* src_dev, uint8_t* dst_dev, int n_frames, size_t src_frame_stride,
                            size_t dst_frame_stride, void* stream) {
    const int rc = pb_check_frames(plan, src_dev, dst_dev, n_frames, 1, src_frame_stride, dst_frame_stride);
    if (rc != PB_OK || n_frames == 0) return rc;
    return pb_launch(plan, pb_route(plan, PB_INTERP_CATMULL_ROM, 1, 0, pb_aligned16(src_dev, src_frame_stride)), src_dev, dst_dev, n_frames,
                     src_frame_stride, dst_frame_stride, (hipStream_t)stream);
}

// a rotation table's checks, shared by the rotation-track entry points: null, alignment, the count per frame, the sum with the plan's own
static int pb_track_table_check(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame) {
    if (!rot3x3_dev) return pb_fail(PB_ERR_INVALID, "null rotation table");
    if ((uintptr_t)rot3x3_dev & 7u) return pb_fail(PB_ERR_INVALID, "the rotation table must be 8-byte aligned");
    if (n_rot_per_frame < 1) return pb_fail(PB_ERR_INVALID, "n_rot_per_frame must be at least 1");
    const PbParams& P = plan->P;
    if (n_rot_per_frame > PB_MAX_ROTATIONS - P.n_rot)
        return pb_fail(PB_ERR_INVALID, "the plan's " + std::to_string(P.n_rot) + " rotations and " + std::to_string(n_rot_per_frame) + " per frame exceed PB_MAX_ROTATIONS (" +
                                           std::to_string(PB_MAX_ROTATIONS) + ")");
    return PB_OK;
}
// the frames of one launch of a rotation-track kernel: chunks of `fpc` frames over the grid's y, which ends at 65535
static int pb_track_fpc() { return std::max(1, pb_knob("PB_TRACK_FRAMES", PB_TRACK_FRAMES)); }  // (the knob: the diagnostic build's, for the measurement of DESIGN 3.13)
// The launches of every rotation-track entry point: one per 65535 chunks, launch(rot, s, d, nf, chunks, fpc) for the nf frames from
// `s` / `d` on with their matrices from `rot` on.  Callers have checked the plan's device: pb_remap_track_u8 and pb_remap_track_px in
// pb_check_frames (which returns before it for no frames at all, as they do before any launch), pb_track_video_call by itself.
extern "C++" template <class LAUNCH>
static int pb_track_launch(int n_frames, const double* rot3x3_dev, int n_rot_per_frame, const void* src, void* dst, size_t src_stride, size_t dst_stride, LAUNCH launch) {
    const int fpc = pb_track_fpc();
    const int per_launch = 65535 * fpc;
    for (int f0 = 0; f0 < n_frames; f0 += per_launch) {
        const int nf = n_frames - f0 < per_launch ? n_frames - f0 : per_launch;
        launch(rot3x3_dev + 9ull * (unsigned)n_rot_per_frame * (unsigned)f0, static_cast<const uint8_t*>(src) + (unsigned long long)f0 * src_stride,
               static_cast<uint8_t*>(dst) + (unsigned long long)f0 * dst_stride, nf, (unsigned)((nf + fpc - 1) / fpc), fpc);
    }
    PB_HIP(hipGetLastError());
    return PB_OK;
}
// the sampling modes of pb_remap_track_u8 and pb_remap_track_px
static int pb_track_interp_check(int interpolation) {
    if (interpolation != PB_INTERP_NEAREST && interpolation != PB_INTERP_BILINEAR && interpolation != PB_INTERP_CATMULL_ROM)
        return pb_fail(PB_ERR_INVALID, "interpolation must be PB_INTERP_NEAREST, PB_INTERP_BILINEAR or PB_INTERP_CATMULL_ROM");
    return PB_OK;
}

// A rotation track: the float64 chain of the plan's parameter block with frame f's matrices behind the plan's own.  No route:
// no table of the plan is certified for these chains, so every plan state takes the same kernels.
int pb_remap_track_u8(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, int interpolation, const uint8_t* src_dev, uint8_t* dst_dev,
                      int n_frames, size_t src_frame_stride, size_t dst_frame_stride, void* stream) {
    const int rc = pb_check_frames(plan, src_dev, dst_dev, n_frames, 1, src_frame_stride, dst_frame_stride);
    if (rc != PB_OK) return rc;
    if (int rt = pb_track_table_check(plan, rot3x3_dev, n_rot_per_frame)) return rt;
    const PbParams& P = plan->P;
    if (int ri = pb_track_interp_check(interpolation)) return ri;
    if (n_frames == 0) return PB_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long npx = (unsigned long long)P.dst.height * P.dst.width;
    // (the stride is part of the test, so what holds for the batch holds for every launch's first frame)
    const int dst_aligned = (((uintptr_t)dst_dev | dst_frame_stride) & 3u) == 0;
    const auto some_frames = [&](const double* rot, const uint8_t* s, uint8_t* d, int nf, unsigned chunks, int fpc) {  // (one launch: nf frames, their matrices from rot on)
        if (interpolation == PB_INTERP_NEAREST) {
            pb_pick_any_kind(P, [&](auto K) {
                hipLaunchKernelGGL(pb_track_kernel_of<K.value>(), dim3(pb_blocks((npx + PB_PX - 1) / PB_PX), chunks), dim3(PB_BLOCK), 0, st, P, rot, n_rot_per_frame, fpc, s, d,
                                   nf, (unsigned long long)src_frame_stride, (unsigned long long)dst_frame_stride, dst_aligned);
            });
        } else {
            pb_pick_any_kind(P, [&](auto K) {
                pb_pick_filter(interpolation, [&](auto F) {
                    hipLaunchKernelGGL((pb_track_interp_kernel_of<K.value, decltype(F)>()), dim3(pb_blocks(npx), chunks), dim3(PB_BLOCK), 0, st, P, rot, n_rot_per_frame, fpc, s, d,
                                       nf, (unsigned long long)src_frame_stride, (unsigned long long)dst_frame_stride);
                });
            });
        }
    };
    return pb_track_launch(n_frames, rot3x3_dev, n_rot_per_frame, src_dev, dst_dev, src_frame_stride, dst_frame_stride, some_frames);
}

// A rotation track of frames whose pixel is not three bytes: pb_remap_track_u8's checks with the pixel size, its launches
// with pb_track_px_kernel / pb_track_px_interp_kernel.  channels 3 of one byte is pb_remap_track_u8 itself.
static bool pb_track_px_format_ok(int channels, int sample_bytes) { return channels >= 1 && channels <= 4 && (sample_bytes == 1 || sample_bytes == 2); }
static const char* const pb_track_px_format_msg = "channels must be 1, 2, 3 or 4 and sample_bytes 1 or 2";
static const char* const pb_track_px_double_msg =
    "pb_remap_track_px takes a double-fisheye source with 8-bit samples only (the reference narrows the blend of 16-bit samples to uint8): use "
    "pb_sample_map_bilinear_px / pb_sample_map_catmull_rom_px or pb_index_from_map_i32 + pb_gather_blend_u8 per frame";
int pb_remap_track_px(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, int interpolation, const void* src_dev, void* dst_dev, int n_frames,
                      size_t src_frame_stride, size_t dst_frame_stride, int channels, int sample_bytes, void* stream) {
    const bool fmt = pb_track_px_format_ok(channels, sample_bytes);
    const int B = fmt ? channels * sample_bytes : 1;  // (a format outside the sets is refused below, in its place: the weakest alignment until then)
    if (B == 3) return pb_remap_track_u8(plan, rot3x3_dev, n_rot_per_frame, interpolation, static_cast<const uint8_t*>(src_dev), static_cast<uint8_t*>(dst_dev),
                                         n_frames, src_frame_stride, dst_frame_stride, stream);
    const int rc = pb_check_frames(plan, src_dev, dst_dev, n_frames, 1, src_frame_stride, dst_frame_stride, false, B);
    if (rc != PB_OK) return rc;
    if (int rt = pb_track_table_check(plan, rot3x3_dev, n_rot_per_frame)) return rt;
    const PbParams& P = plan->P;
    if (int ri = pb_track_interp_check(interpolation)) return ri;
    if (!fmt) return pb_fail(PB_ERR_INVALID, pb_track_px_format_msg);
    if (P.src.kind == PB_KIND_DOUBLE && sample_bytes != 1) return pb_fail(PB_ERR_UNSUPPORTED, pb_track_px_double_msg);
    if (n_frames == 0) return PB_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long npx = (unsigned long long)P.dst.height * P.dst.width;
    const auto some_frames = [&](const double* rot, const uint8_t* s, uint8_t* d, int nf, unsigned chunks, int fpc) {  // (one launch: nf frames, their matrices from rot on)
        if (interpolation == PB_INTERP_NEAREST) {
            pb_pick_any_kind(P, [&](auto K) {
                hipLaunchKernelGGL(pb_track_px_kernel_of<K.value>(), dim3(pb_blocks((npx + PB_PX - 1) / PB_PX), chunks), dim3(PB_BLOCK), 0, st, P, rot, n_rot_per_frame, fpc,
                                   s, d, nf, (unsigned long long)src_frame_stride, (unsigned long long)dst_frame_stride, B);
            });
        } else {
            const auto launch = [&](auto K, auto* sample) {  // (the sample type: uint8_t or uint16_t)
                using SAMPLE = std::remove_pointer_t<decltype(sample)>;
                pb_pick_filter(interpolation, [&](auto F) {
                    hipLaunchKernelGGL((pb_track_px_interp_kernel_of<K.value, decltype(F), SAMPLE>()), dim3(pb_blocks(npx), chunks), dim3(PB_BLOCK), 0, st, P, rot,
                                       n_rot_per_frame, fpc, s, d, nf, (unsigned long long)src_frame_stride, (unsigned long long)dst_frame_stride, channels);
                });
            };
            if (P.src.kind == PB_KIND_DOUBLE) launch(PbInt<PB_KIND_DOUBLE>(), (uint8_t*)nullptr);
            else if (sample_bytes == 1) pb_pick_exact_kind(P, [&](auto K) { launch(K, (uint8_t*)nullptr); });
            else pb_pick_exact_kind(P, [&](auto K) { launch(K, (uint16_t*)nullptr); });
        }
    };
    return pb_track_launch(n_frames, rot3x3_dev, n_rot_per_frame, src_dev, dst_dev, src_frame_stride, dst_frame_stride, some_frames);
}
int pb_remap_track_px_supported(const pb_plan* plan, int channels, int sample_bytes) {
    if (!plan) return pb_fail(PB_ERR_INVALID, "null argument");
    if (!pb_track_px_format_ok(channels, sample_bytes)) return pb_fail(PB_ERR_INVALID, pb_track_px_format_msg);
    return (plan->P.src.kind == PB_KIND_DOUBLE && sample_bytes != 1) ? 0 : 1;
}

// The interpolating modes for frames whose pixel is not uint8 RGB: pb_remap_px's frame checks with the pixel size, the
// interpolation's, the format's, then the route - pb_px_interp_kernel on the bilinear mode's tables, or nothing.  channels 3 of one byte
// is pb_remap_bilinear_u8 / pb_remap_catmull_rom_u8 itself, on every plan those take.
static int pb_interp_px_check(int interpolation, const char* call = "pb_remap_interp_px") {
    if (interpolation == PB_INTERP_NEAREST)
        return pb_fail(PB_ERR_INVALID, std::string(call) + " samples with PB_INTERP_BILINEAR or PB_INTERP_CATMULL_ROM: PB_INTERP_NEAREST is pb_remap_px");
    if (interpolation != PB_INTERP_BILINEAR && interpolation != PB_INTERP_CATMULL_ROM)
        return pb_fail(PB_ERR_INVALID, "interpolation must be PB_INTERP_BILINEAR or PB_INTERP_CATMULL_ROM");
    return PB_OK;
}
int pb_remap_interp_px(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, size_t src_frame_stride, size_t dst_frame_stride, int channels,
                       int sample_bytes, int interpolation, void* stream) {
    const bool fmt = pb_track_px_format_ok(channels, sample_bytes);
    const int B = fmt ? channels * sample_bytes : 1;  // (a format outside the sets is refused below, in its place: the weakest alignment until then)
    const int rc = pb_check_frames(plan, src_dev, dst_dev, n_frames, 1, src_frame_stride, dst_frame_stride, false, B);
    if (rc != PB_OK) return rc;
    if (int ri = pb_interp_px_check(interpolation)) return ri;
    if (!fmt) return pb_fail(PB_ERR_INVALID, pb_track_px_format_msg);
    if (n_frames == 0) return PB_OK;
    const uint8_t* s = static_cast<const uint8_t*>(src_dev);
    uint8_t* d = static_cast<uint8_t*>(dst_dev);
    if (B == 3)
        return interpolation == PB_INTERP_BILINEAR ? pb_remap_bilinear_u8(plan, s, d, n_frames, src_frame_stride, dst_frame_stride, stream)
                                                   : pb_remap_catmull_rom_u8(plan, s, d, n_frames, src_frame_stride, dst_frame_stride, stream);
    const PbRoute r = pb_route(plan, interpolation, 1, 0, false, B, nullptr, sample_bytes);
    if ((r.kind == PbRoute::PX_INTERP || r.kind == PbRoute::PX_INTERP_FLOAT64) && !pb_px_frames_fit(plan, B))
        return pb_fail(PB_ERR_UNSUPPORTED, "pb_remap_interp_px takes frames below 2^31 bytes: use pb_sample_map_bilinear_px / pb_sample_map_catmull_rom_px");
    return pb_launch(plan, r, s, d, n_frames, src_frame_stride, dst_frame_stride, (hipStream_t)stream);
}
int pb_remap_interp_px_supported(const pb_plan* plan, int channels, int sample_bytes, int interpolation) {
    if (!plan) return pb_fail(PB_ERR_INVALID, "null argument");
    if (int ri = pb_interp_px_check(interpolation)) return ri;
    if (!pb_track_px_format_ok(channels, sample_bytes)) return pb_fail(PB_ERR_INVALID, pb_track_px_format_msg);
    const int B = channels * sample_bytes;
    if (B == 3) return 1;
    const PbRoute::Kind k = pb_route(plan, interpolation, 1, 0, false, B, nullptr, sample_bytes).kind;
    return (k == PbRoute::PX_INTERP || k == PbRoute::PX_INTERP_FLOAT64) && pb_px_frames_fit(plan, B);
}

// The interpolating modes for frames of float16 / float32 samples: pb_remap_interp_px's order - the frame checks with the
// pixel size (12 and 16 bytes here alone), the interpolation's, the format's, no frames, then the route - pb_pxf_interp_kernel on the
// bilinear mode's tables, or nothing.
static bool pb_pxf_format_ok(int channels, int sample_bytes) { return channels >= 1 && channels <= 4 && (sample_bytes == 2 || sample_bytes == 4); }
static const char* const pb_pxf_format_msg = "channels must be 1, 2, 3 or 4 and sample_bytes 2 (float16) or 4 (float32)";
int pb_remap_interp_pxf(const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, size_t src_frame_stride, size_t dst_frame_stride, int channels,
                        int sample_bytes, int interpolation, void* stream) {
    const bool fmt = pb_pxf_format_ok(channels, sample_bytes);
    const int B = fmt ? channels * sample_bytes : 1;  // (a format outside the sets is refused below, in its place: the weakest alignment until then)
    const int rc = pb_check_frames(plan, src_dev, dst_dev, n_frames, 1, src_frame_stride, dst_frame_stride, false, B, true);
    if (rc != PB_OK) return rc;
    if (int ri = pb_interp_px_check(interpolation, "pb_remap_interp_pxf")) return ri;
    if (!fmt) return pb_fail(PB_ERR_INVALID, pb_pxf_format_msg);
    if (n_frames == 0) return PB_OK;
    const PbRoute r = pb_route(plan, interpolation, 1, 0, false, B, nullptr, sample_bytes, true);
    if (r.kind == PbRoute::PXF_INTERP && !pb_px_frames_fit(plan, B))
        return pb_fail(PB_ERR_UNSUPPORTED, "pb_remap_interp_pxf takes frames below 2^31 bytes");
    return pb_launch(plan, r, static_cast<const uint8_t*>(src_dev), static_cast<uint8_t*>(dst_dev), n_frames, src_frame_stride, dst_frame_stride, (hipStream_t)stream);
}
int pb_remap_interp_pxf_supported(const pb_plan* plan, int channels, int sample_bytes, int interpolation) {
    if (!plan) return pb_fail(PB_ERR_INVALID, "null argument");
    if (int ri = pb_interp_px_check(interpolation, "pb_remap_interp_pxf")) return ri;
    if (!pb_pxf_format_ok(channels, sample_bytes)) return pb_fail(PB_ERR_INVALID, pb_pxf_format_msg);
    const int B = channels * sample_bytes;
    return pb_route(plan, interpolation, 1, 0, false, B, nullptr, sample_bytes, true).kind == PbRoute::PXF_INTERP && pb_px_frames_fit(plan, B);
}
int pb_plan_px_interp_route(const pb_plan* plan, int channels, int sample_bytes, int interpolation) {
    const int ok = pb_remap_interp_px_supported(plan, channels, sample_bytes, interpolation);
    if (ok != 1) return ok;
    if (channels * sample_bytes == 3) return 3;
    return pb_route(plan, interpolation, 1, 0, false, channels * sample_bytes, nullptr, sample_bytes).kind == PbRoute::PX_INTERP ? 1 : 2;
}

// A rotation track of video frames (bilinear: 3.19): the plain video calls' argument checks, then pb_remap_track_u8's
// table checks; the launches are pb_track_launch's.  Nearest: pb_track_video_kernel; bilinear:
// pb_track_video_bilinear_kernel, a panorama or camera source (both with pairs for NV12).
// A format with `stitch` (pb_track_stitch_nv12 / _planar) takes a double-fisheye source and no other: pb_track_stitch_kernel.
static int pb_track_video_call(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames,
                               const void* src_layout, const void* dst_layout, const PbVideoFmt& v, const uint16_t fill[3], void* stream, int interpolation,
                               const char* name) {
    PbVideoCall c;
    int rc = pb_video_check(plan, src_dev, dst_dev, n_frames, src_layout, dst_layout, v, fill, c);
    if (rc == PB_OK) rc = pb_track_table_check(plan, rot3x3_dev, n_rot_per_frame);
    if (rc != PB_OK || n_frames == 0) return rc;
    rc = pb_check_device(plan);
    if (rc != PB_OK) return rc;
    const PbParams& P = plan->P;
    if (v.stitch && P.src.kind != PB_KIND_DOUBLE)
        return pb_fail(PB_ERR_UNSUPPORTED, std::string(name) + " takes double-fisheye sources: use " + (v.pairs ? "pb_remap_track_nv12" : "pb_remap_track_planar") +
                                               " for a single source");
    if (!v.stitch && P.src.kind == PB_KIND_DOUBLE)
        return pb_fail(PB_ERR_UNSUPPORTED, std::string(name) + " takes single sources (a double fisheye's blend is sample-typed): convert to RGB8 and use pb_remap_track_u8");
    if (interpolation == PB_INTERP_BILINEAR && pb_is_cube(P.src.kind))
        return pb_fail(PB_ERR_UNSUPPORTED, std::string(name) + " takes panorama and camera sources (the bilinear definition of video frames covers no cube map): convert to "
                                                               "RGB8 and use pb_remap_track_u8");
    if (!c.span_fits() || P.src.height >= 32768 || P.src.width >= 32768)
        return pb_fail(PB_ERR_UNSUPPORTED, std::string(name) + " takes frames whose planes span less than 2^31 bytes and sources below 32768 px a side: use a plan per "
                                                               "frame with pb_index_map_i32 and gather the " + v.planes() + " planes");
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long quads = (unsigned long long)P.dst.height * (((unsigned)P.dst.width + PB_PX - 1) / PB_PX);
    const int cx = v.cx(), cy = v.cy();
    const auto some_frames = [&](const double* rot, const uint8_t* s, uint8_t* d, int nf, unsigned chunks, int fpc) {  // (one launch: nf frames, their matrices from rot on)
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(pb_blocks(quads), chunks), dim3(PB_BLOCK), 0, st, P, rot, n_rot_per_frame, fpc, s, d, nf, c.fs.stride, c.fd.stride, c.L, cx, cy);
        };
        pb_pick<1, 0>(v.pairs, [&](auto PAIRS) {
            pb_pick<1, 2>(v.S == 1, [&](auto S) {
                if (v.stitch) launch(pb_track_stitch_kernel<S.value, PAIRS.value != 0>);
                else if (interpolation == PB_INTERP_BILINEAR) pb_pick_kind(P, [&](auto K) { launch(pb_track_video_bilinear_kernel<S.value, K.value, PAIRS.value != 0>); });
                else pb_pick_exact_kind(P, [&](auto K) { launch(pb_track_video_kernel<S.value, K.value, PAIRS.value != 0>); });
            });
        });
    };
    return pb_track_launch(n_frames, rot3x3_dev, n_rot_per_frame, src_dev, dst_dev, c.fs.stride, c.fd.stride, some_frames);
}
int pb_remap_track_nv12(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames,
                        const pb_nv12_layout* src_layout, const pb_nv12_layout* dst_layout, int bytes_per_sample, const uint16_t fill_yuv[3], void* stream) {
    return pb_track_video_call(plan, rot3x3_dev, n_rot_per_frame, src_dev, dst_dev, n_frames, src_layout, dst_layout, pb_fmt_nv12(bytes_per_sample), fill_yuv, stream,
                               PB_INTERP_NEAREST, "pb_remap_track_nv12");
}
int pb_remap_track_nv12_bilinear(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames,
                                 const pb_nv12_layout* src_layout, const pb_nv12_layout* dst_layout, int bytes_per_sample, const uint16_t fill_yuv[3], void* stream) {
    return pb_track_video_call(plan, rot3x3_dev, n_rot_per_frame, src_dev, dst_dev, n_frames, src_layout, dst_layout, pb_fmt_nv12(bytes_per_sample), fill_yuv, stream,
                               PB_INTERP_BILINEAR, "pb_remap_track_nv12_bilinear");
}
int pb_remap_track_planar(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames,
                          const pb_planar_layout* src_layout, const pb_planar_layout* dst_layout, int subsampling, int bytes_per_sample, const uint16_t fill[3],
                          void* stream) {
    return pb_track_video_call(plan, rot3x3_dev, n_rot_per_frame, src_dev, dst_dev, n_frames, src_layout, dst_layout, pb_fmt_planar(subsampling, bytes_per_sample), fill,
                               stream, PB_INTERP_NEAREST, "pb_remap_track_planar");
}
int pb_remap_track_planar_bilinear(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames,
                                   const pb_planar_layout* src_layout, const pb_planar_layout* dst_layout, int subsampling, int bytes_per_sample, const uint16_t fill[3],
                                   void* stream) {
    return pb_track_video_call(plan, rot3x3_dev, n_rot_per_frame, src_dev, dst_dev, n_frames, src_layout, dst_layout, pb_fmt_planar(subsampling, bytes_per_sample), fill,
                               stream, PB_INTERP_BILINEAR, "pb_remap_track_planar_bilinear");
}

// ... of a double fisheye: the same checks and launches around pb_track_stitch_kernel
int pb_track_stitch_nv12(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames,
                         const pb_nv12_layout* src_layout, const pb_nv12_layout* dst_layout, int bytes_per_sample, const uint16_t fill_yuv[3], void* stream) {
    return pb_track_video_call(plan, rot3x3_dev, n_rot_per_frame, src_dev, dst_dev, n_frames, src_layout, dst_layout, pb_fmt_stitch(pb_fmt_nv12(bytes_per_sample)), fill_yuv,
                               stream, PB_INTERP_NEAREST, "pb_track_stitch_nv12");
}
int pb_track_stitch_planar(const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames,
                           const pb_planar_layout* src_layout, const pb_planar_layout* dst_layout, int subsampling, int bytes_per_sample, const uint16_t fill[3],
                           void* stream) {
    return pb_track_video_call(plan, rot3x3_dev, n_rot_per_frame, src_dev, dst_dev, n_frames, src_layout, dst_layout,
                               pb_fmt_stitch(pb_fmt_planar(subsampling, bytes_per_sample)), fill, stream, PB_INTERP_NEAREST, "pb_track_stitch_planar");
}

int pb_index_map_i32(const pb_plan* plan, int32_t* idx_dev, double* weights_dev, void* stream) {
    if (!plan || !idx_dev) return pb_fail(PB_ERR_INVALID, "null argument");
    const int rc = pb_check_device(plan);
    if (rc != PB_OK) return rc;
    const PbParams& P = plan->P;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = pb_blocks((unsigned long long)P.dst.height * P.dst.width);
    if (pb_use_fast(plan))
        pb_launch_direct<1>(plan, nullptr, nullptr, 0, 0, 0, idx_dev, st);
    else
        pb_pick_any_kind(P, [&](auto K) {
            PB_LAUNCH_BY_ROT(P, pb_index_kernel, K.value, dim3(blocks), dim3(PB_BLOCK), 0, st, P, idx_dev, weights_dev);
        });
    PB_HIP(hipGetLastError());
    return PB_OK;
}

#ifdef PB_ABLATION  // diagnostic build only (tests/test_hip_math.py): pb_math.hpp's correctly rounded functions as the gfx950 build evaluates them
}  // extern "C"
__global__ void pb_debug_math_kernel(int fn, const double* __restrict__ in, double* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    switch (fn) {
        case 0: out[i] = pb_asin_svml(in[i]); break;
        case 1: out[i] = pb_acos_svml(in[i]); break;
        case 2: out[i] = pb_atan_svml(in[i]); break;
        case 3: out[i] = pb_tan_svml(in[i]); break;
        case 8: out[i] = pb_asin_libm(in[i]); break;
        case 9: out[i] = pb_acos_libm(in[i]); break;
        case 10: out[i] = pb_atan_libm(in[i]); break;
        case 11: out[i] = pb_tan_libm(in[i]); break;
        case 4: out[i] = pb_sin_np(in[i]); break;
        case 5: out[i] = pb_cos_np(in[i]); break;
        case 6: pb_expi_np(in[i], &out[2 * i], &out[2 * i + 1]); break;
        default: out[i] = pb_arg_np(in[2 * i], in[2 * i + 1]);
    }
}
extern "C" {
// fn (the order of tests/npmath_args.py FUNCTIONS): 0 arcsin, 1 arccos, 2 arctan, 3 tan, 4 sin, 5 cos of n values; 6: np.exp(x * 1j) -> (imag, real) interleaved; 7: n (y, x) pairs -> np.log(x + 1j y).imag;
// 8-11: arcsin, arccos, arctan, tan of the second math flavour (pb_math_libm.hpp)
__attribute__((visibility("default"))) int pb_debug_math(int fn, const double* in_dev, double* out_dev, size_t n, void* stream) {
    if (!in_dev || !out_dev || fn < 0 || fn > 11) return pb_fail(PB_ERR_INVALID, "bad argument");
    if (n) hipLaunchKernelGGL(pb_debug_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fn, in_dev, out_dev, n);
    PB_HIP(hipGetLastError());
    return PB_OK;
}
#endif

#ifdef PB_TRACE
__attribute__((visibility("default"))) int pb_debug_trace(unsigned long long* out, size_t n_words, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(pb_trace), n_words * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(pb_trace)) != hipSuccess || hipMemset(p, 0, sizeof(unsigned long long) * 65536 * 16) != hipSuccess) return -2;
    }
    return 0;
}
__attribute__((visibility("default"))) int pb_debug_trace_frame(const pb_plan* plan, int frame) {
    // record the waves of frame `frame` of a batch launch (4-wave workgroups); frame < 0: whole launches (single frames)
    const unsigned wpf = (plan && frame >= 0) ? plan->nearest.lt.groups : 0xFFFFFFFFu, f = frame >= 0 ? (unsigned)frame : 0u;
    if (hipMemcpyToSymbol(HIP_SYMBOL(pb_trace_wpf), &wpf, sizeof(wpf)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(pb_trace_frame), &f, sizeof(f)) == hipSuccess ? 0 : -1;
}
__attribute__((visibility("default"))) int pb_debug_copy_table_r(const pb_plan* plan, void* host, size_t bytes) {  // the right eye's table of a double-fisheye plan
    if (!plan || !plan->cert.table_r) return -1;
    const size_t have = (size_t)plan->cert.n_tiles * sizeof(PbTileEntry);
    return hipMemcpy(host, plan->cert.table_r, bytes < have ? bytes : have, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
__attribute__((visibility("default"))) int pb_debug_copy_table(const pb_plan* plan, void* host, size_t bytes) {
    if (!plan || !plan->cert.table) return -1;
    const size_t have = (size_t)plan->cert.n_tiles * sizeof(PbTileEntry);
    return hipMemcpy(host, plan->cert.table, bytes < have ? bytes : have, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
#endif

int pb_plan_set_mode(pb_plan* plan, int mode) {
    if (!plan) return pb_fail(PB_ERR_INVALID, "null argument");
    if (mode < PB_MODE_AUTO || mode > PB_MODE_FAST_DIRECT) return pb_fail(PB_ERR_INVALID, "mode out of range");
    plan->mode = mode;
    return PB_OK;
}

int pb_plan_info(const pb_plan* plan, int* fast_path_enabled, long long* stats7, long long* thresholds4) {
    long long* stats5 = stats7;
    if (!plan) return pb_fail(PB_ERR_INVALID, "null argument");
    if (fast_path_enabled)
        *fast_path_enabled = (pb_use_fast(plan) || ((plan->cert.sep_ready || plan->cert.dbl_ready) && plan->mode != PB_MODE_FAITHFUL)) ? 1 : 0;
    if (stats5) {
        const bool have = plan->cert.fast_ready || plan->cert.dbl_ready;  // a double source counts both eyes' tables
        stats5[0] = have ? (long long)plan->cert.n_tiles : -1;
        stats5[1] = have ? (long long)plan->cert.n_fail_tiles : -1;
        stats5[2] = have ? (long long)plan->cert.n_fix_px : -1;
        stats5[3] = have ? plan->cert.diff_pixels : -1;
        stats5[4] = have ? (long long)plan->cert.n_lean_tiles : -1;
        stats5[5] = have ? (long long)plan->cert.n_black_tiles : -1;
        stats5[6] = have ? (long long)plan->cert.n_direct_tiles : -1;
    }
    if (thresholds4) {
        thresholds4[0] = plan->P.inv_lo[0];
        thresholds4[1] = plan->P.inv_hi[0];
        thresholds4[2] = plan->P.inv_lo[1];
        thresholds4[3] = plan->P.inv_hi[1];
    }
    return PB_OK;
}

int pb_coordmap_f64(const pb_proj* dst, double* map_dev, void* stream) {
    std::string why;
    if (!map_dev) return pb_fail(PB_ERR_INVALID, "null argument");
    if (!pb_end_ok(dst, why, PB_ROLE_DST)) return pb_fail(PB_ERR_INVALID, why);
    PbParams P;
    memset(&P, 0, sizeof(P));
    const PbEndX d = pb_to_end(dst);
    P.dst = P.src = d.e;
    P.poly_dst = P.poly_src = d.poly;
    pb_derive(P);
    const unsigned blocks = pb_blocks((unsigned long long)P.dst.height * P.dst.width);
    if (pb_is_cube(P.dst.kind)) hipLaunchKernelGGL(pb_coordmap_cube_kernel, dim3(blocks), dim3(PB_BLOCK), 0, (hipStream_t)stream, P, map_dev);
    else hipLaunchKernelGGL(pb_coordmap_kernel, dim3(blocks), dim3(PB_BLOCK), 0, (hipStream_t)stream, P, map_dev);
    PB_HIP(hipGetLastError());
    return PB_OK;
}

int pb_rotate_f64(const double* rot3x3, double* map_in_dev, double* map_out_dev, int height, int width, void* stream) {
    if (!rot3x3 || !map_in_dev || !map_out_dev) return pb_fail(PB_ERR_INVALID, "null argument");
    if (map_in_dev == map_out_dev) return pb_fail(PB_ERR_INVALID, "map_out_dev must not alias map_in_dev");
    if (height < 1 || width < 1 || (long long)height * width > 0x7FFFFFFFll / 4)
        return pb_fail(PB_ERR_INVALID, "map size out of range");
    PbMat R;
    for (int e = 0; e < 9; ++e) R.m[e] = rot3x3[e];
    const unsigned total = (unsigned)height * (unsigned)width;
    hipLaunchKernelGGL(pb_rotate_kernel, dim3(pb_blocks(total)), dim3(PB_BLOCK), 0, (hipStream_t)stream, R, map_in_dev,
                       map_out_dev, total);
    PB_HIP(hipGetLastError());
    return PB_OK;
}

}  // extern "C"

// The map-stage calls (a materialised (height, width, 3) map sampled from `src`): their shared argument checks, in the order every one of
// them makes them, and their parameters - only the source half is used.  pb_map_planes_ok: the host-evaluated distance planes.
static int pb_map_stage(bool null_argument, const pb_proj* src, unsigned roles, int height, int width, PbParams& P) {
    std::string why;
    if (null_argument) return pb_fail(PB_ERR_INVALID, "null argument");
    if (!pb_end_ok(src, why, roles)) return pb_fail(PB_ERR_INVALID, why);
    if (height < 1 || width < 1 || (long long)height * width > 0x7FFFFFFFll / 4) return pb_fail(PB_ERR_INVALID, "map size out of range");
    memset(&P, 0, sizeof(P));
    const PbEndX x = pb_to_end(src);
    P.src = x.e;
    P.poly_src = x.poly;
    P.dst = P.src;
    P.dst.kind = PB_KIND_PANO;
    P.dst.height = height;
    P.dst.width = width;
    pb_derive(P);
    return PB_OK;
}
static int pb_map_planes_ok(const pb_proj* src, const double* dist_l_dev, const double* dist_r_dev) {
    if (pb_has_lens(src->kind) && src->lens == PB_LENS_CUSTOM && !dist_l_dev)
        return pb_fail(PB_ERR_INVALID, "a PB_LENS_CUSTOM source needs the host-evaluated distance plane(s)");
    if (src->kind == PB_KIND_DOUBLE && dist_l_dev && !dist_r_dev) return pb_fail(PB_ERR_INVALID, "a double source needs both distance planes");
    if (!pb_has_lens(src->kind) && (dist_l_dev || dist_r_dev)) return pb_fail(PB_ERR_INVALID, pb_is_cube(src->kind) ? "a cube source has no lens" : "a panorama source has no lens");
    return PB_OK;
}

// pb_sample_map_bilinear_px and pb_sample_map_catmull_rom_px: the same arguments, checks and launch
static int pb_sample_map_px(int filter, const pb_proj* src, double* map_dev, int height, int width, const double* dist_l_dev, const double* dist_r_dev,
                            const void* img_dev, void* out_dev, int channels, int sample_bytes, void* stream) {
    PbParams P;
    if (int rc = pb_map_stage(!map_dev || !img_dev || !out_dev, src, PB_ROLE_SRC | PB_ROLE_CUSTOM_OK, height, width, P)) return rc;
    if (channels < 1 || channels > 16) return pb_fail(PB_ERR_INVALID, "channels outside [1, 16]");
    if (sample_bytes != 1 && sample_bytes != 2) return pb_fail(PB_ERR_INVALID, "sample_bytes must be 1 or 2");
    if (int rc = pb_map_planes_ok(src, dist_l_dev, dist_r_dev)) return rc;
    const unsigned total = (unsigned)height * (unsigned)width;
    const auto launch = [&](auto* sample) {  // (the sample type: uint8_t or uint16_t)
        using SAMPLE = std::remove_pointer_t<decltype(sample)>;
        if (pb_is_cube(P.src.kind)) {
            pb_pick_cube_kind(P, [&](auto K) {
                pb_pick_filter(filter, [&](auto F) {
                    hipLaunchKernelGGL((pb_sample_map_interp_cube_kernel_of<K.value, decltype(F), SAMPLE>()), dim3(pb_blocks(total)), dim3(PB_BLOCK), 0,
                                       (hipStream_t)stream, P, map_dev, total, static_cast<const SAMPLE*>(img_dev), out_dev, channels);
                });
            });
            return;
        }
        pb_pick_lensed_kind(P, [&](auto K) {
            pb_pick_filter(filter, [&](auto F) {
                hipLaunchKernelGGL((pb_sample_map_interp_kernel<decltype(F), K.value, SAMPLE>), dim3(pb_blocks(total)), dim3(PB_BLOCK), 0, (hipStream_t)stream,
                                   P, map_dev, total, dist_l_dev, dist_r_dev, static_cast<const SAMPLE*>(img_dev), out_dev, channels);
            });
        });
    };
    if (sample_bytes == 1) launch((uint8_t*)nullptr);
    else launch((uint16_t*)nullptr);
    PB_HIP(hipGetLastError());
    return PB_OK;
}

extern "C" {

int pb_sample_map_u8(const pb_proj* src, double* map_dev, int height, int width, const uint8_t* src_dev,
                     uint8_t* dst_dev, void* stream) {
    PbParams P;
    if (int rc = pb_map_stage(!map_dev || !src_dev || !dst_dev, src, PB_ROLE_SRC, height, width, P)) return rc;
    const unsigned total = (unsigned)height * (unsigned)width;
    pb_pick_any_kind(P, [&](auto K) {
        hipLaunchKernelGGL(pb_sample_map_kernel<K.value>, dim3(pb_blocks(total)), dim3(PB_BLOCK), 0, (hipStream_t)stream, P, map_dev, total, src_dev, dst_dev);
    });
    PB_HIP(hipGetLastError());
    return PB_OK;
}

int pb_index_from_map_i32(const pb_proj* src, double* map_dev, int height, int width, const double* dist_l_dev, const double* dist_r_dev,
                          int32_t* idx_dev, double* weights_dev, void* stream) {
    PbParams P;
    if (int rc = pb_map_stage(!map_dev || !idx_dev, src, PB_ROLE_SRC | PB_ROLE_CUSTOM_OK, height, width, P)) return rc;
    if (int rc = pb_map_planes_ok(src, dist_l_dev, dist_r_dev)) return rc;
    const unsigned total = (unsigned)height * (unsigned)width;
    pb_pick_any_kind(P, [&](auto K) {
        hipLaunchKernelGGL(pb_index_from_map_kernel<K.value>, dim3(pb_blocks(total)), dim3(PB_BLOCK), 0, (hipStream_t)stream, P, map_dev, total, dist_l_dev,
                           dist_r_dev, idx_dev, weights_dev);
    });
    PB_HIP(hipGetLastError());
    return PB_OK;
}

int pb_sample_map_bilinear_px(const pb_proj* src, double* map_dev, int height, int width, const double* dist_l_dev, const double* dist_r_dev,
                              const void* img_dev, void* out_dev, int channels, int sample_bytes, void* stream) {
    return pb_sample_map_px(PB_INTERP_BILINEAR, src, map_dev, height, width, dist_l_dev, dist_r_dev, img_dev, out_dev, channels, sample_bytes, stream);
}

int pb_sample_map_catmull_rom_px(const pb_proj* src, double* map_dev, int height, int width, const double* dist_l_dev, const double* dist_r_dev,
                                 const void* img_dev, void* out_dev, int channels, int sample_bytes, void* stream) {
    return pb_sample_map_px(PB_INTERP_CATMULL_ROM, src, map_dev, height, width, dist_l_dev, dist_r_dev, img_dev, out_dev, channels, sample_bytes, stream);
}

int pb_sample_map_bilinear_u8(const pb_proj* src, double* map_dev, int height, int width, const uint8_t* src_dev, uint8_t* dst_dev, void* stream) {
    return pb_sample_map_bilinear_px(src, map_dev, height, width, nullptr, nullptr, src_dev, dst_dev, 3, 1, stream);
}

int pb_gather_px(const int32_t* idx_dev, const void* src_dev, void* dst_dev, size_t n_px, int bytes_per_px, void* stream) {
    if (!idx_dev || !src_dev || !dst_dev) return pb_fail(PB_ERR_INVALID, "null argument");
    if (bytes_per_px < 1 || bytes_per_px > 64) return pb_fail(PB_ERR_INVALID, "bytes_per_px outside [1, 64]");
    if (n_px > 0x7FFFFFFFull) return pb_fail(PB_ERR_INVALID, "too many pixels");
    if (!n_px) return PB_OK;
    hipLaunchKernelGGL(pb_gather_px_kernel, dim3(pb_blocks(n_px)), dim3(PB_BLOCK), 0, (hipStream_t)stream, idx_dev,
                       static_cast<const uint8_t*>(src_dev), static_cast<uint8_t*>(dst_dev), (unsigned long long)n_px, bytes_per_px);
    PB_HIP(hipGetLastError());
    return PB_OK;
}

int pb_gather_blend_u8(const int32_t* idx2_dev, const double* weights2_dev, const void* src_dev, uint8_t* dst_dev, size_t n_px, int channels,
                       int sample_bytes, void* stream) {
    if (!idx2_dev || !weights2_dev || !src_dev || !dst_dev) return pb_fail(PB_ERR_INVALID, "null argument");
    if (channels < 1 || channels > 16) return pb_fail(PB_ERR_INVALID, "channels outside [1, 16]");
    if (sample_bytes != 1 && sample_bytes != 2) return pb_fail(PB_ERR_UNSUPPORTED, "the double-fisheye blend takes 8- or 16-bit unsigned samples");
    if (n_px > 0x7FFFFFFFull) return pb_fail(PB_ERR_INVALID, "too many pixels");
    if (!n_px) return PB_OK;
    if (sample_bytes == 1)
        hipLaunchKernelGGL(pb_gather_blend_kernel<uint8_t>, dim3(pb_blocks(n_px)), dim3(PB_BLOCK), 0, (hipStream_t)stream, idx2_dev, weights2_dev,
                           static_cast<const uint8_t*>(src_dev), dst_dev, (unsigned long long)n_px, channels);
    else
        hipLaunchKernelGGL(pb_gather_blend_kernel<uint16_t>, dim3(pb_blocks(n_px)), dim3(PB_BLOCK), 0, (hipStream_t)stream, idx2_dev, weights2_dev,
                           static_cast<const uint16_t*>(src_dev), dst_dev, (unsigned long long)n_px, channels);
    PB_HIP(hipGetLastError());
    return PB_OK;
}

int pb_map_projection_u8(double* map_dev, int height, int width, uint8_t* out_dev, void* workspace24_dev, void* stream) {
    if (!map_dev || !out_dev || !workspace24_dev) return pb_fail(PB_ERR_INVALID, "null argument");
    if (height < 1 || width < 1 || (long long)height * width > 0x7FFFFFFFll / 4)
        return pb_fail(PB_ERR_INVALID, "map size out of range");
    const unsigned total = (unsigned)height * (unsigned)width;
    hipStream_t st = (hipStream_t)stream;
    static const unsigned long long init[3] = {~0ull, 0ull, 0ull};
    PB_HIP(hipMemcpyAsync(workspace24_dev, init, sizeof(init), hipMemcpyHostToDevice, st));
    unsigned long long* ws = reinterpret_cast<unsigned long long*>(workspace24_dev);
    hipLaunchKernelGGL(pb_mapproj_minmax_kernel, dim3(pb_blocks(total)), dim3(PB_BLOCK), 0, st, map_dev, total, ws);
    hipLaunchKernelGGL(pb_mapproj_colour_kernel, dim3(pb_blocks(total)), dim3(PB_BLOCK), 0, st, map_dev, total, ws, out_dev);
    PB_HIP(hipGetLastError());
    return PB_OK;
}

int pb_synth_frame_u8(uint8_t* frame_dev, int height, int width, uint32_t frame, uint32_t seed, int circle_mask,
                      void* stream) {
    if (!frame_dev) return pb_fail(PB_ERR_INVALID, "null argument");
    if (height < 1 || width < 1 || (long long)height * width > 0x7FFFFFFFll / 4)
        return pb_fail(PB_ERR_INVALID, "frame size out of range");
    if (circle_mask < 0 || circle_mask > 2) return pb_fail(PB_ERR_INVALID, "circle_mask must be 0, 1 or 2");
    const uint32_t fkey = (frame * 0x9E3779B1u) ^ seed;
    const unsigned total = (unsigned)height * (unsigned)width;
    hipLaunchKernelGGL(pb_synth_kernel, dim3(pb_blocks(total)), dim3(PB_BLOCK), 0, (hipStream_t)stream, frame_dev,
                       height, width, fkey, circle_mask);
    PB_HIP(hipGetLastError());
    return PB_OK;
}

// ---- plan persistence ------------------------------------------------------------------
// A prepared plan as one host blob: header, PbParams, then the device tables in a fixed order.  The blob is a
// cache of a computation (like a compiled kernel), valid for this library build (ABI version, struct sizes) and
// integrity-checked (FNV-1a over the payload); it is not a hardened file format.
}  // extern "C"

namespace {
struct PbBlobHeader {
    uint32_t magic, version, params_size, entry_size;
    int32_t fast_ready, sep_ready, dbl_ready, reserved;
    uint32_t n_tiles, n_fail_tiles, n_fix_px, n_lean_tiles, n_black_tiles, n_direct_tiles, n_row_weight_tiles, n_lat_tiles;
    int64_t diff_pixels;
    uint64_t section_bytes[13];
    uint64_t checksum;  // of everything after the header
};
const uint32_t PB_BLOB_MAGIC = 0x4C504250u;  // "PBPL"
const uint32_t PB_BLOB_VERSION = 5;  // 4: tile flags carry PB_TILE_COARSE; 5: ... and the walk bits of the bilinear table slots; the header names the math flavour

struct PbSection {
    PbBlockAny* block;
    size_t bytes;
};
// the plan's certified tables and their sizes (0 = absent), in blob order.  sep_rows / sep_cols: whether the two optional sections are
// there - the writing side says what it holds, the reading side what the blob's header records.
void pb_plan_sections(PbCertified& c, const PbParams& P, bool sep_rows, bool sep_cols, PbSection sec[13]) {
    const size_t nt = c.n_tiles, nf = c.n_fail_tiles ? c.n_fail_tiles : 1, np = c.n_fix_px ? c.n_fix_px : 1;
    const bool tiles = c.fast_ready || c.dbl_ready;
    sec[0] = {&c.table, tiles ? nt * sizeof(PbTileEntry) : 0};
    sec[1] = {&c.table_r, c.dbl_ready ? nt * sizeof(PbTileEntry) : 0};
    sec[2] = {&c.fail_tiles, tiles ? nf * sizeof(int32_t) : 0};
    sec[3] = {&c.fix_px, tiles ? np * sizeof(int32_t) : 0};
    sec[4] = {&c.idx_tab, c.fast_ready ? nf * PB_TILE * PB_TILE * sizeof(int32_t) : 0};
    sec[5] = {&c.fix_idx, c.fast_ready ? np * sizeof(int32_t) : 0};
    sec[6] = {&c.sep_rows, sep_rows ? (size_t)P.dst.height * sizeof(PbSepRow) : 0};
    sec[7] = {&c.sep_cols, sep_cols ? (size_t)P.dst.width * sizeof(PbSepCol) : 0};
    sec[8] = {&c.dbl_tile_fix, c.dbl_ready ? nf * PB_TILE * PB_TILE * sizeof(PbDoubleFix) : 0};
    sec[9] = {&c.dbl_px_fix, c.dbl_ready ? np * sizeof(PbDoubleFix) : 0};
    sec[10] = {&c.lat_tab, (size_t)c.n_lat_tiles * PB_LAT_TILE_DOUBLES * sizeof(double)};
    sec[11] = {&c.saved_l, tiles ? nt * sizeof(int32_t) : 0};
    sec[12] = {&c.saved_r, c.dbl_ready ? nt * sizeof(int32_t) : 0};
}
uint64_t pb_fnv1a(const uint8_t* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) {
        h ^= p[i];
        h *= 1099511628211ull;
    }
    return h;
}
}  // namespace

extern "C" {

int pb_plan_serialize(const pb_plan* plan_c, void* buf, size_t capacity, size_t* size_out) {
    if (!plan_c || !size_out) return pb_fail(PB_ERR_INVALID, "null argument");
    pb_plan* pl = const_cast<pb_plan*>(plan_c);  // sections are described through the blocks' addresses; nothing is modified
    if (!(pl->cert.fast_ready || pl->cert.dbl_ready || pl->cert.sep_ready)) return pb_fail(PB_ERR_UNSUPPORTED, "the plan holds no device tables (not prepared)");
    PbSection sec[13];
    pb_plan_sections(pl->cert, pl->P, pl->cert.sep_rows.holds(), pl->cert.sep_cols.holds(), sec);
    size_t total = sizeof(PbBlobHeader) + sizeof(PbParams);
    for (int i = 0; i < 13; ++i) total += sec[i].bytes;
    *size_out = total;
    if (!buf) return PB_OK;  // size query
    if (capacity < total) return pb_fail(PB_ERR_INVALID, "buffer too small for the serialized plan");
    int dev = -1;
    PB_HIP(hipGetDevice(&dev));
    if (dev != pl->device) return pb_fail(PB_ERR_INVALID, "plan was prepared on another device; create one plan per device");
    uint8_t* out = static_cast<uint8_t*>(buf);
    PbBlobHeader h;
    memset(&h, 0, sizeof(h));
    h.magic = PB_BLOB_MAGIC;
    h.version = PB_BLOB_VERSION;
    h.params_size = (uint32_t)sizeof(PbParams);
    h.entry_size = (uint32_t)sizeof(PbTileEntry);
    h.fast_ready = pl->cert.fast_ready; h.sep_ready = pl->cert.sep_ready; h.dbl_ready = pl->cert.dbl_ready; h.reserved = pl->walk | (PB_MATH_FLAVOUR << 8);
    h.n_tiles = pl->cert.n_tiles; h.n_fail_tiles = pl->cert.n_fail_tiles; h.n_fix_px = pl->cert.n_fix_px; h.n_lean_tiles = pl->cert.n_lean_tiles;
    h.n_black_tiles = pl->cert.n_black_tiles; h.n_direct_tiles = pl->cert.n_direct_tiles; h.n_row_weight_tiles = pl->cert.n_row_weight_tiles;
    h.n_lat_tiles = pl->cert.n_lat_tiles; h.diff_pixels = pl->cert.diff_pixels;
    uint8_t* q = out + sizeof(PbBlobHeader);
    memcpy(q, &pl->P, sizeof(PbParams));
    q += sizeof(PbParams);
    PB_HIP(hipDeviceSynchronize());
    for (int i = 0; i < 13; ++i) {
        h.section_bytes[i] = sec[i].bytes;
        if (!sec[i].bytes) continue;
        if (!sec[i].block->holds()) return pb_fail(PB_ERR_INVALID, "inconsistent plan: a table is missing");
        PB_HIP(hipMemcpy(q, sec[i].block->bytes(), sec[i].bytes, hipMemcpyDeviceToHost));
        q += sec[i].bytes;
    }
    h.checksum = pb_fnv1a(out + sizeof(PbBlobHeader), total - sizeof(PbBlobHeader));
    memcpy(out, &h, sizeof(h));
    return PB_OK;
}

int pb_plan_deserialize(const void* buf, size_t size, pb_plan** out) {
    if (!buf || !out) return pb_fail(PB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (size < sizeof(PbBlobHeader) + sizeof(PbParams)) return pb_fail(PB_ERR_INVALID, "serialized plan truncated");
    const uint8_t* in = static_cast<const uint8_t*>(buf);
    PbBlobHeader h;
    memcpy(&h, in, sizeof(h));
    if (h.magic != PB_BLOB_MAGIC || h.version != PB_BLOB_VERSION || h.params_size != sizeof(PbParams) || h.entry_size != sizeof(PbTileEntry))
        return pb_fail(PB_ERR_INVALID, "serialized plan is not from this library build (magic / version / struct sizes)");
    if (h.checksum != pb_fnv1a(in + sizeof(PbBlobHeader), size - sizeof(PbBlobHeader)))
        return pb_fail(PB_ERR_INVALID, "serialized plan is corrupt (checksum)");
    // the blob's exact tables, thresholds and certified flags are products of ONE math flavour's asin / acos / atan / tan
    if (((h.reserved >> 8) & 0xFF) != PB_MATH_FLAVOUR)
        return pb_fail(PB_ERR_UNSUPPORTED, PB_MATH_FLAVOUR ? "serialized plan was made by libphotonbend_hip.so (the AVX-512 / SVML math flavour); this is libphotonbend_hip_libm.so"
                                                            : "serialized plan was made by libphotonbend_hip_libm.so (glibc's asin / acos / atan / tan); this is libphotonbend_hip.so");
    PbPlanOwner pl(new (std::nothrow) pb_plan());
    if (!pl) return pb_fail(PB_ERR_INVALID, "out of host memory");
    memcpy(&pl->P, in + sizeof(PbBlobHeader), sizeof(PbParams));
    pl->cert.fast_ready = h.fast_ready; pl->cert.sep_ready = h.sep_ready; pl->cert.dbl_ready = h.dbl_ready;
    pb_sep_setup(pl->cert);
    pl->walk = ((h.reserved & 0xFF) <= 3) ? (h.reserved & 0xFF) : 0;
    pl->cert.n_tiles = h.n_tiles; pl->cert.n_fail_tiles = h.n_fail_tiles; pl->cert.n_fix_px = h.n_fix_px; pl->cert.n_lean_tiles = h.n_lean_tiles;
    pl->cert.n_black_tiles = h.n_black_tiles; pl->cert.n_direct_tiles = h.n_direct_tiles; pl->cert.n_row_weight_tiles = h.n_row_weight_tiles;
    pl->cert.n_lat_tiles = h.n_lat_tiles; pl->cert.diff_pixels = h.diff_pixels;
    pl->mode = PB_MODE_AUTO;
    const bool tiles = pl->cert.fast_ready || pl->cert.dbl_ready;
    // the derived half of the parameter block must be what THIS build derives from the blob's own request (a blob whose tables
    // were made for other constants is foreign, whatever its checksum says)
    bool ok = pl->P.n_rot >= 0 && pl->P.n_rot <= PB_MAX_ROTATIONS;
    if (ok) {
        PbParams Q;
        PbEndX ends[2];  // (a polynomial lens: its derived constants too are re-derived, from the blob's coefficients, and these re-validated)
        memset(ends, 0, sizeof(ends));
        ends[0].e = pl->P.dst;
        ends[1].e = pl->P.src;
        const PbPoly* polys[2] = {&pl->P.poly_dst, &pl->P.poly_src};
        std::string why;
        for (int e = 0; e < 2 && ok; ++e)
            if (ends[e].e.lens == PB_LENS_POLYNOMIAL) ok = pb_poly_make(polys[e]->k, polys[e]->max_theta, ends[e].poly, why);
        pb_params_of_request(Q, ends[0], &pl->P.R[0][0], pl->P.n_rot, ends[1]);
        ok = ok && pb_same_request(Q, pl->P);
    }
    ok = ok && (!tiles || pl->cert.n_tiles == pb_num_tiles(pl->P)) && pl->cert.n_fail_tiles <= 2u * pl->cert.n_tiles + 1u &&
              pl->P.win_budget >= PB_DIRECT_LDS_BYTES && pl->P.win_budget <= PB_WINLDS_MAX && (pl->P.win_budget & 15) == 0 &&
              pl->P.n_rot >= 0 && pl->P.n_rot <= PB_MAX_ROTATIONS;
    PbSection sec[13];
    pb_plan_sections(pl->cert, pl->P, h.section_bytes[6] != 0, h.section_bytes[7] != 0, sec);
    size_t total = sizeof(PbBlobHeader) + sizeof(PbParams);
    for (int i = 0; i < 13; ++i) {
        ok = ok && h.section_bytes[i] == sec[i].bytes;
        total += h.section_bytes[i];
    }
    if (!ok || total != size) return pb_fail(PB_ERR_INVALID, "serialized plan is inconsistent (sizes do not match its geometry)");
    int rc = PB_OK;
    if (hipGetDevice(&pl->device) != hipSuccess) rc = PB_ERR_HIP;
    const uint8_t* q = in + sizeof(PbBlobHeader) + sizeof(PbParams);
    for (int i = 0; i < 13 && rc == PB_OK; ++i) {
        if (!sec[i].bytes) continue;
        if (sec[i].block->alloc_bytes(sec[i].bytes) != hipSuccess || hipMemcpy(sec[i].block->bytes(), q, sec[i].bytes, hipMemcpyHostToDevice) != hipSuccess)
            rc = PB_ERR_HIP;
        q += sec[i].bytes;
    }
    if (rc != PB_OK) return pb_fail(rc, std::string("plan upload failed: ") + hipGetErrorString(hipGetLastError()));
    if (pl->nearest.P_dev.alloc(1) != hipSuccess || hipMemcpy(pl->nearest.P_dev, &pl->P, sizeof(PbParams), hipMemcpyHostToDevice) != hipSuccess)
        return pb_fail(PB_ERR_HIP, "plan upload failed: parameter block");
    if ((pl->cert.dbl_ready || pl->cert.fast_ready) && pb_build_bilinear_list(pl.get()) != PB_OK) return PB_ERR_HIP;
    rc = pb_build_bilinear_launch(pl.get());  // derived state: rebuilt, not stored
    if (rc == PB_OK) rc = pb_apply_budget(pl.get(), pl->P.win_budget);
    if (rc != PB_OK) return rc;
    *out = pl.release();
    return PB_OK;
}

// ---- measurement utility: a plain device copy (16 bytes per lane), the practical HBM ceiling next to which
// bench.py reports the remap kernel (MI355X_MICROARCH.md: 8 TB/s spec, ~6.3 TB/s by such a copy) -------------
}  // extern "C"
typedef unsigned pb_u32x4 __attribute__((ext_vector_type(4)));
// every workgroup owns one contiguous 32 KiB chunk: 8 non-temporal 16-byte loads per lane in flight, then 8 non-temporal
// stores - the fastest of the copy shapes measured on MI355X (experiments/exp_copy.hip: 6.35 TB/s read + write on 512 MiB;
// a grid-stride loop of single loads 4.9-5.8, hipMemcpyDtoD 5.35)
__global__ __launch_bounds__(256) void pb_copy16_kernel(const pb_u32x4* __restrict__ src, pb_u32x4* __restrict__ dst, size_t n16) {
    const size_t base = (size_t)blockIdx.x * 2048 + threadIdx.x;
    if (base + 7 * 256 < n16) {
        pb_u32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(src + base + u * 256);
#pragma unroll
        for (int u = 0; u < 8; ++u) __builtin_nontemporal_store(v[u], dst + base + u * 256);
    } else {
        for (size_t i = base; i < n16; i += 256) dst[i] = src[i];
    }
}
extern "C" {
int pb_stream_copy(void* dst_dev, const void* src_dev, size_t bytes, void* stream) {
    if (!dst_dev || !src_dev) return pb_fail(PB_ERR_INVALID, "null argument");
    if ((((uintptr_t)dst_dev | (uintptr_t)src_dev | bytes) & 15u) != 0) return pb_fail(PB_ERR_INVALID, "pb_stream_copy needs 16-byte aligned pointers and size");
    const size_t n16 = bytes / 16;
    if (!n16) return PB_OK;
    const size_t blocks = (n16 + 2047) / 2048;
    if (blocks > 0x7FFFFFFFull) return pb_fail(PB_ERR_INVALID, "pb_stream_copy: too large");
    hipLaunchKernelGGL(pb_copy16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, static_cast<const pb_u32x4*>(src_dev),
                       static_cast<pb_u32x4*>(dst_dev), n16);
    PB_HIP(hipGetLastError());
    return PB_OK;
}

// ---- multi-GPU: one process per GPU, frames sharded, ONE collective (SURVEY 8 e) -----------------------------------------
// RCCL (librccl.so.1; "nccl" on ROCm, over xGMI inside a node) is bound at first use with dlopen - the remap library itself has
// no link-time dependency on it, and a host that brings its own communicator layer (torch.distributed in the Python package)
// never touches these entry points.  The only data-path collective is the broadcast of the parameter block.
}  // extern "C"
#include <dlfcn.h>
namespace {
struct PbNcclId {
    char internal[128];
};
typedef int (*pb_nccl_get_id_t)(PbNcclId*);
typedef int (*pb_nccl_init_t)(void**, int, PbNcclId, int);
typedef int (*pb_nccl_destroy_t)(void*);
typedef int (*pb_nccl_bcast_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef const char* (*pb_nccl_err_t)(int);
struct PbRccl {
    void* lib = nullptr;
    pb_nccl_get_id_t get_id = nullptr;
    pb_nccl_init_t init = nullptr;
    pb_nccl_destroy_t destroy = nullptr;
    pb_nccl_bcast_t bcast = nullptr;
    pb_nccl_err_t err = nullptr;
};
PbRccl* pb_rccl() {
    static PbRccl r = [] {
        PbRccl q;
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            q.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (q.lib) break;
        }
        if (q.lib) {
            q.get_id = (pb_nccl_get_id_t)dlsym(q.lib, "ncclGetUniqueId");
            q.init = (pb_nccl_init_t)dlsym(q.lib, "ncclCommInitRank");
            q.destroy = (pb_nccl_destroy_t)dlsym(q.lib, "ncclCommDestroy");
            q.bcast = (pb_nccl_bcast_t)dlsym(q.lib, "ncclBroadcast");
            q.err = (pb_nccl_err_t)dlsym(q.lib, "ncclGetErrorString");
        }
        return q;
    }();
    return (r.lib && r.get_id && r.init && r.destroy && r.bcast) ? &r : nullptr;
}
int pb_nccl_fail(const PbRccl* r, const char* what, int code) {
    return pb_fail(PB_ERR_HIP, std::string(what) + ": " + ((r && r->err) ? r->err(code) : "RCCL error"));
}
const int PB_BLOCK_POLY = 2 + 2 * 7 + 9 * PB_MAX_ROTATIONS;  // then k1..k4 and max_theta of a polynomial destination lens, then of a polynomial source lens (zeros otherwise)
const int PB_BLOCK_DOUBLES = PB_BLOCK_POLY + 2 * 5;  // the parameter block: photonbend_amd/parallel.py's layout
}  // namespace

struct pb_comm {
    void* comm = nullptr;
    int n_ranks = 1, rank = 0, device = -1;
    double* block_dev = nullptr;
};

extern "C" {

int pb_comm_unique_id(void* id128) {
    if (!id128) return pb_fail(PB_ERR_INVALID, "null argument");
    PbRccl* r = pb_rccl();
    if (!r) return pb_fail(PB_ERR_UNSUPPORTED, "librccl.so.1 could not be loaded");
    const int rc = r->get_id(static_cast<PbNcclId*>(id128));
    return rc == 0 ? PB_OK : pb_nccl_fail(r, "ncclGetUniqueId", rc);
}

int pb_comm_init(int n_ranks, int rank, const void* id128, pb_comm** out) {
    if (!out || !id128) return pb_fail(PB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return pb_fail(PB_ERR_INVALID, "rank outside [0, n_ranks)");
    PbRccl* r = pb_rccl();
    if (!r) return pb_fail(PB_ERR_UNSUPPORTED, "librccl.so.1 could not be loaded");
    pb_comm* c = new (std::nothrow) pb_comm();
    if (!c) return pb_fail(PB_ERR_INVALID, "out of host memory");
    c->n_ranks = n_ranks;
    c->rank = rank;
    if (hipGetDevice(&c->device) != hipSuccess || hipMalloc((void**)&c->block_dev, PB_BLOCK_DOUBLES * sizeof(double)) != hipSuccess) {
        delete c;
        return pb_fail(PB_ERR_HIP, "pb_comm_init: no device memory for the parameter block");
    }
    PbNcclId id;
    memcpy(&id, id128, sizeof(id));
    const int rc = r->init(&c->comm, n_ranks, id, rank);  // one communicator per process, on the current device
    if (rc != 0) {
        (void)hipFree(c->block_dev);
        delete c;
        return pb_nccl_fail(r, "ncclCommInitRank", rc);
    }
    *out = c;
    return PB_OK;
}

int pb_comm_destroy(pb_comm* comm) {
    if (!comm) return PB_OK;
    PbRccl* r = pb_rccl();
    if (r && comm->comm) (void)r->destroy(comm->comm);
    (void)hipFree(comm->block_dev);
    delete comm;
    return PB_OK;
}

int pb_comm_rank(const pb_comm* comm, int* n_ranks, int* rank) {
    if (!comm) return pb_fail(PB_ERR_INVALID, "null argument");
    if (n_ranks) *n_ranks = comm->n_ranks;
    if (rank) *rank = comm->rank;
    return PB_OK;
}

int pb_bcast_params(pb_comm* comm, pb_proj* dst, double* rot3x3, int* n_rot, pb_proj* src, int root, void* stream) {
    if (!comm || !dst || !src || !n_rot || !rot3x3) return pb_fail(PB_ERR_INVALID, "null argument");
    if (root < 0 || root >= comm->n_ranks) return pb_fail(PB_ERR_INVALID, "root outside [0, n_ranks)");
    PbRccl* r = pb_rccl();
    if (!r) return pb_fail(PB_ERR_UNSUPPORTED, "librccl.so.1 could not be loaded");
    hipStream_t st = (hipStream_t)stream;
    double block[PB_BLOCK_DOUBLES];
    memset(block, 0, sizeof(block));
    auto put = [](double* b, const pb_proj& p) { b[0] = p.kind; b[1] = p.lens; b[2] = p.height; b[3] = p.width; b[4] = p.fov; b[5] = p.magnitude; b[6] = p.f_distance; };
    auto get = [](const double* b, pb_proj& p) { p.kind = (int32_t)b[0]; p.lens = (int32_t)b[1]; p.height = (int32_t)b[2]; p.width = (int32_t)b[3]; p.fov = b[4]; p.magnitude = b[5]; p.f_distance = b[6]; };
    // A collective: once the arguments every rank can check alike have passed (above), EVERY rank reaches the broadcast - a root that
    // finds its own request invalid, or cannot upload it, sends a block with a poisoned magic instead of returning early, and all ranks
    // return PB_ERR_INVALID together (the other ranks used to block in ncclBroadcast forever).
    if (comm->rank == root) {
        const bool ok = *n_rot >= 0 && *n_rot <= PB_MAX_ROTATIONS;
        block[0] = ok ? 1346522692.0 : -1.0;  // "PBND": the Python package's magic (photonbend_amd/parallel.py), same layout
        if (ok) {
            block[1] = *n_rot;
            put(block + 2, *dst);
            put(block + 9, *src);
            for (int k = 0; k < 9 * *n_rot; ++k) block[16 + k] = rot3x3[k];
            // a polynomial lens travels as its coefficients (ids are process-local): the lens field says PB_LENS_POLYNOMIAL_BASE
            const pb_proj* ends[2] = {dst, src};
            for (int e = 0; e < 2; ++e) {
                PbPoly L;
                if (!pb_has_lens(ends[e]->kind) || ends[e]->lens < PB_LENS_POLYNOMIAL_BASE) continue;
                if (!pb_poly_lookup(ends[e]->lens, &L)) {  // an id the root never registered must not travel: another rank's registry
                    block[0] = -1.0;                       // may hold a different lens under it - every rank returns PB_ERR_INVALID
                    break;
                }
                block[2 + 7 * e + 1] = PB_LENS_POLYNOMIAL_BASE;
                for (int i = 0; i < 4; ++i) block[PB_BLOCK_POLY + 5 * e + i] = L.k[i];
                block[PB_BLOCK_POLY + 5 * e + 4] = L.max_theta;
            }
        }
        if (hipMemcpyAsync(comm->block_dev, block, sizeof(block), hipMemcpyHostToDevice, st) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipMemsetAsync(comm->block_dev, 0xFF, sizeof(block), st);  // (NaN magic: poisoned)
        }
    }
    const int rc = r->bcast(comm->block_dev, comm->block_dev, PB_BLOCK_DOUBLES, 8 /* ncclFloat64 */, root, comm->comm, st);
    if (rc != 0) return pb_nccl_fail(r, "ncclBroadcast", rc);
    PB_HIP(hipMemcpyAsync(block, comm->block_dev, sizeof(block), hipMemcpyDeviceToHost, st));
    PB_HIP(hipStreamSynchronize(st));
    if (block[0] != 1346522692.0 || !(block[1] >= 0 && block[1] <= PB_MAX_ROTATIONS))
        return pb_fail(PB_ERR_INVALID, "the root's parameter block is invalid (n_rot outside [0, PB_MAX_ROTATIONS], a polynomial lens id the root never registered, a failed upload, or corrupt)");
    *n_rot = (int)block[1];
    get(block + 2, *dst);
    get(block + 9, *src);
    for (int k = 0; k < 9 * *n_rot; ++k) rot3x3[k] = block[16 + k];
    // ... and the receiver (the root included) registers them and writes ITS id into the projection it returns
    pb_proj* ends[2] = {dst, src};
    for (int e = 0; e < 2; ++e) {
        if (!pb_has_lens(ends[e]->kind) || ends[e]->lens != PB_LENS_POLYNOMIAL_BASE) continue;
        int id = 0;
        const int rc = pb_lens_polynomial(block + PB_BLOCK_POLY + 5 * e, block[PB_BLOCK_POLY + 5 * e + 4], &id);
        if (rc != PB_OK) return rc;
        ends[e]->lens = id;
    }
    return PB_OK;
}

int pb_shard_range(int n_items, int n_ranks, int rank, int* first, int* count) {
    if (!first || !count) return pb_fail(PB_ERR_INVALID, "null argument");
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks || n_items < 0) return pb_fail(PB_ERR_INVALID, "bad shard request");
    const int q = n_items / n_ranks, r = n_items % n_ranks;
    *first = rank * q + (rank < r ? rank : r);
    *count = q + (rank < r ? 1 : 0);
    return PB_OK;
}

int pb_remap_batch_sharded(const pb_comm* comm, const pb_plan* plan, const uint8_t* src_dev, uint8_t* dst_dev, int n_frames_total,
                           size_t src_frame_stride, size_t dst_frame_stride, int* first_out, int* count_out, void* stream) {
    if (!comm || !plan || !src_dev || !dst_dev) return pb_fail(PB_ERR_INVALID, "null argument");
    int first = 0, count = 0;
    const int rc = pb_shard_range(n_frames_total, comm->n_ranks, comm->rank, &first, &count);
    if (rc != PB_OK) return rc;
    if (first_out) *first_out = first;
    if (count_out) *count_out = count;
    if (count == 0) return PB_OK;
    // this rank's contiguous share of the batch, addressed in the caller's (rank-local) buffers from frame 0 on
    return pb_remap_u8(plan, src_dev, dst_dev, count, src_frame_stride, dst_frame_stride, stream);
}

// ---- plumbing ----------------------------------------------------------------------
int pb_malloc(void** dev_ptr, size_t bytes) {
    if (!dev_ptr) return pb_fail(PB_ERR_INVALID, "null argument");
    PB_HIP(hipMalloc(dev_ptr, bytes ? bytes : 1));
    return PB_OK;
}
int pb_free(void* dev_ptr) {
    if (dev_ptr) PB_HIP(hipFree(dev_ptr));
    return PB_OK;
}
int pb_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream) {
    PB_HIP(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return PB_OK;
}
int pb_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream) {
    PB_HIP(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return PB_OK;
}
int pb_memset(void* dst_dev, int value, size_t bytes, void* stream) {
    PB_HIP(hipMemsetAsync(dst_dev, value, bytes, (hipStream_t)stream));
    return PB_OK;
}
int pb_stream_create(void** stream) {
    if (!stream) return pb_fail(PB_ERR_INVALID, "null argument");
    hipStream_t s;
    PB_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void*)s;
    return PB_OK;
}
int pb_stream_destroy(void* stream) {
    if (stream) PB_HIP(hipStreamDestroy((hipStream_t)stream));
    return PB_OK;
}
int pb_stream_sync(void* stream) {
    PB_HIP(hipStreamSynchronize((hipStream_t)stream));
    return PB_OK;
}
int pb_event_create(void** event) {
    if (!event) return pb_fail(PB_ERR_INVALID, "null argument");
    hipEvent_t e;
    PB_HIP(hipEventCreate(&e));
    *event = (void*)e;
    return PB_OK;
}
int pb_event_destroy(void* event) {
    if (event) PB_HIP(hipEventDestroy((hipEvent_t)event));
    return PB_OK;
}
int pb_event_record(void* event, void* stream) {
    PB_HIP(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
    return PB_OK;
}
int pb_event_sync(void* event) {
    PB_HIP(hipEventSynchronize((hipEvent_t)event));
    return PB_OK;
}
int pb_event_elapsed_ms(void* start, void* stop, float* ms) {
    if (!ms) return pb_fail(PB_ERR_INVALID, "null argument");
    PB_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return PB_OK;
}
int pb_device_count(int* n) {
    if (!n) return pb_fail(PB_ERR_INVALID, "null argument");
    *n = 0;
    if (hipGetDeviceCount(n) != hipSuccess) {
        (void)hipGetLastError();
        *n = 0;
    }
    return PB_OK;
}
int pb_set_device(int device) {
    PB_HIP(hipSetDevice(device));
    return PB_OK;
}
int pb_get_device(int* device) {
    if (!device) return pb_fail(PB_ERR_INVALID, "null argument");
    PB_HIP(hipGetDevice(device));
    return PB_OK;
}
int pb_device_sync(void) {
    PB_HIP(hipDeviceSynchronize());
    return PB_OK;
}
int pb_stream_wait_event(void* stream, void* event) {
    if (!event) return pb_fail(PB_ERR_INVALID, "null argument");
    PB_HIP(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
    return PB_OK;
}
int pb_host_alloc(void** host_ptr, size_t bytes) {
    if (!host_ptr) return pb_fail(PB_ERR_INVALID, "null argument");
    PB_HIP(hipHostMalloc(host_ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return PB_OK;
}
int pb_host_free(void* host_ptr) {
    if (host_ptr) PB_HIP(hipHostFree(host_ptr));
    return PB_OK;
}
int pb_host_register(void* host_ptr, size_t bytes) {
    if (!host_ptr || !bytes) return pb_fail(PB_ERR_INVALID, "null argument");
    PB_HIP(hipHostRegister(host_ptr, bytes, hipHostRegisterDefault));
    return PB_OK;
}
int pb_host_unregister(void* host_ptr) {
    if (!host_ptr) return pb_fail(PB_ERR_INVALID, "null argument");
    PB_HIP(hipHostUnregister(host_ptr));
    return PB_OK;
}

}  // extern "C"

// ---- supersampled remapping ----------------------------------------------------------------------------------------
static int pb_ss_check(const pb_plan* plan, int n, int interpolation) {
    if (!plan) return pb_fail(PB_ERR_INVALID, "null argument");
    if (n != 2 && n != 4) return pb_fail(PB_ERR_INVALID, "supersample factor must be 2 or 4");
    if (interpolation != PB_INTERP_NEAREST && interpolation != PB_INTERP_BILINEAR) return pb_fail(PB_ERR_INVALID, "interpolation must be PB_INTERP_NEAREST or PB_INTERP_BILINEAR");
    if (plan->P.dst.height % n || plan->P.dst.width % n)
        return pb_fail(PB_ERR_INVALID, "the plan's destination is not divisible by the supersample factor (pass the plan of the n x destination)");
    return PB_OK;
}

static void pb_box_reduce_launch(const void* src, void* dst, unsigned H, unsigned W, int channels, int sample_bytes, int n, int n_frames, hipStream_t st) {
    const unsigned long long n_px = (unsigned long long)H * W * (unsigned)n_frames;
    const unsigned long long want = (n_px + 255) / 256;
    const dim3 grid((unsigned)(want < (1ull << 20) ? want : (1ull << 20))), block(256);
    const uint8_t* s = (const uint8_t*)src;
    uint8_t* d = (uint8_t*)dst;
    if (n == 2 && sample_bytes == 1) hipLaunchKernelGGL((pb_box_reduce_kernel<2, 1>), grid, block, 0, st, s, d, W, channels, n_px);
    else if (n == 2) hipLaunchKernelGGL((pb_box_reduce_kernel<2, 2>), grid, block, 0, st, s, d, W, channels, n_px);
    else if (sample_bytes == 1) hipLaunchKernelGGL((pb_box_reduce_kernel<4, 1>), grid, block, 0, st, s, d, W, channels, n_px);
    else hipLaunchKernelGGL((pb_box_reduce_kernel<4, 2>), grid, block, 0, st, s, d, W, channels, n_px);
}

extern "C" {

int pb_remap_ss_workspace(const pb_plan* plan, int n, int interpolation, unsigned flags, size_t* bytes) {
    if (!bytes) return pb_fail(PB_ERR_INVALID, "null argument");
    const int rc = pb_ss_check(plan, n, interpolation);
    if (rc) return rc;
    // (16-byte aligned frames assumed: the caller's unaligned frames need the workspace too)
    *bytes = pb_route(plan, interpolation, n, flags, true).kind == PbRoute::SS_FUSED ? 0 : 3ull * plan->P.dst.height * plan->P.dst.width;
    return PB_OK;
}

int pb_remap_ss_u8(const pb_plan* plan, int n, int interpolation, const uint8_t* src_dev, uint8_t* dst_dev, int n_frames, size_t src_frame_stride,
                   size_t dst_frame_stride, void* workspace_dev, size_t workspace_bytes, unsigned flags, void* stream) {
    int rc = pb_ss_check(plan, n, interpolation);
    if (rc == PB_OK) rc = pb_check_frames(plan, src_dev, dst_dev, n_frames, n, src_frame_stride, dst_frame_stride);
    if (rc != PB_OK || n_frames == 0) return rc;
    const PbParams& P = plan->P;
    hipStream_t st = (hipStream_t)stream;
    const bool aligned = pb_aligned16(src_dev, src_frame_stride);
    if (pb_route(plan, interpolation, n, flags, aligned).kind == PbRoute::SS_FUSED) {
        const unsigned gpf = plan->nearest.lt.groups;
        pb_each_launch(src_dev, dst_dev, n_frames, src_frame_stride, dst_frame_stride, gpf, [&](const uint8_t* sf, uint8_t* df, int nf) {
            pb_pick_kind(P, [&](auto K) {
                pb_pick<2, 4>(n == 2, [&](auto NS) {
                    hipLaunchKernelGGL((pb_ss_win_kernel<K.value, NS.value>), dim3(gpf * (unsigned)nf), dim3(64 * PB_TILE_WAVES), pb_window_lds_bytes(P), st,
                                       (const PbParams*)plan->nearest.P_dev, pb_hot_of_host(P), plan->nearest.lt.entries, sf, df, gpf, (unsigned long long)src_frame_stride,
                                       (unsigned long long)dst_frame_stride, plan->cert.idx_tab, plan->cert.fix_px, plan->cert.fix_idx);
                });
            });
        });
        PB_HIP(hipGetLastError());
        return PB_OK;
    }
    // generic path: frame by frame, the n x remap into the workspace, then the box reduction into the caller's frame
    const unsigned long long ws_need = 3ull * P.dst.height * P.dst.width;
    if (!workspace_dev || workspace_bytes < ws_need)
        return pb_fail(PB_ERR_INVALID, "workspace smaller than one n x frame (pb_remap_ss_workspace; frames that are not 16-byte aligned need it too)");
    uint8_t* ws = (uint8_t*)workspace_dev;
    const PbRoute frame_route = pb_route(plan, interpolation, 1, 0, aligned);  // (every frame of the batch is aligned alike)
    for (int f = 0; f < n_frames; ++f) {
        rc = pb_launch(plan, frame_route, src_dev + (unsigned long long)f * src_frame_stride, ws, 1, src_frame_stride, ws_need, st);
        if (rc != PB_OK) return rc;
        pb_box_reduce_launch(ws, dst_dev + (unsigned long long)f * dst_frame_stride, (unsigned)P.dst.height / n, (unsigned)P.dst.width / n, 3, 1, n, 1, st);
        PB_HIP(hipGetLastError());
    }
    return PB_OK;
}

int pb_box_reduce(const void* src_dev, void* dst_dev, int height, int width, int channels, int sample_bytes, int n, int n_frames, void* stream) {
    if (!src_dev || !dst_dev) return pb_fail(PB_ERR_INVALID, "null argument");
    if (n != 2 && n != 4) return pb_fail(PB_ERR_INVALID, "supersample factor must be 2 or 4");
    if (sample_bytes != 1 && sample_bytes != 2) return pb_fail(PB_ERR_INVALID, "sample_bytes must be 1 or 2");
    if (channels < 1 || channels > 64) return pb_fail(PB_ERR_INVALID, "channels out of range (1..64)");
    if (height < 1 || width < 1 || n_frames < 0) return pb_fail(PB_ERR_INVALID, "bad shape");
    // the n x frame obeys the projection limit of every map in the library (h * w < 2^29)
    if ((long long)height * width * n * n > 0x7FFFFFFFll / 4) return pb_fail(PB_ERR_INVALID, "n x frame beyond the projection limit (n^2 h w < 2^29)");
    if (n_frames == 0) return PB_OK;
    pb_box_reduce_launch(src_dev, dst_dev, (unsigned)height, (unsigned)width, channels, sample_bytes, n, n_frames, (hipStream_t)stream);
    PB_HIP(hipGetLastError());
    return PB_OK;
}

}  // extern "C"
