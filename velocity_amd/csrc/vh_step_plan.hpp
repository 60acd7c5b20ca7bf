// The launches of a tracked frame, everything that is arithmetic on sizes (internal): the ONE snapshot of the hooks and switches a launch decision reads
// (VhTuning) and the ONE choice of kernel, grid and dynamic LDS for each launch of a step (LkPlan, PyrPlan, RoiWarpPlan, RansacPlan, the track order, the
// session's frame kernels).  Plain C++17, no HIP include: tests/test_step_plan_cpu.py compiles it with g++ and checks every boundary without a GPU.  The
// launchers (vh_lk.hip, vh_image.hip, vh_ransac.hip, vh_api.hip, vh_session.hip) launch what the plan says; the measurements behind each threshold stand
// beside it here.
#pragma once
#include <cstddef>

// ---------------------------------------------------------------------------------------------------------------
// Every hook and switch a launch decision reads, as plain values: the launchers take one snapshot per call (vh_tuning(), vh_kernels.hpp), the plans
// below read nothing else.  The defaults are the library's.  Set by: a vh_debug_* entry (include/velocity_hip.h, PROCESS-WIDE test hooks) and / or an
// environment variable read once per process (experiments only); DESIGN.md section 5 has the table.
struct VhTuning {
    int lk_force = 0;        // vh_debug_force_generic_lk / VH_LK_FORCE: LkRoute id every LK launch takes where its window allows, 0 = by window and load
    int lk3_tpw = 0;         // vh_debug_lk3_tpw / VH_LK3_TPW: launch slots per workgroup of the one-wavefront k_lk3 (0 = by load, n > 0 = n, clamped to LK3_MAX_TPW)
    int lk3_one_level = 1;   // vh_debug_lk3_one_level / VH_LK3_ONE_LEVEL: 1 = jobs with max_level = 0 take the single-level form of k_lk3
    int klt_order = -1;      // vh_debug_klt_order / VH_KLT_ORDER: spatial launch order of the tracks, 1 always, 0 never, -1 by load
    int ransac_path = 0;     // vh_debug_ransac_path: 1 = always the three-kernel path, 2 (and 0) = the fused kernel whenever the problem fits it
    int pyr_rows = 0;        // vh_debug_pyr_rows: 2 / 4 / 8 output rows per thread of k_pyr_down whatever the launch size, 0 = by size
    int ba_force_valu = 0;   // vh_debug_ba_force_valu: 1 = the VALU Schur kernel where it exists (ba_plan, vh_ba_plan.hpp)
    int lko_group = 64;      // VH_LKO_G: streams per set of the block order of k_lk_o AND of k_lk_h (lk_block_xy)
    int lkq_group = 64;      // VH_LKQ_G: ... of k_lk_q
    int lk3_group = 16;      // VH_LK3_G: ... of k_lk3
    int lk_lds_pad = 0;      // VH_LK_LDS_PAD: extra dynamic LDS per k_lk3 workgroup = fewer resident wavefronts per SIMD (the occupancy sensitivity behind DESIGN.md section 9)
    long long lko_min_tracks = 10000;   // VH_LKO_MIN: k_lk_o from this many tracks in flight (15 x 15 windows)
    long long lkh_min_tracks = 128000;  // VH_LKH_MIN: k_lk_h from this many
    int rw_xcd_bands = 0;    // VH_RW_XCD: k_roi_warp walks the ROI in one band of rows per XCD (see the kernel)
    int ba_parts = 0;        // VH_BA_PARTS: cap of the partial systems of a bundle adjustment (ba_nparts, vh_ba_plan.hpp), 0 = unset
    int ba_graph_off = 0;    // VH_BA_GRAPH=0: no solve is replayed from a captured graph
};

// ---------------------------------------------------------------------------------------------------------------
// LK.  The route ids are ABI: vh_debug_force_generic_lk takes them, vh_profile_lk_routes reports them.
// test hook: 1 = per-sample kernel, 2 = strip kernel, 3 = LDS-staged kernel, 4 = 4-tracks-per-wave kernel (15x15), 5 / 6 / 7 = LDS-staged 51x51 kernel with
// 1 / 2 / 4 wavefronts per track, 8 = 8-tracks-per-wave kernel (15x15), 9 = 16-tracks-per-wave kernel (15x15), 0 = default routing.
// PROCESS-WIDE (every context of the process is re-routed, see the record in vh_api.hip) -- a test / experiment switch, not a per-stream control.
enum LkRoute : int {
    LK_ROUTE_NONE = 0,       // nothing launched (no track slot)
    LK_ROUTE_SAMPLE = 1,     // k_lk
    LK_ROUTE_STRIP = 2,      // k_lk_strip<15 | 51 | 0>
    LK_ROUTE_LK3_15 = 3,     // k_lk3<15, 1, 6>
    LK_ROUTE_Q = 4,          // k_lk_q<15>
    LK_ROUTE_LK3_51_W1 = 5,  // k_lk3<51, 1, 4>
    LK_ROUTE_LK3_51_W2 = 6,  // k_lk3<51, 2, 4>
    LK_ROUTE_LK3_51_W4 = 7,  // k_lk3<51, 4, 4>
    LK_ROUTE_O = 8,          // k_lk_o<15>
    LK_ROUTE_H = 9,          // k_lk_h<15>
};

constexpr int LK3_MAX_TPW = 8;              // launch slots one workgroup may solve one after the other (LK3<..>::MAX_TPW, tied by a static_assert in vh_lk.hip)
constexpr unsigned LK_GROUP_ROTATE = 0x10000u;  // LK_GRP_ROTATE of lk_block_xy (tied by a static_assert in vh_lk.hip)
constexpr size_t LK_LDS_DEFAULT_LIMIT = 64 * 1024;  // dynamic LDS a kernel may ask for before hipFuncAttributeMaxDynamicSharedMemorySize is raised
constexpr size_t LK_LDS_WORKGROUP = 160 * 1024;     // LDS of a workgroup

// Which kernel a launch of `batch` streams x `max_n` track slots with window `win` takes (the ids of the test hook above; 2 = the strip kernel of any
// window <= 63, 1 = the per-sample kernel).  vh_launch_lk follows exactly this decision, and the profiling records report it (vh_profile_lk_routes), so
// nobody has to mirror the thresholds.
//
// Default routing, re-measured late in round 5 -- the earlier thresholds had been measured while every LK launch carried ~45 us of serialised statistics
// atomics (StreamWS::lk_stats), which hid what the kernels themselves cost at a few thousand tracks.  51x51 fine stage: the LDS-staged kernel with ONE
// wavefront per track from 640 tracks in flight (2000 tracks: 28.8 us against 33.2 / 43.2 with 2 / 4 wavefronts per track; 768: 37.1 / 39.7 / 41.1 for
// the whole vh_pyr_lk call), 4 wavefronts per track below (128 tracks: 30.8 against 35.3); 2 per track is never the fastest and is kept for the tests.
// 15x15 coarse stages: the one-wave-per-track strip kernel up to 3000 tracks (2000: 20.2 / 27.9 us against 22.2 / 29.4 for 4 tracks per wavefront; 4000:
// 25.6 / 36.6 against 23.1 / 29.2), 4 tracks per wavefront up to 10 000, 8 per wavefront above (12 000: 33.6 / 50.2 against 35.4 / 55.9 us; 8000: a tie),
// 16 per wavefront (k_lk_h) from 128 000.  Measured with three wavefronts per SIMD: both launches of sessions of 64 / 96 / 128 / 256 streams x 2000 tracks, routes 8 and 9 forced
// in one call on one box (profiles/lkh/threshold.json): 147.9 / 242.5 -> 143.6 / 235.0 us at 128 000 tracks, 208.5 / 351.4 -> 202.1 / 336.3 at 192 000, 267.0 / 456.6 ->
// 254.5 / 432.9 at 256 000, 496.8 / 927.1 -> 460.2 / 897.9 at 512 000, shorter in every run.  128 000 is the smallest load measured, not a crossover: below it the
// route is unmeasured, and the threshold may not go below 102 401, where a test pins k_lk_o<15> as the headline's route of its time.  The protocol was
// repeated with the build for four wavefronts per SIMD (profiles/lkh_lds/threshold.json, same loads, nothing below 128 000): the threshold stays.
inline LkRoute lk_route(int batch, int max_n, int win, const VhTuning& t)
{
    const int force = t.lk_force;
    const long long tracks = (long long)max_n * batch;
    const bool force_nw = force >= 5 && force <= 7;
    const bool by_load = force == 0 || force_nw;  // (modes 5..7 with another window than 51: default routing)
    if (win == 15 && force == 3) return LK_ROUTE_LK3_15;
    if (win == 51 && (by_load || force == 3)) {
        if (force_nw) return (LkRoute)force;
        return force == 3 || tracks < 640 ? LK_ROUTE_LK3_51_W4 : LK_ROUTE_LK3_51_W1;
    }
    if (win == 15 && (force == 9 || (by_load && tracks >= t.lkh_min_tracks))) return LK_ROUTE_H;
    if (win == 15 && (force == 8 || (by_load && tracks >= t.lko_min_tracks))) return LK_ROUTE_O;
    if (win == 15 && (force == 4 || (by_load && tracks >= 3000))) return LK_ROUTE_Q;
    if (force != 1 && win <= 63) return LK_ROUTE_STRIP;  // int32 per-lane partial sums are exact up to 16 strips per lane
    return LK_ROUTE_SAMPLE;
}

// the kernel of a route as DESIGN.md and a rocprofv3 trace name it (the strip kernel has an instantiation for each of the tracker's windows and one for the rest)
inline const char* lk_route_name(int route, int win)
{
    switch (route) {
    case LK_ROUTE_SAMPLE: return "k_lk";
    case LK_ROUTE_STRIP: return win == 15 ? "k_lk_strip<15>" : win == 51 ? "k_lk_strip<51>" : "k_lk_strip<0>";
    case LK_ROUTE_LK3_15: return "k_lk3<15, 1, 6>";
    case LK_ROUTE_Q: return "k_lk_q<15>";
    case LK_ROUTE_LK3_51_W1: return "k_lk3<51, 1, 4>";
    case LK_ROUTE_LK3_51_W2: return "k_lk3<51, 2, 4>";
    case LK_ROUTE_LK3_51_W4: return "k_lk3<51, 4, 4>";
    case LK_ROUTE_O: return "k_lk_o<15>";
    case LK_ROUTE_H: return "k_lk_h<15>";
    default: return "none";
    }
}

// Dynamic LDS of the per-sample kernel (the only one for windows above 63): the packed gradient pair (int32) and the template sample (int16) of every
// window pixel, in whole passes of the wavefront.  A workgroup has 160 KiB, so the largest window any route can solve is 165 x 165 (166 is refused).
// vh_pyr_lk asks vh_lk_window_fits before it enqueues anything; the other callers (vh_klt_regional, vh_klt_main, the session) still learn it from
// vh_launch_lk's -2, after their set-up kernels are queued.
inline size_t lk_per_sample_lds(int win) { return (size_t)(((long long)win * win + 63) / 64) * 64 * 6; }
inline bool lk_window_fits(int win) { return win >= 1 && lk_per_sample_lds(win) <= LK_LDS_WORKGROUP; }
inline int lk_max_window()
{
    int win = 64;
    while (lk_window_fits(win + 1)) win++;
    return win;
}
// ... of the strip kernel: 24 bytes per strip (4 window pixels of a row) and lane, kmax strips per lane
inline size_t lk_strip_lds(int win) { return (size_t)((((win + 3) >> 2) * win + 63) / 64) * 64 * 24; }

struct LkPlan {
    int rc;                   // 0, or -2: no kernel holds a win x win window in LDS (nothing is launched; route says which kernel refused)
    LkRoute route;
    const char* name;         // lk_route_name(route, win)
    unsigned grid_x, grid_y;  // grid_y = batch: one row of workgroups per stream (lk_block_xy re-orders them)
    unsigned block;           // threads of a workgroup
    int tracks_per_wave;      // launch slots a wavefront solves side by side: 4 / 8 / 16 for k_lk_q / k_lk_o / k_lk_h, else 1
    int waves_per_track;      // k_lk3<.., NW, ..>: 1 / 2 / 4, else 1
    int tpw;                  // launch slots a workgroup solves one after the other (k_lk3<.., 1, ..> only, else 1): what vh_profile_lk_tpw reports
    int one_level;            // k_lk3: the single-level form of the kernel
    int strip_win;            // k_lk_strip<strip_win>
    unsigned group;           // the kernel's group argument (lk_block_xy), 0 for the kernels that take none
    size_t lds;               // dynamic LDS the host computes: k_lk and k_lk_strip, all of it; k_lk3: VhTuning::lk_lds_pad, added to LK3<..>::LDS_BYTES by the launcher
    int needs_big_lds;        // lds is above the default limit: hipFuncSetAttribute before the launch
};

// group argument of a launch: sets of `g` streams; pinned from 64 streams on (8+ streams share an XCD: their run times even out), rotated below (a stream's
// workgroups visit every XCD, so a stream that carries more tracks than the others cannot hold one XCD -- and with it the in-order dispatcher -- back)
inline unsigned lk_group_arg(unsigned g, int batch) { return g | (batch < 64 ? LK_GROUP_ROTATE : 0u); }

// max_level: LKJob::max_level of every job of the launch where the caller knows it, -1 = not stated
inline LkPlan lk_plan(int batch, int max_n, int win, int max_level, const VhTuning& t)
{
    LkPlan p = {0, LK_ROUTE_NONE, "none", 0u, 0u, 64u, 1, 1, 1, 0, 0, 0u, 0, 0};
    if (max_n <= 0) return p;
    p.route = lk_route(batch, max_n, win, t);
    p.name = lk_route_name(p.route, win);
    p.grid_y = (unsigned)batch;
    const long long tracks = (long long)max_n * batch;
    switch (p.route) {
    case LK_ROUTE_LK3_15:
    case LK_ROUTE_LK3_51_W1:
    case LK_ROUTE_LK3_51_W2:
    case LK_ROUTE_LK3_51_W4: {
        const int nw = p.route == LK_ROUTE_LK3_51_W2 ? 2 : p.route == LK_ROUTE_LK3_51_W4 ? 4 : 1;
        // Launch slots per workgroup (one-wavefront kernel): a 51 x 51 track keeps a workgroup for ~22 us, and starting one (dispatch, LDS allocation, the block
        // remap, the first descriptor loads) is not free: 4 consecutive slots per workgroup measured 3620 -> 3520 us per launch at 512 000 tracks (2: 3580,
        // 8: 3545; A/B on one box).  Only where the launch still has many workgroups per resident slot (256 CUs x 12): below that the tail would cost more.
        const int tpw_auto = nw != 1 ? 1 : tracks >= 98304 ? 4 : tracks >= 49152 ? 2 : 1;
        const int tpw = nw == 1 && t.lk3_tpw > 0 ? t.lk3_tpw : tpw_auto;
        p.waves_per_track = nw;
        p.tpw = tpw < LK3_MAX_TPW ? tpw : LK3_MAX_TPW;
        p.block = 64u * nw;
        p.grid_x = ((unsigned)max_n + p.tpw - 1) / p.tpw;
        // max_level = 0 is one level whatever the frame size is (fill_pyramid): the single-level form of the kernel.  A caller that does not say takes the general one.
        p.one_level = max_level == 0 && t.lk3_one_level ? 1 : 0;
        p.group = lk_group_arg((unsigned)t.lk3_group, batch);
        p.lds = (size_t)t.lk_lds_pad;
        break;
    }
    case LK_ROUTE_Q:
    case LK_ROUTE_O:
    case LK_ROUTE_H:
        p.tracks_per_wave = p.route == LK_ROUTE_Q ? 4 : p.route == LK_ROUTE_O ? 8 : 16;
        p.grid_x = (unsigned)((max_n + p.tracks_per_wave - 1) / p.tracks_per_wave);
        p.group = lk_group_arg((unsigned)(p.route == LK_ROUTE_Q ? t.lkq_group : t.lko_group), batch);  // (k_lk_h: the group argument of k_lk_o)
        break;
    case LK_ROUTE_STRIP:
        p.strip_win = win == 15 || win == 51 ? win : 0;
        p.grid_x = (unsigned)max_n;
        p.lds = lk_strip_lds(win);
        break;
    default:
        if (!lk_window_fits(win)) { p.rc = -2; return p; }
        p.grid_x = (unsigned)max_n;
        p.lds = lk_per_sample_lds(win);
        break;
    }
    p.needs_big_lds = p.lds > LK_LDS_DEFAULT_LIMIT;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------
// pyrDown of one level for `batch` streams (both pyramids of a stream: grid z = 2 batch), and the border ring of the new level
struct PyrPlan {
    int w, h;                         // level lvl + 1 when level 0 is max_w0 x max_h0
    int rows;                         // k_pyr_down<rows>: 2 / 4 / 8 output rows per thread
    unsigned block_x, block_y;
    unsigned grid_x, grid_y, grid_z;
    unsigned ring_groups;             // k_pyr_pad: workgroups per image
};
inline PyrPlan pyr_plan(int lvl, int max_w0, int max_h0, int batch, const VhTuning& t)
{
    PyrPlan p;
    // dims of level lvl+1 when level 0 is max_w0 x max_h0
    p.w = max_w0; p.h = max_h0;
    for (int l = 0; l <= lvl; l++) { p.w = (p.w + 1) / 2; p.h = (p.h + 1) / 2; }
    // 64 x 4 threads: a wavefront is ONE row of 256 output pixels.  Wavefronts of 16 x 4 or 32 x 2 threads (fewer idle lanes in the last column of
    // workgroups: 818 output pixels are 3.2 wavefronts of 256) measured SLOWER -- 451 / 454 against 405 us for pyrDown + rings at 256 streams: a
    // thread's 19 source rows are shared with no other row of its wavefront, and narrower row segments coalesce worse
    p.block_x = 64; p.block_y = 4;
    // 8 output rows per thread (19 source rows in flight, 136 VGPRs) once a launch is far beyond the chip (19 rows read per 16 produced instead of
    // 11 per 8: 271 -> 250 us for the 766 x 451 level of 256 streams; no gain below), 4 rows from ~1 Mpx, 2 for single-stream latency
    const long long px = (long long)p.w * p.h * batch;
    const int rows = t.pyr_rows ? t.pyr_rows : (px >= (1ll << 25) ? 8 : px >= (1ll << 20) ? 4 : 2);
    p.rows = rows == 8 || rows == 4 ? rows : 2;
    p.grid_x = (p.w + 4 * p.block_x - 1) / (4 * p.block_x);
    p.grid_y = (p.h + p.rows * p.block_y - 1) / (p.rows * p.block_y);
    p.grid_z = (unsigned)batch * 2;
    // border ring of the new level when it is a small one (decided per image on the device): a few workgroups per image, each loops over its share --
    // 4 when the launch has many images (327 against 338 us for pyrDown + rings at 256 streams), 32 for a few streams (a ring of <= ~7000 dwords in one pass:
    // with 4 a single-stream step took 6 us longer)
    p.ring_groups = batch >= 16 ? 4 : 32;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------
// ROI warp: one workgroup of 16 x 16 threads covers RW_BLOCK_PX x RW_BLOCK_ROWS pixels of the ROI (16 RW_PX, 16 RW_ROWS RW_LOOP: tied by a static_assert in
// vh_image.hip)
constexpr unsigned RW_BLOCK_PX = 128, RW_BLOCK_ROWS = 16;
struct RoiWarpPlan {
    unsigned block_x, block_y;
    unsigned grid_x, grid_y, grid_z;
    int xcd_bands;  // the kernel's argument
};
inline RoiWarpPlan roi_warp_plan(int max_w, int max_h, int batch, const VhTuning& t)
{
    // 16 x 16 threads: a wavefront covers 4 consecutive ROI rows of 128 pixels, so the bottom source row of one thread row is the top source row of
    // the next INSIDE the wavefront (one L1 fetch instead of two) and the last column of workgroups idles 28 of 1636 pixels instead of 412.  Measured at
    // 256 streams (A/B on one box): 64 x 4 threads (one 512-pixel row per wavefront) 370 us, 32 x 8 375, 16 x 16 301, 16 x 8 292-302, 8 x 32 305
    RoiWarpPlan p;
    p.block_x = 16; p.block_y = 16;
    const unsigned rows = (max_h + RW_BLOCK_ROWS - 1) / RW_BLOCK_ROWS;
    p.grid_x = (max_w + RW_BLOCK_PX - 1) / RW_BLOCK_PX;
    p.grid_y = t.rw_xcd_bands ? (rows + 7u) & ~7u : rows;  // (padded rows: workgroups beyond the ROI leave at once)
    p.grid_z = (unsigned)batch;
    p.xcd_bands = t.rw_xcd_bands;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------
// RANSAC: up to RANSAC_FUSED_MAX_PAIRS pairs: one fused workgroup per stream, pairs / indices / counts resident in LDS (measured faster than the three
// launches at every stream count, 1 .. 256: 4.53 -> 4.48 ms per step at 128 streams); more pairs: hypotheses spread over the chip
constexpr int RANSAC_FUSED_MAX_PAIRS = 3072;  // RANSAC_FUSED_MAX of the kernel (tied by a static_assert in vh_ransac.hip, where the LDS bytes stay)
struct RansacPlan {
    int fused;          // k_ransac_fused<glue>, else k_ransac_compact + k_ransac_score + k_ransac_select
    int glue;           // the fused kernel's template argument: the glue it runs as its epilogue (0: none)
    int glue_ran;       // what vh_launch_ransac returns: the caller need not launch the glue kernel
    int try_attribute;  // fused, and this device has not been asked yet for the kernel's dynamic LDS: ask, then plan again with the answer
};
// glue: 1 / 2 = the KLTmain glue that follows this RANSAC (0: none); glue_ws_given: the caller passed the streams' workspaces; attribute_state: of the
// device, 0 = not tried, 1 = granted, -1 = refused (the three kernels serve every size)
inline RansacPlan ransac_plan(int max_n, int glue, bool glue_ws_given, int attribute_state, const VhTuning& t)
{
    RansacPlan p = {0, 0, 0, 0};
    const int force = t.ransac_path;
    if (max_n <= RANSAC_FUSED_MAX_PAIRS && (force == 2 || force == 0) && attribute_state >= 0) {
        p.fused = 1;
        p.try_attribute = attribute_state == 0;
        p.glue = glue_ws_given && (glue == 1 || glue == 2) ? glue : 0;
        p.glue_ran = glue_ws_given && glue != 0;
    }
    return p;
}

// ---------------------------------------------------------------------------------------------------------------
// spatial launch order of the tracks (k_klt_setup): pays from the load at which a stream's pyramids no longer sit in every L2 anyway (8 streams: no
// difference measured).  The value goes to the kernel as it is.
inline int klt_track_order(int count, int mn, const VhTuning& t) { return t.klt_order >= 0 ? t.klt_order : ((long long)count * mn >= 24000 ? 1 : 0); }

// the session's frame bookkeeping: ONE kernel (k_sess_frame) up to 4096 track slots per stream, else three launches -- more pose tracks than 256 threads
// keep in registers: the 1024-thread pose kernel between the two bookkeeping halves.  Returns the number of launches.
constexpr int SESS_FRAME_ONE_KERNEL_MAX = 4096;
inline int session_frame_plan(int N0) { return N0 <= SESS_FRAME_ONE_KERNEL_MAX ? 1 : 3; }

// fcnMSV1_t (vidExample.py:155-160) can fire for this session: the predicate that both sizes its scratch and gates its launch
inline bool sess_msv_fires(int msv_frame, int nhist) { return msv_frame >= 1 && msv_frame + 1 <= 2048 && msv_frame < nhist; }
