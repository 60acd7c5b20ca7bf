// Recovery by feature matching: vh_match_affine, the stand-in for estimateAffine2D_SURF (utils/KLT.py:10-33) that KLTmain's recovery branch
// (KLT.py:126-133) asks for the frame-to-frame affine when the coarse stage fails.  Algorithm and its NumPy model: tests/match_ref.py; DESIGN.md
// "Recovery by feature matching".
//
// One call -- vh_match_affine_batch, nb frame pairs of one frame size; vh_match_affine is the batch of one -- is ONE device-resident launch sequence on
// the caller's stream:
//   per pair: k_bounding_rect (query ROI) and, per frame and level > 0, the ROI warp kernel (vh_remap_affine: the level images) -> k_match_mask (all
//   masks) -> k_match_box5 (all box sums) -> ONE pass of the batched frame-0 detector over the 2 x levels x nb level images (vh_detect_images) ->
//   k_match_describe (every keypoint of both frames) -> k_match_2nn -> k_match_compact (good pairs, query order) -> RANSAC (vh_launch_ransac over nb
//   jobs, device pair counts) -> k_match_info.
// The pair is a grid dimension of every k_match_* kernel (one launch each whatever nb is); a pair's MatchJob is read from a device table.
// Counts stay on the device: every kernel is launched over the budgets and reads the keypoint counts the detector left.
// Everything is integer except the level-0 position of a keypoint, (x + 0.5) * inv_s - 0.5 in float32 (two roundings: the build has -ffp-contract=off).
#include <atomic>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "vh_ws.hpp"

namespace match_dev {
#define VH_MATCH_PAIRS_QUAL __device__ const
#include "vh_match_pairs.hpp"
#undef VH_MATCH_PAIRS_QUAL
}  // namespace match_dev
#include "vh_match_pairs.hpp"  // the host copy (vh_match_pairs)

#define VH_MATCH_MAX_LEVELS 8
#define VH_MATCH_BORDER 16          // keypoints keep this distance from every edge: the pattern reaches 13 px, the box sum 2 more
#define VH_MATCH_MAX_PER_LEVEL 2048 // the detector's in-LDS selection (no segmented-sort scratch)
static_assert(VH_MATCH_REACH + 2 < VH_MATCH_BORDER, "the descriptor must stay inside the level image");

struct MatchLevel {  // one level image of one frame
    const uint8_t* img;
    int w, h, stride;
    uint8_t* mask;        // w x h, dense
    unsigned short* box;  // w x h, dense: 5x5 box sums (<= 25 * 255)
    float* kp;            // budget x 2: detector output, level coordinates
    int* cnt;             // 1: keypoints found
    float scale, inv_scale;
};

struct MatchJob {  // one frame pair; the kernels read it from a device table
    MatchLevel lv[2][VH_MATCH_MAX_LEVELS];  // [0]: query frame (im1), [1]: train frame (im2)
    int levels, budget[2];
    const int* roi;     // 4: query ROI at level 0 (x0, x1, y0, y1)
    float* pos[2];      // level-0 positions, compacted level-major
    uint8_t* desc[2];   // 32 bytes per keypoint, same order
    int* nn;            // qcap x 4
    uint8_t* good;      // qcap
    int* ngood;         // 1
    float *from, *to;   // qcap x 2 each: the good pairs RANSAC reads
    float* pairs_out;   // caller's qcap x 4 (may be null)
    int ratio_num, ratio_den;
    const int* status;  // RANSAC's verdict on this pair
    const uint8_t* inl; // caller's qcap inlier flags (RANSAC's output)
    double* M;          // caller's 6
    int* info;          // caller's 4
};

static std::atomic<long long> g_match_launches{0};
#define MATCH_LAUNCH(kernel, grid, block, s, ...)                  \
    do {                                                           \
        hipLaunchKernelGGL(kernel, grid, block, 0, s, __VA_ARGS__); \
        g_match_launches.fetch_add(1, std::memory_order_relaxed);  \
    } while (0)

// keypoints of image `img` on the levels before `level` (the compacted index of a level's first keypoint); level = levels: all of them
__device__ __forceinline__ int match_prefix(const MatchJob& J, int img, int level)
{
    int s = 0;
    for (int l = 0; l < level; l++) s += min(*J.lv[img][l].cnt, J.budget[img]);
    return s;
}

// ---- masks of every level of both frames: BORDER px from every edge; the query frame also inside its ROI scaled to the level ----------------------
__global__ __launch_bounds__(256) void k_match_mask(const MatchJob* tab, int levels)
{
    const MatchJob& J = tab[blockIdx.z / (2 * levels)];
    const int img = (blockIdx.z / levels) & 1, l = blockIdx.z % levels;
    const MatchLevel& L = J.lv[img][l];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= L.w || y >= L.h) return;
    int x0 = VH_MATCH_BORDER, x1 = L.w - VH_MATCH_BORDER, y0 = VH_MATCH_BORDER, y1 = L.h - VH_MATCH_BORDER;
    if (img == 0) {
        x0 = max(x0, (int)((float)J.roi[0] * L.scale));
        x1 = min(x1, (int)((float)J.roi[1] * L.scale));
        y0 = max(y0, (int)((float)J.roi[2] * L.scale));
        y1 = min(y1, (int)((float)J.roi[3] * L.scale));
    }
    L.mask[(size_t)y * L.w + x] = (x >= x0 && x < x1 && y >= y0 && y < y1) ? 1 : 0;
}

// ---- 5x5 box sums of every level of both frames (zero outside the image): four neighbouring pixels per thread -------------------------------------
__global__ __launch_bounds__(256) void k_match_box5(const MatchJob* tab, int levels)
{
    const MatchJob& J = tab[blockIdx.z / (2 * levels)];
    const int img = (blockIdx.z / levels) & 1, l = blockIdx.z % levels;
    const MatchLevel& L = J.lv[img][l];
    const int x4 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
    if (x4 >= L.w || y >= L.h) return;
    int s[4] = {0, 0, 0, 0};
    for (int j = -2; j <= 2; j++) {
        const int yy = y + j;
        if (yy < 0 || yy >= L.h) continue;
        const uint8_t* row = L.img + (size_t)yy * L.stride;
        int v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int xx = x4 - 2 + i;
            v[i] = (xx >= 0 && xx < L.w) ? row[xx] : 0;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) s[k] += v[k] + v[k + 1] + v[k + 2] + v[k + 3] + v[k + 4];
    }
    unsigned short* out = L.box + (size_t)y * L.w + x4;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (x4 + k < L.w) out[k] = (unsigned short)s[k];
}

// ---- descriptors: one wavefront per keypoint slot of every level of both frames; four comparisons per lane, each round collected by a ballot -------
__global__ __launch_bounds__(256) void k_match_describe(const MatchJob* tab)
{
    const MatchJob& J = tab[blockIdx.z];
    const int img = blockIdx.y / J.levels, l = blockIdx.y % J.levels;
    const MatchLevel& L = J.lv[img][l];
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (slot >= min(*L.cnt, J.budget[img])) return;  // (wave-uniform)
    const int idx = match_prefix(J, img, l) + slot;
    const float fx = L.kp[2 * slot], fy = L.kp[2 * slot + 1];
    const int x = (int)fx, y = (int)fy;
    // the mask keeps the detector BORDER px inside; a position that is not could only come from a broken detector: an all-zero descriptor, no stray read
    const bool inside = x >= VH_MATCH_REACH && x < L.w - VH_MATCH_REACH && y >= VH_MATCH_REACH && y < L.h - VH_MATCH_REACH;
    uint8_t* d = J.desc[img] + (size_t)idx * 32;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const signed char* o = match_dev::VH_MATCH_PAIRS[r * 64 + lane];
        bool bit = false;
        if (inside) bit = L.box[(size_t)(y + o[1]) * L.w + (x + o[0])] < L.box[(size_t)(y + o[3]) * L.w + (x + o[2])];
        const unsigned long long word = __ballot(bit);  // lane i <-> bit i
        // np.packbits order: comparison 8 j + i is bit 7 - i of byte j
        if (lane < 8) d[r * 8 + lane] = (uint8_t)(__brev((unsigned)((word >> (8 * lane)) & 0xffull)) >> 24);
    }
    if (lane == 0) {
        float* p = J.pos[img] + 2 * (size_t)idx;
        const float ax = fx + 0.5f, ay = fy + 0.5f;
        const float mx = ax * L.inv_scale, my = ay * L.inv_scale;
        p[0] = mx - 0.5f;
        p[1] = my - 0.5f;
    }
}

// ---- 2-nearest-neighbour Hamming matching: one wavefront per query, lanes stride over the train descriptors ---------------------------------------
// A candidate is the key (distance << 20 | train index): smaller key = (distance, index) ascending, all keys of a query distinct.
__global__ __launch_bounds__(256) void k_match_2nn(const MatchJob* tab)
{
    const MatchJob& J = tab[blockIdx.y];
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int nq = match_prefix(J, 0, J.levels), nt = match_prefix(J, 1, J.levels);
    if (q >= nq) return;  // (wave-uniform)
    const uint4* dq = reinterpret_cast<const uint4*>(J.desc[0] + (size_t)q * 32);
    const uint4 a0 = dq[0], a1 = dq[1];
    const uint4* dt = reinterpret_cast<const uint4*>(J.desc[1]);
    unsigned k1 = 0xffffffffu, k2 = 0xffffffffu;
    for (int j = lane; j < nt; j += 64) {
        const uint4 b0 = dt[2 * j], b1 = dt[2 * j + 1];
        const int dist = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
                         __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
        const unsigned key = ((unsigned)dist << 20) | (unsigned)j;
        k2 = min(k2, max(k1, key));
        k1 = min(k1, key);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned o1 = __shfl_xor(k1, o, 64), o2 = __shfl_xor(k2, o, 64);
        k2 = min(max(k1, o1), min(k2, o2));
        k1 = min(k1, o1);
    }
    if (lane == 0) {
        const bool h1 = k1 != 0xffffffffu, h2 = k2 != 0xffffffffu;
        const int d1 = (int)(k1 >> 20), d2 = (int)(k2 >> 20);
        int* nn = J.nn + 4 * (size_t)q;
        nn[0] = h1 ? (int)(k1 & 0xfffffu) : -1;
        nn[1] = h1 ? d1 : -1;
        nn[2] = h2 ? (int)(k2 & 0xfffffu) : -1;
        nn[3] = h2 ? d2 : -1;
        J.good[q] = (h2 && J.ratio_den * d1 < J.ratio_num * d2) ? 1 : 0;
    }
}

// ---- the good pairs, in query order, into the arrays RANSAC reads (and the caller's pair list) -----------------------------------------------------
__global__ __launch_bounds__(1024) void k_match_compact(const MatchJob* tab)
{
    const MatchJob& J = tab[blockIdx.x];
    __shared__ int wcount[16];
    __shared__ int base;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nq = match_prefix(J, 0, J.levels);
    if (tid == 0) base = 0;
    __syncthreads();
    for (int c = 0; c < nq; c += 1024) {
        const int q = c + tid;
        const bool f = q < nq && J.good[q] != 0;
        const unsigned long long bal = __ballot(f);
        const int pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcount[wave] = __popcll(bal);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            const int cw = wcount[w];
            off += w < wave ? cw : 0;
            tot += cw;
        }
        if (f) {
            const int k = off + pre, t = J.nn[4 * (size_t)q];
            const float ax = J.pos[0][2 * (size_t)q], ay = J.pos[0][2 * (size_t)q + 1];
            const float bx = J.pos[1][2 * (size_t)t], by = J.pos[1][2 * (size_t)t + 1];
            J.from[2 * k] = ax; J.from[2 * k + 1] = ay;
            J.to[2 * k] = bx;   J.to[2 * k + 1] = by;
            if (J.pairs_out) reinterpret_cast<float4*>(J.pairs_out)[k] = make_float4(ax, ay, bx, by);
        }
        __syncthreads();
        if (tid == 0) base += tot;
        __syncthreads();
    }
    if (tid == 0) *J.ngood = base;
}

// ---- info = (status, good pairs, inliers, query keypoints) ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_match_info(const MatchJob* tab)
{
    const MatchJob& J = tab[blockIdx.x];
    const int* status = J.status;
    const uint8_t* inl = J.inl;
    double* M = J.M;
    int* info = J.info;
    __shared__ int s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const int ng = *J.ngood, st = *status > 0 ? 1 : 0;
    int c = 0;
    if (st)
        for (int i = threadIdx.x; i < ng; i += 256) c += inl[i] != 0;
    c = vh_wave_sum_i32(c);
    if ((threadIdx.x & 63) == 0) atomicAdd(&s_sum, c);
    __syncthreads();
    if (threadIdx.x == 0) {
        info[0] = st;
        info[1] = ng;
        info[2] = s_sum;
        info[3] = match_prefix(J, 0, J.levels);
    }
    if (!st && threadIdx.x < 6) M[threadIdx.x] = 0.0;
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
struct MatchScratch {
    VhDeviceBlock block;  // laid out by match_carve
    vh_match_stages last;  // what vh_match_stage_ptrs hands out
    int have_last;
};

static const vh_match_params MATCH_DEFAULTS = {5, 500, 1000, 5, 50, 50, 4, 5, 10, 0.01};

static double match_scale(int l) { return pow(2.0, -l / 4.0); }
static void match_dims(int w, int h, int l, int* wl, int* hl)
{
    const double s = match_scale(l);
    *wl = l ? (int)nearbyint(w * s) : w;  // (round half to even, as np.rint)
    *hl = l ? (int)nearbyint(h * s) : h;
}

static int match_check(const vh_match_params& P, int w, int h, const char* fn)
{
    char msg[200];
    const bool ok = P.levels >= 1 && P.levels <= VH_MATCH_MAX_LEVELS && P.query_per_level >= 1 && P.query_per_level <= VH_MATCH_MAX_PER_LEVEL &&
                    P.train_per_level >= 1 && P.train_per_level <= VH_MATCH_MAX_PER_LEVEL && P.block >= 1 && P.block <= 15 && P.border_x >= 0 &&
                    P.border_y >= 0 && P.ratio_num >= 1 && P.ratio_den >= 1 && P.ratio_num <= 1024 && P.ratio_den <= 1024 && P.min_good >= 0 &&
                    std::isfinite(P.quality) && P.quality > 0 && w >= 3 && h >= 3 && w <= 32767 && h <= 32767;
    int wl = 0, hl = 0;
    if (ok) match_dims(w, h, P.levels - 1, &wl, &hl);
    if (!ok || wl < 3 || hl < 3) {
        snprintf(msg, sizeof(msg), "%s: bad arguments (levels 1..8, per-level budgets 1..2048, block 1..15, borders >= 0, ratio terms 1..1024, min_good >= 0, "
                                   "quality > 0, every level at least 3 x 3)", fn);
        return vh_fail(-1, msg);
    }
    return 0;
}

// the pair is part of grid.z of the mask and box-sum kernels and of the detector's tile grid
static int match_check_nb(int nb, const vh_match_params& P, const char* fn)
{
    char msg[160];
    if (nb < 1 || (long long)nb * 2 * P.levels > 65535) {
        snprintf(msg, sizeof(msg), "%s: bad arguments (nb >= 1 and nb x 2 x levels <= 65535)", fn);
        return vh_fail(-1, msg);
    }
    return 0;
}

struct MatchPairBufs {  // per-pair scratch outside the MatchJob
    int *status, *idx, *counts, *m, *bound;
    float4* rpairs;
};
struct MatchLayout {
    int* cnt;         // nb x 2 x VH_MATCH_MAX_LEVELS keypoint counts, zeroed by one memset per call
    MatchJob* jobs;   // nb
    RansacJob* rjobs; // nb
    size_t bytes, level_px;  // level_px: pixels of the 2 x levels level images of one pair
};

// Lays the scratch of nb pairs out (base may be null: sizes only) and fills the jobs' pointers (J, X: nb entries each, may be null).
static MatchLayout match_carve(char* base, int nb, int w, int h, const vh_match_params& P, MatchJob* J, MatchPairBufs* X)
{
    VhCarver A(base);
    const int qcap = P.levels * P.query_per_level, tcap = P.levels * P.train_per_level;
    MatchLayout Y;
    Y.level_px = 0;
    Y.cnt = A.take<int>((size_t)2 * VH_MATCH_MAX_LEVELS * nb);
    Y.jobs = A.take<MatchJob>(nb);
    Y.rjobs = A.take<RansacJob>(nb);
    for (int b = 0; b < nb; b++) {
        int* cnt = Y.cnt + (size_t)b * 2 * VH_MATCH_MAX_LEVELS;
        int* roi = A.take<int>(4);
        int* small = A.take<int>(4);
        for (int img = 0; img < 2; img++) {
            const int budget = img ? P.train_per_level : P.query_per_level;
            for (int l = 0; l < P.levels; l++) {
                int wl, hl;
                match_dims(w, h, l, &wl, &hl);
                const size_t px = (size_t)wl * hl;
                if (b == 0) Y.level_px += px;
                uint8_t* image = A.take<uint8_t>(l ? px : 0);  // (level 0 is the caller's frame: a take of 0 moves nothing)
                uint8_t* mask = A.take<uint8_t>(px);
                unsigned short* box = A.take<unsigned short>(px);
                float* kp = A.take<float>((size_t)2 * budget);
                if (J) {
                    MatchLevel& L = J[b].lv[img][l];
                    if (l) { L.img = image; L.stride = wl; }
                    L.w = wl; L.h = hl; L.mask = mask; L.box = box; L.kp = kp; L.cnt = cnt + img * VH_MATCH_MAX_LEVELS + l;
                    L.scale = (float)match_scale(l);
                    L.inv_scale = (float)(1.0 / match_scale(l));
                }
            }
        }
        float *pos0 = A.take<float>((size_t)2 * qcap), *pos1 = A.take<float>((size_t)2 * tcap);
        uint8_t *desc0 = A.take<uint8_t>((size_t)32 * qcap), *desc1 = A.take<uint8_t>((size_t)32 * tcap);
        int* nn = A.take<int>((size_t)4 * qcap);
        uint8_t* good = A.take<uint8_t>(qcap);
        float *from = A.take<float>((size_t)2 * qcap), *to = A.take<float>((size_t)2 * qcap);
        int* idx = A.take<int>(qcap);
        float4* rpairs = A.take<float4>(qcap);
        int* counts = A.take<int>(VH_RANSAC_ITERS);
        if (J) {
            MatchJob& Q = J[b];
            Q.levels = P.levels; Q.budget[0] = P.query_per_level; Q.budget[1] = P.train_per_level;
            Q.roi = roi; Q.pos[0] = pos0; Q.pos[1] = pos1; Q.desc[0] = desc0; Q.desc[1] = desc1; Q.nn = nn; Q.good = good; Q.ngood = small;
            Q.from = from; Q.to = to; Q.ratio_num = P.ratio_num; Q.ratio_den = P.ratio_den; Q.status = small + 1;
        }
        if (X) { X[b].status = small + 1; X[b].m = small + 2; X[b].bound = small + 3; X[b].idx = idx; X[b].rpairs = rpairs; X[b].counts = counts; }
    }
    Y.bytes = A.bytes();
    return Y;
}

void vh_match_scratch_free(vh_ctx* c)
{
    if (!c || !c->match) return;
    MatchScratch* S = static_cast<MatchScratch*>(c->match);
    S->block.release();
    delete S;
    c->match = nullptr;
}

// scratch for nb pairs of w x h frames with parameters P (never shrinks); growth waits for the stream, and is refused inside a capture
static int match_reserve(vh_ctx* c, int nb, int w, int h, const vh_match_params& P, hipStream_t s)
{
    const MatchLayout Y = match_carve(nullptr, nb, w, h, P, nullptr, nullptr);
    int r = vh_detect_reserve(c, 2 * P.levels * nb, Y.level_px * nb, s);  // the detector's own scratch: one pass over every level image
    if (r) return r;
    if (!c->match && !(c->match = new (std::nothrow) MatchScratch())) return vh_fail(-1, "vh_match: out of host memory");
    MatchScratch* S = static_cast<MatchScratch*>(c->match);
    const size_t had = S->block.bytes;
    r = S->block.reserve(Y.bytes, s, "the matching scratch", "call vh_match_reserve(ctx, w, h, params) or vh_match_reserve_batch before capturing");
    if (S->block.bytes != had) S->have_last = 0;  // (the stage pointers of the last call died with the old block)
    return r;
}

extern "C" VH_API int vh_match_reserve_batch(vh_ctx* c, int nb, int w, int h, const vh_match_params* params_host, void* stream)
{
    if (!c) return vh_fail(-1, "vh_match_reserve_batch: bad arguments");
    const vh_match_params P = params_host ? *params_host : MATCH_DEFAULTS;
    int r = match_check(P, w, h, "vh_match_reserve_batch");
    if (r || (r = match_check_nb(nb, P, "vh_match_reserve_batch"))) return r;
    VH_BIND(c, stream);
    return match_reserve(c, nb, w, h, P, bound_.s);
}

extern "C" VH_API int vh_match_reserve(vh_ctx* c, int w, int h, const vh_match_params* params_host, void* stream)
{
    if (!c) return vh_fail(-1, "vh_match_reserve: bad arguments");
    const vh_match_params P = params_host ? *params_host : MATCH_DEFAULTS;
    int r = match_check(P, w, h, "vh_match_reserve");
    if (r) return r;
    VH_BIND(c, stream);
    return match_reserve(c, 1, w, h, P, bound_.s);
}

// stream-ordered upload of n descriptors, as many per kernel argument as 2 KiB hold
template <typename T, int N>
struct MatchPiece {
    T v[N];
};
template <typename T>
static int match_upload(T* dst, const T* src, int n, hipStream_t s)
{
    constexpr int PER = sizeof(T) >= 2048 ? 1 : (int)(2048 / sizeof(T));
    typedef MatchPiece<T, PER> Piece;
    for (int i0 = 0; i0 < n; i0 += PER) {
        if (n - i0 >= PER) {
            Piece piece;
            memcpy(piece.v, src + i0, sizeof(piece));
            VH_CHECK(vh_store(reinterpret_cast<Piece*>(dst + i0), piece, s));
        } else {
            for (int i = i0; i < n; i++) VH_CHECK(vh_store(dst + i, src[i], s));  // (a whole piece would write past the table's end)
        }
    }
    return 0;
}

// the launch sequence of nb pairs; every argument has been checked.  M [nb][6], inl [nb][qcap], pairs [nb][qcap][4] or null, info [nb][4]
static int match_run(vh_ctx* c, int nb, const uint8_t* const* im1, const uint8_t* const* im2, int w, int h, int stride1, int stride2, const float* const* p1,
                     const int* n, const vh_match_params& P, double* M, uint8_t* inl, float* pairs, int* info, hipStream_t s)
{
    const int qcap = P.levels * P.query_per_level;
    int r = match_reserve(c, nb, w, h, P, s);
    if (r) return r;
    MatchScratch* S = static_cast<MatchScratch*>(c->match);
    std::vector<MatchJob> J((size_t)nb);
    std::vector<MatchPairBufs> X((size_t)nb);
    std::vector<RansacJob> R((size_t)nb);
    memset(J.data(), 0, sizeof(MatchJob) * nb);
    memset(R.data(), 0, sizeof(RansacJob) * nb);
    const MatchLayout Y = match_carve(S->block.p, nb, w, h, P, J.data(), X.data());
    const StreamBufs& B = c->h_bufs[0];
    for (int b = 0; b < nb; b++) {
        MatchJob& Q = J[b];
        Q.lv[0][0].img = im1[b]; Q.lv[0][0].stride = stride1;
        Q.lv[1][0].img = im2[b]; Q.lv[1][0].stride = stride2;
        Q.pairs_out = pairs ? pairs + (size_t)b * qcap * 4 : nullptr;
        Q.inl = inl + (size_t)b * qcap; Q.M = M + 6 * (size_t)b; Q.info = info + 4 * (size_t)b;
        // estimateAffine2D on the good pairs: the device count is the job's n, fewer than min_good (or three) pairs report status 0
        RansacJob& A = R[b];
        A.from = Q.from; A.to = Q.to; A.valid = B.v_all; A.n_ptr = Q.ngood; A.n = qcap; A.min_valid = P.min_good - 1; A.gate_valid = 0;
        A.idx = X[b].idx; A.pairs = X[b].rpairs; A.counts = X[b].counts; A.m_out = X[b].m; A.bound = X[b].bound; A.M = Q.M;
        A.inl = inl + (size_t)b * qcap; A.status = X[b].status;
    }
    VH_CHECK(hipMemsetAsync(Y.cnt, 0, sizeof(int) * 2 * VH_MATCH_MAX_LEVELS * nb, s));
    VH_CHECK(hipMemsetAsync(inl, 0, (size_t)qcap * nb, s));
    VH_CHECK(hipMemsetAsync(M, 0, sizeof(double) * 6 * nb, s));
    if ((r = match_upload(Y.jobs, J.data(), nb, s)) || (r = match_upload(Y.rjobs, R.data(), nb, s))) return r;
    std::vector<vh_detect_image> D((size_t)nb * 2 * P.levels);
    for (int b = 0; b < nb; b++) {
        const MatchJob& Q = J[b];
        if ((r = vh_bounding_rect(c, p1[b], n[b], w, h, P.border_x, P.border_y, const_cast<int*>(Q.roi), s))) return r;
        // level images: level 0 resampled at ((x + 0.5) / s - 0.5, (y + 0.5) / s - 0.5), bilinear
        for (int img = 0; img < 2; img++)
            for (int l = 0; l < P.levels; l++) {
                const MatchLevel& L = Q.lv[img][l];
                D[((size_t)b * 2 + img) * P.levels + l] = vh_detect_image{L.img, L.w, L.h, L.stride, L.mask, L.w, Q.budget[img], L.kp, L.cnt};
                if (!l) continue;
                const double sc = match_scale(l);
                const float T[6] = {(float)(1.0 / sc), 0.f, 0.f, (float)(1.0 / sc), (float)(0.5 / sc - 0.5), (float)(0.5 / sc - 0.5)};
                if ((r = vh_remap_affine(c, Q.lv[img][0].img, w, h, Q.lv[img][0].stride, T, 0, L.w, 0, L.h, const_cast<uint8_t*>(L.img), s))) return r;
            }
    }
    const int nz = 2 * P.levels * nb;
    MATCH_LAUNCH(k_match_mask, dim3((w + 255) / 256, h, nz), dim3(256), s, Y.jobs, P.levels);
    MATCH_LAUNCH(k_match_box5, dim3((w + 255) / 256, (h + 3) / 4, nz), dim3(64, 4), s, Y.jobs, P.levels);
    // corners: ONE pass of the batched frame-0 detector over every level image of every pair (Shi-Tomasi, min_distance 0, masked)
    if ((r = vh_detect_images(c, D.data(), nz, P.quality, P.block, 0, 0.04, s))) return r;
    const int bmax = P.query_per_level > P.train_per_level ? P.query_per_level : P.train_per_level;
    MATCH_LAUNCH(k_match_describe, dim3((bmax + 3) / 4, 2 * P.levels, nb), dim3(256), s, Y.jobs);
    MATCH_LAUNCH(k_match_2nn, dim3((qcap + 3) / 4, nb), dim3(256), s, Y.jobs);
    MATCH_LAUNCH(k_match_compact, dim3(nb), dim3(1024), s, Y.jobs);
    vh_launch_ransac(Y.rjobs, sizeof(RansacJob), nb, qcap, s);
    MATCH_LAUNCH(k_match_info, dim3(nb), dim3(256), s, Y.jobs);
    VH_CHECK(hipGetLastError());

    const MatchJob& Q = J[nb - 1];  // the stages of the call's last pair stay readable (vh_match_stage_ptrs)
    vh_match_stages& V = S->last;
    memset(&V, 0, sizeof(V));
    for (int img = 0; img < 2; img++) {
        for (int l = 0; l < P.levels; l++) V.kp[img][l] = Q.lv[img][l].kp;
        V.pos[img] = Q.pos[img];
        V.desc[img] = Q.desc[img];
    }
    V.cnt = Q.lv[0][0].cnt; V.nn = Q.nn; V.good = Q.good; V.roi = Q.roi; V.levels = P.levels;
    for (int l = 0; l < P.levels; l++) { V.lw[l] = Q.lv[0][l].w; V.lh[l] = Q.lv[0][l].h; }
    S->have_last = 1;
    return 0;
}

extern "C" VH_API int vh_match_affine(vh_ctx* c, const uint8_t* im1, const uint8_t* im2, int w, int h, int stride1, int stride2, const float* p1, int n,
                                      const vh_match_params* params_host, double* M, uint8_t* inl, float* pairs, int* info, void* stream)
{
    if (!c || !im1 || !im2 || !p1 || !M || !inl || !info || n < 1 || stride1 < w || stride2 < w)
        return vh_fail(-1, "vh_match_affine: bad arguments (null pointer, n < 1 or a row stride below the width)");
    const vh_match_params P = params_host ? *params_host : MATCH_DEFAULTS;
    int r = match_check(P, w, h, "vh_match_affine");
    if (r) return r;
    if (P.levels * P.query_per_level > c->max_pts) return vh_fail(-1, "vh_match_affine: levels x query_per_level exceeds the context's max_pts");
    VH_BIND(c, stream);
    return match_run(c, 1, &im1, &im2, w, h, stride1, stride2, &p1, &n, P, M, inl, pairs, info, bound_.s);
}

extern "C" VH_API int vh_match_affine_batch(vh_ctx* c, int nb, const uint8_t* const* im1_host, const uint8_t* const* im2_host, int w, int h, int stride1,
                                            int stride2, const float* const* p1_host, const int* n_host, const vh_match_params* params_host, double* M,
                                            uint8_t* inl, float* pairs, int* info, void* stream)
{
    if (!c || !im1_host || !im2_host || !p1_host || !n_host || !M || !inl || !info || stride1 < w || stride2 < w)
        return vh_fail(-1, "vh_match_affine_batch: bad arguments (null pointer or a row stride below the width)");
    const vh_match_params P = params_host ? *params_host : MATCH_DEFAULTS;
    int r = match_check(P, w, h, "vh_match_affine_batch");
    if (r || (r = match_check_nb(nb, P, "vh_match_affine_batch"))) return r;
    for (int b = 0; b < nb; b++)
        if (!im1_host[b] || !im2_host[b] || !p1_host[b] || n_host[b] < 1)
            return vh_fail(-1, "vh_match_affine_batch: a pair has a null frame, null points or n < 1");
    if (P.levels * P.query_per_level > c->max_pts) return vh_fail(-1, "vh_match_affine_batch: levels x query_per_level exceeds the context's max_pts");
    VH_BIND(c, stream);
    return match_run(c, nb, im1_host, im2_host, w, h, stride1, stride2, p1_host, n_host, P, M, inl, pairs, info, bound_.s);
}

extern "C" VH_API int vh_match_stage_ptrs(vh_ctx* c, vh_match_stages* out)
{
    MatchScratch* S = c ? static_cast<MatchScratch*>(c->match) : nullptr;
    if (!S || !out || !S->have_last) return vh_fail(-1, "vh_match_stage_ptrs: no vh_match_affine call on this context yet");
    *out = S->last;
    return 0;
}

extern "C" VH_API int vh_match_pairs(int* out_host)
{
    if (!out_host) return vh_fail(-1, "vh_match_pairs: bad arguments");
    for (int k = 0; k < VH_MATCH_NPAIRS; k++)
        for (int i = 0; i < 4; i++) out_host[4 * k + i] = VH_MATCH_PAIRS[k][i];
    return 0;
}

extern "C" VH_API long long vh_match_launch_count(void) { return g_match_launches.load(std::memory_order_relaxed); }
