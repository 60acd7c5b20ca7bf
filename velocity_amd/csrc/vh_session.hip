// Tracker session: the body of the reference's frame loop (vidExample.py:133-160) for `batch` independent video
// streams, entirely on the device -- KLTmain, the track-state bookkeeping (K19: vg[vg]=v, vp&=vg, stream compaction,
// pose-track selection, NaN-padded history P), estimateWorldCameraPose(findR=False), the B/S result records and, at
// the MSV frame, fcnMSV1_t.  One step = a fixed sequence of launches over all streams, no host round trip.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

#include <stddef.h>

#include "vh_ws.hpp"
#include "vh_ba.hpp"
#include "vh_pose_dev.hpp"

// History P (vidExample.py:128-129: [5, N0, n] in the reference) is kept FRAME-MAJOR on the device, [nhist][5][N0]: a frame writes its five rows as five
// contiguous runs.  In the reference's layout the entries of one frame are nhist floats apart: 10 000 single-float stores per stream and frame, each into
// its own cache line -- at 256 streams 2.6 M partial-line writes per step, which is what made k_sess_frame take 140 us there and 70 us for one stream.
// velocity_amd/driver.py::TrackerSession.state() hands the reference's [5, N0, nhist] view to the caller.
__device__ __host__ __forceinline__ size_t sess_P(int row, int track, int frame, int N0) { return ((size_t)frame * 5 + row) * (size_t)N0 + track; }

// The recovery branch of KLTmain (KLT.py:130-133) for the session's streams (vh_session_set_fallback; off unless asked for).  The failure predicate is read
// on the HOST: one small record per stream and step.  The rare branch is composed from the stateless entry points -- vh_match_affine_batch over the
// failed streams, then KLTregional per stream with a model -- on a context of the session's own: those entry points park their job descriptors in slot 0
// of the context they are given, where the session's context keeps stream 0's.
#define SESS_FB_CHUNK 16  // failed streams per vh_match_affine_batch call (bounds the matcher's scratch: it is per pair)
struct SessFbRec {
    int flags, n_cur;
    const uint8_t* im0;
    const uint8_t* im;
};
struct SessFallback {
    int on, chunk;
    vh_match_params params;
    vh_ctx* ctx;        // batch 1, the session's (maximum) frame size, max_pts >= max(N0, levels x query_per_level)
    VhPinnedBlock host;  // h_rec, h_M, h_info
    VhDeviceBlock dev;   // d_rec, d_M, d_info, d_inl: both laid out by sess_fb_carve for (batch, chunk, qcap) and regrown whole when qcap grows
    SessFbRec *h_rec, *d_rec;  // [batch]
    double *h_M, *d_M;         // [chunk][6]
    int *h_info, *d_info;      // [chunk][4]
    uint8_t* d_inl;            // [chunk][levels x query_per_level]
    int* counts;        // host [batch][2]: the recovery ran, it found a model
};

// Replenishment (vh_session_set_replenish; off unless asked for): lost tracks are replaced by new corners, which are triangulated on the device once they
// have a baseline.  The state lives BESIDE the streams, not in them: SessStream keeps its layout and a step with the option off touches none of it.
#define SESS_RP_CHUNK 16     // streams per detector pass (bounds the mask planes and the detector's response planes and key segments: they are per stream)
#define SESS_RP_MAXBASE 63   // baseline + 1 ray origins and translations of a stream sit in LDS
struct SessRepl {  // device resident, one per stream
    int* born;     // [N0] the frame at which row g entered (0: a frame-0 track, -1: never used)
    uint8_t* tri;  // [N0] p3[g] is defined
    int n_rows;    // rows used so far: a birth takes rows n_rows.. (tail rows only)
    int n_new;     // corners the detector found in the birth under way
    int due;       // the birth under way got as far as the detector (k_replenish_setup -> k_replenish_append)
    int cnt[3];    // since the slot's initialisation: rows born, promoted, rejected
};
struct SessReplenish {
    int on, chunk;
    vh_replenish_params P;
    VhDeviceBlock dev;  // laid out by sess_rp_carve
    SessRepl* d_rp;     // [batch]
    SessRepl* h_rp;     // host mirror of the pointer fields
    uint8_t* d_mask;    // [chunk] exclusion masks, w x h each (a stream's is ROI-relative: rows rw apart)
    float* d_rows;      // [chunk][max_new + 4][2] corner rows of the detector pass
};

struct vh_session {
    vh_ctx* ctx;
    int batch, N0, nhist, w, h, msv_frame, k_is_f32;
    vh_lk_params coarse, fine;
    VhDeviceBlock arena;  // laid out by sess_carve
    SessStream* d_ss;
    SessStream* h_ss;  // host mirror of the pointer fields and of every slot's camera (w, h, K: vh_session_set_camera) and row stride
    IngestJob* d_ingest;  // [batch] descriptors of the fused BGR ingest
    int* h_frame;      // per stream: frames stepped since its vh_session_init (host mirror of SessStream::frame_i; the
                       // reference fires fcnMSV1_t at `i == msvFrame` of EACH video, vidExample.py:155)
    SessFallback fb;
    SessReplenish rp;
    // anchored points of each slot's clip (vh_session_set_anchors): world points the refinement holds fixed.  Kept beside the streams, not in them:
    // a step neither reads nor writes them
    uint8_t* d_anc_mask;  // [batch][N0] non-zero = track id is anchored
    double* d_anc_xyz;    // [batch][N0][3] its coordinates, in the frame of the clip's camera 0 (rows of unanchored ids: undefined)
    int* h_nanchor;       // per slot: anchors set (host)
    char* h_inited;       // per slot: vh_session_init has run
    double refine_robust; // Huber threshold (pixels) of every refinement (vh_session_set_refine_robust); 0 = off: plain least squares
};

#define SESS_CHECK() VH_CHECK(hipGetLastError())

// ---------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------
// vg[vg] = v ; vp &= vg ; p = p[v] ; pose selection p[vp[vg]] / p3[vp]   (vidExample.py:134-139)
// A thread owns up to 16 CONSECUTIVE current tracks: it loads all of them at once (one memory round trip, not one per 256-track chunk), both
// order-preserving compactions -- the surviving tracks and, among them, the pose tracks -- come from one block-wide exclusive scan of the two
// per-thread counts.  `vp &= vg` only ever changes the entries of CURRENT tracks (a dropped track's vg and vp are already 0), so the two mask
// updates are per-track stores instead of passes over all N0 entries.
template <int NT>
__device__ __forceinline__ void sess_book_a(SessStream& S)
{
    constexpr int EPT = 4096 / NT, NW = NT / 64;
    const int tid = threadIdx.x, n = S.n_cur, wave = tid >> 6, lane = tid & 63;
    __shared__ int s_tot[2][NW], s_base[2];
    uint8_t* const vg = S.vg;
    uint8_t* const vp = S.vp;
    int* const ids = S.ids;
    if (tid == 0) { s_base[0] = 0; s_base[1] = 0; }
    __syncthreads();
    for (int c0 = 0; c0 < n || c0 == 0; c0 += NT * EPT) {  // one pass for up to 4096 tracks
        const int per = min(EPT, (min(n - c0, NT * EPT) + NT - 1) / NT);
        const int b = c0 + tid * per, e = min(n, b + per);
        int id[EPT];
        float px[EPT], py[EPT];
        unsigned fv = 0, fp = 0;  // bit k: track b + k survives / is a pose track
#pragma unroll
        for (int k = 0; k < EPT; k++) {
            const int i = b + k;
            if (k < per && i < e) {
                id[k] = ids[i];
                px[k] = S.p_all[2 * i]; py[k] = S.p_all[2 * i + 1];
                fv |= (S.v[i] != 0 ? 1u : 0u) << k;
            }
        }
#pragma unroll
        for (int k = 0; k < EPT; k++)
            if (k < per && b + k < e) {
                const bool f = (fv >> k) & 1u;
                const bool pv = f && vp[id[k]] != 0;
                vg[id[k]] = f ? 1 : 0;
                vp[id[k]] = pv ? 1 : 0;
                fp |= (pv ? 1u : 0u) << k;
            }
        const int cv = __popc(fv), cp = __popc(fp);
        // block-wide exclusive scan of (cv, cp): wave scan by shuffles, wave totals through LDS
        int sv = cv, sp = cp;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int tv = __shfl_up(sv, o, 64), tp = __shfl_up(sp, o, 64);
            if (lane >= o) { sv += tv; sp += tp; }
        }
        if (lane == 63) { s_tot[0][wave] = sv; s_tot[1][wave] = sp; }
        __syncthreads();  // also: every thread has LOADED its tracks before anybody overwrites ids / p_cur below
        int ov = s_base[0] + sv - cv, op = s_base[1] + sp - cp;
        for (int w = 0; w < wave; w++) { ov += s_tot[0][w]; op += s_tot[1][w]; }
#pragma unroll
        for (int k = 0; k < EPT; k++)
            if (k < per && ((fv >> k) & 1u)) {
                ids[ov] = id[k];
                S.p_cur[2 * ov] = px[k]; S.p_cur[2 * ov + 1] = py[k];
                if ((fp >> k) & 1u) { S.sel_p[op] = ov; S.sel_pw[op] = id[k]; op++; }
                ov++;
            }
        __syncthreads();
        if (tid == 0) {
            for (int w = 0; w < NW; w++) { s_base[0] += s_tot[0][w]; s_base[1] += s_tot[1][w]; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        S.n_cur = s_base[0];
        S.n_pose = s_base[1];
    }
}

// results records B, S and history P (vidExample.py:142-146, 151-153, 164); then advance the frame state
template <int NT>
__device__ __forceinline__ void sess_book_b(SessStream& S, const uint8_t* const* frames, float time_s, float frame_no, const float* times,
                                            const float* frame_nos)
{
    if (times) time_s = times[blockIdx.x];          // independent videos: per-stream timestamp (B[i,12] = CAP_PROP_POS_MSEC / 1000)
    if (frame_nos) frame_no = frame_nos[blockIdx.x];
    const int tid = threadIdx.x, i = S.frame_i + 1, nh = S.nhist, N0 = S.N0;
    if (i < nh) {
        for (int k = tid; k < S.n_cur; k += NT) {
            const int g = S.ids[k];
            S.P[sess_P(0, g, i, N0)] = S.p_cur[2 * k];
            S.P[sess_P(1, g, i, N0)] = S.p_cur[2 * k + 1];
            S.P[sess_P(4, g, i, N0)] = (float)i;
        }
        for (int j = tid; j < S.n_pose; j += NT) {
            const int g = S.sel_pw[j];
            S.P[sess_P(2, g, i, N0)] = (float)S.p_proj[2 * j];
            S.P[sess_P(3, g, i, N0)] = (float)S.p_proj[2 * j + 1];
        }
    }
    if (tid == 0) {
        if (i < nh) {
            float* B = S.B;
            B[14 * i + 12] = time_s;
            B[14 * i + 13] = frame_no;
            const float dt = __fsub_rn(B[14 * i + 12], B[14 * (i - 1) + 12]);
            // dr = norm(t + B[0,0:3] - B[i-1,0:3]) in float32 (vidExample.py:143)
            float ss = 0.f;
            for (int c = 0; c < 3; c++) {
                const float d = __fsub_rn(__fadd_rn(S.t[c], B[c]), B[14 * (i - 1) + c]);
                ss = __fadd_rn(ss, __fmul_rn(d, d));
            }
            const float dr = vh_sqrtf(ss);
            S.r_total = __fadd_rn(S.r_total, dr);
            for (int c = 0; c < 3; c++) {
                B[14 * i + 3 + c] = S.t[c];
                B[14 * i + c] = __fadd_rn(B[c], S.t[c]);
            }
            float* R = S.S + 9 * i;
            R[0] = (float)i; R[1] = 0.f; R[2] = (float)S.n_cur; R[3] = (float)S.res; R[4] = dt;
            R[5] = __fsub_rn(B[14 * i + 12], S.t0); R[6] = dr; R[7] = S.r_total;
            R[8] = __fmul_rn(__fdiv_rn(dr, dt), 3.6f);
        }
        S.im0 = frames[blockIdx.x];
        S.pp ^= 1;
        S.frame_i = i;
    }
}

// A stream whose frame pointer is NULL sits the step out (vh_session_step_some): its workgroup leaves before it has read or written anything, so
// frame_i, pp, im0, the counts, the pose and the records stay exactly what they were.
__global__ __launch_bounds__(256) void k_sess_book_a(SessStream* ss_all, const uint8_t* const* frames)
{
    if (frames[blockIdx.x] == nullptr) return;
    sess_book_a<256>(ss_all[blockIdx.x]);
}
__global__ __launch_bounds__(256) void k_sess_book_b(SessStream* ss_all, const uint8_t* const* frames, float time_s, float frame_no,
                                                     const float* times, const float* frame_nos)
{
    if (frames[blockIdx.x] == nullptr) return;
    sess_book_b<256>(ss_all[blockIdx.x], frames, time_s, frame_no, times, frame_nos);
}

// The whole post-tracking part of a frame in ONE launch (N0 <= 4096): vg[vg] = v, vp &= vg, compaction and pose-track selection
// (vidExample.py:135-139), estimateWorldCameraPose(findR=False) with every LM iteration (NLS.py:9-33,102-129), then the B / S / P records
// (vidExample.py:142-153,164).  Three dependent launches of one workgroup each before; same code, same results.
// 512 threads: the two bookkeeping halves are chains of dependent memory round trips and the LM loop a chain of dependent float64 operations, so two
// wavefronts per SIMD hide what one cannot: 67 -> 56 us at 256 streams (the stand-alone pose kernel gains nothing from it: 2.75 vs 3.05 us per iteration)
#define SESS_NT 512
__global__ __launch_bounds__(SESS_NT) void k_sess_frame(SessStream* ss_all, const uint8_t* const* frames, float time_s, float frame_no,
                                                        const float* times, const float* frame_nos)
{
    if (frames[blockIdx.x] == nullptr) return;  // an idle stream (see k_sess_book_a)
    SessStream& S = ss_all[blockIdx.x];
    sess_book_a<SESS_NT>(S);
    __threadfence_block();
    __syncthreads();
    const PoseJob J = S.pose;
    pose_solve<0, SESS_NT>(J);
    __threadfence_block();
    __syncthreads();
    sess_book_b<SESS_NT>(S, frames, time_s, frame_no, times, frame_nos);
}

// p3[vg] = p3hat - t ; vp = vg   (vidExample.py:159-160)
__global__ __launch_bounds__(256) void k_sess_after_msv(SessStream* ss_all, const uint8_t* const* frames, int msv_frame)
{
    if (frames[blockIdx.x] == nullptr) return;  // an idle stream parked at its MSV frame was re-triangulated when it got there
    SessStream& S = ss_all[blockIdx.x];
    if (S.frame_i != msv_frame) return;  // only the streams whose own frame counter is at the MSV frame
    for (int k = threadIdx.x; k < S.n_cur; k += 256) {
        const int g = S.ids[k];
        for (int c = 0; c < 3; c++) S.p3[3 * g + c] = S.msv_b0[3 * k + c] - (double)S.t[c];
    }
    for (int g = threadIdx.x; g < S.N0; g += 256) S.vp[g] = S.vg[g];
}

// what the host needs to decide whether a stream's recovery runs, and to run it: after KLTmain, before the bookkeeping (p_cur, n_cur and im0 are still the
// previous frame's)
__global__ void k_sess_fb_gather(const SessStream* ss_all, const uint8_t* const* frames, SessFbRec* rec, int batch)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const SessStream& S = ss_all[b];
    // an idle stream still carries the flag word of its last active step: it reports no failure, and its recovery counters do not move
    rec[b] = SessFbRec{frames[b] ? S.klt_flags : 0, S.n_cur, S.im0, frames[b]};
}
__global__ void k_sess_fb_flags(SessStream* S, int bits)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) S->klt_flags |= bits;
}

// frame-0 initialisation (vidExample.py:125-131, 151-153)
// t0_dev / res0_dev / n_dev (all may be null): plate pose, its residual and the number of frame-0 tracks taken from DEVICE memory -- the outputs of
// vh_frame0_init -- instead of the by-value arguments; with n_dev < N0 the tail rows are tracks that never existed (vg 0, history NaN)
__global__ __launch_bounds__(256) void k_sess_init(SessStream* ss, const float* p, const double* p3, const uint8_t* vp, const uint8_t* frame0,
                                                   float t0x, float t0y, float t0z, float time0, float frame_no, float res0, const float* t0_dev,
                                                   const double* res0_dev, const int* n_dev, int stride)
{
    SessStream& S = *ss;
    const int tid = threadIdx.x, N0 = S.N0, nh = S.nhist;
    const int n = n_dev ? min(max(*n_dev, 0), N0) : N0;
    if (t0_dev) { t0x = t0_dev[0]; t0y = t0_dev[1]; t0z = t0_dev[2]; }
    if (res0_dev) res0 = (float)*res0_dev;
    const float nanv = __int_as_float(0x7fc00000);
    for (size_t q = tid; q < (size_t)5 * N0 * nh; q += 256) S.P[q] = nanv;
    for (int q = tid; q < nh * 14; q += 256) S.B[q] = 0.f;
    for (int q = tid; q < nh * 9; q += 256) S.S[q] = 0.f;
    __syncthreads();
    for (int g = n + tid; g < N0; g += 256) { S.vg[g] = 0; S.vp[g] = 0; }
    for (int g = tid; g < n; g += 256) {
        S.vg[g] = 1;
        S.vp[g] = vp[g] ? 1 : 0;
        S.ids[g] = g;
        S.p_cur[2 * g] = p[2 * g]; S.p_cur[2 * g + 1] = p[2 * g + 1];
        for (int c = 0; c < 3; c++) S.p3[3 * g + c] = p3[3 * g + c];
        S.P[sess_P(0, g, 0, N0)] = p[2 * g];
        S.P[sess_P(1, g, 0, N0)] = p[2 * g + 1];
        if (vp[g]) { S.P[sess_P(2, g, 0, N0)] = p[2 * g]; S.P[sess_P(3, g, 0, N0)] = p[2 * g + 1]; }  // p_ = p[vp]
        S.P[sess_P(4, g, 0, N0)] = 0.f;
    }
    if (tid == 0) {
        S.n_cur = n; S.n_pose = 0; S.frame_i = 0; S.pp = 0; S.klt_flags = 0; S.small_ready = 0;
        S.B[0] = t0x; S.B[1] = t0y; S.B[2] = t0z; S.B[12] = time0; S.B[13] = frame_no;
        S.t[0] = t0x; S.t[1] = t0y; S.t[2] = t0z;
        S.t0 = time0; S.r_total = 0.f; S.res = res0_dev ? *res0_dev : (double)res0;
        S.S[0] = 0.f; S.S[2] = (float)n; S.S[3] = res0; S.S[4] = nanv; S.S[8] = nanv;
        S.im0 = frame0;
        S.stride = stride;  // rows of this slot's frames (frame 0 and every later one)
    }
}

// ---- replenishment ------------------------------------------------------------------------------------------------------------------------------
// All four kernels are one workgroup per stream and latency-bound (a few hundred tracks, a chain of dependent loads); a workgroup whose stream is idle,
// not due or in need of nothing leaves at once, so a step never has to know on the host which streams act.
__host__ __device__ __forceinline__ bool repl_birth_due(int f, int msv_frame, int every, int baseline, int nhist)
{
    const int m0 = msv_frame > 0 ? msv_frame : 0;
    return f > m0 && (f - m0) % every == 0 && f + baseline < nhist;
}

// rows of a slot that has just been initialised (k_sess_init ran): the frame-0 tracks are born at 0 and triangulated, the tail rows are free
__global__ __launch_bounds__(256) void k_replenish_init(SessStream* ss, SessRepl* rp, int full)
{
    SessStream& S = *ss;
    SessRepl& R = *rp;
    const int N0 = S.N0, n = full ? N0 : S.n_cur;
    for (int g = threadIdx.x; g < N0; g += 256) {
        R.born[g] = g < n ? 0 : -1;
        R.tri[g] = g < n ? 1 : 0;
        if (g >= n && !full) { S.p3[3 * g] = 0.0; S.p3[3 * g + 1] = 0.0; S.p3[3 * g + 2] = 0.0; }  // (a slot's earlier clip may have left points there)
    }
    if (threadIdx.x == 0) { R.n_rows = n; R.n_new = 0; R.due = 0; R.cnt[0] = R.cnt[1] = R.cnt[2] = 0; }
}

// THE triangulation of one track from nf of its own observations, and its gate (one copy: a newborn row's promotion over its baseline, the start of an
// untrusted track of a partial refinement window over one frame pair).  A, T: [nf][3] ray origins and translations of the frames; pix(j, row): the
// track's float32 pixel of frame j; rays by the slot's float32-rays rule, the point c by fcn2vintercept.  True iff c is finite, lies in front of every
// camera and reprojects within max_reproj pixels in each frame.
template <class Pix>
__device__ __forceinline__ bool sess_triangulate(const double* A, const double* T, int nf, const double* K, int f32, Pix pix, double max_reproj, double* c)
{
    two_view_rays(A, nf, [&](int j, double* u) {
        if (f32) uvec_f32(pix(j, 0), pix(j, 1), (float)K[6], (float)K[7], (float)K[0], u);
        else uvec_f64((double)pix(j, 0), (double)pix(j, 1), K[6], K[7], K[0], u);
    }, c);
    bool ok = isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]);
    double worst = 0.0;
    for (int j = 0; j < nf && ok; j++) {
        const double b0 = c[0] + T[3 * j], b1 = c[1] + T[3 * j + 1], b2 = c[2] + T[3 * j + 2];
        ok = b2 > 0.0;
        double u, v;
        project_cam(K, b0, b1, b2, u, v);
        const double du = u - (double)pix(j, 0), dv = v - (double)pix(j, 1);
        const double e = sqrt(du * du + dv * dv);
        ok = ok && isfinite(e);
        worst = fmax(worst, e);
    }
    return ok && worst < max_reproj;
}

// Promotion: one thread per candidate row.  Rays as fcnMSV1_t builds them, origins float32(B[0, 0:3] - B[born + j, 0:3]) widened (MSV.py:18), the point
// by fcn2vintercept; the gate: finite, in front of every camera of the baseline, reprojected within max_reproj pixels in each of its frames.
__global__ __launch_bounds__(256) void k_replenish_promote(SessStream* ss_all, SessRepl* rp_all, const uint8_t* const* frames, int msv_frame, int every,
                                                           int baseline, double max_reproj)
{
    if (frames[blockIdx.x] == nullptr) return;
    SessStream& S = ss_all[blockIdx.x];
    SessRepl& R = rp_all[blockIdx.x];
    const int f = S.frame_i, born = f - baseline, N0 = S.N0, nf = baseline + 1, tid = threadIdx.x;
    if (f >= S.nhist || !repl_birth_due(born, msv_frame, every, baseline, S.nhist)) return;  // no birth ran `baseline` frames ago
    __shared__ double s_A[3 * (SESS_RP_MAXBASE + 1)], s_T[3 * (SESS_RP_MAXBASE + 1)];
    if (tid < nf)
        for (int c = 0; c < 3; c++) {
            s_A[3 * tid + c] = (double)__fsub_rn(S.B[c], S.B[14 * (born + tid) + c]);
            s_T[3 * tid + c] = (double)S.B[14 * (born + tid) + 3 + c];
        }
    __syncthreads();
    double K[9];
    for (int k = 0; k < 9; k++) K[k] = S.K[k];
    const int f32 = S.msv.f32_rays, n_rows = R.n_rows;
    int good = 0, bad = 0;
    for (int g = tid; g < n_rows; g += 256) {
        if (!S.vg[g] || R.tri[g] || R.born[g] != born) continue;
        auto pix = [&](int j, int row) { return S.P[sess_P(row, g, born + j, N0)]; };
        double c[3];
        if (sess_triangulate(s_A, s_T, nf, K, f32, pix, max_reproj, c)) {
            S.p3[3 * g] = c[0]; S.p3[3 * g + 1] = c[1]; S.p3[3 * g + 2] = c[2];
            R.tri[g] = 1;
            S.vp[g] = 1;
            good++;
        } else {
            bad++;
        }
    }
    if (good) atomicAdd(&R.cnt[1], good);
    if (bad) atomicAdd(&R.cnt[2], bad);
}

// Birth, part 1: per stream of the chunk, the bounding rectangle of the live tracks (boundingRect, images.py:9-19), the exclusion mask and the stream's
// detector descriptor -- written HERE, on the device, so that no step reads a ROI back.  A stream with nothing to do gets empty extents: every detector
// tile of it leaves at once and its corner count comes out 0.
struct ReplSetup {
    F0Clip* tab;
    F0Cam* cam;
    unsigned* cnt;
    uint8_t* mask;
    float* rows;
    size_t plane;
    int cap, c0;
};
__global__ __launch_bounds__(256) void k_replenish_setup(SessStream* ss_all, SessRepl* rp_all, const uint8_t* const* frames, ReplSetup Q, int msv_frame,
                                                         vh_replenish_params P)
{
    const int clip = blockIdx.x, b = Q.c0 + clip, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    SessStream& S = ss_all[b];
    SessRepl& R = rp_all[b];
    __shared__ float s_box[4][4];
    __shared__ int s_roi[4];
    const int n = S.n_cur, target = P.target > 0 ? P.target : (int)S.S[2];
    bool go = frames[b] != nullptr && repl_birth_due(S.frame_i, msv_frame, P.every, P.baseline, S.nhist) && n > 0 && n < target && R.n_rows < S.N0;
    uint8_t* mask = Q.mask + (size_t)clip * Q.plane;
    if (go) {  // (uniform over the workgroup)
        float mnx = 3.0e38f, mny = 3.0e38f, mxx = -3.0e38f, mxy = -3.0e38f;
        for (int i = tid; i < n; i += 256) {
            const float x = S.p_cur[2 * i], y = S.p_cur[2 * i + 1];
            mnx = fminf(mnx, x); mxx = fmaxf(mxx, x); mny = fminf(mny, y); mxy = fmaxf(mxy, y);
        }
        for (int o = 32; o > 0; o >>= 1) {
            mnx = fminf(mnx, __shfl_xor(mnx, o, 64)); mny = fminf(mny, __shfl_xor(mny, o, 64));
            mxx = fmaxf(mxx, __shfl_xor(mxx, o, 64)); mxy = fmaxf(mxy, __shfl_xor(mxy, o, 64));
        }
        if (lane == 0) { s_box[wave][0] = mnx; s_box[wave][1] = mny; s_box[wave][2] = mxx; s_box[wave][3] = mxy; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; w++) {
                mnx = fminf(mnx, s_box[w][0]); mny = fminf(mny, s_box[w][1]); mxx = fmaxf(mxx, s_box[w][2]); mxy = fmaxf(mxy, s_box[w][3]);
            }
            // (live tracks lie within a window of the frame: the clamps only keep the integer arithmetic below defined)
            mnx = fminf(fmaxf(mnx, -1.0e6f), 1.0e6f); mny = fminf(fmaxf(mny, -1.0e6f), 1.0e6f);
            mxx = fminf(fmaxf(mxx, -1.0e6f), 1.0e6f); mxy = fminf(fmaxf(mxy, -1.0e6f), 1.0e6f);
            int x0 = vh_floor(mnx), y0 = vh_floor(mny);
            const int bw = vh_floor(mxx) - x0 + 1, bh = vh_floor(mxy) - y0 + 1;
            int x1 = x0 + bw + P.border_x, y1 = y0 + bh + P.border_y;
            x0 -= P.border_x; y0 -= P.border_y;
            s_roi[0] = max(x0, 1); s_roi[1] = min(x1, S.w); s_roi[2] = max(y0, 1); s_roi[3] = min(y1, S.h);
        }
        __syncthreads();
    }
    const int x0 = go ? s_roi[0] : 0, y0 = go ? s_roi[2] : 0;
    const int rw = go ? s_roi[1] - x0 : 0, rh = go ? s_roi[3] - y0 : 0;
    go = go && rw >= 3 && rh >= 3 && rw >= P.block && rh >= P.block;
    if (go) {
        // the mask: 255, and 0 in the square abs(x - rint(px)) < min_distance, abs(y - rint(py)) < min_distance around every live track
        const size_t px = (size_t)rw * rh;  // (<= the plane: the ROI lies inside the slot's frame, which is at most the session's)
        for (size_t i = tid; i < px; i += 256) mask[i] = 255;
        __syncthreads();
        const int r = (int)ceil(P.min_distance) - 1;  // the integer offsets d with abs(d) < min_distance
        if (r >= 0)
            for (int i = wave; i < n; i += 4) {  // one wavefront per track, its lanes over the cells of the square
                const float fx = S.p_cur[2 * i], fy = S.p_cur[2 * i + 1];
                if (!(fabsf(fx) < 1.0e6f && fabsf(fy) < 1.0e6f)) continue;
                const int cx = (int)rintf(fx) - x0, cy = (int)rintf(fy) - y0;
                const int xa = max(cx - r, 0), xb = min(cx + r + 1, rw), ya = max(cy - r, 0), yb = min(cy + r + 1, rh);
                if (xa >= xb || ya >= yb) continue;
                const int cw = xb - xa, cells = cw * (yb - ya);
                for (int e = lane; e < cells; e += 64) {
                    const int yy = ya + e / cw, xx = xa + e % cw;
                    mask[(size_t)yy * rw + xx] = 0;
                }
            }
    }
    if (tid == 0) {
        F0Clip C;
        C.roi = go ? S.im0 + (size_t)y0 * S.stride + x0 : S.im0;
        C.im = S.im0;
        C.seg = (unsigned long long)clip * Q.plane;
        C.rw = go ? rw : 0; C.rh = go ? rh : 0;
        C.offx = (float)x0; C.offy = (float)y0;
        for (int k = 0; k < 4; k++) C.boxa[k] = 0;
        for (int k = 0; k < 8; k++) C.q[k] = 0.f;
        C.mask = mask; C.mstride = rw;
        C.stride = S.stride;
        C.out = Q.rows + ((size_t)clip * Q.cap + 4) * 2;
        C.n_out = &R.n_new;
        C.max_corners = P.max_new; C.pad_ = 0;
        Q.tab[clip] = C;
        F0Cam M;
        for (int k = 0; k < 9; k++) M.K[k] = S.K[k];
        M.w = S.w; M.h = S.h;
        Q.cam[clip] = M;
        for (int k = 0; k < 4; k++) Q.cnt[4 * clip + k] = 0;
        R.due = go ? 1 : 0;
        R.n_new = 0;
    }
}

// Birth, part 2: the first m = min(corners, target - n_cur, N0 - n_rows) refined corners enter as rows n_rows.. (the list is response-ordered, so a prefix
// equals a smaller budget): tracked, not yet used for the pose (vg = 1, vp = 0), history rows 0, 1, 4 of the frame.  S[f, 2] keeps the count from before.
__global__ __launch_bounds__(256) void k_replenish_append(SessStream* ss_all, SessRepl* rp_all, ReplSetup Q, vh_replenish_params P)
{
    const int clip = blockIdx.x, b = Q.c0 + clip, tid = threadIdx.x;
    SessRepl& R = rp_all[b];
    if (!R.due) return;
    SessStream& S = ss_all[b];
    const int N0 = S.N0, n = S.n_cur, n_rows = R.n_rows, f = S.frame_i, target = P.target > 0 ? P.target : (int)S.S[2];
    const int found = min((int)Q.cnt[4 * clip + 2], P.max_new);
    const int m = min(found, min(target - n, N0 - n_rows));
    const float* row = Q.rows + ((size_t)clip * Q.cap + 4) * 2;
    for (int k = tid; k < m; k += 256) {
        const int g = n_rows + k;
        const float x = row[2 * k], y = row[2 * k + 1];
        S.p_cur[2 * (n + k)] = x; S.p_cur[2 * (n + k) + 1] = y;
        S.ids[n + k] = g;
        S.vg[g] = 1; S.vp[g] = 0;
        R.tri[g] = 0; R.born[g] = f;
        S.P[sess_P(0, g, f, N0)] = x;
        S.P[sess_P(1, g, f, N0)] = y;
        S.P[sess_P(4, g, f, N0)] = (float)f;
    }
    __syncthreads();  // every thread has read n, n_rows and due
    if (tid == 0) {
        if (m > 0) { S.n_cur = n + m; R.n_rows = n_rows + m; R.cnt[0] += m; }
        R.due = 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
// the camera of one slot (vh_session_set_camera): frame size and intrinsics, in the three places the step reads K from
struct SessCamera {
    double K[9];
    int w, h, f32;
};
__global__ void k_sess_camera(SessStream* ss, SessCamera cam)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    SessStream& S = *ss;
    for (int k = 0; k < 9; k++) { S.K[k] = cam.K[k]; S.pose.K[k] = cam.K[k]; S.msv.K[k] = cam.K[k]; }
    S.msv.f32_rays = cam.f32;
    S.w = cam.w; S.h = cam.h; S.stride = cam.w;
}

// The device side of a session as ONE walk (sizes only when base is null): the pointer fields of the host mirror h_ss and of the session itself.
static size_t sess_carve(char* base, vh_session* s)
{
    VhCarver A(base);
    const size_t n0 = s->N0, nhist = s->nhist, small = (size_t)lrint(s->w * 0.25) * (size_t)lrint(s->h * 0.25);
    const size_t msv_rows = sess_msv_fires(s->msv_frame, s->nhist) ? s->msv_frame + 1 : 1;  // one row when fcnMSV1_t can never fire (a 'never' sentinel sizes nothing)
    s->d_ss = A.take<SessStream>(s->batch); s->d_ingest = A.take<IngestJob>(s->batch);
    for (int b = 0; b < s->batch; b++) {
        SessStream& S = s->h_ss[b];
        S.vg = A.take<uint8_t>(n0); S.vp = A.take<uint8_t>(n0);
        S.p_cur = A.take<float>(2 * n0); S.ids = A.take<int>(n0);
        S.p3 = A.take<double>(3 * n0); S.P = A.take<float>(5 * n0 * nhist);
        S.B = A.take<float>(14 * nhist); S.S = A.take<float>(9 * nhist);
        S.p_all = A.take<float>(2 * n0); S.v = A.take<uint8_t>(n0);
        S.sel_p = A.take<int>(n0); S.sel_pw = A.take<int>(n0);
        S.p_proj = A.take<double>(2 * n0);
        S.msv_U = A.take<double>(3 * msv_rows * n0); S.msv_b0 = A.take<double>(3 * n0);
        S.small[0] = A.take<uint8_t>(small); S.small[1] = A.take<uint8_t>(small);
    }
    s->d_anc_mask = A.take<uint8_t>(s->batch * n0);  // (zero = no anchors: the arena is cleared, and the clear is checked)
    s->d_anc_xyz = A.take<double>(3 * s->batch * n0);
    return A.bytes();
}

extern "C" VH_API int vh_session_create(vh_session** out, vh_ctx* ctx, int n0, int nhist, int w, int h, const double* K_host,
                                        int k_is_float32, const vh_lk_params* coarse, const vh_lk_params* fine, int msv_frame)
{
    if (!out || !ctx || !K_host || !coarse || !fine || n0 < 1 || nhist < 2) return vh_fail(-1, "vh_session_create: bad arguments");
    if (n0 > ctx->max_pts || w > ctx->max_w || h > ctx->max_h) return vh_fail(-1, "vh_session_create: exceeds the workspace");
    // a re-triangulation frame the session COULD reach (< nhist) but fcnMSV1_t cannot serve is an error, not a silently skipped step
    if (msv_frame >= 1 && msv_frame < nhist && msv_frame + 1 > 2048)
        return vh_fail(-1, "vh_session_create: msv_frame + 1 > 2048 frames (fcnMSV1_t keeps one ray table entry per frame of the history in LDS; the "
                           "reference has no such limit -- pass msv_frame <= 0 to run without the re-triangulation, or a frame below 2048)");
    vh_session* s = new (std::nothrow) vh_session();
    if (!s) return vh_fail(-1, "out of host memory");
    s->ctx = ctx; s->batch = ctx->batch; s->N0 = n0; s->nhist = nhist; s->w = w; s->h = h; s->msv_frame = msv_frame; s->k_is_f32 = k_is_float32 ? 1 : 0;
    s->coarse = *coarse; s->fine = *fine;
    s->h_ss = new SessStream[s->batch]();
    s->h_frame = new int[s->batch](); s->h_nanchor = new int[s->batch](); s->h_inited = new char[s->batch]();  // (from here on a failure goes through vh_session_destroy)
    const int r = s->arena.reserve(sess_carve(nullptr, s), nullptr, "session", "create the session before capturing", true);
    if (r) { vh_session_destroy(s); return r; }
    sess_carve(s->arena.p, s);
    for (int b = 0; b < s->batch; b++) {
        SessStream& S = s->h_ss[b];
        SessStream* d = s->d_ss + b;
        for (int k = 0; k < 9; k++) S.K[k] = K_host[k];
        S.N0 = n0; S.nhist = nhist; S.w = w; S.h = h; S.stride = w;
        PoseJob& J = S.pose;
        for (int k = 0; k < 9; k++) { J.K[k] = S.K[k]; J.R[k] = (k % 4 == 0) ? 1.0 : 0.0; }
        J.x0[0] = J.x0[1] = J.x0[2] = 0; J.x0[3] = 0; J.x0[4] = 0; J.x0[5] = 1;  // always restarted from t=[0,0,1] (NLS.py:9)
        J.p = S.p_cur; J.pw = S.p3; J.p_sel = S.sel_p; J.pw_sel = S.sel_pw; J.n_ptr = &d->n_pose; J.n = 0; J.mode = 0;
        J.t_out = d->t; J.R_out = nullptr; J.res_out = &d->res; J.p_proj = S.p_proj; J.info_out = d->pose_info;
        MsvJob& M = S.msv;
        memset(&M, 0, sizeof(M));
        for (int k = 0; k < 9; k++) M.K[k] = S.K[k];
        M.P = S.P; M.P_rs = (size_t)n0; M.P_ts = 1; M.P_fs = (size_t)5 * n0;  // the session's frame-major history
        M.B = S.B; M.ids = S.ids; M.ng_ptr = &d->n_cur; M.ng = 0; M.N0 = n0; M.nhist = nhist;
        M.nf = msv_frame + 1; M.max_iter = 1000; M.f32_rays = s->k_is_f32;  // P is float32 always; K as the caller holds it
        M.U = S.msv_U; M.b0 = S.msv_b0; M.x_out = d->msv_x; M.info_out = d->msv_info;
    }
    const hipError_t e = hipMemcpy(s->d_ss, s->h_ss, sizeof(SessStream) * s->batch, hipMemcpyHostToDevice);
    if (e != hipSuccess) { vh_set_error("hipMemcpy(session)", e, __FILE__, __LINE__); vh_session_destroy(s); return (int)e; }
    *out = s;
    return 0;
}

// The recovery's two blocks for `chunk` failed streams per matcher call and qcap query keypoints per pair: sizes only when the carvers have no base.
static void sess_fb_carve(VhCarver& H, VhCarver& D, SessFallback& F, int batch, int chunk, int qcap)
{
    F.h_rec = H.take<SessFbRec>(batch); F.h_M = H.take<double>(6 * (size_t)chunk); F.h_info = H.take<int>(4 * (size_t)chunk);
    F.d_rec = D.take<SessFbRec>(batch); F.d_M = D.take<double>(6 * (size_t)chunk); F.d_info = D.take<int>(4 * (size_t)chunk);
    F.d_inl = D.take<uint8_t>((size_t)qcap * chunk);
}

static void sess_fb_release(SessFallback& F)
{
    F.dev.release(); F.host.release();
    if (F.ctx) vh_ctx_destroy(F.ctx);
    delete[] F.counts;
    memset(&F, 0, sizeof(F));
}

extern "C" VH_API int vh_session_set_fallback(vh_session* s, int on, const vh_match_params* params_host)
{
    if (!s) return vh_fail(-1, "vh_session_set_fallback: bad arguments");
    SessFallback& F = s->fb;
    if (!on) { F.on = 0; return 0; }
    if (s->w < 4 || s->h < 4) return vh_fail(-1, "vh_session_set_fallback: the recovery needs frames of at least 4 x 4");
    const int chunk = s->batch < SESS_FB_CHUNK ? s->batch : SESS_FB_CHUNK;
    // the matcher checks its parameters itself (-1, nothing created); its defaults come back through a context that exists, so the first reserve is
    // on a context sized for the defaults' query budget and repeated if the parameters ask for more
    vh_match_params P = {5, 500, 1000, 5, 50, 50, 4, 5, 10, 0.01};  // (vh_match_affine's defaults, include/velocity_hip.h)
    if (params_host) P = *params_host;
    if (P.levels < 1 || P.levels > 8 || P.query_per_level < 1 || P.query_per_level > 2048) return vh_fail(-1, "vh_session_set_fallback: bad matcher parameters");
    const int qcap = P.levels * P.query_per_level, pts = s->N0 > qcap ? s->N0 : qcap;
    F.on = 0;  // off until everything below is there: a call that fails on the way leaves the recovery off and nothing half-made
    if (F.ctx && F.ctx->max_pts < pts) {  // a larger query budget than the context was made for
        VH_CHECK(hipDeviceSynchronize());
        vh_ctx_destroy(F.ctx);
        F.ctx = nullptr;
    }
    int r = 0;
    if (!F.ctx && (r = vh_ctx_create(&F.ctx, 1, s->w, s->h, pts))) return r;
    if ((r = vh_match_reserve_batch(F.ctx, chunk, s->w, s->h, &P, nullptr))) return r;
    if (!F.counts) F.counts = new int[2 * (size_t)s->batch]();
    VhCarver hs(nullptr), ds(nullptr);
    sess_fb_carve(hs, ds, F, s->batch, chunk, qcap);  // sizes; the pointers stay null unless both blocks are there (the recovery is off)
    if (F.dev.p && ds.bytes() > F.dev.bytes) VH_CHECK(hipDeviceSynchronize());
    static const char* const remedy = "call vh_session_set_fallback before capturing";
    if ((r = F.host.reserve(hs.bytes(), nullptr, "the recovery scratch", remedy)) || (r = F.dev.reserve(ds.bytes(), nullptr, "the recovery scratch", remedy))) return r;
    VhCarver hp(F.host.p), dp(F.dev.p);
    sess_fb_carve(hp, dp, F, s->batch, chunk, qcap);
    F.params = P; F.chunk = chunk; F.on = 1;
    return 0;
}

extern "C" VH_API int vh_session_recoveries(vh_session* s, int* counts_host)
{
    if (!s || !counts_host) return vh_fail(-1, "vh_session_recoveries: bad arguments");
    for (int k = 0; k < 2 * s->batch; k++) counts_host[k] = s->fb.counts ? s->fb.counts[k] : 0;
    return 0;
}

// KLT.py:126-133 for every stream whose coarse stage has just failed; queued between KLTmain and the bookkeeping of the step.  The matcher takes pairs of
// ONE frame size per call, so the failed streams are served in groups of equal (w, h, stride), each of at most `chunk` pairs, in slot order: a session of
// one camera makes exactly the calls it always made.
static int session_recover(vh_session* s, const uint8_t* const* frames_dev, hipStream_t st)
{
    SessFallback& F = s->fb;
    const int nb = s->batch;
    hipLaunchKernelGGL(k_sess_fb_gather, dim3((nb + 63) / 64), dim3(64), 0, st, s->d_ss, frames_dev, F.d_rec, nb);
    VH_CHECK(hipMemcpyAsync(F.h_rec, F.d_rec, sizeof(SessFbRec) * nb, hipMemcpyDeviceToHost, st));
    VH_CHECK(hipStreamSynchronize(st));  // the host read of the option: once per step
    std::vector<int> todo;
    for (int b = 0; b < nb; b++)
        if ((F.h_rec[b].flags & 1) && F.h_rec[b].n_cur > 0) todo.push_back(b);  // `fallback and n > 0` (an empty stream is left alone)
    std::vector<char> served(todo.size(), 0);
    for (size_t first = 0; first < todo.size(); first++) {
        if (served[first]) continue;
        const SessStream& H0 = s->h_ss[todo[first]];
        const int w = H0.w, h = H0.h, stride = H0.stride;
        int failed[SESS_FB_CHUNK], m = 0;
        for (size_t k = first; k < todo.size() && m < F.chunk; k++) {
            const SessStream& Hk = s->h_ss[todo[k]];
            if (served[k] || Hk.w != w || Hk.h != h || Hk.stride != stride) continue;
            served[k] = 1;
            failed[m++] = todo[k];
        }
        const uint8_t *im1[SESS_FB_CHUNK], *im2[SESS_FB_CHUNK];
        const float* p1[SESS_FB_CHUNK];
        int n[SESS_FB_CHUNK];
        for (int i = 0; i < m; i++) {
            const SessFbRec& R = F.h_rec[failed[i]];
            im1[i] = R.im0; im2[i] = R.im; p1[i] = s->h_ss[failed[i]].p_cur; n[i] = R.n_cur;
        }
        int r = vh_match_affine_batch(F.ctx, m, im1, im2, w, h, stride, stride, p1, n, &F.params, F.d_M, F.d_inl, nullptr, F.d_info, st);
        if (r) return r;
        VH_CHECK(hipMemcpyAsync(F.h_M, F.d_M, sizeof(double) * 6 * m, hipMemcpyDeviceToHost, st));
        VH_CHECK(hipMemcpyAsync(F.h_info, F.d_info, sizeof(int) * 4 * m, hipMemcpyDeviceToHost, st));
        VH_CHECK(hipStreamSynchronize(st));  // (failing steps only)
        for (int i = 0; i < m; i++) {
            const int b2 = failed[i];
            const SessStream& H = s->h_ss[b2];
            int bits = 2;
            F.counts[2 * b2]++;
            if (F.h_info[4 * i] > 0) {
                bits |= 4;
                F.counts[2 * b2 + 1]++;
                // KLTregional(im0, im, p0, T23.T, lk_fine, fbt=0.3): T = float32(T23.T), 3 x 2 row-major (KLT.py:58)
                const double* M = F.h_M + 6 * i;
                const float T[6] = {(float)M[0], (float)M[3], (float)M[1], (float)M[4], (float)M[2], (float)M[5]};
                r = vh_klt_regional(F.ctx, im1[i], im2[i], w, h, stride, stride, H.p_cur, n[i], T, &s->fine, 0.3f, 0, H.p_all, H.v, nullptr, st);
                if (r) return r;
            }
            hipLaunchKernelGGL(k_sess_fb_flags, dim3(1), dim3(64), 0, st, s->d_ss + b2, bits);
        }
    }
    SESS_CHECK();
    return 0;
}

// The replenishment's device block as one walk (sizes only when base is null): the per-stream state, then the scratch of one chunk of streams
static size_t sess_rp_carve(char* base, vh_session* s, int chunk, int max_new)
{
    VhCarver A(base);
    SessReplenish& R = s->rp;
    const size_t n0 = s->N0, plane = (size_t)s->w * (size_t)s->h;
    R.d_rp = A.take<SessRepl>(s->batch);
    for (int b = 0; b < s->batch; b++) {
        int* born = A.take<int>(n0);
        uint8_t* tri = A.take<uint8_t>(n0);
        if (base) { R.h_rp[b].born = born; R.h_rp[b].tri = tri; }
    }
    R.d_mask = A.take<uint8_t>((size_t)chunk * plane);
    R.d_rows = A.take<float>((size_t)chunk * (size_t)(max_new + 4) * 2);
    return A.bytes();
}

extern "C" VH_API int vh_session_set_replenish(vh_session* s, const vh_replenish_params* params_host, void* stream)
{
    if (!s) return vh_fail(-1, "vh_session_set_replenish: null session");
    SessReplenish& R = s->rp;
    if (!params_host) { R.on = 0; return 0; }
    const vh_replenish_params P = *params_host;
    char msg[240];
    if (P.every < 1 || P.baseline < 1 || P.baseline > SESS_RP_MAXBASE) {
        snprintf(msg, sizeof(msg), "vh_session_set_replenish: every = %d, baseline = %d: every >= 1 and 1 <= baseline <= %d", P.every, P.baseline, SESS_RP_MAXBASE);
        return vh_fail(-1, msg);
    }
    if (P.max_new < 1 || P.max_new > 2048) {
        snprintf(msg, sizeof(msg), "vh_session_set_replenish: max_new = %d: 1 .. 2048 corners per birth", P.max_new);
        return vh_fail(-1, msg);
    }
    if (!std::isfinite(P.min_distance) || !std::isfinite(P.max_reproj) || !std::isfinite(P.quality) || !std::isfinite(P.harris_k) || P.border_x < 0 || P.border_y < 0 ||
        P.block < 1 || P.block > 15 || P.subpix_win < 1 || P.subpix_win > 7)
        return vh_fail(-1, "vh_session_set_replenish: bad parameters (finite distances and thresholds, border >= 0, block 1 .. 15, subpix_win 1 .. 7)");
    if (s->w < 3 || s->h < 3 || (P.min_distance >= 1 && (s->w > 32767 || s->h > 32767)))
        return vh_fail(-1, "vh_session_set_replenish: frames of 3 x 3 up to 32767 x 32767");
    static const char* const remedy = "call vh_session_set_replenish before capturing";
    VH_BIND(s->ctx, stream);
    hipStream_t st = bound_.s;
    R.on = 0;  // off until everything below is there
    const int chunk = s->batch < SESS_RP_CHUNK ? s->batch : SESS_RP_CHUNK;
    int r = vh_roi_detect_reserve(s->ctx, chunk, s->w, s->h, st, remedy);
    if (r) return r;
    if (!R.h_rp) R.h_rp = new SessRepl[s->batch]();
    const size_t need = sess_rp_carve(nullptr, s, chunk, P.max_new);
    const bool fresh = need > R.dev.bytes;  // (a block that grows is a new block: the slots' rows start over as full)
    if ((r = R.dev.reserve(need, st, "the replenishment's state and scratch", remedy, true))) return r;
    sess_rp_carve(R.dev.p, s, chunk, P.max_new);
    if (fresh) {
        VH_CHECK(hipMemcpyAsync(R.d_rp, R.h_rp, sizeof(SessRepl) * s->batch, hipMemcpyHostToDevice, st));
        VH_CHECK(hipStreamSynchronize(st));  // (h_rp is pageable: the copy has left it)
        // a slot initialised before the option was on counts as full until its next initialisation
        for (int b = 0; b < s->batch; b++) hipLaunchKernelGGL(k_replenish_init, dim3(1), dim3(256), 0, st, s->d_ss + b, R.d_rp + b, 1);
        SESS_CHECK();
    }
    R.P = P; R.chunk = chunk; R.on = 1;
    return 0;
}

extern "C" VH_API int vh_session_replenish_state(vh_session* s, int slot, int* born_host, uint8_t* tri_host, int* counts_host)
{
    if (!s || slot < 0 || slot >= s->batch) return vh_fail(-1, "vh_session_replenish_state: bad arguments");
    const SessReplenish& R = s->rp;
    if (!R.dev.p) return vh_fail(-1, "vh_session_replenish_state: the option was never on (vh_session_set_replenish)");
    SessRepl rec;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&rec, R.d_rp + slot, sizeof(rec), hipMemcpyDeviceToHost);
    if (e == hipSuccess && born_host) e = hipMemcpy(born_host, R.h_rp[slot].born, sizeof(int) * (size_t)s->N0, hipMemcpyDeviceToHost);
    if (e == hipSuccess && tri_host) e = hipMemcpy(tri_host, R.h_rp[slot].tri, (size_t)s->N0, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { vh_set_error("vh_session_replenish_state: reading the state back", e, __FILE__, __LINE__); return (int)e; }
    if (counts_host) { counts_host[0] = rec.n_rows; counts_host[1] = rec.cnt[0]; counts_host[2] = rec.cnt[1]; counts_host[3] = rec.cnt[2]; }
    return 0;
}

// The replenishment of one step, behind the bookkeeping and fcnMSV1_t: promotions, then births.  The host knows from its frame counters whether ANY
// stream is due, the way it knows the MSV frame; which streams act is decided on the device.
static int session_replenish(vh_session* s, const uint8_t* const* frames_dev, const uint8_t* active, hipStream_t st)
{
    SessReplenish& R = s->rp;
    const vh_replenish_params& P = R.P;
    const int nb = s->batch;
    bool promote = false, birth = false;
    for (int b = 0; b < nb; b++) {
        if (active && !active[b]) continue;
        const int f = s->h_frame[b];
        promote = promote || (f < s->nhist && repl_birth_due(f - P.baseline, s->msv_frame, P.every, P.baseline, s->nhist));
        birth = birth || repl_birth_due(f, s->msv_frame, P.every, P.baseline, s->nhist);
    }
    if (promote)
        hipLaunchKernelGGL(k_replenish_promote, dim3(nb), dim3(256), 0, st, s->d_ss, R.d_rp, frames_dev, s->msv_frame, P.every, P.baseline, P.max_reproj);
    if (birth) {
        VhRoiScratch D;
        int r = vh_roi_detect_scratch(s->ctx, R.chunk, s->w, s->h, &D);
        if (r) return r;
        const VhRoiDetect det = {P.max_new, P.block, P.use_harris ? 1 : 0, P.quality, P.harris_k, P.min_distance, P.subpix_win, P.subpix_iter, P.subpix_eps};
        for (int c0 = 0; c0 < nb; c0 += R.chunk) {
            const int n = nb - c0 < R.chunk ? nb - c0 : R.chunk;
            const ReplSetup Q = {D.tab, D.cam, D.cnt, R.d_mask, R.d_rows, D.plane, P.max_new + 4, c0};
            hipLaunchKernelGGL(k_replenish_setup, dim3(n), dim3(256), 0, st, s->d_ss, R.d_rp, frames_dev, Q, s->msv_frame, P);
            if ((r = vh_roi_detect_run(s->ctx, n, s->w, s->h, det, R.d_rows, P.max_new + 4, st))) return r;
            hipLaunchKernelGGL(k_replenish_append, dim3(n), dim3(256), 0, st, s->d_ss, R.d_rp, Q, P);
        }
    }
    SESS_CHECK();
    return 0;
}

extern "C" VH_API void vh_session_destroy(vh_session* s)
{
    if (!s) return;
    (void)hipDeviceSynchronize();
    sess_fb_release(s->fb);
    s->rp.dev.release();
    delete[] s->rp.h_rp;
    s->arena.release();
    delete[] s->h_ss;
    delete[] s->h_frame;
    delete[] s->h_nanchor;
    delete[] s->h_inited;
    delete s;
}

extern "C" VH_API int vh_session_set_camera(vh_session* s, int slot, int w, int h, const double* K_host, int k_is_float32, void* stream)
{
    char msg[200];
    if (!s) return vh_fail(-1, "vh_session_set_camera: null session");
    if (slot < 0 || slot >= s->batch) {
        snprintf(msg, sizeof(msg), "vh_session_set_camera: slot %d is outside the session's %d slots", slot, s->batch);
        return vh_fail(-1, msg);
    }
    if (!K_host) {
        snprintf(msg, sizeof(msg), "vh_session_set_camera: slot %d: null K_host", slot);
        return vh_fail(-1, msg);
    }
    if (w < 4 || h < 4 || w > s->w || h > s->h) {
        snprintf(msg, sizeof(msg), "vh_session_set_camera: slot %d: a %d x %d frame is outside what the session holds (4 x 4 up to %d x %d, each side)", slot, w,
                 h, s->w, s->h);
        return vh_fail(-1, msg);
    }
    VH_BIND(s->ctx, stream);
    SessCamera cam;
    for (int k = 0; k < 9; k++) cam.K[k] = K_host[k];
    cam.w = w; cam.h = h; cam.f32 = k_is_float32 ? 1 : 0;
    hipLaunchKernelGGL(k_sess_camera, dim3(1), dim3(64), 0, bound_.s, s->d_ss + slot, cam);
    SESS_CHECK();
    SessStream& H = s->h_ss[slot];  // the host mirror: what the argument checks and the recovery branch read
    for (int k = 0; k < 9; k++) { H.K[k] = cam.K[k]; H.pose.K[k] = cam.K[k]; H.msv.K[k] = cam.K[k]; }
    H.msv.f32_rays = cam.f32;
    H.w = w; H.h = h; H.stride = w;
    return 0;
}

static int session_init(vh_session* s, int slot, const uint8_t* frame0, int stride, const float* p, const double* p3, const uint8_t* vp,
                        const float* t0_host, float time0, float frame_no, float res0, const float* t0_dev, const double* res0_dev, const int* n_dev,
                        void* stream)
{
    SessStream& H = s->h_ss[slot];
    if (stride < H.w) {
        char msg[160];
        snprintf(msg, sizeof(msg), "vh_session_init: slot %d: row stride %d is below the slot's frame width %d", slot, stride, H.w);
        return vh_fail(-1, msg);
    }
    VH_BIND(s->ctx, stream);
    hipStream_t st = bound_.s;
    hipLaunchKernelGGL(k_sess_init, dim3(1), dim3(256), 0, st, s->d_ss + slot, p, p3, vp, frame0, t0_host ? t0_host[0] : 0.f, t0_host ? t0_host[1] : 0.f,
                       t0_host ? t0_host[2] : 0.f, time0, frame_no, res0, t0_dev, res0_dev, n_dev, stride);
    // quarter-scale copy of frame 0 = im0_small of the first step (pp starts at 0 -> previous index 1)
    int r = vh_resize_quarter(s->ctx, frame0, H.w, H.h, stride, H.small[1], stream);
    H.stride = stride;
    if (r) return r;
    s->h_frame[slot] = 0;  // a (re-)initialised slot starts a new clip: its MSV frame counts from here
    s->h_inited[slot] = 1;
    if (s->h_nanchor[slot] > 0) {  // ... and a new clip is a new plate (a slot that had no anchors queues nothing here)
        s->h_nanchor[slot] = 0;
        VH_CHECK(hipMemsetAsync(s->d_anc_mask + (size_t)slot * s->N0, 0, (size_t)s->N0, st));
    }
    if (s->fb.counts) s->fb.counts[2 * slot] = s->fb.counts[2 * slot + 1] = 0;
    if (s->rp.on) hipLaunchKernelGGL(k_replenish_init, dim3(1), dim3(256), 0, st, s->d_ss + slot, s->rp.d_rp + slot, 0);  // a new clip: its spare rows are free again
    SESS_CHECK();
    return 0;
}

extern "C" VH_API int vh_session_init(vh_session* s, int slot, const uint8_t* frame0, int stride, const float* p, const double* p3,
                                      const uint8_t* vp, const float* t0_host, float time0, float frame_no, float res0, void* stream)
{
    if (!s || slot < 0 || slot >= s->batch || !t0_host) return vh_fail(-1, "vh_session_init: bad arguments");
    return session_init(s, slot, frame0, stride, p, p3, vp, t0_host, time0, frame_no, res0, nullptr, nullptr, nullptr, stream);
}

extern "C" VH_API int vh_session_init_dev(vh_session* s, int slot, const uint8_t* frame0, int stride, const float* p, const double* p3,
                                          const uint8_t* vp, const float* t0_dev, const double* res0_dev, const int* n_dev, float time0,
                                          float frame_no, void* stream)
{
    if (!s || slot < 0 || slot >= s->batch || !t0_dev || !res0_dev) return vh_fail(-1, "vh_session_init_dev: bad arguments");
    return session_init(s, slot, frame0, stride, p, p3, vp, nullptr, time0, frame_no, 0.f, t0_dev, res0_dev, n_dev, stream);
}

// active (host, may be null: every stream steps): the host's copy of "frames_dev[b] is not NULL", for the frame counters it mirrors
static int session_step(vh_session* s, const uint8_t* const* frames_dev, float time_s, float frame_no, const float* times_dev,
                        const float* frame_nos_dev, const uint8_t* active, void* stream)
{
    if (!s || !frames_dev) return vh_fail(-1, "vh_session_step: bad arguments");
    if (s->fb.on) {  // the recovery reads the failure flags on the host: not something a graph can replay
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
        if (cs != hipStreamCaptureStatusNone)
            return vh_fail(-6, "vh_session_step: a session with the recovery on (vh_session_set_fallback) waits for the stream in every step and cannot be "
                               "captured; turn the option off to capture");
    }
    VH_BIND(s->ctx, stream);
    hipStream_t st = bound_.s;
    vh_ctx* c = s->ctx;
    const int nb = s->batch;
    int r = vh_run_klt_main(c, 0, nb, st, s->coarse, s->fine, s->d_ss, frames_dev, s->N0);  // the set-up kernel also fetches this frame's KltIO from the session
    if (r) return r;
    if (s->fb.on && (r = session_recover(s, frames_dev, st))) return r;
    if (session_frame_plan(s->N0) == 1) {
        const int rec = vh_prof_start(s->ctx, st);
        hipLaunchKernelGGL(k_sess_frame, dim3(nb), dim3(SESS_NT), 0, st, s->d_ss, frames_dev, time_s, frame_no, times_dev, frame_nos_dev);
        vh_prof_stop(s->ctx, rec, VH_PROF_SESSION, st);
    } else {  // more pose tracks than 256 threads keep in registers: the 1024-thread pose kernel between the two bookkeeping halves
        hipLaunchKernelGGL(k_sess_book_a, dim3(nb), dim3(256), 0, st, s->d_ss, frames_dev);
        vh_launch_pose(&s->d_ss[0].pose, sizeof(SessStream), nb, 0, s->N0, st, reinterpret_cast<const void* const*>(frames_dev));
        hipLaunchKernelGGL(k_sess_book_b, dim3(nb), dim3(256), 0, st, s->d_ss, frames_dev, time_s, frame_no, times_dev, frame_nos_dev);
    }
    // fcnMSV1_t fires when a stream reaches ITS frame msv_frame (vidExample.py:155), whenever that stream was initialised
    const bool msv_ok = sess_msv_fires(s->msv_frame, s->nhist);
    bool any = false;
    for (int b = 0; b < nb; b++) {
        if (active && !active[b]) continue;  // an idle stream's clock stands still
        const int fi = ++s->h_frame[b];
        if (msv_ok && fi == s->msv_frame) any = true;
    }
    // ONE launch for every stream: a workgroup runs only when its stream stepped in this call and its own frame counter is at the MSV frame (k_msv1_tab)
    if (any) vh_launch_msv1_tab(&s->d_ss[0].msv, sizeof(SessStream), (ptrdiff_t)offsetof(SessStream, frame_i) - (ptrdiff_t)offsetof(SessStream, msv),
                                s->msv_frame, s->msv_frame + 1, nb, st, reinterpret_cast<const void* const*>(frames_dev));
    if (any) hipLaunchKernelGGL(k_sess_after_msv, dim3(nb), dim3(256), 0, st, s->d_ss, frames_dev, s->msv_frame);
    if (s->rp.on && (r = session_replenish(s, frames_dev, active, st))) return r;
    SESS_CHECK();
    return 0;
}

extern "C" VH_API int vh_session_step(vh_session* s, const uint8_t* const* frames_dev, float time_s, float frame_no, void* stream)
{
    return session_step(s, frames_dev, time_s, frame_no, nullptr, nullptr, nullptr, stream);
}

extern "C" VH_API int vh_session_step_v(vh_session* s, const uint8_t* const* frames_dev, const float* time_s_dev, const float* frame_no_dev,
                                        void* stream)
{
    if (!time_s_dev || !frame_no_dev) return vh_fail(-1, "vh_session_step_v: bad arguments");
    return session_step(s, frames_dev, 0.f, 0.f, time_s_dev, frame_no_dev, nullptr, stream);
}

extern "C" VH_API int vh_session_step_some(vh_session* s, const uint8_t* const* frames_dev, const uint8_t* active_host, const float* time_s_dev,
                                           const float* frame_no_dev, void* stream)
{
    if (!active_host || !time_s_dev || !frame_no_dev) return vh_fail(-1, "vh_session_step_some: bad arguments");
    return session_step(s, frames_dev, 0.f, 0.f, time_s_dev, frame_no_dev, active_host, stream);
}

// ---- one record per stream: everything a finished clip hands back, packed for ONE device-to-host copy -------------------------------------------------
// Layout (vh_session_record, byte offsets): a 48-byte header {n_cur, n_pose, frame_i, klt_flags, pose_info[2], t[3], pad, res}, then vg, vp, ids, p, p3,
// B, S and the history P in the REFERENCE's [5][N0][nhist] order; every array starts on a multiple of 8 bytes.
static void sess_record_layout(int N0, int nhist, vh_session_record* L)
{
    size_t off = 0;
    auto put = [&](size_t bytes) { const size_t o = off; off = vh_align_up(off + bytes, 8); return o; };
    L->n_cur = put(4 * sizeof(int)) + 0; L->n_pose = L->n_cur + 4; L->frame_i = L->n_cur + 8; L->klt_flags = L->n_cur + 12;
    L->pose_info = put(2 * sizeof(int));
    L->t = put(3 * sizeof(float));
    L->res = put(sizeof(double));
    L->vg = put((size_t)N0); L->vp = put((size_t)N0);
    L->ids = put(sizeof(int) * (size_t)N0);
    L->p = put(sizeof(float) * 2 * (size_t)N0);
    L->p3 = put(sizeof(double) * 3 * (size_t)N0);
    L->B = put(sizeof(float) * 14 * (size_t)nhist);
    L->S = put(sizeof(float) * 9 * (size_t)nhist);
    L->P = put(sizeof(float) * 5 * (size_t)N0 * (size_t)nhist);
    L->bytes = off;
    L->n0 = N0; L->nhist = nhist;
}

// One launch per record.  Workgroups [0, 5 * ceil(N0 / 64)) transpose the history, one tile of 64 tracks x 64 frames at a time through LDS: the read walks
// the tracks of one frame (the device's frame-major rows), the write walks the frames of one track (the reference's rows) -- both sides coalesced.  The
// workgroups behind them copy the flat arrays; the last one also writes the header.
#define SESS_EXP_TILE 64
#define SESS_EXP_FLAT 8
__global__ __launch_bounds__(256) void k_sess_export(const SessStream* ss, vh_session_record L, char* rec, int tiles)
{
    const SessStream& S = *ss;
    const int N0 = S.N0, nh = S.nhist, tid = threadIdx.x;
    if ((int)blockIdx.x < 5 * tiles) {
        __shared__ float tile[SESS_EXP_TILE][SESS_EXP_TILE + 1];
        const int row = blockIdx.x / tiles, g0 = (blockIdx.x - row * tiles) * SESS_EXP_TILE;
        float* out = reinterpret_cast<float*>(rec + L.P) + (size_t)row * N0 * nh;
        const int lx = tid & 63, ly = tid >> 6;
        for (int f0 = 0; f0 < nh; f0 += SESS_EXP_TILE) {
            for (int f = ly; f < SESS_EXP_TILE; f += 4)
                if (f0 + f < nh && g0 + lx < N0) tile[f][lx] = S.P[sess_P(row, g0 + lx, f0 + f, N0)];
            __syncthreads();
            const int fw = min(SESS_EXP_TILE, nh - f0);  // frames of this tile: consecutive threads walk them, then the next track (adjacent when fw == nhist)
            for (int e = tid; e < SESS_EXP_TILE * fw; e += 256) {
                const int g = e / fw, f = e - g * fw;
                if (g0 + g < N0) out[(size_t)(g0 + g) * nh + f0 + f] = tile[f][g];
            }
            __syncthreads();
        }
        return;
    }
    const int part = blockIdx.x - 5 * tiles, step = SESS_EXP_FLAT * 256, k0 = part * 256 + tid;
    uint8_t* vg = reinterpret_cast<uint8_t*>(rec + L.vg);
    uint8_t* vp = reinterpret_cast<uint8_t*>(rec + L.vp);
    int* ids = reinterpret_cast<int*>(rec + L.ids);
    float* p = reinterpret_cast<float*>(rec + L.p);
    double* p3 = reinterpret_cast<double*>(rec + L.p3);
    float* B = reinterpret_cast<float*>(rec + L.B);
    float* R = reinterpret_cast<float*>(rec + L.S);
    const int n = S.n_cur;
    for (int k = k0; k < N0; k += step) { vg[k] = S.vg[k]; vp[k] = S.vp[k]; ids[k] = k < n ? S.ids[k] : -1; }  // rows past n_cur: no track (-1, 0)
    for (int k = k0; k < 2 * N0; k += step) p[k] = k < 2 * n ? S.p_cur[k] : 0.f;
    for (int k = k0; k < 3 * N0; k += step) p3[k] = S.p3[k];
    for (int k = k0; k < 14 * nh; k += step) B[k] = S.B[k];
    for (int k = k0; k < 9 * nh; k += step) R[k] = S.S[k];
    if (part == SESS_EXP_FLAT - 1 && tid == 0) {
        int* h = reinterpret_cast<int*>(rec + L.n_cur);
        h[0] = n; h[1] = S.n_pose; h[2] = S.frame_i; h[3] = S.klt_flags;
        int* pi = reinterpret_cast<int*>(rec + L.pose_info);
        pi[0] = S.pose_info[0]; pi[1] = S.pose_info[1];
        float* t = reinterpret_cast<float*>(rec + L.t);
        t[0] = S.t[0]; t[1] = S.t[1]; t[2] = S.t[2]; t[3] = 0.f;  // (the pad word: the whole record is defined)
        *reinterpret_cast<double*>(rec + L.res) = S.res;
    }
}

extern "C" VH_API size_t vh_session_export_size(const vh_session* s, vh_session_record* layout_host)
{
    if (!s) { vh_fail(-1, "vh_session_export_size: bad arguments"); return 0; }
    vh_session_record L;
    sess_record_layout(s->N0, s->nhist, &L);
    if (layout_host) *layout_host = L;
    return L.bytes;
}

extern "C" VH_API int vh_session_export(vh_session* s, int slot, void* rec_dev, void* stream)
{
    if (!s || !rec_dev || slot < 0 || slot >= s->batch || (reinterpret_cast<uintptr_t>(rec_dev) & 7)) return vh_fail(-1, "vh_session_export: bad arguments (the record must be 8-byte aligned)");
    vh_session_record L;
    sess_record_layout(s->N0, s->nhist, &L);
    const int tiles = (s->N0 + SESS_EXP_TILE - 1) / SESS_EXP_TILE;
    hipLaunchKernelGGL(k_sess_export, dim3(5 * tiles + SESS_EXP_FLAT), dim3(256), 0, (hipStream_t)stream, s->d_ss + slot, L, reinterpret_cast<char*>(rec_dev), tiles);
    SESS_CHECK();
    return 0;
}

// ---- anchored points of a slot's clip (vh_session_set_anchors): what the refinements below hold fixed ----------------------------------------------------
#define SESS_ANC_CHUNK 96  // anchors per launch: ids and coordinates travel in the kernel arguments (no upload, no host wait), 2688 bytes of them
struct AnchorChunk {
    int id[SESS_ANC_CHUNK];
    double xyz[SESS_ANC_CHUNK][3];
};
// snapshot: the slot's current p3 rows (what frame 0 gave them, when taken before fcnMSV1_t overwrites p3[vg] at the MSV frame)
__global__ __launch_bounds__(128) void k_sess_anchors(const SessStream* ss, uint8_t* mask, double* xyz, AnchorChunk ch, int cnt, int snapshot)
{
    const int t = threadIdx.x;
    if (t >= cnt) return;
    const int id = ch.id[t];
    mask[id] = 1;
    for (int c = 0; c < 3; c++) xyz[3 * (size_t)id + c] = snapshot ? ss->p3[3 * (size_t)id + c] : ch.xyz[t][c];
}

extern "C" VH_API int vh_session_set_anchors(vh_session* s, int slot, const int* ids_host, int n, const double* xyz_host, void* stream)
{
    char msg[200];
    if (!s) return vh_fail(-1, "vh_session_set_anchors: null session");
    if (slot < 0 || slot >= s->batch) {
        snprintf(msg, sizeof(msg), "vh_session_set_anchors: slot %d is outside the session's %d slots", slot, s->batch);
        return vh_fail(-1, msg);
    }
    if (!s->h_inited[slot]) { snprintf(msg, sizeof(msg), "vh_session_set_anchors: slot %d is not initialised (vh_session_init)", slot); return vh_fail(-1, msg); }
    if (n < 0 || n > s->N0) { snprintf(msg, sizeof(msg), "vh_session_set_anchors: slot %d: n = %d anchors, the session has %d tracks", slot, n, s->N0); return vh_fail(-1, msg); }
    if (n > 0 && !ids_host) { snprintf(msg, sizeof(msg), "vh_session_set_anchors: slot %d: null ids for %d anchors", slot, n); return vh_fail(-1, msg); }
    std::vector<char> seen(s->N0, 0);
    for (int k = 0; k < n; k++) {
        const int id = ids_host[k];
        if (id < 0 || id >= s->N0) { snprintf(msg, sizeof(msg), "vh_session_set_anchors: slot %d: id %d is outside [0, %d)", slot, id, s->N0); return vh_fail(-1, msg); }
        if (seen[id]) { snprintf(msg, sizeof(msg), "vh_session_set_anchors: slot %d: id %d is given twice", slot, id); return vh_fail(-1, msg); }
        seen[id] = 1;
    }
    VH_BIND(s->ctx, stream);
    uint8_t* mask = s->d_anc_mask + (size_t)slot * s->N0;
    double* xyz = s->d_anc_xyz + 3 * (size_t)slot * s->N0;
    const int had = s->h_nanchor[slot];
    s->h_nanchor[slot] = n;  // before anything is queued: should a launch below fail, the host count still says what the (partly written) table was asked to hold
    if (had > 0 || n > 0) VH_CHECK(hipMemsetAsync(mask, 0, (size_t)s->N0, bound_.s));
    for (int k0 = 0; k0 < n; k0 += SESS_ANC_CHUNK) {
        AnchorChunk ch;
        memset(&ch, 0, sizeof(ch));
        const int cnt = n - k0 < SESS_ANC_CHUNK ? n - k0 : SESS_ANC_CHUNK;
        for (int k = 0; k < cnt; k++) {
            ch.id[k] = ids_host[k0 + k];
            if (xyz_host) for (int c = 0; c < 3; c++) ch.xyz[k][c] = xyz_host[3 * (size_t)(k0 + k) + c];
        }
        hipLaunchKernelGGL(k_sess_anchors, dim3(1), dim3(128), 0, bound_.s, s->d_ss + slot, mask, xyz, ch, cnt, xyz_host ? 0 : 1);
    }
    SESS_CHECK();
    return 0;
}

// the slot's anchors read back, ascending id (a test accessor: it waits for the device).  Returns their number, -1 on bad arguments
extern "C" VH_API int vh_session_anchors(vh_session* s, int slot, int* ids_host, double* xyz_host)
{
    if (!s || slot < 0 || slot >= s->batch) return vh_fail(-1, "vh_session_anchors: bad arguments");
    std::vector<uint8_t> mask(s->N0);
    std::vector<double> xyz(3 * (size_t)s->N0);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(mask.data(), s->d_anc_mask + (size_t)slot * s->N0, (size_t)s->N0, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(xyz.data(), s->d_anc_xyz + 3 * (size_t)slot * s->N0, sizeof(double) * 3 * (size_t)s->N0, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { vh_set_error("vh_session_anchors: reading the table back", e, __FILE__, __LINE__); return -1; }  // (a count is never negative)
    int n = 0;
    for (int id = 0; id < s->N0; id++) {
        if (!mask[id]) continue;
        if (ids_host) ids_host[n] = id;
        if (xyz_host) for (int c = 0; c < 3; c++) xyz_host[3 * (size_t)n + c] = xyz[3 * (size_t)id + c];
        n++;
    }
    return n;
}

// ---- bundle adjustment of frame windows of the slots' clips (vidExample.py:157, NLS.py:186-250) -----------------------------------------------------------
// Huber weights for every refinement of the session (vh_nls_batch_windows_robust): a host setting like the anchors' count -- nothing is queued
extern "C" VH_API int vh_session_set_refine_robust(vh_session* s, double delta_px)
{
    if (!s) return vh_fail(-1, "vh_session_set_refine_robust: null session");
    if (!(delta_px >= 0.0) || !std::isfinite(delta_px)) {
        char msg[160];
        snprintf(msg, sizeof(msg), "vh_session_set_refine_robust: delta_px = %g must be finite and >= 0 (0 = off)", delta_px);
        return vh_fail(-1, msg);
    }
    s->refine_robust = delta_px;
    return 0;
}

// ONE request path behind both entries: window (slot, first) = frames [first, first + nf) of the slot's clip; vh_session_refine asks for the window
// first = 0 of clips that have just ended, vh_session_refine_windows for any.  pack: the window's tracks, their history, world points, per-frame
// translations and camera -> window w of one vh_nls_batch_windows problem laid out for N0 tracks; unpack: the refined state and the speed derived from it
// -> record w.  The session is only read.
#define SESS_REF_CHUNK 256  // windows per pack / unpack launch: they travel in the kernel arguments (no upload, no host wait)
struct RefReq {  // the windows of one launch (a whole clip: first = 0)
    int slot[SESS_REF_CHUNK];
    int first[SESS_REF_CHUNK];
};
struct RefWs {  // the scratch of one call, carved by refine_ws_layout
    double* z;   // [nwin][2][nf][N0]
    double* x;   // [nwin][3 N0 + 6 nc]
    double* K;   // [nwin][9]
    int* nt;     // [nwin]
    int* ids;    // [nwin][N0] the tracks of each window, ascending (null for vh_session_refine: a whole clip's are the slot's survivors)
    char* ba;    // [nwin] BA workspaces, ba_stride bytes apart
    uint8_t* fixed;  // [nwin][N0] anchored rows of each window (read by the solve only when a slot of the request has anchors)
    size_t z_stride, x_stride, ba_stride;
    uint8_t* tri_mask;  // [nwin][N0] partial windows only (else null): id g of the window starts at the point triangulated for it, tri_xyz
    double* tri_xyz;    // [nwin][N0][3] in the session's coordinates (rows of other ids: undefined)
};
struct RefPart {  // vh_refine_partial_params as the kernel sees them
    int min_obs, msv_frame;
    double start_reproj;
};
// a record of either public layout as the kernels see it: byte offsets taken from vh_refine_record or vh_refine_window_record (refine_view)
struct RefView {
    size_t bytes, head, nt, info, nfix, ids, pw, cw, dr, speed, speed_mean, speed_std, f_first, f_last, trace;
    int rows;         // of cw, dr and speed: nhist | nf
    int head_words;   // int32 words from `head` on: 4 {nt, iterations, converged, nfix} | 6 {slot, first, nt, iterations, converged, nfix}
    int max_iter;
    int with_points;  // ids and pw are in the record
    size_t tail;      // bytes behind everything else: 16 while the session refines with Huber weights (SESS_ROBUST_TAIL), else 0
};
// (table + workspace + view + the other arguments of the pack kernels, the partial one's parameters included: 2352 bytes of the 4 KB a launch may carry)
static_assert(sizeof(RefReq) + sizeof(RefWs) + sizeof(RefView) + 6 * sizeof(void*) + sizeof(RefPart) == 2352, "the refinement request travels in the kernel arguments");

#define SESS_ROBUST_TAIL 16  // {int32 nout_first, int32 nout_last, float32 delta, int32 0} behind a record refined with Huber weights (robust: the threshold, 0 = none)
static void refine_record_layout(int N0, int nhist, int max_iter, vh_refine_record* L, double robust)
{
    size_t off = 0;
    auto put = [&](size_t bytes) { const size_t o = off; off = vh_align_up(off + bytes, 8); return o; };
    L->nt = put(4 * sizeof(int)); L->iterations = L->nt + 4; L->converged = L->nt + 8;  // (iterations, converged: the int[2] info record of the window's solve)
    L->nfix = L->nt + 12;                                                               // (the header's fourth word)
    L->ids = put(sizeof(int) * (size_t)N0);
    L->pw = put(sizeof(double) * 3 * (size_t)N0);
    L->cw = put(sizeof(double) * 3 * (size_t)nhist);
    L->dr = put(sizeof(double) * (size_t)nhist); L->speed = put(sizeof(double) * (size_t)nhist);
    L->speed_mean = put(sizeof(double)); L->speed_std = put(sizeof(double)); L->f_first = put(sizeof(double)); L->f_last = put(sizeof(double));
    L->trace = put(sizeof(double) * 2 * (size_t)max_iter);
    L->bytes = off + (robust > 0 ? SESS_ROBUST_TAIL : 0);
    L->n0 = N0; L->nhist = nhist; L->max_iter = max_iter;
}

static void refine_window_record_layout(int N0, int nf, int max_iter, int with_points, vh_refine_window_record* L, double robust)
{
    size_t off = 0;
    auto put = [&](size_t bytes) { const size_t o = off; off = vh_align_up(off + bytes, 8); return o; };
    L->slot = put(6 * sizeof(int)); L->first = L->slot + 4; L->nt = L->slot + 8;
    L->iterations = L->slot + 12; L->converged = L->slot + 16;  // (iterations, converged: the int[2] info record of the window's solve)
    L->nfix = L->slot + 20;                                      // (the header's sixth word)
    L->cw = put(sizeof(double) * 3 * (size_t)nf);
    L->dr = put(sizeof(double) * (size_t)nf); L->speed = put(sizeof(double) * (size_t)nf);
    L->speed_mean = put(sizeof(double)); L->speed_std = put(sizeof(double)); L->f_first = put(sizeof(double)); L->f_last = put(sizeof(double));
    L->trace = put(sizeof(double) * 2 * (size_t)max_iter);
    L->ids = with_points ? put(sizeof(int) * (size_t)N0) : 0;
    L->pw = with_points ? put(sizeof(double) * 3 * (size_t)N0) : 0;
    L->bytes = off + (robust > 0 ? SESS_ROBUST_TAIL : 0);
    L->n0 = N0; L->nf = nf; L->max_iter = max_iter; L->with_points = with_points ? 1 : 0;
}

// a partial window's record: the window record, then the four counts (the shared fields keep the window record's offsets), then the robust tail
static void refine_partial_record_layout(int N0, int nf, int max_iter, int with_points, vh_refine_partial_record* L, double robust)
{
    refine_window_record_layout(N0, nf, max_iter, with_points, &L->win, 0.0);
    L->nobs = L->win.bytes; L->npart = L->nobs + 4; L->ntri = L->nobs + 8; L->nrej = L->nobs + 12;
    L->win.bytes += 4 * sizeof(int) + (robust > 0 ? SESS_ROBUST_TAIL : 0);
}

// the kernels' view of a public layout (the functions above stay the one source of every offset): head = the record's first header word
template <class Layout>
static RefView refine_view(const Layout& L, size_t head, int rows, int with_points, double robust)
{
    RefView V;
    V.tail = robust > 0 ? SESS_ROBUST_TAIL : 0;
    V.bytes = L.bytes; V.head = head; V.nt = L.nt; V.info = L.iterations; V.nfix = L.nfix; V.ids = L.ids; V.pw = L.pw; V.cw = L.cw; V.dr = L.dr;
    V.speed = L.speed; V.speed_mean = L.speed_mean; V.speed_std = L.speed_std; V.f_first = L.f_first; V.f_last = L.f_last; V.trace = L.trace;
    V.rows = rows; V.head_words = (int)((L.nfix - head) / sizeof(int)) + 1; V.max_iter = L.max_iter; V.with_points = with_points;
    return V;
}

static size_t refine_ws_layout(const vh_session* s, int nslots, int nf, char* base, RefWs* W, bool with_ids = false, bool partial = false)
{
    const size_t N0 = s->N0, nc = nf - 1, nw = nslots;
    VhCarver A(base);
    W->z_stride = 2 * N0 * (size_t)nf; W->x_stride = 3 * N0 + 6 * nc;
    W->ba_stride = vh_align_up(vh_nls_batch_workspace((int)N0, (int)nc), 256);
    W->z = A.take<double>(nw * W->z_stride);
    W->x = A.take<double>(nw * W->x_stride);
    W->K = A.take<double>(9 * nw);
    W->nt = A.take<int>(nw);
    W->ids = with_ids ? A.take<int>(nw * N0) : nullptr;
    W->ba = A.take<char>(nw * W->ba_stride);
    W->fixed = A.take<uint8_t>(nw * N0);  // (behind everything else: no other offset moves)
    W->tri_mask = partial ? A.take<uint8_t>(nw * N0) : nullptr;
    W->tri_xyz = partial ? A.take<double>(3 * nw * N0) : nullptr;
    return A.bytes();
}

// THE packing arithmetic of a refinement window (one copy: the whole clip is the window first = 0): frames [first, first + nf) of stream S and the n tracks
// ids[0..n) -> z, x0 and K of one window of a vh_ba_windows problem laid out for N0 tracks.  The session's points satisfy proj(K (p3 + B[i, 3:6])) and the
// BA fixes its camera 0 at the origin, so the window's points are p3 + B[first, 3:6] and its cameras B[first + c, 3:6] - B[first, 3:6]: float32 values
// widened to double first, the arithmetic in double (first = 0: B[0, 3:6] is 0, both are the session's own values).
// Anchors (am, ax: the slot's mask and coordinates over its N0 ids, null = none; fx: the window's row flags for the solve): a kept track that is anchored
// starts at its anchor's coordinates in place of p3, still + B[first, 3:6], and its row is flagged; padding rows never are.  Returns the anchors among the
// window's tracks (every thread of the workgroup calls this, every thread gets the count).
// Triangulated starts (tm, tx: the window's mask and coordinates over the N0 ids, null = none): a kept track with tm set starts at tx in place of p3.
__device__ __forceinline__ int refine_pack_window(const SessStream& S, const int* ids, int n, int first, int nf, double* z, double* x, double* Kw, int tid,
                                                  const uint8_t* am, const double* ax, uint8_t* fx, const uint8_t* tm = nullptr, const double* tx = nullptr)
{
    const int N0 = S.N0, nc = nf - 1;
    const double nanv = __longlong_as_double(0x7ff8000000000000LL);
    // z = [all u | all v], camera-major / track-minor (NLS.py:198-199), from the frame-major float32 history; rows behind the n tracks: no observation
    const size_t plane = (size_t)nf * N0;
    for (size_t e = tid; e < 2 * plane; e += 256) {
        const int row = e >= plane ? 1 : 0;
        const size_t rem = e - (size_t)row * plane;
        const int f = (int)(rem / N0), k = (int)(rem - (size_t)f * N0);
        z[e] = k < n ? (double)S.P[sess_P(row, ids[k], first + f, N0)] : nanv;
    }
    // x0 = [p3[ids] + B[first, 3:6] | B[first + 1 : first + nf, 3:6] - B[first, 3:6] | 0] (NLS.py:202-203); padding points sit at (0, 0, 1)
    const float* B0 = S.B + 14 * (size_t)first + 3;
    for (int e = tid; e < 3 * N0; e += 256) {
        const int k = e / 3, c = e - 3 * k;
        if (k < n) {
            const int id = ids[k];
            const bool anchored = am && am[id];
            const double* from = anchored ? ax : (tm && tm[id] ? tx : S.p3);
            x[e] = from[3 * (size_t)id + c] + (double)B0[c];
            if (am && c == 0) fx[k] = anchored ? 1 : 0;
        } else {
            x[e] = c == 2 ? 1.0 : 0.0;
            if (am && c == 0) fx[k] = 0;
        }
    }
    for (int e = tid; e < 3 * nc; e += 256) {
        const int i = e / 3 + 1, c = e - 3 * (i - 1);
        x[3 * (size_t)N0 + e] = (double)B0[14 * i + c] - (double)B0[c];
        x[3 * (size_t)N0 + 3 * nc + e] = 0.0;
    }
    if (tid < 9) Kw[tid] = S.K[tid];
    if (!am) return 0;
    __shared__ int s_nfix;
    if (tid == 0) s_nfix = 0;
    __syncthreads();
    int cnt = 0;
    for (int k = tid; k < n; k += 256) cnt += am[ids[k]] ? 1 : 0;
    if (cnt) atomicAdd(&s_nfix, cnt);
    __syncthreads();
    return s_nfix;
}

// where the derived quantities of one solved window go (both record types)
struct RefOut {
    int* nt;        // tracks solved
    const int* info;  // {iterations, converged} the solve wrote
    int* ids;       // [N0] or null
    double* pw;     // [N0][3] or null
    double *cw, *dr, *speed;  // [rows][3], [rows], [rows]
    double *speed_mean, *speed_std, *f_first, *f_last;
    const double* trace;
    int rows, max_iter;
};

// THE unpacking of a solved window: refined points, camera positions (row 0 zero, rows >= nf NaN) and the speed derived from them
__device__ __forceinline__ void refine_unpack_window(const SessStream& S, const int* ids_in, int n, int first, int nf, const double* x, const RefOut& o,
                                                     double* s_speed, int tid)
{
    const int N0 = S.N0;
    const double nanv = __longlong_as_double(0x7ff8000000000000LL);
    const double* cam = x + 3 * (size_t)N0;  // refined positions of cameras 1..nf-1 (camera 0 is the origin)
    if (o.ids)
        for (int k = tid; k < ((N0 + 1) & ~1); k += 256) o.ids[k] = k < n ? ids_in[k] : -1;  // (to the 8-byte boundary the next array starts on: the whole record is defined)
    if (o.pw)
        for (int e = tid; e < 3 * N0; e += 256) o.pw[e] = e < 3 * n ? x[e] : nanv;
    for (int e = tid; e < 3 * o.rows; e += 256) {
        const int i = e / 3;
        o.cw[e] = i == 0 ? 0.0 : (i < nf ? cam[e - 3] : nanv);
    }
    for (int i = tid; i < o.rows; i += 256) {
        double d = nanv, sp = nanv;
        if (i >= 1 && i < nf) {
            double ss = 0.0;
            for (int c = 0; c < 3; c++) {
                const double a = cam[3 * (i - 1) + c] - (i == 1 ? 0.0 : cam[3 * (i - 2) + c]);
                ss += a * a;
            }
            d = sqrt(ss);
            const float dt = __fsub_rn(S.B[14 * (first + i) + 12], S.B[14 * (first + i - 1) + 12]);  // the float32 difference vidExample.py:142 forms
            sp = d / (double)dt * 3.6;
            s_speed[i] = sp;
        }
        o.dr[i] = d; o.speed[i] = sp;
    }
    __syncthreads();
    if (tid == 0) {
        *o.nt = n;
        double m = 0.0, v = 0.0;  // vidExample.py:177: mean and population std over frames 1..nf-1
        for (int i = 1; i < nf; i++) m += s_speed[i];
        m /= (double)(nf - 1);
        for (int i = 1; i < nf; i++) v += (s_speed[i] - m) * (s_speed[i] - m);
        *o.speed_mean = m;
        *o.speed_std = sqrt(v / (double)(nf - 1));
        const int it = min(max(o.info[0], 0), o.max_iter);
        *o.f_first = it > 0 ? o.trace[0] : nanv;
        *o.f_last = it > 0 ? o.trace[2 * (it - 1)] : nanv;
    }
}

// One 256-id block of a selection: the kept ids of the block go behind the *s_base ids kept so far, ascending -- a ballot + the four wavefronts' counts
// give each its place.  Every thread of the workgroup calls this, once per block (barriers inside).
__device__ __forceinline__ void refine_keep(bool keep, int g, int* sel, int* s_cnt, int* s_base, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    __syncthreads();
    int at = *s_base;
    for (int k = 0; k < wave; k++) at += s_cnt[k];
    if (keep) sel[at + __popcll(bal & ((1ull << lane) - 1ull))] = g;
    __syncthreads();
    if (tid == 0) *s_base += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    __syncthreads();
}

// What every pack kernel does once it knows the window's n tracks: refine_pack_window, the count for the solve, and the part of the record the solve
// writes into (info, trace rows up to the iterations it takes) and the header -- {slot, first} where the record has them, then {nt, iterations,
// converged} = 0 and nfix, its last word: defined from the start
__device__ __forceinline__ void refine_pack_rest(const SessStream& S, const int* ids, int n, int slot, int first, int w, int nf, const RefWs& W,
                                                 const RefView& V, char* recs, const uint8_t* anc_mask, const double* anc_xyz, int tid,
                                                 const uint8_t* tm = nullptr, const double* tx = nullptr)
{
    const int N0 = S.N0;
    const int nfix = refine_pack_window(S, ids, n, first, nf, W.z + (size_t)w * W.z_stride, W.x + (size_t)w * W.x_stride, W.K + 9 * (size_t)w, tid,
                                        anc_mask ? anc_mask + (size_t)slot * N0 : nullptr, anc_mask ? anc_xyz + 3 * (size_t)slot * N0 : nullptr,
                                        W.fixed + (size_t)w * N0, tm, tx);
    if (tid == 0) W.nt[w] = n;
    char* rec = recs + (size_t)w * V.bytes;
    const int lead = V.head_words - 4;
    if (tid < V.head_words)
        reinterpret_cast<int*>(rec + V.head)[tid] = tid < lead ? (tid == lead - 2 ? slot : first) : (tid == V.head_words - 1 ? nfix : 0);
    double* trace = reinterpret_cast<double*>(rec + V.trace);
    for (int e = tid; e < 2 * V.max_iter; e += 256) trace[e] = 0.0;
}

// anc_mask / anc_xyz: the session's anchor tables over all slots, null when no slot of the request has anchors
// pack.  SELECT: the window's tracks are the ids whose history row 4 is finite in EVERY frame of the window (NLS.py:190 on the slice) -- not the slot's
// current survivors: a track that died after the window belongs to it.  256 ids at a time read row 4 of the frame-major history (coalesced over
// tracks), a ballot + the four wavefronts' counts give each kept id its place, so the ids come out ascending (into W.ids).  !SELECT (first = 0 of a
// clip that has just had its last frame): the slot's survivors ARE those tracks -- no pass, no scratch.  One workgroup per window.
// rp_all (a session with the replenishment on, else null): every request is SELECTed -- the shortcut assumes that survivors were alive at frame 0 -- and
// a selected track must also be triangulated (tri).
template <bool SELECT>
__global__ __launch_bounds__(256) void k_refine_pack(const SessStream* ss_all, RefReq rq, int w0, int nf, RefWs W, RefView V, char* recs,
                                                     const uint8_t* anc_mask, const double* anc_xyz, const SessRepl* rp_all)
{
    const int w = w0 + blockIdx.x, tid = threadIdx.x;
    const int slot = rq.slot[blockIdx.x], first = rq.first[blockIdx.x];
    const SessStream& S = ss_all[slot];
    const int N0 = S.N0;
    const int* ids = S.ids;
    int n = min(max(S.n_cur, 0), N0);
    if (SELECT) {
        int* sel = W.ids + (size_t)w * N0;
        __shared__ int s_cnt[4], s_base;
        if (tid == 0) s_base = 0;
        __syncthreads();
        for (int g0 = 0; g0 < N0; g0 += 256) {  // (uniform trip count: every lane of every wavefront reaches the ballot and the barriers)
            const int g = g0 + tid;
            bool alive = g < N0 && (!rp_all || rp_all[slot].tri[g]);  // (replenished session: a row not yet triangulated has no world point)
            for (int f = 0; alive && f < nf; f++) alive = isfinite(S.P[sess_P(4, g, first + f, N0)]);
            refine_keep(alive, g, sel, s_cnt, &s_base, tid);
        }
        ids = sel; n = s_base;  // (the ids written above are visible to the whole workgroup: barriers since)
    }
    refine_pack_rest(S, ids, n, slot, first, w, nf, W, V, recs, anc_mask, anc_xyz, tid);
}

// pack, the third selection form (vh_session_refine_windows_partial): the window's tracks are the ids observed in at least min_obs of its nf frames that
// have a usable world point, ascending.  Per 256-id block one thread per id: row 4 of the window frame by frame (coalesced over tracks) gives obs and the
// first and last observed frame; then, between two ballots and with no barrier inside,
//   A  obs == nf (and tri in a replenished session): today's rule;
//   B  the session has established p3[g]: g is anchored, or alive at the MSV frame once that has run, or row 2 of its history (the pose solve's
//      projection, written only while g is a pose track) is finite in some frame up to the slot's counter;
//   C  (start_reproj > 0) neither: the start is triangulated from the first and the last observed frame of the window by sess_triangulate, origins
//      float32(B[0, 0:3] - B[f, 0:3]) widened (MSV.py:18), and the track is admitted iff it passes that gate; the point goes to W.tri_xyz.
// The four counts go straight into the record (the 16 bytes in front of its tail: vh_refine_partial_record).
__global__ __launch_bounds__(256) void k_refine_pack_partial(const SessStream* ss_all, RefReq rq, int w0, int nf, RefWs W, RefView V, char* recs,
                                                             const uint8_t* anc_mask, const double* anc_xyz, const SessRepl* rp_all, RefPart Q)
{
    const int w = w0 + blockIdx.x, tid = threadIdx.x;
    const int slot = rq.slot[blockIdx.x], first = rq.first[blockIdx.x];
    const SessStream& S = ss_all[slot];
    const int N0 = S.N0, last = min(S.frame_i, S.nhist - 1);
    const uint8_t* am = anc_mask ? anc_mask + (size_t)slot * N0 : nullptr;
    const bool msv_ran = Q.msv_frame >= 0 && Q.msv_frame <= last;
    int* sel = W.ids + (size_t)w * N0;
    uint8_t* tm = W.tri_mask + (size_t)w * N0;
    double* tx = W.tri_xyz + 3 * (size_t)w * N0;
    __shared__ int s_cnt[4], s_base, s_tot[4];
    if (tid == 0) s_base = 0;
    if (tid < 4) s_tot[tid] = 0;
    __syncthreads();
    int nobs = 0, npart = 0, ntri = 0, nrej = 0;
    for (int g0 = 0; g0 < N0; g0 += 256) {  // (uniform trip count: every lane of every wavefront reaches the ballot and the barriers)
        const int g = g0 + tid;
        int obs = 0, fa = 0, fb = 0;
        if (g < N0)
            for (int f = 0; f < nf; f++)
                if (isfinite(S.P[sess_P(4, g, first + f, N0)])) {
                    if (!obs) fa = f;
                    fb = f;
                    obs++;
                }
        bool keep = false, tri = false;
        if (g < N0 && obs >= Q.min_obs) {
            keep = obs == nf && (!rp_all || rp_all[slot].tri[g]);
            if (!keep) {
                bool trusted = (am && am[g]) || (msv_ran && isfinite(S.P[sess_P(4, g, Q.msv_frame, N0)]));
                for (int f = 0; !trusted && f <= last; f++) trusted = isfinite(S.P[sess_P(2, g, f, N0)]);
                keep = trusted;
                if (!trusted && Q.start_reproj > 0.0) {
                    double A[6], T[6], K[9], c[3];
                    for (int j = 0; j < 2; j++)
                        for (int k = 0; k < 3; k++) {
                            const float* Bf = S.B + 14 * (size_t)(first + (j ? fb : fa));
                            A[3 * j + k] = (double)__fsub_rn(S.B[k], Bf[k]);
                            T[3 * j + k] = (double)Bf[3 + k];
                        }
                    for (int k = 0; k < 9; k++) K[k] = S.K[k];
                    keep = tri = sess_triangulate(A, T, 2, K, S.msv.f32_rays, [&](int j, int row) { return S.P[sess_P(row, g, first + (j ? fb : fa), N0)]; },
                                                  Q.start_reproj, c);
                    if (tri) for (int k = 0; k < 3; k++) tx[3 * (size_t)g + k] = c[k];
                    else nrej++;
                }
            }
        }
        if (g < N0) tm[g] = tri ? 1 : 0;
        if (keep) { nobs += obs; npart += obs < nf ? 1 : 0; ntri += tri ? 1 : 0; }
        refine_keep(keep, g, sel, s_cnt, &s_base, tid);
    }
    if (nobs) atomicAdd(&s_tot[0], nobs);
    if (npart) atomicAdd(&s_tot[1], npart);
    if (ntri) atomicAdd(&s_tot[2], ntri);
    if (nrej) atomicAdd(&s_tot[3], nrej);
    __syncthreads();  // (also: the ids, tm and tx written above are visible to the whole workgroup)
    if (tid < 4) reinterpret_cast<int*>(recs + (size_t)w * V.bytes + V.bytes - V.tail - 16)[tid] = s_tot[tid];
    refine_pack_rest(S, sel, s_base, slot, first, w, nf, W, V, recs, anc_mask, anc_xyz, tid, tm, tx);
}

// unpack: W.ids is null when the windows are whole clips (the slot's survivors, as packed)
__global__ __launch_bounds__(256) void k_refine_unpack(const SessStream* ss_all, RefReq rq, int w0, int nf, RefWs W, RefView V, char* recs)
{
    const int w = w0 + blockIdx.x, tid = threadIdx.x;
    const SessStream& S = ss_all[rq.slot[blockIdx.x]];
    char* rec = recs + (size_t)w * V.bytes;
    __shared__ double s_speed[256];  // nf <= 256 (the BA's camera limit)
    RefOut o;
    o.nt = reinterpret_cast<int*>(rec + V.nt); o.info = reinterpret_cast<const int*>(rec + V.info);
    o.ids = V.with_points ? reinterpret_cast<int*>(rec + V.ids) : nullptr; o.pw = V.with_points ? reinterpret_cast<double*>(rec + V.pw) : nullptr;
    o.cw = reinterpret_cast<double*>(rec + V.cw); o.dr = reinterpret_cast<double*>(rec + V.dr); o.speed = reinterpret_cast<double*>(rec + V.speed);
    o.speed_mean = reinterpret_cast<double*>(rec + V.speed_mean); o.speed_std = reinterpret_cast<double*>(rec + V.speed_std);
    o.f_first = reinterpret_cast<double*>(rec + V.f_first); o.f_last = reinterpret_cast<double*>(rec + V.f_last);
    o.trace = reinterpret_cast<const double*>(rec + V.trace); o.rows = V.rows; o.max_iter = V.max_iter;
    refine_unpack_window(S, W.ids ? W.ids + (size_t)w * S.N0 : S.ids, W.nt[w], rq.first[blockIdx.x], nf, W.x + (size_t)w * W.x_stride, o, s_speed, tid);
}

// the tail of the records of a request refined with Huber weights: the solve left {count at iteration 0, count at the last iteration run} in each window's
// BA workspace (vh_ba.hpp; 0, 0 for a window that was not solved).  One thread per window
__global__ __launch_bounds__(256) void k_refine_robust_tail(char* recs, size_t rec_bytes, int n, const int* words, size_t words_stride, float delta)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const int* c = reinterpret_cast<const int*>(reinterpret_cast<const char*>(words) + (size_t)w * words_stride);
    int* t = reinterpret_cast<int*>(recs + (size_t)w * rec_bytes + rec_bytes - SESS_ROBUST_TAIL);
    t[0] = c[1]; t[1] = c[2];
    reinterpret_cast<float*>(t)[2] = delta;
    t[3] = 0;
}

struct RefEntry {  // how a public entry words the refusals both share
    const char* name;
    bool windows;            // vh_session_refine_windows: selected tracks, its record; else whole clips
    const char* bad_args;    // null arguments (vh_session_refine: its one message for those, misaligned buffers, no slot and no iteration)
    const char* misaligned;
    const char* unit;        // what nf frames are: "a clip" | "a window"
    const char* per;         // behind the camera limit: "" | " per window"
    const char* noun;        // "slots" | "windows"
};
static const char REF_CLIPS_BAD[] = "vh_session_refine: bad arguments (records 8-byte, workspace 256-byte aligned; at least one slot and one iteration)";
static const RefEntry REF_CLIPS = {"vh_session_refine", false, REF_CLIPS_BAD, REF_CLIPS_BAD, "a clip", "", "slots"};
static const RefEntry REF_WINDOWS = {"vh_session_refine_windows", true,
                                     "vh_session_refine_windows: bad arguments (a null session, window table, record buffer or workspace)",
                                     "vh_session_refine_windows: misaligned buffers (records 8-byte, workspace 256-byte aligned)", "a window", " per window",
                                     "windows"};
static const RefEntry REF_PARTIAL = {"vh_session_refine_windows_partial", true,
                                     "vh_session_refine_windows_partial: bad arguments (a null session, window table, parameters, record buffer or workspace)",
                                     "vh_session_refine_windows_partial: misaligned buffers (records 8-byte, workspace 256-byte aligned)", "a window",
                                     " per window", "windows"};

// THE refinement request: n windows of nf frames -> n records at recs_dev.  The checks both entries share, worded as E's; own(fail, req): the entry's
// own checks of its table, which leaves the windows in req (or returns what fail returned); then the workspace, pack, ONE vh_ba_windows launch
// sequence, unpack.  Every refusal returns before anything is queued.  part (vh_session_refine_windows_partial, else null): the third selection form
// and its record.
template <class Own>
static int refine_request(const RefEntry& E, vh_session* s, const void* table, int n, int nf, int max_iter, int with_points, void* recs_dev, void* workspace,
                          size_t workspace_bytes, void* stream, Own own, const vh_refine_partial_params* part = nullptr)
{
    char msg[240];
    auto fail = [&](const char* fmt, auto... a) {
        const int at = snprintf(msg, sizeof(msg), "%s: ", E.name);
        snprintf(msg + at, sizeof(msg) - at, fmt, a...);
        return vh_fail(-1, msg);
    };
    if (!s || !table || !recs_dev || !workspace) return vh_fail(-1, E.bad_args);
    if ((reinterpret_cast<uintptr_t>(recs_dev) & 7) || (reinterpret_cast<uintptr_t>(workspace) & 255)) return vh_fail(-1, E.misaligned);
    if (n < 1) return E.windows ? fail("nwin = %d: at least one window", n) : vh_fail(-1, E.bad_args);
    if (E.windows && n > 65535) return fail("nwin = %d: at most 65535 windows in one launch sequence", n);
    if (max_iter < 1) return E.windows ? fail("max_iter = %d: at least one iteration", max_iter) : vh_fail(-1, E.bad_args);
    if (nf < 2) return fail("nf = %d: %s needs at least two frames", nf, E.unit);
    if (nf - 1 > 255) return fail("nf = %d: at most 255 free cameras (256 frames)%s", nf, E.per);
    if (nf > s->nhist) return fail("nf = %d exceeds the session's history of %d frames", nf, s->nhist);
    std::vector<vh_refine_window> req;
    if (int r = own(fail, req)) return r;
    RefWs W;
    const bool select = E.windows || s->rp.on;  // (replenished session: survivors need not have been alive at frame 0)
    const size_t need = refine_ws_layout(s, n, nf, reinterpret_cast<char*>(workspace), &W, select, part != nullptr);
    if (workspace_bytes < need) return fail("workspace of %zu bytes, %d %s of %d frames need %zu", workspace_bytes, n, E.noun, nf, need);
    const double robust = s->refine_robust;  // (0: every launch, table and record below is what it is without the option)
    RefView V;
    if (part) {
        vh_refine_partial_record L;
        refine_partial_record_layout(s->N0, nf, max_iter, with_points, &L, robust);
        V = refine_view(L.win, L.win.slot, nf, L.win.with_points, robust);
    } else if (E.windows) {
        vh_refine_window_record L;
        refine_window_record_layout(s->N0, nf, max_iter, with_points, &L, robust);
        V = refine_view(L, L.slot, nf, L.with_points, robust);
    } else {
        vh_refine_record L;
        refine_record_layout(s->N0, s->nhist, max_iter, &L, robust);
        V = refine_view(L, L.nt, s->nhist, 1, robust);
    }
    char* recs = reinterpret_cast<char*>(recs_dev);
    bool anchored = false;  // the tables travel only when a slot of the request has anchors: otherwise the solve is queued as ever, with no table
    for (int k = 0; k < n; k++) anchored = anchored || s->h_nanchor[req[k].slot] > 0;
    auto each_chunk = [&](auto kernel, hipStream_t st, auto... more) {
        for (int w0 = 0; w0 < n; w0 += SESS_REF_CHUNK) {
            RefReq rq;
            const int cnt = n - w0 < SESS_REF_CHUNK ? n - w0 : SESS_REF_CHUNK;
            for (int k = 0; k < SESS_REF_CHUNK; k++) {  // (behind the last window: window w0 again, which no workgroup reads)
                rq.slot[k] = req[w0 + (k < cnt ? k : 0)].slot;
                rq.first[k] = req[w0 + (k < cnt ? k : 0)].first;
            }
            hipLaunchKernelGGL(kernel, dim3(cnt), dim3(256), 0, st, s->d_ss, rq, w0, nf, W, V, recs, more...);
        }
    };
    {
        VH_BIND(s->ctx, stream);
        const uint8_t* mask = anchored ? s->d_anc_mask : nullptr;
        const double* xyz = anchored ? s->d_anc_xyz : nullptr;
        const SessRepl* rp = s->rp.on ? s->rp.d_rp : nullptr;
        if (part) each_chunk(k_refine_pack_partial, bound_.s, mask, xyz, rp, RefPart{part->min_obs, s->msv_frame, (double)part->start_reproj});
        else if (select) each_chunk(k_refine_pack<true>, bound_.s, mask, xyz, rp);
        else each_chunk(k_refine_pack<false>, bound_.s, mask, xyz, rp);
        SESS_CHECK();
    }
    // the windows' info = {iterations, converged} and trace go straight into the records
    int r = vh_ba_windows(s->ctx, s->h_ss[req[0].slot].K, W.z, W.x, s->N0, nf - 1, n, W.nt, W.K, anchored ? W.fixed : nullptr, max_iter, reinterpret_cast<double*>(recs + V.trace),
                          V.bytes / sizeof(double), reinterpret_cast<int*>(recs + V.info), V.bytes / sizeof(int), W.ba, W.ba_stride, stream, robust);
    if (r) return r;
    VH_BIND(s->ctx, stream);
    each_chunk(k_refine_unpack, bound_.s);
    if (robust > 0)
        hipLaunchKernelGGL(k_refine_robust_tail, dim3((n + 255) / 256), dim3(256), 0, bound_.s, recs, V.bytes, n, vh_ba_windows_outlier_words(s->N0, nf - 1, n, W.ba),
                           W.ba_stride, (float)robust);
    SESS_CHECK();
    return 0;
}

extern "C" VH_API size_t vh_session_refine_size(const vh_session* s, int max_iter, vh_refine_record* layout_host)
{
    if (!s || max_iter < 1) { vh_fail(-1, "vh_session_refine_size: bad arguments"); return 0; }
    vh_refine_record L;
    refine_record_layout(s->N0, s->nhist, max_iter, &L, s->refine_robust);
    if (layout_host) *layout_host = L;
    return L.bytes;
}

extern "C" VH_API size_t vh_session_refine_workspace(const vh_session* s, int nslots, int nf)
{
    if (!s || nslots < 1 || nslots > s->batch || nf < 2 || nf - 1 > 255) { vh_fail(-1, "vh_session_refine_workspace: bad arguments"); return 0; }
    RefWs W;
    return refine_ws_layout(s, nslots, nf, nullptr, &W, s->rp.on != 0);
}

extern "C" VH_API int vh_session_refine(vh_session* s, const int* slots_host, int nslots, int nf, int max_iter, void* recs_dev, void* workspace,
                                        size_t workspace_bytes, void* stream)
{
    return refine_request(REF_CLIPS, s, slots_host, nslots, nf, max_iter, 1, recs_dev, workspace, workspace_bytes, stream, [&](auto fail, auto& req) {
        if (nslots > s->batch) return fail("%d slots, the session has %d", nslots, s->batch);
        std::vector<char> seen(s->batch, 0);
        for (int k = 0; k < nslots; k++) {
            const int b = slots_host[k];
            if (b < 0 || b >= s->batch) return fail("slot %d is outside the session's %d slots", b, s->batch);
            if (seen[b]) return fail("slot %d is given twice", b);
            seen[b] = 1;
            if (s->h_frame[b] != nf - 1) return fail("slot %d is at frame %d, not at the last frame nf - 1 = %d of its clip", b, s->h_frame[b], nf - 1);
            req.push_back({b, 0});
        }
        return 0;
    });
}

extern "C" VH_API size_t vh_session_refine_windows_size(const vh_session* s, int nf, int max_iter, int with_points, vh_refine_window_record* layout_host)
{
    if (!s || nf < 2 || max_iter < 1) { vh_fail(-1, "vh_session_refine_windows_size: bad arguments"); return 0; }
    vh_refine_window_record L;
    refine_window_record_layout(s->N0, nf, max_iter, with_points, &L, s->refine_robust);
    if (layout_host) *layout_host = L;
    return L.bytes;
}

extern "C" VH_API size_t vh_session_refine_windows_workspace(const vh_session* s, int nwin, int nf)
{
    if (!s || nwin < 1 || nf < 2 || nf - 1 > 255) { vh_fail(-1, "vh_session_refine_windows_workspace: bad arguments"); return 0; }
    RefWs W;
    return refine_ws_layout(s, nwin, nf, nullptr, &W, true);
}

// the checks of a window table (both window entries)
template <class Fail>
static int refine_check_windows(const vh_session* s, const vh_refine_window* wins_host, int nwin, int nf, Fail fail, std::vector<vh_refine_window>& req)
{
    std::vector<std::vector<int>> seen(s->batch);  // per slot: the window starts given so far
    for (int k = 0; k < nwin; k++) {
        const int b = wins_host[k].slot, first = wins_host[k].first;
        if (b < 0 || b >= s->batch) return fail("window %d: slot %d is outside the session's %d slots", k, b, s->batch);
        if (first < 0) return fail("window %d (slot %d): first = %d is negative", k, b, first);
        const int last_have = s->h_frame[b] < s->nhist - 1 ? s->h_frame[b] : s->nhist - 1;  // (the history holds nhist frames)
        if (first > last_have || nf - 1 > last_have - first)
            return fail("window %d (slot %d, first %d) ends at frame %lld, the slot is at frame %d", k, b, first, (long long)first + nf - 1, last_have);
        for (int f : seen[b])
            if (f == first) return fail("window (slot %d, first %d) is given twice", b, first);
        seen[b].push_back(first);
    }
    req.assign(wins_host, wins_host + nwin);
    return 0;
}

extern "C" VH_API int vh_session_refine_windows(vh_session* s, const vh_refine_window* wins_host, int nwin, int nf, int max_iter, int with_points,
                                                void* recs_dev, void* workspace, size_t workspace_bytes, void* stream)
{
    return refine_request(REF_WINDOWS, s, wins_host, nwin, nf, max_iter, with_points, recs_dev, workspace, workspace_bytes, stream,
                          [&](auto fail, auto& req) { return refine_check_windows(s, wins_host, nwin, nf, fail, req); });
}

extern "C" VH_API size_t vh_session_refine_windows_partial_size(const vh_session* s, int nf, int max_iter, int with_points, vh_refine_partial_record* layout_host)
{
    if (!s || nf < 2 || max_iter < 1) { vh_fail(-1, "vh_session_refine_windows_partial_size: bad arguments"); return 0; }
    vh_refine_partial_record L;
    refine_partial_record_layout(s->N0, nf, max_iter, with_points, &L, s->refine_robust);
    if (layout_host) *layout_host = L;
    return L.win.bytes;
}

extern "C" VH_API size_t vh_session_refine_windows_partial_workspace(const vh_session* s, int nwin, int nf)
{
    if (!s || nwin < 1 || nf < 2 || nf - 1 > 255) { vh_fail(-1, "vh_session_refine_windows_partial_workspace: bad arguments"); return 0; }
    RefWs W;
    return refine_ws_layout(s, nwin, nf, nullptr, &W, true, true);
}

extern "C" VH_API int vh_session_refine_windows_partial(vh_session* s, const vh_refine_window* wins_host, int nwin, int nf, int max_iter, int with_points,
                                                        const vh_refine_partial_params* params_host, void* recs_dev, void* workspace,
                                                        size_t workspace_bytes, void* stream)
{
    if (!params_host) return vh_fail(-1, REF_PARTIAL.bad_args);
    const vh_refine_partial_params P = *params_host;
    return refine_request(REF_PARTIAL, s, wins_host, nwin, nf, max_iter, with_points, recs_dev, workspace, workspace_bytes, stream,
                          [&](auto fail, auto& req) {
                              if (P.min_obs < 2) return fail("min_obs = %d: a track needs at least 2 observations in a window of %d frames", P.min_obs, nf);
                              if (P.min_obs > nf) return fail("min_obs = %d exceeds the window's nf = %d frames", P.min_obs, nf);
                              if (!(P.start_reproj >= 0.f) || !std::isfinite(P.start_reproj))
                                  return fail("start_reproj = %g: the gate of a triangulated start is a finite number of pixels >= 0 (0 = no such starts)", (double)P.start_reproj);
                              return refine_check_windows(s, wins_host, nwin, nf, fail, req);
                          }, &P);
}

// packed track state of every stream for the cross-GPU exchange (K20): per stream a record of 8 + 3*N0 float32 words
// [n_cur, n_pose, frame_i, klt_flags, t0, t1, t2, res | p (N0 x 2, zero padded) | ids (N0 int32 bit patterns, -1 padded)]
__global__ __launch_bounds__(256) void k_sess_pack(const SessStream* ss_all, float* out, int rec)
{
    const SessStream& S = ss_all[blockIdx.x];
    float* o = out + (size_t)blockIdx.x * rec;
    const int N0 = S.N0, n = S.n_cur;
    if (threadIdx.x == 0) {
        o[0] = (float)n; o[1] = (float)S.n_pose; o[2] = (float)S.frame_i; o[3] = (float)S.klt_flags;
        o[4] = S.t[0]; o[5] = S.t[1]; o[6] = S.t[2]; o[7] = (float)S.res;
    }
    for (int k = threadIdx.x; k < N0; k += 256) {
        o[8 + 2 * k] = k < n ? S.p_cur[2 * k] : 0.f;
        o[8 + 2 * k + 1] = k < n ? S.p_cur[2 * k + 1] : 0.f;
        o[8 + 2 * N0 + k] = __int_as_float(k < n ? S.ids[k] : -1);
    }
}

// fused frame ingest for every stream: descriptors from the stream state (the quarter-scale image goes straight into
// the buffer the coming step reads as im_small), then ONE pass over the BGR frames
__global__ void k_sess_ingest_jobs(SessStream* ss_all, IngestJob* jobs, const uint8_t* const* bgr, int bgr_stride, uint8_t* const* gray, int batch)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    SessStream& S = ss_all[b];
    IngestJob J;
    J.bgr = bgr[b]; J.gray = gray[b]; J.small = S.small[S.pp];
    J.w = S.w; J.h = S.h; J.bgr_stride = bgr_stride ? bgr_stride : 3 * S.w; J.gray_stride = S.stride;  // (0: dense rows of this stream's own width)
    J.dw = __double2int_rn(S.w * 0.25); J.dh = __double2int_rn(S.h * 0.25); J.small_stride = J.dw;
    jobs[b] = J;
    if (J.bgr != nullptr) S.small_ready = S.frame_i + 1;
}

extern "C" VH_API int vh_session_ingest_bgr(vh_session* s, const uint8_t* const* bgr_frames_dev, int bgr_stride, uint8_t* const* gray_frames_dev, void* stream)
{
    if (!s || !bgr_frames_dev || !gray_frames_dev || bgr_stride < 0) return vh_fail(-1, "vh_session_ingest_bgr: bad arguments");
    if (bgr_stride) {  // one stride for every stream: it must cover the widest slot (a session of one camera: 3 x its width, as ever)
        int mw = 0;
        for (int b = 0; b < s->batch; b++) mw = s->h_ss[b].w > mw ? s->h_ss[b].w : mw;
        if (bgr_stride < 3 * mw) return vh_fail(-1, "vh_session_ingest_bgr: bgr_stride is below 3 x the widest slot (0 = dense rows per stream)");
    }
    VH_BIND(s->ctx, stream);
    hipStream_t st = bound_.s;
    hipLaunchKernelGGL(k_sess_ingest_jobs, dim3((s->batch + 63) / 64), dim3(64), 0, st, s->d_ss, s->d_ingest, bgr_frames_dev, bgr_stride, gray_frames_dev, s->batch);
    vh_launch_ingest_bgr(s->d_ingest, s->batch, s->w, s->h, st);
    SESS_CHECK();
    return 0;
}

extern "C" VH_API int vh_session_pack_state(vh_session* s, float* out, void* stream)
{
    if (!s || !out) return vh_fail(-1, "vh_session_pack_state: bad arguments");
    hipLaunchKernelGGL(k_sess_pack, dim3(s->batch), dim3(256), 0, (hipStream_t)stream, s->d_ss, out, 8 + 3 * s->N0);
    SESS_CHECK();
    return 0;
}

extern "C" VH_API int vh_session_ptrs(vh_session* s, int slot, vh_session_view* out)
{
    if (!s || !out || slot < 0 || slot >= s->batch) return vh_fail(-1, "vh_session_ptrs: bad arguments");
    const SessStream& H = s->h_ss[slot];
    SessStream* d = s->d_ss + slot;
    out->vg = H.vg; out->vp = H.vp; out->p = H.p_cur; out->ids = H.ids; out->p3 = H.p3; out->P = H.P; out->B = H.B; out->S = H.S;
    out->n_cur = &d->n_cur; out->n_pose = &d->n_pose; out->t = d->t; out->res = &d->res; out->frame_i = &d->frame_i;
    out->klt_flags = &d->klt_flags; out->pose_info = d->pose_info; out->sel_pw = H.sel_pw; out->p_proj = H.p_proj;
    // history layout, in floats: entry (row, track, frame) of P at P[row * P_row_stride + track * P_track_stride + frame * P_frame_stride]
    out->P_row_stride = (size_t)H.N0; out->P_track_stride = 1; out->P_frame_stride = (size_t)5 * H.N0;
    out->n0 = H.N0; out->nhist = H.nhist;
    return 0;
}
