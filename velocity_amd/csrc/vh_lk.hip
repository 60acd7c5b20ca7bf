// Pyramidal Lucas-Kanade track solve (K3+K4+K5).
//
// Replaces cv2calcOpticalFlowPyrLK (utils/KLT.py:37-51): forward LK over all pyramid levels, optional backward LK from
// the result, forward-backward gate, and the map-back of KLTregional (KLT.py:86-89) / the 1/4-scale stage (KLT.py:115).
// Arithmetic follows SURVEY Appendix A: Scharr derivatives (never materialised), 14-bit fixed-point bilinear weights,
// int16 template / gradient windows, exact integer window sums converted once to float32, so every implementation in this
// file returns the same bits.  Five implementations, routed by vh_launch_lk (window size and number of tracks in flight):
//   k_lk            per-sample reference kernel, one wavefront per track (any window; fallback for windows > 63 px)
//   k_lk_strip<W>   strips of 4 samples per lane on packed 16-bit dot products, one wavefront per track, loads from L1/L2
//   k_lk3<W,NW,M>   LDS-staged patch + search region, NW wavefronts per track, vertical strip runs (the 51x51 fine stage)
//   k_lk_q<W>       4 tracks per wavefront, one 16-lane DPP row per track, template in registers (the 15x15 coarse stages)
//   k_lk_o<W>       8 tracks per wavefront, half a DPP row per track, two window rows per lane (the 15x15 coarse stages at full load)
//   k_lk_h<W>       16 tracks per wavefront, a DPP quad per track, four window rows per lane, part of the template in LDS (the 15x15 coarse stages from 128 000 tracks in flight)
// An implementation is its window sampling and its window-sum reduction: a level functor (LK*Level below).  What a track computes from the
// reduced sums (level start, 2x2 system and its gate, Newton update and stop rules, final in-level check), the loop over the levels, the
// forward-backward gate, and a kernel's prologue (job row, launch slot -> point, start point) and epilogue (map-back, output stores, statistics)
// exist once, in vh_lk_shared.hpp.
#include <algorithm>

#include "vh_kernels.hpp"
#include "vh_valu.hpp"
#include "vh_lk_shared.hpp"

// REFLECT_101 sample (image border of the pyramid levels)
__device__ __forceinline__ int pix_r(const ImgDesc& im, int x, int y)
{
    return im.p[(size_t)vh_reflect101_near(y, im.h) * im.stride + vh_reflect101_near(x, im.w)];  // (|x|, |y| within a window of the level)
}

// template window sample: I (x32), Ix, Iy at the bilinear cell whose top-left pixel is (gx, gy)
template <bool INTERIOR>
__device__ __forceinline__ void template_sample(const ImgDesc& im, int gx, int gy, const Win& w, int& iv, int& ix, int& iy)
{
    int q[4][4];
    if (INTERIOR) {
        const uint8_t* p = im.p + (ptrdiff_t)(gy - 1) * im.stride + (gx - 1);
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) q[r][c] = p[r * im.stride + c];
    } else {
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) q[r][c] = pix_r(im, gx - 1 + c, gy - 1 + r);
    }
    // vertical [3 10 3] smooth and [-1 0 1] difference for the two corner rows, all four columns
    int s[2][4], d[2][4];
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            s[b][c] = (q[b][c] + q[b + 2][c]) * 3 + q[b + 1][c] * 10;
            d[b][c] = q[b + 2][c] - q[b][c];
        }
    int gxv[2][2], gyv[2][2];
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
        for (int a = 0; a < 2; a++) {
            gxv[b][a] = s[b][a + 2] - s[b][a];
            gyv[b][a] = (d[b][a] + d[b][a + 2]) * 3 + d[b][a + 1] * 10;
            if (!INTERIOR) {  // derivative image is constant 0 outside the level
                const bool in = (gx + a) >= 0 && (gx + a) < im.w && (gy + b) >= 0 && (gy + b) < im.h;
                if (!in) { gxv[b][a] = 0; gyv[b][a] = 0; }
            }
        }
    iv = vh_descale(q[1][1] * w.w00 + q[1][2] * w.w01 + q[2][1] * w.w10 + q[2][2] * w.w11, W_BITS - 5);
    ix = vh_descale(gxv[0][0] * w.w00 + gxv[0][1] * w.w01 + gxv[1][0] * w.w10 + gxv[1][1] * w.w11, W_BITS);
    iy = vh_descale(gyv[0][0] * w.w00 + gyv[0][1] * w.w01 + gyv[1][0] * w.w10 + gyv[1][1] * w.w11, W_BITS);
}

template <bool INTERIOR>
__device__ __forceinline__ int search_sample(const ImgDesc& im, int gx, int gy, const Win& w)
{
    int q00, q01, q10, q11;
    if (INTERIOR) {
        const uint8_t* p = im.p + (ptrdiff_t)gy * im.stride + gx;
        q00 = p[0]; q01 = p[1]; q10 = p[im.stride]; q11 = p[im.stride + 1];
    } else {
        q00 = pix_r(im, gx, gy); q01 = pix_r(im, gx + 1, gy); q10 = pix_r(im, gx, gy + 1); q11 = pix_r(im, gx + 1, gy + 1);
    }
    return vh_descale(q00 * w.w00 + q01 * w.w01 + q10 * w.w10 + q11 * w.w11, W_BITS - 5);
}

// One point on one level.  All control flow is wave-uniform.
struct LKLevel {  // the level functor of k_lk (see lk_track)
    int win, max_count;
    double eps2;
    short* ldsI;
    int* ldsD;
    int lane, n_iter, n_setup;
    __device__ void operator()(const ImgDesc I, const ImgDesc J, int level, int top_level, float p0x, float p0y, float& nxo, float& nyo, int& status,
                               float& err, bool want_err);
};
__device__ void LKLevel::operator()(const ImgDesc I, const ImgDesc J, int level, int top_level, float p0x, float p0y, float& nxo, float& nyo,
                                    int& status, float& err, bool want_err)
{
    LKStart s;
    if (!lk_level_start(p0x, p0y, level, top_level, win, I, nxo, nyo, status, err, s)) return;
    const float half = s.half;
    const int ipx = s.ipx, ipy = s.ipy;
    float nx = s.nx, ny = s.ny;
    Win w = bilinear_weights(__fsub_rn(s.px, (float)ipx), __fsub_rn(s.py, (float)ipy));
    const int npx = win * win;
    const int xinc = 64 % win, yinc = 64 / win;
    const int x_first = lane % win, y_first = lane / win;

    n_setup++;
    long long sA11 = 0, sA12 = 0, sA22 = 0;
    {
        const bool interior = ipx >= 1 && ipy >= 1 && ipx + win + 1 <= I.w - 1 && ipy + win + 1 <= I.h - 1;
        int x = x_first, y = y_first, k = 0;
        for (int i = lane; i < npx; i += 64, k++) {
            int iv, ix, iy;
            if (interior) template_sample<true>(I, ipx + x, ipy + y, w, iv, ix, iy);
            else template_sample<false>(I, ipx + x, ipy + y, w, iv, ix, iy);
            ldsI[k * 64 + lane] = (short)iv;
            ldsD[k * 64 + lane] = (ix & 0xffff) | (iy << 16);
            sA11 += (long long)(ix * ix);
            sA12 += (long long)(ix * iy);
            sA22 += (long long)(iy * iy);
            x += xinc; y += yinc;
            if (x >= win) { x -= win; y++; }
        }
    }
    sA11 = vh_wave_sum_i64(sA11);
    sA12 = vh_wave_sum_i64(sA12);
    sA22 = vh_wave_sum_i64(sA22);
    LKSys S;
    if (!lk_system(sA11, sA12, sA22, win, S)) {
        if (level == 0) status = 0;
        return;
    }

    float pdx = 0.f, pdy = 0.f;
    for (int j = 0; j < max_count; j++) {
        const int inx = vh_floor(nx), iny = vh_floor(ny);
        if (lk_outside(inx, iny, win, J)) {
            if (level == 0) status = 0;
            break;
        }
        w = bilinear_weights(__fsub_rn(nx, (float)inx), __fsub_rn(ny, (float)iny));
        const bool interior = inx >= 0 && iny >= 0 && inx + win <= J.w - 1 && iny + win <= J.h - 1;
        n_iter++;
        long long sb1 = 0, sb2 = 0;
        int x = x_first, y = y_first, k = 0;
        for (int i = lane; i < npx; i += 64, k++) {
            const int jv = interior ? search_sample<true>(J, inx + x, iny + y, w) : search_sample<false>(J, inx + x, iny + y, w);
            const int diff = jv - (int)ldsI[k * 64 + lane];
            const int dd = ldsD[k * 64 + lane];
            sb1 += (long long)(diff * (int)(short)(dd & 0xffff));
            sb2 += (long long)(diff * (dd >> 16));
            x += xinc; y += yinc;
            if (x >= win) { x -= win; y++; }
        }
        sb1 = vh_wave_sum_i64(sb1);
        sb2 = vh_wave_sum_i64(sb2);
        if (lk_step(S, sb1, sb2, half, j, eps2, nx, ny, nxo, nyo, pdx, pdy)) break;
    }

    if (status && level == 0) {
        float fx, fy;
        int inx, iny;
        if (!lk_final_origin(nxo, nyo, half, win, J, fx, fy, inx, iny)) { status = 0; return; }
        if (!want_err) return;  // err is discarded by the caller (KLT.py:83 `pa, v, _`): only the bounds rule matters
        w = bilinear_weights(__fsub_rn(fx, (float)inx), __fsub_rn(fy, (float)iny));
        const bool interior = inx >= 0 && iny >= 0 && inx + win <= J.w - 1 && iny + win <= J.h - 1;
        long long se = 0;
        int x = x_first, y = y_first, k = 0;
        for (int i = lane; i < npx; i += 64, k++) {
            const int jv = interior ? search_sample<true>(J, inx + x, iny + y, w) : search_sample<false>(J, inx + x, iny + y, w);
            const int diff = jv - (int)ldsI[k * 64 + lane];
            se += (long long)(diff < 0 ? -diff : diff);
            x += xinc; y += yinc;
            if (x >= win) { x -= win; y++; }
        }
        se = vh_wave_sum_i64(se);
        err = lk_err_of((float)se, win);
    }
}

// grid = (max points, batch), block = one wavefront
__global__ __launch_bounds__(64) void k_lk(const void* job_tab, size_t tab_stride)
{
    const LKJob& job = lk_job_row(job_tab, tab_stride, blockIdx.y);
    int pt;
    float px, py;
    if (!lk_slot_start(job, (int)blockIdx.x, pt, px, py)) return;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int kmax = (job.win * job.win + 63) / 64;
    LKLevel lf{job.win, job.max_count, job.eps2, reinterpret_cast<short*>(smem + (size_t)kmax * 64 * 4), reinterpret_cast<int*>(smem), (int)threadIdx.x, 0, 0};
    LKResult R;
    lk_solve(job, px, py, lf, R);
    if (threadIdx.x == 0) {
        lk_store_track(job, pt, R.fx, R.fy, R.st, R.err, R.fbe);
        lk_add_stats(job, blockIdx.x, lf.n_iter, lf.n_setup);
    }
}


// =================================================================================================================
// v2: strip kernel.  One lane handles a horizontal strip of 4 window samples: the 4x7 (set-up) / 2x5 (iteration)
// pixel block of a strip comes from 3 aligned dword loads per row + v_alignbyte, the bilinear / gradient dot products
// run on v_dot2_i32_i16 with packed int16 pairs, the template lives in LDS as lane-private packed int16 quads
// (conflict-free ds_read_b64), and the exact wave sums are DPP row reductions of 16-bit halves (order independent).
// Integer arithmetic is identical to the per-sample kernel above, so results are bit-identical.
// =================================================================================================================

__device__ __forceinline__ int dpp_row_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true);  // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);  // row_mirror
    return v;
}
// exact wave-wide sum of per-lane int32 partials (|v| < 2^31) as int64, uniform result
__device__ __forceinline__ long long wave_sum_i32_wide(int v)
{
    int lo = dpp_row_sum(v & 0xffff), hi = dpp_row_sum(v >> 16);
    // rows 0..3 -> lane 63: row_bcast:15 adds the previous row's total to rows 1 and 3, row_bcast:31 the total of rows 0+1 to rows 2 and 3
    // (two DPP adds and one v_readlane per half instead of four v_readlane and three scalar adds)
    lo += __builtin_amdgcn_update_dpp(0, lo, 0x142, 0xa, 0xf, false);
    hi += __builtin_amdgcn_update_dpp(0, hi, 0x142, 0xa, 0xf, false);
    lo += __builtin_amdgcn_update_dpp(0, lo, 0x143, 0xc, 0xf, false);
    hi += __builtin_amdgcn_update_dpp(0, hi, 0x143, 0xc, 0xf, false);
    const int lo_t = __builtin_amdgcn_readlane(lo, 63), hi_t = __builtin_amdgcn_readlane(hi, 63);
    return (long long)hi_t * 65536ll + (long long)lo_t;
}

// Two (or three) such sums at once, transposing while folding: v_permlane32_swap puts the upper half-wave of one vector beside the lower half-wave
// of another, so ONE add folds two vectors 64 -> 32 lanes; v_permlane16_swap does the same for 16-lane rows.  The four 16-bit halves of two values
// end up in the four rows of one register: 3 swaps + 3 adds + 4 DPP adds + 4 readlanes instead of 24 DPP adds + 6 readlanes (gfx950 only).
__device__ __forceinline__ int fold32_pair(int a, int b)  // lanes 0..31: a[l] + a[l+32], lanes 32..63: b[l-32] + b[l]
{
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)a, (unsigned)b, false, false);
    return (int)(r[0] + r[1]);
}
__device__ __forceinline__ int fold16_pair(int a, int b)  // rows 0/2: a[row] + a[row+1], rows 1/3: b[row-1] + b[row]
{
    const auto r = __builtin_amdgcn_permlane16_swap((unsigned)a, (unsigned)b, false, false);
    return (int)(r[0] + r[1]);
}
__device__ __forceinline__ void wave_sum2_i32_wide(int a, int b, long long& sa, long long& sb)
{
    const int x = fold32_pair(a & 0xffff, a >> 16), y = fold32_pair(b & 0xffff, b >> 16);
    const int z = dpp_row_sum(fold16_pair(x, y));  // rows: a.lo, b.lo, a.hi, b.hi
    sa = (long long)__builtin_amdgcn_readlane(z, 32) * 65536ll + (long long)__builtin_amdgcn_readlane(z, 0);
    sb = (long long)__builtin_amdgcn_readlane(z, 48) * 65536ll + (long long)__builtin_amdgcn_readlane(z, 16);
}
__device__ __forceinline__ long long wave_sum1_i32_wide_swap(int a)
{
    const int x = fold32_pair(a & 0xffff, a >> 16);
    const int z = dpp_row_sum(fold16_pair(x, x));  // rows 0,1: a.lo, rows 2,3: a.hi
    return (long long)__builtin_amdgcn_readlane(z, 32) * 65536ll + (long long)__builtin_amdgcn_readlane(z, 0);
}
// The same two reductions for the pair form of the per-track arithmetic (vh_lk_shared.hpp; one wavefront per track): one more v_permlane32_swap puts the
// (lo, hi) halves of a value into the same lane, and the sum is converted where it lies -- no v_readlane, no recombination on the scalar unit.
// wave_sum2_f32_pair: ((float)sum a | (float)sum b), a pair; wave_sum1_f32_lane0: (float)sum a, of which LANE 0 is the contract (the caller reads it back
// as a scalar; the other lanes happen to hold the same float).
__device__ __forceinline__ float wide_rows_to_f32(int z)  // rows of z: the lo halves in rows 0 and 1, the hi halves in rows 2 and 3
{
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)z, (unsigned)z, false, false);  // r[0]: rows 0, 1, 0, 1 of z; r[1]: rows 2, 3, 2, 3
    return wide_halves_to_f32((int)r[0], (int)r[1]);
}
__device__ __forceinline__ float wave_sum2_f32_pair(int a, int b)
{
    const int x = fold32_pair(a & 0xffff, a >> 16), y = fold32_pair(b & 0xffff, b >> 16);
    return wide_rows_to_f32(dpp_row_sum(fold16_pair(x, y)));  // rows: a.lo, b.lo, a.hi, b.hi
}
__device__ __forceinline__ float wave_sum1_f32_lane0(int a)
{
    const int x = fold32_pair(a & 0xffff, a >> 16);
    return wide_rows_to_f32(dpp_row_sum(fold16_pair(x, x)));  // rows 0,1: a.lo, rows 2,3: a.hi
}

// wave-wide sum when 16 lanes of partials provably fit int32 (one 4-sample strip per lane: 16 * 4 * 8160 * 4080 < 2^31):
// one DPP chain per value instead of two
__device__ __forceinline__ long long wave_sum_i32_rows(int v)
{
    const int r = dpp_row_sum(v);
    return (long long)__builtin_amdgcn_readlane(r, 0) + (long long)__builtin_amdgcn_readlane(r, 16) +
           (long long)__builtin_amdgcn_readlane(r, 32) + (long long)__builtin_amdgcn_readlane(r, 48);
}


// NR rows x 8 bytes starting at pixel (gx, gy): lo = bytes 0..3, hi = bytes 4..7 of every row (interior fast path)
typedef const unsigned __attribute__((address_space(1)))* gptr_u32;  // global (not flat) loads

template <int NR>
__device__ __forceinline__ void load_rows_fast(const ImgDesc& im, int gx, int gy, unsigned* lo, unsigned* hi)
{
    const uint8_t* base = im.p + (ptrdiff_t)gy * im.stride + gx;
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(base + (ptrdiff_t)r * im.stride);
        const unsigned sh = (unsigned)(a & 3);
        gptr_u32 ap = (gptr_u32)(a - sh);
        const unsigned d0 = ap[0], d1 = ap[1], d2 = ap[2];
        lo[r] = __builtin_amdgcn_alignbyte(d1, d0, sh);
        hi[r] = __builtin_amdgcn_alignbyte(d2, d1, sh);
    }
}
// the same block through REFLECT_101 byte loads (windows that touch the border)
template <int NR, int NC>
__device__ __forceinline__ void load_rows_slow(const ImgDesc& im, int gx, int gy, unsigned* lo, unsigned* hi)
{
#pragma unroll
    for (int r = 0; r < NR; r++) {
        unsigned l = 0, h = 0;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const unsigned v = (unsigned)pix_r(im, gx + c, gy + r);
            if (c < 4) l |= v << (8 * c);
            else h |= v << (8 * (c - 4));
        }
        lo[r] = l; hi[r] = h;
    }
}
__device__ __forceinline__ int byte_of(unsigned lo, unsigned hi, int c) { return c < 4 ? (int)((lo >> (8 * c)) & 0xff) : (int)((hi >> (8 * (c - 4))) & 0xff); }

struct StripWeights {
    unsigned wt, wb;  // packed (w00,w01), (w10,w11)
    int w00, w01, w10, w11;
};
__device__ __forceinline__ StripWeights strip_weights(const Win& w)
{
    StripWeights s;
    s.w00 = w.w00; s.w01 = w.w01; s.w10 = w.w10; s.w11 = w.w11;
    s.wt = pack16(w.w00, w.w01); s.wb = pack16(w.w10, w.w11);
    return s;
}

// packed horizontal neighbours (b_c, b_{c+1}), c = 0..3, of one row (lo = bytes 0..3, hi = byte 4..)
__device__ __forceinline__ void strip_row_pairs(unsigned lo, unsigned hi, unsigned* t)
{
    t[0] = __builtin_amdgcn_perm(0u, lo, 0x0c010c00u);
    t[1] = __builtin_amdgcn_perm(0u, lo, 0x0c020c01u);
    t[2] = __builtin_amdgcn_perm(0u, lo, 0x0c030c02u);
    t[3] = __builtin_amdgcn_perm(hi, lo, 0x0c040c03u);
}
// bilinear x32 samples of the 4 strip positions from the packed pairs of the top and bottom row
__device__ __forceinline__ void strip_bilinear_pairs(const unsigned* t, const unsigned* b, const StripWeights& w, unsigned& p01, unsigned& p23)
{
    // descale(acc, 9) = (acc + 256) >> 9 = upper half of (acc + 256) << 7  (acc < 2^22): one v_lshl_add per sample, one v_perm per pair
    int v[4];
#pragma unroll
    for (int c = 0; c < 4; c++)
        v[c] = (dot2(b[c], w.wb, dot2_first(t[c], w.wt)) << (16 - (W_BITS - 5))) + (1 << (W_BITS - 5 - 1 + 16 - (W_BITS - 5)));
    p01 = pack_hi16(v[0], v[1]);
    p23 = pack_hi16(v[2], v[3]);
}
// bilinear x32 samples of the 4 strip positions from 2 rows (lo,hi): returns packed pairs (v0,v1), (v2,v3)
__device__ __forceinline__ void strip_bilinear(const unsigned* lo, const unsigned* hi, const StripWeights& w, unsigned& p01, unsigned& p23)
{
    unsigned t[4], b[4];
    strip_row_pairs(lo[0], hi[0], t);
    strip_row_pairs(lo[1], hi[1], b);
    strip_bilinear_pairs(t, b, w, p01, p23);
}


// set-up of one strip from its 4x7 pixel block: template samples (x32), Scharr gradients, structure-tensor partials
// Interior windows: bilinear interpolation and the Scharr operator are both integer-linear, so
//   sum_k w_k * Scharr(P)[pos + k]  ==  Scharr(V)[pos]   with   V[pos] = sum_k w_k * P[pos + k]   (no rounding before the descale)
// V is needed on a 3 x 6 block for the 4 samples of a strip (18 x 2 v_dot2 on packed byte pairs); the template sample itself
// is descale(V, 9).  Exactly the same integers as interpolating the gradient image, at ~55 % of the instructions.
// the six packed byte pairs (c, c+1), c = 0..5, of one 8-byte patch row
__device__ __forceinline__ void setup_row_pairs(unsigned lo, unsigned hi, unsigned* pr)
{
    pr[0] = __builtin_amdgcn_perm(0u, lo, 0x0c010c00u);
    pr[1] = __builtin_amdgcn_perm(0u, lo, 0x0c020c01u);
    pr[2] = __builtin_amdgcn_perm(0u, lo, 0x0c030c02u);
    pr[3] = __builtin_amdgcn_perm(hi, lo, 0x0c040c03u);
    pr[4] = __builtin_amdgcn_perm(0u, hi, 0x0c010c00u);
    pr[5] = __builtin_amdgcn_perm(0u, hi, 0x0c020c01u);
}
// one row of V from the pairs of two consecutive patch rows
__device__ __forceinline__ void setup_v_row(const unsigned* top, const unsigned* bot, unsigned wt, unsigned wb, int* V)
{
#pragma unroll
    for (int c = 0; c < 6; c++) V[c] = dot2(bot[c], wb, dot2_first(top[c], wt));
}
// template samples, gradients and structure-tensor partials of one strip from its three V rows
__device__ __forceinline__ void setup_from_v(const int* V0, const int* V1, const int* V2, int cnt, uint2* tI, uint2* tX, uint2* tY, int slot,
                                             int& a11, int& a12, int& a22)
{
    // gradients x4 with the rounding folded in (column c of S carries 2^14 c, so S[c+2] - S[c] brings 4 * 2^13), descale + int16 packing by
    // v_perm of the upper halves, zeroing of the samples beyond the window edge by the selector (see setup_from_hg)
    int S4[6], D[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        S4[c] = mad24_v<40>(V1[c], mad24_s<12>(V0[c] + V2[c], c << W_BITS));  // every V fits 23 bits
        D[c] = V2[c] - V0[c];
    }
    int iv[4], ix[4], iy[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        iv[c] = (V1[c + 1] << (16 - (W_BITS - 5))) + (1 << (W_BITS - 5 - 1 + 16 - (W_BITS - 5)));
        ix[c] = S4[c + 2] - S4[c];
        iy[c] = mad24_v<40>(D[c + 1], mad24_s<12>(D[c] + D[c + 2], 4 << (W_BITS - 1)));
    }
    const unsigned sel01 = cnt >= 2 ? 0x07060302u : 0x0c0c0302u, sel23 = cnt >= 4 ? 0x07060302u : (cnt == 3 ? 0x0c0c0302u : 0x0c0c0c0cu);
    const uint2 vI = make_uint2(__builtin_amdgcn_perm((unsigned)iv[1], (unsigned)iv[0], sel01), __builtin_amdgcn_perm((unsigned)iv[3], (unsigned)iv[2], sel23));
    const uint2 vX = make_uint2(__builtin_amdgcn_perm((unsigned)ix[1], (unsigned)ix[0], sel01), __builtin_amdgcn_perm((unsigned)ix[3], (unsigned)ix[2], sel23));
    const uint2 vY = make_uint2(__builtin_amdgcn_perm((unsigned)iy[1], (unsigned)iy[0], sel01), __builtin_amdgcn_perm((unsigned)iy[3], (unsigned)iy[2], sel23));
    tI[slot] = vI; tX[slot] = vX; tY[slot] = vY;
    a11 = dot2(vX.y, vX.y, dot2(vX.x, vX.x, a11));
    a12 = dot2(vX.y, vY.y, dot2(vX.x, vY.x, a12));
    a22 = dot2(vY.y, vY.y, dot2(vY.x, vY.x, a22));
}

// Rolling form for a vertical run of strips: per V row keep its horizontal differences H[c] = V[c+2] - V[c] and its
// horizontally smoothed values G[c] = 3 (V[c] + V[c+2]) + 10 V[c+1], c = 0..3.  Then (exact integer identities)
//   Scharr_x = 3 (H0 + H2) + 10 H1,   Scharr_y = G2 - G0,   so a new strip costs one H row and one G row, not a 3 x 6 block of S / D
// Both gradients are kept x4 with the descale rounding folded in, so that descale(., 14) + int16 packing is the upper half of the word
// (pack_hi16): G4 row g carries the addend 2^14 * g, hence G4[g+2] - G4[g] = 4 (G2 - G0) + 4 * 2^13; |4 * Scharr| < 2^29.
__device__ __forceinline__ void setup_hg_row(const int* V, int* H, int* G4, int g)
{
#pragma unroll
    for (int c = 0; c < 4; c++) {
        H[c] = V[c + 2] - V[c];
        G4[c] = mad24_v<40>(V[c + 1], mad24_s<12>(V[c] + V[c + 2], g << W_BITS));  // every V fits 22 bits
    }
}
// vmask: 0xffffffff for a strip inside the window, 0 for a strip of the last run that hangs below it (stored as zeros)
// sel01 / sel23: the v_perm selectors that pack the two sample pairs -- 0x07060302 keeps both upper halves, 0x0c0c0302 zeroes the second sample,
// 0x0c0c0c0c both: samples beyond the window edge and strips below the window cost no masking instruction
__device__ __forceinline__ void setup_from_hg(const int* H0, const int* H1, const int* H2, const int* G0, const int* G2, const int* Vmid, unsigned sel01,
                                              unsigned sel23, uint2* tI, uint2* tX, uint2* tY, int slot, int& a11, int& a12, int& a22)
{
    int iv[4], ix[4], iy[4];  // the wanted int16 in the upper half of each
#pragma unroll
    for (int c = 0; c < 4; c++) {
        iv[c] = (Vmid[c] << (16 - (W_BITS - 5))) + (1 << (W_BITS - 5 - 1 + 16 - (W_BITS - 5)));
        ix[c] = mad24_v<40>(H1[c], mad24_s<12>(H0[c] + H2[c], 4 << (W_BITS - 1)));
        iy[c] = G2[c] - G0[c];
    }
    const uint2 vI = make_uint2(pack_hi16(iv[0], iv[1]), pack_hi16(iv[2], iv[3]));  // enters only through products with the (masked) gradients
    const uint2 vX = make_uint2(__builtin_amdgcn_perm((unsigned)ix[1], (unsigned)ix[0], sel01), __builtin_amdgcn_perm((unsigned)ix[3], (unsigned)ix[2], sel23));
    const uint2 vY = make_uint2(__builtin_amdgcn_perm((unsigned)iy[1], (unsigned)iy[0], sel01), __builtin_amdgcn_perm((unsigned)iy[3], (unsigned)iy[2], sel23));
    tI[slot] = vI; tX[slot] = vX; tY[slot] = vY;
    a11 = dot2(vX.y, vX.y, dot2(vX.x, vX.x, a11));
    a12 = dot2(vX.y, vY.y, dot2(vX.x, vY.x, a12));
    a22 = dot2(vY.y, vY.y, dot2(vY.x, vY.x, a22));
}

__device__ __forceinline__ void strip_setup_linear(const unsigned* lo, const unsigned* hi, const Win& w0, int cnt, uint2* tI, uint2* tX,
                                                   uint2* tY, int slot, int& a11, int& a12, int& a22)
{
    const unsigned wt = pack16(w0.w00, w0.w01), wb = pack16(w0.w10, w0.w11);
    unsigned pr[4][6];  // pr[r][c] = (byte c, byte c+1) of row r as a packed int16 pair
#pragma unroll
    for (int r = 0; r < 4; r++) setup_row_pairs(lo[r], hi[r], pr[r]);
    int V[3][6];
#pragma unroll
    for (int r = 0; r < 3; r++) setup_v_row(pr[r], pr[r + 1], wt, wb, V[r]);
    setup_from_v(V[0], V[1], V[2], cnt, tI, tX, tY, slot, a11, a12, a22);
}

template <bool FAST>
__device__ __forceinline__ void strip_setup(const unsigned* lo, const unsigned* hi, const Win& w0, const ImgDesc& I, int ipx, int ipy, int x,
                                            int y, int cnt, uint2* tI, uint2* tX, uint2* tY, int slot, int& a11, int& a12, int& a22)
{
    if constexpr (FAST) {
        strip_setup_linear(lo, hi, w0, cnt, tI, tX, tY, slot, a11, a12, a22);
        return;
    }
    constexpr bool fast = FAST;
            // vertical [3 10 3] smooth / [-1 0 1] difference for the two derivative rows, 7 columns
            int sm[2][7], df[2][7];
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int c = 0; c < 7; c++) {
                    const int t = byte_of(lo[r], hi[r], c), m = byte_of(lo[r + 1], hi[r + 1], c), b = byte_of(lo[r + 2], hi[r + 2], c);
                    sm[r][c] = (t + b) * 3 + m * 10;
                    df[r][c] = b - t;
                }
            int gx[2][5], gy[2][5];
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    gx[r][c] = sm[r][c + 2] - sm[r][c];
                    gy[r][c] = (df[r][c] + df[r][c + 2]) * 3 + df[r][c + 1] * 10;
                    if (!fast) {  // the derivative image is constant 0 outside the level
                        const int ax = ipx + x + c, ay = ipy + y + r;
                        if (ax < 0 || ax >= I.w || ay < 0 || ay >= I.h) { gx[r][c] = 0; gy[r][c] = 0; }
                    }
                }
            int iv[4], ix[4], iy[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int q00 = byte_of(lo[1], hi[1], c + 1), q01 = byte_of(lo[1], hi[1], c + 2);
                const int q10 = byte_of(lo[2], hi[2], c + 1), q11 = byte_of(lo[2], hi[2], c + 2);
                // every factor fits 24 signed bits (|pixel| <= 255, |gradient| <= 4080, weights <= 2^14): full-rate v_mad_i32_i24
                iv[c] = vh_descale(__mul24(q00, w0.w00) + __mul24(q01, w0.w01) + __mul24(q10, w0.w10) + __mul24(q11, w0.w11), W_BITS - 5);
                ix[c] = vh_descale(__mul24(gx[0][c], w0.w00) + __mul24(gx[0][c + 1], w0.w01) + __mul24(gx[1][c], w0.w10) + __mul24(gx[1][c + 1], w0.w11), W_BITS);
                iy[c] = vh_descale(__mul24(gy[0][c], w0.w00) + __mul24(gy[0][c + 1], w0.w01) + __mul24(gy[1][c], w0.w10) + __mul24(gy[1][c + 1], w0.w11), W_BITS);
                if (c >= cnt) { iv[c] = 0; ix[c] = 0; iy[c] = 0; }
            }
            const uint2 vI = make_uint2(pack16(iv[0], iv[1]), pack16(iv[2], iv[3]));
            const uint2 vX = make_uint2(pack16(ix[0], ix[1]), pack16(ix[2], ix[3]));
            const uint2 vY = make_uint2(pack16(iy[0], iy[1]), pack16(iy[2], iy[3]));
            tI[slot] = vI; tX[slot] = vX; tY[slot] = vY;
            a11 = dot2(vX.y, vX.y, dot2(vX.x, vX.x, a11));
            a12 = dot2(vX.y, vY.y, dot2(vX.x, vY.x, a12));
            a22 = dot2(vY.y, vY.y, dot2(vY.x, vY.x, a22));
}

template <int WIN_T>
__device__ void lk_level_strip(const ImgDesc I, const ImgDesc J, int win_rt, int level, int top_level, int max_count, double eps2,
                               float p0x, float p0y, float& nxo, float& nyo, int& status, float& err, uint2* tI, uint2* tX, uint2* tY,
                               int lane, int& n_iter, int& n_setup, bool want_err)
{
    const int win = WIN_T ? WIN_T : win_rt;
    const int spr = (win + 3) >> 2;   // strips per window row
    const int nstrips = spr * win;
    const int reach = 4 * spr + 8;    // bytes from the first one that the aligned row reads of a strip row may touch (lk_block_inside)
    LKStart s;
    if (!lk_level_start(p0x, p0y, level, top_level, win, I, nxo, nyo, status, err, s)) return;
    const float half = s.half;
    const int ipx = s.ipx, ipy = s.ipy;
    float nx = s.nx, ny = s.ny;
    const Win w0 = bilinear_weights(__fsub_rn(s.px, (float)ipx), __fsub_rn(s.py, (float)ipy));
    n_setup++;
    // strip coordinates of this lane: s = lane + 64 k -> (row, 4*col); advanced incrementally
    const int j_first = lane % spr, y_first = lane / spr;
    const int jinc = 64 % spr, yinc = 64 / spr;

    int a11 = 0, a12 = 0, a22 = 0;
    {
        // interior window: the patch [ipx-1, ipx+win+1] x [ipy-1, ipy+win+1] lies inside the level (V identity), and so do the aligned 12-byte row
        // reads of a strip (and the padding samples of the last strip)
        const bool fast = lk_block_inside(I, ipx - 1, ipy - 1, win + 3, reach);
        if constexpr (WIN_T != 0 && ((((WIN_T + 3) >> 2) * WIN_T + 63) / 64) <= 2) {
            constexpr int SPR = (WIN_T + 3) >> 2, NS = SPR * WIN_T, KMAX = (NS + 63) / 64, G = KMAX < 3 ? KMAX : 3;
#pragma unroll
            for (int kb = 0; kb < KMAX; kb += G) {
                unsigned lo[G][4], hi[G][4];
#pragma unroll
                for (int g = 0; g < G; g++) {
                    const int k = kb + g, s = lane + 64 * k;
                    if (k < KMAX && s < NS) {
                        const int y = s / SPR, x = 4 * (s - y * SPR);
                        if (fast) load_rows_fast<4>(I, ipx + x - 1, ipy + y - 1, lo[g], hi[g]);
                        else load_rows_slow<4, 7>(I, ipx + x - 1, ipy + y - 1, lo[g], hi[g]);
                    }
                }
#pragma unroll
                for (int g = 0; g < G; g++) {
                    const int k = kb + g, s = lane + 64 * k;
                    if (k < KMAX && s < NS) {
                        const int y = s / SPR, x = 4 * (s - y * SPR), cnt = min(4, WIN_T - x);
                        if (fast) strip_setup<true>(lo[g], hi[g], w0, I, ipx, ipy, x, y, cnt, tI, tX, tY, k * 64 + lane, a11, a12, a22);
                        else strip_setup<false>(lo[g], hi[g], w0, I, ipx, ipy, x, y, cnt, tI, tX, tY, k * 64 + lane, a11, a12, a22);
                    }
                }
            }
        } else {
            int j = j_first, y = y_first, k = 0;
            for (int s = lane; s < nstrips; s += 64, k++) {
                const int x = 4 * j, cnt = min(4, win - x);
                unsigned lo[4], hi[4];
                if (fast) {
                    load_rows_fast<4>(I, ipx + x - 1, ipy + y - 1, lo, hi);
                    strip_setup<true>(lo, hi, w0, I, ipx, ipy, x, y, cnt, tI, tX, tY, k * 64 + lane, a11, a12, a22);
                } else {
                    load_rows_slow<4, 7>(I, ipx + x - 1, ipy + y - 1, lo, hi);
                    strip_setup<false>(lo, hi, w0, I, ipx, ipy, x, y, cnt, tI, tX, tY, k * 64 + lane, a11, a12, a22);
                }
                j += jinc; y += yinc;
                if (j >= spr) { j -= spr; y++; }
            }
        }
    }
    constexpr bool ROWSAFE = WIN_T != 0 && ((WIN_T + 3) >> 2) * WIN_T <= 64;  // one strip per lane
    const long long sA11 = ROWSAFE ? wave_sum_i32_rows(a11) : wave_sum_i32_wide(a11);
    const long long sA12 = ROWSAFE ? wave_sum_i32_rows(a12) : wave_sum_i32_wide(a12);
    const long long sA22 = ROWSAFE ? wave_sum_i32_rows(a22) : wave_sum_i32_wide(a22);
    LKSys S;
    if (!lk_system(sA11, sA12, sA22, win, S)) {
        if (level == 0) status = 0;
        return;
    }

    float pdx = 0.f, pdy = 0.f;
    for (int it = 0; it < max_count; it++) {
        const int inx = vh_floor(nx), iny = vh_floor(ny);
        if (lk_outside(inx, iny, win, J)) {
            if (level == 0) status = 0;
            break;
        }
        const StripWeights w = strip_weights(bilinear_weights(__fsub_rn(nx, (float)inx), __fsub_rn(ny, (float)iny)));
        const bool fast = lk_block_inside(J, inx, iny, win + 1, reach);
        n_iter++;
        int b1 = 0, b2 = 0;
        if constexpr (WIN_T != 0 && ((((WIN_T + 3) >> 2) * WIN_T + 63) / 64) <= 2) {
            // small compile-time window: fully unrolled, all loads of a group of strips issued before the first use so a
            // Newton iteration pays the memory latency once per group instead of once per strip
            constexpr int SPR = (WIN_T + 3) >> 2, NS = SPR * WIN_T, KMAX = (NS + 63) / 64, G = KMAX < 6 ? KMAX : 6;
#pragma unroll
            for (int kb = 0; kb < KMAX; kb += G) {
                unsigned lo[G][2], hi[G][2];
#pragma unroll
                for (int g = 0; g < G; g++) {
                    const int k = kb + g, s = lane + 64 * k;
                    if (k < KMAX && s < NS) {
                        const int y = s / SPR, j = s - y * SPR;
                        if (fast) load_rows_fast<2>(J, inx + 4 * j, iny + y, lo[g], hi[g]);
                        else load_rows_slow<2, 5>(J, inx + 4 * j, iny + y, lo[g], hi[g]);
                    }
                }
#pragma unroll
                for (int g = 0; g < G; g++) {
                    const int k = kb + g, s = lane + 64 * k;
                    if (k < KMAX && s < NS) {
                        unsigned p01, p23;
                        strip_bilinear(lo[g], hi[g], w, p01, p23);
                        const uint2 vI = tI[k * 64 + lane], vX = tX[k * 64 + lane], vY = tY[k * 64 + lane];
                        const unsigned d01 = __builtin_bit_cast(unsigned, as_s2(p01) - as_s2(vI.x));
                        const unsigned d23 = __builtin_bit_cast(unsigned, as_s2(p23) - as_s2(vI.y));
                        b1 = dot2(d23, vX.y, dot2(d01, vX.x, b1));
                        b2 = dot2(d23, vY.y, dot2(d01, vY.x, b2));
                    }
                }
            }
        } else {
            int j = j_first, y = y_first, k = 0;
            for (int s = lane; s < nstrips; s += 64, k++) {
                unsigned lo[2], hi[2];
                if (fast) load_rows_fast<2>(J, inx + 4 * j, iny + y, lo, hi);
                else load_rows_slow<2, 5>(J, inx + 4 * j, iny + y, lo, hi);
                unsigned p01, p23;
                strip_bilinear(lo, hi, w, p01, p23);
                const uint2 vI = tI[k * 64 + lane], vX = tX[k * 64 + lane], vY = tY[k * 64 + lane];
                const unsigned d01 = __builtin_bit_cast(unsigned, as_s2(p01) - as_s2(vI.x));
                const unsigned d23 = __builtin_bit_cast(unsigned, as_s2(p23) - as_s2(vI.y));
                // unused samples of the last strip of a row carry Ix = Iy = 0, so they add nothing
                b1 = dot2(d23, vX.y, dot2(d01, vX.x, b1));
                b2 = dot2(d23, vY.y, dot2(d01, vY.x, b2));
                j += jinc; y += yinc;
                if (j >= spr) { j -= spr; y++; }
            }
        }
        const long long sb1 = ROWSAFE ? wave_sum_i32_rows(b1) : wave_sum_i32_wide(b1);
        const long long sb2 = ROWSAFE ? wave_sum_i32_rows(b2) : wave_sum_i32_wide(b2);
        if (lk_step(S, sb1, sb2, half, it, eps2, nx, ny, nxo, nyo, pdx, pdy)) break;
    }

    if (status && level == 0) {
        float fx, fy;
        int inx, iny;
        if (!lk_final_origin(nxo, nyo, half, win, J, fx, fy, inx, iny)) { status = 0; return; }
        if (!want_err) return;  // err is discarded by the caller (KLT.py:83 `pa, v, _`): only the bounds rule matters
        const StripWeights w = strip_weights(bilinear_weights(__fsub_rn(fx, (float)inx), __fsub_rn(fy, (float)iny)));
        const bool fast = lk_block_inside(J, inx, iny, win + 1, reach);
        int se = 0;
        int j = j_first, y = y_first, k = 0;
        for (int s = lane; s < nstrips; s += 64, k++) {
            const int cnt = min(4, win - 4 * j);
            unsigned lo[2], hi[2];
            if (fast) load_rows_fast<2>(J, inx + 4 * j, iny + y, lo, hi);
            else load_rows_slow<2, 5>(J, inx + 4 * j, iny + y, lo, hi);
            unsigned p01, p23;
            strip_bilinear(lo, hi, w, p01, p23);
            const uint2 vI = tI[k * 64 + lane];
            const short2v d01 = as_s2(p01) - as_s2(vI.x), d23 = as_s2(p23) - as_s2(vI.y);
            const int d[4] = {d01.x, d01.y, d23.x, d23.y};
#pragma unroll
            for (int c = 0; c < 4; c++) se += c < cnt ? (d[c] < 0 ? -d[c] : d[c]) : 0;
            j += jinc; y += yinc;
            if (j >= spr) { j -= spr; y++; }
        }
        const long long sse = ROWSAFE ? wave_sum_i32_rows(se) : wave_sum_i32_wide(se);
        err = lk_err_of(i64_to_f32(sse), win);
    }
}


// XCD-aware, stream-interleaved block order of the batched LK launches (round 4).  The dispatcher deals consecutive workgroups (linear id
// L = y gridDim.x + x) round-robin to the 8 XCDs, in order.  With y = stream and x = track block, a stream's tracks are spread over all eight L2s, each L2
// sees the pyramids of every stream in flight, and the streams run one after the other.  Re-indexed: streams are taken in sets of G (G gridDim.x
// consecutive ids), id q of a set -> stream q mod G of the set, track block q / G.  With G a multiple of 8 every workgroup of stream y has L mod 8 == y mod 8:
// a stream lives in ONE L2 (its pyramid levels are read again and again by neighbouring tracks, both directions, every level and iteration), and G / 8
// streams share an XCD at any time, which evens out their run times for the in-order dispatcher.  (A last set of m < G streams is dealt q mod m: valid,
// XCD-pure only if m is a multiple of 8.)  Pure re-indexing: every (x, y) is produced exactly once, results are unchanged.
// Measured (tools/exp/lko_group_sweep*.sh, C2, one box): coarse k_lk_o at 256 streams 632 / 1076 us (natural order) -> 524 / 935 us for G = 64 .. 256
// (G = 31 / 63: 565 / 960; G = 8, ONE stream per XCD: 1169 / 1369 -- the XCDs drift apart and the in-order dispatcher waits for the slowest); fine k_lk3
// 3830 -> 3661 us at G = 8, 3675 at 16, 3725 at 32.  Small batches gain most: 8 streams 13.2 k -> 18.2 k frames/s, 32 streams 26.4 k -> 34.4 k.
// Most of it is the INTERLEAVING (resident workgroups come from many streams instead of one or two, all at the same pyramid level of the same images);
// the same order rotated off the XCDs (LK_GRP_ROTATE) keeps 95-98 %: 8 streams 17.9 k against 18.3 k pinned, 256 streams 40.9 k against 41.6 k.
#ifndef LK_XCD_REMAP
#define LK_XCD_REMAP 1
#endif
#define LK_GRP_ROTATE 0x10000u  // flag in the group argument: stream (q + q / m) mod m instead of q mod m -- interleaved, but NOT pinned to an XCD
template <bool REMAP>
__device__ __forceinline__ void lk_block_xy(unsigned& bx, unsigned& by, unsigned grp = 8u)
{
    bx = blockIdx.x; by = blockIdx.y;
    const unsigned G = grp & 0xffffu;
    if (REMAP && LK_XCD_REMAP && gridDim.y > 1 && G > 1u) {
        const unsigned nx = gridDim.x, L = blockIdx.y * nx + blockIdx.x;
        const unsigned set = L / (G * nx), q = L - set * G * nx;
        const unsigned m = min(G, gridDim.y - set * G);
        const unsigned xq = q / m;
        by = set * G + ((q - xq * m) + ((grp & LK_GRP_ROTATE) ? xq : 0u)) % m;
        bx = xq;
    }
}
static_assert(LK_GRP_ROTATE == LK_GROUP_ROTATE, "the group argument of a launch is made by lk_group_arg (vh_step_plan.hpp)");

// The level functor of k_lk_strip (see lk_track) only forwards to the function above.  With the level body as the functor's own operator() --
// the form of the other four kernels -- hipcc allocates k_lk_strip<15> differently: 472 instead of 358 v_readlane / v_writelane of parked scalar
// registers, +340 instructions, and a coarse launch of one stream took 20.89 / 28.21 us against the parent's 20.52 / 27.88 us (profiles/lk_shared/ab.json, first_try)
template <int WIN_T>
struct LKStripLevel {
    int win_rt, max_count;
    double eps2;
    uint2 *tI, *tX, *tY;
    int lane, n_iter, n_setup;
    __device__ __forceinline__ void operator()(const ImgDesc& I, const ImgDesc& J, int level, int top_level, float p0x, float p0y, float& nxo, float& nyo,
                                               int& status, float& err, bool want_err)
    {
        lk_level_strip<WIN_T>(I, J, win_rt, level, top_level, max_count, eps2, p0x, p0y, nxo, nyo, status, err, tI, tX, tY, lane, n_iter, n_setup, want_err);
    }
};

template <int WIN_T>
__global__ __launch_bounds__(64) void k_lk_strip(const void* job_tab, size_t tab_stride)
{
    unsigned blk_x, blk_y;
    lk_block_xy<false>(blk_x, blk_y);
    const LKJob& job = lk_job_row(job_tab, tab_stride, blk_y);
    int pt;
    float px, py;
    if (!lk_slot_start(job, (int)blk_x, pt, px, py)) return;
    const int win = WIN_T ? WIN_T : job.win;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int kmax = (((win + 3) >> 2) * win + 63) / 64;
    uint2* tI = reinterpret_cast<uint2*>(smem);
    LKStripLevel<WIN_T> lf{win, job.max_count, job.eps2, tI, tI + kmax * 64, tI + 2 * kmax * 64, (int)threadIdx.x, 0, 0};
    LKResult R;
    lk_solve(job, px, py, lf, R);
    if (threadIdx.x == 0) {
        lk_store_track(job, pt, R.fx, R.fy, R.st, R.err, R.fbe);
        lk_add_stats(job, blk_x, lf.n_iter, lf.n_setup);
    }
}


// =================================================================================================================
// v3: LDS-staged kernel for the two windows the tracker uses (15x15 coarse, 51x51 fine).
// One workgroup of NW wavefronts per track.  Per level and direction the template patch ((WIN+3)^2 pixels of the
// previous image) and a search region ((WIN+1+2M)^2 pixels of the next image around the predicted position) are staged
// into LDS with ONE batch of global loads (REFLECT_101 applied while staging, so the compute loops have no border
// cases); set-up, every Newton iteration and the err pass then read LDS only.  The search region is re-staged if the
// window drifts more than M pixels.  Strip arithmetic, exact sums and control flow are those of the kernels above
// (bit-identical results); with NW > 1 the per-wave sums are combined through LDS.
// =================================================================================================================
template <int WIN, int NW, int M>
struct LK3 {
    static constexpr int T = 64 * NW;
    static constexpr int SPR = (WIN + 3) >> 2;
    static constexpr int NS = SPR * WIN;
    // lane -> (strip column j, run q): every lane owns K vertically consecutive strips of one column, so consecutive
    // strips share patch rows, byte pairs and V rows in registers (a strip's set-up needs 1 new V row instead of 3, a
    // Newton iteration 1 new search row instead of 2)
    // SPLIT (one wavefront, 51x51): 13 strip columns x 4 runs fill 52 lanes only, and 13 strips per lane cover 52 rows.  Instead every lane owns 11
    // strips: lanes 0..51 (column, run) as before with runs of 11 rows = rows 0..43; the 7 rows left (44..50) go to lanes 52..63 -- lane 52+c takes
    // column c < 12 in its first KA = 7 strips; the 7 strips of column 12 go ONE each to the last strip slot of lanes 52..58, whose slots 7..9 walk the
    // three rows above it so that the rolling state (two V rows in the set-up, one row of byte pairs in an iteration) is valid when slot 10 needs it.
    // Slots that hold no strip are kept as zeros by their selector (below).  663 strips in 64 x 11 slots instead of 52 x 13: -2 strips per lane.
    static constexpr bool SPLIT = (NW == 1 && WIN == 51);
    static constexpr int RUNS = SPLIT ? 4 : T / SPR;
    static constexpr int K = SPLIT ? 11 : (WIN + RUNS - 1) / RUNS;
    static constexpr int KA = SPLIT ? WIN - RUNS * K : K;  // strips of a lane's first segment
    static_assert(!SPLIT || (KA == 7 && SPR == 13 && RUNS * SPR + SPR - 1 <= T && KA <= T - RUNS * SPR && K - KA == 4), "split lane mapping");
    static constexpr int PI_ROWS = WIN + 3;                                   // template patch rows
    static constexpr int PI_PITCH = ((4 * (SPR - 1) + 8 + 3) / 4) * 4;        // bytes read per patch row, dword multiple
    static constexpr int RJ = WIN + 1 + 2 * M;                                // search region rows / cols
    static constexpr int PJ_WIDTH = ((2 * M + 4 * (SPR - 1)) >> 2) * 4 + 8;   // a row read takes two dwords
    static constexpr int PJ_PITCH = PJ_WIDTH + 4;                                // odd dword pitch (LDS banks)
    // The template of a lane's K strips (its Scharr gradients, 2 x 8 bytes per strip; the samples themselves enter only through the sums c, see
    // LK3Level) stays in REGISTERS for the whole level: LDS then
    // holds the two image regions only (~7.7 KB per workgroup for 51x51) and the VGPR file, not LDS, bounds the occupancy.  With the template in
    // LDS (24.5 KB per workgroup: 6 workgroups = 3 wavefronts per SIMD) the kernel lost 14 % per workgroup of occupancy taken away.
    // Every lane runs all K strips of its run with NO per-strip branch: strips below the window (the tail of the last run(s)) are computed from
    // whatever the padded buffers hold and kept as ZEROS, so they add nothing to any window sum in the set-up or in the Newton iterations.
    // (Branching on `y < WIN` per strip split the unrolled K loop into exec-masked blocks joined by register moves.)
    static constexpr int LANES = SPLIT ? T : RUNS * SPR;         // active lanes
    static constexpr int PAD_ROWS = SPLIT ? 0 : RUNS * K - WIN;  // window rows the last run(s) hang over the bottom edge
    static constexpr int OFF_PI = 0;
    static constexpr int OFF_PJ = OFF_PI + (PI_ROWS + PAD_ROWS) * PI_PITCH + 8;
    static constexpr int OFF_RED = ((OFF_PJ + (RJ + PAD_ROWS) * PJ_PITCH + 16 + 15) / 16) * 16;
    static constexpr int MAX_TPW = 8;                           // launch slots one workgroup may solve one after the other (k_lk3)
    static constexpr int REC_DW = 6;                            // dwords of a result record: point, fx, fy, status, err, fbe
    static constexpr int OFF_RES = OFF_RED + 2 * NW * 4 * 8;   // their result records, written out after the last one
    // The lane map: what a thread's place in the workgroup alone decides -- its strip column(s) and first row(s), and with them its addresses in the
    // two staged regions and the v_perm selectors that pack (and mask) its gradient pairs.  Slots fall into selector classes: SPLIT 0 = [0, KA),
    // 1 = [KA, K-1), 2 = K-1; otherwise 0 = the slots that always lie inside the window, 1 = the last PAD_ROWS slots of a run (below the window in the
    // last run(s)).  k_lk3 writes the map to LDS once per workgroup (OFF_TAB), LK3Level reads every word back where it is first needed (LDS reads take no
    // VALU slot, and a word read late is not held through the set-up's register peak).  Eleven arrays of one dword per thread (word i of thread t at
    // OFF_TAB + 4 * (i * T + t)): every read goes through the ONE address 4 * t with the array in the offset field, two words are one ds_read2st64_b32,
    // and reads that are far apart in the code cannot be merged into one early 16-byte read.  TAB_COL: the lane's byte offsets in the patch (set-up),
    // TAB_LC: in the search region (iterations), TAB_SEL + 2 c: the selectors of class c (set-up, from the first slot of the class), TAB_JR: columns
    // and rows as numbers (border set-up and err pass)
    struct Lane {
        int jA, rA, jB, rB;
        bool on;
        unsigned s01[3], s23[3];
    };
    static constexpr unsigned SEL_NONE = 0x0c0c0c0cu;
    static constexpr unsigned sel01_of(int cnt) { return cnt >= 2 ? 0x07060302u : (cnt == 1 ? 0x0c0c0302u : SEL_NONE); }
    static constexpr unsigned sel23_of(int cnt) { return cnt >= 4 ? 0x07060302u : (cnt == 3 ? 0x0c0c0302u : SEL_NONE); }
    static constexpr int NCLS = SPLIT ? 3 : 2;
    static constexpr int slot_cls(int k) { return SPLIT ? (k < KA ? 0 : (k < K - 1 ? 1 : 2)) : (k < K - PAD_ROWS ? 0 : 1); }
    static constexpr Lane lane(int tid)
    {
        Lane l{};
        if (SPLIT) {
            constexpr int MAIN = RUNS * SPR;  // 52
            const bool main_lane = tid < MAIN;
            const int run = tid / SPR;
            l.jA = main_lane ? tid - run * SPR : tid - MAIN;
            l.rA = main_lane ? run * K : RUNS * K;
            const bool tail = !main_lane && tid < MAIN + KA;  // carries one strip of the last column in its last slot
            l.jB = main_lane ? l.jA : SPR - 1;
            l.rB = main_lane ? l.rA : (tail ? RUNS * K + (tid - MAIN) - (K - 1) : 0);
            l.on = true;
            const int cntA = WIN - 4 * l.jA < 4 ? WIN - 4 * l.jA : 4, cntL = WIN - 4 * (SPR - 1);
            l.s01[0] = sel01_of(cntA); l.s23[0] = sel23_of(cntA);
            l.s01[1] = main_lane ? l.s01[0] : SEL_NONE; l.s23[1] = main_lane ? l.s23[0] : SEL_NONE;
            l.s01[2] = main_lane ? l.s01[0] : (tail ? sel01_of(cntL) : SEL_NONE); l.s23[2] = main_lane ? l.s23[0] : (tail ? sel23_of(cntL) : SEL_NONE);
        } else {
            const int run = tid / SPR;
            l.jA = l.jB = tid - run * SPR;
            l.rA = l.rB = run * K;
            l.on = run < RUNS;
            const int cnt = WIN - 4 * l.jA < 4 ? WIN - 4 * l.jA : 4;
            // only the last PAD_ROWS strips of a run can hang below the window, and only in runs that start within PAD_ROWS rows of its bottom edge
            const bool below = l.rA + (K - PAD_ROWS > 0 ? K - PAD_ROWS : 0) >= WIN;
            l.s01[0] = sel01_of(cnt); l.s23[0] = sel23_of(cnt);
            l.s01[1] = l.s01[2] = below ? SEL_NONE : l.s01[0]; l.s23[1] = l.s23[2] = below ? SEL_NONE : l.s23[0];
        }
        return l;
    }
    // one selector per class is enough: every slot of a class that holds a strip lies inside the window, for every thread (asserted in LK3Level)
    static constexpr bool classes_hold()
    {
        for (int t = 0; t < T; t++) {
            const Lane l = lane(t);
            if (!l.on) continue;
            for (int k = 0; k < K; k++) {
                const int c = slot_cls(k), row = (k < KA ? l.rA : l.rB) + k;
                if (l.s01[c] != SEL_NONE && (row < 0 || row >= WIN)) return false;
                if (!SPLIT && l.s01[c] == SEL_NONE && row < WIN) return false;
            }
        }
        return true;
    }
    // the lanes of a wavefront whose slots of class c hold a strip (one-wavefront kernels: lane = thread)
    static constexpr unsigned long long live_mask(int c)
    {
        unsigned long long m = 0;
        for (int t = 0; t < 64; t++) m |= (unsigned long long)(lane(t).on && lane(t).s01[c] != SEL_NONE) << t;
        return m;
    }
    static constexpr unsigned long long on_mask()
    {
        unsigned long long m = 0;
        for (int t = 0; t < 64; t++) m |= (unsigned long long)lane(t).on << t;
        return m;
    }
    static constexpr int OFF_TAB = ((OFF_RES + MAX_TPW * 4 * REC_DW + 15) / 16) * 16;
    static constexpr int TAB_COL = 0, TAB_LC = 2, TAB_SEL = 4, TAB_JR = 10, TAB_WORDS = 11;
    static constexpr int LDS_BYTES = OFF_TAB + 4 * TAB_WORDS * T;
    static_assert(NW != 1 || WIN != 51 || LDS_BYTES <= 160 * 1024 / 16, "k_lk3<51, 1, 4>: 16 workgroups per CU (4 wavefronts per SIMD) must fit in LDS");
};

typedef const uint2 __attribute__((address_space(1)))* gptr_u32x2;
typedef int __attribute__((address_space(3)))* lds_i32;
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef u32x4_t __attribute__((address_space(3)))* lds_u32x4;
typedef unsigned u32x4_dw_t __attribute__((ext_vector_type(4), aligned(4)));  // a 16-byte global load needs dword alignment only
typedef const u32x4_dw_t __attribute__((address_space(1)))* gptr_u32x4;
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned __attribute__((address_space(3)))* lds_u32;

// A lane predicate that is a FIXED set of lanes, as a 64-bit literal: the mask is a scalar constant (s_mov) where a compare of the thread index is a vector
// instruction whose result hipcc hoists out of the track loop and, short of scalar registers, parks in a VGPR lane (v_writelane) and fetches again
// (v_readlane) at every use.  Only where lane = thread index, or the predicate is one of the lane index.
__device__ __forceinline__ bool lane_in(unsigned long long mask) { return __builtin_amdgcn_inverse_ballot_w64(mask); }

// stage ROWS x PITCH bytes of image `im` starting at pixel (rx, ry) into LDS (region-aligned rows).  Compile-time
// extents: the loop is fully unrolled and every global load of the batch is issued before the first LDS store, so a
// staging costs one memory round trip.
template <int T, int ROWS, int WIDTH, int PITCH = WIDTH>  // WIDTH bytes of every row are staged, rows are PITCH bytes apart in LDS
__device__ __forceinline__ void stage_region(const ImgDesc& im, int rx, int ry, unsigned* dst, int tid)
{
    constexpr int DPR = WIDTH >> 2, LP = PITCH >> 2;
    // LPR lanes per region row, FOUR dwords of it each, T / LPR rows per batch of loads: a lane keeps its dword columns, so the address of batch `it` is
    // the first one plus the wave-uniform it * RPI * stride (no per-element division, one 32-bit add per batch; hipcc's form of the flat index q / DPR
    // cost ~12 VALU instructions per element).  A lane reads the five aligned dwords that hold its 16 bytes -- one 16-byte load and the dword behind it --
    // and stores four: a 51 x 51 region is 4 batches of 16 rows (one dword per lane, 16 lanes per row: 14 / 15 batches, an address add each).
    // Where a row is no multiple of 4 dwords, its last lane starts at dword DPR - 4 and stores some dwords a second time (the same values), so that
    // no lane reads past byte WIDTH + 4 of a row: what `fast` vouches for.
    constexpr int LPR = DPR <= 4 ? 1 : DPR <= 8 ? 2 : DPR <= 16 ? 4 : 8;
    static_assert(DPR >= 4 && DPR <= 32 && T % LPR == 0, "region rows narrower than 4 or wider than 32 dwords are not staged by this layout");
    constexpr int RPI = T / LPR, NIT = (ROWS + RPI - 1) / RPI;
    const bool fast = rx >= 0 && ry >= 0 && rx + WIDTH + 4 <= im.w && ry + ROWS <= im.h;
    if (fast) {
        const int l = tid & (LPR - 1), r0 = tid / LPR;
        const int d = min(4 * l, DPR - 4);
        // A region of fewer rows than one batch (the 15 x 15 regions, the patch of four wavefronts per track): the lanes below its last row take the
        // place of a lane inside it whose row differs by a multiple of 4 -- the same byte phase -- and do that lane's work a second time.  (No lane
        // may address a row >= ROWS: the row may lie outside the image, and the LDS behind the region is somebody else's.)
        static_assert(ROWS >= 4, "a region has at least four rows");
        const int rh = RPI <= ROWS || r0 < ROWS ? r0 : (r0 & 3);
        const unsigned bsh = (unsigned)(reinterpret_cast<uintptr_t>(im.p) & 3);
        const uint8_t* bp = im.p - bsh;  // dword aligned, wave uniform
        const unsigned off0 = (unsigned)(__mul24(ry + rh, im.stride) + rx + 4 * d) + bsh;
        // A batch steps RPI rows = a multiple of 4 bytes whatever the stride is, so a lane keeps its byte phase and its dword-aligned offset over the
        // whole staging: one 32-bit add of a wave-uniform step per batch (was: add + 2 and)
        static_assert(RPI % 4 == 0, "a batch of rows must keep the byte phase of a lane");
        const unsigned sh = off0 & 3u, aoff = off0 & ~3u;
        // The last batch may hang over the region's last row.  A branch around its loads or its stores would split the staging into two memory round
        // trips (and a branch around a load makes hipcc wait vmcnt(0) per element), so every lane loads and stores in every batch: a lane whose row
        // of the last batch lies below the region does batch 0 a second time instead -- same address, same byte phase, same values to the same place
        // (batch 0 of a lane is row rh, which is inside the region for every lane)
        const auto row_step = [&](int it) { return (it + 1) * RPI <= ROWS || r0 + it * RPI < ROWS ? it * RPI : 0; };
        u32x4_t q[NIT];
        unsigned q4[NIT];
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const uint8_t* ap = bp + (aoff + (unsigned)row_step(it) * (unsigned)im.stride);  // scalar base + 32-bit lane offset
            q[it] = *(gptr_u32x4)ap; q4[it] = ((gptr_u32)ap)[4];  // (dword aligned: a 16-byte global load asks no more)
        }
        unsigned* out = dst + rh * LP + d;
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            unsigned* o = out + row_step(it) * LP;
            o[0] = __builtin_amdgcn_alignbyte(q[it].y, q[it].x, sh);
            o[1] = __builtin_amdgcn_alignbyte(q[it].z, q[it].y, sh);
            o[2] = __builtin_amdgcn_alignbyte(q[it].w, q[it].z, sh);
            o[3] = __builtin_amdgcn_alignbyte(q4[it], q[it].w, sh);
        }
    } else {
        constexpr int TOTAL = ROWS * DPR;
        for (int q = tid; q < TOTAL; q += T) {
            const int r = q / DPR, d = q - r * DPR;
            unsigned v = 0;
#pragma unroll
            for (int c = 0; c < 4; c++) v |= (unsigned)pix_r(im, rx + 4 * d + c, ry + r) << (8 * c);
            dst[r * LP + d] = v;
        }
    }
}

// block-wide exact sum of NV per-lane int32 partials -> int64 totals valid in every thread
template <int NW, int NV, bool ROWSAFE>
__device__ __forceinline__ void block_sum_wide(const int* part, long long* tot, long long* red, int& phase, int wave)
{
    long long w[NV];
    if constexpr (!ROWSAFE && NV >= 2) {
        wave_sum2_i32_wide(part[0], part[1], w[0], w[1]);
        if constexpr (NV == 3) w[2] = wave_sum1_i32_wide_swap(part[2]);
    } else {
#pragma unroll
        for (int k = 0; k < NV; k++) w[k] = ROWSAFE ? wave_sum_i32_rows(part[k]) : wave_sum_i32_wide(part[k]);
    }
    if (NW == 1) {
#pragma unroll
        for (int k = 0; k < NV; k++) tot[k] = w[k];
        return;
    }
    long long* buf = red + phase * NW * 4;  // double buffered: one barrier per reduction
    phase ^= 1;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < NV; k++) buf[wave * 4 + k] = w[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; k++) {
        long long s = 0;
#pragma unroll
        for (int q = 0; q < NW; q++) s += buf[q * 4 + k];
        tot[k] = s;
    }
}

template <int WIN, int NW, int M>
struct LK3Level {  // the level functor of k_lk3 (see lk_track); phase: which half of the double-buffered block reduction comes next
    const LKJob& job;  // max_count and eps2 are read where the iterations start, not held across the direction and level loops
    char* smem;
    int tid;
    int& phase;
    int n_iter, n_setup;
    __device__ __forceinline__ void operator()(const ImgDesc I, const ImgDesc J, int level, int top_level, float p0x, float p0y, float& nxo, float& nyo,
                                               int& status, float& err, bool want_err);
};
template <int WIN, int NW, int M>
__device__ __forceinline__ void LK3Level<WIN, NW, M>::operator()(const ImgDesc I, const ImgDesc J, int level, int top_level, float p0x, float p0y,
                                                                 float& nxo, float& nyo, int& status, float& err, bool want_err)
{
    using C = LK3<WIN, NW, M>;
    // this lane's template gradients (registers: every index below is a compile-time constant).  The template SAMPLES are not kept: with
    // c = sum I * (Ix, Iy) over the lane's strips, sum (J - I) * Ix = sum J * Ix - c  exactly, so the Newton accumulators start at -c
    // (same per-lane partial sums as subtracting per sample; 12 registers and a v_pk_sub per pair less)
    uint2 tI[C::K], tX[C::K], tY[C::K];
    int cI[2] = {0, 0};
    unsigned* pI = reinterpret_cast<unsigned*>(smem + C::OFF_PI);
    unsigned* pJ = reinterpret_cast<unsigned*>(smem + C::OFF_PJ);
    long long* red = reinterpret_cast<long long*>(smem + C::OFF_RED);
    const int wave = tid >> 6;

    // One wavefront per track: the per-track arithmetic runs on PAIRS, x in rows 0 / 2 and y in rows 1 / 3 of one register (vh_lk_shared.hpp): n = (nx | ny),
    // no = (nxo | nyo), pd = (pdx | pdy).  The scalars nxo, nyo carry the position from level to level; `leave` hands them back at every way out.
    constexpr bool PAIR = NW == 1;
    float half, nx = 0.f, ny = 0.f, n = 0.f, no = 0.f;
    int ipx, ipy, rjx, rjy;
    Win w0;
    const auto leave = [&]() {
        if constexpr (PAIR) { nxo = pair_x(no); nyo = pair_y(no); }
    };
    if constexpr (PAIR) {
        LKStartPair s;
        no = pair_of(nxo, nyo);
        if (!lk_level_start_pair(pair_of(p0x, p0y), level, top_level, WIN, I, no, status, err, s)) { leave(); return; }
        half = s.half; ipx = s.ipx; ipy = s.ipy; n = s.n;
        w0 = bilinear_weights_pair(__fsub_rn(s.p, (float)s.ip));
        const int rj = vh_floor(n);
        rjx = pair_x(rj) - M; rjy = pair_y(rj) - M;
    } else {
        LKStart s;
        if (!lk_level_start(p0x, p0y, level, top_level, WIN, I, nxo, nyo, status, err, s)) return;
        half = s.half; ipx = s.ipx; ipy = s.ipy; nx = s.nx; ny = s.ny;
        w0 = bilinear_weights(__fsub_rn(s.px, (float)ipx), __fsub_rn(s.py, (float)ipy));
        rjx = vh_floor(nx) - M; rjy = vh_floor(ny) - M;
    }
    n_setup++;

    // one batch of global loads: template patch + search region around the predicted position
    __syncthreads();  // previous users of the patch buffers are done
    stage_region<C::T, C::PI_ROWS, C::PI_PITCH>(I, ipx - 1, ipy - 1, pI, tid);
    stage_region<C::T, C::RJ, C::PJ_WIDTH, C::PJ_PITCH>(J, rjx, rjy, pJ, tid);
    __syncthreads();

    const bool inside_I = ipx >= 1 && ipy >= 1 && ipx + WIN + 1 <= I.w - 1 && ipy + WIN + 1 <= I.h - 1;
    // this lane's strips: slots 0..KA-1 = column jA, window rows rA + k; slots KA..K-1 = column jB, rows rB + k (one segment unless C::SPLIT).
    // The map depends on the thread alone (LK3::Lane): k_lk3 wrote it to LDS before the first track, and every word of it comes back where it is first
    // needed (LDS loads take no VALU slot): ~50 loop-invariant registers stay out of the track loop, and no word is held through the set-up's register
    // peak unless the set-up uses it -- what brought the one-wavefront 51 x 51 kernel under 128 VGPRs (LK3_FINE_WAVES).
    // cls_sel(c): the v_perm selectors that pack (and mask) the gradient pairs of the slots of class c (LK3::slot_cls)
    static_assert(C::classes_hold(), "a selector class mixes slots inside and below the window");
    // (explicit LDS pointers, as the result records of k_lk3)
    const lds_u32 tab = (lds_u32)(smem + C::OFF_TAB) + tid;
    const auto tab_pair = [&](int i) { return u32x2_t{tab[i * C::T], tab[(i + 1) * C::T]}; };
    const auto cls_sel = [&](int c) { return tab_pair(C::TAB_SEL + 2 * c); };
    // (column and row as numbers: the border set-up and the err pass only, each reads the word itself)
    const auto lane_jr = [&]() { return tab[C::TAB_JR * C::T]; };
    constexpr unsigned long long ON = C::on_mask(), LIVE[3] = {C::live_mask(0), C::live_mask(1), C::live_mask(C::NCLS - 1)};
    const bool lane_on = C::LANES == C::T ? true : (C::T == 64 ? lane_in(ON) : tid < C::LANES);
    // (k is a compile-time constant wherever these are used: the strip loops are fully unrolled)
    const auto slot_col = [&](unsigned jr, int k) { return (int)((k < C::KA ? jr : jr >> 16) & 255u); };
    const auto slot_row = [&](unsigned jr, int k) { return (int)((k < C::KA ? jr >> 8 : jr >> 24) & 255u) + k; };
    const auto slot_live = [&](int k) {  // the slot holds a strip of the window
        if (C::T == 64) return lane_in(LIVE[C::slot_cls(k)]);
        return cls_sel(C::slot_cls(k)).x != C::SEL_NONE;
    };
    constexpr int slot_base = 0, slot_stride = 1;
    constexpr int PIP = C::PI_PITCH >> 2;
    int part[3] = {0, 0, 0};
    if (lane_on && inside_I) {
        // interior: rolling V rows (see strip_setup_linear): patch rows y .. y+3 feed strip y; one new row per strip
        const unsigned wt = pack16(w0.w00, w0.w01), wb = pack16(w0.w10, w0.w11);
        const u32x2_t col = tab_pair(C::TAB_COL);
        const unsigned* colA = reinterpret_cast<const unsigned*>(smem + col.x);  // pI + jA + rA * PIP
        const unsigned* colB = reinterpret_cast<const unsigned*>(smem + col.y);  // pI + jB + rB * PIP
        const auto patch_row = [&](int k, int dr) { return (k < C::KA ? colA : colB) + (k + dr) * PIP; };  // patch row slot_row(k) + dr, this lane's 8 bytes
        unsigned prB[6];
        int H0[4], H1[4], G0[4], G1[4], Vm[4];  // of V rows y, y+1 (Vm = the middle row's sample columns, for the template value)
        {
            unsigned pr0[6], prA[6];
            int V0[6], V1[6];
            const unsigned* r0 = patch_row(0, 0);
            setup_row_pairs(r0[0], r0[1], pr0);
            setup_row_pairs(r0[PIP], r0[PIP + 1], prA);
            setup_row_pairs(r0[2 * PIP], r0[2 * PIP + 1], prB);
            setup_v_row(pr0, prA, wt, wb, V0);
            setup_v_row(prA, prB, wt, wb, V1);
            setup_hg_row(V0, H0, G0, 0);
            setup_hg_row(V1, H1, G1, 1);
#pragma unroll
            for (int c = 0; c < 4; c++) Vm[c] = V1[c + 1];
        }
        // One patch row is read one strip ahead of its use and a scheduling barrier closes every strip: left alone, hipcc hoists the LDS reads of all
        // K strips to the top of the unrolled loop and interleaves the strips (248 VGPRs for K = 13)
        unsigned nlo, nhi;
        {
            const unsigned* rn = patch_row(0, 3);
            nlo = rn[0]; nhi = rn[1];
        }
        // the selectors of a class are read at the class's first slot: one pair of registers serves all classes
        u32x2_t sel = cls_sel(C::slot_cls(0));  // (four wavefronts per track: every slot is of class 1)
#pragma unroll
        for (int k = 0; k < C::K; k++) {
            {   // no branch per strip: see LK3 (rows past the patch read the padding / the next buffer: harmless garbage, masked by the selector)
                const unsigned clo = nlo, chi = nhi;
                if (k > 0 && C::slot_cls(k) != C::slot_cls(k - 1)) sel = cls_sel(C::slot_cls(k));
                if (k + 1 < C::K) {
                    const unsigned* rn = patch_row(k + 1, 3);
                    nlo = rn[0]; nhi = rn[1];
                }
                unsigned prN[6];
                int V2[6], H2[4], G2[4];
                setup_row_pairs(clo, chi, prN);
                setup_v_row(prB, prN, wt, wb, V2);
                setup_hg_row(V2, H2, G2, k + 2);
                setup_from_hg(H0, H1, H2, G0, G2, Vm, sel.x, sel.y, tI, tX, tY, slot_base + k * slot_stride, part[0], part[1], part[2]);
                cI[0] = dot2(tI[k].y, tX[k].y, dot2(tI[k].x, tX[k].x, cI[0]));
                cI[1] = dot2(tI[k].y, tY[k].y, dot2(tI[k].x, tY[k].x, cI[1]));
#pragma unroll
                for (int c = 0; c < 4; c++) { H0[c] = H1[c]; H1[c] = H2[c]; G0[c] = G1[c]; G1[c] = G2[c]; Vm[c] = V2[c + 1]; }
#pragma unroll
                for (int c = 0; c < 6; c++) prB[c] = prN[c];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else if (lane_on) {
        const unsigned jr = lane_jr();
#pragma unroll
        for (int k = 0; k < C::K; k++) {
            const int y = slot_row(jr, k), j = slot_col(jr, k);
            if (!slot_live(k)) {  // slots without a strip are zeros (the iterations read every slot)
                const uint2 z = make_uint2(0u, 0u);
                tI[slot_base + k * slot_stride] = z; tX[slot_base + k * slot_stride] = z; tY[slot_base + k * slot_stride] = z;
            } else {
                unsigned lo[4], hi[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const unsigned* row = pI + (y + r) * PIP + j;
                    lo[r] = row[0]; hi[r] = row[1];
                }
                strip_setup<false>(lo, hi, w0, I, ipx, ipy, 4 * j, y, min(4, WIN - 4 * j), tI, tX, tY, slot_base + k * slot_stride, part[0], part[1], part[2]);
                cI[0] = dot2(tI[k].y, tX[k].y, dot2(tI[k].x, tX[k].x, cI[0]));
                cI[1] = dot2(tI[k].y, tY[k].y, dot2(tI[k].x, tY[k].x, cI[1]));
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the K strips of this (rare) border path sequential: register pressure
        }
    }
    LKSys S;
    bool solvable;
    if constexpr (PAIR) {  // the three sums are converted in the lanes the reduction leaves them in; lk_system itself is not symmetric and stays scalar
        const float s11_12 = wave_sum2_f32_pair(part[0], part[1]);
        // (all three as scalars, the third from lane 0 of 64 equal ones: a sum left in a vector register counts as divergent, and the gate's branch with it)
        solvable = lk_system(pair_x(s11_12), pair_y(s11_12), pair_x(wave_sum1_f32_lane0(part[2])), WIN, S);
    } else {
        long long sA[3];
        block_sum_wide<NW, 3, (C::K == 1 && C::T == 64)>(part, sA, red, phase, wave);
        solvable = lk_system(sA[0], sA[1], sA[2], WIN, S);
    }
    if (!solvable) {
        if (level == 0) status = 0;
        leave();
        return;
    }
    LKSysPair SP{};
    if constexpr (PAIR) SP = lk_system_pair(S);
    const int ncI[2] = {-cI[0], -cI[1]};
    constexpr int PJP = C::PJ_PITCH >> 2;
    // C::OFF_PJ + 4 * (rA * PJP + jA) and the same of (rB, jB): (((inx - rjx) + 4 j) >> 2 = ((inx - rjx) >> 2) + j).  Out of the table they are opaque to the
    // compiler, as the iterations need them (below).  An `asm volatile` must never do that job: it counts as a possible store to any memory, and every load
    // of the pyramid descriptors behind it turns from a scalar load into a per-lane global load (round 5: +17 vector loads, -17 scalar loads and +48 VALU
    // instructions per track, +25 % wait cycles, +4-5 % kernel time -- what made every earlier form of this change slower than the code it shortened)
    const u32x2_t lc = tab_pair(C::TAB_LC);
    const unsigned lcA = lc.x, lcB = lc.y;

    // packed byte pairs of window row y (strip column j) of the staged search region at window origin (inx, iny)
    // The strip starts at byte `off` of the staged row: its 5 bytes lie inside the two dwords at off >> 2, and the byte pair (c, c+1) is ONE
    // v_perm of those two dwords with the selector 0x0c000c00 + (c + sh) * 0x00010001 + 0x00010000, sh = off & 3 (wave uniform: no alignbyte)
    auto region_row_pairs = [&](int inx, int iny, int j, int y, unsigned* t) {
        const int off = (inx - rjx) + 4 * j;
        const unsigned sel0 = 0x0c010c00u + (unsigned)__builtin_amdgcn_readfirstlane((inx - rjx) & 3) * 0x00010001u;
        const unsigned* row = pJ + (iny - rjy + y) * (C::PJ_PITCH >> 2) + (off >> 2);
        const unsigned d0 = row[0], d1 = row[1];
#pragma unroll
        for (int c = 0; c < 4; c++) t[c] = __builtin_amdgcn_perm(d1, d0, sel0 + (unsigned)c * 0x00010001u);
    };
    auto region_holds = [&](int inx, int iny) { return inx >= rjx && iny >= rjy && inx + WIN + 1 <= rjx + C::RJ && iny + WIN + 1 <= rjy + C::RJ; };
    auto restage = [&](int inx, int iny) {
        rjx = inx - M; rjy = iny - M;
        __syncthreads();
        stage_region<C::T, C::RJ, C::PJ_WIDTH, C::PJ_PITCH>(J, rjx, rjy, pJ, tid);
        __syncthreads();
    };

    float pdx = 0.f, pdy = 0.f, pd = 0.f;
    const int max_count = job.max_count;
    const double eps2 = job.eps2;
    for (int it = 0; it < max_count; it++) {
        // iteration 0 of a top level (the only level of the fine stage) stands on the template origin: its integer origin and its weights are the set-up's,
        // and the region was staged around it (lk_iter_at_template_origin; wave uniform, a scalar branch)
        const bool moved = !lk_iter_at_template_origin(it, level, top_level);
        int inx = ipx, iny = ipy, in = 0;
        if (moved) {
            if constexpr (PAIR) { in = vh_floor(n); inx = pair_x(in); iny = pair_y(in); }
            else { inx = vh_floor(nx); iny = vh_floor(ny); }
        }
        if (lk_outside(inx, iny, WIN, J)) {
            if (level == 0) status = 0;
            break;
        }
        Win wn = w0;
        if (moved) {
            if (!region_holds(inx, iny)) restage(inx, iny);
            wn = PAIR ? bilinear_weights_pair(__fsub_rn(n, (float)in)) : bilinear_weights(__fsub_rn(nx, (float)inx), __fsub_rn(ny, (float)iny));
        }
        const StripWeights w = strip_weights(wn);
        n_iter++;
        int b[2] = {ncI[0], ncI[1]};  // (lanes without strips keep -c: the first strip of the others starts from it without a copy)
        if (lane_on) {
            // rows are read one strip ahead of their use, a scheduling barrier closes every strip (see the set-up loop)
            const unsigned sel0 = 0x0c010c00u + (unsigned)__builtin_amdgcn_readfirstlane((inx - rjx) & 3) * 0x00010001u;
            // address of the lane's first search row = (lane constant, fixed for the level) + (wave-uniform offset of this iteration's window origin); the
            // lane constants were made opaque at level entry, so the compiler keeps ONE base register per column and puts the row step
            // (k + dr) * PJ_PITCH <= 816 bytes into the offset fields of ds_read2_b32 instead of folding OFF_PJ into every access (one v_add per row)
            const int uo = __builtin_amdgcn_readfirstlane(4 * ((iny - rjy) * PJP + ((inx - rjx) >> 2)));
            const unsigned* rowA = reinterpret_cast<const unsigned*>(smem + (lcA + (unsigned)uo));
            const unsigned* rowB = reinterpret_cast<const unsigned*>(smem + (lcB + (unsigned)uo));
            const auto region_row = [&](int k, int dr) { return (k < C::KA ? rowA : rowB) + (k + dr) * PJP; };  // search row slot_row(k) + dr
            unsigned top[4];
            {
                const unsigned* row = region_row(0, 0);
                const unsigned d0 = row[0], d1 = row[1];
#pragma unroll
                for (int c = 0; c < 4; c++) top[c] = __builtin_amdgcn_perm(d1, d0, sel0 + (unsigned)c * 0x00010001u);
            }
            unsigned n0 = region_row(0, 1)[0], n1 = region_row(0, 1)[1];
#pragma unroll
            for (int k = 0; k < C::K; k++) {
                {   // every slot, no branch: the gradients of slots without a strip are zeros (set-up)
                    const unsigned c0 = n0, c1 = n1;
                    if (k + 1 < C::K) {
                        n0 = region_row(k + 1, 1)[0];
                        n1 = region_row(k + 1, 1)[1];
                    }
                    unsigned bot[4], p01, p23;  // the bottom row of strip y is the top row of strip y+1
#pragma unroll
                    for (int c = 0; c < 4; c++) bot[c] = __builtin_amdgcn_perm(c1, c0, sel0 + (unsigned)c * 0x00010001u);
                    strip_bilinear_pairs(top, bot, w, p01, p23);
                    const int slot = slot_base + k * slot_stride;
                    const uint2 vX = tX[slot], vY = tY[slot];
                    if (k == 0) {  // the chains start at -c, which the next iteration needs again: three-address first link, no copy
                        b[0] = dot2(p23, vX.y, dot2_keep(p01, vX.x, ncI[0]));
                        b[1] = dot2(p23, vY.y, dot2_keep(p01, vY.x, ncI[1]));
                    } else {
                        b[0] = dot2(p23, vX.y, dot2(p01, vX.x, b[0]));
                        b[1] = dot2(p23, vY.y, dot2(p01, vY.x, b[1]));
                    }
#pragma unroll
                    for (int c = 0; c < 4; c++) top[c] = bot[c];
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if constexpr (PAIR) {
            if (lk_step_pair(SP, wave_sum2_f32_pair(b[0], b[1]), half, it, eps2, n, no, pd)) break;
        } else {
            long long sb[2];
            block_sum_wide<NW, 2, (C::K == 1 && C::T == 64)>(b, sb, red, phase, wave);
            if (lk_step(S, sb[0], sb[1], half, it, eps2, nx, ny, nxo, nyo, pdx, pdy)) break;
        }
    }
    leave();

    if (status && level == 0) {
        float fx = 0.f, fy = 0.f, f = 0.f;
        int inx, iny, in = 0;
        if (!(PAIR ? lk_final_origin_pair(no, half, WIN, J, f, in, inx, iny) : lk_final_origin(nxo, nyo, half, WIN, J, fx, fy, inx, iny))) {
            status = 0;
            return;
        }
        // err is discarded by the caller (KLT.py:83 `pa, v, _`): only the bounds rule matters.  (want_err says which pass this is; whether the job asks for err
        // is read here, where it matters, not carried through the track as one more scalar)
        if (!want_err || !job.err_out) return;
        if (!region_holds(inx, iny)) restage(inx, iny);
        const StripWeights w = strip_weights(PAIR ? bilinear_weights_pair(__fsub_rn(f, (float)in))
                                                  : bilinear_weights(__fsub_rn(fx, (float)inx), __fsub_rn(fy, (float)iny)));
        int se[1] = {0};
        if (lane_on) {
            const unsigned jr = lane_jr();
#pragma unroll
            for (int k = 0; k < C::K; k++) {
                if (slot_live(k)) {
                    const int y = slot_row(jr, k), j = slot_col(jr, k), cnt = min(4, WIN - 4 * j);
                    unsigned top[4], bot[4], p01, p23;
                    region_row_pairs(inx, iny, j, y, top);
                    region_row_pairs(inx, iny, j, y + 1, bot);
                    strip_bilinear_pairs(top, bot, w, p01, p23);
                    // template samples of strip y again from the staged patch (rows y+1, y+2; byte columns 1..5 of the lane's 8 bytes)
                    uint2 vI;
                    {
                        const unsigned* r1 = pI + (y + 1) * (C::PI_PITCH >> 2) + j;
                        const unsigned* r2 = r1 + (C::PI_PITCH >> 2);
                        unsigned tp[4], bt[4];
                        strip_row_pairs(__builtin_amdgcn_alignbyte(r1[1], r1[0], 1), r1[1] >> 8, tp);
                        strip_row_pairs(__builtin_amdgcn_alignbyte(r2[1], r2[0], 1), r2[1] >> 8, bt);
                        strip_bilinear_pairs(tp, bt, strip_weights(w0), vI.x, vI.y);
                    }
                    const short2v d01 = as_s2(p01) - as_s2(vI.x), d23 = as_s2(p23) - as_s2(vI.y);
                    const int d[4] = {d01.x, d01.y, d23.x, d23.y};
#pragma unroll
                    for (int c = 0; c < 4; c++) se[0] += c < cnt ? (d[c] < 0 ? -d[c] : d[c]) : 0;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        long long sse[1];
        block_sum_wide<NW, 1, (C::K == 1 && C::T == 64)>(se, sse, red, phase, wave);
        err = lk_err_of(i64_to_f32(sse[0]), WIN);
    }
}

// (forcing 5 or 6 workgroups per CU through the second launch bound spills and measured 3-8 % slower; a 128-VGPR cap
// + a 3-pixel search margin to fit 7 workgroups of the 2-wave variant per CU: 11 spilled registers, 5 % slower: not used)
// Wavefronts per SIMD the one-wavefront 51 x 51 kernel is compiled for: it needs 127 VGPRs and 10 208 bytes of LDS, so FOUR workgroups per SIMD (16 per CU)
// are resident without a spilled register (tests/test_gpu_lk3_residency.py asks the runtime).  A/B on one box against the same code held at three
// wavefronts: fine launch 1741 -> 1646 us, the headline +1.6 % (profiles/lk3_residency/ab.json).  (-DLK3_FINE_WAVES=3: experiments only.)
// (With the per-track arithmetic on pairs, profiles/lk3_pair/: 121 VGPRs.)
// (profiles/lk3_setup/: 124 VGPRs, and 120 in the single-level form the fine stage runs.)
#ifndef LK3_FINE_WAVES
#define LK3_FINE_WAVES 4
#endif
#define LK3_WAVES (NW == 1 ? (WIN == 51 ? LK3_FINE_WAVES : 3) : 4)
// ONE_LEVEL: jobs with max_level = 0 (the fine stage), see lk_track
template <int WIN, int NW, int M, bool ONE_LEVEL = false>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(LK3_WAVES))) void k_lk3(const void* job_tab, size_t tab_stride, unsigned grp, unsigned tpw)
{
    unsigned blk_x0, blk_y0;
    lk_block_xy<true>(blk_x0, blk_y0, grp);
    const unsigned blk_x = (unsigned)__builtin_amdgcn_readfirstlane((int)blk_x0), blk_y = (unsigned)__builtin_amdgcn_readfirstlane((int)blk_y0);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int phase = 0, tot_iter = 0, tot_setup = 0;
    unsigned ndone = 0;
    {   // this thread's lane map (LK3::Lane), once per workgroup and ahead of the track loop: a store inside the loop body would turn the descriptors' scalar
        // loads into vector loads (see the end of the loop)
        using C = LK3<WIN, NW, M>;
        constexpr int PIP = C::PI_PITCH >> 2, PJP = C::PJ_PITCH >> 2;
        const typename C::Lane l = C::lane((int)threadIdx.x);
        const lds_u32 tab = (lds_u32)(smem + C::OFF_TAB) + threadIdx.x;
        tab[(C::TAB_COL + 0) * C::T] = (unsigned)(C::OFF_PI + 4 * (l.jA + l.rA * PIP));
        tab[(C::TAB_COL + 1) * C::T] = (unsigned)(C::OFF_PI + 4 * (l.jB + l.rB * PIP));
        tab[(C::TAB_LC + 0) * C::T] = (unsigned)(C::OFF_PJ + 4 * (l.rA * PJP + l.jA));
        tab[(C::TAB_LC + 1) * C::T] = (unsigned)(C::OFF_PJ + 4 * (l.rB * PJP + l.jB));
#pragma unroll
        for (int c = 0; c < 3; c++) { tab[(C::TAB_SEL + 2 * c) * C::T] = l.s01[c]; tab[(C::TAB_SEL + 2 * c + 1) * C::T] = l.s23[c]; }
        tab[C::TAB_JR * C::T] = (unsigned)(l.jA | l.rA << 8 | l.jB << 16 | l.rB << 24);
        __syncthreads();
    }
    // A workgroup solves `tpw` consecutive launch slots one after the other (tracks that are neighbours in the launch order): fewer, longer-lived
    // workgroups.  Everything but the slot counter is re-derived per track (scalar loads of the job descriptor): values kept live across the loop cost
    // scalar registers the track code spills
#pragma unroll 1
    for (unsigned ti = 0; ti < tpw; ti++) {
        const LKJob& job = lk_job_row(job_tab, tab_stride, blk_y);
        // the point index and the start position are workgroup uniform and live until the epilogue: as SCALARS (their loads come back in vector registers,
        // and hipcc then parks them in scratch for the length of the kernel: 7 spilled registers, 28 bytes of scratch traffic per lane and track)
        int pt;
        float px, py;
        if (!lk_slot_start<true>(job, (int)(blk_x * tpw + ti), pt, px, py)) break;
        LK3Level<WIN, NW, M> lf{job, smem, (int)threadIdx.x, phase, 0, 0};

        // forward pass, then (fbt >= 0) the backward pass from its result: ONE copy of the track code in a loop over the direction -- two inlined copies
        // doubled the kernel and recomputed the per-lane mapping / masks of LK3Level in each
        float fx = 0.f, fy = 0.f, err = 0.f, bx = 0.f, by = 0.f;
        int st = 0, st2 = 0;
        const int ndir = job.fbt >= 0.f ? 2 : 1;
    #pragma unroll 1
        for (int dir = 0; dir < ndir; dir++) {
            if (dir == 1 && !st && !job.fbe_out) break;  // forward status 0 (block uniform): the backward pass cannot change v or p (see lk_solve)
            const PyrDesc& PA = dir ? job.J : job.I;
            const PyrDesc& PB = dir ? job.I : job.J;
            float ox, oy, e;
            int s;
            lk_track<ONE_LEVEL>(PA, PB, dir ? fx : px, dir ? fy : py, ox, oy, s, e, dir == 0, lf);
            if (dir == 0) { fx = ox; fy = oy; st = s; err = e; }
            else { bx = ox; by = oy; st2 = s; }
        }
        const float fbt = job.fbt;  // (read again: one scalar load instead of a register held across both passes)
        const float fbe = fbt >= 0.f ? lk_fb_gate(px, py, bx, by, fbt, st2, st) : 0.f;
        // the track's results wait in LDS: a global store inside this loop would make every descriptor load of the NEXT track a possibly-clobbered load,
        // i.e. a vector load instead of a scalar one (the same effect as the volatile asm of DESIGN.md section 9)
        if (NW == 1 ? lane_in(1ull) : threadIdx.x == 0) {
            // (an explicit LDS pointer: through a generic one hipcc counts these stores as possible writes to the job descriptors too)
            lds_i32 rec = (lds_i32)(smem + LK3<WIN, NW, M>::OFF_RES) + LK3<WIN, NW, M>::REC_DW * ti;
            rec[0] = pt; rec[1] = __float_as_int(fx); rec[2] = __float_as_int(fy); rec[3] = st != 0;
            rec[4] = __float_as_int(err); rec[5] = __float_as_int(fbe);
        }
        tot_iter += lf.n_iter; tot_setup += lf.n_setup;
        ndone = ti + 1;
        // The LAST memory operation of the loop body must not be a plain store: hipcc's scalar-load test (is a load clobbered anywhere in the function?) takes
        // whatever definition reaches the loop header over the back edge at face value when it is a store -- LDS or not -- and only looks through fences
        // and barriers with alias analysis.  With the record stores last, every descriptor load of the track code became a vector load.
        __syncthreads();
    }
    const LKJob& job = lk_job_row(job_tab, tab_stride, blk_y);
    if (threadIdx.x < ndone) {
        const int* rec = reinterpret_cast<const int*>(smem + LK3<WIN, NW, M>::OFF_RES) + LK3<WIN, NW, M>::REC_DW * threadIdx.x;
        lk_store_track(job, rec[0], __int_as_float(rec[1]), __int_as_float(rec[2]), rec[3], __int_as_float(rec[4]), __int_as_float(rec[5]));
    }
    if (threadIdx.x == 0 && ndone) lk_add_stats(job, blk_x, tot_iter, tot_setup);
}

// =================================================================================================================
// v4: quarter-wave kernel for small windows (WIN <= 16, the 15x15 coarse stages).
// One DPP row (16 lanes) per track, 4 tracks per wavefront: lane r owns window row r and its (WIN+3)/4 strips, the
// template quads stay in registers (no LDS at all), the exact window sums are 16-lane DPP reductions, and what used to be
// wave-uniform scalar work (weights, the 2x2 solve, the stop rules) is one vector instruction stream serving 4 tracks.
// A one-wave-per-track kernel spends about half of its instructions of a 15x15 Newton iteration on that uniform part
// and on the wave reduction; here it is shared 4 ways.  Rows of the search window are loaded once per lane and handed
// to the lane above through DPP (the bilinear cell needs rows r and r+1).  Same integers, same float sequence per
// track as the kernels above: bit-identical results.
// =================================================================================================================
__device__ __forceinline__ long long row16_sum_wide(int v)
{
    const int lo = dpp_row_sum(v & 0xffff), hi = dpp_row_sum(v >> 16);
    return (long long)hi * 65536ll + (long long)lo;
}
__device__ __forceinline__ unsigned dpp_from_next_lane(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xf, 0xf, true);  // row_shl:1 -> lane i reads lane i+1
}
// acc += dot2(a of lane i+1, b): the second link of a bilinear chain takes the packed pair of the row below straight from the neighbour lane
__device__ __forceinline__ int dot2c_next_lane(int acc, unsigned a, unsigned b)
{
    asm("v_dot2c_i32_i16_dpp %0, %1, %2 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(acc) : "v"(a), "v"(b));
    return acc;
}
// packed byte pair (c, c+1) of a row held as aligned words a[0..]
__device__ __forceinline__ unsigned row_pair(const unsigned* a, int c)
{
    const int w = c >> 2, q = c & 3;
    return q == 0 ? __builtin_amdgcn_perm(0u, a[w], 0x0c010c00u)
         : q == 1 ? __builtin_amdgcn_perm(0u, a[w], 0x0c020c01u)
         : q == 2 ? __builtin_amdgcn_perm(0u, a[w], 0x0c030c02u)
                  : __builtin_amdgcn_perm(a[w + 1], a[w], 0x0c040c03u);
}
// The interior paths keep the dwords a lane loaded as they are -- `sh` bytes in front of the pixel, sh = byte phase of the address -- and fold the
// phase into the v_perm that builds a byte pair anyway: pair (c, c+1) is bytes (c & 3) + sh and (c & 3) + sh + 1 <= 7 of the two neighbouring dwords
// (c >> 2, (c >> 2) + 1).  The selectors are per lane, four per loaded block of rows (one for every c & 3), where aligning the words to the pixel
// first cost a v_alignbyte per word and row.
struct PairSel {
    unsigned q[4];
};
__device__ __forceinline__ PairSel pair_selectors(unsigned sh)
{
    PairSel s;
    s.q[0] = 0x0c010c00u + sh * 0x00010001u;
#pragma unroll
    for (int k = 1; k < 4; k++) s.q[k] = s.q[0] + (unsigned)k * 0x00010001u;
    return s;
}
__device__ __forceinline__ unsigned row_pair(const unsigned* d, const PairSel& s, int c) { return __builtin_amdgcn_perm(d[(c >> 2) + 1], d[c >> 2], s.q[c & 3]); }

typedef unsigned __attribute__((aligned(1))) u32_unaligned;
typedef const u32_unaligned __attribute__((address_space(1)))* gptr_u32_unaligned;
// ROWS consecutive rows of image im from pixel (gx, gy): NWORDS + 1 dwords per row, d[rr][i] = bytes 4i - sh .. 4i - sh + 3 counted from the pixel;
// returns sh (0..3), ONE phase for all the rows.  NWORDS = dwords the pairs read counted from the pixel: the bytes touched are a subset of what
// load_row_words<NWORDS> touches.
// fast: scalar base + 32-bit lane offset (the form of stage_region; the base is moved to the corner of the border ring, so the offset of a window that
// reaches into the ring stays positive), one 32-bit add per further row.  Rows a multiple of 4 bytes apart -- every level the library builds -- are
// aligned dword loads.  Any other pitch (level 0 of a caller's image) keeps the phase of the first row: the further rows are then dword loads at an
// unaligned address, which the global memory path serves, and they stay within 3 bytes in front of the pixel like the aligned ones (lk_block_inside).
// !fast: REFLECT_101 byte loads packed at phase 0, addressed from the same scalar base (a second base pointer live in the Newton loops is one more
// scalar pair for hipcc to park in a VGPR lane).  Offsets are 32-bit and rows and pitch go through a 24-bit multiply: a level is smaller than 4 GiB,
// as in stage_region.
template <int NWORDS, int ROWS>
__device__ __forceinline__ unsigned load_rows_words(const ImgDesc& im, int gx, int gy, bool fast, unsigned (*d)[NWORDS + 1])
{
    unsigned sh = 0;
    const uint8_t* corner = im.p - (ptrdiff_t)im.pad * (im.stride + 1);
    const unsigned bsh = (unsigned)(reinterpret_cast<uintptr_t>(corner) & 3);
    const uint8_t* bp = corner - bsh;                               // dword aligned, wave uniform
    const unsigned org = (unsigned)(im.pad * (im.stride + 1)) + bsh;  // pixel (0, 0) from bp
    if (fast) {
        const unsigned off0 = (unsigned)(__mul24(gy, im.stride) + gx) + org;
        sh = off0 & 3u;
        const unsigned aoff = off0 & ~3u;
#pragma unroll
        for (int rr = 0; rr < ROWS; rr++) {
            gptr_u32_unaligned ap = (gptr_u32_unaligned)(bp + (aoff + (unsigned)rr * (unsigned)im.stride));
#pragma unroll
            for (int i = 0; i <= NWORDS; i++) d[rr][i] = ap[i];
        }
    } else {
#pragma unroll
        for (int rr = 0; rr < ROWS; rr++) {
            const uint8_t* row = bp + (org + (unsigned)vh_reflect101_near(gy + rr, im.h) * (unsigned)im.stride);
            // every row computes its own column indices (the empty asm hides that they are the same): kept from row to row, the 4 NWORDS of them cost
            // k_lk_o 20 VGPRs, and with them scratch at four wavefronts per SIMD
            int gxr = gx;
            if (rr > 0) asm("; row %1" : "+v"(gxr) : "n"(rr));
            // all column indices first (branch free), then all byte loads: one memory round trip per row
            unsigned b[4 * NWORDS];
#pragma unroll
            for (int k = 0; k < 4 * NWORDS; k++) b[k] = row[vh_reflect101_near(gxr + k, im.w)];
#pragma unroll
            for (int i = 0; i < NWORDS; i++) d[rr][i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | (b[4 * i + 3] << 24);
            d[rr][NWORDS] = 0;
        }
    }
    return sh;
}

// bilinear x32 samples of row r's NS strips at (x0, y0 + r) of image im: lane r holds row y0 + r, the row below comes from lane r + 1
template <int NS, int WIN>
__device__ __forceinline__ void lkq_sample_row(const ImgDesc& im, int x0, int y0, int r, bool fast, unsigned wt, unsigned wb, unsigned* p01, unsigned* p23)
{
    static_assert(WIN <= 4 * NS, "pairs up to (WIN - 1, WIN): NS dwords from the pixel");
    unsigned top[1][NS + 1];
    const PairSel sel = pair_selectors(load_rows_words<NS, 1>(im, x0, y0 + r, fast, top));
    int v[4 * NS];
#pragma unroll
    for (int c = 0; c < 4 * NS; c++) {
        if (c >= WIN) { v[c] = 0; continue; }  // columns >= WIN are never used (zero template gradients there, masked in the err sum): not computed
        const unsigned pr = row_pair(top[0], sel, c);
        v[c] = (dot2c_next_lane(dot2_first(pr, wt), pr, wb) << (16 - (W_BITS - 5))) + (1 << (W_BITS - 5 - 1 + 16 - (W_BITS - 5)));
    }
#pragma unroll
    for (int j = 0; j < NS; j++) {
        p01[j] = pack_hi16(v[4 * j], v[4 * j + 1]);
        p23[j] = pack_hi16(v[4 * j + 2], v[4 * j + 3]);
    }
}

// The border set-ups: NWORDS dwords of one image row ALIGNED to pixel (gx, gy), word i = bytes 4i..4i+3 (row_pair(a, c) takes its pairs from them)
template <int NWORDS>
__device__ __forceinline__ void load_row_words(const ImgDesc& im, int gx, int gy, bool fast, unsigned* a)
{
    if (fast) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(im.p + (ptrdiff_t)gy * im.stride + gx);
        const unsigned sh = (unsigned)(p & 3);
        gptr_u32 ap = (gptr_u32)(p - sh);
        unsigned d[NWORDS + 1];
#pragma unroll
        for (int i = 0; i <= NWORDS; i++) d[i] = ap[i];
#pragma unroll
        for (int i = 0; i < NWORDS; i++) a[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
    } else {
        const uint8_t* row = im.p + (size_t)vh_reflect101_near(gy, im.h) * im.stride;
        // all column indices first (branch free), then all byte loads: one memory round trip per row
        unsigned b[4 * NWORDS];
#pragma unroll
        for (int k = 0; k < 4 * NWORDS; k++) b[k] = row[vh_reflect101_near(gx + k, im.w)];
#pragma unroll
        for (int i = 0; i < NWORDS; i++) a[i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | (b[4 * i + 3] << 24);
    }
}

template <int WIN>
struct LKQLevel {  // the level functor of k_lk_q (see lk_track); r: this lane's place in its track's lanes
    int max_count;
    double eps2;
    int r, n_iter, n_setup;
    __device__ __forceinline__ void operator()(const ImgDesc I, const ImgDesc J, int level, int top_level, float p0x, float p0y, float& nxo, float& nyo,
                                               int& status, float& err, bool want_err);
};
template <int WIN>
__device__ __forceinline__ void LKQLevel<WIN>::operator()(const ImgDesc I, const ImgDesc J, int level, int top_level, float p0x, float p0y, float& nxo,
                                                          float& nyo, int& status, float& err, bool want_err)
{
    constexpr int NS = (WIN + 3) >> 2;  // strips per row
    constexpr int reach = WIN + 9;      // bytes from the first one that the aligned row reads of a lane may touch (lk_block_inside)
    LKStart s;
    if (!lk_level_start(p0x, p0y, level, top_level, WIN, I, nxo, nyo, status, err, s)) return;
    const float half = s.half;
    const int ipx = s.ipx, ipy = s.ipy;
    float nx = s.nx, ny = s.ny;
    const Win w0 = bilinear_weights(__fsub_rn(s.px, (float)ipx), __fsub_rn(s.py, (float)ipy));
    n_setup++;

    int a11 = 0, a12 = 0, a22 = 0;
    // template gradients of this lane's row (registers); the template SAMPLES are not kept: sum (J - I) Ix = sum J Ix - cI (see LK3Level)
    uint2 tX[NS], tY[NS];
    int cI[2] = {0, 0};
#pragma unroll
    for (int j = 0; j < NS; j++) { tX[j] = make_uint2(0, 0); tY[j] = make_uint2(0, 0); }
    // interior window: the (WIN+3)^2 patch [ipx-1, ipx+WIN+1] x [ipy-1, ipy+WIN+1] lies inside the level, so the V identity holds, and so do the
    // aligned 24-byte row reads
    const bool fast_I = lk_block_inside(I, ipx - 1, ipy - 1, WIN + 3, reach);
    const unsigned w0t = pack16(w0.w00, w0.w01), w0b = pack16(w0.w10, w0.w11);
    if (fast_I) {
        // Interior window, all 16 lanes of the track (lane WIN feeds lane WIN-1).  Lane r reads patch rows r .. r+2 and builds V rows r and r+1 over
        // the NC = 4 NS + 2 columns its NS adjacent strips share (V = bilinear weights . patch, no rounding: see strip_setup_linear); V row r+2 is
        // the neighbour's second row (DPP).  Scharr of V, vertical pass first:  S = 3 (V_r + V_r+2) + 10 V_r+1,  dV = V_r+2 - V_r,
        //   Ix = S[c+2] - S[c],   Iy = 3 (dV[c] + dV[c+2]) + 10 dV[c+1]
        // both kept x4 with the rounding folded in (column c of S carries 2^14 c), so descale + int16 packing is the upper half (pack_hi16).
        constexpr int NC = 4 * NS + 2;
        unsigned a[3][NS + 2];  // (pairs up to (NC - 1, NC): NS + 1 dwords from the pixel)
        const PairSel sel = pair_selectors(load_rows_words<NS + 1, 3>(I, ipx - 1, ipy + r - 1, true, a));
        int S4[NC], dV[NC], V1[NC];
        auto column = [&](int c) {
            const unsigned q0 = row_pair(a[0], sel, c), q1 = row_pair(a[1], sel, c), q2 = row_pair(a[2], sel, c);
            const int v0 = dot2(q1, w0b, dot2_first(q0, w0t));
            V1[c] = dot2(q2, w0b, dot2_first(q1, w0t));
            const int v2 = (int)dpp_from_next_lane((unsigned)V1[c]);
            S4[c] = mad24_v<40>(V1[c], mad24_s<12>(v0 + v2, c << W_BITS));
            dV[c] = v2 - v0;
        };
        column(0); column(1);
#pragma unroll
        for (int j = 0; j < NS; j++) {
            // strip j needs columns 4j .. 4j+5: four new ones per strip, and a scheduling barrier per strip keeps the column window short
            // (left alone hipcc builds all 18 columns first: 157 VGPRs)
#pragma unroll
            for (int c = 0; c < 4; c++) column(4 * j + 2 + c);
            constexpr int full = 4;
            const int cnt = WIN - 4 * j < full ? WIN - 4 * j : full;
            int iv[4], ix[4], iy[4];  // the wanted int16 in the upper half of each
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int col = 4 * j + c;
                iv[c] = (V1[col + 1] << (16 - (W_BITS - 5))) + (1 << (W_BITS - 5 - 1 + 16 - (W_BITS - 5)));
                ix[c] = S4[col + 2] - S4[col];
                iy[c] = mad24_v<40>(dV[col + 1], mad24_s<12>(dV[col] + dV[col + 2], 4 << (W_BITS - 1)));
            }
            // masking by selector (see setup_from_hg): cnt is a compile-time constant here, only the row mask is per lane
            const unsigned sel01 = r < WIN ? (cnt >= 2 ? 0x07060302u : 0x0c0c0302u) : 0x0c0c0c0cu;
            const unsigned sel23 = r < WIN ? (cnt >= 4 ? 0x07060302u : (cnt == 3 ? 0x0c0c0302u : 0x0c0c0c0cu)) : 0x0c0c0c0cu;
            const uint2 vI = make_uint2(pack_hi16(iv[0], iv[1]), pack_hi16(iv[2], iv[3]));
            const uint2 vX = make_uint2(__builtin_amdgcn_perm((unsigned)ix[1], (unsigned)ix[0], sel01), __builtin_amdgcn_perm((unsigned)ix[3], (unsigned)ix[2], sel23));
            const uint2 vY = make_uint2(__builtin_amdgcn_perm((unsigned)iy[1], (unsigned)iy[0], sel01), __builtin_amdgcn_perm((unsigned)iy[3], (unsigned)iy[2], sel23));
            tX[j] = vX; tY[j] = vY;
            a11 = dot2(vX.y, vX.y, dot2(vX.x, vX.x, a11));
            a12 = dot2(vX.y, vY.y, dot2(vX.x, vY.x, a12));
            a22 = dot2(vY.y, vY.y, dot2(vY.x, vY.x, a22));
            cI[0] = dot2(vI.y, vX.y, dot2(vI.x, vX.x, cI[0]));
            cI[1] = dot2(vI.y, vY.y, dot2(vI.x, vY.x, cI[1]));
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        // Window at the image border (most tracks on the tiny top levels of a 5-level pyramid).  The derivative image is 0 OUTSIDE the level, so the V
        // identity does not hold: the Scharr gradients of the integer pixels are built, zeroed outside, then interpolated like any other image.
        // Everything stays packed int16 (S = 3 (P_up + P_down) + 10 P <= 4080, D = P_down - P_up, Gx = S[k+1] - S[k-1], Gy = 3 (D[k-1] + D[k+1]) + 10 D[k]):
        // lane r holds pixel rows r-1 .. r+1 and gradient row r of the window as byte / int16 PAIRS (k, k+1), so a sample is two v_dot2 -- the
        // second one reading the pair of gradient row r+1 straight from lane r+1 (DPP) -- exactly like the search-image sampling.  All 16 lanes
        // take part (lane WIN feeds lane WIN-1).  REFLECT_101 is in the row loads; same integers as strip_setup<false>.
        unsigned a[3][NS + 1];
#pragma unroll
        for (int rr = 0; rr < 3; rr++) load_row_words<NS + 1>(I, ipx - 1, ipy + r - 1 + rr, I.pad >= VH_LV_PAD, a[rr]);  // bordered level: plain dword loads
        // bit c of M: gradient pixel (ipx + c, ipy + r) lies inside the level
        const int ay = ipy + r, cs = max(0, -ipx), ce = min(4 * NS, I.w - 1 - ipx);
        const unsigned M = (ay >= 0 && ay < I.h && ce >= cs) ? (((2u << ce) - 1u) & ~((1u << cs) - 1u)) : 0u;
        short2v Sp[4 * NS + 2], Dp[4 * NS + 2];
        unsigned Pm[4 * NS + 2];
        auto colb = [&](int k) {
            const unsigned pt = row_pair(a[0], k), pb = row_pair(a[2], k);
            Pm[k] = row_pair(a[1], k);
            const short2v k3 = {3, 3}, k10 = {10, 10};
            Sp[k] = (as_s2(pt) + as_s2(pb)) * k3 + as_s2(Pm[k]) * k10;
            Dp[k] = as_s2(pb) - as_s2(pt);
        };
        colb(0); colb(1);
#pragma unroll
        for (int j = 0; j < NS; j++) {
#pragma unroll
            for (int c = 0; c < 4; c++) colb(4 * j + 2 + c);
            const int cnt = WIN - 4 * j < 4 ? WIN - 4 * j : 4;
            int iv[4], ix[4], iy[4];  // the wanted int16 in the upper half of each
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int col = 4 * j + c;
                const short2v k3 = {3, 3}, k10 = {10, 10};
                // (pixel col, col + 1) of the gradient row: Gx = S[k+1] - S[k-1] with k = col + 1 in patch columns
                const unsigned m = (unsigned)__builtin_amdgcn_sbfe((int)M, col, 1) & 0xffffu | ((unsigned)__builtin_amdgcn_sbfe((int)M, col + 1, 1) << 16);
                const unsigned gx = __builtin_bit_cast(unsigned, Sp[col + 2] - Sp[col]) & m;
                const unsigned gy = __builtin_bit_cast(unsigned, (Dp[col] + Dp[col + 2]) * k3 + Dp[col + 1] * k10) & m;
                ix[c] = (dot2c_next_lane(dot2_first(gx, w0t), gx, w0b) << 2) + (4 << (W_BITS - 1));
                iy[c] = (dot2c_next_lane(dot2_first(gy, w0t), gy, w0b) << 2) + (4 << (W_BITS - 1));
                iv[c] = (dot2c_next_lane(dot2_first(Pm[col + 1], w0t), Pm[col + 1], w0b) << (16 - (W_BITS - 5))) + (1 << (W_BITS - 5 - 1 + 16 - (W_BITS - 5)));
            }
            const unsigned sel01 = r < WIN ? (cnt >= 2 ? 0x07060302u : 0x0c0c0302u) : 0x0c0c0c0cu;
            const unsigned sel23 = r < WIN ? (cnt >= 4 ? 0x07060302u : (cnt == 3 ? 0x0c0c0302u : 0x0c0c0c0cu)) : 0x0c0c0c0cu;
            const uint2 vI = make_uint2(pack_hi16(iv[0], iv[1]), pack_hi16(iv[2], iv[3]));
            const uint2 vX = make_uint2(__builtin_amdgcn_perm((unsigned)ix[1], (unsigned)ix[0], sel01), __builtin_amdgcn_perm((unsigned)ix[3], (unsigned)ix[2], sel23));
            const uint2 vY = make_uint2(__builtin_amdgcn_perm((unsigned)iy[1], (unsigned)iy[0], sel01), __builtin_amdgcn_perm((unsigned)iy[3], (unsigned)iy[2], sel23));
            tX[j] = vX; tY[j] = vY;
            a11 = dot2(vX.y, vX.y, dot2(vX.x, vX.x, a11));
            a12 = dot2(vX.y, vY.y, dot2(vX.x, vY.x, a12));
            a22 = dot2(vY.y, vY.y, dot2(vY.x, vY.x, a22));
            cI[0] = dot2(vI.y, vX.y, dot2(vI.x, vX.x, cI[0]));
            cI[1] = dot2(vI.y, vY.y, dot2(vI.x, vY.x, cI[1]));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    LKSys S;
    if (!lk_system(row16_sum_wide(a11), row16_sum_wide(a12), row16_sum_wide(a22), WIN, S)) {
        if (level == 0) status = 0;
        return;
    }

    float pdx = 0.f, pdy = 0.f;
    for (int it = 0; it < max_count; it++) {
        const int inx = vh_floor(nx), iny = vh_floor(ny);
        if (lk_outside(inx, iny, WIN, J)) {
            if (level == 0) status = 0;
            break;
        }
        const StripWeights w = strip_weights(bilinear_weights(__fsub_rn(nx, (float)inx), __fsub_rn(ny, (float)iny)));
        const bool fast = J.pad >= VH_LV_PAD || lk_block_inside(J, inx, iny, WIN + 1, reach);  // bordered level, or rows inside the level
        n_iter++;
        unsigned p01[NS], p23[NS];
        lkq_sample_row<NS, WIN>(J, inx, iny, r, fast, w.wt, w.wb, p01, p23);  // lane r = row r (lane WIN holds the last bottom row)
        int b1 = -cI[0], b2 = -cI[1];
#pragma unroll
        for (int j = 0; j < NS; j++) {
            // rows >= WIN and samples beyond the window edge carry Ix = Iy = 0, so they add nothing
            b1 = dot2(p23[j], tX[j].y, dot2(p01[j], tX[j].x, b1));
            b2 = dot2(p23[j], tY[j].y, dot2(p01[j], tY[j].x, b2));
        }
        if (lk_step(S, row16_sum_wide(b1), row16_sum_wide(b2), half, it, eps2, nx, ny, nxo, nyo, pdx, pdy)) break;
    }

    if (status && level == 0) {
        float fx, fy;
        int inx, iny;
        if (!lk_final_origin(nxo, nyo, half, WIN, J, fx, fy, inx, iny)) { status = 0; return; }
        if (!want_err) return;
        const StripWeights w = strip_weights(bilinear_weights(__fsub_rn(fx, (float)inx), __fsub_rn(fy, (float)iny)));
        const bool fast = J.pad >= VH_LV_PAD || lk_block_inside(J, inx, iny, WIN + 1, reach);  // bordered level, or rows inside the level
        unsigned p01[NS], p23[NS], i01[NS], i23[NS];
        lkq_sample_row<NS, WIN>(J, inx, iny, r, fast, w.wt, w.wb, p01, p23);
        // the template samples again (not kept by the set-up): the same bilinear sampling of I at the template origin
        lkq_sample_row<NS, WIN>(I, ipx, ipy, r, fast_I || I.pad >= VH_LV_PAD, w0t, w0b, i01, i23);
        int se = 0;
#pragma unroll
        for (int j = 0; j < NS; j++) {
            const short2v d01 = as_s2(p01[j]) - as_s2(i01[j]), d23 = as_s2(p23[j]) - as_s2(i23[j]);
            const int d[4] = {d01.x, d01.y, d23.x, d23.y};
            const int cnt = WIN - 4 * j < 4 ? WIN - 4 * j : 4;
#pragma unroll
            for (int c = 0; c < 4; c++) se += (c < cnt && r < WIN) ? (d[c] < 0 ? -d[c] : d[c]) : 0;
        }
        err = lk_err_of(i64_to_f32(row16_sum_wide(se)), WIN);
    }
}

template <int WIN>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void k_lk_q(const void* job_tab, size_t tab_stride, unsigned grp)
{
    static_assert(WIN <= 15, "lane WIN of every 16-lane row carries the extra bottom row");
    unsigned blk_x, blk_y;
    lk_block_xy<true>(blk_x, blk_y, grp);
    const LKJob& job = lk_job_row(job_tab, tab_stride, blk_y);
    const int slot = (int)blk_x * 4 + (threadIdx.x >> 4);
    int pt;
    float px, py;
    if (!lk_slot_start(job, slot, pt, px, py)) return;  // whole 16-lane rows leave together
    LKQLevel<WIN> lf{job.max_count, job.eps2, (int)(threadIdx.x & 15), 0, 0};
    LKResult R;
    lk_solve(job, px, py, lf, R);
    if (lf.r == 0) {
        lk_store_track(job, pt, R.fx, R.fy, R.st, R.err, R.fbe);
        lk_add_stats(job, (unsigned)slot, lf.n_iter, lf.n_setup);
    }
}

// =================================================================================================================
// v5: eighth-wave kernel for the 15x15 coarse stages at full load.
// 8 tracks per wavefront: a track owns 8 consecutive lanes (half a DPP row), lane r owns window rows 2r and 2r+1 (row 15 of lane 7 is a
// dummy that carries zero gradients).  What k_lk_q spends per 4 tracks on the per-track "uniform" work -- weights, the three window sums and
// minEig, the 2x2 solve, the stop rules, every DPP reduction: ~37 % of its instructions -- serves 8 tracks here, and the template set-up
// shares V rows inside a lane: a lane builds V rows 2r, 2r+1, 2r+2 from its four patch rows (3 per 2 window rows instead of 2 per row) and
// takes V row 2r+3 from lane r+1.  In the Newton iterations a lane loads its own two search rows; the row below its second row is the first
// row of lane r+1 (v_dot2c_i32_i16_dpp).  Window sums are 8-lane DPP reductions (quad_perm, quad_perm, row_half_mirror).  Lane 7 of a track
// reads lane 0 of the next track through DPP only for its dummy row.  Same integers, same float sequence per track: bit-identical results.
// =================================================================================================================
__device__ __forceinline__ int dpp_oct_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true);  // row_half_mirror: lane i <-> lane 7 - i of its half row
    return v;
}
// exact 8-lane sum of int32 partials as the float32 the int64 -> float32 conversion gives: hi * 2^16 + lo is exact in float64 (|hi| < 2^19, lo < 2^19),
// the final conversion rounds once
__device__ __forceinline__ float oct_sum_f32(int v)
{
    const int lo = dpp_oct_sum(v & 0xffff), hi = dpp_oct_sum(v >> 16);
    return (float)__fma_rn((double)hi, 65536.0, (double)lo);
}
// bilinear x32 samples of window rows 2r and 2r+1 (NS strips each) at (x0, y0) of image im: the lane holds image rows y0 + 2r and y0 + 2r + 1,
// the row below them is the first row of lane r + 1
template <int NS, int WIN>
__device__ __forceinline__ void lko_sample_rows(const ImgDesc& im, int x0, int y0, int r, bool fast, unsigned wt, unsigned wb, unsigned* a01,
                                                unsigned* a23, unsigned* b01, unsigned* b23)
{
    static_assert(WIN <= 4 * NS, "pairs up to (WIN - 1, WIN): NS dwords from the pixel");
    unsigned rows[2][NS + 1];
    const PairSel sel = pair_selectors(load_rows_words<NS, 2>(im, x0, y0 + 2 * r, fast, rows));
    const unsigned *top = rows[0], *mid = rows[1];
    constexpr int SH = 16 - (W_BITS - 5), RND = 1 << (W_BITS - 5 - 1 + 16 - (W_BITS - 5));
#pragma unroll
    for (int j = 0; j < NS; j++) {
        int va[4] = {0, 0, 0, 0}, vb[4] = {0, 0, 0, 0};  // columns >= WIN are never used (zero template gradients there): not computed
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (4 * j + c >= WIN) continue;
            const unsigned pa = row_pair(top, sel, 4 * j + c), pb = row_pair(mid, sel, 4 * j + c);
            va[c] = (dot2(pb, wb, dot2_first(pa, wt)) << SH) + RND;
            vb[c] = (dot2c_next_lane(dot2_first(pb, wt), pa, wb) << SH) + RND;
        }
        a01[j] = pack_hi16(va[0], va[1]); a23[j] = pack_hi16(va[2], va[3]);
        b01[j] = pack_hi16(vb[0], vb[1]); b23[j] = pack_hi16(vb[2], vb[3]);
    }
}

template <int WIN>
struct LKOLevel {  // the level functor of k_lk_o (see lk_track); r: this lane's place in its track's lanes
    int max_count;
    double eps2;
    int r, n_iter, n_setup;
    __device__ __forceinline__ void operator()(const ImgDesc I, const ImgDesc J, int level, int top_level, float p0x, float p0y, float& nxo, float& nyo,
                                               int& status, float& err, bool want_err);
};
template <int WIN>
__device__ __forceinline__ void LKOLevel<WIN>::operator()(const ImgDesc I, const ImgDesc J, int level, int top_level, float p0x, float p0y, float& nxo,
                                                          float& nyo, int& status, float& err, bool want_err)
{
    constexpr int NS = (WIN + 3) >> 2;  // strips per row
    constexpr int reach = WIN + 9;      // bytes from the first one that the aligned row reads of a lane may touch (lk_block_inside)
    LKStart s;
    if (!lk_level_start(p0x, p0y, level, top_level, WIN, I, nxo, nyo, status, err, s)) return;
    const float half = s.half;
    const int ipx = s.ipx, ipy = s.ipy;
    float nx = s.nx, ny = s.ny;
    const Win w0 = bilinear_weights(__fsub_rn(s.px, (float)ipx), __fsub_rn(s.py, (float)ipy));
    n_setup++;

    int a11 = 0, a12 = 0, a22 = 0;
    uint2 tXa[NS], tYa[NS], tXb[NS], tYb[NS];  // template gradients of window rows 2r (a) and 2r + 1 (b)
    int cI[2] = {0, 0};
    const bool fast_I = lk_block_inside(I, ipx - 1, ipy - 1, WIN + 3, reach);
    const unsigned w0t = pack16(w0.w00, w0.w01), w0b = pack16(w0.w10, w0.w11);
    const bool rowb = 2 * r + 1 < WIN;  // (row 2r is always a window row)
    // accumulate one strip of one window row: template samples vI, gradients vX / vY (already masked)
    auto accumulate = [&](uint2 vI, uint2 vX, uint2 vY) {
        a11 = dot2(vX.y, vX.y, dot2(vX.x, vX.x, a11));
        a12 = dot2(vX.y, vY.y, dot2(vX.x, vY.x, a12));
        a22 = dot2(vY.y, vY.y, dot2(vY.x, vY.x, a22));
        cI[0] = dot2(vI.y, vX.y, dot2(vI.x, vX.x, cI[0]));
        cI[1] = dot2(vI.y, vY.y, dot2(vI.x, vY.x, cI[1]));
    };
    if (fast_I) {
        // Lane r reads patch rows 2r .. 2r+3 (patch row 0 = image row ipy - 1) and builds V rows 2r, 2r+1, 2r+2 over the NC columns its strips share
        // (V = bilinear weights . patch, no rounding); V row 2r+3 is the neighbour's V row 2(r+1)+1 (DPP).  Window row w uses V rows w, w+1, w+2:
        //   S = 3 (V_w + V_w+2) + 10 V_w+1,  dV = V_w+2 - V_w,  Ix = S[c+2] - S[c],  Iy = 3 (dV[c] + dV[c+2]) + 10 dV[c+1]   (see LKQLevel)
        constexpr int NC = 4 * NS + 2;
        unsigned a[4][NS + 2];  // (pairs up to (NC - 1, NC): NS + 1 dwords from the pixel)
        const PairSel sel = pair_selectors(load_rows_words<NS + 1, 4>(I, ipx - 1, ipy - 1 + 2 * r, true, a));
        int SA[NC], SB[NC], dA[NC], dB[NC], CA[NC], CB[NC];
        auto column = [&](int c) {
            const unsigned q0 = row_pair(a[0], sel, c), q1 = row_pair(a[1], sel, c), q2 = row_pair(a[2], sel, c), q3 = row_pair(a[3], sel, c);
            const int va = dot2(q1, w0b, dot2_first(q0, w0t));
            const int vb = dot2(q2, w0b, dot2_first(q1, w0t));
            const int vc = dot2(q3, w0b, dot2_first(q2, w0t));
            const int vd = (int)dpp_from_next_lane((unsigned)vb);
            CA[c] = vb; CB[c] = vc;
            SA[c] = mad24_v<40>(vb, mad24_s<12>(va + vc, c << W_BITS));
            dA[c] = vc - va;
            SB[c] = mad24_v<40>(vc, mad24_s<12>(vb + vd, c << W_BITS));
            dB[c] = vd - vb;
        };
        column(0); column(1);
#pragma unroll
        for (int j = 0; j < NS; j++) {
            const int cnt = WIN - 4 * j < 4 ? WIN - 4 * j : 4;
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (c < cnt) column(4 * j + 2 + c);  // (window column k uses V columns k .. k+2)
            const unsigned s01 = cnt >= 2 ? 0x07060302u : 0x0c0c0302u, s23 = cnt >= 4 ? 0x07060302u : (cnt == 3 ? 0x0c0c0302u : 0x0c0c0c0cu);
            const unsigned sb01 = rowb ? s01 : 0x0c0c0c0cu, sb23 = rowb ? s23 : 0x0c0c0c0cu;
            int iv[4] = {0, 0, 0, 0}, ix[4] = {0, 0, 0, 0}, iy[4] = {0, 0, 0, 0};
            // window row 2r
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if (c >= cnt) continue;
                const int col = 4 * j + c;
                iv[c] = (CA[col + 1] << (16 - (W_BITS - 5))) + (1 << (W_BITS - 5 - 1 + 16 - (W_BITS - 5)));
                ix[c] = SA[col + 2] - SA[col];
                iy[c] = mad24_v<40>(dA[col + 1], mad24_s<12>(dA[col] + dA[col + 2], 4 << (W_BITS - 1)));
            }
            {
                const uint2 vI = make_uint2(pack_hi16(iv[0], iv[1]), pack_hi16(iv[2], iv[3]));
                const uint2 vX = make_uint2(__builtin_amdgcn_perm((unsigned)ix[1], (unsigned)ix[0], s01), __builtin_amdgcn_perm((unsigned)ix[3], (unsigned)ix[2], s23));
                const uint2 vY = make_uint2(__builtin_amdgcn_perm((unsigned)iy[1], (unsigned)iy[0], s01), __builtin_amdgcn_perm((unsigned)iy[3], (unsigned)iy[2], s23));
                tXa[j] = vX; tYa[j] = vY;
                accumulate(vI, vX, vY);
            }
            // window row 2r + 1
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if (c >= cnt) continue;
                const int col = 4 * j + c;
                iv[c] = (CB[col + 1] << (16 - (W_BITS - 5))) + (1 << (W_BITS - 5 - 1 + 16 - (W_BITS - 5)));
                ix[c] = SB[col + 2] - SB[col];
                iy[c] = mad24_v<40>(dB[col + 1], mad24_s<12>(dB[col] + dB[col + 2], 4 << (W_BITS - 1)));
            }
            {
                const uint2 vI = make_uint2(pack_hi16(iv[0], iv[1]), pack_hi16(iv[2], iv[3]));
                const uint2 vX = make_uint2(__builtin_amdgcn_perm((unsigned)ix[1], (unsigned)ix[0], sb01), __builtin_amdgcn_perm((unsigned)ix[3], (unsigned)ix[2], sb23));
                const uint2 vY = make_uint2(__builtin_amdgcn_perm((unsigned)iy[1], (unsigned)iy[0], sb01), __builtin_amdgcn_perm((unsigned)iy[3], (unsigned)iy[2], sb23));
                tXb[j] = vX; tYb[j] = vY;
                accumulate(vI, vX, vY);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        // Window at the image border: the derivative image is 0 OUTSIDE the level, so the Scharr gradients of the integer pixels are built (packed
        // int16 pairs (k, k+1), see LKQLevel), zeroed outside, then interpolated like any other image.  Lane r holds pixel rows 2r-1 .. 2r+2 of the
        // window (image rows ipy + 2r - 1 ..) and gradient rows 2r, 2r+1; gradient / pixel row 2r+2 is lane r+1's first row (DPP).
        unsigned a[4][NS + 1];
#pragma unroll
        for (int rr = 0; rr < 4; rr++) load_row_words<NS + 1>(I, ipx - 1, ipy - 1 + 2 * r + rr, I.pad >= VH_LV_PAD, a[rr]);
        const int ay = ipy + 2 * r, cs = max(0, -ipx), ce = min(4 * NS, I.w - 1 - ipx);
        const unsigned Mc = ce >= cs ? (((2u << ce) - 1u) & ~((1u << cs) - 1u)) : 0u;
        const unsigned MA = (ay >= 0 && ay < I.h) ? Mc : 0u, MB = (ay + 1 >= 0 && ay + 1 < I.h) ? Mc : 0u;
        short2v SpA[4 * NS + 2], DpA[4 * NS + 2], SpB[4 * NS + 2], DpB[4 * NS + 2];
        unsigned PA[4 * NS + 2], PB[4 * NS + 2];
        const short2v k3 = {3, 3}, k10 = {10, 10};
        auto colb = [&](int k) {
            const unsigned p0 = row_pair(a[0], k), p3 = row_pair(a[3], k);
            PA[k] = row_pair(a[1], k);
            PB[k] = row_pair(a[2], k);
            SpA[k] = (as_s2(p0) + as_s2(PB[k])) * k3 + as_s2(PA[k]) * k10;
            DpA[k] = as_s2(PB[k]) - as_s2(p0);
            SpB[k] = (as_s2(PA[k]) + as_s2(p3)) * k3 + as_s2(PB[k]) * k10;
            DpB[k] = as_s2(p3) - as_s2(PA[k]);
        };
        colb(0); colb(1);
        constexpr int SH = 16 - (W_BITS - 5), RND = 1 << (W_BITS - 5 - 1 + 16 - (W_BITS - 5));
#pragma unroll
        for (int j = 0; j < NS; j++) {
            const int cnt = WIN - 4 * j < 4 ? WIN - 4 * j : 4;
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (c < cnt) colb(4 * j + 2 + c);
            const unsigned s01 = cnt >= 2 ? 0x07060302u : 0x0c0c0302u, s23 = cnt >= 4 ? 0x07060302u : (cnt == 3 ? 0x0c0c0302u : 0x0c0c0c0cu);
            const unsigned sb01 = rowb ? s01 : 0x0c0c0c0cu, sb23 = rowb ? s23 : 0x0c0c0c0cu;
            int ivA[4] = {0, 0, 0, 0}, ixA[4] = {0, 0, 0, 0}, iyA[4] = {0, 0, 0, 0}, ivB[4] = {0, 0, 0, 0}, ixB[4] = {0, 0, 0, 0}, iyB[4] = {0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if (c >= cnt) continue;
                const int col = 4 * j + c;
                const unsigned ma = (unsigned)__builtin_amdgcn_sbfe((int)MA, col, 1) & 0xffffu | ((unsigned)__builtin_amdgcn_sbfe((int)MA, col + 1, 1) << 16);
                const unsigned mb = (unsigned)__builtin_amdgcn_sbfe((int)MB, col, 1) & 0xffffu | ((unsigned)__builtin_amdgcn_sbfe((int)MB, col + 1, 1) << 16);
                const unsigned gxa = __builtin_bit_cast(unsigned, SpA[col + 2] - SpA[col]) & ma;
                const unsigned gya = __builtin_bit_cast(unsigned, (DpA[col] + DpA[col + 2]) * k3 + DpA[col + 1] * k10) & ma;
                const unsigned gxb = __builtin_bit_cast(unsigned, SpB[col + 2] - SpB[col]) & mb;
                const unsigned gyb = __builtin_bit_cast(unsigned, (DpB[col] + DpB[col + 2]) * k3 + DpB[col + 1] * k10) & mb;
                ixA[c] = (dot2(gxb, w0b, dot2_first(gxa, w0t)) << 2) + (4 << (W_BITS - 1));
                iyA[c] = (dot2(gyb, w0b, dot2_first(gya, w0t)) << 2) + (4 << (W_BITS - 1));
                ivA[c] = (dot2(PB[col + 1], w0b, dot2_first(PA[col + 1], w0t)) << SH) + RND;
                ixB[c] = (dot2c_next_lane(dot2_first(gxb, w0t), gxa, w0b) << 2) + (4 << (W_BITS - 1));
                iyB[c] = (dot2c_next_lane(dot2_first(gyb, w0t), gya, w0b) << 2) + (4 << (W_BITS - 1));
                ivB[c] = (dot2c_next_lane(dot2_first(PB[col + 1], w0t), PA[col + 1], w0b) << SH) + RND;
            }
            {
                const uint2 vI = make_uint2(pack_hi16(ivA[0], ivA[1]), pack_hi16(ivA[2], ivA[3]));
                const uint2 vX = make_uint2(__builtin_amdgcn_perm((unsigned)ixA[1], (unsigned)ixA[0], s01), __builtin_amdgcn_perm((unsigned)ixA[3], (unsigned)ixA[2], s23));
                const uint2 vY = make_uint2(__builtin_amdgcn_perm((unsigned)iyA[1], (unsigned)iyA[0], s01), __builtin_amdgcn_perm((unsigned)iyA[3], (unsigned)iyA[2], s23));
                tXa[j] = vX; tYa[j] = vY;
                accumulate(vI, vX, vY);
            }
            {
                const uint2 vI = make_uint2(pack_hi16(ivB[0], ivB[1]), pack_hi16(ivB[2], ivB[3]));
                const uint2 vX = make_uint2(__builtin_amdgcn_perm((unsigned)ixB[1], (unsigned)ixB[0], sb01), __builtin_amdgcn_perm((unsigned)ixB[3], (unsigned)ixB[2], sb23));
                const uint2 vY = make_uint2(__builtin_amdgcn_perm((unsigned)iyB[1], (unsigned)iyB[0], sb01), __builtin_amdgcn_perm((unsigned)iyB[3], (unsigned)iyB[2], sb23));
                tXb[j] = vX; tYb[j] = vY;
                accumulate(vI, vX, vY);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    LKSys S;
    if (!lk_system(oct_sum_f32(a11), oct_sum_f32(a12), oct_sum_f32(a22), WIN, S)) {
        if (level == 0) status = 0;
        return;
    }

    float pdx = 0.f, pdy = 0.f;
    for (int it = 0; it < max_count; it++) {
        const int inx = vh_floor(nx), iny = vh_floor(ny);
        if (lk_outside(inx, iny, WIN, J)) {
            if (level == 0) status = 0;
            break;
        }
        const StripWeights w = strip_weights(bilinear_weights(__fsub_rn(nx, (float)inx), __fsub_rn(ny, (float)iny)));
        const bool fast = J.pad >= VH_LV_PAD || lk_block_inside(J, inx, iny, WIN + 1, reach);
        n_iter++;
        unsigned pa01[NS], pa23[NS], pb01[NS], pb23[NS];
        lko_sample_rows<NS, WIN>(J, inx, iny, r, fast, w.wt, w.wb, pa01, pa23, pb01, pb23);
        int b1 = -cI[0], b2 = -cI[1];
#pragma unroll
        for (int j = 0; j < NS; j++) {
            b1 = dot2(pa23[j], tXa[j].y, dot2(pa01[j], tXa[j].x, b1));
            b2 = dot2(pa23[j], tYa[j].y, dot2(pa01[j], tYa[j].x, b2));
            b1 = dot2(pb23[j], tXb[j].y, dot2(pb01[j], tXb[j].x, b1));
            b2 = dot2(pb23[j], tYb[j].y, dot2(pb01[j], tYb[j].x, b2));
        }
        if (lk_step(S, oct_sum_f32(b1), oct_sum_f32(b2), half, it, eps2, nx, ny, nxo, nyo, pdx, pdy)) break;
    }

    if (status && level == 0) {
        float fx, fy;
        int inx, iny;
        if (!lk_final_origin(nxo, nyo, half, WIN, J, fx, fy, inx, iny)) { status = 0; return; }
        if (!want_err) return;
        const StripWeights w = strip_weights(bilinear_weights(__fsub_rn(fx, (float)inx), __fsub_rn(fy, (float)iny)));
        const bool fast = J.pad >= VH_LV_PAD || lk_block_inside(J, inx, iny, WIN + 1, reach);
        unsigned pa01[NS], pa23[NS], pb01[NS], pb23[NS], ia01[NS], ia23[NS], ib01[NS], ib23[NS];
        lko_sample_rows<NS, WIN>(J, inx, iny, r, fast, w.wt, w.wb, pa01, pa23, pb01, pb23);
        lko_sample_rows<NS, WIN>(I, ipx, ipy, r, fast_I || I.pad >= VH_LV_PAD, w0t, w0b, ia01, ia23, ib01, ib23);
        int se = 0;
#pragma unroll
        for (int j = 0; j < NS; j++) {
            const short2v da01 = as_s2(pa01[j]) - as_s2(ia01[j]), da23 = as_s2(pa23[j]) - as_s2(ia23[j]);
            const short2v db01 = as_s2(pb01[j]) - as_s2(ib01[j]), db23 = as_s2(pb23[j]) - as_s2(ib23[j]);
            const int da[4] = {da01.x, da01.y, da23.x, da23.y}, db[4] = {db01.x, db01.y, db23.x, db23.y};
            const int cnt = WIN - 4 * j < 4 ? WIN - 4 * j : 4;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                se += c < cnt ? (da[c] < 0 ? -da[c] : da[c]) : 0;
                se += (c < cnt && rowb) ? (db[c] < 0 ? -db[c] : db[c]) : 0;
            }
        }
        err = lk_err_of(oct_sum_f32(se), WIN);
    }
}

template <int WIN>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void k_lk_o(const void* job_tab, size_t tab_stride, unsigned grp)
{
    static_assert(WIN == 15, "8 lanes x 2 rows: row 15 is the dummy that feeds nothing");
    unsigned blk_x, blk_y;
    lk_block_xy<true>(blk_x, blk_y, grp);
    const LKJob& job = lk_job_row(job_tab, tab_stride, blk_y);
    const int slot = (int)blk_x * 8 + (threadIdx.x >> 3);
    int pt;
    float px, py;
    if (!lk_slot_start(job, slot, pt, px, py)) return;  // whole 8-lane groups leave together
    LKOLevel<WIN> lf{job.max_count, job.eps2, (int)(threadIdx.x & 7), 0, 0};
    LKResult R;
    lk_solve(job, px, py, lf, R);
    if (lf.r == 0) {
        lk_store_track(job, pt, R.fx, R.fy, R.st, R.err, R.fbe);
        lk_add_stats(job, (unsigned)slot, lf.n_iter, lf.n_setup);
    }
}

#ifndef VH_LKH_WAVES
#define VH_LKH_WAVES 4  // wavefronts per SIMD k_lk_h is compiled for (profiles/lkh_lds/resources.md; 3: experiments)
#endif
// =================================================================================================================
// v6: sixteenth-wave kernel for the 15x15 coarse stages at the largest loads.
// 16 tracks per wavefront: a track owns 4 consecutive lanes (one DPP quad), lane r owns window rows 4r .. 4r+3 (row 15 of lane 3 is the dummy that
// carries zero gradients).  The per-track chain of k_lk_o -- weights, window tests, row addresses, selectors, the window sums, the 2x2 solve and the
// stop rules -- serves 16 tracks here, and the template set-up shares more V rows inside a lane: a lane builds V rows 4r .. 4r+4 from six patch rows
// (5 per 4 window rows where k_lk_o builds 3 per 2) and takes V row 4r+5 from lane r+1.  In the Newton iterations a lane loads its own four search
// rows; the row below its fourth row is the first row of lane r+1 (v_dot2c_i32_i16_dpp).  Window sums are 4-lane DPP reductions (two quad_perm
// steps).  Lane 3 of a track reads lane 0 of the next track through DPP only for its dummy row.  Same integers, same float sequence per track:
// bit-identical results.
// Four wavefronts per SIMD (128 VGPRs, no scratch): 40 dwords per lane -- the y gradients and the last strip of the x gradients of the template, and
// what a track carries from level to level -- live in 10 240 bytes of LDS per wavefront, see LKHLevel.
// =================================================================================================================
__device__ __forceinline__ int dpp_quad_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);  // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);  // quad_perm [2,3,0,1]
    return v;
}
// exact 4-lane sum of int32 partials as the float32 the int64 -> float32 conversion gives (the conversion of oct_sum_f32): the 16-bit halves are
// summed apart -- |hi| < 2^17, lo < 2^18 over four lanes -- hi * 2^16 + lo is exact in float64, the final conversion rounds once.
// A lane holds 4 rows x 15 columns = 60 samples of at most 8160 x 4080 each (operand bounds): the int32 partial cannot wrap.
static_assert(60ll * 8160 * 4080 < (1ll << 31), "a lane's 60-sample partial sum must fit int32");
__device__ __forceinline__ float quad_sum_f32(int v)
{
    const int lo = dpp_quad_sum(v & 0xffff), hi = dpp_quad_sum(v >> 16);
    return (float)__fma_rn((double)hi, 65536.0, (double)lo);
}
// The !fast form of load_rows_words for ONE row (REFLECT_101 byte loads packed at phase 0, the same addressing), four bytes in flight at a time: beside
// the sixteen template registers per row kind that is all this kernel has room for.  Border windows of levels without a border ring only.
template <int NWORDS, int ROW>
__device__ __forceinline__ void lkh_row_bytes(const ImgDesc& im, int gx, int gy, unsigned* d)
{
    // every row computes its own column indices (the empty asm hides that they are the same, see load_rows_words): kept from row to row they cost 16 VGPRs
    asm("; row %1" : "+v"(gx) : "n"(ROW));
    const uint8_t* corner = im.p - (ptrdiff_t)im.pad * (im.stride + 1);
    const unsigned bsh = (unsigned)(reinterpret_cast<uintptr_t>(corner) & 3);
    const uint8_t* bp = corner - bsh;
    const unsigned org = (unsigned)(im.pad * (im.stride + 1)) + bsh;
    const uint8_t* row = bp + (org + (unsigned)vh_reflect101_near(gy, im.h) * (unsigned)im.stride);
#pragma unroll
    for (int i = 0; i < NWORDS; i++) {
        unsigned b[4];
#pragma unroll
        for (int k = 0; k < 4; k++) b[k] = row[vh_reflect101_near(gx + 4 * i + k, im.w)];
        unsigned w = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        asm volatile("; word %1" : "+v"(w) : "n"(i));  // packed HERE: hipcc otherwise sinks the packing to the first use and keeps every byte in a register of its own
        d[i] = w;
    }
    d[NWORDS] = 0;
}
// bilinear x32 samples of window rows 4r .. 4r+3 (NS strips each) at (x0, y0) of image im: the lane holds image rows y0 + 4r .. y0 + 4r + 3, the row
// below them is the first row of lane r + 1.  f(k, j, h, p) takes columns 2h, 2h + 1 of strip j of the lane's row k as a packed int16 pair.  pre(j)
// runs ahead of strip j's arithmetic, half a strip of it before the first f(., j, ...) call: where the consumer issues the LDS reads of what it pairs strip j with (the
// sched_barrier keeps them there: hipcc would sink them to their use, or hoist all of them above the first strip).
template <int NS, int WIN, class P, class F>
__device__ __forceinline__ void lkh_sample_rows(const ImgDesc& im, int x0, int y0, int r, bool fast, unsigned wt, unsigned wb, P&& pre, F&& f)
{
    static_assert(WIN <= 4 * NS, "pairs up to (WIN - 1, WIN): NS dwords from the pixel");
    unsigned rows[4][NS + 1];
    unsigned sh = 0;
    if (fast) sh = load_rows_words<NS, 4>(im, x0, y0 + 4 * r, true, rows);
    else {
        // byte loads, a dword of one row at a time: with the 64 bytes of the four rows in flight together the kernel does not fit its registers
        lkh_row_bytes<NS, 0>(im, x0, y0 + 4 * r, rows[0]);
        lkh_row_bytes<NS, 1>(im, x0, y0 + 4 * r + 1, rows[1]);
        lkh_row_bytes<NS, 2>(im, x0, y0 + 4 * r + 2, rows[2]);
        lkh_row_bytes<NS, 3>(im, x0, y0 + 4 * r + 3, rows[3]);
    }
    const PairSel sel = pair_selectors(sh);
    constexpr int SH = 16 - (W_BITS - 5), RND = 1 << (W_BITS - 5 - 1 + 16 - (W_BITS - 5));
#pragma unroll
    for (int j = 0; j < NS; j++) {
        pre(j);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int h = 0; h < 2; h++) {  // a pair of columns at a time: no more than eight samples live
            int v[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};  // columns >= WIN are never used (zero template gradients there): not computed
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int c = 4 * j + 2 * h + e;
                if (c >= WIN) continue;
                unsigned p[4];
#pragma unroll
                for (int k = 0; k < 4; k++) p[k] = row_pair(rows[k], sel, c);
#pragma unroll
                for (int k = 0; k < 3; k++) v[k][e] = (dot2(p[k + 1], wb, dot2_first(p[k], wt)) << SH) + RND;
                v[3][e] = (dot2c_next_lane(dot2_first(p[3], wt), p[0], wb) << SH) + RND;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) f(k, j, h, pack_hi16(v[k][0], v[k][1]));
        }
    }
}

template <int WIN>
struct LKHLevel {  // the level functor of k_lk_h (see lk_track); r: this lane's place in its track's lanes
    int max_count;
    double eps2;
    int r, n_iter, n_setup;
    // The template gradients of a lane are 4 rows x NS strips x 2 dwords each of Ix and Iy: 64 registers, which do not fit beside the rest at four
    // wavefronts per SIMD.  LDS_CHUNKS x 16 bytes of them per lane live in LDS instead: all of Iy (chunk 2j + h: columns 2h, 2h + 1 of strip j, one dword
    // for each of the four rows) and the first half of the last strip of Ix (chunk 2 NS).  The last strip has ONE column in its second half (the other is
    // masked to zero), so Ix and Iy of that column share a dword: chunk 2 NS - 1 holds (Ix | Iy << 16) of column WIN - 1 for each row.  Chunk c of lane l
    // is the 16 bytes at 1024 c + 16 l of the workgroup's (= wavefront's) LDS: every access a ds_write_b128 / ds_read_b128 off one base register `tl`
    // with the chunk in the offset field, no bank conflict.  A lane reads only what it wrote: no barrier.  Every level of both passes reuses the slots,
    // and so does the err pass once the template is dead.
    // The chunk this frees (PARK) holds what a track keeps from its first level to its epilogue and a level reads once: the start point of the pass,
    // the point index and the launch slot -- four registers that the set-ups, which are what the kernel's register count is, do not carry.
    static constexpr int NS = (WIN + 3) >> 2, LDS_CHUNKS = 2 * NS + 2, LDS_BYTES = LDS_CHUNKS * 1024, PARK = 2 * NS + 1;
    static_assert(LDS_BYTES <= 160 * 1024 / 16, "16 one-wavefront workgroups per CU (4 wavefronts per SIMD) must fit in LDS");
    static_assert(WIN - 4 * (NS - 1) == 3, "the last strip must have exactly one column in its second half");
    lds_u32x4 tl;  // chunk 0 of this lane
    __device__ __forceinline__ void put(int chunk, const unsigned (&d)[4]) const { tl[64 * chunk] = u32x4_t{d[0], d[1], d[2], d[3]}; }
    __device__ __forceinline__ void park(float sx, float sy, int pt, int slot) const
    {
        tl[64 * PARK] = u32x4_t{__float_as_uint(sx), __float_as_uint(sy), (unsigned)pt, (unsigned)slot};
    }
    __device__ __forceinline__ u32x4_t parked() const { return tl[64 * PARK]; }
    // (p0x, p0y): NOT read -- the pass starts at the parked point
    __device__ __forceinline__ void operator()(const ImgDesc I, const ImgDesc J, int level, int top_level, float p0x, float p0y, float& nxo, float& nyo,
                                               int& status, float& err, bool want_err);
};
template <int WIN>
__device__ __forceinline__ void LKHLevel<WIN>::operator()(const ImgDesc I, const ImgDesc J, int level, int top_level, float, float, float& nxo,
                                                          float& nyo, int& status, float& err, bool want_err)
{
    constexpr int reach = WIN + 9;  // bytes from the first one that the aligned row reads of a lane may touch (lk_block_inside)
    const u32x4_t start = parked();
    const float p0x = __uint_as_float(start[0]), p0y = __uint_as_float(start[1]);
    LKStart s;
    if (!lk_level_start(p0x, p0y, level, top_level, WIN, I, nxo, nyo, status, err, s)) return;
    const float half = s.half;
    const int ipx = s.ipx, ipy = s.ipy;
    const Win w0 = bilinear_weights(__fsub_rn(s.px, (float)ipx), __fsub_rn(s.py, (float)ipy));
    n_setup++;

    int a11 = 0, a12 = 0, a22 = 0;
    uint2 tX[4][NS - 1];  // x template gradients of window rows 4r .. 4r + 3, all strips but the last; the last one and the y gradients: LDS (see `tl`)
    int cI[2] = {0, 0};
    const bool fast_I = lk_block_inside(I, ipx - 1, ipy - 1, WIN + 3, reach);
    const unsigned w0t = pack16(w0.w00, w0.w01), w0b = pack16(w0.w10, w0.w11);
    const bool rowd = 4 * r + 3 < WIN;  // (rows 4r .. 4r + 2 are always window rows)
    // Half h (columns 2h, 2h + 1) of strip j of the lane's four rows, as either set-up has just produced it -- template samples gI, gradients gX / gY,
    // already masked: into the window sums (integer sums: the order does not matter), and kept for the iterations HERE, in registers or in LDS, so that
    // the set-up holds neither a whole strip nor more of the template than the iterations do
    auto keep_half = [&](int j, int h, const unsigned (&gI)[4], const unsigned (&gX)[4], const unsigned (&gY)[4]) {
#pragma unroll
        for (int k = 0; k < 4; k++) {  // (one chain per sum: a second one each is five registers the set-up does not have, see profiles/lkh_lds/resources.md)
            a11 = dot2(gX[k], gX[k], a11);
            a12 = dot2(gX[k], gY[k], a12);
            a22 = dot2(gY[k], gY[k], a22);
            cI[0] = dot2(gI[k], gX[k], cI[0]);
            cI[1] = dot2(gI[k], gY[k], cI[1]);
        }
        if (j < NS - 1) {
            put(2 * j + h, gY);
#pragma unroll
            for (int k = 0; k < 4; k++) (h ? tX[k][j].y : tX[k][j].x) = gX[k];
        } else if (h == 0) {
            put(2 * j, gY);
            put(2 * NS, gX);
        } else {
            unsigned q[4];  // (the upper halves of gX and gY are the masked column)
#pragma unroll
            for (int k = 0; k < 4; k++) q[k] = gX[k] | gY[k] << 16;
            put(2 * j + 1, q);
        }
    };
    if (fast_I) {
        // Lane r reads patch rows 4r .. 4r+5 (patch row 0 = image row ipy - 1) and builds V rows 4r .. 4r+4 over the NC columns its strips share
        // (V = bilinear weights . patch, no rounding); V row 4r+5 is the neighbour's second V row (DPP).  Window row w uses V rows w, w+1, w+2:
        //   S = 3 (V_w + V_w+2) + 10 V_w+1,  dV = V_w+2 - V_w,  Ix = S[c+2] - S[c],  Iy = 3 (dV[c] + dV[c+2]) + 10 dV[c+1]   (see LKQLevel)
        constexpr int NC = 4 * NS + 2;
        unsigned a[6][NS + 2];  // (pairs up to (NC - 1, NC): NS + 1 dwords from the pixel)
        const PairSel sel = pair_selectors(load_rows_words<NS + 1, 6>(I, ipx - 1, ipy - 1 + 4 * r, true, a));
        int Sv[4][NC], dV[4][NC], Cv[4][NC];
        auto column = [&](int c) {
            unsigned q[6];
#pragma unroll
            for (int k = 0; k < 6; k++) q[k] = row_pair(a[k], sel, c);
            int V[6];
#pragma unroll
            for (int k = 0; k < 5; k++) V[k] = dot2(q[k + 1], w0b, dot2_first(q[k], w0t));
            V[5] = (int)dpp_from_next_lane((unsigned)V[1]);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                Cv[k][c] = V[k + 1];
                Sv[k][c] = mad24_v<40>(V[k + 1], mad24_s<12>(V[k] + V[k + 2], c << W_BITS));
                dV[k][c] = V[k + 2] - V[k];
            }
        };
        column(0); column(1);
        // a strip in two halves of two columns, so that no more than three columns of S / dV / C per row are live
#pragma unroll
        for (int j = 0; j < NS; j++) {
            const int cnt = WIN - 4 * j < 4 ? WIN - 4 * j : 4;
            const unsigned s01 = cnt >= 2 ? 0x07060302u : 0x0c0c0302u, s23 = cnt >= 4 ? 0x07060302u : (cnt == 3 ? 0x0c0c0302u : 0x0c0c0c0cu);
#pragma unroll
            for (int h = 0; h < 2; h++) {
#pragma unroll
                for (int c = 2 * h; c < 2 * h + 2; c++)
                    if (c < cnt) column(4 * j + 2 + c);  // (window column k uses V columns k .. k+2)
                const unsigned sh = h ? s23 : s01, sdh = rowd ? sh : 0x0c0c0c0cu;
                unsigned gI[4], gX[4], gY[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    int iv[2] = {0, 0}, ix[2] = {0, 0}, iy[2] = {0, 0};
#pragma unroll
                    for (int c = 2 * h; c < 2 * h + 2; c++) {
                        if (c >= cnt) continue;
                        const int col = 4 * j + c;
                        iv[c & 1] = (Cv[k][col + 1] << (16 - (W_BITS - 5))) + (1 << (W_BITS - 5 - 1 + 16 - (W_BITS - 5)));
                        ix[c & 1] = Sv[k][col + 2] - Sv[k][col];
                        iy[c & 1] = mad24_v<40>(dV[k][col + 1], mad24_s<12>(dV[k][col] + dV[k][col + 2], 4 << (W_BITS - 1)));
                    }
                    const unsigned m = k == 3 ? sdh : sh;
                    gI[k] = pack_hi16(iv[0], iv[1]);
                    gX[k] = __builtin_amdgcn_perm((unsigned)ix[1], (unsigned)ix[0], m);
                    gY[k] = __builtin_amdgcn_perm((unsigned)iy[1], (unsigned)iy[0], m);
                }
                keep_half(j, h, gI, gX, gY);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else {
        // Window at the image border: the derivative image is 0 OUTSIDE the level, so the Scharr gradients of the integer pixels are built (packed
        // int16 pairs (k, k+1), see LKQLevel), zeroed outside, then interpolated like any other image.  Lane r holds pixel rows 4r-1 .. 4r+4 of the
        // window (image rows ipy + 4r - 1 ..) and gradient rows 4r .. 4r+3; gradient / pixel row 4r+4 is lane r+1's first row (DPP).
        unsigned a[6][NS + 1];
#pragma unroll
        for (int rr = 0; rr < 6; rr++) {
            load_row_words<NS + 1>(I, ipx - 1, ipy - 1 + 4 * r + rr, I.pad >= VH_LV_PAD, a[rr]);
            __builtin_amdgcn_sched_barrier(0);  // (a row's byte loads at a time: six rows of them in flight do not fit the registers)
        }
        const int ay = ipy + 4 * r, cs = max(0, -ipx), ce = min(4 * NS, I.w - 1 - ipx);
        const unsigned Mc = ce >= cs ? (((2u << ce) - 1u) & ~((1u << cs) - 1u)) : 0u;
        unsigned Mr[4];
#pragma unroll
        for (int k = 0; k < 4; k++) Mr[k] = (ay + k >= 0 && ay + k < I.h) ? Mc : 0u;
        short2v Sp[4][4 * NS + 2], Dp[4][4 * NS + 2];
        unsigned Pp[4][4 * NS + 2];
        const short2v k3 = {3, 3}, k10 = {10, 10};
        auto colb = [&](int c) {
            unsigned p[6];
#pragma unroll
            for (int k = 0; k < 6; k++) p[k] = row_pair(a[k], c);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                Pp[k][c] = p[k + 1];
                Sp[k][c] = (as_s2(p[k]) + as_s2(p[k + 2])) * k3 + as_s2(p[k + 1]) * k10;
                Dp[k][c] = as_s2(p[k + 2]) - as_s2(p[k]);
            }
        };
        colb(0); colb(1);
        constexpr int SH = 16 - (W_BITS - 5), RND = 1 << (W_BITS - 5 - 1 + 16 - (W_BITS - 5));
#pragma unroll
        for (int j = 0; j < NS; j++) {
            const int cnt = WIN - 4 * j < 4 ? WIN - 4 * j : 4;
            const unsigned s01 = cnt >= 2 ? 0x07060302u : 0x0c0c0302u, s23 = cnt >= 4 ? 0x07060302u : (cnt == 3 ? 0x0c0c0302u : 0x0c0c0c0cu);
#pragma unroll
            for (int h = 0; h < 2; h++) {
#pragma unroll
                for (int c = 2 * h; c < 2 * h + 2; c++)
                    if (c < cnt) colb(4 * j + 2 + c);
                const unsigned sh = h ? s23 : s01, sdh = rowd ? sh : 0x0c0c0c0cu;
                int iv[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}}, ix[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}}, iy[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
#pragma unroll
                for (int c = 2 * h; c < 2 * h + 2; c++) {
                    if (c >= cnt) continue;
                    const int col = 4 * j + c, e = c & 1;
                    unsigned gx[4], gy[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const unsigned m = ((unsigned)__builtin_amdgcn_sbfe((int)Mr[k], col, 1) & 0xffffu) | ((unsigned)__builtin_amdgcn_sbfe((int)Mr[k], col + 1, 1) << 16);
                        gx[k] = __builtin_bit_cast(unsigned, Sp[k][col + 2] - Sp[k][col]) & m;
                        gy[k] = __builtin_bit_cast(unsigned, (Dp[k][col] + Dp[k][col + 2]) * k3 + Dp[k][col + 1] * k10) & m;
                    }
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        ix[k][e] = (dot2(gx[k + 1], w0b, dot2_first(gx[k], w0t)) << 2) + (4 << (W_BITS - 1));
                        iy[k][e] = (dot2(gy[k + 1], w0b, dot2_first(gy[k], w0t)) << 2) + (4 << (W_BITS - 1));
                        iv[k][e] = (dot2(Pp[k + 1][col + 1], w0b, dot2_first(Pp[k][col + 1], w0t)) << SH) + RND;
                    }
                    ix[3][e] = (dot2c_next_lane(dot2_first(gx[3], w0t), gx[0], w0b) << 2) + (4 << (W_BITS - 1));
                    iy[3][e] = (dot2c_next_lane(dot2_first(gy[3], w0t), gy[0], w0b) << 2) + (4 << (W_BITS - 1));
                    iv[3][e] = (dot2c_next_lane(dot2_first(Pp[3][col + 1], w0t), Pp[0][col + 1], w0b) << SH) + RND;
                }
                unsigned gI[4], gX[4], gY[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const unsigned m = k == 3 ? sdh : sh;
                    gI[k] = pack_hi16(iv[k][0], iv[k][1]);
                    gX[k] = __builtin_amdgcn_perm((unsigned)ix[k][1], (unsigned)ix[k][0], m);
                    gY[k] = __builtin_amdgcn_perm((unsigned)iy[k][1], (unsigned)iy[k][0], m);
                }
                keep_half(j, h, gI, gX, gY);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    LKSys S;
    if (!lk_system(quad_sum_f32(a11), quad_sum_f32(a12), quad_sum_f32(a22), WIN, S)) {
        if (level == 0) status = 0;
        return;
    }

    float nx = __fsub_rn(nxo, half), ny = __fsub_rn(nyo, half);  // (LKStart::nx, ny, taken here: two registers fewer across the set-up)
    float pdx = 0.f, pdy = 0.f;
    for (int it = 0; it < max_count; it++) {
        const int inx = vh_floor(nx), iny = vh_floor(ny);
        if (lk_outside(inx, iny, WIN, J)) {
            if (level == 0) status = 0;
            break;
        }
        const StripWeights w = strip_weights(bilinear_weights(__fsub_rn(nx, (float)inx), __fsub_rn(ny, (float)iny)));
        const bool fast = J.pad >= VH_LV_PAD || lk_block_inside(J, inx, iny, WIN + 1, reach);
        n_iter++;
        int b1 = -cI[0], b2 = -cI[1];
        // the LDS part of strip j is read ahead of the strip's own arithmetic (pre), one strip of it before the sums below use it
        u32x4_t yA = {0, 0, 0, 0}, yB = yA, xA = yA;  // Iy of columns 0, 1 | 2, 3 of the strip, a dword per row; Ix of columns 0, 1 of the last strip
        lkh_sample_rows<NS, WIN>(J, inx, iny, r, fast, w.wt, w.wb, [&](int j) {
            yA = tl[64 * (2 * j)]; yB = tl[64 * (2 * j + 1)];
            if (j == NS - 1) xA = tl[64 * (2 * NS)];
        }, [&](int k, int j, int h, unsigned p) {
            // (one chain per sum: two independent ones each fit the registers but measure no shorter, profiles/lkh_lds/resources.md)
            if (j < NS - 1) {
                b1 = dot2(p, h ? tX[k][j].y : tX[k][j].x, b1);
                b2 = dot2(p, h ? yB[k] : yA[k], b2);
            } else if (h == 0) {
                b1 = dot2(p, xA[k], b1);
                b2 = dot2(p, yA[k], b2);
            } else {  // p = (sample of column WIN - 1 | 0), yB = (Ix | Iy) of that column
                b1 = dot2(p, yB[k], b1);
                b2 = dot2(p << 16, yB[k], b2);
            }
        });
        if (lk_step(S, quad_sum_f32(b1), quad_sum_f32(b2), half, it, eps2, nx, ny, nxo, nyo, pdx, pdy)) break;
    }

    if (status && level == 0) {
        float fx, fy;
        int inx, iny;
        if (!lk_final_origin(nxo, nyo, half, WIN, J, fx, fy, inx, iny)) { status = 0; return; }
        if (!want_err) return;
        const StripWeights w = strip_weights(bilinear_weights(__fsub_rn(fx, (float)inx), __fsub_rn(fy, (float)iny)));
        const bool fast = J.pad >= VH_LV_PAD || lk_block_inside(J, inx, iny, WIN + 1, reach);
        // the template is dead by now: its slots (chunks 2j + h) hold the samples of I while J is sampled -- 32 registers beside the byte rows of a
        // border window were what four wavefronts per SIMD spilled
        unsigned si[4];
        lkh_sample_rows<NS, WIN>(I, ipx, ipy, r, fast_I || I.pad >= VH_LV_PAD, w0t, w0b, [](int) {}, [&](int k, int j, int h, unsigned p) {
            si[k] = p;
            if (k == 3) put(2 * j + h, si);
        });
        int se = 0;
        u32x4_t iA = {0, 0, 0, 0}, iB = iA;
        lkh_sample_rows<NS, WIN>(J, inx, iny, r, fast, w.wt, w.wb, [&](int j) { iA = tl[64 * (2 * j)]; iB = tl[64 * (2 * j + 1)]; },
                                 [&](int k, int j, int h, unsigned p) {
            const short2v d2 = as_s2(p) - as_s2(h ? iB[k] : iA[k]);
            const int d[2] = {d2.x, d2.y};
            const int cnt = WIN - 4 * j < 4 ? WIN - 4 * j : 4;
#pragma unroll
            for (int e = 0; e < 2; e++) se += (2 * h + e < cnt && (k < 3 || rowd)) ? (d[e] < 0 ? -d[e] : d[e]) : 0;
        });
        err = lk_err_of(quad_sum_f32(se), WIN);
    }
}

template <int WIN>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(VH_LKH_WAVES))) void k_lk_h(const void* job_tab, size_t tab_stride, unsigned grp)
{
    static_assert(WIN == 15, "4 lanes x 4 rows: row 15 is the dummy that feeds nothing");
    unsigned blk_x, blk_y;
    lk_block_xy<true>(blk_x, blk_y, grp);
    const LKJob& job = lk_job_row(job_tab, tab_stride, blk_y);
    const int slot = (int)blk_x * 16 + (threadIdx.x >> 2);
    int pt;
    float px, py;
    if (!lk_slot_start(job, slot, pt, px, py)) return;  // whole quads leave together
    __shared__ __attribute__((aligned(16))) u32x4_t tmpl[LKHLevel<WIN>::LDS_CHUNKS * 64];  // (explicitly LDS pointers from here on: a generic-pointer store in
    // the track code would turn the descriptor's scalar loads into per-lane vector loads, see k_lk3)
    LKHLevel<WIN> lf{job.max_count, job.eps2, (int)(threadIdx.x & 3), 0, 0, (lds_u32x4)tmpl + threadIdx.x};
    // lk_solve with the start point of each pass, the point index and the slot parked in LDS (LKHLevel::PARK) instead of carried in registers: the
    // forward start point, which the gate needs again, is read a second time from the parked point index
    // The slot is parked as 4 slot + r, the lane's index in the launch: r is read back with it after each pass and is not carried either.
    lf.park(px, py, pt, 4 * slot + lf.r);
    LKResult R;
    lk_track(job.I, job.J, 0.f, 0.f, R.fx, R.fy, R.st, R.err, job.err_out != nullptr, lf);
    R.fbe = 0.f;
    u32x4_t id = lf.parked();
    if (job.fbt >= 0.f) {
        float bx = 0.f, by = 0.f, e2, sx, sy;
        int st2 = 0;
        if (R.st || job.fbe_out) {
            lf.r = (int)(id[3] & 3);
            lf.park(R.fx, R.fy, (int)id[2], (int)id[3]);
            lk_track(job.J, job.I, 0.f, 0.f, bx, by, st2, e2, false, lf);
            id = lf.parked();
            R.fx = __uint_as_float(id[0]); R.fy = __uint_as_float(id[1]);  // (the same bits, not carried through the pass)
        }
        lk_point_start(job, (int)id[2], sx, sy);
        R.fbe = lk_fb_gate(sx, sy, bx, by, job.fbt, st2, R.st);
    }
    if ((id[3] & 3) == 0) {
        lk_store_track(job, (int)id[2], R.fx, R.fy, R.st, R.err, R.fbe);
        lk_add_stats(job, id[3] >> 2, lf.n_iter, lf.n_setup);
    }
}

// test hook (vh_debug_lkh_residency): what the runtime makes of k_lk_h<15> -- workgroups per CU, registers, scratch bytes per lane, LDS bytes per
// workgroup (static: the kernel is launched without dynamic LDS).  Launches nothing.
int vh_lkh_residency(int out[4])
{
    const void* fn = reinterpret_cast<const void*>(k_lk_h<15>);
    int blocks = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, 64, 0);
    if (e != hipSuccess) return (int)e;
    hipFuncAttributes a;
    e = hipFuncGetAttributes(&a, fn);
    if (e != hipSuccess) return (int)e;
    out[0] = blocks; out[1] = a.numRegs; out[2] = (int)a.localSizeBytes; out[3] = (int)a.sharedSizeBytes;
    return 0;
}

// test hook (vh_debug_lk3_residency): what the runtime makes of k_lk3<51, 1, 4> at the dynamic LDS size launch_lk3 passes -- workgroups per CU, registers,
// scratch bytes per lane, LDS bytes per workgroup.  Launches nothing.  The kernel has two forms (general and single-level, see lk_track): of each figure
// the WORSE of the two is reported (fewest workgroups, most registers, scratch and LDS).
int vh_lk3_residency(int out[4])
{
    const void* fns[2] = {reinterpret_cast<const void*>(k_lk3<51, 1, 4, false>), reinterpret_cast<const void*>(k_lk3<51, 1, 4, true>)};
    const int lds = LK3<51, 1, 4>::LDS_BYTES + vh_tuning().lk_lds_pad;
    for (int f = 0; f < 2; f++) {
        int blocks = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fns[f], 64, (size_t)lds);
        if (e != hipSuccess) return (int)e;
        hipFuncAttributes a;
        e = hipFuncGetAttributes(&a, fns[f]);
        if (e != hipSuccess) return (int)e;
        const int v[4] = {blocks, a.numRegs, (int)a.localSizeBytes, (int)a.sharedSizeBytes + lds};
        for (int k = 0; k < 4; k++) out[k] = f == 0 ? v[k] : (k == 0 ? std::min(out[k], v[k]) : std::max(out[k], v[k]));
    }
    return 0;
}

template <int WIN, int NW, int M>
static int launch_lk3(const LkPlan& p, const void* job_tab, size_t tab_stride, hipStream_t s)
{
    static_assert(LK3<WIN, NW, M>::MAX_TPW == LK3_MAX_TPW, "lk_plan clamps the slots per workgroup");
    const int lds = LK3<WIN, NW, M>::LDS_BYTES + (int)p.lds;
    const dim3 grid(p.grid_x, p.grid_y);
    if (p.one_level)
        hipLaunchKernelGGL((k_lk3<WIN, NW, M, true>), grid, dim3(p.block), lds, s, job_tab, tab_stride, p.group, (unsigned)p.tpw);
    else
        hipLaunchKernelGGL((k_lk3<WIN, NW, M, false>), grid, dim3(p.block), lds, s, job_tab, tab_stride, p.group, (unsigned)p.tpw);
    return 0;
}

// k_lk and k_lk_strip: all of their dynamic LDS is the host's figure, above the default limit for the larger windows
template <class Kernel>
static int launch_lk_lds(Kernel kernel, const LkPlan& p, const void* job_tab, size_t tab_stride, hipStream_t s)
{
    if (p.needs_big_lds) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kernel, dim3(p.grid_x, p.grid_y), dim3(p.block), p.lds, s, job_tab, tab_stride);
    return 0;
}

// k_lk_q, k_lk_o and k_lk_h: no dynamic LDS, the group argument of the block order
template <class Kernel>
static int launch_lk_group(Kernel kernel, const LkPlan& p, const void* job_tab, size_t tab_stride, hipStream_t s)
{
    hipLaunchKernelGGL(kernel, dim3(p.grid_x, p.grid_y), dim3(p.block), 0, s, job_tab, tab_stride, p.group);
    return 0;
}

// one-line forms of the plan (vh_step_plan.hpp) for vh_pyr_lk, vh_profile_lk_routes and their callers
int vh_lk_route(int batch, int max_n, int win) { return lk_route(batch, max_n, win, vh_tuning()); }
const char* vh_lk_route_name(int route, int win) { return lk_route_name(route, win); }
bool vh_lk_window_fits(int win) { return lk_window_fits(win); }
int vh_lk_max_window() { return lk_max_window(); }

// launches what lk_plan says: one hipLaunchKernelGGL per instantiation
int vh_launch_lk(const void* job_tab, size_t tab_stride, int batch, int max_n, int win, hipStream_t s, int* route_out, int* tpw_out, int max_level)
{
    const LkPlan p = lk_plan(batch, max_n, win, max_level, vh_tuning());
    if (route_out) *route_out = p.route;
    if (tpw_out) *tpw_out = p.tpw;
    if (p.rc) return p.rc;
    switch (p.route) {
    case LK_ROUTE_NONE: return 0;
    case LK_ROUTE_LK3_15: return launch_lk3<15, 1, 6>(p, job_tab, tab_stride, s);
    case LK_ROUTE_LK3_51_W1: return launch_lk3<51, 1, 4>(p, job_tab, tab_stride, s);
    case LK_ROUTE_LK3_51_W2: return launch_lk3<51, 2, 4>(p, job_tab, tab_stride, s);
    case LK_ROUTE_LK3_51_W4: return launch_lk3<51, 4, 4>(p, job_tab, tab_stride, s);
    case LK_ROUTE_O: return launch_lk_group(k_lk_o<15>, p, job_tab, tab_stride, s);
    case LK_ROUTE_H: return launch_lk_group(k_lk_h<15>, p, job_tab, tab_stride, s);
    case LK_ROUTE_Q: return launch_lk_group(k_lk_q<15>, p, job_tab, tab_stride, s);
    case LK_ROUTE_STRIP:
        if (p.strip_win == 15) return launch_lk_lds(k_lk_strip<15>, p, job_tab, tab_stride, s);
        if (p.strip_win == 51) return launch_lk_lds(k_lk_strip<51>, p, job_tab, tab_stride, s);
        return launch_lk_lds(k_lk_strip<0>, p, job_tab, tab_stride, s);
    case LK_ROUTE_SAMPLE: break;
    }
    return launch_lk_lds(k_lk, p, job_tab, tab_stride, s);
}
