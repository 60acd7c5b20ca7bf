// What every pyramidal-LK kernel of vh_lk.hip shares: the per-track scalar arithmetic of one level, the loop over the
// levels, and a kernel's prologue and epilogue.  The kernels differ only in how they sample a window and reduce a window sum; everything a track
// computes FROM the reduced sums is defined here once, so the float sequence per track -- and with it the bit-identity of the implementations --
// holds by construction.  Every function keeps an explicit __f*_rn / __d*_rn call per rounding: nothing here may be contracted or reassociated.
// Also here, because both sides use them: the fixed-point scales (W_BITS, LK_FLT_SCALE), the bilinear weights of a window origin (Win,
// bilinear_weights: every level computes them from the origins the functions below return) and the one-rounding int64 -> float32 conversion of a
// window sum (i64_to_f32).
// The level arithmetic exists in TWO forms of the same float sequence, next to each other below: the scalar form (lk_level_start, lk_step,
// lk_final_origin, bilinear_weights: k_lk, k_lk_strip, k_lk_q, k_lk_o and k_lk3 with more than one wavefront per track) and the pair form (the *_pair
// functions: k_lk3 with ONE wavefront per track, <51, 1, 4> and <15, 1, 6>), which runs the x and the y statement of the scalar form in two lanes at once.
#pragma once
#include "vh_kernels.hpp"
#include "vh_valu.hpp"

#define W_BITS 14
#define LK_FLT_SCALE (1.f / (1 << 20))

// The per-track inputs of a launch (count, launch order, start points) hang off pointers that were themselves loaded from the job descriptor: read
// through a GLOBAL pointer (where the address is workgroup uniform they then come through the scalar cache), not through the generic one hipcc
// assumes -- a workgroup otherwise starts with a chain of three dependent flat loads before its first image row is requested
typedef const int __attribute__((address_space(1)))* gptr_i32;
typedef const float __attribute__((address_space(1)))* gptr_f32;
#define LK_N_OF(job) ((job).n_ptr ? *(gptr_i32)(job).n_ptr : (job).n)

// (float)v for |v| < 2^53 with ONE rounding: hi * 2^32 + lo is exact in float64, the final conversion rounds once -- identical to the
// int64 -> float32 conversion, in 5 instructions instead of the compiler's ~15-instruction sequence
__device__ __forceinline__ float i64_to_f32(long long v)
{
    const double d = __dadd_rn(__dmul_rn((double)(int)(v >> 32), 4294967296.0), (double)(unsigned)(v & 0xffffffffll));
    return (float)d;
}

struct Win {
    int w00, w01, w10, w11;
};

__device__ __forceinline__ Win bilinear_weights(float a, float b)
{
    Win w;
    const float ia = __fsub_rn(1.f, a), ib = __fsub_rn(1.f, b);
    w.w00 = vh_round(__fmul_rn(__fmul_rn(ia, ib), (float)(1 << W_BITS)));
    w.w01 = vh_round(__fmul_rn(__fmul_rn(a, ib), (float)(1 << W_BITS)));
    w.w10 = vh_round(__fmul_rn(__fmul_rn(ia, b), (float)(1 << W_BITS)));
    w.w11 = (1 << W_BITS) - w.w00 - w.w01 - w.w10;
    return w;
}

// ---- one level of one track ------------------------------------------------------------------------------------------------------------------------

// a window whose origin is the integer pixel (ix, iy) lies wholly outside the level
__device__ __forceinline__ bool lk_outside(int ix, int iy, int win, const ImgDesc& im) { return ix < -win || ix >= im.w || iy < -win || iy >= im.h; }

// The aligned dword row reads of an e x e pixel block at (x, y) may run past either end of a row (`reach` bytes from x at most): harmless inside the
// level, excluded where they would leave it (first row to the left, last row to the right).  The template patch of a window at (ipx, ipy) is the block
// e = win + 3 at (ipx - 1, ipy - 1) (then the V identity of strip_setup_linear holds as well), a search window at (inx, iny) the block e = win + 1.
__device__ __forceinline__ bool lk_block_inside(const ImgDesc& im, int x, int y, int e, int reach)
{
    return x >= 0 && y >= 0 && x + e + 1 <= im.w && y + e <= im.h && !(y == 0 && x < 3) && !(y + e == im.h && x + reach > im.w);
}

// Level start: the template origin (px, py) with its integer part (ipx, ipy), and the predicted origin (nx, ny) of the search window; (nxo, nyo), the
// track's position on the level (window CENTRE), is carried from level to level.
struct LKStart {
    float half, px, py, nx, ny;
    int ipx, ipy;
};
// false: the template origin lies outside the level -- the level is skipped, and on level 0 the track is dead
__device__ __forceinline__ bool lk_level_start(float p0x, float p0y, int level, int top_level, int win, const ImgDesc& I, float& nxo, float& nyo,
                                               int& status, float& err, LKStart& s)
{
    s.half = (float)(win - 1) * 0.5f;
    const float lscale = __uint_as_float((unsigned)(127 - level) << 23);  // 2^-level exactly = (float)(1. / (1 << level)), without the f64 division
    const float cx = __fmul_rn(p0x, lscale), cy = __fmul_rn(p0y, lscale);
    if (level != top_level) { nxo = __fmul_rn(nxo, 2.f); nyo = __fmul_rn(nyo, 2.f); }
    else { nxo = cx; nyo = cy; }
    s.px = __fsub_rn(cx, s.half); s.py = __fsub_rn(cy, s.half);
    s.nx = __fsub_rn(nxo, s.half); s.ny = __fsub_rn(nyo, s.half);
    s.ipx = vh_floor(s.px); s.ipy = vh_floor(s.py);
    if (lk_outside(s.ipx, s.ipy, win, I)) {
        if (level == 0) { status = 0; err = 0.f; }
        return false;
    }
    return true;
}

// The first Newton iteration of the TOP level samples J where the template was sampled in I.  There lk_level_start sets nxo = cx (no = c), so
// s.nx = cx - half is the same subtraction of the same operands as s.px: s.nx == s.px and s.ny == s.py (s.n == s.p) bit for bit.  Iteration 0 then has
// floor(nx) = ipx, floor(ny) = ipy, the fractions nx - ipx = px - ipx, and with them the four bilinear weights (and their packed pairs) of the template
// origin: a level functor may take all of them from its set-up instead of computing the chain again, and a region staged around floor(s.n) holds this
// window by construction.  (A stage with max_level = 0 has nothing but top levels.)  From iteration 1 on, and on every lower level, n has moved.
__device__ __forceinline__ bool lk_iter_at_template_origin(int it, int level, int top_level) { return it == 0 && level == top_level; }

// The 2x2 system of a level from the three window sums of Ix Ix, Ix Iy, Iy Iy (exact integers, converted once to float32): false when the
// min-eigenvalue / determinant gate rejects the window.  iD = 1 / determinant.
struct LKSys {
    float A11, A12, A22, iD;
};
__device__ __forceinline__ bool lk_system(float s11, float s12, float s22, int win, LKSys& S)
{
    S.A11 = __fmul_rn(s11, LK_FLT_SCALE); S.A12 = __fmul_rn(s12, LK_FLT_SCALE); S.A22 = __fmul_rn(s22, LK_FLT_SCALE);
    const float D = __fsub_rn(__fmul_rn(S.A11, S.A22), __fmul_rn(S.A12, S.A12));
    const float dA = __fsub_rn(S.A11, S.A22);
    const float disc = __fadd_rn(__fmul_rn(dA, dA), __fmul_rn(__fmul_rn(4.f, S.A12), S.A12));
    const float minEig = __fdiv_rn(__fsub_rn(__fadd_rn(S.A22, S.A11), vh_sqrtf(disc)), (float)(2 * win * win));
    if (minEig < 1e-4f || D < 1.1920929e-07f) return false;
    S.iD = __fdiv_rn(1.f, D);
    return true;
}
__device__ __forceinline__ bool lk_system(long long s11, long long s12, long long s22, int win, LKSys& S)
{
    return lk_system(i64_to_f32(s11), i64_to_f32(s12), i64_to_f32(s22), win, S);
}

// One Newton update from the two window sums of (J - I) Ix, (J - I) Iy of iteration `it`: moves the search origin (nx, ny) and the position
// (nxo, nyo); true when the level is finished (step below eps, or the +-0.01 oscillation rule, which takes half of the last step back).
__device__ __forceinline__ bool lk_step(const LKSys& S, float sb1, float sb2, float half, int it, double eps2, float& nx, float& ny, float& nxo,
                                        float& nyo, float& pdx, float& pdy)
{
    const float b1 = __fmul_rn(sb1, LK_FLT_SCALE), b2 = __fmul_rn(sb2, LK_FLT_SCALE);
    const float dx = __fmul_rn(__fsub_rn(__fmul_rn(S.A12, b2), __fmul_rn(S.A22, b1)), S.iD);
    const float dy = __fmul_rn(__fsub_rn(__fmul_rn(S.A12, b1), __fmul_rn(S.A11, b2)), S.iD);
    nx = __fadd_rn(nx, dx); ny = __fadd_rn(ny, dy);
    nxo = __fadd_rn(nx, half); nyo = __fadd_rn(ny, half);
    if (__dadd_rn(__dmul_rn((double)dx, (double)dx), __dmul_rn((double)dy, (double)dy)) <= eps2) return true;
    if (it > 0 && fabsf(__fadd_rn(dx, pdx)) < 0.01f && fabsf(__fadd_rn(dy, pdy)) < 0.01f) {
        nxo = __fsub_rn(nxo, __fmul_rn(dx, 0.5f));
        nyo = __fsub_rn(nyo, __fmul_rn(dy, 0.5f));
        return true;
    }
    pdx = dx; pdy = dy;
    return false;
}
__device__ __forceinline__ bool lk_step(const LKSys& S, long long sb1, long long sb2, float half, int it, double eps2, float& nx, float& ny,
                                        float& nxo, float& nyo, float& pdx, float& pdy)
{
    return lk_step(S, i64_to_f32(sb1), i64_to_f32(sb2), half, it, eps2, nx, ny, nxo, nyo, pdx, pdy);
}

// After the iterations of level 0: the final window origin (fx, fy) with its integer part, where the err pass samples J.  False: it left the level
// (the track is dead).
__device__ __forceinline__ bool lk_final_origin(float nxo, float nyo, float half, int win, const ImgDesc& J, float& fx, float& fy, int& inx, int& iny)
{
    fx = __fsub_rn(nxo, half); fy = __fsub_rn(nyo, half);
    inx = vh_floor(fx); iny = vh_floor(fy);
    return !lk_outside(inx, iny, win, J);
}
__device__ __forceinline__ float lk_err_of(float sum_abs, int win) { return __fmul_rn(sum_abs, __fdiv_rn(1.f, (float)(32 * win * win))); }

// ---- the same level on PAIRS --------------------------------------------------------------------------------------------------------------------------
// Where ONE wavefront owns a track (k_lk3 with NW == 1: <51, 1, 4> and <15, 1, 6>) the functions above would compute the same floats on all 64 lanes, and
// they are symmetric in x and y almost line for line.  A PAIR is one register that holds the x value in the lanes of DPP rows 0 and 2 and the y value in the
// lanes of rows 1 and 3 (lanes 0 and 16 are read back: pair_x / pair_y) -- where the exact reduction of two window sums leaves them anyway.  Each function
// below is its scalar namesake above with the x and the y statement as ONE statement on a pair: per component the float operations and their order are
// literally the same (every rounding still its own __f*_rn / __d*_rn call), so the results are the same bits.  The few cross terms (A12 b2 / A12 b1, dx^2 +
// dy^2, the weight products) take the other component through pair_other, an LDS-pipe lane swap that takes no VALU slot.  What has to be a scalar -- an integer
// origin, the weights, the stop decision -- is read back with v_readlane and is then an SGPR.
// The scalar form stays the definition for every other kernel (k_lk, k_lk_strip, k_lk_q, k_lk_o and k_lk3 with NW > 1, whose sums come back through LDS into
// every thread); a change to one form is a change to both.

// rows 0 / 2: x, rows 1 / 3: y (one v_mov_dpp whose row mask leaves the even rows as they are; no v_cndmask)
__device__ __forceinline__ float pair_of(float x, float y)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(y), 0xE4, 0xa, 0xf, false));  // quad_perm [0,1,2,3], rows 1 and 3
}
// lane l gets lane l ^ 16: (x | y) -> (y | x).  ds_swizzle, bit mode: and 0x1f, or 0, xor 0x10
__device__ __forceinline__ int pair_other(int p) { return __builtin_amdgcn_ds_swizzle(p, 0x401f); }
__device__ __forceinline__ float pair_other(float p) { return __int_as_float(pair_other(__float_as_int(p))); }
__device__ __forceinline__ double pair_other(double p)
{
    return __hiloint2double(pair_other(__double2hiint(p)), pair_other(__double2loint(p)));
}
__device__ __forceinline__ int pair_x(int p) { return __builtin_amdgcn_readlane(p, 0); }
__device__ __forceinline__ int pair_y(int p) { return __builtin_amdgcn_readlane(p, 16); }
__device__ __forceinline__ float pair_x(float p) { return __int_as_float(pair_x(__float_as_int(p))); }
__device__ __forceinline__ float pair_y(float p) { return __int_as_float(pair_y(__float_as_int(p))); }

// (float)(hi * 65536 + lo), the exact window sum whose 16-bit halves were summed apart (wave_sum2_i32_wide: |hi| <= 64 * 2^15, 0 <= lo < 64 * 2^16), with ONE
// rounding and without leaving the lane: hi * 65536 + lo is exact in float64 (< 2^38), so this is the float i64_to_f32 gives for the recombined int64
__device__ __forceinline__ float wide_halves_to_f32(int lo, int hi) { return (float)__dadd_rn(__dmul_rn((double)hi, 65536.0), (double)lo); }

// bilinear_weights of the fractions (a | b): (ia ib | ib ia) and (a ib | b ia) are two products, scaled, rounded and converted once each
__device__ __forceinline__ Win bilinear_weights_pair(float ab)
{
    Win w;
    const float iab = __fsub_rn(1.f, ab), iba = pair_other(iab);
    const int m00 = vh_round(__fmul_rn(__fmul_rn(iab, iba), (float)(1 << W_BITS)));
    const int m01 = vh_round(__fmul_rn(__fmul_rn(ab, iba), (float)(1 << W_BITS)));
    w.w00 = pair_x(m00);
    w.w01 = pair_x(m01);
    w.w10 = pair_y(m01);
    w.w11 = (1 << W_BITS) - w.w00 - w.w01 - w.w10;
    return w;
}

// lk_level_start: p0 = (p0x | p0y), no = (nxo | nyo)
struct LKStartPair {
    float half, p, n;  // (px | py), (nx | ny)
    int ip;            // (ipx | ipy), and as scalars:
    int ipx, ipy;
};
__device__ __forceinline__ bool lk_level_start_pair(float p0, int level, int top_level, int win, const ImgDesc& I, float& no, int& status, float& err,
                                                    LKStartPair& s)
{
    s.half = (float)(win - 1) * 0.5f;
    const float lscale = __uint_as_float((unsigned)(127 - level) << 23);
    const float c = __fmul_rn(p0, lscale);
    if (level != top_level) no = __fmul_rn(no, 2.f);
    else no = c;
    s.p = __fsub_rn(c, s.half);
    s.n = __fsub_rn(no, s.half);
    s.ip = vh_floor(s.p);
    s.ipx = pair_x(s.ip); s.ipy = pair_y(s.ip);
    if (lk_outside(s.ipx, s.ipy, win, I)) {
        if (level == 0) { status = 0; err = 0.f; }
        return false;
    }
    return true;
}

// what lk_step reads of a level's system: A12 and iD in every lane, the diagonal as (A22 | A11)
struct LKSysPair {
    float A12, Ad, iD;
};
__device__ __forceinline__ LKSysPair lk_system_pair(const LKSys& S) { return LKSysPair{S.A12, pair_of(S.A22, S.A11), S.iD}; }

// lk_step: sb = (sb1 | sb2) as floats, n = (nx | ny), no = (nxo | nyo), pd = (pdx | pdy)
__device__ __forceinline__ bool lk_step_pair(const LKSysPair& S, float sb, float half, int it, double eps2, float& n, float& no, float& pd)
{
    const float b = __fmul_rn(sb, LK_FLT_SCALE);
    const float d = __fmul_rn(__fsub_rn(pair_other(__fmul_rn(S.A12, b)), __fmul_rn(S.Ad, b)), S.iD);  // (dx | dy)
    n = __fadd_rn(n, d);
    no = __fadd_rn(n, half);
    const double q = __dmul_rn((double)d, (double)d);
    if (__builtin_amdgcn_ballot_w64(__dadd_rn(q, pair_other(q)) <= eps2) & 1ull) return true;  // lane 0: dx^2 + dy^2
    constexpr unsigned long long XY = 1ull | 1ull << 16;
    if (it > 0 && (__builtin_amdgcn_ballot_w64(fabsf(__fadd_rn(d, pd)) < 0.01f) & XY) == XY) {
        no = __fsub_rn(no, __fmul_rn(d, 0.5f));
        return true;
    }
    pd = d;
    return false;
}

// lk_final_origin: f = (fx | fy), in = its integer part as a pair, (inx, iny) the same as scalars
__device__ __forceinline__ bool lk_final_origin_pair(float no, float half, int win, const ImgDesc& J, float& f, int& in, int& inx, int& iny)
{
    f = __fsub_rn(no, half);
    in = vh_floor(f);
    inx = pair_x(in); iny = pair_y(in);
    return !lk_outside(inx, iny, win, J);
}

// ---- one track --------------------------------------------------------------------------------------------------------------------------------------

// All levels of one track, coarse to fine.  `lf` is a kernel's level functor: lf(I, J, level, top_level, px, py, ox, oy, status, err, want_err) solves one
// level and keeps what the kernel needs from level to level (its lanes' place in the window, LDS pointers, the statistics counts) as its state.
// ONE_LEVEL: the launcher vouches that the job has max_level = 0, hence one level (fill_pyramid).  The level functor is then entered with level =
// top_level = 0 as CONSTANTS: the level loop, the per-level descriptor addressing, 2^-level and every `level != top_level` / `level == 0` test fold away
// in the ONE copy of the functor's body, and with them the scalars a kernel otherwise carries (or parks) through the track for them.
template <bool ONE_LEVEL = false, class LevelFn>
__device__ __forceinline__ void lk_track(const PyrDesc& PI, const PyrDesc& PJ, float px, float py, float& ox, float& oy, int& status, float& err,
                                         bool want_err, LevelFn& lf)
{
    const int nl = min(PI.nlevels, PJ.nlevels);
    status = 1;
    err = 0.f;
    ox = 0.f; oy = 0.f;
    if constexpr (ONE_LEVEL) {
        lf(PI.lv[0], PJ.lv[0], 0, 0, px, py, ox, oy, status, err, want_err);
        return;
    }
    for (int level = nl - 1; level >= 0; level--) lf(PI.lv[level], PJ.lv[level], level, nl - 1, px, py, ox, oy, status, err, want_err);
}

// forward-backward gate (KLT.py:50): returns fbe, the distance between the start point and where the backward pass ended
__device__ __forceinline__ float lk_fb_gate(float px, float py, float bx, float by, float fbt, int st2, int& st)
{
    const float ddx = __fsub_rn(px, bx), ddy = __fsub_rn(py, by);
    const float fbe = vh_sqrtf(__fadd_rn(__fmul_rn(ddx, ddx), __fmul_rn(ddy, ddy)));
    st = st && st2 && (fbe < fbt);
    return fbe;
}

// what a track returns: the forward result in LK image coordinates, its status after the gate, err of the forward pass, forward-backward error
struct LKResult {
    float fx, fy, err, fbe;
    int st;
};
// Forward pass, then (fbt >= 0) the backward pass from its result and the gate.
// Forward status 0: `v = v & v2 & (fbe < fbt)` is 0 whatever the backward pass finds, and the point returned is the forward one, so the backward pass
// is skipped unless the caller asked for fbe itself (vh_pyr_lk); in the 4- / 8-tracks-per-wavefront kernels the dead tracks' lanes sit out the pass
// (exec mask), and a wavefront whose tracks are all dead skips it.  (k_lk3 runs the two passes as ONE copy of the track code in a loop.)
template <class LevelFn>
__device__ __forceinline__ void lk_solve(const LKJob& job, float px, float py, LevelFn& lf, LKResult& R)
{
    lk_track(job.I, job.J, px, py, R.fx, R.fy, R.st, R.err, job.err_out != nullptr, lf);
    R.fbe = 0.f;
    if (job.fbt >= 0.f) {
        float bx = 0.f, by = 0.f, e2;
        int st2 = 0;
        if (R.st || job.fbe_out) lk_track(job.J, job.I, R.fx, R.fy, bx, by, st2, e2, false, lf);
        R.fbe = lk_fb_gate(px, py, bx, by, job.fbt, st2, R.st);
    }
}

// ---- kernel prologue and epilogue ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ const LKJob& lk_job_row(const void* job_tab, size_t tab_stride, unsigned row)
{
    return *reinterpret_cast<const LKJob*>(reinterpret_cast<const char*>(job_tab) + (size_t)row * tab_stride);
}

// Launch slot -> point (LKJob::order) and its start point in LK image coordinates; false: the slot is beyond the job's tracks.
// UNIFORM: the slot is the same for the whole workgroup, and the point index and the start position come back as SCALARS (readfirstlane).
// the start point of point `pt` in LK image coordinates
__device__ __forceinline__ void lk_point_start(const LKJob& job, int pt, float& px, float& py)
{
    const float qx = ((gptr_f32)job.p_in)[2 * pt], qy = ((gptr_f32)job.p_in)[2 * pt + 1];
    px = __fsub_rn(__fmul_rn(qx, job.in_scale), job.in_off[0]);
    py = __fsub_rn(__fmul_rn(qy, job.in_scale), job.in_off[1]);
}
template <bool UNIFORM = false>
__device__ __forceinline__ bool lk_slot_start(const LKJob& job, int slot, int& pt, float& px, float& py)
{
    if (slot >= LK_N_OF(job)) return false;
    pt = job.order ? ((gptr_i32)job.order)[slot] : slot;
    if (UNIFORM) pt = __builtin_amdgcn_readfirstlane(pt);
    lk_point_start(job, pt, px, py);
    if (UNIFORM) {
        px = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(px)));
        py = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(py)));
    }
    return true;
}

// map-back of one track to frame coordinates (LKJob::out_mode) and its output stores: ONE thread per track calls this
__device__ __forceinline__ void lk_store_track(const LKJob& job, int pt, float fx, float fy, int st, float err, float fbe)
{
    float ox, oy;
    if (job.out_mode == VH_OUT_SCALE) {
        ox = __fdiv_rn(fx, job.out_scale);
        oy = __fdiv_rn(fy, job.out_scale);
    } else {
        const float ax = __fadd_rn(fx, job.in_off[0]), ay = __fadd_rn(fy, job.in_off[1]);
        if (job.out_mode == VH_OUT_TRANSLATE) {
            ox = __fadd_rn(ax, job.out_off[0]);
            oy = __fadd_rn(ay, job.out_off[1]);
        } else {
            ox = __fadd_rn(__fadd_rn(__fmul_rn(ax, job.T[0]), __fmul_rn(ay, job.T[2])), job.T[4]);
            oy = __fadd_rn(__fadd_rn(__fmul_rn(ax, job.T[1]), __fmul_rn(ay, job.T[3])), job.T[5]);
        }
    }
    job.p_out[2 * pt] = ox;
    job.p_out[2 * pt + 1] = oy;
    job.v_out[pt] = (uint8_t)(st != 0);
    if (job.err_out) job.err_out[pt] = err;
    if (job.fbe_out) job.fbe_out[pt] = fbe;
    if (job.praw_out) { job.praw_out[2 * pt] = fx; job.praw_out[2 * pt + 1] = fy; }
}

// statistics of the tracks one thread answers for (counters spread over VH_LK_STAT_SLOTS lines: see StreamWS::lk_stats)
__device__ __forceinline__ void lk_add_stats(const LKJob& job, unsigned slot, int n_iter, int n_setup)
{
    if (!job.stats) return;
    unsigned long long* st = job.stats + (size_t)(slot & (VH_LK_STAT_SLOTS - 1)) * 16;
    atomicAdd(&st[0], (unsigned long long)n_iter);
    atomicAdd(&st[1], (unsigned long long)n_setup);
}
