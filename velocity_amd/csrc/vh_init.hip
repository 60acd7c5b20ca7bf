// Frame-0 initialisation: cv2.goodFeaturesToTrack(roi, 1000, 0.01, 0, blockSize=5,
// useHarrisDetector=True) and cv2.cornerSubPix(im, p, (5,5), (-1,-1), (EPS+MAX_ITER, 100, 0.001)), vidExample.py:110-115.
//
// ONE detector serves every entry: the k_f0b_* kernels, with the clip (an image or the plate ROI of a frame) as a grid dimension.  vh_good_features and
// vh_good_features2 run it on one whole-image clip, vh_frame0_init is vh_frame0_init_batch with one clip, vh_detect_images (vh_match.hip) runs it on images
// of different sizes.  Sobel sums and the block x block sums of their products are exact integers (scaled once), the response (Harris or the minimum
// eigenvalue) is a fixed float32 expression, the maximum is an order-independent atomic max on an order-preserving integer image of the float.  The
// thresholded 3x3 local maxima are compacted per clip as 64-bit keys (response bits << 32 | pixel index); the max_corners largest are found by a radix
// select and sorted descending (in LDS up to 2048 keys, by rocPRIM's segmented sort above; ties: higher index first, like OpenCV's pointer
// comparison) -- no sort over every pixel.  min_distance >= 1 walks the candidates greedily instead (k_f0b_spread).
// cornerSubPix: one thread per corner runs OpenCV's iteration verbatim (float32 bilinear patch, float64 accumulation in row-major order), so results
// are bit-identical to the CPU restatement; the Gaussian masks are computed once per context on the host (vh_subpix_masks_create).
#include <math.h>
#include <string.h>

#include <cstring>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <vector>

#include "vh_ws.hpp"

__device__ __forceinline__ unsigned f2ord(float f)
{
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned u)
{
    const unsigned b = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __uint_as_float(b);
}

// cornerSubPix of corner q (k_init_subpix, k_f0b_subpix: one thread per corner)
#define SUBPIX_MAXWIN 7
__device__ __forceinline__ void subpix_corner(const uint8_t* im, int w, int h, size_t st, float* pts, int q, int win, int max_iter, double eps2,
                                              const float* mask)
{
    const int ww = 2 * win + 1, pw = ww + 2;
    float buf[(2 * SUBPIX_MAXWIN + 3) * (2 * SUBPIX_MAXWIN + 3)];
    const float tx = pts[2 * q], ty = pts[2 * q + 1];
    float cx = tx, cy = ty;
    int iter = 0;
    double err = 0;
    do {
        // getRectSubPix(8u -> 32f), replicated border
        {
            const float ox = __fsub_rn(cx, (float)(pw - 1) * 0.5f), oy = __fsub_rn(cy, (float)(pw - 1) * 0.5f);
            const int ipx = vh_floor(ox), ipy = vh_floor(oy);
            const float a = __fsub_rn(ox, (float)ipx), b = __fsub_rn(oy, (float)ipy);
            const float a11 = __fmul_rn(__fsub_rn(1.f, a), __fsub_rn(1.f, b)), a12 = __fmul_rn(a, __fsub_rn(1.f, b));
            const float a21 = __fmul_rn(__fsub_rn(1.f, a), b), a22 = __fmul_rn(a, b);
            for (int i = 0; i < pw; i++) {
                const int y0 = min(max(ipy + i, 0), h - 1), y1 = min(max(ipy + i + 1, 0), h - 1);
                for (int j = 0; j < pw; j++) {
                    const int x0 = min(max(ipx + j, 0), w - 1), x1 = min(max(ipx + j + 1, 0), w - 1);
                    float v = __fmul_rn((float)im[(size_t)y0 * st + x0], a11);
                    v = __fadd_rn(v, __fmul_rn((float)im[(size_t)y0 * st + x1], a12));
                    v = __fadd_rn(v, __fmul_rn((float)im[(size_t)y1 * st + x0], a21));
                    v = __fadd_rn(v, __fmul_rn((float)im[(size_t)y1 * st + x1], a22));
                    buf[i * pw + j] = v;
                }
            }
        }
        double a = 0, b = 0, c = 0, bb1 = 0, bb2 = 0;
        for (int i = 0; i < ww; i++) {
            const float* sp = buf + (i + 1) * pw + 1;
            const double py = (double)(i - win);
            for (int j = 0; j < ww; j++) {
                const double m = (double)mask[i * ww + j];
                const double tgx = (double)__fsub_rn(sp[j + 1], sp[j - 1]), tgy = (double)__fsub_rn(sp[j + pw], sp[j - pw]);
                const double gxx = __dmul_rn(__dmul_rn(tgx, tgx), m), gxy = __dmul_rn(__dmul_rn(tgx, tgy), m), gyy = __dmul_rn(__dmul_rn(tgy, tgy), m);
                const double px = (double)(j - win);
                a = __dadd_rn(a, gxx); b = __dadd_rn(b, gxy); c = __dadd_rn(c, gyy);
                bb1 = __dadd_rn(bb1, __dadd_rn(__dmul_rn(gxx, px), __dmul_rn(gxy, py)));
                bb2 = __dadd_rn(bb2, __dadd_rn(__dmul_rn(gxy, px), __dmul_rn(gyy, py)));
            }
        }
        const double det = __dsub_rn(__dmul_rn(a, c), __dmul_rn(b, b));
        if (fabs(det) <= 2.220446049250313e-16 * 2.220446049250313e-16) break;
        const double sc = __ddiv_rn(1.0, det);
        const float nx = (float)__dsub_rn(__dadd_rn((double)cx, __dmul_rn(__dmul_rn(c, sc), bb1)), __dmul_rn(__dmul_rn(b, sc), bb2));
        const float ny = (float)__dadd_rn(__dsub_rn((double)cy, __dmul_rn(__dmul_rn(b, sc), bb1)), __dmul_rn(__dmul_rn(a, sc), bb2));
        const double ex = (double)__fsub_rn(nx, cx), ey = (double)__fsub_rn(ny, cy);
        err = __dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey));
        cx = nx; cy = ny;
        if (cx < 0 || cx >= (float)w || cy < 0 || cy >= (float)h) break;
    } while (++iter < max_iter && err > eps2);
    if (fabsf(__fsub_rn(cx, tx)) > (float)win || fabsf(__fsub_rn(cy, ty)) > (float)win) { cx = tx; cy = ty; }
    pts[2 * q] = cx; pts[2 * q + 1] = cy;
}

__global__ __launch_bounds__(64) void k_init_subpix(const uint8_t* im, int w, int h, size_t st, float* pts, int n, int win, int max_iter, double eps2,
                                                    const float* mask)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    subpix_corner(im, w, h, st, pts, q, win, max_iter, eps2, mask);
}

static int subpix_mask_offset(int win)  // masks of half-sizes 1 .. win-1 come first
{
    int off = 0;
    for (int k = 1; k < win; k++) off += (2 * k + 1) * (2 * k + 1);
    return off;
}

// cornerSubPix's Gaussian window for every half-size (679 floats), computed on the host in OpenCV's float32 order (bit-identical to the CPU
// restatement) and uploaded synchronously: once per context, by vh_ctx_create, so that no frame-0 call ever uploads anything
int vh_subpix_masks_create(float** out)
{
    const int mask_floats = subpix_mask_offset(SUBPIX_MAXWIN + 1);
    VH_CHECK(hipMalloc((void**)out, sizeof(float) * mask_floats));
    float* hm = new float[mask_floats];
    for (int win = 1; win <= SUBPIX_MAXWIN; win++) {
        float* m = hm + subpix_mask_offset(win);
        const int ww = 2 * win + 1;
        for (int i = 0; i < ww; i++) {
            const float y = (float)(i - win) / win, vy = expf(-y * y);
            for (int j = 0; j < ww; j++) {
                const float x = (float)(j - win) / win;
                m[i * ww + j] = (float)(vy * expf(-x * x));
            }
        }
    }
    const hipError_t e = hipMemcpy(*out, hm, sizeof(float) * mask_floats, hipMemcpyHostToDevice);  // synchronous: hm dies here
    delete[] hm;
    if (e != hipSuccess) { (void)hipFree(*out); *out = nullptr; }
    VH_CHECK(e);
    return 0;
}

// needs no detector scratch: the masks belong to the context
extern "C" VH_API int vh_corner_subpix(vh_ctx* c, const uint8_t* im, int w, int h, int stride, float* pts, int n, int win, int max_iter,
                                       double eps, void* stream)
{
    if (!c || win < 1 || win > SUBPIX_MAXWIN || n < 0) return vh_fail(-1, "vh_corner_subpix: bad arguments (window half-size 1..7)");
    if (n == 0) return 0;
    VH_BIND(c, stream);
    max_iter = max_iter < 1 ? 1 : (max_iter > 100 ? 100 : max_iter);
    if (eps < 0) eps = 0;
    hipLaunchKernelGGL(k_init_subpix, dim3((n + 63) / 64), dim3(64), 0, bound_.s, im, w, h, (size_t)stride, pts, n, win, max_iter, eps * eps,
                       c->subpix_mask + subpix_mask_offset(win));
    VH_CHECK(hipGetLastError());
    return 0;
}

// p3 = addcol0(image2world(K, R, t, p).astype(float)) @ R + t (vidExample.py:119, common.py:49-55); vp = insidebbox(p, boxa) (:126, images.py:22-27);
// n_out = 4 + corners found.  float64 throughout (the reference's float32 inverse carries ~1e-7; the contract is 1e-4): H = [R[0:2]; t] @ K, its
// inverse by the adjugate, q = [x y 1] @ inv(H), (X, Y) = q[0:2] / q[2], p3 = X R[0] + Y R[1] + t
// row i < cap of one clip (k_f0b_world); boxa: the clip's boundingRect(q, border 0)
__device__ __forceinline__ void frame0_world_row(int i, int n, const double* K, const int* boxa, const double* R, const float* t, const float* p, double* p3, uint8_t* vp)
{
    if (i >= n) { vp[i] = 0; p3[3 * i] = 0; p3[3 * i + 1] = 0; p3[3 * i + 2] = 0; return; }
    const double td[3] = {(double)t[0], (double)t[1], (double)t[2]};
    double H[9];
    for (int c = 0; c < 3; c++) {
        H[0 + c] = R[0] * K[0 + c] + R[1] * K[3 + c] + R[2] * K[6 + c];
        H[3 + c] = R[3] * K[0 + c] + R[4] * K[3 + c] + R[5] * K[6 + c];
        H[6 + c] = td[0] * K[0 + c] + td[1] * K[3 + c] + td[2] * K[6 + c];
    }
    const double c00 = H[4] * H[8] - H[5] * H[7], c01 = H[5] * H[6] - H[3] * H[8], c02 = H[3] * H[7] - H[4] * H[6];
    const double det = H[0] * c00 + H[1] * c01 + H[2] * c02;
    const double Hi[9] = {c00 / det, (H[2] * H[7] - H[1] * H[8]) / det, (H[1] * H[5] - H[2] * H[4]) / det,
                          c01 / det, (H[0] * H[8] - H[2] * H[6]) / det, (H[2] * H[3] - H[0] * H[5]) / det,
                          c02 / det, (H[1] * H[6] - H[0] * H[7]) / det, (H[0] * H[4] - H[1] * H[3]) / det};
    const float xf = p[2 * i], yf = p[2 * i + 1];
    const double x = (double)xf, y = (double)yf;
    const double q0 = x * Hi[0] + y * Hi[3] + Hi[6];
    const double q1 = x * Hi[1] + y * Hi[4] + Hi[7];
    const double q2 = x * Hi[2] + y * Hi[5] + Hi[8];
    const double X = q0 / q2, Y = q1 / q2;
    p3[3 * i] = X * R[0] + Y * R[3] + td[0];
    p3[3 * i + 1] = X * R[1] + Y * R[4] + td[1];
    p3[3 * i + 2] = X * R[2] + Y * R[5] + td[2];
    vp[i] = (xf > (float)boxa[0] && xf < (float)boxa[1] && yf > (float)boxa[2] && yf < (float)boxa[3]) ? 1 : 0;
}

// boundingRect(x, imshape, border) of a few host points (images.py:9-19; floor on all four edges like the device kernel k_bounding_rect)
static void host_bounding_rect(const float* q, int n, int imw, int imh, int bx, int by, int* roi)
{
    float mnx = q[0], mxx = q[0], mny = q[1], mxy = q[1];
    for (int i = 1; i < n; i++) {
        mnx = fminf(mnx, q[2 * i]); mxx = fmaxf(mxx, q[2 * i]);
        mny = fminf(mny, q[2 * i + 1]); mxy = fmaxf(mxy, q[2 * i + 1]);
    }
    int x0 = (int)floorf(mnx), y0 = (int)floorf(mny);
    const int bw = (int)floorf(mxx) - x0 + 1, bh = (int)floorf(mxy) - y0 + 1;
    int x1 = x0 + bw + bx, y1 = y0 + bh + by;
    x0 -= bx; y0 -= by;
    roi[0] = x0 > 1 ? x0 : 1; roi[1] = x1 < imw ? x1 : imw; roi[2] = y0 > 1 ? y0 : 1; roi[3] = y1 < imh ? y1 : imh;
}

// ---------------------------------------------------------------------------------------------------------------
// The detector and vh_frame0_init_batch: vidExample.py:105-127 for nb clips of one frame size as one launch sequence per chunk of clips.  Every stage
// runs with the clip as a grid dimension; a clip finds its ROI, frame and scratch segment in the chunk's descriptor table (F0Clip).  A clip's results do
// not depend on the clips beside it or on the chunking.  The candidates are compacted per clip and the max_corners largest keys are found by a radix
// select (keys are unique -- the pixel index is part of each -- so their unsigned descending order is a full sort's order).
// ---------------------------------------------------------------------------------------------------------------
#define F0B_TW 64        // Harris / candidate tile: 64 x 16 pixels, 256 threads
#define F0B_TH 16
#define F0B_PIECE 16     // descriptors per upload (one kernel argument of 16 x 128 bytes; kernel arguments end at 4 KB)
#define F0B_SEL_MAX 2048 // max_corners up to this: selected keys sorted in LDS; above: rocPRIM segmented sort
#define F0B_WIN 2048     // k_f0b_spread: candidates per window (sorted in LDS)
#define F0B_EMPTY 0xffffffffu
static const size_t F0B_BUDGET = (size_t)1 << 30;  // the scratch block of a context sized by the first call (include/velocity_hip.h)

// (F0Clip, the descriptor of one clip, and F0Cam, its camera: vh_ws.hpp -- the session's replenishment writes them on the device)
struct F0ClipPiece {
    F0Clip c[F0B_PIECE];
};
struct F0Shared {
    double plate[12];
};
struct F0CamPiece {
    F0Cam c[F0B_PIECE];
};
static_assert(sizeof(F0CamPiece) <= 3072, "one kernel argument (vh_store)");

// Sobel 3x3 (aperture 3, REFLECT_101; the pair (dx, dy) per pixel) into an LDS tile with a (block - 1) halo, response of 64 x 16 pixels, per-clip maximum over the pixels the clip's mask keeps.
// HARRIS: the block x block sums of the products and det - k trace^2 in float32; otherwise the minimum eigenvalue of the same structure tensor (OpenCV's calcMinEigenVal:
// a = sxx s2 / 2, b = sxy s2, c = syy s2 / 2, (a + c) - sqrt((a - c)^2 + b^2), every step rounded to float32).  REFLECT_101 is relative to the clip's
// ROI: a halo entry holds the Sobel pair of the reflected pixel.
template <bool HARRIS>
__global__ __launch_bounds__(256) void k_f0b_harris(const F0Clip* tab, int block, float s2, float kf, float* resp_base, unsigned* cnt)
{
    const F0Clip& C = tab[blockIdx.z];
    const int rw = C.rw, rh = C.rh, tx0 = blockIdx.x * F0B_TW, ty0 = blockIdx.y * F0B_TH;
    if (tx0 >= rw || ty0 >= rh) return;  // the whole tile lies outside this clip's ROI (grid sized for the chunk's largest)
    __shared__ int2 g[(F0B_TH + 14) * (F0B_TW + 14)];
    const int r0 = block / 2, gw = F0B_TW + block - 1, gh = F0B_TH + block - 1;
    const uint8_t* im = C.roi;
    const size_t st = (size_t)C.stride;
    for (int i = threadIdx.x; i < gw * gh; i += 256) {
        const int ly = i / gw, lx = i - ly * gw;
        const int x = vh_reflect101(tx0 - r0 + lx, rw), y = vh_reflect101(ty0 - r0 + ly, rh);
        const int xm = vh_reflect101(x - 1, rw), xp = vh_reflect101(x + 1, rw), ym = vh_reflect101(y - 1, rh), yp = vh_reflect101(y + 1, rh);
        const uint8_t *q0 = im + (size_t)ym * st, *q1 = im + (size_t)y * st, *q2 = im + (size_t)yp * st;
        g[i] = make_int2((q0[xp] - q0[xm]) + 2 * (q1[xp] - q1[xm]) + (q2[xp] - q2[xm]), (q2[xm] - q0[xm]) + 2 * (q2[x] - q0[x]) + (q2[xp] - q0[xp]));
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, x = tx0 + lx;
    float* resp = resp_base + C.seg;
    const uint8_t* mask = C.mask;
    unsigned o = 0u;
    for (int k = 0; k < F0B_TH / 4; k++) {
        const int ly = (threadIdx.x >> 6) + 4 * k, y = ty0 + ly;
        if (x < rw && y < rh) {
            int sxx = 0, sxy = 0, syy = 0;
            for (int j = 0; j < block; j++)
                for (int i = 0; i < block; i++) {
                    const int2 v = g[(ly + j) * gw + lx + i];
                    sxx += v.x * v.x; sxy += v.x * v.y; syy += v.y * v.y;
                }
            float r;
            if (HARRIS) {
                const float a = __fmul_rn((float)sxx, s2), b = __fmul_rn((float)sxy, s2), c = __fmul_rn((float)syy, s2);
                const float tr = __fadd_rn(a, c);
                r = __fsub_rn(__fsub_rn(__fmul_rn(a, c), __fmul_rn(b, b)), __fmul_rn(__fmul_rn(kf, tr), tr));
            } else {
                const float a = __fmul_rn(__fmul_rn((float)sxx, s2), 0.5f), b = __fmul_rn((float)sxy, s2), c = __fmul_rn(__fmul_rn((float)syy, s2), 0.5f);
                const float d = __fsub_rn(a, c);
                r = __fsub_rn(__fadd_rn(a, c), sqrtf(__fadd_rn(__fmul_rn(d, d), __fmul_rn(b, b))));  // (sqrtf: correctly rounded; __fsqrt_rn is not)
            }
            resp[(size_t)y * rw + x] = r;
            if (!mask || mask[(size_t)y * C.mstride + x]) o = max(o, f2ord(r));
        }
    }
    for (int s = 32; s > 0; s >>= 1) o = max(o, (unsigned)__shfl_xor((int)o, s, 64));  // every lane takes part, inside the ROI or not
    if (lx == 0 && o) atomicMax(&cnt[4 * blockIdx.z], o);
}

// the thresholded 3x3 local maxima the clip's mask keeps, appended to the clip's key segment through its counter (one atomic per wavefront)
__global__ __launch_bounds__(256) void k_f0b_candidates(const F0Clip* tab, double quality, const float* resp_base, unsigned long long* keys_base, unsigned* cnt)
{
    const F0Clip& C = tab[blockIdx.z];
    const int rw = C.rw, rh = C.rh, tx0 = blockIdx.x * F0B_TW, ty0 = blockIdx.y * F0B_TH;
    if (tx0 >= rw || ty0 >= rh) return;
    const float* resp = resp_base + C.seg;
    unsigned long long* keys = keys_base + C.seg;
    unsigned* count = &cnt[4 * blockIdx.z + 1];
    const float thr = (float)((double)ord2f(cnt[4 * blockIdx.z]) * quality);
    const int lane = threadIdx.x & 63, x = tx0 + lane;
    const unsigned cap = (unsigned)rw * (unsigned)rh;
    for (int k = 0; k < F0B_TH / 4; k++) {
        const int y = ty0 + (threadIdx.x >> 6) + 4 * k;
        bool hit = false;
        unsigned long long key = 0;
        if (x >= 1 && y >= 1 && x < rw - 1 && y < rh - 1) {
            const float v0 = resp[(size_t)y * rw + x];
            if (v0 > thr) {  // THRESH_TOZERO; survivors are compared with the thresholded neighbours
                float m = v0;
#pragma unroll
                for (int j = -1; j <= 1; j++)
#pragma unroll
                    for (int i = -1; i <= 1; i++) {
                        const float u = resp[(size_t)(y + j) * rw + x + i];
                        if (u > thr && u > m) m = u;
                    }
                hit = v0 == m && v0 != 0.f && (!C.mask || C.mask[(size_t)y * C.mstride + x]);
                key = ((unsigned long long)__float_as_uint(v0) << 32) | (unsigned)(y * rw + x);
            }
        }
        const unsigned long long bal = __ballot(hit);
        if (bal) {
            const int leader = __ffsll((long long)bal) - 1;
            unsigned base = 0;
            if (lane == leader) base = atomicAdd(count, (unsigned)__popcll(bal));
            base = (unsigned)__shfl((int)base, leader, 64);
            const unsigned slot = base + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
            if (hit && slot < cap) keys[slot] = key;
        }
    }
}

// The K-th largest of the keys below `hi` in keys[0:count) (K < their number; 1024 threads): radix select, 8-bit digits from the top byte down, stopping
// as soon as the digit's bin holds exactly the keys still wanted.  The K largest keys below hi are exactly those >= the result.
__device__ __forceinline__ unsigned long long f0b_radix_select(const unsigned long long* keys, unsigned count, unsigned K, unsigned long long hi,
                                                               unsigned* hist, unsigned* s_bin, unsigned* s_krem, unsigned* s_done)
{
    const int tid = threadIdx.x;
    unsigned long long prefix = 0, himask = 0;
    unsigned krem = K;  // keys still wanted among those matching prefix on the bits decided so far
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (unsigned i = tid; i < count; i += 1024) {
            const unsigned long long k = keys[i];
            if (k < hi && ((k ^ prefix) & himask) == 0) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {  // the bin holding rank krem, counted from the top: lane l owns bins 4l .. 4l+3
            const unsigned h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
            const unsigned own = h0 + h1 + h2 + h3;
            unsigned v = own;  // -> sum over lanes >= tid
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned t = (unsigned)__shfl_down((int)v, off, 64);
                if (tid + off < 64) v += t;
            }
            unsigned above = v - own;
            if (above < krem && krem <= above + own) {
                const unsigned hb[4] = {h0, h1, h2, h3};
                for (int q = 3; q >= 0; q--) {
                    if (krem <= above + hb[q]) {
                        *s_bin = 4 * tid + q;
                        *s_krem = krem - above;
                        *s_done = hb[q] == krem - above;
                        break;
                    }
                    above += hb[q];
                }
            }
        }
        __syncthreads();
        prefix |= (unsigned long long)*s_bin << shift;
        himask |= 0xffull << shift;
        krem = *s_krem;
        if (*s_done) break;  // (uniform: read from LDS after the barrier)
    }
    return prefix;
}

// s[0:K) sorted descending in LDS (bitonic over the next power of two, zero padded: real keys are > 0, their response is not +-0); 1024 threads,
// called after the barrier that follows the gather of s
__device__ __forceinline__ void f0b_lds_sort_desc(unsigned long long* s, unsigned K)
{
    const unsigned tid = threadIdx.x;
    unsigned P = 1;
    while (P < K) P <<= 1;
    for (unsigned i = K + tid; i < P; i += 1024) s[i] = 0;
    __syncthreads();
    for (unsigned k = 2; k <= P; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned i = tid; i < P; i += 1024) {
                const unsigned l = i ^ j;
                if (l > i) {
                    const unsigned long long a = s[i], b = s[l];
                    if ((i & k) == 0 ? a < b : a > b) { s[i] = b; s[l] = a; }
                }
            }
            __syncthreads();
        }
}

// Where the detector writes a clip's corners: its row C.out, behind the 4 plate corners q when qhead (vh_frame0_init_batch: p = concatenate((q,
// corners)), vidExample.py:116), from the start otherwise (vh_good_features2).  The count goes to cnt[4 * clip + 2] and, when set, *C.n_out.
__device__ __forceinline__ float* f0b_corner_row(const F0Clip& C, int qhead)
{
    float* p = C.out;
    if (!qhead) return p;
    if (threadIdx.x < 8) p[threadIdx.x] = C.q[threadIdx.x];
    return p + 8;
}

// One workgroup per clip: K = min(candidates, the budget) -- the clip's own when LDS_SORT, the chunk's otherwise; the keys >= the K-th largest
// (f0b_radix_select) are gathered and -- LDS_SORT -- sorted descending in LDS and written as corners + the ROI origin
// (vidExample.py:110-112: `goodFeaturesToTrack(roi, ...) + np.float32([boxb[0], boxb[2]])`: integer-valued float32, exact), or gathered into the clip's segment of `gsel` for the segmented sort.
template <bool LDS_SORT>
__global__ __launch_bounds__(1024) void k_f0b_select(const F0Clip* tab, int max_corners, const unsigned long long* keys_base, unsigned* cnt, int qhead,
                                                     unsigned long long* gsel, int* seg_begin, int* seg_end)
{
    const int clip = blockIdx.x, tid = threadIdx.x;
    const F0Clip& C = tab[clip];
    if (LDS_SORT) max_corners = min(C.max_corners, F0B_SEL_MAX);
    __shared__ unsigned hist[256];
    __shared__ unsigned long long s_sel[LDS_SORT ? F0B_SEL_MAX : 1];
    __shared__ unsigned s_bin, s_krem, s_done, s_n;
    const unsigned npx = (unsigned)C.rw * (unsigned)C.rh;
    const unsigned count = min(cnt[4 * clip + 1], npx), K = min(count, (unsigned)max_corners);
    const unsigned long long* keys = keys_base + C.seg;
    unsigned long long T = 0;  // the selection: every key >= T (exactly K keys)
    if (count > K) T = f0b_radix_select(keys, count, K, ~0ull, hist, &s_bin, &s_krem, &s_done);
    if (tid == 0) s_n = 0;
    __syncthreads();
    unsigned long long* dst = LDS_SORT ? s_sel : gsel + (size_t)clip * max_corners;
    for (unsigned i = tid; i < count; i += 1024) {
        const unsigned long long k = keys[i];
        if (k >= T) {
            const unsigned slot = atomicAdd(&s_n, 1u);
            if (slot < K) dst[slot] = k;
        }
    }
    float* p = f0b_corner_row(C, qhead);
    if (tid == 0) {
        cnt[4 * clip + 2] = K;
        if (C.n_out) *C.n_out = (int)K;
    }
    if (!LDS_SORT) {
        if (tid == 0) { seg_begin[clip] = clip * max_corners; seg_end[clip] = clip * max_corners + (int)K; }
        return;
    }
    f0b_lds_sort_desc(s_sel, K);
    for (unsigned i = tid; i < K; i += 1024) {
        const unsigned idx = (unsigned)(s_sel[i] & 0xffffffffull);
        p[2 * i] = __fadd_rn((float)(idx % (unsigned)C.rw), C.offx);
        p[2 * i + 1] = __fadd_rn((float)(idx / (unsigned)C.rw), C.offy);
    }
}

// corners of the segmented-sort route (max_corners > F0B_SEL_MAX)
__global__ __launch_bounds__(256) void k_f0b_emit(const F0Clip* tab, int max_corners, const unsigned long long* sorted, const unsigned* cnt, int qhead)
{
    const int clip = blockIdx.y;
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cnt[4 * clip + 2]) return;
    const F0Clip& C = tab[clip];
    const unsigned idx = (unsigned)(sorted[(size_t)clip * max_corners + i] & 0xffffffffull);
    float* p = C.out + (qhead ? 8 : 0);
    p[2 * i] = __fadd_rn((float)(idx % (unsigned)C.rw), C.offx);
    p[2 * i + 1] = __fadd_rn((float)(idx / (unsigned)C.rw), C.offy);
}

// goodFeaturesToTrack's minDistance >= 1: walk the candidates in descending key order and keep one iff no corner kept so far lies at squared distance
// < min_distance^2 (`lim`: the smallest integer >= min_distance^2, so an integer d^2 < lim exactly when d^2 < min_distance^2), until max_corners are
// kept.  One 1024-thread workgroup per clip.  The candidates come in windows of up to F0B_WIN keys: the largest keys below the previous window's
// smallest (f0b_radix_select), sorted in LDS.  Wavefront 0 walks a window in chunks of 64, one candidate per lane:
//   - against the corners kept so far: an occupancy grid of cell x cell cells (cell = floor(min_distance), so every conflict lies in the 3 x 3 cells
//     around; a cell holds at most `slots` kept corners: 1 for cell <= 2, else 4, one per quarter, whose diagonal is shorter than min_distance),
//     packed (y << 16 | x).  It lives in the clip's response plane, which k_f0b_candidates was the last to read: gw x gh x slots <= rw x rh words.
//   - against the earlier lanes of the chunk: a 64-bit conflict mask per lane from positions broadcast by v_readlane,
//   - then a wave-uniform serial pass over the surviving lanes in order accepts a lane iff its mask meets no lane accepted before it.
// The result is exactly the sequential greedy walk.
__global__ __launch_bounds__(1024) void k_f0b_spread(const F0Clip* tab, int max_corners, const unsigned long long* keys_base, unsigned* grid_base,
                                                     unsigned* cnt, int qhead, int cell, int slots, int lim)
{
    const int clip = blockIdx.x, tid = threadIdx.x;
    const F0Clip& C = tab[clip];
    __shared__ unsigned hist[256];
    __shared__ unsigned long long s_sel[F0B_WIN];
    __shared__ unsigned s_bin, s_krem, s_done, s_n, s_acc;
    const int rw = C.rw, rh = C.rh;
    const unsigned count = min(cnt[4 * clip + 1], (unsigned)rw * (unsigned)rh);
    const unsigned long long* keys = keys_base + C.seg;
    unsigned* grid = grid_base + C.seg;
    const int gw = (rw + cell - 1) / cell, gh = (rh + cell - 1) / cell;
    for (unsigned i = tid; i < (unsigned)(gw * gh * slots); i += 1024) grid[i] = F0B_EMPTY;
    float* p = f0b_corner_row(C, qhead);
    if (tid == 0) s_acc = 0;
    __syncthreads();
    unsigned long long hi = ~0ull;  // the keys still to walk are those below hi
    unsigned left = count, kept = 0;
    while (left > 0) {
        const unsigned W = min(left, (unsigned)F0B_WIN);
        const unsigned long long T = left > W ? f0b_radix_select(keys, count, W, hi, hist, &s_bin, &s_krem, &s_done) : 0ull;
        if (tid == 0) s_n = 0;
        __syncthreads();
        for (unsigned i = tid; i < count; i += 1024) {
            const unsigned long long k = keys[i];
            if (k >= T && k < hi) {
                const unsigned slot = atomicAdd(&s_n, 1u);
                if (slot < W) s_sel[slot] = k;
            }
        }
        __syncthreads();
        f0b_lds_sort_desc(s_sel, W);
        if (tid < 64) {
            const int lane = tid;
            unsigned na = kept;
            for (unsigned base = 0; base < W && na < (unsigned)max_corners; base += 64) {
                const unsigned i = base + lane;
                const bool valid = i < W;
                const unsigned idx = valid ? (unsigned)(s_sel[i] & 0xffffffffull) : 0u;
                const int y = (int)(idx / (unsigned)rw), x = (int)idx - y * rw;
                const int cx = x / cell, cy = y / cell, cid = cy * gw + cx;
                const unsigned pos = ((unsigned)y << 16) | (unsigned)x;
                bool ok = valid;
                int own = 0;  // corners kept in the lane's own cell
                if (valid) {
                    for (int yy = max(cy - 1, 0); yy <= min(cy + 1, gh - 1); yy++)
                        for (int xx = max(cx - 1, 0); xx <= min(cx + 1, gw - 1); xx++) {
                            const unsigned* g = grid + (size_t)(yy * gw + xx) * slots;
                            for (int q = 0; q < slots; q++) {
                                const unsigned e = g[q];
                                if (e == F0B_EMPTY) break;
                                const int dx = x - (int)(e & 0xffffu), dy = y - (int)(e >> 16);
                                if (dx * dx + dy * dy < lim) ok = false;
                                own += (xx == cx && yy == cy) ? 1 : 0;
                            }
                        }
                }
                unsigned long long conf = 0, same = 0;  // earlier lanes of the chunk within the distance / in the same cell
                for (int j = 0; j < 64; j++) {
                    const unsigned pj = (unsigned)__builtin_amdgcn_readlane((int)pos, j);
                    const int cj = __builtin_amdgcn_readlane(cid, j);
                    const int dx = x - (int)(pj & 0xffffu), dy = y - (int)(pj >> 16);
                    if (j < lane && dx * dx + dy * dy < lim) conf |= 1ull << j;
                    if (j < lane && cj == cid) same |= 1ull << j;
                }
                const unsigned long long cand = __ballot(ok);
                unsigned long long acc = 0;
                unsigned room = (unsigned)max_corners - na;
                for (unsigned long long m = cand; m && room; m &= m - 1) {  // wave-uniform, in key order
                    const int j = __ffsll((long long)m) - 1;
                    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)conf, j);
                    const unsigned hi32 = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(conf >> 32), j);
                    if (!((((unsigned long long)hi32 << 32) | lo) & acc)) { acc |= 1ull << j; room--; }
                }
                if ((acc >> lane) & 1ull) {
                    const unsigned r = na + (unsigned)__popcll(acc & ((1ull << lane) - 1ull));
                    p[2 * r] = __fadd_rn((float)x, C.offx);
                    p[2 * r + 1] = __fadd_rn((float)y, C.offy);
                    const int q = own + __popcll(acc & same);
                    if (q < slots) grid[(size_t)cid * slots + q] = pos;
                }
                na += (unsigned)__popcll(acc);
                __threadfence_block();  // the next chunk's lanes read what this one's wrote
            }
            if (lane == 0) s_acc = na;
        }
        __syncthreads();
        kept = s_acc;
        if (kept >= (unsigned)max_corners) break;
        hi = T;
        left -= W;
    }
    if (tid == 0) {
        cnt[4 * clip + 2] = kept;
        if (C.n_out) *C.n_out = (int)kept;
    }
}

__global__ __launch_bounds__(64) void k_f0b_subpix(const F0Clip* tab, const F0Cam* cam, int b0, int cap, const unsigned* cnt, int max_corners, int win,
                                                   int max_iter, double eps2, const float* mask, float* p_out)
{
    const int clip = blockIdx.y, q = blockIdx.x * 64 + threadIdx.x;
    if (q >= min((int)cnt[4 * clip + 2], max_corners)) return;
    subpix_corner(tab[clip].im, cam[clip].w, cam[clip].h, (size_t)tab[clip].stride, p_out + (size_t)(b0 + clip) * cap * 2 + 8, q, win, max_iter, eps2, mask);
}

// per clip: zero the counters, build the plate-pose job of vh_frame0_init (estimateWorldCameraPose(K, q, plate, findR=True) from x0 = [0, 0, 0, 0, 0, 1])
__global__ __launch_bounds__(64) void k_f0b_setup(const F0Shared* sh, const F0Cam* cam, int b0, int n, int cap, float* p_out, float* t_out, double* R_out, double* res_out,
                                                  unsigned* cnt, int* info, PoseJob* pose)
{
    const int clip = blockIdx.x * 64 + threadIdx.x;
    if (clip >= n) return;
    const size_t b = (size_t)(b0 + clip);
    for (int k = 0; k < 4; k++) cnt[4 * clip + k] = 0;
    PoseJob P;
    for (int i = 0; i < 9; i++) { P.K[i] = cam[clip].K[i]; P.R[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    for (int i = 0; i < 6; i++) P.x0[i] = i == 5 ? 1.0 : 0.0;
    P.p = p_out + b * cap * 2; P.pw = sh->plate; P.p_sel = nullptr; P.pw_sel = nullptr; P.n_ptr = nullptr; P.n = 4; P.mode = 1;
    P.t_out = t_out + 3 * b; P.R_out = R_out + 9 * b; P.res_out = res_out + b; P.p_proj = nullptr; P.info_out = info + 2 * clip;
    pose[clip] = P;
}

__global__ __launch_bounds__(256) void k_f0b_world(const F0Clip* tab, const F0Cam* cam, int b0, int cap, const unsigned* cnt, const double* R_out,
                                                   const float* t_out, const float* p_out, double* p3_out, uint8_t* vp_out, int* n_out)
{
    const int clip = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const size_t b = (size_t)(b0 + clip);
    const int n = min(4 + (int)cnt[4 * clip + 2], cap);
    if (i == 0) n_out[b] = n;
    if (i >= cap) return;
    frame0_world_row(i, n, cam[clip].K, tab[clip].boxa, R_out + 9 * b, t_out + 3 * b, p_out + b * cap * 2, p3_out + b * cap * 3, vp_out + b * cap);
}

// what a caller does ahead of a capture so that the entry it called finds its scratch (the -6 message names it)
static const char* const F0B_RESERVE_ONE = "call vh_init_reserve(ctx, w, h) before capturing";
static const char* const F0B_RESERVE_BATCH = "call vh_init_reserve_batch(ctx, nb, w, h) before capturing";
static const char* const F0B_RESERVE_MATCH = "call vh_match_reserve(ctx, w, h, params) or vh_match_reserve_batch before capturing";
static const char* const F0B_RESERVE_SORT = "make one eager call with this max_corners before capturing";

static size_t batch_clip_bytes(size_t px) { return 12 * px + 24 + sizeof(F0Clip) + sizeof(F0Cam) + sizeof(PoseJob); }

// the two blocks of the scratch as one walk each (sizes only when base is null)
static size_t batch_carve(char* base, int clips, size_t pix, InitBatchScratch& B)
{
    VhCarver A(base);
    const size_t tab_n = (size_t)(clips + F0B_PIECE - 1) / F0B_PIECE * F0B_PIECE;
    B.resp = A.take<float>(pix); B.keys = A.take<unsigned long long>(pix);
    B.cnt = A.take<unsigned>((size_t)4 * clips); B.info = A.take<int>((size_t)2 * clips);
    B.tab = A.take<F0Clip>(tab_n); B.cam = A.take<F0Cam>(tab_n);
    B.shared = A.take<F0Shared>(1); B.pose = A.take<PoseJob>(clips);
    return A.bytes();
}
static size_t batch_sel_carve(char* base, int clips, size_t keys, size_t sort_bytes, InitBatchScratch& B)
{
    VhCarver A(base);
    B.sel = A.take<unsigned long long>(keys); B.sorted = A.take<unsigned long long>(keys);
    B.seg = A.take<int>((size_t)2 * clips); B.sort_tmp = A.take<char>(sort_bytes);  // rocPRIM's temporary storage, last
    B.sort_bytes = sort_bytes; B.sel_cap = keys;
    return A.bytes();
}

// scratch for chunks of up to `clips` (>= 1) clips and `pix` ROI pixels in all (never shrinks): a refused growth leaves it as it was, a failed one empty (explicit_size kept)
static int batch_reserve(vh_ctx* c, int clips, size_t pix, hipStream_t s, const char* remedy)
{
    InitBatchScratch& B = c->init_batch;
    if (B.clips_cap >= clips && B.pix_cap >= pix) return 0;
    clips = clips > B.clips_cap ? clips : B.clips_cap;
    pix = pix > B.pix_cap ? pix : B.pix_cap;
    InitBatchScratch sized;
    const size_t had = B.main.bytes;
    const int r = B.main.reserve(batch_carve(nullptr, clips, pix, sized), s, "frame-0 scratch", remedy);
    if (r && B.main.p) return r;
    if (r) clips = 0, pix = 0;
    // The sort block (its segment table is sized by clips_cap) goes only with a main block that reserve() replaced: capture check made, stream waited for.  Where the
    // rounded size still fitted, reserve() did nothing and no offset moved: the sort block stays, and a new clips_cap makes batch_sel_reserve lay it out again.
    if (B.main.bytes != had) { B.sort.release(); batch_sel_carve(nullptr, 0, 0, 0, B); }
    if (clips != B.clips_cap) B.sel_cap = 0;
    B.clips_cap = clips; B.pix_cap = pix;
    batch_carve(B.main.p, clips, pix, B);
    return r;
}

// the segmented-sort route's block for max_corners above F0B_SEL_MAX
static int batch_sel_reserve(vh_ctx* c, int max_corners, hipStream_t s)
{
    InitBatchScratch& B = c->init_batch;
    const size_t need = (size_t)B.clips_cap * max_corners;
    if (B.sel_cap >= need) return 0;
    if (need > 0x7fffffffu) return vh_fail(-1, "frame-0 detector: clips x max_corners exceeds the segmented sort's range");
    size_t bytes = 0;  // (a size query reads none of its pointers)
    VH_CHECK(rocprim::segmented_radix_sort_keys_desc(nullptr, bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned)need,
                                                     (unsigned)B.clips_cap, (int*)nullptr, (int*)nullptr, 0, 64, 0));
    InitBatchScratch sized;
    const int r = B.sort.reserve(batch_sel_carve(nullptr, B.clips_cap, need, bytes, sized), s, "frame-0 scratch", F0B_RESERVE_SORT);
    if (r && B.sort.p) return r;  // (refused; a block that already held the rounded size was kept and is laid out again: it holds nothing between calls)
    batch_sel_carve(B.sort.p, B.clips_cap, r ? 0 : need, r ? 0 : bytes, B);
    return r;
}

void vh_init_scratch_free(vh_ctx* c)
{
    if (!c) return;
    c->init_batch.main.release(); c->init_batch.sort.release();
    (void)hipFree(c->subpix_mask);
    c->subpix_mask = nullptr;
}

extern "C" VH_API int vh_init_reserve_batch(vh_ctx* c, int nb, int w, int h, void* stream)
{
    if (!c || nb < 1 || w < 1 || h < 1) return vh_fail(-1, "vh_init_reserve_batch: bad arguments");
    VH_BIND(c, stream);
    const int r = batch_reserve(c, nb, (size_t)nb * w * h, bound_.s, F0B_RESERVE_BATCH);
    if (r) return r;
    c->init_batch.explicit_size = 1;
    return 0;
}

// The one-image entries (vh_good_features, vh_good_features2, vh_frame0_init) on an image of up to max(w x h, the context's max_w x max_h) pixels only
// queue kernels after this: scratch for chunks of the size the context already has (at least one clip) and that many pixels.  It leaves the chunking of
// vh_frame0_init_batch alone (explicit_size is vh_init_reserve_batch's).
extern "C" VH_API int vh_init_reserve(vh_ctx* c, int w, int h, void* stream)
{
    if (!c || w < 1 || h < 1) return vh_fail(-1, "vh_init_reserve: bad arguments");
    VH_BIND(c, stream);
    size_t pixels = (size_t)w * h;
    const size_t ctx_px = (size_t)c->max_w * (size_t)c->max_h;
    if (pixels < ctx_px && ctx_px <= ((size_t)1 << 26)) pixels = ctx_px;  // any image the context was created for fits: no growth later
    const int clips = c->init_batch.clips_cap > 1 ? c->init_batch.clips_cap : 1;
    return batch_reserve(c, clips, pixels, bound_.s, F0B_RESERVE_ONE);
}

// The detector's parameters of one call (vh_frame0_init_batch2 / vh_good_features2)
struct F0Detect {
    int max_corners, block, use_harris;
    double quality, k, min_distance;
};

static int f0b_detect_check(const F0Detect& D, int w, int h, const char* fn)
{
    char msg[160];
    if (!std::isfinite(D.min_distance)) {
        snprintf(msg, sizeof(msg), "%s: min_distance must be finite", fn);
        return vh_fail(-1, msg);
    }
    if (D.min_distance >= 1 && (w > 32767 || h > 32767)) {  // k_f0b_spread packs (y << 16 | x) and squares int distances
        snprintf(msg, sizeof(msg), "%s: min_distance >= 1 needs a frame of at most 32767 x 32767", fn);
        return vh_fail(-1, msg);
    }
    return 0;
}

// the detector stages of one chunk of n clips (descriptors at d_tab, their host copies at h, counters zeroed).  A clip brings its own frame stride, corner
// row, count pointer and corner budget, so one chunk may hold images of different sizes (the level images of vh_match_affine_batch).  The per-clip budget is
// served by the in-LDS selection only: the spacing and segmented-sort routes lay their scratch out for one budget and refuse a mixed chunk.
// The tile grid is sized for the chunk's largest ROI; the tiles beyond a smaller clip's ROI return at once.
static int f0b_detect(InitBatchScratch& B, const F0Clip* d_tab, const F0Clip* h, int n, const F0Detect& D, int qhead, hipStream_t s)
{
    int mw = 0, mh = 0, max_corners = 0;
    bool mixed = false;
    for (int i = 0; i < n; i++) {
        mw = h[i].rw > mw ? h[i].rw : mw;
        mh = h[i].rh > mh ? h[i].rh : mh;
        max_corners = h[i].max_corners > max_corners ? h[i].max_corners : max_corners;
        mixed = mixed || h[i].max_corners != h[0].max_corners;
    }
    if (mixed && (D.min_distance >= 1 || max_corners > F0B_SEL_MAX))
        return vh_fail(-1, "batched detector: clips of different corner budgets need min_distance < 1 and budgets of at most 2048");
    const double scale = 1.0 / (4.0 * D.block * 255.0);
    const dim3 tiles((mw + F0B_TW - 1) / F0B_TW, (mh + F0B_TH - 1) / F0B_TH, n);
    if (D.use_harris)
        hipLaunchKernelGGL(k_f0b_harris<true>, tiles, dim3(256), 0, s, d_tab, D.block, (float)(scale * scale), (float)D.k, B.resp, B.cnt);
    else
        hipLaunchKernelGGL(k_f0b_harris<false>, tiles, dim3(256), 0, s, d_tab, D.block, (float)(scale * scale), (float)D.k, B.resp, B.cnt);
    hipLaunchKernelGGL(k_f0b_candidates, tiles, dim3(256), 0, s, d_tab, D.quality, B.resp, B.keys, B.cnt);
    if (D.min_distance >= 1) {  // (minDistance < 1, negative included, spaces nothing, as in cv2)
        const double md = D.min_distance, md2 = md * md;
        const int cell = md >= 32768.0 ? 32768 : (int)floor(md), slots = cell <= 2 ? 1 : 4;
        const int lim = md2 >= 2147483647.0 ? 0x7fffffff : (int)ceil(md2);
        hipLaunchKernelGGL(k_f0b_spread, dim3(n), dim3(1024), 0, s, d_tab, max_corners, B.keys, reinterpret_cast<unsigned*>(B.resp), B.cnt, qhead, cell, slots,
                           lim);
    } else if (max_corners <= F0B_SEL_MAX) {
        hipLaunchKernelGGL(k_f0b_select<true>, dim3(n), dim3(1024), 0, s, d_tab, max_corners, B.keys, B.cnt, qhead, nullptr, nullptr, nullptr);
    } else {
        int* seg_end = B.seg + B.clips_cap;
        hipLaunchKernelGGL(k_f0b_select<false>, dim3(n), dim3(1024), 0, s, d_tab, max_corners, B.keys, B.cnt, qhead, B.sel, B.seg, seg_end);
        size_t bytes = 0;
        const unsigned size = (unsigned)n * (unsigned)max_corners;
        VH_CHECK(rocprim::segmented_radix_sort_keys_desc(nullptr, bytes, B.sel, B.sorted, size, (unsigned)n, B.seg, seg_end, 0, 64, s));
        if (bytes > B.sort_bytes) return vh_fail(-1, "frame-0 detector: segmented sort scratch too small");
        bytes = B.sort_bytes;
        VH_CHECK(rocprim::segmented_radix_sort_keys_desc(B.sort_tmp, bytes, B.sel, B.sorted, size, (unsigned)n, B.seg, seg_end, 0, 64, s));
        hipLaunchKernelGGL(k_f0b_emit, dim3((max_corners + 255) / 256, n), dim3(256), 0, s, d_tab, max_corners, B.sorted, B.cnt, qhead);
    }
    return 0;
}

// stream-ordered upload of n descriptors to d_tab, F0B_PIECE per kernel argument
static int f0b_upload(F0Clip* d_tab, const F0Clip* h, int n, hipStream_t s)
{
    for (int p0 = 0; p0 < n; p0 += F0B_PIECE) {
        F0ClipPiece piece;
        memset(&piece, 0, sizeof(piece));
        for (int i = 0; i < F0B_PIECE && p0 + i < n; i++) piece.c[i] = h[p0 + i];
        VH_CHECK(vh_store(reinterpret_cast<F0ClipPiece*>(d_tab + p0), piece, s));
    }
    return 0;
}

// the cameras of the same n clips, beside their descriptors
static int f0b_upload_cams(F0Cam* d_cam, const vh_clip_camera* h, int n, hipStream_t s)
{
    for (int p0 = 0; p0 < n; p0 += F0B_PIECE) {
        F0CamPiece piece;
        memset(&piece, 0, sizeof(piece));
        for (int i = 0; i < F0B_PIECE && p0 + i < n; i++) {
            for (int k = 0; k < 9; k++) piece.c[i].K[k] = h[p0 + i].K[k];
            piece.c[i].w = h[p0 + i].w; piece.c[i].h = h[p0 + i].h;
        }
        VH_CHECK(vh_store(reinterpret_cast<F0CamPiece*>(d_cam + p0), piece, s));
    }
    return 0;
}

// THE frame-0 sequence (vh_frame0_init_batch3; the other entries replicate one camera): cams = nb host cameras, one per clip
static int frame0_batch_run(vh_ctx* c, int nb, const uint8_t* const* frames_host, const vh_clip_camera* cams, const float* q_host,
                            const double* plate_host, int border_x, int border_y, const F0Detect& D, int subpix_win, int subpix_iter, double subpix_eps,
                            float* p_out, double* p3_out, uint8_t* vp_out, float* t_out, double* R_out, double* res_out, int* n_out, int* roi_host,
                            void* stream, const char* fn, const char* remedy)
{
    // every check before anything is queued
    char msg[160];
    if (!c || !frames_host || !cams || !q_host || !plate_host || !p_out || !p3_out || !vp_out || !t_out || !R_out || !res_out || !n_out) {
        snprintf(msg, sizeof(msg), "%s: null argument", fn);
        return vh_fail(-1, msg);
    }
    const int max_corners = D.max_corners;
    if (nb < 1 || max_corners < 1 || D.block < 1 || D.block > 15 || subpix_win < 1 || subpix_win > SUBPIX_MAXWIN) {
        snprintf(msg, sizeof(msg), "%s: bad arguments", fn);
        return vh_fail(-1, msg);
    }
    int r = 0;
    for (int b = 0; b < nb; b++) {  // every clip's camera
        const int w = cams[b].w, h = cams[b].h;
        if (w < 3 || h < 3 || cams[b].stride < w) {
            snprintf(msg, sizeof(msg), "%s: bad arguments (clip %d: a %d x %d frame with row stride %d)", fn, b, w, h, cams[b].stride);
            return vh_fail(-1, msg);
        }
        char who[96];
        snprintf(who, sizeof(who), "%s: clip %d", fn, b);
        if ((r = f0b_detect_check(D, w, h, b ? who : fn))) return r;
    }
    std::vector<F0Clip> clips(nb);
    std::vector<int> rois(8 * (size_t)nb);  // boxa, boxb of every clip
    size_t max_px = 0;
    for (int b = 0; b < nb; b++) {
        if (!frames_host[b]) {
            snprintf(msg, sizeof(msg), "%s: clip %d has a null frame", fn, b);
            return vh_fail(-1, msg);
        }
        F0Clip& C = clips[b];
        memset(&C, 0, sizeof(C));
        const int w = cams[b].w, h = cams[b].h, stride = cams[b].stride;
        int* boxb = &rois[8 * b + 4];
        host_bounding_rect(q_host + 8 * b, 4, w, h, 0, 0, C.boxa);  // vidExample.py:107
        host_bounding_rect(q_host + 8 * b, 4, w, h, border_x, border_y, boxb);  // :108
        memcpy(&rois[8 * b], C.boxa, sizeof(C.boxa));
        C.rw = boxb[1] - boxb[0];
        C.rh = boxb[3] - boxb[2];
        if (C.rw < 3 || C.rh < 3) {
            snprintf(msg, sizeof(msg), "%s: the plate ROI of clip %d is empty", fn, b);
            return vh_fail(-1, msg);
        }
        C.im = frames_host[b];
        C.roi = frames_host[b] + (size_t)boxb[2] * stride + boxb[0];
        C.offx = (float)boxb[0];
        C.offy = (float)boxb[2];
        for (int i = 0; i < 8; i++) C.q[i] = q_host[8 * b + i];
        C.stride = stride;
        C.max_corners = max_corners;
        C.out = p_out + (size_t)b * (4 + max_corners) * 2;
        const size_t px = (size_t)C.rw * C.rh;
        max_px = px > max_px ? px : max_px;
    }
    VH_BIND(c, stream);
    hipStream_t s = bound_.s;
    InitBatchScratch& B = c->init_batch;
    // (the spacing stage needs no scratch of its own: its occupancy grid reuses the clip's response plane)
    if (B.explicit_size && B.clips_cap > 0) {  // chunks of the reserved size; grown only for a ROI larger than the whole scratch (a scratch lost to a failed growth is sized like a first call's)
        r = batch_reserve(c, B.clips_cap, max_px, s, remedy);
    } else {                // as many clips per chunk as the budget holds
        const size_t fit = F0B_BUDGET / batch_clip_bytes(max_px);
        const int want = (int)(fit < 1 ? 1 : (fit < (size_t)nb ? fit : (size_t)nb));
        r = batch_reserve(c, want, (size_t)want * max_px, s, remedy);
    }
    if (r) return r;
    if (max_corners > F0B_SEL_MAX && D.min_distance < 1 && (r = batch_sel_reserve(c, max_corners, s))) return r;
    if (roi_host) memcpy(roi_host, rois.data(), sizeof(int) * 8 * nb);
    F0Shared sh;
    for (int i = 0; i < 12; i++) sh.plate[i] = plate_host[i];
    F0Shared* d_sh = reinterpret_cast<F0Shared*>(B.shared);
    F0Clip* d_tab = reinterpret_cast<F0Clip*>(B.tab);
    F0Cam* d_cam = reinterpret_cast<F0Cam*>(B.cam);
    VH_CHECK(vh_store(d_sh, sh, s));
    const int cap = 4 + max_corners;
    const int iters = subpix_iter < 1 ? 1 : (subpix_iter > 100 ? 100 : subpix_iter);
    const double eps = subpix_eps < 0 ? 0 : subpix_eps;
    const float* mask = c->subpix_mask + subpix_mask_offset(subpix_win);
    for (int b0 = 0; b0 < nb;) {
        // one chunk: as many clips as the scratch holds, their ROI planes back to back
        int n = 0;
        size_t px = 0;
        while (b0 + n < nb && n < B.clips_cap && n < 65535 && px + (size_t)clips[b0 + n].rw * clips[b0 + n].rh <= B.pix_cap) {  // (grid.z <= 65535)
            F0Clip& C = clips[b0 + n];
            C.seg = px;
            px += (size_t)C.rw * C.rh;
            n++;
        }
        if ((r = f0b_upload(d_tab, &clips[b0], n, s)) || (r = f0b_upload_cams(d_cam, cams + b0, n, s))) return r;
        hipLaunchKernelGGL(k_f0b_setup, dim3((n + 63) / 64), dim3(64), 0, s, d_sh, d_cam, b0, n, cap, p_out, t_out, R_out, res_out, B.cnt, B.info, B.pose);
        r = f0b_detect(B, d_tab, &clips[b0], n, D, 1, s);
        if (r) return r;
        hipLaunchKernelGGL(k_f0b_subpix, dim3((max_corners + 63) / 64, n), dim3(64), 0, s, d_tab, d_cam, b0, cap, B.cnt, max_corners,
                           subpix_win, iters, eps * eps, mask, p_out);
        vh_launch_pose(B.pose, sizeof(PoseJob), n, 1, 4, s);
        hipLaunchKernelGGL(k_f0b_world, dim3((cap + 255) / 256, n), dim3(256), 0, s, d_tab, d_cam, b0, cap, B.cnt, R_out, t_out, p_out, p3_out, vp_out, n_out);
        VH_CHECK(hipGetLastError());
        b0 += n;
    }
    return 0;
}

// the entries of ONE camera (vh_frame0_init, vh_frame0_init_batch, vh_frame0_init_batch2): that camera for every clip
static int frame0_one_camera(vh_ctx* c, int nb, const uint8_t* const* frames_host, int w, int h, int stride, const float* q_host, const double* K_host,
                             const double* plate_host, int border_x, int border_y, const F0Detect& D, int subpix_win, int subpix_iter, double subpix_eps,
                             float* p_out, double* p3_out, uint8_t* vp_out, float* t_out, double* R_out, double* res_out, int* n_out, int* roi_host,
                             void* stream, const char* fn, const char* remedy)
{
    char msg[160];
    if (!K_host) {
        snprintf(msg, sizeof(msg), "%s: null argument", fn);
        return vh_fail(-1, msg);
    }
    vh_clip_camera cam;
    cam.w = w; cam.h = h; cam.stride = stride; cam.k_is_float32 = 0;
    for (int i = 0; i < 9; i++) cam.K[i] = K_host[i];
    const std::vector<vh_clip_camera> cams((size_t)(nb > 0 ? nb : 1), cam);
    return frame0_batch_run(c, nb, frames_host, cams.data(), q_host, plate_host, border_x, border_y, D, subpix_win, subpix_iter, subpix_eps, p_out, p3_out,
                            vp_out, t_out, R_out, res_out, n_out, roi_host, stream, fn, remedy);
}

extern "C" VH_API int vh_frame0_init_batch(vh_ctx* c, int nb, const uint8_t* const* frames_host, int w, int h, int stride, const float* q_host,
                                           const double* K_host, const double* plate_host, int border_x, int border_y, int max_corners, double quality,
                                           int block, double k, int subpix_win, int subpix_iter, double subpix_eps, float* p_out, double* p3_out,
                                           uint8_t* vp_out, float* t_out, double* R_out, double* res_out, int* n_out, int* roi_host, void* stream)
{
    const F0Detect D = {max_corners, block, 1, quality, k, 0.0};
    return frame0_one_camera(c, nb, frames_host, w, h, stride, q_host, K_host, plate_host, border_x, border_y, D, subpix_win, subpix_iter, subpix_eps, p_out,
                             p3_out, vp_out, t_out, R_out, res_out, n_out, roi_host, stream, "vh_frame0_init_batch", F0B_RESERVE_BATCH);
}

extern "C" VH_API int vh_frame0_init_batch2(vh_ctx* c, int nb, const uint8_t* const* frames_host, int w, int h, int stride, const float* q_host,
                                            const double* K_host, const double* plate_host, int border_x, int border_y, int max_corners, double quality,
                                            int block, double k, int use_harris, double min_distance, int subpix_win, int subpix_iter, double subpix_eps,
                                            float* p_out, double* p3_out, uint8_t* vp_out, float* t_out, double* R_out, double* res_out, int* n_out,
                                            int* roi_host, void* stream)
{
    const F0Detect D = {max_corners, block, use_harris ? 1 : 0, quality, k, min_distance};
    return frame0_one_camera(c, nb, frames_host, w, h, stride, q_host, K_host, plate_host, border_x, border_y, D, subpix_win, subpix_iter, subpix_eps, p_out,
                             p3_out, vp_out, t_out, R_out, res_out, n_out, roi_host, stream, "vh_frame0_init_batch2", F0B_RESERVE_BATCH);
}

extern "C" VH_API int vh_frame0_init_batch3(vh_ctx* c, int nb, const uint8_t* const* frames_host, const vh_clip_camera* cams_host, const float* q_host,
                                            const double* plate_host, int border_x, int border_y, int max_corners, double quality, int block, double k,
                                            int use_harris, double min_distance, int subpix_win, int subpix_iter, double subpix_eps, float* p_out,
                                            double* p3_out, uint8_t* vp_out, float* t_out, double* R_out, double* res_out, int* n_out, int* roi_host,
                                            void* stream)
{
    const F0Detect D = {max_corners, block, use_harris ? 1 : 0, quality, k, min_distance};
    return frame0_batch_run(c, nb, frames_host, cams_host, q_host, plate_host, border_x, border_y, D, subpix_win, subpix_iter, subpix_eps, p_out, p3_out,
                            vp_out, t_out, R_out, res_out, n_out, roi_host, stream, "vh_frame0_init_batch3", F0B_RESERVE_BATCH);
}

// frame 0 of one video: the batch of one clip.  Its output layout is the single call's (cap = 4 + max_corners rows, roi_host int[8])
extern "C" VH_API int vh_frame0_init(vh_ctx* c, const uint8_t* im, int w, int h, int stride, const float* q_host, const double* K_host,
                                     const double* plate_host, int border_x, int border_y, int max_corners, double quality, int block, double k,
                                     int subpix_win, int subpix_iter, double subpix_eps, float* p_out, double* p3_out, uint8_t* vp_out, float* t_out,
                                     double* R_out, double* res_out, int* n_out, int* roi_host, void* stream)
{
    const F0Detect D = {max_corners, block, 1, quality, k, 0.0};
    return frame0_one_camera(c, 1, &im, w, h, stride, q_host, K_host, plate_host, border_x, border_y, D, subpix_win, subpix_iter, subpix_eps, p_out, p3_out,
                             vp_out, t_out, R_out, res_out, n_out, roi_host, stream, "vh_frame0_init", F0B_RESERVE_ONE);
}

// one chunk of whole-image clips whose scratch the caller has reserved (batch_reserve: n clips, the sum of their pixels): response planes back to back
static int f0b_run_clips(vh_ctx* c, F0Clip* clips, int n, const F0Detect& D, hipStream_t s)
{
    InitBatchScratch& B = c->init_batch;
    size_t px = 0;
    for (int i = 0; i < n; i++) {
        clips[i].seg = px;
        px += (size_t)clips[i].rw * clips[i].rh;
    }
    if (n > B.clips_cap || px > B.pix_cap) return vh_fail(-1, "batched detector: scratch smaller than the chunk");
    F0Clip* d_tab = reinterpret_cast<F0Clip*>(B.tab);
    int r = f0b_upload(d_tab, clips, n, s);
    if (r) return r;
    VH_CHECK(hipMemsetAsync(B.cnt, 0, sizeof(unsigned) * 4 * n, s));
    return f0b_detect(B, d_tab, clips, n, D, 0, s);
}

// ---- the detector on device-written ROI descriptors (vh_ws.hpp: VhRoiDetect; the session's replenishment) -----------------------------------------------
int vh_roi_detect_reserve(vh_ctx* c, int clips, int w, int h, hipStream_t s, const char* remedy)
{
    return batch_reserve(c, clips, (size_t)clips * (size_t)w * (size_t)h, s, remedy);
}

int vh_roi_detect_scratch(vh_ctx* c, int clips, int w, int h, VhRoiScratch* out)
{
    InitBatchScratch& B = c->init_batch;
    const size_t plane = (size_t)w * (size_t)h;
    if (!B.main.p || B.clips_cap < clips || B.pix_cap < (size_t)clips * plane) return vh_fail(-1, "batched detector: the ROI scratch was not reserved");
    out->tab = reinterpret_cast<F0Clip*>(B.tab); out->cam = reinterpret_cast<F0Cam*>(B.cam); out->cnt = B.cnt; out->plane = plane;
    return 0;
}

int vh_roi_detect_run(vh_ctx* c, int clips, int w, int h, const VhRoiDetect& D, float* rows, int cap, hipStream_t s)
{
    if (clips < 1 || clips > 65535 || D.max_corners < 1 || D.max_corners > F0B_SEL_MAX || D.max_corners + 4 > cap || D.block < 1 || D.block > 15 || D.win < 1 ||
        D.win > SUBPIX_MAXWIN)
        return vh_fail(-1, "batched detector on device ROIs: bad arguments");
    const F0Detect F = {D.max_corners, D.block, D.use_harris, D.quality, D.k, D.min_distance};
    int r = f0b_detect_check(F, w, h, "batched detector on device ROIs");
    if (r) return r;
    VhRoiScratch R;
    if ((r = vh_roi_detect_scratch(c, clips, w, h, &R))) return r;
    // what f0b_detect reads of the host descriptors: the largest ROI (the grid) and the budgets
    std::vector<F0Clip> sized((size_t)clips);
    memset(sized.data(), 0, sizeof(F0Clip) * (size_t)clips);
    for (int i = 0; i < clips; i++) { sized[i].rw = w; sized[i].rh = h; sized[i].max_corners = D.max_corners; }
    if ((r = f0b_detect(c->init_batch, R.tab, sized.data(), clips, F, 0, s))) return r;
    const int iters = D.max_iter < 1 ? 1 : (D.max_iter > 100 ? 100 : D.max_iter);
    const double eps = D.eps < 0 ? 0 : D.eps;
    hipLaunchKernelGGL(k_f0b_subpix, dim3((D.max_corners + 63) / 64, clips), dim3(64), 0, s, R.tab, R.cam, 0, cap, R.cnt, D.max_corners, D.win, iters, eps * eps,
                       c->subpix_mask + subpix_mask_offset(D.win), rows);
    VH_CHECK(hipGetLastError());
    return 0;
}

int vh_detect_reserve(vh_ctx* c, int clips, size_t pixels, hipStream_t s) { return batch_reserve(c, clips, pixels, s, F0B_RESERVE_MATCH); }

// goodFeaturesToTrack (Shi-Tomasi or Harris, min_distance 0, masked) of n images of any sizes, strides and budgets (each at most 2048) as ONE pass of the
// batch kernels; per image bit-identical to vh_good_features2 on it alone.  Scratch: vh_detect_reserve(n, the sum of the images' pixels).
int vh_detect_images(vh_ctx* c, const vh_detect_image* im, int n, double quality, int block, int use_harris, double k, hipStream_t s)
{
    if (n < 1 || n > 65535) return vh_fail(-1, "vh_detect_images: 1 .. 65535 images");  // (grid.z)
    std::vector<F0Clip> clips((size_t)n);
    for (int i = 0; i < n; i++) {
        F0Clip& C = clips[i];
        memset(&C, 0, sizeof(C));
        if (!im[i].im || !im[i].corners || !im[i].count || im[i].w < 3 || im[i].h < 3 || im[i].stride < im[i].w || (im[i].mask && im[i].mask_stride < im[i].w) ||
            im[i].max_corners < 1 || im[i].max_corners > F0B_SEL_MAX)
            return vh_fail(-1, "vh_detect_images: bad image descriptor");
        C.roi = C.im = im[i].im;
        C.rw = im[i].w;
        C.rh = im[i].h;
        C.stride = im[i].stride;
        C.mask = im[i].mask;
        C.mstride = im[i].mask_stride;
        C.max_corners = im[i].max_corners;
        C.out = im[i].corners;
        C.n_out = im[i].count;
    }
    const F0Detect D = {0, block, use_harris ? 1 : 0, quality, k, 0.0};
    return f0b_run_clips(c, clips.data(), n, D, s);
}

// goodFeaturesToTrack of one image: one clip whose ROI is the whole image, origin 0 (fn: the entry that was called)
static int good_features_one(vh_ctx* c, const uint8_t* im, int w, int h, int stride, const uint8_t* mask, int mask_stride, const F0Detect& D, float* corners,
                             int* count, void* stream, const char* fn)
{
    if (!c || !im || !corners || !count || w < 3 || h < 3 || stride < w || (mask && mask_stride < w) || D.max_corners < 1 || D.block < 1 || D.block > 15) {
        char msg[160];
        snprintf(msg, sizeof(msg), "%s: bad arguments", fn);
        return vh_fail(-1, msg);
    }
    int r = f0b_detect_check(D, w, h, fn);
    if (r) return r;
    VH_BIND(c, stream);
    hipStream_t s = bound_.s;
    if ((r = batch_reserve(c, 1, (size_t)w * h, s, F0B_RESERVE_ONE))) return r;
    if (D.max_corners > F0B_SEL_MAX && D.min_distance < 1 && (r = batch_sel_reserve(c, D.max_corners, s))) return r;
    F0Clip C;
    memset(&C, 0, sizeof(C));
    C.roi = C.im = im;
    C.rw = w;
    C.rh = h;
    C.stride = stride;
    C.mask = mask;
    C.mstride = mask_stride;
    C.max_corners = D.max_corners;
    C.out = corners;
    C.n_out = count;
    if ((r = f0b_run_clips(c, &C, 1, D, s))) return r;
    VH_CHECK(hipGetLastError());
    return 0;
}

// the reference's call (vidExample.py:110): Harris, min_distance 0, no mask
extern "C" VH_API int vh_good_features(vh_ctx* c, const uint8_t* im, int w, int h, int stride, int max_corners, double quality, int block,
                                       double k, float* corners, int* count, void* stream)
{
    const F0Detect D = {max_corners, block, 1, quality, k, 0.0};
    return good_features_one(c, im, w, h, stride, nullptr, 0, D, corners, count, stream, "vh_good_features");
}

extern "C" VH_API int vh_good_features2(vh_ctx* c, const uint8_t* im, int w, int h, int stride, const uint8_t* mask, int mask_stride, int max_corners,
                                        double quality, double min_distance, int block, int use_harris, double k, float* corners, int* count, void* stream)
{
    const F0Detect D = {max_corners, block, use_harris ? 1 : 0, quality, k, min_distance};
    return good_features_one(c, im, w, h, stride, mask, mask_stride, D, corners, count, stream, "vh_good_features2");
}
