/*
 * libvelocity_hip -- C ABI of the MI355X-native KLT + NLS hot path of ultralytics/velocity.
 *
 * The reference has no FFI / plugin interface: its boundary is the set of Python call sites in vidExample.py
 * (SURVEY.md section 8b).  Every entry point below names the reference function (file:line) it replaces; the Python
 * binding a maintainer would add is velocity_amd/_lib.py (ctypes) and is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter is marked "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous on it, inputs are
 *     borrowed and never modified, outputs are caller-allocated;
 *   - images are uint8, pixel (x,y) at base[y*stride + x]; points are float32 (x,y) pairs; poses follow the
 *     reference's row-vector layout (uv1 ~ [X Y Z] @ K, X_cam = X_w @ R + t, affine [x y 1] @ T with T 3x2);
 *   - a vh_ctx serves ONE HIP stream at a time: the stateless entry points (vh_pyr_lk, vh_pose, vh_remap_affine, ...) park their small job
 *     descriptors in slot 0 of the workspace they are given, so calls that may overlap on different streams / threads need their own vh_ctx
 *     (both bindings do this: velocity_amd/_lib.py::workspace and vh_torch_ops.cpp keep one per (device, stream)).  The library enforces the rule:
 *     an entry point that is handed another stream than the context's previous call first waits for the work queued through the context on that
 *     previous stream (a serialisation, never a race);
 *   - camera intrinsics K_host are 9 float64 in the reference's MATLAB layout [[fx,0,0],[s,fy,0],[cx,cy,1]] (a float32 K widens exactly);
 *   - return value 0 = success, otherwise a hipError_t (or a negative vh error); vh_last_error() describes it.
 *     Numerical non-convergence is NOT an error: like the reference (NLS.py:126-127,178-179; KLT.py:129) the call
 *     succeeds and reports it through an info/flags output so the host shim can print the same warning.
 */
#ifndef VELOCITY_HIP_H
#define VELOCITY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VH_API __attribute__((visibility("default")))

typedef struct vh_ctx vh_ctx;         /* device workspace for `batch` independent video streams               */
typedef struct vh_session vh_session; /* per-frame tracker state of `batch` streams (vidExample.py loop body) */

/* Lucas-Kanade parameters: cv2 winSize=(win,win), maxLevel, criteria=(EPS|COUNT, max_count, eps)  (KLT.py:106-107) */
typedef struct {
    int win;
    int max_level;
    int max_count;
    double eps;
} vh_lk_params;

/* device pointers to the intermediate results of the last vh_klt_main call of one stream (parity tests) */
typedef struct {
    const float* p_small;     /* n x 2  stage-1 result at full resolution (KLT.py:114-115)  */
    const uint8_t* v_small;   /* n      after the RANSAC inlier gate (KLT.py:117)           */
    const double* t_trans;    /* 2      mean translation (KLT.py:121-123)                   */
    const int* roi;           /* 4      x0,x1,y0,y1 (KLT.py:60)                             */
    const float* p_coarse;    /* n x 2  stage-2 result (KLT.py:124)                         */
    const uint8_t* v_coarse;  /* n                                                          */
    const double* t23;        /* 6      2x3 affine (KLT.py:127)                             */
    const uint8_t* warped;    /* ROI-sized affine warp, row stride = roi width rounded up to a multiple of 4 (KLT.py:73)  */
    const int* flags;         /* 1      bit0: coarse-affine failure (KLT.py:128-130)        */
} vh_klt_stages;

VH_API int vh_version(void);
/* identity of the sources + compiler this binary was built from: "<sha256(csrc, this header, flags)[:24]>-<sha256(hipcc --version)[:8]>"
 * (velocity_amd/_build.py::build_id).  The Python loader refuses a library whose id is not the tree's; bench.py and pytest print it. */
VH_API const char* vh_build_id(void);
VH_API const char* vh_last_error(void);
/* utility: synchronous device -> host copy of a raw device pointer (used to read the stage pointers below) */
VH_API int vh_copy_to_host(void* dst_host, const void* src_dev, size_t bytes, void* stream);

/* ---- workspace ------------------------------------------------------------------------------------------------ */
VH_API int vh_ctx_create(vh_ctx** out, int batch, int max_w, int max_h, int max_pts);
VH_API void vh_ctx_destroy(vh_ctx* ctx);

/* ---- image stages (K1, K2, K8, K9) ---------------------------------------------------------------------------- */
/* cv2.resize(im, (0,0), fx=.25, fy=.25, INTER_NEAREST), utils/KLT.py:111-113.  dst: round(h/4) x round(w/4), dense */
VH_API int vh_resize_quarter(vh_ctx* ctx, const uint8_t* src, int w, int h, int stride, uint8_t* dst, void* stream);
/* frame ingest, optional rescale: cv2.resize(im, (0,0), fx=scale, fy=scale, interpolation=INTER_NEAREST), vidExample.py:99-102.
 * dst: round(h fy) x round(w fx) with row stride dst_stride */
VH_API int vh_resize_nearest(vh_ctx* ctx, const uint8_t* src, int w, int h, int stride, double fx, double fy, uint8_t* dst, int dst_stride,
                             void* stream);
/* frame ingest, cv2.cvtColor(imbgr, cv2.COLOR_BGR2GRAY), vidExample.py:91.
 * bgr: uint8 [h][w][3] with row stride stride_bytes; gray: uint8 [h][w] with row stride gray_stride */
VH_API int vh_bgr2gray(vh_ctx* ctx, const uint8_t* bgr, int w, int h, int stride_bytes, uint8_t* gray, int gray_stride, void* stream);
/* the same pass also writing the quarter-scale image KLTmain starts from (cv2.resize(.25, INTER_NEAREST), KLT.py:111-113): small = round(h/4) x round(w/4),
 * dense (may be NULL: gray only) */
VH_API int vh_ingest_bgr(vh_ctx* ctx, const uint8_t* bgr, int w, int h, int stride_bytes, uint8_t* gray, int gray_stride, uint8_t* small, void* stream);
/* cv2.pyrDown as used inside cv2.calcOpticalFlowPyrLK (KLT.py:45,48).  dst: (h+1)/2 x (w+1)/2, dense */
VH_API int vh_pyr_down(vh_ctx* ctx, const uint8_t* src, int w, int h, int stride, uint8_t* dst, void* stream);
/* meshgrid + affine + cv2.remap(INTER_LINEAR), utils/KLT.py:70-73.  T: host, 3x2 row-major float32.  dst dense ROI */
VH_API int vh_remap_affine(vh_ctx* ctx, const uint8_t* im, int w, int h, int stride, const float* T_host, int x0, int x1, int y0,
                           int y1, uint8_t* dst, void* stream);
/* im[y0+dy:y1+dy, x0+dx:x1+dx] with zero padding outside the frame, utils/KLT.py:65-68 (SURVEY App. B intent) */
VH_API int vh_crop_shift(vh_ctx* ctx, const uint8_t* im, int w, int h, int stride, int x0, int x1, int y0, int y1, int dx, int dy,
                         uint8_t* dst, void* stream);
/* boundingRect(x, imshape, border), utils/images.py:9-19.  roi_out: device int[4] = x0,x1,y0,y1 */
VH_API int vh_bounding_rect(vh_ctx* ctx, const float* p, int n, int imw, int imh, int bx, int by, int* roi_out, void* stream);

/* ---- tracker -------------------------------------------------------------------------------------------------- */
/* cv2calcOpticalFlowPyrLK(im1, im2, p1, None, fbt, **lk), utils/KLT.py:37-51.  fbt < 0 means fbt=None.
 * Outputs: p2 n x 2, v n (uint8 0/1), err n (may be NULL), fbe n (may be NULL).
 * Windows from 3 to 165: a larger one does not fit a workgroup's LDS and is refused (non-zero, vh_last_error names it) before anything is enqueued. */
VH_API int vh_pyr_lk(vh_ctx* ctx, const uint8_t* im1, const uint8_t* im2, int w, int h, int stride1, int stride2, const float* p1,
                     int n, const vh_lk_params* lk_host, float fbt, float* p2, uint8_t* v, float* err, float* fbe, void* stream);
/* cv2.estimateAffine2D(from[valid], to[valid], method=RANSAC), utils/KLT.py:116,127 (deterministic stand-in, see
 * DESIGN.md).  valid may be NULL (all).  Outputs: M device double[6] (2x3), inl device uint8[n], status device int[1]: 1 = model found,
 * 0 = none, -1 = the inliers' refit is out of the representable range (|coordinate| >= 2^31, or a centred coordinate >= sqrt(2^42 / inliers): no
 * inliers, no model). */
VH_API int vh_ransac_affine(vh_ctx* ctx, const float* from, const float* to, const uint8_t* valid, int n, double* M, uint8_t* inl,
                            int* status, void* stream);
/* KLTmain(im, im0, im0_small, p0), utils/KLT.py:99-134, for stream slot `slot` of the workspace.
 * im0_small may be NULL.  Outputs: p_all n x 2 (every point; the shim returns p_all[v]), v n, im_small
 * round(h/4) x round(w/4), flags device int[1] (bit0: "KLT coarse-affine failure", KLT.py:129). */
VH_API int vh_klt_main(vh_ctx* ctx, int slot, const uint8_t* im, const uint8_t* im0, const uint8_t* im0_small, int w, int h, int stride,
                       int stride0, const float* p0, int n, const vh_lk_params* coarse_host, const vh_lk_params* fine_host,
                       float* p_all, uint8_t* v, uint8_t* im_small, int* flags, void* stream);
VH_API int vh_klt_stage_ptrs(vh_ctx* ctx, int slot, vh_klt_stages* out_host);
/* KLTregional(im0, im, p0, T, lk, fbt, translateFlag), utils/KLT.py:55-95.  T_host: 3x2 row-major float32 (host).
 * Outputs: p_out n x 2 (frame coordinates), v_out n, roi_out device int[4] = x0,x1,y0,y1 (may be NULL). */
VH_API int vh_klt_regional(vh_ctx* ctx, const uint8_t* im0, const uint8_t* im, int w, int h, int stride0, int stride, const float* p0,
                           int n, const float* T_host, const vh_lk_params* lk_host, float fbt, int translate, float* p_out,
                           uint8_t* v_out, int* roi_out, void* stream);

/* ---- NLS pose (K11-K13) ---------------------------------------------------------------------------------------- */
/* estimateWorldCameraPose(K, p, p3, t, R, findR), utils/NLS.py:9-33 -> fcnNLS_t (:102-129) / fcnNLS_Rt (:133-183).
 * K_host: 9 doubles (MATLAB layout; a float32 K widens exactly -- estimateWorldCameraPose does K.astype(float), NLS.py:22-24),
 * x0_host: 6 doubles [rpy(R), t], R_host: 9 doubles.
 * Outputs: t_out float[3]; R_out double[9] (findR: float32-rounded rpy2dcm, else R); res_out double[1] = rms(p - p_proj);
 * p_proj double[n x 2] (may be NULL); info int[2] = {iterations, converged}. */
VH_API int vh_pose(vh_ctx* ctx, const double* K_host, const float* p, const double* pw, int n, const double* x0_host,
                   const double* R_host, int findR, float* t_out, double* R_out, double* res_out, double* p_proj, int* info,
                   void* stream);
/* world2image(K, R, t, pw), utils/common.py:58-64.  C_host = [R; t] @ K (4x3 row-major, host).  out n x 2 */
VH_API int vh_world2image(vh_ctx* ctx, const double* C_host, const double* pw, int n, double* out, void* stream);
/* image2world(K, R, t, p), utils/common.py:49-55.  Hi_host = inv([R[0:2]; t] @ K) (3x3, host).  out n x 2 */
VH_API int vh_image2world(vh_ctx* ctx, const double* Hi_host, const double* p, int n, double* out, void* stream);
/* pixel2uvec(K, p), utils/common.py:122-126.  out n x 3 */
VH_API int vh_pixel2uvec(vh_ctx* ctx, double cx, double cy, double f, const double* p, int n, double* out, void* stream);
/* the same when K and p are float32 on the caller's side: numpy then computes (and returns) float32.  p n x 2, out n x 3 float32 */
VH_API int vh_pixel2uvec_f32(vh_ctx* ctx, float cx, float cy, float f, const float* p, int n, float* out, void* stream);

/* ---- triangulation (K15, K16) ---------------------------------------------------------------------------------- */
/* fcn2vintercept(A, U), utils/MSV.py:98-142.  A [nf,3], U [3,nf,nv], out [nv,3] (all device, float64) */
VH_API int vh_two_view_intercept(vh_ctx* ctx, const double* A, const double* U, int nf, int nv, double* out, void* stream);
/* fcnNvintercept(A, U), utils/MSV.py:146-175: N-ray least-squares intersection.  Same layouts. */
VH_API int vh_n_view_intercept(vh_ctx* ctx, const double* A, const double* U, int nf, int nv, double* out, void* stream);
/* fcnMSV1_t(K, P, B, vg, ii), utils/MSV.py:8-49.  P float32 [5,N0,nhist], B float32 [nhist,14], ids = nonzero(vg)
 * (int32, ng entries).  f32_rays: K and P were float32 on the caller's side (numpy then builds the rays in float32).
 * Outputs: x_out float[3], b0 double[ng x 3], info int[2]; U_scratch double[3*(ii+1)*ng]. */
VH_API int vh_msv1_t(vh_ctx* ctx, const double* K_host, const float* P, const float* B, const int* ids, int ng, int N0, int nhist,
                     int ii, int f32_rays, double* U_scratch, float* x_out, double* b0, int* info, void* stream);


/* ---- bundle adjustment (K14) ------------------------------------------------------------------------------------- */
/* fcnNLS_batch(K, P, pw, cw), utils/NLS.py:186-250: dense LM over tie points and cameras 1..nc, +I damping, step 0.9.
 * The host shim applies the track filter and packs z / x exactly as NLS.py:190-203 does:
 *   z [2*nt*(nc+1)] float64 = [all u | all v], camera-major / track-minor;  x [3 nt + 6 nc] = points | cam pos | cam rpy.
 * x is updated in place.  trace [max_iter][2] = (rms(z - zhat), rms(delta)) per iteration (what NLS.py:238 prints),
 * info int[2] = {iterations, converged}.  workspace: vh_nls_batch_workspace(nt, nc) bytes of device memory.
 * nc <= 255 free cameras (the reference has no limit; -1 above).  The reduced camera system is FORMED on the matrix cores -- one 128-wide Schur launch up
 * to 21 cameras, a 256-wide two-pass Schur kernel for 22..42, a materialised Z + K-split SYRK for 43..255 -- and SOLVED by a matrix-core block
 * Gauss-Jordan up to 20 cameras (124 unknowns), a register-resident VALU Gauss-Jordan at 21 cameras (126 unknowns), and from 22 cameras by a
 * left-looking Cholesky, one launch per 32 columns.  The workspace grows with (6 nc)^2 per partial system: ask vh_nls_batch_workspace, never guess. */
VH_API size_t vh_nls_batch_workspace(int nt, int nc);
/* Opt-in (default OFF): replay a repeated whole solve as ONE hipGraph launch.  A captured sequence bakes the device pointers it was captured with
 * (z, x, trace, info, workspace), so the caller promises POINTER STABILITY: the same buffers are passed on every call (a sliding-window solver that
 * owns its arrays; bench.py).  With on = 1 the second call with an identical job descriptor captures (one synchronous instantiate in that call's
 * latency), later ones replay; any other descriptor is launched plainly; at most 8 sequences are kept (least recently used is dropped after a stream
 * synchronisation).  Callers whose buffers come from an allocator per call (the torch ops, the numpy shim) leave it off.  on = 0 also stops the
 * replay of sequences captured earlier. */
VH_API int vh_ba_graph_replay(vh_ctx* ctx, int on);
VH_API int vh_nls_batch(vh_ctx* ctx, const double* K_host, const double* z, double* x, int nt, int nc, int max_iter, double* trace,
                        int* info, void* workspace, size_t workspace_bytes, void* stream);

/* nwin independent fcnNLS_batch problems of the same shape (one sliding window per video stream) solved by ONE launch sequence
 * (grid.y = window): z [nwin][2 nt (nc+1)], x [nwin][3 nt + 6 nc], trace [nwin][max_iter][2], info [nwin][2]; workspace = nwin blocks
 * of workspace_bytes_per_window >= vh_nls_batch_workspace(nt, nc) bytes (a multiple of 256).  Every window takes exactly the steps
 * vh_nls_batch would take on it (its own stop flag included). */
VH_API int vh_nls_batch_multi(vh_ctx* ctx, const double* K_host, const double* z, double* x, int nt, int nc, int nwin, int max_iter,
                              double* trace, int* info, void* workspace, size_t workspace_bytes_per_window, void* stream);

/* vh_nls_batch_multi for windows that keep DIFFERENT numbers of full-length tracks (NLS.py:190: tracks die on each stream's own gates) and have
 * different cameras, still one launch sequence.  nt_win_dev: device int[nwin], 0 <= nt_w <= nt (NULL: nt for every window);  K_win_dev: device
 * double[nwin][9], row-major (NULL: K_host for every window).  Both tables are read on the device when the kernels run: no count comes back to
 * the host, so a kernel queued earlier on the stream may write them.  Every window is laid out for the common nt (the strides of the multi call);
 * rows i >= nt_w of a window are padding, for which the caller gives NaN measurements (z) and any finite point (x).  An unobserved point has zero
 * residual and zero Jacobian rows, so its block of the normal equations is the bare +I damping: it adds exact zeros to the window's reduced camera
 * system, its own step is zero (its rows of x come back byte for byte), and only the two rms divisors nx = 3 nt_w + 6 nc, nz = 2 nt_w (nc + 1) are
 * taken from the true count.  Window w therefore takes the steps vh_nls_batch takes on its first nt_w tracks with its own K, up to the order of
 * the partial sums.  A window with nt_w = 0 is not solved: info {0, 0}, x untouched.  With both tables NULL this is vh_nls_batch_multi, bit for bit. */
VH_API int vh_nls_batch_windows(vh_ctx* ctx, const double* K_host, const double* z, double* x, int nt, int nc, int nwin, const int* nt_win_dev,
                                const double* K_win_dev, int max_iter, double* trace, int* info, void* workspace,
                                size_t workspace_bytes_per_window, void* stream);

/* vh_nls_batch_windows with ANCHORED points: the scale gauge of fcnNLS_batch is held only by the +I damping (camera 0 is fixed and nothing else, and
 * scaling every point and camera position by one factor leaves every reprojection unchanged), so a solve returns the scale its start had.  Points whose
 * coordinates are known -- the licence-plate corners, vidExample.py:116-119 -- pin it.  fixed_dev: device uint8[nwin][nt], non-zero = row i of the
 * window is anchored (NULL: none).  An anchored point's three Jacobian columns are exact zeros: it takes no step (its rows of x come back byte for
 * byte) while its measurements still constrain the cameras that see it.  Nothing else changes: damping, the 0.9 gain, the stop rule and the divisors
 * nx = 3 nt_w + 6 nc, nz of the iteration record (an anchored point still counts as rows of x; its delta is 0).  Flags of padding rows are ignored
 * (their Jacobian is zero already).  The table is read on the device when the kernels run.  With fixed_dev == NULL this is vh_nls_batch_windows. */
VH_API int vh_nls_batch_windows_fixed(vh_ctx* ctx, const double* K_host, const double* z, double* x, int nt, int nc, int nwin, const int* nt_win_dev,
                                      const double* K_win_dev, const uint8_t* fixed_dev, int max_iter, double* trace, int* info, void* workspace,
                                      size_t workspace_bytes_per_window, void* stream);

/* vh_nls_batch_windows_fixed with HUBER weights on the 2-D reprojection error of a measurement pair: plain least squares gives a measurement 30 pixels
 * off the quadratic pull of one 0.1 pixels off, and one such measurement is enough to ruin a speed.  delta_px: the threshold in pixels, finite, >= 0
 * (anything else is refused by name before a launch is queued).  Per iteration, at the state it starts from: s2 = ru^2 + rv^2; a measurement with
 * s2 > delta_px^2 has the weight w = delta_px / sqrt(s2), every other w = 1, and its residual pair and its 18 Jacobian entries are multiplied by
 * sqrt(w) in k_ba_jac, so every route of the BA plan solves (J^T W J + I) delta = J^T W r (iteratively reweighted least squares: the weights are
 * recomputed every iteration).  Unchanged: the +I damping, the 0.9 gain, the stop rule, the divisors nx and nz, "no observation" (exact zeros) and
 * the anchors, with which it composes (an anchored point's own columns are zero, its camera columns and its residual are weighted).  trace[:, 0]
 * stays the UNWEIGHTED rms residual, so f compares with and without the weights.  nout_dev: device int32[nwin][max_iter] or NULL: the number of
 * measurements with s2 > delta_px^2 at the start of every iteration run (0 for the iterations that did not run).  delta_px = 0 is
 * vh_nls_batch_windows_fixed bit for bit (nout all zero); the same workspace size serves it.  Not covered: fcnNLS_batch2, the sharded phases
 * (vh_nls_batch_phase), the per-frame pose solve, other losses (Cauchy, Tukey), an automatic choice of delta_px. */
VH_API int vh_nls_batch_windows_robust(vh_ctx* ctx, const double* K_host, const double* z, double* x, int nt, int nc, int nwin, const int* nt_win_dev,
                                       const double* K_win_dev, const uint8_t* fixed_dev, double delta_px, int* nout_dev, int max_iter, double* trace,
                                       int* info, void* workspace, size_t workspace_bytes_per_window, void* stream);

/* fcnNLS_batch2(K, P, pw, cw), utils/NLS.py:253-328: the constrained sibling -- tie points, ONE joint rotation applied to the
 * points and a straight-line camera trajectory (elevation, azimuth, one range per camera 1..nc; camera 0 at the origin).
 * Same z packing, damping (+I), step (0.9) and stop rule (rms(delta) < 1e-7); the reference runs at most 20 iterations.
 *   x [3 nt + 5 + nc] float64 = points | joint rpy (3) | el, az | ranges (nc)   (NLS.py:274), updated in place.
 * trace / info / workspace as vh_nls_batch (the same workspace size serves both). */
VH_API int vh_nls_batch2(vh_ctx* ctx, const double* K_host, const double* z, double* x, int nt, int nc, int max_iter, double* trace,
                         int* info, void* workspace, size_t workspace_bytes, void* stream);

/* One phase of a point-sharded BA iteration (multi-GPU fcnNLS_batch): this rank owns nt of the nt_total
 * tie points, the nc free cameras are replicated.  phase 0: init; 1: local normal equations -> [S | rhs | sums] span inside
 * the workspace (the caller all-reduces span_doubles float64 at span_offset bytes); 2: solve + update (the caller
 * then all-reduces ONLY sum delta^2 = the span's third-from-last double; sum r^2 was final after phase 1); 3: iteration record (trace, info, stop flag).  rank0 != 0 on one rank. */
VH_API int vh_nls_batch_phase(vh_ctx* ctx, const double* K_host, const double* z, double* x, int nt, int nc, int nt_total, int rank0,
                              int phase, int it, double* trace, int* info, void* workspace, size_t workspace_bytes,
                              size_t* span_offset, size_t* span_doubles, void* stream);

/* ---- frame-0 initialisation ---------------------------------------------------------- */
/* ONE detector and ONE frame-0 sequence serve every entry of this section: the batch kernels of vh_frame0_init_batch, with the clip as a grid
 * dimension.  vh_good_features and vh_good_features2 run the detector on one whole-image clip, vh_frame0_init is vh_frame0_init_batch with nb = 1.
 * Scratch: per context, about 12 bytes per ROI pixel of a chunk of clips, created by the first call that needs it or by vh_init_reserve /
 * vh_init_reserve_batch; the cornerSubPix masks belong to the context from vh_ctx_create on. */
/* cv2.goodFeaturesToTrack(roi, maxCorners, qualityLevel, 0, blockSize=block, useHarrisDetector=True, k), vidExample.py:110: vh_good_features2 with
 * use_harris = 1, min_distance = 0 and no mask (the same code; the response, the candidates and their order are described there).
 * corners: device float [max_corners x 2] (x, y) sorted by response; count: device int[1].  -1: a null pointer, w or h < 3, stride < w,
 * max_corners < 1, block outside 1..15. */
VH_API int vh_good_features(vh_ctx* ctx, const uint8_t* im, int w, int h, int stride, int max_corners, double quality, int block,
                            double k, float* corners, int* count, void* stream);
/* cv2.cornerSubPix(im, pts, (win,win), (-1,-1), (EPS+MAX_ITER, max_iter, eps)), vidExample.py:113-115.  pts refined in place.  Needs no scratch:
 * one kernel launch, legal under stream capture on any context. */
VH_API int vh_corner_subpix(vh_ctx* ctx, const uint8_t* im, int w, int h, int stride, float* pts, int n, int win, int max_iter,
                            double eps, void* stream);

/* The detector scratch of this context (a block: response planes, candidate keys, counters, descriptors) for the one-image entries: created by the first
 * frame-0 call for the image at hand, or explicitly here -- e.g. before a stream capture, inside which it can be neither allocated nor grown (-6;
 * vh_last_error names this call).  After it, vh_good_features, vh_good_features2, vh_corner_subpix and vh_frame0_init on an image (ROI) of up to
 * max(w x h, the context's max_w x max_h) pixels only queue kernels.  It keeps the chunk size the context has (at least one clip) and does not fix it:
 * the chunking of vh_frame0_init_batch is vh_init_reserve_batch's to set.
 * One case it does not cover: max_corners > 2048 (with min_distance < 1) sorts through a second block sized by the budget, which exists only after
 * one eager call with that budget; inside a capture such a call returns -6 until then.  (The first-generation detector, a full sort of every pixel,
 * had no such case.) */
VH_API int vh_init_reserve(vh_ctx* ctx, int w, int h, void* stream);
/* Frame-0 initialisation of one video, vidExample.py:105-127, as ONE device-resident launch sequence (no host round trip between its steps):
 *   boxa / boxb = boundingRect(q, imshape, border=(0,0) / (border_x, border_y))                (:107-108, images.py:9-19; q_host: the 4 clicked corners, host)
 *   p = goodFeaturesToTrack(im[boxb], max_corners, quality, 0, blockSize=block, useHarrisDetector=True, k) + boxb origin      (:109-112)
 *   p = cornerSubPix(im, p, (win, win), (-1,-1), (EPS + MAX_ITER, subpix_iter, subpix_eps))                                   (:113-115)
 *   p = concatenate((q, p))                                                                                                    (:116)
 *   t, R, res = estimateWorldCameraPose(K, q, plate, findR=True)          (:118; plate_host: worldPointsLicensePlate, 4 x 3 float64, host)
 *   p3 = addcol0(image2world(K, R, t, p)) @ R + t                                                                              (:119)
 *   vp = insidebbox(p, boxa)                                                                                                   (:126, images.py:22-27)
 * Outputs (device, sized for 4 + max_corners tracks): p_out [.. x 2] float32, p3_out [.. x 3] float64, vp_out uint8, t_out float[3], R_out double[9]
 * (float32-rounded like NLS.py:180), res_out double[1], n_out int[1] = 4 + corners found (rows beyond it: vp 0, p3 0).  roi_host (may be NULL): host
 * int[8] = boxa, boxb.  The outputs feed vh_session_init directly.
 * This is vh_frame0_init_batch (below) with nb = 1, whose output layout for one clip is exactly this one.  Every argument is checked before anything
 * is queued or written, roi_host included: -1 for a null argument, w or h < 3, stride < w, max_corners < 1, block outside 1..15, subpix_win outside
 * 1..7, or an empty plate ROI (boxb below 3 x 3). */
VH_API int vh_frame0_init(vh_ctx* ctx, const uint8_t* im, int w, int h, int stride, const float* q_host, const double* K_host,
                          const double* plate_host, int border_x, int border_y, int max_corners, double quality, int block, double k,
                          int subpix_win, int subpix_iter, double subpix_eps, float* p_out, double* p3_out, uint8_t* vp_out, float* t_out,
                          double* R_out, double* res_out, int* n_out, int* roi_host, void* stream);
/* (vh_version >= 106) frame-0 initialisation of nb clips of ONE frame size, vidExample.py:105-127 for each, as one device launch sequence per chunk of
 * clips (below).  A clip's results do not depend on the clips beside it: they are what vh_frame0_init (this call with nb = 1) gives for it.
 *   frames_host: host array of nb device pointers (w x h frames, row stride `stride`); q_host: host float [nb][4][2]; K_host, plate_host and every
 *   parameter after them are shared by the batch.  Each clip's boxa / boxb come from its own q, so the ROI sizes may differ between clips.
 *   Outputs (device, clip b in row b, rows dense at cap = 4 + max_corners): p_out [nb][cap][2], p3_out [nb][cap][3], vp_out [nb][cap], t_out [nb][3],
 *   R_out [nb][9], res_out [nb], n_out [nb]; roi_host (may be NULL): host int [nb][8] = boxa, boxb.
 * Every argument is checked before anything is queued: -1 (and no output written) for the checks of vh_frame0_init, nb < 1, a null frame pointer or a
 * clip whose ROI is empty (vh_last_error names the clip).  The candidates of a clip are compacted and its max_corners strongest are found by a radix
 * select (max_corners <= 2048: sorted in LDS; above: a segmented sort) -- no full-ROI sort.
 * Scratch: per context, about 12 bytes per ROI pixel of a chunk.  vh_init_reserve_batch(ctx, nb, w, h) sizes it for nb clips of a w x h ROI and fixes
 * the chunk size: a call with more clips runs in chunks of that many (results do not depend on the chunking).  Without it, the first call sizes the
 * scratch for as many of its clips as fit 1 GiB, later calls grow it the same way.  Once the scratch fits, a call only queues kernels (legal under
 * stream capture); allocation or growth inside a capture returns -6, as does a max_corners above 2048 whose sort scratch does not exist yet (one
 * eager call with that budget creates it). */
VH_API int vh_init_reserve_batch(vh_ctx* ctx, int nb, int w, int h, void* stream);
VH_API int vh_frame0_init_batch(vh_ctx* ctx, int nb, const uint8_t* const* frames_host, int w, int h, int stride, const float* q_host,
                                const double* K_host, const double* plate_host, int border_x, int border_y, int max_corners, double quality,
                                int block, double k, int subpix_win, int subpix_iter, double subpix_eps, float* p_out, double* p3_out,
                                uint8_t* vp_out, float* t_out, double* R_out, double* res_out, int* n_out, int* roi_host, void* stream);

/* (vh_version >= 107) cv2.goodFeaturesToTrack(im, max_corners, quality, min_distance, mask=mask, blockSize=block, useHarrisDetector=use_harris, k) on
 * the batch kernels of vh_frame0_init_batch with one clip.  vh_good_features above is this call with use_harris = 1, min_distance = 0 and no mask:
 * the same code, kept as the entry of the reference's call.
 *   Response: the integer Sobel pair (aperture 3, REFLECT_101) and the block x block sums of its products, exact integers, scaled by
 *   s2 = (float)(scale^2), scale = 1 / (4 block 255): a = sxx s2, b = sxy s2, c = syy s2.  Harris (use_harris != 0): (a c - b b) - (k (a + c)) (a + c);
 *   otherwise the minimum eigenvalue (a = sxx s2 / 2, b = sxy s2, c = syy s2 / 2, (a + c) - sqrt((a - c)^2 + b^2)), float32
 *   with round-to-nearest at every step (a correctly rounded sqrt).  The threshold is quality times the maximum over the pixels where mask != 0 (all pixels without a mask); the
 *   candidates are the interior 3x3 maxima of the thresholded response that the mask keeps, ordered by response (ties: larger pixel index first).
 *   min_distance < 1 (negative included): the first max_corners candidates.  Otherwise a candidate is kept iff no corner kept before it lies at
 *   squared distance < min_distance^2, until max_corners are kept -- for integer positions exactly OpenCV's grid of cvRound(min_distance) cells.
 *   mask: device uint8 w x h (row stride mask_stride), or NULL.  corners: device float [max_corners x 2] (x, y); count: device int[1].
 *   -1: bad arguments, max_corners < 1 included, or a NaN / infinite min_distance.  Scratch: that of vh_frame0_init_batch (one clip of w x h; vh_init_reserve).
 *   Inside a stream capture max_corners > 2048 with min_distance < 1 needs one eager call with that budget first (vh_init_reserve, above). */
VH_API int vh_good_features2(vh_ctx* ctx, const uint8_t* im, int w, int h, int stride, const uint8_t* mask, int mask_stride, int max_corners,
                             double quality, double min_distance, int block, int use_harris, double k, float* corners, int* count, void* stream);
/* (vh_version >= 107) vh_frame0_init_batch with the detector of vh_good_features2 (no mask): use_harris = 0 selects the minimum eigenvalue, min_distance
 * >= 1 spaces the corners.  use_harris = 1, min_distance = 0 gives vh_frame0_init_batch's results bit for bit, through the same kernels.  The spacing
 * stage needs no extra scratch (it reuses the clip's response plane) and handles any max_corners without the segmented sort. */
VH_API int vh_frame0_init_batch2(vh_ctx* ctx, int nb, const uint8_t* const* frames_host, int w, int h, int stride, const float* q_host,
                                 const double* K_host, const double* plate_host, int border_x, int border_y, int max_corners, double quality,
                                 int block, double k, int use_harris, double min_distance, int subpix_win, int subpix_iter, double subpix_eps,
                                 float* p_out, double* p3_out, uint8_t* vp_out, float* t_out, double* R_out, double* res_out, int* n_out,
                                 int* roi_host, void* stream);
/* (vh_version >= 111) the camera of one clip of vh_frame0_init_batch3: its frame size, the row stride of its frame and its intrinsics (K in the layout of
 * K_host above; k_is_float32 states how the caller holds K -- frame 0 computes in float64 either way, the field travels with the camera so that the
 * same record serves vh_session_set_camera). */
typedef struct vh_clip_camera {
    int w, h, stride, k_is_float32;
    double K[9];
} vh_clip_camera;
/* (vh_version >= 111) vh_frame0_init_batch2 for clips of DIFFERENT cameras: cams_host, a host array of nb vh_clip_camera, takes the place of the shared
 * w, h, stride and K_host; the plate and every detector parameter stay shared by the batch.  Clip b's boundingRect, its argument checks, its cornerSubPix
 * and its pose / image2world use cams_host[b] alone.  This is THE frame-0 implementation: vh_frame0_init, vh_frame0_init_batch and vh_frame0_init_batch2
 * are this call with one camera replicated (the same kernels, the same results bit for bit), and a clip's outputs are what vh_frame0_init gives for it
 * alone.  Outputs, chunking and scratch as vh_frame0_init_batch (vh_init_reserve_batch(ctx, nb, w, h) with the LARGEST w x h of the clips to come).
 * Every argument is checked before anything is queued: -1 for what vh_frame0_init_batch2 refuses, with vh_last_error naming the clip whose camera has
 * w or h < 3, stride < w, a null frame or an empty plate ROI. */
VH_API int vh_frame0_init_batch3(vh_ctx* ctx, int nb, const uint8_t* const* frames_host, const vh_clip_camera* cams_host, const float* q_host,
                                 const double* plate_host, int border_x, int border_y, int max_corners, double quality, int block, double k,
                                 int use_harris, double min_distance, int subpix_win, int subpix_iter, double subpix_eps, float* p_out, double* p3_out,
                                 uint8_t* vp_out, float* t_out, double* R_out, double* res_out, int* n_out, int* roi_host, void* stream);

/* ---- recovery by feature matching (vh_version >= 108) ------------------------------------------------------------ */
/* Parameters of vh_match_affine; NULL means the defaults in brackets.  levels [5]: images per frame at scale 2^(-l/4), 1..8; query_per_level [500] /
 * train_per_level [1000]: corner budget per level of im1 / im2, 1..2048; block [5]: blockSize of the detector; border_x, border_y [50, 50]: border of the
 * query ROI boundingRect(p1, shape, border); a match is good iff ratio_den * d1 < ratio_num * d2 [4, 5]; min_good [10]: fewer good matches report
 * status 0; quality [0.01]: qualityLevel of the detector. */
typedef struct {
    int levels, query_per_level, train_per_level, block, border_x, border_y, ratio_num, ratio_den, min_good;
    double quality;
} vh_match_params;
/* estimateAffine2D_SURF(im1, im2, p1, scale=1), utils/KLT.py:10-33 (stand-in, see DESIGN.md "Recovery by feature matching"): the affine im1 -> im2 from
 * multi-scale Shi-Tomasi corners (the detector of vh_good_features2 under a mask: 16 px from every edge, im1 also inside boundingRect(p1) scaled to the
 * level), 256-bit intensity-comparison descriptors on the 5x5 box sum of each level image, brute-force 2-nearest-neighbour Hamming matching with the
 * ratio test, and vh_ransac_affine on the good pairs.  ONE device-resident launch sequence: no count leaves the device between detection and RANSAC.
 * Deviation from the reference: it grows the ROI border by 10 px in a host loop until it has 10 good matches, without a bound; this call makes one pass
 * with the fixed border and reports status 0 instead.
 *   p1: device float [n x 2], n >= 1.  cap = levels * query_per_level must not exceed the context's max_pts.
 *   Outputs (device): M double[6] (2x3; zeros without a model), inl uint8[cap] (inlier flag of good pair k; zeros beyond the good pairs),
 *   pairs float[cap x 4] (may be NULL): good pair k = (query x, y, train x, y) in level-0 coordinates, query order,
 *   info int[4] = status (1 model found, 0 none), good pairs, inliers, query keypoints.
 * -1 (nothing queued): null pointers, n < 1, parameters out of the ranges above, a frame whose smallest level is below 3 x 3, cap > max_pts. */
VH_API int vh_match_affine(vh_ctx* ctx, const uint8_t* im1, const uint8_t* im2, int w, int h, int stride1, int stride2, const float* p1, int n,
                           const vh_match_params* params_host, double* M, uint8_t* inl, float* pairs, int* info, void* stream);
/* scratch of vh_match_affine (level images, masks, box sums, keypoints, descriptors; about 20 bytes per frame pixel) and of the detector it drives:
 * created by the first call, or here -- e.g. before a stream capture, inside which it cannot grow (-6). */
VH_API int vh_match_reserve(vh_ctx* ctx, int w, int h, const vh_match_params* params_host, void* stream);
/* (vh_version >= 109) vh_match_affine for nb frame pairs of ONE frame size as one launch sequence: every matcher kernel runs once with the pair as a
 * grid dimension, the detector makes one pass over the 2 x levels x nb level images, RANSAC is one launch over nb jobs (vh_match_affine is the batch of
 * one).  im1_host, im2_host, p1_host: HOST arrays of nb device pointers, n_host: host int[nb].  Outputs (device): M double[nb][6], inl uint8[nb][cap],
 * pairs float[nb][cap][4] (may be NULL), info int[nb][4]; each pair's are bit-identical to vh_match_affine on that pair alone.
 * vh_match_stage_ptrs then shows the LAST pair of the call.
 * -1 (nothing queued): what vh_match_affine refuses, nb < 1, nb x 2 x levels > 65535, a null entry in a pointer array, an n below 1. */
VH_API int vh_match_affine_batch(vh_ctx* ctx, int nb, const uint8_t* const* im1_host, const uint8_t* const* im2_host, int w, int h, int stride1,
                                 int stride2, const float* const* p1_host, const int* n_host, const vh_match_params* params_host, double* M, uint8_t* inl,
                                 float* pairs, int* info, void* stream);
/* vh_match_reserve for calls of up to nb pairs (the scratch is per pair: about 20 bytes per frame pixel, and 34 more in the detector) */
VH_API int vh_match_reserve_batch(vh_ctx* ctx, int nb, int w, int h, const vh_match_params* params_host, void* stream);
/* device pointers to the intermediate results of the last vh_match_affine call of a context (parity tests).  Image 0 is the query (im1), 1 the train image */
typedef struct {
    const float* kp[2][8];    /* detector output of every level, level coordinates (x, y), cnt[image][level] rows          */
    const int* cnt;           /* [2][8] keypoints per image and level                                                      */
    const float* pos[2];      /* level-0 positions of all keypoints of an image, level-major, detector order in a level    */
    const uint8_t* desc[2];   /* 32 bytes per keypoint, same order (np.packbits bit order)                                 */
    const int* nn;            /* per query keypoint: nearest train index, its distance, second nearest index, its distance */
    const uint8_t* good;      /* per query keypoint: passed the ratio test                                                 */
    const int* roi;           /* 4: boundingRect(p1, shape, border) = x0, x1, y0, y1                                       */
    int levels, lw[8], lh[8]; /* level sizes                                                                               */
} vh_match_stages;
VH_API int vh_match_stage_ptrs(vh_ctx* ctx, vh_match_stages* out_host);
/* the descriptor's sampling pattern as compiled into the kernel: out_host int[256 x 4] = (ax, ay, bx, by) */
VH_API int vh_match_pairs(int* out_host);
/* kernels of vh_match.hip queued by this process so far (tests: a default KLTmain queues none) */
VH_API long long vh_match_launch_count(void);

/* ---- tracker session: the frame loop body of vidExample.py:133-160 on the device, for ctx->batch streams ------- */
/* device pointers into the state of one stream (read with vh_copy_to_host / torch) */
typedef struct {
    const uint8_t* vg;      /* N0      global validity mask (vidExample.py:125,135)            */
    const uint8_t* vp;      /* N0      pose-track mask (vidExample.py:126,136,160)             */
    const float* p;         /* n_cur x 2 compacted current points                              */
    const int* ids;         /* n_cur   global ids of the rows of p                             */
    const double* p3;       /* N0 x 3  world points                                            */
    const float* P;         /* history (vidExample.py:128-129,151-153), FRAME-MAJOR [nhist][5][N0]: entry (row, track, frame) at
                             * P[(frame * 5 + row) * N0 + track]; the reference's array is its transpose to [5,N0,nhist]  */
    const float* B;         /* [nhist,14]  (vidExample.py:44,142-146)                          */
    const float* S;         /* [nhist,9]   (vidExample.py:45,164)                              */
    const int* n_cur;
    const int* n_pose;
    const float* t;         /* 3       last pose translation                                   */
    const double* res;      /* 1       last rms reprojection residual                          */
    const int* frame_i;
    const int* klt_flags;
    const int* pose_info;   /* 2       iterations, converged                                   */
    const int* sel_pw;      /* n_pose  global ids of the pose tracks                           */
    const double* p_proj;   /* n_pose x 2                                                      */
    /* (vh_version >= 104) layout of P in floats: entry (row, track, frame) at P[row * P_row_stride + track * P_track_stride + frame * P_frame_stride].
     * Today (N0, 1, 5 N0) = frame-major [nhist][5][N0]; the reference's [5,N0,nhist] would read (N0 nhist, nhist, 1).  A C consumer indexes
     * through these, never through a remembered layout (version 103 changed it from the reference's, silently for such a consumer). */
    size_t P_row_stride, P_track_stride, P_frame_stride;
    int n0, nhist;
} vh_session_view;

/* w x h: the LARGEST frame a slot of the session can hold, and with K_host / k_is_float32 the camera every slot starts with (vh_session_set_camera gives a
 * slot its own).  K_host: 9 doubles; k_is_float32 != 0: the caller's K array is float32 (vidExample.py:29-33), so fcnMSV1_t builds its rays in
 * float32 like numpy does.  n0 = number of initial tracks, nhist = number of frames of history (P, B, S rows),
 * msv_frame = frame index at which fcnMSV1_t re-triangulates (vidExample.py:155; <= 0 disables; a frame the history reaches -- < nhist -- must be below
 * 2048: -1 otherwise, the limit of vh_msv1_t). */
VH_API int vh_session_create(vh_session** out, vh_ctx* ctx, int n0, int nhist, int w, int h, const double* K_host,
                             int k_is_float32, const vh_lk_params* coarse_host, const vh_lk_params* fine_host, int msv_frame);
VH_API void vh_session_destroy(vh_session* s);
/* (vh_version >= 111) the camera of ONE slot: frame size w x h and intrinsics (K_host: 9 doubles; k_is_float32 as in vh_session_create) that the slot's
 * next vh_session_init / vh_session_init_dev and the steps after it use -- the slot's frames, its quarter-scale images, its pose fit and its fcnMSV1_t.
 * The streams of a session may so differ in resolution and focal length; every launch of a step is sized for the session's w x h and a smaller stream's
 * surplus workgroups leave at once.  Stream-ordered (one small launch, no host wait): legal between two steps while earlier steps are still queued; the
 * slot's state of its previous clip is void from the call on (initialise it again before its next active step).  A slot that never gets the call keeps
 * the session's w, h and K.  -1 (vh_last_error names the slot and the limit; nothing written): a bad slot, a null K_host, w or h below 4, w above the
 * session's w or h above its h (a portrait frame does not fit a landscape session of the same area: each side must fit). */
VH_API int vh_session_set_camera(vh_session* s, int slot, int w, int h, const double* K_host, int k_is_float32, void* stream);
/* frame-0 state of stream `slot` (vidExample.py:116-131): p n0 x 2, p3 n0 x 3, vp n0 (device); t0_host = plate pose t.  frame0: the slot's w x h frame
 * (vh_session_set_camera; the session's size without it) with rows `stride` >= w bytes apart -- the row stride of every later frame of the slot too. */
VH_API int vh_session_init(vh_session* s, int slot, const uint8_t* frame0, int stride, const float* p, const double* p3,
                           const uint8_t* vp, const float* t0_host, float time0, float frame_no, float res0, void* stream);
/* the same straight from the outputs of vh_frame0_init, all still on the device (no read-back between frame 0 and the loop): t0_dev float[3], res0_dev
 * double[1], n_dev int[1] = number of frame-0 tracks (may be NULL: n0).  With *n_dev < n0 the session runs the first *n_dev rows; the rest are tracks
 * that never existed (vg = 0, history NaN, S[0,2] = *n_dev). */
VH_API int vh_session_init_dev(vh_session* s, int slot, const uint8_t* frame0, int stride, const float* p, const double* p3, const uint8_t* vp,
                               const float* t0_dev, const double* res0_dev, const int* n_dev, float time0, float frame_no, void* stream);
/* one frame for every stream: frames_dev = device array of ctx->batch frame pointers (stream b's frame has that slot's size and the row stride of its frame 0) */
VH_API int vh_session_step(vh_session* s, const uint8_t* const* frames_dev, float time_s, float frame_no, void* stream);
/* the same with one timestamp / frame number PER STREAM (device float[batch] each): independent videos with their own
 * CAP_PROP_POS_MSEC / frame counters (vidExample.py:142: B[i,12:14]).  The frames of step i must stay alive until step i+1 has
 * run (they are that step's im0). */
VH_API int vh_session_step_v(vh_session* s, const uint8_t* const* frames_dev, const float* time_s_dev, const float* frame_no_dev,
                             void* stream);
/* (vh_version >= 110) vh_session_step_v in which a stream may SIT THE STEP OUT: two cameras of different frame rates, a slot whose clip has ended while
 * its neighbours run on, a slot no clip has been given yet.  Idleness is stated once per side and the two must agree:
 *   - the DEVICE learns it from the frame table: frames_dev[b] == NULL <=> stream b is idle;
 *   - the HOST learns it from active_host, a host uint8[batch]: active_host[b] == 0 <=> stream b is idle (the library mirrors each stream's frame
 *     counter on the host to decide whether the MSV launches are queued; it never reads the device table).
 * The step is the same fixed launch sequence as ever; an idle stream is a descriptor with empty extents (no tracks, nothing to resize, no pyramid to
 * build) that every launch passes by.  After the step an idle stream's whole state -- masks, points, history, records, frame counter, previous frame,
 * quarter-scale images, klt_flags, recovery counters -- is byte for byte what it was, and nothing of it was used: a slot that was never initialised is a
 * legal idle stream.  A stream parked at its MSV frame is NOT re-triangulated when a neighbour reaches its own, and with the recovery on it reports no
 * failure whatever flag its last active step left.  time_s_dev[b] / frame_no_dev[b] of an idle stream are not read.
 * Frame lifetime: the frame of a stream's active step is read again (as im0) by that stream's NEXT ACTIVE step and must stay alive until that step has
 * run, however many idle steps lie between.
 * vh_session_step and vh_session_step_v are unchanged: every stream steps, every frame pointer must be non-NULL; for an active stream the three entries
 * compute bit-identical results. */
VH_API int vh_session_step_some(vh_session* s, const uint8_t* const* frames_dev, const uint8_t* active_host, const float* time_s_dev,
                                const float* frame_no_dev, void* stream);
/* (vh_version >= 110) everything a stream hands back, packed into ONE contiguous device record by one launch, for one device-to-host copy per finished
 * clip (vh_session_ptrs + one vh_copy_to_host per array stops the device fourteen times).  The fields are BYTE OFFSETS into the record; a C consumer
 * reads through them, never through a remembered layout.  Every array starts on a multiple of 8 bytes. */
typedef struct {
    size_t bytes;                               /* size of the record                                                         */
    size_t n_cur, n_pose, frame_i, klt_flags;   /* int32 each                                                                 */
    size_t pose_info;                           /* int32[2]   iterations, converged                                           */
    size_t t;                                   /* float32[3] last pose translation                                           */
    size_t res;                                 /* float64    last rms reprojection residual                                  */
    size_t vg, vp;                              /* uint8[n0]                                                                  */
    size_t ids;                                 /* int32[n0]  rows [0, n_cur) as vh_session_view::ids, -1 behind them         */
    size_t p;                                   /* float32[n0][2]  rows [0, n_cur) as vh_session_view::p, 0 behind them       */
    size_t p3;                                  /* float64[n0][3]                                                             */
    size_t B, S;                                /* float32[nhist][14], float32[nhist][9]                                      */
    size_t P;                                   /* float32[5][n0][nhist]: the REFERENCE's order (vidExample.py:128), transposed on the device */
    int n0, nhist;
} vh_session_record;
/* size in bytes of a record of this session (0 and vh_last_error on a NULL session); layout_host (may be NULL) receives the offsets */
VH_API size_t vh_session_export_size(const vh_session* s, vh_session_record* layout_host);
/* packs stream `slot` into rec_dev (device memory, vh_session_export_size bytes, 8-byte aligned) on `stream`: one launch, no scratch, no wait */
VH_API int vh_session_export(vh_session* s, int slot, void* rec_dev, void* stream);

/* Anchored points of a slot's clip: world points whose coordinates are known -- the licence-plate corners, tracks 0..3 of every clip, whose frame-0
 * coordinates come from the plate's size (vidExample.py:116-119) -- and which vh_session_refine / vh_session_refine_windows therefore hold fixed
 * (vh_nls_batch_windows_fixed): they pin the scale of the adjustment, which is otherwise held only by the +I damping.  A step neither reads nor writes them.
 *   ids_host  n distinct track ids in [0, n0);  n = 0 clears the slot's anchors
 *   xyz_host  their coordinates, float64[n][3], in the frame of the clip's camera 0;  NULL: the slot's current p3 rows of those ids, taken in stream
 *             order (after a device-side frame-0 batch, and BEFORE the re-triangulation frame: fcnMSV1_t overwrites p3 of the surviving tracks)
 * Queues one clear and one small launch per 96 anchors on `stream`: no upload, no host wait.  A refined window starts an anchored track at the
 * anchor's coordinates + B[first, 3:6] in place of p3 and flags its row; an anchored track that is not alive in a window is simply not among its
 * tracks, and a window with nfix = 0 is solved free and says so.  What anchoring does NOT do: for first > 0 the anchors are placed by the tracker's
 * own B[first, 3:6]; windows are still separate solves; the plate's frame-0 pose error is inherited.  vh_session_init / vh_session_init_dev clear
 * the slot's anchors: a new clip is a new plate.  Returns -1 with vh_last_error naming the cause, and nothing queued, for: a slot outside the session
 * or not initialised, n < 0 or n > n0, an id outside [0, n0), an id given twice. */
VH_API int vh_session_set_anchors(vh_session* s, int slot, const int* ids_host, int n, const double* xyz_host, void* stream);
/* the slot's anchors read back, ascending id: ids_host int[n0], xyz_host float64[n0][3] (either may be NULL).  Returns their number (-1 on bad
 * arguments).  Waits for the device: an accessor for tests. */
VH_API int vh_session_anchors(vh_session* s, int slot, int* ids_host, double* xyz_host);

/* Bundle adjustment of finished clips, straight from the session (default OFF: nothing calls it unless asked).  The refinement the reference's author
 * sketched at vidExample.py:157 -- fcnNLS_batch(K, P[:, :, 0:i], p3, B[0:i, 3:6]), utils/NLS.py:186-250 -- for slots whose clips have had all their nf
 * frames (frame counter nf - 1): tracks = the slot's surviving tracks (vh_session_view::ids, the tracks NLS.py:190 keeps: ascending id), z from the
 * float32 history (NLS.py:198-199), x0 = [p3[ids] | B[1:nf, 3:6] | 0] (NLS.py:202-203), K the slot's own.  The slots of one call are the windows of ONE
 * vh_nls_batch_windows launch sequence (nt = n0, nc = nf - 1): their track counts and cameras may differ, their nf may not (other lengths: another
 * call, or windows of one length through vh_session_refine_windows below).  One record per slot, byte offsets as in vh_session_record: */
typedef struct {
    size_t bytes;                               /* size of a record (a multiple of 8)                                         */
    size_t nt, iterations, converged;           /* int32 each: tracks solved, LM iterations taken, rms(delta) < 1e-7 reached   */
    size_t ids;                                 /* int32[n0]        rows [0, nt) global track ids, -1 behind them             */
    size_t pw;                                  /* float64[n0][3]   rows [0, nt) refined world points, NaN behind them        */
    size_t cw;                                  /* float64[nhist][3] refined camera positions: row 0 zero, rows >= nf NaN     */
    size_t dr, speed;                           /* float64[nhist]   dr_i = |cw_i - cw_(i-1)|, speed_i = dr_i / (B[i,12] - B[i-1,12]) * 3.6 with the float32
                                                                    time difference of vidExample.py:142; entry 0 and entries >= nf NaN */
    size_t speed_mean, speed_std;               /* float64: mean and (population) std of speed[1:nf] (vidExample.py:177)      */
    size_t f_first, f_last;                     /* float64: rms residual (pixels) of the first and of the last iteration, NaN when none ran */
    size_t trace;                               /* float64[max_iter][2] rms(z - zhat), rms(delta) per iteration, 0 behind them */
    int n0, nhist, max_iter;
    size_t nfix;                                /* int32: anchored points among the nt tracks (vh_session_set_anchors); 0: solved free.  In the record it is
                                                   the word behind `converged`, which was padding: no offset moved.  Appended HERE, behind every older
                                                   member, so a caller compiled against the older header reads what it always read */
} vh_refine_record;
/* size in bytes of a record for max_iter iterations (0 and vh_last_error on bad arguments); layout_host (may be NULL) receives the offsets */
VH_API size_t vh_session_refine_size(const vh_session* s, int max_iter, vh_refine_record* layout_host);
/* bytes of device scratch a vh_session_refine call of nslots slots and nf frames needs (0 and vh_last_error on bad arguments) */
VH_API size_t vh_session_refine_workspace(const vh_session* s, int nslots, int nf);
/* Queues kernels only -- pack, the BA launch sequence, unpack -- on `stream`: no allocation, no host wait, legal between two steps.  It reads the
 * session and writes nothing of it: every stream steps on as if the call had not happened.  recs_dev: nslots records (8-byte aligned), in the order
 * of slots_host.  A slot without a surviving track is not solved: iterations 0, converged 0, cw = B[0:nf, 3:6].  Returns -1 with vh_last_error
 * naming the slot and the limit, and nothing queued, for: a slot outside the session or given twice, nf < 2, nf - 1 > 255 (the BA's camera limit),
 * nf > nhist, a slot whose frame counter is not nf - 1, max_iter < 1, a workspace below vh_session_refine_workspace(s, nslots, nf). */
VH_API int vh_session_refine(vh_session* s, const int* slots_host, int nslots, int nf, int max_iter, void* recs_dev, void* workspace,
                             size_t workspace_bytes, void* stream);

/* Bundle adjustment of ANY frame window of a clip, many windows per call (default OFF, like vh_session_refine, which is the window first = 0 of a clip
 * that has just ended.  vh_version stays 111: a consumer tests for the symbols).  Window (slot, first) with the call's common length nf is frames
 * [first, first + nf) of the slot's clip: the reference's fcnNLS_batch(K, P[:, :, first:first+nf], pw, cw) in the coordinates of the window's first camera.
 *   tracks  the ids with isfinite(P[4, id, f]) for EVERY f of the window (NLS.py:190 on the slice), ascending -- selected from the history, not the
 *           slot's current survivors: a track that died after the window belongs to it
 *   z       the float32 history of the window's frames (NLS.py:198-199)
 *   x0      the session's points satisfy proj(K (p3 + B[i, 3:6])) and the BA fixes its camera 0 at the origin with R = I: points p3[id] + B[first, 3:6],
 *           camera positions B[first + c, 3:6] - B[first, 3:6] for c = 1 .. nf-1, rpy 0; float32 values widened to double first, arithmetic in double
 *   K       the slot's own
 * All windows of a call -- of any slots, of clips of any lengths, finished or still running -- are the windows of ONE vh_nls_batch_windows launch
 * sequence (nt = n0, nc = nf - 1).  Clips of more than 256 frames are refined this way: the BA's 255-camera limit is per window.  What windows do NOT
 * do: without anchors (vh_session_set_anchors) each window's scale gauge is held only by the +I damping, and windows are independent solves (no shared
 * points, no global adjustment). */
typedef struct { int slot; int first; } vh_refine_window;   /* frames [first, first + nf) of the slot's clip */
/* One record per window, byte offsets as in vh_refine_record; sized by nf, not by nhist (a long clip has many windows).  Every byte is defined. */
typedef struct {
    size_t bytes;                               /* size of a record (a multiple of 8)                                         */
    size_t slot, first;                         /* int32 each: the window as given                                            */
    size_t nt, iterations, converged;           /* int32 each: tracks solved, LM iterations taken, rms(delta) < 1e-7 reached   */
    size_t cw;                                  /* float64[nf][3]  refined camera positions RELATIVE TO THE WINDOW'S FIRST CAMERA: row 0 zero */
    size_t dr, speed;                           /* float64[nf]     dr_j = |cw_j - cw_(j-1)|, speed_j = dr_j / (B[first+j,12] - B[first+j-1,12]) * 3.6 with
                                                                   the float32 time difference of vidExample.py:142; entry 0 NaN */
    size_t speed_mean, speed_std;               /* float64: mean and (population) std of speed[1:nf] (vidExample.py:177)      */
    size_t f_first, f_last;                     /* float64: rms residual (pixels) of the first and of the last iteration, NaN when none ran */
    size_t trace;                               /* float64[max_iter][2] rms(z - zhat), rms(delta) per iteration, 0 behind them */
    size_t ids;                                 /* with_points only (else 0): int32[n0] rows [0, nt) global track ids, -1 behind them */
    size_t pw;                                  /* with_points only (else 0): float64[n0][3] rows [0, nt) refined points IN THE WINDOW'S COORDINATES
                                                   (subtract B[first, 3:6] for the session's), NaN behind them                 */
    size_t nfix;                                /* int32: anchored points among the window's nt tracks; 0: solved free (the record header's spare word:
                                                   no offset moved).  The last of the offsets: none of the older ones changed place in this struct */
    int n0, nf, max_iter, with_points;
} vh_refine_window_record;
/* size in bytes of a record of a window of nf frames (0 and vh_last_error on bad arguments); layout_host (may be NULL) receives the offsets */
VH_API size_t vh_session_refine_windows_size(const vh_session* s, int nf, int max_iter, int with_points, vh_refine_window_record* layout_host);
/* bytes of device scratch a call of nwin windows of nf frames needs: it grows with nwin (0 and vh_last_error on bad arguments) */
VH_API size_t vh_session_refine_windows_workspace(const vh_session* s, int nwin, int nf);
/* Queues kernels only -- select + pack, the BA launch sequence, unpack -- on `stream`: no allocation, no host wait, legal between two steps; it reads
 * the session and writes nothing of it.  recs_dev: nwin records (8-byte aligned) in the order of wins_host; workspace 256-byte aligned.  A slot may
 * appear in many windows and need not be finished: a window must lie within the frames the slot has had, first >= 0 and first + nf - 1 <= the slot's
 * frame counter.  A window without a track is not solved: iterations 0, converged 0, cw = the tracker's relative positions.  Returns -1 with
 * vh_last_error naming the window and the limit, and nothing queued, for: a slot outside the session, first < 0, a window past the slot's frame
 * counter, the same (slot, first) given twice, nf < 2, nf - 1 > 255 (the BA's camera limit, per window), nf > nhist, max_iter < 1, nwin < 1 (or above
 * the 65535 windows of one launch sequence), misaligned buffers, a workspace below vh_session_refine_windows_workspace(s, nwin, nf). */
VH_API int vh_session_refine_windows(vh_session* s, const vh_refine_window* wins_host, int nwin, int nf, int max_iter, int with_points, void* recs_dev,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* The same windows with tracks that live through PART of a window (default OFF; vh_version stays: a consumer tests for the symbol).  A window takes
 * the ids observed -- isfinite(P[4, id, f]) -- in at least min_obs of its nf frames for which there is a world point to start from; a missing
 * measurement is "no observation" to the solve: zero residual, zero Jacobian rows.  With i the slot's frame counter, a track g of the window is
 *   A  observed in all nf frames (and, in a replenished session, triangulated): the rule of vh_session_refine_windows, unchanged; or
 *   B  observed in >= min_obs frames and its p3[g] is established: row 2 of its history (the pose solve's projection, written only while g is a pose
 *      track) is finite in some frame 0..i, or the MSV frame has run (0 <= msv_frame <= i) and g was alive in it, or g is anchored; or
 *   C  (start_reproj > 0 only) neither, observed in >= min_obs frames: its start is triangulated from its first and its last observed frame of the
 *      window, by the arithmetic of a replenished row's promotion on that one pair (rays by the slot's float32-rays rule, origins
 *      float32(B[0, 0:3] - B[f, 0:3])), and it is admitted iff that point is finite, lies in front of both cameras and reprojects within start_reproj
 *      pixels in both frames; otherwise it counts as rejected.
 * Tracks ascending; starts p3[g], the anchor or the triangulated point, each + B[first, 3:6]; everything else as vh_session_refine_windows.  The rms
 * residual f is taken over all 2 nt nf entries, the zeros of the missing ones included (as the reference forms it).  With min_obs = nf and
 * start_reproj = 0 a window is exactly vh_session_refine_windows's.  What this does NOT do: starts from more than two views, a sparse
 * layout (the solve stays dense over nt x nf: a missing measurement costs what an observed one costs), points shared between windows. */
typedef struct {
    int min_obs;          /* 2 <= min_obs <= nf */
    float start_reproj;   /* pixels, finite, >= 0; 0: no triangulated starts */
} vh_refine_partial_params;
/* One record per window: vh_refine_window_record (every shared field at the offset vh_session_refine_windows_size gives it), then four int32 counts.
 * win.bytes is the size of THIS record (16 more than the window record's).  Every byte is defined. */
typedef struct {
    vh_refine_window_record win;
    size_t nobs;    /* int32: observed measurement pairs among the window's nt x nf */
    size_t npart;   /* int32: tracks among the nt observed in fewer than nf frames    */
    size_t ntri;    /* int32: tracks admitted through C (their starts were triangulated) */
    size_t nrej;    /* int32: C candidates that failed the gate (not among the nt)    */
} vh_refine_partial_record;
VH_API size_t vh_session_refine_windows_partial_size(const vh_session* s, int nf, int max_iter, int with_points, vh_refine_partial_record* layout_host);
/* bytes of device scratch a call of nwin windows needs (vh_session_refine_windows_workspace plus the triangulated starts) */
VH_API size_t vh_session_refine_windows_partial_workspace(const vh_session* s, int nwin, int nf);
/* Promises and refusals of vh_session_refine_windows (kernels only, no allocation, no host wait, the session is only read, one BA launch sequence for
 * all windows, every refusal before anything is queued), and: NULL params_host, min_obs < 2, min_obs > nf, start_reproj < 0 or not finite. */
VH_API int vh_session_refine_windows_partial(vh_session* s, const vh_refine_window* wins_host, int nwin, int nf, int max_iter, int with_points,
                                             const vh_refine_partial_params* params_host, void* recs_dev, void* workspace, size_t workspace_bytes,
                                             void* stream);

/* Huber weights for every refinement of the session (default OFF; vh_version stays: a consumer tests for the symbol).  A session setting, like the
 * anchors and the replenishment's parameters: delta_px pixels, finite and >= 0, 0 = off; nothing is queued.  While it is non-zero,
 * vh_session_refine, vh_session_refine_windows and vh_session_refine_windows_partial solve their windows through vh_nls_batch_windows_robust -- partial
 * tracks, replenished rows, two-view starts and recovered motions are where a wrong measurement is most likely, and one is enough to ruin a speed -- and
 * each of their records grows by a 16-byte tail at the offset that was its `bytes`:
 *     int32 nout_first   measurements with s2 > delta_px^2 at iteration 0
 *     int32 nout_last    ... at the last iteration run (both 0 for a window that was not solved)
 *     float32 delta      the threshold
 *     int32 0
 * and the three *_size queries report the larger `bytes` (no offset of the layouts moves; the four counts of a partial record stay where they are,
 * in front of the tail).  f_first, f_last and the trace stay the UNWEIGHTED rms residual.  With the setting at 0 every record is byte for byte what it
 * is without this call.  Not covered: the per-frame pose solve, other losses (Cauchy, Tukey), an automatic choice of delta_px.  Returns -1 with
 * vh_last_error naming the value, and the setting unchanged, for a negative or non-finite delta_px. */
VH_API int vh_session_set_refine_robust(vh_session* s, double delta_px);
VH_API int vh_session_ptrs(vh_session* s, int slot, vh_session_view* out_host);
/* (vh_version >= 109) the recovery branch of KLTmain (utils/KLT.py:130-133) inside the session; default OFF: a step then queues exactly the launches it
 * always did and a stream whose coarse stage fails reports klt_flags & 1 and goes on with what the blind fine stage kept.
 * on != 0 (params_host: the matcher's parameters, NULL = defaults) creates everything the branch needs -- a private context of the session's (maximum) frame
 * size, the matcher's scratch for up to 16 pairs, a pinned host block and a device block -- so no step allocates.  Every step then, between KLTmain and the bookkeeping:
 *   - reads {klt_flags, n_cur} of every stream back: ONE small device-to-host copy and ONE hipStreamSynchronize PER STEP, whether a stream failed or not.
 *     The host therefore no longer runs ahead of the device; leave the option off for clips that do not need it.
 *   - for the streams with klt_flags & 1 and n_cur > 0: vh_match_affine_batch(im0, frame, p, n_cur) (at most 16 pairs per call, one call per distinct frame size among them), a second
 *     synchronisation to read status and M, and for every stream with a model KLTregional(im0, im, p0, T23.T, lk_fine, fbt = 0.3) into that stream's KLTmain
 *     outputs.  klt_flags gets bit 1 (the recovery ran) and, with a model, bit 2.  Without a model the blind fine stage's result stands.
 * A step of a session with the option on CANNOT be captured into a graph (it waits for the stream): under a stream capture it returns -6 before
 * anything is queued.  on == 0 turns the option off again and keeps what was created. */
VH_API int vh_session_set_fallback(vh_session* s, int on, const vh_match_params* params_host);
/* counts_host int[batch][2]: steps of each stream (since its vh_session_init) in which the recovery ran / in which it found a model */
VH_API int vh_session_recoveries(vh_session* s, int* counts_host);
/* ---- replacing lost tracks with new corners (an extension beyond the reference; vh_version stays 111: a consumer tests for the symbols) --------------
 * Default OFF: a step then queues exactly the launches it always did.  With the option on a session's rows are the frame-0 tracks of a slot's clip
 * (vh_session_init_dev with *n_dev < n0) plus spare TAIL rows, which births fill in ascending order -- ids stays ascending and a history row never holds
 * two tracks.  Per slot the session keeps born int32[n0] (the frame at which row g entered: 0 for frame-0 tracks, -1 for a row never used), tri uint8[n0]
 * (p3[g] is defined: 1 for frame-0 tracks) and n_rows (rows used so far).  m0 = max(msv_frame, 0).
 *   birth      at a stream's own frame f, behind that frame's bookkeeping and fcnMSV1_t, when f > m0, (f - m0) % every == 0 and f + baseline < nhist;
 *              not when n_cur == 0, n_cur >= target, n_rows == n0, or the bounding rectangle of the live tracks (+ border, clipped like
 *              boundingRect) is below 3 x 3 or below block.  goodFeaturesToTrack(frame[roi], max_new, quality, min_distance, mask, block, use_harris,
 *              harris_k) + the ROI origin, mask = 0 where abs(x - rint(px)) < min_distance and abs(y - rint(py)) < min_distance for a live track
 *              (px, py), then cornerSubPix on the whole frame; the first min(count, target - n_cur, n0 - n_rows) corners enter as rows n_rows.. with
 *              vg = 1, vp = 0, tri = 0, born = f and history rows 0, 1, 4 of frame f.  S[f, 2] keeps the count from before the birth.
 *   promotion  at frame born + baseline every live row with tri == 0 born then is triangulated: fcn2vintercept over its baseline + 1 rays (built as
 *              fcnMSV1_t builds them) with origins float32(B[0, 0:3] - B[born + j, 0:3]).  p3[g] = C0, tri = 1, vp = 1 iff C0 is finite, lies in front
 *              of every camera (C0_z + B[born + j, 5] > 0) and reprojects within max_reproj pixels in every frame of the baseline; otherwise the row
 *              stays tracked with vp = 0.
 * No step reads anything back: a step with a birth or promotion due queues a fixed launch sequence over all streams, in which the workgroup of a stream
 * that is idle, not due or in need of nothing leaves at once.  Everything is created by vh_session_set_replenish (the detector's scratch of the
 * session's context for 16 streams at a time, the mask planes, the state), so no step allocates and a step may be captured; the set call itself may not
 * (-6, "call vh_session_set_replenish before capturing").  Refinement on a session with the option on selects, for whole clips too, the tracks alive
 * through the window that are triangulated (tri). */
typedef struct vh_replenish_params {
    int every, baseline;        /* >= 1; baseline <= 63 */
    int target;                 /* live tracks a birth refills to; <= 0: the slot's frame-0 track count */
    int max_new;                /* corner budget of one birth, 1 .. 2048 */
    double min_distance;        /* pixels, finite */
    int border_x, border_y;     /* >= 0 */
    double max_reproj;          /* pixels */
    /* the detector and cornerSubPix settings (the clip's frame-0 settings) */
    double quality, harris_k;
    int block, use_harris;      /* block 1 .. 15 */
    int subpix_win, subpix_iter; /* win 1 .. 7 */
    double subpix_eps;
} vh_replenish_params;
/* params_host NULL: off (what was created is kept).  Otherwise on, with these parameters.  Call it before the slots are initialised: a slot initialised
 * earlier counts as full (no births) until its next vh_session_init / vh_session_init_dev.  -1 for parameters outside the ranges above. */
VH_API int vh_session_set_replenish(vh_session* s, const vh_replenish_params* params_host, void* stream);
/* born_host int32[n0], tri_host uint8[n0] (either may be NULL), counts_host int[4] = {n_rows, rows born, promoted, rejected} since the slot's
 * initialisation.  Waits for the device: for tests and for the results of a finished clip.  -1 when the option was never on. */
VH_API int vh_session_replenish_state(vh_session* s, int slot, int* born_host, uint8_t* tri_host, int* counts_host);
/* Packed track state of every stream for the cross-GPU exchange (RCCL all-gather, DESIGN.md "multi-GPU"):
 * out = device float32 [batch][8 + 3*n0]: {n_cur, n_pose, frame_i, klt_flags, t[3], res | p (n0 x 2) | ids (n0, int32 bits)} */
/* Fused frame ingest for every stream of the session (vidExample.py:91 + KLT.py:111-113 in ONE pass over the BGR frames): bgr_frames_dev / gray_frames_dev =
 * device arrays of ctx->batch pointers (stream b: h_b x w_b x 3 at that slot's size, rows bgr_stride bytes apart -- bgr_stride == 0: dense rows of
 * 3 w_b bytes for every stream, the form for slots of different widths; a non-zero value is one stride for all streams and must cover the widest slot --
 * and w_b x h_b gray destinations owned by the caller with the slot's row stride; a null BGR pointer skips the stream).  Writes the gray frames and, straight into the session, the quarter-scale images the next vh_session_step starts from (that step then
 * skips its own resize); pass the same gray frames to that step. */
VH_API int vh_session_ingest_bgr(vh_session* s, const uint8_t* const* bgr_frames_dev, int bgr_stride, uint8_t* const* gray_frames_dev, void* stream);
VH_API int vh_session_pack_state(vh_session* s, float* out, void* stream);

/* The vh_debug_* switches below are PROCESS-WIDE (atomics): they re-route every context of the process, and exist for the parity tests and A/B
 * experiments only -- every route they select is bit-identical to the default one.  Not a per-stream control; do not flip them in a multi-tenant process
 * for anything but a test.  They are test hooks, not controls: one record in the library holds them all, and every launch reads one snapshot of it.
 *
 *   entry                        values (anything else is stored as given unless noted)                          default   read by
 *   vh_debug_force_generic_lk    0: by window and load, 1..9: the LK kernel of that id where its window allows     0         every LK launch
 *   vh_debug_lk3_tpw             0: by load, 1..8: launch slots per workgroup (n < 0 -> 0, n > 8 acts as 8)         0         LK launches of routes 3 and 5
 *   vh_debug_lk3_one_level       0 / 1 (any non-zero value -> 1)                                                  1         LK launches of routes 3, 5, 6, 7
 *   vh_debug_ransac_path         0: by size, 1: three kernels, 2: fused kernel where the problem fits (as 0)       0         every RANSAC launch
 *   vh_debug_pyr_rows            0: by size, 2 / 4 / 8 rows per thread (anything else -> 0)                        0         every pyrDown launch
 *   vh_debug_klt_order           -1: by load, 0: never, 1: always                                                 -1        vh_klt_main, vh_session_step*
 *   vh_debug_ba_force_valu       0 / 1                                                                            0         every bundle adjustment entry
 *   vh_debug_lk3_residency, vh_debug_lkh_residency: queries, they set nothing
 * (DESIGN.md section 5 lists the environment variables that give four of them another start value, and the experiment switches that have no entry.)
 *
 * test hook: route every LK window through one implementation -- 1: per-sample kernel, 2: strip kernel, 3: LDS-staged
 * kernel, 4: 4-tracks-per-wavefront kernel (15x15 windows; others as in 2), 5 / 6 / 7: LDS-staged 51x51 kernel with 1 / 2 / 4
 * wavefronts per track (other windows: default routing), 8: 8-tracks-per-wavefront kernel k_lk_o (15x15 windows; others as in 2),
 * 9: 16-tracks-per-wavefront kernel k_lk_h, four wavefronts per SIMD with 40 dwords per lane in LDS (15x15 windows; others as in 2), 0: default routing per window and load.  All are bit-identical. */
VH_API void vh_debug_force_generic_lk(int on);

/* test hook (vh_version >= 105): launch slots one workgroup of the one-wavefront LDS-staged LK kernel (k_lk3<.., 1, ..>, routes 3 and 5) solves one after the
 * other -- 0: chosen by load (1 below 49 152 tracks in flight, 2 from there, 4 from 98 304), n > 0: n (clamped to 8).  Bit-identical results. */
VH_API void vh_debug_lk3_tpw(int n);
/* test hook: 1 (the default): an LK job with max_level = 0 takes the single-level form of the LDS-staged kernel k_lk3 (routes 3, 5, 6, 7), 0: it takes
 * the general form, whose level loop then runs once.  Bit-identical results. */
VH_API void vh_debug_lk3_one_level(int on);
/* test hook (vh_version >= 111): residency of the one-wavefront 51x51 LDS-staged kernel (k_lk3<51, 1, 4>, route 5) as the runtime sees it, at the dynamic
 * LDS size its launches pass -- out[0]: workgroups per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor), out[1]: registers per lane, out[2]: scratch bytes
 * per lane, out[3]: LDS bytes per workgroup (hipFuncGetAttributes + the dynamic size).  Launches no kernel.  The kernel has a general and a single-level
 * form (vh_debug_lk3_one_level): of each figure the worse of the two is reported. */
VH_API int vh_debug_lk3_residency(int out[4]);
/* test hook: the same four figures for the 16-tracks-per-wavefront 15x15 kernel (k_lk_h<15>, route 9), whose LDS is static: out[3] is
 * hipFuncGetAttributes' sharedSizeBytes.  Launches no kernel. */
VH_API int vh_debug_lkh_residency(int out[4]);

/* test hook: estimateAffine2D stand-in -- 1: always the three-kernel path (hypotheses spread over the chip), 2: the fused
 * one-workgroup-per-stream kernel whenever the problem fits it (latency path), 0: default routing by batch size.  Bit-identical results. */
VH_API void vh_debug_ransac_path(int mode);

/* test hook: 1 accumulates the reduced camera system of vh_nls_batch on the VALU instead of the f64 matrix cores */
VH_API void vh_debug_ba_force_valu(int on);
/* test hook: pyrDown with 2 / 4 / 8 output rows per thread whatever the launch size (0: chosen by size) */
VH_API void vh_debug_pyr_rows(int rows);
/* test hook: the LK launches of vh_klt_main / vh_session_step walk a stream's tracks in spatial order (a counting sort of the previous positions by
 * 64 x 32-px cell, k_klt_setup) -- 1: always, 0: never, -1: default (from 24000 tracks in flight).  Launch order only: outputs keep the caller's
 * indices and every result is bit-identical. */
VH_API void vh_debug_klt_order(int mode);

/* ---- measurement aids (bench.py): HIP-event timing of the LK launches + Newton-iteration statistics ------------- */
VH_API int vh_profile_begin(vh_ctx* ctx, int max_launches);
/* all outputs host arrays of 3 (KLTmain stage 0: quarter scale, 1: coarse ROI, 2: fine) */
VH_API int vh_profile_end(vh_ctx* ctx, double* ms_sum, int* launches, unsigned long long* iters, unsigned long long* setups);
/* every profiled stage of the same run: 0-2 the LK launches of KLTmain, 3 ROI warp, 4 pyrDown (+ border ring), 5 RANSAC, 6 quarter-scale resize,
 * 7 session frame kernel, 8-12 bundle adjustment (Jacobian, Schur complement, reduction, solve, update).  ms_sum / launches: nstages entries. */
VH_API int vh_profile_detail(vh_ctx* ctx, int all_stages);  /* before vh_profile_begin: 1 = every stage (default), 0 = the LK launches only */
VH_API int vh_profile_end_stages(vh_ctx* ctx, int nstages, double* ms_sum, int* launches);
/* the kernel each of the three LK launches of the last vh_klt_main / vh_session_step took (the launcher's own routing decision, so nobody mirrors its
 * thresholds): routes_host int[3] (ids of vh_debug_force_generic_lk), names_host char[3][32] (may be NULL) */
VH_API int vh_profile_lk_routes(vh_ctx* ctx, int* routes_host, char* names_host);
/* (vh_version >= 105) launch slots per workgroup of the same three launches (see vh_debug_lk3_tpw): tpw_host int[3]; a stateless vh_pyr_lk call reports
 * its route and slot count through entry 0 (like its iteration counters) */
VH_API int vh_profile_lk_tpw(vh_ctx* ctx, int* tpw_host);
/* host copy of every stream's ROI (x0, x1, y0, y1) of the last KLTmain call (images.py:9-19 as KLT.py:121-123 applies it): 4 ints per stream */
VH_API int vh_klt_rois(vh_ctx* ctx, int* roi_host);

#ifdef __cplusplus
}
#endif
#endif /* VELOCITY_HIP_H */
