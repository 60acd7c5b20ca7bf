// Bundle-adjustment job descriptors (internal).
#pragma once
#include "vh_common.hpp"

struct BaJob {  // passed by value to every BA kernel
    double K[9];
    const double* z;  // [2 * nt * (nc+1)] measurements, [all u | all v], camera-major / track-minor (NLS.py:198-199)
    double* x;        // model 0: [3 nt + 6 nc] points | camera positions | camera rpy (NLS.py:203)
                      // model 1: [3 nt + 3 + 2 + nc] points | joint rpy | el, az | camera ranges (NLS.py:274)
    double* camR;     // model 0: [(nc+1)][4][9] R(rpy) and its three forward-difference neighbours
                      // model 1: [4][9] joint R and neighbours, then [(nc+1)][4][3] camera offsets: base, +d el, +d az, +d range
    double* r;        // [m][2] residuals z - zhat
    double* Jp;       // [m][2][3] d(u,v)/d(point)
    double* Jc;       // [m][2][6] d(u,v)/d(camera pos, rpy)
    double* tp;       // [nt][3]  (U+I)^-1 gp
    double* Lc;       // [nt][6]  lower-triangular Cholesky factor of (U+I)^-1 = L L^T (l00 l10 l11 l20 l21 l22): matrix-core path only
    double* Y;        // [nt][6 nc][3]  (U+I)^-1 W   (matrix-core path: Z = L^T W instead, zmode = 1)
    double* Spart;    // [nparts][(6 nc)^2]
    double* Rpart;    // [nparts][6 nc]  (43+ cameras: [max(nparts, BA_ZB_MAX)][6 nc], one partial per k_ba_zbuild workgroup)
    double* Dpart;    // 43+ cameras only: [BA_ZB_MAX][36 nc] partial diagonal blocks V_c of the k_ba_zbuild workgroups
    double* Sfull;    // [6 nc][6 nc + 1]
    double* dc;       // [6 nc]
    double* acc;      // [2] sum r^2, sum delta^2
    double* rslot;    // [16] partial sums of r^2 (k_ba_jac spreads its atomics, k_ba_reduce folds them into acc[0])
    double* trace;    // [max_iter][2] rms(z - zhat), rms(delta) (what NLS.py:238 prints)
    int* info;        // [2] iterations, converged
    int* done;
    unsigned* ticket;
    double nx_total, nz_total;  // normalisation of rms(delta) / rms(residual): whole-problem sizes (sharded runs)
    int nt, nc;
    int nq;     // reduced unknowns: 6 nc (model 0) or nc + 5 (model 1)
    int model;  // 0: fcnNLS_batch (free cameras, NLS.py:186-250); 1: fcnNLS_batch2 (joint rotation + straight-line trajectory, NLS.py:253-328)
    int add_identity, count_cams, defer_finalize;
    int dbg;    // experiment switches (VH_BA_DBG, tools/ba_dbg.sh).  Read by k_ba_schur_mfma: 1 skip MFMA, 2 skip the diagonal blocks (VALU), 4 skip global fetch, 8 skip barrier,
                // 16 skip parking the raw records in LDS, 32 skip forming Z.  Read by ba_plan (vh_ba_plan.hpp), ignored on the device: 64 VALU Gauss-Jordan solve, 256 right-looking Cholesky (two launches per panel)
    int zmode;  // 1: Y holds Z = L^T W and Spart holds only the upper-triangle 16x16 tiles (k_ba_schur_mfma); 0: Y = (U+I)^-1 W, full Spart
    // batched independent windows (vh_nls_batch_multi): blockIdx.y selects the window; every pointer above is window 0's
    int nwin;
    size_t ws_stride;                // bytes between the workspaces of consecutive windows
    size_t z_stride, x_stride;       // doubles between consecutive windows' z / x
    size_t trace_stride;             // doubles
    size_t info_stride;              // ints
    // windows of different track counts and cameras (vh_nls_batch_windows): every window is laid out for nt tracks, rows >= nt_win[w] are padding
    // (NaN measurements: exact zeros everywhere, see k_ba_jac).  Both tables are read on the device; null = nt tracks / K for every window
    const int* nt_win;               // [nwin] true track counts: the two rms divisors of the iteration record, and the start flag of an empty window
    const double* K_win;             // [nwin][9] intrinsics of each window
    // anchored (fixed) points (vh_nls_batch_windows_fixed): a flagged row has exact zeros for its three Jacobian columns (k_ba_jac), so U_i + I = I,
    // tp_i = 0, W_i = 0: it takes no step and subtracts nothing from the reduced system, while its measurements still add Jc^T Jc and Jc^T r to its
    // cameras.  It still counts as rows of x (nx, nz are unchanged).  Null = no anchors
    const uint8_t* fixed;            // [nwin][nt] non-zero = anchored
    // Huber weights (vh_nls_batch_windows_robust): a measurement pair whose reprojection error at the start of the iteration has s2 = ru^2 + rv^2 > delta^2
    // gets w = delta / sqrt(s2), and k_ba_jac<*, true> scales its residual pair and its 18 Jacobian entries by sqrt(w) -- after the NaN and anchor rules, before
    // anything else reads them, so J^T W J and J^T W r follow on every route of the plan (IRLS: the weights are those of the current state).  The rms residual of
    // the trace stays the unweighted one.  The block counts of down-weighted measurements meet in the int at double 24 of the window's flag block
    // (ba_outlier_counter); the kernel that writes the iteration record moves the sum to nout[it] and clears it.  delta = 0: off, the plain kernels run
    double delta;                    // pixels, >= 0
    int* nout;                       // [nwin][nout_stride] down-weighted measurements at the start of every iteration (may be null)
    size_t nout_stride;              // ints
};

struct BaProblem {  // every field defaults to zero / null: an entry point sets what it uses (ba_problem in vh_api.hip fills the single-window defaults)
    double K[9] = {};
    const double* z = nullptr;
    double* x = nullptr;
    double* trace = nullptr;
    int* info = nullptr;
    void* workspace = nullptr;
    int nt = 0, nc = 0, max_iter = 0, nparts = 0;
    int phase = 0, it = 0;   // phase -1: whole solve; 0..3: the pieces of one sharded iteration (see vh_ba_run)
    int add_identity = 0, count_cams = 0, defer_finalize = 0;
    double nx_total = 0, nz_total = 0;
    int model = 0;       // see BaJob::model
    int force_valu = 0;  // test hook: 1 = accumulate the reduced camera system on the VALU instead of the matrix cores
    int nwin = 0;        // independent windows solved by the same launches (>= 1); z, x, trace, info and workspace are arrays of nwin
    size_t ws_stride = 0, z_stride = 0, x_stride = 0, trace_stride = 0, info_stride = 0;  // see BaJob (ignored when nwin == 1)
    const int* nt_win = nullptr;  // see BaJob (device, may be null)
    const double* K_win = nullptr;
    const uint8_t* fixed = nullptr;
    double delta = 0;        // see BaJob (0 = plain least squares)
    int* nout = nullptr;
    size_t nout_stride = 0;
    struct vh_ctx* ctx = nullptr;  // may be null: per-kernel HIP-event timing when its profiling is on (vh_profile_begin)
    void** graph_cache = nullptr;  // may be null: where the owner (vh_ctx) keeps the replayable launch sequences of whole solves (vh_ba_graph_cache_free)
};
void vh_ba_graph_cache_free(void* cache);

// A robust solve (delta > 0) leaves three ints in each window's workspace, at int BA_OUTLIER_WORD of its flag block: the running count of down-weighted
// measurements (0 between iterations), the count at iteration 0 and the count at the last iteration run (0, 0 when none ran: k_ba_init clears the block).
// vh_ba_outlier_words: their address in window 0's workspace (later windows: the workspace stride further)
#define BA_OUTLIER_WORD 48
const int* vh_ba_outlier_words(int nt, int nc, int nparts, void* workspace);
// ... of the windows of a vh_ba_windows call (vh_api.hip: it knows the partial systems such a call uses)
const int* vh_ba_windows_outlier_words(int nt, int nc, int nwin, void* workspace);

size_t vh_ba_workspace_bytes(int nt, int nc, int nparts);
int vh_ba_run(const BaProblem& P, hipStream_t s);
void vh_ba_exchange_span(const BaProblem& P, size_t* offset_bytes, size_t* n_doubles);
// vh_nls_batch_windows_fixed (include/velocity_hip.h) with the caller's own distances between the windows' trace (doubles) and info (ints) records (vh_api.hip)
// delta_px > 0: Huber weights, and nout (device, may be null) receives the per-iteration counts, nout_stride ints between windows
int vh_ba_windows(struct vh_ctx* c, const double* K_host, const double* z, double* x, int nt, int nc, int nwin, const int* nt_win_dev,
                  const double* K_win_dev, const uint8_t* fixed_dev, int max_iter, double* trace, size_t trace_stride, int* info, size_t info_stride,
                  void* workspace, size_t workspace_bytes_per_window, void* stream, double delta_px = 0.0, int* nout = nullptr, size_t nout_stride = 0);
