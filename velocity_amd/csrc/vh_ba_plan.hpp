// Bundle adjustment, everything that is arithmetic on sizes (internal): the tuning constants the host decisions read, the number of partial
// systems, the ONE walk over the workspace (sizing and carving) and the ONE choice of kernels for a solve (BaPlan).  Plain C++17, no HIP include:
// tests/test_ba_plan_cpu.py compiles it with g++ and checks every boundary without a GPU.  vh_ba.hip launches what the plan says.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>

#define BA_THREADS 256
#define BA_EPT 64  // Schur entries owned by one thread per pass
#define BA_MAX_NC 255                       // free cameras: a k_ba_jac workgroup (256 threads) owns whole points, one thread per frame (the reference has no limit)
#define BA_MAX_NC_VALU 128                  // ... of the VALU Schur kernel (test hook / fcnNLS_batch2's trajectory model excepted: nc + 5 unknowns)
#define BA_ZB_MAX 256                        // workgroups of k_ba_zbuild (43+ cameras): one partial right-hand side / set of diagonal blocks each
#define BA_NPAD 128                          // padded width of the reduced system in k_ba_schur_mfma<128>; <256> is twice that
#define BA_SCHUR_THREADS 512                 // k_ba_schur_mfma: 4 consumer + 4 producer wavefronts
#define BA_ZB_PL 4  // points a k_ba_zbuild block works on at a time (threadIdx.y)
#define BA_GJ_MAXQ 124  // the last pivot block must end before the rhs column (127)
#define BA_GJ_WAVES 8   // one 16-row tile row per wavefront, two wavefronts per SIMD: the per-round hand-over (accumulator read-back, LDS publish, waits) is
                        // per-wavefront serial work, so halving each wavefront's share and letting two of them interleave on a SIMD shortens the round
#define BA_CH_NB 32                           // columns of a Cholesky panel
#define BA_CL_RB 32                           // rows below the diagonal block owned by one k_ba_chol_left workgroup
#define BA_CL_KC 128                          // columns of L per LDS stage
#define BA_CL_XP (BA_CL_KC + 2)               // pitch = 4 banks mod 64: the 16 rows x 4 columns of an MFMA operand read hit 64 different banks
#define BA_CL_LDS ((BA_CH_NB + BA_CL_RB) * BA_CL_XP * 8)
#define BA_CB_THREADS 1024                    // k_ba_chol_back
#define BA_UZ_LPP 32  // lanes per point of k_ba_update_z

// partials of the reduced system: one workgroup per ~16 points, at most 256 (512 / 1024 measured 20 % slower at C5: the reduction grows); with many
// cameras fewer, so that the partial systems of one window stay below 256 MB; fewer per window when many windows fill the chip anyway (the partials
// are reduced through HBM): 512 / nwin, at least 16.  parts_env: the VH_BA_PARTS experiment switch (0 = unset), read once per process by vh_api.hip
inline int ba_nparts(int nt, int nc, int nwin, int parts_env)
{
    const int pmax = parts_env > 0 ? parts_env : 256;
    int p = nt / 16;
    p = p < 1 ? 1 : (p > pmax ? pmax : p);
    const long long per = 8ll * (6ll * nc) * (6ll * nc), cap = per > 0 ? (256ll << 20) / per : 256;
    if (cap < p) p = cap < 1 ? 1 : (int)cap;
    if (nwin <= 1) return p;
    const int wcap = 512 / nwin < 16 ? 16 : 512 / nwin;
    return p > wcap ? wcap : p;
}

// ---------------------------------------------------------------------------------------------------------------
// The workspace of one window: the fields in their order, every one rounded up to 256 bytes, 1024 spare bytes behind the last.  Returns the byte
// count; with a base (and a Job: BaJob, or BaFields below) it also points the job's fields into [base, base + count).  Buffers are sized for
// 6 nc >= nc + 5 unknowns whatever the model.
struct BaFields {  // the members of BaJob that live in the workspace
    double *camR, *r, *Jp, *Jc, *tp, *Lc, *Y, *Spart, *Rpart, *Dpart, *Sfull, *acc, *dc, *rslot;
    int* done;
    unsigned* ticket;
};
template <class Job>
inline size_t ba_workspace_walk(int nt, int nc, int nparts, void* base, Job* J)
{
    const size_t nf = nc + 1, nq = 6 * (size_t)nc, m = (size_t)nt * nf;
    const bool big = nq > 252;  // 43+ cameras: per-workgroup partials of k_ba_zbuild (see there)
    const struct { double* Job::*field; size_t n; } extents[] = {
        {&Job::camR, 36 * nf}, {&Job::r, 2 * m}, {&Job::Jp, 6 * m}, {&Job::Jc, 12 * m}, {&Job::tp, 3 * (size_t)nt}, {&Job::Lc, 6 * (size_t)nt},
        {&Job::Y, 3 * nq * nt}, {&Job::Spart, (size_t)nparts * nq * nq},
        {&Job::Rpart, (big ? std::max((size_t)nparts, (size_t)BA_ZB_MAX) : (size_t)nparts) * nq}, {&Job::Dpart, big ? (size_t)BA_ZB_MAX * 36 * nc : 0},
        {&Job::Sfull, nq * (nq + 1) + 4},  // augmented system followed by the 4 accumulators: ONE all-reduce span
        {&Job::dc, nq},
        {&Job::rslot, 32},                 // the flag block: done, ticket and the 16 partial sums (below)
    };
    size_t b = 0;
    for (const auto& e : extents) {
        if (base && J) J->*e.field = reinterpret_cast<double*>(static_cast<char*>(base) + b);
        b += (e.n * sizeof(double) + 255) / 256 * 256;
    }
    if (base && J) {
        double* flags = J->rslot;
        J->acc = J->Sfull + nq * (nq + 1);
        J->done = reinterpret_cast<int*>(flags);
        J->ticket = reinterpret_cast<unsigned*>(flags) + 4;
        J->rslot = flags + 8;  // doubles 8..23 of the 32-double flag block
    }
    return b + 1024;
}
inline size_t ba_workspace_bytes(int nt, int nc, int nparts) { return ba_workspace_walk<BaFields>(nt, nc, nparts, nullptr, nullptr); }

// ---------------------------------------------------------------------------------------------------------------
// Which kernels solve a problem of nt points, nc free cameras, nparts partial systems and nwin windows, and with which grids (vh_ba_run launches
// exactly this; DESIGN.md section 6 has the table).  All ints and size_t, zeroed first: whole solves are recognised by the plan's bytes (graph replay).
enum BaSchur : int { BA_SCHUR_VALU, BA_SCHUR_MFMA128, BA_SCHUR_MFMA256, BA_SCHUR_SYRK };
enum BaSolve : int { BA_SOLVE_GJ_MFMA, BA_SOLVE_GJ_VALU, BA_SOLVE_CHOL_LEFT, BA_SOLVE_CHOL_RIGHT };
enum BaUpdate : int { BA_UPDATE_POINTS, BA_UPDATE_Z_LATENCY, BA_UPDATE_Z4 };
struct BaPlan {
    size_t lds_valu, lds_mfma;  // dynamic LDS of k_ba_points / k_ba_schur_mfma
    int nq;                     // reduced unknowns: 6 nc (model 0) or nc + 5 (model 1)
    int nparts;                 // partial systems written by k_ba_points / k_ba_schur_mfma (as given)
    BaSchur schur;              // k_ba_points | k_ba_schur_mfma<128, 0> | k_ba_schur_mfma<256, 0> + <256, 1> | k_ba_zbuild + k_ba_syrk_mfma
    BaSolve solve;              // k_ba_solve_mfma | k_ba_solve<8, 8, 16> | k_ba_chol_left + k_ba_chol_back | k_ba_chol_panel + k_ba_chol_update + k_ba_chol_back
    BaUpdate update;            // k_ba_update | k_ba_update_z<1024> | k_ba_update_z4
    int zmode;                  // BaJob::zmode: every Schur route but the VALU one
    int npass;                  // launches of k_ba_points (BA_THREADS x BA_EPT entries of S each)
    int nm, npairs;             // SYRK: macro tiles of 128 per dimension, upper-triangle pairs of them
    int nsplit;                 // partial systems k_ba_reduce sums: the K-splits of k_ba_syrk_mfma, else nparts
    int nzb;                    // SYRK: workgroups of k_ba_zbuild (0 otherwise)
    int upd_blocks;             // point blocks of the update kernel (k_ba_update_z adds one for the cameras)
    int reduce_ns;              // k_ba_reduce<16> (1024 threads) or <4> (256 threads)
    int needs_big_lds;          // k_ba_schur_mfma<256, *> and k_ba_chol_left need their dynamic-LDS limit raised (hipFuncSetAttribute) before the launch
};

// dbg: VH_BA_DBG.  Bits 1..32 are k_ba_schur_mfma's ablations (BaJob::dbg) and decide nothing here; 64: VALU Gauss-Jordan where the matrix-core one
// would run; 256: right-looking Cholesky.  Returns 0, or -3 for a problem no kernel takes.
inline int ba_plan(int nt, int nc, int nparts, int nwin, int model, int force_valu_hook, int dbg, BaPlan* out)
{
    BaPlan& p = *out;
    memset(&p, 0, sizeof(p));  // padding included
    if (nc > BA_MAX_NC) return -3;
    if (nwin < 1) nwin = 1;
    const int nq = model == 1 ? nc + 5 : 6 * nc;
    const long long nent = (long long)nq * nq;
    p.nq = nq;
    p.nparts = nparts;
    p.npass = (int)((nent + (long long)BA_THREADS * BA_EPT - 1) / ((long long)BA_THREADS * BA_EPT));
    p.lds_valu = sizeof(double) * (size_t)(6 * nq + 12 * (nc + 1) + 16);
    const int npad = nq <= BA_NPAD ? BA_NPAD : 2 * BA_NPAD;  // matrix-core Schur kernel: 128-wide (<= 21 cameras) or 256-wide in two passes (<= 42)
    p.lds_mfma = sizeof(double) * (size_t)(24 * npad + 2 * 4 * (20 * nc + 10) + 4 * npad);
    // the VALU test hook (vh_debug_ba_force_valu) is honoured where the VALU Schur kernel exists (<= BA_MAX_NC_VALU cameras) and ignored above: a flag
    // left set by another test or thread must not turn a valid call into a failure
    const bool force_valu = force_valu_hook && nq <= 6 * BA_MAX_NC_VALU;
    const bool use_mfma = nq <= 252 && !force_valu && model == 0;  // model 1 has nc + 5 unknowns: nothing for the matrix cores to do
    // 43..255 cameras: Z materialised + K-split SYRK on the matrix cores (k_ba_zbuild / k_ba_syrk_mfma).  nm macro tiles of 128 per dimension; the
    // first `nsplit` partial systems are used: about one resident round of workgroups (2 per CU), every split at least one LDS stage of points
    const bool use_syrk = nq > 252 && !force_valu && model == 0;
    if (!use_syrk && !use_mfma && nq > 6 * BA_MAX_NC_VALU) return -3;  // the VALU Schur kernel keeps 6 nc / 256 right-hand-side entries per thread and 3 x 6 nc doubles of LDS
    p.schur = use_syrk ? BA_SCHUR_SYRK : !use_mfma ? BA_SCHUR_VALU : npad == BA_NPAD ? BA_SCHUR_MFMA128 : BA_SCHUR_MFMA256;
    p.zmode = (use_mfma || use_syrk) ? 1 : 0;
    p.nm = (nq + 127) / 128;
    p.npairs = p.nm * (p.nm + 1) / 2;
    p.nsplit = use_syrk ? std::max(1, std::min(std::min(nparts, std::max(1, 512 / (p.npairs * (int)std::min(nwin, 512)))), (nt + 10) / 11)) : nparts;
    p.nzb = use_syrk ? std::max(1, std::min(BA_ZB_MAX, (nt + 2 * BA_ZB_PL - 1) / (2 * BA_ZB_PL))) : 0;  // workgroups of k_ba_zbuild: at least two rounds of points each
    p.reduce_ns = p.nsplit >= 128 ? 16 : 4;
    p.needs_big_lds = ((use_mfma && p.lds_mfma > 64 * 1024) || nq > BA_GJ_MAXQ) ? 1 : 0;
    // up to 124 unknowns (20 cameras): block Gauss-Jordan on the matrix cores; 125..127 (21 cameras: 126): the register-resident VALU Gauss-Jordan;
    // 128+ unknowns (22+ cameras): left-looking blocked Cholesky, ONE launch per 32-column panel, + the back-substitution (right-looking: the kernels
    // of round 4, two launches per panel, kept as the second implementation for the tests)
    p.solve = (nq <= BA_GJ_MAXQ && !(dbg & 64)) ? BA_SOLVE_GJ_MFMA : nq + 1 <= 128 ? BA_SOLVE_GJ_VALU : (dbg & 256) ? BA_SOLVE_CHOL_RIGHT : BA_SOLVE_CHOL_LEFT;
    // one wavefront per point, grid-strided: every block ends with an atomic on one address, so keep the block count low
    const int upd_cap = nwin > 1 ? std::max(16, 1024 / nwin) : 256;
    const bool uz_latency = (long long)nwin * nt <= 20000;  // few points in flight: the 32-lanes-per-point kernel (one memory round trip); else every lane busy
    const int uz_ppb = uz_latency ? 1024 / BA_UZ_LPP : BA_THREADS / 4;  // points per block and pass of k_ba_update_z / k_ba_update_z4
    p.update = !p.zmode ? BA_UPDATE_POINTS : uz_latency ? BA_UPDATE_Z_LATENCY : BA_UPDATE_Z4;
    p.upd_blocks = std::min(p.zmode ? (nt + uz_ppb - 1) / uz_ppb : (nt + BA_THREADS / 64 - 1) / (BA_THREADS / 64), upd_cap);
    return 0;
}
