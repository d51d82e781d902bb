// LocalBA: what the kernels (csrc/lba.hip) and the host plan (csrc/lba_plan.h) share -- the device-side descriptor of a window with
// the records it points to, the task record of the launch lists, and the constants that decide both a kernel's indexing and the
// host's layout.  No HIP runtime calls and no other header of the library: host C++ and kernels.  Internal to the library.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define AOS2_LBA_HD __host__ __device__
#else
#define AOS2_LBA_HD
#endif

namespace aos2 {

struct Cam {
    double fx, fy, cx, cy, bf;
    float bf_f;  // cam_project takes bf as `const float&` (types_six_dof_expmap.cpp:150)
    double delta_mono, delta_stereo;  // Huber deltas (float sqrt -> double, Optimizer.cc:570-571)
};

// Levenberg-Marquardt / SparseOptimizer::optimize state of one window (levenberg.cpp:61-164, sparse_optimizer.cpp:354-419)
struct LmState {
    double lambda, ni, currentChi, iniChi;
    double final_chi2, final_lambda;
    int32_t phase;      // 0: first optimize() running, 1: first finished, 2: second running, 3: finished
    int32_t run;        // the trial kernels execute
    int32_t lin;        // the system is (re)linearised at the current estimates (after an accepted step)
    int32_t initp;      // start of an optimize() call: residuals, system, lambda init pending
    int32_t xmark;      // transition: the outlier pass runs
    int32_t it, qmax, nBad;
    int32_t iters_max[2], iters_done[2], trials[2];
    int32_t polls;      // evaluations of terminate() so far (the host's entry check is the first)
    int32_t stop_poll;  // the poll at which the stop flag was first seen set (0 = never)
    int32_t stop_at_poll;  // test hook: the flag counts as set from this poll on (0 = off)
    int32_t n_active;   // level-0 edges of the second optimisation
    int32_t solver_failed;  // trials whose reduced system hit a zero pivot
    int32_t blocks_done;    // workgroups of the current k_points launch that delivered their partial sums
    int32_t ntr;            // trials recorded below (AOS2_LBA_TRACE=1 prints them)
    // Where the edges' _error of the LAST residual evaluation can be re-formed from (the trials do not store 24 bytes per edge;
    // the two passes that read _error -- the outlier pass and the final check -- re-form it): 0 = nowhere, the stored values
    // stand (no evaluation since they were written); 1 = the current estimates (evaluation at the start of an optimisation, or
    // an accepted trial); 2 = the backup, which after a rejected trial holds the trial's estimates (pop() swaps).
    int32_t err_at;
    int32_t pad_;
    double tr_rho[48], tr_temp[48], tr_cur[48], tr_lambda[48];
};

// The kernel that factorises a window's reduced system: k_ldlt_reg (the matrix in registers, up to 40 free keyframes) or
// k_ldlt_dev (in place in device memory, any size)
enum LdltForm : int { kLdltDev = 0, kLdltReg = 2 };

// What the one-thread-per-landmark kernels need of an edge before they can go to its keyframe, packed and kept in the order of the
// landmarks' edge lists (position a of LbaWin::pt_k: a landmark's records are neighbours): two 16-byte loads in place of the
// index pt_k[a] and, behind it, eight scattered loads of the per-edge arrays.  Copies: the per-edge arrays stay what every other
// kernel reads.  k_prepare builds the records, k_transition keeps the flags in step with e_robust / e_level1.
struct EdgeRec {
    float obs[3], w;   // in_obs, in_w of the edge
    int32_t pose;      // e_pose
    int32_t pl_pos;    // pl_pos
    uint32_t flags;    // kEdgeStereo | kEdgeRobust | kEdgeLevel1
    uint32_t pad_;
};
static_assert(sizeof(EdgeRec) == 32, "an edge record is two 16-byte loads");
constexpr uint32_t kEdgeStereo = 1, kEdgeRobust = 2, kEdgeLevel1 = 4;

// device-side view of one window
struct LbaWin {
    int n_poses, n_points, n_edges, np, nl, n_items;
    int iters1, iters2;              // optimize(5), optimize(10) (Optimizer.cc:661, 708)
    // raw float32 inputs as the reference holds them (staged), converted by k_prepare (Converter.cc:37-47, 83-90)
    const float *in_Tcw, *in_xyz, *in_obs, *in_w;   // (observations and information weights stay float32: the kernels widen them on
                                                     // load -- exact -- instead of reading converted double copies, 16 bytes per edge and use)
    double *pose, *point;            // estimates, contiguous [7 n_poses | 3 n_points]
    double *bk;                      // SparseOptimizer::push backup of the same span
    int est_n;
    const int32_t *e_pose, *e_point;
    const uint8_t *e_stereo;
    uint8_t *e_robust, *e_level1;
    double *err;                     // n_edges x 3, last computed _error
    Cam cam;
    const int32_t *pl_pos;           // edge -> its position in the landmark's free-keyframe edge list (-1: fixed keyframe)
    const int32_t *hpose, *hpoint;   // hidx -> pose / point index
    const int32_t *pt_off, *pt_k;    // edges by point (insertion order)
    const int32_t *ps_off, *ps_k;    // edges by free pose
    const int32_t *pl_off, *pl_ph;   // free-pose edges by point, ascending pose hidx: the pose hidx of each position
    // Schur complement by items: item = (landmark, free-pose edges ka <= kb of it), ranked by (pose, pose) block in
    // upper-triangular order, landmark order inside a block (build_schur_items)
    const int32_t *it_ka, *it_kb, *it_l, *blk_off;
    // k_schur's packed units (build_schur_units): rows of <= 16 items of ONE off-diagonal block, 16 rows per workgroup
    const int32_t *sr_o0, *sr_info, *sr_ij;   // per row: first item; items | row-in-block << 8 | rows-of-block << 16; i1 | i2 << 16
    int n_srows;
    // Linearisation record of a free-keyframe edge, DENSE by its position in the pl list (a landmark's records are
    // neighbours): {a = x / z, b = y / z, iz = 1 / z of the camera-frame point, robustified information w} -- 32 bytes in
    // place of the edge's 144-byte Hpl block J_pose^T (w Omega) J_point, which factors as -E^T C R (EdgeLin below; R: the
    // keyframe's rotation at the linearisation point, Rl) and is applied in that form.  w < 0 marks a stereo edge (|w| is
    // the weight); a masked edge holds zeros: every product it takes part in is +-0.
    double *lrec;
    double *lomr;                    // 3 per free-keyframe edge (position like lrec): omr = -rho' Omega e of the linearisation (k_schur forms b_p from it)
    double *Rl;                      // 9 per free keyframe (hidx): rotation the system was linearised at (k_lin)
    double *Hpp, *Hll, *b, *x, *Hs, *bs;
    double *tmp;                     // scale terms of the poses (6 np)
    double *scal;                    // [3] solve ok
    double *part;                    // per-landmark sums of k_points: chi2 terms [0, nl), scale terms [nl, 2 nl)
    int n_part;                      // workgroups of a k_points launch for this window
    EdgeRec *erec;                   // per position of pt_k: the edge's record (the walk layout's kernels)
    int npad;                        // 6 np rounded up to a multiple of 16
    LdltForm ldlt_form;
    int hs_ld;                       // leading dimension of Hs: always npad now (both forms take the padded matrix)
    LmState *st;
    const int32_t *abort_word;       // mapped host memory: the forwarded pbStopFlag
    float *out_Tcw, *out_xyz;        // Converter::toCvMat / toCvMat(Vector3d) write-back (Optimizer.cc:763-778)
    double *out_chi2;
    uint8_t *out_outlier;
};

// (the kernels' code depends on the members' offsets: a change here is a change of every kernel, to be measured as one)
static_assert(sizeof(LbaWin) == 520 && offsetof(LbaWin, st) == 472, "LbaWin's layout is fixed");

// One workgroup's share of a launch: (window, what).  The host lays the work of ALL windows of a call out as task lists (one per
// kernel family) instead of grids padded to the largest window -- the windows of a batch differ (10-40 keyframes, 2-6 k points),
// and a workgroup that only finds out it has nothing to do still holds a slot for two dependent loads.
struct SchurTask {
    int32_t w;      // window (-1: padding)
    int32_t code;   // k_schur: kind << 28 | argument; k_lin: kind << 28 | block; k_points: block
};

// ---- constants of the kernels that the host's layout depends on (each is explained at its kernel in lba.hip)
// k_points / k_lin<false>: landmarks per 256-thread workgroup, threads per landmark
constexpr int kLmBlock = 32, kLmSlots = 8;
// k_points_walk / k_lin<true>: the keyframe state of a window is staged in LDS up to this size
constexpr int kWalkLdsBytes = 16 * 1024;
AOS2_LBA_HD constexpr int walk_lds_bytes(int n_poses, int np) { return 8 * (7 * n_poses + 15 * np); }
// k_schur's kinds of work unit (SchurTask.code = kind << 28 | argument -- DIAG: i; BIG: block rank; PACK: first row)
constexpr int kSchurDiag = 0, kSchurBig = 1, kSchurPack = 2;
// k_ldlt_dev: the largest padded reduced system whose panel and vectors fit a CU's LDS (npad = 928, 154 free keyframes) ...
constexpr int kLdMaxNpad = 928, kLdMaxNp = kLdMaxNpad / 6;
// ... and k_ldlt_reg: the largest one it holds in registers (16 * kLrMaxNb of ldlt_reg.h, 40 free keyframes; lba.hip asserts the tie)
constexpr int kLrMaxNpad = 240;

}  // namespace aos2
