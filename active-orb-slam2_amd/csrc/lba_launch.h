// LocalBA: the launch helpers of csrc/lba.hip, the only unit that holds (and launches) the kernels.  csrc/lba_solve.hip and
// csrc/lba_taps.hip enqueue a window group's program through these.  Internal to the library.
#pragma once
#include "lba_math.h"
#include "lba_plan.h"

namespace aos2 {

// the streams a launch sequence is enqueued on: its own, and the one the second reduced-system kernel runs on, forked and joined
struct StreamSet {
    hipStream_t q, q2;
    hipEvent_t fork, join;
};

// What a launch sequence runs on: the descriptor array its task lists index (`wins`), the first descriptor and the number of
// windows of the kernels that take one workgroup row per window (`blk`, nw), the lists, the largest dimensions, the streams
struct Prog : StreamSet {
    const LbaWin *wins, *blk;
    int nw;
    const SchurTask *schur, *pts, *lin;
    size_t n_schur, n_pts, n_lin;
    GroupDims D;
};
inline Prog make_prog(const LbaWin *wins, const LbaWin *blk, int nw, const TaskLists &T, const DevTasks &d, const GroupDims &D, const StreamSet &Q)
{
    return Prog{Q, wins, blk, nw, d.schur, d.pts, d.lin, T.schur.size(), T.pts.size(), T.lin.size(), D};
}

// ---- enqueueing.  What the launches of a call share besides their Prog:
struct LaunchCtx {
    aos2_lba *s;
    bool walk;              // the landmark kernels' layout (LmLayout::walk)
    bool stagger_pending;   // two groups: the second group's stream has not been released yet (enqueue_trial)
};

// The reduced-system kernels take their LDS dynamically: each kernel's cap is declared once per device binding ...
int ldlt_declare_lds();
// ... and every launch goes through enqueue_ldlt, which sizes it.  Both forms over the descriptors blk[0 .. nw): mx_npad_reg /
// mx_npad_dev: the largest padded size among the windows of that form, 0 = none (the kernel is not launched)
void enqueue_ldlt(const LbaWin *blk, int nw, int mx_npad_reg, int mx_npad_dev, hipStream_t q_reg, hipStream_t q_dev);

void enqueue_prepare(const LaunchCtx &C, const Prog &P);
void enqueue_points(const LaunchCtx &C, const Prog &P, int solve);
void enqueue_lin(const LaunchCtx &C, const Prog &P, int init);
void enqueue_init(const LaunchCtx &C, const Prog &P);
void enqueue_schur(const Prog &P);
void enqueue_reduced(LaunchCtx &C, const Prog &P, bool first_group);
void enqueue_trial(LaunchCtx &C, const Prog &P, bool first_group);
void enqueue_transition(const Prog &P);
void enqueue_final(const Prog &P);
// the whole procedure of a group's windows: optimisation k gets slots[k] trials and runs if iters[k] > 0
void enqueue_program(LaunchCtx &C, const Prog &P, bool first_group, const int (&iters)[2], const int (&slots)[2]);

}  // namespace aos2
