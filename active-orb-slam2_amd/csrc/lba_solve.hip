// Optimizer::LocalBundleAdjustment on the device, the host side of a call: the handle, the steps of aos2_lba_solve_batch and the
// C API.  The plan of a call (index structures, arena layout, task lists) is csrc/lba_plan.h; the kernels and their launch helpers
// are csrc/lba.hip (csrc/lba_launch.h).  No kernel here.
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <memory>

#include "lba_solve.h"

namespace aos2 {

int lba_handle_init(aos2_lba *s)
{
    int st = bind_device(s->device);
    if (st) return st;
    if (s->dev_ready) return AOS2_OK;
    // The optimiser's kernels are few workgroups on a latency-bound chain; the tracking kernels that share the device in a
    // running system (extraction, searches) are wide and throughput-bound.  On a high-priority stream the optimiser's
    // workgroups are dispatched ahead of the waiting ones of those kernels.
    if ((st = stream_create(&s->stream, true))) return st;
    for (auto &e : s->ev) AOS2_HIP_CHECK(hipEventCreate(&e));
    {
        if ((st = stream_create(&s->stream2, true))) return st;
        AOS2_HIP_CHECK(hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming));
        AOS2_HIP_CHECK(hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming));
    }
    if ((st = ldlt_declare_lds())) return st;
    s->dev_ready = true;
    return AOS2_OK;
}

// The second window group's streams and events, created when a call first runs two groups: a handle that never does keeps two
// streams.  (The runtime maps the streams of a priority class onto GPU_MAX_HW_QUEUES = 4 hardware queues by creation order and
// serialises those that share one: two handles solving side by side, each with four streams, had their main streams on the same
// queue in some processes and not in others -- 50 k against 60 k frames/s of the composite from run to run.)
static int lba_group_streams(aos2_lba *s)
{
    if (s->stream_b) return AOS2_OK;
    if (int st_ = stream_create(&s->stream_b, true)) return st_;
    if (int st_ = stream_create(&s->stream2_b, true)) return st_;
    for (hipEvent_t *ev : {&s->ev_fork_b, &s->ev_join_b, &s->ev_up, &s->ev_stag, &s->ev_done_b}) AOS2_HIP_CHECK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    return AOS2_OK;
}

StreamSet group_streams(const aos2_lba *s, int g)
{
    return g == 0 ? StreamSet{s->stream, s->stream2, s->ev_fork, s->ev_join} : StreamSet{s->stream_b, s->stream2_b, s->ev_fork_b, s->ev_join_b};
}

static bool stop_requested(const aos2_lba_problem_t *p) { return p->stop_flag && *p->stop_flag != 0; }

// worker threads of a batch's per-window host work (structure build, staging): the handle's setting, else
// AOS2_LBA_HOST_THREADS, else the host's cores shared among the ranks of the node (LOCAL_WORLD_SIZE / WORLD_SIZE as the
// launcher exports them: 8 ranks x 2 handles x 32 threads would be 512 threads on 256 cores), at most 32, at most one per window
static int lba_host_threads(const aos2_lba *s, int nw)
{
    int n = s->host_threads;
    if (n <= 0)
        if (const char *e = getenv("AOS2_LBA_HOST_THREADS")) n = atoi(e);
    if (n <= 0) {
        int ranks = 1;
        const char *e = getenv("LOCAL_WORLD_SIZE");
        if (!e) e = getenv("WORLD_SIZE");
        if (e && atoi(e) > 1) ranks = atoi(e);
        n = std::min(32, std::max(1, (int)std::thread::hardware_concurrency() / ranks));
    }
    return std::max(1, std::min(n, nw));
}

// ROCTx ranges around the host-side phases of a solve (AOS2_ROCTX=1; rocprofv3 --marker-trace shows them next to the
// kernels).  The library is looked up at run time: no link dependency.  g2o's statistics buckets
// (Thirdparty/g2o/g2o/core/batch_stats.h, filled in block_solver.hpp:441-453 and sparse_optimizer.cpp:376-414) map to
// the kernels of the device program: timeResiduals -> k_points, timeLinearize + timeQuadraticForm -> k_lin,
// timeSchurComplement -> k_schur, timeLinearSolver -> k_ldlt_reg / k_ldlt_dev, timeUpdate -> the pose
// update inside the LDL^T kernel and the landmark update inside k_points.
struct RoctxRange {
    typedef int (*push_t)(const char *);
    typedef int (*pop_t)();
    static void resolve(push_t &push, pop_t &pop)
    {
        static push_t s_push = nullptr;
        static pop_t s_pop = nullptr;
        static bool tried = false;
        if (!tried) {
            tried = true;
            const char *v = getenv("AOS2_ROCTX");
            if (v && atoi(v) != 0) {
                void *h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
                if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
                if (h) {
                    s_push = (push_t)dlsym(h, "roctxRangePushA");
                    s_pop = (pop_t)dlsym(h, "roctxRangePop");
                }
            }
        }
        push = s_push;
        pop = s_pop;
    }
    pop_t pop_ = nullptr;
    explicit RoctxRange(const char *name)
    {
        push_t push;
        resolve(push, pop_);
        if (push && pop_) push(name); else pop_ = nullptr;
    }
    ~RoctxRange()
    {
        if (pop_) pop_();
    }
};

// ---- the steps of aos2_lba_solve_batch

// Validates the call and settles the windows whose stop flag is set on entry (Optimizer.cc:656-658: return before optimising when
// the flag is already set; nothing is written back); `act` lists the others
static int settle_entry(const aos2_lba *s, const aos2_lba_problem_t *problems, aos2_lba_result_t *results, int n_problems, std::vector<int> &act, bool &want_chi2)
{
    want_chi2 = false;
    for (int w = 0; w < n_problems; ++w) {
        const aos2_lba_problem_t *p = problems + w;
        aos2_lba_result_t *r = results + w;
        if (p->n_poses <= 0 || p->n_points <= 0 || p->n_edges <= 0 || !p->pose_Tcw || !p->pose_fixed || !p->pose_id ||
            !p->point_xyz || !p->point_id || !p->edge_pose || !p->edge_point || !p->edge_obs || !p->edge_stereo ||
            !p->edge_inv_sigma2 || !r->pose_Tcw || !r->point_xyz) {
            set_error("bad LocalBA problem %d", w);
            return AOS2_ERR_ARG;
        }
        want_chi2 |= r->edge_chi2 != nullptr;   // (the edges' vertex indices are checked with the structure build, a thread per window)
    }
    for (int w = 0; w < n_problems; ++w) {
        const aos2_lba_problem_t *p = problems + w;
        aos2_lba_result_t *r = results + w;
        r->iters_done_first = r->iters_done_second = 0;
        r->trials_first = r->trials_second = 0;
        r->final_chi2 = r->final_lambda = 0;
        r->ms_device = 0;
        r->polls = 1;
        r->stop_poll = 0;
        r->status = AOS2_OK;
        if (stop_requested(p) || s->debug_stop_at_poll == 1) {
            memcpy(r->pose_Tcw, p->pose_Tcw, sizeof(float) * 16 * p->n_poses);
            memcpy(r->point_xyz, p->point_xyz, sizeof(float) * 3 * p->n_points);
            if (r->edge_outlier) memset(r->edge_outlier, 0, p->n_edges);
            r->status = AOS2_ERR_STOPPED;
            r->stop_poll = 1;
        } else
            act.push_back(w);
    }
    return AOS2_OK;
}

// Window groups.  A trial is three wide launches (Schur, back-substitution, linearisation: every window's landmarks) and one
// narrow one (the reduced systems: ONE workgroup per window, the longest launch of the mixed batch, during which most of the device
// idles).  A batch of many windows runs as TWO groups with the same program each, on their own streams, the second started
// behind the first group's first Schur launch: one group's reduced systems are factorised while the other group's landmark
// kernels fill the device.  Windows are dealt to the groups by size (edges), largest first, so both get the same mix; the
// windows of a group are neighbours in the descriptor array.  (aos2_lba_set_window_groups overrides.)
// Returns the number of groups; group g is act[goff[g] .. goff[g + 1]), `act` reordered accordingly.
static int deal_groups(const aos2_lba *s, const aos2_lba_problem_t *problems, std::vector<int> &act, int (&goff)[3])
{
    const int nw = (int)act.size();
    int G = s->window_groups ? s->window_groups : nw >= 16 ? 2 : 1;
    if (G > nw) G = 1;
    goff[0] = 0;
    goff[1] = goff[2] = nw;
    if (G == 2) {
        std::vector<int> order(act);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return problems[a].n_edges > problems[b].n_edges; });
        std::vector<int> g0, g1;
        for (size_t k = 0; k < order.size(); ++k) (((k & 3) == 0 || (k & 3) == 3) ? g0 : g1).push_back(order[k]);   // a b b a | a b b a ...
        act = g0;
        act.insert(act.end(), g1.begin(), g1.end());
        goff[1] = (int)g0.size();
    }
    return G;
}

// Staging, a pool thread per window.  A window's staged region goes to the device as soon as it is assembled: its upload overlaps
// the staging of the other windows (one copy of everything after the staging cost 0.4 ms more per 32-window call)
static int stage_and_upload(aos2_lba *s, WindowPool &pool, const aos2_lba_problem_t *problems, const std::vector<int> &act, const std::vector<Pass> &passes,
                            const ArenaPlan &A)
{
    const int nw = (int)act.size();
    uint8_t *base = s->arena.p, *hin = s->h_in.p;
    std::vector<uint8_t> up_fail(nw, 0);
    pool.run(nw, [&](int i) {
        stage_window(hin, A.L[i], problems[act[i]], passes[i]);
        const size_t r0 = A.L[i].in_Tcw, r1 = i + 1 < nw ? A.L[i + 1].in_Tcw : A.o_tasks;
        if (hipSetDevice(s->device) != hipSuccess || hipMemcpyAsync(base + r0, hin + r0, r1 - r0, hipMemcpyHostToDevice, s->stream) != hipSuccess)
            up_fail[i] = 1;
    });
    for (int i = 0; i < nw; ++i)
        if (up_fail[i]) {
            set_error("LocalBA: upload of window %d failed", act[i]);
            return AOS2_ERR_HIP;
        }
    return AOS2_OK;
}

int build_and_upload(aos2_lba *s, const aos2_lba_problem_t *problems, const std::vector<int> &act, const int (&goff)[3], int G, const LmLayout &lay,
                     bool want_chi2, Uploaded &U)
{
    const int nw = (int)act.size();
    int st;
    // ---- per-window structure (host; windows in parallel when there are several), the groups' task lists
    auto rg = std::make_unique<RoctxRange>("LocalBA::buildStructure (index mapping, edge lists, Schur items)");
    if (!s->lba_cache) s->lba_cache = new LbaCache();
    std::vector<Pass> &passes = static_cast<LbaCache *>(s->lba_cache)->passes;
    U.passes = &passes;
    if ((int)passes.size() < nw) passes.resize(nw);
    WindowPool &pool = static_cast<LbaCache *>(s->lba_cache)->pool;
    if (nw > 1) pool.start(lba_host_threads(s, nw));
    if ((st = build_structures(pool, problems, act.data(), nw, passes))) return st;
    rg = std::make_unique<RoctxRange>("LocalBA::stage + upload");
    TaskLists(&TL)[2] = U.TL;
    size_t n_all_tasks = 0;
    for (int g = 0; g < G; ++g) {
        std::vector<int> ids(goff[g + 1] - goff[g]);
        std::iota(ids.begin(), ids.end(), goff[g]);
        build_tasks(passes, ids, false, lay, TL[g]);   // (the groups' kernels index the whole descriptor array)
        n_all_tasks += TL[g].size();
    }

    // ---- arena: layout, allocation, staging + upload (parallel), descriptors
    ArenaPlan &A = U.A;
    plan_arena(problems, act, passes, lay, n_all_tasks, want_chi2, A);
    if ((st = s->arena.alloc(A.bytes + 256))) return st;
    if ((st = s->h_in.alloc(A.o_cont + A.cont_bytes + 256))) return st;
    if ((st = s->h_stage.alloc(A.res_bytes + 256))) return st;
    if ((st = s->h_abort.alloc((size_t)nw + 1))) return st;
    uint8_t *base = s->arena.p, *hin = s->h_in.p;
    int32_t *d_abort = nullptr;
    AOS2_HIP_CHECK(hipHostGetDevicePointer((void **)&d_abort, s->h_abort.p, 0));
    bool &any_flag = U.any_flag;
    any_flag = false;
    for (int i = 0; i < nw; ++i) {
        s->h_abort.p[i] = 0;
        any_flag |= problems[act[i]].stop_flag != nullptr;
    }
    if ((st = stage_and_upload(s, pool, problems, act, passes, A))) return st;
    LbaWin *hw = U.hw = reinterpret_cast<LbaWin *>(hin + A.o_wins);
    GroupDims(&gd)[2] = U.gd;
    int &max_i1 = U.max_i1, &max_i2 = U.max_i2;
    for (int i = 0; i < nw; ++i) {
        const aos2_lba_problem_t &p = problems[act[i]];
        describe_window(hw[i], base, p, passes[i], A.L[i], d_abort + i, want_chi2);
        gd[i >= goff[1] ? 1 : 0].add(p, passes[i], A.L[i]);
        max_i1 = std::max(max_i1, p.iters_first);
        max_i2 = std::max(max_i2, p.iters_second);
    }
    hipStream_t q = s->stream;
    // the task lists of the groups, one after the other: [schur | points | lin] per group
    DevTasks(&dt)[2] = U.dt;
    {
        size_t o = A.o_tasks;
        for (int g = 0; g < G; ++g) dt[g] = put_tasks(TL[g], hin, base, o);
    }
    AOS2_HIP_CHECK(hipMemcpyAsync(base + A.o_tasks, hin + A.o_tasks, A.staged_bytes - A.o_tasks, hipMemcpyHostToDevice, q));   // the task lists, the descriptors
    AOS2_HIP_CHECK(hipEventRecord(s->ev[0], q));
    if (G == 2) {   // the second group's stream starts behind the upload
        AOS2_HIP_CHECK(hipEventRecord(s->ev_up, q));
        AOS2_HIP_CHECK(hipStreamWaitEvent(s->stream_b, s->ev_up, 0));
    }
    return AOS2_OK;
}

// what the steps after the upload work on
struct Batch {
    const aos2_lba_problem_t *problems;
    const std::vector<int> &act;        // the windows that run, in descriptor order
    const std::vector<Pass> &passes;    // their structures ...
    const ArenaPlan &A;                 // ... and regions
    LmLayout lay;
    const LbaWin *hw;                   // the host's copy of their descriptors
    bool any_flag;                      // a window has a stop flag: forwarded to the abort words while the device runs
    const LmState *state_of(const aos2_lba *s, int i) const { return reinterpret_cast<const LmState *>(s->h_stage.p + (A.L[i].st - A.o_res)); }
};

// Ends the programs with the final check; the results (and states) come back as one copy; the host forwards pbStopFlag into the
// mapped abort words meanwhile
static int finish(aos2_lba *s, const Prog *progs, int n_progs, const Batch &Bt)
{
    hipStream_t q = s->stream;
    for (int g = 0; g < n_progs; ++g) enqueue_final(progs[g]);
    if (n_progs == 2) {
        AOS2_HIP_CHECK(hipEventRecord(s->ev_done_b, s->stream_b));
        AOS2_HIP_CHECK(hipStreamWaitEvent(q, s->ev_done_b, 0));
    }
    AOS2_HIP_CHECK(hipEventRecord(s->ev[1], q));
    AOS2_HIP_CHECK(hipMemcpyAsync(s->h_stage.p, s->arena.p + Bt.A.o_res, Bt.A.res_bytes, hipMemcpyDeviceToHost, q));
    if (Bt.any_flag) {
        AOS2_HIP_CHECK(hipEventRecord(s->ev[2], q));
        while (hipEventQuery(s->ev[2]) == hipErrorNotReady)
            for (size_t i = 0; i < Bt.act.size(); ++i)
                if (stop_requested(Bt.problems + Bt.act[i])) __atomic_store_n(&s->h_abort.p[i], 1, __ATOMIC_RELAXED);
    }
    AOS2_HIP_CHECK(hipStreamSynchronize(q));
    AOS2_HIP_CHECK(hipGetLastError());
    return AOS2_OK;
}

// One continuation round: the windows that are not finished when a program has run (steps rejected by the gain ratio) get another,
// sized for what they still need at most if no further step is rejected, compacted: their descriptors and task lists, which address
// them by position, go to the continuation region.  *done: there was no such window.
static int continuation_round(LaunchCtx &C, const Batch &Bt, int max_i2, int round, bool *done)
{
    aos2_lba *s = C.s;
    const ArenaPlan &A = Bt.A;
    std::vector<int> todo;
    int need1 = 0, need2 = 0;
    bool before_second = false;
    for (int i = 0; i < (int)Bt.act.size(); ++i) {
        const LmState *ls = Bt.state_of(s, i);
        if (ls->phase == 3) continue;
        todo.push_back(i);
        if (ls->phase == 0) need1 = std::max(need1, std::max(1, ls->iters_max[0] - ls->it));
        if (ls->phase <= 1) before_second = true;
        if (ls->phase == 2) need2 = std::max(need2, std::max(1, ls->iters_max[1] - ls->it));
    }
    *done = todo.empty();
    if (*done) return AOS2_OK;
    if (round > 64) {   // 2 x 10 iterations x 10 trials at most: cannot happen
        set_error("internal: LocalBA program did not finish");
        return AOS2_ERR_ARG;
    }
    if (before_second) need2 = std::max(need2, max_i2);
    TaskLists TC;
    static const bool force_one_queue = getenv("AOS2_LBA_CONT_ONE_QUEUE") != nullptr;   // (test hook: the one-queue fallback on every continuation)
    if (!continuation_tasks(Bt.passes, todo, Bt.lay, A, force_one_queue, TC)) {
        set_error("internal: continuation region");
        return AOS2_ERR_ARG;
    }
    uint8_t *hc = s->h_in.p + A.o_cont;
    const uint8_t *dc = s->arena.p + A.o_cont;
    GroupDims D;
    for (size_t k = 0; k < todo.size(); ++k) {
        const int i = todo[k];
        reinterpret_cast<LbaWin *>(hc)[k] = Bt.hw[i];
        D.add(Bt.problems[Bt.act[i]], Bt.passes[i], A.L[i]);
    }
    size_t o = sizeof(LbaWin) * todo.size();
    const DevTasks dt = put_tasks(TC, hc, dc, o);
    AOS2_HIP_CHECK(hipMemcpyAsync(s->arena.p + A.o_cont, hc, o, hipMemcpyHostToDevice, s->stream));
    const Prog PC = make_prog((const LbaWin *)dc, (const LbaWin *)dc, (int)todo.size(), TC, dt, D, group_streams(s, 0));
    for (int t = 0; t < need1; ++t) enqueue_trial(C, PC, false);
    if (before_second) {
        enqueue_transition(PC);
        enqueue_init(C, PC);
    }
    for (int t = 0; t < need2; ++t) enqueue_trial(C, PC, false);
    s->last_trial_slots += need1 + need2;
    s->last_window_slots += (long long)(need1 + need2) * (long long)todo.size();
    s->last_host_rounds++;
    return finish(s, &PC, 1, Bt);
}

static void write_back(const aos2_lba *s, const Batch &Bt, aos2_lba_result_t *results)
{
    const ArenaPlan &A = Bt.A;
    const int nw = (int)Bt.act.size();
    if (getenv("AOS2_LBA_TRACE"))
        for (int i = 0; i < nw; ++i) {
            const LmState *ls = Bt.state_of(s, i);
            for (int t = 0; t < ls->ntr; ++t)
                fprintf(stderr, "[lba] win %d trial %2d lambda %.6e chi %.9e -> %.9e rho %.6e\n", i, t, ls->tr_lambda[t], ls->tr_cur[t], ls->tr_temp[t], ls->tr_rho[t]);
        }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, s->ev[0], s->ev[1]);
    for (int i = 0; i < nw; ++i) {
        const aos2_lba_problem_t *p = Bt.problems + Bt.act[i];
        aos2_lba_result_t *r = results + Bt.act[i];
        const WinLayout &l = A.L[i];
        const uint8_t *hb = s->h_stage.p;
        const LmState *ls = Bt.state_of(s, i);
        memcpy(r->pose_Tcw, hb + (l.out_Tcw - A.o_res), 64 * (size_t)p->n_poses);
        memcpy(r->point_xyz, hb + (l.out_xyz - A.o_res), 12 * (size_t)p->n_points);
        if (r->edge_outlier) memcpy(r->edge_outlier, hb + (l.out_outlier - A.o_res), (size_t)p->n_edges);
        if (r->edge_chi2) memcpy(r->edge_chi2, hb + (l.out_chi2 - A.o_res), 8 * (size_t)p->n_edges);
        r->iters_done_first = ls->iters_done[0];
        r->iters_done_second = ls->iters_done[1];
        r->trials_first = ls->trials[0];
        r->trials_second = ls->trials[1];
        r->final_chi2 = ls->final_chi2;
        r->final_lambda = ls->final_lambda;
        r->polls = ls->polls;
        r->stop_poll = ls->stop_poll;
        r->ms_device = ms;
    }
}

}  // namespace aos2

using namespace aos2;

extern "C" {

int aos2_lba_create(int device, aos2_lba_t **out)
{
    if (!out) return AOS2_ERR_ARG;
    aos2_lba *s = new aos2_lba();
    s->device = device;
    *out = s;
    return AOS2_OK;
}

void aos2_lba_destroy(aos2_lba_t *s)
{
    if (!s) return;
    delete static_cast<LbaCache *>(s->lba_cache);
    if (s->dev_ready) {
        (void)hipSetDevice(s->device);
        (void)hipStreamSynchronize(s->stream);
        s->arena.release();
        s->h_stage.release();
        s->h_in.release();
        s->h_abort.release();
        for (auto &e : s->ev) (void)hipEventDestroy(e);
        (void)hipEventDestroy(s->ev_fork);
        (void)hipEventDestroy(s->ev_join);
        if (s->stream_b) {
            for (hipEvent_t e : {s->ev_fork_b, s->ev_join_b, s->ev_up, s->ev_stag, s->ev_done_b}) (void)hipEventDestroy(e);
            (void)hipStreamSynchronize(s->stream_b);
            (void)hipStreamDestroy(s->stream2_b);
            (void)hipStreamDestroy(s->stream_b);
        }
        (void)hipStreamDestroy(s->stream2);
        (void)hipStreamDestroy(s->stream);
    }
    delete s;
}

int aos2_lba_set_host_threads(aos2_lba_t *s, int n)
{
    if (!s || n < 0) {
        set_error("aos2_lba_set_host_threads: bad argument");
        return AOS2_ERR_ARG;
    }
    s->host_threads = n;
    return AOS2_OK;
}

int aos2_lba_set_window_groups(aos2_lba_t *s, int n)
{
    if (!s || n < 0 || n > 2) {
        set_error("aos2_lba_set_window_groups: 0 (default), 1 or 2");
        return AOS2_ERR_ARG;
    }
    s->window_groups = n;
    return AOS2_OK;
}

int aos2_lba_last_program(const aos2_lba_t *s, int32_t *trial_slots, int32_t *host_rounds)
{
    if (!s) {
        set_error("aos2_lba_last_program: no handle");
        return AOS2_ERR_ARG;
    }
    if (trial_slots) *trial_slots = s->last_trial_slots;
    if (host_rounds) *host_rounds = s->last_host_rounds;
    return AOS2_OK;
}

int aos2_lba_last_window_slots(const aos2_lba_t *s, int64_t *window_slots)
{
    if (!s || !window_slots) {
        set_error("aos2_lba_last_window_slots: bad argument");
        return AOS2_ERR_ARG;
    }
    *window_slots = s->last_window_slots;
    return AOS2_OK;
}

int aos2_lba_debug_stop_at_poll(aos2_lba_t *s, int poll)
{
    if (!s || poll < 0) return AOS2_ERR_ARG;
    s->debug_stop_at_poll = poll;
    return AOS2_OK;
}

int aos2_lba_solve_batch(aos2_lba_t *s, const aos2_lba_problem_t *problems, aos2_lba_result_t *results, int n_problems)
{
    if (!s || !problems || !results || n_problems <= 0) {
        set_error("bad LocalBA batch");
        return AOS2_ERR_ARG;
    }
    // ---- the windows that run, dealt to one or two groups
    std::vector<int> act;
    bool want_chi2;
    int st = settle_entry(s, problems, results, n_problems, act, want_chi2);
    if (st) return st;
    const int nw = (int)act.size();
    if (nw == 0) return AOS2_OK;
    if ((st = lba_handle_init(s))) return st;
    int goff[3];
    const int G = deal_groups(s, problems, act, goff);
    if (G == 2 && (st = lba_group_streams(s))) return st;
    // layout of the landmark kernels: kLmSlots threads per landmark while the landmarks of the call cannot fill the device
    // (one or a few windows: latency), one thread per landmark beyond (throughput); same results either way.
    // AOS2_LBA_LAYOUT=slots|walk forces one (tests).
    size_t total_points = 0;
    for (int i = 0; i < nw; ++i) total_points += (size_t)problems[act[i]].n_points;
    bool walk = total_points > 16000;
    if (const char *e = getenv("AOS2_LBA_LAYOUT")) walk = !strcmp(e, "walk");
    const LmLayout lay = lm_layout(walk);

    // ---- per-window structure, task lists, arena, staging + upload, descriptors
    Uploaded U;
    if ((st = build_and_upload(s, problems, act, goff, G, lay, want_chi2, U))) return st;
    const std::vector<Pass> &passes = *U.passes;
    const ArenaPlan &A = U.A;
    const int max_i1 = U.max_i1, max_i2 = U.max_i2;
    uint8_t *base = s->arena.p;

    // ---- the program
    auto rg = std::make_unique<RoctxRange>("LocalBA::optimize(5) + outlier pass + optimize(10) + inlier check (one device program)");
    // As many trials as iterations per optimisation -- what every window needs whose steps are all accepted.  A window
    // with rejected steps is not finished when the program ends: it leaves with the others' results and gets a continuation round
    // sized for what it still needs, together with the (few) windows like it, compacted (continuation_round).  Rounds 2-4 enqueued one spare
    // trial per optimisation for EVERY window instead (AOS2_LBA_SPARE_SLOTS=1): 13 % of the launches of a batch whose windows need none.
    const int spare = getenv("AOS2_LBA_SPARE_SLOTS") ? atoi(getenv("AOS2_LBA_SPARE_SLOTS")) : 0;
    const int iters[2] = {max_i1, max_i2}, slots[2] = {max_i1 > 0 ? max_i1 + spare : 0, max_i2 > 0 ? max_i2 + spare : 0};
    s->last_trial_slots = slots[0] + slots[1];
    s->last_window_slots = (long long)(slots[0] + slots[1]) * nw;
    s->last_host_rounds = 1;
    const LbaWin *dw = (const LbaWin *)(base + A.o_wins);
    LaunchCtx C{s, walk, G == 2};
    Prog PG[2];
    for (int g = 0; g < G; ++g) {
        PG[g] = make_prog(dw, dw + goff[g], goff[g + 1] - goff[g], U.TL[g], U.dt[g], U.gd[g], group_streams(s, g));
        enqueue_program(C, PG[g], g == 0, iters, slots);
    }
    const Batch Bt{problems, act, passes, A, lay, U.hw, U.any_flag};
    if ((st = finish(s, PG, G, Bt))) return st;

    // ---- continuation rounds, write-back
    for (int round = 0;; ++round) {
        bool done;
        if ((st = continuation_round(C, Bt, max_i2, round, &done))) return st;
        if (done) break;
    }
    rg = std::make_unique<RoctxRange>("LocalBA::write-back");
    write_back(s, Bt, results);
    return AOS2_OK;
}

int aos2_lba_solve(aos2_lba_t *s, const aos2_lba_problem_t *p, aos2_lba_result_t *r)
{
    if (!s || !p || !r) {
        set_error("bad LocalBA problem");
        return AOS2_ERR_ARG;
    }
    const int st = aos2_lba_solve_batch(s, p, r, 1);
    return st ? st : r->status;
}

}  // extern "C"
