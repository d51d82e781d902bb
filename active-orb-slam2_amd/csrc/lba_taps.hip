// LocalBA's test taps: the host phase without a device, the reduced-system kernels alone, the assembled system of a trial, and a
// trial's landmark half with the LM decision.  They run the solve's own plan (csrc/lba_plan.h), host phase (csrc/lba_solve.h) and
// launch helpers (csrc/lba_launch.h).  No kernel here.
#include <chrono>

#include "lba_solve.h"

using namespace aos2;

// What the assembly tap and the trial tap (`name`) do before their own launches: the check of the problems and, through out_ok(w), of
// the tap's own output struct; what the host phase refuses, before a device is looked for; the handle; all windows as one group, the
// landmark layout as the caller says (1 = walk); the solve's host phase up to the upload; the group's Prog.
struct TapSetup {
    Uploaded U;
    LaunchCtx C;
    Prog P;
};
template <class OutOk>
static int tap_setup(const char *name, aos2_lba *s, const aos2_lba_problem_t *problems, int n_problems, int layout, bool second_runs, bool want_chi2,
                     OutOk &&out_ok, TapSetup &T)
{
    for (int w = 0; w < n_problems; ++w) {
        const aos2_lba_problem_t *p = problems + w;
        if (p->n_poses <= 0 || p->n_points <= 0 || p->n_edges <= 0 || !p->pose_Tcw || !p->pose_fixed || !p->pose_id || !p->point_xyz || !p->point_id ||
            !p->edge_pose || !p->edge_point || !p->edge_obs || !p->edge_stereo || !p->edge_inv_sigma2 || p->iters_first < 1 ||
            (second_runs && p->iters_second < 1) || !out_ok(w)) {
            set_error("%s: bad problem or output %d", name, w);
            return AOS2_ERR_ARG;
        }
    }
    int st;
    {
        std::vector<Pass> probe(n_problems);
        WindowPool serial;
        if ((st = build_structures(serial, problems, nullptr, n_problems, probe))) return st;
        for (int w = 0; w < n_problems; ++w)
            if (probe[w].np < 1) {
                set_error("%s: problem %d has no free keyframe with an edge", name, w);
                return AOS2_ERR_ARG;
            }
    }
    if ((st = lba_handle_init(s))) return st;
    const int nw = n_problems;
    std::vector<int> act(nw);
    std::iota(act.begin(), act.end(), 0);
    const int goff[3] = {0, nw, nw};
    const bool walk = layout == 1;
    if ((st = build_and_upload(s, problems, act, goff, 1, lm_layout(walk), want_chi2, T.U))) return st;
    const LbaWin *dw = (const LbaWin *)(s->arena.p + T.U.A.o_wins);
    T.C = LaunchCtx{s, walk, false};
    T.P = make_prog(dw, dw, nw, T.U.TL[0], T.U.dt[0], T.U.gd[0], group_streams(s, 0));
    return AOS2_OK;
}

extern "C" {

// The host part of aos2_lba_solve_batch without a device: the per-window index structures (build_pass, Schur items and units)
// and the staging copies (into pageable memory here), on `threads` worker threads.  For measuring / testing how the host phases of
// several ranks share a node's cores (tests/test_sharding_cpu.py); returns the wall time of the two phases.
int aos2_lba_debug_host_phase(const aos2_lba_problem_t *problems, int n_problems, int threads, double *build_ms, double *stage_ms)
{
    if (!problems || n_problems <= 0 || threads <= 0) {
        set_error("aos2_lba_debug_host_phase: bad argument");
        return AOS2_ERR_ARG;
    }
    std::vector<Pass> passes(n_problems);
    WindowPool pool;
    if (n_problems > 1 && threads > 1) pool.start(std::min(threads, n_problems));
    const auto t0 = std::chrono::steady_clock::now();
    if (int st = build_structures(pool, problems, nullptr, n_problems, passes)) return st;
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<std::vector<uint8_t>> stage(n_problems);
    pool.run(n_problems, [&](int i) {
        WinLayout l{};
        Bump B;
        layout_staged(problems[i], passes[i], B, l);
        stage[i].resize(B.size);
        stage_window(stage[i].data(), l, problems[i], passes[i]);
    });
    const auto t2 = std::chrono::steady_clock::now();
    if (build_ms) *build_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (stage_ms) *stage_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    return AOS2_OK;
}

// Test tap: k_ldlt_reg / k_ldlt_dev alone.  One hand-made window descriptor and state per case -- only the members the two kernels read --
// over a padded matrix filled like k_schur and k_prepare leave it; launched through enqueue_ldlt like a trial's.
int aos2_debug_lba_reduced_solve_device(int n_cases, const int32_t *np, const int32_t *form, const double *H, const double *bs, const double *b_pose,
                                        const double *lambda, const double *T, double *x, double *T_out, double *T_backup, double *scale_terms,
                                        uint8_t *ok, int device)
{
    if (n_cases < 1 || !np || !form || !H || !bs || !b_pose || !lambda || !T || !x || !T_out || !T_backup || !scale_terms || !ok) {
        set_error("aos2_debug_lba_reduced_solve_device: bad argument");
        return AOS2_ERR_ARG;
    }
    for (int c = 0; c < n_cases; ++c) {
        if (form[c] != kLdltDev && form[c] != kLdltReg) {
            set_error("aos2_debug_lba_reduced_solve_device: case %d: form %d (0 = k_ldlt_dev, 2 = k_ldlt_reg)", c, form[c]);
            return AOS2_ERR_ARG;
        }
        if (np[c] < 1 || np[c] > (form[c] == kLdltReg ? kLrMaxNpad / 6 : kLdMaxNp)) {
            set_error("aos2_debug_lba_reduced_solve_device: case %d: %d free keyframes, form %d takes 1..%d", c, np[c], form[c],
                      form[c] == kLdltReg ? kLrMaxNpad / 6 : kLdMaxNp);
            return AOS2_ERR_ARG;
        }
    }
    int st = bind_device(device);
    if (st) return st;
    if ((st = ldlt_declare_lds())) return st;
    // regions of a case in one buffer (offsets in bytes)
    struct CaseLayout {
        size_t Hs, bs, b, x, tmp, scal, pose, bk, hpose, st;
        int n, npad;
    };
    std::vector<CaseLayout> L(n_cases);
    Bump B;
    const size_t o_wins = B.take(sizeof(LbaWin) * (size_t)n_cases);
    int mx_npad[2] = {0, 0};   // register form, device-memory form
    for (int c = 0; c < n_cases; ++c) {
        CaseLayout &l = L[c];
        l.n = 6 * np[c];
        l.npad = (l.n + 15) & ~15;
        int &mx = mx_npad[form[c] == kLdltReg ? 0 : 1];
        mx = std::max(mx, l.npad);
        const size_t n8 = 8 * (size_t)l.n, p56 = 56 * (size_t)np[c];
        l.Hs = B.take(8 * (size_t)l.npad * l.npad); l.bs = B.take(n8); l.b = B.take(n8); l.x = B.take(n8); l.tmp = B.take(n8);
        l.scal = B.take(64); l.pose = B.take(p56); l.bk = B.take(p56); l.hpose = B.take(4 * (size_t)np[c]); l.st = B.take(sizeof(LmState));
    }
    std::vector<uint8_t> host(B.size, 0);
    DevBuf<uint8_t> dev;
    if ((st = dev.alloc(B.size))) return st;
    size_t oH = 0, ov = 0, oT = 0;   // the case's place in the caller's arrays (doubles)
    for (int c = 0; c < n_cases; ++c) {
        const CaseLayout &l = L[c];
        const int n = l.n, npad = l.npad;
        double *Hs = (double *)(host.data() + l.Hs);
        for (int r = 0; r < npad; ++r)
            for (int q = 0; q < npad; ++q) Hs[(size_t)r * npad + q] = r < n && q < n ? H[oH + (size_t)r * n + q] : r == q ? 1.0 : 0.0;
        memcpy(host.data() + l.bs, bs + ov, 8 * (size_t)n);
        memcpy(host.data() + l.b, b_pose + ov, 8 * (size_t)n);
        memcpy(host.data() + l.x, x + ov, 8 * (size_t)n);
        memcpy(host.data() + l.tmp, scale_terms + ov, 8 * (size_t)n);
        ((double *)(host.data() + l.scal))[3] = -1.0;   // (neither kernel ran: ok = 255)
        memcpy(host.data() + l.pose, T + oT, 56 * (size_t)np[c]);
        memset(host.data() + l.bk, 0xFF, 56 * (size_t)np[c]);   // (NaNs: the backup is the kernel's)
        for (int i = 0; i < np[c]; ++i) ((int32_t *)(host.data() + l.hpose))[i] = i;
        LmState *S = (LmState *)(host.data() + l.st);
        S->run = 1;
        S->lambda = lambda[c];
        LbaWin &W = ((LbaWin *)(host.data() + o_wins))[c];
        W.np = np[c]; W.npad = npad; W.hs_ld = npad; W.ldlt_form = (LdltForm)form[c];
        W.Hs = (double *)(dev.p + l.Hs); W.bs = (double *)(dev.p + l.bs); W.b = (double *)(dev.p + l.b); W.x = (double *)(dev.p + l.x);
        W.tmp = (double *)(dev.p + l.tmp); W.scal = (double *)(dev.p + l.scal);
        W.pose = (double *)(dev.p + l.pose); W.bk = (double *)(dev.p + l.bk); W.n_poses = np[c];
        W.hpose = (const int32_t *)(dev.p + l.hpose);
        W.st = (LmState *)(dev.p + l.st);
        oH += (size_t)n * n; ov += n; oT += 7 * (size_t)np[c];
    }
    st = [&]() -> int {
        AOS2_HIP_CHECK(hipMemcpy(dev.p, host.data(), B.size, hipMemcpyHostToDevice));
        enqueue_ldlt((const LbaWin *)(dev.p + o_wins), n_cases, mx_npad[0], mx_npad[1], 0, 0);
        AOS2_HIP_CHECK(hipGetLastError());
        AOS2_HIP_CHECK(hipDeviceSynchronize());
        AOS2_HIP_CHECK(hipMemcpy(host.data(), dev.p, B.size, hipMemcpyDeviceToHost));
        return AOS2_OK;
    }();
    dev.release();
    if (st) return st;
    ov = oT = 0;
    for (int c = 0; c < n_cases; ++c) {
        const CaseLayout &l = L[c];
        memcpy(x + ov, host.data() + l.x, 8 * (size_t)l.n);
        memcpy(scale_terms + ov, host.data() + l.tmp, 8 * (size_t)l.n);
        memcpy(T_out + oT, host.data() + l.pose, 56 * (size_t)np[c]);
        memcpy(T_backup + oT, host.data() + l.bk, 56 * (size_t)np[c]);
        const double s3 = ((const double *)(host.data() + l.scal))[3];
        ok[c] = s3 == 1.0 ? 1 : s3 == 0.0 ? 0 : 255;
        ov += l.n; oT += 7 * (size_t)np[c];
    }
    return AOS2_OK;
}

// Test tap: the system a Levenberg-Marquardt trial solves, as the shipped kernels assemble it.  The host phase is aos2_lba_solve_batch's
// (build_and_upload), the launches go through its helpers; one group, the landmark layout as the caller says.
int aos2_debug_lba_assemble_device(aos2_lba_t *s, const aos2_lba_problem_t *problems, int n_problems, int layout, int stage, const double *lambda,
                                   aos2_lba_system_t *out)
{
    if (!s || !problems || !out || n_problems < 1 || (layout != 0 && layout != 1) || (stage != 0 && stage != 1)) {
        set_error("aos2_debug_lba_assemble_device: bad argument (layout 0 = slots, 1 = walk; stage 0 or 1)");
        return AOS2_ERR_ARG;
    }
    auto out_ok = [&](int w) {
        const aos2_lba_system_t *o = out + w;
        return o->hpose && o->hpoint && o->pose && o->point && o->e_level1 && o->e_robust && o->Hpp_init && o->b_init && o->b_p && o->Hll && o->b_l &&
               o->Hs && o->bs && o->blk_off && o->units;
    };
    TapSetup T;
    int st = tap_setup("aos2_debug_lba_assemble_device", s, problems, n_problems, layout, stage == 1, false, out_ok, T);
    if (st) return st;
    const int nw = n_problems;
    const std::vector<Pass> &passes = *T.U.passes;
    const ArenaPlan &A = T.U.A;
    LaunchCtx &C = T.C;
    const Prog &P = T.P;
    uint8_t *base = s->arena.p;
    // Hpp and the pose part of b as the first linearisation left them, copied aside between k_lm_init and k_schur
    std::vector<size_t> o_snap(nw);
    Bump SB;
    for (int i = 0; i < nw; ++i) o_snap[i] = SB.take(8 * 42 * (size_t)passes[i].np);
    DevBuf<uint8_t> snap;
    if ((st = snap.alloc(SB.size))) return st;
    std::vector<uint8_t> host(A.bytes), hsnap(SB.size);
    st = [&]() -> int {
        enqueue_prepare(C, P);
        if (stage == 1) {
            enqueue_init(C, P);
            for (int t = 0; t < T.U.max_i1; ++t) enqueue_trial(C, P, true);
            enqueue_transition(P);
        }
        enqueue_init(C, P);
        for (int i = 0; i < nw; ++i) {
            const size_t n36 = 8 * 36 * (size_t)passes[i].np, n6 = 8 * 6 * (size_t)passes[i].np;
            if (lambda && lambda[i] > 0) AOS2_HIP_CHECK(hipMemcpyAsync(base + A.L[i].st + offsetof(LmState, lambda), lambda + i, 8, hipMemcpyHostToDevice, P.q));
            AOS2_HIP_CHECK(hipMemcpyAsync(snap.p + o_snap[i], base + A.L[i].Hpp, n36, hipMemcpyDeviceToDevice, P.q));
            AOS2_HIP_CHECK(hipMemcpyAsync(snap.p + o_snap[i] + n36, base + A.L[i].b, n6, hipMemcpyDeviceToDevice, P.q));
        }
        enqueue_schur(P);
        AOS2_HIP_CHECK(hipGetLastError());
        AOS2_HIP_CHECK(hipStreamSynchronize(P.q));
        AOS2_HIP_CHECK(hipMemcpy(host.data(), base, A.bytes, hipMemcpyDeviceToHost));
        AOS2_HIP_CHECK(hipMemcpy(hsnap.data(), snap.p, SB.size, hipMemcpyDeviceToHost));
        return AOS2_OK;
    }();
    snap.release();
    if (st) return st;
    for (int i = 0; i < nw; ++i) {
        const aos2_lba_problem_t &p = problems[i];
        const Pass &S = passes[i];
        const WinLayout &l = A.L[i];
        aos2_lba_system_t &o = out[i];
        const uint8_t *h = host.data();
        const LmState *ls = (const LmState *)(h + l.st);
        const size_t np = S.np, nl = S.nl, npad = l.npad;
        o.np = S.np; o.nl = S.nl; o.npad = l.npad;
        o.phase = ls->phase; o.trials_first = ls->trials[0]; o.iters_done_first = ls->iters_done[0];
        o.lambda = ls->lambda; o.current_chi = ls->currentChi;
        memcpy(o.hpose, S.hpose.data(), 4 * np);
        memcpy(o.hpoint, S.hpoint.data(), 4 * nl);
        memcpy(o.blk_off, S.blk_off.data(), 4 * (np * (np + 1) / 2 + 1));
        o.n_units = (int32_t)S.units.size();
        memcpy(o.units, S.units.data(), 4 * S.units.size());
        memcpy(o.pose, h + l.est, 8 * 7 * (size_t)p.n_poses);
        memcpy(o.point, h + l.est + 8 * 7 * (size_t)p.n_poses, 8 * 3 * (size_t)p.n_points);
        memcpy(o.e_level1, h + l.level1, (size_t)p.n_edges);
        memcpy(o.e_robust, h + l.robust, (size_t)p.n_edges);
        memcpy(o.Hpp_init, hsnap.data() + o_snap[i], 8 * 36 * np);
        memcpy(o.b_init, hsnap.data() + o_snap[i] + 8 * 36 * np, 8 * 6 * np);
        memcpy(o.b_p, h + l.b, 8 * 6 * np);
        memcpy(o.Hll, h + l.Hll, 8 * 9 * nl);
        memcpy(o.b_l, h + l.b + 8 * 6 * np, 8 * 3 * nl);
        memcpy(o.Hs, h + l.Hs, 8 * npad * npad);
        memcpy(o.bs, h + l.bs, 8 * 6 * np);
    }
    return AOS2_OK;
}

// Test tap: the landmark half of a trial and the LM decision, the outlier pass and the final check, read between the shipped launches.
// Host phase and helpers as the assembly tap; a snapshot is a synchronisation and a copy of the arena (the windows are small).
int aos2_debug_lba_trial_device(aos2_lba_t *s, const aos2_lba_problem_t *problems, int n_problems, int layout, int trials_before, const double *lambda,
                                const uint8_t *force_solver_failed, int tail, aos2_lba_trial_t *out)
{
    if (!s || !problems || !out || n_problems < 1 || (layout != 0 && layout != 1) || trials_before < 0 || tail < 0 || tail > 2) {
        set_error("aos2_debug_lba_trial_device: bad argument (layout 0 = slots, 1 = walk; trials_before >= 0; tail 0, 1 or 2)");
        return AOS2_ERR_ARG;
    }
    auto out_ok = [&](int w) {
        const aos2_lba_trial_t *o = out + w;
        return o->hpose && o->hpoint && o->pt_off && o->pt_k && o->pl_pos;
    };
    TapSetup T;
    int st = tap_setup("aos2_debug_lba_trial_device", s, problems, n_problems, layout, false, true, out_ok, T);
    if (st) return st;
    const int nw = n_problems;
    const std::vector<Pass> &passes = *T.U.passes;
    const ArenaPlan &A = T.U.A;
    LaunchCtx &C = T.C;
    const Prog &P = T.P;
    uint8_t *base = s->arena.p;
    std::vector<uint8_t> host(A.bytes);
    for (int i = 0; i < nw; ++i) {
        const Pass &S = passes[i];
        aos2_lba_trial_t &o = out[i];
        o.np = S.np; o.nl = S.nl; o.n_pl = (int32_t)S.pl_k.size(); o.n_part = A.L[i].n_part;
        memcpy(o.hpose, S.hpose.data(), 4 * (size_t)S.np);
        memcpy(o.hpoint, S.hpoint.data(), 4 * (size_t)S.nl);
        memcpy(o.pt_off, S.pt_off.data(), 4 * S.pt_off.size());
        memcpy(o.pt_k, S.pt_k.data(), 4 * S.pt_k.size());
        memcpy(o.pl_pos, S.pl_pos.data(), 4 * S.pl_pos.size());
        for (auto &sn : o.snap) sn.taken = 0;
    }
    hipStream_t q = s->stream;
    auto snapshot = [&](int k) -> int {
        AOS2_HIP_CHECK(hipGetLastError());
        AOS2_HIP_CHECK(hipStreamSynchronize(q));
        AOS2_HIP_CHECK(hipMemcpy(host.data(), base, A.bytes, hipMemcpyDeviceToHost));
        for (int i = 0; i < nw; ++i) {
            const aos2_lba_problem_t &p = problems[i];
            const Pass &S = passes[i];
            const WinLayout &l = A.L[i];
            aos2_lba_trial_snap_t &o = out[i].snap[k];
            const uint8_t *h = host.data();
            const size_t NP = p.n_poses, NL = p.n_points, E = p.n_edges, np = S.np, nl = S.nl, est = 8 * (7 * NP + 3 * NL);
            auto put = [&](void *dst, size_t off, size_t bytes) {
                if (dst && bytes) memcpy(dst, h + off, bytes);
            };
            o.taken = 1;
            const LmState *ls = (const LmState *)(h + l.st);
            aos2_lba_lm_state_t &t = o.st;
            t.lambda = ls->lambda; t.ni = ls->ni; t.currentChi = ls->currentChi; t.iniChi = ls->iniChi;
            t.final_chi2 = ls->final_chi2; t.final_lambda = ls->final_lambda;
            t.phase = ls->phase; t.run = ls->run; t.lin = ls->lin; t.initp = ls->initp; t.xmark = ls->xmark;
            t.it = ls->it; t.qmax = ls->qmax; t.nBad = ls->nBad;
            for (int j = 0; j < 2; ++j) {
                t.iters_done[j] = ls->iters_done[j];
                t.trials[j] = ls->trials[j];
            }
            t.polls = ls->polls; t.stop_poll = ls->stop_poll; t.n_active = ls->n_active; t.solver_failed = ls->solver_failed;
            t.err_at = ls->err_at; t.ntr = ls->ntr;
            memcpy(t.tr_rho, ls->tr_rho, sizeof t.tr_rho); memcpy(t.tr_temp, ls->tr_temp, sizeof t.tr_temp);
            memcpy(t.tr_cur, ls->tr_cur, sizeof t.tr_cur); memcpy(t.tr_lambda, ls->tr_lambda, sizeof t.tr_lambda);
            o.scal3 = ((const double *)(h + l.scal))[3];
            put(o.est, l.est, est); put(o.bk, l.bk, est);
            put(o.x, l.x, 8 * (6 * np + 3 * nl)); put(o.b, l.b, 8 * (6 * np + 3 * nl));
            put(o.Hll, l.Hll, 72 * nl); put(o.Rl, l.Rl, 72 * np); put(o.tmp, l.tmp, 48 * np); put(o.part, l.part, 16 * nl);
            put(o.e_level1, l.level1, E); put(o.e_robust, l.robust, E);
            put(o.err, l.err, 24 * E); put(o.lrec, l.lrec, 32 * S.pl_k.size());
            if (o.erec_flags)
                for (size_t a = 0; a < E; ++a) o.erec_flags[a] = ((const EdgeRec *)(h + l.erec))[a].flags;
            put(o.out_Tcw, l.out_Tcw, 64 * NP); put(o.out_xyz, l.out_xyz, 12 * NL);
            put(o.out_chi2, l.out_chi2, 8 * E); put(o.out_outlier, l.out_outlier, E);
        }
        return AOS2_OK;
    };
    static const double zero = 0.0;
    enqueue_prepare(C, P);
    enqueue_init(C, P);
    for (int i = 0; i < nw; ++i)
        if (lambda && lambda[i] > 0) AOS2_HIP_CHECK(hipMemcpyAsync(base + A.L[i].st + offsetof(LmState, lambda), lambda + i, 8, hipMemcpyHostToDevice, q));
    // The second optimisation starts where the solve's programs start it: behind iters_first trials when every step was accepted
    // (enqueue_program), behind whichever later trial ends the first optimisation otherwise (continuation_round) -- both launches are
    // gated by the state (xmark, initp), so they are enqueued before every trial from there on
    auto between = [&](int t) {
        if (t < T.U.max_i1) return;
        enqueue_transition(P);
        enqueue_init(C, P);
    };
    for (int t = 0; t < trials_before; ++t) {
        between(t);
        enqueue_trial(C, P, true);
    }
    between(trials_before);
    enqueue_reduced(C, P, true);
    for (int i = 0; i < nw; ++i)
        if (force_solver_failed && force_solver_failed[i]) AOS2_HIP_CHECK(hipMemcpyAsync(base + A.L[i].scal + 24, &zero, 8, hipMemcpyHostToDevice, q));
    if ((st = snapshot(0))) return st;
    enqueue_points(C, P, 1);
    if ((st = snapshot(1))) return st;
    enqueue_lin(C, P, 0);
    if ((st = snapshot(2))) return st;
    if (tail >= 1) {
        enqueue_transition(P);
        if ((st = snapshot(3))) return st;
    }
    if (tail == 2) {
        enqueue_final(P);
        if ((st = snapshot(4))) return st;
    }
    return AOS2_OK;
}

}  // extern "C"
