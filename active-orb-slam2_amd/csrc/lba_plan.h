// LocalBA: the host plan of a call -- the index structures of a window (index mapping, edge lists, Schur items and units), the byte
// layout of the arena, the staging copies, the window descriptors and the task lists of the launches.  Every index a LocalBA kernel
// dereferences is decided here.  Host C++ on the standard library alone, no HIP: csrc/lba_solve.hip and csrc/lba_taps.hip run it,
// and tests/cpp/lba_plan_check.cpp compiles it stand-alone under the sanitizers and checks what the comments below promise.
// Internal to the library.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <numeric>
#include <thread>
#include <vector>

#include "../../include/aos2.h"
#include "lba_window.h"

namespace aos2 {

void set_error(const char *fmt, ...);   // (aos2_common.h's; a stand-alone program supplies its own)

// index mapping and edge lists of a window: initializeOptimization(level 0) + buildIndexMapping + the symbolic part of
// buildStructure for ALL edges (the second optimisation masks edges instead of rebuilding)
struct Pass {
    std::vector<int32_t> k_ph, k_lh, hpose, hpoint, pt_off, pt_k, ps_off, ps_k, pl_off, pl_k;
    std::vector<int32_t> pl_pos, pl_ph;   // edge -> position in pl_k (-1: fixed keyframe); position -> pose hidx
    std::vector<int32_t> it_ka, it_kb, it_l, blk_off;   // Schur items (k_schur_items / k_schur_blocks)
    std::vector<int32_t> sr_o0, sr_info, sr_ij, units;    // k_schur's row table and unit codes (build_schur_units)
    int np = 0, nl = 0;
};
// worker threads of a handle for the per-window host work of a batch (structure build, staging): created once -- 32
// std::thread per phase cost ~1 ms per call
struct WindowPool {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv_go, cv_done;
    std::function<void(int)> fn;
    int n_items = 0, generation = 0, running = 0;
    std::atomic<int> next{0};
    bool quit = false;
    void start(int n)
    {
        int born;
        {
            std::lock_guard<std::mutex> lk(m);
            born = generation;   // a thread added later starts with the jobs after its creation, not with a finished one
        }
        active = n;
        for (int t = (int)th.size(); t < n; ++t)
            th.emplace_back([this, born, idx = t] {
                int seen = born;
                for (;;) {
                    {
                        std::unique_lock<std::mutex> lk(m);
                        cv_go.wait(lk, [&] { return quit || generation != seen; });
                        if (quit) return;
                        seen = generation;
                    }
                    if (idx < active)
                        for (int i; (i = next.fetch_add(1)) < n_items;) fn(i);
                    std::lock_guard<std::mutex> lk(m);
                    if (--running == 0) cv_done.notify_one();
                }
            });
    }
    int active = 0;   // workers that take items of the current job (a lowered host_threads setting: the others just check in)
    void run(int n, std::function<void(int)> f)
    {
        if (n <= 1 || th.empty()) {
            for (int i = 0; i < n; ++i) f(i);
            return;
        }
        std::unique_lock<std::mutex> lk(m);
        fn = std::move(f);
        n_items = n;
        next = 0;
        running = (int)th.size();
        ++generation;
        cv_go.notify_all();
        cv_done.wait(lk, [&] { return running == 0; });
    }
    ~WindowPool()
    {
        {
            std::lock_guard<std::mutex> lk(m);
            quit = true;
        }
        cv_go.notify_all();
        for (auto &t : th) t.join();
    }
};

inline bool build_pass(const aos2_lba_problem_t *p, Pass &S)
{
    // (the vectors keep their storage from call to call: a 24 k-edge window holds ~1.5 MB of index lists, and fresh
    // allocations of that size are mmap / page faults / munmap every time -- 2 ms per 32-window call, half of it at scope exit)
    S.hpose.clear(); S.hpoint.clear(); S.it_ka.clear(); S.it_kb.clear(); S.it_l.clear(); S.blk_off.clear();
    S.np = S.nl = 0;
    const int E = p->n_edges;
    std::vector<uint8_t> pose_act(p->n_poses, 0), point_act(p->n_points, 0);
    for (int e = 0; e < E; ++e) {
        pose_act[p->edge_pose[e]] = 1;
        point_act[p->edge_point[e]] = 1;
    }
    std::vector<int32_t> pose_h(p->n_poses, -1), point_h(p->n_points, -1);
    for (int i = 0; i < p->n_poses; ++i)
        if (pose_act[i] && !p->pose_fixed[i]) S.hpose.push_back(i);
    auto by_pose_id = [&](int a, int b) { return p->pose_id[a] < p->pose_id[b]; };
    if (!std::is_sorted(S.hpose.begin(), S.hpose.end(), by_pose_id)) std::stable_sort(S.hpose.begin(), S.hpose.end(), by_pose_id);
    for (int i = 0; i < p->n_points; ++i)
        if (point_act[i]) S.hpoint.push_back(i);
    auto by_point_id = [&](int a, int b) { return p->point_id[a] < p->point_id[b]; };
    if (!std::is_sorted(S.hpoint.begin(), S.hpoint.end(), by_point_id)) std::stable_sort(S.hpoint.begin(), S.hpoint.end(), by_point_id);
    S.np = (int)S.hpose.size();
    S.nl = (int)S.hpoint.size();
    for (int i = 0; i < S.np; ++i) pose_h[S.hpose[i]] = i;
    for (int i = 0; i < S.nl; ++i) point_h[S.hpoint[i]] = i;
    S.k_ph.resize(E);
    S.k_lh.resize(E);
    S.pt_off.assign(S.nl + 1, 0);
    S.ps_off.assign(S.np + 1, 0);
    S.pl_off.assign(S.nl + 1, 0);
    for (int k = 0; k < E; ++k) {
        S.k_ph[k] = pose_h[p->edge_pose[k]];
        S.k_lh[k] = point_h[p->edge_point[k]];
        S.pt_off[S.k_lh[k] + 1]++;
        if (S.k_ph[k] >= 0) {
            S.ps_off[S.k_ph[k] + 1]++;
            S.pl_off[S.k_lh[k] + 1]++;
        }
    }
    for (int i = 0; i < S.nl; ++i) {
        S.pt_off[i + 1] += S.pt_off[i];
        S.pl_off[i + 1] += S.pl_off[i];
    }
    for (int i = 0; i < S.np; ++i) S.ps_off[i + 1] += S.ps_off[i];
    S.pt_k.resize(S.pt_off[S.nl]);
    S.ps_k.resize(S.ps_off[S.np]);
    S.pl_k.resize(S.pl_off[S.nl]);
    std::vector<int> f1(S.nl, 0), f2(S.np, 0), f3(S.nl, 0);
    for (int k = 0; k < E; ++k) {
        const int l = S.k_lh[k], ph = S.k_ph[k];
        S.pt_k[S.pt_off[l] + f1[l]++] = k;
        if (ph >= 0) {
            S.ps_k[S.ps_off[ph] + f2[ph]++] = k;
            S.pl_k[S.pl_off[l] + f3[l]++] = k;
        }
    }
    // per landmark: ascending pose index, ties in edge order (a stable insertion sort: the runs are a handful of
    // edges long, and std::stable_sort would allocate a buffer for each of the thousands of runs)
    for (int l = 0; l < S.nl; ++l) {
        int32_t *q = S.pl_k.data() + S.pl_off[l];
        const int m = S.pl_off[l + 1] - S.pl_off[l];
        for (int i = 1; i < m; ++i) {
            const int32_t v = q[i], key = S.k_ph[v];
            int j = i - 1;
            for (; j >= 0 && S.k_ph[q[j]] > key; --j) q[j + 1] = q[j];
            q[j + 1] = v;
        }
        for (int i = 1; i < m; ++i)
            if (S.k_ph[q[i]] == S.k_ph[q[i - 1]]) return false;   // two edges between one keyframe and one landmark
    }
    S.pl_pos.assign(E, -1);
    S.pl_ph.resize(S.pl_k.size());
    for (size_t a = 0; a < S.pl_k.size(); ++a) {
        S.pl_pos[S.pl_k[a]] = (int32_t)a;
        S.pl_ph[a] = S.k_ph[S.pl_k[a]];
    }
    return true;
}

// items ranked by (pose, pose) block -- upper block triangle, row-major -- and by landmark inside a block (counting
// sort; this order is the summation order of k_schur_blocks)
inline void build_schur_items(Pass &S)
{
    size_t n = 0;
    for (int l = 0; l < S.nl; ++l) {
        const size_t m = (size_t)(S.pl_off[l + 1] - S.pl_off[l]);
        n += m * (m + 1) / 2;
    }
    const int np = S.np;
    const size_t nblk = (size_t)np * (np + 1) / 2;
    S.it_ka.resize(n); S.it_kb.resize(n); S.it_l.resize(n);
    S.blk_off.assign(nblk + 1, 0);
    // block of (i1 <= i2) = row_base[i1] + i2 (pl_k is sorted by pose, so a <= b gives i1 <= i2)
    std::vector<int32_t> row_base(np > 0 ? np : 1);
    const std::vector<int32_t> &ph = S.pl_ph;
    for (int i = 0; i < np; ++i) row_base[i] = i * np - i * (i - 1) / 2 - i;
    for (int l = 0; l < S.nl; ++l) {
        const int32_t *q = ph.data() + S.pl_off[l];
        const int m = S.pl_off[l + 1] - S.pl_off[l];
        for (int a = 0; a < m; ++a) {
            int32_t *cnt = S.blk_off.data() + row_base[q[a]] + 1;
            for (int b = a; b < m; ++b) cnt[q[b]]++;
        }
    }
    for (size_t i = 0; i < nblk; ++i) S.blk_off[i + 1] += S.blk_off[i];
    std::vector<int32_t> fill(S.blk_off.begin(), S.blk_off.end() - 1);
    for (int l = 0; l < S.nl; ++l) {
        const int c0 = S.pl_off[l], m = S.pl_off[l + 1] - c0;
        const int32_t *q = ph.data() + c0;
        for (int a = 0; a < m; ++a) {   // (items name the two edges by their positions in the pl list = the indices of the dense Hpl array)
            int32_t *f = fill.data() + row_base[q[a]];
            const int32_t ka = c0 + a;
            for (int b = a; b < m; ++b) {
                const int slot = f[q[b]]++;
                S.it_ka[slot] = ka;
                S.it_kb[slot] = c0 + b;
                S.it_l[slot] = l;
            }
        }
    }
}

// k_schur's units of a window (see the kernel): DIAG units first (the long ones must not be dispatched last), then the BIG
// off-diagonal blocks, then the PACK units -- off-diagonal blocks in rank order, ceil(n / 16) rows each (an empty block keeps one
// row: its zeros are written like any other sum), a block never split across two units.
inline void build_schur_units(Pass &S)
{
    S.sr_o0.clear(); S.sr_info.clear(); S.sr_ij.clear(); S.units.clear();
    const int np = S.np;
    for (int i = 0; i < np; ++i) S.units.push_back((kSchurDiag << 28) | i);
    std::vector<int32_t> pack_first;
    int in_unit = 0;
    for (int i1 = 0, blk = 0; i1 < np; ++i1)
        for (int i2 = i1; i2 < np; ++i2, ++blk) {
            if (i2 == i1) continue;
            const int o0 = S.blk_off[blk], n = S.blk_off[blk + 1] - o0;
            if (n > 256) {
                S.units.push_back((kSchurBig << 28) | blk);
                continue;
            }
            const int nrows = std::max(1, (n + 15) / 16);
            if (in_unit + nrows > 16) {   // pad the unit: a block's rows stay together
                for (; in_unit < 16; ++in_unit) {
                    S.sr_o0.push_back(0); S.sr_info.push_back(0); S.sr_ij.push_back(0);
                }
                in_unit = 0;
            }
            if (in_unit == 0) pack_first.push_back((int32_t)S.sr_o0.size());
            for (int r = 0; r < nrows; ++r) {
                S.sr_o0.push_back(o0 + 16 * r);
                S.sr_info.push_back(std::max(0, std::min(16, n - 16 * r)) | (r << 8) | (nrows << 16));
                S.sr_ij.push_back(i1 | (i2 << 16));
            }
            in_unit = (in_unit + nrows) % 16;
        }
    for (int32_t f : pack_first) S.units.push_back((kSchurPack << 28) | f);
}

// byte offsets of one window's regions in the arena
struct WinLayout {
    // staged (uploaded)
    size_t in_Tcw, in_xyz, in_obs, in_w, e_pose, e_point, e_stereo, pl_pos, hpose, hpoint, pt_off, pt_k, ps_off, ps_k,
        pl_off, pl_k, it_ka, it_kb, it_l, blk_off, sr_o0, sr_info, sr_ij;
    // device only
    size_t est, bk, robust, level1, err, lrec, lomr, Rl, Hpp, Hll, b, x, Hs, bs, tmp, scal, part, erec;
    // results (downloaded)
    size_t out_Tcw, out_xyz, out_outlier, out_chi2, st;
    int n_part, npad;
    LdltForm ldlt_form;
    size_t n_items;
};

struct Bump {
    size_t size = 0;
    size_t take(size_t bytes, size_t align = 256)
    {
        const size_t off = (size + align - 1) & ~(align - 1);
        size = off + bytes;
        return off;
    }
};

// ---- the per-window host work: index structures, arena regions, staging

// The index structures of n windows -- window i is problems[ids ? ids[i] : i] -- into passes[0 .. n), a pool thread per window,
// after the range check of the edges' vertex indices
inline int build_structures(WindowPool &pool, const aos2_lba_problem_t *problems, const int *ids, int n, std::vector<Pass> &passes)
{
    std::vector<uint8_t> pass_ok(n, 1);
    std::vector<int> bad_edge(n, -1);
    pool.run(n, [&](int i) {
        const aos2_lba_problem_t *p = problems + (ids ? ids[i] : i);
        for (int e = 0; e < p->n_edges; ++e)
            if (p->edge_pose[e] < 0 || p->edge_pose[e] >= p->n_poses || p->edge_point[e] < 0 || p->edge_point[e] >= p->n_points) {
                bad_edge[i] = e;
                return;
            }
        pass_ok[i] = build_pass(p, passes[i]) ? 1 : 0;
        if (pass_ok[i] && passes[i].np > 0) {
            build_schur_items(passes[i]);
            build_schur_units(passes[i]);
        } else
            passes[i].units.clear();
    });
    for (int i = 0; i < n; ++i)
        if (bad_edge[i] >= 0) {
            set_error("problem %d: edge %d references a vertex out of range", ids ? ids[i] : i, bad_edge[i]);
            return AOS2_ERR_ARG;
        }
    for (int i = 0; i < n; ++i)
        if (!pass_ok[i]) {   // (cannot come from the reference: KeyFrame observations are a map MapPoint -> index)
            set_error("problem %d: two edges connect the same keyframe and map point", ids ? ids[i] : i);
            return AOS2_ERR_ARG;
        }
    for (int i = 0; i < n; ++i)
        if (passes[i].np > kLdMaxNp) {   // (k_ldlt_dev's panel and vectors would not fit a CU's LDS: kLdMaxDynLds)
            set_error("problem %d: %d free keyframes, the reduced-system solve takes at most %d", ids ? ids[i] : i, passes[i].np, kLdMaxNp);
            return AOS2_ERR_ARG;
        }
    return AOS2_OK;
}

// The landmark kernels' layout of a call (see aos2_lba_solve_batch) and the block sizes that follow from it
struct LmLayout {
    bool walk;
    int lm_per_block, lin_block;
    int points_blocks(const Pass &S) const { return std::max(1, (S.nl + lm_per_block - 1) / lm_per_block); }   // workgroups of a k_points launch
    int lin_blocks(const Pass &S) const { return (S.nl + lin_block - 1) / lin_block; }                         // landmark workgroups of a k_lin launch
};
// one thread per landmark (k_points_walk: 128 per workgroup, k_lin<true>: 256) or kLmSlots threads per landmark
inline LmLayout lm_layout(bool walk) { return LmLayout{walk, walk ? 128 : kLmBlock, walk ? 256 : kLmBlock}; }

// The staged regions of a window, in arena order: fn(its WinLayout member, the host array it is filled from, the array's bytes,
// bytes of tail).  A region is array + tail long.  The layout and the staging copy both go through this one list.
template <class Layout, class Fn>
inline void for_each_staged(const aos2_lba_problem_t &p, const Pass &S, Layout &l, Fn &&fn)
{
    const size_t NP = p.n_poses, NL = p.n_points, E = p.n_edges;
    fn(l.in_Tcw, p.pose_Tcw, 64 * NP, 0); fn(l.in_xyz, p.point_xyz, 12 * NL, 0); fn(l.in_obs, p.edge_obs, 12 * E, 0); fn(l.in_w, p.edge_inv_sigma2, 4 * E, 0);
    fn(l.e_pose, p.edge_pose, 4 * E, 0); fn(l.e_point, p.edge_point, 4 * E, 0); fn(l.e_stereo, p.edge_stereo, E, 0);
    auto list = [&](auto &off, const std::vector<int32_t> &v, size_t tail) { fn(off, v.data(), 4 * v.size(), tail); };
    list(l.pl_pos, S.pl_pos, 0);   // (one per edge)
    list(l.hpose, S.hpose, 4); list(l.hpoint, S.hpoint, 4);
    list(l.pt_off, S.pt_off, 0); list(l.pt_k, S.pt_k, 4);   // (the offset lists hold nl + 1 or np + 1 entries: never empty)
    list(l.ps_off, S.ps_off, 0); list(l.ps_k, S.ps_k, 4);
    list(l.pl_off, S.pl_off, 0); list(l.pl_k, S.pl_ph, 4);
    list(l.it_ka, S.it_ka, 4); list(l.it_kb, S.it_kb, 4); list(l.it_l, S.it_l, 4);
    list(l.blk_off, S.blk_off, 4);
    list(l.sr_o0, S.sr_o0, 4); list(l.sr_info, S.sr_info, 4); list(l.sr_ij, S.sr_ij, 4);
}

inline void layout_staged(const aos2_lba_problem_t &p, const Pass &S, Bump &B, WinLayout &l)
{
    for_each_staged(p, S, l, [&](size_t &off, const void *, size_t bytes, size_t tail) { off = B.take(bytes + tail); });
    l.n_items = S.it_ka.size();
}

// the window's staged regions into the staging buffer `dst` (which mirrors the arena)
inline void stage_window(uint8_t *dst, const WinLayout &l, const aos2_lba_problem_t &p, const Pass &S)
{
    for_each_staged(p, S, l, [&](size_t off, const void *src, size_t bytes, size_t) {
        if (bytes) memcpy(dst + off, src, bytes);
    });
}

// the device-only regions, and which reduced-system kernel the window takes
inline void layout_scratch(const aos2_lba_problem_t &p, const Pass &S, const LmLayout &lay, Bump &B, WinLayout &l)
{
    const size_t NP = p.n_poses, NL = p.n_points, E = p.n_edges;
    const size_t n6 = 6 * (size_t)S.np, dim = n6 + 3 * (size_t)S.nl;
    l.est = B.take(8 * (7 * NP + 3 * NL)); l.bk = B.take(8 * (7 * NP + 3 * NL));
    l.robust = B.take(E); l.level1 = B.take(E);
    l.err = B.take(24 * E);
    l.lrec = B.take(32 * (S.pl_k.size() + 1)); l.lomr = B.take(24 * (S.pl_k.size() + 1)); l.Rl = B.take(72 * (size_t)S.np + 8);
    l.Hpp = B.take(288 * (size_t)S.np + 8); l.Hll = B.take(72 * (size_t)S.nl + 8);
    l.b = B.take(8 * dim + 8); l.x = B.take(8 * dim + 8);
    l.npad = (int)((n6 + 15) & ~(size_t)15);
    // the register-resident form serves every window of up to 40 free keyframes
    l.ldlt_form = l.npad <= kLrMaxNpad ? kLdltReg : kLdltDev;
    // (both forms take the reduced system padded: k_schur writes it with leading dimension npad, k_ldlt_dev factorises it in place)
    l.Hs = B.take(8 * (size_t)l.npad * l.npad + 8); l.bs = B.take(8 * n6 + 8);
    l.tmp = B.take(8 * n6 + 8);
    l.n_part = lay.points_blocks(S);
    l.scal = B.take(64); l.part = B.take(16 * (size_t)std::max(S.nl, 1) + 8);
    l.erec = B.take(sizeof(EdgeRec) * (E + 1));
}

// the regions that come back in one copy: the window's state, then its results
inline void layout_results(const aos2_lba_problem_t &p, bool want_chi2, Bump &B, WinLayout &l)
{
    const size_t NP = p.n_poses, NL = p.n_points, E = p.n_edges;
    l.st = B.take(sizeof(LmState), 64);
    l.out_Tcw = B.take(64 * NP, 64); l.out_xyz = B.take(12 * NL, 64); l.out_outlier = B.take(E, 64);
    l.out_chi2 = want_chi2 ? B.take(8 * E, 64) : 0;
}

// the device-side view of a window whose regions lie at `base` + l
inline void describe_window(LbaWin &W, uint8_t *base, const aos2_lba_problem_t &p, const Pass &S, const WinLayout &l, const int32_t *abort_word, bool want_chi2)
{
    memset(&W, 0, sizeof(W));
    W.n_poses = p.n_poses; W.n_points = p.n_points; W.n_edges = p.n_edges;
    W.np = S.np; W.nl = S.nl; W.n_items = (int)l.n_items;
    W.iters1 = p.iters_first; W.iters2 = p.iters_second;
    W.in_Tcw = (const float *)(base + l.in_Tcw); W.in_xyz = (const float *)(base + l.in_xyz);
    W.in_obs = (const float *)(base + l.in_obs); W.in_w = (const float *)(base + l.in_w);
    W.pose = (double *)(base + l.est); W.point = W.pose + 7 * (size_t)p.n_poses;
    W.bk = (double *)(base + l.bk);
    W.est_n = 7 * p.n_poses + 3 * p.n_points;
    W.e_pose = (const int32_t *)(base + l.e_pose); W.e_point = (const int32_t *)(base + l.e_point);
    W.e_stereo = base + l.e_stereo; W.e_robust = base + l.robust; W.e_level1 = base + l.level1;
    W.err = (double *)(base + l.err);
    W.cam.fx = (double)p.fx; W.cam.fy = (double)p.fy; W.cam.cx = (double)p.cx; W.cam.cy = (double)p.cy;
    W.cam.bf = (double)p.bf; W.cam.bf_f = p.bf;
    W.cam.delta_mono = (double)(float)std::sqrt(5.991);
    W.cam.delta_stereo = (double)(float)std::sqrt(7.815);
    W.pl_pos = (const int32_t *)(base + l.pl_pos);
    W.hpose = (const int32_t *)(base + l.hpose); W.hpoint = (const int32_t *)(base + l.hpoint);
    W.pt_off = (const int32_t *)(base + l.pt_off); W.pt_k = (const int32_t *)(base + l.pt_k);
    W.ps_off = (const int32_t *)(base + l.ps_off); W.ps_k = (const int32_t *)(base + l.ps_k);
    W.pl_off = (const int32_t *)(base + l.pl_off); W.pl_ph = (const int32_t *)(base + l.pl_k);
    W.it_ka = (const int32_t *)(base + l.it_ka); W.it_kb = (const int32_t *)(base + l.it_kb);
    W.it_l = (const int32_t *)(base + l.it_l); W.blk_off = (const int32_t *)(base + l.blk_off);
    W.sr_o0 = (const int32_t *)(base + l.sr_o0); W.sr_info = (const int32_t *)(base + l.sr_info); W.sr_ij = (const int32_t *)(base + l.sr_ij);
    W.n_srows = (int)S.sr_o0.size();
    W.lrec = (double *)(base + l.lrec); W.lomr = (double *)(base + l.lomr); W.Rl = (double *)(base + l.Rl); W.Hpp = (double *)(base + l.Hpp);
    W.Hll = (double *)(base + l.Hll); W.b = (double *)(base + l.b); W.x = (double *)(base + l.x);
    W.Hs = (double *)(base + l.Hs); W.bs = (double *)(base + l.bs);
    W.tmp = (double *)(base + l.tmp); W.scal = (double *)(base + l.scal); W.part = (double *)(base + l.part);
    W.n_part = l.n_part;
    W.erec = (EdgeRec *)(base + l.erec); W.npad = l.npad; W.ldlt_form = l.ldlt_form;
    W.hs_ld = l.npad;
    W.st = (LmState *)(base + l.st);
    W.abort_word = abort_word;
    W.out_Tcw = (float *)(base + l.out_Tcw); W.out_xyz = (float *)(base + l.out_xyz);
    W.out_outlier = base + l.out_outlier;
    W.out_chi2 = want_chi2 ? (double *)(base + l.out_chi2) : nullptr;
}

// ---- what a launch sequence runs on

// the largest dimensions of a set of windows, and which reduced-system kernels it needs
struct GroupDims {
    bool any_glob = false, any_reg = false;
    int mx_E = 0, mx_pts = 0, mx_npad_glob = 0, mx_npad_reg = 0;
    int walk_lds = 0;   // dynamic LDS of the walks: the largest keyframe state among the windows that stage it (walk_lds_bytes)
    void add(const aos2_lba_problem_t &p, const Pass &S, const WinLayout &l)
    {
        if (S.np > 0) {
            if (l.ldlt_form == kLdltReg) {
                any_reg = true;
                mx_npad_reg = std::max(mx_npad_reg, l.npad);
            } else {
                any_glob = true;
                mx_npad_glob = std::max(mx_npad_glob, l.npad);
            }
        }
        mx_E = std::max(mx_E, p.n_edges);
        mx_pts = std::max(mx_pts, std::max(p.n_points, p.n_poses));
        if (walk_lds_bytes(p.n_poses, S.np) <= kWalkLdsBytes) walk_lds = std::max(walk_lds, walk_lds_bytes(p.n_poses, S.np));
    }
};

struct TaskLists {
    std::vector<SchurTask> schur, pts, lin;
    size_t size() const { return schur.size() + pts.size() + lin.size(); }
};

// The task lists of a set of windows `ids` (indices into passes), addressed by their position in `ids` (by_position: a compacted
// descriptor array) or by ids[position].
// k_schur's list: the units of all windows, window w on XCD w' (workgroups go round-robin to the 8 XCDs in linear-id order,
// each with an L2 of its own -- 4 MB, about one window's working set: the Hpl blocks a window's items share are then served by
// one L2), the windows dealt to the XCDs largest first (every XCD gets about the same number of units), two windows of an XCD
// at a time, unit by unit -- their DIAG units first.  Padding entries (w = -1) keep the 8 queues in step.
// The landmark kernels' lists: block b of every window before block b + 1 of any (the windows advance side by side); k_lin: every
// landmark block first (the long dependent chains of the launch), then one task per free keyframe
inline void build_tasks(const std::vector<Pass> &passes, const std::vector<int> &ids, bool by_position, const LmLayout &lay, TaskLists &T, bool one_queue = false)
{
    auto wmap = [&](int k) { return by_position ? k : ids[k]; };
    std::vector<SchurTask> &tasks = T.schur;
    const int nwg = (int)ids.size();
    std::vector<int> order(nwg);
    std::iota(order.begin(), order.end(), 0);
    // (dealt by unit count.  By estimated cost instead -- a DIAG / BIG unit = 2 + ceil(items / 256) workgroup rounds, a PACK unit one --
    // the mixed 64-window batch took 4.15 / 4.17 / 4.14 ms against 4.14 / 4.13 / 4.12: the XCD queues are not what k_schur's tail waits for)
    auto weight = [&](int k) { return passes[ids[k]].units.size(); };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return weight(a) > weight(b); });
    const int NX = nwg >= 8 && !one_queue ? 8 : 1;
    std::vector<std::vector<int>> xw(NX);
    std::vector<size_t> load(NX, 0);
    for (int k : order) {
        const int x = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        xw[x].push_back(k);
        load[x] += weight(k);
    }
    std::vector<std::vector<SchurTask>> qx(NX);
    for (int x = 0; x < NX; ++x)
        for (size_t k = 0; k < xw[x].size(); k += 2) {
            const int a = xw[x][k], b = k + 1 < xw[x].size() ? xw[x][k + 1] : -1;
            const std::vector<int32_t> &ua = passes[ids[a]].units;
            static const std::vector<int32_t> none;
            const std::vector<int32_t> &ub = b >= 0 ? passes[ids[b]].units : none;
            for (size_t u = 0; u < std::max(ua.size(), ub.size()); ++u) {
                if (u < ua.size()) qx[x].push_back(SchurTask{wmap(a), ua[u]});
                if (u < ub.size()) qx[x].push_back(SchurTask{wmap(b), ub[u]});
            }
        }
    size_t mxq = 0;
    for (auto &q_ : qx) mxq = std::max(mxq, q_.size());
    tasks.assign(mxq * NX, SchurTask{-1, 0});
    for (int x = 0; x < NX; ++x)
        for (size_t k = 0; k < qx[x].size(); ++k) tasks[k * NX + x] = qx[x][k];
    int mx_pb = 0, mx_lb = 0, mx_k = 0;
    std::vector<int> npb(nwg), nlb(nwg);
    for (int k = 0; k < nwg; ++k) {
        const Pass &S = passes[ids[k]];
        npb[k] = lay.points_blocks(S);   // = WinLayout::n_part
        nlb[k] = lay.lin_blocks(S);
        mx_pb = std::max(mx_pb, npb[k]); mx_lb = std::max(mx_lb, nlb[k]); mx_k = std::max(mx_k, S.np);
    }
    T.pts.clear();
    T.lin.clear();
    for (int b = 0; b < mx_pb; ++b)
        for (int k = 0; k < nwg; ++k)
            if (b < npb[k]) T.pts.push_back(SchurTask{wmap(k), b});
    for (int b = 0; b < mx_lb; ++b)
        for (int k = 0; k < nwg; ++k)
            if (b < nlb[k]) T.lin.push_back(SchurTask{wmap(k), b});
    for (int kf = 0; kf < mx_k; ++kf)
        for (int k = 0; k < nwg; ++k)
            if (kf < passes[ids[k]].np) T.lin.push_back(SchurTask{wmap(k), (1 << 28) | kf});
}

// the device addresses of a TaskLists
struct DevTasks {
    const SchurTask *schur, *pts, *lin;
};
// Writes the three lists of T behind each other at byte offset `o` of the staging buffer `host`, which mirrors the device memory
// at `dev`; `o` moves on to the end of what was written
inline DevTasks put_tasks(const TaskLists &T, uint8_t *host, const uint8_t *dev, size_t &o)
{
    DevTasks d;
    const std::vector<SchurTask> *lists[3] = {&T.schur, &T.pts, &T.lin};
    const SchurTask **where[3] = {&d.schur, &d.pts, &d.lin};
    for (int k = 0; k < 3; ++k) {
        *where[k] = (const SchurTask *)(dev + o);
        if (!lists[k]->empty()) memcpy(host + o, lists[k]->data(), sizeof(SchurTask) * lists[k]->size());
        o += sizeof(SchurTask) * lists[k]->size();
    }
    return d;
}

// The arena of a call: [staged regions of all windows | task lists of the groups | descriptors] (the part that is uploaded)
// [continuation region][device-only regions of all windows][states and results of all windows] (the part that comes back)
struct ArenaPlan {
    std::vector<WinLayout> L;
    size_t o_tasks, o_wins, staged_bytes, o_cont, cont_bytes, o_res, res_bytes, bytes;
};
inline void plan_arena(const aos2_lba_problem_t *problems, const std::vector<int> &act, const std::vector<Pass> &passes, const LmLayout &lay, size_t n_all_tasks,
                       bool want_chi2, ArenaPlan &A)
{
    const int nw = (int)act.size();
    A.L.resize(nw);
    Bump B;
    for (int i = 0; i < nw; ++i) layout_staged(problems[act[i]], passes[i], B, A.L[i]);
    A.o_tasks = B.take(sizeof(SchurTask) * n_all_tasks + 8);
    A.o_wins = B.take(sizeof(LbaWin) * (size_t)nw);
    A.staged_bytes = B.size;
    // (a continuation round runs on the windows that are not finished, compacted: their descriptors and task lists go here)
    // Sized for ANY subset of the windows, not for the first round's lists: a subset is dealt to the 8 queues anew (largest first; with
    // queues of about equal length the padded list holds about sum + 8 x max units -- a first round of fewer than 8 windows per group
    // is not padded at all, and the dealing is not monotone on subsets); the landmark / linearisation lists of a subset are parts of
    // the full ones.  A subset whose padded list is longer still falls back to one unpadded queue (continuation_tasks), which always fits.
    size_t cont_tasks = 0, cont_max_units = 0;
    for (int i = 0; i < nw; ++i) {
        const Pass &S = passes[i];
        cont_max_units = std::max(cont_max_units, S.units.size());
        cont_tasks += S.units.size() + (size_t)lay.points_blocks(S) + (size_t)lay.lin_blocks(S) + (size_t)S.np;
    }
    cont_tasks += 8 * cont_max_units;
    A.cont_bytes = sizeof(LbaWin) * (size_t)nw + sizeof(SchurTask) * std::max(cont_tasks, n_all_tasks) + 64;
    A.o_cont = B.take(A.cont_bytes);
    for (int i = 0; i < nw; ++i) layout_scratch(problems[act[i]], passes[i], lay, B, A.L[i]);
    A.o_res = B.take(0);
    for (int i = 0; i < nw; ++i) layout_results(problems[act[i]], want_chi2, B, A.L[i]);
    A.res_bytes = B.size - A.o_res;
    A.bytes = B.size;
}

// The task lists of a continuation round over the windows `todo` (positions in passes), which address the compacted descriptors by
// position: dealt to the queues like a first round's, or -- should that pad past the continuation region (the dealing is not monotone
// on subsets), or with force_one_queue -- as one unpadded queue, whose length is the subset's sum and always fits.  False: the
// descriptors and the lists do not fit A.cont_bytes.
inline bool continuation_tasks(const std::vector<Pass> &passes, const std::vector<int> &todo, const LmLayout &lay, const ArenaPlan &A, bool force_one_queue, TaskLists &TC)
{
    auto bytes = [&] { return sizeof(LbaWin) * todo.size() + sizeof(SchurTask) * TC.size(); };
    build_tasks(passes, todo, true, lay, TC);
    if (force_one_queue || bytes() > A.cont_bytes) build_tasks(passes, todo, true, lay, TC, true);
    return bytes() <= A.cont_bytes;
}

}  // namespace aos2
