// The host plan of LocalBA (csrc/lba_plan.h) stand-alone on the CPU: tests/test_lba_plan_cpu.py builds this with
// -fsanitize=address,undefined and runs it.  For every window set: build_structures -> build_tasks -> plan_arena, heap buffers of
// EXACTLY ArenaPlan::staged_bytes and ::bytes (an overrun of either is the sanitizer's to find), stage_window / put_tasks /
// describe_window into them, then the LbaWin is walked through its own pointers, the way the kernels index it, and what the
// comments of lba_plan.h and lba_window.h promise is asserted.  Windows come from a fixed LCG.  Prints "ok".
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <string>
#include <utility>

#include "../../active-orb-slam2_amd/csrc/lba_plan.h"

static std::string g_error;
namespace aos2 {
void set_error(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}
}  // namespace aos2
using namespace aos2;

static const char *g_what = "";
[[noreturn]] __attribute__((noinline, cold)) static void failed(int line, const char *what)
{
    fprintf(stderr, "%s:%d: [%s] %s\n", __FILE__, line, g_what, what);
    exit(1);
}
#define CHECK(c)                         \
    do {                                 \
        if (!(c)) failed(__LINE__, #c);  \
    } while (0)

static uint32_t g_lcg = 12345u;
static uint32_t lcg() { return g_lcg = g_lcg * 1664525u + 1013904223u; }
static float lcg_float() { return (float)(lcg() >> 8) / (float)(1 << 24); }

// ---- a window: its arrays and the problem that points at them
struct Win {
    std::string name;
    std::vector<float> Tcw, xyz, obs, w;
    std::vector<uint8_t> fixed, stereo;
    std::vector<int64_t> pose_id, point_id;
    std::vector<int32_t> e_pose, e_point;
    int add_pose(bool fix, int64_t id)
    {
        fixed.push_back(fix ? 1 : 0);
        pose_id.push_back(id);
        for (int k = 0; k < 16; ++k) Tcw.push_back(lcg_float());
        return (int)fixed.size() - 1;
    }
    int add_point(int64_t id)
    {
        point_id.push_back(id);
        for (int k = 0; k < 3; ++k) xyz.push_back(lcg_float());
        return (int)point_id.size() - 1;
    }
    void add_edge(int pose, int point)
    {
        e_pose.push_back(pose);
        e_point.push_back(point);
        for (int k = 0; k < 3; ++k) obs.push_back(lcg_float());
        w.push_back(lcg_float());
        stereo.push_back(lcg() >> 31);
    }
    // a point with an edge to each of the given poses
    void add_seen_point(std::initializer_list<int> poses)
    {
        const int l = add_point((int64_t)point_id.size());
        for (int p : poses) add_edge(p, l);
    }
    aos2_lba_problem_t problem() const
    {
        aos2_lba_problem_t p{};
        p.n_poses = (int32_t)fixed.size(); p.n_points = (int32_t)point_id.size(); p.n_edges = (int32_t)e_pose.size();
        p.pose_Tcw = Tcw.data(); p.pose_fixed = fixed.data(); p.pose_id = pose_id.data();
        p.point_xyz = xyz.data(); p.point_id = point_id.data();
        p.edge_pose = e_pose.data(); p.edge_point = e_point.data(); p.edge_obs = obs.data(); p.edge_stereo = stereo.data();
        p.edge_inv_sigma2 = w.data();
        p.fx = 500.f; p.fy = 501.f; p.cx = 320.f; p.cy = 240.f; p.bf = 40.f;
        p.stop_flag = nullptr;
        p.iters_first = 5; p.iters_second = 10;
        return p;
    }
};

// (a) 1 free + 1 fixed keyframe, 1 point, 2 edges: np = 1, no off-diagonal block
static Win win_a()
{
    Win W; W.name = "a";
    W.add_pose(false, 1); W.add_pose(true, 0);
    W.add_seen_point({0, 1});
    return W;
}
// (b) 2 free keyframes sharing 1 point: one block, one item, one PACK row
static Win win_b()
{
    Win W; W.name = "b";
    W.add_pose(false, 0); W.add_pose(false, 1);
    W.add_seen_point({0, 1});
    return W;
}
// (c) an edgeless keyframe and an edgeless point among active ones, ids descending: the sort path
static Win win_c()
{
    Win W; W.name = "c";
    for (int i = 0; i < 4; ++i) W.add_pose(i == 3, 40 - i);   // pose 1 stays edgeless, pose 3 is fixed
    for (int l = 0; l < 4; ++l) W.add_point(90 - l);           // point 2 stays edgeless
    W.add_edge(2, 3); W.add_edge(0, 3); W.add_edge(3, 0); W.add_edge(2, 0); W.add_edge(0, 1); W.add_edge(3, 3); W.add_edge(2, 1);
    return W;
}
// (d) a point seen only by fixed keyframes
static Win win_d()
{
    Win W; W.name = "d";
    W.add_pose(false, 0); W.add_pose(true, 1); W.add_pose(true, 2);
    W.add_seen_point({0, 1});
    W.add_seen_point({1, 2});
    return W;
}
// (e) 2 free keyframes sharing n points: 17 = 2 rows, 256 = a full 16-row unit, 257 = BIG
static Win win_e(int n)
{
    Win W; W.name = "e" + std::to_string(n);
    W.add_pose(false, 0); W.add_pose(false, 1);
    for (int l = 0; l < n; ++l) W.add_seen_point({l & 1, 1 - (l & 1)});
    return W;
}
// (f) 7 free keyframes; off-diagonal block b of the 21 takes 1 + b % 9 rows, block 5 is empty (it keeps one row): the rows
// are 1 2 3 4 5 1 | 7 8 (9 does not fit: padded) | 9 1 2 3 | 4 5 6 | 7 8 | 9 1 2 3
static Win win_f()
{
    Win W; W.name = "f";
    for (int i = 0; i < 7; ++i) W.add_pose(false, i);
    int b = 0;
    for (int i1 = 0; i1 < 7; ++i1)
        for (int i2 = i1 + 1; i2 < 7; ++i2, ++b) {
            const int rows = 1 + b % 9, n = b == 5 ? 0 : 16 * (rows - 1) + 1 + (7 * b) % 16;
            for (int k = 0; k < n; ++k) W.add_seen_point({i2, i1});
        }
    return W;
}
// (g) all keyframes fixed: np = 0
static Win win_g()
{
    Win W; W.name = "g";
    W.add_pose(true, 0); W.add_pose(true, 1);
    W.add_seen_point({0, 1});
    W.add_seen_point({1});
    return W;
}
// (h) a star: one point seen by n free keyframes (40: register form, 41: device-memory form, 155: refused), one more each
static Win win_h(int n)
{
    Win W; W.name = "h" + std::to_string(n);
    for (int i = 0; i < n; ++i) W.add_pose(false, i);
    const int l = W.add_point(0);
    for (int i = 0; i < n; ++i) W.add_edge(i, l);
    W.add_seen_point({0});
    return W;
}

// ---- the checks

struct Region {
    const uint8_t *p;
    size_t bytes;
    bool result;
};

// the index structures of a window, read through the descriptor's pointers as the kernels read them
static void check_window(const LbaWin &W, const aos2_lba_problem_t &p, const Pass &S, const LmLayout &lay)
{
    const int E = p.n_edges, np = W.np, nl = W.nl;
    CHECK(W.n_poses == p.n_poses && W.n_points == p.n_points && W.n_edges == E && np == S.np && nl == S.nl);
    // hidx -> vertex: the free keyframes / the points that have an edge, by id
    std::vector<int> pose_h(p.n_poses, -1), point_h(p.n_points, -1);
    std::vector<int> pose_deg(p.n_poses, 0), point_deg(p.n_points, 0);
    for (int k = 0; k < E; ++k) {
        CHECK(W.e_pose[k] == p.edge_pose[k] && W.e_point[k] == p.edge_point[k]);
        pose_deg[p.edge_pose[k]]++;
        point_deg[p.edge_point[k]]++;
    }
    int want_np = 0, want_nl = 0;
    for (int i = 0; i < p.n_poses; ++i) want_np += pose_deg[i] > 0 && !p.pose_fixed[i];
    for (int i = 0; i < p.n_points; ++i) want_nl += point_deg[i] > 0;
    CHECK(np == want_np && nl == want_nl);
    for (int i = 0; i < np; ++i) {
        const int v = W.hpose[i];
        CHECK(v >= 0 && v < p.n_poses && pose_h[v] < 0 && pose_deg[v] > 0 && !p.pose_fixed[v]);
        CHECK(i == 0 || p.pose_id[W.hpose[i - 1]] < p.pose_id[v]);
        pose_h[v] = i;
    }
    for (int i = 0; i < nl; ++i) {
        const int v = W.hpoint[i];
        CHECK(v >= 0 && v < p.n_points && point_h[v] < 0 && point_deg[v] > 0);
        CHECK(i == 0 || p.point_id[W.hpoint[i - 1]] < p.point_id[v]);
        point_h[v] = i;
    }
    // pt_k: a permutation of the edges grouped by hpoint, insertion order inside a landmark
    CHECK(W.pt_off[0] == 0 && W.pt_off[nl] == E);
    std::vector<uint8_t> seen(E, 0);
    for (int l = 0; l < nl; ++l) {
        CHECK(W.pt_off[l] <= W.pt_off[l + 1]);
        for (int a = W.pt_off[l]; a < W.pt_off[l + 1]; ++a) {
            const int k = W.pt_k[a];
            CHECK(k >= 0 && k < E && !seen[k] && W.e_point[k] == W.hpoint[l]);
            CHECK(a == W.pt_off[l] || W.pt_k[a - 1] < k);
            seen[k] = 1;
        }
    }
    // ps_k: the free-pose edges by hpose
    int n_free = 0;
    for (int k = 0; k < E; ++k) n_free += pose_h[p.edge_pose[k]] >= 0;
    CHECK(W.ps_off[0] == 0 && W.ps_off[np] == n_free);
    std::fill(seen.begin(), seen.end(), 0);
    for (int i = 0; i < np; ++i) {
        CHECK(W.ps_off[i] <= W.ps_off[i + 1]);
        for (int a = W.ps_off[i]; a < W.ps_off[i + 1]; ++a) {
            const int k = W.ps_k[a];
            CHECK(k >= 0 && k < E && !seen[k] && W.e_pose[k] == W.hpose[i]);
            seen[k] = 1;
        }
    }
    // the pl list: pl_pos is its inverse; inside a landmark the pose hidx ascends strictly
    const int n_pl = W.pl_off[nl];
    CHECK(W.pl_off[0] == 0 && n_pl == n_free && (int)S.pl_k.size() == n_pl);
    std::vector<int> pl_edge(n_pl, -1);
    for (int k = 0; k < E; ++k) {
        const int a = W.pl_pos[k];
        if (pose_h[p.edge_pose[k]] < 0) {
            CHECK(a == -1);
            continue;
        }
        CHECK(a >= 0 && a < n_pl && pl_edge[a] < 0);
        pl_edge[a] = k;
    }
    size_t want_items = 0;
    for (int l = 0; l < nl; ++l) {
        const int a0 = W.pl_off[l], a1 = W.pl_off[l + 1];
        CHECK(a0 <= a1);
        want_items += (size_t)(a1 - a0) * (size_t)(a1 - a0 + 1) / 2;
        for (int a = a0; a < a1; ++a) {
            CHECK(S.pl_k[a] == pl_edge[a] && W.e_point[pl_edge[a]] == W.hpoint[l]);
            CHECK(W.pl_ph[a] >= 0 && W.pl_ph[a] < np && W.hpose[W.pl_ph[a]] == W.e_pose[pl_edge[a]]);
            CHECK(a == a0 || W.pl_ph[a - 1] < W.pl_ph[a]);
        }
    }
    // the landmark kernels' blocks cover the landmarks
    CHECK(W.n_part == lay.points_blocks(S) && W.n_part >= 1 && (long)W.n_part * lay.lm_per_block >= nl && (long)lay.lin_blocks(S) * lay.lin_block >= nl);
    CHECK(W.npad % 16 == 0 && W.npad >= 6 * np && W.npad < 6 * np + 16 && W.hs_ld == W.npad);
    CHECK(W.ldlt_form == (np <= 40 ? kLdltReg : kLdltDev));
    if (np == 0) return;   // (no Schur items, no units: build_structures leaves the lists of an earlier call)
    // Schur items: ranked by block (upper triangle, row-major), landmarks ascending inside a block
    const int nblk = np * (np + 1) / 2;
    CHECK((size_t)W.n_items == want_items && W.blk_off[0] == 0 && W.blk_off[nblk] == W.n_items);
    for (int i1 = 0, blk = 0; i1 < np; ++i1)
        for (int i2 = i1; i2 < np; ++i2, ++blk) {
            CHECK(blk == i1 * np - i1 * (i1 - 1) / 2 + (i2 - i1));   // (k_schur's rank of a block)
            CHECK(W.blk_off[blk] <= W.blk_off[blk + 1]);
            for (int o = W.blk_off[blk]; o < W.blk_off[blk + 1]; ++o) {
                const int ka = W.it_ka[o], kb = W.it_kb[o], l = W.it_l[o];
                CHECK(l >= 0 && l < nl && ka >= W.pl_off[l] && ka <= kb && kb < W.pl_off[l + 1]);
                CHECK(W.pl_ph[ka] == i1 && W.pl_ph[kb] == i2);
                CHECK(o == W.blk_off[blk] || W.it_l[o - 1] < l);
            }
        }
    // Schur units: a DIAG per free keyframe; every off-diagonal block once -- a BIG unit, or consecutive rows of one PACK unit
    std::vector<int> diag(np, 0), covered(nblk, 0);
    std::vector<int> packs;
    for (int32_t code : S.units) {
        const int kind = code >> 28, arg = code & 0x0fffffff;
        if (kind == kSchurDiag) {
            CHECK(arg < np && packs.empty());
            diag[arg]++;
        } else if (kind == kSchurBig) {
            CHECK(arg < nblk && packs.empty());
            int rem = arg, i1 = 0;   // (the kernel's decoding of the rank)
            while (rem >= np - i1) {
                rem -= np - i1;
                ++i1;
            }
            CHECK(rem > 0 && W.blk_off[arg + 1] - W.blk_off[arg] > 256);
            covered[arg]++;
        } else {
            CHECK(kind == kSchurPack && arg % 16 == 0 && arg == 16 * (int)packs.size() && arg < W.n_srows);
            packs.push_back(arg);
        }
    }
    for (int i = 0; i < np; ++i) CHECK(diag[i] == 1);
    CHECK((int)packs.size() == (W.n_srows + 15) / 16 && (int)S.sr_o0.size() == W.n_srows);
    for (int r = 0; r < W.n_srows;) {
        const int info = W.sr_info[r];
        if (info == 0) {   // padding: to the end of the unit
            CHECK(r % 16 != 0 && W.sr_o0[r] == 0 && W.sr_ij[r] == 0);
            ++r;
            CHECK(r % 16 == 0 || (r < W.n_srows && W.sr_info[r] == 0));
            continue;
        }
        const int nrows = info >> 16, i1 = W.sr_ij[r] & 0xffff, i2 = W.sr_ij[r] >> 16;
        CHECK(i1 < i2 && i2 < np);
        const int blk = i1 * np - i1 * (i1 - 1) / 2 + (i2 - i1), o0 = W.blk_off[blk], n = W.blk_off[blk + 1] - o0;
        CHECK(n <= 256 && nrows == std::max(1, (n + 15) / 16) && r % 16 + nrows <= 16 && r + nrows <= W.n_srows);
        for (int k = 0; k < nrows; ++k) {
            CHECK(W.sr_info[r + k] == (std::max(0, std::min(16, n - 16 * k)) | (k << 8) | (nrows << 16)));
            CHECK(W.sr_o0[r + k] == o0 + 16 * k && W.sr_ij[r + k] == W.sr_ij[r]);
        }
        covered[blk]++;
        r += nrows;
    }
    for (int i1 = 0, blk = 0; i1 < np; ++i1)
        for (int i2 = i1; i2 < np; ++i2, ++blk) CHECK(covered[blk] == (i1 == i2 ? 0 : 1));
}

// The regions a window's descriptor points to: array + tail as lba_plan.h lays them out (for_each_staged, layout_scratch,
// layout_results), restated here from the window's dimensions
static void window_regions(const LbaWin &W, const Pass &S, bool want_chi2, std::vector<Region> &staged, std::vector<Region> &rest)
{
    const size_t NP = W.n_poses, NL = W.n_points, E = W.n_edges, np = W.np, nl = W.nl, n_pl = S.pl_k.size(), n6 = 6 * np;
    const size_t items = S.it_ka.size(), nboff = S.blk_off.size(), rows = S.sr_o0.size(), npad = W.npad;
    auto st = [&](const void *q, size_t bytes) { staged.push_back(Region{(const uint8_t *)q, bytes, false}); };
    auto sc = [&](const void *q, size_t bytes) { rest.push_back(Region{(const uint8_t *)q, bytes, false}); };
    auto rs = [&](const void *q, size_t bytes) { rest.push_back(Region{(const uint8_t *)q, bytes, true}); };
    st(W.in_Tcw, 64 * NP); st(W.in_xyz, 12 * NL); st(W.in_obs, 12 * E); st(W.in_w, 4 * E);
    st(W.e_pose, 4 * E); st(W.e_point, 4 * E); st(W.e_stereo, E); st(W.pl_pos, 4 * E);
    st(W.hpose, 4 * np + 4); st(W.hpoint, 4 * nl + 4);
    st(W.pt_off, 4 * (nl + 1)); st(W.pt_k, 4 * E + 4); st(W.ps_off, 4 * (np + 1)); st(W.ps_k, 4 * n_pl + 4);
    st(W.pl_off, 4 * (nl + 1)); st(W.pl_ph, 4 * n_pl + 4);
    st(W.it_ka, 4 * items + 4); st(W.it_kb, 4 * items + 4); st(W.it_l, 4 * items + 4); st(W.blk_off, 4 * nboff + 4);
    st(W.sr_o0, 4 * rows + 4); st(W.sr_info, 4 * rows + 4); st(W.sr_ij, 4 * rows + 4);
    CHECK(W.point == W.pose + 7 * NP && W.est_n == (int)(7 * NP + 3 * NL));
    sc(W.pose, 8 * (7 * NP + 3 * NL)); sc(W.bk, 8 * (7 * NP + 3 * NL));
    sc(W.e_robust, E); sc(W.e_level1, E); sc(W.err, 24 * E);
    sc(W.lrec, 32 * (n_pl + 1)); sc(W.lomr, 24 * (n_pl + 1)); sc(W.Rl, 72 * np + 8);
    sc(W.Hpp, 288 * np + 8); sc(W.Hll, 72 * nl + 8); sc(W.b, 8 * (n6 + 3 * nl) + 8); sc(W.x, 8 * (n6 + 3 * nl) + 8);
    sc(W.Hs, 8 * npad * npad + 8); sc(W.bs, 8 * n6 + 8); sc(W.tmp, 8 * n6 + 8);
    sc(W.scal, 64); sc(W.part, 16 * std::max(nl, (size_t)1) + 8); sc(W.erec, sizeof(EdgeRec) * (E + 1));
    rs(W.st, sizeof(LmState)); rs(W.out_Tcw, 64 * NP); rs(W.out_xyz, 12 * NL); rs(W.out_outlier, E);
    if (want_chi2)
        rs(W.out_chi2, 8 * E);
    else
        CHECK(W.out_chi2 == nullptr);
}

// The three task lists over the windows pass_of[0 .. n): w is w0 + the position in pass_of.  k_schur's list: dealt to the eight
// queues (8 or more windows: the length is a multiple of 8), one unpadded queue, or -- a continuation round, which falls back
// to one queue when the dealt list does not fit -- either
enum Queues { kDealt, kOneQueue, kEither };
static void check_tasks(const SchurTask *schur, size_t n_schur, const SchurTask *pts, size_t n_pts, const SchurTask *lin, size_t n_lin,
                        const std::vector<Pass> &passes, const std::vector<int> &pass_of, int w0, const LmLayout &lay, Queues queues)
{
    const int n = (int)pass_of.size();
    // pts: every (window, block < n_part) once, block-major
    std::set<std::pair<int, int>> got;
    size_t want = 0;
    for (int k = 0; k < n; ++k) want += lay.points_blocks(passes[pass_of[k]]);
    CHECK(n_pts == want);
    for (size_t t = 0; t < n_pts; ++t) {
        const int k = pts[t].w - w0;
        CHECK(k >= 0 && k < n && pts[t].code >= 0 && pts[t].code < lay.points_blocks(passes[pass_of[k]]));
        CHECK(got.insert({k, pts[t].code}).second && (t == 0 || pts[t - 1].code <= pts[t].code));
    }
    // lin: every landmark block, then every free keyframe, once
    got.clear();
    want = 0;
    size_t want_kf = 0;
    for (int k = 0; k < n; ++k) {
        want += lay.lin_blocks(passes[pass_of[k]]);
        want_kf += passes[pass_of[k]].np;
    }
    CHECK(n_lin == want + want_kf);
    for (size_t t = 0; t < n_lin; ++t) {
        const int k = lin[t].w - w0, kind = lin[t].code >> 28, blk = lin[t].code & 0x0fffffff;
        CHECK(k >= 0 && k < n && kind == (t < want ? 0 : 1));
        CHECK(blk < (kind ? passes[pass_of[k]].np : lay.lin_blocks(passes[pass_of[k]])) && got.insert({k, lin[t].code}).second);
    }
    // schur: every unit of every window once, and padding
    got.clear();
    want = 0;
    for (int k = 0; k < n; ++k) want += passes[pass_of[k]].units.size();
    size_t real = 0;
    for (size_t t = 0; t < n_schur; ++t) {
        if (schur[t].w == -1) {
            CHECK(queues != kOneQueue && n >= 8);
            continue;
        }
        const int k = schur[t].w - w0;
        CHECK(k >= 0 && k < n);
        const std::vector<int32_t> &u = passes[pass_of[k]].units;
        CHECK(std::find(u.begin(), u.end(), schur[t].code) != u.end() && got.insert({k, schur[t].code}).second);
        ++real;
    }
    const bool dealt = n_schur % 8 == 0 && n_schur >= want;   // eight queues, padded to the longest
    CHECK(real == want && (queues == kDealt && n >= 8 ? dealt : queues == kEither && n >= 8 ? dealt || n_schur == want : n_schur == want));
}

// one call: the windows wins[...] as G groups, under one landmark layout; `subsets`: continuation rounds to try
static void check_call(const std::vector<const Win *> &wins, bool walk, int G, bool want_chi2, int threads, const std::vector<std::vector<int>> &subsets)
{
    const int nw = (int)wins.size();
    const LmLayout lay = lm_layout(walk);
    CHECK(lay.walk == walk && lay.lm_per_block == (walk ? 128 : kLmBlock) && lay.lin_block == (walk ? 256 : kLmBlock));
    std::vector<aos2_lba_problem_t> problems;
    for (const Win *w : wins) problems.push_back(w->problem());
    std::vector<int> act(nw);
    std::iota(act.begin(), act.end(), 0);
    std::vector<Pass> passes(nw);
    WindowPool pool;
    if (threads > 1) pool.start(threads);
    CHECK(build_structures(pool, problems.data(), act.data(), nw, passes) == AOS2_OK);
    const int goff[3] = {0, G == 2 ? nw / 2 : nw, nw};
    TaskLists TL[2];
    size_t n_all_tasks = 0;
    for (int g = 0; g < G; ++g) {
        std::vector<int> ids(goff[g + 1] - goff[g]);
        std::iota(ids.begin(), ids.end(), goff[g]);
        build_tasks(passes, ids, false, lay, TL[g]);
        n_all_tasks += TL[g].size();
    }
    ArenaPlan A;
    plan_arena(problems.data(), act, passes, lay, n_all_tasks, want_chi2, A);
    CHECK(A.staged_bytes <= A.o_cont && A.o_cont + A.cont_bytes <= A.o_res && A.o_res + A.res_bytes == A.bytes);
    CHECK(A.o_tasks + sizeof(SchurTask) * n_all_tasks <= A.o_wins && A.o_wins + sizeof(LbaWin) * nw == A.staged_bytes);
    // the staging buffer and the arena, exactly as long as the plan says
    std::unique_ptr<uint8_t[]> hin(new uint8_t[A.staged_bytes]), arena(new uint8_t[A.bytes]);
    uint8_t *base = arena.get();
    pool.run(nw, [&](int i) { stage_window(hin.get(), A.L[i], problems[i], passes[i]); });
    DevTasks dt[2];
    size_t o = A.o_tasks;
    for (int g = 0; g < G; ++g) dt[g] = put_tasks(TL[g], hin.get(), base, o);
    CHECK(o == A.o_tasks + sizeof(SchurTask) * n_all_tasks);
    LbaWin *hw = reinterpret_cast<LbaWin *>(hin.get() + A.o_wins);
    static const int32_t abort_words[16] = {};
    GroupDims gd[2];
    for (int i = 0; i < nw; ++i) {
        describe_window(hw[i], base, problems[i], passes[i], A.L[i], abort_words + i, want_chi2);
        gd[i >= goff[1] ? 1 : 0].add(problems[i], passes[i], A.L[i]);
    }
    memcpy(base, hin.get(), A.staged_bytes);   // the upload
    const LbaWin *dw = reinterpret_cast<const LbaWin *>(base + A.o_wins);
    // ---- regions: inside the buffer, disjoint, the staged ones inside the window's uploaded range, the results in [o_res, bytes)
    std::vector<Region> all;
    all.push_back(Region{base + A.o_tasks, sizeof(SchurTask) * n_all_tasks + 8, false});
    all.push_back(Region{base + A.o_wins, sizeof(LbaWin) * (size_t)nw, false});
    all.push_back(Region{base + A.o_cont, A.cont_bytes, false});
    for (int i = 0; i < nw; ++i) {
        std::vector<Region> staged, rest;
        window_regions(dw[i], passes[i], want_chi2, staged, rest);
        const size_t r0 = A.L[i].in_Tcw, r1 = i + 1 < nw ? A.L[i + 1].in_Tcw : A.o_tasks;   // (what stage_and_upload sends for the window)
        for (const Region &r : staged) CHECK(r.p >= base + r0 && r.p + r.bytes <= base + r1);
        for (const Region &r : rest) {
            if (r.result)
                CHECK(r.p >= base + A.o_res && r.p + r.bytes <= base + A.bytes);
            else
                CHECK(r.p >= base + A.o_cont + A.cont_bytes && r.p + r.bytes <= base + A.o_res);
        }
        all.insert(all.end(), staged.begin(), staged.end());
        all.insert(all.end(), rest.begin(), rest.end());
        CHECK(dw[i].abort_word == abort_words + i && dw[i].iters1 == 5 && dw[i].iters2 == 10 && dw[i].cam.bf_f == 40.f);
        CHECK((const uint8_t *)dw[i].st == base + A.L[i].st);
    }
    std::sort(all.begin(), all.end(), [](const Region &a, const Region &b) { return a.p < b.p; });
    for (size_t k = 0; k < all.size(); ++k) {
        CHECK(all[k].p >= base && all[k].p + all[k].bytes <= base + A.bytes);
        CHECK(k == 0 || all[k - 1].p + all[k - 1].bytes <= all[k].p);
    }
    // ---- the windows' structures, the groups' task lists as the kernels find them
    for (int i = 0; i < nw; ++i) {
        check_window(dw[i], problems[i], passes[i], lay);
        const uint8_t *h = hin.get();
        CHECK(!memcmp(h + A.L[i].in_Tcw, problems[i].pose_Tcw, 64 * (size_t)problems[i].n_poses));
        CHECK(!memcmp(dw[i].in_obs, problems[i].edge_obs, 12 * (size_t)problems[i].n_edges));
    }
    for (int g = 0; g < G; ++g) {
        std::vector<int> ids(goff[g + 1] - goff[g]);
        std::iota(ids.begin(), ids.end(), goff[g]);
        CHECK((const uint8_t *)dt[g].schur >= base + A.o_tasks && (const uint8_t *)(dt[g].lin + TL[g].lin.size()) <= base + A.o_wins);
        check_tasks(dt[g].schur, TL[g].schur.size(), dt[g].pts, TL[g].pts.size(), dt[g].lin, TL[g].lin.size(), passes, ids, goff[g], lay, kDealt);
        CHECK(gd[g].walk_lds <= kWalkLdsBytes && gd[g].mx_npad_reg <= kLrMaxNpad && gd[g].mx_npad_glob <= kLdMaxNpad);
    }
    // ---- continuation rounds: any subset's descriptors and lists fit the continuation region, as dealt or as one queue
    for (const std::vector<int> &todo : subsets)
        for (int force = 0; force < 2; ++force) {
            TaskLists TC;
            CHECK(continuation_tasks(passes, todo, lay, A, force != 0, TC));
            std::unique_ptr<uint8_t[]> hc(new uint8_t[A.cont_bytes]);
            for (size_t k = 0; k < todo.size(); ++k) reinterpret_cast<LbaWin *>(hc.get())[k] = hw[todo[k]];
            size_t oc = sizeof(LbaWin) * todo.size();
            const DevTasks dc = put_tasks(TC, hc.get(), hc.get(), oc);
            CHECK(oc <= A.cont_bytes);
            check_tasks(dc.schur, TC.schur.size(), dc.pts, TC.pts.size(), dc.lin, TC.lin.size(), passes, todo, 0, lay, force ? kOneQueue : kEither);
        }
}

static void check_refused(const Win &W, const char *message)
{
    g_what = message;
    const aos2_lba_problem_t p = W.problem();
    std::vector<Pass> passes(1);
    WindowPool pool;
    g_error.clear();
    CHECK(build_structures(pool, &p, nullptr, 1, passes) == AOS2_ERR_ARG);
    CHECK(g_error == message);
}

enum { kA, kB, kC, kD, kE17, kE256, kE257, kF, kG, kH40, kH41, kWindows };

// what the cases are for, asserted on their structures
static void check_cases(const std::vector<Win> &W)
{
    g_what = "cases";
    std::vector<Pass> one(1);
    const Pass &S = one[0];
    auto pass_of = [&](int w) {
        const aos2_lba_problem_t p = W[w].problem();
        WindowPool pool;
        CHECK(build_structures(pool, &p, nullptr, 1, one) == AOS2_OK);
    };
    auto kinds = [&](int kind) { return (int)std::count_if(S.units.begin(), S.units.end(), [&](int32_t u) { return u >> 28 == kind; }); };
    pass_of(kA);
    CHECK(S.np == 1 && S.nl == 1 && S.units.size() == 1 && S.sr_o0.empty());
    pass_of(kB);
    CHECK(S.np == 2 && S.it_ka.size() == 3 && S.sr_o0.size() == 1 && kinds(kSchurPack) == 1);
    pass_of(kC);
    CHECK(S.np == 2 && S.nl == 3 && S.hpose[0] == 2 && S.hpose[1] == 0 && S.hpoint[0] == 3 && S.hpoint[2] == 0);
    pass_of(kD);
    CHECK(S.np == 1 && S.nl == 2 && S.pl_off[2] - S.pl_off[1] == 0);
    pass_of(kE17);
    CHECK(S.sr_o0.size() == 2 && kinds(kSchurBig) == 0);
    pass_of(kE256);
    CHECK(S.sr_o0.size() == 16 && kinds(kSchurBig) == 0 && kinds(kSchurPack) == 1);
    pass_of(kE257);
    CHECK(S.sr_o0.empty() && kinds(kSchurBig) == 1 && kinds(kSchurPack) == 0);
    pass_of(kF);
    CHECK(S.np == 7 && S.blk_off[7] - S.blk_off[6] == 0 /* block (0, 6) is empty */ && std::count(S.sr_info.begin(), S.sr_info.end(), 0) > 0);
    for (int bq = 0, r = 0; r < (int)S.sr_info.size(); ++r)
        if (S.sr_info[r] && ((S.sr_info[r] >> 8) & 255) == 0) {
            CHECK(S.sr_info[r] >> 16 == (bq == 5 ? 1 : 1 + bq % 9));
            ++bq;
        }
    pass_of(kG);
    CHECK(S.np == 0 && S.nl == 2 && S.units.empty());
    pass_of(kH40);
    CHECK(S.np == 40 && S.sr_o0.size() >= 780);
    pass_of(kH41);
    CHECK(S.np == 41);
}

int main()
{
    std::vector<Win> W;
    for (int w = 0; w < kWindows; ++w)
        W.push_back(w == kA ? win_a() : w == kB ? win_b() : w == kC ? win_c() : w == kD ? win_d() : w == kE17 ? win_e(17) : w == kE256 ? win_e(256) :
                    w == kE257 ? win_e(257) : w == kF ? win_f() : w == kG ? win_g() : win_h(w == kH40 ? 40 : 41));
    check_cases(W);
    std::vector<const Win *> nine;
    for (int w : {kA, kF, kC, kD, kE257, kB, kG, kH40, kH41}) nine.push_back(&W[w]);
    // the continuation rounds tried on the nine: one window, three, all but one, all
    std::vector<std::vector<int>> subsets = {{0}, {2, 5, 8}, {}, {}};
    for (int i = 0; i < 9; ++i) {
        if (i != 4) subsets[2].push_back(i);
        subsets[3].push_back(i);
    }
    const std::vector<std::vector<int>> first = {{0}}, three = {{2, 5, 8}};
    std::string what;
    for (int walk = 0; walk < 2; ++walk) {
        for (const Win &w : W) {
            what = w.name + (walk ? " walk" : " slots");
            g_what = what.c_str();
            check_call({&w}, walk != 0, 1, walk != 0, 1, first);
        }
        g_what = walk ? "nine walk" : "nine slots";
        check_call(nine, walk != 0, 1, walk == 0, 4, subsets);
        g_what = walk ? "nine in two groups walk" : "nine in two groups slots";
        check_call(nine, walk != 0, 2, true, 4, three);
    }
    // refusals, with the messages of build_structures
    Win R = win_b();
    R.add_edge(1, 0);
    check_refused(R, "problem 0: two edges connect the same keyframe and map point");
    R.e_pose[2] = 0;
    R.e_point[2] = 1;
    check_refused(R, "problem 0: edge 2 references a vertex out of range");
    R.e_point[2] = 0;
    R.e_pose[0] = -1;
    check_refused(R, "problem 0: edge 0 references a vertex out of range");
    check_refused(win_h(155), "problem 0: 155 free keyframes, the reduced-system solve takes at most 154");
    puts("ok");
    return 0;
}
