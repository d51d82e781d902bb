// The one list of the resident local map's arrays (csrc/local_map_arrays.h) without a GPU: what lm_each visits, the layout of
// the graph block, the view behind it and a delta's block against the call order these blocks have always had (written out
// here on aos2::Regions directly), a round trip of the host mirror through a block, and the values of an appended row.
// Built with -fsanitize=address,undefined by tests/test_capi_cpu.py: a region that ran past its block would stop the program.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "local_map_arrays.h"
#include "regions.h"

using namespace aos2;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
            return 1;                                                   \
        }                                                               \
    } while (0)

// the order of the graph block and of the view behind it, by name
static size_t graph_block(const LmCounts &c, bool view, size_t off[17])
{
    const uint8_t *u8[5];
    const int32_t *i32[10];
    const int8_t *i8;
    const float *f32[2];
    const size_t np = c.point_rows, nk = c.link_rows;
    Regions<17> R;
    int n = 0;
    off[n++] = R.add(u8[0], np);                    // point_bad
    off[n++] = R.add(u8[1], nk);                    // kf_bad
    off[n++] = R.add(i32[0], np);                   // point_nobs
    off[n++] = R.add(i32[1], np + 1);               // obs_off
    off[n++] = R.add(i32[2], c.obs);                // obs_kf
    off[n++] = R.add(i32[3], c.match_rows + 1);     // kf_mp_off
    off[n++] = R.add(i32[4], c.mp);                 // kf_mp
    off[n++] = R.add(i32[5], nk * 10);              // kf_best
    off[n++] = R.add(i32[6], nk + 1);               // kf_child_off
    off[n++] = R.add(i32[7], c.child);              // kf_child
    off[n++] = R.add(i32[8], nk);                   // kf_parent
    if (view) {
        off[n++] = R.add(i32[9], c.obs);            // obs_idx
        off[n++] = R.add(i8, c.mp);                 // kf_octave
        off[n++] = R.add(f32[0], c.mp);             // kf_depth
        off[n++] = R.add(u8[2], c.mp);              // kf_stereo
        off[n++] = R.add(f32[1], nk);               // kf_th_depth
        off[n++] = R.add(u8[3], nk);                // kf_flags
    }
    return R.bytes();
}

// ... and of a delta's block
static size_t delta_block(const LmCounts &c, bool view)
{
    const uint8_t *u8[4];
    const int32_t *i32[14];
    const int8_t *i8;
    const float *f32[2];
    const size_t npr = c.point_rows, nmr = c.match_rows, nlr = c.link_rows;
    Regions<20> Q;
    Q.add(i32[0], npr); Q.add(u8[0], npr); Q.add(i32[1], npr); Q.add(i32[2], npr + 1); Q.add(i32[3], c.obs);   // point rows
    Q.add(i32[4], nmr); Q.add(i32[5], nmr + 1); Q.add(i32[6], c.mp);                                        // match rows
    Q.add(i32[7], nlr); Q.add(u8[1], nlr); Q.add(i32[8], nlr * 10); Q.add(i32[9], nlr + 1); Q.add(i32[10], c.child);
    Q.add(i32[11], nlr);                                                                                    // link rows
    if (view) {
        Q.add(i32[12], c.obs); Q.add(i8, c.mp); Q.add(f32[0], c.mp); Q.add(u8[2], c.mp); Q.add(f32[1], nlr); Q.add(u8[3], nlr);
    }
    return Q.bytes();
}

// the planted graph: 3 points observed by {0, 1}, {}, {1}; 2 keyframes of 2 and 3 features; children {1}, {}
static LmArrays<LmVec> planted()
{
    LmArrays<LmVec> V;
    V.point_bad = {0, 1, 0};
    V.point_nobs = {3, 0, 1};
    V.obs_off = {0, 2, 2, 3};
    V.obs_kf = {0, 1, 1};
    V.kf_bad = {0, 0};
    V.kf_mp_off = {0, 2, 5};
    V.kf_mp = {0, -1, 2, 0, -1};
    V.kf_best.assign(20, -1);
    V.kf_best[0] = 1;
    V.kf_best[10] = 0;
    V.kf_child_off = {0, 1, 1};
    V.kf_child = {1};
    V.kf_parent = {-1, 0};
    V.obs_idx = {0, 2, 0};
    V.kf_octave = {0, 1, 2, 3, -1};
    V.kf_depth = {1.f, 2.f, 0.5f, -1.f, 4.f};
    V.kf_stereo = {1, 0, 0, 1, 0};
    V.kf_th_depth = {2.f, 3.f};
    V.kf_flags = {1, 2};
    return V;
}

template <class A>
static bool same(const A &a, const A &b, int parts)
{
    bool ok = true;
    lm_each(a, b, parts, [&](const auto &x, const auto &y, LmLen, auto) { ok = ok && x == y; });
    return ok;
}

// through a block of exactly the laid-out size and back
static bool round_trip(const LmArrays<LmVec> &V, const LmCounts &c, int parts, size_t want_bytes)
{
    LmArrays<LmPtr> P = {};
    Regions<17> R;
    lm_layout(R, P, c, parts);
    if (R.bytes() != want_bytes) return false;
    std::vector<uint8_t> block(R.bytes());
    R.bind(block.data());
    lm_copy(P, lm_data(V), c, parts);
    LmArrays<LmVec> W;
    lm_take(W, P, c, parts);
    return same(V, W, parts);
}

int main()
{
    const int both = kLmGraph | kLmView;
    static_assert(sizeof(LmArrays<LmPtr>) == 17 * sizeof(void *), "17 arrays");
    {   // every array once
        LmArrays<LmPtr> a = {}, b = {};
        for (int parts : {(int)kLmGraph, (int)kLmView, both}) {
            std::set<const void *> seen_a, seen_b;
            int n = 0;
            lm_each(a, b, parts, [&](auto &x, auto &y, LmLen, auto) {
                seen_a.insert(&x);
                seen_b.insert(&y);
                ++n;
            });
            const int want = parts == both ? 17 : parts == kLmGraph ? 11 : 6;
            CHECK(n == want && (int)seen_a.size() == want && (int)seen_b.size() == want);
            for (const void *p : seen_a) CHECK(p >= (const void *)&a && p < (const void *)(&a + 1));
            for (const void *p : seen_b) CHECK(p >= (const void *)&b && p < (const void *)(&b + 1));
        }
    }
    const LmCounts graph = {3, 2, 2, 3, 5, 1}, empty = {0, 0, 0, 0, 0, 0};
    size_t want_off[17], bytes[2];
    for (int view = 0; view < 2; ++view) {   // the block: sizes, and every array where it has always been
        const size_t want = graph_block(graph, view, want_off);
        CHECK(want == (view ? 4098u : 2568u));
        LmArrays<LmPtr> P = {};
        Regions<17> R;
        lm_layout(R, P, graph, view ? both : (int)kLmGraph);
        CHECK(R.bytes() == want);
        CHECK(R.n == (view ? 17 : 11));
        for (int i = 0; i < R.n; ++i) CHECK(R.region[i].off == want_off[i] && want_off[i] == 256u * i);
        alignas(256) static uint8_t base[4352];
        R.bind(base);
        const void *in_order[17] = {P.point_bad, P.kf_bad, P.point_nobs, P.obs_off, P.obs_kf, P.kf_mp_off, P.kf_mp, P.kf_best, P.kf_child_off,
                                    P.kf_child, P.kf_parent, P.obs_idx, P.kf_octave, P.kf_depth, P.kf_stereo, P.kf_th_depth, P.kf_flags};
        for (int i = 0; i < 17; ++i) CHECK(in_order[i] == (i < R.n ? base + 256 * i : nullptr));
        bytes[view] = want;
    }
    CHECK(graph_block(empty, false, want_off) == 768u);
    {
        LmArrays<LmPtr> P = {};
        Regions<17> R;
        lm_layout(R, P, empty, kLmGraph);
        CHECK(R.bytes() == 768u);
    }
    // the mirror through a block and back: the planted graph with and without the view, and the empty map (zero-length arrays)
    const LmArrays<LmVec> V = planted();
    CHECK(round_trip(V, graph, kLmGraph, bytes[0]) && round_trip(V, graph, both, bytes[1]));
    LmArrays<LmVec> E;
    E.obs_off = E.kf_mp_off = E.kf_child_off = {0};
    CHECK(round_trip(E, empty, kLmGraph, 768u) && round_trip(E, empty, both, graph_block(empty, true, want_off)));
    {   // lm_data names the vectors' storage; lm_copy moves what the counts say
        const LmArrays<LmPtr> P = lm_data(V);
        CHECK(P.kf_best == V.kf_best.data() && P.kf_flags == V.kf_flags.data());
        CHECK(!lm_null_with_length(P, graph, both));
        LmArrays<LmPtr> N = P;
        N.kf_octave = nullptr;
        CHECK(lm_null_with_length(N, graph, both) && !lm_null_with_length(N, graph, kLmGraph));
        CHECK(!lm_null_with_length(LmArrays<LmPtr>{}, LmCounts{0, 0, 0, 0, 0, 0}, kLmView));
    }
    size_t delta_bytes[2];
    for (int view = 0; view < 2; ++view) {   // a delta of 2 point rows, 1 match row and 1 link row
        const LmCounts dc = {2, 1, 1, 3, 4, 2};
        LmArrays<LmPtr> D = {};
        const int32_t *row[3] = {nullptr, nullptr, nullptr};
        Regions<20> Q;
        lm_layout_delta(Q, row, D, dc, view ? both : (int)kLmGraph);
        CHECK(Q.bytes() == delta_block(dc, view) && Q.n == (view ? 20 : 14));
        std::vector<uint8_t> block(Q.bytes());
        Q.bind(block.data());
        CHECK((const void *)row[0] == block.data() && (const void *)D.point_bad == block.data() + 256);
        CHECK((const void *)row[1] == block.data() + 5 * 256 && (const void *)row[2] == block.data() + 8 * 256);
        CHECK((const void *)D.kf_bad == block.data() + 9 * 256 && (const void *)D.kf_parent == block.data() + 13 * 256);
        CHECK(view ? (const void *)D.obs_idx == block.data() + 14 * 256 : D.obs_idx == nullptr);
        delta_bytes[view] = Q.bytes();
    }
    {   // an appended row that a delta does not name
        LmArrays<LmVec> W;
        lm_each(W, W, both, [](auto &v, auto &, LmLen l, auto fill) {
            if (l == kLmPerPoint || l == kLmPerLink || l == kLmLinkNb) v.assign(1, fill);
        });
        CHECK(W.point_bad[0] == 1 && W.point_nobs[0] == 0 && W.kf_bad[0] == 1 && W.kf_best[0] == -1 && W.kf_parent[0] == -1);
        CHECK(W.kf_th_depth[0] == 0.f && W.kf_flags[0] == 0);
        CHECK(W.obs_off.empty() && W.obs_kf.empty() && W.kf_mp.empty() && W.kf_octave.empty());
    }
    printf("local_map_arrays_test ok: 11 + 6 arrays; graph block %zu / %zu bytes, empty map 768; delta block %zu / %zu bytes\n", bytes[0],
           bytes[1], delta_bytes[0], delta_bytes[1]);
    return 0;
}
