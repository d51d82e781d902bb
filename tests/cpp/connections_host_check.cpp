// TEST INFRASTRUCTURE: the host side of KeyFrame::UpdateConnections (active-orb-slam2_amd/csrc/connections.h: the argument checks and
// the serial loop that aos2_debug_update_connections_host runs) as a stand-alone program, so that it can be built with
// -fsanitize=address,undefined and run on the CPU.  Seeded random graphs and batches in both forms of the matches, every capacity from
// 0 up, each output array allocated at EXACTLY its size (a write behind one is a heap overflow the sanitizer reports), checked
// against a second count with std::map written here; then the refusals.  Exit status 0 and "ok" on success.
#include "../../active-orb-slam2_amd/csrc/connections.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>

using namespace aos2;

static int failures = 0;
#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("line %d: %s\n", __LINE__, #c);                \
            ++failures;                                                \
        }                                                              \
    } while (0)

struct Graph {
    std::vector<uint8_t> point_bad;
    std::vector<int32_t> obs_off, obs_kf, kf_mp_off, kf_mp;
    LmGraph G = {};
    Graph(std::mt19937 &rng, int nk, int np)
    {
        obs_off.push_back(0);
        for (int p = 0; p < np; ++p) {
            point_bad.push_back(rng() % 10 == 0);
            for (int k = 0; k < nk; ++k)
                if (rng() % 3 == 0) obs_kf.push_back(k);
            obs_off.push_back((int32_t)obs_kf.size());
        }
        kf_mp_off.push_back(0);
        for (int k = 0; k < nk; ++k) {
            const int nf = (int)(rng() % 40);
            for (int f = 0; f < nf; ++f) kf_mp.push_back(np && rng() % 5 ? (int32_t)(rng() % np) : -1);
            kf_mp_off.push_back((int32_t)kf_mp.size());
        }
        G.n_points = np; G.n_kfs = nk;
        G.point_bad = point_bad.data(); G.obs_off = obs_off.data(); G.obs_kf = obs_kf.data();
        G.kf_mp_off = kf_mp_off.data(); G.kf_mp = kf_mp.data();
    }
};

static void run_case(std::mt19937 &rng)
{
    const int nk = 1 + (int)(rng() % 20), np = (int)(rng() % 60), n = (int)(rng() % 6), th = 1 + (int)(rng() % 5);
    const Graph g(rng, nk, np);
    const bool explicit_mp = rng() % 2;
    const int mp_cap = explicit_mp ? (int)(rng() % 30) : 0, conn_cap = (int)(rng() % (nk + 2)), ordered_cap = (int)(rng() % (nk + 2));
    std::vector<int32_t> kf(n), n_mp(n), mp((size_t)n * mp_cap);
    for (int k = 0; k < n; ++k) {
        kf[k] = explicit_mp ? (int32_t)(rng() % (nk + 1)) - 1 : (int32_t)(rng() % nk);
        n_mp[k] = mp_cap ? (int32_t)(rng() % (mp_cap + 1)) : 0;
        for (int i = 0; i < mp_cap; ++i) mp[(size_t)k * mp_cap + i] = (int32_t)(rng() % (np + 4)) - 1;
    }
    std::vector<int32_t> n_conn(n), n_ordered(n), conn_kf((size_t)n * conn_cap), conn_w((size_t)n * conn_cap),
        ordered_kf((size_t)n * ordered_cap), ordered_w((size_t)n * ordered_cap);
    static int32_t none;   // (a zero-length std::vector may hand out NULL; the explicit form needs a pointer)
    const ConnArgs a = {th, n, kf.data(), explicit_mp ? (n ? n_mp.data() : &none) : nullptr, explicit_mp ? (mp.empty() ? &none : mp.data()) : nullptr,
                        mp_cap, n_conn.data(), conn_cap ? conn_kf.data() : nullptr, conn_cap ? conn_w.data() : nullptr, conn_cap,
                        n_ordered.data(), ordered_cap ? ordered_kf.data() : nullptr, ordered_cap ? ordered_w.data() : nullptr, ordered_cap};
    char why[200] = "";
    if (conn_check(a, nk, why, sizeof why)) {
        std::printf("a valid case was refused: %s\n", why);
        ++failures;
        return;
    }
    conn_host_run(g.G, a);
    for (int k = 0; k < n; ++k) {
        std::map<int, int> counter;
        const int32_t *m = explicit_mp ? mp.data() + (size_t)k * mp_cap : g.kf_mp.data() + g.kf_mp_off[kf[k]];
        const int nm = explicit_mp ? n_mp[k] : g.kf_mp_off[kf[k] + 1] - g.kf_mp_off[kf[k]];
        for (int i = 0; i < nm; ++i) {
            if (m[i] < 0 || m[i] >= np || g.point_bad[m[i]]) continue;
            for (int e = g.obs_off[m[i]]; e < g.obs_off[m[i] + 1]; ++e)
                if (g.obs_kf[e] != kf[k]) counter[g.obs_kf[e]]++;
        }
        std::vector<std::pair<int, int>> listed;
        std::pair<int, int> top(0, -1);
        for (const auto &kv : counter) {
            if (kv.second > top.first) top = std::make_pair(kv.second, kv.first);
            if (kv.second >= th) listed.push_back(std::make_pair(kv.second, kv.first));
        }
        if (listed.empty() && !counter.empty()) listed.push_back(top);
        std::sort(listed.rbegin(), listed.rend());
        EXPECT(n_conn[k] == (int)counter.size());
        EXPECT(n_ordered[k] == (int)listed.size());
        int j = 0;
        for (const auto &kv : counter) {
            if (j >= conn_cap) break;
            EXPECT(conn_kf[(size_t)k * conn_cap + j] == kv.first && conn_w[(size_t)k * conn_cap + j] == kv.second);
            ++j;
        }
        for (; j < conn_cap; ++j) EXPECT(conn_kf[(size_t)k * conn_cap + j] == -1 && conn_w[(size_t)k * conn_cap + j] == 0);
        for (j = 0; j < ordered_cap; ++j) {
            const bool in = j < (int)listed.size();
            EXPECT(ordered_kf[(size_t)k * ordered_cap + j] == (in ? listed[j].second : -1));
            EXPECT(ordered_w[(size_t)k * ordered_cap + j] == (in ? listed[j].first : 0));
        }
    }
}

static void refusals()
{
    int32_t kf[1] = {0}, n_mp[1] = {1}, mp[2] = {0, 0}, out[6][2];
    const ConnArgs ok = {3, 1, kf, nullptr, nullptr, 0, out[0], out[1], out[2], 2, out[3], out[4], out[5], 2};
    char why[200];
    EXPECT(!conn_check(ok, 2, why, sizeof why));
    ConnArgs a = ok;
    a.th = 0; EXPECT(conn_check(a, 2, why, sizeof why));
    a = ok; a.n = -1; EXPECT(conn_check(a, 2, why, sizeof why));
    a = ok; a.conn_cap = -1; EXPECT(conn_check(a, 2, why, sizeof why));
    a = ok; a.ordered_cap = -1; EXPECT(conn_check(a, 2, why, sizeof why));
    a = ok; a.mp_cap = 2; EXPECT(conn_check(a, 2, why, sizeof why));
    a = ok; a.n_mp = n_mp; EXPECT(conn_check(a, 2, why, sizeof why));
    a = ok; a.mp = mp; EXPECT(conn_check(a, 2, why, sizeof why));
    a = ok; a.kf = nullptr; EXPECT(conn_check(a, 2, why, sizeof why));
    a = ok; a.n_conn = nullptr; EXPECT(conn_check(a, 2, why, sizeof why));
    a = ok; a.conn_w = nullptr; EXPECT(conn_check(a, 2, why, sizeof why));
    a = ok; a.ordered_kf = nullptr; EXPECT(conn_check(a, 2, why, sizeof why));
    a = ok; kf[0] = 2; EXPECT(conn_check(a, 2, why, sizeof why));
    kf[0] = -1; EXPECT(conn_check(a, 2, why, sizeof why));
    a.n_mp = n_mp; a.mp = mp; a.mp_cap = 2; EXPECT(!conn_check(a, 2, why, sizeof why));   // -1 with explicit matches
    n_mp[0] = 3; EXPECT(conn_check(a, 2, why, sizeof why));
    n_mp[0] = -1; EXPECT(conn_check(a, 2, why, sizeof why));
    n_mp[0] = 2; mp[1] = -2; EXPECT(conn_check(a, 2, why, sizeof why));
    char tiny[8];
    EXPECT(conn_check(a, 2, tiny, sizeof tiny) && tiny[7] == 0);   // (the reason is cut to the buffer)
}

int main()
{
    std::mt19937 rng(20240611);
    for (int i = 0; i < 2000; ++i) run_case(rng);
    refusals();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
