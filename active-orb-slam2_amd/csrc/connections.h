// KeyFrame::UpdateConnections (src/KeyFrame.cc:350-440) over the resident graph of aos2_local_map_*: what csrc/connections.hip
// shares with the host tap aos2_debug_update_connections_host (csrc/debug_taps.hip) -- the argument checks, the per-item functions
// (which match entry counts, whom an entry counts for, the two keys that carry the orders of :389-413 and :415-422) and the serial
// loop itself, which is the tap.  The kernel calls the per-item functions with a lane per match entry and a lane per counter, the
// serial loop in the reference's own order on one core.  They read the graph through LmGraph (csrc/local_map_arrays.h), device or
// host addresses.  No HIP runtime calls and no other header of the library: host C++ and kernels.  Internal to the library.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "local_map_arrays.h"

#if defined(__HIPCC__)
#define AOS2_CONN_HD __host__ __device__ __forceinline__
#else
#define AOS2_CONN_HD inline
#endif

namespace aos2 {

// the arguments of aos2_local_map_update_connections behind the handle (include/aos2.h), host addresses
struct ConnArgs {
    int th, n;
    const int32_t *kf, *n_mp, *mp;
    int mp_cap;
    int32_t *n_conn, *conn_kf, *conn_w;
    int conn_cap;
    int32_t *n_ordered, *ordered_kf, *ordered_w;
    int ordered_cap;
};

// :366-371  whether a match entry counts: not NULL, a row of the table, not isBad()
AOS2_CONN_HD bool conn_entry_counts(const LmGraph &G, int pMP)
{
    return pMP >= 0 && pMP < G.n_points && !G.point_bad[pMP];
}

// :373-380  KFcounter[mit->first]++ for every observation of the point but the keyframe's own; count(row) is the increment.  No
// isBad() test on the observer.  kf = -1 (a keyframe the graph does not know) skips nothing.
template <class Count>
AOS2_CONN_HD void conn_observers(const LmGraph &G, int kf, int pMP, Count &&count)
{
    const int e1 = G.obs_off[pMP + 1];
    for (int e = G.obs_off[pMP]; e < e1; ++e) {
        const int pKFi = G.obs_kf[e];
        if (pKFi == kf) continue;   // :375
        count(pKFi);
    }
}

// :415-422  sort(vPairs) on (weight, KeyFrame*) ascending, reversed by push_front: descending keys of (weight, row).  Unique per
// keyframe, and > 0 (a listed weight is >= 1).
AOS2_CONN_HD unsigned long long conn_order_key(int w, int row) { return ((unsigned long long)(uint32_t)w << 32) | (uint32_t)row; }
AOS2_CONN_HD int conn_key_weight(unsigned long long key) { return (int)(key >> 32); }
AOS2_CONN_HD int conn_key_row(unsigned long long key) { return (int)(uint32_t)key; }
// :397-401  pKFmax = the first strict maximum in ascending row = the largest (weight, LOWEST row): NOT the order above
AOS2_CONN_HD unsigned long long conn_max_key(int w, int row) { return conn_order_key(w, 0x7fffffff - row); }
AOS2_CONN_HD int conn_max_row(unsigned long long key) { return 0x7fffffff - conn_key_row(key); }

// where the matches of item k come from: the uploaded list, or the resident row of kf[k]
AOS2_CONN_HD const int32_t *conn_matches(const LmGraph &G, int kf, const int32_t *n_mp, const int32_t *mp, int mp_cap, int k, int &n)
{
    if (mp) {
        n = n_mp[k];
        return mp + (size_t)k * mp_cap;
    }
    n = G.kf_mp_off[kf + 1] - G.kf_mp_off[kf];
    return G.kf_mp + G.kf_mp_off[kf];
}

inline int conn_refuse(char *msg, size_t len, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
inline int conn_refuse(char *msg, size_t len, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, len, fmt, ap);
    va_end(ap);
    return 1;
}

// The checks of aos2_local_map_update_connections on its own arguments against a graph of n_keyframes rows: 0, or 1 with the
// reason in msg.  The graph is not read.
inline int conn_check(const ConnArgs &a, int n_keyframes, char *msg, size_t len)
{
    if (a.th < 1) return conn_refuse(msg, len, "th = %d is below 1", a.th);
    if (a.n < 0 || a.mp_cap < 0 || a.conn_cap < 0 || a.ordered_cap < 0)
        return conn_refuse(msg, len, "negative count or capacity (%d keyframes, room for %d matches, %d connections, %d ordered)", a.n,
                           a.mp_cap, a.conn_cap, a.ordered_cap);
    if ((a.mp != nullptr) != (a.n_mp != nullptr)) return conn_refuse(msg, len, "mp and n_mp come together");
    if (!a.mp && a.mp_cap > 0) return conn_refuse(msg, len, "mp is NULL with room for %d matches", a.mp_cap);
    if (a.n > 0 && (!a.kf || !a.n_conn || !a.n_ordered)) return conn_refuse(msg, len, "kf, n_conn or n_ordered is NULL");
    if (a.n > 0 && a.conn_cap > 0 && (!a.conn_kf || !a.conn_w)) return conn_refuse(msg, len, "conn_kf or conn_w is NULL");
    if (a.n > 0 && a.ordered_cap > 0 && (!a.ordered_kf || !a.ordered_w)) return conn_refuse(msg, len, "ordered_kf or ordered_w is NULL");
    for (int k = 0; k < a.n; ++k) {
        if (a.kf[k] < (a.mp ? -1 : 0) || a.kf[k] >= n_keyframes)
            return conn_refuse(msg, len, "kf[%d] = %d is outside [%d, %d)", k, a.kf[k], a.mp ? -1 : 0, n_keyframes);
        if (!a.mp) continue;
        if (a.n_mp[k] < 0 || a.n_mp[k] > a.mp_cap) return conn_refuse(msg, len, "n_mp[%d] = %d is outside [0, %d]", k, a.n_mp[k], a.mp_cap);
        for (int i = 0; i < a.n_mp[k]; ++i)
            if (a.mp[(size_t)k * a.mp_cap + i] < -1)
                return conn_refuse(msg, len, "mp[%d][%d] = %d is below -1", k, i, a.mp[(size_t)k * a.mp_cap + i]);
    }
    return 0;
}

// one row of an output pair: the first min(count, cap) entries, then -1 / 0 up to the capacity
template <class At>
inline void conn_write_row(int32_t *kf, int32_t *w, int cap, int count, At &&at)
{
    for (int j = 0; j < cap; ++j) {
        const unsigned long long key = j < count ? at(j) : conn_order_key(0, -1);
        kf[j] = conn_key_row(key);
        w[j] = conn_key_weight(key);
    }
}

// The function as the reference runs it, one keyframe, one match entry and one observation at a time (the arguments have passed
// conn_check and the graph its own check).
inline void conn_host_run(const LmGraph &G, const ConnArgs &a)
{
    std::vector<int32_t> KFcounter(G.n_kfs);
    std::vector<unsigned long long> all, vPairs;
    for (int k = 0; k < a.n; ++k) {
        const int kf = a.kf[k];
        std::fill(KFcounter.begin(), KFcounter.end(), 0);
        int nm;
        const int32_t *vpMP = conn_matches(G, kf, a.n_mp, a.mp, a.mp_cap, k, nm);
        for (int i = 0; i < nm; ++i) {   // :363-381
            if (!conn_entry_counts(G, vpMP[i])) continue;
            conn_observers(G, kf, vpMP[i], [&](int pKFi) { KFcounter[pKFi]++; });
        }
        all.clear();
        vPairs.clear();
        unsigned long long best = 0;
        for (int r = 0; r < G.n_kfs; ++r) {   // :389-413 in ascending row
            const int w = KFcounter[r];
            if (w <= 0) continue;
            all.push_back(conn_order_key(w, r));
            best = std::max(best, conn_max_key(w, r));
            if (w >= a.th) vPairs.push_back(conn_order_key(w, r));
        }
        if (!all.empty() && vPairs.empty()) vPairs.push_back(conn_order_key(conn_key_weight(best), conn_max_row(best)));
        std::sort(vPairs.begin(), vPairs.end(), [](unsigned long long x, unsigned long long y) { return x > y; });   // :415-422
        a.n_conn[k] = (int32_t)all.size();   // :384: empty = both counts 0
        a.n_ordered[k] = (int32_t)vPairs.size();
        if (a.conn_cap > 0)
            conn_write_row(a.conn_kf + (size_t)k * a.conn_cap, a.conn_w + (size_t)k * a.conn_cap, a.conn_cap, (int)all.size(),
                           [&](int j) { return all[j]; });
        if (a.ordered_cap > 0)
            conn_write_row(a.ordered_kf + (size_t)k * a.ordered_cap, a.ordered_w + (size_t)k * a.ordered_cap, a.ordered_cap,
                           (int)vPairs.size(), [&](int j) { return vPairs[j]; });
    }
}

}  // namespace aos2
