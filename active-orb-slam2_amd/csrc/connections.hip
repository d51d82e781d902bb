// KeyFrame::UpdateConnections (src/KeyFrame.cc:350-440) for a batch of keyframes over the graph that an aos2_local_map handle
// keeps in HBM: the counting stage and the ordering.  Integer work only; every keyframe
// of the batch is independent (the counting stage reads points and observations, never connection weights).  One kernel, a
// workgroup per keyframe:
//   count    a lane per match entry (strided), the per-item functions of csrc/connections.h, integer atomic adds on a counter per
//            keyframe of the graph (LDS while n_keyframes fits, zeroed global scratch otherwise: csrc/lm_counters.h)
//   compact  one pass over the counters in tiles of the workgroup's width, two exclusive scans: KFcounter in ascending row goes
//            straight to the output, the counters >= th become a key list (weight << 32 | row); the maximum as (weight, lowest
//            row) in one 64-bit atomicMax
//   order    the key list sorted descending by a normalised bitonic network (every exchange in one direction, so a list of any
//            length needs no padding), in LDS while it fits kConnLdsSort entries, in place in global scratch beyond that; with
//            nothing >= th the list is the single maximum
// The keyframes of a batch run in groups whose scratch fits the handle's bound, one group after the other on the handle's
// stream; the outputs lie in one device block and come back in one copy.  The resident graph is never written.
#include <algorithm>

#include "aos2_common.h"
#include "connections.h"
#include "lm_counters.h"
#include "local_map.h"
#include "regions.h"
#include "wave_ops.h"

using namespace aos2;

namespace {

constexpr int kNT = 256;             // threads of k_conn
constexpr int kConnLdsSort = 2048;   // entries of the ordered list that are sorted in LDS (16 KiB beside the 32 KiB of counters)

// one call's arguments and results on the device (the whole batch), and the scratch of one group
struct ConnDev {
    int th, mp_cap, conn_cap, ordered_cap, lds_entries;
    const int32_t *kf, *n_mp, *mp;   // mp NULL: the resident matches
    int32_t *n_conn, *conn_kf, *conn_w, *n_ordered, *ordered_kf, *ordered_w;
    int32_t *cnt;                // [group][n_kfs], the global form only: zero at entry
    unsigned long long *keys;    // [group][n_kfs]
};

// a[0 .. n) descending, the whole workgroup (n is uniform).  The normalised bitonic network: the first step of a merge of blocks
// of k pairs i with its mirror i ^ (k - 1), the others i with i + j, and EVERY exchange puts the larger key at the lower index.
// A partner at or behind n stands for a key below all others (the keys are > 0) and would never move: the pair is skipped.
__device__ __forceinline__ void conn_sort_desc(unsigned long long *a, int n, bool global)
{
    for (int k = 2; (k >> 1) < n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x;; t += kNT) {
                const int i = (t / j) * 2 * j + t % j;
                if (i >= n) break;
                const int p = j == (k >> 1) ? (i ^ (k - 1)) : i + j;
                if (p >= n) continue;
                const unsigned long long x = a[i], y = a[p];
                if (x < y) {
                    a[i] = y;
                    a[p] = x;
                }
            }
            if (global) __threadfence();
            __syncthreads();
        }
}

// :363-430 for keyframe k0 + blockIdx.x of the batch
template <bool kLds>
__global__ __launch_bounds__(kNT) void k_conn(LmGraph G, ConnDev C, int k0)
{
    __shared__ int32_t s_cnt[kLds ? kLmLdsKfs : 1];
    __shared__ unsigned long long s_keys[kConnLdsSort];
    __shared__ int32_t s_wa[kNT / 64], s_wb[kNT / 64];
    __shared__ unsigned long long s_best;
    const int g = blockIdx.x, k = k0 + g, tid = threadIdx.x, nk = G.n_kfs;
    int32_t *cnt = kLds ? s_cnt : C.cnt + (size_t)g * nk;
    unsigned long long *keys = C.keys + (size_t)g * nk;
    if constexpr (kLds)
        for (int r = tid; r < nk; r += kNT) cnt[r] = 0;
    if (tid == 0) s_best = 0ull;
    __syncthreads();
    // :363-381
    const int kf = C.kf[k];
    int nm;
    const int32_t *vpMP = conn_matches(G, kf, C.n_mp, C.mp, C.mp_cap, k, nm);
    for (int i = tid; i < nm; i += kNT) {
        const int pMP = vpMP[i];
        if (!conn_entry_counts(G, pMP)) continue;
        conn_observers(G, kf, pMP, [&](int pKFi) { atomicAdd(&cnt[pKFi], 1); });
    }
    __threadfence();
    __syncthreads();
    // :389-413 and :428  KFcounter in ascending row; the counters >= th as keys; pKFmax = the largest (weight, lowest row)
    int32_t *conn_kf = C.conn_kf + (size_t)k * C.conn_cap, *conn_w = C.conn_w + (size_t)k * C.conn_cap;
    int n_all = 0, n_hi = 0;
    for (int base = 0; base < nk; base += kNT) {
        const int r = base + tid;
        const int w = r < nk ? lm_load<kLds>(cnt + r) : 0;
        const bool any = w > 0, hi = w >= C.th;   // (th >= 1: hi implies any)
        int total_all, total_hi;
        const int pos_all = block_excl_scan_i32<kNT>(any ? 1 : 0, s_wa, total_all);
        const int pos_hi = block_excl_scan_i32<kNT>(hi ? 1 : 0, s_wb, total_hi);
        if (any) {
            if (n_all + pos_all < C.conn_cap) {
                conn_kf[n_all + pos_all] = r;
                conn_w[n_all + pos_all] = w;
            }
            atomicMax(&s_best, conn_max_key(w, r));
        }
        if (hi) keys[n_hi + pos_hi] = conn_order_key(w, r);
        n_all += total_all;
        n_hi += total_hi;
        __syncthreads();
    }
    int n_ord = n_hi;
    if (n_all > 0 && n_hi == 0) {   // :409-413  nothing over the threshold: the single maximum (:384: an empty counter lists nothing)
        n_ord = 1;
        if (tid == 0) keys[0] = conn_order_key(conn_key_weight(s_best), conn_max_row(s_best));
    }
    __threadfence();
    __syncthreads();
    // :415-422
    const bool in_lds = n_ord <= C.lds_entries;
    unsigned long long *list = in_lds ? s_keys : keys;
    if (in_lds) {
        for (int j = tid; j < n_ord; j += kNT) s_keys[j] = keys[j];
        __syncthreads();
    }
    conn_sort_desc(list, n_ord, !in_lds);
    // :428-430  the first min(count, cap) entries of each row, -1 / 0 behind them
    int32_t *ordered_kf = C.ordered_kf + (size_t)k * C.ordered_cap, *ordered_w = C.ordered_w + (size_t)k * C.ordered_cap;
    for (int j = tid; j < C.ordered_cap; j += kNT) {
        const unsigned long long key = j < n_ord ? list[j] : conn_order_key(0, -1);
        ordered_kf[j] = conn_key_row(key);
        ordered_w[j] = conn_key_weight(key);
    }
    for (int j = n_all + tid; j < C.conn_cap; j += kNT) {
        conn_kf[j] = -1;
        conn_w[j] = 0;
    }
    if (tid == 0) {
        C.n_conn[k] = n_all;
        C.n_ordered[k] = n_ord;
    }
}

}  // namespace

extern "C" {

int aos2_local_map_debug_connections_sort(aos2_local_map_t *h, int lds_entries)
{
    if (!h || lds_entries > kConnLdsSort) {
        set_error("bad argument (at most %d entries of an ordered list are sorted in LDS)", kConnLdsSort);
        return AOS2_ERR_ARG;
    }
    h->conn.lds_entries = lds_entries <= 0 ? 0 : lds_entries;
    return AOS2_OK;
}

int aos2_local_map_update_connections(aos2_local_map_t *h, int th, int n, const int32_t *kf, const int32_t *n_mp, const int32_t *mp,
                                      int mp_cap, int32_t *n_conn, int32_t *conn_kf, int32_t *conn_w, int conn_cap, int32_t *n_ordered,
                                      int32_t *ordered_kf, int32_t *ordered_w, int ordered_cap)
{
    if (!h) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    static const char *const pre = "update connections";
    if (!h->has_graph) return lm_fail(pre, "aos2_local_map_set comes first");
    const ConnArgs A = {th, n, kf, n_mp, mp, mp_cap, n_conn, conn_kf, conn_w, conn_cap, n_ordered, ordered_kf, ordered_w, ordered_cap};
    char why[200];
    if (conn_check(A, h->n_kfs, why, sizeof why)) return lm_fail(pre, "%s", why);
    // the bound: one keyframe's counters and key list
    const int64_t nk = h->n_kfs;
    const int64_t per_kf = 12 * nk + 16;
    if (per_kf > h->scratch_bytes)
        return lm_fail(pre, "%lld keyframes need %lld bytes of scratch per keyframe of the batch, the bound is %lld", (long long)nk,
                       (long long)per_kf, (long long)h->scratch_bytes);
    ConnState &K = h->conn;
    K.timer.timed = false;
    h->last_groups = 0;
    if (n == 0) return AOS2_OK;
    int st;
    if ((st = bind_device(h->device))) return st;
    if ((st = local_map_upload(h, kLmGraph))) return st;
    if (!h->stream && (st = stream_create(&h->stream, false))) return st;
    const size_t B = (size_t)n;
    const int group = (int)std::min<int64_t>(n, h->scratch_bytes / per_kf);
    ConnDev C = {};
    Regions<2> RS;
    RS.add(C.cnt, (size_t)group * nk); RS.add(C.keys, (size_t)group * nk);
    if ((st = h->d_scratch.alloc((RS.bytes() + 256) / 4))) return st;
    RS.bind(reinterpret_cast<uint8_t *>(h->d_scratch.p));
    // one block: what goes in, then what comes back; the page-locked staging has the same layout
    Regions<9> R;
    R.add(C.kf, B);
    if (mp) {
        R.add(C.n_mp, B);
        R.add(C.mp, B * mp_cap);
    }
    const size_t in_bytes = R.bytes();
    const size_t out0 = R.add(C.n_conn, B);
    R.add(C.n_ordered, B); R.add(C.conn_kf, B * conn_cap); R.add(C.conn_w, B * conn_cap); R.add(C.ordered_kf, B * ordered_cap);
    R.add(C.ordered_w, B * ordered_cap);
    if ((st = K.d_io.alloc(R.bytes() + 256)) || (st = K.io.alloc(R.bytes() + 256))) return st;
    R.bind(K.io.p);   // (the staging first: the same fields name the inputs' places)
    memcpy(const_cast<int32_t *>(C.kf), kf, B * 4);
    if (mp) {
        memcpy(const_cast<int32_t *>(C.n_mp), n_mp, B * 4);
        memcpy(const_cast<int32_t *>(C.mp), mp, B * mp_cap * 4);
    }
    R.bind(K.d_io.p);
    C.th = th; C.mp_cap = mp_cap; C.conn_cap = conn_cap; C.ordered_cap = ordered_cap;
    C.lds_entries = K.lds_entries > 0 ? K.lds_entries : kConnLdsSort;
    const bool lds = h->n_kfs <= h->lds_kfs;
    hipStream_t q = h->stream;
    if ((st = K.timer.begin(q))) return st;
    AOS2_HIP_CHECK(hipMemcpyAsync(K.d_io.p, K.io.p, in_bytes, hipMemcpyHostToDevice, q));
    for (int k0 = 0; k0 < n; k0 += group) {
        const int gs = std::min(group, n - k0);
        if (!lds && nk) AOS2_HIP_CHECK(hipMemsetAsync(C.cnt, 0, (size_t)gs * nk * 4, q));
        if (lds) hipLaunchKernelGGL(k_conn<true>, dim3(gs), dim3(kNT), 0, q, h->G, C, k0);
        else hipLaunchKernelGGL(k_conn<false>, dim3(gs), dim3(kNT), 0, q, h->G, C, k0);
        AOS2_HIP_CHECK(hipGetLastError());
        ++h->last_groups;
    }
    AOS2_HIP_CHECK(hipMemcpyAsync(K.io.p + out0, K.d_io.p + out0, R.bytes() - out0, hipMemcpyDeviceToHost, q));
    if ((st = K.timer.end(q, true))) return st;
    const uint8_t *out = K.io.p + out0;
    memcpy(n_conn, span_copy(out, C.n_conn, C.n_conn), B * 4);
    memcpy(n_ordered, span_copy(out, C.n_conn, C.n_ordered), B * 4);
    if (conn_cap > 0) {
        memcpy(conn_kf, span_copy(out, C.n_conn, C.conn_kf), B * conn_cap * 4);
        memcpy(conn_w, span_copy(out, C.n_conn, C.conn_w), B * conn_cap * 4);
    }
    if (ordered_cap > 0) {
        memcpy(ordered_kf, span_copy(out, C.n_conn, C.ordered_kf), B * ordered_cap * 4);
        memcpy(ordered_w, span_copy(out, C.n_conn, C.ordered_w), B * ordered_cap * 4);
    }
    return AOS2_OK;
}

float aos2_local_map_last_connections_device_ms(aos2_local_map_t *h)
{
    return h ? h->conn.timer.ms() : -1.f;
}

}  // extern "C"
