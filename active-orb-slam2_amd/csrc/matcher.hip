// ORBmatcher hot path on gfx950: 256-bit Hamming (xor + popcount) brute force, SearchByBoW and the
// two SearchByProjection variants (reference src/ORBmatcher.cc:45-129, 159-288, 1328-1470,
// DescriptorDistance :1647-1663).  Integer VALU work; descriptors stay L2/LDS resident.
//
// The reference loops are sequential over the query set (a later query sees the features an
// earlier one took, :87-89, :209, :1403-1405).  Each problem therefore runs on ONE wave: the
// 64 lanes share the candidate set of the current query (Hamming distances + a two-smallest
// reduction with the reference's first-wins tie-break), while the greedy bookkeeping is
// wave-uniform.  Independent problems ((KF,F) pairs) are spread over the grid.
#include <type_traits>
#include <vector>

#include "aos2_common.h"
#include "matcher_handle.h"
#include "regions.h"
#include "search_device.h"
#include "wave_ops.h"

namespace aos2 {

// ---------------------------------------------------------------------------------------------
// Brute force: best and second best train descriptor per query.  Block = 256 threads = 256
// queries; the train set is streamed through LDS in 256-descriptor tiles (8 KB), every lane
// reads the same train word (LDS broadcast).  grid.y splits the train set; partial results are
// merged by a second tiny kernel.  key = dist << 20 | train index  (first index wins ties).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hamming_best2_kernel(const uint8_t *__restrict__ q, int nq,
                                                            const uint8_t *__restrict__ t, int nt,
                                                            int t_per_split, uint32_t *__restrict__ part1,
                                                            uint32_t *__restrict__ part2)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[256 * 8];
    const int qi = blockIdx.x * 256 + threadIdx.x;
    const int t0 = blockIdx.y * t_per_split, t1 = min(nt, t0 + t_per_split);
    Desc dq{};
    if (qi < nq) dq = load_desc(q + (size_t)qi * 32);
    uint32_t k1 = KEY_NONE, k2 = KEY_NONE;
    for (int base = t0; base < t1; base += 256) {
        const int cnt = min(256, t1 - base);
        __syncthreads();
        for (int i = threadIdx.x; i < cnt * 2; i += 256)
            reinterpret_cast<uint4 *>(tile)[i] = reinterpret_cast<const uint4 *>(t + (size_t)base * 32)[i];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const uint4 a = reinterpret_cast<const uint4 *>(tile)[2 * j];
            const uint4 b = reinterpret_cast<const uint4 *>(tile)[2 * j + 1];
            int d = __popc(dq.w[0] ^ a.x) + __popc(dq.w[1] ^ a.y) + __popc(dq.w[2] ^ a.z) + __popc(dq.w[3] ^ a.w) +
                    __popc(dq.w[4] ^ b.x) + __popc(dq.w[5] ^ b.y) + __popc(dq.w[6] ^ b.z) + __popc(dq.w[7] ^ b.w);
            const uint32_t key = ((uint32_t)d << 20) | (uint32_t)(base + j);
            if (key < k1) {
                k2 = k1;
                k1 = key;
            } else if (key < k2)
                k2 = key;
        }
    }
    if (qi < nq) {
        part1[(size_t)blockIdx.y * nq + qi] = k1;
        part2[(size_t)blockIdx.y * nq + qi] = k2;
    }
}

__global__ void hamming_merge_kernel(const uint32_t *__restrict__ part1, const uint32_t *__restrict__ part2,
                                     int nq, int splits, int32_t *__restrict__ best_idx,
                                     int32_t *__restrict__ best_dist, int32_t *__restrict__ second_dist)
{
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    uint32_t k1 = KEY_NONE, k2 = KEY_NONE;
    for (int s = 0; s < splits; ++s) merge2(k1, k2, part1[(size_t)s * nq + qi], part2[(size_t)s * nq + qi]);
    best_idx[qi] = k1 == KEY_NONE ? -1 : (int32_t)(k1 & 0xfffff);
    best_dist[qi] = key_dist(k1);
    second_dist[qi] = key_dist(k2);
}

// SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)  :159-288
struct BowQuery {
    int32_t kf_idx;   // realIdxKF
    int32_t f_beg;    // start of the frame's bucket in node_idx_f
    int32_t f_cnt;    // bucket size
    int32_t ent_off;  // offset of this query's entries
};

struct BowPairDev {
    int n_kf, n_f, n_queries;
    const uint8_t *desc_kf, *desc_f;
    const float *angle_kf, *angle_f;
    const int32_t *node_idx_f;
    const BowQuery *queries;  // in the reference's visiting order (common nodes ascending, KF features in node order)
    Entry *entries;
    int32_t *match_f;   // n_f
    uint32_t *bin_f;    // n_f scratch: bit b set = pushed into rotHist[b]
    int32_t *nmatches;  // 1
    // SearchByBoW(KF1, KF2) :522-655 (kf_kf != 0): "kf" = KF1, "f" = KF2
    int kf_kf;
    const uint8_t *f_has_mp;  // vpMapPoints2[idx2] && !isBad(); candidates without one are skipped (:572-577)
    int32_t *match_1;         // n_kf: vpMatches12 as KF2 feature indices
    int32_t *bin_1;           // n_kf scratch: rotHist bin + 1 of a matched KF1 feature
    int32_t *choice;          // n_queries scratch of the parallel stage B
};

// rotation consistency of both forms (:263-283, :632-652) by `nt` threads; returns the pushed entries it removed
__device__ __forceinline__ int bow_cull(const BowPairDev &P, const int *histo, int tid, int nt)
{
    const RotCull c = rot_cull(histo);
    if (!P.kf_kf)
        cull_by_mask(c.culled, P.bin_f, P.match_f, P.n_f, tid, nt, -1);
    else
        cull_by_bin1(c.culled, P.bin_1, P.match_1, P.n_kf, tid, nt, -1);
    return c.removed;
}

// stage A: grid = (max queries, pairs); one wave per query
__global__ __launch_bounds__(64) void bow_distances_kernel(const BowPairDev *__restrict__ pairs)
{
    const BowPairDev P = pairs[blockIdx.y];
    if ((int)blockIdx.x >= P.n_queries) return;
    const BowQuery q = P.queries[blockIdx.x];
    const Desc dKF = load_desc(P.desc_kf + (size_t)q.kf_idx * 32);
    for (int j = threadIdx.x; j < q.f_cnt; j += 64) {
        const int realIdxF = P.node_idx_f[q.f_beg + j];
        const int dist = hamming(dKF, load_desc(P.desc_f + (size_t)realIdxF * 32));
        Entry e;
        e.key = ((uint32_t)dist << 20) | (uint32_t)j;
        e.payload = (uint32_t)realIdxF;
        P.entries[q.ent_off + j] = e;
    }
}

// stage B: one wave per pair
__global__ __launch_bounds__(64) void bow_resolve_kernel(const BowPairDev *__restrict__ pairs, float nnratio,
                                                         int check_ori)
{
    extern __shared__ uint8_t taken[];  // vpMapPointMatches[j] != NULL
    __shared__ int histo[HISTO];
    const BowPairDev P = pairs[blockIdx.x];
    const int lane = threadIdx.x;
    if (!P.kf_kf) {
        for (int i = lane; i < P.n_f; i += 64) {
            P.match_f[i] = -1;
            P.bin_f[i] = 0;
            taken[i] = 0;
        }
    } else {
        for (int i = lane; i < P.n_f; i += 64) taken[i] = P.f_has_mp[i] ? 0 : 1;  // vbMatched2 || !pMP2 || isBad
        for (int i = lane; i < P.n_kf; i += 64) {
            P.match_1[i] = -1;
            P.bin_1[i] = 0;
        }
    }
    if (lane < HISTO) histo[lane] = 0;
    __syncthreads();
    int nmatches = 0;
    // queries are read 64 at a time (one per lane) and broadcast with shuffles; the entries of
    // the next two queries are prefetched, so no global-memory latency sits on the serial chain
    BowQuery qreg{0, 0, 0, 0};
    auto query_at = [&](int qi) {
        BowQuery r;
        const int src = qi & 63;
        r.kf_idx = __shfl(qreg.kf_idx, src);
        r.f_beg = __shfl(qreg.f_beg, src);
        r.f_cnt = __shfl(qreg.f_cnt, src);
        r.ent_off = __shfl(qreg.ent_off, src);
        return r;
    };
    auto fetch = [&](const BowQuery &qq) {
        Entry r{KEY_NONE, 0};
        if (lane < qq.f_cnt) r = P.entries[qq.ent_off + lane];
        return r;
    };
    Entry e1{KEY_NONE, 0}, e2{KEY_NONE, 0};
    BowQuery q1{0, 0, 0, 0}, q2{0, 0, 0, 0};
    if (P.n_queries > 0) {
        if (lane < P.n_queries) qreg = P.queries[lane];
        q1 = query_at(0);
        e1 = fetch(q1);
        if (P.n_queries > 1) {
            q2 = query_at(1);
            e2 = fetch(q2);
        }
    }
    for (int qi = 0; qi < P.n_queries; ++qi) {
        const BowQuery q = q1;
        Entry e = e1;
        q1 = q2;
        e1 = e2;
        if (qi + 2 < P.n_queries) {
            if (((qi + 2) & 63) == 0) {  // next chunk of queries (uniform branch)
                qreg = BowQuery{0, 0, 0, 0};
                if (qi + 2 + lane < P.n_queries) qreg = P.queries[qi + 2 + lane];
            }
            q2 = query_at(qi + 2);
            e2 = fetch(q2);
        }
        const WaveBest2 b = wave_best2(P.entries + q.ent_off, q.f_cnt, e, lane,
                                       [&](const Entry &c) { return !taken[c.payload]; });  // vpMapPointMatches[realIdxF] (:209)
        const int bestDist1 = key_dist(b.k1), bestDist2 = key_dist(b.k2);
        // (KF, F): bestDist1 <= TH_LOW (:237); (KF, KF): bestDist1 < TH_LOW (:599)
        const bool low = P.kf_kf ? bestDist1 < TH_LOW : bestDist1 <= TH_LOW;
        if (low && (float)bestDist1 < __fmul_rn(nnratio, (float)bestDist2)) {
            const int bestIdxF = (int)b.payload1();
            if (lane == 0) {
                taken[bestIdxF] = 1;
                int bin = 0;
                if (check_ori) {
                    bin = rot_bin(__fsub_rn(P.angle_kf[q.kf_idx], P.angle_f[bestIdxF]));
                    histo[bin]++;
                }
                if (!P.kf_kf) {
                    P.match_f[bestIdxF] = q.kf_idx;
                    if (check_ori) P.bin_f[bestIdxF] |= 1u << bin;
                } else {
                    P.match_1[q.kf_idx] = bestIdxF;
                    P.bin_1[q.kf_idx] = bin + 1;
                }
            }
            nmatches++;
            lds_fence();
        }
    }
    __syncthreads();
    if (check_ori) nmatches -= bow_cull(P, histo, lane, 64);
    if (lane == 0) *P.nmatches = nmatches;
}

// parallel stage B of both SearchByBoW forms (resolve_fixpoint): every match hides its frame feature (:209, :577)
__global__ __launch_bounds__(512) void bow_resolve_fix_kernel(const BowPairDev *__restrict__ pairs, float nnratio, int check_ori)
{
    constexpr int NT = 512;
    extern __shared__ int32_t fix_lds[];
    __shared__ int histo[HISTO];
    __shared__ int total;
    const BowPairDev P = pairs[blockIdx.x];
    const int tid = threadIdx.x;
    if (!P.kf_kf) {
        for (int i = tid; i < P.n_f; i += NT) {
            P.match_f[i] = -1;
            P.bin_f[i] = 0;
        }
    } else {
        for (int i = tid; i < P.n_kf; i += NT) {
            P.match_1[i] = -1;
            P.bin_1[i] = 0;
        }
    }
    if (tid < HISTO) histo[tid] = 0;
    if (tid == 0) total = 0;
    resolve_fixpoint<NT>(
        P.n_f, P.n_queries, fix_lds, P.choice, 0xffffffffu,
        [&](int i) { return (P.kf_kf && !P.f_has_mp[i]) ? -1 : INT_MAX; },   // vbMatched2 || !pMP2 || isBad (:572-577)
        [&](int q, int &cnt) {
            const BowQuery bq = P.queries[q];
            cnt = bq.f_cnt;
            return (const Entry *)(P.entries + bq.ent_off);
        },
        [&](int, const Best2 &b) {
            const int bestDist1 = key_dist(b.k1), bestDist2 = key_dist(b.k2);
            // (KF, F): bestDist1 <= TH_LOW (:237); (KF, KF): bestDist1 < TH_LOW (:599)
            const bool low = P.kf_kf ? bestDist1 < TH_LOW : bestDist1 <= TH_LOW;
            return (low && (float)bestDist1 < __fmul_rn(nnratio, (float)bestDist2)) ? (int)b.p1 : -1;
        },
        [&](int) { return true; });
    int cnt = 0;
    for (int q = tid; q < P.n_queries; q += NT) {
        const int c = P.choice[q];
        if (c < 0) continue;
        const int kf = P.queries[q].kf_idx;
        int bin = 0;
        if (check_ori) {
            bin = rot_bin(__fsub_rn(P.angle_kf[kf], P.angle_f[c]));
            atomicAdd(&histo[bin], 1);
        }
        if (!P.kf_kf) {   // a frame feature is chosen by at most one query
            P.match_f[c] = kf;
            if (check_ori) P.bin_f[c] = 1u << bin;
        } else {
            P.match_1[kf] = c;
            P.bin_1[kf] = bin + 1;
        }
        ++cnt;
    }
    int nmatches = block_total(&total, cnt);
    if (check_ori) nmatches -= bow_cull(P, histo, tid, NT);
    if (tid == 0) *P.nmatches = nmatches;
}

// ---------------------------------------------------------------------------------------------
// SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo)  :657-823.
// vbMatched2 is declared but never set by the reference, so the KF1 features are independent: one
// wave per query, lanes over the KF2 bucket.  The sequential rule "dist <= bestDist and the geometry
// holds -> take it" (:728, :741-745) selects the smallest distance and, among equals, the LAST
// candidate visited: key = dist << 20 | (0xFFFFF - position).
// ---------------------------------------------------------------------------------------------
struct TriQuery {
    int32_t idx1, f_beg, f_cnt;
};

struct TriPairDev {
    int n1, n2, n_queries, only_stereo;
    const uint8_t *desc1, *desc2, *has_mp2;
    const float *x1, *y1, *angle1, *u_right1, *x2, *y2, *angle2, *u_right2;
    const int32_t *octave2;
    const float *scale_factors2, *level_sigma2_2;
    float F12[9], ex, ey;
    const int32_t *node_idx2;
    const TriQuery *queries;
    int32_t *match12;   // n1
    int32_t *nmatches;
};

__global__ __launch_bounds__(64) void triang_match_kernel(const TriPairDev *__restrict__ pairs)
{
    const TriPairDev &P = pairs[blockIdx.y];
    if ((int)blockIdx.x >= P.n_queries) return;
    const TriQuery q = P.queries[blockIdx.x];
    const int lane = threadIdx.x;
    const Desc d1 = load_desc(P.desc1 + (size_t)q.idx1 * 32);
    const float kx = P.x1[q.idx1], ky = P.y1[q.idx1];
    const bool bStereo1 = P.u_right1[q.idx1] >= 0;
    const EpiLine line = epi_line(P.F12, kx, ky);
    uint32_t key = KEY_NONE, pay = 0;
    for (int j = lane; j < q.f_cnt; j += 64) {
        const int idx2 = P.node_idx2[q.f_beg + j];
        if (P.has_mp2[idx2]) continue;                       // :723
        const bool bStereo2 = P.u_right2[idx2] >= 0;
        if (P.only_stereo && !bStereo2) continue;
        const int dist = hamming(d1, load_desc(P.desc2 + (size_t)idx2 * 32));
        if (dist > TH_LOW) continue;                         // :734 (bestDist never exceeds TH_LOW)
        const int oct = P.octave2[idx2];
        if (!epi_admits(line, P.x2[idx2], P.y2[idx2], !bStereo1 && !bStereo2, P.ex, P.ey, P.scale_factors2[oct],
                        P.level_sigma2_2[oct]))
            continue;
        const uint32_t k = ((uint32_t)dist << 20) | (0xFFFFFu - (uint32_t)j);
        if (k < key) {
            key = k;
            pay = (uint32_t)idx2;
        }
    }
    uint32_t k1 = key, k2 = KEY_NONE;
    wave_min2(k1, k2);
    if (k1 != KEY_NONE) {
        const unsigned long long own = __ballot(key == k1);
        const int best = (int)read_owner(pay, own);
        if (lane == 0) P.match12[q.idx1] = best;
    }
}

__global__ __launch_bounds__(64) void triang_finish_kernel(const TriPairDev *__restrict__ pairs, int check_ori)
{
    const TriPairDev &P = pairs[blockIdx.x];
    triang_finish_body(P.n1, P.angle1, P.angle2, P.match12, P.nmatches, check_ori);
}

// ---------------------------------------------------------------------------------------------
// MapPoint::ComputeDistinctiveDescriptors  src/MapPoint.cc:275-340, batched over map points: one wave
// per point, lane = row of the N x N distance matrix.  The row median vDists[0.5*(N-1)] is found by
// bisection on the value (distances are 0..256) instead of sorting; the first row with the smallest
// median wins (strict '<', :326-330).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void distinctive_kernel(int n_points, const int32_t *__restrict__ off,
                                                         const uint8_t *__restrict__ desc, int32_t *__restrict__ best)
{
    const int p = blockIdx.x;
    if (p >= n_points) return;
    const int lane = threadIdx.x;
    const int beg = off[p], N = off[p + 1] - off[p];
    if (N <= 0) {
        if (lane == 0) best[p] = -1;
        return;
    }
    const uint8_t *d = desc + (size_t)beg * 32;
    const int kth = (N - 1) / 2;  // (int)(0.5 * (N - 1))
    uint32_t key = KEY_NONE;
    for (int i = lane; i < N; i += 64) {
        const Desc di = load_desc(d + (size_t)i * 32);
        int lo = 0, hi = 256;
        while (lo < hi) {  // smallest v with #{j : dist(i, j) <= v} >= kth + 1
            const int mid = (lo + hi) >> 1;
            int c = 0;
            for (int j = 0; j < N; ++j) c += (j == i ? 0 : hamming(di, load_desc(d + (size_t)j * 32))) <= mid;
            if (c >= kth + 1) hi = mid; else lo = mid + 1;
        }
        const uint32_t k = ((uint32_t)lo << 20) | (uint32_t)i;
        key = min(key, k);
    }
    uint32_t k1 = key, k2 = KEY_NONE;
    wave_min2(k1, k2);
    if (lane == 0) best[p] = (int32_t)(k1 & 0xFFFFFu);
}

__global__ __launch_bounds__(64) void proj_mp_entries_kernel(FrameDev F, ProjMpDev P, float th, QuerySlot *slots,
                                                             Entry *pool, int32_t *pool_used, int pool_cap, int phase = 0)
{
    proj_mp_entries_body(F, P, th, slots, pool, pool_used, pool_cap, blockIdx.x, 0, phase);
}

// the scan between the two passes of the two-pass form: one problem, one workgroup
__global__ __launch_bounds__(256) void proj_mp_scan_slots_kernel(QuerySlot *__restrict__ slots, const int32_t *__restrict__ nq_of, int nq_cap,
                                                                 int share, int32_t *__restrict__ overflow)
{
    scan_slots_body(slots, nq_of, nq_cap, share, overflow);
}

__global__ __launch_bounds__(64) void proj_mp_resolve_kernel(FrameDev F, ProjMpDev P, float nnratio,
                                                             const QuerySlot *__restrict__ slots,
                                                             const Entry *__restrict__ pool, int32_t *match_f,
                                                             int32_t *nmatches_out)
{
    proj_mp_resolve_body(F, P, nnratio, slots, pool, match_f, nmatches_out);
}

__global__ __launch_bounds__(1024) void proj_mp_resolve_fix_kernel(FrameDev F, ProjMpDev P, float nnratio,
                                                                   const QuerySlot *__restrict__ slots,
                                                                   const Entry *__restrict__ pool, int32_t *match_f,
                                                                   int32_t *nmatches_out, int32_t *choice)
{
    proj_mp_resolve_fix_body<1024>(F, P, nnratio, slots, pool, match_f, nmatches_out, choice);
}

// batched form: problem = blockIdx.y (stage A) / blockIdx.x (stage B); one entry pool shared through pool_used
struct ProjMpItem {
    FrameDev F;
    ProjMpDev P;
    QuerySlot *slots;
    int32_t *match_f, *nmatches, *choice;
    int32_t *pool_used;        // this problem's entry counter
    int32_t pool_base, pool_cap;
};
__global__ __launch_bounds__(64) void proj_mp_entries_batch_kernel(const ProjMpItem *__restrict__ items, float th, Entry *pool)
{
    const ProjMpItem &it = items[blockIdx.y];
    if ((int)blockIdx.x >= it.P.n_mp) return;
    proj_mp_entries_body(it.F, it.P, th, it.slots, pool, it.pool_used, it.pool_cap, blockIdx.x, it.pool_base);
}
__global__ __launch_bounds__(64) void proj_mp_resolve_batch_kernel(const ProjMpItem *__restrict__ items, float nnratio,
                                                                   const Entry *__restrict__ pool)
{
    const ProjMpItem &it = items[blockIdx.x];
    proj_mp_resolve_body(it.F, it.P, nnratio, it.slots, pool, it.match_f, it.nmatches);
}

__global__ __launch_bounds__(256) void proj_mp_resolve_fix_batch_kernel(const ProjMpItem *__restrict__ items, float nnratio,
                                                                        const Entry *__restrict__ pool)
{
    const ProjMpItem &it = items[blockIdx.x];
    proj_mp_resolve_fix_body<256>(it.F, it.P, nnratio, it.slots, pool, it.match_f, it.nmatches, it.choice);
}

__global__ __launch_bounds__(64) void proj_last_entries_kernel(FrameDev F, ProjLastDev P, float th, int mono,
                                                               QuerySlot *slots, Entry *pool, int32_t *pool_used,
                                                               int pool_cap)
{
    proj_last_entries_body(F, P, th, mono, slots, pool, pool_used, pool_cap, blockIdx.x);
}

__global__ __launch_bounds__(64) void proj_last_resolve_kernel(FrameDev F, ProjLastDev P, int check_ori,
                                                               const QuerySlot *__restrict__ slots,
                                                               const Entry *__restrict__ pool, int32_t *match_f,
                                                               uint32_t *bin_f, int32_t *nmatches_out)
{
    extern __shared__ uint8_t state[];
    __shared__ int histo[HISTO];
    const int lane = threadIdx.x;
    for (int i = lane; i < F.n_f; i += 64) {
        state[i] = F.f_mp_state[i];
        match_f[i] = -1;
        bin_f[i] = 0;
    }
    if (lane < HISTO) histo[lane] = 0;
    __syncthreads();
    int nmatches = 0;
    SlotStream Q;
    Q.init(slots, pool, P.n_last, lane);
    for (int i = 0; i < P.n_last; i++) {
        QuerySlot s;
        Entry e;
        Q.next(i, s, e);
        if (s.cnt <= 0) continue;
        const Pick b = pick_best2(pool + s.ent_off, s.cnt, e, state, lane);
        if (key_dist(b.k1) <= TH_HIGH) {
            if (lane == 0) {
                match_f[b.idx1] = i;
                state[b.idx1] = P.has_obs[i] ? 2 : 1;
                if (check_ori) {
                    const int bin = rot_bin(__fsub_rn(P.last_angle[i], F.kp_angle[b.idx1]));
                    // a feature can be pushed several times when a zero-observation point is
                    // overwritten (:1432): it is reset if ANY of its bins is culled, and nmatches
                    // drops once per pushed entry (:1459-1460)
                    histo[bin]++;
                    bin_f[b.idx1] |= 1u << bin;
                }
            }
            nmatches++;
            lds_fence();
        }
    }
    __syncthreads();
    if (check_ori) {
        const RotCull c = rot_cull(histo);
        cull_by_mask(c.culled, bin_f, match_f, F.n_f, lane, 64, -2);  // set to NULL (:1459)
        nmatches -= c.removed;
    }
    if (lane == 0) *nmatches_out = nmatches;
}

__global__ __launch_bounds__(1024) void proj_last_resolve_fix_kernel(FrameDev F, ProjLastDev P, int check_ori,
                                                                     const QuerySlot *__restrict__ slots,
                                                                     const Entry *__restrict__ pool, int32_t *match_f,
                                                                     uint32_t *bin_f, int32_t *nmatches_out, int32_t *choice)
{
    proj_last_resolve_fix_body<1024>(F, P, check_ori, slots, pool, match_f, bin_f, nmatches_out, choice);
}

__global__ __launch_bounds__(256) void assign_grid_kernel(int n, const float *__restrict__ kp_x, const float *__restrict__ kp_y,
                                                          float min_x, float min_y, float gwi, float ghi,
                                                          int32_t *__restrict__ grid_off, int32_t *__restrict__ grid_idx)
{
    assign_grid_body(n, kp_x, kp_y, min_x, min_y, gwi, ghi, grid_off, grid_idx);
}

// Frame::ComputeStereoFromRGBD (src/Frame.cc:672-693)
__global__ void stereo_from_rgbd_kernel(int n, const float *__restrict__ kp_x, const float *__restrict__ kp_y,
                                        const float *__restrict__ kpun_x, const float *__restrict__ depth_img, int stride,
                                        float mbf, float *__restrict__ u_right, float *__restrict__ depth)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float d = depth_img[(size_t)(int)kp_y[i] * stride + (int)kp_x[i]];   // imDepth.at<float>(v, u): indices truncate
    float ur = -1.0f, dp = -1.0f;
    if (d > 0) {
        dp = d;
        ur = __fsub_rn(kpun_x[i], __fdiv_rn(mbf, d));
    }
    u_right[i] = ur;
    depth[i] = dp;
}

// Frame::isInFrustum (src/Frame.cc:298-354) for a batch of map points: one thread per point
__global__ void is_in_frustum_kernel(ProjGenDev P, float min_x, float max_x, float min_y, float max_y, int n_levels,
                                     float cos_limit, uint8_t *in_view, float *proj_x, float *proj_y, float *proj_xr,
                                     int32_t *pred_level, float *view_cos)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n_pts) return;
    uint8_t ok = 0;
    float u = 0, v = 0, ur = 0, vc = 0;
    int lvl = 0;
    const float pw[3] = {P.pos[3 * i], P.pos[3 * i + 1], P.pos[3 * i + 2]};
    float pc[3];
    xform3(P.R, P.t, pw, pc);
    if (!(pc[2] < 0.0f)) {
        const float invz = __fdiv_rn(1.0f, pc[2]);
        const float uu = __fadd_rn(__fmul_rn(__fmul_rn(P.fx, pc[0]), invz), P.cx);
        const float vv = __fadd_rn(__fmul_rn(__fmul_rn(P.fy, pc[1]), invz), P.cy);
        if (!(uu < min_x || uu > max_x) && !(vv < min_y || vv > max_y)) {
            const float PO[3] = {__fsub_rn(pw[0], P.Ow[0]), __fsub_rn(pw[1], P.Ow[1]), __fsub_rn(pw[2], P.Ow[2])};
            const float dist = norm3d(PO);
            if (!(dist < __fmul_rn(0.8f, P.min_dist[i]) || dist > __fmul_rn(1.2f, P.max_dist[i]))) {   // Get{Min,Max}DistanceInvariance()
                const double dot = __dadd_rn(__dadd_rn(__dmul_rn((double)PO[0], (double)P.normal[3 * i]),
                                                       __dmul_rn((double)PO[1], (double)P.normal[3 * i + 1])),
                                             __dmul_rn((double)PO[2], (double)P.normal[3 * i + 2]));
                const float viewCos = (float)__ddiv_rn(dot, (double)dist);
                if (!(viewCos < cos_limit)) {
                    const float ratio = __fdiv_rn(P.max_dist[i], dist);
                    const float lg = (float)log((double)ratio);
                    int nScale = (int)ceilf(__fdiv_rn(lg, P.log_scale_factor));
                    if (nScale < 0) nScale = 0;
                    else if (nScale >= n_levels) nScale = n_levels - 1;
                    ok = 1;
                    u = uu;
                    v = vv;
                    ur = __fsub_rn(uu, __fmul_rn(P.bf, invz));
                    lvl = nScale;
                    vc = viewCos;
                }
            }
        }
    }
    in_view[i] = ok;
    proj_x[i] = u;
    proj_y[i] = v;
    proj_xr[i] = ur;
    pred_level[i] = lvl;
    view_cos[i] = vc;
}

// modes 0, 1, 3: one wave per point, no shared state
__global__ __launch_bounds__(64) void projgen_best_kernel(FrameDev F, ProjGenDev P, int thr, int32_t *best_idx,
                                                          int32_t *best_dist)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    int bi = -1, bd = 256;
    const ProjSetup S = proj_gen_setup(F, P, i);
    if (S.ok) {
        const Window w = window_cells(F, S.u, S.v, S.radius);
        if (w.ok) {
            uint32_t pay;
            const uint32_t k = window_best(F, P, w, load_desc(P.desc + (size_t)i * 32), S, lane, pay);
            if (k != KEY_NONE && (int)(k >> 20) <= thr) {
                bi = (int)pay;
                bd = (int)(k >> 20);
            }
        }
    }
    if (lane == 0) {
        best_idx[i] = bi;
        best_dist[i] = bd;
    }
}

// SearchBySim3 agreement (:1306-1323)
__global__ void sim3_agree_kernel(const int32_t *__restrict__ vn1, const int32_t *__restrict__ vn2, int n1, int n2,
                                  int32_t *match12, int32_t *nfound)
{
    const int i1 = blockIdx.x * blockDim.x + threadIdx.x;
    if (i1 >= n1) return;
    int m = -1;
    const int idx2 = vn1[i1];
    if (idx2 >= 0 && idx2 < n2 && vn2[idx2] == i1) m = idx2;
    match12[i1] = m;
    if (m >= 0) atomicAdd(nfound, 1);
}

// modes 2, 4 stage A: entries of the window into the pool
__global__ __launch_bounds__(64) void projgen_entries_kernel(FrameDev F, ProjGenDev P, QuerySlot *slots, Entry *pool,
                                                             int32_t *pool_used, int pool_cap)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    QuerySlot s{0, 0};
    const ProjSetup S = proj_gen_setup(F, P, i);
    if (S.ok) {
        const Window w = window_cells(F, S.u, S.v, S.radius);
        if (w.ok) {
            const int pop = window_population(F, w, lane);
            if (pop > 0) s = claim_slot(slots, i, P.n_pts, pop, 0, pool_cap, 0, pool_used, lane);
            if (s.cnt > 0) {
                // mode 2: levels [pred-1, pred] tested per candidate (:379-382) == the level filter of the
                // Frame version; mode 4: GetFeaturesInArea(u, v, radius, pred-1, pred+1) (:1537).  A level
                // window starting at 0 or below disables only the lower test, like bCheckLevels (Frame.cc:379).
                const int lo = S.level - 1, hi = P.mode == 4 ? S.level + 1 : S.level;
                window_entries(F, w, load_desc(P.desc + (size_t)i * 32), S.u, S.v, S.radius, lo, hi, 0.0f,
                               __builtin_huge_valf(), lane, pool + s.ent_off);
            }
        }
    }
    if (lane == 0) slots[i] = s;
}

// modes 2, 4 stage B: the reference's greedy loop over the points
__global__ __launch_bounds__(64) void projgen_resolve_kernel(FrameDev F, ProjGenDev P, int thr, int check_ori,
                                                             const QuerySlot *__restrict__ slots,
                                                             const Entry *__restrict__ pool, int32_t *match_f,
                                                             int32_t *bin_f, int32_t *nmatches_out)
{
    extern __shared__ uint8_t state[];  // != 0: vpMatched[idx] / mvpMapPoints[idx] is set
    __shared__ int histo[HISTO];
    const int lane = threadIdx.x;
    for (int i = lane; i < F.n_f; i += 64) {
        state[i] = F.f_mp_state[i] != 0;
        match_f[i] = -1;
        bin_f[i] = 0;
    }
    if (lane < HISTO) histo[lane] = 0;
    __syncthreads();
    int nmatches = 0;
    SlotStream Q;
    Q.init(slots, pool, P.n_pts, lane);
    for (int i = 0; i < P.n_pts; i++) {
        QuerySlot s;
        Entry e;
        Q.next(i, s, e);
        if (s.cnt <= 0) continue;
        const Pick b = pick_best2(pool + s.ent_off, s.cnt, e, state, lane, true);
        if (key_dist(b.k1) <= thr) {
            if (lane == 0) {
                match_f[b.idx1] = i;
                state[b.idx1] = 1;
                if (check_ori) {
                    const int bin = rot_bin(__fsub_rn(P.q_angle[i], F.kp_angle[b.idx1]));
                    histo[bin]++;
                    bin_f[b.idx1] = bin + 1;
                }
            }
            nmatches++;
            lds_fence();
        }
    }
    __syncthreads();
    if (check_ori) {
        const RotCull c = rot_cull(histo);
        cull_by_bin1(c.culled, bin_f, match_f, F.n_f, lane, 64, -2);  // set to NULL (:1589)
        nmatches -= c.removed;
    }
    if (lane == 0) *nmatches_out = nmatches;
}

// modes 2, 4 parallel stage B (resolve_fixpoint): every match hides its feature, so a feature has one owner
__global__ __launch_bounds__(1024) void projgen_resolve_fix_kernel(FrameDev F, ProjGenDev P, int thr, int check_ori,
                                                                   const QuerySlot *__restrict__ slots,
                                                                   const Entry *__restrict__ pool, int32_t *match_f,
                                                                   int32_t *bin_f, int32_t *nmatches_out, int32_t *choice)
{
    constexpr int NT = 1024;
    extern __shared__ int32_t fix_lds[];
    __shared__ int histo[HISTO];
    __shared__ int total;
    const int tid = threadIdx.x;
    for (int i = tid; i < F.n_f; i += NT) {
        match_f[i] = -1;
        bin_f[i] = 0;
    }
    if (tid < HISTO) histo[tid] = 0;
    if (tid == 0) total = 0;
    resolve_fixpoint<NT>(
        F.n_f, P.n_pts, fix_lds, choice, 0xffffffu, [&](int i) { return F.f_mp_state[i] != 0 ? -1 : INT_MAX; },
        SlotEntries{slots, pool},
        [&](int, const Best2 &b) { return (b.k1 != KEY_NONE && (int)(b.k1 >> 20) <= thr) ? (int)(b.p1 & 0xffffffu) : -1; },
        [&](int) { return true; });
    int cnt = 0;
    for (int q = tid; q < P.n_pts; q += NT) {
        const int c = choice[q];
        if (c < 0) continue;
        match_f[c] = q;
        if (check_ori) {
            const int bin = rot_bin(__fsub_rn(P.q_angle[q], F.kp_angle[c]));
            atomicAdd(&histo[bin], 1);
            bin_f[c] = bin + 1;
        }
        ++cnt;
    }
    int nmatches = block_total(&total, cnt);
    if (check_ori) {
        const RotCull c = rot_cull(histo);
        cull_by_bin1(c.culled, bin_f, match_f, F.n_f, tid, NT, -2);  // set to NULL (:1589)
        nmatches -= c.removed;
    }
    if (tid == 0) *nmatches_out = nmatches;
}

// ---------------------------------------------------------------------------------------------
// SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)  :405-520 (monocular bootstrap).
// Stage A: one wave per level-0 F1 feature, window of F2 around vbPrevMatched[i1] restricted to level 0.
// Stage B: the greedy loop with its two per-F2 tables in LDS: vMatchedDistance (a candidate is skipped
// while an earlier match holds it with a distance <= ours, :443) and vnMatches21 (a better later match
// steals the F2 feature and un-matches its previous owner, :462-466).
// ---------------------------------------------------------------------------------------------
struct InitDev {
    int n1;
    const uint8_t *desc1;
    const int32_t *octave1;
    const float *angle1, *prev_xy;
    float window;
};

__global__ __launch_bounds__(64) void init_entries_kernel(FrameDev F2, InitDev P, QuerySlot *slots, Entry *pool,
                                                          int32_t *pool_used, int pool_cap)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    QuerySlot s{0, 0};
    if (P.octave1[i] <= 0) {  // level1 > 0 -> continue (:421-423)
        const float x = P.prev_xy[2 * i], y = P.prev_xy[2 * i + 1];
        const Window w = window_cells(F2, x, y, P.window);
        if (w.ok) {
            const int pop = window_population(F2, w, lane);
            if (pop > 0) s = claim_slot(slots, i, P.n1, pop, 0, pool_cap, 0, pool_used, lane);
            if (s.cnt > 0) {
                const int lvl = P.octave1[i];
                window_entries(F2, w, load_desc(P.desc1 + (size_t)i * 32), x, y, P.window, lvl, lvl, 0.0f,
                               __builtin_huge_valf(), lane, pool + s.ent_off);
            }
        }
    }
    if (lane == 0) slots[i] = s;
}

__global__ __launch_bounds__(64) void init_resolve_kernel(FrameDev F2, InitDev P, float nnratio, int check_ori,
                                                          const QuerySlot *__restrict__ slots,
                                                          const Entry *__restrict__ pool, int32_t *match12,
                                                          int32_t *bin_1, int32_t *nmatches_out)
{
    extern __shared__ uint16_t init_lds[];
    uint16_t *md = init_lds;               // vMatchedDistance (0xFFFF = INT_MAX)
    uint16_t *m21 = init_lds + F2.n_f;     // vnMatches21 + 1 (0 = -1)
    __shared__ int histo[HISTO];
    const int lane = threadIdx.x;
    for (int i = lane; i < F2.n_f; i += 64) {
        md[i] = 0xFFFFu;
        m21[i] = 0;
    }
    for (int i = lane; i < P.n1; i += 64) {
        match12[i] = -1;
        bin_1[i] = 0;
    }
    if (lane < HISTO) histo[lane] = 0;
    __syncthreads();
    int nmatches = 0;
    SlotStream Q;
    Q.init(slots, pool, P.n1, lane);
    for (int i1 = 0; i1 < P.n1; i1++) {
        QuerySlot s;
        Entry e;
        Q.next(i1, s, e);
        if (s.cnt <= 0) continue;
        const WaveBest2 b = wave_best2(pool + s.ent_off, s.cnt, e, lane, [&](const Entry &c) {   // !(vMatchedDistance[i2] <= dist)
            return c.key != KEY_NONE && (uint32_t)md[c.payload & 0xffffffu] > (c.key >> 20);
        });
        if (b.k1 == KEY_NONE) continue;
        const int bestDist = (int)(b.k1 >> 20);
        const float second = b.k2 == KEY_NONE ? 2147483648.0f : (float)(int)(b.k2 >> 20);  // (float)INT_MAX
        if (bestDist <= TH_LOW && (float)bestDist < __fmul_rn(second, nnratio)) {
            const int bestIdx2 = (int)(b.payload1() & 0xffffffu);
            const int prev = (int)m21[bestIdx2];
            if (lane == 0) {
                if (prev > 0) match12[prev - 1] = -1;
                match12[i1] = bestIdx2;
                m21[bestIdx2] = (uint16_t)(i1 + 1);
                md[bestIdx2] = (uint16_t)bestDist;
                if (check_ori) {
                    const int bin = rot_bin(__fsub_rn(P.angle1[i1], F2.kp_angle[bestIdx2]));
                    histo[bin]++;
                    bin_1[i1] = bin + 1;
                }
            }
            nmatches += prev > 0 ? 0 : 1;  // nmatches-- for the stolen match, nmatches++ for the new one
            lds_fence();
        }
    }
    __threadfence_block();
    __syncthreads();
    if (check_ori) {
        // a stolen match is already -1 and its histogram entry stays: count the matches actually reset (:497-501), not the entries
        const int drop = cull_by_bin1(rot_cull(histo).culled, bin_1, match12, P.n1, lane, 64, -1);
        nmatches -= wave_sum_i32(drop);
    }
    if (lane == 0) *nmatches_out = nmatches;
}

}  // namespace aos2

using namespace aos2;

// LDS budget of the fixed-point resolve kernels (two int32 copies of B[n_f]): default dynamic-LDS limit
constexpr size_t kFixLdsBytes = 44 * 1024;   // + the 16 KB overflow arena of resolve_fixpoint_impl: within the 64 KB of a workgroup

namespace aos2 {

int matcher_init(aos2_matcher *m)
{
    int st = bind_device(m->device);
    if (st) return st;
    if (m->dev_ready) return AOS2_OK;
    if (int st_ = stream_create(&m->stream, false)) return st_;
    for (auto &e : m->ev) AOS2_HIP_CHECK(hipEventCreate(&e));
    {
        const char *v = getenv("AOS2_SERIAL_RESOLVE");
        m->serial_resolve = v && atoi(v) != 0;
    }
    m->dev_ready = true;
    return AOS2_OK;
}

// stage B of a search over a frame of n_f features: the parallel fixed-point kernel while its two LDS copies of B[n_f] fit,
// else (or with AOS2_SERIAL_RESOLVE=1) the one-wave sequential loop
static bool use_fix_resolve(const aos2_matcher *m, int n_f) { return (size_t)n_f * 8 <= kFixLdsBytes && !m->serial_resolve; }

// room for `entries` candidate entries in the handle's pool -> pool.  Entry offsets are 32-bit: 2^31 entries = 16 GiB of the
// device's 288 GB; beyond that AOS2_ERR_CAPACITY, below it only the allocation itself can fail.
static int pool_reserve(aos2_matcher *m, size_t entries, const char *what, Entry *&pool)
{
    if (entries > ((size_t)1 << 31) - 2) {
        set_error("%s: %zu candidate entries exceed the pool's index range", what, entries);
        return AOS2_ERR_CAPACITY;
    }
    if (int st = m->pool.alloc(entries + 1)) return st;
    pool = reinterpret_cast<Entry *>(m->pool.p);
    return AOS2_OK;
}

// stages the frame's arrays and describes them in F (whose pointer fields the arena fills: F stays where it is until then)
static void frame_dev(Arena &A, const aos2_frame_view_t *f, FrameDev &F)
{
    const size_t n = (size_t)f->n_f;
    F = FrameDev{};
    F.n_f = f->n_f;
    F.n_levels = f->n_levels;
    A.in(F.desc_f, f->desc_f, n * 32);
    A.in(F.kp_x, f->kp_x, n * 4);
    A.in(F.kp_y, f->kp_y, n * 4);
    A.in(F.kp_angle, f->kp_angle, n * 4);
    A.in(F.u_right, f->u_right, n * 4);
    A.in(F.scale_factors, f->scale_factors, (size_t)f->n_levels * 4);
    A.in(F.kp_octave, f->kp_octave, n * 4);
    A.in(F.grid_off, f->grid_off, (size_t)(GRID_COLS * GRID_ROWS + 1) * 4);
    A.in(F.grid_idx, f->grid_idx, (size_t)f->grid_off[GRID_COLS * GRID_ROWS] * 4);
    A.in(F.f_mp_state, f->f_mp_state, n);
    F.min_x = f->min_x; F.min_y = f->min_y; F.max_x = f->max_x; F.max_y = f->max_y;
    F.grid_w_inv = f->grid_w_inv; F.grid_h_inv = f->grid_h_inv;
}

static int check_frame(const aos2_frame_view_t *f)
{
    if (!f || f->n_f < 0 || !f->grid_off || (f->n_f > 0 && (!f->desc_f || !f->kp_x || !f->kp_y || !f->kp_octave ||
        !f->kp_angle || !f->u_right || !f->f_mp_state)) || !f->scale_factors || f->n_levels <= 0) {
        set_error("bad frame view");
        return AOS2_ERR_ARG;
    }
    if (f->n_f > 60000) {
        set_error("n_f %d exceeds the LDS state table (60000)", f->n_f);
        return AOS2_ERR_ARG;
    }
    // the arrays that become device-side indices: mGrid as CSR (monotone offsets, every listed feature exists) and the
    // pyramid levels (they index scale_factors[] / level_sigma2[])
    constexpr int NC = GRID_COLS * GRID_ROWS;
    if (f->grid_off[0] != 0) {
        set_error("bad frame view: grid_off[0] = %d", f->grid_off[0]);
        return AOS2_ERR_ARG;
    }
    for (int c = 0; c < NC; ++c)
        if (f->grid_off[c + 1] < f->grid_off[c]) {
            set_error("bad frame view: grid_off decreases at cell %d", c);
            return AOS2_ERR_ARG;
        }
    const int listed = f->grid_off[NC];
    if (listed > f->n_f || (listed > 0 && !f->grid_idx)) {
        set_error("bad frame view: the grid lists %d features of %d%s", listed, f->n_f, f->grid_idx ? "" : " (grid_idx is NULL)");
        return AOS2_ERR_ARG;
    }
    for (int i = 0; i < listed; ++i)
        if ((unsigned)f->grid_idx[i] >= (unsigned)f->n_f) {
            set_error("bad frame view: grid_idx[%d] = %d is not a feature", i, f->grid_idx[i]);
            return AOS2_ERR_ARG;
        }
    for (int i = 0; i < f->n_f; ++i)
        if ((unsigned)f->kp_octave[i] >= (unsigned)f->n_levels) {
            set_error("bad frame view: kp_octave[%d] = %d outside the %d pyramid levels", i, f->kp_octave[i], f->n_levels);
            return AOS2_ERR_ARG;
        }
    return AOS2_OK;
}

// levels handed in per query (mnTrackScaleLevel, LastFrame octaves, keyframe octaves): they index the frame's scale tables
// (only of the queries the reference reads them for: mnTrackScaleLevel of a point that is not in view, or the octave of a
// LastFrame feature without a usable map point, may be stale / uninitialised there -- `live` = that gate, NULL = all)
static int check_levels(const int32_t *lv, int n, int n_levels, const char *what, const uint8_t *live = nullptr)
{
    if (n > 0 && !lv) {
        set_error("%s is NULL", what);
        return AOS2_ERR_ARG;
    }
    for (int i = 0; i < n; ++i)
        if ((!live || live[i]) && (unsigned)lv[i] >= (unsigned)n_levels) {
            set_error("%s[%d] = %d outside the %d pyramid levels", what, i, lv[i], n_levels);
            return AOS2_ERR_ARG;
        }
    return AOS2_OK;
}

// merge-join of two FeatureVectors (SearchByBoW :181-258, SearchForTriangulation :691-772): for every vocabulary node
// both sides hold, each(i1, b0, bc) for the side-1 features i1 under it, in node order; b0 / bc = where side 2 lists its
// features under that node (node_idx2[b0 .. b0 + bc)).  The visiting order is the reference's.  False: a side-1 feature
// index outside [0, n1).
template <class Each>
static bool fv_join(int n_nodes1, const int32_t *id1, const int32_t *off1, const int32_t *idx1, int n1, int n_nodes2,
                    const int32_t *id2, const int32_t *off2, Each each)
{
    int i1 = 0, i2 = 0;
    while (i1 < n_nodes1 && i2 < n_nodes2) {
        const int a = id1[i1], b = id2[i2];
        if (a == b) {
            const int b0 = off2[i2], bc = off2[i2 + 1] - b0;
            for (int k = off1[i1]; k < off1[i1 + 1]; ++k) {
                if (idx1[k] < 0 || idx1[k] >= n1) return false;
                each(idx1[k], b0, bc);
            }
            i1++;
            i2++;
        } else if (a < b) {
            while (i1 < n_nodes1 && id1[i1] < b) i1++;  // lower_bound
        } else {
            while (i2 < n_nodes2 && id2[i2] < a) i2++;
        }
    }
    return true;
}

}  // namespace aos2

extern "C" {

int aos2_matcher_create(float nnratio, int check_orientation, int device, aos2_matcher_t **out)
{
    if (!out) return AOS2_ERR_ARG;
    aos2_matcher *m = new aos2_matcher();
    m->nnratio = nnratio;
    m->check_ori = check_orientation ? 1 : 0;
    m->device = device;
    *out = m;
    return AOS2_OK;
}

void aos2_matcher_destroy(aos2_matcher_t *m)
{
    if (!m) return;
    if (m->dev_ready) {
        (void)hipSetDevice(m->device);
        (void)hipStreamSynchronize(m->stream);
        m->arena.release();
        m->h_in.release();
        m->h_out.release();
        m->part.release();
        m->pool.release();
        m->fr_angle.release();
        m->fr_host.release();
        for (auto &e : m->ev) (void)hipEventDestroy(e);
        (void)hipStreamDestroy(m->stream);
    }
    delete m;
}

float aos2_matcher_last_device_ms(const aos2_matcher_t *m) { return m ? m->last_ms : 0.f; }

int aos2_descriptor_distance(const uint8_t *a, const uint8_t *b)
{
    int dist = 0;
    for (int i = 0; i < 4; ++i) {
        uint64_t x, y;
        memcpy(&x, a + 8 * i, 8);
        memcpy(&y, b + 8 * i, 8);
        dist += __builtin_popcountll(x ^ y);
    }
    return dist;
}

static int hamming_run(aos2_matcher *m, const uint8_t *d_q, int nq, const uint8_t *d_t, int nt, int32_t *d_bi,
                       int32_t *d_bd, int32_t *d_sd, int iters, float *avg_ms)
{
    const int splits = std::max(1, std::min(64, (nt + 255) / 256));
    const int t_per_split = (((nt + splits - 1) / splits) + 255) & ~255;
    const int eff_splits = (nt + t_per_split - 1) / t_per_split;
    int st = m->part.alloc((size_t)2 * eff_splits * nq);
    if (st) return st;
    uint32_t *p1 = m->part.p, *p2 = m->part.p + (size_t)eff_splits * nq;
    AOS2_HIP_CHECK(hipEventRecord(m->ev[0], m->stream));
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(hamming_best2_kernel, dim3((nq + 255) / 256, eff_splits), dim3(256), 0, m->stream, d_q, nq,
                           d_t, nt, t_per_split, p1, p2);
        hipLaunchKernelGGL(hamming_merge_kernel, dim3((nq + 255) / 256), dim3(256), 0, m->stream, p1, p2, nq,
                           eff_splits, d_bi, d_bd, d_sd);
    }
    AOS2_HIP_CHECK(hipEventRecord(m->ev[1], m->stream));
    AOS2_HIP_CHECK(hipStreamSynchronize(m->stream));
    AOS2_HIP_CHECK(hipGetLastError());
    if (avg_ms) {
        float ms = 0;
        AOS2_HIP_CHECK(hipEventElapsedTime(&ms, m->ev[0], m->ev[1]));
        *avg_ms = ms / iters;
    }
    return AOS2_OK;
}

int aos2_matcher_hamming_best2_device(aos2_matcher_t *m, const uint8_t *d_q, int nq, const uint8_t *d_t, int nt,
                                      int32_t *d_best_idx, int32_t *d_best_dist, int32_t *d_second_dist, int iters,
                                      float *avg_ms)
{
    if (!m || !d_q || !d_t || nq <= 0 || nt <= 0 || nt >= (1 << 20) || !d_best_idx || !d_best_dist || !d_second_dist ||
        iters <= 0) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = matcher_init(m);
    if (st) return st;
    return hamming_run(m, d_q, nq, d_t, nt, d_best_idx, d_best_dist, d_second_dist, iters, avg_ms);
}

int aos2_matcher_hamming_best2(aos2_matcher_t *m, const uint8_t *q, int nq, const uint8_t *t, int nt,
                               int32_t *best_idx, int32_t *best_dist, int32_t *second_dist)
{
    if (!m || !q || !t || nq <= 0 || nt <= 0 || nt >= (1 << 20) || !best_idx || !best_dist || !second_dist) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = matcher_init(m);
    if (st) return st;
    Arena A{m};
    const uint8_t *d_q, *d_t;
    int32_t *d_bi, *d_bd, *d_sd;
    A.in(d_q, q, (size_t)nq * 32);
    A.in(d_t, t, (size_t)nt * 32);
    A.scratch(d_bi, (size_t)nq * 4);
    A.scratch(d_bd, (size_t)nq * 4);
    A.scratch(d_sd, (size_t)nq * 4);
    if ((st = A.upload())) return st;
    if ((st = hamming_run(m, d_q, nq, d_t, nt, d_bi, d_bd, d_sd, 1, nullptr))) return st;
    A.fetch(best_idx, d_bi, (size_t)nq * 4);
    A.fetch(best_dist, d_bd, (size_t)nq * 4);
    A.fetch(second_dist, d_sd, (size_t)nq * 4);
    return A.finish();
}

// shared by SearchByBoW(KF, F) (kf_kf = 0, match_out[p] has n_f entries) and SearchByBoW(KF1, KF2)
// (kf_kf = 1, f_has_mp[p] = has_mp2, match_out[p] has n_kf entries)
// dev_inputs: desc_kf / desc_f / angle_kf / angle_f of the pairs are DEVICE arrays (the descriptors and keys of frames that
// already live in HBM, e.g. a device-resident Frames batch): they are used in place; the FeatureVector CSRs, kf_has_mp
// and the results stay host arrays (a few KB per pair)
static int bow_run(aos2_matcher_t *m, const aos2_bow_pair_t *pairs, const uint8_t *const *f_has_mp, int n_pairs, int kf_kf,
                   int32_t *const *match_f, int32_t *nmatches, bool dev_inputs = false)
{
    int st = matcher_init(m);
    if (st) return st;
    Arena A{m};
    std::vector<BowPairDev> dev(n_pairs);
    std::vector<BowQuery> queries;
    int max_nf = 0, max_q = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const aos2_bow_pair_t &P = pairs[p];
        if (P.n_kf < 0 || P.n_f < 0 || P.n_nodes_kf < 0 || P.n_nodes_f < 0 || !match_f[p]) {
            set_error("bad BoW pair %d", p);
            return AOS2_ERR_ARG;
        }
        // on the host: the visiting order of the KF features and the bucket each one is compared against
        queries.clear();
        size_t ent = 0;
        const bool in_range = fv_join(P.n_nodes_kf, P.node_id_kf, P.node_off_kf, P.node_idx_kf, P.n_kf, P.n_nodes_f, P.node_id_f,
                                      P.node_off_f, [&](int kf, int b0, int bc) {
                                          if (!P.kf_has_mp[kf]) return;  // no map point / bad (:194-198)
                                          queries.push_back(BowQuery{kf, b0, bc, (int32_t)ent});
                                          ent += (size_t)bc;
                                      });
        if (!in_range) {
            set_error("BoW pair %d: feature index out of range", p);
            return AOS2_ERR_ARG;
        }
        if (ent > (size_t)1 << 28) {
            set_error("BoW pair %d needs %zu distance entries", p, ent);
            return AOS2_ERR_ARG;
        }
        BowPairDev &D = dev[p];
        D.n_kf = P.n_kf; D.n_f = P.n_f; D.n_queries = (int)queries.size();
        D.kf_kf = kf_kf;
        if (dev_inputs) {
            D.desc_kf = P.desc_kf; D.desc_f = P.desc_f; D.angle_kf = P.angle_kf; D.angle_f = P.angle_f;
        } else {
            A.in(D.desc_kf, P.desc_kf, (size_t)P.n_kf * 32);
            A.in(D.desc_f, P.desc_f, (size_t)P.n_f * 32);
            A.in(D.angle_kf, P.angle_kf, (size_t)P.n_kf * 4);
            A.in(D.angle_f, P.angle_f, (size_t)P.n_f * 4);
        }
        A.in(D.node_idx_f, P.node_idx_f, (size_t)(P.n_nodes_f ? P.node_off_f[P.n_nodes_f] : 0) * 4);
        A.in(D.queries, queries.data(), queries.size() * sizeof(BowQuery));
        A.scratch(D.entries, ent * sizeof(Entry) + 8);
        A.out(D.match_f, (size_t)P.n_f * 4 + 4);
        A.scratch(D.bin_f, (size_t)P.n_f * 4 + 4);
        A.out(D.nmatches, 4);
        A.scratch(D.choice, queries.size() * 4 + 4);   // (parallel stage B)
        if (kf_kf) {
            A.in(D.f_has_mp, f_has_mp[p], (size_t)P.n_f);
            const size_t m1 = A.out(D.match_1, (size_t)P.n_kf * 8 + 8);   // match_1 | bin_1
            A.bind(D.bin_1, m1 + (size_t)P.n_kf * 4);
        }
        max_nf = std::max(max_nf, P.n_f);
        max_q = std::max(max_q, D.n_queries);
    }
    if (max_nf > 60000) {
        set_error("n_f %d exceeds the LDS flag table (60000)", max_nf);
        return AOS2_ERR_ARG;
    }
    const BowPairDev *d_pairs;
    A.hole(d_pairs, sizeof(BowPairDev) * n_pairs);
    if ((st = A.alloc())) return st;
    A.fill_hole(d_pairs, dev.data(), sizeof(BowPairDev) * n_pairs);
    if ((st = A.upload())) return st;
    if ((st = A.begin())) return st;
    if (max_q > 0) hipLaunchKernelGGL(bow_distances_kernel, dim3(max_q, n_pairs), dim3(64), 0, m->stream, d_pairs);
    if (use_fix_resolve(m, max_nf))
        hipLaunchKernelGGL(bow_resolve_fix_kernel, dim3(n_pairs), dim3(512), (size_t)max_nf * 8 + 16, m->stream, d_pairs,
                           m->nnratio, m->check_ori);
    else
        hipLaunchKernelGGL(bow_resolve_kernel, dim3(n_pairs), dim3(64), (size_t)max_nf + 16, m->stream, d_pairs, m->nnratio,
                           m->check_ori);
    for (int p = 0; p < n_pairs; ++p) {
        if (!kf_kf)
            A.fetch(match_f[p], dev[p].match_f, (size_t)pairs[p].n_f * 4);
        else
            A.fetch(match_f[p], dev[p].match_1, (size_t)pairs[p].n_kf * 4);
        A.fetch(&nmatches[p], dev[p].nmatches, 4);
    }
    return A.end();
}

int aos2_matcher_search_by_bow(aos2_matcher_t *m, const aos2_bow_pair_t *pairs, int n_pairs, int32_t *const *match_f,
                               int32_t *nmatches)
{
    if (!m || !pairs || n_pairs <= 0 || !match_f || !nmatches) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    return bow_run(m, pairs, nullptr, n_pairs, 0, match_f, nmatches);
}

int aos2_matcher_search_by_bow_device(aos2_matcher_t *m, const aos2_bow_pair_t *pairs, int n_pairs, int32_t *const *match_f,
                                      int32_t *nmatches)
{
    if (!m || !pairs || n_pairs <= 0 || !match_f || !nmatches) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    return bow_run(m, pairs, nullptr, n_pairs, 0, match_f, nmatches, true);
}

// mvKeys[i].angle of [n][cap] keypoints (28-byte cv::KeyPoint records) as the dense float array the search reads
__global__ void key_angles_kernel(const aos2_keypoint_t *__restrict__ kps, float *__restrict__ angle, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) angle[i] = kps[i].angle;
}

int aos2_matcher_search_by_bow_frames(aos2_matcher_t *m, const aos2_bow_frames_t *q, int32_t *match_f, int32_t *nmatches)
{
    if (!m || !q || !match_f || !nmatches || q->n_frames <= 0 || q->cap <= 0 || !q->d_desc_kf || !q->d_kps_kf || !q->d_n_kf || !q->d_desc_f ||
        !q->d_kps_f || !q->d_n_f || !q->kf_has_mp || !q->d_kf_fv_node || !q->d_kf_fv_off || !q->d_kf_fv_idx || !q->d_kf_n_fv ||
        !q->d_f_fv_node || !q->d_f_fv_off || !q->d_f_fv_idx || !q->d_f_n_fv) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = matcher_init(m);
    if (st) return st;
    const size_t n = (size_t)q->n_frames, cap = (size_t)q->cap, tot = n * cap;
    if ((st = m->fr_angle.alloc(2 * tot))) return st;
    // host copies: per side n counts | n fv counts | fv_node [n][cap] | fv_off [n][cap + 1] | fv_idx [n][cap]
    const size_t side = 4 * (2 * n + tot + n * (cap + 1) + tot);
    if ((st = m->fr_host.alloc(2 * side))) return st;
    hipStream_t s = m->stream;
    hipLaunchKernelGGL(key_angles_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, q->d_kps_kf, m->fr_angle.p, tot);
    hipLaunchKernelGGL(key_angles_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, q->d_kps_f, m->fr_angle.p + tot, tot);
    struct Side { int32_t *n, *n_fv, *node, *off, *idx; } H[2];
    const int32_t *src[2][5] = {{q->d_n_kf, q->d_kf_n_fv, q->d_kf_fv_node, q->d_kf_fv_off, q->d_kf_fv_idx},
                                {q->d_n_f, q->d_f_n_fv, q->d_f_fv_node, q->d_f_fv_off, q->d_f_fv_idx}};
    const size_t cnt[5] = {n, n, tot, n * (cap + 1), tot};
    for (int k = 0; k < 2; ++k) {
        int32_t *base = reinterpret_cast<int32_t *>(m->fr_host.p + k * side);
        int32_t **dst[5] = {&H[k].n, &H[k].n_fv, &H[k].node, &H[k].off, &H[k].idx};
        for (int a = 0; a < 5; ++a) {
            *dst[a] = base;
            AOS2_HIP_CHECK(hipMemcpyAsync(base, src[k][a], 4 * cnt[a], hipMemcpyDeviceToHost, s));
            base += cnt[a];
        }
    }
    AOS2_HIP_CHECK(hipStreamSynchronize(s));
    std::vector<aos2_bow_pair_t> pairs(n);
    std::vector<int32_t *> mptr(n);
    for (size_t b = 0; b < n; ++b) {
        aos2_bow_pair_t &P = pairs[b];
        P.n_kf = H[0].n[b]; P.n_f = H[1].n[b];
        if (P.n_kf < 0 || P.n_kf > (int)cap || P.n_f < 0 || P.n_f > (int)cap || H[0].n_fv[b] < 0 || H[0].n_fv[b] > (int)cap || H[1].n_fv[b] < 0 ||
            H[1].n_fv[b] > (int)cap) {
            set_error("frame %zu: counts outside the capacity %zu", b, cap);
            return AOS2_ERR_ARG;
        }
        // the FeatureVector CSRs came back from the device (a transform that was not ordered before this call leaves stale
        // buffers): bow_run uses them as host copy lengths and indices, so offsets must be monotone from 0 and indices in range
        for (int k = 0; k < 2; ++k) {
            const int32_t *off = H[k].off + b * (cap + 1), *idx = H[k].idx + b * cap;
            const int nfv = H[k].n_fv[b], nfe = k == 0 ? P.n_kf : P.n_f;
            bool ok = nfv == 0 || off[0] == 0;
            for (int v = 0; ok && v < nfv; ++v) ok = off[v + 1] >= off[v] && off[v + 1] <= (int32_t)cap;
            for (int e = 0; ok && nfv > 0 && e < off[nfv]; ++e) ok = idx[e] >= 0 && idx[e] < nfe;
            if (!ok) {
                set_error("frame %zu: inconsistent FeatureVector (%s side): offsets not monotone within the capacity or a feature index out of range",
                          b, k == 0 ? "keyframe" : "frame");
                return AOS2_ERR_ARG;
            }
        }
        P.desc_kf = q->d_desc_kf + b * cap * 32; P.desc_f = q->d_desc_f + b * cap * 32;
        P.angle_kf = m->fr_angle.p + b * cap; P.angle_f = m->fr_angle.p + tot + b * cap;
        P.kf_has_mp = q->kf_has_mp + b * cap;
        P.n_nodes_kf = H[0].n_fv[b]; P.n_nodes_f = H[1].n_fv[b];
        P.node_id_kf = H[0].node + b * cap; P.node_off_kf = H[0].off + b * (cap + 1); P.node_idx_kf = H[0].idx + b * cap;
        P.node_id_f = H[1].node + b * cap; P.node_off_f = H[1].off + b * (cap + 1); P.node_idx_f = H[1].idx + b * cap;
        mptr[b] = match_f + b * cap;
    }
    return bow_run(m, pairs.data(), nullptr, (int)n, 0, mptr.data(), nmatches, true);
}

int aos2_matcher_search_by_bow_kf(aos2_matcher_t *m, const aos2_bow_kf_pair_t *pairs, int n_pairs, int32_t *const *match12,
                                  int32_t *nmatches)
{
    if (!m || !pairs || n_pairs <= 0 || !match12 || !nmatches) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    std::vector<aos2_bow_pair_t> v(n_pairs);
    std::vector<const uint8_t *> hm2(n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        const aos2_bow_kf_pair_t &K = pairs[p];
        if (K.n2 > 0 && !K.has_mp2) {
            set_error("bad BoW pair %d", p);
            return AOS2_ERR_ARG;
        }
        aos2_bow_pair_t &B = v[p];
        B.n_kf = K.n1; B.n_f = K.n2;
        B.desc_kf = K.desc1; B.desc_f = K.desc2;
        B.kf_has_mp = K.has_mp1;
        B.angle_kf = K.angle1; B.angle_f = K.angle2;
        B.n_nodes_kf = K.n_nodes1; B.n_nodes_f = K.n_nodes2;
        B.node_id_kf = K.node_id1; B.node_off_kf = K.node_off1; B.node_idx_kf = K.node_idx1;
        B.node_id_f = K.node_id2; B.node_off_f = K.node_off2; B.node_idx_f = K.node_idx2;
        hm2[p] = K.has_mp2;
    }
    return bow_run(m, v.data(), hm2.data(), n_pairs, 1, match12, nmatches);
}

int aos2_matcher_search_for_triangulation(aos2_matcher_t *m, const aos2_triang_pair_t *pairs, int n_pairs, int only_stereo,
                                          int32_t *const *match12, int32_t *nmatches)
{
    if (!m || !pairs || n_pairs <= 0 || !match12 || !nmatches) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = matcher_init(m);
    if (st) return st;
    Arena A{m};
    std::vector<TriPairDev> dev(n_pairs);
    std::vector<TriQuery> queries;
    std::vector<int32_t> init;
    int max_q = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const aos2_triang_pair_t &P = pairs[p];
        if (P.n1 < 0 || P.n2 < 0 || P.n_nodes1 < 0 || P.n_nodes2 < 0 || !match12[p] || P.n_levels2 <= 0) {
            set_error("bad triangulation pair %d", p);
            return AOS2_ERR_ARG;
        }
        queries.clear();
        const bool in_range = fv_join(P.n_nodes1, P.node_id1, P.node_off1, P.node_idx1, P.n1, P.n_nodes2, P.node_id2, P.node_off2,
                                      [&](int idx1, int b0, int bc) {
                                          if (P.has_mp1[idx1]) return;                            // :700-703
                                          if (only_stereo && !(P.u_right1[idx1] >= 0)) return;    // :705-709
                                          queries.push_back(TriQuery{idx1, b0, bc});
                                      });
        if (!in_range) {
            set_error("triangulation pair %d: feature index out of range", p);
            return AOS2_ERR_ARG;
        }
        const size_t n1 = (size_t)P.n1, n2 = (size_t)P.n2;
        TriPairDev &D = dev[p];
        D.n1 = P.n1; D.n2 = P.n2; D.n_queries = (int)queries.size(); D.only_stereo = only_stereo;
        memcpy(D.F12, P.F12, sizeof(D.F12));
        D.ex = P.ex; D.ey = P.ey;
        A.in(D.desc1, P.desc1, n1 * 32);
        A.in(D.desc2, P.desc2, n2 * 32);
        A.in(D.has_mp2, P.has_mp2, n2);
        A.in(D.x1, P.x1, n1 * 4);
        A.in(D.y1, P.y1, n1 * 4);
        A.in(D.angle1, P.angle1, n1 * 4);
        A.in(D.u_right1, P.u_right1, n1 * 4);
        A.in(D.x2, P.x2, n2 * 4);
        A.in(D.y2, P.y2, n2 * 4);
        A.in(D.angle2, P.angle2, n2 * 4);
        A.in(D.u_right2, P.u_right2, n2 * 4);
        A.in(D.octave2, P.octave2, n2 * 4);
        A.in(D.scale_factors2, P.scale_factors2, (size_t)P.n_levels2 * 4);
        A.in(D.level_sigma2_2, P.level_sigma2_2, (size_t)P.n_levels2 * 4);
        A.in(D.node_idx2, P.node_idx2, (size_t)(P.n_nodes2 ? P.node_off2[P.n_nodes2] : 0) * 4);
        A.in(D.queries, queries.data(), queries.size() * sizeof(TriQuery));
        init.assign(n1 + 1, -1);
        A.in(D.match12, init.data(), (n1 + 1) * 4);  // match12 = -1 (:681)
        A.scratch(D.nmatches, 8);
        max_q = std::max(max_q, D.n_queries);
    }
    TriPairDev *d_pairs;
    A.hole(d_pairs, sizeof(TriPairDev) * n_pairs);
    if ((st = A.alloc())) return st;
    A.fill_hole(d_pairs, dev.data(), sizeof(TriPairDev) * n_pairs);
    if ((st = A.upload())) return st;
    if ((st = A.begin())) return st;
    if (max_q > 0) hipLaunchKernelGGL(triang_match_kernel, dim3(max_q, n_pairs), dim3(64), 0, m->stream, d_pairs);
    hipLaunchKernelGGL(triang_finish_kernel, dim3(n_pairs), dim3(64), 0, m->stream, d_pairs, m->check_ori);
    for (int p = 0; p < n_pairs; ++p) {
        if (pairs[p].n1 > 0) A.fetch(match12[p], dev[p].match12, (size_t)pairs[p].n1 * 4);
        A.fetch(&nmatches[p], dev[p].nmatches, 4);
    }
    return A.end();
}

int aos2_compute_distinctive_descriptors(aos2_matcher_t *m, int n_points, const int32_t *off, const uint8_t *desc,
                                         int32_t *best_idx)
{
    if (!m || n_points < 0 || (n_points > 0 && (!off || !best_idx))) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if (n_points == 0) return AOS2_OK;
    for (int p = 0; p < n_points; ++p)
        if (off[p + 1] < off[p] || off[0] != 0) {
            set_error("observation offsets must start at 0 and ascend");
            return AOS2_ERR_ARG;
        }
    const size_t total = (size_t)off[n_points];
    if (total > 0 && !desc) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = matcher_init(m);
    if (st) return st;
    Arena A{m};
    const int32_t *d_off;
    const uint8_t *d_desc;
    int32_t *d_best;
    A.in(d_off, off, (size_t)(n_points + 1) * 4);
    A.in(d_desc, desc, total * 32);
    A.scratch(d_best, (size_t)n_points * 4);
    if ((st = A.upload())) return st;
    if ((st = A.begin())) return st;
    hipLaunchKernelGGL(distinctive_kernel, dim3(n_points), dim3(64), 0, m->stream, n_points, d_off, d_desc, d_best);
    A.fetch(best_idx, d_best, (size_t)n_points * 4);
    return A.end();
}

// one SearchByProjection(Frame, map points) problem -- the single call, or an item of the batch: the frame and the map
// points, the results, then the scratch of the two stages
static void proj_mp_item(Arena &A, const aos2_frame_view_t *f, const aos2_proj_mp_t *p, ProjMpItem &it)
{
    const size_t n = (size_t)p->n_mp;
    frame_dev(A, f, it.F);
    ProjMpDev &P = it.P;
    P = ProjMpDev{};
    P.n_mp = p->n_mp;
    A.in(P.track_in_view, p->track_in_view, n);
    A.in(P.desc, p->desc, n * 32);
    A.in(P.has_obs, p->has_obs, n);
    A.in(P.pred_level, p->pred_level, n * 4);
    A.in(P.view_cos, p->view_cos, n * 4);
    A.in(P.proj_x, p->proj_x, n * 4);
    A.in(P.proj_y, p->proj_y, n * 4);
    A.in(P.proj_xr, p->proj_xr, n * 4);
    A.out(it.match_f, (size_t)f->n_f * 4 + 4);
    A.out(it.nmatches, 8);   // nmatches, and a word for the entry counter / overflow flag of the single call
    A.scratch(it.slots, (n + 1) * sizeof(QuerySlot));
    A.scratch(it.choice, (n + 1) * 4);
}

int aos2_matcher_search_by_projection(aos2_matcher_t *m, const aos2_frame_view_t *f, const aos2_proj_mp_t *p, float th,
                                      int32_t *match_f, int32_t *nmatches)
{
    if (!m || !p || !match_f || !nmatches || p->n_mp < 0) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = check_frame(f);
    if (st) return st;
    if (p->n_mp > 0 && (!p->track_in_view || !p->desc || !p->has_obs || !p->view_cos || !p->proj_x || !p->proj_y || !p->proj_xr)) {
        set_error("bad map point set (NULL array)");
        return AOS2_ERR_ARG;
    }
    if ((st = check_levels(p->pred_level, p->n_mp, f->n_levels, "pred_level", p->track_in_view))) return st;
    if ((st = matcher_init(m))) return st;
    Arena A{m};
    ProjMpItem it{};
    proj_mp_item(A, f, p, it);
    const FrameDev &F = it.F;
    const ProjMpDev &P = it.P;
    // Entry pool.  Usual sizes: every query owns a slice that holds the whole frame (one pass, no counting).  Large local
    // maps (n_mp x n_f x 8 B beyond 64 MB): the pool is sized from the REAL window populations -- count pass, scan, fill
    // pass -- starting from a budget of 64 entries per query and, if the windows of this call hold more (the scan reports
    // the total), once more with exactly that many.  No size limit other than device memory.
    const size_t worst = (size_t)p->n_mp * (size_t)f->n_f;   // a window holds at most every feature
    const bool two_pass = worst * sizeof(Entry) > ((size_t)64 << 20) || getenv("AOS2_PROJ_TWO_PASS") != nullptr;
    size_t pool_cap = two_pass ? std::max<size_t>((size_t)p->n_mp * 64, 1024) : worst;
    if (const char *e = getenv("AOS2_PROJ_POOL_BUDGET")) pool_cap = two_pass ? (size_t)std::max(1, atoi(e)) : pool_cap;   // (tests: force the retry)
    if ((st = A.upload())) return st;
    int32_t *d_used = it.nmatches + 1;
    for (int attempt = 0;; ++attempt) {
        Entry *d_pool;
        if ((st = pool_reserve(m, pool_cap, "projection search", d_pool))) return st;
        AOS2_HIP_CHECK(hipMemsetAsync(d_used, 0, 4, m->stream));
        if (attempt == 0 && (st = A.begin())) return st;   // (a second attempt is timed with the first)
        if (p->n_mp > 0) {
            if (!two_pass)
                hipLaunchKernelGGL(proj_mp_entries_kernel, dim3(p->n_mp), dim3(64), 0, m->stream, F, P, th, it.slots, d_pool, d_used,
                                   (int)pool_cap, 0);
            else {
                hipLaunchKernelGGL(proj_mp_entries_kernel, dim3(p->n_mp), dim3(64), 0, m->stream, F, P, th, it.slots, d_pool, d_used,
                                   (int)pool_cap, 1);
                hipLaunchKernelGGL(proj_mp_scan_slots_kernel, dim3(1), dim3(256), 0, m->stream, it.slots, (const int32_t *)nullptr,
                                   p->n_mp, (int)pool_cap, d_used);
                hipLaunchKernelGGL(proj_mp_entries_kernel, dim3(p->n_mp), dim3(64), 0, m->stream, F, P, th, it.slots, d_pool, d_used,
                                   (int)pool_cap, 2);
            }
        }
        if (use_fix_resolve(m, f->n_f))
            hipLaunchKernelGGL(proj_mp_resolve_fix_kernel, dim3(1), dim3(1024), (size_t)f->n_f * 8 + 16, m->stream, F, P, m->nnratio,
                               it.slots, d_pool, it.match_f, it.nmatches, it.choice);
        else   // the one-wave sequential loop: frames with more features than the LDS copy of B holds, or AOS2_SERIAL_RESOLVE=1
            hipLaunchKernelGGL(proj_mp_resolve_kernel, dim3(1), dim3(64), (size_t)f->n_f + 16, m->stream, F, P, m->nnratio, it.slots,
                               d_pool, it.match_f, it.nmatches);
        int32_t tail[2] = {0, 0};   // nmatches, overflow word
        A.fetch(match_f, it.match_f, (size_t)f->n_f * 4);
        A.fetch(tail, it.nmatches, 8);
        if ((st = A.end())) return st;
        if (two_pass && (size_t)tail[1] > pool_cap && attempt == 0) {   // the windows hold tail[1] entries: once more, exactly sized
            pool_cap = (size_t)tail[1];
            continue;
        }
        *nmatches = tail[0];
        break;
    }
    return AOS2_OK;
}

int aos2_matcher_search_by_projection_batch(aos2_matcher_t *m, const aos2_frame_view_t *frames, const aos2_proj_mp_t *problems,
                                            int n_problems, float th, int32_t *const *match_f, int32_t *nmatches)
{
    if (!m || !frames || !problems || n_problems <= 0 || !match_f || !nmatches) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st;
    size_t pool_cap = 0;
    int max_mp = 0, max_nf = 0;
    for (int i = 0; i < n_problems; ++i) {
        if ((st = check_frame(&frames[i]))) return st;
        const aos2_proj_mp_t &pi = problems[i];
        if (pi.n_mp < 0 || !match_f[i] || (pi.n_mp > 0 && (!pi.track_in_view || !pi.desc || !pi.has_obs || !pi.view_cos || !pi.proj_x ||
                                                             !pi.proj_y || !pi.proj_xr))) {
            set_error("bad projection problem %d", i);
            return AOS2_ERR_ARG;
        }
        if ((st = check_levels(pi.pred_level, pi.n_mp, frames[i].n_levels, "pred_level", pi.track_in_view))) return st;
        // entry budget: a search window rarely holds more than a few dozen features; 512 per map point (or the
        // whole frame if smaller) is the bound here -- AOS2_ERR_CAPACITY if a problem ever needs more
        pool_cap += (size_t)problems[i].n_mp * (size_t)std::min(frames[i].n_f, 512);
        max_mp = std::max(max_mp, problems[i].n_mp);
        max_nf = std::max(max_nf, frames[i].n_f);
    }
    if ((st = matcher_init(m))) return st;
    Entry *d_pool;
    if ((st = pool_reserve(m, pool_cap, "batched projection search", d_pool))) return st;
    Arena A{m};
    std::vector<ProjMpItem> items(n_problems);
    size_t pool_next = 0;
    for (int i = 0; i < n_problems; ++i) {
        ProjMpItem &it = items[i];
        proj_mp_item(A, &frames[i], &problems[i], it);
        it.pool_cap = (int32_t)((size_t)problems[i].n_mp * (size_t)std::min(frames[i].n_f, 512));
        it.pool_base = (int32_t)pool_next;
        pool_next += (size_t)it.pool_cap;
    }
    const ProjMpItem *d_items;
    int32_t *d_used;
    A.hole(d_items, sizeof(ProjMpItem) * (size_t)n_problems);
    const size_t used_tok = A.out(d_used, (size_t)n_problems * 256 + 8);   // one counter per problem, 256 B apart
    for (int i = 0; i < n_problems; ++i) A.bind(items[i].pool_used, used_tok + 256 * (size_t)i);
    if ((st = A.alloc())) return st;
    A.fill_hole(d_items, items.data(), sizeof(ProjMpItem) * (size_t)n_problems);
    if ((st = A.upload())) return st;
    AOS2_HIP_CHECK(hipMemsetAsync(d_used, 0, (size_t)n_problems * 256, m->stream));
    if ((st = A.begin())) return st;
    if (max_mp > 0)
        hipLaunchKernelGGL(proj_mp_entries_batch_kernel, dim3(max_mp, n_problems), dim3(64), 0, m->stream, d_items, th,
                           d_pool);
    if (use_fix_resolve(m, max_nf))
        hipLaunchKernelGGL(proj_mp_resolve_fix_batch_kernel, dim3(n_problems), dim3(256), (size_t)max_nf * 8 + 16, m->stream, d_items,
                           m->nnratio, d_pool);
    else
        hipLaunchKernelGGL(proj_mp_resolve_batch_kernel, dim3(n_problems), dim3(64), (size_t)max_nf + 16, m->stream, d_items,
                           m->nnratio, d_pool);
    std::vector<int32_t> used((size_t)n_problems * 64);
    A.fetch(used.data(), d_used, (size_t)n_problems * 256);
    for (int i = 0; i < n_problems; ++i) {
        A.fetch(match_f[i], items[i].match_f, (size_t)frames[i].n_f * 4);
        A.fetch(&nmatches[i], items[i].nmatches, 4);
    }
    if ((st = A.end())) return st;
    for (int i = 0; i < n_problems; ++i)
        if (used[(size_t)i * 64] > 0) {   // overflow flag = a window population that did not fit its slice
            set_error("batched projection search: a search window of problem %d holds %d features, more than the %d "
                      "budgeted per map point; use aos2_matcher_search_by_projection per frame", i, used[(size_t)i * 64],
                      std::min(frames[i].n_f, 512));
            return AOS2_ERR_CAPACITY;
        }
    return AOS2_OK;
}

int aos2_matcher_search_by_projection_last(aos2_matcher_t *m, const aos2_frame_view_t *cur, const aos2_proj_last_t *p,
                                           float th, int mono, int32_t *match_f, int32_t *nmatches)
{
    if (!m || !p || !match_f || !nmatches || p->n_last < 0) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = check_frame(cur);
    if (st) return st;
    if (p->n_last > 0 && (!p->last_valid || !p->world_pos || !p->desc || !p->last_angle || !p->has_obs)) {
        set_error("bad last-frame point set (NULL array)");
        return AOS2_ERR_ARG;
    }
    if ((st = check_levels(p->last_octave, p->n_last, cur->n_levels, "last_octave", p->last_valid))) return st;
    if ((st = matcher_init(m))) return st;
    Arena A{m};
    const size_t n = (size_t)p->n_last, pool_cap = n * (size_t)cur->n_f;
    FrameDev F;
    frame_dev(A, cur, F);
    ProjLastDev P{};
    P.n_last = p->n_last;
    A.in(P.last_valid, p->last_valid, n);
    A.in(P.desc, p->desc, n * 32);
    A.in(P.has_obs, p->has_obs, n);
    A.in(P.world_pos, p->world_pos, n * 12);
    A.in(P.last_angle, p->last_angle, n * 4);
    A.in(P.last_octave, p->last_octave, n * 4);
    memcpy(P.Tcw, p->Tcw, sizeof(P.Tcw));
    memcpy(P.Tlw, p->Tlw, sizeof(P.Tlw));
    P.fx = p->fx; P.fy = p->fy; P.cx = p->cx; P.cy = p->cy; P.mb = p->mb; P.mbf = p->mbf;
    int32_t *d_match, *d_n, *d_choice;
    uint32_t *d_bin;
    QuerySlot *d_slots;
    A.out(d_match, (size_t)cur->n_f * 4 + 4);
    A.scratch(d_bin, (size_t)cur->n_f * 4 + 4);
    A.out(d_n, 8);   // nmatches, entry counter
    A.scratch(d_slots, (n + 1) * sizeof(QuerySlot));
    A.scratch(d_choice, (n + 1) * 4);
    Entry *d_pool;
    if ((st = pool_reserve(m, pool_cap, "projection search from the last frame", d_pool))) return st;
    if ((st = A.upload())) return st;
    AOS2_HIP_CHECK(hipMemsetAsync(d_n + 1, 0, 4, m->stream));
    if ((st = A.begin())) return st;
    if (p->n_last > 0)
        hipLaunchKernelGGL(proj_last_entries_kernel, dim3(p->n_last), dim3(64), 0, m->stream, F, P, th, mono ? 1 : 0, d_slots,
                           d_pool, d_n + 1, (int)pool_cap);
    if (use_fix_resolve(m, cur->n_f))
        hipLaunchKernelGGL(proj_last_resolve_fix_kernel, dim3(1), dim3(1024), (size_t)cur->n_f * 8 + 16, m->stream, F, P,
                           m->check_ori, d_slots, d_pool, d_match, d_bin, d_n, d_choice);
    else
        hipLaunchKernelGGL(proj_last_resolve_kernel, dim3(1), dim3(64), (size_t)cur->n_f + 16, m->stream, F, P, m->check_ori,
                           d_slots, d_pool, d_match, d_bin, d_n);
    A.fetch(match_f, d_match, (size_t)cur->n_f * 4);
    A.fetch(nmatches, d_n, 4);
    return A.end();
}

// ---- projection family -------------------------------------------------
static int check_points(const aos2_proj_points_t *p, int mode)
{
    if (!p || p->n_pts < 0 || (p->n_pts > 0 && (!p->valid || !p->pos || !p->max_dist || !p->min_dist || !p->desc)) ||
        (p->n_pts > 0 && mode <= 2 && !p->normal) || (mode == 0 && !p->inv_level_sigma2) ||
        (p->n_pts > 0 && mode == 4 && !p->q_angle) || !(p->log_scale_factor > 0)) {
        set_error("bad point set");
        return AOS2_ERR_ARG;
    }
    return AOS2_OK;
}

// stages the point set and describes it in P (bound by the arena, like a frame).  Modes 0-4 are the searches; mode 5 is
// Frame::isInFrustum, which has no descriptors: positions, ranges, normals and the first camera only.  An optional
// array the caller left out (check_points says which a mode needs) stays a null pointer.
static void points_dev(Arena &A, const aos2_proj_points_t *p, int mode, int n_levels, ProjGenDev &P)
{
    const size_t n = (size_t)p->n_pts;
    const bool search = mode != 5;
    P = ProjGenDev{};
    P.n_pts = p->n_pts;
    P.mode = mode;
    if (search) {
        A.in(P.valid, p->valid, n);
        A.in(P.desc, p->desc, n * 32);
    }
    A.in(P.pos, p->pos, n * 12);
    A.in(P.max_dist, p->max_dist, n * 4);
    A.in(P.min_dist, p->min_dist, n * 4);
    if (p->normal) A.in(P.normal, p->normal, n * 12);
    if (search && p->q_angle) A.in(P.q_angle, p->q_angle, n * 4);
    if (search && p->inv_level_sigma2) A.in(P.inv_level_sigma2, p->inv_level_sigma2, (size_t)n_levels * 4);
    memcpy(P.R, p->R, sizeof(P.R)); memcpy(P.t, p->t, sizeof(P.t)); memcpy(P.Ow, p->Ow, sizeof(P.Ow));
    if (search) {
        memcpy(P.R2, p->R2, sizeof(P.R2)); memcpy(P.t2, p->t2, sizeof(P.t2));
        P.th = p->th;
    }
    P.fx = p->fx; P.fy = p->fy; P.cx = p->cx; P.cy = p->cy; P.bf = p->bf;
    P.log_scale_factor = p->log_scale_factor;
}

// independent points: modes 0 (Fuse), 1 (Fuse with Scw)
int aos2_matcher_fuse(aos2_matcher_t *m, const aos2_frame_view_t *kf, const aos2_proj_points_t *p, int sim3,
                      int32_t *best_idx, int32_t *best_dist, int32_t *n_fused)
{
    const int mode = sim3 ? 1 : 0;
    if (!m || !best_idx || !best_dist) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = check_frame(kf);
    if (st) return st;
    if ((st = check_points(p, mode))) return st;
    if (n_fused) *n_fused = 0;
    if (p->n_pts == 0) return AOS2_OK;
    if ((st = matcher_init(m))) return st;
    Arena A{m};
    FrameDev F;
    ProjGenDev P;
    int32_t *d_best;   // best_idx | best_dist
    frame_dev(A, kf, F);
    points_dev(A, p, mode, kf->n_levels, P);
    A.scratch(d_best, (size_t)p->n_pts * 8 + 8);
    if ((st = A.upload())) return st;
    if ((st = A.begin())) return st;
    hipLaunchKernelGGL(projgen_best_kernel, dim3(p->n_pts), dim3(64), 0, m->stream, F, P, TH_LOW, d_best, d_best + p->n_pts);
    A.fetch(best_idx, d_best, (size_t)p->n_pts * 4);
    A.fetch(best_dist, d_best + p->n_pts, (size_t)p->n_pts * 4);
    if ((st = A.end())) return st;
    if (n_fused) {
        int c = 0;
        for (int i = 0; i < p->n_pts; ++i) c += best_idx[i] >= 0;
        *n_fused = c;
    }
    return AOS2_OK;
}

int aos2_matcher_search_by_sim3(aos2_matcher_t *m, const aos2_frame_view_t *kf1, const aos2_frame_view_t *kf2,
                                const aos2_proj_points_t *p12, const aos2_proj_points_t *p21, int32_t *match12,
                                int32_t *n_found)
{
    if (!m || !match12 || !n_found) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st;
    if ((st = check_frame(kf1)) || (st = check_frame(kf2)) || (st = check_points(p12, 3)) || (st = check_points(p21, 3))) return st;
    if (p12->n_pts != kf1->n_f || p21->n_pts != kf2->n_f) {
        set_error("SearchBySim3: one (possibly invalid) map point per keyframe feature is expected");
        return AOS2_ERR_ARG;
    }
    *n_found = 0;
    if (p12->n_pts == 0) return AOS2_OK;
    if ((st = matcher_init(m))) return st;
    Arena A{m};
    const size_t n1 = (size_t)p12->n_pts, n2 = (size_t)p21->n_pts;
    FrameDev F1, F2;
    ProjGenDev P12, P21;
    int32_t *d_best1, *d_best2, *d_match, *d_n;
    frame_dev(A, kf1, F1);
    frame_dev(A, kf2, F2);
    points_dev(A, p12, 3, kf2->n_levels, P12);
    points_dev(A, p21, 3, kf1->n_levels, P21);
    A.scratch(d_best1, (n1 + 1) * 8);
    A.scratch(d_best2, (n2 + 1) * 8);
    A.scratch(d_match, (n1 + 1) * 4);
    A.scratch(d_n, 8);
    if ((st = A.upload())) return st;
    AOS2_HIP_CHECK(hipMemsetAsync(d_n, 0, 8, m->stream));
    if ((st = A.begin())) return st;
    hipLaunchKernelGGL(projgen_best_kernel, dim3((unsigned)n1), dim3(64), 0, m->stream, F2, P12, TH_HIGH, d_best1, d_best1 + n1);
    if (n2 > 0)
        hipLaunchKernelGGL(projgen_best_kernel, dim3((unsigned)n2), dim3(64), 0, m->stream, F1, P21, TH_HIGH, d_best2, d_best2 + n2);
    hipLaunchKernelGGL(sim3_agree_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, m->stream, d_best1, d_best2, (int)n1,
                       (int)n2, d_match, d_n);
    A.fetch(match12, d_match, n1 * 4);
    A.fetch(n_found, d_n, 4);
    return A.end();
}

int aos2_frame_assign_features_to_grid(aos2_matcher_t *m, int n, const float *kp_x, const float *kp_y, float min_x,
                                       float min_y, float grid_w_inv, float grid_h_inv, int32_t *grid_off, int32_t *grid_idx,
                                       int32_t *n_in_grid)
{
    if (!m || n < 0 || !grid_off || (n > 0 && (!kp_x || !kp_y || !grid_idx))) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if (n > 32000) {
        set_error("AssignFeaturesToGrid: more than 32000 features");
        return AOS2_ERR_CAPACITY;
    }
    int st = matcher_init(m);
    if (st) return st;
    constexpr int NC = GRID_COLS * GRID_ROWS;
    Arena A{m};
    const float *d_x, *d_y;
    int32_t *d_off, *d_idx;
    A.in(d_x, kp_x, (size_t)n * 4);
    A.in(d_y, kp_y, (size_t)n * 4);
    A.scratch(d_off, (size_t)(NC + 1) * 4);
    A.scratch(d_idx, (size_t)n * 4 + 4);
    if ((st = A.upload())) return st;
    if ((st = A.begin())) return st;
    hipLaunchKernelGGL(assign_grid_kernel, dim3(1), dim3(256), (size_t)(NC + 1) * 4 + (size_t)n * 2 + 16, m->stream, n, d_x, d_y,
                       min_x, min_y, grid_w_inv, grid_h_inv, d_off, d_idx);
    A.fetch(grid_off, d_off, (size_t)(NC + 1) * 4);
    if (n > 0) A.fetch(grid_idx, d_idx, (size_t)n * 4);
    if ((st = A.end())) return st;
    if (n_in_grid) *n_in_grid = grid_off[NC];
    return AOS2_OK;
}

int aos2_frame_stereo_from_rgbd(aos2_matcher_t *m, int n, const float *kp_x, const float *kp_y, const float *kpun_x,
                                const float *depth_img, int w, int h, int stride, float mbf, float *u_right, float *depth)
{
    if (!m || n < 0 || (n > 0 && (!kp_x || !kp_y || !kpun_x || !depth_img || !u_right || !depth)) || w <= 0 || h <= 0 ||
        stride < w) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if (n == 0) return AOS2_OK;
    for (int i = 0; i < n; ++i)
        if (!((int)kp_x[i] >= 0 && (int)kp_x[i] < w && (int)kp_y[i] >= 0 && (int)kp_y[i] < h)) {
            set_error("ComputeStereoFromRGBD: keypoint %d (%g, %g) outside the depth image", i, kp_x[i], kp_y[i]);
            return AOS2_ERR_ARG;
        }
    int st = matcher_init(m);
    if (st) return st;
    Arena A{m};
    const float *d_x, *d_y, *d_xun, *d_img;
    float *d_out;   // u_right | depth
    A.in(d_x, kp_x, (size_t)n * 4);
    A.in(d_y, kp_y, (size_t)n * 4);
    A.in(d_xun, kpun_x, (size_t)n * 4);
    A.in(d_img, depth_img, (size_t)stride * h * 4);
    A.scratch(d_out, (size_t)n * 8 + 8);
    if ((st = A.upload())) return st;
    if ((st = A.begin())) return st;
    hipLaunchKernelGGL(stereo_from_rgbd_kernel, dim3((n + 255) / 256), dim3(256), 0, m->stream, n, d_x, d_y, d_xun, d_img, stride,
                       mbf, d_out, d_out + n);
    A.fetch(u_right, d_out, (size_t)n * 4);
    A.fetch(depth, d_out + n, (size_t)n * 4);
    return A.end();
}

int aos2_frame_is_in_frustum(aos2_matcher_t *m, const aos2_proj_points_t *p, float min_x, float max_x, float min_y,
                             float max_y, int n_levels, float viewing_cos_limit, uint8_t *track_in_view, float *proj_x,
                             float *proj_y, float *proj_xr, int32_t *pred_level, float *view_cos)
{
    if (!m || n_levels <= 0) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if (!p || p->n_pts < 0 || (p->n_pts > 0 && (!p->pos || !p->max_dist || !p->min_dist || !p->normal)) ||
        !(p->log_scale_factor > 0)) {
        set_error("bad point set");
        return AOS2_ERR_ARG;
    }
    int st;
    if (p->n_pts == 0) return AOS2_OK;
    if (!track_in_view || !proj_x || !proj_y || !proj_xr || !pred_level || !view_cos) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if ((st = matcher_init(m))) return st;
    Arena A{m};
    const size_t n = (size_t)p->n_pts;
    ProjGenDev P;
    float *d_px;   // proj_x | proj_y | proj_xr | view_cos | pred_level | track_in_view
    points_dev(A, p, 5, n_levels, P);
    A.scratch(d_px, n * 24 + 64);
    if ((st = A.upload())) return st;
    float *d_py = d_px + n, *d_pr = d_py + n, *d_vc = d_pr + n;
    int32_t *d_lv = reinterpret_cast<int32_t *>(d_vc + n);
    uint8_t *d_iv = reinterpret_cast<uint8_t *>(d_lv + n);
    if ((st = A.begin())) return st;
    hipLaunchKernelGGL(is_in_frustum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->stream, P, min_x, max_x, min_y,
                       max_y, n_levels, viewing_cos_limit, d_iv, d_px, d_py, d_pr, d_lv, d_vc);
    A.fetch(proj_x, d_px, n * 4);
    A.fetch(proj_y, d_py, n * 4);
    A.fetch(proj_xr, d_pr, n * 4);
    A.fetch(view_cos, d_vc, n * 4);
    A.fetch(pred_level, d_lv, n * 4);
    A.fetch(track_in_view, d_iv, n);
    return A.end();
}

// greedy modes 2 (SearchByProjection(pKF, Scw, ...)) and 4 (SearchByProjection(CurrentFrame, pKF, ...))
static int projgen_serial(aos2_matcher_t *m, const aos2_frame_view_t *f, const aos2_proj_points_t *p, int mode, int thr,
                          int check_ori, int32_t *match_f, int32_t *nmatches)
{
    if (!m || !match_f || !nmatches) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = check_frame(f);
    if (st) return st;
    if ((st = check_points(p, mode))) return st;
    if ((st = matcher_init(m))) return st;
    Arena A{m};
    // one slice of n_f entries per point, so that no window can overflow its slice
    const size_t pool_cap = (size_t)p->n_pts * (size_t)f->n_f;
    FrameDev F;
    ProjGenDev P;
    int32_t *d_match, *d_bin, *d_n, *d_choice;
    QuerySlot *d_slots;
    frame_dev(A, f, F);
    points_dev(A, p, mode, f->n_levels, P);
    A.scratch(d_match, (size_t)f->n_f * 4 + 4);
    A.scratch(d_bin, (size_t)f->n_f * 4 + 4);
    A.scratch(d_n, 8);   // nmatches, entry counter
    A.scratch(d_slots, (size_t)(p->n_pts + 1) * sizeof(QuerySlot));
    A.scratch(d_choice, (size_t)(p->n_pts + 1) * 4);
    Entry *d_pool;
    if ((st = pool_reserve(m, pool_cap, "projection search from a keyframe", d_pool))) return st;
    if ((st = A.upload())) return st;
    AOS2_HIP_CHECK(hipMemsetAsync(d_n + 1, 0, 4, m->stream));
    if ((st = A.begin())) return st;
    if (p->n_pts > 0)
        hipLaunchKernelGGL(projgen_entries_kernel, dim3(p->n_pts), dim3(64), 0, m->stream, F, P, d_slots, d_pool, d_n + 1,
                           (int)pool_cap);
    if (use_fix_resolve(m, f->n_f))
        hipLaunchKernelGGL(projgen_resolve_fix_kernel, dim3(1), dim3(1024), (size_t)f->n_f * 8 + 16, m->stream, F, P, thr, check_ori,
                           d_slots, d_pool, d_match, d_bin, d_n, d_choice);
    else
        hipLaunchKernelGGL(projgen_resolve_kernel, dim3(1), dim3(64), (size_t)f->n_f + 16, m->stream, F, P, thr, check_ori, d_slots,
                           d_pool, d_match, d_bin, d_n);
    if (f->n_f > 0) A.fetch(match_f, d_match, (size_t)f->n_f * 4);
    A.fetch(nmatches, d_n, 4);
    return A.end();
}

int aos2_matcher_search_by_projection_kf(aos2_matcher_t *m, const aos2_frame_view_t *kf, const aos2_proj_points_t *p,
                                         int32_t *match_f, int32_t *nmatches)
{
    return projgen_serial(m, kf, p, 2, TH_LOW, 0, match_f, nmatches);
}

int aos2_matcher_search_by_projection_reloc(aos2_matcher_t *m, const aos2_frame_view_t *frame, const aos2_proj_points_t *p,
                                            int orb_dist, int32_t *match_f, int32_t *nmatches)
{
    if (!m) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    return projgen_serial(m, frame, p, 4, orb_dist, m->check_ori, match_f, nmatches);
}

int aos2_matcher_search_for_initialization(aos2_matcher_t *m, const aos2_frame_view_t *f2, int n1, const uint8_t *desc1,
                                           const int32_t *octave1, const float *angle1, const float *prev_xy,
                                           int window_size, int32_t *match12, int32_t *nmatches)
{
    if (!m || n1 < 0 || !nmatches || (n1 > 0 && (!desc1 || !octave1 || !angle1 || !prev_xy || !match12))) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = check_frame(f2);
    if (st) return st;
    *nmatches = 0;
    if (n1 == 0) return AOS2_OK;
    if (n1 >= 65535 || f2->n_f > 15000) {
        set_error("SearchForInitialization: %d x %d features exceed the LDS match tables (65534 / 15000)", n1, f2->n_f);
        return AOS2_ERR_CAPACITY;
    }
    if ((st = matcher_init(m))) return st;
    Arena A{m};
    const size_t n = (size_t)n1, pool_cap = n * (size_t)f2->n_f;
    FrameDev F;
    InitDev P{};
    int32_t *d_match, *d_n;   // match12 | match21; nmatches, entry counter
    QuerySlot *d_slots;
    frame_dev(A, f2, F);
    P.n1 = n1;
    P.window = (float)window_size;
    A.in(P.desc1, desc1, n * 32);
    A.in(P.octave1, octave1, n * 4);
    A.in(P.angle1, angle1, n * 4);
    A.in(P.prev_xy, prev_xy, n * 8);
    A.scratch(d_match, n * 8 + 8);
    A.scratch(d_n, 8);
    A.scratch(d_slots, (n + 1) * sizeof(QuerySlot));
    Entry *d_pool;
    if ((st = pool_reserve(m, pool_cap, "initialization search", d_pool))) return st;
    if ((st = A.upload())) return st;
    AOS2_HIP_CHECK(hipMemsetAsync(d_n + 1, 0, 4, m->stream));
    if ((st = A.begin())) return st;
    hipLaunchKernelGGL(init_entries_kernel, dim3(n1), dim3(64), 0, m->stream, F, P, d_slots, d_pool, d_n + 1, (int)pool_cap);
    hipLaunchKernelGGL(init_resolve_kernel, dim3(1), dim3(64), (size_t)f2->n_f * 4 + 16, m->stream, F, P, m->nnratio, m->check_ori,
                       d_slots, d_pool, d_match, d_match + n1, d_n);
    A.fetch(match12, d_match, n * 4);
    A.fetch(nmatches, d_n, 4);
    return A.end();
}

}  // extern "C"
