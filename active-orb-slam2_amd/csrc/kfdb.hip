// KeyFrameDatabase (src/KeyFrameDatabase.cc) on the device: the BowVectors of the keyframes resident in one arena, and the
// candidates of DetectLoopCandidates (:76-197) / DetectRelocalizationCandidates (:199-309) for a batch of queries in one call.
//
// The reference walks an inverted file; its result depends on that file only through three things: how many words a keyframe
// shares with the query, which keyframe the walk meets first (ascending first common word, then add order), and the L1 score of
// the pairs that share enough.  The device forms those per (query, added slot) pair without the file:
//   k_kfdb_walk    a wave per pair: 64 words of the slot's row per round, a binary search of the query's row in LDS per lane, the common
//                  words and the first one from ballots, the double sum as one chain over the ballot's bits in lane order
//   k_kfdb_head    the number of sharing slots and maxCommonWords of every query
//   k_kfdb_rank    the place of every scored slot in the scored list (and of every sharing slot in lKFsSharingWords, if that list
//                  is wanted) by counting smaller keys (keys are distinct)
//   k_kfdb_select  a workgroup per query: the cut, the scored and matched lists, the accumulation, the retain and the dedupe
// The arithmetic is csrc/kfdb.h, shared with aos2_debug_kfdb_host, which runs the reference's own algorithm on one core.
#include <algorithm>
#include <climits>
#include <vector>

#include "aos2_common.h"
#include "kfdb.h"
#include "wave_ops.h"

using namespace aos2;

namespace {

constexpr int kNT = 256;            // threads of every workgroup here
constexpr int kWaves = kNT / 64;
constexpr int kSlotsPerWave = 2;    // pairs a wave of k_kfdb_walk takes: the query is staged once per 8 pairs, and one query against a
                                    // few thousand slots still fills the device
constexpr int kStage = 2048;        // query words staged in LDS (24 KiB); a longer query is read from memory
constexpr uint64_t kNoKey = ~0ull;

struct SlotDev {
    int64_t off;
    int32_t len;
    int32_t rank;   // place among the added slots in add order, -1: not added
    int32_t neigh[AOS2_KFDB_NEIGHBOURS];
};

struct QueryDev {
    const uint32_t *w;
    const double *v;
    int32_t n, mode;
    float min_score;
    int32_t excl_off, n_excl;   // LOOP: ranks of the excluded added slots
    int32_t want;               // bit 0: scored list, bit 1: sharing list
};

struct HeadDev {
    int32_t n_sharing, max_words;   // formed by k_kfdb_head
    int32_t n_scored;               // formed by k_kfdb_rank (an integer atomic per scored slot; zeroed before)
    int32_t min_words, n_matched, n_candidates;
    float best_acc;
    uint32_t pool_off;              // where k_kfdb_select packed this query's lists
};

struct Scratch {   // [nq][n_added] each
    int32_t *words;
    uint32_t *first;
    float *score;
    int32_t *mark;     // dedupe: the first retained entry whose pBestKF is this slot
    int32_t *sh;       // lKFsSharingWords as ranks
    int32_t *sc;       // the scored list as ranks
    int32_t *m;        // lScoreAndMatch as ranks
    float *acc;        // lAccScoreAndMatch
    int32_t *best;
    int32_t *cand;     // the returned slots
};

// One (query, slot) pair by a wave: nw = common words, fw = the first of them, s = the sum of their terms in ascending word id.
// The lanes take 64 words of the SLOT's row per round (one coalesced load) and search the QUERY's ascending row, which sits in
// LDS: the ten dependent probes of a search cost LDS latency, not memory latency.  The common words come up in ascending word
// id either way round, so the first of them and the order of the sum are the reference's.
__device__ __forceinline__ void pair_wave(const uint32_t *qw, const double *qv, int nq, const uint32_t *sw, const double *sv, int ns,
                                          int &nw, uint32_t &fw, double &s)
{
    const int lane = threadIdx.x & 63;
    nw = 0;
    fw = 0;
    s = 0.0;
    if (nq <= 0) return;
    const uint32_t lo = qw[0], hi = qw[nq - 1];
    for (int base = 0; base < ns; base += 64) {
        const int i = base + lane;
        const bool in = i < ns;
        const uint32_t w = in ? sw[i] : 0u;
        int p = -1;
        if (in && w >= lo && w <= hi) p = kfdb_find(qw, nq, w);
        unsigned long long mask = __ballot(p >= 0);
        if (mask == 0) continue;
        const double t = p >= 0 ? kfdb_term(qv[p], sv[i]) : 0.0;   // vi = the query's value: the first argument of score()
        if (nw == 0) fw = (uint32_t)__builtin_amdgcn_readlane((int)w, __builtin_amdgcn_readfirstlane(__builtin_ctzll(mask)));
        nw += __popcll(mask);
        while (mask) {   // lane order = ascending word id: the reference's order of additions
            const int b = __builtin_amdgcn_readfirstlane(__builtin_ctzll(mask));
            s += readlane_f64(t, b);
            mask &= mask - 1;
        }
    }
}

// the query's rows, staged in LDS when they fit
__device__ __forceinline__ void stage_query(const QueryDev &q, uint32_t *s_w, double *s_v, const uint32_t *&qw, const double *&qv)
{
    qw = q.w;
    qv = q.v;
    if (q.n <= kStage) {
        for (int i = threadIdx.x; i < q.n; i += kNT) {
            s_w[i] = q.w[i];
            s_v[i] = q.v[i];
        }
        qw = s_w;
        qv = s_v;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kNT) void k_kfdb_walk(const QueryDev *Q, const uint32_t *aw, const double *av, const SlotDev *S,
                                                   const int32_t *added, int n_added, const int32_t *excl, Scratch X)
{
    __shared__ uint32_t s_w[kStage];
    __shared__ double s_v[kStage];
    const int q = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const QueryDev qd = Q[q];
    const uint32_t *qw;
    const double *qv;
    stage_query(qd, s_w, s_v, qw, qv);
    for (int k = 0; k < kSlotsPerWave; ++k) {
        const int a = (blockIdx.x * kWaves + wave) * kSlotsPerWave + k;   // wave-uniform
        if (a >= n_added) break;
        bool ex = false;
        if (qd.mode == AOS2_KFDB_LOOP)
            for (int e = lane; e < qd.n_excl; e += 64) ex |= excl[qd.excl_off + e] == a;
        const bool excluded = __ballot(ex) != 0;
        const SlotDev sd = S[added[a]];
        int nw = 0;
        uint32_t fw = 0;
        double s = 0.0;
        if (!excluded) pair_wave(qw, qv, qd.n, aw + sd.off, av + sd.off, sd.len, nw, fw, s);
        if (lane == 0) {
            const size_t o = (size_t)q * n_added + a;
            X.words[o] = nw;
            X.first[o] = fw;
            X.score[o] = kfdb_score(s);
            X.mark[o] = INT_MAX;
        }
    }
}

// lKFsSharingWords.size() and maxCommonWords (:113-118 / :228-233) of every query: a workgroup per query over its row of word
// counts.  (Formed by atomics of the walk's waves they cost more than the walk: thousands of updates of one address.)
__global__ __launch_bounds__(kNT) void k_kfdb_head(int n_added, Scratch X, HeadDev *H)
{
    __shared__ int32_t s_n[kWaves], s_max[kWaves];
    const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t row = (size_t)q * n_added;
    int n = 0, mx = 0;
    for (int a = threadIdx.x; a < n_added; a += kNT) {
        const int wd = X.words[row + a];
        n += wd > 0;
        mx = max(mx, wd);
    }
    n = wave_sum_i32(n);
    mx = wave_max_i32(mx);
    if (lane == 0) {
        s_n[wave] = n;
        s_max[wave] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) {
            n += s_n[w];
            mx = max(mx, s_max[w]);
        }
        H[q].n_sharing = n;
        H[q].max_words = mx;
    }
}

// The places in the reference's lists by counting smaller keys (keys are distinct): of every scored slot among the scored ones,
// always, and of every sharing slot among the sharing ones when the caller wants lKFsSharingWords itself.  Workgroups none of
// whose slots needs a place leave at once: without the sharing list only those that hold a scored slot walk the keys.
__global__ __launch_bounds__(kNT) void k_kfdb_rank(const QueryDev *Q, int n_added, Scratch X, HeadDev *H)
{
    __shared__ uint64_t s_key[kNT];
    __shared__ uint8_t s_scored[kNT];
    const int q = blockIdx.y;
    if (H[q].n_sharing == 0) return;
    const int min_words = kfdb_min_common(H[q].max_words);
    const bool want_sharing = (Q[q].want & 2) != 0;
    const size_t row = (size_t)q * n_added;
    const int a = blockIdx.x * kNT + threadIdx.x;
    const int wd = a < n_added ? X.words[row + a] : 0;
    const uint64_t key = wd > 0 ? kfdb_key(X.first[row + a], (uint32_t)a) : kNoKey;
    const bool scored = wd > min_words, listed = want_sharing && wd > 0;
    if (!__syncthreads_or(scored || listed)) return;
    int before = 0, scored_before = 0;
    for (int base = 0; base < n_added; base += kNT) {
        const int b = base + threadIdx.x;
        const int wb = b < n_added ? X.words[row + b] : 0;
        s_key[threadIdx.x] = wb > 0 ? kfdb_key(X.first[row + b], (uint32_t)b) : kNoKey;
        s_scored[threadIdx.x] = wb > min_words;
        __syncthreads();
        if (scored || listed)
            for (int j = 0; j < kNT; ++j) {
                const int less = s_key[j] < key;
                before += less;
                scored_before += less & s_scored[j];
            }
        __syncthreads();
    }
    if (listed) X.sh[row + before] = a;
    if (scored) {
        X.sc[row + scored_before] = a;
        atomicAdd(&H[q].n_scored, 1);
    }
}

// what a neighbour contributes to the accumulation of query q (:159 / :273-276)
struct LookDev {
    const QueryDev *Q;
    const HeadDev *H;
    const SlotDev *S;
    const float *reloc;
    const int32_t *words;
    const float *score;
    int q, n_added, n_slots, mode, min_words;
    __device__ bool operator()(int32_t slot, float &val) const
    {
        if (slot >= n_slots) return false;
        const int r = S[slot].rank;
        if (r < 0) return false;
        const size_t o = (size_t)q * n_added + r;
        const int wd = words[o];
        if (mode == AOS2_KFDB_LOOP) {
            if (wd <= min_words) return false;
            val = score[o];
            return true;
        }
        if (wd <= 0) return false;
        if (wd > min_words) {
            val = score[o];
            return true;
        }
        // shares a word, not scored: mRelocScore as the last RELOC query that scored the slot left it -- an earlier query of
        // this call, or reloc_score as it was before the call
        for (int j = q - 1; j >= 0; --j) {
            if (Q[j].mode != AOS2_KFDB_RELOC) continue;
            const size_t oj = (size_t)j * n_added + r;
            if (words[oj] > kfdb_min_common(H[j].max_words)) {
                val = score[oj];
                return true;
            }
        }
        val = reloc[slot];
        return true;
    }
};

__global__ __launch_bounds__(kNT) void k_kfdb_select(const QueryDev *Q, const SlotDev *S, int n_slots, const int32_t *added,
                                                     int n_added, const float *reloc, Scratch X, HeadDev *H, uint32_t *pool,
                                                     uint32_t *pool_cursor)
{
    __shared__ int32_t s_wsum[kWaves];
    __shared__ float s_max[kNT];
    __shared__ uint32_t s_base;
    const int q = blockIdx.x, tid = threadIdx.x;
    const QueryDev qd = Q[q];
    const size_t row = (size_t)q * n_added;
    const int n_sh = H[q].n_sharing, max_words = H[q].max_words;
    const int min_words = kfdb_min_common(max_words);
    const float start = qd.mode == AOS2_KFDB_LOOP ? qd.min_score : 0.0f;

    // lScoreAndMatch (:125-139 / :242-253): the scored list, which k_kfdb_rank has put in order, cut at minScore
    const int n_sc = H[q].n_scored;
    int n_m = 0;
    for (int base = 0; base < n_sc; base += kNT) {
        const int i = base + tid;
        const int a = i < n_sc ? X.sc[row + i] : -1;
        const bool f_m = a >= 0 && (qd.mode == AOS2_KFDB_RELOC || X.score[row + a] >= qd.min_score);
        int tot_m;
        const int em = block_excl_scan_i32<kNT>(f_m, s_wsum, tot_m);
        if (f_m) X.m[row + n_m + em] = a;
        __syncthreads();
        n_m += tot_m;
    }

    // the accumulation (:148-173 / :262-287): an entry per thread, its neighbours in row order
    const LookDev look{Q, H, S, reloc, X.words, X.score, q, n_added, n_slots, qd.mode, min_words};
    float best_acc = start;
    for (int i = tid; i < n_m; i += kNT) {
        const int a = X.m[row + i];
        const int32_t slot = added[a];
        float acc;
        int32_t best;
        kfdb_accumulate(X.score[row + a], slot, S[slot].neigh, look, acc, best);
        X.acc[row + i] = acc;
        X.best[row + i] = best;
        if (acc > best_acc) best_acc = acc;   // (:171 / :285; over the whole list: the maximum, the start value on ties)
    }
    s_max[tid] = best_acc;
    __syncthreads();
    for (int w = kNT / 2; w > 0; w >>= 1) {
        if (tid < w && s_max[tid + w] > s_max[tid]) s_max[tid] = s_max[tid + w];
        __syncthreads();
    }
    best_acc = s_max[0];
    const float retain = kfdb_retain(best_acc);

    // retain and dedupe (:182-193 / :294-306): an entry is returned if no earlier retained entry has the same pBestKF
    for (int i = tid; i < n_m; i += kNT)
        if (X.acc[row + i] > retain) atomicMin(&X.mark[row + S[X.best[row + i]].rank], i);
    __syncthreads();
    int n_c = 0;
    for (int base = 0; base < n_m; base += kNT) {
        const int i = base + tid;
        bool f = false;
        int32_t best = -1;
        if (i < n_m && X.acc[row + i] > retain) {
            best = X.best[row + i];
            f = X.mark[row + S[best].rank] == i;
        }
        int tot;
        const int e = block_excl_scan_i32<kNT>(f, s_wsum, tot);
        if (f) X.cand[row + n_c + e] = best;
        __syncthreads();
        n_c += tot;
    }
    // the lists, packed for one copy to the host: candidates | scored slot, words, score | sharing slot, words
    const uint32_t need = (uint32_t)n_c + ((qd.want & 1) ? 3u * n_sc : 0u) + ((qd.want & 2) ? 2u * n_sh : 0u);
    if (tid == 0) {
        s_base = atomicAdd(pool_cursor, need);
        H[q].min_words = min_words;
        H[q].n_matched = n_m;
        H[q].n_candidates = n_c;
        H[q].best_acc = best_acc;
        H[q].pool_off = s_base;
    }
    __syncthreads();
    uint32_t *out = pool + s_base;
    for (int i = tid; i < n_c; i += kNT) out[i] = (uint32_t)X.cand[row + i];
    out += n_c;
    if (qd.want & 1) {
        for (int i = tid; i < n_sc; i += kNT) {
            const int a = X.sc[row + i];
            out[i] = (uint32_t)added[a];
            out[n_sc + i] = (uint32_t)X.words[row + a];
            out[2 * n_sc + i] = __float_as_uint(X.score[row + a]);
        }
        out += 3 * n_sc;
    }
    if (qd.want & 2)
        for (int i = tid; i < n_sh; i += kNT) {
            const int a = X.sh[row + i];
            out[i] = (uint32_t)added[a];
            out[n_sh + i] = (uint32_t)X.words[row + a];
        }
}

// aos2_kfdb_scores: a wave per explicit slot
__global__ __launch_bounds__(kNT) void k_kfdb_scores(QueryDev qd, const uint32_t *aw, const double *av, const SlotDev *S,
                                                     const int32_t *slots, int n, float *scores)
{
    __shared__ uint32_t s_w[kStage];
    __shared__ double s_v[kStage];
    const uint32_t *qw;
    const double *qv;
    stage_query(qd, s_w, s_v, qw, qv);
    const int i = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i >= n) return;
    const SlotDev sd = S[slots[i]];
    int nw;
    uint32_t fw;
    double s;
    pair_wave(qw, qv, qd.n, aw + sd.off, av + sd.off, sd.len, nw, fw, s);
    if ((threadIdx.x & 63) == 0) scores[i] = kfdb_score(s);
}

enum { kFree = 0, kPut = 1, kAdded = 2 };

struct Slot {
    int64_t off = 0;
    int32_t len = 0;
    int32_t state = kFree;
    uint64_t seq = 0;       // the add counter's value at add()
    float reloc = 0.0f;     // mRelocScore
    int32_t neigh[AOS2_KFDB_NEIGHBOURS];
};

struct QueryOut {   // one query's result before it goes into the caller's buffers
    std::vector<int32_t> cand, sc_slot, sc_words, sh_slot, sh_words;
    std::vector<float> sc_score;
    int32_t max_words = 0, min_words = 0, n_matched = 0;
    float best_acc = 0;
};

struct QueryHost {   // a validated query with its rows on the host (host path) or on the device (device path)
    const uint32_t *w = nullptr;
    const double *v = nullptr;
    int n = 0;
};

}  // namespace

struct aos2_kfdb {
    int device = 0;
    uint32_t n_words = 0;
    std::vector<uint32_t> w;            // the arena's mirror: every put row, words and values
    std::vector<double> v;
    std::vector<Slot> slots;
    std::vector<int32_t> free_slots;
    uint64_t add_counter = 0;
    std::vector<int32_t> added;         // the added slots in add order
    std::vector<int32_t> rank_of;       // slot -> place in `added`, -1
    std::vector<std::vector<int32_t>> inv;   // mvInvertedFile of the host tap
    // members of the host tap's keyframes: mnLoopQuery / mnRelocQuery, mnLoopWords / mnRelocWords, mLoopScore
    std::vector<uint64_t> q_stamp, x_stamp;
    std::vector<int32_t> q_words;
    std::vector<float> q_score;
    uint64_t stamp = 0;
    // device side
    bool dev_ready = false, table_dirty = true, reloc_dirty = true;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {};
    DevBuf<uint32_t> d_w;
    DevBuf<double> d_v;
    int64_t d_cap = 0, d_used = 0;
    DevBuf<SlotDev> d_slots;
    DevBuf<int32_t> d_added, d_excl, d_i32, d_list;
    DevBuf<float> d_reloc, d_f32;
    DevBuf<uint32_t> d_u32, d_pool, d_qw;
    DevBuf<double> d_qv;
    DevBuf<QueryDev> d_q;
    DevBuf<HeadDev> d_head;
    PinnedBuf<uint32_t> h_pool;
    PinnedBuf<HeadDev> h_head;
    float last_ms = 0;
};

namespace {

bool slot_put(const aos2_kfdb *db, int32_t s) { return s >= 0 && (size_t)s < db->slots.size() && db->slots[s].state != kFree; }

void refresh_ranks(aos2_kfdb *db)
{
    db->rank_of.assign(db->slots.size(), -1);
    for (size_t a = 0; a < db->added.size(); ++a) db->rank_of[db->added[a]] = (int32_t)a;
}

int put_row(aos2_kfdb *db, const uint32_t *words, const double *values, int n, int32_t *slot)
{
    for (int i = 0; i < n; ++i)
        if (words[i] >= db->n_words || (i > 0 && words[i] <= words[i - 1])) {
            set_error("kfdb put: word ids must ascend and lie below the vocabulary's %u words", db->n_words);
            return AOS2_ERR_ARG;
        }
    int32_t s;
    if (!db->free_slots.empty()) {
        s = db->free_slots.back();
        db->free_slots.pop_back();
    } else {
        s = (int32_t)db->slots.size();
        db->slots.emplace_back();
        db->q_stamp.push_back(0);
        db->x_stamp.push_back(0);
        db->q_words.push_back(0);
        db->q_score.push_back(0.0f);
        db->rank_of.push_back(-1);
    }
    Slot &S = db->slots[s];
    S = Slot();
    S.off = (int64_t)db->w.size();
    S.len = n;
    S.state = kPut;
    std::fill(S.neigh, S.neigh + AOS2_KFDB_NEIGHBOURS, -1);
    db->w.insert(db->w.end(), words, words + n);
    db->v.insert(db->v.end(), values, values + n);
    db->q_stamp[s] = db->x_stamp[s] = 0;
    db->table_dirty = db->reloc_dirty = true;
    *slot = s;
    return AOS2_OK;
}

void erase_slot(aos2_kfdb *db, int32_t s)   // erase(KeyFrame*) :48-67
{
    const Slot &S = db->slots[s];
    for (int i = 0; i < S.len; ++i) {
        std::vector<int32_t> &l = db->inv[db->w[S.off + i]];
        for (size_t k = 0; k < l.size(); ++k)
            if (l[k] == s) {
                l.erase(l.begin() + k);
                break;
            }
    }
    db->added.erase(std::find(db->added.begin(), db->added.end(), s));
    db->slots[s].state = kPut;
    refresh_ranks(db);
    db->table_dirty = true;
}

int init_device(aos2_kfdb *db)
{
    if (int st = bind_device(db->device)) return st;
    if (db->dev_ready) return AOS2_OK;
    if (int st = stream_create(&db->stream, false)) return st;
    for (auto &e : db->ev) AOS2_HIP_CHECK(hipEventCreate(&e));
    db->dev_ready = true;
    return AOS2_OK;
}

// the arena (it grows by doubling; a growth uploads the mirror again), the slot table, the added list and reloc_score
int sync_device(aos2_kfdb *db)
{
    int st;
    if ((st = init_device(db))) return st;
    const int64_t used = (int64_t)db->w.size();
    if (used > db->d_cap || !db->d_w.p) {
        int64_t cap = std::max<int64_t>(db->d_cap, 1 << 16);
        while (cap < used) cap *= 2;
        AOS2_HIP_CHECK(hipStreamSynchronize(db->stream));
        db->d_w.release();
        db->d_v.release();
        if ((st = db->d_w.alloc((size_t)cap)) || (st = db->d_v.alloc((size_t)cap))) return st;
        db->d_cap = cap;
        db->d_used = 0;
    }
    if (used > db->d_used) {
        const size_t o = (size_t)db->d_used, n = (size_t)(used - db->d_used);
        AOS2_HIP_CHECK(hipMemcpyAsync(db->d_w.p + o, db->w.data() + o, n * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
        AOS2_HIP_CHECK(hipMemcpyAsync(db->d_v.p + o, db->v.data() + o, n * sizeof(double), hipMemcpyHostToDevice, db->stream));
        db->d_used = used;
    }
    const size_t ns = db->slots.size();
    if (db->table_dirty) {
        std::vector<SlotDev> t(ns);
        for (size_t s = 0; s < ns; ++s) {
            const Slot &S = db->slots[s];
            t[s].off = S.off;
            t[s].len = S.state == kFree ? 0 : S.len;
            t[s].rank = db->rank_of[s];
            for (int k = 0; k < AOS2_KFDB_NEIGHBOURS; ++k) t[s].neigh[k] = S.neigh[k];
        }
        if ((st = db->d_slots.alloc(ns)) || (st = db->d_added.alloc(db->added.size()))) return st;
        if (ns) AOS2_HIP_CHECK(hipMemcpyAsync(db->d_slots.p, t.data(), ns * sizeof(SlotDev), hipMemcpyHostToDevice, db->stream));
        if (!db->added.empty())
            AOS2_HIP_CHECK(hipMemcpyAsync(db->d_added.p, db->added.data(), db->added.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                          db->stream));
        AOS2_HIP_CHECK(hipStreamSynchronize(db->stream));   // (t is pageable and leaves scope)
        db->table_dirty = false;
    }
    if (db->reloc_dirty) {
        std::vector<float> r(ns);
        for (size_t s = 0; s < ns; ++s) r[s] = db->slots[s].reloc;
        if ((st = db->d_reloc.alloc(ns))) return st;
        if (ns) AOS2_HIP_CHECK(hipMemcpyAsync(db->d_reloc.p, r.data(), ns * sizeof(float), hipMemcpyHostToDevice, db->stream));
        AOS2_HIP_CHECK(hipStreamSynchronize(db->stream));
        db->reloc_dirty = false;
    }
    return AOS2_OK;
}

// everything that is AOS2_ERR_ARG about a query, checked before anything runs
int check_query(const aos2_kfdb *db, const aos2_kfdb_query_t &q, bool need_mode)
{
    if (need_mode && q.mode != AOS2_KFDB_LOOP && q.mode != AOS2_KFDB_RELOC) {
        set_error("kfdb: mode %d", q.mode);
        return AOS2_ERR_ARG;
    }
    if (q.slot >= 0) {
        if (!slot_put(db, q.slot)) {
            set_error("kfdb: query slot %d is not put", q.slot);
            return AOS2_ERR_ARG;
        }
    } else {
        if (q.n_words < 0 || (q.n_words > 0 && (!q.words || !q.values))) {
            set_error("kfdb: query without words");
            return AOS2_ERR_ARG;
        }
        if (!q.on_device)
            for (int i = 0; i < q.n_words; ++i)
                if (q.words[i] >= db->n_words || (i > 0 && q.words[i] <= q.words[i - 1])) {
                    set_error("kfdb: query word ids must ascend and lie below the vocabulary's %u words", db->n_words);
                    return AOS2_ERR_ARG;
                }
    }
    if (need_mode && q.mode == AOS2_KFDB_LOOP && (q.n_excluded < 0 || (q.n_excluded > 0 && !q.excluded))) {
        set_error("kfdb: excluded slots");
        return AOS2_ERR_ARG;
    }
    return AOS2_OK;
}

int check_detect(const aos2_kfdb *db, const aos2_kfdb_query_t *queries, const aos2_kfdb_result_t *results, int nq)
{
    if (!db || nq < 0 || (nq > 0 && (!queries || !results))) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    for (int i = 0; i < nq; ++i) {
        if (int st = check_query(db, queries[i], true)) return st;
        const aos2_kfdb_result_t &r = results[i];
        const bool sc = r.scored_slot || r.scored_words || r.scored_score, sh = r.sharing_slot || r.sharing_words;
        if (r.cap_candidates < 0 || (r.cap_candidates > 0 && !r.candidates) ||
            (sc && (!r.scored_slot || !r.scored_words || !r.scored_score || r.cap_scored < 0)) ||
            (sh && (!r.sharing_slot || !r.sharing_words || r.cap_sharing < 0))) {
            set_error("kfdb: result %d: a list without its arrays or with a negative capacity", i);
            return AOS2_ERR_ARG;
        }
    }
    return AOS2_OK;
}

int emit(const QueryOut &o, aos2_kfdb_result_t &r)
{
    int st = AOS2_OK;
    auto put = [&](const auto &src, auto *dst, int cap) {
        if (!dst) return;
        if ((int)src.size() > cap) st = AOS2_ERR_CAPACITY;
        std::copy(src.begin(), src.begin() + std::min<size_t>(src.size(), (size_t)cap), dst);
    };
    r.n_candidates = (int32_t)o.cand.size();
    if ((int)o.cand.size() > r.cap_candidates) st = AOS2_ERR_CAPACITY;
    put(o.cand, r.candidates, r.cap_candidates);
    r.n_sharing = (int32_t)o.sh_slot.size();
    r.max_common_words = o.max_words;
    r.min_common_words = o.min_words;
    r.n_scored = (int32_t)o.sc_slot.size();
    r.n_matched = o.n_matched;
    r.best_acc_score = o.best_acc;
    put(o.sc_slot, r.scored_slot, r.cap_scored);
    put(o.sc_words, r.scored_words, r.cap_scored);
    put(o.sc_score, r.scored_score, r.cap_scored);
    put(o.sh_slot, r.sharing_slot, r.cap_sharing);
    put(o.sh_words, r.sharing_words, r.cap_sharing);
    if (st) set_error("kfdb: a result list did not fit its capacity");
    return st;
}

// the query's rows on the host (a slot: the mirror; device arrays: copied down into `keep`)
int query_on_host(aos2_kfdb *db, const aos2_kfdb_query_t &q, std::vector<uint32_t> &kw, std::vector<double> &kv, QueryHost &out)
{
    if (q.slot >= 0) {
        const Slot &S = db->slots[q.slot];
        out.w = db->w.data() + S.off;
        out.v = db->v.data() + S.off;
        out.n = S.len;
        return AOS2_OK;
    }
    out.w = q.words;
    out.v = q.values;
    out.n = q.n_words;
    if (q.on_device && q.n_words > 0) {
        if (int st = bind_device(db->device)) return st;
        kw.resize(q.n_words);
        kv.resize(q.n_words);
        AOS2_HIP_CHECK(hipMemcpy(kw.data(), q.words, sizeof(uint32_t) * q.n_words, hipMemcpyDeviceToHost));
        AOS2_HIP_CHECK(hipMemcpy(kv.data(), q.values, sizeof(double) * q.n_words, hipMemcpyDeviceToHost));
        for (int i = 0; i < q.n_words; ++i)
            if (kw[i] >= db->n_words || (i > 0 && kw[i] <= kw[i - 1])) {
                set_error("kfdb: query word ids must ascend and lie below the vocabulary's %u words", db->n_words);
                return AOS2_ERR_ARG;
            }
        out.w = kw.data();
        out.v = kv.data();
    }
    return AOS2_OK;
}

// src/KeyFrameDatabase.cc:76-197 / :199-309 over the inverted file, statement by statement
void host_detect(aos2_kfdb *db, const aos2_kfdb_query_t &q, const QueryHost &Q, QueryOut &o)
{
    const bool loop = q.mode == AOS2_KFDB_LOOP;
    const uint64_t id = ++db->stamp;   // pKF->mnId / F->mnId: an id that does not repeat
    o = QueryOut();
    o.best_acc = loop ? q.min_score : 0.0f;
    if (loop)
        for (int i = 0; i < q.n_excluded; ++i)
            if (slot_put(db, q.excluded[i])) db->x_stamp[q.excluded[i]] = id;   // spConnectedKeyFrames
    for (int i = 0; i < Q.n; ++i)
        for (int32_t s : db->inv[Q.w[i]]) {
            if (db->q_stamp[s] != id) {
                db->q_words[s] = 0;
                if (!loop || db->x_stamp[s] != id) {
                    db->q_stamp[s] = id;
                    o.sh_slot.push_back(s);
                }
            }
            db->q_words[s]++;
        }
    if (o.sh_slot.empty()) return;
    for (int32_t s : o.sh_slot) {
        o.sh_words.push_back(db->q_words[s]);
        if (db->q_words[s] > o.max_words) o.max_words = db->q_words[s];
    }
    const int min_words = o.min_words = kfdb_min_common(o.max_words);
    std::vector<std::pair<float, int32_t>> match;
    for (int32_t s : o.sh_slot) {
        if (db->q_words[s] <= min_words) continue;
        const Slot &S = db->slots[s];
        const float si = kfdb_score(kfdb_merge_sum(Q.w, Q.v, Q.n, db->w.data() + S.off, db->v.data() + S.off, S.len));
        if (loop) db->q_score[s] = si;
        else {
            db->slots[s].reloc = si;
            db->reloc_dirty = true;
        }
        o.sc_slot.push_back(s);
        o.sc_words.push_back(db->q_words[s]);
        o.sc_score.push_back(si);
        if (!loop || si >= q.min_score) match.emplace_back(si, s);
    }
    o.n_matched = (int32_t)match.size();
    if (match.empty()) return;
    auto look = [&](int32_t s, float &val) {
        if (!slot_put(db, s) || db->q_stamp[s] != id) return false;
        if (loop) {
            if (db->q_words[s] <= min_words) return false;
            val = db->q_score[s];
        } else {
            val = db->slots[s].reloc;
        }
        return true;
    };
    std::vector<std::pair<float, int32_t>> accs;
    for (const auto &m : match) {
        float acc;
        int32_t best;
        kfdb_accumulate(m.first, m.second, db->slots[m.second].neigh, look, acc, best);
        accs.emplace_back(acc, best);
        if (acc > o.best_acc) o.best_acc = acc;
    }
    const float retain = kfdb_retain(o.best_acc);
    for (const auto &e : accs)
        if (e.first > retain && std::find(o.cand.begin(), o.cand.end(), e.second) == o.cand.end()) o.cand.push_back(e.second);
}

// the device path of aos2_kfdb_detect; outs[i] is filled for every query
int device_detect(aos2_kfdb *db, const aos2_kfdb_query_t *queries, const aos2_kfdb_result_t *results, int nq,
                  std::vector<QueryOut> &outs)
{
    int st;
    if ((st = sync_device(db))) return st;
    const int n_added = (int)db->added.size();
    // query descriptors; host rows and the excluded ranks go up in one block each
    std::vector<QueryDev> qd(nq);
    std::vector<uint32_t> hw;
    std::vector<double> hv;
    std::vector<int32_t> excl;
    std::vector<size_t> hoff(nq, 0);
    for (int i = 0; i < nq; ++i) {
        const aos2_kfdb_query_t &q = queries[i];
        QueryDev &d = qd[i];
        d.mode = q.mode;
        d.min_score = q.min_score;
        d.want = ((results[i].scored_slot || q.mode == AOS2_KFDB_RELOC) ? 1 : 0) | (results[i].sharing_slot ? 2 : 0);
        d.excl_off = (int32_t)excl.size();
        if (q.mode == AOS2_KFDB_LOOP)
            for (int e = 0; e < q.n_excluded; ++e)
                if (slot_put(db, q.excluded[e]) && db->rank_of[q.excluded[e]] >= 0) excl.push_back(db->rank_of[q.excluded[e]]);
        d.n_excl = (int32_t)excl.size() - d.excl_off;
        if (q.slot >= 0) {
            d.w = db->d_w.p + db->slots[q.slot].off;
            d.v = db->d_v.p + db->slots[q.slot].off;
            d.n = db->slots[q.slot].len;
        } else if (q.on_device) {
            d.w = q.words;
            d.v = q.values;
            d.n = q.n_words;
        } else {
            hoff[i] = hw.size();
            hw.insert(hw.end(), q.words, q.words + q.n_words);
            hv.insert(hv.end(), q.values, q.values + q.n_words);
            d.n = q.n_words;
        }
    }
    if ((st = db->d_qw.alloc(hw.size())) || (st = db->d_qv.alloc(hv.size())) || (st = db->d_excl.alloc(excl.size())) ||
        (st = db->d_q.alloc(nq)) || (st = db->d_head.alloc(nq + 1)) || (st = db->h_head.alloc(nq + 1)))
        return st;
    for (int i = 0; i < nq; ++i)
        if (queries[i].slot < 0 && !queries[i].on_device) {
            qd[i].w = db->d_qw.p + hoff[i];
            qd[i].v = db->d_qv.p + hoff[i];
        }
    const size_t cells = (size_t)nq * n_added;
    if ((st = db->d_i32.alloc(cells * 7)) || (st = db->d_u32.alloc(cells)) || (st = db->d_f32.alloc(cells * 2)) ||
        (st = db->d_pool.alloc(cells * 6)) || (st = db->h_pool.alloc(cells * 6)))
        return st;
    Scratch X;
    X.words = db->d_i32.p;
    X.mark = X.words + cells;
    X.sh = X.mark + cells;
    X.sc = X.sh + cells;
    X.m = X.sc + cells;
    X.best = X.m + cells;
    X.cand = X.best + cells;
    X.first = db->d_u32.p;
    X.score = db->d_f32.p;
    X.acc = X.score + cells;
    hipStream_t s = db->stream;
    if (!hw.empty()) {
        AOS2_HIP_CHECK(hipMemcpyAsync(db->d_qw.p, hw.data(), hw.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        AOS2_HIP_CHECK(hipMemcpyAsync(db->d_qv.p, hv.data(), hv.size() * sizeof(double), hipMemcpyHostToDevice, s));
    }
    if (!excl.empty()) AOS2_HIP_CHECK(hipMemcpyAsync(db->d_excl.p, excl.data(), excl.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    AOS2_HIP_CHECK(hipMemcpyAsync(db->d_q.p, qd.data(), nq * sizeof(QueryDev), hipMemcpyHostToDevice, s));
    AOS2_HIP_CHECK(hipMemsetAsync(db->d_head.p, 0, (nq + 1) * sizeof(HeadDev), s));
    uint32_t *cursor = (uint32_t *)(db->d_head.p + nq);   // the spare head: the pool's cursor
    AOS2_HIP_CHECK(hipEventRecord(db->ev[0], s));
    const int per_wg = kWaves * kSlotsPerWave;
    hipLaunchKernelGGL(k_kfdb_walk, dim3((n_added + per_wg - 1) / per_wg, nq), dim3(kNT), 0, s, db->d_q.p, db->d_w.p, db->d_v.p,
                       db->d_slots.p, db->d_added.p, n_added, db->d_excl.p, X);
    AOS2_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_kfdb_head, dim3(nq), dim3(kNT), 0, s, n_added, X, db->d_head.p);
    AOS2_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_kfdb_rank, dim3((n_added + kNT - 1) / kNT, nq), dim3(kNT), 0, s, db->d_q.p, n_added, X, db->d_head.p);
    AOS2_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_kfdb_select, dim3(nq), dim3(kNT), 0, s, db->d_q.p, db->d_slots.p, (int)db->slots.size(), db->d_added.p,
                       n_added, db->d_reloc.p, X, db->d_head.p, db->d_pool.p, cursor);
    AOS2_HIP_CHECK(hipGetLastError());
    AOS2_HIP_CHECK(hipEventRecord(db->ev[1], s));
    AOS2_HIP_CHECK(hipMemcpyAsync(db->h_head.p, db->d_head.p, (nq + 1) * sizeof(HeadDev), hipMemcpyDeviceToHost, s));
    AOS2_HIP_CHECK(hipStreamSynchronize(s));
    AOS2_HIP_CHECK(hipEventElapsedTime(&db->last_ms, db->ev[0], db->ev[1]));
    const uint32_t filled = *(const uint32_t *)(db->h_head.p + nq);
    if (filled) {
        AOS2_HIP_CHECK(hipMemcpyAsync(db->h_pool.p, db->d_pool.p, (size_t)filled * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        AOS2_HIP_CHECK(hipStreamSynchronize(s));
    }
    for (int i = 0; i < nq; ++i) {
        const HeadDev &h = db->h_head.p[i];
        QueryOut &o = outs[i];
        const uint32_t *p = db->h_pool.p + h.pool_off;
        o.max_words = h.max_words;
        o.min_words = h.min_words;
        o.n_matched = h.n_matched;
        o.best_acc = h.best_acc;
        o.cand.assign((const int32_t *)p, (const int32_t *)p + h.n_candidates);
        p += h.n_candidates;
        if (qd[i].want & 1) {
            const int n = h.n_scored;
            o.sc_slot.assign((const int32_t *)p, (const int32_t *)p + n);
            o.sc_words.assign((const int32_t *)p + n, (const int32_t *)p + 2 * n);
            o.sc_score.assign((const float *)p + 2 * n, (const float *)p + 3 * n);
            p += 3 * n;
            if (queries[i].mode == AOS2_KFDB_RELOC)   // mRelocScore = si :250: the host's copy follows the device's
                for (int k = 0; k < n; ++k) db->slots[o.sc_slot[k]].reloc = o.sc_score[k];
        } else {
            o.sc_slot.resize(h.n_scored);   // (counts only)
        }
        if (qd[i].want & 2) {
            o.sh_slot.assign((const int32_t *)p, (const int32_t *)p + h.n_sharing);
            o.sh_words.assign((const int32_t *)p + h.n_sharing, (const int32_t *)p + 2 * h.n_sharing);
        } else {
            o.sh_slot.resize(h.n_sharing);
        }
        if (queries[i].mode == AOS2_KFDB_RELOC && h.n_scored > 0) db->reloc_dirty = true;
    }
    return AOS2_OK;
}

int detect(aos2_kfdb *db, const aos2_kfdb_query_t *queries, aos2_kfdb_result_t *results, int nq, bool on_host)
{
    if (int st = check_detect(db, queries, results, nq)) return st;
    if (nq == 0) return AOS2_OK;
    std::vector<QueryOut> outs(nq);
    if (on_host) {
        // device rows come down (and are checked) before any query runs: a refusal leaves reloc_score as it was
        std::vector<QueryHost> Q(nq);
        std::vector<std::vector<uint32_t>> kws(nq);
        std::vector<std::vector<double>> kvs(nq);
        for (int i = 0; i < nq; ++i)
            if (int st = query_on_host(db, queries[i], kws[i], kvs[i], Q[i])) return st;
        for (int i = 0; i < nq; ++i) host_detect(db, queries[i], Q[i], outs[i]);
    } else if (db->added.empty()) {
        for (int i = 0; i < nq; ++i) outs[i].best_acc = queries[i].mode == AOS2_KFDB_LOOP ? queries[i].min_score : 0.0f;
    } else {
        if (int st = device_detect(db, queries, results, nq, outs)) return st;
    }
    int st = AOS2_OK;
    for (int i = 0; i < nq; ++i)
        if (int e = emit(outs[i], results[i])) st = e;
    return st;
}

int check_scores(const aos2_kfdb *db, const aos2_kfdb_query_t *q, const int32_t *slots, int n, const float *scores,
                 const float *min_score)
{
    if (!db || !q || n < 0 || !min_score || (n > 0 && (!slots || !scores))) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if (int st = check_query(db, *q, false)) return st;
    for (int i = 0; i < n; ++i)
        if (!slot_put(db, slots[i])) {
            set_error("kfdb scores: slot %d is not put", slots[i]);
            return AOS2_ERR_ARG;
        }
    return AOS2_OK;
}

// float minScore = 1; ... if(score<minScore) minScore = score (src/LoopClosing.cc:126-140)
void min_from_one(const float *scores, int n, float *min_score)
{
    float m = 1.0f;
    for (int i = 0; i < n; ++i)
        if (scores[i] < m) m = scores[i];
    *min_score = m;
}

}  // namespace

extern "C" {

int aos2_kfdb_create(const aos2_vocabulary_t *voc, int device, aos2_kfdb_t **out)
{
    if (!voc || !out) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if (aos2_vocabulary_scoring(voc) != AOS2_SCORING_L1_NORM) {
        set_error("kfdb: only L1_NORM (the ORB vocabulary's scoring) is implemented");
        return AOS2_ERR_ARG;
    }
    aos2_kfdb *db = new aos2_kfdb();
    db->device = device;
    db->n_words = aos2_vocabulary_size(voc);
    db->inv.resize(db->n_words);
    *out = db;
    return AOS2_OK;
}

void aos2_kfdb_destroy(aos2_kfdb_t *db)
{
    if (!db) return;
    if (db->dev_ready) {
        (void)hipSetDevice(db->device);
        (void)hipStreamSynchronize(db->stream);
        db->d_w.release(); db->d_v.release(); db->d_slots.release(); db->d_added.release(); db->d_excl.release();
        db->d_i32.release(); db->d_list.release(); db->d_reloc.release(); db->d_f32.release(); db->d_u32.release();
        db->d_pool.release(); db->d_qw.release(); db->d_qv.release(); db->d_q.release(); db->d_head.release();
        db->h_pool.release(); db->h_head.release();
        for (auto &e : db->ev) (void)hipEventDestroy(e);
        (void)hipStreamDestroy(db->stream);
    }
    delete db;
}

int aos2_kfdb_put(aos2_kfdb_t *db, const uint32_t *words, const double *values, int n, int32_t *slot)
{
    if (!db || !slot || n < 0 || (n > 0 && (!words || !values))) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    return put_row(db, words, values, n, slot);
}

int aos2_kfdb_put_device(aos2_kfdb_t *db, aos2_vocabulary_t *voc, int batch, const uint32_t *d_words, const double *d_values,
                         const int32_t *d_n_bow, int cap, int32_t *slots)
{
    if (!db || batch < 0 || cap <= 0 || (batch > 0 && (!d_words || !d_values || !d_n_bow || !slots))) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if (batch == 0) return AOS2_OK;
    if (int st = init_device(db)) return st;
    if (voc)
        if (void *vs = aos2_vocabulary_stream(voc)) AOS2_HIP_CHECK(hipStreamSynchronize((hipStream_t)vs));
    // the rows join the arena through its mirror: the counts decide where every row goes, so they have to come down anyway
    std::vector<int32_t> n(batch);
    std::vector<uint32_t> w((size_t)batch * cap);
    std::vector<double> v((size_t)batch * cap);
    AOS2_HIP_CHECK(hipMemcpy(n.data(), d_n_bow, sizeof(int32_t) * batch, hipMemcpyDeviceToHost));
    AOS2_HIP_CHECK(hipMemcpy(w.data(), d_words, sizeof(uint32_t) * w.size(), hipMemcpyDeviceToHost));
    AOS2_HIP_CHECK(hipMemcpy(v.data(), d_values, sizeof(double) * v.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; ++b)
        if (n[b] < 0 || n[b] > cap) {
            set_error("kfdb put: row %d holds %d words of %d", b, n[b], cap);
            return AOS2_ERR_ARG;
        }
    for (int b = 0; b < batch; ++b)
        if (int st = put_row(db, w.data() + (size_t)b * cap, v.data() + (size_t)b * cap, n[b], slots + b)) {
            for (int k = 0; k < b; ++k) aos2_kfdb_drop(db, slots[k]);
            return st;
        }
    return AOS2_OK;
}

int aos2_kfdb_add(aos2_kfdb_t *db, int32_t slot)
{
    if (!db || !slot_put(db, slot) || db->slots[slot].state == kAdded) {
        set_error("kfdb add: slot %d is not put or is added already", slot);
        return AOS2_ERR_ARG;
    }
    Slot &S = db->slots[slot];
    for (int i = 0; i < S.len; ++i) db->inv[db->w[S.off + i]].push_back(slot);   // :44-45
    S.seq = db->add_counter++;
    S.state = kAdded;
    db->rank_of[slot] = (int32_t)db->added.size();
    db->added.push_back(slot);
    db->table_dirty = true;
    return AOS2_OK;
}

int aos2_kfdb_erase(aos2_kfdb_t *db, int32_t slot)
{
    if (!db || !slot_put(db, slot)) {
        set_error("kfdb erase: slot %d is not put", slot);
        return AOS2_ERR_ARG;
    }
    if (db->slots[slot].state == kAdded) erase_slot(db, slot);
    return AOS2_OK;
}

int aos2_kfdb_drop(aos2_kfdb_t *db, int32_t slot)
{
    if (!db || !slot_put(db, slot)) {
        set_error("kfdb drop: slot %d is not put", slot);
        return AOS2_ERR_ARG;
    }
    if (db->slots[slot].state == kAdded) erase_slot(db, slot);
    db->slots[slot].state = kFree;   // (the row's entries stay in the arena unread)
    db->free_slots.push_back(slot);
    db->table_dirty = true;
    return AOS2_OK;
}

int aos2_kfdb_clear(aos2_kfdb_t *db)
{
    if (!db) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    for (int32_t s : db->added) db->slots[s].state = kPut;
    db->added.clear();
    db->inv.assign(db->n_words, std::vector<int32_t>());   // :71-72
    refresh_ranks(db);
    db->table_dirty = true;
    return AOS2_OK;
}

int aos2_kfdb_size(const aos2_kfdb_t *db) { return db ? (int)db->added.size() : 0; }
int64_t aos2_kfdb_arena_capacity(const aos2_kfdb_t *db) { return db ? db->d_cap : 0; }
float aos2_kfdb_last_device_ms(const aos2_kfdb_t *db) { return db ? db->last_ms : 0.0f; }

int aos2_kfdb_set_neighbours(aos2_kfdb_t *db, int n, const int32_t *slots, const int32_t *neigh)
{
    if (!db || n < 0 || (n > 0 && (!slots || !neigh))) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    for (int i = 0; i < n; ++i)
        if (!slot_put(db, slots[i])) {
            set_error("kfdb neighbours: slot %d is not put", slots[i]);
            return AOS2_ERR_ARG;
        }
    for (int i = 0; i < n; ++i)
        std::copy(neigh + (size_t)i * AOS2_KFDB_NEIGHBOURS, neigh + (size_t)(i + 1) * AOS2_KFDB_NEIGHBOURS, db->slots[slots[i]].neigh);
    if (n) db->table_dirty = true;
    return AOS2_OK;
}

int aos2_kfdb_detect(aos2_kfdb_t *db, const aos2_kfdb_query_t *queries, aos2_kfdb_result_t *results, int nq)
{
    return detect(db, queries, results, nq, false);
}

int aos2_debug_kfdb_host(aos2_kfdb_t *db, const aos2_kfdb_query_t *queries, aos2_kfdb_result_t *results, int nq)
{
    return detect(db, queries, results, nq, true);
}

int aos2_kfdb_scores(aos2_kfdb_t *db, const aos2_kfdb_query_t *query, const int32_t *slots, int n, float *scores, float *min_score)
{
    if (int st = check_scores(db, query, slots, n, scores, min_score)) return st;
    if (n == 0) {
        *min_score = 1.0f;
        return AOS2_OK;
    }
    int st;
    if ((st = sync_device(db))) return st;
    QueryDev d = {};
    const bool host_rows = query->slot < 0 && !query->on_device;
    d.n = query->slot >= 0 ? db->slots[query->slot].len : query->n_words;
    if ((st = db->d_qw.alloc(host_rows ? d.n : 0)) || (st = db->d_qv.alloc(host_rows ? d.n : 0)) || (st = db->d_list.alloc(n)) ||
        (st = db->d_f32.alloc(n)))
        return st;
    hipStream_t s = db->stream;
    if (query->slot >= 0) {
        d.w = db->d_w.p + db->slots[query->slot].off;
        d.v = db->d_v.p + db->slots[query->slot].off;
    } else if (query->on_device) {
        d.w = query->words;
        d.v = query->values;
    } else {
        d.w = db->d_qw.p;
        d.v = db->d_qv.p;
        if (d.n) {
            AOS2_HIP_CHECK(hipMemcpyAsync(db->d_qw.p, query->words, d.n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            AOS2_HIP_CHECK(hipMemcpyAsync(db->d_qv.p, query->values, d.n * sizeof(double), hipMemcpyHostToDevice, s));
        }
    }
    AOS2_HIP_CHECK(hipMemcpyAsync(db->d_list.p, slots, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    AOS2_HIP_CHECK(hipEventRecord(db->ev[0], s));
    hipLaunchKernelGGL(k_kfdb_scores, dim3((n + kWaves - 1) / kWaves), dim3(kNT), 0, s, d, db->d_w.p, db->d_v.p, db->d_slots.p,
                       db->d_list.p, n, db->d_f32.p);
    AOS2_HIP_CHECK(hipGetLastError());
    AOS2_HIP_CHECK(hipEventRecord(db->ev[1], s));
    AOS2_HIP_CHECK(hipMemcpyAsync(scores, db->d_f32.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
    AOS2_HIP_CHECK(hipStreamSynchronize(s));
    AOS2_HIP_CHECK(hipEventElapsedTime(&db->last_ms, db->ev[0], db->ev[1]));
    min_from_one(scores, n, min_score);
    return AOS2_OK;
}

int aos2_debug_kfdb_scores_host(aos2_kfdb_t *db, const aos2_kfdb_query_t *query, const int32_t *slots, int n, float *scores,
                                float *min_score)
{
    if (int st = check_scores(db, query, slots, n, scores, min_score)) return st;
    std::vector<uint32_t> kw;
    std::vector<double> kv;
    QueryHost Q;
    if (int st = query_on_host(db, *query, kw, kv, Q)) return st;
    for (int i = 0; i < n; ++i) {
        const Slot &S = db->slots[slots[i]];
        scores[i] = kfdb_score(kfdb_merge_sum(Q.w, Q.v, Q.n, db->w.data() + S.off, db->v.data() + S.off, S.len));
    }
    min_from_one(scores, n, min_score);
    return AOS2_OK;
}

}  // extern "C"
