// The device layer of the descriptor searches: the types, constants and __device__ routines that the matcher's kernels
// (matcher.hip) and the kernels of the device-resident frame batches (frames.hip, frames_keyframe.hip) share -- descriptor
// distance and the two-smallest reductions, the rotation histogram, the two-stage (entries, then resolve) structure of the
// greedy searches with its parallel fixed-point stage B, the Frame::GetFeaturesInArea window walk, and the bodies of
// SearchByProjection(F, vpMapPoints), SearchByProjection(Current, Last), the projection family's set-up,
// Frame::AssignFeaturesToGrid and SearchForTriangulation's gates.  Device code only: no kernel, no host function; the
// kernels around these bodies and everything only one of the translation units uses stay in that unit.
#pragma once
#include <climits>

#include "aos2_common.h"
#include "wave_ops.h"

namespace aos2 {

constexpr int TH_HIGH = AOS2_TH_HIGH;
constexpr int TH_LOW = AOS2_TH_LOW;
constexpr int HISTO = AOS2_HISTO_LENGTH;
constexpr int GRID_COLS = AOS2_GRID_COLS;
constexpr int GRID_ROWS = AOS2_GRID_ROWS;
constexpr uint32_t KEY_NONE = 0xffffffffu;

struct Desc {
    uint32_t w[8];
};

__device__ __forceinline__ Desc load_desc(const uint8_t *p)
{
    Desc d;
    const uint4 a = *reinterpret_cast<const uint4 *>(p);
    const uint4 b = *reinterpret_cast<const uint4 *>(p + 16);
    d.w[0] = a.x; d.w[1] = a.y; d.w[2] = a.z; d.w[3] = a.w;
    d.w[4] = b.x; d.w[5] = b.y; d.w[6] = b.z; d.w[7] = b.w;
    return d;
}

__device__ __forceinline__ int hamming(const Desc &a, const Desc &b)
{
    int d = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d += __popc(a.w[i] ^ b.w[i]);
    return d;
}

// Hamming distance of a key; "no candidate" reads as 256, above every real distance
__device__ __forceinline__ int key_dist(uint32_t k) { return k == KEY_NONE ? 256 : (int)(k >> 20); }

// merge two (smallest, second smallest) pairs
__device__ __forceinline__ void merge2(uint32_t &k1, uint32_t &k2, uint32_t o1, uint32_t o2)
{
    const uint32_t lo = min(k1, o1), hi = max(k1, o1);
    k2 = min(hi, min(k2, o2));
    k1 = lo;
}

// Two smallest keys of the wave, result uniform.  The serial matcher loops sit on this latency, so
// no LDS crossbar (ds_bpermute) is used: four DPP butterfly steps reduce each 16-lane row at VALU
// speed (every step merges two disjoint lane sets), then the four row results are read into SGPRs.
__device__ __forceinline__ void wave_min2(uint32_t &k1, uint32_t &k2)
{
    merge2(k1, k2, dpp_u32<0xB1>(k1), dpp_u32<0xB1>(k2));    // quad_perm [1,0,3,2]
    merge2(k1, k2, dpp_u32<0x4E>(k1), dpp_u32<0x4E>(k2));    // quad_perm [2,3,0,1]
    merge2(k1, k2, dpp_u32<0x141>(k1), dpp_u32<0x141>(k2));  // row_half_mirror
    merge2(k1, k2, dpp_u32<0x140>(k1), dpp_u32<0x140>(k2));  // row_mirror
    uint32_t a1 = __builtin_amdgcn_readlane(k1, 0), a2 = __builtin_amdgcn_readlane(k2, 0);
    merge2(a1, a2, __builtin_amdgcn_readlane(k1, 16), __builtin_amdgcn_readlane(k2, 16));
    merge2(a1, a2, __builtin_amdgcn_readlane(k1, 32), __builtin_amdgcn_readlane(k2, 32));
    merge2(a1, a2, __builtin_amdgcn_readlane(k1, 48), __builtin_amdgcn_readlane(k2, 48));
    k1 = a1;
    k2 = a2;
}

// Single-wave kernels: lane 0's LDS write (taken/state flags) must be visible to the other lanes'
// later LDS reads.  LDS operations of one wave execute in order, so only the compiler has to be
// kept from reordering; a full __syncthreads() would also drain the prefetched global loads
// (vmcnt(0)) and put their latency back on the serial chain.
__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// value of `v` in the (unique) lane selected by a ballot mask, uniform result
__device__ __forceinline__ uint32_t read_owner(uint32_t v, unsigned long long mask)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, __ffsll((long long)mask) - 1);
}

// ---------------------------------------------------------------------------------------------
// rotation histogram helpers (ComputeThreeMaxima :1601-1642, bin quirk factor = 1/30 kept, :172)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int rot_bin(float rot)
{
    const float factor = 1.0f / HISTO;
    if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
    int bin = (int)roundf(__fmul_rn(rot, factor));
    if (bin == HISTO) bin = 0;
    return bin;
}

__device__ __forceinline__ void three_maxima(const int *histo, int &ind1, int &ind2, int &ind3)
{
    int max1 = 0, max2 = 0, max3 = 0;
    ind1 = ind2 = ind3 = -1;
    for (int i = 0; i < HISTO; i++) {
        const int s = histo[i];
        if (s > max1) {
            max3 = max2; max2 = max1; max1 = s;
            ind3 = ind2; ind2 = ind1; ind1 = i;
        } else if (s > max2) {
            max3 = max2; max2 = s;
            ind3 = ind2; ind2 = i;
        } else if (s > max3) {
            max3 = s;
            ind3 = i;
        }
    }
    if ((float)max2 < __fmul_rn(0.1f, (float)max1)) {
        ind2 = -1;
        ind3 = -1;
    } else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) {
        ind3 = -1;
    }
}

// The rotation-consistency verdict of a finished histogram: bit b of `culled` = bin b is none of the three maxima, `removed`
// = the pushed entries of those bins -- nmatches drops once per pushed entry (:281, :650, :1459-1460), not once per match.
struct RotCull {
    uint32_t culled;
    int removed;
};

__device__ __forceinline__ RotCull rot_cull(const int *histo)
{
    int i1, i2, i3;
    three_maxima(histo, i1, i2, i3);
    RotCull c{0, 0};
    for (int i = 0; i < HISTO; ++i)
        if (i != i1 && i != i2 && i != i3) {
            c.culled |= 1u << i;
            c.removed += histo[i];
        }
    return c;
}

// Reset the matches of the culled bins to `null_v`; thread `tid` of `nt` takes every nt-th element.
// bins[i] = bit mask of the bins element i was pushed into (it goes if ANY of them is culled)
__device__ __forceinline__ void cull_by_mask(uint32_t culled, const uint32_t *bins, int32_t *match, int n, int tid, int nt,
                                             int32_t null_v)
{
    for (int i = tid; i < n; i += nt)
        if (bins[i] & culled) match[i] = null_v;
}

// bin1[i] = bin + 1 of element i, 0 = never pushed.  Returns how many still-set matches this thread reset (a caller
// whose matches can be withdrawn after the push counts its drops with it; the others ignore it).
__device__ __forceinline__ int cull_by_bin1(uint32_t culled, const int32_t *bin1, int32_t *match, int n, int tid, int nt,
                                            int32_t null_v)
{
    int drop = 0;
    for (int i = tid; i < n; i += nt) {
        const int bn = bin1[i];
        if (bn > 0 && ((culled >> (bn - 1)) & 1u)) {
            drop += match[i] >= 0;
            match[i] = null_v;
        }
    }
    return drop;
}

// ---------------------------------------------------------------------------------------------
// Two-stage structure of the three search methods (SURVEY.md App. E option (a)):
//   stage A (parallel, one wave per query): enumerate the query's candidates in the reference's
//           visiting order and compute the Hamming distances -> entries {key, payload},
//           key = dist << 20 | visiting position (KEY_NONE for candidates the static gates reject);
//   stage B (sequential, one wave per problem): the reference's greedy loop over the queries;
//           per query one coalesced read of its entries (prefetched one query ahead), the
//           "already taken" mask applied from LDS, a two-smallest wave reduction, the accept
//           test, and the state update.  (best, second) of the strict '<' loops = the two
//           smallest keys, so ties resolve exactly like the reference.
// ---------------------------------------------------------------------------------------------
struct Entry {
    uint32_t key;      // dist << 20 | position, KEY_NONE = rejected before the distance test
    uint32_t payload;  // feature index | octave << 24
};

// Stage B, one query: the two smallest keys among the candidates `admit` lets through.  Every lane keeps the two smallest of
// its own candidates (and their payloads), the wave reduces the keys; keys are unique (they carry the visiting position), so
// a key names the lane that holds its payload.  A caller that never asks for payload2() leaves my2 / p2 dead, and the
// compiler drops their bookkeeping.
struct WaveBest2 {
    uint32_t k1, k2;            // the wave's smallest / second smallest key (uniform), KEY_NONE = none
    uint32_t my1, my2, p1, p2;  // this lane's own two and their payloads
    __device__ __forceinline__ uint32_t payload1() const { return read_owner(p1, __ballot(my1 == k1)); }   // k1 != KEY_NONE
    __device__ __forceinline__ uint32_t payload2() const                                                    // k2 != KEY_NONE
    {
        const unsigned long long first = __ballot(my1 == k2);   // the wave's second is some lane's first or second
        return first ? read_owner(p1, first) : read_owner(p2, __ballot(my2 == k2));
    }
};

// ent[0 .. cnt) = the query's entries, e = this lane's entry of the first 64 (prefetched); admit(entry) is asked for the
// entries inside the list only
template <class Admit>
__device__ __forceinline__ WaveBest2 wave_best2(const Entry *__restrict__ ent, int cnt, Entry e, int lane, Admit admit)
{
    WaveBest2 r;
    r.my1 = r.my2 = KEY_NONE;
    r.p1 = r.p2 = 0;
    for (int j0 = 0; j0 < cnt; j0 += 64) {
        if (j0 > 0) e = (j0 + lane < cnt) ? ent[j0 + lane] : Entry{KEY_NONE, 0};
        if (j0 + lane < cnt && admit(e)) {
            if (e.key < r.my1) {
                r.my2 = r.my1; r.p2 = r.p1;
                r.my1 = e.key; r.p1 = e.payload;
            } else if (e.key < r.my2) {
                r.my2 = e.key; r.p2 = e.payload;
            }
        }
    }
    r.k1 = r.my1;
    r.k2 = r.my2;
    wave_min2(r.k1, r.k2);
    return r;
}


// ---------------------------------------------------------------------------------------------
// Stage B without the serial chain (the greedy searches).  The reference's loops are greedy assignments: query q
// (a map point / keyframe feature, visited in a fixed order) sees feature f as taken iff an EARLIER query that
// "blocks" chose f, or f was taken before the call.  Let B[f] = the smallest such q (-1: before the call, INT_MAX:
// never).  Then every query can decide on its own ("f is blocked for q iff B[f] < q") and B follows from the
// decisions: a fixed point that is unique and equal to the sequential result (induction over q: the decision of q
// only reads B restricted to queries < q).  Iterating "all decisions from the previous B, in parallel -> next B"
// makes at least one more leading query final per pass and in practice converges in a handful of passes, because
// conflicts between search windows are rare (2-3 passes on the bench problems: 1500-3000 queries, 1000-2000 features).  One workgroup per problem, B double-buffered in LDS, the decisions
// (choice[q] = feature or -1) in global scratch; the caller turns the final decisions into the method's outputs.
// ---------------------------------------------------------------------------------------------
constexpr int kFixQpt = 3;   // queries per thread whose candidates stay in registers over the passes (VGPR budget of a 1024-thread workgroup)

struct Best2 {
    uint32_t k1, k2, p1, p2;   // smallest / second smallest key among the free candidates and their payloads
};

// (key, payload) pairs ordered by key (keys are unique: they carry the visiting position): branch-free insert of a
// candidate into the running (smallest, second smallest) pair
__device__ __forceinline__ void best2_insert(unsigned long long &b1, unsigned long long &b2, unsigned long long kk)
{
    const unsigned long long lo = kk < b1 ? kk : b1, hi = kk < b1 ? b1 : kk;
    b1 = lo;
    b2 = hi < b2 ? hi : b2;
}

__device__ __forceinline__ Best2 best2_unpack(unsigned long long b1, unsigned long long b2)
{
    return Best2{(uint32_t)(b1 >> 32), (uint32_t)(b2 >> 32), (uint32_t)b1, (uint32_t)b2};
}

// entries [j0, j0 + W) of a list of cnt, KEY_NONE beyond its end: W loads in one memory round trip
template <int W>
__device__ __forceinline__ void load_entries(const Entry *ent, int j0, int cnt, Entry (&eb)[W])
{
#pragma unroll
    for (int u = 0; u < W; ++u) eb[u] = j0 + u < cnt ? ent[j0 + u] : Entry{KEY_NONE, 0};
}

// the valid entries of eb[] that are free for query q (B[feature] >= q) go into the running pair; all B reads are issued together
template <int W>
__device__ __forceinline__ void scan_free(const Entry (&eb)[W], const int32_t *B, int q, uint32_t idx_mask,
                                          unsigned long long &b1, unsigned long long &b2)
{
    int bv[W];
#pragma unroll
    for (int u = 0; u < W; ++u) bv[u] = eb[u].key != KEY_NONE ? B[eb[u].payload & idx_mask] : -1;
#pragma unroll
    for (int u = 0; u < W; ++u) {
        const bool free_ = eb[u].key != KEY_NONE && bv[u] >= q;
        best2_insert(b1, b2, free_ ? ((unsigned long long)eb[u].key << 32) | eb[u].payload : ~0ull);
    }
}

// a whole list in global memory, 8 entries per round trip (a window / bucket rarely holds more)
__device__ __forceinline__ void scan_best2_free(const Entry *__restrict__ ent, int cnt, const int32_t *B, int q,
                                                uint32_t idx_mask, unsigned long long &b1, unsigned long long &b2)
{
    for (int j0 = 0; j0 < cnt; j0 += 8) {
        Entry eb[8];
        load_entries(ent, j0, cnt, eb);
        scan_free(eb, B, q, idx_mask, b1, b2);
    }
}

// initB(f) -> -1 (taken before the call) or INT_MAX; ent_of(q, cnt) -> the query's entries; accept(q, Best2) -> chosen
// feature or -1; blocks(q) -> whether a choice of q hides the feature from later queries.  All NT threads call it.
// CACHED (n_q <= kFixQpt * NT): up to kFixQpt queries per thread keep their (up to 8) valid entries, their blocking flag and their current
// decision in registers, so a pass touches only LDS (B) -- no global round trips on the pass loop.
template <int NT, bool CACHED, class InitB, class EntOf, class Accept, class Blocks>
__device__ __forceinline__ void resolve_fixpoint_impl(int n_f, int n_q, int32_t *lds, int32_t *choice, uint32_t idx_mask,
                                                      InitB initB, EntOf ent_of, Accept accept, Blocks blocks)
{
    __shared__ int changed;
    // valid candidates beyond the 8 a query keeps in registers (wide windows: SearchByProjection(Current, Last) with th = 15
    // has them for ~10 % of the queries): an LDS arena, so that no query walks its entries in global memory on the pass loop
    // (one such query made every pass ~20 us long).  A query that finds the arena full falls back to that walk.
    constexpr int kOvfCap = 2048;
    __shared__ Entry ovf_arena[kOvfCap];
    __shared__ int ovf_used;
    const int tid = threadIdx.x;
    int32_t *Bc = lds, *Bn = lds + n_f;
    for (int i = tid; i < n_f; i += NT) Bc[i] = initB(i);
    if (tid == 0) ovf_used = 0;
    constexpr int QPT = CACHED ? kFixQpt : 1;
    Entry ce[QPT][8];
    const Entry *cent[QPT];
    int ccnt[QPT], cchoice[QPT], covo[QPT], covn[QPT];
    bool cblk[QPT], covf[QPT];
    if (CACHED) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < QPT; ++j) {
            const int q = tid + NT * j;
            ccnt[j] = 0;
            cent[j] = nullptr;
            cchoice[j] = -2;
            cblk[j] = false;
            covf[j] = false;
            covo[j] = -1;
            covn[j] = 0;
            if (q < n_q) {
                cent[j] = ent_of(q, ccnt[j]);
                cblk[j] = blocks(q);
            }
            // keep the VALID entries (a window's population is mostly features rejected by the level / radius tests
            // before the distance, key == KEY_NONE): a shift register, so the array is only indexed statically.
#pragma unroll
            for (int u = 0; u < 8; ++u) ce[j][u] = Entry{KEY_NONE, 0};
            int nvalid = 0;
            for (int j0 = 0; j0 < ccnt[j]; j0 += 8) {
                Entry eb[8];
                load_entries(cent[j], j0, ccnt[j], eb);
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (eb[u].key != KEY_NONE) {
#pragma unroll
                        for (int w = 7; w > 0; --w) ce[j][w] = ce[j][w - 1];
                        ce[j][0] = eb[u];
                        ++nvalid;
                    }
            }
            covf[j] = nvalid > 8;
            if (nvalid > 8) {   // the registers hold the LAST 8 valid entries; the first nvalid - 8 go to the arena
                const int extra = nvalid - 8;
                const int off = atomicAdd(&ovf_used, extra);
                if (off + extra <= kOvfCap) {
                    covo[j] = off;
                    covn[j] = extra;
                    int w = 0;
                    for (int j0 = 0; j0 < ccnt[j] && w < extra; j0 += 8) {
                        Entry eb[8];
                        load_entries(cent[j], j0, ccnt[j], eb);
#pragma unroll
                        for (int u = 0; u < 8; ++u)
                            if (eb[u].key != KEY_NONE && w < extra) ovf_arena[off + w++] = eb[u];
                    }
                }
            }
        }
    } else {
        for (int q = tid; q < n_q; q += NT) choice[q] = -2;
    }
    __syncthreads();
    for (;;) {
        if (tid == 0) changed = 0;
        for (int i = tid; i < n_f; i += NT) Bn[i] = initB(i);
        __syncthreads();
        bool ch = false;
        if (CACHED) {
#pragma unroll
            for (int j = 0; j < QPT; ++j) {
                const int q = tid + NT * j;
                unsigned long long b1 = ~0ull, b2 = ~0ull;
                scan_free(ce[j], Bc, q, idx_mask, b1, b2);
                if (covf[j]) {   // more than 8 valid candidates
                    if (covo[j] >= 0) {
                        for (int t0 = 0; t0 < covn[j]; t0 += 4) {   // 4 entries (and their B lookups) in flight
                            Entry e[4];
                            load_entries(ovf_arena + covo[j], t0, covn[j], e);
                            scan_free(e, Bc, q, idx_mask, b1, b2);
                        }
                    } else {
                        b1 = b2 = ~0ull;
                        scan_best2_free(cent[j], ccnt[j], Bc, q, idx_mask, b1, b2);
                    }
                }
                const int c = ccnt[j] > 0 ? accept(q, best2_unpack(b1, b2)) : -1;   // (q >= n_q: ccnt = 0)
                ch |= c != cchoice[j];
                cchoice[j] = c;
                if (c >= 0 && cblk[j]) atomicMin(&Bn[c], q);
            }
        } else {
            for (int q = tid; q < n_q; q += NT) {
                int cnt = 0;
                const Entry *ent = ent_of(q, cnt);
                unsigned long long b1 = ~0ull, b2 = ~0ull;
                scan_best2_free(ent, cnt, Bc, q, idx_mask, b1, b2);
                const int c = cnt > 0 ? accept(q, best2_unpack(b1, b2)) : -1;
                if (c != choice[q]) {
                    ch = true;
                    choice[q] = c;
                }
                if (c >= 0 && blocks(q)) atomicMin(&Bn[c], q);
            }
        }
        if (ch) changed = 1;
        __syncthreads();
        if (!changed) break;   // the decisions reproduced themselves: B is the fixed point
        int32_t *t = Bc; Bc = Bn; Bn = t;
        __syncthreads();
    }
    if (CACHED) {
#pragma unroll
        for (int j = 0; j < QPT; ++j) {
            const int q = tid + NT * j;
            if (q < n_q) choice[q] = cchoice[j];
        }
        __syncthreads();   // the callers read choice[] with a different thread -> query mapping
    }
}

template <int NT, class InitB, class EntOf, class Accept, class Blocks>
__device__ __forceinline__ void resolve_fixpoint(int n_f, int n_q, int32_t *lds, int32_t *choice, uint32_t idx_mask,
                                                 InitB initB, EntOf ent_of, Accept accept, Blocks blocks)
{
    if (n_q <= kFixQpt * NT)   // uniform
        resolve_fixpoint_impl<NT, true>(n_f, n_q, lds, choice, idx_mask, initB, ent_of, accept, blocks);
    else
        resolve_fixpoint_impl<NT, false>(n_f, n_q, lds, choice, idx_mask, initB, ent_of, accept, blocks);
}

// after the fixed point: the workgroup's sum of the threads' counts of accepted queries (*total zeroed before the resolve)
__device__ __forceinline__ int block_total(int *total, int cnt)
{
    if (cnt) atomicAdd(total, cnt);
    __syncthreads();
    return *total;
}

// epipolar line l = x1' F12 of a KF1 point in KF2 (:142-144) and den = a^2 + b^2
struct EpiLine {
    float a, b, c, den;
};

__device__ __forceinline__ EpiLine epi_line(const float *F12, float kx, float ky)
{
    EpiLine l;
    l.a = __fadd_rn(__fadd_rn(__fmul_rn(kx, F12[0]), __fmul_rn(ky, F12[3])), F12[6]);
    l.b = __fadd_rn(__fadd_rn(__fmul_rn(kx, F12[1]), __fmul_rn(ky, F12[4])), F12[7]);
    l.c = __fadd_rn(__fadd_rn(__fmul_rn(kx, F12[2]), __fmul_rn(ky, F12[5])), F12[8]);
    l.den = __fadd_rn(__fmul_rn(l.a, l.a), __fmul_rn(l.b, l.b));
    return l;
}

// the geometric gate of a KF2 candidate at (x2, y2): a pair without stereo on either side must not sit on the epipole (ex, ey)
// (:739-745; sf = scale factor of the candidate's level), then CheckDistEpipolarLine (:139-157; sigma2 = its level's sigma^2)
__device__ __forceinline__ bool epi_admits(const EpiLine &l, float x2, float y2, bool both_mono, float ex, float ey, float sf,
                                           float sigma2)
{
    if (both_mono) {
        const float dx = __fsub_rn(ex, x2), dy = __fsub_rn(ey, y2);
        if (__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < __fmul_rn(100.0f, sf)) return false;
    }
    const float num = __fadd_rn(__fadd_rn(__fmul_rn(l.a, x2), __fmul_rn(l.b, y2)), l.c);
    if (l.den == 0.0f) return false;
    const float dsqr = __fdiv_rn(__fmul_rn(num, num), l.den);
    return (double)dsqr < __dmul_rn(3.84, (double)sigma2);
}

// rotation consistency (:776-808) + count of one pair by one wave: match12[0 .. n1) against the angle rows of the two keyframes;
// the bin of a match is recomputed from its two angles
__device__ __forceinline__ void triang_finish_body(int n1, const float *angle1, const float *angle2, int32_t *match12, int32_t *nmatches_out, int check_ori)
{
    __shared__ int histo[HISTO];
    const int lane = threadIdx.x;
    if (lane < HISTO) histo[lane] = 0;
    __syncthreads();
    int cnt = 0;
    for (int i = lane; i < n1; i += 64) {
        const int m2 = match12[i];
        if (m2 >= 0) {
            cnt++;
            if (check_ori) atomicAdd(&histo[rot_bin(__fsub_rn(angle1[i], angle2[m2]))], 1);
        }
    }
    __syncthreads();
    cnt = wave_sum_i32(cnt);
    if (check_ori) {
        const RotCull c = rot_cull(histo);
        for (int i = lane; i < n1; i += 64) {
            const int m2 = match12[i];
            if (m2 >= 0 && ((c.culled >> rot_bin(__fsub_rn(angle1[i], angle2[m2]))) & 1u)) match12[i] = -1;
        }
        cnt -= c.removed;
    }
    if (lane == 0) *nmatches_out = cnt;
}

// ---------------------------------------------------------------------------------------------
// Frame::GetFeaturesInArea (src/Frame.cc:356-409) candidate walk shared by both projection
// searches.  Lanes take grid cells of the window (ix-major, iy-minor like the reference loops);
// a wave prefix sum over the cell populations gives every candidate its position in the
// reference's visiting order, which is the tie-break of the strict '<' updates.
// ---------------------------------------------------------------------------------------------
struct FrameDev {
    int n_f, n_levels;
    const uint8_t *desc_f;
    const float *kp_x, *kp_y, *kp_angle, *u_right, *scale_factors;
    const int32_t *kp_octave;
    float min_x, min_y, max_x, max_y, grid_w_inv, grid_h_inv;
    const int32_t *grid_off, *grid_idx;
    const uint8_t *f_mp_state;
};

// The sticky "did not fit" word of a search (read by the host after the stream drained; may live in page-locked HOST memory:
// frames.hip).  A plain system-scope store: any non-zero value raises the capacity error, the value (one of the window
// populations that did not fit) only feeds its message -- an integer max is not a PCIe AtomicOp, and nothing here needs one.
__device__ __forceinline__ void overflow_note(int32_t *word, int need)
{
    __hip_atomic_store(word, need, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct Window {
    int x0, x1, y0, y1;  // cell range, valid iff ok
    bool ok;
};

__device__ __forceinline__ Window window_cells(const FrameDev &F, float x, float y, float r)
{
    Window w;
    w.ok = false;
    w.x0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, F.min_x), r), F.grid_w_inv)));
    if (w.x0 >= GRID_COLS) return w;
    w.x1 = min(GRID_COLS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, F.min_x), r), F.grid_w_inv)));
    if (w.x1 < 0) return w;
    w.y0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, F.min_y), r), F.grid_h_inv)));
    if (w.y0 >= GRID_ROWS) return w;
    w.y1 = min(GRID_ROWS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, F.min_y), r), F.grid_h_inv)));
    if (w.y1 < 0) return w;
    w.ok = true;
    return w;
}

// population of the window (all features of its cells, before any gate); wave-uniform result
__device__ __forceinline__ int window_population(const FrameDev &F, const Window &w, int lane)
{
    const int ny = w.y1 - w.y0 + 1, ncell = (w.x1 - w.x0 + 1) * ny;
    int total = 0;
    for (int c = lane; c < ncell; c += 64) {
        const int cell = (w.x0 + c / ny) * GRID_ROWS + w.y0 + c % ny;
        total += F.grid_off[cell + 1] - F.grid_off[cell];
    }
    return wave_sum_i32(total);
}

// the same number by ONE thread: the cells of a grid column are neighbours in the CSR, so a column of the window is one
// difference of offsets (the counting pass of the two-pass form runs a thread per query instead of a wave per query)
__device__ __forceinline__ int window_population_solo(const FrameDev &F, const Window &w)
{
    int total = 0;
    for (int ix = w.x0; ix <= w.x1; ++ix) total += F.grid_off[ix * GRID_ROWS + w.y1 + 1] - F.grid_off[ix * GRID_ROWS + w.y0];
    return total;
}

// stage A body: writes one entry per feature of the window at out[position]
__device__ __forceinline__ void window_entries(const FrameDev &F, const Window &w, const Desc &dq, float x, float y,
                                               float r, int minLevel, int maxLevel, float xr_proj, float xr_tol,
                                               int lane, Entry *out)
{
    // One candidate per lane.  The cells of a grid column are neighbours in the CSR, so the window is (x1 - x0 + 1) runs of
    // grid_idx, and position k of the window -- cells column by column, the features of a cell in their CSR order: the order
    // GetFeaturesInArea returns them in -- is element k of the concatenated runs.  (A lane per CELL walking the cell's
    // features one after the other kept 20-40 % of the lanes busy on a chain of dependent gathers as long as the fullest
    // cell.)
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    const int ncol = w.x1 - w.x0 + 1;   // <= GRID_COLS = 64: one lane per column
    int cb = 0, cnt = 0;
    if (lane < ncol) {
        const int c0 = (w.x0 + lane) * GRID_ROWS;
        cb = F.grid_off[c0 + w.y0];
        cnt = F.grid_off[c0 + w.y1 + 1] - cb;
    }
    const int incl = wave_incl_scan_i32(cnt);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    const int delta = cb - (incl - cnt);   // run start - first position of the column
    for (int k0 = 0; k0 < total; k0 += 64) {
        const int k = k0 + lane;
        int src = 0;
        for (int c = 0; c < ncol; ++c) {   // (uniform) the last column that starts at or before k
            const int first = __builtin_amdgcn_readlane(incl - cnt, c), d = __builtin_amdgcn_readlane(delta, c);
            if (k >= first) src = k + d;
        }
        if (k < total) {
            const int idx = F.grid_idx[src];
            // everything the gates and the distance need of the candidate is requested at once: gate by gate (octave, then position,
            // then uRight, then the descriptor) is four dependent round trips on a wave whose whole life is a handful of them
            const int oct = F.kp_octave[idx];
            const float kx = F.kp_x[idx], ky = F.kp_y[idx], ur = F.u_right[idx];
            const Desc dc = load_desc(F.desc_f + (size_t)idx * 32);
            Entry e;
            e.key = KEY_NONE;
            e.payload = (uint32_t)idx | ((uint32_t)oct << 24);
            bool pass = true;
            if (bCheckLevels) {
                if (oct < minLevel) pass = false;
                if (maxLevel >= 0 && oct > maxLevel) pass = false;
            }
            {
                const float distx = __fsub_rn(kx, x), disty = __fsub_rn(ky, y);
                if (!(fabsf(distx) < r && fabsf(disty) < r)) pass = false;
            }
            if (ur > 0) {
                const float er = fabsf(__fsub_rn(xr_proj, ur));
                if (er > xr_tol) pass = false;
            }
            if (pass) {
                const int dist = hamming(dq, dc);
                e.key = ((uint32_t)dist << 20) | (uint32_t)k;
            }
            out[k] = e;
        }
    }
}

struct QuerySlot {
    int32_t cnt;      // window population (0 = query skipped / empty window)
    int32_t ent_off;  // offset of its entries in the pool
};
// what the counting pass of a two-pass window search found out about a query with a non-empty window: the fill pass (a wave per
// query, hundreds of thousands of them per batch, each a chain of dependent loads) reads this record and its slot instead of
// repeating map point -> position -> projection -> octave -> scale factor -> window
struct QueryRec {
    float u, v, radius, ur;
    int16_t minL, maxL;
    int32_t row;      // descriptor row of the query
};
static_assert(sizeof(QueryRec) == 24, "QueryRec layout");

__device__ __forceinline__ QueryRec query_rec(float u, float v, float radius, float ur, int minL, int maxL, int row)
{
    QueryRec r;
    r.u = u; r.v = v; r.radius = radius; r.ur = ur;
    r.minL = (int16_t)minL; r.maxL = (int16_t)maxL; r.row = row;
    return r;
}

// Stage A, fill pass of the two-pass form with the counting pass's record: slot + record, then straight to the window
// (desc = the descriptor table the record's row refers to)
__device__ __forceinline__ void fill_from_record(const FrameDev &F, const uint8_t *desc, const QuerySlot *slots,
                                                 const QueryRec *rec, Entry *pool, int i, int lane)
{
    const QuerySlot sl = slots[i];
    if (sl.cnt <= 0) return;
    const QueryRec r = rec[i];
    const Window w = window_cells(F, r.u, r.v, r.radius);
    window_entries(F, w, load_desc(desc + (size_t)r.row * 32), r.u, r.v, r.radius, r.minL, r.maxL, r.ur, r.radius, lane,
                   pool + sl.ent_off);
}

// Stage A: where the `pop` (> 0) entries of query i go.  One-pass form (phase 0): query i of n owns a fixed slice of its
// problem's region [pool_base, pool_base + pool_cap) -- no shared counter: ~100 k same-address atomics serialised in one L2
// channel (0.94 ms for 64 frames); a window that does not fit its slice raises the sticky overflow word for the host.  Fill
// pass of the two-pass form (phase 2): the slot the scan assigned, if the counting pass saw the same population.
// Returns {pop, offset}, or cnt = -1: no room (the caller writes no entries).
__device__ __forceinline__ QuerySlot claim_slot(const QuerySlot *slots, int i, int n, int pop, int pool_base, int pool_cap,
                                                int phase, int32_t *pool_used, int lane)
{
    const int stride = phase == 2 ? pop : pool_cap / max(n, 1);
    const int off = phase == 2 ? slots[i].ent_off : pool_base + i * stride;
    if (pop > stride && lane == 0) overflow_note(pool_used, pop);
    if (pop <= stride && (phase != 2 || slots[i].cnt == pop)) return QuerySlot{pop, off};
    return QuerySlot{-1, 0};
}

// best / second of one query in the stage B of the window searches
struct Pick {
    uint32_t k1, k2;
    int idx1, oct1, oct2;   // feature and octave of the best, octave of the second; -1 = none
};

// candidates whose feature holds a map point with observations (state 2) are skipped -- with skip_any, any map point (state != 0)
__device__ __forceinline__ Pick pick_best2(const Entry *__restrict__ ent, int cnt, Entry e, const uint8_t *state,
                                           int lane, bool skip_any = false)
{
    const WaveBest2 b = wave_best2(ent, cnt, e, lane, [&](const Entry &c) {
        if (c.key == KEY_NONE) return false;
        const uint8_t stv = state[c.payload & 0xffffffu];
        return skip_any ? stv == 0 : stv != 2;
    });
    Pick r;
    r.k1 = b.k1;
    r.k2 = b.k2;
    r.idx1 = -1;
    r.oct1 = r.oct2 = -1;
    if (b.k1 != KEY_NONE) {
        const uint32_t pl = b.payload1();
        r.idx1 = (int)(pl & 0xffffffu);
        r.oct1 = (int)(pl >> 24);
    }
    if (b.k2 != KEY_NONE) r.oct2 = (int)(b.payload2() >> 24);
    return r;
}

// stage-B query stream: the slot of query i + 2 is fetched with a wave-uniform (scalar) load and its first 64
// entries with one vector load, two queries ahead of their use, so neither latency sits on the serial chain
struct SlotStream {
    const QuerySlot *slots;
    const Entry *pool;
    int n, lane;
    QuerySlot s1, s2;
    Entry e1, e2;
    __device__ __forceinline__ QuerySlot at(int i) const
    {
        const int iu = __builtin_amdgcn_readfirstlane(i);  // tell the compiler the index is uniform
        return slots[iu];
    }
    __device__ __forceinline__ Entry fetch(const QuerySlot &q) const
    {
        Entry r{KEY_NONE, 0};
        if (lane < q.cnt) r = pool[q.ent_off + lane];
        return r;
    }
    __device__ __forceinline__ void init(const QuerySlot *sl, const Entry *pl, int n_, int lane_)
    {
        slots = sl; pool = pl; n = n_; lane = lane_;
        s1 = s2 = QuerySlot{0, 0};
        e1 = e2 = Entry{KEY_NONE, 0};
        if (n > 0) {
            s1 = at(0);
            e1 = fetch(s1);
            if (n > 1) {
                s2 = at(1);
                e2 = fetch(s2);
            }
        }
    }
    // returns query i (slot + first 64 entries) and advances the prefetch window
    __device__ __forceinline__ void next(int i, QuerySlot &s, Entry &e)
    {
        s = s1;
        e = e1;
        s1 = s2;
        e1 = e2;
        if (i + 2 < n) {
            s2 = at(i + 2);
            e2 = fetch(s2);
        }
    }
};

// the ent_of of resolve_fixpoint for the searches whose stage A wrote slots into a pool
struct SlotEntries {
    const QuerySlot *slots;
    const Entry *pool;
    __device__ __forceinline__ const Entry *operator()(int q, int &cnt) const
    {
        const QuerySlot s = slots[q];
        cnt = s.cnt;
        return pool + s.ent_off;
    }
};

struct ProjMpDev {
    int n_mp;
    const uint8_t *track_in_view, *desc, *has_obs;
    const int32_t *pred_level;
    const float *view_cos, *proj_x, *proj_y, *proj_xr;
    const int32_t *desc_idx;   // optional: row of `desc` that holds query i's descriptor (a map-point table), else row i
};

__device__ __forceinline__ float mp_radius(const FrameDev &F, const ProjMpDev &P, int i, float th)
{
    float r = (double)P.view_cos[i] > 0.998 ? 2.5f : 4.0f;  // RadiusByViewingCos :131-137
    if (th != 1.0f) r = __fmul_rn(r, th);
    return __fmul_rn(r, F.scale_factors[P.pred_level[i]]);
}

// SearchByProjection(Frame&, const vector<MapPoint*>&, th)  :45-129, stage A: one wave per map point
// pool_base / pool_cap: this problem's region of the entry pool, cut into one fixed slice per map point (a counter
// shared by all waves serialised ~100 k same-address atomics in one L2 channel: 0.94 ms for 64 frames); pool_used is
// only an overflow flag
// phase 0: the query's entries go to its fixed slice of the pool (below).  Two-pass form (device-resident frames):
// phase 1 only counts the window populations (slots[i].cnt), a scan assigns slots[i].ent_off, phase 2 fills.
// kSolo (phase 1 only): the caller is one thread, not a wave.
template <bool kSolo = false>
__device__ __forceinline__ void proj_mp_entries_body(const FrameDev &F, const ProjMpDev &P, float th, QuerySlot *slots,
                                                     Entry *pool, int32_t *pool_used, int pool_cap, int i, int pool_base = 0,
                                                     int phase = 0, QueryRec *rec = nullptr)
{
    const int lane = kSolo ? 0 : (int)(threadIdx.x & 63);   // a wave per query (workgroups may hold several waves)
    if (phase == 2 && rec) {
        fill_from_record(F, P.desc, slots, rec, pool, i, lane);
        return;
    }
    QuerySlot s{0, 0};
    if (P.track_in_view[i]) {
        const float rs = mp_radius(F, P, i, th);
        const Window w = window_cells(F, P.proj_x[i], P.proj_y[i], rs);
        if (w.ok) {
            const int pop = kSolo ? window_population_solo(F, w) : window_population(F, w, lane);
            if (pop > 0 && (phase == 1 || kSolo)) {
                s.cnt = pop;
                if (rec && lane == 0) {
                    const int lvl = P.pred_level[i];
                    rec[i] = query_rec(P.proj_x[i], P.proj_y[i], rs, P.proj_xr[i], lvl - 1, lvl, P.desc_idx ? P.desc_idx[i] : i);
                }
            } else if (pop > 0) {
                s = claim_slot(slots, i, P.n_mp, pop, pool_base, pool_cap, phase, pool_used, lane);
                if (s.cnt > 0) {
                    const int lvl = P.pred_level[i];
                    const size_t drow = P.desc_idx ? (size_t)P.desc_idx[i] : (size_t)i;
                    window_entries(F, w, load_desc(P.desc + drow * 32), P.proj_x[i], P.proj_y[i], rs, lvl - 1, lvl,
                                   P.proj_xr[i], rs, lane, pool + s.ent_off);
                }
            }
        }
    }
    if (lane == 0 && phase != 2) slots[i] = s;
}

// exclusive scan of the window populations of one frame's queries -> entry offsets inside the frame's share of the pool;
// a frame whose windows hold more than its share gets no entries and raises the sticky flag.  The body of the scan-slots
// kernels (frames.hip: a workgroup per frame of the batch; matcher.hip: the one problem of its two-pass form); 256 threads.
__device__ __forceinline__ void scan_slots_body(QuerySlot *__restrict__ slots, const int32_t *__restrict__ nq_of, int nq_cap, int share,
                                                int32_t *__restrict__ overflow)
{
    __shared__ int32_t wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    QuerySlot *sl = slots + (size_t)b * nq_cap;
    const int nq = nq_of ? min(nq_of[b], nq_cap) : nq_cap;
    int carry = 0;   // entries of the chunks before this one (uniform)
    for (int q0 = 0; q0 < nq; q0 += 256) {
        const int q = q0 + tid;
        const int v = q < nq ? max(sl[q].cnt, 0) : 0;
        int total;
        const int excl = carry + block_excl_scan_i32<256>(v, wsum, total);
        if (q < nq) sl[q].ent_off = (int)((size_t)b * share) + excl;
        carry += total;
        __syncthreads();   // wsum is read before the next chunk writes it
    }
    if (carry > share) {
        for (int q = tid; q < nq; q += 256) sl[q].cnt = 0;
        if (tid == 0) overflow_note(overflow, carry);   // (the word is in host memory)
    }
}

// stage B
__device__ __forceinline__ void proj_mp_resolve_body(const FrameDev &F, const ProjMpDev &P, float nnratio,
                                                     const QuerySlot *__restrict__ slots, const Entry *__restrict__ pool,
                                                     int32_t *match_f, int32_t *nmatches_out)
{
    extern __shared__ uint8_t state[];
    const int lane = threadIdx.x;
    for (int i = lane; i < F.n_f; i += 64) {
        state[i] = F.f_mp_state[i];
        match_f[i] = -1;
    }
    __syncthreads();
    int nmatches = 0;
    SlotStream Q;
    Q.init(slots, pool, P.n_mp, lane);
    for (int iMP = 0; iMP < P.n_mp; iMP++) {
        QuerySlot s;
        Entry e;
        Q.next(iMP, s, e);
        if (s.cnt <= 0) continue;  // not in view, empty window (vIndices.empty()) -- nothing to do
        const Pick b = pick_best2(pool + s.ent_off, s.cnt, e, state, lane);
        const int bestDist = key_dist(b.k1), bestDist2 = key_dist(b.k2);
        if (bestDist <= TH_HIGH) {
            if (b.oct1 == b.oct2 && (float)bestDist > __fmul_rn(nnratio, (float)bestDist2)) continue;
            if (lane == 0) {
                match_f[b.idx1] = iMP;
                state[b.idx1] = P.has_obs[iMP] ? 2 : 1;
            }
            nmatches++;
            lds_fence();
        }
    }
    if (lane == 0) *nmatches_out = nmatches;
}

// parallel stage B of SearchByProjection(F, vpMapPoints, th) (resolve_fixpoint above): a map point WITH observations
// hides its feature from later map points (:62-64); match_f[f] = the LAST map point that chose f (:94 overwrites)
template <int NT>
__device__ __forceinline__ void proj_mp_resolve_fix_body(const FrameDev &F, const ProjMpDev &P, float nnratio,
                                                         const QuerySlot *__restrict__ slots, const Entry *__restrict__ pool,
                                                         int32_t *match_f, int32_t *nmatches_out, int32_t *choice)
{
    extern __shared__ int32_t fix_lds[];
    __shared__ int total;
    const int tid = threadIdx.x;
    for (int i = tid; i < F.n_f; i += NT) match_f[i] = -1;
    if (tid == 0) total = 0;
    resolve_fixpoint<NT>(
        F.n_f, P.n_mp, fix_lds, choice, 0xffffffu, [&](int i) { return F.f_mp_state[i] == 2 ? -1 : INT_MAX; },
        SlotEntries{slots, pool},
        [&](int, const Best2 &b) {
            const int bestDist = key_dist(b.k1), bestDist2 = key_dist(b.k2);
            const int oct1 = b.k1 == KEY_NONE ? -1 : (int)(b.p1 >> 24), oct2 = b.k2 == KEY_NONE ? -1 : (int)(b.p2 >> 24);
            if (bestDist <= TH_HIGH && !(oct1 == oct2 && (float)bestDist > __fmul_rn(nnratio, (float)bestDist2)))
                return (int)(b.p1 & 0xffffffu);
            return -1;
        },
        [&](int q) { return P.has_obs[q] != 0; });
    int cnt = 0;
    for (int q = tid; q < P.n_mp; q += NT) {
        const int c = choice[q];
        if (c >= 0) {
            atomicMax(&match_f[c], q);
            ++cnt;
        }
    }
    const int nmatches = block_total(&total, cnt);
    if (tid == 0) *nmatches_out = nmatches;
}

struct ProjLastDev {
    int n_last;
    const uint8_t *last_valid, *desc, *has_obs;
    const float *world_pos, *last_angle;
    const int32_t *last_octave;
    float Tcw[16], Tlw[16];
    float fx, fy, cx, cy, mb, mbf;
    // optional (device-resident frames): LastFrame.mvpMapPoints as rows of a map-point table (world_pos / desc / has_obs
    // are then the table's arrays) and LastFrame.mvbOutlier; last_valid is unused
    const int32_t *mp_idx;
    const uint8_t *outlier;
};

__device__ __forceinline__ bool proj_last_blocks(const ProjLastDev &P, int q)
{
    if (!P.mp_idx) return P.has_obs[q] != 0;
    const int row = P.mp_idx[q];
    return row >= 0 && P.has_obs[row] != 0;
}

// SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono)  :1328-1470
// stage A: one wave per last-frame feature: project, window, distances
template <bool kSolo = false>
__device__ __forceinline__ void proj_last_entries_body(const FrameDev &F, const ProjLastDev &P, float th, int mono,
                                                       QuerySlot *slots, Entry *pool, int32_t *pool_used, int pool_cap,
                                                       int i, int pool_base = 0, int phase = 0, QueryRec *rec = nullptr)
{
    const int lane = kSolo ? 0 : (int)(threadIdx.x & 63);   // a wave per query (workgroups may hold several waves)
    if (phase == 2 && rec) {
        fill_from_record(F, P.desc, slots, rec, pool, i, lane);
        return;
    }
    QuerySlot s{0, 0};
    const float *T = P.Tcw, *Tl = P.Tlw;
    int row = i;
    bool valid;
    if (P.mp_idx) {
        row = P.mp_idx[i];
        valid = row >= 0 && !P.outlier[i];
    } else
        valid = P.last_valid[i] != 0;
    if (valid) {
        // twc = -Rcw^T tcw (cv::gemm general path: double accumulation) ; tlc = Rlw twc + tlw (:1339-1346)
        float twc[3], tlc2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double sacc = __dadd_rn(__dadd_rn(__dmul_rn((double)T[k], (double)T[3]), __dmul_rn((double)T[4 + k], (double)T[7])),
                                          __dmul_rn((double)T[8 + k], (double)T[11]));
            twc[k] = (float)__dmul_rn(sacc, -1.0);
        }
        tlc2 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(Tl[8], twc[0]), __fmul_rn(Tl[9], twc[1])), __fmul_rn(Tl[10], twc[2])), Tl[11]);
        const bool bForward = tlc2 > P.mb && !mono;
        const bool bBackward = -tlc2 > P.mb && !mono;
        const float X0 = P.world_pos[3 * (size_t)row], X1 = P.world_pos[3 * (size_t)row + 1], X2 = P.world_pos[3 * (size_t)row + 2];
        float x3Dc[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float sacc = __fadd_rn(__fadd_rn(__fmul_rn(T[r * 4], X0), __fmul_rn(T[r * 4 + 1], X1)), __fmul_rn(T[r * 4 + 2], X2));
            x3Dc[r] = __fadd_rn(sacc, T[r * 4 + 3]);
        }
        const float invzc = (float)__ddiv_rn(1.0, (double)x3Dc[2]);
        const float u = __fadd_rn(__fmul_rn(__fmul_rn(P.fx, x3Dc[0]), invzc), P.cx);
        const float v = __fadd_rn(__fmul_rn(__fmul_rn(P.fy, x3Dc[1]), invzc), P.cy);
        const bool inside = !(invzc < 0) && !(u < F.min_x || u > F.max_x) && !(v < F.min_y || v > F.max_y);
        if (inside) {
            const int nLastOctave = P.last_octave[i];
            const float radius = __fmul_rn(th, F.scale_factors[nLastOctave]);
            int minL, maxL;
            if (bForward) {
                minL = nLastOctave;
                maxL = -1;
            } else if (bBackward) {
                minL = 0;
                maxL = nLastOctave;
            } else {
                minL = nLastOctave - 1;
                maxL = nLastOctave + 1;
            }
            const Window w = window_cells(F, u, v, radius);
            if (w.ok) {
                const int pop = kSolo ? window_population_solo(F, w) : window_population(F, w, lane);
                const float ur = __fsub_rn(u, __fmul_rn(P.mbf, invzc));
                if (pop > 0 && (phase == 1 || kSolo)) {
                    s.cnt = pop;
                    if (rec && lane == 0) rec[i] = query_rec(u, v, radius, ur, minL, maxL, row);
                } else if (pop > 0) {
                    s = claim_slot(slots, i, P.n_last, pop, pool_base, pool_cap, phase, pool_used, lane);
                    if (s.cnt > 0)
                        window_entries(F, w, load_desc(P.desc + (size_t)row * 32), u, v, radius, minL, maxL, ur, radius, lane,
                                       pool + s.ent_off);
                }
            }
        }
    }
    if (lane == 0 && phase != 2) slots[i] = s;
}

// parallel stage B of SearchByProjection(CurrentFrame, LastFrame, th, bMono) (resolve_fixpoint)
template <int NT>
__device__ __forceinline__ void proj_last_resolve_fix_body(const FrameDev &F, const ProjLastDev &P, int check_ori,
                                                           const QuerySlot *__restrict__ slots,
                                                           const Entry *__restrict__ pool, int32_t *match_f,
                                                           uint32_t *bin_f, int32_t *nmatches_out, int32_t *choice)
{
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
        F.n_f, P.n_last, fix_lds, choice, 0xffffffu, [&](int i) { return F.f_mp_state[i] == 2 ? -1 : INT_MAX; },
        SlotEntries{slots, pool},
        [&](int, const Best2 &b) { return (b.k1 != KEY_NONE && (int)(b.k1 >> 20) <= TH_HIGH) ? (int)(b.p1 & 0xffffffu) : -1; },
        [&](int q) { return proj_last_blocks(P, q); });
    int cnt = 0;
    for (int q = tid; q < P.n_last; q += NT) {
        const int c = choice[q];
        if (c >= 0) {
            atomicMax(&match_f[c], q);
            if (check_ori) {
                // a feature can be pushed several times when a zero-observation point is overwritten (:1432): it is
                // reset if ANY of its bins is culled, and nmatches drops once per pushed entry (:1459-1460)
                const int bin = rot_bin(__fsub_rn(P.last_angle[q], F.kp_angle[c]));
                atomicAdd(&histo[bin], 1);
                atomicOr(&bin_f[c], 1u << bin);
            }
            ++cnt;
        }
    }
    int nmatches = block_total(&total, cnt);
    if (check_ori) {
        const RotCull c = rot_cull(histo);
        cull_by_mask(c.culled, bin_f, match_f, F.n_f, tid, NT, -2);  // set to NULL (:1459)
        nmatches -= c.removed;
    }
    if (tid == 0) *nmatches_out = nmatches;
}

// ---------------------------------------------------------------------------------------------
// Projection family: map points projected into a keyframe / frame and matched to
// the most similar feature of a window.
//   mode 0  Fuse(pKF, vpMapPoints, th)                         :825-975    independent points
//   mode 1  Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)        :977-1100   independent points
//   mode 2  SearchByProjection(pKF, Scw, vpPoints, vpMatched)   :290-403    greedy over vpMatched
//   mode 3  one direction of SearchBySim3                       :1148-1303  independent points
//   mode 4  SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) :1472-1599  greedy + rotation
// cv::Mat arithmetic as the reference performs it (DESIGN.md conventions): R*p+t in float left to right,
// cv::norm and Mat::dot with double accumulation, log() = correctly rounded float logarithm.
// ---------------------------------------------------------------------------------------------
struct ProjGenDev {
    int n_pts, mode;
    const uint8_t *valid, *desc;
    const float *pos, *max_dist, *min_dist, *normal, *q_angle, *inv_level_sigma2;
    float R[9], t[3], Ow[3], R2[9], t2[3];
    float fx, fy, cx, cy, bf, log_scale_factor, th;
};

__device__ __forceinline__ void xform3(const float *R, const float *t, const float *p, float *o)
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
        o[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[3 * r], p[0]), __fmul_rn(R[3 * r + 1], p[1])), __fmul_rn(R[3 * r + 2], p[2])), t[r]);
}
__device__ __forceinline__ float norm3d(const float *v)
{
    const double s = __dadd_rn(__dadd_rn(__dmul_rn((double)v[0], (double)v[0]), __dmul_rn((double)v[1], (double)v[1])),
                               __dmul_rn((double)v[2], (double)v[2]));
    return (float)sqrt(s);
}

struct ProjSetup {
    bool ok;
    float u, v, ur, radius;
    int level;
};

// everything before GetFeaturesInArea; wave-uniform
__device__ __forceinline__ ProjSetup proj_gen_setup(const FrameDev &F, const ProjGenDev &P, int i)
{
    ProjSetup S;
    S.ok = false;
    S.u = S.v = S.ur = S.radius = 0.0f;
    S.level = 0;
    if (!P.valid[i]) return S;
    const float pw[3] = {P.pos[3 * i], P.pos[3 * i + 1], P.pos[3 * i + 2]};
    float pc[3];
    xform3(P.R, P.t, pw, pc);
    if (P.mode == 3) {  // p3Dc2 = sR21 * p3Dc1 + t21 (:1163)
        float c2[3];
        xform3(P.R2, P.t2, pc, c2);
        pc[0] = c2[0]; pc[1] = c2[1]; pc[2] = c2[2];
    }
    float u, v, invz;
    if (P.mode == 4) {  // :1505-1516: no depth test, u = fx*xc*invzc + cx, closed bounds
        invz = (float)__ddiv_rn(1.0, (double)pc[2]);
        u = __fadd_rn(__fmul_rn(__fmul_rn(P.fx, pc[0]), invz), P.cx);
        v = __fadd_rn(__fmul_rn(__fmul_rn(P.fy, pc[1]), invz), P.cy);
        if (u < F.min_x || u > F.max_x) return S;
        if (v < F.min_y || v > F.max_y) return S;
    } else {
        if (pc[2] < 0.0f) return S;
        // `1/z` (float division) in :852 and :329, `1.0/z` (double division, then float) in :1026 and :1170
        invz = (P.mode == 0 || P.mode == 2) ? __fdiv_rn(1.0f, pc[2]) : (float)__ddiv_rn(1.0, (double)pc[2]);
        const float x = __fmul_rn(pc[0], invz), y = __fmul_rn(pc[1], invz);
        u = __fadd_rn(__fmul_rn(P.fx, x), P.cx);
        v = __fadd_rn(__fmul_rn(P.fy, y), P.cy);
        if (!(u >= F.min_x && u < F.max_x && v >= F.min_y && v < F.max_y)) return S;  // KeyFrame::IsInImage
    }
    float dist3D;
    if (P.mode == 3) {
        dist3D = norm3d(pc);  // cv::norm(p3Dc2) :1185
    } else {
        const float PO[3] = {__fsub_rn(pw[0], P.Ow[0]), __fsub_rn(pw[1], P.Ow[1]), __fsub_rn(pw[2], P.Ow[2])};
        dist3D = norm3d(PO);
        if (P.mode != 4) {  // viewing angle below 60 deg: PO.dot(Pn) < 0.5*dist3D
            const double dot = __dadd_rn(__dadd_rn(__dmul_rn((double)PO[0], (double)P.normal[3 * i]),
                                                   __dmul_rn((double)PO[1], (double)P.normal[3 * i + 1])),
                                         __dmul_rn((double)PO[2], (double)P.normal[3 * i + 2]));
            if (dist3D < __fmul_rn(0.8f, P.min_dist[i]) || dist3D > __fmul_rn(1.2f, P.max_dist[i])) return S;
            if (dot < __dmul_rn(0.5, (double)dist3D)) return S;
        }
    }
    // range gate: Get{Min,Max}DistanceInvariance() = 0.8f * mfMinDistance / 1.2f * mfMaxDistance (src/MapPoint.cc:413-423);
    // PredictScale below takes the raw mfMaxDistance (:427-459) -- min_dist / max_dist carry the raw members
    const float maxd = P.max_dist[i];
    if (dist3D < __fmul_rn(0.8f, P.min_dist[i]) || dist3D > __fmul_rn(1.2f, maxd)) return S;
    // MapPoint::PredictScale (src/MapPoint.cc:427-459)
    const float ratio = __fdiv_rn(maxd, dist3D);
    const float lg = (float)log((double)ratio);
    int nScale = (int)ceilf(__fdiv_rn(lg, P.log_scale_factor));
    if (nScale < 0) nScale = 0;
    else if (nScale >= F.n_levels) nScale = F.n_levels - 1;
    S.level = nScale;
    S.radius = __fmul_rn(P.th, F.scale_factors[nScale]);
    S.u = u;
    S.v = v;
    S.ur = __fsub_rn(u, __fmul_rn(P.bf, invz));
    S.ok = true;
    return S;
}

// Frame::AssignFeaturesToGrid (src/Frame.cc:259-274, PosInGrid :411-424): one workgroup; cell of every feature,
// per-cell counts by LDS atomics, exclusive scan, and a stable fill (rank of a feature inside its cell = number of
// earlier features of the same cell, which is the push_back order of the reference)
__device__ __forceinline__ void assign_grid_body(int n, const float *__restrict__ kp_x, const float *__restrict__ kp_y,
                                                 float min_x, float min_y, float gwi, float ghi,
                                                 int32_t *__restrict__ grid_off, int32_t *__restrict__ grid_idx)
{
    extern __shared__ int32_t gsh[];
    constexpr int NC = GRID_COLS * GRID_ROWS;
    int32_t *cnt = gsh;                                  // NC + 1
    int16_t *cell = reinterpret_cast<int16_t *>(gsh + NC + 1);   // n
    __shared__ int32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int c = tid; c <= NC; c += 256) cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int px = (int)roundf(__fmul_rn(__fsub_rn(kp_x[i], min_x), gwi));
        const int py = (int)roundf(__fmul_rn(__fsub_rn(kp_y[i], min_y), ghi));
        const int c = (px < 0 || px >= GRID_COLS || py < 0 || py >= GRID_ROWS) ? -1 : px * GRID_ROWS + py;
        cell[i] = (int16_t)c;
        if (c >= 0) atomicAdd(&cnt[c], 1);
    }
    __syncthreads();
    // exclusive scan of the NC counts: thread t owns the kPer consecutive cells [t kPer, (t + 1) kPer)
    constexpr int kPer = NC / 256;
    static_assert(NC % 256 == 0 && NC <= 4096, "grid cells per thread; 12-bit cell numbers");
    int own[kPer], tsum = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        own[k] = cnt[tid * kPer + k];
        tsum += own[k];
    }
    int total;
    int excl = block_excl_scan_i32<256>(tsum, wsum, total);   // (its barrier also: every thread has read its counts before the offsets overwrite them)
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int c = tid * kPer + k;
        grid_off[c] = excl;
        cnt[c] = excl;   // from here on: the cell's fill cursor
        excl += own[k];
    }
    if (tid == 255) grid_off[NC] = excl;
    __syncthreads();
    // stable fill by ONE wave, 64 features at a time in index order: the lanes that share a cell find each other with 12
    // ballots (one per bit of the cell number), take consecutive places behind the cell's cursor in lane order, and the
    // last of them advances the cursor (LDS operations of a wave complete in order, so the next chunk sees it).  The
    // former per-feature count of earlier features in the same cell was O(n^2 / 256) LDS reads.
    if (wave == 0) {
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const int c = i < n ? cell[i] : -1;
            unsigned long long m = __ballot(c >= 0);
#pragma unroll
            for (int bit = 0; bit < 12; ++bit) {
                const bool one = (c >> bit) & 1;
                const unsigned long long bb = __ballot(one);
                m &= one ? bb : ~bb;
            }
            if (c >= 0) {
                const int below = __popcll(m & ((1ull << lane) - 1ull));
                const int base = cnt[c];
                grid_idx[base + below] = i;
                if (below == __popcll(m) - 1) cnt[c] = base + below + 1;
            }
        }
    }
}

// best candidate of a window for the independent modes: min over (dist << 20 | visiting position)
__device__ __forceinline__ uint32_t window_best(const FrameDev &F, const ProjGenDev &P, const Window &w, const Desc &dq,
                                                const ProjSetup &S, int lane, uint32_t &payload)
{
    // One candidate per lane, like window_entries: a lane per grid COLUMN finds the column's run of grid_idx, position k of the
    // window (cells column by column, the features of a cell in their CSR order) is element k of the concatenated runs.  (A lane
    // per cell walking its features one after the other is a chain of dependent gathers as long as the fullest cell -- the
    // form this routine had until round 3.)
    const int ncol = w.x1 - w.x0 + 1;   // <= GRID_COLS = 64
    int cb = 0, cnt = 0;
    if (lane < ncol) {
        const int c0 = (w.x0 + lane) * GRID_ROWS;
        cb = F.grid_off[c0 + w.y0];
        cnt = F.grid_off[c0 + w.y1 + 1] - cb;
    }
    const int incl = wave_incl_scan_i32(cnt);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    const int delta = cb - (incl - cnt);   // run start - first position of the column
    uint32_t key = KEY_NONE;
    payload = 0;
    for (int k0 = 0; k0 < total; k0 += 64) {
        const int k = k0 + lane;
        int src = 0;
        for (int c = 0; c < ncol; ++c) {   // (uniform) the last column that starts at or before k
            const int first = __builtin_amdgcn_readlane(incl - cnt, c), d = __builtin_amdgcn_readlane(delta, c);
            if (k >= first) src = k + d;
        }
        if (k < total) {
            const int idx = F.grid_idx[src];
            // (the candidate's position, octave, uRight and descriptor are requested together: gate by gate they are dependent round trips)
            const float kx = F.kp_x[idx], ky = F.kp_y[idx];
            const int oct = F.kp_octave[idx];
            const float kr = P.mode == 0 ? F.u_right[idx] : 0.0f;
            const Desc dc = load_desc(F.desc_f + (size_t)idx * 32);
            bool pass = fabsf(__fsub_rn(kx, S.u)) < S.radius && fabsf(__fsub_rn(ky, S.v)) < S.radius;
            if (oct < S.level - 1 || oct > S.level) pass = false;
            if (pass && P.mode == 0) {  // reprojection error gates of Fuse (:911-935)
                const float ex = __fsub_rn(S.u, kx), ey = __fsub_rn(S.v, ky);
                float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                double lim = 5.99;
                if (kr >= 0) {
                    const float er = __fsub_rn(S.ur, kr);
                    e2 = __fadd_rn(e2, __fmul_rn(er, er));
                    lim = 7.8;
                }
                if ((double)__fmul_rn(e2, P.inv_level_sigma2[oct]) > lim) pass = false;
            }
            if (pass) {
                const int dist = hamming(dq, dc);
                const uint32_t kk = ((uint32_t)dist << 20) | (uint32_t)k;
                if (kk < key) {
                    key = kk;
                    payload = (uint32_t)idx;
                }
            }
        }
    }
    uint32_t k1 = key, k2 = KEY_NONE;
    wave_min2(k1, k2);
    if (k1 != KEY_NONE) payload = read_owner(payload, __ballot(key == k1));
    return k1;
}

}  // namespace aos2
