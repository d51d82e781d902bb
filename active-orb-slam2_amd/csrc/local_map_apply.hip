// aos2_local_map_apply (include/aos2.h): one keyframe's changes applied to the graph that an
// aos2_local_map handle keeps in HBM, without the graph crossing PCIe again.  The delta names the rows that change and carries
// their new content; the new arrays are built from the current device block and the uploaded delta into the handle's SECOND
// block, and the handle then points at that one.  The kernels of csrc/local_map.hip and csrc/kf_culling.hip keep reading exact
// CSR arrays through LmGraph.  Integer and byte moves only (the two float arrays of the view move as 32-bit words).
//   k_lma_rows     a lane per row of the observation family (rows = points) and of the children family (rows = keyframes): the
//                  row's new length -- the delta's if the row is named (binary search in the ascending row list), the old one
//                  otherwise, 0 for an appended row -- its per-row scalars from the same source, and the exclusive scan of the
//                  lengths INSIDE the workgroup's tile of rows; the tile's sum goes to totals[workgroup]
//   k_lma_totals   ONE workgroup per family loops over the totals (any number of them) and turns them into their exclusive scan
//   k_lma_add      every row adds its tile's base
//   k_lma_copy     8 lanes per row: the entries of every row to their new place, from the old array or from the delta, obs_idx
//                  with obs_kf under the same offsets
//   k_lma_matches  a workgroup per keyframe: the match rows keep their offsets (a keyframe's N never changes), so this family is
//                  appended to, not scanned; kf_octave / kf_depth / kf_stereo move with kf_mp
// The three steps of the scan are separate launches on the handle's stream: the kernel boundary is the only ordering between
// workgroups, no workgroup waits for another one.
#include <algorithm>
#include <vector>

#include "aos2_common.h"
#include "local_map.h"
#include "regions.h"
#include "wave_ops.h"

using namespace aos2;

namespace {

constexpr int kRT = 256;             // threads of every kernel here
constexpr int kTileDefault = 1024;   // rows one workgroup scans
constexpr int kRowLanes = 8;         // lanes of k_lma_copy per row (an observation list holds ~7 entries, a child list fewer)
constexpr int64_t kMaxRows = (int64_t)1 << 30;

// one array in the three blocks of a rebuild: the resident block, the uploaded delta, the block being written
template <class T>
struct LmaSrc {
    const T *old, *d;
    T *nw;
};
// one CSR family rebuilt by the scan: its rows before and after, the delta's rows, the offsets, the entries and the array
// parallel to them (obs_idx; NULL = none)
struct LmaFam {
    int n_rows, n_old, n_d;
    const int32_t *d_row;
    int32_t *totals;
    LmaSrc<int32_t> off, flat, idx;
};
// what k_lma_rows reads beside them, the per-row scalars: of a point with family 0, of a keyframe's links with family 1 (the
// view's NULL = no view; kf_th_depth as 32-bit words)
struct LmaRows {
    LmaSrc<uint8_t> point_bad, kf_bad, kf_flags;
    LmaSrc<int32_t> point_nobs, kf_best, kf_parent;
    LmaSrc<uint32_t> kf_th_depth;
};
struct LmaArgs {
    LmaFam f[2];
    LmaRows s;
    int tile;
};
struct LmaMatch {
    int n_rows, n_old, n_d, n_mp_old, s0;   // s0: the delta slot of the first appended keyframe
    const int32_t *d_row;
    LmaSrc<int32_t> off, mp;
    LmaSrc<uint8_t> octave, stereo;   // NULL = no view; the int8_t octaves move as bytes
    LmaSrc<uint32_t> depth;           // ... the floats as 32-bit words
};

// element r of a per-row array after the delta: the delta's (at s) if the row is named, the old one if the row existed, the
// empty slot's otherwise
template <class T, class I>
__device__ __forceinline__ T lma_pick(const LmaSrc<T> &a, int slot, bool old, I r, I s, T fill)
{
    return slot >= 0 ? a.d[s] : (old ? a.old[r] : fill);
}

// the slot of row r in the ascending list, -1 = not named
__device__ __forceinline__ int lma_slot(const int32_t *rows, int n, int r)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rows[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && rows[lo] == r ? lo : -1;
}

__global__ __launch_bounds__(kRT) void k_lma_rows(LmaArgs A)
{
    __shared__ int32_t s_wsum[kRT / 64];
    const int fam = blockIdx.y, tid = threadIdx.x;
    const LmaFam &F = A.f[fam];
    const LmaRows &S = A.s;
    if ((int64_t)blockIdx.x * A.tile >= F.n_rows) return;   // (the grid is the larger family's)
    const int r0 = blockIdx.x * A.tile;
    int run = 0;
    for (int c = 0; c < A.tile; c += kRT) {
        const int i = c + tid, r = r0 + i;
        const bool in = i < A.tile && r < F.n_rows;
        int len = 0;
        if (in) {
            const int slot = lma_slot(F.d_row, F.n_d, r);
            const bool old = slot < 0 && r < F.n_old;
            if (slot >= 0) len = F.off.d[slot + 1] - F.off.d[slot];
            else if (old) len = F.off.old[r + 1] - F.off.old[r];
            if (fam == 0) {
                S.point_bad.nw[r] = lma_pick(S.point_bad, slot, old, r, slot, lm_fill::point_bad);
                S.point_nobs.nw[r] = lma_pick(S.point_nobs, slot, old, r, slot, lm_fill::point_nobs);
            } else {
                S.kf_bad.nw[r] = lma_pick(S.kf_bad, slot, old, r, slot, lm_fill::kf_bad);
                S.kf_parent.nw[r] = lma_pick(S.kf_parent, slot, old, r, slot, lm_fill::kf_parent);
                for (int j = 0; j < kLmNeighbours; ++j)
                    S.kf_best.nw[(size_t)r * kLmNeighbours + j] = lma_pick(S.kf_best, slot, old, (size_t)r * kLmNeighbours + j,
                                                                           (size_t)slot * kLmNeighbours + j, lm_fill::kf_best);
                if (S.kf_th_depth.nw) {
                    S.kf_th_depth.nw[r] = lma_pick(S.kf_th_depth, slot, old, r, slot, __float_as_uint(lm_fill::kf_th_depth));
                    S.kf_flags.nw[r] = lma_pick(S.kf_flags, slot, old, r, slot, lm_fill::kf_flags);
                }
            }
        }
        int total;
        const int ex = block_excl_scan_i32<kRT>(len, s_wsum, total);
        if (in) F.off.nw[r] = run + ex;
        run += total;
        __syncthreads();
    }
    if (tid == 0) F.totals[blockIdx.x] = run;
}

// one workgroup per family; min(tile, kRT) totals per step, so that the debug tile also reaches the loop
__global__ __launch_bounds__(kRT) void k_lma_totals(LmaArgs A)
{
    __shared__ int32_t s_wsum[kRT / 64];
    const LmaFam &F = A.f[blockIdx.x];
    const int tid = threadIdx.x;
    const int tiles = (int)(((int64_t)F.n_rows + A.tile - 1) / A.tile), step = min(A.tile, kRT);
    int run = 0;
    for (int c = 0; c < tiles; c += step) {
        const int i = c + tid;
        const bool in = tid < step && i < tiles;
        const int v = in ? F.totals[i] : 0;
        int total;
        const int ex = block_excl_scan_i32<kRT>(v, s_wsum, total);
        if (in) F.totals[i] = run + ex;
        run += total;
        __syncthreads();
    }
    if (tid == 0) F.off.nw[F.n_rows] = run;
}

__global__ __launch_bounds__(kRT) void k_lma_add(LmaArgs A)
{
    const LmaFam &F = A.f[blockIdx.y];
    const int stride = gridDim.x * kRT;
    for (int r = blockIdx.x * kRT + threadIdx.x; r < F.n_rows; r += stride) F.off.nw[r] += F.totals[r / A.tile];
}

__global__ __launch_bounds__(kRT) void k_lma_copy(LmaArgs A)
{
    const LmaFam &F = A.f[blockIdx.y];
    const int sub = threadIdx.x % kRowLanes, stride = gridDim.x * (kRT / kRowLanes);
    for (int r = blockIdx.x * (kRT / kRowLanes) + threadIdx.x / kRowLanes; r < F.n_rows; r += stride) {
        const int d0 = F.off.nw[r], len = F.off.nw[r + 1] - d0;
        if (len <= 0) continue;
        const int slot = lma_slot(F.d_row, F.n_d, r);
        if (slot < 0 && r >= F.n_old) continue;   // (an appended row that is not named is empty: never reached)
        const int s0 = slot >= 0 ? F.off.d[slot] : F.off.old[r];
        const int32_t *src = (slot >= 0 ? F.flat.d : F.flat.old) + s0;
        const int32_t *isrc = F.idx.nw ? (slot >= 0 ? F.idx.d : F.idx.old) + s0 : nullptr;
        for (int j = sub; j < len; j += kRowLanes) {
            F.flat.nw[d0 + j] = src[j];
            if (isrc) F.idx.nw[d0 + j] = isrc[j];
        }
    }
}

// workgroup r of n_rows + 1: offset r, and (r < n_rows) the entries of keyframe r
__global__ __launch_bounds__(kRT) void k_lma_matches(LmaMatch M)
{
    const int r = blockIdx.x, tid = threadIdx.x;
    // rows up to the old count keep their offsets; the appended rows are the tail of the delta's rows, in order
    const int d0 = r <= M.n_old ? M.off.old[r] : M.n_mp_old + (M.off.d[M.s0 + (r - M.n_old)] - M.off.d[M.s0]);
    if (tid == 0) M.off.nw[r] = d0;
    if (r >= M.n_rows) return;
    const int d1 = r + 1 <= M.n_old ? M.off.old[r + 1] : M.n_mp_old + (M.off.d[M.s0 + (r + 1 - M.n_old)] - M.off.d[M.s0]);
    const int slot = lma_slot(M.d_row, M.n_d, r);
    if (slot < 0 && r >= M.n_old) return;   // (an appended keyframe is always named)
    const int s0 = slot >= 0 ? M.off.d[slot] : M.off.old[r];
    const int len = min(d1 - d0, slot >= 0 ? M.off.d[slot + 1] - s0 : M.off.old[r + 1] - s0);   // (equal: the host has checked)
    const bool d = slot >= 0;
    for (int j = tid; j < len; j += kRT) {
        M.mp.nw[d0 + j] = (d ? M.mp.d : M.mp.old)[s0 + j];
        if (M.octave.nw) {
            M.octave.nw[d0 + j] = (d ? M.octave.d : M.octave.old)[s0 + j];
            M.depth.nw[d0 + j] = (d ? M.depth.d : M.depth.old)[s0 + j];
            M.stereo.nw[d0 + j] = (d ? M.stereo.d : M.stereo.old)[s0 + j];
        }
    }
}

const char *const kPre = "local map delta";   // of every error text here

// a row list: strictly ascending, inside [0, n_new)
bool bad_row_list(const int32_t *row, int n, int n_new, const char *what)
{
    if (n < 0) return lm_fail(kPre, "%s holds %d rows", what, n);
    if (n > 0 && !row) return lm_fail(kPre, "%s is NULL", what);
    for (int i = 0; i < n; ++i) {
        if (row[i] < 0 || row[i] >= n_new) return lm_fail(kPre, "%s[%d] = %d is outside [0, %d)", what, i, row[i], n_new);
        if (i && row[i] <= row[i - 1]) return lm_fail(kPre, "%s is not strictly ascending at %d", what, i);
    }
    return false;
}

// the graph's counts after the delta, the entries from the row lengths the handle keeps
LmCounts new_counts(const aos2_local_map *h, const aos2_local_map_delta_t *d)
{
    LmCounts c = h->counts();
    c.point_rows = (size_t)d->n_points;
    c.match_rows = c.link_rows = (size_t)d->n_keyframes;
    for (int i = 0; i < d->n_point_rows; ++i) {
        const int r = d->point_row[i];
        c.obs += (d->obs_off[i + 1] - d->obs_off[i]) - (r < h->n_points ? h->row_obs[r] : 0);
    }
    for (int i = 0; i < d->n_kf_mp_rows; ++i)
        if (d->kf_mp_row[i] >= h->n_kfs) c.mp += d->kf_mp_off[i + 1] - d->kf_mp_off[i];
    for (int i = 0; i < d->n_kf_link_rows; ++i) {
        const int r = d->kf_link_row[i];
        c.child += (d->kf_child_off[i + 1] - d->kf_child_off[i]) - (r < h->n_kfs ? h->row_child[r] : 0);
    }
    return c;
}

// the counts and row lengths of the handle after a delta that has been applied, in O(delta)
void commit_counts(aos2_local_map *h, const aos2_local_map_delta_t *d)
{
    const LmCounts c = new_counts(h, d);
    const int nk0 = h->n_kfs;
    h->row_obs.resize(d->n_points, 0);
    h->row_feat.resize(d->n_keyframes, 0);
    h->row_child.resize(d->n_keyframes, 0);
    for (int i = 0; i < d->n_point_rows; ++i) h->row_obs[d->point_row[i]] = d->obs_off[i + 1] - d->obs_off[i];
    for (int i = 0; i < d->n_kf_mp_rows; ++i)
        if (d->kf_mp_row[i] >= nk0) {
            h->row_feat[d->kf_mp_row[i]] = d->kf_mp_off[i + 1] - d->kf_mp_off[i];
            h->max_features = std::max(h->max_features, h->row_feat[d->kf_mp_row[i]]);
        }
    for (int i = 0; i < d->n_kf_link_rows; ++i) h->row_child[d->kf_link_row[i]] = d->kf_child_off[i + 1] - d->kf_child_off[i];
    h->n_obs = (int64_t)c.obs; h->n_mp = (int64_t)c.mp; h->n_child = (int64_t)c.child;
    h->n_points = d->n_points;
    h->n_kfs = d->n_keyframes;
    h->has_graph = true;
}

// where every row of a rebuilt CSR array comes from
struct RowSrc {
    bool delta;
    int32_t start, len;
};
std::vector<RowSrc> plan_rows(int n_new, int n_old, const std::vector<int32_t> &old_off, int n_d, const int32_t *d_row, const int32_t *d_off,
                              std::vector<int32_t> &new_off)
{
    std::vector<RowSrc> plan(n_new);
    new_off.assign((size_t)n_new + 1, 0);
    int s = 0;
    for (int r = 0; r < n_new; ++r) {
        if (s < n_d && d_row[s] == r) {
            plan[r] = RowSrc{true, d_off[s], d_off[s + 1] - d_off[s]};
            ++s;
        } else if (r < n_old)
            plan[r] = RowSrc{false, old_off[r], old_off[r + 1] - old_off[r]};
        else
            plan[r] = RowSrc{false, 0, 0};
        new_off[r + 1] = new_off[r] + plan[r].len;
    }
    return plan;
}
template <class T>
void move_rows(const std::vector<RowSrc> &plan, const std::vector<int32_t> &new_off, std::vector<T> &arr, const T *d_arr)
{
    std::vector<T> out((size_t)new_off.back());
    for (size_t r = 0; r < plan.size(); ++r) {
        const T *src = plan[r].delta ? d_arr : arr.data();
        std::copy(src + plan[r].start, src + plan[r].start + plan[r].len, out.begin() + new_off[r]);
    }
    arr.swap(out);
}
template <class T>
void put_rows(std::vector<T> &arr, int n_new, T fill, int n_d, const int32_t *d_row, const T *d_val, int width = 1)
{
    arr.resize((size_t)n_new * width, fill);
    for (int i = 0; i < n_d; ++i) std::copy(d_val + (size_t)i * width, d_val + (size_t)(i + 1) * width, arr.begin() + (size_t)d_row[i] * width);
}

template <class T>
T *rw(const T *p) { return const_cast<T *>(p); }
template <class To, class T>
LmaSrc<To> lma_as(const LmaSrc<T> &a)   // (only here: the kernels move float arrays as 32-bit words, int8_t octaves as bytes)
{
    static_assert(sizeof(To) == sizeof(T), "the same width");
    return LmaSrc<To>{reinterpret_cast<const To *>(a.old), reinterpret_cast<const To *>(a.d), reinterpret_cast<To *>(a.nw)};
}

// a delta's arrays as the internal struct; the offsets of a row set without rows (which may be NULL) are the one 0
LmArrays<LmPtr> delta_arrays(const aos2_local_map_delta_t *d, bool view)
{
    static const int32_t zero = 0;
    LmArrays<LmPtr> A = lm_from_public(*d, view ? d->view : nullptr);
    if (!d->n_point_rows) A.obs_off = &zero;
    if (!d->n_kf_mp_rows) A.kf_mp_off = &zero;
    if (!d->n_kf_link_rows) A.kf_child_off = &zero;
    return A;
}
LmCounts delta_counts(const aos2_local_map_delta_t *d, const LmArrays<LmPtr> &A)
{
    const size_t npr = (size_t)d->n_point_rows, nmr = (size_t)d->n_kf_mp_rows, nlr = (size_t)d->n_kf_link_rows;
    return LmCounts{npr, nmr, nlr, (size_t)A.obs_off[npr], (size_t)A.kf_mp_off[nmr], (size_t)A.kf_child_off[nlr]};
}

int apply_device(aos2_local_map *h, const aos2_local_map_delta_t *d)
{
    KfcState &K = h->kfc;
    const bool view = K.has_view;
    const int parts = kLmGraph | h->view_part();
    const int np = d->n_points, nk = d->n_keyframes, np0 = h->n_points, nk0 = h->n_kfs;
    const int npr = d->n_point_rows, nmr = d->n_kf_mp_rows, nlr = d->n_kf_link_rows;
    const LmCounts c = new_counts(h, d);
    const int tile = h->apply_tile > 0 ? h->apply_tile : kTileDefault;
    const int tiles0 = (int)(((int64_t)np + tile - 1) / tile), tiles1 = (int)(((int64_t)nk + tile - 1) / tile);

    int st;
    if ((st = bind_device(h->device))) return st;
    AOS2_HIP_CHECK(hipDeviceSynchronize());   // (the ordering contract of aos2_local_map_set: calls enqueued before this one are done)
    if (!h->stream && (st = stream_create(&h->stream, false))) return st;
    h->apply_timer.timed = false;

    // the new block: the graph, the view, and behind them the totals of the scan (not part of what a download copies)
    LmGraph G = {};
    int32_t *totals0, *totals1;
    G.n_points = np; G.n_kfs = nk;
    Regions<19> R;
    lm_layout(R, G, c, parts);
    const size_t block_bytes = R.bytes();
    R.add(totals0, std::max(tiles0, 1)); R.add(totals1, std::max(tiles1, 1));
    const size_t need = R.bytes() + 256;
    h->last_apply_realloc = 0;
    if (!h->d_spare.p || h->d_spare.n < need) {
        if ((st = h->d_spare.alloc(need + need / 4))) return st;
        h->last_apply_realloc = 1;
    }
    R.bind(h->d_spare.p);

    // the delta: one page-locked buffer, one copy
    const LmArrays<LmPtr> src = delta_arrays(d, view);
    const LmCounts dc = delta_counts(d, src);
    const int32_t *src_row[3] = {d->point_row, d->kf_mp_row, d->kf_link_row};
    LmArrays<LmPtr> D = {};
    const int32_t *row[3];
    Regions<20> Q;
    lm_layout_delta(Q, row, D, dc, parts);
    const size_t d_bytes = Q.bytes();
    if ((st = h->delta_stage.alloc(d_bytes + 256))) return st;
    if ((st = h->d_delta.alloc(d_bytes + 256))) return st;
    Q.bind(h->delta_stage.p);
    lm_copy(D, src, dc, parts);
    for (int s = 0; s < 3; ++s)
        if (const size_t n = lm_rows(dc, s)) memcpy(rw(row[s]), src_row[s], n * sizeof(int32_t));
    for (int i = 0; i < nlr; ++i)   // set<KeyFrame*> spChilds: ascending row, as aos2_local_map_set stores it
        std::sort(rw(D.kf_child) + src.kf_child_off[i], rw(D.kf_child) + src.kf_child_off[i + 1]);
    hipStream_t q = h->stream;
    if ((st = h->apply_timer.begin(q))) return st;
    AOS2_HIP_CHECK(hipMemcpyAsync(h->d_delta.p, h->delta_stage.p, d_bytes, hipMemcpyHostToDevice, q));
    Q.bind(h->d_delta.p);

    // every array in its three blocks: the resident one, the delta, the new one (the view's stay NULL without a view)
    LmArrays<LmaSrc> T = {};
    lm_each(T, h->G, parts, [](auto &a, auto *p, LmLen, auto) { a.old = p; });
    lm_each(T, D, parts, [](auto &a, auto *p, LmLen, auto) { a.d = p; });
    lm_each(T, G, parts, [](auto &a, auto *p, LmLen, auto) { a.nw = rw(p); });
    const LmaArgs A = {{LmaFam{np, np0, npr, row[0], totals0, T.obs_off, T.obs_kf, T.obs_idx},
                        LmaFam{nk, nk0, nlr, row[2], totals1, T.kf_child_off, T.kf_child, {}}},
                       LmaRows{T.point_bad, T.kf_bad, T.kf_flags, T.point_nobs, T.kf_best, T.kf_parent, lma_as<uint32_t>(T.kf_th_depth)}, tile};
    const LmaMatch M = {nk, nk0, nmr, (int)h->n_mp, nmr - (nk - nk0), row[1], T.kf_mp_off, T.kf_mp,
                        lma_as<uint8_t>(T.kf_octave), T.kf_stereo, lma_as<uint32_t>(T.kf_depth)};
    const int max_rows = std::max(np, nk), max_tiles = std::max(std::max(tiles0, tiles1), 1);
    const int add_blocks = std::max(1, std::min(2048, (max_rows + kRT - 1) / kRT));
    const int copy_rows = kRT / kRowLanes, copy_blocks = std::max(1, std::min(8192, (max_rows + copy_rows - 1) / copy_rows));
    hipLaunchKernelGGL(k_lma_rows, dim3(max_tiles, 2), dim3(kRT), 0, q, A);
    hipLaunchKernelGGL(k_lma_totals, dim3(2), dim3(kRT), 0, q, A);
    hipLaunchKernelGGL(k_lma_add, dim3(add_blocks, 2), dim3(kRT), 0, q, A);
    hipLaunchKernelGGL(k_lma_copy, dim3(copy_blocks, 2), dim3(kRT), 0, q, A);
    hipLaunchKernelGGL(k_lma_matches, dim3(nk + 1), dim3(kRT), 0, q, M);
    AOS2_HIP_CHECK(hipGetLastError());
    if ((st = h->apply_timer.end(q, true))) return st;
    // the new block is complete: it becomes the handle's, the previous one the spare
    std::swap(h->d_graph, h->d_spare);
    h->G = G;
    K.in_graph_block = view;
    h->block_bytes = block_bytes;
    h->host_stale = true;
    h->last_apply_bytes = (int64_t)d_bytes;
    return AOS2_OK;
}

int apply(aos2_local_map *h, const aos2_local_map_delta_t *d, bool force_host)
{
    if (int st = local_map_apply_check(h, d)) return st;
    KfcState &K = h->kfc;
    const bool resident = !h->dirty && (!K.has_view || !K.dirty);
    if (resident && !force_host) {
        if (int st = apply_device(h, d)) return st;
        commit_counts(h, d);
        h->last_apply_path = 1;
        return AOS2_OK;
    }
    if (int st = local_map_refresh_host(h)) return st;
    local_map_apply_host(h, d);
    h->dirty = true;   // the next consumer uploads the graph and the view
    if (K.has_view) K.dirty = true;
    h->last_apply_path = 0;
    h->last_apply_realloc = 0;
    h->last_apply_bytes = 0;
    h->apply_timer.timed = false;
    return bind_device(h->device);
}

}  // namespace

namespace aos2 {

int local_map_apply_check(const aos2_local_map *h, const aos2_local_map_delta_t *d)
{
    if (!h || !d) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    const int np = d->n_points, nk = d->n_keyframes, np0 = h->n_points, nk0 = h->n_kfs;
    const int npr = d->n_point_rows, nmr = d->n_kf_mp_rows, nlr = d->n_kf_link_rows;
    if (np < np0 || nk < nk0)
        return lm_fail(kPre, "%d points and %d keyframes are fewer than the handle's %d and %d (rows only get appended)", np, nk, np0, nk0);
    if (np > kMaxRows || nk > kMaxRows)
        return lm_fail(kPre, "more than 2^30 rows");
    if (bad_row_list(d->point_row, npr, np, "point_row") || bad_row_list(d->kf_mp_row, nmr, nk, "kf_mp_row") ||
        bad_row_list(d->kf_link_row, nlr, nk, "kf_link_row"))
        return AOS2_ERR_ARG;
    // (ascending and inside the count: the appended keyframes are all named exactly when the tail of the list holds that many)
    const int n_app = nk - nk0;
    for (int pass = 0; pass < 2; ++pass) {
        const int32_t *row = pass ? d->kf_link_row : d->kf_mp_row;
        const int n = pass ? nlr : nmr;
        if (n_app > 0 && (n < n_app || row[n - n_app] != nk0))
            return lm_fail(kPre, "an appended keyframe is missing from %s", pass ? "kf_link_row" : "kf_mp_row");
    }
    if ((npr > 0 && (!d->point_bad || !d->point_nobs)) || (nlr > 0 && (!d->kf_bad || !d->kf_best || !d->kf_parent)))
        return lm_fail(kPre, "an array is NULL");
    // (an offsets array of a row set without rows is not read)
    if ((npr && lm_bad_offsets(kPre, d->obs_off, npr, "obs_off")) || (nmr && lm_bad_offsets(kPre, d->kf_mp_off, nmr, "kf_mp_off")) ||
        (nlr && lm_bad_offsets(kPre, d->kf_child_off, nlr, "kf_child_off")))
        return AOS2_ERR_ARG;
    const LmArrays<LmPtr> A = delta_arrays(d, true);
    const LmCounts dc = delta_counts(d, A);
    if (lm_bad_values(kPre, A.obs_kf, dc.obs, 0, nk, "obs_kf") || lm_bad_values(kPre, A.kf_mp, dc.mp, -1, np, "kf_mp") ||
        lm_bad_values(kPre, A.kf_best, (int64_t)nlr * kLmNeighbours, -1, nk, "kf_best") ||
        lm_bad_values(kPre, A.kf_child, dc.child, 0, nk, "kf_child") || lm_bad_values(kPre, A.kf_parent, nlr, -1, nk, "kf_parent"))
        return AOS2_ERR_ARG;
    if (lm_listed_twice(kPre, npr, d->point_row, A.obs_off, A.obs_kf, nk)) return AOS2_ERR_ARG;
    for (int i = 0; i < nmr; ++i) {   // Frame::N of a keyframe never changes
        const int r = d->kf_mp_row[i], len = d->kf_mp_off[i + 1] - d->kf_mp_off[i];
        if (r < nk0 && len != h->row_feat[r])
            return lm_fail(kPre, "the match row of keyframe %d holds %d entries, the keyframe has %d features", r, len, h->row_feat[r]);
    }
    const aos2_kf_culling_view_t *v = d->view;
    if ((v != nullptr) != h->kfc.has_view)
        return lm_fail(kPre, v ? "a view is given, the handle holds none" : "the handle holds a culling view, the delta carries none");
    if (v) {
        if (lm_null_with_length(A, dc, kLmView))
            return lm_fail(kPre, "an array of the view is NULL");
        if (lm_bad_obs_idx(kPre, npr, d->point_row, A.obs_off, A.obs_kf, A.obs_idx, [&](int kf) {
                const int slot = nmr - (nk - kf);   // (of an appended keyframe: they are the tail of kf_mp_row)
                return kf < nk0 ? h->row_feat[kf] : A.kf_mp_off[slot + 1] - A.kf_mp_off[slot];
            }))
            return AOS2_ERR_ARG;
    }
    const LmCounts c = new_counts(h, d);
    const size_t lim = ((size_t)1 << 31) - 1;
    if (c.obs > lim || c.mp > lim || c.child > lim)
        return lm_fail(kPre, "more than 2^31 - 1 entries in an array");
    return AOS2_OK;
}

void local_map_apply_host(aos2_local_map *h, const aos2_local_map_delta_t *d)
{
    const int parts = kLmGraph | h->view_part();
    const LmArrays<LmPtr> D = delta_arrays(d, h->kfc.has_view);
    LmArrays<LmVec> &M = h->M;
    const int n_new[3] = {d->n_points, d->n_keyframes, d->n_keyframes}, n_old[3] = {h->n_points, h->n_kfs, h->n_kfs};
    const int n_d[3] = {d->n_point_rows, d->n_kf_mp_rows, d->n_kf_link_rows};
    const int32_t *const row[3] = {d->point_row, d->kf_mp_row, d->kf_link_row};
    // where the rows of the three CSR arrays come from: observations over points, matches and children over keyframes
    const std::vector<int32_t> *const old_off[3] = {&M.obs_off, &M.kf_mp_off, &M.kf_child_off};
    const int32_t *const d_off[3] = {D.obs_off, D.kf_mp_off, D.kf_child_off};
    std::vector<int32_t> off[3];
    std::vector<RowSrc> plan[3];
    for (int s = 0; s < 3; ++s) plan[s] = plan_rows(n_new[s], n_old[s], *old_off[s], n_d[s], row[s], d_off[s], off[s]);
    lm_each(M, D, parts, [&](auto &arr, auto *d_arr, LmLen l, auto fill) {
        const int s = lm_row_set(l);
        if (l == kLmPerObs || l == kLmPerMatch || l == kLmPerChild) move_rows(plan[s], off[s], arr, d_arr);
        else if (l == kLmPerPoint || l == kLmPerLink || l == kLmLinkNb)
            put_rows(arr, n_new[s], fill, n_d[s], row[s], d_arr, l == kLmLinkNb ? kLmNeighbours : 1);
    });
    M.obs_off.swap(off[0]);
    M.kf_mp_off.swap(off[1]);
    M.kf_child_off.swap(off[2]);
    for (int i = 0; i < n_d[2]; ++i) {   // a named row's children in ascending row
        const int r = row[2][i];
        std::sort(M.kf_child.begin() + M.kf_child_off[r], M.kf_child.begin() + M.kf_child_off[r + 1]);
    }
    commit_counts(h, d);
}

void local_map_recount(aos2_local_map *h)
{
    const int np = h->n_points, nk = h->n_kfs;
    h->row_obs.resize(np);
    h->row_feat.resize(nk);
    h->row_child.resize(nk);
    const LmArrays<LmVec> &M = h->M;
    for (int p = 0; p < np; ++p) h->row_obs[p] = M.obs_off[p + 1] - M.obs_off[p];
    for (int k = 0; k < nk; ++k) {
        h->row_feat[k] = M.kf_mp_off[k + 1] - M.kf_mp_off[k];
        h->row_child[k] = M.kf_child_off[k + 1] - M.kf_child_off[k];
    }
    h->n_obs = M.obs_off[np];
    h->n_mp = M.kf_mp_off[nk];
    h->n_child = M.kf_child_off[nk];
}

int local_map_refresh_host(aos2_local_map *h)
{
    if (!h->host_stale) return AOS2_OK;
    if (int st = bind_device(h->device)) return st;
    // Only a rebuild on the device leaves the mirror stale, and it lays the view out behind the graph: the block in d_graph
    // holds both, at the offsets the same layout gives here.
    const int parts = kLmGraph | h->view_part();
    LmArrays<LmPtr> B = {};
    Regions<17> R;
    lm_layout(R, B, h->counts(), parts);
    if ((h->kfc.has_view && !h->kfc.in_graph_block) || R.bytes() != h->block_bytes) {
        set_error("local map: the stale mirror does not match the rebuilt block (%zu bytes, %zu expected)", h->block_bytes, R.bytes());
        return AOS2_ERR_HIP;
    }
    std::vector<uint8_t> buf(h->block_bytes + 1);
    AOS2_HIP_CHECK(hipMemcpy(buf.data(), h->d_graph.p, h->block_bytes, hipMemcpyDeviceToHost));   // the one download
    R.bind(buf.data());
    lm_take(h->M, B, h->counts(), parts);
    h->host_stale = false;
    return AOS2_OK;
}

}  // namespace aos2

extern "C" {

int aos2_local_map_apply(aos2_local_map_t *h, const aos2_local_map_delta_t *d) { return apply(h, d, false); }

int aos2_debug_local_map_apply_host(aos2_local_map_t *h, const aos2_local_map_delta_t *d) { return apply(h, d, true); }

int aos2_local_map_last_apply(const aos2_local_map_t *h, int32_t *path, int32_t *reallocated, float *device_ms)
{
    if (!h) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if (path) *path = h->last_apply_path;
    if (reallocated) *reallocated = h->last_apply_realloc;
    if (device_ms) {
        *device_ms = h->apply_timer.ms();
    }
    return AOS2_OK;
}

int64_t aos2_local_map_last_apply_bytes(const aos2_local_map_t *h) { return h ? h->last_apply_bytes : 0; }

int aos2_local_map_debug_apply_tile(aos2_local_map_t *h, int rows)
{
    if (!h) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    h->apply_tile = rows <= 0 ? 0 : rows;
    return AOS2_OK;
}

}  // extern "C"
